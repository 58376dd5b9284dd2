// mgx_semi3d.hip -- grid transfers of a SEMI-COARSENED 3D hierarchy (x-split layout): the coarse level halves only the
// axes of a mask m in 1..6 (bit 0 = x, 1 = y, 2 = z) and keeps the others.  DESIGN.md section 12.
//
// The reference has no such operators; their arithmetic is fixed here (and restated in tests/semi_restated.py), all in
// `real`, left to right as written, weights powers of two:
//   restriction, fine centre C = (2c along halved axes, c along kept ones), Ma / Pa = its neighbours at -1 / +1 along a:
//     one halved axis a      (1/2) C + (1/4) (Ma + Pa)
//     two halved axes a < b  (1/4) C + (1/8) ((Ma + Pa) + (Mb + Pb)) + (1/16) ((MaMb + PaMb) + (MaPb + PaPb))
//   interpolation of a fine interior point, S = its odd halved axes in ascending order, c[..] = coarse value at the base
//   (F >> 1 along halved axes, F along kept ones) plus 1 along the listed axes:
//     c[],   (1/2) (c[] + c[a]),   (1/4) (((c[] + c[a]) + c[b]) + c[a,b])
//
// Kernels:
//   residual_restrict_axes3d_xs_kernel   coarse_f = R_m(CalculateResidual(v, f)), the residual never stored: lane i of a
//                                        wave owns the fine x-pair {2i, 2i+1} of a few rows and marches along z with the
//                                        three v planes of its column in registers (residual_restrict3d_xs_kernel's
//                                        recipe); x-neighbours come from the adjacent lanes
//   interpolate_axes3d_xs_kernel         v (+)= I_m(coarse_v) on the interior, one fine cell of the coarse mesh per thread
//   restrict_axes3d_xs_kernel            Restrict with the boundary injected (FMG only)
#include "mgx_kernels3d.hpp"

namespace mgx {

// offset (dx, dy, dz) with `s` along axis `a` and `t` along axis `b` (b < 0: none)
template <class real, class Get>
__device__ __forceinline__ real semi_at(Get get, int a, int s, int b = -1, int t = 0) {
    const int dx = (a == 0 ? s : 0) + (b == 0 ? t : 0), dy = (a == 1 ? s : 0) + (b == 1 ? t : 0), dz = (a == 2 ? s : 0) + (b == 2 ? t : 0);
    return get(dx, dy, dz);
}

// restriction at one coarse interior point; get(dx, dy, dz) = fine value at that offset from the fine centre
template <class real, int MASK, class Get>
__device__ __forceinline__ real semi_restrict_point(Get get) {
    constexpr int A = (MASK & 1) ? 0 : (MASK & 2) ? 1 : 2;                                      // first halved axis
    constexpr int B = (MASK & 1) && (MASK & 2) ? 1 : ((MASK & 3) && (MASK & 4)) ? 2 : -1;        // second one, if any
    const real C = get(0, 0, 0);
    if constexpr (B < 0) {
        return (real)0.5 * C + (real)0.25 * (semi_at<real>(get, A, -1) + semi_at<real>(get, A, 1));
    } else {
        return (real)0.25 * C +
               (real)0.125 * ((semi_at<real>(get, A, -1) + semi_at<real>(get, A, 1)) + (semi_at<real>(get, B, -1) + semi_at<real>(get, B, 1))) +
               (real)0.0625 * ((semi_at<real>(get, A, -1, B, -1) + semi_at<real>(get, A, 1, B, -1)) +
                               (semi_at<real>(get, A, -1, B, 1) + semi_at<real>(get, A, 1, B, 1)));
    }
}

// interpolated value of one fine point; o[d] = fine index odd along the HALVED axis d (0 on kept axes);
// get(dx, dy, dz) = coarse value at the base plus that offset
template <class real, class Get>
__device__ __forceinline__ real semi_interpolate_point(int ox, int oy, int oz, Get get) {
    const int a = ox ? 0 : oy ? 1 : oz ? 2 : -1;
    const int b = (ox && oy) ? 1 : ((ox || oy) && oz) ? 2 : -1;
    if (a < 0) return get(0, 0, 0);
    if (b < 0) return (real)0.5 * (get(0, 0, 0) + semi_at<real>(get, a, 1));
    return (real)0.25 * (((get(0, 0, 0) + semi_at<real>(get, a, 1)) + semi_at<real>(get, b, 1)) + semi_at<real>(get, a, 1, b, 1));
}

// ------------------------------------------------------------------ residual + restrict, streaming
// A wave covers the fine x-pairs of one tile of a row group and the coarse planes [pz0, pz1) of its run.  Per lane: the v rows
// around CR coarse rows (2 CR + 3 fine rows where y is halved, CR + 2 where it is kept) of three consecutive fine planes, carried
// along z, so that every v plane is loaded once per row group; f is read once.  Where x is halved, coarse column i sits under
// the even entry of pair i and takes the residual at x - 1 from the odd entry of lane i - 1: lane 0 of a wave is a halo lane
// and a wave produces 63 coarse columns.  Where x is kept, the coarse row has the fine row's geometry, both entries of a pair are
// coarse points and a wave stores two full runs of 64 consecutive reals.  Coarse boundary points are not written.
template <class real, int MASK, int MODE, int CR, int TYW>
__global__ void __launch_bounds__(64 * TYW)
    residual_restrict_axes3d_xs_kernel(const real* __restrict__ v, const real* __restrict__ f, int sx, int sy, int sz, real qx, real qy,
                                       real qz, real* __restrict__ coarse, int cx, int cy, int cz, int pzchunk, int gx, int gy) {
    constexpr bool HX = (MASK & 1) != 0, HY = (MASK & 2) != 0, HZ = (MASK & 4) != 0;
    constexpr int NRR = HY ? 2 * CR + 1 : CR;  // residual rows per lane
    constexpr int NR = NRR + 2;                // v rows per lane: one more on either side
    constexpr int NK = HZ ? 3 : 1;             // residual planes under one coarse plane
    constexpr int K0 = HZ ? 1 : 0;             // the centre one
    const Geo<XSplit, real> gf(sx, sy), gc(cx, cy);
    const int lane = threadIdx.x;
    const int bx = blockIdx.x % gx, by = (blockIdx.x / gx) % gy, bz = blockIdx.x / (gx * gy);
    const int npair = (sx + 1) >> 1;  // x-pairs of a fine row; the last one holds x = sx - 1 alone
    const int iu = (HX ? bx * 63 : bx * 64) + lane;
    const int i = min(iu, npair - 1);  // lanes past the row stay active (their neighbours read them) and store nothing
    const int cyb = 1 + (by * TYW + __builtin_amdgcn_readfirstlane(threadIdx.y)) * CR;
    if (cyb > cy - 2) return;
    const int pz0 = 1 + bz * pzchunk;
    const int pz1 = min(pz0 + pzchunk, cz - 1);
    if (pz0 >= pz1) return;
    const bool hasB = iu <= npair - 2;             // the odd-x entry 2i+1 exists (and is interior)
    const bool xinA = iu >= 1 && iu <= npair - 2;  // x = 2i is interior
    const int yf0 = HY ? 2 * cyb - 2 : cyb - 1;
    size_t roff[NR];
    bool yin[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const int y = yf0 + r;
        roff[r] = (size_t)min(y, sy - 1) * gf.P;
        yin[r] = y >= 1 && y <= sy - 2;
    }
    const size_t PL = gf.PL;
    const int iB = gf.H + (hasB ? i : 0);
    auto loadA = [&](int g, real(&A)[NR]) __attribute__((always_inline)) {
        const size_t pb = (size_t)g * PL + i;
#pragma unroll
        for (int r = 0; r < NR; r++) A[r] = v[pb + roff[r]];
    };
    auto loadB = [&](int g, real(&B)[NR]) __attribute__((always_inline)) {
        const size_t pb = (size_t)g * PL + iB;
#pragma unroll
        for (int r = 0; r < NR; r++) B[r] = v[pb + roff[r]];
    };
    // residuals of fine plane g on the rows 1 .. NR-2 of the window for x = 2i (rA) and x = 2i+1 (rB); 0 outside the interior
    auto resid = [&](int g, const real(&AP)[NR], const real(&BP)[NR], const real(&AC)[NR], const real(&BC)[NR], const real(&AN)[NR],
                     const real(&BN)[NR], real(&rA)[NRR], real(&rB)[NRR]) __attribute__((always_inline)) {
        const bool zin = g >= 1 && g <= sz - 2;
        const size_t pb = (size_t)g * PL;
#pragma unroll
        for (int r = 1; r < NR - 1; r++) {
            const real fA = __builtin_nontemporal_load(&f[pb + roff[r] + i]);
            const real fB = __builtin_nontemporal_load(&f[pb + roff[r] + iB]);
            real Bl = wave_from_prev_lane<real>(BC[r]);  // v(2i-1): odd entry of lane i-1
            real Ar = wave_from_next_lane<real>(AC[r]);  // v(2i+2): even entry of lane i+1
            if (lane == 0 && i > 0) Bl = v[pb + roff[r] + gf.H + i - 1];  // wave edges: load them
            if (lane == 63 && hasB) Ar = v[pb + roff[r] + i + 1];
            const real a = residual3d_point<real, MODE>(Bl, BC[r], AC[r - 1], AC[r + 1], AP[r], AN[r], AC[r], fA, qx, qy, qz);
            const real b = residual3d_point<real, MODE>(AC[r], Ar, BC[r - 1], BC[r + 1], BP[r], BN[r], BC[r], fB, qx, qy, qz);
            rA[r - 1] = (zin && yin[r] && xinA) ? a : (real)0;
            rB[r - 1] = (zin && yin[r] && hasB) ? b : (real)0;
        }
    };
    real AP[NR], BP[NR], AC[NR], BC[NR], AN[NR], BN[NR];
    real rA[NK][NRR], rB[NK][NRR];
    auto shift = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < NR; r++) { AP[r] = AC[r]; BP[r] = BC[r]; AC[r] = AN[r]; BC[r] = BN[r]; }
    };
    if constexpr (HZ) {  // v planes 2pz0-2, 2pz0-1, 2pz0 and the residual of plane 2pz0-1
        loadA(2 * pz0 - 2, AP); loadB(2 * pz0 - 2, BP);
        loadA(2 * pz0 - 1, AC); loadB(2 * pz0 - 1, BC);
        loadA(2 * pz0, AN);     loadB(2 * pz0, BN);
        resid(2 * pz0 - 1, AP, BP, AC, BC, AN, BN, rA[0], rB[0]);
    } else {  // v planes pz0-1 and pz0
        loadA(pz0 - 1, AN); loadB(pz0 - 1, BN);
        shift();
        loadA(pz0, AN); loadB(pz0, BN);
    }
    for (int pz = pz0; pz < pz1; pz++) {
        if constexpr (HZ) {
            shift();
            loadA(2 * pz + 1, AN); loadB(2 * pz + 1, BN);
            resid(2 * pz, AP, BP, AC, BC, AN, BN, rA[1], rB[1]);
            shift();
            loadA(2 * pz + 2, AN); loadB(2 * pz + 2, BN);
            resid(2 * pz + 1, AP, BP, AC, BC, AN, BN, rA[2], rB[2]);
        } else {
            shift();
            loadA(pz + 1, AN); loadB(pz + 1, BN);
            resid(pz, AP, BP, AC, BC, AN, BN, rA[0], rB[0]);
        }
        real lB[NK][NRR];  // x halved: the residual at x = 2i-1
        if constexpr (HX) {
#pragma unroll
            for (int k = 0; k < NK; k++)
#pragma unroll
                for (int r = 0; r < NRR; r++) lB[k][r] = wave_from_prev_lane<real>(rB[k][r]);
        }
#pragma unroll
        for (int c = 0; c < CR; c++) {
            const int py = cyb + c;
            const int rc = HY ? 2 * c + 1 : c;  // residual row of the fine centre
            if (py <= cy - 2) {
                const size_t crow = gc.row(py, pz);
                if constexpr (HX) {
                    const real e = semi_restrict_point<real, MASK>([&](int dx, int dy, int dz) __attribute__((always_inline)) {
                        return dx < 0 ? lB[K0 + dz][rc + dy] : dx > 0 ? rB[K0 + dz][rc + dy] : rA[K0 + dz][rc + dy];
                    });
                    if (lane > 0 && xinA) __builtin_nontemporal_store(e, &coarse[crow + gc.pos(i)]);
                } else {
                    const real ea = semi_restrict_point<real, MASK>([&](int, int dy, int dz) __attribute__((always_inline)) { return rA[K0 + dz][rc + dy]; });
                    const real eb = semi_restrict_point<real, MASK>([&](int, int dy, int dz) __attribute__((always_inline)) { return rB[K0 + dz][rc + dy]; });
                    if (xinA) __builtin_nontemporal_store(ea, &coarse[crow + i]);
                    if (hasB) __builtin_nontemporal_store(eb, &coarse[crow + gc.H + i]);
                }
            }
        }
        if constexpr (HZ) {  // plane 2pz+1 is the next step's plane 2(pz+1)-1
#pragma unroll
            for (int r = 0; r < NRR; r++) { rA[0][r] = rA[2][r]; rB[0][r] = rB[2][r]; }
        }
    }
}

// boundary points of an x-split array := 0 (pads are not touched)
template <class real>
__global__ void __launch_bounds__(256) rim_zero3d_xs_kernel(real* __restrict__ a, int sx, int sy, int sz) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y, z = blockIdx.z;
    if (x >= sx || y >= sy) return;
    if (!(x == 0 || x == sx - 1 || y == 0 || y == sy - 1 || z == 0 || z == sz - 1)) return;
    const Geo<XSplit, real> g(sx, sy);
    a[g.pos(x) + g.row(y, z)] = (real)0;
}

// ------------------------------------------------------------------ interpolate (+ correct)
// One thread per fine cell of the coarse mesh: the x-pair {2i, 2i+1} of one row (y kept) or of the rows 2j, 2j+1 (y halved) of
// one plane (z kept) or of the planes 2k, 2k+1 (z halved).  Its coarse values are loaded once: columns i, i+1 where x is
// halved, the pair's own two entries where it is kept.  ADD: fine = fine + value (one addition), else fine = value.
template <class real, int MASK, bool ADD>
__global__ void __launch_bounds__(256) interpolate_axes3d_xs_kernel(real* __restrict__ fine, int sx, int sy, int sz,
                                                                    const real* __restrict__ coarse, int cx, int cy, int ncy) {
    constexpr bool HX = (MASK & 1) != 0, HY = (MASK & 2) != 0, HZ = (MASK & 4) != 0;
    constexpr int DY = HY ? 2 : 1, DZ = HZ ? 2 : 1;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int jy = blockIdx.y * blockDim.y + threadIdx.y;
    const int jz = blockIdx.z;
    if (i >= (sx - 1) / 2 || jy >= ncy) return;
    const Geo<XSplit, real> gf(sx, sy), gc(cx, cy);
    const int y0 = HY ? 2 * jy : 1 + jy, z0 = HZ ? 2 * jz : 1 + jz;  // first fine row / plane of the cell
    const int cy0 = HY ? jy : y0, cz0 = HZ ? jz : z0;                // base coarse row / plane
    const int p0 = HX ? gc.pos(i) : i, p1 = HX ? gc.pos(i + 1) : gc.H + i;
    real cv[DZ][DY][2];
#pragma unroll
    for (int dz = 0; dz < DZ; dz++)
#pragma unroll
        for (int dy = 0; dy < DY; dy++) {
            const size_t row = gc.row(cy0 + dy, cz0 + dz);
            cv[dz][dy][0] = coarse[row + p0];
            cv[dz][dy][1] = coarse[row + p1];
        }
#pragma unroll
    for (int oz = 0; oz < DZ; oz++)
#pragma unroll
        for (int oy = 0; oy < DY; oy++)
#pragma unroll
            for (int ox = 0; ox < 2; ox++) {
                const int x = 2 * i + ox, y = y0 + oy, z = z0 + oz;
                if (x == 0 || y == 0 || z == 0) continue;
                const real e = semi_interpolate_point<real>(HX ? ox : 0, oy, oz, [&](int dx, int dy, int dz) __attribute__((always_inline)) {
                    return cv[dz][dy][HX ? dx : ox];
                });
                const size_t fi = gf.row(y, z) + i + ox * gf.H;
                if (ADD) fine[fi] = fine[fi] + e;
                else fine[fi] = e;
            }
}

// ------------------------------------------------------------------ restrict (boundary injected)
template <class real, int MASK>
__global__ void __launch_bounds__(256) restrict_axes3d_xs_kernel(const real* __restrict__ fine, int fx, int fy, real* __restrict__ coarse,
                                                                 int cx, int cy, int cz) {
    constexpr bool HX = (MASK & 1) != 0, HY = (MASK & 2) != 0, HZ = (MASK & 4) != 0;
    const int px = blockIdx.x * blockDim.x + threadIdx.x, py = blockIdx.y * blockDim.y + threadIdx.y, pz = blockIdx.z;
    if (px >= cx || py >= cy) return;
    const Geo<XSplit, real> gf(fx, fy), gc(cx, cy);
    const int x = HX ? 2 * px : px, y = HY ? 2 * py : py, z = HZ ? 2 * pz : pz;
    const size_t ci = gc.pos(px) + gc.row(py, pz);
    if (px == 0 || px == cx - 1 || py == 0 || py == cy - 1 || pz == 0 || pz == cz - 1) {
        coarse[ci] = fine[gf.pos(x) + gf.row(y, z)];  // injection, as Restrict does (N3/MultiGrid3D.cpp:113-119)
        return;
    }
    coarse[ci] = semi_restrict_point<real, MASK>([&](int dx, int dy, int dz) { return fine[gf.pos(x + dx) + gf.row(y + dy, z + dz)]; });
}

// =========================================================================== host side
// the mask of the axes that cn halves (bit 0 = x, 1 = y, 2 = z); MGX_ERR_SIZE when the sizes are no such pair
static int axes_mask(const int fn[3], const int cn[3], const char* what, int* mask) {
    MGX_REQUIRE(fn && cn, MGX_ERR_INVALID, "%s: size array is NULL", what);
    *mask = 0;
    for (int d = 0; d < 3; d++) {
        MGX_REQUIRE(valid_size(fn[d]), MGX_ERR_SIZE, "%s: size[%d] = %d is not odd and >= 3", what, d, fn[d]);
        if (cn[d] == fn[d]) continue;
        MGX_REQUIRE(cn[d] == (fn[d] - 1) / 2 + 1, MGX_ERR_SIZE, "%s: coarse size[%d] = %d is neither %d nor (%d-1)/2+1", what, d, cn[d], fn[d],
                    fn[d]);
        *mask |= 1 << d;
    }
    MGX_REQUIRE(*mask != 0, MGX_ERR_SIZE, "%s: the coarse sizes halve no axis", what);
    MGX_REQUIRE((double)fn[0] * fn[1] * fn[2] < 2147483647.0 * 4, MGX_ERR_SIZE, "%s: grid too large", what);
    return MGX_OK;
}

static inline dim3 blk() { return dim3(64, 4, 1); }

template <class real>
static int restrict_axes3d(mgx_ctx* ctx, const real* fine, const int fn[3], real* coarse, const int cn[3], int mask) {
    MGX_USE(ctx);
    with_value<1, 2, 3, 4, 5, 6>(mask, [&](auto m) __attribute__((always_inline)) {
        MGX_LAUNCH((restrict_axes3d_xs_kernel<real, decltype(m)::value>), dim3(ceil_div(cn[0], 64), ceil_div(cn[1], 4), cn[2]), blk(), 0,
                   ctx->compute, fine, fn[0], fn[1], coarse, cn[0], cn[1], cn[2]);
    });
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

template <class real, bool ADD>
static int interpolate_axes3d(mgx_ctx* ctx, real* fine, const int fn[3], const real* coarse, const int cn[3], int mask) {
    MGX_USE(ctx);
    const int ncy = (mask & 2) ? cn[1] - 1 : fn[1] - 2, ncz = (mask & 4) ? cn[2] - 1 : fn[2] - 2;
    with_value<1, 2, 3, 4, 5, 6>(mask, [&](auto m) __attribute__((always_inline)) {
        MGX_LAUNCH((interpolate_axes3d_xs_kernel<real, decltype(m)::value, ADD>), dim3(ceil_div((fn[0] - 1) / 2, 64), ceil_div(ncy, 4), ncz),
                   blk(), 0, ctx->compute, fine, fn[0], fn[1], fn[2], coarse, cn[0], cn[1], ncy);
    });
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// coarse rows per lane: as many as the register file takes at four waves per SIMD
template <int MASK>
struct AxesRows {
    static constexpr int value = !(MASK & 2) ? 4 : (MASK & 4) ? 1 : 2;
};

template <class real>
static int residual_restrict_axes3d(mgx_ctx* ctx, const real* v, const real* f, const int n[3], const real h[3], int mode, real* coarse_f,
                                    const int cn[3], int mask, int coarse_rim_is_zero) {
    MGX_USE(ctx);
    const ResidualScale<real> s = residual_scale<real>(ctx, h, mode);
    if (!coarse_rim_is_zero)
        MGX_LAUNCH((rim_zero3d_xs_kernel<real>), dim3(ceil_div(cn[0], 64), ceil_div(cn[1], 4), cn[2]), blk(), 0, ctx->compute, coarse_f,
                   cn[0], cn[1], cn[2]);
    if (cn[0] > 2 && cn[1] > 2 && cn[2] > 2) {
        constexpr int TYW = 4;
        with_value<1, 2, 3, 4, 5, 6>(mask, [&](auto m) __attribute__((always_inline)) {
            constexpr int M = decltype(m)::value, CR = AxesRows<M>::value;
            const int gx = (M & 1) ? ceil_div(cn[0] - 2, 63) : ceil_div((n[0] - 1) / 2, 64);
            const int gy = ceil_div(cn[1] - 2, TYW * CR);
            // runs of 16 coarse planes, halved while the launch has fewer than four workgroups per CU
            int pzchunk = 16;
            while (pzchunk > 2 && (long long)gx * gy * ceil_div(cn[2] - 2, pzchunk) < 4LL * ctx->num_cus) pzchunk >>= 1;
            const int gz = ceil_div(cn[2] - 2, pzchunk);
            with_value<0, 1, 2, 3>(s.mode, [&](auto md) __attribute__((always_inline)) {
                MGX_LAUNCH((residual_restrict_axes3d_xs_kernel<real, M, decltype(md)::value, CR, TYW>), dim3((unsigned)(gx * gy * gz)),
                           dim3(64, TYW, 1), 0, ctx->compute, v, f, n[0], n[1], n[2], s.qx, s.qy, s.qz, coarse_f, cn[0], cn[1], cn[2], pzchunk,
                           gx, gy);
            });
        });
    }
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

}  // namespace mgx

#define MGX_SEMI3D_API(SFX, real)                                                                                                       \
    extern "C" int mgx3dxs_restrict_axes_##SFX(mgx_ctx* ctx, const real* fine, const int fn[3], real* coarse, const int cn[3]) {         \
        MGX_REQUIRE(ctx && fine && coarse, MGX_ERR_INVALID, "restrict_axes: NULL argument");                                            \
        int mask = 0;                                                                                                                    \
        MGX_TRY_RET(mgx::axes_mask(fn, cn, "restrict_axes", &mask));                                                                     \
        if (mask == 7) return mgx3dxs_restrict_##SFX(ctx, fine, fn, coarse, cn);                                                         \
        return mgx::restrict_axes3d<real>(ctx, fine, fn, coarse, cn, mask);                                                              \
    }                                                                                                                                    \
    extern "C" int mgx3dxs_interpolate_axes_##SFX(mgx_ctx* ctx, real* fine, const int fn[3], const real* coarse, const int cn[3]) {      \
        MGX_REQUIRE(ctx && fine && coarse, MGX_ERR_INVALID, "interpolate_axes: NULL argument");                                         \
        int mask = 0;                                                                                                                    \
        MGX_TRY_RET(mgx::axes_mask(fn, cn, "interpolate_axes", &mask));                                                                  \
        if (mask == 7) return mgx3dxs_interpolate_##SFX(ctx, fine, fn, coarse, cn);                                                      \
        return mgx::interpolate_axes3d<real, false>(ctx, fine, fn, coarse, cn, mask);                                                    \
    }                                                                                                                                    \
    extern "C" int mgx3dxs_residual_restrict_axes_##SFX(mgx_ctx* ctx, const real* v, const real* f, const int n[3], const real h[3],     \
                                                        int mode, real* coarse_f, const int cn[3], int coarse_rim_is_zero) {            \
        MGX_REQUIRE(ctx && v && f && h && coarse_f, MGX_ERR_INVALID, "residual_restrict_axes: NULL argument");                           \
        MGX_REQUIRE(mode == MGX_RESIDUAL_REF_COMPAT || mode == MGX_RESIDUAL_CORRECT, MGX_ERR_INVALID,                                    \
                    "residual_restrict_axes: bad mode %d", mode);                                                                        \
        int mask = 0;                                                                                                                    \
        MGX_TRY_RET(mgx::axes_mask(n, cn, "residual_restrict_axes", &mask));                                                             \
        if (mask == 7)                                                                                                                   \
            return coarse_rim_is_zero ? mgx3dxs_residual_restrict_keep_rim_##SFX(ctx, v, f, n, h, mode, coarse_f, cn)                    \
                                      : mgx3dxs_residual_restrict_##SFX(ctx, v, f, n, h, mode, coarse_f, cn);                            \
        return mgx::residual_restrict_axes3d<real>(ctx, v, f, n, h, mode, coarse_f, cn, mask, coarse_rim_is_zero);                       \
    }                                                                                                                                    \
    extern "C" int mgx3dxs_interpolate_correct_axes_##SFX(mgx_ctx* ctx, real* v, const int n[3], const real* coarse_v, const int cn[3]) { \
        MGX_REQUIRE(ctx && v && coarse_v, MGX_ERR_INVALID, "interpolate_correct_axes: NULL argument");                                   \
        int mask = 0;                                                                                                                    \
        MGX_TRY_RET(mgx::axes_mask(n, cn, "interpolate_correct_axes", &mask));                                                           \
        if (mask == 7) return mgx3dxs_interpolate_correct_##SFX(ctx, v, n, coarse_v, cn);                                                \
        return mgx::interpolate_axes3d<real, true>(ctx, v, n, coarse_v, cn, mask);                                                       \
    }

MGX_SEMI3D_API(f32, float)
MGX_SEMI3D_API(f64, double)
