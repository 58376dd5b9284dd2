// mgx_semi3d.hpp -- what the transfers of a semi-coarsened step share with the shifted operators (mgx_shift3d.hip): the
// restriction stencils and the streaming residual + restrict kernel.  See mgx_semi3d.hip.
#pragma once
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
// SHIFT (mgx_shift3d.hip): the residual of (Laplacian - s) v = f, i.e. s * v is added to every residual; with it the kernel also
// takes MASK = 7, where the restriction is the reference's full weighting (restrict3d_point).
template <class real, int MASK, int MODE, int CR, int TYW, bool SHIFT = false>
__global__ void __launch_bounds__(64 * TYW)
    residual_restrict_axes3d_xs_kernel(const real* __restrict__ v, const real* __restrict__ f, int sx, int sy, int sz, real qx, real qy,
                                       real qz, real* __restrict__ coarse, int cx, int cy, int cz, int pzchunk, int gx, int gy, real s = 0) {
    static_assert(MASK != 7 || SHIFT, "all three axes halved: residual_restrict3d_xs_kernel");
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
            real a = residual3d_point<real, MODE>(Bl, BC[r], AC[r - 1], AC[r + 1], AP[r], AN[r], AC[r], fA, qx, qy, qz);
            real b = residual3d_point<real, MODE>(AC[r], Ar, BC[r - 1], BC[r + 1], BP[r], BN[r], BC[r], fB, qx, qy, qz);
            if constexpr (SHIFT) {
                a = a + s * AC[r];
                b = b + s * BC[r];
            }
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
                    auto get = [&](int dx, int dy, int dz) __attribute__((always_inline)) {
                        return dx < 0 ? lB[K0 + dz][rc + dy] : dx > 0 ? rB[K0 + dz][rc + dy] : rA[K0 + dz][rc + dy];
                    };
                    real e;
                    if constexpr (MASK == 7) e = restrict3d_point<real>(get);
                    else e = semi_restrict_point<real, MASK>(get);
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

// coarse rows per lane: as many as the register file takes at four waves per SIMD
template <int MASK>
struct AxesRows {
    static constexpr int value = !(MASK & 2) ? 4 : (MASK & 4) ? 1 : 2;
};

}  // namespace mgx
