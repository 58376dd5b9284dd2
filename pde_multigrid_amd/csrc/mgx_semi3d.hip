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
//   rim_zero3d_xs_kernel                 boundary points := 0; the operators of mgx_stencil3d.hpp call rim_zero3d_xs (mgx_host3d.hpp)
// The stencils and the first kernel live in mgx_semi3d.hpp: mgx_shift3d.hip instantiates that kernel with a shift.
#include "mgx_host3d.hpp"
#include "mgx_semi3d.hpp"

namespace mgx {

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

// boundary points of an x-split array := 0 (pads are not touched)
template <class real>
__global__ void __launch_bounds__(256) rim_zero3d_xs_kernel(real* __restrict__ a, int sx, int sy, int sz) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y, z = blockIdx.z;
    if (x >= sx || y >= sy) return;
    if (!(x == 0 || x == sx - 1 || y == 0 || y == sy - 1 || z == 0 || z == sz - 1)) return;
    const Geo<XSplit, real> g(sx, sy);
    a[g.pos(x) + g.row(y, z)] = (real)0;
}

// =========================================================================== host side
template <class real>
void rim_zero3d_xs(mgx_ctx* ctx, real* a, const int n[3]) {
    MGX_LAUNCH((rim_zero3d_xs_kernel<real>), dim3(ceil_div(n[0], 64), ceil_div(n[1], 4), n[2]), blk(), 0, ctx->compute, a, n[0], n[1], n[2]);
}
template void rim_zero3d_xs<float>(mgx_ctx*, float*, const int[3]);
template void rim_zero3d_xs<double>(mgx_ctx*, double*, const int[3]);

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

template <class real>
static int residual_restrict_axes3d(mgx_ctx* ctx, const real* v, const real* f, const int n[3], const real h[3], int mode, real* coarse_f,
                                    const int cn[3], int mask, int coarse_rim_is_zero) {
    MGX_USE(ctx);
    const ResidualScale<real> s = residual_scale<real>(ctx, h, mode);
    if (!coarse_rim_is_zero)
        rim_zero3d_xs<real>(ctx, coarse_f, cn);
    if (cn[0] > 2 && cn[1] > 2 && cn[2] > 2) {
        constexpr int TYW = 4;
        with_value<1, 2, 3, 4, 5, 6>(mask, [&](auto m) __attribute__((always_inline)) {
            constexpr int M = decltype(m)::value, CR = AxesRows<M>::value;
            const int gx = (M & 1) ? ceil_div(cn[0] - 2, 63) : ceil_div((n[0] - 1) / 2, 64);
            const int gy = ceil_div(cn[1] - 2, TYW * CR);
            // runs of 16 coarse planes, halved while the launch has fewer than four workgroups per CU
            int pzchunk = 16;
            if (ctx->rr_pzchunk > 0) pzchunk = ctx->rr_pzchunk;  // "residual_restrict3d.pzchunk": the same bits for every run length
            else
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
