// mgx_krylov3d.hip -- the vector kernels of the multigrid-preconditioned flexible CG solve (mgMultiGrid3D_<r>_PCG), x-split layout.
// An addition: the reference has no Krylov solver.
//
// All four kernels stream interior points only (boundary and pad entries are neither read as data nor written) and walk the
// arrays the same way: one wavefront per x-row (y, z), its lanes over the row's storage positions j in [0, P) (the even-x
// half, then the odd-x half from H on), so every access of a wave is one contiguous run of a half-row.  Each lane handles
// KJ positions per step, loads first, so that KJ loads per array are in flight.  Reductions are accumulated in double in a
// fixed order: per lane in loop order, wavefront-wide shuffles, the block's four waves in a fixed order into one partial per
// block, then cg_final_kernel adds the partials in a fixed order -- the same bits on every run.
//
//   laplace_dot3d_xs_kernel   q = A p (A = the CORRECT-mode Laplacian, q = -residual(p, f = 0)), partials of <p, q>
//   cg_update3d_xs_kernel     [x += alpha p;] r -= alpha q, partials of <r, r>
//   dot2_3d_xs_kernel         partials of <a, b> and <a, c>
//   cg_direction3d_xs_kernel  [x += alpha p;] p = z + beta p   (or p = z)
//   cg_final_kernel           sum of the partials -> device double(s)
//   cg_scalars_kernel         alpha / beta of the iteration from the sums (one thread)
#include "mgx_internal.hpp"
#include "mgx_kernels3d.hpp"

namespace mgx {

constexpr int KJ = 4;          // positions per lane and step
constexpr int KROWS = 4;       // rows (waves) per block
constexpr int KSTEP = 64 * KJ; // positions of a row per wave and step

// x of storage position j of an x-split row (pads give x >= sx)
__device__ __forceinline__ int xs_x(int j, int H) { return j < H ? 2 * j : 2 * (j - H) + 1; }

// the wave's sum into part[wave]; the block then combines its four waves in a fixed order
__device__ __forceinline__ void wave_sum(double acc, double* part) {
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (threadIdx.x == 0) part[threadIdx.y] = acc;
}

template <class real, int MODE>
__global__ void __launch_bounds__(256) laplace_dot3d_xs_kernel(const real* __restrict__ p, real* __restrict__ q, int sx, int sy,
                                                               real hx2, real hy2, real hz2, double* __restrict__ partial) {
    const Geo<XSplit, real> g(sx, sy);
    const int y = 1 + blockIdx.x * KROWS + threadIdx.y, z = 1 + blockIdx.y;
    const int H = g.H, P = g.P;
    const size_t PL = g.PL;
    double acc = 0.0;
    if (y < sy - 1) {
        const size_t row = g.row(y, z);
        for (int j0 = 0; j0 < P; j0 += KSTEP) {
            real O[KJ], E[KJ], N[KJ], S[KJ], D[KJ], U[KJ], c[KJ];
            bool in[KJ];
#pragma unroll
            for (int k = 0; k < KJ; k++) {
                const int j = j0 + k * 64 + threadIdx.x, x = xs_x(j, H);
                in[k] = j < P && x >= 1 && x <= sx - 2;
                if (in[k]) {
                    const size_t i = row + j;
                    O[k] = p[row + XSplit::pos(x - 1, H)];
                    E[k] = p[row + XSplit::pos(x + 1, H)];
                    N[k] = p[i - P];
                    S[k] = p[i + P];
                    D[k] = p[i - PL];
                    U[k] = p[i + PL];
                    c[k] = p[i];
                }
            }
#pragma unroll
            for (int k = 0; k < KJ; k++)
                if (in[k]) {
                    // -residual3d(p, f = 0): the residual's own expression, negated (negation is exact)
                    const real t = -residual3d_point<real, MODE>(O[k], E[k], N[k], S[k], D[k], U[k], c[k], (real)0, hx2, hy2, hz2);
                    q[row + j0 + k * 64 + threadIdx.x] = t;
                    acc += (double)c[k] * (double)t;
                }
        }
    }
    __shared__ double part[1][KROWS];
    wave_sum(acc, part[0]);
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
}

template <class real, bool X>
__global__ void __launch_bounds__(256) cg_update3d_xs_kernel(real* __restrict__ x, const real* __restrict__ p, real* __restrict__ r,
                                                             const real* __restrict__ q, int sx, int sy,
                                                             const double* __restrict__ dev_alpha, double* __restrict__ partial) {
    const Geo<XSplit, real> g(sx, sy);
    const int y = 1 + blockIdx.x * KROWS + threadIdx.y, z = 1 + blockIdx.y;
    const int H = g.H, P = g.P;
    const real a = (real)*dev_alpha;
    double acc = 0.0;
    if (y < sy - 1) {
        const size_t row = g.row(y, z);
        for (int j0 = 0; j0 < P; j0 += KSTEP) {
            real xv[KJ], pv[KJ], rv[KJ], qv[KJ];
            bool in[KJ];
#pragma unroll
            for (int k = 0; k < KJ; k++) {
                const int j = j0 + k * 64 + threadIdx.x, xx = xs_x(j, H);
                in[k] = j < P && xx >= 1 && xx <= sx - 2;
                if (in[k]) {
                    const size_t i = row + j;
                    if (X) {
                        xv[k] = x[i];
                        pv[k] = p[i];
                    }
                    rv[k] = r[i];
                    qv[k] = q[i];
                }
            }
#pragma unroll
            for (int k = 0; k < KJ; k++)
                if (in[k]) {
                    const size_t i = row + j0 + k * 64 + threadIdx.x;
                    if (X) x[i] = xv[k] + a * pv[k];
                    const real t = rv[k] - a * qv[k];
                    r[i] = t;
                    acc += (double)t * (double)t;
                }
        }
    }
    __shared__ double part[1][KROWS];
    wave_sum(acc, part[0]);
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
}

// partials of <a, b> at partial[block] and, with TWO, of <a, c> at partial[nblocks + block]
template <class real, bool TWO>
__global__ void __launch_bounds__(256) dot2_3d_xs_kernel(const real* __restrict__ a, const real* __restrict__ b, const real* __restrict__ c,
                                                         int sx, int sy, double* __restrict__ partial) {
    const Geo<XSplit, real> g(sx, sy);
    const int y = 1 + blockIdx.x * KROWS + threadIdx.y, z = 1 + blockIdx.y;
    const int H = g.H, P = g.P;
    double ab = 0.0, ac = 0.0;
    if (y < sy - 1) {
        const size_t row = g.row(y, z);
        for (int j0 = 0; j0 < P; j0 += KSTEP) {
            real av[KJ], bv[KJ], cv[KJ];
            bool in[KJ];
#pragma unroll
            for (int k = 0; k < KJ; k++) {
                const int j = j0 + k * 64 + threadIdx.x, xx = xs_x(j, H);
                in[k] = j < P && xx >= 1 && xx <= sx - 2;
                if (in[k]) {
                    const size_t i = row + j;
                    av[k] = a[i];
                    bv[k] = b[i];
                    if (TWO) cv[k] = c[i];
                }
            }
#pragma unroll
            for (int k = 0; k < KJ; k++)
                if (in[k]) {
                    ab += (double)av[k] * (double)bv[k];
                    if (TWO) ac += (double)av[k] * (double)cv[k];
                }
        }
    }
    __shared__ double part[2][KROWS];
    wave_sum(ab, part[0]);
    if (TWO) wave_sum(ac, part[1]);
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        const size_t nb = (size_t)gridDim.x * gridDim.y, blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        partial[blk] = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
        if (TWO) partial[nb + blk] = (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
    }
}

// X: x += alpha p (the old p); P_: p = z + beta p (BETA) or p = z
template <class real, bool X, bool P_, bool BETA>
__global__ void __launch_bounds__(256) cg_direction3d_xs_kernel(real* __restrict__ x, real* __restrict__ p, const real* __restrict__ z,
                                                                int sx, int sy, const double* __restrict__ dev_alpha,
                                                                const double* __restrict__ dev_beta) {
    const Geo<XSplit, real> g(sx, sy);
    const int y = 1 + blockIdx.x * KROWS + threadIdx.y, zz = 1 + blockIdx.y;
    if (y >= sy - 1) return;
    const int H = g.H, P = g.P;
    const real a = X ? (real)*dev_alpha : (real)0, b = BETA ? (real)*dev_beta : (real)0;
    const size_t row = g.row(y, zz);
    for (int j0 = 0; j0 < P; j0 += KSTEP) {
        real xv[KJ], pv[KJ], zv[KJ];
        bool in[KJ];
#pragma unroll
        for (int k = 0; k < KJ; k++) {
            const int j = j0 + k * 64 + threadIdx.x, xx = xs_x(j, H);
            in[k] = j < P && xx >= 1 && xx <= sx - 2;
            if (in[k]) {
                const size_t i = row + j;
                if (X) xv[k] = x[i];
                if (X || BETA) pv[k] = p[i];
                if (P_) zv[k] = z[i];
            }
        }
#pragma unroll
        for (int k = 0; k < KJ; k++)
            if (in[k]) {
                const size_t i = row + j0 + k * 64 + threadIdx.x;
                if (X) x[i] = xv[k] + a * pv[k];
                if (P_) p[i] = BETA ? zv[k] + b * pv[k] : zv[k];
            }
    }
}

// out[s] = sum of partial[s * count .. (s + 1) * count), one block per sum, fixed order
__global__ void __launch_bounds__(1024) cg_final_kernel(const double* __restrict__ partial, size_t count, double* __restrict__ out) {
    __shared__ double s[1024];
    const double* pp = partial + (size_t)blockIdx.x * count;
    double acc = 0.0;
    for (size_t i = threadIdx.x; i < count; i += 1024) acc += pp[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = s[0];
}

// the scalar steps of flexible CG on the state vector of mgx.h (MGX_CG_*)
__global__ void cg_scalars_kernel(double* s, int step) {
    if (step == 0) {  // alpha = <r,z> / <p,q>; a breakdown leaves NaN, which the update turns into a NaN norm
        const double pq = s[MGX_CG_PQ], al = s[MGX_CG_RZ] / pq;
        s[MGX_CG_ALPHA] = (pq == 0.0 || !__builtin_isfinite(pq) || !__builtin_isfinite(al)) ? __builtin_nan("") : al;
    } else if (step == 1) {  // beta = -alpha <z,q> / <r,z>_old (Polak-Ribiere), then <r,z> := <r,z>_new
        s[MGX_CG_BETA] = -s[MGX_CG_ALPHA] * s[MGX_CG_ZQ] / s[MGX_CG_RZ];
        s[MGX_CG_RZ] = s[MGX_CG_ZR];
    } else {  // restart: <r,z> := <r,z>_new
        s[MGX_CG_RZ] = s[MGX_CG_ZR];
    }
}

// ------------------------------------------------------------------ host side
static int krylov_check(const int n[3], const char* what) {
    MGX_REQUIRE(n, MGX_ERR_INVALID, "%s: NULL size", what);
    for (int d = 0; d < 3; d++)
        MGX_REQUIRE(valid_size(n[d]), MGX_ERR_SIZE, "%s: size[%d] = %d is not odd and >= 3", what, d, n[d]);
    MGX_REQUIRE(n[2] - 2 <= 65535, MGX_ERR_SIZE, "%s: %d planes are too many", what, n[2]);
    return MGX_OK;
}
static dim3 krylov_grid(const int n[3]) { return dim3((unsigned)ceil_div(n[1] - 2, KROWS), (unsigned)(n[2] - 2)); }
static dim3 krylov_block() { return dim3(64, KROWS, 1); }

size_t krylov_work_elems(const int n[3]) {
    if (krylov_check(n, "krylov_work_elems")) return 0;
    const dim3 g = krylov_grid(n);
    return 2 * (size_t)g.x * g.y;
}

static int krylov_final(mgx_ctx* ctx, const double* work, size_t count, int nsums, double* dev_sum) {
    MGX_LAUNCH(cg_final_kernel, dim3(nsums), dim3(1024), 0, ctx->compute, work, count, dev_sum);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

template <class real>
int laplace_dot3d(mgx_ctx* ctx, const real* p, real* q, const int n[3], const real h[3], double* dev_work, double* dev_sum) {
    MGX_REQUIRE(ctx && p && q && h && dev_work && dev_sum, MGX_ERR_INVALID, "laplace_dot: NULL argument");
    MGX_USE(ctx);
    MGX_TRY_RET(krylov_check(n, "laplace_dot"));
    const ResidualScale<real> s = residual_scale<real>(ctx, h, MGX_RESIDUAL_CORRECT);  // as mgx3dxs_residual forms them: MODE 1 or 3
    const dim3 g = krylov_grid(n);
    with_value<1, 3>(s.mode, [&](auto m) __attribute__((always_inline)) {
        MGX_LAUNCH((laplace_dot3d_xs_kernel<real, decltype(m)::value>), g, krylov_block(), 0, ctx->compute, p, q, n[0], n[1], s.qx, s.qy,
                   s.qz, dev_work);
    });
    MGX_LAUNCH_CHECK();
    return krylov_final(ctx, dev_work, (size_t)g.x * g.y, 1, dev_sum);
}

template <class real>
int cg_update3d(mgx_ctx* ctx, real* x, const real* p, real* r, const real* q, const int n[3], const double* dev_alpha, double* dev_work,
                double* dev_sum) {
    MGX_REQUIRE(ctx && r && q && (!x || p) && dev_alpha && dev_work && dev_sum, MGX_ERR_INVALID, "cg_update: NULL argument");
    MGX_USE(ctx);
    MGX_TRY_RET(krylov_check(n, "cg_update"));
    const dim3 g = krylov_grid(n);
    if (x) MGX_LAUNCH((cg_update3d_xs_kernel<real, true>), g, krylov_block(), 0, ctx->compute, x, p, r, q, n[0], n[1], dev_alpha, dev_work);
    else MGX_LAUNCH((cg_update3d_xs_kernel<real, false>), g, krylov_block(), 0, ctx->compute, x, p, r, q, n[0], n[1], dev_alpha, dev_work);
    MGX_LAUNCH_CHECK();
    return krylov_final(ctx, dev_work, (size_t)g.x * g.y, 1, dev_sum);
}

template <class real>
int dot2_3d(mgx_ctx* ctx, const real* a, const real* b, const real* c, const int n[3], double* dev_work, double* dev_sum) {
    MGX_REQUIRE(ctx && a && b && dev_work && dev_sum, MGX_ERR_INVALID, "dot2: NULL argument");
    MGX_USE(ctx);
    MGX_TRY_RET(krylov_check(n, "dot2"));
    const dim3 g = krylov_grid(n);
    if (c) MGX_LAUNCH((dot2_3d_xs_kernel<real, true>), g, krylov_block(), 0, ctx->compute, a, b, c, n[0], n[1], dev_work);
    else MGX_LAUNCH((dot2_3d_xs_kernel<real, false>), g, krylov_block(), 0, ctx->compute, a, b, c, n[0], n[1], dev_work);
    MGX_LAUNCH_CHECK();
    return krylov_final(ctx, dev_work, (size_t)g.x * g.y, c ? 2 : 1, dev_sum);
}

template <class real>
int cg_direction3d(mgx_ctx* ctx, real* x, real* p, const real* z, const int n[3], const double* dev_alpha, const double* dev_beta) {
    MGX_REQUIRE(ctx && p && (!x || dev_alpha), MGX_ERR_INVALID, "cg_direction: NULL argument");
    MGX_REQUIRE(x || z, MGX_ERR_INVALID, "cg_direction: nothing to do (x and z are NULL)");
    MGX_USE(ctx);
    MGX_TRY_RET(krylov_check(n, "cg_direction"));
    const dim3 g = krylov_grid(n);
#define MGX_DIR(X, P_, B)                                                                                                     \
    MGX_LAUNCH((cg_direction3d_xs_kernel<real, X, P_, B>), g, krylov_block(), 0, ctx->compute, x, p, z, n[0], n[1], dev_alpha, \
               dev_beta)
    if (!z) MGX_DIR(true, false, false);
    else if (x && dev_beta) MGX_DIR(true, true, true);
    else if (x) MGX_DIR(true, true, false);
    else if (dev_beta) MGX_DIR(false, true, true);
    else MGX_DIR(false, true, false);
#undef MGX_DIR
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

}  // namespace mgx

extern "C" {

int mgx_cg_scalars(mgx_ctx* ctx, double* dev_state, int step) {
    MGX_REQUIRE(ctx && dev_state, MGX_ERR_INVALID, "cg_scalars: NULL argument");
    MGX_REQUIRE(step >= 0 && step <= 2, MGX_ERR_INVALID, "cg_scalars: bad step %d", step);
    MGX_USE(ctx);
    MGX_LAUNCH(mgx::cg_scalars_kernel, dim3(1), dim3(1), 0, ctx->compute, dev_state, step);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

#define MGX_STAMP_KRYLOV(SFX, real)                                                                                           \
    size_t mgx3dxs_krylov_work_elems_##SFX(const int n[3]) { return mgx::krylov_work_elems(n); }                                \
    int mgx3dxs_laplace_dot_##SFX(mgx_ctx* ctx, const real* p, real* q, const int n[3], const real h[3], double* dev_work,       \
                                  double* dev_sum) {                                                                          \
        return mgx::laplace_dot3d<real>(ctx, p, q, n, h, dev_work, dev_sum);                                                  \
    }                                                                                                                         \
    int mgx3dxs_cg_update_##SFX(mgx_ctx* ctx, real* x, const real* p, real* r, const real* q, const int n[3],                  \
                                const double* dev_alpha, double* dev_work, double* dev_sum) {                                 \
        return mgx::cg_update3d<real>(ctx, x, p, r, q, n, dev_alpha, dev_work, dev_sum);                                      \
    }                                                                                                                         \
    int mgx3dxs_dot2_##SFX(mgx_ctx* ctx, const real* a, const real* b, const real* c, const int n[3], double* dev_work,         \
                           double* dev_sum) {                                                                                 \
        return mgx::dot2_3d<real>(ctx, a, b, c, n, dev_work, dev_sum);                                                        \
    }                                                                                                                         \
    int mgx3dxs_cg_direction_##SFX(mgx_ctx* ctx, real* x, real* p, const real* z, const int n[3], const double* dev_alpha,      \
                                   const double* dev_beta) {                                                                  \
        return mgx::cg_direction3d<real>(ctx, x, p, z, n, dev_alpha, dev_beta);                                               \
    }
MGX_STAMP_KRYLOV(f32, float)
MGX_STAMP_KRYLOV(f64, double)
#undef MGX_STAMP_KRYLOV

}  // extern "C"
