// mgx_krylov3d.hip -- the vector kernels of the multigrid-preconditioned flexible CG solve (mgMultiGrid3D_<r>_PCG), x-split layout.
// An addition: the reference has no Krylov solver.
//
// All four kernels stream interior points only (boundary and pad entries are neither read as data nor written) and walk the
// arrays the same way, the row walk of mgx_stencil3d.hpp, with its fixed-order sums -- the same bits on every run.
//
//   residual_op3d_xs_kernel<real, PlainOp, MODE, true> (mgx_stencil3d.hpp)
//                             q = A p (A = the CORRECT-mode Laplacian, q = -residual(p, f = 0)), partials of <p, q>
//   cg_update3d_xs_kernel     [x += alpha p;] r -= alpha q, partials of <r, r>
//   dot2_3d_xs_kernel         partials of <a, b> and <a, c>
//   cg_direction3d_xs_kernel  [x += alpha p;] p = z + beta p   (or p = z)
//   cg_final_kernel           sum of the partials -> device double(s)
//   cg_scalars_kernel         alpha / beta of the iteration from the sums (one thread)
//
// Below them the kernels of the mixed-precision solve (mgMultiGrid3D_f64_PCG_mixed), which read or write the fp32 twin's arrays.
#include "mgx_internal.hpp"
#include "mgx_stencil3d.hpp"

namespace mgx {

// the CORRECT-mode Laplacian, for q = A p alone: the residual's own expression and nothing added (a shift of 0 would change the
// sign of a zero residual)
template <class real>
struct PlainOp {
    static constexpr bool HAS_A = false, HAS_S = false, HAS_C = false;
    real qx, qy, qz;  // as mgx3dxs_residual forms them: residual_scale's, MODE 1, or 3 with exact reciprocals
    int mode;
    PlainOp(const mgx_ctx* ctx, const real h[3], real) {
        const ResidualScale<real> sc = residual_scale<real>(ctx, h, MGX_RESIDUAL_CORRECT);
        qx = sc.qx, qy = sc.qy, qz = sc.qz, mode = sc.mode;
    }
    template <class F>
    static void with_mode(int mode, F&& f) {
        with_value<1, 3>(mode, f);
    }
    template <int MODE>
    __device__ __forceinline__ real residual(const Star7<real>& v, real f, const Star7<real>&) const {
        return residual3d_point<real, MODE>(v.O, v.E, v.N, v.S, v.D, v.U, v.C, f, qx, qy, qz);
    }
};

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
    __shared__ double part[KROWS];
    block_sum(acc, part, partial);
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


// ------------------------------------------------------------------ mixed precision (mgMultiGrid3D_f64_PCG_mixed)
// The iterate, the residual and every sum stay fp64; the preconditioner's right-hand side r32 and its result z32 are fp32
// arrays of the fp32 twin hierarchy.  The two precisions have different x-split geometries (at 513 points per row fp64 has
// H = 272, P = 528, fp32 H = 288, P = 544): every array is addressed through its own Geo, and within a half-row both are
// contiguous, so every wave access stays one coalesced run.  s is a power of two (the host's scaling rule): r32 = (float)(r s)
// and z = (double)z32 * (1 / s) are then exact rescalings, and the V-cycle being linear, M(s r) / s = M(r) bit for bit.
//
//   demote3d_xs_kernel                      r32 = (float)(r s)
//   cg_update_demote3d_xs_kernel            [x += alpha p;] r -= alpha q, r32 = (float)(r s), partials of <r, r>
//   dot2_mixed3d_xs_kernel                  partials of <z, b> and <z, c>, z = (double)z32 * (1 / s)
//   cg_direction_mixed3d_xs_kernel          [x += alpha p;] p = z + beta p (or p = z), z = (double)z32 * (1 / s)
//   correct_mixed3d_xs_kernel               xo = x + z (the first launch of the two-launch form of the next kernel)
//   correct_residual_demote3d_xs_kernel     [xo = x + z;] r = b - A xo, r32 = (float)(r s), partials of <r, r>: z-marching

// fp32 storage position of the point at fp64 storage position j of the same row
__device__ __forceinline__ int xs_j32(int j, int H, int H32) { return j < H ? j : j - H + H32; }

__global__ void __launch_bounds__(256) demote3d_xs_kernel(const double* __restrict__ r, float* __restrict__ r32, int sx, int sy,
                                                          double s) {
    const Geo<XSplit, double> g(sx, sy);
    const Geo<XSplit, float> g32(sx, sy);
    const int y = 1 + blockIdx.x * KROWS + threadIdx.y, z = 1 + blockIdx.y;
    if (y >= sy - 1) return;
    const int H = g.H, P = g.P, H32 = g32.H;
    const size_t row = g.row(y, z), row32 = g32.row(y, z);
    for (int j0 = 0; j0 < P; j0 += KSTEP) {
        double rv[KJ];
        bool in[KJ];
#pragma unroll
        for (int k = 0; k < KJ; k++) {
            const int j = j0 + k * 64 + threadIdx.x, x = xs_x(j, H);
            in[k] = j < P && x >= 1 && x <= sx - 2;
            if (in[k]) rv[k] = r[row + j];
        }
#pragma unroll
        for (int k = 0; k < KJ; k++)
            if (in[k]) r32[row32 + xs_j32(j0 + k * 64 + threadIdx.x, H, H32)] = (float)(rv[k] * s);
    }
}

template <bool X>
__global__ void __launch_bounds__(256) cg_update_demote3d_xs_kernel(double* __restrict__ x, const double* __restrict__ p,
                                                                    double* __restrict__ r, const double* __restrict__ q,
                                                                    float* __restrict__ r32, int sx, int sy, double s,
                                                                    const double* __restrict__ dev_alpha, double* __restrict__ partial) {
    const Geo<XSplit, double> g(sx, sy);
    const Geo<XSplit, float> g32(sx, sy);
    const int y = 1 + blockIdx.x * KROWS + threadIdx.y, z = 1 + blockIdx.y;
    const int H = g.H, P = g.P, H32 = g32.H;
    const double a = *dev_alpha;
    double acc = 0.0;
    if (y < sy - 1) {
        const size_t row = g.row(y, z), row32 = g32.row(y, z);
        for (int j0 = 0; j0 < P; j0 += KSTEP) {
            double xv[KJ], pv[KJ], rv[KJ], qv[KJ];
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
                    const int j = j0 + k * 64 + threadIdx.x;
                    if (X) x[row + j] = xv[k] + a * pv[k];
                    const double t = rv[k] - a * qv[k];
                    r[row + j] = t;
                    r32[row32 + xs_j32(j, H, H32)] = (float)(t * s);
                    acc += t * t;
                }
        }
    }
    __shared__ double part[KROWS];
    block_sum(acc, part, partial);
}

// partials of <z, b> at partial[block] and, with TWO, of <z, c> at partial[nblocks + block]
template <bool TWO>
__global__ void __launch_bounds__(256) dot2_mixed3d_xs_kernel(const float* __restrict__ z32, double inv_s, const double* __restrict__ b,
                                                              const double* __restrict__ c, int sx, int sy, double* __restrict__ partial) {
    const Geo<XSplit, double> g(sx, sy);
    const Geo<XSplit, float> g32(sx, sy);
    const int y = 1 + blockIdx.x * KROWS + threadIdx.y, z = 1 + blockIdx.y;
    const int H = g.H, P = g.P, H32 = g32.H;
    double zb = 0.0, zc = 0.0;
    if (y < sy - 1) {
        const size_t row = g.row(y, z), row32 = g32.row(y, z);
        for (int j0 = 0; j0 < P; j0 += KSTEP) {
            double zv[KJ], bv[KJ], cv[KJ];
            bool in[KJ];
#pragma unroll
            for (int k = 0; k < KJ; k++) {
                const int j = j0 + k * 64 + threadIdx.x, xx = xs_x(j, H);
                in[k] = j < P && xx >= 1 && xx <= sx - 2;
                if (in[k]) {
                    zv[k] = (double)z32[row32 + xs_j32(j, H, H32)] * inv_s;
                    bv[k] = b[row + j];
                    if (TWO) cv[k] = c[row + j];
                }
            }
#pragma unroll
            for (int k = 0; k < KJ; k++)
                if (in[k]) {
                    zb += zv[k] * bv[k];
                    if (TWO) zc += zv[k] * cv[k];
                }
        }
    }
    __shared__ double part[2][KROWS];
    wave_sum(zb, part[0]);
    if (TWO) wave_sum(zc, part[1]);
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        const size_t nb = (size_t)gridDim.x * gridDim.y, blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        partial[blk] = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
        if (TWO) partial[nb + blk] = (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
    }
}

// X: x += alpha p (the old p); p = z + beta p (BETA) or p = z
template <bool X, bool BETA>
__global__ void __launch_bounds__(256) cg_direction_mixed3d_xs_kernel(double* __restrict__ x, double* __restrict__ p,
                                                                      const float* __restrict__ z32, double inv_s, int sx, int sy,
                                                                      const double* __restrict__ dev_alpha,
                                                                      const double* __restrict__ dev_beta) {
    const Geo<XSplit, double> g(sx, sy);
    const Geo<XSplit, float> g32(sx, sy);
    const int y = 1 + blockIdx.x * KROWS + threadIdx.y, zz = 1 + blockIdx.y;
    if (y >= sy - 1) return;
    const int H = g.H, P = g.P, H32 = g32.H;
    const double a = X ? *dev_alpha : 0.0, b = BETA ? *dev_beta : 0.0;
    const size_t row = g.row(y, zz), row32 = g32.row(y, zz);
    for (int j0 = 0; j0 < P; j0 += KSTEP) {
        double xv[KJ], pv[KJ], zv[KJ];
        bool in[KJ];
#pragma unroll
        for (int k = 0; k < KJ; k++) {
            const int j = j0 + k * 64 + threadIdx.x, xx = xs_x(j, H);
            in[k] = j < P && xx >= 1 && xx <= sx - 2;
            if (in[k]) {
                if (X) xv[k] = x[row + j];
                if (X || BETA) pv[k] = p[row + j];
                zv[k] = (double)z32[row32 + xs_j32(j, H, H32)] * inv_s;
            }
        }
#pragma unroll
        for (int k = 0; k < KJ; k++)
            if (in[k]) {
                const size_t i = row + j0 + k * 64 + threadIdx.x;
                if (X) x[i] = xv[k] + a * pv[k];
                p[i] = BETA ? zv[k] + b * pv[k] : zv[k];
            }
    }
}

// xo = x + (double)z32 * (1 / s) on the interior
__global__ void __launch_bounds__(256) correct_mixed3d_xs_kernel(const double* __restrict__ x, double* __restrict__ xo,
                                                                 const float* __restrict__ z32, double inv_s, int sx, int sy) {
    const Geo<XSplit, double> g(sx, sy);
    const Geo<XSplit, float> g32(sx, sy);
    const int y = 1 + blockIdx.x * KROWS + threadIdx.y, zz = 1 + blockIdx.y;
    if (y >= sy - 1) return;
    const int H = g.H, P = g.P, H32 = g32.H;
    const size_t row = g.row(y, zz), row32 = g32.row(y, zz);
    for (int j0 = 0; j0 < P; j0 += KSTEP) {
        double xv[KJ], zv[KJ];
        bool in[KJ];
#pragma unroll
        for (int k = 0; k < KJ; k++) {
            const int j = j0 + k * 64 + threadIdx.x, xx = xs_x(j, H);
            in[k] = j < P && xx >= 1 && xx <= sx - 2;
            if (in[k]) {
                xv[k] = x[row + j];
                zv[k] = (double)z32[row32 + xs_j32(j, H, H32)] * inv_s;
            }
        }
#pragma unroll
        for (int k = 0; k < KJ; k++)
            if (in[k]) xo[row + j0 + k * 64 + threadIdx.x] = xv[k] + zv[k];
    }
}

// The hot pass of the mixed defect correction: [xo = x + (double)z32 / s on the interior;] r = b - A xo; r32 = (float)(r s);
// partials of <r, r>.  Built like residual_restrict3d_xs_kernel: lane i of a wave owns the x-pair {2i, 2i+1} (storage
// positions i and H + i) of TR consecutive rows plus one halo row on either side and marches through a chunk of planes;
// the corrected x of three planes stays in registers, plane k+1 is corrected as it is loaded and plane k's residual is
// formed from it.  The x-neighbours come from the adjacent lanes by wave shuffle (lane 63 loads x = 2i + 2 itself), the
// y-halo rows and the halo plane on either side of the chunk are corrected redundantly.  Lane 0 of a wave only supplies
// x = 2i - 1 to lane 1 (the next wave's lane 0 is this wave's lane 63), so a wave produces 63 columns.  The correction is
// out of place: a neighbour's halo row must still read the uncorrected x, so xo != x, and xo's boundary is the caller's
// (the kernel writes interior points only).  Without CORR the residual is that of x itself and nothing but r32 is stored.
template <int MODE, bool CORR, int TR, int TYW>
__global__ void __launch_bounds__(64 * TYW)
    correct_residual_demote3d_xs_kernel(const double* __restrict__ x, double* __restrict__ xo, const double* __restrict__ b,
                                        const float* __restrict__ z32, float* __restrict__ r32, int sx, int sy, int sz, double qx,
                                        double qy, double qz, double inv_sz, double s, int zchunk, double* __restrict__ partial) {
    constexpr int NR = TR + 2;
    const Geo<XSplit, double> g(sx, sy);
    const Geo<XSplit, float> g32(sx, sy);
    const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int cx = (sx + 1) / 2;
    const int ic = blockIdx.x * 63 + lane;
    const int icc = min(ic, cx - 1);  // lanes past the row keep in step (shuffles) on the last column and store nothing
    const int y0 = 1 + (blockIdx.y * TYW + wave) * TR;
    const int z0 = 1 + blockIdx.z * zchunk, z1 = min(z0 + zchunk, sz - 1);
    const bool own = ic <= cx - 1 && (lane > 0 || ic == 0);
    const bool xinA = ic >= 1 && ic <= cx - 2;  // x = 2i is interior
    const bool hasB = ic <= cx - 2;             // x = 2i + 1 exists and is interior
    const bool wA = own && lane > 0 && xinA, wB = own && hasB;
    const int jB = g.H + (hasB ? icc : 0), jB32 = g32.H + (hasB ? icc : 0);
    double acc = 0.0;
    if (y0 <= sy - 2) {
        size_t roff[NR], roff32[NR];
        bool yin[NR];
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int y = y0 - 1 + r;
            roff[r] = (size_t)min(y, sy - 1) * g.P;
            roff32[r] = (size_t)min(y, sy - 1) * g32.P;
            yin[r] = y >= 1 && y <= sy - 2;
        }
        // x of plane gz (the corrected x with CORR) for the NR rows
        auto load = [&](int gz, double (&A)[NR], double (&B)[NR]) {
            const size_t pb = (size_t)gz * g.PL, pb32 = (size_t)gz * g32.PL;
            const bool zin = gz >= 1 && gz <= sz - 2;
#pragma unroll
            for (int r = 0; r < NR; r++) {
                A[r] = x[pb + roff[r] + icc];
                B[r] = x[pb + roff[r] + jB];
            }
            if (CORR && zin) {
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    if (yin[r] && xinA) A[r] = A[r] + (double)z32[pb32 + roff32[r] + icc] * inv_sz;
                    if (yin[r] && hasB) B[r] = B[r] + (double)z32[pb32 + roff32[r] + jB32] * inv_sz;
                }
            }
        };
        auto store = [&](int gz, const double (&A)[NR], const double (&B)[NR]) {
            const size_t pb = (size_t)gz * g.PL;
#pragma unroll
            for (int r = 1; r < NR - 1; r++)
                if (yin[r]) {
                    if (wA) xo[pb + roff[r] + icc] = A[r];
                    if (wB) xo[pb + roff[r] + jB] = B[r];
                }
        };
        double AP[NR], BP[NR], AC[NR], BC[NR], AN[NR], BN[NR];
        load(z0 - 1, AP, BP);
        load(z0, AC, BC);
        if (CORR) store(z0, AC, BC);
        for (int gz = z0; gz < z1; gz++) {
            load(gz + 1, AN, BN);
            if (CORR && gz + 1 < z1) store(gz + 1, AN, BN);
            const size_t pb = (size_t)gz * g.PL, pb32 = (size_t)gz * g32.PL;
#pragma unroll
            for (int r = 1; r < NR - 1; r++) {
                const double fA = b[pb + roff[r] + icc], fB = b[pb + roff[r] + jB];
                const double Bl = __shfl_up(BC[r], 1, 64);  // x = 2i - 1: the odd entry of lane i - 1
                double Ar = __shfl_down(AC[r], 1, 64);      // x = 2i + 2: the even entry of lane i + 1
                if (lane == 63 && hasB) {                   // wave edge: load (and correct) it
                    Ar = x[pb + roff[r] + icc + 1];
                    if (CORR && yin[r] && ic + 1 <= cx - 2) Ar = Ar + (double)z32[pb32 + roff32[r] + icc + 1] * inv_sz;
                }
                const double ra = residual3d_point<double, MODE>(Bl, BC[r], AC[r - 1], AC[r + 1], AP[r], AN[r], AC[r], fA, qx, qy, qz);
                const double rb = residual3d_point<double, MODE>(AC[r], Ar, BC[r - 1], BC[r + 1], BP[r], BN[r], BC[r], fB, qx, qy, qz);
                if (yin[r]) {
                    if (wA) {
                        r32[pb32 + roff32[r] + icc] = (float)(ra * s);
                        acc += ra * ra;
                    }
                    if (wB) {
                        r32[pb32 + roff32[r] + jB32] = (float)(rb * s);
                        acc += rb * rb;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < NR; r++) {
                AP[r] = AC[r]; BP[r] = BC[r];
                AC[r] = AN[r]; BC[r] = BN[r];
            }
        }
    }
    __shared__ double part[TYW];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (lane == 0 && wave == 0) {
        double t = part[0];
        for (int w = 1; w < TYW; w++) t += part[w];
        partial[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = t;
    }
}

// ------------------------------------------------------------------ host side
size_t krylov_work_elems(const int n[3]) {
    if (rows_check(n, "krylov_work_elems")) return 0;
    const dim3 g = krylov_grid(n);
    return 2 * (size_t)g.x * g.y;
}

int krylov_final(mgx_ctx* ctx, const double* work, size_t count, int nsums, double* dev_sum) {  // (declared in mgx_host3d.hpp)
    MGX_LAUNCH(cg_final_kernel, dim3(nsums), dim3(1024), 0, ctx->compute, work, count, dev_sum);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

template <class real>
int cg_update3d(mgx_ctx* ctx, real* x, const real* p, real* r, const real* q, const int n[3], const double* dev_alpha, double* dev_work,
                double* dev_sum, bool finalize) {  // (declared in mgx_host3d.hpp, as are the two below)
    MGX_REQUIRE(ctx && r && q && (!x || p) && dev_alpha && dev_work && dev_sum, MGX_ERR_INVALID, "cg_update: NULL argument");
    MGX_USE(ctx);
    MGX_TRY_RET(rows_check(n, "cg_update"));
    const dim3 g = krylov_grid(n);
    if (x) MGX_LAUNCH((cg_update3d_xs_kernel<real, true>), g, krylov_block(), 0, ctx->compute, x, p, r, q, n[0], n[1], dev_alpha, dev_work);
    else MGX_LAUNCH((cg_update3d_xs_kernel<real, false>), g, krylov_block(), 0, ctx->compute, x, p, r, q, n[0], n[1], dev_alpha, dev_work);
    MGX_LAUNCH_CHECK();
    return finalize ? krylov_final(ctx, dev_work, (size_t)g.x * g.y, 1, dev_sum) : MGX_OK;
}

template <class real>
int dot2_3d(mgx_ctx* ctx, const real* a, const real* b, const real* c, const int n[3], double* dev_work, double* dev_sum, bool finalize) {
    MGX_REQUIRE(ctx && a && b && dev_work && dev_sum, MGX_ERR_INVALID, "dot2: NULL argument");
    MGX_USE(ctx);
    MGX_TRY_RET(rows_check(n, "dot2"));
    const dim3 g = krylov_grid(n);
    if (c) MGX_LAUNCH((dot2_3d_xs_kernel<real, true>), g, krylov_block(), 0, ctx->compute, a, b, c, n[0], n[1], dev_work);
    else MGX_LAUNCH((dot2_3d_xs_kernel<real, false>), g, krylov_block(), 0, ctx->compute, a, b, c, n[0], n[1], dev_work);
    MGX_LAUNCH_CHECK();
    return finalize ? krylov_final(ctx, dev_work, (size_t)g.x * g.y, c ? 2 : 1, dev_sum) : MGX_OK;
}

template <class real>
int cg_direction3d(mgx_ctx* ctx, real* x, real* p, const real* z, const int n[3], const double* dev_alpha, const double* dev_beta) {
    MGX_REQUIRE(ctx && p && (!x || dev_alpha), MGX_ERR_INVALID, "cg_direction: NULL argument");
    MGX_REQUIRE(x || z, MGX_ERR_INVALID, "cg_direction: nothing to do (x and z are NULL)");
    MGX_USE(ctx);
    MGX_TRY_RET(rows_check(n, "cg_direction"));
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

// (mgx_rim3d.hip calls the three: the interior launches of its entries for all unknowns)
#define MGX_INSTANTIATE_KRYLOV(real)                                                                                                      \
    template int cg_update3d<real>(mgx_ctx*, real*, const real*, real*, const real*, const int[3], const double*, double*, double*, bool); \
    template int dot2_3d<real>(mgx_ctx*, const real*, const real*, const real*, const int[3], double*, double*, bool);                     \
    template int cg_direction3d<real>(mgx_ctx*, real*, real*, const real*, const int[3], const double*, const double*);
MGX_INSTANTIATE_KRYLOV(float)
MGX_INSTANTIATE_KRYLOV(double)
#undef MGX_INSTANTIATE_KRYLOV

// ---- mixed precision
// the z-marching pass: TR rows per wave (mixed3d.rows), four waves per block, runs of zchunk planes (mixed3d.zchunk; 0 =
// 16, halved while the launch has fewer than four workgroups per CU)
struct CrdPlan {
    int TR, zchunk;
    dim3 grid, block;
    int mode;      // MODE of the residual: 1 dividing, 3 exact reciprocals
    int launches;  // 2: the streaming correction first, then the pass without it; 1: the pass alone (correcting, if asked to)
    double qx, qy, qz;
};
constexpr int CRD_TYW = 4;
static CrdPlan crd_plan(const mgx_ctx* ctx, const int n[3], const double h[3], bool with_correction) {
    CrdPlan p;
    const ResidualScale<double> sc = residual_scale<double>(ctx, h, MGX_RESIDUAL_CORRECT);  // as mgx3dxs_residual forms them
    p.mode = sc.mode;
    p.qx = sc.qx, p.qy = sc.qy, p.qz = sc.qz;
    p.launches = with_correction && !ctx->mixed_fused ? 2 : 1;
    p.TR = ctx->mixed_rows;
    const unsigned gx = (unsigned)ceil_div(std::max((n[0] + 1) / 2 - 1, 1), 63), gy = (unsigned)ceil_div(n[1] - 2, p.TR * CRD_TYW);
    p.zchunk = ctx->mixed_zchunk;
    if (p.zchunk <= 0) {
        p.zchunk = 16;
        while (p.zchunk > 2 && (long long)gx * gy * ceil_div(n[2] - 2, p.zchunk) < 4 * 256) p.zchunk /= 2;
    }
    p.grid = dim3(gx, gy, (unsigned)ceil_div(n[2] - 2, p.zchunk));
    p.block = dim3(64, CRD_TYW, 1);
    return p;
}

// partials any mixed kernel writes: the Krylov kernels' count or the z-marching pass's at its smallest tiles (2 rows per wave,
// one plane per run), whichever is larger
size_t mixed_work_elems(const int n[3]) {
    if (rows_check(n, "mixed_work_elems")) return 0;
    const size_t crd = (size_t)ceil_div(std::max((n[0] + 1) / 2 - 1, 1), 63) * ceil_div(n[1] - 2, 2 * CRD_TYW) * (size_t)(n[2] - 2);
    return std::max(krylov_work_elems(n), crd);
}

int demote3d(mgx_ctx* ctx, const double* r, float* r32, double s, const int n[3]) {
    MGX_REQUIRE(ctx && r && r32, MGX_ERR_INVALID, "demote: NULL argument");
    MGX_USE(ctx);
    MGX_TRY_RET(rows_check(n, "demote"));
    MGX_LAUNCH(demote3d_xs_kernel, krylov_grid(n), krylov_block(), 0, ctx->compute, r, r32, n[0], n[1], s);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

int cg_update_demote3d(mgx_ctx* ctx, double* x, const double* p, double* r, const double* q, float* r32, double s, const int n[3],
                       const double* dev_alpha, double* dev_work, double* dev_sum) {
    MGX_REQUIRE(ctx && r && q && r32 && (!x || p) && dev_alpha && dev_work && dev_sum, MGX_ERR_INVALID, "cg_update_demote: NULL argument");
    MGX_USE(ctx);
    MGX_TRY_RET(rows_check(n, "cg_update_demote"));
    const dim3 g = krylov_grid(n);
    if (x) MGX_LAUNCH(cg_update_demote3d_xs_kernel<true>, g, krylov_block(), 0, ctx->compute, x, p, r, q, r32, n[0], n[1], s, dev_alpha, dev_work);
    else MGX_LAUNCH(cg_update_demote3d_xs_kernel<false>, g, krylov_block(), 0, ctx->compute, x, p, r, q, r32, n[0], n[1], s, dev_alpha, dev_work);
    MGX_LAUNCH_CHECK();
    return krylov_final(ctx, dev_work, (size_t)g.x * g.y, 1, dev_sum);
}

int dot2_mixed3d(mgx_ctx* ctx, const float* z32, double inv_s, const double* b, const double* c, const int n[3], double* dev_work,
                 double* dev_sum) {
    MGX_REQUIRE(ctx && z32 && b && dev_work && dev_sum, MGX_ERR_INVALID, "dot2_mixed: NULL argument");
    MGX_USE(ctx);
    MGX_TRY_RET(rows_check(n, "dot2_mixed"));
    const dim3 g = krylov_grid(n);
    if (c) MGX_LAUNCH(dot2_mixed3d_xs_kernel<true>, g, krylov_block(), 0, ctx->compute, z32, inv_s, b, c, n[0], n[1], dev_work);
    else MGX_LAUNCH(dot2_mixed3d_xs_kernel<false>, g, krylov_block(), 0, ctx->compute, z32, inv_s, b, c, n[0], n[1], dev_work);
    MGX_LAUNCH_CHECK();
    return krylov_final(ctx, dev_work, (size_t)g.x * g.y, c ? 2 : 1, dev_sum);
}

int cg_direction_mixed3d(mgx_ctx* ctx, double* x, double* p, const float* z32, double inv_s, const int n[3], const double* dev_alpha,
                         const double* dev_beta) {
    MGX_REQUIRE(ctx && p && z32 && (!x || dev_alpha), MGX_ERR_INVALID, "cg_direction_mixed: NULL argument");
    MGX_USE(ctx);
    MGX_TRY_RET(rows_check(n, "cg_direction_mixed"));
    const dim3 g = krylov_grid(n);
#define MGX_DIR(X, B) \
    MGX_LAUNCH((cg_direction_mixed3d_xs_kernel<X, B>), g, krylov_block(), 0, ctx->compute, x, p, z32, inv_s, n[0], n[1], dev_alpha, dev_beta)
    if (x && dev_beta) MGX_DIR(true, true);
    else if (x) MGX_DIR(true, false);
    else if (dev_beta) MGX_DIR(false, true);
    else MGX_DIR(false, false);
#undef MGX_DIR
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

int correct_residual_demote3d(mgx_ctx* ctx, const double* x, double* xo, const double* b, const float* z32, double inv_sz, float* r32,
                              double s, const int n[3], const double h[3], double* dev_work, double* dev_sum) {
    MGX_REQUIRE(ctx && x && b && r32 && h && dev_work && dev_sum, MGX_ERR_INVALID, "correct_residual_demote: NULL argument");
    MGX_REQUIRE(!z32 || (xo && xo != x), MGX_ERR_INVALID, "correct_residual_demote: the correction needs an output array xo != x");
    MGX_USE(ctx);
    MGX_TRY_RET(rows_check(n, "correct_residual_demote"));
    const CrdPlan p = crd_plan(ctx, n, h, z32 != nullptr);
    bool corr = z32 != nullptr;
    if (p.launches == 2) {  // the two-launch form: a streaming correction, then the pass without it
        MGX_LAUNCH(correct_mixed3d_xs_kernel, krylov_grid(n), krylov_block(), 0, ctx->compute, x, xo, z32, inv_sz, n[0], n[1]);
        MGX_LAUNCH_CHECK();
        x = xo;
        corr = false;
    }
    with_value<1, 3>(p.mode, [&](auto m) __attribute__((always_inline)) {
        with_value<2, 4, 8>(p.TR, [&](auto tr) __attribute__((always_inline)) {
            constexpr int M = decltype(m)::value, TR = decltype(tr)::value;
            if (corr)
                MGX_LAUNCH((correct_residual_demote3d_xs_kernel<M, true, TR, CRD_TYW>), p.grid, p.block, 0, ctx->compute, x, xo, b, z32, r32,
                           n[0], n[1], n[2], p.qx, p.qy, p.qz, inv_sz, s, p.zchunk, dev_work);
            else
                MGX_LAUNCH((correct_residual_demote3d_xs_kernel<M, false, TR, CRD_TYW>), p.grid, p.block, 0, ctx->compute, x, xo, b, z32,
                           r32, n[0], n[1], n[2], p.qx, p.qy, p.qz, inv_sz, s, p.zchunk, dev_work);
        });
    });
    MGX_LAUNCH_CHECK();
    return krylov_final(ctx, dev_work, (size_t)p.grid.x * p.grid.y * p.grid.z, 1, dev_sum);
}

// what correct_residual_demote3d launches: the plan it launches from
int correct_residual_demote_plan3d(const mgx_ctx* ctx, const int n[3], const double h[3], int with_correction, int* out) {
    MGX_REQUIRE(ctx && h && out, MGX_ERR_INVALID, "correct_residual_demote_plan: NULL argument");
    MGX_TRY_RET(rows_check(n, "correct_residual_demote_plan"));
    const CrdPlan p = crd_plan(ctx, n, h, with_correction != 0);
    out[MGX_CRD_ROWS] = p.TR;
    out[MGX_CRD_ZCHUNK] = p.zchunk;
    out[MGX_CRD_GX] = (int)p.grid.x;
    out[MGX_CRD_GY] = (int)p.grid.y;
    out[MGX_CRD_GZ] = (int)p.grid.z;
    out[MGX_CRD_MODE] = p.mode;
    out[MGX_CRD_LAUNCHES] = p.launches;
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
        return mgx::apply_op_dot3d<mgx::PlainOp<real>, real>(ctx, p, nullptr, q, n, h, (real)0, dev_work, dev_sum, "laplace_dot");\
    }                                                                                                                         \
    int mgx3dxs_cg_update_##SFX(mgx_ctx* ctx, real* x, const real* p, real* r, const real* q, const int n[3],                  \
                                const double* dev_alpha, double* dev_work, double* dev_sum) {                                 \
        return mgx::cg_update3d<real>(ctx, x, p, r, q, n, dev_alpha, dev_work, dev_sum, true);                                     \
    }                                                                                                                         \
    int mgx3dxs_dot2_##SFX(mgx_ctx* ctx, const real* a, const real* b, const real* c, const int n[3], double* dev_work,         \
                           double* dev_sum) {                                                                                 \
        return mgx::dot2_3d<real>(ctx, a, b, c, n, dev_work, dev_sum, true);                                                     \
    }                                                                                                                         \
    int mgx3dxs_cg_direction_##SFX(mgx_ctx* ctx, real* x, real* p, const real* z, const int n[3], const double* dev_alpha,      \
                                   const double* dev_beta) {                                                                  \
        return mgx::cg_direction3d<real>(ctx, x, p, z, n, dev_alpha, dev_beta);                                               \
    }
MGX_STAMP_KRYLOV(f32, float)
MGX_STAMP_KRYLOV(f64, double)
#undef MGX_STAMP_KRYLOV

size_t mgx3dxs_mixed_work_elems_f64(const int n[3]) { return mgx::mixed_work_elems(n); }
int mgx3dxs_demote_f64(mgx_ctx* ctx, const double* r, float* r32, double s, const int n[3]) { return mgx::demote3d(ctx, r, r32, s, n); }
int mgx3dxs_cg_update_demote_f64(mgx_ctx* ctx, double* x, const double* p, double* r, const double* q, float* r32, double s, const int n[3],
                                 const double* dev_alpha, double* dev_work, double* dev_sum) {
    return mgx::cg_update_demote3d(ctx, x, p, r, q, r32, s, n, dev_alpha, dev_work, dev_sum);
}
int mgx3dxs_dot2_mixed_f64(mgx_ctx* ctx, const float* z32, double inv_s, const double* b, const double* c, const int n[3], double* dev_work,
                           double* dev_sum) {
    return mgx::dot2_mixed3d(ctx, z32, inv_s, b, c, n, dev_work, dev_sum);
}
int mgx3dxs_cg_direction_mixed_f64(mgx_ctx* ctx, double* x, double* p, const float* z32, double inv_s, const int n[3],
                                   const double* dev_alpha, const double* dev_beta) {
    return mgx::cg_direction_mixed3d(ctx, x, p, z32, inv_s, n, dev_alpha, dev_beta);
}
int mgx3dxs_correct_residual_demote_f64(mgx_ctx* ctx, const double* x, double* xo, const double* b, const float* z32, double inv_sz,
                                        float* r32, double s, const int n[3], const double h[3], double* dev_work, double* dev_sum) {
    return mgx::correct_residual_demote3d(ctx, x, xo, b, z32, inv_sz, r32, s, n, h, dev_work, dev_sum);
}
int mgx3dxs_correct_residual_demote_plan_f64(const mgx_ctx* ctx, const int n[3], const double h[3], int with_correction,
                                             int out[MGX_CRD_PLAN]) {
    return mgx::correct_residual_demote_plan3d(ctx, n, h, with_correction, out);
}

}  // extern "C"
