// mgx_eigen3d.hip -- the block vector kernels of the eigensolver (mgMultiGrid3D_f64_Eigen, host/mg_eigen3d.inc; DESIGN.md
// section 21), x-split layout, fp64.  An addition: the reference has no eigensolver.
//
// LOBPCG with block size k works on a basis of up to 3k level-0 vectors and their images under the operator.  Formed pair
// by pair, its Gram matrices would read every vector some 6k times per iteration; these kernels take the vectors in groups
// of four, so that a launch reading eight vectors yields sixteen (or thirty-two) inner products.
//
//   block_gram3d_xs_kernel      partials of <U_i, V_j>_W and, with c, of <U_i, c V_j>_W for up to 4 x 4 pairs
//   block_combine3d_xs_kernel   out_i = sum_j Y[j][i] S_j for up to 12 inputs and 4 outputs
//   block_residual3d_xs_kernel  r_i = AX_i + mu_i (c X_i), partials of <r_i, r_i>_W and <X_i, X_i>_W, up to 4 vectors
//   eigen_start3d_xs_kernel     the hashed start vector
//
// Every kernel walks ALL grid points by storage position, one wavefront per x-row, and skips the pads.  The weight of a point
// is formed from its position and the mask bc: 0 at a Dirichlet point (a point on a face whose bit is clear), otherwise 1/2
// per face it lies on -- the trapezoid weights W of DESIGN.md 16.  One launch therefore serves every mask and there is no
// companion launch for the face unknowns.  Entries of Dirichlet points and pads are never read as data.
//
// Sums: per lane in loop order, wavefront-wide shuffles, the block's four waves in a fixed order into one partial per block
// and sum, cg_final_kernel (mgx_krylov3d.hip) over the partials -- the same bits on every run.  LDS holds the block's wave
// sums only, each written before it is read.  No kernel waits for another workgroup.
#include "mgx_internal.hpp"
#include "mgx_host3d.hpp"
#include "mgx_stencil3d.hpp"

namespace mgx {

constexpr int EG = 4;        // vectors per group
constexpr int EIN = 12;      // inputs of a combination
constexpr int EKJ = 2;       // positions per lane and step
constexpr int ERY = 4;       // rows per wave of the summing kernels: one wave sum per ERY rows
constexpr int ESTEP = 64 * EKJ;
static_assert(KROWS == 4, "the block partials below add the sums of exactly four waves");

// bits of the faces the row (y, z) lies on, and of the faces column x adds
__device__ __forceinline__ int eig_on_yz(int y, int z, int sy, int sz) {
    return (y == 0) << 2 | (y == sy - 1) << 3 | (z == 0) << 4 | (z == sz - 1) << 5;
}
__device__ __forceinline__ int eig_on_x(int x, int sx) { return (x == 0) | (x == sx - 1) << 1; }
// 1/2 per set bit (an axis has at most one: sizes are >= 3)
__device__ __forceinline__ double eig_half_pow(int on) {
    const int f = __builtin_popcount(on);
    return f == 0 ? 1.0 : f == 1 ? 0.5 : f == 2 ? 0.25 : 0.125;
}

struct GramArgs {
    const double* u[EG];
    const double* v[EG];
};

// sum s = i * NV + j: <U_i, V_j>_W; with C the sums NU * NV + i * NV + j: <U_i, c V_j>_W.  partial[s * blocks + block].
template <int NU, int NV, bool C>
__global__ void __launch_bounds__(256) block_gram3d_xs_kernel(GramArgs a, const double* __restrict__ c, int sx, int sy, int sz, int bc,
                                                              double* __restrict__ partial) {
    constexpr int NS = NU * NV * (C ? 2 : 1);
    const Geo<XSplit, double> g(sx, sy);
    const int z = blockIdx.y, H = g.H, P = g.P;
    double acc[NU][NV], acc_c[NU][NV];
#pragma unroll
    for (int i = 0; i < NU; i++)
#pragma unroll
        for (int j = 0; j < NV; j++) acc[i][j] = 0.0, acc_c[i][j] = 0.0;
    for (int ry = 0; ry < ERY; ry++) {
        const int y = (blockIdx.x * KROWS + threadIdx.y) * ERY + ry;
        if (y >= sy) break;
        const int on_yz = eig_on_yz(y, z, sy, sz);
        if (on_yz & ~bc) continue;  // a row of Dirichlet points
        const double w_yz = eig_half_pow(on_yz);
        const size_t row = g.row(y, z);
        for (int j0 = 0; j0 < P; j0 += ESTEP) {
            double uv[NU][EKJ], vv[NV][EKJ], cv[EKJ], w[EKJ];
            bool in[EKJ];
#pragma unroll
            for (int k = 0; k < EKJ; k++) {
                const int j = j0 + k * 64 + threadIdx.x, x = xs_x(j, H);
                const int on_x = eig_on_x(x, sx);
                in[k] = j < P && x < sx && !(on_x & ~bc);
                w[k] = on_x ? w_yz * 0.5 : w_yz;
                if (in[k]) {
                    const size_t p = row + j;
#pragma unroll
                    for (int i = 0; i < NU; i++) uv[i][k] = a.u[i][p];
#pragma unroll
                    for (int i = 0; i < NV; i++) vv[i][k] = a.v[i][p];
                    if (C) cv[k] = c[p];
                }
            }
#pragma unroll
            for (int k = 0; k < EKJ; k++)
                if (in[k]) {
#pragma unroll
                    for (int i = 0; i < NU; i++) {
                        const double wu = w[k] * uv[i][k];
#pragma unroll
                        for (int j = 0; j < NV; j++) {
                            acc[i][j] += wu * vv[j][k];
                            if (C) acc_c[i][j] += wu * (cv[k] * vv[j][k]);
                        }
                    }
                }
        }
    }
    __shared__ double part[2 * EG * EG][KROWS];
#pragma unroll
    for (int i = 0; i < NU; i++)
#pragma unroll
        for (int j = 0; j < NV; j++) {
            wave_sum(acc[i][j], part[i * NV + j]);
            if (C) wave_sum(acc_c[i][j], part[NU * NV + i * NV + j]);
        }
    __syncthreads();
    const int t = threadIdx.y * 64 + threadIdx.x;
    if (t < NS) {
        const size_t nb = (size_t)gridDim.x * gridDim.y, blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        partial[(size_t)t * nb + blk] = (part[t][0] + part[t][1]) + (part[t][2] + part[t][3]);
    }
}

struct CombineArgs {
    const double* in[EIN];
    double* out[EG];
    double y[EIN][EG];
};

// out_i = ((Y[0][i] S_0 + Y[1][i] S_1) + Y[2][i] S_2) + ... : products and sums in this order, none contracted.  A thread reads
// all its inputs at a point before it writes, so an output may be one of the inputs.  Unknowns only.
template <int NIN, int NOUT>
__global__ void __launch_bounds__(256) block_combine3d_xs_kernel(CombineArgs a, int sx, int sy, int sz, int bc) {
    const Geo<XSplit, double> g(sx, sy);
    const int y = blockIdx.x * KROWS + threadIdx.y, z = blockIdx.y, H = g.H, P = g.P;
    if (y >= sy) return;
    const int on_yz = eig_on_yz(y, z, sy, sz);
    if (on_yz & ~bc) return;
    const size_t row = g.row(y, z);
    for (int j0 = 0; j0 < P; j0 += ESTEP) {
        double s[NIN][EKJ];
        bool in[EKJ];
#pragma unroll
        for (int k = 0; k < EKJ; k++) {
            const int j = j0 + k * 64 + threadIdx.x, x = xs_x(j, H);
            in[k] = j < P && x < sx && !(eig_on_x(x, sx) & ~bc);
            if (in[k]) {
#pragma unroll
                for (int i = 0; i < NIN; i++) s[i][k] = a.in[i][row + j];
            }
        }
#pragma unroll
        for (int k = 0; k < EKJ; k++)
            if (in[k]) {
#pragma unroll
                for (int o = 0; o < NOUT; o++) {
                    double t = a.y[0][o] * s[0][k];
#pragma unroll
                    for (int i = 1; i < NIN; i++) t = t + a.y[i][o] * s[i][k];
                    a.out[o][row + j0 + k * 64 + threadIdx.x] = t;
                }
            }
    }
}

struct ResidualArgs {
    const double* ax[EG];
    const double* x[EG];
    double* r[EG];
    double mu[EG];
};

// r_i = AX_i + mu_i (c X_i) (without c: mu_i X_i) at the unknowns, 0 at the Dirichlet points; sums i: <r_i, r_i>_W, N + i: <X_i, X_i>_W
template <int N, bool C>
__global__ void __launch_bounds__(256) block_residual3d_xs_kernel(ResidualArgs a, const double* __restrict__ c, int sx, int sy, int sz, int bc,
                                                                  double* __restrict__ partial) {
    const Geo<XSplit, double> g(sx, sy);
    const int z = blockIdx.y, H = g.H, P = g.P;
    double rr[N], xx[N];
#pragma unroll
    for (int i = 0; i < N; i++) rr[i] = 0.0, xx[i] = 0.0;
    for (int ry = 0; ry < ERY; ry++) {
        const int y = (blockIdx.x * KROWS + threadIdx.y) * ERY + ry;
        if (y >= sy) break;
        const int on_yz = eig_on_yz(y, z, sy, sz);
        const bool row_in = !(on_yz & ~bc);
        const double w_yz = eig_half_pow(on_yz);
        const size_t row = g.row(y, z);
        for (int j0 = 0; j0 < P; j0 += ESTEP) {
            double av[N][EKJ], xv[N][EKJ], cv[EKJ], w[EKJ];
            bool in[EKJ], pt[EKJ];
#pragma unroll
            for (int k = 0; k < EKJ; k++) {
                const int j = j0 + k * 64 + threadIdx.x, x = xs_x(j, H);
                const int on_x = eig_on_x(x, sx);
                pt[k] = j < P && x < sx;
                in[k] = pt[k] && row_in && !(on_x & ~bc);
                w[k] = on_x ? w_yz * 0.5 : w_yz;
                if (in[k]) {
                    const size_t p = row + j;
#pragma unroll
                    for (int i = 0; i < N; i++) av[i][k] = a.ax[i][p], xv[i][k] = a.x[i][p];
                    if (C) cv[k] = c[p];
                }
            }
#pragma unroll
            for (int k = 0; k < EKJ; k++) {
                const size_t p = row + j0 + k * 64 + threadIdx.x;
                if (in[k]) {
#pragma unroll
                    for (int i = 0; i < N; i++) {
                        const double cx = C ? cv[k] * xv[i][k] : xv[i][k];
                        const double r = av[i][k] + a.mu[i] * cx;
                        a.r[i][p] = r;
                        rr[i] += (w[k] * r) * r;
                        xx[i] += (w[k] * xv[i][k]) * xv[i][k];
                    }
                } else if (pt[k]) {
#pragma unroll
                    for (int i = 0; i < N; i++) a.r[i][p] = 0.0;
                }
            }
        }
    }
    __shared__ double part[2 * EG][KROWS];
#pragma unroll
    for (int i = 0; i < N; i++) {
        wave_sum(rr[i], part[i]);
        wave_sum(xx[i], part[N + i]);
    }
    __syncthreads();
    const int t = threadIdx.y * 64 + threadIdx.x;
    if (t < 2 * N) {
        const size_t nb = (size_t)gridDim.x * gridDim.y, blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        partial[(size_t)t * nb + blk] = (part[t][0] + part[t][1]) + (part[t][2] + part[t][3]);
    }
}

// the start vectors: a fixed integer hash of (index, x, y, z) mapped into (-1, 1)
__host__ __device__ __forceinline__ double eigen_start_value(unsigned index, unsigned x, unsigned y, unsigned z) {
    unsigned h = (index + 1u) * 0x9E3779B1u ^ x * 0x85EBCA77u ^ y * 0xC2B2AE3Du ^ z * 0x27D4EB2Fu;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return ((double)h + 0.5) * (1.0 / 2147483648.0) - 1.0;  // exact in double: |value| <= 1 - 2^-32
}

__global__ void __launch_bounds__(256) eigen_start3d_xs_kernel(double* __restrict__ v, int index, int sx, int sy, int sz, int bc) {
    const Geo<XSplit, double> g(sx, sy);
    const int y = blockIdx.x * KROWS + threadIdx.y, z = blockIdx.y, H = g.H, P = g.P;
    if (y >= sy) return;
    const bool row_in = !(eig_on_yz(y, z, sy, sz) & ~bc);
    const size_t row = g.row(y, z);
    for (int j = threadIdx.x; j < P; j += 64) {
        const int x = xs_x(j, H);
        if (x >= sx) continue;
        const bool in = row_in && !(eig_on_x(x, sx) & ~bc);
        v[row + j] = in ? eigen_start_value((unsigned)index, (unsigned)x, (unsigned)y, (unsigned)z) : 0.0;
    }
}

// ------------------------------------------------------------------ host side
static dim3 eig_grid_rows(const int n[3]) { return dim3((unsigned)ceil_div(n[1], KROWS), (unsigned)n[2]); }
static dim3 eig_grid_sums(const int n[3]) { return dim3((unsigned)ceil_div(n[1], KROWS * ERY), (unsigned)n[2]); }

static int eig_check(const int n[3], int bc, const char* what) {
    MGX_TRY_RET(rows_check(n, what));
    MGX_REQUIRE(n[2] <= 65535, MGX_ERR_SIZE, "%s: %d planes are too many", what, n[2]);
    MGX_REQUIRE(bc >= 0 && bc <= 63, MGX_ERR_INVALID, "%s: bc = %d is outside 0 .. 63", what, bc);
    return MGX_OK;
}

static size_t block_work_elems(const int n[3]) {
    if (rows_check(n, "block_work_elems") || n[2] > 65535) return 0;
    const dim3 g = eig_grid_sums(n);
    return (size_t)2 * EG * EG * g.x * g.y;
}

static int block_gram3d(mgx_ctx* ctx, int nu, const double* const* U, int nv, const double* const* V, const double* c, const int n[3], int bc,
                        double* dev_work, double* dev_out) {
    MGX_REQUIRE(ctx && U && V && n && dev_work && dev_out, MGX_ERR_INVALID, "block_gram: NULL argument");
    MGX_REQUIRE(nu >= 1 && nu <= EG && nv >= 1 && nv <= EG, MGX_ERR_INVALID, "block_gram: group sizes %d, %d outside 1 .. %d", nu, nv, EG);
    GramArgs a = {};
    for (int i = 0; i < nu; i++) MGX_REQUIRE((a.u[i] = U[i]) != nullptr, MGX_ERR_INVALID, "block_gram: U[%d] is NULL", i);
    for (int i = 0; i < nv; i++) MGX_REQUIRE((a.v[i] = V[i]) != nullptr, MGX_ERR_INVALID, "block_gram: V[%d] is NULL", i);
    MGX_TRY_RET(eig_check(n, bc, "block_gram"));
    MGX_USE(ctx);
    const dim3 g = eig_grid_sums(n);
    with_value<1, 2, 3, 4>(nu, [&](auto cu) __attribute__((always_inline)) {
        with_value<1, 2, 3, 4>(nv, [&](auto cv) __attribute__((always_inline)) {
            constexpr int NU = decltype(cu)::value, NV = decltype(cv)::value;
            if (c) MGX_LAUNCH((block_gram3d_xs_kernel<NU, NV, true>), g, krylov_block(), 0, ctx->compute, a, c, n[0], n[1], n[2], bc, dev_work);
            else MGX_LAUNCH((block_gram3d_xs_kernel<NU, NV, false>), g, krylov_block(), 0, ctx->compute, a, c, n[0], n[1], n[2], bc, dev_work);
        });
    });
    MGX_LAUNCH_CHECK();
    return krylov_final(ctx, dev_work, (size_t)g.x * g.y, nu * nv * (c ? 2 : 1), dev_out);
}

static int block_combine3d(mgx_ctx* ctx, int nin, const double* const* S, int nout, double* const* out, const double* Y, const int n[3],
                           int bc) {
    MGX_REQUIRE(ctx && S && out && Y && n, MGX_ERR_INVALID, "block_combine: NULL argument");
    MGX_REQUIRE(nin >= 1 && nin <= EIN && nout >= 1 && nout <= EG, MGX_ERR_INVALID, "block_combine: %d inputs, %d outputs outside 1 .. %d, 1 .. %d",
                nin, nout, EIN, EG);
    CombineArgs a = {};
    for (int i = 0; i < nin; i++) MGX_REQUIRE((a.in[i] = S[i]) != nullptr, MGX_ERR_INVALID, "block_combine: S[%d] is NULL", i);
    for (int i = 0; i < nout; i++) MGX_REQUIRE((a.out[i] = out[i]) != nullptr, MGX_ERR_INVALID, "block_combine: out[%d] is NULL", i);
    for (int i = 0; i < nin; i++)
        for (int o = 0; o < nout; o++) a.y[i][o] = Y[i * nout + o];
    MGX_TRY_RET(eig_check(n, bc, "block_combine"));
    MGX_USE(ctx);
    const dim3 g = eig_grid_rows(n);
    with_value<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12>(nin, [&](auto ci) __attribute__((always_inline)) {
        with_value<1, 2, 3, 4>(nout, [&](auto co) __attribute__((always_inline)) {
            MGX_LAUNCH((block_combine3d_xs_kernel<decltype(ci)::value, decltype(co)::value>), g, krylov_block(), 0, ctx->compute, a, n[0], n[1],
                       n[2], bc);
        });
    });
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

static int block_residual3d(mgx_ctx* ctx, int nvec, const double* const* AX, const double* const* X, const double* c, const double* mu,
                            double* const* Rv, const int n[3], int bc, double* dev_work, double* dev_out) {
    MGX_REQUIRE(ctx && AX && X && mu && Rv && n && dev_work && dev_out, MGX_ERR_INVALID, "block_residual: NULL argument");
    MGX_REQUIRE(nvec >= 1 && nvec <= EG, MGX_ERR_INVALID, "block_residual: %d vectors outside 1 .. %d", nvec, EG);
    ResidualArgs a = {};
    for (int i = 0; i < nvec; i++) {
        MGX_REQUIRE(AX[i] && X[i] && Rv[i], MGX_ERR_INVALID, "block_residual: vector %d is NULL", i);
        a.ax[i] = AX[i], a.x[i] = X[i], a.r[i] = Rv[i], a.mu[i] = mu[i];
    }
    MGX_TRY_RET(eig_check(n, bc, "block_residual"));
    MGX_USE(ctx);
    const dim3 g = eig_grid_sums(n);
    with_value<1, 2, 3, 4>(nvec, [&](auto cn) __attribute__((always_inline)) {
        constexpr int N = decltype(cn)::value;
        if (c) MGX_LAUNCH((block_residual3d_xs_kernel<N, true>), g, krylov_block(), 0, ctx->compute, a, c, n[0], n[1], n[2], bc, dev_work);
        else MGX_LAUNCH((block_residual3d_xs_kernel<N, false>), g, krylov_block(), 0, ctx->compute, a, c, n[0], n[1], n[2], bc, dev_work);
    });
    MGX_LAUNCH_CHECK();
    return krylov_final(ctx, dev_work, (size_t)g.x * g.y, 2 * nvec, dev_out);
}

static int eigen_start3d(mgx_ctx* ctx, double* v, int index, const int n[3], int bc) {
    MGX_REQUIRE(ctx && v && n, MGX_ERR_INVALID, "eigen_start: NULL argument");
    MGX_REQUIRE(index >= 0, MGX_ERR_INVALID, "eigen_start: index %d < 0", index);
    MGX_TRY_RET(eig_check(n, bc, "eigen_start"));
    MGX_USE(ctx);
    MGX_LAUNCH(eigen_start3d_xs_kernel, eig_grid_rows(n), krylov_block(), 0, ctx->compute, v, index, n[0], n[1], n[2], bc);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

}  // namespace mgx

extern "C" {

size_t mgx3dxs_block_work_elems_f64(const int n[3]) { return mgx::block_work_elems(n); }
int mgx3dxs_block_gram_f64(mgx_ctx* ctx, int nu, const double* const* U, int nv, const double* const* V, const double* c, const int n[3], int bc,
                           double* dev_work, double* dev_out) {
    return mgx::block_gram3d(ctx, nu, U, nv, V, c, n, bc, dev_work, dev_out);
}
int mgx3dxs_block_combine_f64(mgx_ctx* ctx, int nin, const double* const* S, int nout, double* const* out, const double* Y, const int n[3],
                              int bc) {
    return mgx::block_combine3d(ctx, nin, S, nout, out, Y, n, bc);
}
int mgx3dxs_block_residual_f64(mgx_ctx* ctx, int nvec, const double* const* AX, const double* const* X, const double* c, const double* mu,
                               double* const* R, const int n[3], int bc, double* dev_work, double* dev_out) {
    return mgx::block_residual3d(ctx, nvec, AX, X, c, mu, R, n, bc, dev_work, dev_out);
}
int mgx3dxs_eigen_start_f64(mgx_ctx* ctx, double* v, int index, const int n[3], int bc) { return mgx::eigen_start3d(ctx, v, index, n, bc); }

}  // extern "C"
