// mgx_shift3d.hip -- the operators of the SHIFTED problem (Laplacian - s) u = f, s >= 0, x-split layout: the implicit step of
// diffusion (s = 1 / (kappa dt)) and the screened Poisson equation.  DESIGN.md section 13.
//
// The reference has no such operator; the arithmetic is fixed here (and restated in tests/shift_restated.py), all in `real`,
// left to right as written, nothing contracted.  hx2 .. are the squared spacings, the names those of relax3d_point /
// residual3d_point (mgx_kernels3d.hpp):
//   smoother   v = num / den, num = relax3d_point's numerator, den = 2*(hy2*hz2 + hx2*hz2 + hx2*hy2) + s*hx2*hy2*hz2.  den is
//              the same for every point of a level: the host forms it once.  fp32 takes relax3d_point_rd's route, the quotient
//              as (float)((double)num * (1.0 / (double)den)) with a real division for results below FLT_MIN: its proof asks
//              nothing of den but to be an fp32 number.
//   residual   r = residual3d_point<real, 1>(...) + s*c on the interior (MGX_RESIDUAL_CORRECT only; with exact reciprocals of
//              the squared spacings where residual_scale allows them), 0 on the boundary
//   operator   q = A p = -(residual of p with f = 0) = Laplacian p - s p
// With s = 0 every one of them gives the bits of the unshifted operator (x + 0 = x for the positive den, r + 0*c = r up to
// the sign of a zero residual).
//
// Kernels:
//   relax_shift3d_xs_kernel          one colour pass, relax3d_xs_kernel's recipe: lane j owns the x-pair {2j, 2j+1} of R rows
//                                    and marches along z with its column in registers; non-temporal stores; XCD-aware tiles
//   relax_shift_zero3d_xs_kernel     the first red pass on a level that counts as zero: f in, red out, v not read
//   residual_shift3d_xs_kernel       r and / or the partials of <r, r>; with LAP: q = A p and the partials of <p, q>
//   shift_rhs3d_xs_kernel            f = (-(s*u)) - qscale*q, the right-hand side of a backward Euler step
//   residual_restrict_axes3d_xs_kernel<..., SHIFT = true> (mgx_semi3d.hpp)   Restrict(residual) for the masks 1 .. 7
#include <cmath>

#include "mgx_semi3d.hpp"

namespace mgx {

template <class real>
__device__ __forceinline__ real relax_shift3d_point(real O, real E, real N, real S, real D, real U, real f, real hx2, real hy2, real hz2,
                                                    real den, double rd) {
    const real num = O * (hy2 * hz2) + E * (hy2 * hz2) + N * (hx2 * hz2) + S * (hx2 * hz2) + D * (hx2 * hy2) + U * (hx2 * hy2) -
                     f * hx2 * hy2 * hz2;
    if constexpr (sizeof(real) == 4) {
        real q = (real)((double)num * rd);
        if (__builtin_expect(!(__builtin_fabsf(q) >= 1.17549435e-38f), 0)) q = num / den;
        return q;
    } else {
        return num / den;
    }
}

// ------------------------------------------------------------------ relax, one colour
// relax3d_xs_kernel (mgx_kernels3d.hip) with the shifted denominator: the same lane / row / plane assignment, the same loads
// (per step and lane R streaming loads of v and of f, the side value from the neighbouring lane, the two edge rows from L1 /
// L2), the same stores.  den and rd = 1 / den (fp32's route) are kernel arguments.
template <class real, int TYW, int R>
__global__ void __launch_bounds__(64 * TYW)
    relax_shift3d_xs_kernel(const real* __restrict__ vin, real* __restrict__ vout, const real* __restrict__ f, int sx, int sy, int zbeg,
                            int zend, real hx2, real hy2, real hz2, real den, double rd, int colour, int zchunk, int gx, int gy,
                            int xcd_mode) {
    const Geo<XSplit, real> g(sx, sy);
    const int H = g.H;
    const int M = (sx + 1) >> 1;  // entries of the even-x half (the odd-x half has M-1)
    int bx, by, bz;
    tile_of_block(xcd_mode, gx, gy, bx, by, bz);
    const int j = bx * 64 + threadIdx.x;
    const int y0 = 1 + (by * TYW + __builtin_amdgcn_readfirstlane(threadIdx.y)) * R;  // wave-uniform
    if (y0 >= sy - 1 || j >= M - 1) return;  // x = 2j+q <= sx-2 needs j <= M-2
    const int nrows = min(R, sy - 1 - y0);    // rows y0 .. y0+nrows-1 are interior
    const int z0 = zbeg + bz * zchunk;
    const int z1 = min(z0 + zchunk, zend);
    if (z0 >= z1) return;
    const size_t sxy = g.PL;
    const int P = g.P;
    // row bases at plane z0; rows past sy-1 are clamped onto it (loads stay valid, nothing is stored for r >= nrows)
    size_t rowb[R];
#pragma unroll
    for (int r = 0; r < R; r++) rowb[r] = g.row(min(y0 + r, sy - 1), z0);
    int q = (colour + y0 + z0) & 1;  // parity of row r is q ^ (r & 1)
    real c_prev[R], c_cur[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int qr = q ^ (r & 1);
        c_prev[r] = vin[rowb[r] - sxy + qr * H + j];  // (half q_r,   j, plane z0-1)
        c_cur[r] = vin[rowb[r] + (1 - qr) * H + j];   // (half 1-q_r, j, plane z0)
    }
    for (int z = z0; z < z1; z++) {
        real U[R], side[R], fv[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int hq = (q ^ (r & 1)) * H;
            U[r] = vin[rowb[r] + sxy + hq + j];
            fv[r] = f[rowb[r] + hq + j];
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int qr = q ^ (r & 1);
            // the side value is the "own" value of the neighbouring lane (j+1 when q_r = 1, j-1 when q_r = 0).  The wave's edge
            // lane, and the last active lane (lane j+1 = M-1 has exited), load it; lane j = 0 with q_r = 0 (x = 0, never
            // written) reads index M-1 of half 0 instead of index -1 and discards the result
            const real nb = qr ? __shfl_down(c_cur[r], 1, 64) : __shfl_up(c_cur[r], 1, 64);
            const bool edge = qr ? (threadIdx.x == 63 || j == M - 2) : (threadIdx.x == 0);
            side[r] = edge ? vin[rowb[r] + (1 - qr) * H + j + (qr ? 1 : -1) + (qr | j ? 0 : M)] : nb;
        }
        const real Nedge = vin[rowb[0] - P + q * H + j];
        const real Sedge = vin[rowb[R - 1] + P + (q ^ ((R - 1) & 1)) * H + j];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int qr = q ^ (r & 1);
            const real W = qr ? c_cur[r] : side[r];
            const real E = qr ? side[r] : c_cur[r];
            const real N = r == 0 ? Nedge : c_cur[r - 1];
            const real S = r == R - 1 ? Sedge : c_cur[r + 1];
            const real out = relax_shift3d_point<real>(W, E, N, S, c_prev[r], U[r], fv[r], hx2, hy2, hz2, den, rd);
            if ((qr | j) && r < nrows) __builtin_nontemporal_store(out, &vout[rowb[r] + qr * H + j]);  // x = 2j+q_r >= 1
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            c_prev[r] = c_cur[r];
            c_cur[r] = U[r];
            rowb[r] += sxy;
        }
        q ^= 1;
    }
}

// the first red pass of a level that counts as all zeros (boundary entries zero in memory): the point expression on six zero
// neighbours, evaluated as such (the signs of zeros are those of the generic pass on a zeroed array); v is not read
template <class real>
__global__ void __launch_bounds__(256) relax_shift_zero3d_xs_kernel(real* __restrict__ v, const real* __restrict__ f, int sx, int sy, real hx2,
                                                                    real hy2, real hz2, real den, double rd) {
    const int y = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int z = 1 + blockIdx.z;
    if (y >= sy - 1) return;
    const int x = 2 * (blockIdx.x * blockDim.x + threadIdx.x) + ((y + z) & 1);
    if (x < 1 || x >= sx - 1) return;
    const Geo<XSplit, real> g(sx, sy);
    const size_t idx = g.row(y, z) + g.pos(x);
    const real zero = (real)0;
    __builtin_nontemporal_store(relax_shift3d_point<real>(zero, zero, zero, zero, zero, zero, f[idx], hx2, hy2, hz2, den, rd), &v[idx]);
}

// ------------------------------------------------------------------ residual / operator with a sum
// The Krylov kernels' walk (mgx_krylov3d.hip): one wave per interior x-row, its lanes over the row's storage positions, SJ
// positions per lane and step with the loads first; sums in double in a fixed order (per lane in loop order, wave shuffles,
// the block's four waves in order, one partial per block, then the final kernel).
constexpr int SJ = 4, SROWS = 4, SSTEP = 64 * SJ;

__device__ __forceinline__ int shift_x_of(int j, int H) { return j < H ? 2 * j : 2 * (j - H) + 1; }  // pads give x >= sx

__device__ __forceinline__ void shift_block_sum(double acc, double* part, double* __restrict__ partial) {
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (threadIdx.x == 0) part[threadIdx.y] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// LAP = false: r = residual(v, f) + s v (stored unless out is NULL), partials of <r, r> unless partial is NULL
// LAP = true:  out = q = -(residual(v, 0) + s v), partials of <v, q>
template <class real, int MODE, bool LAP>
__global__ void __launch_bounds__(256) residual_shift3d_xs_kernel(const real* __restrict__ v, const real* __restrict__ f, real* __restrict__ out,
                                                                  int sx, int sy, real qx, real qy, real qz, real s,
                                                                  double* __restrict__ partial) {
    const Geo<XSplit, real> g(sx, sy);
    const int y = 1 + blockIdx.x * SROWS + threadIdx.y, z = 1 + blockIdx.y;
    const int H = g.H, P = g.P;
    const size_t PL = g.PL;
    double acc = 0.0;
    if (y < sy - 1) {
        const size_t row = g.row(y, z);
        for (int j0 = 0; j0 < P; j0 += SSTEP) {
            real O[SJ], E[SJ], N[SJ], S[SJ], D[SJ], U[SJ], c[SJ], fv[SJ];
            bool in[SJ];
#pragma unroll
            for (int k = 0; k < SJ; k++) {
                const int j = j0 + k * 64 + threadIdx.x, x = shift_x_of(j, H);
                in[k] = j < P && x >= 1 && x <= sx - 2;
                if (in[k]) {
                    const size_t i = row + j;
                    O[k] = v[row + XSplit::pos(x - 1, H)];
                    E[k] = v[row + XSplit::pos(x + 1, H)];
                    N[k] = v[i - P];
                    S[k] = v[i + P];
                    D[k] = v[i - PL];
                    U[k] = v[i + PL];
                    c[k] = v[i];
                    fv[k] = LAP ? (real)0 : f[i];
                }
            }
#pragma unroll
            for (int k = 0; k < SJ; k++)
                if (in[k]) {
                    real t = residual3d_point<real, MODE>(O[k], E[k], N[k], S[k], D[k], U[k], c[k], fv[k], qx, qy, qz) + s * c[k];
                    if (LAP) t = -t;  // negation is exact
                    if (out) out[row + j0 + k * 64 + threadIdx.x] = t;
                    acc += LAP ? (double)c[k] * (double)t : (double)t * (double)t;
                }
        }
    }
    if (partial) {  // (uniform over the launch)
        __shared__ double part[SROWS];
        shift_block_sum(acc, part, partial);
    }
}

// f = (-(s*u)) - qscale*q on the interior (q == NULL: f = -(s*u))
template <class real, bool Q>
__global__ void __launch_bounds__(256) shift_rhs3d_xs_kernel(const real* __restrict__ u, const real* __restrict__ q, real qscale, real s,
                                                             real* __restrict__ f, int sx, int sy) {
    const Geo<XSplit, real> g(sx, sy);
    const int y = 1 + blockIdx.x * SROWS + threadIdx.y, z = 1 + blockIdx.y;
    if (y >= sy - 1) return;
    const int H = g.H, P = g.P;
    const size_t row = g.row(y, z);
    for (int j0 = 0; j0 < P; j0 += SSTEP) {
        real uv[SJ], qv[SJ];
        bool in[SJ];
#pragma unroll
        for (int k = 0; k < SJ; k++) {
            const int j = j0 + k * 64 + threadIdx.x, x = shift_x_of(j, H);
            in[k] = j < P && x >= 1 && x <= sx - 2;
            if (in[k]) {
                uv[k] = u[row + j];
                if (Q) qv[k] = q[row + j];
            }
        }
#pragma unroll
        for (int k = 0; k < SJ; k++)
            if (in[k]) {
                real t = -(s * uv[k]);
                if (Q) t = t - qscale * qv[k];
                f[row + j0 + k * 64 + threadIdx.x] = t;
            }
    }
}

// =========================================================================== host side
static int shift_check(const int n[3], double s, const char* what, bool rows_grid) {
    MGX_REQUIRE(n, MGX_ERR_INVALID, "%s: size array is NULL", what);
    MGX_REQUIRE(std::isfinite(s) && s >= 0, MGX_ERR_INVALID, "%s: the shift %g is not finite and >= 0", what, s);
    for (int d = 0; d < 3; d++) MGX_REQUIRE(valid_size(n[d]), MGX_ERR_SIZE, "%s: size[%d] = %d is not odd and >= 3", what, d, n[d]);
    MGX_REQUIRE((double)n[0] * n[1] * n[2] < 2147483647.0 * 4, MGX_ERR_SIZE, "%s: grid too large", what);
    MGX_REQUIRE(!rows_grid || n[2] - 2 <= 65535, MGX_ERR_SIZE, "%s: %d planes are too many", what, n[2]);
    return MGX_OK;
}

// what the smoother's kernels take besides the squared spacings: den and, for fp32's route, 1 / den in double
template <class real>
struct ShiftDen {
    real hx2, hy2, hz2, den;
    double rd;
    ShiftDen(const real h[3], real s) : hx2(h[0] * h[0]), hy2(h[1] * h[1]), hz2(h[2] * h[2]) {
        den = 2 * (hy2 * hz2 + hx2 * hz2 + hx2 * hy2) + s * hx2 * hy2 * hz2;
        rd = sizeof(real) == 4 ? 1.0 / (double)den : 0.0;
    }
};

// one colour pass over the planes 1 .. sz-2: relax3d_xs_kernel's launch geometry (four waves of four rows, fewer on small
// levels; runs of four planes, halved while the launch has fewer than eight workgroups per CU)
template <class real>
static void relax_shift3d_pass(mgx_ctx* ctx, real* v, const real* f, const int n[3], const ShiftDen<real>& d, int colour) {
    const int sx = n[0], sy = n[1], zbeg = 1, zend = n[2] - 1;
    int ty = 4, rows = 4;
    while (rows > 1 && rows * ty > sy - 2) rows >>= 1;
    while (ty > 1 && rows * ty > sy - 2) ty >>= 1;
    const int gx = ceil_div((sx + 1) / 2 - 1, 64), gy = ceil_div(sy - 2, ty * rows);
    int zchunk = 4;
    while (zchunk > 1 && (long long)gx * gy * ceil_div(zend - zbeg, zchunk) < 8LL * ctx->num_cus) zchunk >>= 1;
    const unsigned nblocks = (unsigned)gx * gy * ceil_div(zend - zbeg, zchunk);
    const int xcd = ctx->relax_xcd == 1 ? 1 : 0;
    with_value<1, 2, 4>(ty, [&](auto t) __attribute__((always_inline)) {
        with_value<1, 2, 4>(rows, [&](auto r) __attribute__((always_inline)) {
            constexpr int TYW = decltype(t)::value, RR = decltype(r)::value;
            note_relax_kernel<real>(ctx, "relax_shift3d_xs_kernel", TYW, RR, 0);
            MGX_LAUNCH((relax_shift3d_xs_kernel<real, TYW, RR>), dim3(nblocks), dim3(64, TYW, 1), 0, ctx->compute, (const real*)v, v, f, sx, sy,
                       zbeg, zend, d.hx2, d.hy2, d.hz2, d.den, d.rd, colour, zchunk, gx, gy, xcd);
        });
    });
}

template <class real>
static int relax_shift3d(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], real s, int ncycles, int from_zero,
                         int rim_is_zero) {
    const char* what = from_zero ? "relax_shift_from_zero" : "relax_shift";
    MGX_REQUIRE(ctx && v && f && h, MGX_ERR_INVALID, "%s: NULL argument", what);
    MGX_TRY_RET(shift_check(n, (double)s, what, false));
    MGX_REQUIRE(ncycles >= 0, MGX_ERR_INVALID, "%s: ncycles = %d < 0", what, ncycles);
    MGX_USE(ctx);
    const ShiftDen<real> d(h, s);
    int s0 = 0;
    if (from_zero && (!rim_is_zero || ncycles == 0)) {  // v := 0 everywhere, then generic passes
        MGX_TRY_RET(fill_zero(ctx, v, Geo<XSplit, real>(n[0], n[1]).PL * (size_t)n[2] * sizeof(real)));
    } else if (from_zero) {  // nothing is filled and the first red pass does not read v
        note_relax_kernel<real>(ctx, "relax_shift_zero3d_xs_kernel", 0, 0, 0);
        MGX_LAUNCH((relax_shift_zero3d_xs_kernel<real>), dim3(ceil_div((n[0] + 1) / 2, 64), ceil_div(n[1] - 2, 4), n[2] - 2), dim3(64, 4, 1), 0,
                   ctx->compute, v, f, n[0], n[1], d.hx2, d.hy2, d.hz2, d.den, d.rd);
        s0 = 1;
    }
    for (int p = s0; p < 2 * ncycles; p++) relax_shift3d_pass<real>(ctx, v, f, n, d, p & 1);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

static dim3 shift_rows_grid(const int n[3]) { return dim3((unsigned)ceil_div(n[1] - 2, SROWS), (unsigned)(n[2] - 2)); }

template <class real>
static int residual_shift3d(mgx_ctx* ctx, const real* v, const real* f, real* r, const int n[3], const real h[3], real s, double* dev_work,
                            double* dev_sumsq) {
    MGX_REQUIRE(ctx && v && f && h && (r || dev_sumsq) && (!dev_sumsq || dev_work), MGX_ERR_INVALID, "residual_shift: NULL argument");
    MGX_TRY_RET(shift_check(n, (double)s, "residual_shift", true));
    MGX_USE(ctx);
    const ResidualScale<real> sc = residual_scale<real>(ctx, h, MGX_RESIDUAL_CORRECT);  // MODE 1, or 3 with exact reciprocals
    const dim3 g = shift_rows_grid(n);
    if (r)  // the boundary of r is 0, as mgx3dxs_residual leaves it
        MGX_LAUNCH((rim_zero3d_xs_kernel<real>), dim3(ceil_div(n[0], 64), ceil_div(n[1], 4), n[2]), dim3(64, 4, 1), 0, ctx->compute, r, n[0], n[1],
                   n[2]);
    with_value<1, 3>(sc.mode, [&](auto m) __attribute__((always_inline)) {
        MGX_LAUNCH((residual_shift3d_xs_kernel<real, decltype(m)::value, false>), g, dim3(64, SROWS, 1), 0, ctx->compute, v, f, r, n[0], n[1],
                   sc.qx, sc.qy, sc.qz, s, dev_sumsq ? dev_work : (double*)nullptr);
    });
    MGX_LAUNCH_CHECK();
    return dev_sumsq ? krylov_final(ctx, dev_work, (size_t)g.x * g.y, 1, dev_sumsq) : MGX_OK;
}

template <class real>
static int laplace_dot_shift3d(mgx_ctx* ctx, const real* p, real* q, const int n[3], const real h[3], real s, double* dev_work, double* dev_sum) {
    MGX_REQUIRE(ctx && p && q && h && dev_work && dev_sum, MGX_ERR_INVALID, "laplace_dot_shift: NULL argument");
    MGX_TRY_RET(shift_check(n, (double)s, "laplace_dot_shift", true));
    MGX_USE(ctx);
    const ResidualScale<real> sc = residual_scale<real>(ctx, h, MGX_RESIDUAL_CORRECT);
    const dim3 g = shift_rows_grid(n);
    with_value<1, 3>(sc.mode, [&](auto m) __attribute__((always_inline)) {
        MGX_LAUNCH((residual_shift3d_xs_kernel<real, decltype(m)::value, true>), g, dim3(64, SROWS, 1), 0, ctx->compute, p, (const real*)nullptr, q,
                   n[0], n[1], sc.qx, sc.qy, sc.qz, s, dev_work);
    });
    MGX_LAUNCH_CHECK();
    return krylov_final(ctx, dev_work, (size_t)g.x * g.y, 1, dev_sum);
}

template <class real>
static int shift_rhs3d(mgx_ctx* ctx, const real* u, const real* q, real qscale, real s, real* f, const int n[3]) {
    MGX_REQUIRE(ctx && u && f, MGX_ERR_INVALID, "shift_rhs: NULL argument");
    MGX_TRY_RET(shift_check(n, (double)s, "shift_rhs", true));
    MGX_USE(ctx);
    const dim3 g = shift_rows_grid(n);
    if (q) MGX_LAUNCH((shift_rhs3d_xs_kernel<real, true>), g, dim3(64, SROWS, 1), 0, ctx->compute, u, q, qscale, s, f, n[0], n[1]);
    else MGX_LAUNCH((shift_rhs3d_xs_kernel<real, false>), g, dim3(64, SROWS, 1), 0, ctx->compute, u, q, qscale, s, f, n[0], n[1]);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// coarse_f = R_mask(residual): the launch of mgx_semi3d.hip's residual_restrict_axes3d with the shift, and with mask 7
template <class real>
static int residual_restrict_shift3d(mgx_ctx* ctx, const real* v, const real* f, const int n[3], const real h[3], real s, real* coarse_f,
                                     const int cn[3], int coarse_rim_is_zero) {
    MGX_REQUIRE(ctx && v && f && h && coarse_f, MGX_ERR_INVALID, "residual_restrict_shift: NULL argument");
    MGX_REQUIRE(std::isfinite((double)s) && s >= 0, MGX_ERR_INVALID, "residual_restrict_shift: the shift %g is not finite and >= 0", (double)s);
    int mask = 0;
    MGX_TRY_RET(axes_mask(n, cn, "residual_restrict_shift", &mask));
    MGX_USE(ctx);
    const ResidualScale<real> sc = residual_scale<real>(ctx, h, MGX_RESIDUAL_CORRECT);
    if (!coarse_rim_is_zero)
        MGX_LAUNCH((rim_zero3d_xs_kernel<real>), dim3(ceil_div(cn[0], 64), ceil_div(cn[1], 4), cn[2]), dim3(64, 4, 1), 0, ctx->compute, coarse_f,
                   cn[0], cn[1], cn[2]);
    if (cn[0] > 2 && cn[1] > 2 && cn[2] > 2) {
        constexpr int TYW = 4;
        with_value<1, 2, 3, 4, 5, 6, 7>(mask, [&](auto m) __attribute__((always_inline)) {
            constexpr int M = decltype(m)::value, CR = AxesRows<M>::value;
            const int gx = (M & 1) ? ceil_div(cn[0] - 2, 63) : ceil_div((n[0] - 1) / 2, 64);
            const int gy = ceil_div(cn[1] - 2, TYW * CR);
            int pzchunk = 16;  // runs of 16 coarse planes, halved while the launch has fewer than four workgroups per CU
            while (pzchunk > 2 && (long long)gx * gy * ceil_div(cn[2] - 2, pzchunk) < 4LL * ctx->num_cus) pzchunk >>= 1;
            const int gz = ceil_div(cn[2] - 2, pzchunk);
            with_value<1, 3>(sc.mode, [&](auto md) __attribute__((always_inline)) {
                MGX_LAUNCH((residual_restrict_axes3d_xs_kernel<real, M, decltype(md)::value, CR, TYW, true>), dim3((unsigned)(gx * gy * gz)),
                           dim3(64, TYW, 1), 0, ctx->compute, v, f, n[0], n[1], n[2], sc.qx, sc.qy, sc.qz, coarse_f, cn[0], cn[1], cn[2], pzchunk,
                           gx, gy, s);
            });
        });
    }
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

}  // namespace mgx

#define MGX_SHIFT3D_API(SFX, real)                                                                                                          \
    extern "C" int mgx3dxs_relax_shift_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], real s, int ncycles) {  \
        return mgx::relax_shift3d<real>(ctx, v, f, n, h, s, ncycles, 0, 0);                                                                 \
    }                                                                                                                                       \
    extern "C" int mgx3dxs_relax_shift_from_zero_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], real s,       \
                                                       int ncycles, int rim_is_zero) {                                                      \
        return mgx::relax_shift3d<real>(ctx, v, f, n, h, s, ncycles, 1, rim_is_zero);                                                       \
    }                                                                                                                                       \
    extern "C" int mgx3dxs_residual_shift_##SFX(mgx_ctx* ctx, const real* v, const real* f, real* r, const int n[3], const real h[3],       \
                                                real s, double* dev_work, double* dev_sumsq) {                                              \
        return mgx::residual_shift3d<real>(ctx, v, f, r, n, h, s, dev_work, dev_sumsq);                                                     \
    }                                                                                                                                       \
    extern "C" int mgx3dxs_residual_restrict_shift_##SFX(mgx_ctx* ctx, const real* v, const real* f, const int n[3], const real h[3],       \
                                                         real s, real* coarse_f, const int cn[3], int coarse_rim_is_zero) {                 \
        return mgx::residual_restrict_shift3d<real>(ctx, v, f, n, h, s, coarse_f, cn, coarse_rim_is_zero);                                  \
    }                                                                                                                                       \
    extern "C" int mgx3dxs_laplace_dot_shift_##SFX(mgx_ctx* ctx, const real* p, real* q, const int n[3], const real h[3], real s,           \
                                                   double* dev_work, double* dev_sum) {                                                     \
        return mgx::laplace_dot_shift3d<real>(ctx, p, q, n, h, s, dev_work, dev_sum);                                                       \
    }                                                                                                                                       \
    extern "C" int mgx3dxs_shift_rhs_##SFX(mgx_ctx* ctx, const real* u, const real* q, real qscale, real s, real* f, const int n[3]) {      \
        return mgx::shift_rhs3d<real>(ctx, u, q, qscale, s, f, n);                                                                          \
    }

MGX_SHIFT3D_API(f32, float)
MGX_SHIFT3D_API(f64, double)
