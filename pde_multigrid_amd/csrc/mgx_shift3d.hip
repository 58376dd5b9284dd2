// mgx_shift3d.hip -- the operators of the SHIFTED problem (Laplacian - s) u = f, s >= 0, x-split layout: the implicit step of
// diffusion (s = 1 / (kappa dt)) and the screened Poisson equation.  DESIGN.md section 13.
//
// The reference has no such operator; the arithmetic is fixed here (and restated in tests/op_restated.py), all in `real`,
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
// The operator's policy, ShiftOp, is in mgx_ops3d.hpp; this file holds what only this operator has; the kernels and their host drivers are the
// shared ones of mgx_stencil3d.hpp, instantiated with the policy:
//   relax_op3d_xs_kernel<real, ShiftOp, TYW, R>       one colour pass ("relax_shift3d_xs_kernel" to last_relax_kernel())
//   relax_op_zero3d_xs_kernel<real, ShiftOp>          the first red pass on a level that counts as zero: f in, red out, v not read
//   residual_op3d_xs_kernel<real, ShiftOp, MODE, LAP> r and / or the partials of <r, r>; with LAP: q = A p and the partials of <p, q>
//   shift_rhs3d_xs_kernel                             f = (-(s*u)) - qscale*q, the right-hand side of a backward Euler step
//   residual_restrict_axes3d_xs_kernel<..., SHIFT = true> (mgx_semi3d.hpp)   Restrict(residual) for the masks 1 .. 7
#include "mgx_ops3d.hpp"

namespace mgx {

// f = (-(s*u)) - qscale*q on the interior (q == NULL: f = -(s*u))
template <class real, bool Q>
__global__ void __launch_bounds__(256) shift_rhs3d_xs_kernel(const real* __restrict__ u, const real* __restrict__ q, real qscale, real s,
                                                             real* __restrict__ f, int sx, int sy) {
    const Geo<XSplit, real> g(sx, sy);
    const int y = 1 + blockIdx.x * KROWS + threadIdx.y, z = 1 + blockIdx.y;
    if (y >= sy - 1) return;
    const int H = g.H, P = g.P;
    const size_t row = g.row(y, z);
    for (int j0 = 0; j0 < P; j0 += KSTEP) {
        real uv[KJ], qv[KJ];
        bool in[KJ];
#pragma unroll
        for (int k = 0; k < KJ; k++) {
            const int j = j0 + k * 64 + threadIdx.x, x = xs_x(j, H);
            in[k] = j < P && x >= 1 && x <= sx - 2;
            if (in[k]) {
                uv[k] = u[row + j];
                if (Q) qv[k] = q[row + j];
            }
        }
#pragma unroll
        for (int k = 0; k < KJ; k++)
            if (in[k]) {
                real t = -(s * uv[k]);
                if (Q) t = t - qscale * qv[k];
                f[row + j0 + k * 64 + threadIdx.x] = t;
            }
    }
}

// =========================================================================== host side
template <class real>
static int shift_rhs3d(mgx_ctx* ctx, const real* u, const real* q, real qscale, real s, real* f, const int n[3]) {
    MGX_REQUIRE(ctx && u && f, MGX_ERR_INVALID, "shift_rhs: NULL argument");
    const double sd = (double)s;
    MGX_TRY_RET(rows_check(n, "shift_rhs", &sd));
    MGX_USE(ctx);
    const dim3 g = krylov_grid(n);
    if (q) MGX_LAUNCH((shift_rhs3d_xs_kernel<real, true>), g, krylov_block(), 0, ctx->compute, u, q, qscale, s, f, n[0], n[1]);
    else MGX_LAUNCH((shift_rhs3d_xs_kernel<real, false>), g, krylov_block(), 0, ctx->compute, u, q, qscale, s, f, n[0], n[1]);
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
        rim_zero3d_xs<real>(ctx, coarse_f, cn);
    if (cn[0] > 2 && cn[1] > 2 && cn[2] > 2) {
        constexpr int TYW = 4;
        with_value<1, 2, 3, 4, 5, 6, 7>(mask, [&](auto m) __attribute__((always_inline)) {
            constexpr int M = decltype(m)::value, CR = AxesRows<M>::value;
            const int gx = (M & 1) ? ceil_div(cn[0] - 2, 63) : ceil_div((n[0] - 1) / 2, 64);
            const int gy = ceil_div(cn[1] - 2, TYW * CR);
            int pzchunk = 16;  // runs of 16 coarse planes, halved while the launch has fewer than four workgroups per CU
            if (ctx->rr_pzchunk > 0) pzchunk = ctx->rr_pzchunk;  // "residual_restrict3d.pzchunk": the same bits for every run length
            else
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

// (the shared drivers take the coefficient array where this operator has none: NULL)
#define MGX_SHIFT3D_API(SFX, real)                                                                                                          \
    extern "C" int mgx3dxs_relax_shift_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], real s, int ncycles) {  \
        return mgx::relax_op3d<mgx::ShiftOp<real>, real>(ctx, v, f, nullptr, n, h, s, ncycles, 0, 0, "relax_shift");                        \
    }                                                                                                                                       \
    extern "C" int mgx3dxs_relax_shift_from_zero_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], real s,       \
                                                       int ncycles, int rim_is_zero) {                                                      \
        return mgx::relax_op3d<mgx::ShiftOp<real>, real>(ctx, v, f, nullptr, n, h, s, ncycles, 1, rim_is_zero, "relax_shift_from_zero");    \
    }                                                                                                                                       \
    extern "C" int mgx3dxs_residual_shift_##SFX(mgx_ctx* ctx, const real* v, const real* f, real* r, const int n[3], const real h[3],       \
                                                real s, double* dev_work, double* dev_sumsq) {                                              \
        return mgx::residual_op3d<mgx::ShiftOp<real>, real>(ctx, v, f, nullptr, r, n, h, s, dev_work, dev_sumsq, "residual_shift");         \
    }                                                                                                                                       \
    extern "C" int mgx3dxs_residual_restrict_shift_##SFX(mgx_ctx* ctx, const real* v, const real* f, const int n[3], const real h[3],       \
                                                         real s, real* coarse_f, const int cn[3], int coarse_rim_is_zero) {                 \
        return mgx::residual_restrict_shift3d<real>(ctx, v, f, n, h, s, coarse_f, cn, coarse_rim_is_zero);                                  \
    }                                                                                                                                       \
    extern "C" int mgx3dxs_laplace_dot_shift_##SFX(mgx_ctx* ctx, const real* p, real* q, const int n[3], const real h[3], real s,           \
                                                   double* dev_work, double* dev_sum) {                                                     \
        return mgx::apply_op_dot3d<mgx::ShiftOp<real>, real>(ctx, p, nullptr, q, n, h, s, dev_work, dev_sum, "laplace_dot_shift");          \
    }                                                                                                                                       \
    extern "C" int mgx3dxs_shift_rhs_##SFX(mgx_ctx* ctx, const real* u, const real* q, real qscale, real s, real* f, const int n[3]) {      \
        return mgx::shift_rhs3d<real>(ctx, u, q, qscale, s, f, n);                                                                          \
    }

MGX_SHIFT3D_API(f32, float)
MGX_SHIFT3D_API(f64, double)
