// mgx_cap3d.hip -- the operators of div(a grad u) - (s c) u = f with a CAPACITY c >= 0 at the grid nodes next to the coefficient
// a > 0, s >= 0, x-split layout: the implicit step of c u_t = kappa div(a grad u) + q (conductivity and volumetric heat capacity
// jump together in a composite), a reaction term that varies in space, screened problems that are purely elliptic where c = 0.
// DESIGN.md section 17.
//
// The arithmetic is mgx_coef3d.hip's (restated in tests/op_restated.py) with ONE more operation per point, in `real`:
//   sc = s * c_P            c_P the capacity at the updated point itself (f's index; nothing of c is read around it)
// and then relax_coef3d_point / residual_coef3d_point with sc where they take s.  With c == 1 every result has the bits of the
// coefficient operator.  c is never written and its values are not checked here.  At an unknown on a Neumann face the operator
// takes the capacity of that point: only the centre is read, so nothing is mirrored.
//
// The operator's policy, CapOp, is in mgx_ops3d.hpp and carries the array; the kernels and their host drivers are the shared ones of
// mgx_stencil3d.hpp, instantiated with the policy in this unit only (the drivers of mgx_rim3d.hpp reach the kernels of the face
// unknowns, which mgx_wall3d.hip instantiates for CapOp too, through that unit's launch functions):
//   relax_op3d_xs_kernel<real, CapOp, TYW, R>      one colour pass ("relax_cap3d_xs_kernel" to last_relax_kernel()): the coefficient
//                                                  pass plus one streaming load of c per step and row, 3.0 words per point and pass
//   relax_op_zero3d_xs_kernel<real, CapOp>         the first red pass on a level that counts as zero
//   residual_op3d_xs_kernel<real, CapOp, 1, LAP>   r and / or the partials of <r, r>; with LAP: q = A p and the partials of <p, q>
//   cap_rhs3d_xs_kernel, rim_cap_rhs3d_xs_kernel   f = (-((s*c)*u)) - qscale*q, the right-hand side of a backward Euler step
#include "mgx_rim3d.hpp"

namespace mgx {

// f = (-((s*c)*u)) - qscale*q on the interior (q == NULL: f = -((s*c)*u)): shift_rhs3d_xs_kernel's expression with s*c_P for s
template <class real, bool Q>
__global__ void __launch_bounds__(256) cap_rhs3d_xs_kernel(const real* __restrict__ u, const real* __restrict__ c, const real* __restrict__ q,
                                                           real qscale, real s, real* __restrict__ f, int sx, int sy) {
    const Geo<XSplit, real> g(sx, sy);
    const int y = 1 + blockIdx.x * KROWS + threadIdx.y, z = 1 + blockIdx.y;
    if (y >= sy - 1) return;
    const int H = g.H, P = g.P;
    const size_t row = g.row(y, z);
    for (int j0 = 0; j0 < P; j0 += KSTEP) {
        real uv[KJ], cv[KJ], qv[KJ];
        bool in[KJ];
#pragma unroll
        for (int k = 0; k < KJ; k++) {
            const int j = j0 + k * 64 + threadIdx.x, x = xs_x(j, H);
            in[k] = j < P && x >= 1 && x <= sx - 2;
            if (in[k]) {
                uv[k] = u[row + j];
                cv[k] = c[row + j];
                if (Q) qv[k] = q[row + j];
            }
        }
#pragma unroll
        for (int k = 0; k < KJ; k++)
            if (in[k]) {
                const real sc = s * cv[k];
                real t = -(sc * uv[k]);
                if (Q) t = t - qscale * qv[k];
                f[row + j0 + k * 64 + threadIdx.x] = t;
            }
    }
}

// ... and on the face unknowns
template <class real>
__global__ void __launch_bounds__(RIM_THREADS) rim_cap_rhs3d_xs_kernel(const real* __restrict__ u, const real* __restrict__ c,
                                                                       const real* __restrict__ q, real qscale, real s, real* __restrict__ f,
                                                                       Rim R) {
    const Geo<XSplit, real> g(R.sx, R.sy);
    RIM_FOR_EACH_POINT(R, g, x, y, z) {
        const size_t i = g.row(y, z) + g.pos(x);
        const real sc = s * c[i];
        real t = -(sc * u[i]);
        if (q) t = t - qscale * q[i];
        f[i] = t;
    }
}

// =========================================================================== host side
template <class real>
static int cap_rhs3d(mgx_ctx* ctx, const real* u, const real* c, const real* q, real qscale, real s, real* f, const int n[3], int bc,
                     const char* what) {
    MGX_REQUIRE(ctx && u && c && f && n, MGX_ERR_INVALID, "%s: NULL argument", what);
    RIM_BC_CHECK(bc, what);
    const double sd = (double)s;
    MGX_TRY_RET(rows_check(n, what, &sd));
    Rim R = {};
    if (bc) MGX_TRY_RET(rim_list<real>(n, bc, what, R));
    MGX_USE(ctx);
    const dim3 g = krylov_grid(n);
    if (q) MGX_LAUNCH((cap_rhs3d_xs_kernel<real, true>), g, krylov_block(), 0, ctx->compute, u, c, q, qscale, s, f, n[0], n[1]);
    else MGX_LAUNCH((cap_rhs3d_xs_kernel<real, false>), g, krylov_block(), 0, ctx->compute, u, c, q, qscale, s, f, n[0], n[1]);
    if (bc) MGX_LAUNCH((rim_cap_rhs3d_xs_kernel<real>), dim3(rim_blocks(R)), dim3(RIM_THREADS), 0, ctx->compute, u, c, q, qscale, s, f, R);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

}  // namespace mgx

#define MGX_CAP3D_API(SFX, real)                                                                                                             \
    extern "C" int mgx3dxs_relax_cap_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const real* c, const int n[3],               \
                                           const real h[3], real s, int ncycles) {                                                           \
        return mgx::relax_op3d<mgx::CapOp<real>, real>(ctx, v, f, a, n, h, s, ncycles, 0, 0, "relax_cap", c);                                \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_relax_cap_from_zero_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const real* c, const int n[3],     \
                                                     const real h[3], real s, int ncycles, int rim_is_zero) {                                \
        return mgx::relax_op3d<mgx::CapOp<real>, real>(ctx, v, f, a, n, h, s, ncycles, 1, rim_is_zero, "relax_cap_from_zero", c);            \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_residual_cap_##SFX(mgx_ctx* ctx, const real* v, const real* f, const real* a, const real* c, real* r,             \
                                              const int n[3], const real h[3], real s, double* dev_work, double* dev_sumsq) {                \
        return mgx::residual_op3d<mgx::CapOp<real>, real>(ctx, v, f, a, r, n, h, s, dev_work, dev_sumsq, "residual_cap", c);                 \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_apply_cap_dot_##SFX(mgx_ctx* ctx, const real* p, const real* a, const real* c, real* q, const int n[3],           \
                                               const real h[3], real s, double* dev_work, double* dev_sum) {                                 \
        return mgx::apply_op_dot3d<mgx::CapOp<real>, real>(ctx, p, a, q, n, h, s, dev_work, dev_sum, "apply_cap_dot", c);                    \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_cap_rhs_##SFX(mgx_ctx* ctx, const real* u, const real* c, const real* q, real qscale, real s, real* f,            \
                                         const int n[3]) {                                                                                   \
        return mgx::cap_rhs3d<real>(ctx, u, c, q, qscale, s, f, n, 0, "cap_rhs");                                                            \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_relax_cap_bc_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const real* c, const int n[3],            \
                                              const real h[3], real s, int ncycles, int bc) {                                                \
        return mgx::relax_op3d_bc<mgx::CapOp<real>, real>(ctx, v, f, a, n, h, s, ncycles, bc, mgx::NO_WALL<real>, "relax_cap_bc", c);        \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_residual_cap_bc_##SFX(mgx_ctx* ctx, const real* v, const real* f, const real* a, const real* c, real* r,          \
                                                 const int n[3], const real h[3], real s, double* dev_work, double* dev_sumsq, int bc) {     \
        return mgx::residual_op3d_bc<mgx::CapOp<real>, real>(ctx, v, f, a, r, n, h, s, dev_work, dev_sumsq, bc,                              \
                                                             mgx::NO_WALL<real>, "residual_cap_bc", c);                                      \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_apply_cap_dot_bc_##SFX(mgx_ctx* ctx, const real* p, const real* a, const real* c, real* q, const int n[3],        \
                                                  const real h[3], real s, double* dev_work, double* dev_sum, int bc) {                      \
        return mgx::apply_op_dot3d_bc<mgx::CapOp<real>, real>(ctx, p, a, q, n, h, s, dev_work, dev_sum, bc,                                  \
                                                              mgx::NO_WALL<real>, "apply_cap_dot_bc", c);                                    \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_relax_cap_wall_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const real* c, const int n[3],          \
                                                const real h[3], real s, int ncycles, int bc, const real beta[6]) {                          \
        return mgx::relax_op3d_bc<mgx::CapOp<real>, real>(ctx, v, f, a, n, h, s, ncycles, bc, beta, "relax_cap_wall", c);                    \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_relax_cap_pin_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const real* c, const int n[3], const real h[3], real s, int ncycles, int bc, const real beta[6], const unsigned* idx, \
            const unsigned end[2], const real* val) {                                                                                        \
        MGX_REQUIRE(end, MGX_ERR_INVALID, "relax_cap_pin: NULL argument");                                                                   \
        const mgx::PinList<real> pin = {idx, {end[0], end[1]}, val};                                                                         \
        return mgx::relax_op3d_bc<mgx::CapOp<real>, real>(ctx, v, f, a, n, h, s, ncycles, bc, beta, "relax_cap_pin", c, &pin);               \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_residual_cap_wall_##SFX(mgx_ctx* ctx, const real* v, const real* f, const real* a, const real* c, real* r,        \
                                                   const int n[3], const real h[3], real s, double* dev_work, double* dev_sumsq, int bc,     \
                                                   const real beta[6]) {                                                                     \
        return mgx::residual_op3d_bc<mgx::CapOp<real>, real>(ctx, v, f, a, r, n, h, s, dev_work, dev_sumsq, bc, beta, "residual_cap_wall",   \
                                                               c);                                                                           \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_apply_cap_dot_wall_##SFX(mgx_ctx* ctx, const real* p, const real* a, const real* c, real* q, const int n[3],      \
                                                    const real h[3], real s, double* dev_work, double* dev_sum, int bc, const real beta[6]) {\
        return mgx::apply_op_dot3d_bc<mgx::CapOp<real>, real>(ctx, p, a, q, n, h, s, dev_work, dev_sum, bc, beta, "apply_cap_dot_wall", c);  \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_cap_rhs_bc_##SFX(mgx_ctx* ctx, const real* u, const real* c, const real* q, real qscale, real s, real* f,         \
                                            const int n[3], int bc) {                                                                        \
        return mgx::cap_rhs3d<real>(ctx, u, c, q, qscale, s, f, n, bc, "cap_rhs_bc");                                                        \
    }

MGX_CAP3D_API(f32, float)
MGX_CAP3D_API(f64, double)
