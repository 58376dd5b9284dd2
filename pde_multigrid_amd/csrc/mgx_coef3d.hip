// mgx_coef3d.hip -- the operators of the VARIABLE-COEFFICIENT problem div(a grad u) - s u = f, a > 0 given at the grid nodes,
// s >= 0, x-split layout: heterogeneous diffusion (conductivity, permeability, 1 / density).  DESIGN.md section 14.
//
// The reference has no such operator; the arithmetic is fixed here (and restated in tests/op_restated.py), all in `real`,
// left to right as written, nothing contracted.  O/E = x-1/x+1, N/S = y-1/y+1, D/U = z-1/z+1, c the centre; aO .. aU, aC the
// coefficient at the same seven points; qx = (real)0.5 / (h[0]*h[0]) (likewise qy, qz), formed by the host once per call:
//   AW = aO + aC  AE = aE + aC  AN = aN + aC  AS = aS + aC  AD = aD + aC  AU = aU + aC
//   tx = qx*(AW*(O - c) + AE*(E - c))   ty = qy*(AN*(N - c) + AS*(S - c))   tz = qz*(AD*(D - c) + AU*(U - c))
//   residual   r = (((f - tx) - ty) - tz) + s*c on the interior, 0 on the boundary
//   operator   q = A p = -(residual of p with f = 0)
//   smoother   v = num / den (a real division in both precisions),
//              den = ((qx*(AW + AE) + qy*(AN + AS)) + qz*(AD + AU)) + s
//              num = ((qx*(AW*O + AE*E) + qy*(AN*N + AS*S)) + qz*(AD*D + AU*U)) - f
// The conservative 7-point form with arithmetic-mean face coefficients, the 1/2 of each mean folded into q*.  a is read on
// the boundary too (interior points next to a face read it there) and never written.
//
// The operator's policy, CoefOp, is in mgx_ops3d.hpp; the kernels and their host drivers are the shared ones of mgx_stencil3d.hpp,
// instantiated with the policy:
//   relax_op3d_xs_kernel<real, CoefOp, TYW, R>     one colour pass ("relax_coef3d_xs_kernel" to last_relax_kernel()), a marched
//                                                  next to v: per step and row it loads one entry of v, one of f and BOTH entries
//                                                  of a's pair at plane z+1 (2.5 words per point and pass with the store); no LDS
//   relax_op_zero3d_xs_kernel<real, CoefOp>        the first red pass on a level that counts as zero: f and a in, red out, v not read
//   residual_op3d_xs_kernel<real, CoefOp, 1, LAP>  r and / or the partials of <r, r>; with LAP: q = A p and the partials of <p, q>
#include "mgx_ops3d.hpp"

#define MGX_COEF3D_API(SFX, real)                                                                                                            \
    extern "C" int mgx3dxs_relax_coef_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const int n[3], const real h[3], real s,    \
                                            int ncycles) {                                                                                   \
        return mgx::relax_op3d<mgx::CoefOp<real>, real>(ctx, v, f, a, n, h, s, ncycles, 0, 0, "relax_coef");                                 \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_relax_coef_from_zero_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const int n[3], const real h[3],  \
                                                      real s, int ncycles, int rim_is_zero) {                                                \
        return mgx::relax_op3d<mgx::CoefOp<real>, real>(ctx, v, f, a, n, h, s, ncycles, 1, rim_is_zero, "relax_coef_from_zero");             \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_residual_coef_##SFX(mgx_ctx* ctx, const real* v, const real* f, const real* a, real* r, const int n[3],           \
                                               const real h[3], real s, double* dev_work, double* dev_sumsq) {                               \
        return mgx::residual_op3d<mgx::CoefOp<real>, real>(ctx, v, f, a, r, n, h, s, dev_work, dev_sumsq, "residual_coef");                  \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_apply_coef_dot_##SFX(mgx_ctx* ctx, const real* p, const real* a, real* q, const int n[3], const real h[3],        \
                                                real s, double* dev_work, double* dev_sum) {                                                 \
        return mgx::apply_op_dot3d<mgx::CoefOp<real>, real>(ctx, p, a, q, n, h, s, dev_work, dev_sum, "apply_coef_dot");                     \
    }

MGX_COEF3D_API(f32, float)
MGX_COEF3D_API(f64, double)
