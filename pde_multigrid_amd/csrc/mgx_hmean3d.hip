// mgx_hmean3d.hip -- the operators of div(a grad u) - s u = f and div(a grad u) - (s c) u = f with HARMONIC-MEAN face
// coefficients, x-split layout: the discretisation for a coefficient that belongs to the nodes (voxel data, a CT scan, a layer one
// node thick), where the material interface lies midway between two nodes and the face carries the series conductance
// 2 aP aQ / (aP + aQ).  DESIGN.md section 19.
//
// The arithmetic is mgx_coef3d.hip's / mgx_cap3d.hip's (restated in tests/op_restated.py) with ONE difference, in `real`:
//   AW = (real)4 * ((aO * aC) / (aO + aC))   (likewise AE .. AU)   where those form   AW = aO + aC
// the doubled harmonic mean, a plain IEEE division in both precisions; q* = (real)0.5 / h*^2, den, num, tx, ty, tz and the se forms
// of the walls are unchanged and in the same association.  Product and sum commute: a face has the same bits seen from either of
// its nodes and the operator is symmetric bit for bit.  Where both values are the same power of two the doubled mean is aO + aC
// exactly: a constant coefficient 2^k gives the bits of the arithmetic operator.  The entries check nothing about a's range; the
// host layer (set_coefficient / set_face_mean) keeps a * a normal and finite.
//
// The policies, HarmOp and HarmCapOp, are in mgx_ops3d.hpp; the kernels and their host drivers are the shared ones of
// mgx_stencil3d.hpp, instantiated with the policies in this unit only (the drivers of mgx_rim3d.hpp reach the kernels of the face
// unknowns, which mgx_wall3d.hip instantiates for both, through that unit's launch functions):
//   relax_op3d_xs_kernel<real, Harm(Cap)Op, TYW, R>      one colour pass ("relax_hmean3d_xs_kernel" / "relax_hmean_cap3d_xs_kernel" to
//                                                        last_relax_kernel()): the data movement of the coefficient / capacity pass,
//                                                        2.5 / 3.0 words per point and pass, and six more divisions per update
//   relax_op_zero3d_xs_kernel<real, Harm(Cap)Op>         the first red pass on a level that counts as zero
//   residual_op3d_xs_kernel<real, Harm(Cap)Op, 1, LAP>   r and / or the partials of <r, r>; with LAP: q = A p and the partials of <p, q>
// One set of entries per precision, in the _wall form: bc = 0 is the interior form, all betas zero the _bc form; c == NULL means no
// capacity (HarmOp).
#include "mgx_rim3d.hpp"

#define MGX_HMEAN3D_API(SFX, real)                                                                                                           \
    extern "C" int mgx3dxs_relax_hmean_wall_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const real* c, const int n[3],        \
                                                  const real h[3], real s, int ncycles, int bc, const real beta[6]) {                        \
        if (c) return mgx::relax_op3d_bc<mgx::HarmCapOp<real>, real>(ctx, v, f, a, n, h, s, ncycles, bc, beta, "relax_hmean_wall", c);       \
        return mgx::relax_op3d_bc<mgx::HarmOp<real>, real>(ctx, v, f, a, n, h, s, ncycles, bc, beta, "relax_hmean_wall");                    \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_relax_hmean_pin_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const real* c, const int n[3], const real h[3], real s, int ncycles, int bc, const real beta[6], const unsigned* idx, \
            const unsigned end[2], const real* val) {                                                                                        \
        MGX_REQUIRE(end, MGX_ERR_INVALID, "relax_hmean_pin: NULL argument");                                                                 \
        const mgx::PinList<real> pin = {idx, {end[0], end[1]}, val};                                                                         \
        if (c) return mgx::relax_op3d_bc<mgx::HarmCapOp<real>, real>(ctx, v, f, a, n, h, s, ncycles, bc, beta, "relax_hmean_pin", c, &pin);  \
        return mgx::relax_op3d_bc<mgx::HarmOp<real>, real>(ctx, v, f, a, n, h, s, ncycles, bc, beta, "relax_hmean_pin", nullptr, &pin);      \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_relax_hmean_from_zero_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const real* c, const int n[3],   \
                                                       const real h[3], real s, int ncycles, int rim_is_zero) {                              \
        if (c) return mgx::relax_op3d<mgx::HarmCapOp<real>, real>(ctx, v, f, a, n, h, s, ncycles, 1, rim_is_zero, "relax_hmean_from_zero", c); \
        return mgx::relax_op3d<mgx::HarmOp<real>, real>(ctx, v, f, a, n, h, s, ncycles, 1, rim_is_zero, "relax_hmean_from_zero");            \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_residual_hmean_wall_##SFX(mgx_ctx* ctx, const real* v, const real* f, const real* a, const real* c, real* r,      \
                                                     const int n[3], const real h[3], real s, double* dev_work, double* dev_sumsq, int bc,   \
                                                     const real beta[6]) {                                                                   \
        if (c)                                                                                                                               \
            return mgx::residual_op3d_bc<mgx::HarmCapOp<real>, real>(ctx, v, f, a, r, n, h, s, dev_work, dev_sumsq, bc, beta,                \
                                                                     "residual_hmean_wall", c);                                              \
        return mgx::residual_op3d_bc<mgx::HarmOp<real>, real>(ctx, v, f, a, r, n, h, s, dev_work, dev_sumsq, bc, beta, "residual_hmean_wall"); \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_apply_hmean_dot_wall_##SFX(mgx_ctx* ctx, const real* p, const real* a, const real* c, real* q, const int n[3],    \
                                                      const real h[3], real s, double* dev_work, double* dev_sum, int bc,                    \
                                                      const real beta[6]) {                                                                  \
        if (c)                                                                                                                               \
            return mgx::apply_op_dot3d_bc<mgx::HarmCapOp<real>, real>(ctx, p, a, q, n, h, s, dev_work, dev_sum, bc, beta,                    \
                                                                      "apply_hmean_dot_wall", c);                                            \
        return mgx::apply_op_dot3d_bc<mgx::HarmOp<real>, real>(ctx, p, a, q, n, h, s, dev_work, dev_sum, bc, beta, "apply_hmean_dot_wall"); \
    }

MGX_HMEAN3D_API(f32, float)
MGX_HMEAN3D_API(f64, double)
