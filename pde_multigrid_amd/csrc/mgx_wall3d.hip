// mgx_wall3d.hip -- the operators on the FACE UNKNOWNS: homogeneous Neumann faces and CONVECTIVE (Robin) and
// PRESCRIBED-FLUX walls (section 18) for the shifted, the variable-coefficient and the capacity operator, x-split layout.
//
// At an unknown on a face of the mask every operator is the interior's point expression on a star whose out-of-range entry is
// replaced by the opposite one (mgx_rim3d.hip describes the list of face points and the launch).  On such a face the wall law is  a du/dn + beta u = g  (n outward, beta >= 0, both constants per face, in
// the units of the hierarchy's operator div(a grad u)).  The mirrored star of section 15 is the flux through the inner half-face of
// the half cell at a face unknown; the wall adds 2 (g - beta u_P) / h per wall face the point lies on, h the spacing along that
// face's axis.  So the operator gains a DIAGONAL term at the face unknowns and nothing else changes:
//   d_k  = ((real)2 * beta_k) / h_axis(k)     once per call, on the host, from the level's own spacings (mgx_rim3d.hpp)
//   d(P) = the sum, in the order x, y, z, of the d_k of the faces P lies on (the d_k of a face whose bit is clear is 0)
//   d(P) == 0: the interior's point expression, Op::relax / Op::residual -- every point of a call without a wall (all betas zero:
//              the homogeneous Neumann faces), which therefore has the bits of the mirrored star alone
//   d(P) != 0: the operator's own point expression with the effective shift se = s + d(P) (CapOp: s * c_P + d(P)) where it takes
//              s -- Op::relax_wall / Op::residual_wall of mgx_ops3d.hpp; the shifted smoother then divides in `real`
// g touches the right-hand side of level 0 only: f[P] -= ((real)2 * g_k) / h_axis(k), face by face in the order x, y, z
// (wall_rhs3d_xs_kernel).
//
// The three kernels -- colour pass, residual, apply + dot -- take an operator policy and the six d_k by value and are instantiated
// for ShiftOp, CoefOp, CapOp and their harmonic-mean forms HarmOp and HarmCapOp in this unit only: one instance per operator and
// precision serves the _bc and the _wall entries.  The host drivers are in mgx_rim3d.hpp and are instantiated, with the interior
// kernels, in mgx_rim3d.hip, mgx_cap3d.hip and mgx_hmean3d.hip: they
// reach the kernels through the launch functions at the end of this file.  No LDS beyond the partial sums' four doubles, no scratch.
#include "mgx_rim3d.hpp"

namespace mgx {

// d(P): x, then y, then z (a point lies on at most one face per axis; adding the 0 of an unflagged face is exact)
template <class real>
__device__ __forceinline__ real wall_diag(const WallD<real>& w, const Rim& R, int x, int y, int z) {
    real d = x == 0 ? w.d[0] : x == R.sx - 1 ? w.d[1] : (real)0;
    d = d + (y == 0 ? w.d[2] : y == R.sy - 1 ? w.d[3] : (real)0);
    d = d + (z == 0 ? w.d[4] : z == R.sz - 1 ? w.d[5] : (real)0);
    return d;
}

// one colour pass on the face unknowns
template <class real, class Op>
__global__ void __launch_bounds__(RIM_THREADS) face_relax3d_xs_kernel(real* __restrict__ v, const real* __restrict__ f, const real* __restrict__ a,
                                                                      Rim R, Op op, WallD<real> w, int colour) {
    const Geo<XSplit, real> g(R.sx, R.sy);
    RIM_FOR_EACH_POINT(R, g, x, y, z) {
        if (((x + y + z) & 1) != colour) continue;
        const size_t i = g.row(y, z) + g.pos(x);
        const Star7<real> vs = rim_star<real, false>(v, g, R, x, y, z);
        Star7<real> as = {};
        if constexpr (Op::HAS_A) as = rim_star<real, true>(a, g, R, x, y, z);
        real cP = (real)0;
        if constexpr (Op::HAS_C) cP = op.c[i];
        const real d = wall_diag<real>(w, R, x, y, z);
        if (d != (real)0) {
            v[i] = op.relax_wall(vs, f[i], as, op.wall_shift(d, cP));
        } else {
            if constexpr (Op::HAS_C) v[i] = op.relax(vs, f[i], as, cP);
            else v[i] = op.relax(vs, f[i], as);
        }
    }
}

// r on the face unknowns (out == NULL: not stored) and the block's partial of its squares (partial == NULL: none): per thread in
// list order, wavefront-wide shuffles, the four waves in a fixed order -- the same bits on every run
template <class real, class Op, int MODE>
__global__ void __launch_bounds__(RIM_THREADS) face_residual3d_xs_kernel(const real* __restrict__ v, const real* __restrict__ f,
                                                                         const real* __restrict__ a, real* __restrict__ out, Rim R, Op op,
                                                                         WallD<real> w, double* __restrict__ partial) {
    const Geo<XSplit, real> g(R.sx, R.sy);
    double acc = 0.0;
    RIM_FOR_EACH_POINT(R, g, x, y, z) {
        const size_t i = g.row(y, z) + g.pos(x);
        const Star7<real> vs = rim_star<real, true>(v, g, R, x, y, z);
        Star7<real> as = {};
        if constexpr (Op::HAS_A) as = rim_star<real, true>(a, g, R, x, y, z);
        real cP = (real)0;
        if constexpr (Op::HAS_C) cP = op.c[i];
        const real d = wall_diag<real>(w, R, x, y, z);
        real t;
        if (d != (real)0) t = op.template residual_wall<MODE>(vs, f[i], as, op.wall_shift(d, cP));
        else if constexpr (Op::HAS_C) t = op.template residual<MODE>(vs, f[i], as, cP);
        else t = op.template residual<MODE>(vs, f[i], as);
        if (out) out[i] = t;
        acc += (double)t * (double)t;
    }
    if (partial) {  // (uniform over the launch)
        __shared__ double part[RIM_THREADS / 64];
        rim_block_sum(acc, part, partial + blockIdx.x);
    }
}

// q = A p = -(the residual of (p, 0)) on the reflected star, partials of <p, q>_W
template <class real, class Op, int MODE>
__global__ void __launch_bounds__(RIM_THREADS) face_apply_dot3d_xs_kernel(const real* __restrict__ p, const real* __restrict__ a,
                                                                          real* __restrict__ q, Rim R, Op op, WallD<real> w,
                                                                          double* __restrict__ partial) {
    const Geo<XSplit, real> g(R.sx, R.sy);
    double acc = 0.0;
    RIM_FOR_EACH_POINT(R, g, x, y, z) {
        const Star7<real> vs = rim_star<real, true>(p, g, R, x, y, z);
        Star7<real> as = {};
        if constexpr (Op::HAS_A) as = rim_star<real, true>(a, g, R, x, y, z);
        const size_t i = g.row(y, z) + g.pos(x);
        real cP = (real)0;
        if constexpr (Op::HAS_C) cP = op.c[i];
        const real d = wall_diag<real>(w, R, x, y, z);
        real t;
        if (d != (real)0) t = -op.template residual_wall<MODE>(vs, (real)0, as, op.wall_shift(d, cP));
        else if constexpr (Op::HAS_C) t = -op.template residual<MODE>(vs, (real)0, as, cP);
        else t = -op.template residual<MODE>(vs, (real)0, as);  // negation is exact
        q[i] = t;
        acc += rim_weight(R, x, y, z) * ((double)vs.C * (double)t);
    }
    __shared__ double part[RIM_THREADS / 64];
    rim_block_sum(acc, part, partial + blockIdx.x);
}

// f -= gq_k on the face unknowns, gq_k = ((real)2 * g_k) / h_axis(k): successively for the faces the point lies on, x, y, z
template <class real>
__global__ void __launch_bounds__(RIM_THREADS) wall_rhs3d_xs_kernel(real* __restrict__ f, Rim R, WallD<real> gq) {
    const Geo<XSplit, real> g(R.sx, R.sy);
    RIM_FOR_EACH_POINT(R, g, x, y, z) {
        const size_t i = g.row(y, z) + g.pos(x);
        const real gx = x == 0 ? gq.d[0] : x == R.sx - 1 ? gq.d[1] : (real)0;
        const real gy = y == 0 ? gq.d[2] : y == R.sy - 1 ? gq.d[3] : (real)0;
        const real gz = z == 0 ? gq.d[4] : z == R.sz - 1 ? gq.d[5] : (real)0;
        real t = f[i];
        if (gx != (real)0) t = t - gx;
        if (gy != (real)0) t = t - gy;
        if (gz != (real)0) t = t - gz;
        if (gx != (real)0 || gy != (real)0 || gz != (real)0) f[i] = t;
    }
}

// =========================================================================== host side
template <class Op, class real>
void face_relax_launch(mgx_ctx* ctx, real* v, const real* f, const real* a, const Rim& R, const Op& op, const WallD<real>& w, int colour) {
    MGX_LAUNCH((face_relax3d_xs_kernel<real, Op>), dim3(rim_blocks(R)), dim3(RIM_THREADS), 0, ctx->compute, v, f, a, R, op, w, colour);
}

template <class Op, class real>
void face_residual_launch(mgx_ctx* ctx, const real* v, const real* f, const real* a, real* out, const Rim& R, const Op& op,
                          const WallD<real>& w, unsigned nb, double* partial) {
    Op::with_mode(op.mode, [&](auto m) __attribute__((always_inline)) {
        MGX_LAUNCH((face_residual3d_xs_kernel<real, Op, decltype(m)::value>), dim3(nb), dim3(RIM_THREADS), 0, ctx->compute, v, f, a, out, R, op,
                   w, partial);
    });
}

template <class Op, class real>
void face_apply_dot_launch(mgx_ctx* ctx, const real* p, const real* a, real* q, const Rim& R, const Op& op, const WallD<real>& w,
                           unsigned nb, double* partial) {
    Op::with_mode(op.mode, [&](auto m) __attribute__((always_inline)) {
        MGX_LAUNCH((face_apply_dot3d_xs_kernel<real, Op, decltype(m)::value>), dim3(nb), dim3(RIM_THREADS), 0, ctx->compute, p, a, q, R, op, w,
                   partial);
    });
}

#define MGX_WALL3D_LAUNCHERS(Op, real)                                                                                                    \
    template void face_relax_launch<Op<real>, real>(mgx_ctx*, real*, const real*, const real*, const Rim&, const Op<real>&,               \
                                                    const WallD<real>&, int);                                                             \
    template void face_residual_launch<Op<real>, real>(mgx_ctx*, const real*, const real*, const real*, real*, const Rim&, const Op<real>&, \
                                                       const WallD<real>&, unsigned, double*);                                            \
    template void face_apply_dot_launch<Op<real>, real>(mgx_ctx*, const real*, const real*, real*, const Rim&, const Op<real>&,            \
                                                        const WallD<real>&, unsigned, double*);
MGX_WALL3D_LAUNCHERS(ShiftOp, float)
MGX_WALL3D_LAUNCHERS(ShiftOp, double)
MGX_WALL3D_LAUNCHERS(CoefOp, float)
MGX_WALL3D_LAUNCHERS(CoefOp, double)
MGX_WALL3D_LAUNCHERS(CapOp, float)
MGX_WALL3D_LAUNCHERS(CapOp, double)
MGX_WALL3D_LAUNCHERS(HarmOp, float)  // harmonic-mean faces (section 19): the drivers are instantiated in mgx_hmean3d.hip
MGX_WALL3D_LAUNCHERS(HarmOp, double)
MGX_WALL3D_LAUNCHERS(HarmCapOp, float)
MGX_WALL3D_LAUNCHERS(HarmCapOp, double)

// f -= 2 g / h on the face unknowns of the mask's faces with g_k != 0; all g zero: nothing is launched
template <class real>
static int wall_rhs3d(mgx_ctx* ctx, real* f, const int n[3], const real h[3], const real g[6], int bc) {
    MGX_REQUIRE(ctx && f && n && h && g, MGX_ERR_INVALID, "wall_rhs: NULL argument");
    RIM_BC_CHECK(bc, "wall_rhs");
    bool any;
    MGX_TRY_RET(wall_data_check<real>(g, h, bc, true, "wall_rhs", &any));
    MGX_TRY_RET(rows_check(n, "wall_rhs", nullptr, false));
    MGX_REQUIRE((double)n[0] * n[1] * n[2] < 2147483647.0 * 4, MGX_ERR_SIZE, "wall_rhs: grid too large");
    for (int d = 0; d < 3; d++)
        MGX_REQUIRE(std::isfinite((double)h[d]) && h[d] > 0, MGX_ERR_INVALID, "wall_rhs: the spacing h[%d] = %g is not finite and > 0", d,
                    (double)h[d]);
    if (!any) return MGX_OK;
    MGX_USE(ctx);
    Rim R;
    MGX_TRY_RET(rim_list<real>(n, bc, "wall_rhs", R));
    MGX_LAUNCH((wall_rhs3d_xs_kernel<real>), dim3(rim_blocks(R)), dim3(RIM_THREADS), 0, ctx->compute, f, R, wall_diagonal<real>(g, h));
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

}  // namespace mgx

#define MGX_WALL3D_API(SFX, real)                                                                                                   \
    extern "C" int mgx3dxs_wall_rhs_##SFX(mgx_ctx* ctx, real* f, const int n[3], const real h[3], const real g[6], int bc) {        \
        return mgx::wall_rhs3d<real>(ctx, f, n, h, g, bc);                                                                          \
    }

MGX_WALL3D_API(f32, float)
MGX_WALL3D_API(f64, double)
