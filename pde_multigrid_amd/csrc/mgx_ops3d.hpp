// mgx_ops3d.hpp -- the operator policies of mgx_stencil3d.hpp that more than one file instantiates: ShiftOp, (Laplacian - s) u = f
// (its arithmetic is described in mgx_shift3d.hip), CoefOp, div(a grad u) - s u = f (mgx_coef3d.hip,
// section 14), and CapOp, div(a grad u) - (s c) u = f with a capacity c at every node (mgx_cap3d.hip, section 17).
// mgx_shift3d.hip and mgx_coef3d.hip build the interior kernels from the first two, mgx_cap3d.hip those of CapOp, mgx_wall3d.hip
// the kernels of the face unknowns (Neumann faces, section 15, and the walls of section 18) from all three: the point expressions
// exist once.  A policy's relax_wall / residual_wall take the zeroth-order coefficient of the point, se, as an argument; CoefOp's and
// CapOp's relax / residual are these with se = s or s * c_P, ShiftOp's relax keeps its own form with the level's denominator.
// HarmOp and HarmCapOp (mgx_hmean3d.hip, section 19) are CoefOp and CapOp with harmonic-mean face coefficients.
#pragma once
#include "mgx_stencil3d.hpp"

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

// den and, for fp32's route, rd = 1 / den in double are the same for every point of a level
template <class real>
struct ShiftOp {
    static constexpr bool HAS_A = false, HAS_S = true, HAS_C = false;
    static constexpr const char *relax_kernel = "relax_shift3d_xs_kernel", *zero_kernel = "relax_shift_zero3d_xs_kernel";
    real hx2, hy2, hz2, den;  // the smoother's
    double rd;
    real qx, qy, qz, s;  // the residual's: residual_scale's, MODE 1, or 3 with exact reciprocals
    int mode;
    ShiftOp(const mgx_ctx* ctx, const real h[3], real s_) : s(s_) {
        const ResidualScale<real> sc = residual_scale<real>(ctx, h, MGX_RESIDUAL_CORRECT);
        hx2 = sc.hx2, hy2 = sc.hy2, hz2 = sc.hz2;
        den = 2 * (hy2 * hz2 + hx2 * hz2 + hx2 * hy2) + s * hx2 * hy2 * hz2;
        rd = sizeof(real) == 4 ? 1.0 / (double)den : 0.0;
        qx = sc.qx, qy = sc.qy, qz = sc.qz, mode = sc.mode;
    }
    static int rows(const mgx_ctx*) { return 4; }  // ("relax3d.rows" is not read)
    template <class F>
    static void with_mode(int mode, F&& f) {
        with_value<1, 3>(mode, f);
    }
    __device__ __forceinline__ real relax(const Star7<real>& v, real f, const Star7<real>&) const {
        return relax_shift3d_point<real>(v.O, v.E, v.N, v.S, v.D, v.U, f, hx2, hy2, hz2, den, rd);
    }
    template <int MODE>
    __device__ __forceinline__ real residual(const Star7<real>& v, real f, const Star7<real>&) const {
        return residual3d_point<real, MODE>(v.O, v.E, v.N, v.S, v.D, v.U, v.C, f, qx, qy, qz) + s * v.C;
    }
    // a wall face (mgx_wall3d.hip) adds d to the zeroth-order term of a face unknown: the effective shift se and
    // the point expressions with it -- the smoother a plain division in `real` in both precisions
    __device__ __forceinline__ real wall_shift(real d, real) const { return s + d; }
    __device__ __forceinline__ real relax_wall(const Star7<real>& v, real f, const Star7<real>&, real se) const {
        const real num = v.O * (hy2 * hz2) + v.E * (hy2 * hz2) + v.N * (hx2 * hz2) + v.S * (hx2 * hz2) + v.D * (hx2 * hy2) + v.U * (hx2 * hy2) -
                         f * hx2 * hy2 * hz2;
        const real denP = 2 * (hy2 * hz2 + hx2 * hz2 + hx2 * hy2) + se * hx2 * hy2 * hz2;
        return num / denP;
    }
    template <int MODE>
    __device__ __forceinline__ real residual_wall(const Star7<real>& v, real f, const Star7<real>&, real se) const {
        return residual3d_point<real, MODE>(v.O, v.E, v.N, v.S, v.D, v.U, v.C, f, qx, qy, qz) + se * v.C;
    }
};

// the point expressions of the conservative 7-point form from its six (doubled) face coefficients AW .. AU on
template <class real>
__device__ __forceinline__ real relax_faces3d_point(real O, real E, real N, real S, real D, real U, real f, real AW, real AE, real AN, real AS,
                                                    real AD, real AU, real qx, real qy, real qz, real s) {
    const real den = ((qx * (AW + AE) + qy * (AN + AS)) + qz * (AD + AU)) + s;
    const real num = ((qx * (AW * O + AE * E) + qy * (AN * N + AS * S)) + qz * (AD * D + AU * U)) - f;
    return num / den;
}

template <class real>
__device__ __forceinline__ real residual_faces3d_point(real O, real E, real N, real S, real D, real U, real c, real f, real AW, real AE, real AN,
                                                       real AS, real AD, real AU, real qx, real qy, real qz, real s) {
    const real tx = qx * (AW * (O - c) + AE * (E - c));
    const real ty = qy * (AN * (N - c) + AS * (S - c));
    const real tz = qz * (AD * (D - c) + AU * (U - c));
    return (((f - tx) - ty) - tz) + s * c;
}

template <class real>
__device__ __forceinline__ real relax_coef3d_point(real O, real E, real N, real S, real D, real U, real f, real aO, real aE, real aN, real aS,
                                                   real aD, real aU, real aC, real qx, real qy, real qz, real s) {
    const real AW = aO + aC, AE = aE + aC, AN = aN + aC, AS = aS + aC, AD = aD + aC, AU = aU + aC;
    return relax_faces3d_point<real>(O, E, N, S, D, U, f, AW, AE, AN, AS, AD, AU, qx, qy, qz, s);
}

template <class real>
__device__ __forceinline__ real residual_coef3d_point(real O, real E, real N, real S, real D, real U, real c, real f, real aO, real aE, real aN,
                                                      real aS, real aD, real aU, real aC, real qx, real qy, real qz, real s) {
    const real AW = aO + aC, AE = aE + aC, AN = aN + aC, AS = aS + aC, AD = aD + aC, AU = aU + aC;
    return residual_faces3d_point<real>(O, E, N, S, D, U, c, f, AW, AE, AN, AS, AD, AU, qx, qy, qz, s);
}

// qx = (real)0.5 / hx2 .. : half the reciprocal squared spacings (the 1/2 of the face means)
template <class real>
struct CoefOp {
    static constexpr bool HAS_A = true, HAS_S = true, HAS_C = false;
    static constexpr const char *relax_kernel = "relax_coef3d_xs_kernel", *zero_kernel = "relax_coef_zero3d_xs_kernel";
    static constexpr int mode = 1;  // (the expressions divide by nothing the host could invert: one MODE)
    real qx, qy, qz, s;
    CoefOp(const mgx_ctx*, const real h[3], real s_) : s(s_) {
        const real hx2 = h[0] * h[0], hy2 = h[1] * h[1], hz2 = h[2] * h[2];
        qx = (real)0.5 / hx2;
        qy = (real)0.5 / hy2;
        qz = (real)0.5 / hz2;
    }
    // "relax3d.rows" below 4 lowers the rows per lane (fp64 with four rows: 124 VGPRs, four waves per SIMD; with two: 74, six)
    static int rows(const mgx_ctx* ctx) { return ctx->relax_rows < 4 ? ctx->relax_rows : 4; }
    template <class F>
    static void with_mode(int, F&& f) {
        f(std::integral_constant<int, 1>());
    }
    __device__ __forceinline__ real relax(const Star7<real>& v, real f, const Star7<real>& a) const { return relax_wall(v, f, a, s); }
    template <int MODE>
    __device__ __forceinline__ real residual(const Star7<real>& v, real f, const Star7<real>& a) const {
        return residual_wall<MODE>(v, f, a, s);
    }
    // the point expressions with se where they take s; at a wall face (section 18) the effective shift se = s + d
    __device__ __forceinline__ real wall_shift(real d, real) const { return s + d; }
    __device__ __forceinline__ real relax_wall(const Star7<real>& v, real f, const Star7<real>& a, real se) const {
        return relax_coef3d_point<real>(v.O, v.E, v.N, v.S, v.D, v.U, f, a.O, a.E, a.N, a.S, a.D, a.U, a.C, qx, qy, qz, se);
    }
    template <int MODE>
    __device__ __forceinline__ real residual_wall(const Star7<real>& v, real f, const Star7<real>& a, real se) const {
        return residual_coef3d_point<real>(v.O, v.E, v.N, v.S, v.D, v.U, v.C, f, a.O, a.E, a.N, a.S, a.D, a.U, a.C, qx, qy, qz, se);
    }
};

// div(a grad u) - (s c) u = f: CoefOp's expressions with sc = s * c_P, one rounding in `real`, where they take s.  c is the
// capacity at the updated point only (f's index), read through the policy: the kernels of the other policies take no further
// argument.  c == 1 gives CoefOp's bits (s * 1 = s).
template <class real>
struct CapOp {
    static constexpr bool HAS_A = true, HAS_S = true, HAS_C = true;
    static constexpr const char *relax_kernel = "relax_cap3d_xs_kernel", *zero_kernel = "relax_cap_zero3d_xs_kernel";
    static constexpr int mode = 1;
    real qx, qy, qz, s;
    const real* c;  // the level's capacity array (never written)
    CapOp(const mgx_ctx*, const real h[3], real s_, const real* c_) : s(s_), c(c_) {
        const real hx2 = h[0] * h[0], hy2 = h[1] * h[1], hz2 = h[2] * h[2];
        qx = (real)0.5 / hx2;
        qy = (real)0.5 / hy2;
        qz = (real)0.5 / hz2;
    }
    // "relax3d.rows" below 4 lowers the rows per lane, as for CoefOp.  fp64 with four rows: 132 VGPRs, three waves per SIMD, 638 us
    // per colour pass at 513^3; with two: 78, six waves, 658 us -- four stays the default
    static int rows(const mgx_ctx* ctx) { return ctx->relax_rows < 4 ? ctx->relax_rows : 4; }
    template <class F>
    static void with_mode(int, F&& f) {
        f(std::integral_constant<int, 1>());
    }
    __device__ __forceinline__ real relax(const Star7<real>& v, real f, const Star7<real>& a, real cP) const {
        return relax_wall(v, f, a, s * cP);
    }
    template <int MODE>
    __device__ __forceinline__ real residual(const Star7<real>& v, real f, const Star7<real>& a, real cP) const {
        return residual_wall<MODE>(v, f, a, s * cP);
    }
    // CoefOp's point expressions with se where they take s; at a wall face (section 18) the effective shift se = s * c_P + d
    __device__ __forceinline__ real wall_shift(real d, real cP) const { return s * cP + d; }
    __device__ __forceinline__ real relax_wall(const Star7<real>& v, real f, const Star7<real>& a, real se) const {
        return relax_coef3d_point<real>(v.O, v.E, v.N, v.S, v.D, v.U, f, a.O, a.E, a.N, a.S, a.D, a.U, a.C, qx, qy, qz, se);
    }
    template <int MODE>
    __device__ __forceinline__ real residual_wall(const Star7<real>& v, real f, const Star7<real>& a, real se) const {
        return residual_coef3d_point<real>(v.O, v.E, v.N, v.S, v.D, v.U, v.C, f, a.O, a.E, a.N, a.S, a.D, a.U, a.C, qx, qy, qz, se);
    }
};

// ------------------------------------------------------------------ harmonic-mean faces (mgx_hmean3d.hip)
// CoefOp's / CapOp's operators for a coefficient that belongs to the nodes (voxel data): the material interface lies midway between
// two nodes and the face carries the series conductance 2 aP aQ / (aP + aQ).  The one difference is the doubled face coefficient,
//   AW = (real)4 * ((aO * aC) / (aO + aC))   (likewise AE .. AU)   for   AW = aO + aC,
// a plain IEEE division in `real` in both precisions; everything after it is relax_faces3d_point / residual_faces3d_point, the
// expressions relax_coef3d_point / residual_coef3d_point continue with.  Product and sum commute, so a face has the same bits
// seen from either of its nodes: the operator is symmetric bit for bit.  Where the two values are the same power of two the
// doubled mean is exactly aO + aC and the results have the arithmetic operator's bits (a == 1: 4 * (1 / 2) = 2).  The host keeps
// a * a normal and finite.
template <class real>
__device__ __forceinline__ real hmean_face(real aQ, real aC) {
    return (real)4 * ((aQ * aC) / (aQ + aC));
}

template <class real>
__device__ __forceinline__ real relax_hmean3d_point(real O, real E, real N, real S, real D, real U, real f, real aO, real aE, real aN, real aS,
                                                    real aD, real aU, real aC, real qx, real qy, real qz, real s) {
    return relax_faces3d_point<real>(O, E, N, S, D, U, f, hmean_face(aO, aC), hmean_face(aE, aC), hmean_face(aN, aC), hmean_face(aS, aC),
                                     hmean_face(aD, aC), hmean_face(aU, aC), qx, qy, qz, s);
}

template <class real>
__device__ __forceinline__ real residual_hmean3d_point(real O, real E, real N, real S, real D, real U, real c, real f, real aO, real aE, real aN,
                                                       real aS, real aD, real aU, real aC, real qx, real qy, real qz, real s) {
    return residual_faces3d_point<real>(O, E, N, S, D, U, c, f, hmean_face(aO, aC), hmean_face(aE, aC), hmean_face(aN, aC), hmean_face(aS, aC),
                                        hmean_face(aD, aC), hmean_face(aU, aC), qx, qy, qz, s);
}

// CoefOp with harmonic faces: its scalars, its flags and its MODE; the point expressions and the kernels' names are its own
template <class real>
struct HarmOp : CoefOp<real> {
    static constexpr const char *relax_kernel = "relax_hmean3d_xs_kernel", *zero_kernel = "relax_hmean_zero3d_xs_kernel";
    using CoefOp<real>::CoefOp;
    __device__ __forceinline__ real relax(const Star7<real>& v, real f, const Star7<real>& a) const { return relax_wall(v, f, a, this->s); }
    template <int MODE>
    __device__ __forceinline__ real residual(const Star7<real>& v, real f, const Star7<real>& a) const {
        return residual_wall<MODE>(v, f, a, this->s);
    }
    __device__ __forceinline__ real relax_wall(const Star7<real>& v, real f, const Star7<real>& a, real se) const {
        return relax_hmean3d_point<real>(v.O, v.E, v.N, v.S, v.D, v.U, f, a.O, a.E, a.N, a.S, a.D, a.U, a.C, this->qx, this->qy, this->qz, se);
    }
    template <int MODE>
    __device__ __forceinline__ real residual_wall(const Star7<real>& v, real f, const Star7<real>& a, real se) const {
        return residual_hmean3d_point<real>(v.O, v.E, v.N, v.S, v.D, v.U, v.C, f, a.O, a.E, a.N, a.S, a.D, a.U, a.C, this->qx, this->qy,
                                            this->qz, se);
    }
};

// CapOp with harmonic faces
template <class real>
struct HarmCapOp : CapOp<real> {
    static constexpr const char *relax_kernel = "relax_hmean_cap3d_xs_kernel", *zero_kernel = "relax_hmean_cap_zero3d_xs_kernel";
    using CapOp<real>::CapOp;
    __device__ __forceinline__ real relax(const Star7<real>& v, real f, const Star7<real>& a, real cP) const {
        return relax_wall(v, f, a, this->s * cP);
    }
    template <int MODE>
    __device__ __forceinline__ real residual(const Star7<real>& v, real f, const Star7<real>& a, real cP) const {
        return residual_wall<MODE>(v, f, a, this->s * cP);
    }
    __device__ __forceinline__ real relax_wall(const Star7<real>& v, real f, const Star7<real>& a, real se) const {
        return relax_hmean3d_point<real>(v.O, v.E, v.N, v.S, v.D, v.U, f, a.O, a.E, a.N, a.S, a.D, a.U, a.C, this->qx, this->qy, this->qz, se);
    }
    template <int MODE>
    __device__ __forceinline__ real residual_wall(const Star7<real>& v, real f, const Star7<real>& a, real se) const {
        return residual_hmean3d_point<real>(v.O, v.E, v.N, v.S, v.D, v.U, v.C, f, a.O, a.E, a.N, a.S, a.D, a.U, a.C, this->qx, this->qy,
                                            this->qz, se);
    }
};

}  // namespace mgx
