// mgx_rim3d.hpp -- what the units that work on the face unknowns share (mgx_rim3d.hip, mgx_wall3d.hip, mgx_cap3d.hip; DESIGN.md
// sections 15 and 18): the list of face points, the reflected star, the weight and the block sum of the solve's inner product, the
// wall data, and the host drivers of the operator entries with a mask.  A driver launches the interior kernels of the unit that
// instantiates it (mgx_rim3d.hip for ShiftOp and CoefOp, mgx_cap3d.hip for CapOp, mgx_hmean3d.hip for HarmOp and HarmCapOp) and the face kernels of mgx_wall3d.hip, their one
// home, through that unit's launch functions; a homogeneous Neumann face is a wall with beta = 0.  The transfers and the vector
// kernels of the solve are in mgx_rim3d.hip.
#pragma once
#include "mgx_ops3d.hpp"

namespace mgx {

typedef unsigned long long u64;

// the list of face points of a grid: the faces in the order z-low, z-high, y-low, y-high, x-low, x-high, end[k] = the number of
// listed points of the faces 0 .. k (a face whose bit is clear lists none)
// -- in 32 bits, so that a thread finds its point with 32-bit divisions: a grid whose list is longer is MGX_ERR_SIZE
struct Rim {
    int sx, sy, sz, bc;
    unsigned end[6];
};

template <class real>
static int rim_list(const int n[3], int bc, const char* what, Rim& r) {
    r.sx = n[0], r.sy = n[1], r.sz = n[2], r.bc = bc;
    const u64 P = (u64)Geo<XSplit, real>(n[0], n[1]).P;
    const u64 cnt[6] = {P * (u64)n[1], P * (u64)n[1], P * (u64)(n[2] - 2), P * (u64)(n[2] - 2), (u64)(n[1] - 2) * (u64)(n[2] - 2),
                        (u64)(n[1] - 2) * (u64)(n[2] - 2)};
    const int bit[6] = {4, 5, 2, 3, 0, 1};
    u64 acc = 0;
    for (int k = 0; k < 6; k++) {
        if ((bc >> bit[k]) & 1) acc += cnt[k];
        MGX_REQUIRE(acc < 0xffffffffull, MGX_ERR_SIZE, "%s: %llu face points are too many", what, acc);
        r.end[k] = (unsigned)acc;
    }
    return MGX_OK;
}

constexpr int RIM_THREADS = 256;
constexpr int RIM_MAX_BLOCKS = 4096;
static unsigned rim_blocks(const Rim& r) {
    const u64 b = ((u64)r.end[5] + RIM_THREADS - 1) / RIM_THREADS;
    return (unsigned)(b < 1 ? 1 : b > RIM_MAX_BLOCKS ? RIM_MAX_BLOCKS : b);
}

// i reflected into [0, n) for -1 <= i <= n
__device__ __forceinline__ int rim_reflect(int i, int n) { return i < 0 ? -i : i >= n ? 2 * (n - 1) - i : i; }

// point t of the list: its coordinates; false for a pad position and for a point that is no unknown
template <class real>
__device__ __forceinline__ bool rim_point(const Rim& R, const Geo<XSplit, real>& g, unsigned t, int& x, int& y, int& z) {
    int k = 0;
    while (k < 5 && t >= R.end[k]) k++;
    const unsigned u = t - (k ? R.end[k - 1] : 0);
    if (k < 4) {  // whole rows: storage position j of row u / P
        const unsigned row = u / (unsigned)g.P;
        x = xs_x((int)(u - row * (unsigned)g.P), g.H);
        if (x >= R.sx) return false;
        if (k < 2) y = (int)row, z = k == 0 ? 0 : R.sz - 1;
        else y = k == 2 ? 0 : R.sy - 1, z = 1 + (int)row;
    } else {
        const unsigned q = u / (unsigned)(R.sy - 2);
        x = k == 4 ? 0 : R.sx - 1, y = 1 + (int)(u - q * (unsigned)(R.sy - 2)), z = 1 + (int)q;
    }
    const int on = (x == 0) | (x == R.sx - 1) << 1 | (y == 0) << 2 | (y == R.sy - 1) << 3 | (z == 0) << 4 | (z == R.sz - 1) << 5;
    return (on & ~R.bc) == 0;
}

// the reflected star of p around (x, y, z) (C: the centre too)
template <class real, bool C>
__device__ __forceinline__ Star7<real> rim_star(const real* __restrict__ p, const Geo<XSplit, real>& g, const Rim& R, int x, int y, int z) {
    const int xm = rim_reflect(x - 1, R.sx), xp = rim_reflect(x + 1, R.sx);
    const int ym = rim_reflect(y - 1, R.sy), yp = rim_reflect(y + 1, R.sy);
    const int zm = rim_reflect(z - 1, R.sz), zp = rim_reflect(z + 1, R.sz);
    const size_t row = g.row(y, z);
    const int j = g.pos(x);
    Star7<real> s;
    s.O = p[row + g.pos(xm)];
    s.E = p[row + g.pos(xp)];
    s.N = p[g.row(ym, z) + j];
    s.S = p[g.row(yp, z) + j];
    s.D = p[g.row(y, zm) + j];
    s.U = p[g.row(y, zp) + j];
    s.C = C ? p[row + j] : (real)0;
    return s;
}

#define RIM_FOR_EACH_POINT(R, g, x, y, z)                                                                                  \
    for (u64 t_ = (u64)blockIdx.x * RIM_THREADS + threadIdx.x; t_ < (R).end[5]; t_ += (u64)gridDim.x * RIM_THREADS)        \
        if (int x, y, z; rim_point<real>(R, g, (unsigned)t_, x, y, z))

// ------------------------------------------------------------------ the operator of the solve on the face unknowns (section 16)
// The flexible CG of a hierarchy with a mask works in the inner product <a, b>_W = sum of W a b over all unknowns, W = 1/2 per
// Neumann face an unknown lies on (the trapezoid weights A is symmetric in), 1 in the interior: the interior kernels of
// mgx_krylov3d.hip run unchanged and the kernels here add the face unknowns' terms, their block partials behind the interior
// launch's (the vector kernels: mgx_rim3d.hip).  W is a power of two: a weighted term is the unweighted one, rescaled exactly.
__device__ __forceinline__ double rim_weight(const Rim& R, int x, int y, int z) {
    const int faces = (x == 0 || x == R.sx - 1) + (y == 0 || y == R.sy - 1) + (z == 0 || z == R.sz - 1);
    return faces == 1 ? 0.5 : faces == 2 ? 0.25 : 0.125;
}

// the block's sum of acc into *partial: per thread in list order, wavefront-wide shuffles, the four waves in a fixed order
__device__ __forceinline__ void rim_block_sum(double acc, double* part, double* __restrict__ partial) {
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) *partial = (part[0] + part[1]) + (part[2] + part[3]);
}

// =========================================================================== host side
#define RIM_BC_CHECK(bc, what) MGX_REQUIRE((bc) >= 0 && (bc) <= 63, MGX_ERR_INVALID, "%s: bc = %d is outside 0 .. 63", what, bc)

// ------------------------------------------------------------------ convective and prescribed-flux walls (section 18)
// On a face of the mask the wall law a du/dn + beta u = g adds 2 (g - beta u_P) / h to the half cell's balance: the operator gains
// the diagonal d_k = ((real)2 * beta_k) / h_axis(k) at the face unknowns, formed here once per call from the level's own spacings.
// The face kernels (mgx_wall3d.hip, their one home) take the six d_k by value; a homogeneous Neumann face is the wall with
// beta = 0, where they compute the plain point expression.  beta in the order of the mask's bits.
template <class real>
struct WallD {
    real d[6];
};

// the betas of a call without a wall (the _bc entries)
template <class real>
static const real NO_WALL[6] = {0, 0, 0, 0, 0, 0};

// the launches over the face unknowns, defined and instantiated for every policy of mgx_ops3d.hpp in mgx_wall3d.hip
template <class Op, class real>
void face_relax_launch(mgx_ctx* ctx, real* v, const real* f, const real* a, const Rim& R, const Op& op, const WallD<real>& w, int colour);
template <class Op, class real>
void face_residual_launch(mgx_ctx* ctx, const real* v, const real* f, const real* a, real* out, const Rim& R, const Op& op,
                          const WallD<real>& w, unsigned nb, double* partial);
template <class Op, class real>
void face_apply_dot_launch(mgx_ctx* ctx, const real* p, const real* a, real* q, const Rim& R, const Op& op, const WallD<real>& w,
                           unsigned nb, double* partial);

// the wall data of a call against its mask: v[k] finite, >= 0 unless `flux`, 0 on a face whose bit is clear, and small enough for
// the term ((real)2 * v[k]) / h_axis(k) the kernels work with to be finite in `real` (fp32: a beta near FLT_MAX, or a large one on a
// fine level, would make it inf and the results NaN); *any = some v[k] != 0 (any == NULL: not asked)
template <class real>
static int wall_data_check(const real v[6], const real h[3], int bc, bool flux, const char* what, bool* any = nullptr) {
    if (any) *any = false;
    for (int k = 0; k < 6; k++) {
        MGX_REQUIRE(std::isfinite((double)v[k]) && (flux || v[k] >= 0), MGX_ERR_INVALID, "%s: %s[%d] = %g is not finite%s", what,
                    flux ? "g" : "beta", k, (double)v[k], flux ? "" : " and >= 0");
        MGX_REQUIRE(v[k] == 0 || ((bc >> k) & 1), MGX_ERR_INVALID, "%s: %s[%d] = %g on face %d, which the mask %d does not flag", what,
                    flux ? "g" : "beta", k, (double)v[k], k, bc);
        MGX_REQUIRE(v[k] == 0 || std::isfinite((double)(((real)2 * v[k]) / h[k >> 1])), MGX_ERR_INVALID,
                    "%s: 2 * %s[%d] / h = 2 * %g / %g is not finite in this precision", what, flux ? "g" : "beta", k, (double)v[k],
                    (double)h[k >> 1]);
        if (any && v[k] != 0) *any = true;
    }
    return MGX_OK;
}

template <class real>
static WallD<real> wall_diagonal(const real beta[6], const real h[3]) {
    WallD<real> w;
    for (int k = 0; k < 6; k++) w.d[k] = ((real)2 * beta[k]) / h[k >> 1];
    return w;
}

// ------------------------------------------------------------------ pinned interior nodes (section 22)
// the list of a level's pinned points (device arrays): 32-bit storage offsets, the red points first, each colour sorted by offset,
// end[0] = the red ones, end[1] = all; val in list order, NULL = zeros.  The kernel and its launch: mgx_pin3d.hip, their one home.
template <class real>
struct PinList {
    const unsigned* idx;
    unsigned end[2];
    const real* val;
};
template <class real>
void pin_put_launch(mgx_ctx* ctx, real* v, const unsigned* idx, const real* val, unsigned first, unsigned count);

// ---- the drivers of the entries with a mask: one per operation, for the _bc entries (beta = NO_WALL) and the _wall entries alike.
// With bc = 0 (no beta can be non-zero then) nothing but the interior driver runs.
// ncycles red+black sweeps, each colour pass the interior launch and the face launch of that colour -- and, with a pin list, the
// launch that puts that colour's pinned values back, which the interior launch has overwritten and the next pass reads
template <class Op, class real>
static int relax_op3d_bc(mgx_ctx* ctx, real* v, const real* f, const real* a, const int n[3], const real h[3], real s, int ncycles, int bc,
                         const real beta[6], const char* what, const real* c = nullptr, const PinList<real>* pin = nullptr) {
    MGX_REQUIRE(ctx && v && f && (a || !Op::HAS_A) && (c || !Op::HAS_C) && n && h && beta, MGX_ERR_INVALID, "%s: NULL argument", what);
    RIM_BC_CHECK(bc, what);
    MGX_TRY_RET(wall_data_check<real>(beta, h, bc, false, what));
    if (pin && !pin->end[1]) pin = nullptr;  // an empty list: the entry without one
    MGX_REQUIRE(!pin || (pin->idx && pin->end[0] <= pin->end[1]), MGX_ERR_INVALID, "%s: bad pin list (idx %p, end %u, %u)", what,
                pin ? (const void*)pin->idx : nullptr, pin ? pin->end[0] : 0u, pin ? pin->end[1] : 0u);
    if (!bc && !pin) return relax_op3d<Op, real>(ctx, v, f, a, n, h, s, ncycles, 0, 0, what, c);
    const double sd = (double)s;
    MGX_TRY_RET(rows_check(n, what, &sd, false));
    MGX_REQUIRE(ncycles >= 0, MGX_ERR_INVALID, "%s: ncycles = %d < 0", what, ncycles);
    MGX_USE(ctx);
    const Op op = make_op<Op, real>(ctx, h, s, c);
    const WallD<real> w = wall_diagonal<real>(beta, h);
    Rim R = {};
    if (bc) MGX_TRY_RET(rim_list<real>(n, bc, what, R));
    for (int p = 0; p < 2 * ncycles; p++) {
        relax_op3d_pass<Op, real>(ctx, v, f, a, n, op, p & 1);
        if (bc) face_relax_launch<Op, real>(ctx, v, f, a, R, op, w, p & 1);
        if (pin) {
            const unsigned first = (p & 1) ? pin->end[0] : 0u;
            pin_put_launch<real>(ctx, v, pin->idx, pin->val, first, ((p & 1) ? pin->end[1] : pin->end[0]) - first);
        }
    }
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// r = the residual on all unknowns, 0 on the Dirichlet points (r == NULL: not stored); *dev_sumsq = the sum of its squares over all
// unknowns (NULL: none).  The face launch has at most as many blocks as the interior launch has partials: the work array of
// mgx3dxs_krylov_work_elems doubles, twice that count, holds both.
template <class Op, class real>
static int residual_op3d_bc(mgx_ctx* ctx, const real* v, const real* f, const real* a, real* r, const int n[3], const real h[3], real s,
                            double* dev_work, double* dev_sumsq, int bc, const real beta[6], const char* what, const real* c = nullptr) {
    MGX_REQUIRE(ctx && v && f && (a || !Op::HAS_A) && (c || !Op::HAS_C) && n && h && (r || dev_sumsq) && (!dev_sumsq || dev_work) && beta,
                MGX_ERR_INVALID, "%s: NULL argument", what);
    RIM_BC_CHECK(bc, what);
    MGX_TRY_RET(wall_data_check<real>(beta, h, bc, false, what));
    if (!bc) return residual_op3d<Op, real>(ctx, v, f, a, r, n, h, s, dev_work, dev_sumsq, what, c);
    const double sd = (double)s;
    MGX_TRY_RET(rows_check(n, what, &sd));
    MGX_USE(ctx);
    Rim R;
    MGX_TRY_RET(rim_list<real>(n, bc, what, R));
    if (r)  // every boundary point first: the Dirichlet points keep the 0
        rim_zero3d_xs<real>(ctx, r, n);
    const Op op = make_op<Op, real>(ctx, h, s, c);
    const WallD<real> w = wall_diagonal<real>(beta, h);
    MGX_TRY_RET((residual_op3d_launch<Op, false>(ctx, v, f, a, r, n, op, dev_work, dev_sumsq, false)));
    const dim3 g = krylov_grid(n);
    const size_t interior = (size_t)g.x * g.y;
    unsigned nb = rim_blocks(R);
    if (dev_sumsq && nb > interior) nb = (unsigned)interior;
    face_residual_launch<Op, real>(ctx, v, f, a, r, R, op, w, nb, dev_sumsq ? dev_work + interior : (double*)nullptr);
    MGX_LAUNCH_CHECK();
    return dev_sumsq ? krylov_final(ctx, dev_work, interior + nb, 1, dev_sumsq) : MGX_OK;
}

// q = A p on all unknowns and *dev_sum = <p, q>_W
template <class Op, class real>
static int apply_op_dot3d_bc(mgx_ctx* ctx, const real* p, const real* a, real* q, const int n[3], const real h[3], real s, double* dev_work,
                             double* dev_sum, int bc, const real beta[6], const char* what, const real* c = nullptr) {
    MGX_REQUIRE(ctx && p && (a || !Op::HAS_A) && (c || !Op::HAS_C) && q && n && h && dev_work && dev_sum && beta, MGX_ERR_INVALID,
                "%s: NULL argument", what);
    RIM_BC_CHECK(bc, what);
    MGX_TRY_RET(wall_data_check<real>(beta, h, bc, false, what));
    if (!bc) return apply_op_dot3d<Op, real>(ctx, p, a, q, n, h, s, dev_work, dev_sum, what, c);
    const double sd = (double)s;
    MGX_TRY_RET(rows_check(n, what, &sd));
    Rim R;
    MGX_TRY_RET(rim_list<real>(n, bc, what, R));
    MGX_USE(ctx);
    const Op op = make_op<Op, real>(ctx, h, s, c);
    const WallD<real> w = wall_diagonal<real>(beta, h);
    MGX_TRY_RET((residual_op3d_launch<Op, true>(ctx, p, (const real*)nullptr, a, q, n, op, dev_work, dev_sum, false)));
    const dim3 g = krylov_grid(n);
    const size_t interior = (size_t)g.x * g.y;
    const unsigned nb = rim_blocks(R);
    face_apply_dot_launch<Op, real>(ctx, p, a, q, R, op, w, nb, dev_work + interior);
    MGX_LAUNCH_CHECK();
    return krylov_final(ctx, dev_work, interior + nb, 1, dev_sum);
}

}  // namespace mgx
