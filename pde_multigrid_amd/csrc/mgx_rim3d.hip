// mgx_rim3d.hip -- homogeneous NEUMANN faces for the shifted and the variable-coefficient operator, x-split layout.  DESIGN.md
// section 15.
//
// A mask bc of six bits (bit 0 x-low, 1 x-high, 2 y-low, 3 y-high, 4 z-low, 5 z-high) makes the faces whose bit is set
// homogeneous Neumann, du/dn = 0.  A grid point is an UNKNOWN when it is interior, or when it lies on one or more Neumann faces
// and on no Dirichlet face (Dirichlet wins on shared edges and corners; Dirichlet entries of v are data and are never written).
// At an unknown on a face every operator is the interior's point expression on a star whose out-of-range entry is replaced by the
// opposite one (on x-low O := E, for v and for a; on an edge or corner on each axis): there is no new point arithmetic here, the
// kernels call Op::relax / Op::residual<MODE> (mgx_ops3d.hpp; the operator kernels of mgx_wall3d.hip, with every beta zero),
// restrict3d_point and interpolate3d_point (mgx_kernels3d.hpp) on reflected indices.
//
// The tuned interior kernels run unchanged; every entry below is the existing entry followed by (the colour passes: interleaved
// with) a RIM launch over the face unknowns, all six faces of a call in one launch.  Points of one colour are independent and the
// rim launch of a colour reads only points of the other colour, so a colour pass is the interior launch plus the rim launch of that
// colour, in stream order.  With bc = 0 nothing but the existing entry runs.
//
// The rim launch: a 1-D grid whose threads stride over the list of face points -- the two z-faces as whole planes (row pitch P
// positions per row: the lanes of a wave run along a row's storage positions, pads skipped), the two y-faces as whole rows of the
// planes 1 .. sz-2, the two x-faces as the points (y, z) of the open square, the lanes along y.  The x-faces are the first and the
// last entry of a row's even-x half: one line per point whatever the lane order; with the lanes along y the rows above and below
// are the neighbouring lanes' own lines.  Only the faces whose bit is set are listed, and a listed point that lies on a Dirichlet
// face as well is skipped.  No scratch; the residual's partial sums go behind the interior launch's in the caller's work array.
//
// The list, the reflected star and the drivers of the operator entries are in mgx_rim3d.hpp; the kernels of the operators on the
// face unknowns are in mgx_wall3d.hip, one set for the _bc entries and the _wall entries (section 18).  This file instantiates the
// drivers for ShiftOp and CoefOp (mgx_cap3d.hip: for CapOp) and holds the transfers and vector kernels.
#include "mgx_rim3d.hpp"

namespace mgx {

// coarse = restrict3d_point on the 27 reflected fine values, at the coarse face unknowns (R lists the COARSE grid)
template <class real>
__global__ void __launch_bounds__(RIM_THREADS) rim_restrict3d_xs_kernel(const real* __restrict__ fine, int fsx, int fsy, int fsz,
                                                                        real* __restrict__ coarse, Rim R) {
    const Geo<XSplit, real> gc(R.sx, R.sy), gf(fsx, fsy);
    RIM_FOR_EACH_POINT(R, gc, x, y, z) {
        auto get = [&](int dx, int dy, int dz) __attribute__((always_inline)) {
            return fine[gf.row(rim_reflect(2 * y + dy, fsy), rim_reflect(2 * z + dz, fsz)) + gf.pos(rim_reflect(2 * x + dx, fsx))];
        };
        coarse[gc.row(y, z) + gc.pos(x)] = restrict3d_point<real>(get);
    }
}

// fine (+)= interpolate3d_point at the fine face unknowns (R lists the FINE grid).  A face coordinate is even, so on the axis of
// its face a point reads the coarse point of the same face only.
template <class real, bool ADD>
__global__ void __launch_bounds__(RIM_THREADS) rim_interpolate3d_xs_kernel(real* __restrict__ fine, const real* __restrict__ coarse, int csx,
                                                                           int csy, Rim R) {
    const Geo<XSplit, real> gf(R.sx, R.sy), gc(csx, csy);
    RIM_FOR_EACH_POINT(R, gf, x, y, z) {
        auto get = [&](int dx, int dy, int dz) __attribute__((always_inline)) {
            return coarse[gc.row((y >> 1) + dy, (z >> 1) + dz) + gc.pos((x >> 1) + dx)];
        };
        const real e = interpolate3d_point<real>(x & 1, y & 1, z & 1, get);
        const size_t i = gf.row(y, z) + gf.pos(x);
        fine[i] = ADD ? fine[i] + e : e;
    }
}

// f = (-(s*u)) - qscale*q on the face unknowns (q == NULL: f = -(s*u))
template <class real>
__global__ void __launch_bounds__(RIM_THREADS) rim_shift_rhs3d_xs_kernel(const real* __restrict__ u, const real* __restrict__ q, real qscale,
                                                                         real s, real* __restrict__ f, Rim R) {
    const Geo<XSplit, real> g(R.sx, R.sy);
    RIM_FOR_EACH_POINT(R, g, x, y, z) {
        const size_t i = g.row(y, z) + g.pos(x);
        real t = -(s * u[i]);
        if (q) t = t - qscale * q[i];
        f[i] = t;
    }
}

// the face unknowns := value
template <class real>
__global__ void __launch_bounds__(RIM_THREADS) rim_set3d_xs_kernel(real* __restrict__ v, real value, Rim R) {
    const Geo<XSplit, real> g(R.sx, R.sy);
    RIM_FOR_EACH_POINT(R, g, x, y, z) v[g.row(y, z) + g.pos(x)] = value;
}

// [x += alpha p;] r -= alpha q, partials of <r, r> (unweighted: the stopping rule's norm)
template <class real, bool X>
__global__ void __launch_bounds__(RIM_THREADS) rim_cg_update3d_xs_kernel(real* __restrict__ xv, const real* __restrict__ p, real* __restrict__ r,
                                                                         const real* __restrict__ q, Rim R,
                                                                         const double* __restrict__ dev_alpha, double* __restrict__ partial) {
    const Geo<XSplit, real> g(R.sx, R.sy);
    const real al = (real)*dev_alpha;
    double acc = 0.0;
    RIM_FOR_EACH_POINT(R, g, x, y, z) {
        const size_t i = g.row(y, z) + g.pos(x);
        if (X) xv[i] = xv[i] + al * p[i];
        const real t = r[i] - al * q[i];
        r[i] = t;
        acc += (double)t * (double)t;
    }
    __shared__ double part[RIM_THREADS / 64];
    rim_block_sum(acc, part, partial + blockIdx.x);
}

// partials of <a, b>_W at pab[block] and, with TWO, of <a, c>_W at pac[block]
template <class real, bool TWO>
__global__ void __launch_bounds__(RIM_THREADS) rim_dot2_3d_xs_kernel(const real* __restrict__ a, const real* __restrict__ b,
                                                                     const real* __restrict__ c, Rim R, double* __restrict__ pab,
                                                                     double* __restrict__ pac) {
    const Geo<XSplit, real> g(R.sx, R.sy);
    double ab = 0.0, ac = 0.0;
    RIM_FOR_EACH_POINT(R, g, x, y, z) {
        const size_t i = g.row(y, z) + g.pos(x);
        const double w = rim_weight(R, x, y, z), av = (double)a[i];
        ab += w * (av * (double)b[i]);
        if (TWO) ac += w * (av * (double)c[i]);
    }
    __shared__ double part[2][RIM_THREADS / 64];
    rim_block_sum(ab, part[0], pab + blockIdx.x);
    if (TWO) rim_block_sum(ac, part[1], pac + blockIdx.x);
}

// partials of the UNWEIGHTED sum of a^2 over the face unknowns (the stopping rule's norm of a stored residual)
template <class real>
__global__ void __launch_bounds__(RIM_THREADS) rim_sumsq3d_xs_kernel(const real* __restrict__ a, Rim R, double* __restrict__ partial) {
    const Geo<XSplit, real> g(R.sx, R.sy);
    double acc = 0.0;
    RIM_FOR_EACH_POINT(R, g, x, y, z) {
        const double av = (double)a[g.row(y, z) + g.pos(x)];
        acc += av * av;
    }
    __shared__ double part[RIM_THREADS / 64];
    rim_block_sum(acc, part, partial + blockIdx.x);
}

// X: x += alpha p (the old p); P_: p = z + beta p (BETA) or p = z
template <class real, bool X, bool P_, bool BETA>
__global__ void __launch_bounds__(RIM_THREADS) rim_cg_direction3d_xs_kernel(real* __restrict__ xv, real* __restrict__ p,
                                                                            const real* __restrict__ zv, Rim R,
                                                                            const double* __restrict__ dev_alpha,
                                                                            const double* __restrict__ dev_beta) {
    const Geo<XSplit, real> g(R.sx, R.sy);
    const real al = X ? (real)*dev_alpha : (real)0, be = BETA ? (real)*dev_beta : (real)0;
    RIM_FOR_EACH_POINT(R, g, x, y, z) {
        const size_t i = g.row(y, z) + g.pos(x);
        const real pv = (X || BETA) ? p[i] : (real)0;
        if (X) xv[i] = xv[i] + al * pv;
        if (P_) p[i] = BETA ? zv[i] + be * pv : zv[i];
    }
}

// the projection a -= mean_W(a): partials of sum_W(a) over the face unknowns ...
template <class real>
__global__ void __launch_bounds__(RIM_THREADS) rim_sum3d_xs_kernel(const real* __restrict__ a, Rim R, double* __restrict__ partial) {
    const Geo<XSplit, real> g(R.sx, R.sy);
    double acc = 0.0;
    RIM_FOR_EACH_POINT(R, g, x, y, z) acc += rim_weight(R, x, y, z) * (double)a[g.row(y, z) + g.pos(x)];
    __shared__ double part[RIM_THREADS / 64];
    rim_block_sum(acc, part, partial + blockIdx.x);
}

// ... and of sum(a) over the interior, with the row walk of dot2_3d_xs_kernel (mgx_krylov3d.hip)
template <class real>
__global__ void __launch_bounds__(256) sum3d_xs_kernel(const real* __restrict__ a, int sx, int sy, double* __restrict__ partial) {
    const Geo<XSplit, real> g(sx, sy);
    const int y = 1 + blockIdx.x * KROWS + threadIdx.y, z = 1 + blockIdx.y;
    const int H = g.H, P = g.P;
    double acc = 0.0;
    if (y < sy - 1) {
        const size_t row = g.row(y, z);
        for (int j0 = 0; j0 < P; j0 += KSTEP) {
            real av[KJ];
            bool in[KJ];
#pragma unroll
            for (int k = 0; k < KJ; k++) {
                const int j = j0 + k * 64 + threadIdx.x, xx = xs_x(j, H);
                in[k] = j < P && xx >= 1 && xx <= sx - 2;
                if (in[k]) av[k] = a[row + j];
            }
#pragma unroll
            for (int k = 0; k < KJ; k++)
                if (in[k]) acc += (double)av[k];
        }
    }
    __shared__ double part[KROWS];
    block_sum(acc, part, partial);
}

// *out = (the sum of partial[0 .. count), in cg_final_kernel's order) / sumw: one block
__global__ void __launch_bounds__(1024) mean_final_kernel(const double* __restrict__ partial, size_t count, double sumw, double* __restrict__ out) {
    __shared__ double s[1024];
    double acc = 0.0;
    for (size_t i = threadIdx.x; i < count; i += 1024) acc += partial[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s[0] / sumw;
}

// out[s] = the sum of the interior partials work[s nI .. (s + 1) nI) and the rim partials work[2 nI + s nR .. 2 nI + (s + 1) nR),
// s = 0, 1: dot2's two sums, one block each, fixed order
__global__ void __launch_bounds__(1024) rim_final2_kernel(const double* __restrict__ work, size_t nI, size_t nR, double* __restrict__ out) {
    __shared__ double s[1024];
    const double *pi = work + (size_t)blockIdx.x * nI, *pr = work + 2 * nI + (size_t)blockIdx.x * nR;
    double acc = 0.0;
    for (size_t i = threadIdx.x; i < nI; i += 1024) acc += pi[i];
    for (size_t i = threadIdx.x; i < nR; i += 1024) acc += pr[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = s[0];
}

// a -= (real)*dev_mean on the interior ...
template <class real>
__global__ void __launch_bounds__(256) subtract3d_xs_kernel(real* __restrict__ a, int sx, int sy, const double* __restrict__ dev_mean) {
    const Geo<XSplit, real> g(sx, sy);
    const int y = 1 + blockIdx.x * KROWS + threadIdx.y, z = 1 + blockIdx.y;
    if (y >= sy - 1) return;
    const int H = g.H, P = g.P;
    const real m = (real)*dev_mean;
    const size_t row = g.row(y, z);
    for (int j = threadIdx.x; j < P; j += 64) {
        const int xx = xs_x(j, H);
        if (xx >= 1 && xx <= sx - 2) a[row + j] = a[row + j] - m;
    }
}

// ... and on the face unknowns
template <class real>
__global__ void __launch_bounds__(RIM_THREADS) rim_subtract3d_xs_kernel(real* __restrict__ a, Rim R, const double* __restrict__ dev_mean) {
    const Geo<XSplit, real> g(R.sx, R.sy);
    const real m = (real)*dev_mean;
    RIM_FOR_EACH_POINT(R, g, x, y, z) {
        const size_t i = g.row(y, z) + g.pos(x);
        a[i] = a[i] - m;
    }
}

// =========================================================================== host side
// the coarse sizes of a transfer with a mask: a level of its own, odd and >= 3 (the existing entries ask that of the fine sizes only)
static int rim_coarse_check(const int cn[3], const char* what) {
    for (int d = 0; d < 3; d++)
        MGX_REQUIRE(valid_size(cn[d]), MGX_ERR_SIZE, "%s: coarse size[%d] = %d is not odd and >= 3", what, d, cn[d]);
    return MGX_OK;
}

template <class real>
static int rim_set3d(mgx_ctx* ctx, real* v, const int n[3], real value, int bc) {
    MGX_REQUIRE(ctx && v && n, MGX_ERR_INVALID, "set_rim_bc: NULL argument");
    RIM_BC_CHECK(bc, "set_rim_bc");
    MGX_TRY_RET(rows_check(n, "set_rim_bc", nullptr, false));
    MGX_REQUIRE((double)n[0] * n[1] * n[2] < 2147483647.0 * 4, MGX_ERR_SIZE, "set_rim_bc: grid too large");
    if (!bc) return MGX_OK;
    MGX_USE(ctx);
    Rim R;
    MGX_TRY_RET(rim_list<real>(n, bc, "set_rim_bc", R));
    MGX_LAUNCH((rim_set3d_xs_kernel<real>), dim3(rim_blocks(R)), dim3(RIM_THREADS), 0, ctx->compute, v, value, R);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// ---- the solve's vector entries for all unknowns.  Each checks its arguments and the mask before it uses any of them; with bc = 0
// it is the existing entry.  Work array (krylov_work_elems_bc doubles): the interior launch's partials, count = its blocks, as it
// lays them out, the rim launch's behind them.
template <class real>
static size_t krylov_work_elems_bc(const int n[3]) {
    Rim R;
    if (rows_check(n, "krylov_work_elems_bc") || rim_list<real>(n, 63, "krylov_work_elems_bc", R)) return 0;
    const dim3 g = krylov_grid(n);
    return 2 * ((size_t)g.x * g.y + rim_blocks(R));  // (a mask's list is at most as long as that of all six faces)
}

template <class real>
static int cg_update3d_bc(mgx_ctx* ctx, real* x, const real* p, real* r, const real* q, const int n[3], const double* dev_alpha,
                          double* dev_work, double* dev_sum, int bc) {
    MGX_REQUIRE(ctx && r && q && (!x || p) && n && dev_alpha && dev_work && dev_sum, MGX_ERR_INVALID, "cg_update_bc: NULL argument");
    RIM_BC_CHECK(bc, "cg_update_bc");
    if (!bc) return cg_update3d<real>(ctx, x, p, r, q, n, dev_alpha, dev_work, dev_sum, true);
    MGX_TRY_RET(rows_check(n, "cg_update_bc"));
    Rim R;
    MGX_TRY_RET(rim_list<real>(n, bc, "cg_update_bc", R));
    MGX_TRY_RET(cg_update3d<real>(ctx, x, p, r, q, n, dev_alpha, dev_work, dev_sum, false));
    const dim3 g = krylov_grid(n);
    const size_t interior = (size_t)g.x * g.y;
    const unsigned nb = rim_blocks(R);
    if (x) MGX_LAUNCH((rim_cg_update3d_xs_kernel<real, true>), dim3(nb), dim3(RIM_THREADS), 0, ctx->compute, x, p, r, q, R, dev_alpha,
                      dev_work + interior);
    else MGX_LAUNCH((rim_cg_update3d_xs_kernel<real, false>), dim3(nb), dim3(RIM_THREADS), 0, ctx->compute, x, p, r, q, R, dev_alpha,
                    dev_work + interior);
    MGX_LAUNCH_CHECK();
    return krylov_final(ctx, dev_work, interior + nb, 1, dev_sum);
}

template <class real>
static int dot2_3d_bc(mgx_ctx* ctx, const real* a, const real* b, const real* c, const int n[3], double* dev_work, double* dev_sum, int bc) {
    MGX_REQUIRE(ctx && a && b && n && dev_work && dev_sum, MGX_ERR_INVALID, "dot2_bc: NULL argument");
    RIM_BC_CHECK(bc, "dot2_bc");
    if (!bc) return dot2_3d<real>(ctx, a, b, c, n, dev_work, dev_sum, true);
    MGX_TRY_RET(rows_check(n, "dot2_bc"));
    Rim R;
    MGX_TRY_RET(rim_list<real>(n, bc, "dot2_bc", R));
    MGX_TRY_RET(dot2_3d<real>(ctx, a, b, c, n, dev_work, dev_sum, false));
    const dim3 g = krylov_grid(n);
    const size_t interior = (size_t)g.x * g.y;
    const unsigned nb = rim_blocks(R);
    if (!c) {
        MGX_LAUNCH((rim_dot2_3d_xs_kernel<real, false>), dim3(nb), dim3(RIM_THREADS), 0, ctx->compute, a, b, c, R, dev_work + interior,
                   (double*)nullptr);
        MGX_LAUNCH_CHECK();
        return krylov_final(ctx, dev_work, interior + nb, 1, dev_sum);
    }
    // the interior launch has put <a, c>'s partials directly behind <a, b>'s: the rim's go behind both, summed by a final of their own
    MGX_LAUNCH((rim_dot2_3d_xs_kernel<real, true>), dim3(nb), dim3(RIM_THREADS), 0, ctx->compute, a, b, c, R, dev_work + 2 * interior,
               dev_work + 2 * interior + nb);
    MGX_LAUNCH(rim_final2_kernel, dim3(2), dim3(1024), 0, ctx->compute, (const double*)dev_work, interior, (size_t)nb, dev_sum);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// *dev_sum = the unweighted sum of a^2 over all unknowns (bc = 0: dot2(a, a)'s bits)
template <class real>
static int sumsq3d_bc(mgx_ctx* ctx, const real* a, const int n[3], double* dev_work, double* dev_sum, int bc) {
    MGX_REQUIRE(ctx && a && n && dev_work && dev_sum, MGX_ERR_INVALID, "sumsq_bc: NULL argument");
    RIM_BC_CHECK(bc, "sumsq_bc");
    if (!bc) return dot2_3d<real>(ctx, a, a, nullptr, n, dev_work, dev_sum, true);
    MGX_TRY_RET(rows_check(n, "sumsq_bc"));
    Rim R;
    MGX_TRY_RET(rim_list<real>(n, bc, "sumsq_bc", R));
    MGX_TRY_RET(dot2_3d<real>(ctx, a, a, nullptr, n, dev_work, dev_sum, false));
    const dim3 g = krylov_grid(n);
    const size_t interior = (size_t)g.x * g.y;
    const unsigned nb = rim_blocks(R);
    MGX_LAUNCH((rim_sumsq3d_xs_kernel<real>), dim3(nb), dim3(RIM_THREADS), 0, ctx->compute, a, R, dev_work + interior);
    MGX_LAUNCH_CHECK();
    return krylov_final(ctx, dev_work, interior + nb, 1, dev_sum);
}

template <class real>
static int cg_direction3d_bc(mgx_ctx* ctx, real* x, real* p, const real* z, const int n[3], const double* dev_alpha, const double* dev_beta,
                             int bc) {
    MGX_REQUIRE(ctx && p && n && (!x || dev_alpha), MGX_ERR_INVALID, "cg_direction_bc: NULL argument");
    MGX_REQUIRE(x || z, MGX_ERR_INVALID, "cg_direction_bc: nothing to do (x and z are NULL)");
    RIM_BC_CHECK(bc, "cg_direction_bc");
    if (!bc) return cg_direction3d<real>(ctx, x, p, z, n, dev_alpha, dev_beta);
    MGX_TRY_RET(rows_check(n, "cg_direction_bc"));
    Rim R;
    MGX_TRY_RET(rim_list<real>(n, bc, "cg_direction_bc", R));
    MGX_TRY_RET(cg_direction3d<real>(ctx, x, p, z, n, dev_alpha, dev_beta));
#define MGX_DIR(X, P_, B)                                                                                                               \
    MGX_LAUNCH((rim_cg_direction3d_xs_kernel<real, X, P_, B>), dim3(rim_blocks(R)), dim3(RIM_THREADS), 0, ctx->compute, x, p, z, R, dev_alpha, \
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

// *dev_mean = sum_W(a) / sum(W), a -= (real)*dev_mean at every unknown; sum(W) = the product over the axes of the axis's interior
// points plus half a point per Neumann end
template <class real>
static int project3d_bc(mgx_ctx* ctx, real* a, const int n[3], double* dev_work, double* dev_mean, int bc) {
    MGX_REQUIRE(ctx && a && n && dev_work && dev_mean, MGX_ERR_INVALID, "project_bc: NULL argument");
    RIM_BC_CHECK(bc, "project_bc");
    MGX_TRY_RET(rows_check(n, "project_bc"));
    Rim R = {};
    if (bc) MGX_TRY_RET(rim_list<real>(n, bc, "project_bc", R));
    MGX_USE(ctx);
    double sumw = 1.0;
    for (int d = 0; d < 3; d++) sumw *= (double)(n[d] - 2) + 0.5 * (((bc >> (2 * d)) & 1) + ((bc >> (2 * d + 1)) & 1));
    const dim3 g = krylov_grid(n);
    const size_t interior = (size_t)g.x * g.y;
    const unsigned nb = bc ? rim_blocks(R) : 0;
    MGX_LAUNCH((sum3d_xs_kernel<real>), g, krylov_block(), 0, ctx->compute, (const real*)a, n[0], n[1], dev_work);
    if (bc) MGX_LAUNCH((rim_sum3d_xs_kernel<real>), dim3(nb), dim3(RIM_THREADS), 0, ctx->compute, (const real*)a, R, dev_work + interior);
    MGX_LAUNCH(mean_final_kernel, dim3(1), dim3(1024), 0, ctx->compute, (const double*)dev_work, interior + nb, sumw, dev_mean);
    MGX_LAUNCH((subtract3d_xs_kernel<real>), g, krylov_block(), 0, ctx->compute, a, n[0], n[1], (const double*)dev_mean);
    if (bc) MGX_LAUNCH((rim_subtract3d_xs_kernel<real>), dim3(nb), dim3(RIM_THREADS), 0, ctx->compute, a, R, (const double*)dev_mean);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

}  // namespace mgx

// each transfer entry runs the existing entry first: it checks the sizes (the coarse ones are (n - 1) / 2 + 1) before the rim launch,
// which makes the context's device current itself
#define MGX_RIM3D_API(SFX, real)                                                                                                             \
    extern "C" int mgx3dxs_relax_shift_bc_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], real s, int ncycles,   \
                                                int bc) {                                                                                    \
        return mgx::relax_op3d_bc<mgx::ShiftOp<real>, real>(ctx, v, f, nullptr, n, h, s, ncycles, bc, mgx::NO_WALL<real>, "relax_shift_bc"); \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_relax_coef_bc_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const int n[3], const real h[3], real s,  \
                                               int ncycles, int bc) {                                                                        \
        return mgx::relax_op3d_bc<mgx::CoefOp<real>, real>(ctx, v, f, a, n, h, s, ncycles, bc, mgx::NO_WALL<real>, "relax_coef_bc");         \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_residual_shift_bc_##SFX(mgx_ctx* ctx, const real* v, const real* f, real* r, const int n[3], const real h[3],      \
                                                   real s, double* dev_work, double* dev_sumsq, int bc) {                                    \
        return mgx::residual_op3d_bc<mgx::ShiftOp<real>, real>(ctx, v, f, nullptr, r, n, h, s, dev_work, dev_sumsq, bc,                       \
                                                               mgx::NO_WALL<real>, "residual_shift_bc");                                      \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_residual_coef_bc_##SFX(mgx_ctx* ctx, const real* v, const real* f, const real* a, real* r, const int n[3],         \
                                                  const real h[3], real s, double* dev_work, double* dev_sumsq, int bc) {                    \
        return mgx::residual_op3d_bc<mgx::CoefOp<real>, real>(ctx, v, f, a, r, n, h, s, dev_work, dev_sumsq, bc,                             \
                                                              mgx::NO_WALL<real>, "residual_coef_bc");                                       \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_relax_shift_wall_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], real s, int ncycles,\
                                                  int bc, const real beta[6]) {                                                              \
        return mgx::relax_op3d_bc<mgx::ShiftOp<real>, real>(ctx, v, f, nullptr, n, h, s, ncycles, bc, beta, "relax_shift_wall");             \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_relax_coef_wall_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const int n[3], const real h[3], real s,\
                                                 int ncycles, int bc, const real beta[6]) {                                                  \
        return mgx::relax_op3d_bc<mgx::CoefOp<real>, real>(ctx, v, f, a, n, h, s, ncycles, bc, beta, "relax_coef_wall");                     \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_residual_shift_wall_##SFX(mgx_ctx* ctx, const real* v, const real* f, real* r, const int n[3], const real h[3],   \
                                                     real s, double* dev_work, double* dev_sumsq, int bc, const real beta[6]) {              \
        return mgx::residual_op3d_bc<mgx::ShiftOp<real>, real>(ctx, v, f, nullptr, r, n, h, s, dev_work, dev_sumsq, bc, beta,                \
                                                                 "residual_shift_wall");                                                     \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_residual_coef_wall_##SFX(mgx_ctx* ctx, const real* v, const real* f, const real* a, real* r, const int n[3],      \
                                                    const real h[3], real s, double* dev_work, double* dev_sumsq, int bc,                    \
                                                    const real beta[6]) {                                                                    \
        return mgx::residual_op3d_bc<mgx::CoefOp<real>, real>(ctx, v, f, a, r, n, h, s, dev_work, dev_sumsq, bc, beta, "residual_coef_wall");  \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_relax_shift_pin_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], real s, int ncycles, int bc, const real beta[6], const unsigned* idx, \
            const unsigned end[2], const real* val) {                                                                                        \
        MGX_REQUIRE(end, MGX_ERR_INVALID, "relax_shift_pin: NULL argument");                                                                 \
        const mgx::PinList<real> pin = {idx, {end[0], end[1]}, val};                                                                         \
        return mgx::relax_op3d_bc<mgx::ShiftOp<real>, real>(ctx, v, f, nullptr, n, h, s, ncycles, bc, beta, "relax_shift_pin", nullptr, &pin); \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_relax_coef_pin_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const int n[3], const real h[3], real s, int ncycles, int bc, const real beta[6], const unsigned* idx, \
            const unsigned end[2], const real* val) {                                                                                        \
        MGX_REQUIRE(end, MGX_ERR_INVALID, "relax_coef_pin: NULL argument");                                                                  \
        const mgx::PinList<real> pin = {idx, {end[0], end[1]}, val};                                                                         \
        return mgx::relax_op3d_bc<mgx::CoefOp<real>, real>(ctx, v, f, a, n, h, s, ncycles, bc, beta, "relax_coef_pin", nullptr, &pin);       \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_restrict_bc_##SFX(mgx_ctx* ctx, const real* fine, const int fn[3], real* coarse, const int cn[3], int bc) {        \
        MGX_REQUIRE(ctx && fine && fn && coarse && cn, MGX_ERR_INVALID, "restrict_bc: NULL argument");                                       \
        RIM_BC_CHECK(bc, "restrict_bc");                                                                                                     \
        if (bc) MGX_TRY_RET(mgx::rim_coarse_check(cn, "restrict_bc"));                                                                       \
        MGX_TRY_RET(mgx3dxs_restrict_##SFX(ctx, fine, fn, coarse, cn));                                                                      \
        if (!bc) return MGX_OK;                                                                                                              \
        mgx::Rim R;                                                                                                                          \
        MGX_TRY_RET(mgx::rim_list<real>(cn, bc, "restrict_bc", R));                                                                          \
        MGX_USE(ctx);                                                                                                                        \
        MGX_LAUNCH((mgx::rim_restrict3d_xs_kernel<real>), dim3(mgx::rim_blocks(R)), dim3(mgx::RIM_THREADS), 0, ctx->compute, fine, fn[0],    \
                   fn[1], fn[2], coarse, R);                                                                                                 \
        MGX_LAUNCH_CHECK();                                                                                                                  \
        return MGX_OK;                                                                                                                       \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_interpolate_bc_##SFX(mgx_ctx* ctx, real* fine, const int fn[3], const real* coarse, const int cn[3], int bc) {     \
        MGX_REQUIRE(ctx && fine && fn && coarse && cn, MGX_ERR_INVALID, "interpolate_bc: NULL argument");                                    \
        RIM_BC_CHECK(bc, "interpolate_bc");                                                                                                  \
        if (bc) MGX_TRY_RET(mgx::rim_coarse_check(cn, "interpolate_bc"));                                                                    \
        MGX_TRY_RET(mgx3dxs_interpolate_##SFX(ctx, fine, fn, coarse, cn));                                                                   \
        if (!bc) return MGX_OK;                                                                                                              \
        mgx::Rim R;                                                                                                                          \
        MGX_TRY_RET(mgx::rim_list<real>(fn, bc, "interpolate_bc", R));                                                                       \
        MGX_USE(ctx);                                                                                                                        \
        MGX_LAUNCH((mgx::rim_interpolate3d_xs_kernel<real, false>), dim3(mgx::rim_blocks(R)), dim3(mgx::RIM_THREADS), 0, ctx->compute, fine, \
                   coarse, cn[0], cn[1], R);                                                                                                 \
        MGX_LAUNCH_CHECK();                                                                                                                  \
        return MGX_OK;                                                                                                                       \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_interpolate_correct_bc_##SFX(mgx_ctx* ctx, real* v, const int n[3], const real* coarse_v, const int cn[3],         \
                                                        int bc) {                                                                            \
        MGX_REQUIRE(ctx && v && n && coarse_v && cn, MGX_ERR_INVALID, "interpolate_correct_bc: NULL argument");                              \
        RIM_BC_CHECK(bc, "interpolate_correct_bc");                                                                                          \
        if (bc) MGX_TRY_RET(mgx::rim_coarse_check(cn, "interpolate_correct_bc"));                                                            \
        MGX_TRY_RET(mgx3dxs_interpolate_correct_##SFX(ctx, v, n, coarse_v, cn));                                                             \
        if (!bc) return MGX_OK;                                                                                                              \
        mgx::Rim R;                                                                                                                          \
        MGX_TRY_RET(mgx::rim_list<real>(n, bc, "interpolate_correct_bc", R));                                                                \
        MGX_USE(ctx);                                                                                                                        \
        MGX_LAUNCH((mgx::rim_interpolate3d_xs_kernel<real, true>), dim3(mgx::rim_blocks(R)), dim3(mgx::RIM_THREADS), 0, ctx->compute, v,     \
                   coarse_v, cn[0], cn[1], R);                                                                                               \
        MGX_LAUNCH_CHECK();                                                                                                                  \
        return MGX_OK;                                                                                                                       \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_shift_rhs_bc_##SFX(mgx_ctx* ctx, const real* u, const real* q, real qscale, real s, real* f, const int n[3],       \
                                              int bc) {                                                                                      \
        MGX_REQUIRE(ctx && u && f && n, MGX_ERR_INVALID, "shift_rhs_bc: NULL argument");                                                     \
        RIM_BC_CHECK(bc, "shift_rhs_bc");                                                                                                    \
        MGX_TRY_RET(mgx3dxs_shift_rhs_##SFX(ctx, u, q, qscale, s, f, n));                                                                    \
        if (!bc) return MGX_OK;                                                                                                              \
        mgx::Rim R;                                                                                                                          \
        MGX_TRY_RET(mgx::rim_list<real>(n, bc, "shift_rhs_bc", R));                                                                          \
        MGX_USE(ctx);                                                                                                                        \
        MGX_LAUNCH((mgx::rim_shift_rhs3d_xs_kernel<real>), dim3(mgx::rim_blocks(R)), dim3(mgx::RIM_THREADS), 0, ctx->compute, u, q, qscale,  \
                   s, f, R);                                                                                                                 \
        MGX_LAUNCH_CHECK();                                                                                                                  \
        return MGX_OK;                                                                                                                       \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_set_rim_bc_##SFX(mgx_ctx* ctx, real* v, const int n[3], real value, int bc) {                                     \
        return mgx::rim_set3d<real>(ctx, v, n, value, bc);                                                                                   \
    }

MGX_RIM3D_API(f32, float)
MGX_RIM3D_API(f64, double)

#define MGX_RIM3D_KRYLOV_API(SFX, real)                                                                                                      \
    extern "C" size_t mgx3dxs_krylov_work_elems_bc_##SFX(const int n[3]) { return mgx::krylov_work_elems_bc<real>(n); }                      \
    extern "C" int mgx3dxs_laplace_dot_shift_bc_##SFX(mgx_ctx* ctx, const real* p, real* q, const int n[3], const real h[3], real s,          \
                                                      double* dev_work, double* dev_sum, int bc) {                                           \
        return mgx::apply_op_dot3d_bc<mgx::ShiftOp<real>, real>(ctx, p, nullptr, q, n, h, s, dev_work, dev_sum, bc,                          \
                                                                mgx::NO_WALL<real>, "laplace_dot_shift_bc");                                 \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_apply_coef_dot_bc_##SFX(mgx_ctx* ctx, const real* p, const real* a, real* q, const int n[3], const real h[3],      \
                                                   real s, double* dev_work, double* dev_sum, int bc) {                                      \
        return mgx::apply_op_dot3d_bc<mgx::CoefOp<real>, real>(ctx, p, a, q, n, h, s, dev_work, dev_sum, bc,                                 \
                                                               mgx::NO_WALL<real>, "apply_coef_dot_bc");                                     \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_laplace_dot_shift_wall_##SFX(mgx_ctx* ctx, const real* p, real* q, const int n[3], const real h[3], real s,       \
                                                        double* dev_work, double* dev_sum, int bc, const real beta[6]) {                     \
        return mgx::apply_op_dot3d_bc<mgx::ShiftOp<real>, real>(ctx, p, nullptr, q, n, h, s, dev_work, dev_sum, bc, beta,                    \
                                                                  "laplace_dot_shift_wall");                                                 \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_apply_coef_dot_wall_##SFX(mgx_ctx* ctx, const real* p, const real* a, real* q, const int n[3], const real h[3],   \
                                                     real s, double* dev_work, double* dev_sum, int bc, const real beta[6]) {                \
        return mgx::apply_op_dot3d_bc<mgx::CoefOp<real>, real>(ctx, p, a, q, n, h, s, dev_work, dev_sum, bc, beta, "apply_coef_dot_wall");   \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_cg_update_bc_##SFX(mgx_ctx* ctx, real* x, const real* p, real* r, const real* q, const int n[3],                  \
                                              const double* dev_alpha, double* dev_work, double* dev_sum, int bc) {                          \
        return mgx::cg_update3d_bc<real>(ctx, x, p, r, q, n, dev_alpha, dev_work, dev_sum, bc);                                              \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_dot2_bc_##SFX(mgx_ctx* ctx, const real* a, const real* b, const real* c, const int n[3], double* dev_work,         \
                                         double* dev_sum, int bc) {                                                                          \
        return mgx::dot2_3d_bc<real>(ctx, a, b, c, n, dev_work, dev_sum, bc);                                                                \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_sumsq_bc_##SFX(mgx_ctx* ctx, const real* a, const int n[3], double* dev_work, double* dev_sum, int bc) {            \
        return mgx::sumsq3d_bc<real>(ctx, a, n, dev_work, dev_sum, bc);                                                                      \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_cg_direction_bc_##SFX(mgx_ctx* ctx, real* x, real* p, const real* z, const int n[3], const double* dev_alpha,      \
                                                 const double* dev_beta, int bc) {                                                           \
        return mgx::cg_direction3d_bc<real>(ctx, x, p, z, n, dev_alpha, dev_beta, bc);                                                       \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_project_bc_##SFX(mgx_ctx* ctx, real* a, const int n[3], double* dev_work, double* dev_mean, int bc) {              \
        return mgx::project3d_bc<real>(ctx, a, n, dev_work, dev_mean, bc);                                                                   \
    }

MGX_RIM3D_KRYLOV_API(f32, float)
MGX_RIM3D_KRYLOV_API(f64, double)
