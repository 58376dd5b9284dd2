// mgx_small3d.hip -- the levels of at most 17 points per axis (SMALL_MAX, mgx_host3d.hpp), resident in the LDS of ONE workgroup.
//   relax3d_small_kernel      all sweeps of a Relax call on such a level (relax3d of mgx_kernels3d.hip calls relax3d_small)
//   cycle3d_tail_kernel       the whole V-cycle below 17^3: every level of the tail in LDS
// Same per-point expressions (mgx_kernels3d.hpp), colour and operator order as the launch-per-operator path: bit-identical.
#include "mgx_host3d.hpp"

namespace mgx {

// ------------------------------------------------------------------ relax, whole small level in one workgroup
// Levels up to 17^3 (<= 4913 points) are pure launch latency with one launch per colour pass (about 5 us each;
// the thesis runs 3000 sweeps per level).  Here ONE workgroup keeps v and f of the whole level in LDS (2 x 38 KB
// in fp64) and runs all `ncycles` red-black sweeps with a barrier between colour passes.  Same per-point
// expression, same colour order: bit-identical to the multi-launch path.
// (SMALL_MAX = 17: mgx_host3d.hpp)
// Who updates which point in a colour pass.  With point t owned by thread t % 1024 the colours alternate from lane to lane
// (every extent is odd), so each pass ran all five slots of a thread with half the lanes off.  Instead slot k of colour c of
// thread t is the (t + 1024 k)-th INTERIOR point of that colour in x-fastest order: two slots per colour cover 17^3 and all
// lanes of a slot work.  The interior extents are odd too, so the m-th interior point has colour (m + 1) & 1.
constexpr int SMALL_CS = (((SMALL_MAX - 2) * (SMALL_MAX - 2) * (SMALL_MAX - 2) + 1) / 2 + 1023) / 1024;  // slots per colour
struct SmallOwn {
    int at[2][SMALL_CS];  // index of the point in the level's LDS array (natural order), -1 = no point
};
__device__ __forceinline__ void small_own(SmallOwn& o, int sx, int sy, int sz) {
    const int mx = sx - 2, mxy = mx * (sy - 2), mn = mxy * (sz - 2), sxy = sx * sy;
    const SmallDiv dxy(mxy), dx(mx);
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
        for (int k = 0; k < SMALL_CS; k++) {
            const int m = 2 * ((int)threadIdx.x + 1024 * k) + ((c + 1) & 1);
            o.at[c][k] = -1;
            if (m < mn) {
                const int iz = dxy(m), iy = dx(m - iz * mxy), ix = m - iz * mxy - iy * mx;
                o.at[c][k] = (iz + 1) * sxy + (iy + 1) * sx + ix + 1;
            }
        }
}
// `ncycles` red-black sweeps of a level held in LDS (sv, sf in natural order); ends with a barrier.  f of the owned points
// stays in registers; the fp32 quotient is formed as in relax3d_point_rd (same bits as the division).
template <class real>
__device__ __forceinline__ void small_relax3(real* sv, const real* sf, int sx, int sxy, const SmallOwn& o, real hx2, real hy2, real hz2,
                                             int ncycles) {
    real fv[2][SMALL_CS];
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
        for (int k = 0; k < SMALL_CS; k++) fv[c][k] = o.at[c][k] >= 0 ? sf[o.at[c][k]] : (real)0;
    const double rd = relax3d_rd<real>(hx2, hy2, hz2);
    auto pass = [&](const int (&at)[SMALL_CS], const real (&ff)[SMALL_CS]) {
#pragma unroll
        for (int k = 0; k < SMALL_CS; k++) {
            const int t = at[k];
            if (t >= 0)
                sv[t] = relax3d_point_rd<real>(sv[t - 1], sv[t + 1], sv[t - sx], sv[t + sx], sv[t - sxy], sv[t + sxy], ff[k], hx2, hy2, hz2, rd);
        }
        __syncthreads();
    };
    for (int c = 0; c < ncycles; c++) {
        pass(o.at[0], fv[0]);  // red = 0 first (N3/MultiGrid3D.cpp:515)
        pass(o.at[1], fv[1]);  // then black (:544)
    }
}

template <class real, class L>
__global__ void __launch_bounds__(1024) relax3d_small_kernel(real* __restrict__ v, const real* __restrict__ f, int sx, int sy,
                                                             int sz, real hx2, real hy2, real hz2, int ncycles) {
    __shared__ real sv[SMALL_MAX * SMALL_MAX * SMALL_MAX];
    __shared__ real sf[SMALL_MAX * SMALL_MAX * SMALL_MAX];
    constexpr int PT = (SMALL_MAX * SMALL_MAX * SMALL_MAX + 1023) / 1024;  // points per thread
    const Geo<L, real> g(sx, sy);
    const int n = sx * sy * sz, sxy = sx * sy;
    size_t gidx[PT];
    bool inner[PT];  // an interior point (written back)
#pragma unroll
    for (int k = 0; k < PT; k++) {
        const int t = threadIdx.x + k * 1024;
        inner[k] = false;
        gidx[k] = 0;
        if (t < n) {
            const int z = SmallDiv(sxy)(t), y = SmallDiv(sx)(t - z * sxy), x = t - z * sxy - y * sx;
            gidx[k] = g.row(y, z) + g.pos(x);
            sv[t] = v[gidx[k]];
            sf[t] = f[gidx[k]];
            inner[k] = x > 0 && x < sx - 1 && y > 0 && y < sy - 1 && z > 0 && z < sz - 1;
        }
    }
    SmallOwn own;
    small_own(own, sx, sy, sz);
    __syncthreads();
    small_relax3<real>(sv, sf, sx, sxy, own, hx2, hy2, hz2, ncycles);
#pragma unroll
    for (int k = 0; k < PT; k++)
        if (inner[k]) v[gidx[k]] = sv[threadIdx.x + k * 1024];
}

// ------------------------------------------------------------------ the whole cycle below 17^3 in one workgroup
// Levels up to 17^3 cost one launch of about 5 us per operator (relax, residual+restrict, fill, correct: 5 launches per
// level and cycle, 20 for the levels 17 ... 3 of the bench hierarchy) although they hold a few thousand points.  Here ONE
// workgroup keeps v and f of every such level in LDS (93 KB in fp64 + a residual scratch of the top level) and runs
// MultiGrid3D::VCycle from the top level of the tail down to the coarsest level and back (N3/MultiGrid3D.cpp:623-647):
// same per-point expressions, same colour order, same operator order -- bit-identical to the launch-per-operator path.
constexpr int TAIL3_MAXLEV = 6;
constexpr int TAIL3_PT = (SMALL_MAX * SMALL_MAX * SMALL_MAX + 1023) / 1024;  // points per thread of a 17^3 level
template <class real>
struct Tail3 {
    int nlev;
    int sx[TAIL3_MAXLEV], sy[TAIL3_MAXLEV], sz[TAIL3_MAXLEV];
    real* v[TAIL3_MAXLEV];
    real* f[TAIL3_MAXLEV];
    real hx[TAIL3_MAXLEV], hy[TAIL3_MAXLEV], hz[TAIL3_MAXLEV];
};

template <class real, class L>
__global__ void __launch_bounds__(1024) cycle3d_tail_kernel(Tail3<real> T, int v1, int v2, int mode, int top_zero) {
    extern __shared__ __align__(16) unsigned char smem3[];
    real* base = (real*)smem3;
    int offv[TAIL3_MAXLEV], offf[TAIL3_MAXLEV];
    int o = 0;
#pragma unroll
    for (int l = 0; l < TAIL3_MAXLEV; l++) {
        const int n = l < T.nlev ? T.sx[l] * T.sy[l] * T.sz[l] : 0;
        offv[l] = o;
        o += n;
        offf[l] = o;
        o += n;
    }
    real* sr = base + o;  // residual of the level being restricted (as large as the top level)
    {   // top level of the tail: v as it stands (or the zeroed error of a coarse level, without reading it), f
        const Geo<L, real> g(T.sx[0], T.sy[0]);
        const int sx = T.sx[0], sxy = T.sx[0] * T.sy[0], n = sxy * T.sz[0];
        const SmallDiv dxy(sxy), dx(sx);
        for (int t = threadIdx.x; t < n; t += 1024) {
            const int z = dxy(t), y = dx(t - z * sxy), x = t - z * sxy - y * sx;
            const size_t gi = g.row(y, z) + g.pos(x);
            base[offv[0] + t] = top_zero ? (real)0 : T.v[0][gi];
            base[offf[0] + t] = T.f[0][gi];
        }
    }
    __syncthreads();
    const int last = T.nlev - 1;
    int kind[TAIL3_PT];
    auto classify = [&](int sx, int sy, int sz) {  // colour of the interior points this thread owns, -1 otherwise
        const int sxy = sx * sy, n = sxy * sz;
        const SmallDiv dxy(sxy), dx(sx);
#pragma unroll
        for (int k = 0; k < TAIL3_PT; k++) {
            const int t = threadIdx.x + k * 1024;
            kind[k] = -1;
            if (t < n) {
                const int z = dxy(t), y = dx(t - z * sxy), x = t - z * sxy - y * sx;
                if (x > 0 && x < sx - 1 && y > 0 && y < sy - 1 && z > 0 && z < sz - 1) kind[k] = (x + y + z) & 1;
            }
        }
    };
    for (int l = 0; l <= last; l++) {  // way down                                            N3/MultiGrid3D.cpp:626-635
        real* sv = base + offv[l];
        real* sf = base + offf[l];
        const int sx = T.sx[l], sy = T.sy[l], sz = T.sz[l], sxy = sx * sy, n = sxy * sz;
        const real hx2 = T.hx[l] * T.hx[l], hy2 = T.hy[l] * T.hy[l], hz2 = T.hz[l] * T.hz[l];  // :498-500
        SmallOwn own;
        small_own(own, sx, sy, sz);
        small_relax3<real>(sv, sf, sx, sxy, own, hx2, hy2, hz2, v1);  // :626
        if (l == last) {
            small_relax3<real>(sv, sf, sx, sxy, own, hx2, hy2, hz2, v2);  // :645 on the coarsest level
            break;
        }
        classify(sx, sy, sz);
#pragma unroll
        for (int k = 0; k < TAIL3_PT; k++) {  // CalculateResidual (:723), 0 on the boundary (:704-705)
            const int t = threadIdx.x + k * 1024;
            if (t < n) {
                real r = (real)0;
                if (kind[k] >= 0) {  // mode | 2: the host found every level's squared spacings to be powers of two (residual3d_point)
                    const real O = sv[t - 1], E = sv[t + 1], N = sv[t - sx], S = sv[t + sx], D = sv[t - sxy], U = sv[t + sxy], c = sv[t], ff = sf[t];
                    switch (mode) {
                        case 0: r = residual3d_point<real, 0>(O, E, N, S, D, U, c, ff, hx2, hy2, hz2); break;
                        case 1: r = residual3d_point<real, 1>(O, E, N, S, D, U, c, ff, hx2, hy2, hz2); break;
                        case 2: r = residual3d_point<real, 2>(O, E, N, S, D, U, c, ff, (real)1 / hx2, (real)1 / hy2, (real)1 / hz2); break;
                        default: r = residual3d_point<real, 3>(O, E, N, S, D, U, c, ff, (real)1 / hx2, (real)1 / hy2, (real)1 / hz2); break;
                    }
                }
                sr[t] = r;
            }
        }
        __syncthreads();
        const int cx = T.sx[l + 1], cy = T.sy[l + 1], cz = T.sz[l + 1], cxy = cx * cy;
        real* cv = base + offv[l + 1];
        real* cf = base + offf[l + 1];
        const SmallDiv dcxy(cxy), dcx(cx);
        for (int t = threadIdx.x; t < cxy * cz; t += 1024) {  // Restrict (:122-180), boundary = injection of a zero residual (:113-119)
            const int pz = dcxy(t), py = dcx(t - pz * cxy), px = t - pz * cxy - py * cx;
            real out = (real)0;
            if (px > 0 && px < cx - 1 && py > 0 && py < cy - 1 && pz > 0 && pz < cz - 1) {
                const real* c = sr + 2 * px + 2 * py * sx + 2 * pz * sxy;
                out = restrict3d_point<real>([&](int dx, int dy, int dz) { return c[dx + dy * sx + dz * sxy]; });
            }
            cf[t] = out;
            cv[t] = (real)0;  // setToValue(coarse v, 0, true)   :634
        }
        __syncthreads();
    }
    for (int l = last - 1; l >= 0; l--) {  // way up                                          N3/MultiGrid3D.cpp:638-645
        real* sv = base + offv[l];
        real* sf = base + offf[l];
        const real* c = base + offv[l + 1];
        const int sx = T.sx[l], sy = T.sy[l], sz = T.sz[l], sxy = sx * sy;
        const int cx = T.sx[l + 1], cxy = cx * T.sy[l + 1];
        const real hx2 = T.hx[l] * T.hx[l], hy2 = T.hy[l] * T.hy[l], hz2 = T.hz[l] * T.hz[l];
        classify(sx, sy, sz);
        const SmallDiv dxy(sxy), dx(sx);
#pragma unroll
        for (int k = 0; k < TAIL3_PT; k++)
            if (kind[k] >= 0) {  // Interpolate into the error, ApplyCorrection (:216-329, :672)
                const int t = threadIdx.x + k * 1024;
                const int z = dxy(t), y = dx(t - z * sxy), x = t - z * sxy - y * sx;
                const real* cc = c + (x >> 1) + (y >> 1) * cx + (z >> 1) * cxy;
                const real e = interpolate3d_point<real>(x & 1, y & 1, z & 1, [&](int dx, int dy, int dz) { return cc[dx + dy * cx + dz * cxy]; });
                sv[t] = sv[t] + e;
            }
        __syncthreads();
        SmallOwn own;
        small_own(own, sx, sy, sz);
        small_relax3<real>(sv, sf, sx, sxy, own, hx2, hy2, hz2, v2);  // :645
    }
    // what the launch-per-operator path leaves behind: v of every level, the restricted residual in f below the top
    for (int l = 0; l <= last; l++) {
        const Geo<L, real> g(T.sx[l], T.sy[l]);
        const int sx = T.sx[l], sxy = T.sx[l] * T.sy[l], n = sxy * T.sz[l];
        const SmallDiv dxy(sxy), dx(sx);
        for (int t = threadIdx.x; t < n; t += 1024) {
            const int z = dxy(t), y = dx(t - z * sxy), x = t - z * sxy - y * sx;
            const size_t gi = g.row(y, z) + g.pos(x);
            T.v[l][gi] = base[offv[l] + t];
            if (l > 0) T.f[l][gi] = base[offf[l] + t];
        }
    }
}

// =========================================================================== host side
// all `ncycles` sweeps of a level that fits (relax3d has asked SMALL_MAX and "relax3d.small")
template <class real, class L>
int relax3d_small(mgx_ctx* ctx, real* v, const real* f, const int n[3], real hx2, real hy2, real hz2, int ncycles) {
    MGX_LAUNCH((relax3d_small_kernel<real, L>), dim3(1), dim3(1024), 0, ctx->compute, v, f, n[0], n[1], n[2], hx2, hy2,
                       hz2, ncycles);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// levels[0 .. nlev) of a hierarchy (the top level of the tail first), each at most 17 points per axis; n = {sx0, sy0,
// sz0, sx1, ...}, h likewise; v / f are HOST arrays of device pointers in layout L
static bool tail3_fits(int nlev, const int* n, size_t elem) {
    if (!n || nlev < 1 || nlev > TAIL3_MAXLEV) return false;
    size_t e = (size_t)n[0] * n[1] * n[2];
    for (int l = 0; l < nlev; l++) {
        if (n[3 * l] > SMALL_MAX || n[3 * l + 1] > SMALL_MAX || n[3 * l + 2] > SMALL_MAX) return false;
        e += (size_t)2 * n[3 * l] * n[3 * l + 1] * n[3 * l + 2];
    }
    return e * elem <= 150 * 1024;
}

template <class real, class L>
int cycle3d_tail(mgx_ctx* ctx, int nlev, real* const* v, real* const* f, const int* n, const real* h, int v1, int v2, int mode,
                 int top_zero) {
    MGX_REQUIRE(ctx && v && f && n && h, MGX_ERR_INVALID, "vcycle_tail3d: NULL argument");
    MGX_USE(ctx);
    MGX_REQUIRE(v1 >= 0 && v2 >= 0, MGX_ERR_INVALID, "vcycle_tail3d: negative sweep count");
    MGX_REQUIRE(mode == MGX_RESIDUAL_REF_COMPAT || mode == MGX_RESIDUAL_CORRECT, MGX_ERR_INVALID, "vcycle_tail3d: bad mode %d", mode);
    MGX_REQUIRE(tail3_fits(nlev, n, sizeof(real)), MGX_ERR_SIZE, "vcycle_tail3d: the levels do not fit (at most %d levels of at most %d^3)",
                TAIL3_MAXLEV, SMALL_MAX);
    Tail3<real> T;
    memset(&T, 0, sizeof T);
    T.nlev = nlev;
    size_t elems = (size_t)n[0] * n[1] * n[2];
    for (int l = 0; l < nlev; l++) {
        const int* nl = n + 3 * l;
        int st = check_n3(nl, "vcycle_tail3d");
        if (st) return st;
        if (l > 0) {
            st = check_coarse3(n + 3 * (l - 1), nl, "vcycle_tail3d");
            if (st) return st;
        }
        MGX_REQUIRE(v[l] && f[l], MGX_ERR_INVALID, "vcycle_tail3d: NULL level array");
        T.sx[l] = nl[0]; T.sy[l] = nl[1]; T.sz[l] = nl[2];
        T.v[l] = v[l]; T.f[l] = f[l];
        T.hx[l] = h[3 * l]; T.hy[l] = h[3 * l + 1]; T.hz[l] = h[3 * l + 2];
        elems += (size_t)2 * nl[0] * nl[1] * nl[2];
    }
    const size_t lds = elems * sizeof(real);
    if (lds > 64 * 1024)
        MGX_HIP(hipFuncSetAttribute((const void*)cycle3d_tail_kernel<real, L>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    bool rcp = ctx->rr_rcp != 0;  // residual_scale's rule, on every level
    for (int l = 0; l < nlev && rcp; l++) rcp = exact_reciprocals(h + 3 * l);
    MGX_LAUNCH((cycle3d_tail_kernel<real, L>), dim3(1), dim3(1024), lds, ctx->compute, T, v1, v2, mode | (rcp ? 2 : 0), top_zero);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

#define MGX_X(real, L) template int relax3d_small<real, L>(mgx_ctx*, real*, const real*, const int[3], real, real, real, int);
MGX_X(float, Natural) MGX_X(double, Natural) MGX_X(float, XSplit) MGX_X(double, XSplit)
#undef MGX_X

}  // namespace mgx

#define MGX_DEFINE_OPS3D(PFX, L, SFX, real)                                                                      \
    int PFX##vcycle_tail_##SFX(mgx_ctx* ctx, int nlev, real* const* v, real* const* f, const int* n,             \
                               const real* h, int v1, int v2, int mode, int top_zero) {                          \
        return mgx::cycle3d_tail<real, L>(ctx, nlev, v, f, n, h, v1, v2, mode, top_zero);                        \
    }                                                                                                            \
    int PFX##vcycle_tail_fits_##SFX(const mgx_ctx* ctx, int nlev, const int* n) {                                \
        return ctx && ctx->relax_small && mgx::tail3_fits(nlev, n, sizeof(real));                                \
    }

extern "C" {
MGX_DEFINE_OPS3D(mgx3d_, mgx::Natural, f32, float)
MGX_DEFINE_OPS3D(mgx3d_, mgx::Natural, f64, double)
MGX_DEFINE_OPS3D(mgx3dxs_, mgx::XSplit, f32, float)
MGX_DEFINE_OPS3D(mgx3dxs_, mgx::XSplit, f64, double)
}
