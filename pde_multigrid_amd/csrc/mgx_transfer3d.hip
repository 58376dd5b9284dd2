// mgx_transfer3d.hip -- the transfers between levels, the fills and the reductions of the 3D hierarchy, both layouts
// (mgx_kernels3d.hpp), with their z-slab forms.  Per-point expressions in the reference's association order: bit-identical.
//
// Kernels (reference function each one replaces):
//   residual3d_kernel         MultiGrid3D::CalculateResidual          N3/MultiGrid3D.cpp:678-730
//   restrict3d_kernel         MultiGrid3D::Restrict                   N3/MultiGrid3D.cpp:50-184
//   interpolate3d_kernel      MultiGrid3D::Interpolate (+ApplyCorrection when ADD)
//                                                                     N3/MultiGrid3D.cpp:186-335, 649-676
//   correct3d_kernel          MultiGrid3D::ApplyCorrection            N3/MultiGrid3D.cpp:649-676
//   set3d_kernel              MultiGrid3D::setToValue                 N3/MultiGrid3D.cpp:587-621
//   init_f3d_kernel           Grid3D::InitF                           N3/Grid3D.cpp:78-96
//   (CalculateResidual + Restrict fused, no residual array: mgx_rr3d.hip)
//   interpolate3d_xs_kernel   Interpolate (+ApplyCorrection, optionally one colour only), XSplit
//   correct_pset3d_xs_kernel  the correction of the tile-edge cells of the correcting red pass (mgx_pipe3d.hip); shares
//                             interp_cell_xs with interpolate3d_xs_kernel, so the two stay in one unit
//   relayout3d_kernel         Natural <-> XSplit (upload / download of the hierarchy)
//   sumsq_kernel, residual_sumsq3d_kernel, residual_sumsq_final_kernel, diff_stats3d_kernel   norms and Grid3D::PrintDiff
#include "mgx_host3d.hpp"

namespace mgx {

// ------------------------------------------------------------------ diagnostics (PrintDiff as a reduction)
// diff = realSol - approxSol with realSol = (real)(sin(PI x) sin(PI y) sin(PI z)) from host sin tables
// (Grid3D::PrintDiff, N3/Grid3D.cpp:136-159, writes one text line per point; here the three usual norms are
// reduced on the device: out[0] = sum |diff|, out[1] = max |diff| (as the bit pattern of a non-negative double),
// out[2] = sum diff^2, out[3] = sum realSol^2.
template <class real, class L>
__global__ void __launch_bounds__(256) diff_stats3d_kernel(const real* __restrict__ v, int sx, int sy, int sz,
                                                           const double* __restrict__ tx, const double* __restrict__ ty,
                                                           const double* __restrict__ tz, double* __restrict__ out) {
    const Geo<L, real> g(sx, sy);
    const int y = blockIdx.y, z = blockIdx.z;
    double s1 = 0, mx = 0, s2 = 0, sr = 0;
    for (int x = threadIdx.x; x < sx; x += blockDim.x) {
        const real realSol = (real)(tx[x] * ty[y] * tz[z]);
        const real diff = realSol - v[g.row(y, z) + g.pos(x)];
        const double a = fabs((double)diff);
        s1 += a;
        mx = a > mx ? a : mx;
        s2 += (double)diff * (double)diff;
        sr += (double)realSol * (double)realSol;
    }
    for (int off = 32; off > 0; off >>= 1) {  // wavefront-wide reduction
        s1 += __shfl_down(s1, off, 64);
        s2 += __shfl_down(s2, off, 64);
        sr += __shfl_down(sr, off, 64);
        const double o = __shfl_down(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    __shared__ double p1[4], p2[4], p3[4], pm[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { p1[wave] = s1; p2[wave] = s2; p3[wave] = sr; pm[wave] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        double a = 0, b = 0, c = 0, m = 0;
        for (int w = 0; w < nw; w++) { a += p1[w]; b += p2[w]; c += p3[w]; m = pm[w] > m ? pm[w] : m; }
        atomicAdd(out + 0, a);
        atomicMax((unsigned long long*)(out + 1), (unsigned long long)__double_as_longlong(m));
        atomicAdd(out + 2, b);
        atomicAdd(out + 3, c);
    }
}

// ------------------------------------------------------------------ residual
template <class real, class L, int MODE>
__global__ void __launch_bounds__(256) residual3d_kernel(const real* __restrict__ v, const real* __restrict__ f,
                                                         real* __restrict__ r, int sx, int sy, int sz, real hx2,
                                                         real hy2, real hz2) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    const int z = blockIdx.z;
    if (x >= sx || y >= sy) return;
    const Geo<L, real> g(sx, sy);
    const int H = g.H, P = g.P;
    const size_t sxy = g.PL;
    const size_t row = g.row(y, z);
    const size_t i = row + L::pos(x, H);
    if (x == 0 || x == sx - 1 || y == 0 || y == sy - 1 || z == 0 || z == sz - 1) {
        r[i] = (real)0;  // N3/MultiGrid3D.cpp:704-705
        return;
    }
    r[i] = residual3d_point<real, MODE>(v[row + L::pos(x - 1, H)], v[row + L::pos(x + 1, H)], v[i - P], v[i + P],
                                        v[i - sxy], v[i + sxy], v[i], f[i], hx2, hy2, hz2);
}

// ------------------------------------------------------------------ restrict
template <class real, class L>
__global__ void __launch_bounds__(256) restrict3d_kernel(const real* __restrict__ fine, int fx, int fy,
                                                         real* __restrict__ coarse, int cx, int cy, int cz, int fzoff,
                                                         int czoff, int pzbeg) {
    // z-slab form: cz = GLOBAL coarse planes; `fine` / `coarse` start at global planes fzoff / czoff; this launch covers
    // the global coarse planes pzbeg + blockIdx.z (whole grid: all three are 0)
    const int px = blockIdx.x * blockDim.x + threadIdx.x;
    const int py = blockIdx.y * blockDim.y + threadIdx.y;
    const int pz = pzbeg + blockIdx.z;
    if (px >= cx || py >= cy) return;
    const Geo<L, real> gf(fx, fy), gc(cx, cy);
    const int FH = gf.H;
    const size_t ci = gc.pos(px) + gc.row(py, pz - czoff);
    const real* c = fine + gf.row(2 * py, 2 * pz - fzoff);  // row base of the fine centre
    const int gx = 2 * px;
    if (px == 0 || px == cx - 1 || py == 0 || py == cy - 1 || pz == 0 || pz == cz - 1) {
        coarse[ci] = c[L::pos(gx, FH)];  // injection, N3/MultiGrid3D.cpp:113-119
        return;
    }
    const ptrdiff_t sy_ = gf.P, sz_ = (ptrdiff_t)gf.PL;
    coarse[ci] = restrict3d_point<real>([&](int dx, int dy, int dz) { return c[L::pos(gx + dx, FH) + dy * sy_ + dz * sz_]; });
}

// ------------------------------------------------------------------ interpolate (+ correct)
// ADD = false: fine = I(coarse) on the interior        (Interpolate)
// ADD = true : fine = fine + I(coarse) on the interior (Interpolate into a scratch error
//              array followed by ApplyCorrection, N3/MultiGrid3D.cpp:638-642, fused)
template <class real, class L, bool ADD>
__global__ void __launch_bounds__(256) interpolate3d_kernel(real* __restrict__ fine, int fx, int fy, int fz,
                                                            const real* __restrict__ coarse, int cx, int cy) {
    const int x = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int y = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int z = 1 + blockIdx.z;
    if (x >= fx - 1 || y >= fy - 1 || z >= fz - 1) return;
    const Geo<L, real> gf(fx, fy), gc(cx, cy);
    const int CH = gc.H;
    const size_t cxy = gc.PL;
    const size_t fi = gf.pos(x) + gf.row(y, z);
    const real* c = coarse + gc.row(y >> 1, z >> 1);
    const int gx = x >> 1;
    const real e = interpolate3d_point<real>(
        x & 1, y & 1, z & 1, [&](int dx, int dy, int dz) { return c[L::pos(gx + dx, CH) + (size_t)dy * gc.P + (size_t)dz * cxy]; });
    if (ADD) fine[fi] = fine[fi] + e;  // N3/MultiGrid3D.cpp:672
    else fine[fi] = e;
}

// XSplit form: one thread per coarse cell (i, py, pz) produces the 2 x 2 x 2 fine points
// (2i | 2i+1, 2py | 2py+1, 2pz | 2pz+1) from the 8 coarse values c[i..i+1][py..py+1][pz..pz+1] it loads once.
// Fine accesses are contiguous per half-row (lane i -> even half index i and odd half index i); the
// parity class of every point is a compile-time constant after unrolling, so there is no divergence.
// Slab form: pz = pzbeg + blockIdx.z is a GLOBAL coarse plane; the fine / coarse arrays start at global
// planes fzoff / czoff (0 for whole grids).  The host passes only pz whose fine planes 2pz, 2pz+1 are
// owned and interior-or-skipped (z = 0 is skipped here, z <= fz-2 follows from pz <= cz-2).
// COLOUR >= 0: only the fine points with (x + y + z) % 2 == COLOUR are written (the half-row of that parity in
// every row).  The cycle uses COLOUR = 1 when a red-black sweep follows: the red pass overwrites every red interior
// point from black neighbours only, so a corrected red value would never be read.
// [zmin, zmax): the global fine planes that may be written (a slab's ghost planes: the cell's other plane, and the coarse
// plane only it needs, may lie outside the local arrays)
template <class real, bool ADD, int COLOUR>
__device__ __forceinline__ void interp_cell_xs(real* __restrict__ fine, const Geo<XSplit, real>& gf, int fzoff,
                                               const real* __restrict__ coarse, const Geo<XSplit, real>& gc, int czoff, int i, int py,
                                               int pz, int zmin = 1, int zmax = 0x7fffffff) {
    const int FH = gf.H, CH = gc.H;
    const size_t cxy = gc.PL, fxy = gf.PL;
    real c[2][2][2];
#pragma unroll
    for (int dz = 0; dz < 2; dz++)
#pragma unroll
        for (int dy = 0; dy < 2; dy++)
#pragma unroll
            for (int dx = 0; dx < 2; dx++)
                c[dx][dy][dz] = (dz == 0 || 2 * pz + 1 < zmax)
                                    ? coarse[XSplit::pos(i + dx, CH) + (size_t)(py + dy) * gc.P + (size_t)(pz + dz - czoff) * cxy]
                                    : (real)0;
    auto get = [&](int dx, int dy, int dz) { return c[dx][dy][dz]; };
#pragma unroll
    for (int dz = 0; dz < 2; dz++) {
        const int z = 2 * pz + dz;
        if (z < 1 || z < zmin || z >= zmax) continue;
#pragma unroll
        for (int dy = 0; dy < 2; dy++) {
            const int y = 2 * py + dy;
            if (y < 1) continue;
            const size_t row = (size_t)y * gf.P + (size_t)(z - fzoff) * fxy;
            if (COLOUR < 0 || ((COLOUR + dy + dz) & 1) == 0) {  // x = 2i
                const real e0 = interpolate3d_point<real>(0, dy, dz, get);
                if (i >= 1) fine[row + i] = ADD ? fine[row + i] + e0 : e0;
            }
            if (COLOUR < 0 || ((COLOUR + dy + dz) & 1) == 1) {  // x = 2i+1
                const real e1 = interpolate3d_point<real>(1, dy, dz, get);
                fine[row + FH + i] = ADD ? fine[row + FH + i] + e1 : e1;
            }
        }
    }
}

template <class real, bool ADD, int COLOUR = -1>
__global__ void __launch_bounds__(256) interpolate3d_xs_kernel(real* __restrict__ fine, int fx, int fy, int fzoff,
                                                               const real* __restrict__ coarse, int cx, int cy, int czoff,
                                                               int pzbeg) {
    const Geo<XSplit, real> gf(fx, fy), gc(cx, cy);
    const int i = blockIdx.x * 64 + threadIdx.x;
    const int py = blockIdx.y * blockDim.y + threadIdx.y;
    const int pz = pzbeg + blockIdx.z;
    if (i >= ((fx + 1) >> 1) - 1 || py >= cy - 1) return;  // fine x = 2i+1 <= fx-2, fine y = 2py+1 <= fy-2
    interp_cell_xs<real, ADD, COLOUR>(fine, gf, fzoff, coarse, gc, czoff, i, py, pz);
}

// The set P of relax3d_xs_pipe_kernel<.., VAR = 2>: black points of the coarse cells (i, py, pz) with py % PH == 0 (part 0:
// the two fine rows a workgroup tile of the correcting pass sees just outside itself and, from the neighbouring tile's
// point of view, its own first / last row) or i % PW in {0, PW - 1}, i > 0 (part 1: the pairs next to a tile's left /
// right edge; cells of part 0 are skipped there) get v += Interpolate(coarse) in place before the pass runs.
// Slab form: fine / coarse are local arrays starting at the global planes fzoff / czoff, the cells pzbeg ... are visited and
// only the global fine planes [zmin, zmax) are written.
template <class real>
__global__ void __launch_bounds__(256) correct_pset3d_xs_kernel(real* __restrict__ fine, int fx, int fy, const real* __restrict__ coarse,
                                                                int cx, int cy, int PW, int PH, int part, int fzoff = 0, int czoff = 0,
                                                                int pzbeg = 0, int zmin = 1, int zmax = 0x7fffffff) {
    const Geo<XSplit, real> gf(fx, fy), gc(cx, cy);
    const int M = (fx + 1) >> 1;
    const int pz = pzbeg + blockIdx.z;
    int i, py;
    if (part == 0) {
        i = blockIdx.x * 64 + threadIdx.x;
        py = (blockIdx.y * blockDim.y + threadIdx.y) * PH;
    } else {
        const int c = blockIdx.x;  // column group c >> 1 (1, 2, ...), its pair PW g - 1 (c even) or PW g (c odd)
        i = ((c >> 1) + 1) * PW - 1 + (c & 1);
        py = blockIdx.y * 256 + threadIdx.y * 64 + threadIdx.x;
        if (py % PH == 0) return;
    }
    if (i >= M - 1 || py >= cy - 1) return;
    interp_cell_xs<real, true, 1>(fine, gf, fzoff, coarse, gc, czoff, i, py, pz, zmin, zmax);
}

template <class real, class L>
__global__ void __launch_bounds__(256) correct3d_kernel(real* __restrict__ fine, const real* __restrict__ err, int sx,
                                                        int sy, int sz) {
    const int x = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int y = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int z = 1 + blockIdx.z;
    if (x >= sx - 1 || y >= sy - 1 || z >= sz - 1) return;
    const Geo<L, real> g(sx, sy);
    const size_t i = g.pos(x) + g.row(y, z);
    fine[i] = fine[i] + err[i];
}

template <class real, class L>
__global__ void __launch_bounds__(256) set3d_kernel(real* __restrict__ g, int sx, int sy, int sz, real value, int lo) {
    const int x = lo + blockIdx.x * blockDim.x + threadIdx.x;
    const int y = lo + blockIdx.y * blockDim.y + threadIdx.y;
    const int z = lo + blockIdx.z;
    if (x >= sx - lo || y >= sy - lo || z >= sz - lo) return;
    const Geo<L, real> ge(sx, sy);
    g[ge.pos(x) + ge.row(y, z)] = value;
}

// f = (real)(((c * tx[x]) * ty[y]) * tz[z]) in double: Grid3D::InitF's left-to-right product
// -3*PI*PI*sin(PI*x)*sin(PI*y)*sin(PI*z) with the three sines tabulated on the host.
template <class real, class L>
__global__ void __launch_bounds__(256) init_f3d_kernel(real* __restrict__ f, int sx, int sy, int sz, double c,
                                                       const double* __restrict__ tx, const double* __restrict__ ty,
                                                       const double* __restrict__ tz) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    const int z = blockIdx.z;
    if (x >= sx || y >= sy) return;
    const Geo<L, real> g(sx, sy);
    f[g.pos(x) + g.row(y, z)] = (real)(c * tx[x] * ty[y] * tz[z]);
}

// dst(layout LD) = src(layout LS), same sizes
template <class real, class LS, class LD>
__global__ void __launch_bounds__(256) relayout3d_kernel(const real* __restrict__ src, real* __restrict__ dst, int sx, int sy) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    const int z = blockIdx.z;
    if (x >= sx || y >= sy) return;
    const Geo<LS, real> gs(sx, sy);
    const Geo<LD, real> gd(sx, sy);
    dst[gd.row(y, z) + gd.pos(x)] = src[gs.row(y, z) + gs.pos(x)];
}

// ------------------------------------------------------------------ sum of squares
template <class real>
__global__ void __launch_bounds__(256) sumsq_kernel(const real* __restrict__ x, size_t count, double* __restrict__ out) {
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        const double t = (double)x[i];
        acc += t * t;
    }
    // wavefront-wide (64 lanes) shuffle reduction, then one LDS hop across the 4 waves
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    __shared__ double part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, (part[0] + part[1]) + (part[2] + part[3]));
}

// ------------------------------------------------------------------ sum of squares of the residual (no residual array)
// One block per row (y, z) of the planes [zbeg, zend): the residual of its interior points is squared and summed in
// double -- wavefront-wide shuffle reduction, the waves of the block combined in a fixed order -- into
// partial[row]; residual_sumsq_final_kernel then adds the partials in a fixed order, so the result does not depend
// on scheduling (same bits on every run and, after the all-reduce, on every rank).  An addition: the reference has no
// norm.
template <class real, class L, int MODE>
__global__ void __launch_bounds__(256) residual_sumsq3d_kernel(const real* __restrict__ v, const real* __restrict__ f, int sx,
                                                               int sy, int zbeg, real hx2, real hy2, real hz2,
                                                               double* __restrict__ partial) {
    const Geo<L, real> g(sx, sy);
    const int y = 1 + blockIdx.x, z = zbeg + blockIdx.y;
    const int H = g.H, P = g.P;
    const size_t sxy = g.PL, row = g.row(y, z);
    double acc = 0.0;
    for (int x = 1 + threadIdx.x; x < sx - 1; x += 256) {
        const size_t i = row + L::pos(x, H);
        const real r = residual3d_point<real, MODE>(v[row + L::pos(x - 1, H)], v[row + L::pos(x + 1, H)], v[i - P], v[i + P],
                                                    v[i - sxy], v[i + sxy], v[i], f[i], hx2, hy2, hz2);
        acc += (double)r * (double)r;
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    __shared__ double part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ void __launch_bounds__(1024) residual_sumsq_final_kernel(const double* __restrict__ partial, size_t count,
                                                                    double* __restrict__ out) {
    __shared__ double s[1024];
    double acc = 0.0;
    for (size_t i = threadIdx.x; i < count; i += 1024) acc += partial[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s[0];
}

// =========================================================================== host side
template <class real, class L>
int residual3d(mgx_ctx* ctx, const real* v, const real* f, real* r, const int n[3], const real h[3], int mode) {
    MGX_REQUIRE(ctx && v && f && r && h, MGX_ERR_INVALID, "residual3d: NULL argument");
    MGX_USE(ctx);
    int st = check_n3(n, "residual3d");
    if (st) return st;
    MGX_REQUIRE(mode == MGX_RESIDUAL_REF_COMPAT || mode == MGX_RESIDUAL_CORRECT, MGX_ERR_INVALID, "residual3d: bad mode %d", mode);
    const ResidualScale<real> s = residual_scale<real>(ctx, h, mode);
    with_value<0, 1, 2, 3>(s.mode, [&](auto m) __attribute__((always_inline)) {
        MGX_LAUNCH((residual3d_kernel<real, L, decltype(m)::value>), grd(n[0], n[1], n[2]), blk(), 0, ctx->compute, v, f, r, n[0], n[1],
                   n[2], s.qx, s.qy, s.qz);
    });
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

template <class real, class L>
int restrict3d(mgx_ctx* ctx, const real* fine, const int fn[3], real* coarse, const int cn[3]) {
    MGX_REQUIRE(ctx && fine && coarse, MGX_ERR_INVALID, "restrict3d: NULL argument");
    MGX_USE(ctx);
    int st = check_n3(fn, "restrict3d");
    if (st) return st;
    st = check_coarse3(fn, cn, "restrict3d");
    if (st) return st;
    MGX_LAUNCH((restrict3d_kernel<real, L>), grd(cn[0], cn[1], cn[2]), blk(), 0, ctx->compute, fine, fn[0], fn[1],
                       coarse, cn[0], cn[1], cn[2], 0, 0, 0);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// Restrict on a z-slab: the global coarse planes [pzbeg, pzend); fine planes 2pz-1 .. 2pz+1 must be present in `fine`
template <class real>
int restrict3d_slab(mgx_ctx* ctx, const real* fine, const int fn[3], int fzoff, real* coarse, const int cn[3], int czoff,
                    int pzbeg, int pzend) {
    MGX_REQUIRE(ctx && fine && coarse, MGX_ERR_INVALID, "restrict_slab: NULL argument");
    MGX_USE(ctx);
    int st = check_n3(fn, "restrict_slab");
    if (st) return st;
    st = check_coarse3(fn, cn, "restrict_slab");
    if (st) return st;
    MGX_REQUIRE(pzbeg >= 0 && pzend <= cn[2] && pzbeg <= pzend && fzoff >= 0 && czoff >= 0 && czoff <= pzbeg, MGX_ERR_INVALID,
                "restrict_slab: bad plane range");
    if (pzbeg == pzend) return MGX_OK;
    MGX_LAUNCH((restrict3d_kernel<real, XSplit>), grd(cn[0], cn[1], pzend - pzbeg), blk(), 0, ctx->compute, fine, fn[0],
                       fn[1], coarse, cn[0], cn[1], cn[2], fzoff, czoff, pzbeg);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

template <class real, class L, bool ADD>
int interpolate3d(mgx_ctx* ctx, real* fine, const int fn[3], const real* coarse, const int cn[3]) {
    MGX_REQUIRE(ctx && fine && coarse, MGX_ERR_INVALID, "interpolate3d: NULL argument");
    MGX_USE(ctx);
    int st = check_n3(fn, "interpolate3d");
    if (st) return st;
    st = check_coarse3(fn, cn, "interpolate3d");
    if (st) return st;
    if (L::xsplit)
        MGX_LAUNCH((interpolate3d_xs_kernel<real, ADD>), grd((fn[0] + 1) / 2 - 1, cn[1] - 1, cn[2] - 1), blk(), 0,
                           ctx->compute, fine, fn[0], fn[1], 0, coarse, cn[0], cn[1], 0, 0);
    else
        MGX_LAUNCH((interpolate3d_kernel<real, L, ADD>), grd(fn[0] - 2, fn[1] - 2, fn[2] - 2), blk(), 0, ctx->compute,
                           fine, fn[0], fn[1], fn[2], coarse, cn[0], cn[1]);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

template <class real, class L>
int correct3d(mgx_ctx* ctx, real* fine, const int fn[3], const real* err, const int en[3]) {
    MGX_REQUIRE(ctx && fine && err && en, MGX_ERR_INVALID, "apply_correction3d: NULL argument");
    MGX_USE(ctx);
    int st = check_n3(fn, "apply_correction3d");
    if (st) return st;
    for (int d = 0; d < 3; d++)  // N3/MultiGrid3D.cpp:660-662
        MGX_REQUIRE(fn[d] == en[d], MGX_ERR_SIZE, "apply_correction3d: size[%d] %d != %d", d, fn[d], en[d]);
    MGX_LAUNCH((correct3d_kernel<real, L>), grd(fn[0] - 2, fn[1] - 2, fn[2] - 2), blk(), 0, ctx->compute, fine, err,
                       fn[0], fn[1], fn[2]);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

template <class real, class L>
int set3d(mgx_ctx* ctx, real* g, const int n[3], real value, int modify_boundaries) {
    MGX_REQUIRE(ctx && g, MGX_ERR_INVALID, "set3d: NULL argument");
    MGX_USE(ctx);
    int st = check_n3(n, "set3d");
    if (st) return st;
    const int lo = modify_boundaries ? 0 : 1;
    if (modify_boundaries && value == (real)0 && !std::signbit(value)) {
        // the cycle's "coarse v := 0" (N3/MultiGrid3D.cpp:634): +0.0 is all-zero bits, the pad entries of the x-split
        // layout are zero by invariant -> one fill of the whole array at memset speed
        const size_t elems = Geo<L, real>(n[0], n[1]).PL * (size_t)n[2];  // natural layout: PL = n[0] * n[1]
        return fill_zero(ctx, g, elems * sizeof(real));
    }
    MGX_LAUNCH((set3d_kernel<real, L>), grd(n[0] - 2 * lo, n[1] - 2 * lo, n[2] - 2 * lo), blk(), 0, ctx->compute, g,
                       n[0], n[1], n[2], value, lo);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// setToValue(grid, value, false) on the local planes [zbeg, zend) of an x-split slab: their (x, y)-interior points
template <class real>
int set3d_slab(mgx_ctx* ctx, real* g, int sx, int sy, int zbeg, int zend, real value) {
    MGX_REQUIRE(ctx && g, MGX_ERR_INVALID, "set_slab: NULL argument");
    MGX_USE(ctx);
    MGX_REQUIRE(valid_size(sx) && valid_size(sy) && zbeg >= 0 && zend >= zbeg, MGX_ERR_SIZE, "set_slab: bad sizes");
    if (zend == zbeg) return MGX_OK;
    // set3d_kernel with lo = 1 writes the planes 1 .. sz-2 of the array it is given: hand it the planes zbeg-1 .. zend
    const Geo<XSplit, real> ge(sx, sy);
    MGX_LAUNCH((set3d_kernel<real, XSplit>), grd(sx - 2, sy - 2, zend - zbeg), blk(), 0, ctx->compute,
                       g + ge.PL * (size_t)zbeg - ge.PL, sx, sy, zend - zbeg + 2, value, 1);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

template <class real, class L>
int init_f3d(mgx_ctx* ctx, real* f, const int n[3], double c, const double* tx, const double* ty, const double* tz) {
    MGX_REQUIRE(ctx && f && tx && ty && tz, MGX_ERR_INVALID, "init_f3d: NULL argument");
    MGX_USE(ctx);
    int st = check_n3(n, "init_f3d");
    if (st) return st;
    const size_t cnt = (size_t)n[0] + n[1] + n[2];
    void* ws = nullptr;
    st = workspace(ctx, cnt * sizeof(double), &ws);
    if (st) return st;
    double* d = (double*)ws;
    MGX_HIP(hipMemcpyAsync(d, tx, n[0] * sizeof(double), hipMemcpyHostToDevice, ctx->compute));
    MGX_HIP(hipMemcpyAsync(d + n[0], ty, n[1] * sizeof(double), hipMemcpyHostToDevice, ctx->compute));
    MGX_HIP(hipMemcpyAsync(d + n[0] + n[1], tz, n[2] * sizeof(double), hipMemcpyHostToDevice, ctx->compute));
    MGX_LAUNCH((init_f3d_kernel<real, L>), grd(n[0], n[1], n[2]), blk(), 0, ctx->compute, f, n[0], n[1], n[2], c, d,
                       d + n[0], d + n[0] + n[1]);
    MGX_LAUNCH_CHECK();
    MGX_HIP(hipStreamSynchronize(ctx->compute));  // host tables may be freed by the caller
    return MGX_OK;
}

template <class real, class LS, class LD>
int relayout3d(mgx_ctx* ctx, const real* src, real* dst, const int n[3]) {
    MGX_REQUIRE(ctx && src && dst, MGX_ERR_INVALID, "relayout3d: NULL argument");
    MGX_USE(ctx);
    MGX_REQUIRE(src != dst, MGX_ERR_INVALID, "relayout3d: in-place conversion is not supported");
    int st = check_n3(n, "relayout3d");
    if (st) return st;
    MGX_LAUNCH((relayout3d_kernel<real, LS, LD>), grd(n[0], n[1], n[2]), blk(), 0, ctx->compute, src, dst, n[0], n[1]);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// sum over the (x, y)-interior points of the local planes [zbeg, zend) of the squared residual -> *dev_out (a device
// double), asynchronously on the compute stream; the planes zbeg-1 and zend must hold valid v (ghosts / boundary)
template <class real>
int residual_sumsq3d_slab(mgx_ctx* ctx, const real* v, const real* f, int sx, int sy, const real h[3], int mode, int zbeg,
                          int zend, double* dev_out) {
    MGX_REQUIRE(ctx && v && f && h && dev_out, MGX_ERR_INVALID, "residual_sumsq_slab: NULL argument");
    MGX_USE(ctx);
    MGX_REQUIRE(valid_size(sx) && valid_size(sy), MGX_ERR_SIZE, "residual_sumsq_slab: sizes %d x %d are not odd and >= 3", sx, sy);
    MGX_REQUIRE(zbeg >= 1 && zend >= zbeg, MGX_ERR_INVALID, "residual_sumsq_slab: bad plane range");
    MGX_REQUIRE(mode == MGX_RESIDUAL_REF_COMPAT || mode == MGX_RESIDUAL_CORRECT, MGX_ERR_INVALID, "bad residual mode %d", mode);
    if (zend == zbeg) {
        MGX_HIP(hipMemsetAsync(dev_out, 0, sizeof(double), ctx->compute));
        return MGX_OK;
    }
    const ResidualScale<real> s = residual_scale<real>(ctx, h, mode);
    const size_t rows = (size_t)(sy - 2) * (size_t)(zend - zbeg);
    void* ws = nullptr;
    MGX_TRY_RET(workspace(ctx, rows * sizeof(double), &ws));
    const dim3 g(sy - 2, zend - zbeg);
    with_value<0, 1, 2, 3>(s.mode, [&](auto m) __attribute__((always_inline)) {
        MGX_LAUNCH((residual_sumsq3d_kernel<real, XSplit, decltype(m)::value>), g, dim3(256), 0, ctx->compute, v, f, sx, sy, zbeg, s.qx,
                   s.qy, s.qz, (double*)ws);
    });
    MGX_LAUNCH(residual_sumsq_final_kernel, dim3(1), dim3(1024), 0, ctx->compute, (const double*)ws, rows, dev_out);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

template <class real>
int interpolate_correct3d_slab(mgx_ctx* ctx, real* v, const int n[3], int fzoff, const real* coarse_v, const int cn[3],
                               int czoff, int pzbeg, int pzend, int colour, bool add) {
    MGX_REQUIRE(ctx && v && coarse_v, MGX_ERR_INVALID, "interpolate_correct_slab: NULL argument");
    MGX_USE(ctx);
    int st = check_n3(n, "interpolate_correct_slab");
    if (st) return st;
    st = check_coarse3(n, cn, "interpolate_correct_slab");
    if (st) return st;
    MGX_REQUIRE(pzbeg >= 0 && pzend <= cn[2] - 1 && pzbeg <= pzend && fzoff >= 0 && czoff >= 0 && czoff <= pzbeg, MGX_ERR_INVALID,
                "interpolate_correct_slab: bad plane range");
    MGX_REQUIRE(colour >= -1 && colour <= 1, MGX_ERR_INVALID, "interpolate_correct_slab: colour %d not in {-1, 0, 1}", colour);
    if (pzbeg == pzend) return MGX_OK;
    const dim3 g = grd((n[0] + 1) / 2 - 1, cn[1] - 1, pzend - pzbeg);
    if (!add) {  // plain Interpolate (FMG, N3/MultiGrid3D.cpp:577): all interior points of the fine planes
        MGX_LAUNCH((interpolate3d_xs_kernel<real, false, -1>), g, blk(), 0, ctx->compute, v, n[0], n[1], fzoff, coarse_v,
                           cn[0], cn[1], czoff, pzbeg);
        MGX_LAUNCH_CHECK();
        return MGX_OK;
    }
    if (colour < 0)
        MGX_LAUNCH((interpolate3d_xs_kernel<real, true, -1>), g, blk(), 0, ctx->compute, v, n[0], n[1], fzoff, coarse_v,
                           cn[0], cn[1], czoff, pzbeg);
    else if (colour == 0)
        MGX_LAUNCH((interpolate3d_xs_kernel<real, true, 0>), g, blk(), 0, ctx->compute, v, n[0], n[1], fzoff, coarse_v,
                           cn[0], cn[1], czoff, pzbeg);
    else
        MGX_LAUNCH((interpolate3d_xs_kernel<real, true, 1>), g, blk(), 0, ctx->compute, v, n[0], n[1], fzoff, coarse_v,
                           cn[0], cn[1], czoff, pzbeg);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// the set P (tile-edge cells of that pass) corrected in place: the coarse cells covering the GLOBAL fine planes [zmin, zmax),
// which are the only ones written.  v / coarse_v are local arrays starting at the global planes fzoff / czoff; every coarse
// plane a written fine plane interpolates from must exist locally.
template <class real>
void corr_pset_launch(mgx_ctx* ctx, real* v, int sx, int sy, int fzoff, const real* coarse_v, const int cn[3], int czoff, int zmin,
                      int zmax) {
    PipePlan p;
    pipe_plan<real>(ctx, PipePass::Corr, sx, sy, zmin, zmax, 0, p);
    // the tile of the correcting pass: 128 pairs x 16 rows (relax3d_xs_pipe_kernel<real, 2, 8, 2>) or, fp32 on wide levels,
    // 256 pairs x 16 rows (relax3d_xs_pipe_v2_kernel<real, 2, 8, 2>)
    const int PW = p.v2 ? 256 : 128;
    constexpr int PH = 8;
    const int M = (sx + 1) / 2;
    const int pzbeg = zmin / 2, pzend = (zmax - 1) / 2 + 1;
    if (pzend <= pzbeg) return;
    const int nk = (cn[1] - 2) / PH + 1;
    // relax3d_xs_pipe_kernel<.., 2> and the unrolled two-pair kernel (mgx_pipe2_step.inc) correct everything they read themselves
    if (p.corrects_edges()) return;
    MGX_LAUNCH((correct_pset3d_xs_kernel<real>), dim3(ceil_div(M - 1, 64), ceil_div(nk, 4), pzend - pzbeg), blk(), 0, ctx->compute, v,
                       sx, sy, coarse_v, cn[0], cn[1], PW, PH, 0, fzoff, czoff, pzbeg, zmin, zmax);
}

// z-slab form of the set P (multi-GPU post-smoothing, csrc/host/mg_dist3d.inc; the correcting red pass on a slab:
// relax3d_corr_colour_slab, mgx_kernels3d.hip).  n / cn: GLOBAL sizes; v starts at global plane fzoff (even), coarse_v at
// czoff <= fzoff / 2.
template <class real>
int correct_pset3d_slab(mgx_ctx* ctx, real* v, const int n[3], int fzoff, const real* coarse_v, const int cn[3], int czoff, int zmin,
                        int zmax) {
    MGX_REQUIRE(ctx && v && coarse_v, MGX_ERR_INVALID, "correct_pset_slab: NULL argument");
    MGX_USE(ctx);
    int st = check_n3(n, "correct_pset_slab");
    if (st) return st;
    st = check_coarse3(n, cn, "correct_pset_slab");
    if (st) return st;
    MGX_REQUIRE(fzoff >= 0 && czoff >= 0 && zmin >= 1 && zmin >= fzoff && zmax <= n[2] - 1 && zmin / 2 >= czoff, MGX_ERR_INVALID,
                "correct_pset_slab: bad plane window");
    MGX_REQUIRE(corr_fused_level_takes(ctx, n[0], n[1], n[2]), MGX_ERR_INVALID, "correct_pset_slab: the level is not taken (ask corr_fused_takes)");
    corr_pset_launch<real>(ctx, v, n[0], n[1], fzoff, coarse_v, cn, czoff, zmin, zmax);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

template <class real, class L>
int diff_stats3d(mgx_ctx* ctx, const real* v, const int n[3], const double* tx, const double* ty, const double* tz,
                 double host_out[4]) {
    MGX_REQUIRE(ctx && v && tx && ty && tz && host_out, MGX_ERR_INVALID, "diff_stats3d: NULL argument");
    MGX_USE(ctx);
    int st = check_n3(n, "diff_stats3d");
    if (st) return st;
    const size_t cnt = (size_t)n[0] + n[1] + n[2];
    void* ws = nullptr;
    st = workspace(ctx, (cnt + 4) * sizeof(double), &ws);
    if (st) return st;
    double* d = (double*)ws;
    MGX_HIP(hipMemsetAsync(d, 0, 4 * sizeof(double), ctx->compute));
    MGX_HIP(hipMemcpyAsync(d + 4, tx, n[0] * sizeof(double), hipMemcpyHostToDevice, ctx->compute));
    MGX_HIP(hipMemcpyAsync(d + 4 + n[0], ty, n[1] * sizeof(double), hipMemcpyHostToDevice, ctx->compute));
    MGX_HIP(hipMemcpyAsync(d + 4 + n[0] + n[1], tz, n[2] * sizeof(double), hipMemcpyHostToDevice, ctx->compute));
    MGX_LAUNCH((diff_stats3d_kernel<real, L>), dim3(1, n[1], n[2]), dim3(n[0] >= 256 ? 256 : 64), 0, ctx->compute, v, n[0],
                       n[1], n[2], d + 4, d + 4 + n[0], d + 4 + n[0] + n[1], d);
    MGX_LAUNCH_CHECK();
    MGX_HIP(hipMemcpyAsync(host_out, d, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->compute));
    MGX_HIP(hipStreamSynchronize(ctx->compute));
    return MGX_OK;
}

template <class real>
int norm2(mgx_ctx* ctx, const real* x, size_t count, double* host_sumsq) {
    MGX_REQUIRE(ctx && (x || !count) && host_sumsq, MGX_ERR_INVALID, "norm2: NULL argument");
    MGX_USE(ctx);
    void* ws = nullptr;
    int st = workspace(ctx, sizeof(double), &ws);
    if (st) return st;
    MGX_HIP(hipMemsetAsync(ws, 0, sizeof(double), ctx->compute));
    if (count) {
        size_t blocks = (count + 255) / 256;
        const size_t cap = (size_t)ctx->num_cus * 8;
        if (blocks > cap) blocks = cap;
        MGX_LAUNCH((sumsq_kernel<real>), dim3((unsigned)blocks), dim3(256), 0, ctx->compute, x, count, (double*)ws);
        MGX_LAUNCH_CHECK();
    }
    MGX_HIP(hipMemcpyAsync(host_sumsq, ws, sizeof(double), hipMemcpyDeviceToHost, ctx->compute));
    MGX_HIP(hipStreamSynchronize(ctx->compute));
    return MGX_OK;
}

#define MGX_X(real)                                                                                                                  \
    template int interpolate_correct3d_slab<real>(mgx_ctx*, real*, const int[3], int, const real*, const int[3], int, int, int, int, bool); \
    template void corr_pset_launch<real>(mgx_ctx*, real*, int, int, int, const real*, const int[3], int, int, int);
MGX_X(float) MGX_X(double)
#undef MGX_X

}  // namespace mgx

#define MGX_DEFINE_OPS3D(PFX, L, SFX, real)                                                                      \
    int PFX##residual_##SFX(mgx_ctx* ctx, const real* v, const real* f, real* r, const int n[3], const real h[3], \
                            int mode) {                                                                          \
        return mgx::residual3d<real, L>(ctx, v, f, r, n, h, mode);                                               \
    }                                                                                                            \
    int PFX##restrict_##SFX(mgx_ctx* ctx, const real* fine, const int fn[3], real* coarse, const int cn[3]) {     \
        return mgx::restrict3d<real, L>(ctx, fine, fn, coarse, cn);                                              \
    }                                                                                                            \
    int PFX##interpolate_##SFX(mgx_ctx* ctx, real* fine, const int fn[3], const real* coarse, const int cn[3]) {  \
        return mgx::interpolate3d<real, L, false>(ctx, fine, fn, coarse, cn);                                    \
    }                                                                                                            \
    int PFX##apply_correction_##SFX(mgx_ctx* ctx, real* fine, const int fn[3], const real* err, const int en[3]) { \
        return mgx::correct3d<real, L>(ctx, fine, fn, err, en);                                                  \
    }                                                                                                            \
    int PFX##set_##SFX(mgx_ctx* ctx, real* grid, const int n[3], real value, int modify_boundaries) {            \
        return mgx::set3d<real, L>(ctx, grid, n, value, modify_boundaries);                                      \
    }                                                                                                            \
    int PFX##interpolate_correct_##SFX(mgx_ctx* ctx, real* v, const int n[3], const real* coarse_v,              \
                                       const int cn[3]) {                                                        \
        return mgx::interpolate3d<real, L, true>(ctx, v, n, coarse_v, cn);                                       \
    }                                                                                                            \
    int PFX##init_f_##SFX(mgx_ctx* ctx, real* f, const int n[3], double c, const double* host_tx,                \
                          const double* host_ty, const double* host_tz) {                                        \
        return mgx::init_f3d<real, L>(ctx, f, n, c, host_tx, host_ty, host_tz);                                  \
    }                                                                                                            \
    int PFX##diff_stats_##SFX(mgx_ctx* ctx, const real* v, const int n[3], const double* host_tx,                \
                              const double* host_ty, const double* host_tz, double host_out[4]) {                \
        return mgx::diff_stats3d<real, L>(ctx, v, n, host_tx, host_ty, host_tz, host_out);                       \
    }

#define MGX_DEFINE_MISC3D(SFX, real)                                                                             \
    int mgx3dxs_residual_sumsq_slab_##SFX(mgx_ctx* ctx, const real* v, const real* f, int sx, int sy,            \
                                          const real h[3], int mode, int zbeg, int zend, double* dev_out) {      \
        return mgx::residual_sumsq3d_slab<real>(ctx, v, f, sx, sy, h, mode, zbeg, zend, dev_out);                \
    }                                                                                                            \
    int mgx3dxs_interpolate_correct_slab_##SFX(mgx_ctx* ctx, real* v, const int n[3], int fzoff,                 \
                                               const real* coarse_v, const int cn[3], int czoff, int pzbeg,      \
                                               int pzend) {                                                      \
        return mgx::interpolate_correct3d_slab<real>(ctx, v, n, fzoff, coarse_v, cn, czoff, pzbeg, pzend, -1);   \
    }                                                                                                            \
    int mgx3dxs_set_interior_slab_##SFX(mgx_ctx* ctx, real* grid, int sx, int sy, int zbeg, int zend,            \
                                        real value) {                                                            \
        return mgx::set3d_slab<real>(ctx, grid, sx, sy, zbeg, zend, value);                                      \
    }                                                                                                            \
    int mgx3dxs_restrict_slab_##SFX(mgx_ctx* ctx, const real* fine, const int fn[3], int fzoff, real* coarse,     \
                                    const int cn[3], int czoff, int pzbeg, int pzend) {                          \
        return mgx::restrict3d_slab<real>(ctx, fine, fn, fzoff, coarse, cn, czoff, pzbeg, pzend);                \
    }                                                                                                            \
    int mgx3dxs_interpolate_slab_##SFX(mgx_ctx* ctx, real* fine, const int fn[3], int fzoff, const real* coarse, \
                                       const int cn[3], int czoff, int pzbeg, int pzend) {                       \
        return mgx::interpolate_correct3d_slab<real>(ctx, fine, fn, fzoff, coarse, cn, czoff, pzbeg, pzend, -1,  \
                                                     false);                                                     \
    }                                                                                                            \
    int mgx3dxs_interpolate_correct_colour_slab_##SFX(mgx_ctx* ctx, real* v, const int n[3], int fzoff,          \
                                                      const real* coarse_v, const int cn[3], int czoff,          \
                                                      int pzbeg, int pzend, int colour) {                        \
        return mgx::interpolate_correct3d_slab<real>(ctx, v, n, fzoff, coarse_v, cn, czoff, pzbeg, pzend,        \
                                                     colour);                                                    \
    }                                                                                                            \
    int mgx3dxs_correct_pset_slab_##SFX(mgx_ctx* ctx, real* v, const int n[3], int fzoff, const real* coarse_v,  \
                                        const int cn[3], int czoff, int zmin, int zmax) {                        \
        return mgx::correct_pset3d_slab<real>(ctx, v, n, fzoff, coarse_v, cn, czoff, zmin, zmax);                \
    }                                                                                                            \
    int mgx3dxs_interpolate_correct_colour_##SFX(mgx_ctx* ctx, real* v, const int n[3], const real* coarse_v,    \
                                                 const int cn[3], int colour) {                                  \
        return mgx::interpolate_correct3d_slab<real>(ctx, v, n, 0, coarse_v, cn, 0, 0, cn ? cn[2] - 1 : 0,       \
                                                     colour);                                                    \
    }                                                                                                            \
    int mgx3dxs_pack_##SFX(mgx_ctx* ctx, const real* natural, real* xsplit, const int n[3]) {                    \
        return mgx::relayout3d<real, mgx::Natural, mgx::XSplit>(ctx, natural, xsplit, n);                        \
    }                                                                                                            \
    int mgx3dxs_unpack_##SFX(mgx_ctx* ctx, const real* xsplit, real* natural, const int n[3]) {                  \
        return mgx::relayout3d<real, mgx::XSplit, mgx::Natural>(ctx, xsplit, natural, n);                        \
    }                                                                                                            \
    int mgx_norm2_##SFX(mgx_ctx* ctx, const real* x, size_t count, double* host_sumsq) {                         \
        return mgx::norm2<real>(ctx, x, count, host_sumsq);                                                      \
    }

extern "C" {
MGX_DEFINE_OPS3D(mgx3d_, mgx::Natural, f32, float)
MGX_DEFINE_OPS3D(mgx3d_, mgx::Natural, f64, double)
MGX_DEFINE_OPS3D(mgx3dxs_, mgx::XSplit, f32, float)
MGX_DEFINE_OPS3D(mgx3dxs_, mgx::XSplit, f64, double)
MGX_DEFINE_MISC3D(f32, float)
MGX_DEFINE_MISC3D(f64, double)
}
