// mgx_coef3d.hip -- the operators of the VARIABLE-COEFFICIENT problem div(a grad u) - s u = f, a > 0 given at the grid nodes,
// s >= 0, x-split layout: heterogeneous diffusion (conductivity, permeability, 1 / density).  DESIGN.md section 14.
//
// The reference has no such operator; the arithmetic is fixed here (and restated in tests/coef_restated.py), all in `real`,
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
// Kernels:
//   relax_coef3d_xs_kernel          one colour pass, relax_shift3d_xs_kernel's recipe with a marched next to v: lane j owns the
//                                   x-pair {2j, 2j+1} of R rows and marches along z; per step and row it loads one entry of v,
//                                   one of f and BOTH entries of a's pair at plane z+1 (2.5 words per point and pass with the
//                                   store); non-temporal stores; XCD-aware tiles; no LDS
//   relax_coef_zero3d_xs_kernel     the first red pass on a level that counts as zero: f and a in, red out, v not read
//   residual_coef3d_xs_kernel       r and / or the partials of <r, r>; with LAP: q = A p and the partials of <p, q>
#include <cmath>

#include "mgx_semi3d.hpp"

namespace mgx {

template <class real>
__device__ __forceinline__ real relax_coef3d_point(real O, real E, real N, real S, real D, real U, real f, real aO, real aE, real aN, real aS,
                                                   real aD, real aU, real aC, real qx, real qy, real qz, real s) {
    const real AW = aO + aC, AE = aE + aC, AN = aN + aC, AS = aS + aC, AD = aD + aC, AU = aU + aC;
    const real den = ((qx * (AW + AE) + qy * (AN + AS)) + qz * (AD + AU)) + s;
    const real num = ((qx * (AW * O + AE * E) + qy * (AN * N + AS * S)) + qz * (AD * D + AU * U)) - f;
    return num / den;
}

template <class real>
__device__ __forceinline__ real residual_coef3d_point(real O, real E, real N, real S, real D, real U, real c, real f, real aO, real aE, real aN,
                                                      real aS, real aD, real aU, real aC, real qx, real qy, real qz, real s) {
    const real AW = aO + aC, AE = aE + aC, AN = aN + aC, AS = aS + aC, AD = aD + aC, AU = aU + aC;
    const real tx = qx * (AW * (O - c) + AE * (E - c));
    const real ty = qy * (AN * (N - c) + AS * (S - c));
    const real tz = qz * (AD * (D - c) + AU * (U - c));
    return (((f - tx) - ty) - tz) + s * c;
}

// ------------------------------------------------------------------ relax, one colour
// Row r of the tile has parity q_r at plane z: the lane updates x = 2j + q_r, whose x-neighbours are the pair's other entry
// (half 1 - q_r, index j) and the "side" entry, the other entry of the neighbouring lane.  v is marched as in
// relax_shift3d_xs_kernel (c_prev = the own column at z-1, c_cur = the pair's other entry at z, U = the own column at z+1; at
// z+1 the parities flip and U becomes the other entry).  a is marched the same way, but the centre needs it too, so both
// entries of the pair stay in registers: a_c (half q_r) and a_x (half 1 - q_r) at plane z, a_d = the own column at z-1 (the
// a_x of the step before), and per step BOTH entries at z+1 are loaded (a_uc, a_ux) -- the 1.0 word per point of a.  aN / aS
// are the a_x of the rows above / below (their parity is the opposite one), the two edge rows come from cache, the side value
// by shuffle exactly as v's.
template <class real, int TYW, int R>
__global__ void __launch_bounds__(64 * TYW)
    relax_coef3d_xs_kernel(const real* __restrict__ vin, real* __restrict__ vout, const real* __restrict__ f, const real* __restrict__ a, int sx,
                           int sy, int zbeg, int zend, real qx, real qy, real qz, real s, int colour, int zchunk, int gx, int gy, int xcd_mode) {
    const Geo<XSplit, real> g(sx, sy);
    const int H = g.H;
    const int M = (sx + 1) >> 1;  // entries of the even-x half (the odd-x half has M-1)
    int bx, by, bz;
    tile_of_block(xcd_mode, gx, gy, bx, by, bz);
    const int j = bx * 64 + threadIdx.x;
    const int y0 = 1 + (by * TYW + __builtin_amdgcn_readfirstlane(threadIdx.y)) * R;  // wave-uniform
    if (y0 >= sy - 1 || j >= M - 1) return;  // x = 2j+q <= sx-2 needs j <= M-2
    const int nrows = min(R, sy - 1 - y0);    // rows y0 .. y0+nrows-1 are interior
    const int z0 = zbeg + bz * zchunk;
    const int z1 = min(z0 + zchunk, zend);
    if (z0 >= z1) return;
    const size_t sxy = g.PL;
    const int P = g.P;
    // row bases at plane z0; rows past sy-1 are clamped onto it (loads stay valid, nothing is stored for r >= nrows)
    size_t rowb[R];
#pragma unroll
    for (int r = 0; r < R; r++) rowb[r] = g.row(min(y0 + r, sy - 1), z0);
    int q = (colour + y0 + z0) & 1;  // parity of row r is q ^ (r & 1)
    real c_prev[R], c_cur[R], a_d[R], a_c[R], a_x[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int qr = q ^ (r & 1);
        c_prev[r] = vin[rowb[r] - sxy + qr * H + j];  // (half q_r,   j, plane z0-1)
        c_cur[r] = vin[rowb[r] + (1 - qr) * H + j];   // (half 1-q_r, j, plane z0)
        a_d[r] = a[rowb[r] - sxy + qr * H + j];
        a_c[r] = a[rowb[r] + qr * H + j];
        a_x[r] = a[rowb[r] + (1 - qr) * H + j];
    }
    for (int z = z0; z < z1; z++) {
        real U[R], side[R], fv[R], a_uc[R], a_ux[R], a_side[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int hq = (q ^ (r & 1)) * H, hx = H - hq;
            U[r] = vin[rowb[r] + sxy + hq + j];
            fv[r] = f[rowb[r] + hq + j];
            a_uc[r] = a[rowb[r] + sxy + hq + j];
            a_ux[r] = a[rowb[r] + sxy + hx + j];
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int qr = q ^ (r & 1);
            // the side values are the "other" entries of the neighbouring lane (j+1 when q_r = 1, j-1 when q_r = 0).  The wave's
            // edge lane, and the last active lane (lane j+1 = M-1 has exited), load them; lane j = 0 with q_r = 0 (x = 0, never
            // written) reads an entry further up the row instead of index -1 and discards the result
            const real nb = qr ? __shfl_down(c_cur[r], 1, 64) : __shfl_up(c_cur[r], 1, 64);
            const real anb = qr ? __shfl_down(a_x[r], 1, 64) : __shfl_up(a_x[r], 1, 64);
            const bool edge = qr ? (threadIdx.x == 63 || j == M - 2) : (threadIdx.x == 0);
            const size_t si = rowb[r] + (1 - qr) * H + j + (qr ? 1 : -1) + (qr | j ? 0 : M);
            side[r] = edge ? vin[si] : nb;
            a_side[r] = edge ? a[si] : anb;
        }
        const int qS = q ^ ((R - 1) & 1);
        const real Nedge = vin[rowb[0] - P + q * H + j], aNedge = a[rowb[0] - P + q * H + j];
        const real Sedge = vin[rowb[R - 1] + P + qS * H + j], aSedge = a[rowb[R - 1] + P + qS * H + j];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int qr = q ^ (r & 1);
            const real W = qr ? c_cur[r] : side[r], aW = qr ? a_x[r] : a_side[r];
            const real E = qr ? side[r] : c_cur[r], aE = qr ? a_side[r] : a_x[r];
            const real N = r == 0 ? Nedge : c_cur[r - 1], aN = r == 0 ? aNedge : a_x[r - 1];
            const real S = r == R - 1 ? Sedge : c_cur[r + 1], aS = r == R - 1 ? aSedge : a_x[r + 1];
            const real out = relax_coef3d_point<real>(W, E, N, S, c_prev[r], U[r], fv[r], aW, aE, aN, aS, a_d[r], a_uc[r], a_c[r], qx, qy, qz, s);
            if ((qr | j) && r < nrows) __builtin_nontemporal_store(out, &vout[rowb[r] + qr * H + j]);  // x = 2j+q_r >= 1
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            c_prev[r] = c_cur[r];
            c_cur[r] = U[r];
            a_d[r] = a_x[r];  // at z+1 the row's parity flips: its own column is the other entry of now
            a_c[r] = a_ux[r];
            a_x[r] = a_uc[r];
            rowb[r] += sxy;
        }
        q ^= 1;
    }
}

// the first red pass of a level that counts as all zeros (boundary entries zero in memory): the point expression on six zero
// neighbours, evaluated as such (the signs of zeros are those of the generic pass on a zeroed array); v is not read
template <class real>
__global__ void __launch_bounds__(256) relax_coef_zero3d_xs_kernel(real* __restrict__ v, const real* __restrict__ f, const real* __restrict__ a,
                                                                   int sx, int sy, real qx, real qy, real qz, real s) {
    const int y = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int z = 1 + blockIdx.z;
    if (y >= sy - 1) return;
    const int x = 2 * (blockIdx.x * blockDim.x + threadIdx.x) + ((y + z) & 1);
    if (x < 1 || x >= sx - 1) return;
    const Geo<XSplit, real> g(sx, sy);
    const size_t row = g.row(y, z), idx = row + g.pos(x);
    const real zero = (real)0;
    const real out = relax_coef3d_point<real>(zero, zero, zero, zero, zero, zero, f[idx], a[row + g.pos(x - 1)], a[row + g.pos(x + 1)], a[idx - g.P],
                                              a[idx + g.P], a[idx - g.PL], a[idx + g.PL], a[idx], qx, qy, qz, s);
    __builtin_nontemporal_store(out, &v[idx]);
}

// ------------------------------------------------------------------ residual / operator with a sum
// residual_shift3d_xs_kernel's walk (mgx_shift3d.hip): one wave per interior x-row, its lanes over the row's storage positions,
// CJ positions per lane and step with the loads first; sums in double in a fixed order (per lane in loop order, wave shuffles,
// the block's four waves in order, one partial per block, then the final kernel).
constexpr int CJ = 4, CROWS = 4, CSTEP = 64 * CJ;

__device__ __forceinline__ int coef_x_of(int j, int H) { return j < H ? 2 * j : 2 * (j - H) + 1; }  // pads give x >= sx

__device__ __forceinline__ void coef_block_sum(double acc, double* part, double* __restrict__ partial) {
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (threadIdx.x == 0) part[threadIdx.y] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// LAP = false: r = residual(v, f) (stored unless out is NULL), partials of <r, r> unless partial is NULL
// LAP = true:  out = q = -(residual(v, 0)), partials of <v, q>
template <class real, bool LAP>
__global__ void __launch_bounds__(256) residual_coef3d_xs_kernel(const real* __restrict__ v, const real* __restrict__ f, const real* __restrict__ a,
                                                                 real* __restrict__ out, int sx, int sy, real qx, real qy, real qz, real s,
                                                                 double* __restrict__ partial) {
    const Geo<XSplit, real> g(sx, sy);
    const int y = 1 + blockIdx.x * CROWS + threadIdx.y, z = 1 + blockIdx.y;
    const int H = g.H, P = g.P;
    const size_t PL = g.PL;
    double acc = 0.0;
    if (y < sy - 1) {
        const size_t row = g.row(y, z);
        for (int j0 = 0; j0 < P; j0 += CSTEP) {
            real O[CJ], E[CJ], N[CJ], S[CJ], D[CJ], U[CJ], c[CJ], fv[CJ], aO[CJ], aE[CJ], aN[CJ], aS[CJ], aD[CJ], aU[CJ], aC[CJ];
            bool in[CJ];
#pragma unroll
            for (int k = 0; k < CJ; k++) {
                const int j = j0 + k * 64 + threadIdx.x, x = coef_x_of(j, H);
                in[k] = j < P && x >= 1 && x <= sx - 2;
                if (in[k]) {
                    const size_t i = row + j, iw = row + XSplit::pos(x - 1, H), ie = row + XSplit::pos(x + 1, H);
                    O[k] = v[iw]; aO[k] = a[iw];
                    E[k] = v[ie]; aE[k] = a[ie];
                    N[k] = v[i - P]; aN[k] = a[i - P];
                    S[k] = v[i + P]; aS[k] = a[i + P];
                    D[k] = v[i - PL]; aD[k] = a[i - PL];
                    U[k] = v[i + PL]; aU[k] = a[i + PL];
                    c[k] = v[i]; aC[k] = a[i];
                    fv[k] = LAP ? (real)0 : f[i];
                }
            }
#pragma unroll
            for (int k = 0; k < CJ; k++)
                if (in[k]) {
                    real t = residual_coef3d_point<real>(O[k], E[k], N[k], S[k], D[k], U[k], c[k], fv[k], aO[k], aE[k], aN[k], aS[k], aD[k], aU[k],
                                                         aC[k], qx, qy, qz, s);
                    if (LAP) t = -t;  // negation is exact
                    if (out) out[row + j0 + k * 64 + threadIdx.x] = t;
                    acc += LAP ? (double)c[k] * (double)t : (double)t * (double)t;
                }
        }
    }
    if (partial) {  // (uniform over the launch)
        __shared__ double part[CROWS];
        coef_block_sum(acc, part, partial);
    }
}

// =========================================================================== host side
static int coef_check(const int n[3], double s, const char* what, bool rows_grid) {
    MGX_REQUIRE(n, MGX_ERR_INVALID, "%s: size array is NULL", what);
    MGX_REQUIRE(std::isfinite(s) && s >= 0, MGX_ERR_INVALID, "%s: the shift %g is not finite and >= 0", what, s);
    for (int d = 0; d < 3; d++) MGX_REQUIRE(valid_size(n[d]), MGX_ERR_SIZE, "%s: size[%d] = %d is not odd and >= 3", what, d, n[d]);
    MGX_REQUIRE((double)n[0] * n[1] * n[2] < 2147483647.0 * 4, MGX_ERR_SIZE, "%s: grid too large", what);
    MGX_REQUIRE(!rows_grid || n[2] - 2 <= 65535, MGX_ERR_SIZE, "%s: %d planes are too many", what, n[2]);
    return MGX_OK;
}

// qx = (real)0.5 / hx2 .. : half the reciprocal squared spacings (the 1/2 of the face means)
template <class real>
struct CoefScale {
    real qx, qy, qz;
    explicit CoefScale(const real h[3]) {
        const real hx2 = h[0] * h[0], hy2 = h[1] * h[1], hz2 = h[2] * h[2];
        qx = (real)0.5 / hx2;
        qy = (real)0.5 / hy2;
        qz = (real)0.5 / hz2;
    }
};

// one colour pass over the planes 1 .. sz-2: relax_shift3d_pass's launch geometry (four waves of four rows, fewer on small
// levels; runs of four planes, halved while the launch has fewer than eight workgroups per CU).  "relax3d.rows" below 4 lowers
// the rows per lane (fp64 with four rows: 124 VGPRs, four waves per SIMD; with two: 74, six)
template <class real>
static void relax_coef3d_pass(mgx_ctx* ctx, real* v, const real* f, const real* a, const int n[3], const CoefScale<real>& c, real s, int colour) {
    const int sx = n[0], sy = n[1], zbeg = 1, zend = n[2] - 1;
    int ty = 4, rows = ctx->relax_rows < 4 ? ctx->relax_rows : 4;
    while (rows > 1 && rows * ty > sy - 2) rows >>= 1;
    while (ty > 1 && rows * ty > sy - 2) ty >>= 1;
    const int gx = ceil_div((sx + 1) / 2 - 1, 64), gy = ceil_div(sy - 2, ty * rows);
    int zchunk = 4;
    while (zchunk > 1 && (long long)gx * gy * ceil_div(zend - zbeg, zchunk) < 8LL * ctx->num_cus) zchunk >>= 1;
    const unsigned nblocks = (unsigned)gx * gy * ceil_div(zend - zbeg, zchunk);
    const int xcd = ctx->relax_xcd == 1 ? 1 : 0;
    with_value<1, 2, 4>(ty, [&](auto t) __attribute__((always_inline)) {
        with_value<1, 2, 4>(rows, [&](auto r) __attribute__((always_inline)) {
            constexpr int TYW = decltype(t)::value, RR = decltype(r)::value;
            note_relax_kernel<real>(ctx, "relax_coef3d_xs_kernel", TYW, RR, 0);
            MGX_LAUNCH((relax_coef3d_xs_kernel<real, TYW, RR>), dim3(nblocks), dim3(64, TYW, 1), 0, ctx->compute, (const real*)v, v, f, a, sx, sy,
                       zbeg, zend, c.qx, c.qy, c.qz, s, colour, zchunk, gx, gy, xcd);
        });
    });
}

template <class real>
static int relax_coef3d(mgx_ctx* ctx, real* v, const real* f, const real* a, const int n[3], const real h[3], real s, int ncycles, int from_zero,
                        int rim_is_zero) {
    const char* what = from_zero ? "relax_coef_from_zero" : "relax_coef";
    MGX_REQUIRE(ctx && v && f && a && h, MGX_ERR_INVALID, "%s: NULL argument", what);
    MGX_TRY_RET(coef_check(n, (double)s, what, false));
    MGX_REQUIRE(ncycles >= 0, MGX_ERR_INVALID, "%s: ncycles = %d < 0", what, ncycles);
    MGX_USE(ctx);
    const CoefScale<real> c(h);
    int s0 = 0;
    if (from_zero && (!rim_is_zero || ncycles == 0)) {  // v := 0 everywhere, then generic passes
        MGX_TRY_RET(fill_zero(ctx, v, Geo<XSplit, real>(n[0], n[1]).PL * (size_t)n[2] * sizeof(real)));
    } else if (from_zero) {  // nothing is filled and the first red pass does not read v
        note_relax_kernel<real>(ctx, "relax_coef_zero3d_xs_kernel", 0, 0, 0);
        MGX_LAUNCH((relax_coef_zero3d_xs_kernel<real>), dim3(ceil_div((n[0] + 1) / 2, 64), ceil_div(n[1] - 2, 4), n[2] - 2), dim3(64, 4, 1), 0,
                   ctx->compute, v, f, a, n[0], n[1], c.qx, c.qy, c.qz, s);
        s0 = 1;
    }
    for (int p = s0; p < 2 * ncycles; p++) relax_coef3d_pass<real>(ctx, v, f, a, n, c, s, p & 1);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

static dim3 coef_rows_grid(const int n[3]) { return dim3((unsigned)ceil_div(n[1] - 2, CROWS), (unsigned)(n[2] - 2)); }

template <class real>
static int residual_coef3d(mgx_ctx* ctx, const real* v, const real* f, const real* a, real* r, const int n[3], const real h[3], real s,
                           double* dev_work, double* dev_sumsq) {
    MGX_REQUIRE(ctx && v && f && a && h && (r || dev_sumsq) && (!dev_sumsq || dev_work), MGX_ERR_INVALID, "residual_coef: NULL argument");
    MGX_TRY_RET(coef_check(n, (double)s, "residual_coef", true));
    MGX_USE(ctx);
    const CoefScale<real> c(h);
    const dim3 g = coef_rows_grid(n);
    if (r)  // the boundary of r is 0, as mgx3dxs_residual leaves it
        MGX_LAUNCH((rim_zero3d_xs_kernel<real>), dim3(ceil_div(n[0], 64), ceil_div(n[1], 4), n[2]), dim3(64, 4, 1), 0, ctx->compute, r, n[0], n[1],
                   n[2]);
    MGX_LAUNCH((residual_coef3d_xs_kernel<real, false>), g, dim3(64, CROWS, 1), 0, ctx->compute, v, f, a, r, n[0], n[1], c.qx, c.qy, c.qz, s,
               dev_sumsq ? dev_work : (double*)nullptr);
    MGX_LAUNCH_CHECK();
    return dev_sumsq ? krylov_final(ctx, dev_work, (size_t)g.x * g.y, 1, dev_sumsq) : MGX_OK;
}

template <class real>
static int apply_coef_dot3d(mgx_ctx* ctx, const real* p, const real* a, real* q, const int n[3], const real h[3], real s, double* dev_work,
                            double* dev_sum) {
    MGX_REQUIRE(ctx && p && a && q && h && dev_work && dev_sum, MGX_ERR_INVALID, "apply_coef_dot: NULL argument");
    MGX_TRY_RET(coef_check(n, (double)s, "apply_coef_dot", true));
    MGX_USE(ctx);
    const CoefScale<real> c(h);
    const dim3 g = coef_rows_grid(n);
    MGX_LAUNCH((residual_coef3d_xs_kernel<real, true>), g, dim3(64, CROWS, 1), 0, ctx->compute, p, (const real*)nullptr, a, q, n[0], n[1], c.qx,
               c.qy, c.qz, s, dev_work);
    MGX_LAUNCH_CHECK();
    return krylov_final(ctx, dev_work, (size_t)g.x * g.y, 1, dev_sum);
}

}  // namespace mgx

#define MGX_COEF3D_API(SFX, real)                                                                                                            \
    extern "C" int mgx3dxs_relax_coef_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const int n[3], const real h[3], real s,    \
                                            int ncycles) {                                                                                   \
        return mgx::relax_coef3d<real>(ctx, v, f, a, n, h, s, ncycles, 0, 0);                                                                \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_relax_coef_from_zero_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const int n[3], const real h[3],  \
                                                      real s, int ncycles, int rim_is_zero) {                                                \
        return mgx::relax_coef3d<real>(ctx, v, f, a, n, h, s, ncycles, 1, rim_is_zero);                                                      \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_residual_coef_##SFX(mgx_ctx* ctx, const real* v, const real* f, const real* a, real* r, const int n[3],           \
                                               const real h[3], real s, double* dev_work, double* dev_sumsq) {                               \
        return mgx::residual_coef3d<real>(ctx, v, f, a, r, n, h, s, dev_work, dev_sumsq);                                                    \
    }                                                                                                                                        \
    extern "C" int mgx3dxs_apply_coef_dot_##SFX(mgx_ctx* ctx, const real* p, const real* a, real* q, const int n[3], const real h[3],        \
                                                real s, double* dev_work, double* dev_sum) {                                                 \
        return mgx::apply_coef_dot3d<real>(ctx, p, a, q, n, h, s, dev_work, dev_sum);                                                        \
    }

MGX_COEF3D_API(f32, float)
MGX_COEF3D_API(f64, double)
