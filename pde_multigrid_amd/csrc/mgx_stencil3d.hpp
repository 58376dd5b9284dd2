// mgx_stencil3d.hpp -- what the 7-point operators of the x-split layout share: the row walk of the Krylov kernels (mgx_krylov3d.hip)
// and the residual / operator kernel built on it, the colour pass of the smoother and its from-zero first pass, and the host
// drivers that launch them.  Each is written once and takes the operator as a policy `Op`, passed to the kernels by value:
//   PlainOp  (mgx_krylov3d.hip)  the CORRECT-mode Laplacian                         q = A p only
//   ShiftOp  (mgx_ops3d.hpp)     (Laplacian - s) u = f                             DESIGN.md section 13
//   CoefOp   (mgx_ops3d.hpp)     div(a grad u) - s u = f, a at the grid nodes      DESIGN.md section 14
//   CapOp    (mgx_ops3d.hpp)     div(a grad u) - (s c) u = f, c at the grid nodes  DESIGN.md section 17
//   HarmOp, HarmCapOp (mgx_ops3d.hpp)  CoefOp and CapOp with harmonic-mean faces      DESIGN.md section 19
// A policy holds
//   Op(ctx, h, s)                          the operator's scalars for a level with spacings h, formed by the host once per call
//                                          (with HAS_C: Op(ctx, h, s, c), and op.c is the capacity array)
//   HAS_A, HAS_S, HAS_C                    does it read a coefficient array / take a shift (checked to be finite and >= 0) / read
//                                          a capacity at the updated point
//   relax(v, f, a)                         the smoother's point expression (v.C is not read); with HAS_C relax(v, f, a, cP)
//   residual<MODE>(v, f, a), with_mode()   the residual's point expression (with HAS_C a fourth argument cP) and the MODEs the
//                                          host picks from (op.mode)
//   rows(ctx), relax_kernel, zero_kernel   the colour pass: its rows per lane and the names last_relax_kernel() reports
// and keeps its arithmetic to itself: all in `real`, left to right as written there, nothing contracted.
#pragma once
#include <cmath>

#include "mgx_host3d.hpp"
#include "mgx_semi3d.hpp"

namespace mgx {

// an array's values around one point: O/E = x-1/x+1, N/S = y-1/y+1, D/U = z-1/z+1, C the centre
template <class real>
struct Star7 {
    real O, E, N, S, D, U, C;
};

// ------------------------------------------------------------------ the row walk
// One wavefront per interior x-row (y, z), its lanes over the row's storage positions j in [0, P) (the even-x half, then the
// odd-x half from H on), so every access of a wave is one contiguous run of a half-row.  Each lane handles KJ positions per
// step, loads first, so that KJ loads per array are in flight.  Reductions are accumulated in double in a fixed order: per lane
// in loop order, wavefront-wide shuffles, the block's four waves in a fixed order into one partial per block, then
// cg_final_kernel adds the partials in a fixed order -- the same bits on every run.
constexpr int KJ = 4;           // positions per lane and step
constexpr int KROWS = 4;        // rows (waves) per block
constexpr int KSTEP = 64 * KJ;  // positions of a row per wave and step

// x of storage position j of an x-split row (pads give x >= sx)
__device__ __forceinline__ int xs_x(int j, int H) { return j < H ? 2 * j : 2 * (j - H) + 1; }

// the wave's sum into part[wave]
__device__ __forceinline__ void wave_sum(double acc, double* part) {
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (threadIdx.x == 0) part[threadIdx.y] = acc;
}
// ... and the block's four waves in a fixed order into the block's partial
__device__ __forceinline__ void block_sum(double acc, double* part, double* __restrict__ partial) {
    wave_sum(acc, part);
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

static dim3 krylov_grid(const int n[3]) { return dim3((unsigned)ceil_div(n[1] - 2, KROWS), (unsigned)(n[2] - 2)); }
static dim3 krylov_block() { return dim3(64, KROWS, 1); }

// the sizes of an entry and its shift (s == NULL: it takes none, and its kernels index any number of points).  rows_grid: the
// launch has one block row per interior plane
static int rows_check(const int n[3], const char* what, const double* s = nullptr, bool rows_grid = true) {
    MGX_REQUIRE(n, MGX_ERR_INVALID, "%s: size array is NULL", what);
    MGX_REQUIRE(!s || (std::isfinite(*s) && *s >= 0), MGX_ERR_INVALID, "%s: the shift %g is not finite and >= 0", what, s ? *s : 0.0);
    for (int d = 0; d < 3; d++) MGX_REQUIRE(valid_size(n[d]), MGX_ERR_SIZE, "%s: size[%d] = %d is not odd and >= 3", what, d, n[d]);
    MGX_REQUIRE(!s || (double)n[0] * n[1] * n[2] < 2147483647.0 * 4, MGX_ERR_SIZE, "%s: grid too large", what);
    MGX_REQUIRE(!rows_grid || n[2] - 2 <= 65535, MGX_ERR_SIZE, "%s: %d planes are too many", what, n[2]);
    return MGX_OK;
}

// LAP = false: r = op's residual of (v, f) (stored unless out is NULL), partials of <r, r> unless partial is NULL
// LAP = true:  out = q = A v = -(op's residual of (v, 0)), partials of <v, q>
template <class real, class Op, int MODE, bool LAP>
__global__ void __launch_bounds__(256) residual_op3d_xs_kernel(const real* __restrict__ v, const real* __restrict__ f, const real* __restrict__ a,
                                                               real* __restrict__ out, int sx, int sy, Op op, double* __restrict__ partial) {
    const Geo<XSplit, real> g(sx, sy);
    const int y = 1 + blockIdx.x * KROWS + threadIdx.y, z = 1 + blockIdx.y;
    const int H = g.H, P = g.P;
    const size_t PL = g.PL;
    double acc = 0.0;
    if (y < sy - 1) {
        const size_t row = g.row(y, z);
        for (int j0 = 0; j0 < P; j0 += KSTEP) {
            Star7<real> vs[KJ], as[KJ];  // (as: with Op::HAS_A)
            real fv[KJ], cv[KJ];  // (cv: with Op::HAS_C)
            bool in[KJ];
#pragma unroll
            for (int k = 0; k < KJ; k++) {
                const int j = j0 + k * 64 + threadIdx.x, x = xs_x(j, H);
                in[k] = j < P && x >= 1 && x <= sx - 2;
                if (in[k]) {
                    auto load = [&](real& vx, real& ax, size_t i) __attribute__((always_inline)) {
                        vx = v[i];
                        if constexpr (Op::HAS_A) ax = a[i];
                    };
                    const size_t i = row + j, iw = row + XSplit::pos(x - 1, H), ie = row + XSplit::pos(x + 1, H);
                    load(vs[k].O, as[k].O, iw);
                    load(vs[k].E, as[k].E, ie);
                    load(vs[k].N, as[k].N, i - P);
                    load(vs[k].S, as[k].S, i + P);
                    load(vs[k].D, as[k].D, i - PL);
                    load(vs[k].U, as[k].U, i + PL);
                    load(vs[k].C, as[k].C, i);
                    fv[k] = LAP ? (real)0 : f[i];
                    if constexpr (Op::HAS_C) cv[k] = op.c[i];
                }
            }
#pragma unroll
            for (int k = 0; k < KJ; k++)
                if (in[k]) {
                    real t;
                    if constexpr (Op::HAS_C) t = op.template residual<MODE>(vs[k], fv[k], as[k], cv[k]);
                    else t = op.template residual<MODE>(vs[k], fv[k], as[k]);
                    if (LAP) t = -t;  // negation is exact
                    if (LAP || out) out[row + j0 + k * 64 + threadIdx.x] = t;
                    acc += LAP ? (double)vs[k].C * (double)t : (double)t * (double)t;
                }
        }
    }
    if (LAP || partial) {  // (uniform over the launch)
        __shared__ double part[KROWS];
        block_sum(acc, part, partial);
    }
}

// ------------------------------------------------------------------ relax, one colour
// relax3d_xs_kernel's recipe (mgx_kernels3d.hip): the same lane / row / plane assignment, the same loads and stores.  Lane j owns
// the x-pair {2j, 2j+1} of R rows and marches along z.  Row r of the tile has parity q_r at plane z: the lane updates
// x = 2j + q_r, whose x-neighbours are the pair's other entry (half 1 - q_r, index j) and the "side" entry, the other entry of
// the neighbouring lane.  Of v the lane keeps c_prev = the own column at z-1 and c_cur = the pair's other entry at z, and loads
// U = the own column at z+1 (at z+1 the parities flip and U becomes the other entry): per step and row one streaming load of v
// and one of f, the side value from the neighbouring lane, the two edge rows from L1 / L2; non-temporal stores; XCD-aware tiles.
// With Op::HAS_A the coefficient is marched the same way, but the centre needs it too, so both entries of the pair stay in
// registers: a_c (half q_r) and a_x (half 1 - q_r) at plane z, a_d = the own column at z-1 (the a_x of the step before), and per
// step BOTH entries at z+1 are loaded (a_uc, a_ux) -- 1.0 word per point of a.  aN / aS are the a_x of the rows above / below
// (their parity is the opposite one), the two edge rows come from cache, the side value by shuffle exactly as v's.  Without
// HAS_A none of this exists.  With Op::HAS_C the capacity is read at the updated point alone, with f's index: one more streaming
// load per step and row (3.0 words per point and pass against 2.5), nothing marched.
template <class real, class Op, int TYW, int R>
__global__ void __launch_bounds__(64 * TYW)
    relax_op3d_xs_kernel(const real* __restrict__ vin, real* __restrict__ vout, const real* __restrict__ f, const real* __restrict__ a, int sx,
                         int sy, int zbeg, int zend, Op op, int colour, int zchunk, int gx, int gy, int xcd_mode) {
    constexpr int RA = Op::HAS_A ? R : 1;  // rows of the coefficient's registers
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
    real c_prev[R], c_cur[R], a_d[RA], a_c[RA], a_x[RA];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int qr = q ^ (r & 1);
        c_prev[r] = vin[rowb[r] - sxy + qr * H + j];  // (half q_r,   j, plane z0-1)
        c_cur[r] = vin[rowb[r] + (1 - qr) * H + j];   // (half 1-q_r, j, plane z0)
        if constexpr (Op::HAS_A) {
            a_d[r] = a[rowb[r] - sxy + qr * H + j];
            a_c[r] = a[rowb[r] + qr * H + j];
            a_x[r] = a[rowb[r] + (1 - qr) * H + j];
        }
    }
    for (int z = z0; z < z1; z++) {
        real U[R], side[R], fv[R], a_uc[RA], a_ux[RA], a_side[RA], cv[Op::HAS_C ? R : 1];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int hq = (q ^ (r & 1)) * H;
            U[r] = vin[rowb[r] + sxy + hq + j];
            fv[r] = f[rowb[r] + hq + j];
            if constexpr (Op::HAS_C) cv[r] = op.c[rowb[r] + hq + j];
            if constexpr (Op::HAS_A) {
                a_uc[r] = a[rowb[r] + sxy + hq + j];
                a_ux[r] = a[rowb[r] + sxy + (H - hq) + j];
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int qr = q ^ (r & 1);
            // the side values are the "other" entries of the neighbouring lane (j+1 when q_r = 1, j-1 when q_r = 0).  The wave's
            // edge lane, and the last active lane (lane j+1 = M-1 has exited), load them; lane j = 0 with q_r = 0 (x = 0, never
            // written) reads index M-1 of half 0 instead of index -1 and discards the result
            const real nb = qr ? __shfl_down(c_cur[r], 1, 64) : __shfl_up(c_cur[r], 1, 64);
            real anb = 0;
            if constexpr (Op::HAS_A) anb = qr ? __shfl_down(a_x[r], 1, 64) : __shfl_up(a_x[r], 1, 64);
            const bool edge = qr ? (threadIdx.x == 63 || j == M - 2) : (threadIdx.x == 0);
            const size_t si = rowb[r] + (1 - qr) * H + j + (qr ? 1 : -1) + (qr | j ? 0 : M);
            side[r] = edge ? vin[si] : nb;
            if constexpr (Op::HAS_A) a_side[r] = edge ? a[si] : anb;
        }
        const int qS = q ^ ((R - 1) & 1);
        real aNedge = 0, aSedge = 0;
        const real Nedge = vin[rowb[0] - P + q * H + j];
        if constexpr (Op::HAS_A) aNedge = a[rowb[0] - P + q * H + j];
        const real Sedge = vin[rowb[R - 1] + P + qS * H + j];
        if constexpr (Op::HAS_A) aSedge = a[rowb[R - 1] + P + qS * H + j];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int qr = q ^ (r & 1);
            Star7<real> vs, as;  // (as: with Op::HAS_A)
            vs.O = qr ? c_cur[r] : side[r];
            vs.E = qr ? side[r] : c_cur[r];
            vs.N = r == 0 ? Nedge : c_cur[r - 1];
            vs.S = r == R - 1 ? Sedge : c_cur[r + 1];
            vs.D = c_prev[r];
            vs.U = U[r];
            vs.C = 0;  // (the point itself: not read)
            if constexpr (Op::HAS_A) {
                as.O = qr ? a_x[r] : a_side[r];
                as.E = qr ? a_side[r] : a_x[r];
                as.N = r == 0 ? aNedge : a_x[r - 1];
                as.S = r == R - 1 ? aSedge : a_x[r + 1];
                as.D = a_d[r];
                as.U = a_uc[r];
                as.C = a_c[r];
            }
            real out;
            if constexpr (Op::HAS_C) out = op.relax(vs, fv[r], as, cv[r]);
            else out = op.relax(vs, fv[r], as);
            if ((qr | j) && r < nrows) __builtin_nontemporal_store(out, &vout[rowb[r] + qr * H + j]);  // x = 2j+q_r >= 1
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            c_prev[r] = c_cur[r];
            c_cur[r] = U[r];
            if constexpr (Op::HAS_A) {
                a_d[r] = a_x[r];  // at z+1 the row's parity flips: its own column is the other entry of now
                a_c[r] = a_ux[r];
                a_x[r] = a_uc[r];
            }
            rowb[r] += sxy;
        }
        q ^= 1;
    }
}

// the first red pass of a level that counts as all zeros (boundary entries zero in memory): the point expression on six zero
// neighbours, evaluated as such (the signs of zeros are those of the generic pass on a zeroed array); v is not read
template <class real, class Op>
__global__ void __launch_bounds__(256) relax_op_zero3d_xs_kernel(real* __restrict__ v, const real* __restrict__ f, const real* __restrict__ a,
                                                                 int sx, int sy, Op op) {
    const int y = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int z = 1 + blockIdx.z;
    if (y >= sy - 1) return;
    const int x = 2 * (blockIdx.x * blockDim.x + threadIdx.x) + ((y + z) & 1);
    if (x < 1 || x >= sx - 1) return;
    const Geo<XSplit, real> g(sx, sy);
    const size_t row = g.row(y, z), idx = row + g.pos(x);
    Star7<real> as = {};
    if constexpr (Op::HAS_A)
        as = {a[row + g.pos(x - 1)], a[row + g.pos(x + 1)], a[idx - g.P], a[idx + g.P], a[idx - g.PL], a[idx + g.PL], a[idx]};
    if constexpr (Op::HAS_C) __builtin_nontemporal_store(op.relax(Star7<real>{}, f[idx], as, op.c[idx]), &v[idx]);
    else __builtin_nontemporal_store(op.relax(Star7<real>{}, f[idx], as), &v[idx]);
}

// =========================================================================== host side
// `what` is the entry point's name in its error texts; `a` is NULL for an operator without a coefficient array, `c` for one without
// a capacity array.
template <class Op, class real>
static Op make_op(const mgx_ctx* ctx, const real h[3], real s, const real* c) {
    if constexpr (Op::HAS_C) return Op(ctx, h, s, c);
    else return Op(ctx, h, s);
}

// one colour pass over the planes 1 .. sz-2: relax3d_xs_kernel's launch geometry (four waves of Op::rows() rows, fewer on small
// levels; runs of four planes, halved while the launch has fewer than eight workgroups per CU, or runs of "relax3d.zchunk" planes
// where that is set: the same bits for every run length).  The run length launched is the last number of last_relax_kernel()
template <class Op, class real>
static void relax_op3d_pass(mgx_ctx* ctx, real* v, const real* f, const real* a, const int n[3], const Op& op, int colour) {
    const int sx = n[0], sy = n[1], zbeg = 1, zend = n[2] - 1;
    int ty = 4, rows = Op::rows(ctx);
    while (rows > 1 && rows * ty > sy - 2) rows >>= 1;
    while (ty > 1 && rows * ty > sy - 2) ty >>= 1;
    const int gx = ceil_div((sx + 1) / 2 - 1, 64), gy = ceil_div(sy - 2, ty * rows);
    int zchunk = 4;
    if (ctx->relax_zchunk > 0) zchunk = ctx->relax_zchunk;
    else
        while (zchunk > 1 && (long long)gx * gy * ceil_div(zend - zbeg, zchunk) < 8LL * ctx->num_cus) zchunk >>= 1;
    const unsigned nblocks = (unsigned)gx * gy * ceil_div(zend - zbeg, zchunk);
    const int xcd = ctx->relax_xcd == 1 ? 1 : 0;
    with_value<1, 2, 4>(ty, [&](auto t) __attribute__((always_inline)) {
        with_value<1, 2, 4>(rows, [&](auto r) __attribute__((always_inline)) {
            constexpr int TYW = decltype(t)::value, RR = decltype(r)::value;
            note_relax_kernel<real>(ctx, Op::relax_kernel, TYW, RR, zchunk);
            MGX_LAUNCH((relax_op3d_xs_kernel<real, Op, TYW, RR>), dim3(nblocks), dim3(64, TYW, 1), 0, ctx->compute, (const real*)v, v, f, a, sx, sy,
                       zbeg, zend, op, colour, zchunk, gx, gy, xcd);
        });
    });
}

// ncycles red+black sweeps; from_zero: v counts as all zeros (rim_is_zero: and its boundary is zero in memory)
template <class Op, class real>
static int relax_op3d(mgx_ctx* ctx, real* v, const real* f, const real* a, const int n[3], const real h[3], real s, int ncycles, int from_zero,
                      int rim_is_zero, const char* what, const real* c = nullptr) {
    MGX_REQUIRE(ctx && v && f && (a || !Op::HAS_A) && (c || !Op::HAS_C) && h, MGX_ERR_INVALID, "%s: NULL argument", what);
    const double sd = (double)s;
    MGX_TRY_RET(rows_check(n, what, &sd, false));
    MGX_REQUIRE(ncycles >= 0, MGX_ERR_INVALID, "%s: ncycles = %d < 0", what, ncycles);
    MGX_USE(ctx);
    const Op op = make_op<Op, real>(ctx, h, s, c);
    int s0 = 0;
    if (from_zero && (!rim_is_zero || ncycles == 0)) {  // v := 0 everywhere, then generic passes
        MGX_TRY_RET(fill_zero(ctx, v, Geo<XSplit, real>(n[0], n[1]).PL * (size_t)n[2] * sizeof(real)));
    } else if (from_zero) {  // nothing is filled and the first red pass does not read v
        note_relax_kernel<real>(ctx, Op::zero_kernel, 0, 0, 0);
        MGX_LAUNCH((relax_op_zero3d_xs_kernel<real, Op>), dim3(ceil_div((n[0] + 1) / 2, 64), ceil_div(n[1] - 2, 4), n[2] - 2), dim3(64, 4, 1), 0,
                   ctx->compute, v, f, a, n[0], n[1], op);
        s0 = 1;
    }
    for (int p = s0; p < 2 * ncycles; p++) relax_op3d_pass<Op, real>(ctx, v, f, a, n, op, p & 1);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// the launch of residual_op3d_xs_kernel and the final sum (dev_sum == NULL: none; finalize = false: the partials are left in
// dev_work[0, grid.x * grid.y) for a caller that adds partials of its own before the final sum)
template <class Op, bool LAP, class real>
static int residual_op3d_launch(mgx_ctx* ctx, const real* v, const real* f, const real* a, real* out, const int n[3], const Op& op,
                                double* dev_work, double* dev_sum, bool finalize = true) {
    const dim3 g = krylov_grid(n);
    Op::with_mode(op.mode, [&](auto m) __attribute__((always_inline)) {
        MGX_LAUNCH((residual_op3d_xs_kernel<real, Op, decltype(m)::value, LAP>), g, krylov_block(), 0, ctx->compute, v, f, a, out, n[0], n[1], op,
                   dev_sum ? dev_work : (double*)nullptr);
    });
    MGX_LAUNCH_CHECK();
    return dev_sum && finalize ? krylov_final(ctx, dev_work, (size_t)g.x * g.y, 1, dev_sum) : MGX_OK;
}

// r = the residual (r == NULL: not stored; its boundary is 0), *dev_sumsq = <r, r> (NULL: not summed)
template <class Op, class real>
static int residual_op3d(mgx_ctx* ctx, const real* v, const real* f, const real* a, real* r, const int n[3], const real h[3], real s,
                         double* dev_work, double* dev_sumsq, const char* what, const real* c = nullptr) {
    MGX_REQUIRE(ctx && v && f && (a || !Op::HAS_A) && (c || !Op::HAS_C) && h && (r || dev_sumsq) && (!dev_sumsq || dev_work), MGX_ERR_INVALID, "%s: NULL argument",
                what);
    const double sd = (double)s;
    MGX_TRY_RET(rows_check(n, what, Op::HAS_S ? &sd : nullptr));
    MGX_USE(ctx);
    if (r)  // the boundary of r is 0, as mgx3dxs_residual leaves it
        rim_zero3d_xs<real>(ctx, r, n);
    return residual_op3d_launch<Op, false>(ctx, v, f, a, r, n, make_op<Op, real>(ctx, h, s, c), dev_work, dev_sumsq);
}

// q = A p on the interior, *dev_sum = <p, q>
template <class Op, class real>
static int apply_op_dot3d(mgx_ctx* ctx, const real* p, const real* a, real* q, const int n[3], const real h[3], real s, double* dev_work,
                          double* dev_sum, const char* what, const real* c = nullptr) {
    MGX_REQUIRE(ctx && p && (a || !Op::HAS_A) && (c || !Op::HAS_C) && q && h && dev_work && dev_sum, MGX_ERR_INVALID, "%s: NULL argument", what);
    const double sd = (double)s;
    MGX_TRY_RET(rows_check(n, what, Op::HAS_S ? &sd : nullptr));
    MGX_USE(ctx);
    return residual_op3d_launch<Op, true>(ctx, p, (const real*)nullptr, a, q, n, make_op<Op, real>(ctx, h, s, c), dev_work, dev_sum);
}

}  // namespace mgx
