// mgx_kernels3d.hip -- 3D Poisson multigrid for gfx950 (MI355X), fp32 + fp64: the colour-pass smoothers, Jacobi and the
// one-level composites of the cycle.
//
// Every kernel evaluates the per-point expression of the reference in the reference's
// association order, in `real`, with true IEEE division and without FMA contraction
// (this file is compiled with -ffp-contract=off), so results are bit-identical to the
// serial CPU loops: red-black Gauss-Seidel is order-independent within a colour
// (SURVEY.md section 0, fact 7).
//
// Two array layouts (mgx_kernels3d.hpp):
//   Natural  idx = x + y*sx + z*sx*sy          the reference layout, used at the ABI boundary
//   XSplit   idx = (x>>1) + (x&1)*H + y*sx + z*sx*sy, H = (sx+1)/2
//            every x-row is de-interleaved into its even-x half followed by its odd-x half.
//            In row (y,z) the points of colour c are exactly the half with x parity
//            (c+y+z)&1, so one colour pass of the smoother reads and writes contiguous
//            half-rows: a red+black sweep moves 3 reals per point through HBM (read the
//            other colour, read f of this colour, write this colour) instead of the 6 the
//            interleaved layout needs.  Rows and planes keep their natural order, so z-slabs
//            and ghost planes stay contiguous.
//
// Kernels (reference function each one replaces):
//   relax3d_colour_kernel     one colour of MultiGrid3D::Relax, Natural   N3/MultiGrid3D.cpp:489-567
//   relax3d_zero_colour_kernel  the first red pass of a level that counts as all zeros (both layouts)
//   relax3d_xs_kernel         one colour of MultiGrid3D::Relax, XSplit, with many small workgroups and re-loaded edges (smaller
//                             levels, thin z-ranges; wide levels and long runs go to the pipelined kernels of mgx_pipe3d.hip)
//   jacobi3d_kernel           weighted Jacobi (not in the reference)
// Host side: relax3d_xs_pass chooses the kernel of a colour pass, relax3d / relax3d_from_zero the path of a Relax call (levels
// <= 17^3: mgx_small3d.hip; cache-resident levels: mgx_resident3d.hip), the z-slab forms of the passes, and the one-level
// composites smooth_residual_restrict3d_xs (the way down) and interpolate_correct_relax3d_xs / _block3_xs (the way up), which
// string together the launches of the other units (mgx_host3d.hpp).  The transfers, fills and reductions: mgx_transfer3d.hip;
// CalculateResidual + Restrict fused: mgx_rr3d.hip.
#include "mgx_host3d.hpp"

namespace mgx {

// ------------------------------------------------------------------ relax, one colour, Natural
// One thread per point of the colour.  x = 2*ix + p with p = (colour + y + z) & 1 so that
// (x + y + z) % 2 == colour  (red = 0: N3/MultiGrid3D.cpp:515, black = 1: :544).
template <class real>
__global__ void __launch_bounds__(256) relax3d_colour_kernel(real* __restrict__ v, const real* __restrict__ f, int sx,
                                                             int sy, int sz, real hx2, real hy2, real hz2, int colour) {
    const int y = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int z = 1 + blockIdx.z;
    if (y >= sy - 1) return;
    const int p = (colour + y + z) & 1;
    const int x = 2 * (blockIdx.x * blockDim.x + threadIdx.x) + p;
    if (x < 1 || x >= sx - 1) return;
    const size_t sxy = (size_t)sx * sy;
    const size_t i = x + (size_t)y * sx + (size_t)z * sxy;
    const real O = v[i - 1], E = v[i + 1];
    const real N = v[i - sx], S = v[i + sx];
    const real D = v[i - sxy], U = v[i + sxy];
    v[i] = relax3d_point<real>(O, E, N, S, D, U, f[i], hx2, hy2, hz2);
}

// ------------------------------------------------------------------ relax, first red pass on v = 0
// The coarse error starts every cycle as zero (setToValue(coarse v, 0, true), N3/MultiGrid3D.cpp:634).  The first colour
// pass of the pre-smoothing then reads only zeros: its result is relax3d_point(0, 0, 0, 0, 0, 0, f) -- evaluated as such,
// so the IEEE result (signs of zeros included) is what the generic pass computes from a zeroed array -- and neither the
// zero fill of v nor the read of v is needed: f of the colour is streamed in, v of the colour streamed out.  The other
// colour's interior points are stale afterwards; the pass that follows reads only this colour and rewrites them all.
// Requires the boundary entries of v to be zero in memory (the host layer tracks that).
template <class real, class L>
__global__ void __launch_bounds__(256) relax3d_zero_colour_kernel(real* __restrict__ v, const real* __restrict__ f, int sx, int sy,
                                                                  real hx2, real hy2, real hz2, int colour, int zbeg) {
    const int y = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int z = zbeg + blockIdx.z;  // local plane; `colour` already includes the parity of a slab's global z offset
    if (y >= sy - 1) return;
    const int p = (colour + y + z) & 1;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // x = 2i + p
    const int x = 2 * i + p;
    if (x < 1 || x >= sx - 1) return;
    const Geo<L, real> g(sx, sy);
    const size_t idx = g.row(y, z) + g.pos(x);
    const real zero = (real)0;
    __builtin_nontemporal_store(relax3d_point<real>(zero, zero, zero, zero, zero, zero, f[idx], hx2, hy2, hz2), &v[idx]);
}

// ------------------------------------------------------------------ relax, one colour, XSplit
// Lane j of a wave owns the x-pair {2j, 2j+1} of R consecutive rows and marches through the planes
// [z0, z1) of its z-chunk.  In plane z the point of `colour` in the pair of row y is x = 2j + q,
// q = (colour + y + z) & 1; it lives in half q of the row at index j.  Its six neighbours are of the
// other colour (never written in this pass, so updating in place is race-free):
//   W, E : half 1-q of the same row, indices j-1+q and j+q; one of them is index j ("own"),
//          the other ("side") belongs to the neighbouring lane
//   N, S : half q, index j, rows y-1 / y+1  = the "own" values of the adjacent rows (q flips with y),
//          so inside a thread's R rows they are registers; only the two outer rows are loaded
//   D, U : half q, index j, planes z-1 / z+1 = the "own" values of the previous / next step
//          (q flips with z): the column is carried in registers
// Per step and thread: R streaming loads of v (U), R of f, R side loads and 2 edge-row loads that
// hit in L1/L2, R stores.  All R rows' loads are issued before the first use, which keeps
// R x 16 bytes of HBM traffic in flight per lane.  vin and vout alias the same array; the entries
// read and the entries written are disjoint by colour, which is what makes __restrict__ legitimate.
// The results are written with non-temporal stores: they are next read by the following colour pass, long after
// they would have been evicted, and keeping them out of L2 leaves it to the re-used other-colour rows/planes
// (measured +9 %; non-temporal loads of f or v do not pay).
// ABL != 0 builds diagnostic variants for tools/ablate_relax.py ("relax3d.ablate"; results are WRONG except 16):
// 1 = no f load, 2 = no store (one lane keeps the value alive), 4 = no side / edge-row loads, 8 = no division,
// 16 = plain instead of non-temporal stores (correct results; A/B switch).
template <class real, int TYW, int R, int ABL = 0>
__global__ void __launch_bounds__(64 * TYW)
    relax3d_xs_kernel(const real* __restrict__ vin, real* __restrict__ vout, const real* __restrict__ f, int sx, int sy,
                      int zbeg, int zend, real hx2, real hy2, real hz2, int colour, int zchunk, int gx, int gy,
                      int xcd_mode, int nz1 = 0x7fffffff, int zbeg2 = 0, int zend2 = 0) {
    // nz1, [zbeg2, zend2): a SECOND range of planes in the same launch (the two edge planes of a z-slab, which the neighbours wait
    // for: one launch instead of two) -- the z-chunks from number nz1 on belong to it
    const Geo<XSplit, real> g(sx, sy);
    const int H = g.H;
    const int M = (sx + 1) >> 1;  // entries of the even-x half (the odd-x half has M-1)
    const double rd = relax3d_rd<real>(hx2, hy2, hz2);  // fp32: the division by multiplication (relax3d_point_rd)
    // 1-D grid decoded to (bx, by, bz).  Workgroups are dealt round-robin over the 8 XCDs
    // (MI355X_MICROARCH.md: blocks b and b+8 share an XCD, each XCD has its own 4 MiB L2).
    //   xcd_mode 0: plain order, x fastest, then y tiles, then z-chunks
    //   xcd_mode 1: every XCD gets one contiguous run of that order
    //   xcd_mode 2: every XCD owns a contiguous set of xy tiles (a y-slab) and walks through its
    //               z-chunks in order, so the two planes that consecutive z-chunks both read, and
    //               the edge rows of y-adjacent tiles, are still in that XCD's L2 when re-read.
    // Speed only: any mapping gives the same result (the grid holds 8*ceil(T/8)*gz blocks in mode 2).
    unsigned b = blockIdx.x;
    int bx, by, bz;
    if (xcd_mode == 2) {
        const unsigned T = gx * gy, Tx = (T + 7u) >> 3, k = b & 7u, i = b >> 3;
        const unsigned tile = k * Tx + i % Tx;
        if (tile >= T) return;
        bz = i / Tx;
        bx = tile % gx;
        by = tile / gx;
    } else {
        if (xcd_mode == 1) {
            const unsigned nb = gridDim.x, k = b & 7u, per = nb >> 3, rem = nb & 7u;
            b = k * per + (k < rem ? k : rem) + (b >> 3);
        }
        bx = b % gx;
        by = (b / gx) % gy;
        bz = b / (gx * gy);
    }
    const int j = bx * 64 + threadIdx.x;
    // one wave per row group: y (hence the colour parity q and every row offset) is wave-uniform -> SGPRs
    const int y0 = 1 + (by * TYW + __builtin_amdgcn_readfirstlane(threadIdx.y)) * R;
    if (y0 >= sy - 1 || j >= M - 1) return;  // x = 2j+q <= sx-2 needs j <= M-2
    const int nrows = min(R, sy - 1 - y0);    // rows y0 .. y0+nrows-1 are interior
    // planes [zbeg, zend) of the local array are updated (1 .. sz-2 for a whole grid; the owned planes of
    // a z-slab, whose neighbours below / above are ghost planes); `colour` already includes the parity of
    // the slab's global z offset
    if (bz >= nz1) {
        bz -= nz1;
        zbeg = zbeg2;
        zend = zend2;
    }
    const int z0 = zbeg + bz * zchunk;
    const int z1 = min(z0 + zchunk, zend);
    if (z0 >= z1) return;
    const size_t sxy = g.PL;
    const int P = g.P;
    // row bases at plane z0.  Row y0+nrows may be the boundary row sy-1: it is loaded like any other row
    // because its "own" value is the S neighbour of the last interior row; rows past sy-1 are clamped
    // onto it (loads stay valid, nothing is stored for r >= nrows)
    size_t rowb[R];
#pragma unroll
    for (int r = 0; r < R; r++) rowb[r] = g.row(min(y0 + r, sy - 1), z0);
    int q = (colour + y0 + z0) & 1;  // parity of row r is q ^ (r & 1)
    real c_prev[R], c_cur[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int qr = q ^ (r & 1);
        c_prev[r] = vin[rowb[r] - sxy + qr * H + j];   // (half q_r,   j, plane z0-1)
        c_cur[r] = vin[rowb[r] + (1 - qr) * H + j];    // (half 1-q_r, j, plane z0)
    }
    // EARLY (ABL & 32): the values that come from outside the thread's own column -- N of row 0, S of row R-1 and
    // the side value of the wave's edge lanes -- are loaded one plane ahead, in the same step in which the
    // neighbouring wave streams exactly those entries in as its U.  Both requests then reach L2 together (one
    // fill) instead of a full step apart, by which time the XCD's waves have streamed more than the 4 MiB of L2
    // through it and the line has been evicted (PMC: these re-loads were 27-50 % misses).
    constexpr bool EARLY = (ABL & 32) != 0;
    auto side_edge = [&](int r, int qr) -> bool {  // does this lane load its side value from memory?
        return qr ? (threadIdx.x == 63 || j == M - 2) : (threadIdx.x == 0);
    };
    auto side_addr = [&](int r, int qr, size_t plane_off) -> size_t {
        return rowb[r] + plane_off + (1 - qr) * H + j + (qr ? 1 : -1) + (qr | j ? 0 : M);
    };
    real Nnext = 0, Snext = 0, side_next[R];
    size_t rowS = g.row(min(y0 + R, sy - 1), z0);  // the row below the thread's rows (clamped: never past the plane)
    if (EARLY) {
        Nnext = vin[rowb[0] - P + q * H + j];
        Snext = vin[rowS + (q ^ ((R - 1) & 1)) * H + j];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int qr = q ^ (r & 1);
            side_next[r] = 0;
            if (side_edge(r, qr)) side_next[r] = vin[side_addr(r, qr, 0)];
        }
    }
    for (int z = z0; z < z1; z++) {
        real U[R], side[R], fv[R];
        real Nedge, Sedge;
        // lane j = 0 with q_r = 0 (x = 0, a boundary point that is never written) would read index -1:
        // it reads index M-1 of half 0 instead and the result is discarded
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int qr = q ^ (r & 1);
            const int hq = qr * H;
            U[r] = vin[rowb[r] + sxy + hq + j];
            fv[r] = (ABL & 1) ? (real)1 : f[rowb[r] + hq + j];
        }
        if (EARLY) {
            Nedge = Nnext;
            Sedge = Snext;
            // plane z+1 (parities flipped); past the last plane of the chunk the values are not used, the loads stay
            // inside the array (plane z1 <= sz-1 exists)
            Nnext = vin[rowb[0] + sxy - P + (q ^ 1) * H + j];
            rowS += sxy;
            Snext = vin[rowS + (q ^ 1 ^ ((R - 1) & 1)) * H + j];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int qr = q ^ (r & 1);
                const real nb = qr ? __shfl_down(c_cur[r], 1, 64) : __shfl_up(c_cur[r], 1, 64);
                side[r] = side_edge(r, qr) ? side_next[r] : nb;
                if (side_edge(r, qr ^ 1)) side_next[r] = vin[side_addr(r, qr ^ 1, sxy)];
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int qr = q ^ (r & 1);
                if (ABL & 4) {
                    side[r] = c_cur[r];
                } else {
                    // the side value is the "own" value of the neighbouring lane: wave shuffle instead of a second load;
                    // neighbour lane: j+1 when q_r = 1, j-1 when q_r = 0 (q_r is wave-uniform).  The wave's edge lane,
                    // and the last active lane (its neighbour j+1 = M-1 holds the boundary entry but has exited), load.
                    const real nb = qr ? __shfl_down(c_cur[r], 1, 64) : __shfl_up(c_cur[r], 1, 64);
                    side[r] = side_edge(r, qr) ? vin[side_addr(r, qr, 0)] : nb;
                }
            }
            Nedge = (ABL & 4) ? c_cur[0] : vin[rowb[0] - P + q * H + j];
            Sedge = (ABL & 4) ? c_cur[R - 1] : vin[rowb[R - 1] + P + (q ^ ((R - 1) & 1)) * H + j];
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int qr = q ^ (r & 1);
            const real W = qr ? c_cur[r] : side[r];
            const real E = qr ? side[r] : c_cur[r];
            const real N = r == 0 ? Nedge : c_cur[r - 1];
            const real S = r == R - 1 ? Sedge : c_cur[r + 1];
            real out = relax3d_point_rd<real>(W, E, N, S, c_prev[r], U[r], fv[r], hx2, hy2, hz2, rd);
            if (ABL & 8) out = (W + E + N + S + c_prev[r] + U[r] - fv[r]) * hx2;
            if (ABL & 2) {
                if (out == (real)123456.789) vout[rowb[r] + qr * H + j] = out;
            } else if ((qr | j) && r < nrows) {  // x = 2j+q_r >= 1
                if (ABL & 16) vout[rowb[r] + qr * H + j] = out;
                else __builtin_nontemporal_store(out, &vout[rowb[r] + qr * H + j]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            c_prev[r] = c_cur[r];
            c_cur[r] = U[r];
            rowb[r] += sxy;
        }
        q ^= 1;
    }
}

// ------------------------------------------------------------------ weighted Jacobi (addition)
// north_star names weighted Jacobi next to red-black Gauss-Seidel; the reference only has the latter (Jacobi is
// pseudo-code in the thesis).  One sweep: vout = v + omega * (u - v), u = the Gauss-Seidel value of
// relax3d_point evaluated on the OLD iterate for every interior point (boundary copied).  Parity is unpinned by
// the reference; the oracle restates this expression and the tests require bit-equality with it.
template <class real, class L>
__global__ void __launch_bounds__(256) jacobi3d_kernel(const real* __restrict__ v, real* __restrict__ vout,
                                                       const real* __restrict__ f, int sx, int sy, int sz, real hx2, real hy2,
                                                       real hz2, real omega) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    const int z = blockIdx.z;
    if (x >= sx || y >= sy) return;
    const Geo<L, real> g(sx, sy);
    const int H = g.H, P = g.P;
    const size_t sxy = g.PL;
    const size_t row = g.row(y, z);
    const size_t i = row + L::pos(x, H);
    const real c = v[i];
    if (x == 0 || x == sx - 1 || y == 0 || y == sy - 1 || z == 0 || z == sz - 1) {
        vout[i] = c;
        return;
    }
    const real u = relax3d_point<real>(v[row + L::pos(x - 1, H)], v[row + L::pos(x + 1, H)], v[i - P], v[i + P], v[i - sxy],
                                       v[i + sxy], f[i], hx2, hy2, hz2);
    vout[i] = c + omega * (u - c);
}

// =========================================================================== host side
template <class real>
static int relax3d_natural(mgx_ctx* ctx, real* v, const real* f, const int n[3], real hx2, real hy2, real hz2, int ncycles) {
    dim3 g(ceil_div((n[0] + 1) / 2, 64), ceil_div(n[1] - 2, 4), n[2] - 2);
    for (int k = 0; k < ncycles; k++)
        for (int colour = 0; colour < 2; colour++)
            MGX_LAUNCH((relax3d_colour_kernel<real>), g, blk(), 0, ctx->compute, v, f, n[0], n[1], n[2], hx2, hy2,
                               hz2, colour);
    return MGX_OK;
}

template <class real, int TYW, int R>
static void launch_xs(mgx_ctx* ctx, real* v, const real* f, int sx, int sy, int zbeg, int zend, real hx2, real hy2,
                      real hz2, int colour, int zchunk) {
    const int M = (sx + 1) / 2;
    const int gx = ceil_div(M - 1, 64), gy = ceil_div(sy - 2, TYW * R), gz = ceil_div(zend - zbeg, zchunk);
    const unsigned nblocks = ctx->relax_xcd == 2 ? 8u * ((gx * gy + 7) / 8) * gz : (unsigned)gx * gy * gz;
#ifdef MGX_DIAGNOSTICS
    if (TYW == 4 && R == 4 && ctx->relax_ablate) {  // diagnostics only
#define MGX_ABL(A)                                                                                                   \
    case A:                                                                                                          \
        MGX_LAUNCH((relax3d_xs_kernel<real, 4, 4, A>), dim3(nblocks), dim3(64, 4, 1), 0, ctx->compute,          \
                           (const real*)v, v, f, sx, sy, zbeg, zend, hx2, hy2, hz2, colour, zchunk, gx, gy, ctx->relax_xcd); \
        return;
        switch (ctx->relax_ablate) {
            MGX_ABL(1) MGX_ABL(2) MGX_ABL(3) MGX_ABL(4) MGX_ABL(5) MGX_ABL(7) MGX_ABL(8) MGX_ABL(12) MGX_ABL(15) MGX_ABL(16) MGX_ABL(32)
            default: break;
        }
#undef MGX_ABL
    }
#endif
    note_relax_kernel<real>(ctx, "relax3d_xs_kernel", TYW, R, 0);
    MGX_LAUNCH((relax3d_xs_kernel<real, TYW, R>), dim3(nblocks), dim3(64, TYW, 1), 0, ctx->compute,
                       (const real*)v, v, f, sx, sy, zbeg, zend, hx2, hy2, hz2, colour, zchunk, gx, gy, ctx->relax_xcd);
}

template <class real, int TYW>
static void launch_xs_rows(mgx_ctx* ctx, real* v, const real* f, int sx, int sy, int zbeg, int zend, real hx2, real hy2,
                           real hz2, int colour, int zchunk, int rows) {
    switch (rows) {
        case 1: launch_xs<real, TYW, 1>(ctx, v, f, sx, sy, zbeg, zend, hx2, hy2, hz2, colour, zchunk); break;
        case 2: launch_xs<real, TYW, 2>(ctx, v, f, sx, sy, zbeg, zend, hx2, hy2, hz2, colour, zchunk); break;
        case 8: launch_xs<real, TYW, 8>(ctx, v, f, sx, sy, zbeg, zend, hx2, hy2, hz2, colour, zchunk); break;
        default: launch_xs<real, TYW, 4>(ctx, v, f, sx, sy, zbeg, zend, hx2, hy2, hz2, colour, zchunk); break;
    }
}

// one colour pass over the local planes [zbeg, zend) of an x-split array with sx x sy rows
template <class real>
static void relax3d_xs_pass(mgx_ctx* ctx, real* v, const real* f, int sx, int sy, int zbeg, int zend, real hx2, real hy2,
                            real hz2, int colour) {
    if (zend <= zbeg || sx < 3 || sy < 3) return;
    if (ctx->relax_lds != 0 && relax3d_xs_pass_lds<real>(ctx, v, f, sx, sy, zbeg, zend, hx2, hy2, hz2, colour)) return;
    int ty = ctx->relax_ty, rows = ctx->relax_rows, zchunk = ctx->relax_zchunk;
    // levels of 129-point rows (one wave wide), fp64, library defaults: eight waves of two rows, runs of two planes -- 14.9 against 16.0 us
    // per sweep at 129^3 (tools/sweep_relax.py --n 129; the shapes differ by a few per cent, the level is latency, not bytes)
    if (sizeof(real) == 8 && (sx + 1) / 2 - 1 == 64 && sy - 2 >= 64 && zend - zbeg >= 16 && ty == 4 && rows == 4 && zchunk <= 0) {
        ty = 8;
        rows = 2;
        zchunk = 2;
    }
    while (rows > 1 && rows * ty > sy - 2) rows >>= 1;  // small levels: do not idle most of a block
    while (ty > 1 && rows * ty > sy - 2) ty >>= 1;
    if (zchunk <= 0) {
        const long long tiles = (long long)ceil_div((sx + 1) / 2 - 1, 64) * ceil_div(sy - 2, ty * rows);
        zchunk = 4;  // measured best at 513^3 (tools/sweep_relax.py): short chunks, many blocks
        while (zchunk > 1 && tiles * ceil_div(zend - zbeg, zchunk) < 8LL * ctx->num_cus) zchunk >>= 1;
    }
    switch (ty) {
        case 1: launch_xs_rows<real, 1>(ctx, v, f, sx, sy, zbeg, zend, hx2, hy2, hz2, colour, zchunk, rows); break;
        case 2: launch_xs_rows<real, 2>(ctx, v, f, sx, sy, zbeg, zend, hx2, hy2, hz2, colour, zchunk, rows); break;
        case 8: launch_xs_rows<real, 8>(ctx, v, f, sx, sy, zbeg, zend, hx2, hy2, hz2, colour, zchunk, rows); break;
        default: launch_xs_rows<real, 4>(ctx, v, f, sx, sy, zbeg, zend, hx2, hy2, hz2, colour, zchunk, rows); break;
    }
}

// one colour pass over TWO short runs of planes [zb1, ze1) and [zb2, ze2) in ONE launch of relax3d_xs_kernel (the bottom and the top
// edge of a z-slab: a middle rank relaxes them first, in front of its ghost exchange); false = not taken (a run of 8 or more planes:
// the caller makes two passes)
template <class real>
static bool relax3d_xs_pass2(mgx_ctx* ctx, real* v, const real* f, int sx, int sy, int zb1, int ze1, int zb2, int ze2, real hx2, real hy2,
                             real hz2, int colour) {
    const int pmin = ctx->relax_lds == 0 ? (1 << 30) : pipe_min_planes<real>(sx);  // runs the pipelined kernel would take: two passes
    if (!ctx->slab_edges_merged || ze1 <= zb1 || ze2 <= zb2 || ze1 - zb1 >= pmin || ze2 - zb2 >= pmin || sx < 3 || sy < 3) return false;
    constexpr int TYW = 4, R = 4;
    const int zchunk = 1;
    const int M = (sx + 1) / 2;
    const int gx = ceil_div(M - 1, 64), gy = ceil_div(sy - 2, TYW * R), gz1 = ze1 - zb1, gz2 = ze2 - zb2;
    note_relax_kernel<real>(ctx, "relax3d_xs_kernel", TYW, R, 0);
    MGX_LAUNCH((relax3d_xs_kernel<real, TYW, R>), dim3((unsigned)gx * gy * (gz1 + gz2)), dim3(64, TYW, 1), 0, ctx->compute, (const real*)v, v, f,
                       sx, sy, zb1, ze1, hx2, hy2, hz2, colour, zchunk, gx, gy, 0, gz1, zb2, ze2);
    return true;
}

// `ncycles` red-black sweeps = 2*ncycles colour passes.  On large levels the passes are time-skewed over
// z-slabs ("wavefront" order): slab by slab, pass s runs on the planes [a-s, a+B-s) right after pass s-1 ran
// on [a-s+1, a+B-s+1).  Pass s at plane z needs pass s-1 only at planes z-1, z, z+1, so every point still sees
// exactly the values it would see with whole-grid passes (bit-identical result), but a slab's v and f
// (B planes, sized to sit in the 256 MiB Infinity Cache) are re-used by all passes before they leave the
// chip: HBM sees about one read of v and f and one write of v per call instead of one per sweep.
template <class real>
static int relax3d_xsplit(mgx_ctx* ctx, real* v, const real* f, const int n[3], real hx2, real hy2, real hz2, int ncycles) {
    const int npass = 2 * ncycles, zb = 1, ze = n[2] - 1;
    const size_t plane_bytes = (size_t)n[0] * n[1] * sizeof(real);
    int B = ctx->relax_wave_planes;
    if (B < 0) {  // automatic: v + f of a slab (plus the skew margin) in about 64 MiB
        B = (int)((64u << 20) / (2 * plane_bytes));
        if (B * 4 > ze - zb || B < 2 * npass) B = 0;  // small level, or slabs thinner than the skew: whole-grid passes
    }
    if (B <= 0 || npass < 2) {
        for (int s = 0; s < npass; s++) relax3d_xs_pass<real>(ctx, v, f, n[0], n[1], zb, ze, hx2, hy2, hz2, s & 1);
        return MGX_OK;
    }
    for (int a = zb; a < ze + npass - 1; a += B)
        for (int s = 0; s < npass; s++) {
            const int lo = a - s > zb ? a - s : zb;
            const int hi = a + B - s < ze ? a + B - s : ze;
            if (hi > lo) relax3d_xs_pass<real>(ctx, v, f, n[0], n[1], lo, hi, hx2, hy2, hz2, s & 1);
        }
    return MGX_OK;
}

template <class real, class L>
int relax3d(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], int ncycles) {
    MGX_REQUIRE(ctx && v && f && h, MGX_ERR_INVALID, "relax3d: NULL argument");
    MGX_USE(ctx);
    int st = check_n3(n, "relax3d");
    if (st) return st;
    MGX_REQUIRE(ncycles >= 0, MGX_ERR_INVALID, "relax3d: ncycles = %d < 0", ncycles);
    const real hx2 = h[0] * h[0], hy2 = h[1] * h[1], hz2 = h[2] * h[2];  // N3/MultiGrid3D.cpp:498-500
    if (ncycles > 0 && n[0] <= SMALL_MAX && n[1] <= SMALL_MAX && n[2] <= SMALL_MAX && ctx->relax_small) {
        return relax3d_small<real, L>(ctx, v, f, n, hx2, hy2, hz2, ncycles);  // mgx_small3d.hip
    }
    if (L::xsplit && ncycles > 0 && relax3d_resident_takes(ctx, n, ncycles)) st = relax3d_resident<real>(ctx, v, f, n, hx2, hy2, hz2, ncycles, 0);
    else if (L::xsplit) st = relax3d_xsplit<real>(ctx, v, f, n, hx2, hy2, hz2, ncycles);
    else st = relax3d_natural<real>(ctx, v, f, n, hx2, hy2, hz2, ncycles);
    if (st) return st;
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// v := 0 (everywhere), then `ncycles` red-black sweeps: the start of the pre-smoothing of a coarse level
// (N3/MultiGrid3D.cpp:634 + :626).  rim_is_zero != 0: the caller vouches that the boundary entries (and, x-split, the pad
// entries) of v are zero already; then nothing is filled and the first red pass does not read v.
template <class real, class L>
int relax3d_from_zero(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], int ncycles, int rim_is_zero) {
    MGX_REQUIRE(ctx && v && f && h, MGX_ERR_INVALID, "relax_from_zero3d: NULL argument");
    MGX_USE(ctx);
    int st = check_n3(n, "relax_from_zero3d");
    if (st) return st;
    MGX_REQUIRE(ncycles >= 0, MGX_ERR_INVALID, "relax_from_zero3d: ncycles = %d < 0", ncycles);
    const bool small = n[0] <= SMALL_MAX && n[1] <= SMALL_MAX && n[2] <= SMALL_MAX && ctx->relax_small;
    if (!rim_is_zero || ncycles == 0 || small || !ctx->relax_zero_first) {
        const size_t elems = Geo<L, real>(n[0], n[1]).PL * (size_t)n[2];
        st = fill_zero(ctx, v, elems * sizeof(real));
        if (st) return st;
        return relax3d<real, L>(ctx, v, f, n, h, ncycles);
    }
    const real hx2 = h[0] * h[0], hy2 = h[1] * h[1], hz2 = h[2] * h[2];  // :498-500
    if (L::xsplit && relax3d_resident_takes(ctx, n, ncycles)) {  // all passes in one launch, the tile starts as zeros
        st = relax3d_resident<real>(ctx, v, f, n, hx2, hy2, hz2, ncycles, 1);
        if (st) return st;
        MGX_LAUNCH_CHECK();
        return MGX_OK;
    }
    int s0 = 1;
    if (L::xsplit && relax3d_xs_first_sweep_zero<real>(ctx, v, f, n[0], n[1], n[2], hx2, hy2, hz2)) s0 = 2;  // red and black in one launch
    else
        MGX_LAUNCH((relax3d_zero_colour_kernel<real, L>), dim3(ceil_div((n[0] + 1) / 2, 64), ceil_div(n[1] - 2, 4), n[2] - 2), blk(), 0,
                           ctx->compute, v, f, n[0], n[1], hx2, hy2, hz2, 0, 1);
    for (int s = s0; s < 2 * ncycles; s++) {
        if (L::xsplit) relax3d_xs_pass<real>(ctx, v, f, n[0], n[1], 1, n[2] - 1, hx2, hy2, hz2, s & 1);
        else
            MGX_LAUNCH((relax3d_colour_kernel<real>), dim3(ceil_div((n[0] + 1) / 2, 64), ceil_div(n[1] - 2, 4), n[2] - 2), blk(), 0,
                               ctx->compute, v, f, n[0], n[1], n[2], hx2, hy2, hz2, s & 1);
    }
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// The fused launch alone on a z-slab (or the whole grid): black pass of the GLOBAL fine planes [2 pzbeg - 1, 2 pzend - 1] +
// residual + restrict into the GLOBAL coarse planes [pzbeg, pzend).  n / cn global sizes, v / f start at global plane fzoff,
// coarse_f at global coarse plane czoff.  Reads the red values of the fine planes [2 pzbeg - 3, 2 pzend + 1] (clipped to the
// grid) and f; the coarse planes are zeroed first (boundary entries stay 0).
template <class real>
int relax_rr3d_slab(mgx_ctx* ctx, real* v, const real* f, const int n[3], int fzoff, const real h[3], int mode, real* coarse_f,
                    const int cn[3], int czoff, int pzbeg, int pzend) {
    MGX_TRY_RET(check_rr_args(ctx, ctx && v && f && h && coarse_f, n, cn, "relax_rr_slab"));
    MGX_REQUIRE(mode == MGX_RESIDUAL_REF_COMPAT || mode == MGX_RESIDUAL_CORRECT, MGX_ERR_INVALID, "relax_rr_slab: bad mode %d", mode);
    MGX_REQUIRE(pzbeg >= 1 && pzend <= cn[2] - 1 && pzbeg < pzend && czoff >= 0 && czoff <= pzbeg && fzoff >= 0 && (fzoff & 1) == 0 &&
                    fzoff <= (2 * pzbeg - 3 > 0 ? 2 * pzbeg - 3 : 0),
                MGX_ERR_INVALID, "relax_rr_slab: coarse planes [%d, %d) with offsets %d / %d", pzbeg, pzend, fzoff, czoff);
    MGX_REQUIRE(relax_rr3d_xs_takes(ctx, n, cn, sizeof(real)), MGX_ERR_INVALID, "relax_rr_slab: the level is not taken (ask relax_rr_takes)");
    const Geo<XSplit, real> gc(cn[0], cn[1]);
    MGX_TRY_RET(fill_zero(ctx, coarse_f + gc.PL * (size_t)(pzbeg - czoff), gc.PL * (size_t)(pzend - pzbeg) * sizeof(real)));
    MGX_REQUIRE(relax_rr3d_xs_launch<real>(ctx, v, f, n, h, mode, coarse_f, cn, fzoff, czoff, pzbeg, pzend), MGX_ERR_INVALID,
                "relax_rr_slab: launch refused");
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// The way down on one level: Relax(ncycles) (from_zero: on v = 0, as relax3d_from_zero), CalculateResidual, Restrict
// (N3/MultiGrid3D.cpp:626-632).  Where the level takes it the last black pass runs inside the residual+restrict launch
// (relax_rr3d_xs_kernel); otherwise the operators are called one after the other.
template <class real>
int smooth_residual_restrict3d_xs(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], int ncycles, int from_zero,
                                  int v_rim_is_zero, int mode, real* coarse_f, const int cn[3], int coarse_rim_is_zero) {
    MGX_TRY_RET(check_rr_args(ctx, ctx && v && f && h && coarse_f, n, cn, "smooth_residual_restrict3d"));
    MGX_REQUIRE(ncycles >= 0, MGX_ERR_INVALID, "smooth_residual_restrict3d: ncycles = %d < 0", ncycles);
    MGX_REQUIRE(mode == MGX_RESIDUAL_REF_COMPAT || mode == MGX_RESIDUAL_CORRECT, MGX_ERR_INVALID,
                "smooth_residual_restrict3d: bad mode %d", mode);
    ctx->last_rr_kernel[0] = 0;
    ctx->last_block3_kernel[0] = 0;
    if (ncycles < 1 || !relax_rr3d_xs_takes(ctx, n, cn, sizeof(real))) {
        MGX_TRY_RET((from_zero ? relax3d_from_zero<real, XSplit>(ctx, v, f, n, h, ncycles, v_rim_is_zero) : relax3d<real, XSplit>(ctx, v, f, n, h, ncycles)));
        return residual_restrict3d<real, XSplit>(ctx, v, f, n, h, mode, coarse_f, cn, coarse_rim_is_zero != 0);
    }
    const real hx2 = h[0] * h[0], hy2 = h[1] * h[1], hz2 = h[2] * h[2];  // :498-500
    int s = 0;
    if (from_zero) {
        if (v_rim_is_zero && ctx->relax_zero_first) {  // relax3d_from_zero: the first red pass does not read v
            if (2 * ncycles - 1 >= 2 && relax3d_xs_first_sweep_zero<real>(ctx, v, f, n[0], n[1], n[2], hx2, hy2, hz2)) {
                s = 2;  // the whole first sweep in one launch
            } else {
                MGX_LAUNCH((relax3d_zero_colour_kernel<real, XSplit>), dim3(ceil_div((n[0] + 1) / 2, 64), ceil_div(n[1] - 2, 4), n[2] - 2),
                                   blk(), 0, ctx->compute, v, f, n[0], n[1], hx2, hy2, hz2, 0, 1);
                s = 1;
            }
        } else {
            MGX_TRY_RET(fill_zero(ctx, v, Geo<XSplit, real>(n[0], n[1]).PL * (size_t)n[2] * sizeof(real)));
        }
    }
    // the last three passes are R, B, R; the rr kernel's black pass overwrites the B values without reading them, so one launch
    // that reads black and f and stores red only (in place) stands for the three (mgx_block3d.hip)
    const bool b3 = !from_zero && 2 * ncycles - 1 - s >= 3 && relax_block3_takes(ctx, n, sizeof(real), 1);
    for (; s < 2 * ncycles - 1 - (b3 ? 3 : 0); s++) relax3d_xs_pass<real>(ctx, v, f, n[0], n[1], 1, n[2] - 1, hx2, hy2, hz2, s & 1);
    if (b3) relax3d_xs_block3_launch<real>(ctx, v, v, f, n, hx2, hy2, hz2, 0, false);
    if (!coarse_rim_is_zero) MGX_TRY_RET(fill_zero(ctx, coarse_f, Geo<XSplit, real>(cn[0], cn[1]).PL * (size_t)cn[2] * sizeof(real)));
    MGX_REQUIRE(relax_rr3d_xs_launch<real>(ctx, v, f, n, h, mode, coarse_f, cn, 0, 0, 1, cn[2] - 1), MGX_ERR_INVALID,
                "smooth_residual_restrict3d: the fused launch refused a level it had accepted");
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// ------------------------------------------------------------------ z-slab forms (multi-GPU)
// A slab is a local array of consecutive z-planes of an (sx, sy, szg) level, starting at global plane
// zoff, x-split layout.  Planes the caller does not list as "to update" act as ghost / boundary planes.
template <class real>
int relax3d_colour_slab(mgx_ctx* ctx, real* v, const real* f, int sx, int sy, const real h[3], int colour, int zbeg,
                        int zend, int zoff) {
    MGX_REQUIRE(ctx && v && f && h, MGX_ERR_INVALID, "relax_colour_slab: NULL argument");
    MGX_USE(ctx);
    MGX_REQUIRE(valid_size(sx) && valid_size(sy), MGX_ERR_SIZE, "relax_colour_slab: sizes %d x %d are not odd and >= 3", sx, sy);
    MGX_REQUIRE((colour == 0 || colour == 1) && zbeg >= 1 && zend >= zbeg && zoff >= 0, MGX_ERR_INVALID,
                "relax_colour_slab: bad colour / plane range");
    const real hx2 = h[0] * h[0], hy2 = h[1] * h[1], hz2 = h[2] * h[2];
    relax3d_xs_pass<real>(ctx, v, f, sx, sy, zbeg, zend, hx2, hy2, hz2, (colour + zoff) & 1);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// the same for the two edges of a slab, local planes [zb1, ze1) and [zb2, ze2), in one launch where both are short
template <class real>
int relax3d_colour_slab2(mgx_ctx* ctx, real* v, const real* f, int sx, int sy, const real h[3], int colour, int zb1, int ze1, int zb2,
                         int ze2, int zoff) {
    MGX_REQUIRE(ctx && v && f && h, MGX_ERR_INVALID, "relax_colour_slab2: NULL argument");
    MGX_USE(ctx);
    MGX_REQUIRE(valid_size(sx) && valid_size(sy), MGX_ERR_SIZE, "relax_colour_slab2: sizes %d x %d are not odd and >= 3", sx, sy);
    MGX_REQUIRE((colour == 0 || colour == 1) && zb1 >= 1 && ze1 >= zb1 && zb2 >= ze1 && ze2 >= zb2 && zoff >= 0, MGX_ERR_INVALID,
                "relax_colour_slab2: bad colour / plane ranges");
    const real hx2 = h[0] * h[0], hy2 = h[1] * h[1], hz2 = h[2] * h[2];
    const int c = (colour + zoff) & 1;
    if (!relax3d_xs_pass2<real>(ctx, v, f, sx, sy, zb1, ze1, zb2, ze2, hx2, hy2, hz2, c)) {
        relax3d_xs_pass<real>(ctx, v, f, sx, sy, zb1, ze1, hx2, hy2, hz2, c);
        relax3d_xs_pass<real>(ctx, v, f, sx, sy, zb2, ze2, hx2, hy2, hz2, c);
    }
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// the first colour pass on a slab whose v counts as all zeros (relax3d_zero_colour_kernel): local planes [zbeg, zend)
template <class real>
int relax3d_zero_colour_slab(mgx_ctx* ctx, real* v, const real* f, int sx, int sy, const real h[3], int colour, int zbeg, int zend,
                             int zoff) {
    MGX_REQUIRE(ctx && v && f && h, MGX_ERR_INVALID, "relax_zero_colour_slab: NULL argument");
    MGX_USE(ctx);
    MGX_REQUIRE(valid_size(sx) && valid_size(sy), MGX_ERR_SIZE, "relax_zero_colour_slab: sizes %d x %d are not odd and >= 3", sx, sy);
    MGX_REQUIRE((colour == 0 || colour == 1) && zbeg >= 1 && zend >= zbeg && zoff >= 0, MGX_ERR_INVALID,
                "relax_zero_colour_slab: bad colour / plane range");
    if (zend == zbeg) return MGX_OK;
    const real hx2 = h[0] * h[0], hy2 = h[1] * h[1], hz2 = h[2] * h[2];
    MGX_LAUNCH((relax3d_zero_colour_kernel<real, XSplit>), dim3(ceil_div((sx + 1) / 2, 64), ceil_div(sy - 2, 4), zend - zbeg), blk(), 0,
                       ctx->compute, v, f, sx, sy, hx2, hy2, hz2, (colour + zoff) & 1, zbeg);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// v += Interpolate(coarse_v) on the interior, then `ncycles` >= 1 red-black sweeps (N3/MultiGrid3D.cpp:638-645), x-split
// layout.  On levels wide enough for the pipelined smoother most of the correction never goes through memory: the set P
// (the cells on the edges of the smoother's workgroup tiles, about 1/8 of the black points) is corrected in place, the
// first red pass reads every other black value through the correction (relax3d_xs_pipe_kernel, VAR = 2), and the black
// pass that follows recomputes all black interior points from red.  Elsewhere: the black points are corrected in place,
// then the sweeps.  Both give the bits of interpolate_correct + relax.

// Does a call with a partner array run the way up's passes 2, 3, 4 (B, R, B) as one launch (relax3d_xs_block3_kernel, both
// colours stored)?  Levels that take the correcting red pass and the three-pass launch's rule (fp64, from 385-point rows on),
// two sweeps or more.
static bool block3_up_takes(const mgx_ctx* ctx, const int n[3], size_t elem, int ncycles) {
    return ncycles >= 2 && corr_fused_takes(ctx, n[0], n[1], n[2], n[2] - 2) && relax_block3_takes(ctx, n, elem, 2);
}

// Does the way up run R', B, R as ONE in-place launch that reads black through the correction and stores red only
// (relax3d_xs_block3_kernel, CORR), followed by plain passes from B on?  The levels of block3_up_takes, under a switch of its own
// ("relax3d.block3_corr").
static bool block3_corr_takes(const mgx_ctx* ctx, const int n[3], size_t elem, int ncycles) {
    return ncycles >= 2 && corr_fused_takes(ctx, n[0], n[1], n[2], n[2] - 2) && relax_block3_takes(ctx, n, elem, 4);
}

// v += Interpolate(coarse_v), then `ncycles` sweeps, with the passes R', B, R in one launch where block3_corr_takes says so: no
// partner array, no face copy, nothing of v but its red interior points written by that launch.  Elsewhere as
// interpolate_correct_relax3d_xs without a partner.
template <class real>
int interpolate_correct_relax3d_xs(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], const real* coarse_v,
                                   const int cn[3], int ncycles, real* w = nullptr, int w_rim_valid = 0);
template <class real>
int interpolate_correct_relax_block3_xs(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], const real* coarse_v,
                                        const int cn[3], int ncycles) {
    MGX_REQUIRE(ctx && v && f && h && coarse_v, MGX_ERR_INVALID, "interpolate_correct_relax_block3: NULL argument");
    MGX_USE(ctx);
    int st = check_n3(n, "interpolate_correct_relax_block3");
    if (st) return st;
    st = check_coarse3(n, cn, "interpolate_correct_relax_block3");
    if (st) return st;
    MGX_REQUIRE(ncycles >= 1, MGX_ERR_INVALID, "interpolate_correct_relax_block3: ncycles = %d < 1", ncycles);
    if (!block3_corr_takes(ctx, n, sizeof(real), ncycles)) return interpolate_correct_relax3d_xs<real>(ctx, v, f, n, h, coarse_v, cn, ncycles, nullptr, 0);
    ctx->last_corr_kernel[0] = 0;
    const real hx2 = h[0] * h[0], hy2 = h[1] * h[1], hz2 = h[2] * h[2];  // :498-500
    relax3d_xs_block3_launch<real>(ctx, v, v, f, n, hx2, hy2, hz2, 0, false, coarse_v, cn);
    for (int s = 3; s < 2 * ncycles; s++) relax3d_xs_pass<real>(ctx, v, f, n[0], n[1], 1, n[2] - 1, hx2, hy2, hz2, s & 1);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// w != nullptr: a second array of the level's size as ping-pong partner for the sweeps (mgx3dxs_relax_pp); on the levels
// block3_up_takes, the scratch array between the correcting red pass and the three-pass launch.  w_rim_valid != 0: the caller
// vouches that w's boundary entries equal v's.
template <class real>
int interpolate_correct_relax3d_xs(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], const real* coarse_v,
                                   const int cn[3], int ncycles, real* w, int w_rim_valid) {
    MGX_REQUIRE(ctx && v && f && h && coarse_v, MGX_ERR_INVALID, "interpolate_correct_relax3d: NULL argument");
    MGX_USE(ctx);
    int st = check_n3(n, "interpolate_correct_relax3d");
    if (st) return st;
    st = check_coarse3(n, cn, "interpolate_correct_relax3d");
    if (st) return st;
    MGX_REQUIRE(ncycles >= 1, MGX_ERR_INVALID, "interpolate_correct_relax3d: ncycles = %d < 1 (use interpolate_correct)", ncycles);
    ctx->last_corr_kernel[0] = 0;
    ctx->last_block3_kernel[0] = 0;
    const real hx2 = h[0] * h[0], hy2 = h[1] * h[1], hz2 = h[2] * h[2];  // :498-500
    const int sx = n[0], sy = n[1], sz = n[2], zb = 1, ze = sz - 1;
    if (!corr_fused_takes(ctx, sx, sy, sz, ze - zb)) {
        st = interpolate_correct3d_slab<real>(ctx, v, n, 0, coarse_v, cn, 0, 0, cn[2] - 1, 1);
        if (st) return st;
        if (w) return relax3d_xs_pp<real>(ctx, v, w, f, n, h, ncycles, w_rim_valid);
        return relax3d<real, XSplit>(ctx, v, f, n, h, ncycles);
    }
    corr_pset_launch<real>(ctx, v, sx, sy, 0, coarse_v, cn, 0, 1, sz - 1);
    // The passes after the correcting red pass R' are B, R, B, ...  B, R, B need only red and f, so R' stores red into w
    // instead (reading black from v), and one launch reads red and the faces from w and writes both colours of every interior
    // point into v (mgx_block3d.hip).  It stores a tile's values while the neighbouring tiles still read theirs as halo: it
    // cannot run in place.
    const bool b3 = w && w != v && block3_up_takes(ctx, n, sizeof(real), ncycles);
    if (b3 && !w_rim_valid) copy_rim3d_xs<real>(ctx, v, w, n);
    corr_red_launch<real>(ctx, v, f, sx, sy, zb, ze, hx2, hy2, hz2, 0, coarse_v, cn[0], cn[1], sz, (sz - 1) >> 1, 0, b3 ? w : nullptr);
    if (b3) relax3d_xs_block3_launch<real>(ctx, w, v, f, n, hx2, hy2, hz2, 1, true);
    for (int s = b3 ? 4 : 1; s < 2 * ncycles; s++) relax3d_xs_pass<real>(ctx, v, f, sx, sy, zb, ze, hx2, hy2, hz2, s & 1);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// z-slab form of the correcting red pass (multi-GPU post-smoothing, csrc/host/mg_dist3d.inc; the set P before it:
// correct_pset3d_slab, mgx_transfer3d.hip).  n / cn: GLOBAL sizes; v / f start at global plane fzoff (even), coarse_v at
// czoff <= fzoff / 2 and holds cplanes planes.
template <class real>
int relax3d_corr_colour_slab(mgx_ctx* ctx, real* v, const real* f, const int n[3], int fzoff, const real h[3], const real* coarse_v,
                             const int cn[3], int czoff, int cplanes, int zbeg, int zend) {
    MGX_REQUIRE(ctx && v && f && h && coarse_v, MGX_ERR_INVALID, "relax_corr_colour_slab: NULL argument");
    MGX_USE(ctx);
    int st = check_n3(n, "relax_corr_colour_slab");
    if (st) return st;
    st = check_coarse3(n, cn, "relax_corr_colour_slab");
    if (st) return st;
    MGX_REQUIRE(fzoff >= 0 && (fzoff & 1) == 0 && czoff >= 0 && fzoff / 2 >= czoff && cplanes >= 1 && zbeg >= 1 && zend >= zbeg,
                MGX_ERR_INVALID, "relax_corr_colour_slab: bad plane ranges (the slab must start on an even global plane)");
    MGX_REQUIRE(corr_fused_level_takes(ctx, n[0], n[1], n[2]), MGX_ERR_INVALID,
                "relax_corr_colour_slab: the level is not taken (ask corr_fused_takes)");
    if (zend == zbeg) return MGX_OK;
    const int ckmax = czoff + cplanes - 1 - fzoff / 2;
    MGX_REQUIRE(ckmax >= (zend >> 1), MGX_ERR_INVALID, "relax_corr_colour_slab: the coarse slab does not reach the plane above the fine range");
    const real hx2 = h[0] * h[0], hy2 = h[1] * h[1], hz2 = h[2] * h[2];
    const Geo<XSplit, real> gc(cn[0], cn[1]);
    corr_red_launch<real>(ctx, v, f, n[0], n[1], zbeg, zend, hx2, hy2, hz2, 0, coarse_v + gc.PL * (size_t)(fzoff / 2 - czoff), cn[0], cn[1],
                          n[2] - fzoff, ckmax, fzoff);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

template <class real, class L>
int jacobi3d(mgx_ctx* ctx, real* v, real* tmp, const real* f, const int n[3], const real h[3], real omega, int ncycles) {
    MGX_REQUIRE(ctx && v && tmp && f && h, MGX_ERR_INVALID, "jacobi3d: NULL argument");
    MGX_USE(ctx);
    MGX_REQUIRE(v != tmp, MGX_ERR_INVALID, "jacobi3d: v and tmp must differ");
    int st = check_n3(n, "jacobi3d");
    if (st) return st;
    MGX_REQUIRE(ncycles >= 0, MGX_ERR_INVALID, "jacobi3d: ncycles = %d < 0", ncycles);
    const real hx2 = h[0] * h[0], hy2 = h[1] * h[1], hz2 = h[2] * h[2];
    real *src = v, *dst = tmp;
    for (int k = 0; k < ncycles; k++) {
        MGX_LAUNCH((jacobi3d_kernel<real, L>), grd(n[0], n[1], n[2]), blk(), 0, ctx->compute, (const real*)src, dst, f,
                           n[0], n[1], n[2], hx2, hy2, hz2, omega);
        real* t = src; src = dst; dst = t;
    }
    MGX_LAUNCH_CHECK();
    if (src != v) {
        const Geo<L, real> g(n[0], n[1]);
        MGX_HIP(hipMemcpyAsync(v, src, sizeof(real) * g.PL * (size_t)n[2], hipMemcpyDeviceToDevice, ctx->compute));
    }
    return MGX_OK;
}

// the colour-pass smoother for other translation units (mgx_sweep3d.hip falls back to it)
template <class real>
int relax3d_xs_colour_passes(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], int ncycles) {
    return relax3d<real, XSplit>(ctx, v, f, n, h, ncycles);
}
template int relax3d_xs_colour_passes<float>(mgx_ctx*, float*, const float*, const int[3], const float[3], int);
template int relax3d_xs_colour_passes<double>(mgx_ctx*, double*, const double*, const int[3], const double[3], int);
template <class real>
int relax3d_xs_from_zero(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], int ncycles, int rim_is_zero) {
    return relax3d_from_zero<real, XSplit>(ctx, v, f, n, h, ncycles, rim_is_zero);
}
template int relax3d_xs_from_zero<float>(mgx_ctx*, float*, const float*, const int[3], const float[3], int, int);
template int relax3d_xs_from_zero<double>(mgx_ctx*, double*, const double*, const int[3], const double[3], int, int);

}  // namespace mgx

#define MGX_DEFINE_OPS3D(PFX, L, SFX, real)                                                                      \
    int PFX##relax_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], int ncycles) {    \
        return mgx::relax3d<real, L>(ctx, v, f, n, h, ncycles);                                                  \
    }                                                                                                            \
    int PFX##relax_from_zero_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3],        \
                                   int ncycles, int rim_is_zero) {                                               \
        return mgx::relax3d_from_zero<real, L>(ctx, v, f, n, h, ncycles, rim_is_zero);                           \
    }                                                                                                            \
    int PFX##jacobi_##SFX(mgx_ctx* ctx, real* v, real* tmp, const real* f, const int n[3], const real h[3],      \
                          real omega, int ncycles) {                                                             \
        return mgx::jacobi3d<real, L>(ctx, v, tmp, f, n, h, omega, ncycles);                                     \
    }

#define MGX_DEFINE_MISC3D(SFX, real)                                                                             \
    size_t mgx3dxs_plane_elems_##SFX(int sx, int sy) { return mgx::Geo<mgx::XSplit, real>(sx, sy).PL; }          \
    size_t mgx3dxs_elems_##SFX(const int n[3]) {                                                                 \
        return n ? mgx::Geo<mgx::XSplit, real>(n[0], n[1]).PL * (size_t)n[2] : 0;                                \
    }                                                                                                            \
    int mgx3dxs_relax_colour_slab_##SFX(mgx_ctx* ctx, real* v, const real* f, int sx, int sy, const real h[3],   \
                                        int colour, int zbeg, int zend, int zoff) {                              \
        return mgx::relax3d_colour_slab<real>(ctx, v, f, sx, sy, h, colour, zbeg, zend, zoff);                   \
    }                                                                                                            \
    int mgx3dxs_relax_colour_slab2_##SFX(mgx_ctx* ctx, real* v, const real* f, int sx, int sy, const real h[3],  \
                                         int colour, int zb1, int ze1, int zb2, int ze2, int zoff) {             \
        return mgx::relax3d_colour_slab2<real>(ctx, v, f, sx, sy, h, colour, zb1, ze1, zb2, ze2, zoff);          \
    }                                                                                                            \
    int mgx3dxs_relax_zero_colour_slab_##SFX(mgx_ctx* ctx, real* v, const real* f, int sx, int sy,               \
                                             const real h[3], int colour, int zbeg, int zend, int zoff) {        \
        return mgx::relax3d_zero_colour_slab<real>(ctx, v, f, sx, sy, h, colour, zbeg, zend, zoff);              \
    }                                                                                                            \
    int mgx3dxs_interpolate_correct_relax_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3],            \
                                                const real h[3], const real* coarse_v, const int cn[3],          \
                                                int ncycles) {                                                   \
        return mgx::interpolate_correct_relax3d_xs<real>(ctx, v, f, n, h, coarse_v, cn, ncycles);                \
    }                                                                                                            \
    int mgx3dxs_smooth_residual_restrict_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3],            \
                                               const real h[3], int ncycles, int from_zero, int v_rim_is_zero,   \
                                               int mode, real* coarse_f, const int cn[3],                        \
                                               int coarse_rim_is_zero) {                                         \
        return mgx::smooth_residual_restrict3d_xs<real>(ctx, v, f, n, h, ncycles, from_zero, v_rim_is_zero, mode, \
                                                        coarse_f, cn, coarse_rim_is_zero);                       \
    }                                                                                                            \
    int mgx3dxs_relax_rr_takes_##SFX(const mgx_ctx* ctx, const int n[3], const int cn[3]) {                     \
        return ctx && n && cn && mgx::relax_rr3d_xs_takes(ctx, n, cn, sizeof(real));                             \
    }                                                                                                            \
    int mgx3dxs_relax_rr_slab_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3], int fzoff,            \
                                    const real h[3], int mode, real* coarse_f, const int cn[3], int czoff,       \
                                    int pzbeg, int pzend) {                                                      \
        return mgx::relax_rr3d_slab<real>(ctx, v, f, n, fzoff, h, mode, coarse_f, cn, czoff, pzbeg, pzend);      \
    }                                                                                                            \
    int mgx3dxs_block3_up_takes_##SFX(const mgx_ctx* ctx, const int n[3], int ncycles) {                         \
        return ctx && n && mgx::block3_up_takes(ctx, n, sizeof(real), ncycles);                                  \
    }                                                                                                            \
    int mgx3dxs_block3_corr_takes_##SFX(const mgx_ctx* ctx, const int n[3], int ncycles) {                       \
        return ctx && n && mgx::block3_corr_takes(ctx, n, sizeof(real), ncycles);                                \
    }                                                                                                            \
    int mgx3dxs_interpolate_correct_relax_block3_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3],     \
                                                       const real h[3], const real* coarse_v, const int cn[3],   \
                                                       int ncycles) {                                            \
        return mgx::interpolate_correct_relax_block3_xs<real>(ctx, v, f, n, h, coarse_v, cn, ncycles);           \
    }                                                                                                            \
    int mgx3dxs_relax_corr_colour_slab_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3], int fzoff,    \
                                             const real h[3], const real* coarse_v, const int cn[3], int czoff,  \
                                             int cplanes, int zbeg, int zend) {                                  \
        return mgx::relax3d_corr_colour_slab<real>(ctx, v, f, n, fzoff, h, coarse_v, cn, czoff, cplanes, zbeg,   \
                                                   zend);                                                        \
    }                                                                                                            \
    int mgx3dxs_interpolate_correct_relax_pp_##SFX(mgx_ctx* ctx, real* v, real* w, const real* f, const int n[3], \
                                                   const real h[3], const real* coarse_v, const int cn[3],       \
                                                   int ncycles, int w_rim_valid) {                               \
        if (!w) return mgx::fail(MGX_ERR_INVALID, "interpolate_correct_relax_pp: w is NULL");                    \
        return mgx::interpolate_correct_relax3d_xs<real>(ctx, v, f, n, h, coarse_v, cn, ncycles, w, w_rim_valid); \
    }

extern "C" {
MGX_DEFINE_OPS3D(mgx3d_, mgx::Natural, f32, float)
MGX_DEFINE_OPS3D(mgx3d_, mgx::Natural, f64, double)
MGX_DEFINE_OPS3D(mgx3dxs_, mgx::XSplit, f32, float)
MGX_DEFINE_OPS3D(mgx3dxs_, mgx::XSplit, f64, double)
MGX_DEFINE_MISC3D(f32, float)
MGX_DEFINE_MISC3D(f64, double)
}
