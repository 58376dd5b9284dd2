// mgx_kernels3d.hip -- 3D Poisson multigrid operators for gfx950 (MI355X), fp32 + fp64.
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
//   relax3d_xs_pipe_kernel    one colour of MultiGrid3D::Relax, XSplit: THE hot kernel (levels >= 257 rows wide).
//                             One workgroup per CU marches a long run of planes; neighbours' edge rows / lanes
//                             through LDS, loads one plane ahead, stores one plane behind, one barrier per plane
//   relax3d_xs_kernel         the same pass with many small workgroups and re-loaded edges (smaller levels,
//                             thin z-ranges); relax3d_xs_lds_kernel: LDS edges without the software pipeline (A/B)
//   relax3d_small_kernel      all sweeps of a Relax call on a level <= 17^3 in one workgroup (LDS resident)
//   residual3d_kernel         MultiGrid3D::CalculateResidual          N3/MultiGrid3D.cpp:678-730
//   restrict3d_kernel         MultiGrid3D::Restrict                   N3/MultiGrid3D.cpp:50-184
//   interpolate3d_kernel      MultiGrid3D::Interpolate (+ApplyCorrection when ADD)
//                                                                     N3/MultiGrid3D.cpp:186-335, 649-676
//   correct3d_kernel          MultiGrid3D::ApplyCorrection            N3/MultiGrid3D.cpp:649-676
//   set3d_kernel              MultiGrid3D::setToValue                 N3/MultiGrid3D.cpp:587-621
//   init_f3d_kernel           Grid3D::InitF                           N3/Grid3D.cpp:78-96
//   (CalculateResidual + Restrict fused, no residual array: mgx_rr3d.hip)
//   interpolate3d_xs_kernel   Interpolate (+ApplyCorrection, optionally one colour only), XSplit
//   relayout3d_kernel         Natural <-> XSplit (upload / download of the hierarchy)
#include <type_traits>

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

#ifdef MGX_DIAGNOSTICS  // the A/B kernel without the software pipeline: measured slower, tools builds only
// ------------------------------------------------------------------ relax, one colour, XSplit, edges through LDS
// Same lane/row/plane assignment and the same per-point expression as relax3d_xs_kernel, but a workgroup is a
// WX x WY arrangement of waves over an (x, y) tile of 64*WX pairs x R*WY rows, and the values a wave needs from
// outside its own registers -- the "own" entries of the rows just above / below its R rows (N of row 0, S of row
// R-1) and of the lanes next to lane 0 / lane 63 (the W or E "side" value) -- are handed over by the neighbouring
// wave of the workgroup through LDS instead of being loaded again.  In relax3d_xs_kernel those re-loads are
// (R+2)/R of the v stream plus one extra 128-byte line per row and wave edge, and the PMC counters show that most
// of them miss in L2 (profiles/: FETCH_SIZE is 1.39x the v stream at R = 4).  Here only the rim of the workgroup
// tile is loaded from memory.  One s_barrier per plane; the LDS slots are double-buffered by plane parity, so a
// wave may run at most one plane ahead of its neighbours.  Every wave stays alive for the barriers: lanes past
// the end of the row and waves past the last row are clamped onto valid entries and store nothing.
template <class real, int WX, int WY, int R>
__global__ void __launch_bounds__(64 * WX * WY)
    relax3d_xs_lds_kernel(const real* __restrict__ vin, real* __restrict__ vout, const real* __restrict__ f, int sx, int sy,
                          int zbeg, int zend, real hx2, real hy2, real hz2, int colour, int zchunk, int gx, int gy,
                          int xcd_mode) {
    __shared__ real ey[2][WY][WX][2][64];  // [slot][wy][wx][first / last row][lane]: c_cur of rows 0 and R-1
    __shared__ real ex[2][WY][WX][2][R];   // [slot][wy][wx][lane 0 / lane 63][row]:  c_cur of the wave's edge lanes
    const Geo<XSplit, real> g(sx, sy);
    const int H = g.H;
    const int M = (sx + 1) >> 1;
    unsigned b = blockIdx.x;
    if (xcd_mode == 1) {  // every XCD gets one contiguous run of the plain order (see relax3d_xs_kernel)
        const unsigned nb = gridDim.x, k = b & 7u, per = nb >> 3, rem = nb & 7u;
        b = k * per + (k < rem ? k : rem) + (b >> 3);
    }
    const int bx = b % gx, by = (b / gx) % gy, bz = b / (gx * gy);
    const int lane = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int wx = w % WX, wy = w / WX;
    const int jn = (bx * WX + wx) * 64 + lane;  // nominal pair index
    const bool lane_on = jn < M - 1;            // x = 2j+q <= sx-2 needs j <= M-2
    const int j = lane_on ? jn : M - 2;
    const int y0 = 1 + (by * WY + wy) * R;
    const int nrows = max(0, min(R, sy - 1 - y0));
    const int z0 = zbeg + bz * zchunk;
    const int z1 = min(z0 + zchunk, zend);
    if (z0 >= z1) return;  // uniform over the workgroup
    const size_t sxy = g.PL;
    const int P = g.P;
    size_t rowb[R];
#pragma unroll
    for (int r = 0; r < R; r++) rowb[r] = g.row(min(y0 + r, sy - 1), z0);
    int q = (colour + y0 + z0) & 1;
    real c_prev[R], c_cur[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int qr = q ^ (r & 1);
        c_prev[r] = vin[rowb[r] - sxy + qr * H + j];
        c_cur[r] = vin[rowb[r] + (1 - qr) * H + j];
    }
    auto publish = [&](int slot, const real (&c)[R]) {
        ey[slot][wy][wx][0][lane] = c[0];
        ey[slot][wy][wx][1][lane] = c[R - 1];
        if (lane == 0 || lane == 63) {
#pragma unroll
            for (int r = 0; r < R; r++) ex[slot][wy][wx][lane == 63][r] = c[r];
        }
    };
    publish(z0 & 1, c_cur);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int z = z0; z < z1; z++) {
        const int slot = z & 1;
        real U[R], side[R], fv[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int qr = q ^ (r & 1);
            U[r] = vin[rowb[r] + sxy + qr * H + j];
            fv[r] = f[rowb[r] + qr * H + j];
        }
        // N of row 0 / S of row R-1: from the wave above / below, or from memory on the rim of the tile
        const real Nedge = wy > 0 ? ey[slot][wy - 1][wx][1][lane] : vin[rowb[0] - P + q * H + j];
        const real Sedge = wy < WY - 1 ? ey[slot][wy + 1][wx][0][lane]
                                       : vin[rowb[R - 1] + P + (q ^ ((R - 1) & 1)) * H + j];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int qr = q ^ (r & 1);
            const int ho = (1 - qr) * H;
            // side value = "own" value of pair j+1 (q_r = 1) or j-1 (q_r = 0): the neighbouring lane, the neighbouring
            // wave's edge lane (LDS), or memory (rim of the tile; pair M-1 holds only the boundary entry x = sx-1)
            real nb;
            if (qr) {
                nb = __shfl_down(c_cur[r], 1, 64);
                if (lane == 63 && wx < WX - 1) nb = ex[slot][wy][wx + 1][0][r];
                if (jn == M - 2 || (lane == 63 && wx == WX - 1)) nb = vin[rowb[r] + ho + j + 1];
            } else {
                nb = __shfl_up(c_cur[r], 1, 64);
                if (lane == 0 && wx > 0) nb = ex[slot][wy][wx - 1][1][r];
                if (lane == 0 && wx == 0) nb = vin[rowb[r] + ho + j - 1 + (j ? 0 : M)];  // j = 0: x = 0, result discarded
            }
            side[r] = nb;
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int qr = q ^ (r & 1);
            const real W = qr ? c_cur[r] : side[r];
            const real E = qr ? side[r] : c_cur[r];
            const real N = r == 0 ? Nedge : c_cur[r - 1];
            const real S = r == R - 1 ? Sedge : c_cur[r + 1];
            const real out = relax3d_point<real>(W, E, N, S, c_prev[r], U[r], fv[r], hx2, hy2, hz2);
            if (lane_on && (qr | j) && r < nrows) __builtin_nontemporal_store(out, &vout[rowb[r] + qr * H + j]);
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            c_prev[r] = c_cur[r];
            c_cur[r] = U[r];
            rowb[r] += sxy;
        }
        q ^= 1;
        publish(slot ^ 1, c_cur);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
}

#endif  // MGX_DIAGNOSTICS

// ------------------------------------------------------------------ relax, one colour, XSplit, LDS edges + prefetch
// relax3d_xs_lds_kernel with the streaming loads software-pipelined one plane ahead, so that the per-plane barrier
// no longer exposes the load latency.  In step z (plane z) a wave
//   1. issues the stores of plane z-1 (results are held one step in registers) and the loads of the NEXT step
//      (U of plane z+2, f of plane z+1, rim values of plane z+1),
//   2. publishes its edge entries of plane z+1 to the LDS slot (z+1)&1,
//   3. reads the neighbours' edge entries of plane z from slot z&1 and computes plane z,
//   4. meets the other waves at one s_barrier,
//   5. waits for what it issued in 1 (explicit s_waitcnt vmcnt(0)) and renames the register sets.
// Loads and stores therefore have the whole step (LDS traffic, ~40 fp64 operations per point, the barrier) to
// complete, and a wave has memory requests in flight all the time instead of only while it waits for them.
//
// (CORR on a z-slab: vin / f / vout and `coarse` are local arrays; the host shifts `coarse` so that local fine plane z
// interpolates from coarse planes z >> 1 (+1), hands in szg = global plane count - global index of local plane 0, zg0 = that
// global index (local plane 0 is the grid's boundary plane, which carries no correction, only where zg0 = 0), and
// ckmax = the last coarse plane (in that indexing) that exists locally: staging requests are clamped to it.)
// VAR = 2 ("CORR"): the pass reads the other colour THROUGH the coarse-grid correction -- every own-column value of the
// other colour that enters the registers gets e = Interpolate(coarse)(x, y, z) added if it is an interior point: exactly
// what Interpolate + ApplyCorrection (N3/MultiGrid3D.cpp:638-642) would have stored there.  The first red pass of the
// post-smoothing then needs no corrected array: corrected red values are never read (the red pass rewrites every red
// interior point from black neighbours alone) and corrected black values are only read by THIS pass (the black pass that
// follows rewrites every black interior point from red).  The coarse values under the tile (WY R / 2 + 1 rows x 64 WX + 1
// columns per coarse plane) are staged in LDS by the whole workgroup, one coarse plane every other step, in a ring of
// three planes (a wave is at most one step ahead of another: while planes p, p + 1 are read, only p + 2 can be written).
// A plane is requested three steps before it is first read, by the last loads of its step, which stay in flight over the
// step's end (the explicit wait leaves them outstanding; waited for in the requesting step they cost 59 us per pass);
// it is stored at the end of the next step, and the correction of an arriving entry is formed before the step's barrier,
// while the entry is still on its way: nothing is added between the arrival of a step's loads and the issue of the next
// ones.  (Holding the coarse values in registers instead costs 16 VGPRs, which spills, and a spill reload inside the loop
// waits -- vmcnt is in order -- for the prefetches issued before it: 2.5 x slower.)
template <class real>
__device__ __forceinline__ real interp_xs_at(const real* __restrict__ coarse, int CH, int CP, size_t CPL, int x, int y, int z) {
    const real* c = coarse + (size_t)(y >> 1) * CP + (size_t)(z >> 1) * CPL;
    const int gx = x >> 1;
    return interpolate3d_point<real>(x & 1, y & 1, z & 1,
                                     [&](int dx, int dy, int dz) { return c[XSplit::pos(gx + dx, CH) + dy * CP + (size_t)dz * CPL]; });
}

// CSP (diagnostic builds, TIMING ONLY, wrong results): the unrolled loop's loads and stores follow the access pattern of a colour-contiguous
// layout (row pitch H, the colour's / the other colour's points of a plane in its first / second half) instead of the x-split one
template <class real, int WX, int WY, int R, bool FNT = false, int VAR = 0, int UNR = 0, int CSP = 0>
__global__ void __launch_bounds__(64 * WX * WY, 4)  // four waves per SIMD whatever the shape: 8-wave workgroups run two to a CU
    relax3d_xs_pipe_kernel(const real* __restrict__ vin, real* __restrict__ vout, const real* __restrict__ f, int sx, int sy,
                           int zbeg, int zend, real hx2, real hy2, real hz2, int colour, int zchunk, int gx, int gy,
                           int xcd_mode, const real* __restrict__ coarse = nullptr, int cx = 0, int cy = 0, int szg = 0, int ckmax = 0, int zg0 = 0) {
    constexpr bool CORR = VAR == 2;
    // VAR == 3: the BLACK pass of the first sweep of a level that counts as all zeros (zero boundary in memory), with the red
    // pass before it folded in: the caller hands f as `vin`; every other-colour value the pass reads is the red pass's result
    // relax3d_point(0, ..., 0, f) of the f just loaded (0 on a face of the grid), formed when the load has arrived, and the
    // red entries of the lane's own pairs are stored next to the black results.  2 instead of 2.5 words per point, one launch.
    constexpr bool ZERO1 = VAR == 3;
    const double rd = relax3d_rd<real>(hx2, hy2, hz2);  // fp32: the division by multiplication (relax3d_point_rd)
    static_assert(!CORR || R == 2, "the correcting variant is written for 2 rows per lane");
    static_assert(!CORR || (WX * WY >= WY * R / 2 + 2 && WY > 1), "one wave per staged coarse row; a wave has at most one edge row (above or below)");
    static_assert(!CORR || WX >= 2, "a wave of the correcting variant has at most one rim (left or right)");
    constexpr int KR = WY * R / 2 + 2, KC = 64 * WX + 2;  // coarse rows / columns staged per plane: the cells under the tile and one more on every side
    __shared__ real ey[2][WY][WX][2][64];
    __shared__ real ex[2][WY][WX][2][R];
    __shared__ real sK[CORR ? 3 : 1][CORR ? KR : 1][CORR ? KC : 1];
    const Geo<XSplit, real> g(sx, sy);
    const int H = g.H;
    const int M = (sx + 1) >> 1;
#ifdef MGX_DIAGNOSTICS  // TIMING ONLY (wrong results), the unrolled loop: bits 4 ... of xcd_mode switch parts of a step off (tools/pipe_ablate.py)
    const int ABLP = xcd_mode >> 4;
    xcd_mode &= 15;
#else
    constexpr int ABLP = 0;
#endif
    unsigned b = blockIdx.x;
    if (xcd_mode == 1) {
        const unsigned nb = gridDim.x, k = b & 7u, per = nb >> 3, rem = nb & 7u;
        b = k * per + (k < rem ? k : rem) + (b >> 3);
    }
    const int bx = b % gx, by = (b / gx) % gy, bz = b / (gx * gy);
    const int lane = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int wx = w % WX, wy = w / WX;
    const int jn = (bx * WX + wx) * 64 + lane;
    const bool lane_on = jn < M - 1;
    const int j = lane_on ? jn : M - 2;
    const int y0 = 1 + (by * WY + wy) * R;
    const int nrows = max(0, min(R, sy - 1 - y0));
    const int z0 = zbeg + bz * zchunk;
    const int z1 = min(z0 + zchunk, zend);
    if (z0 >= z1) return;
    const int sxy = (int)g.PL;  // 32-bit offsets inside one plane pair; the plane base pointers below are 64-bit
    const bool rimR = j == M - 2 || (lane == 63 && wx == WX - 1);  // E side (q_r = 1 rows) comes from memory
    const bool rimL = lane == 0 && wx == 0;                         // W side (q_r = 0 rows) comes from memory
    const int wyN = wy > 0 ? wy - 1 : 0, wyS = wy < WY - 1 ? wy + 1 : WY - 1;
    const int wxL = wx > 0 ? wx - 1 : 0, wxR = wx < WX - 1 ? wx + 1 : WX - 1;
    // uniform row offsets inside a plane (rows past sy-1 are clamped onto it: loads stay valid, nothing is stored)
    int roff[R];
#pragma unroll
    for (int r = 0; r < R; r++) roff[r] = min(y0 + r, sy - 1) * g.P;
    const int roffN = (y0 - 1) * g.P, roffS = min(y0 + R, sy - 1) * g.P;
    // plane z of the arrays (uniform 64-bit pointers, advanced by one plane per step)
    const real* pv = vin + (size_t)z0 * g.PL;
    const real* pf = f + (size_t)z0 * g.PL;
    real* po = vout + (size_t)z0 * g.PL;
    int q = (colour + y0 + z0) & 1;
    real cp[R], cc[R], cu[R], cn[R], fc[R], fn[R], xc[R], xn[R], oc[R], op[R];
    real Nc = 0, Sc = 0, Nn = 0, Sn = 0;
    // CORR: coarse geometry; this thread's share of the staging of one coarse plane (wave w < KR: row w of the staged
    // rows, columns lane, lane + 64, ... and, lanes 0 and 1, the last two); where this lane's own coarse cell sits in the
    // staged tile (column 0 is the coarse column left of the tile)
    const Geo<XSplit, real> gcs(CORR ? cx : 3, CORR ? cy : 3);
    const int CH = gcs.H, CP = gcs.P;
    const size_t CPL = gcs.PL;
    const int cy0t = CORR ? (by * WY * R) / 2 : 0, cx0t = bx * WX * 64;  // first coarse row / column under the tile
    int kg[WX + 1];  // element offsets (inside a coarse plane) of the entries this thread stages
    const bool kload = CORR && w < KR, klast = kload && lane < 2;
#pragma unroll
    for (int a = 0; a <= WX; a++)
        kg[a] = CORR ? min(cy0t + w, cy - 1) * CP + XSplit::pos(min(max(cx0t - 1 + lane + 64 * a, 0), cx - 1), CH) : 0;
    real kt[WX + 1];  // a coarse plane on its way into LDS
#pragma unroll
    for (int a = 0; a <= WX; a++) kt[a] = 0;
    const int kmy = wy * (R / 2) * KC + wx * 64 + lane + 1;  // sK offset of coarse cell (column j, row (y0 - 1) / 2) inside a plane slot
    // The values a workgroup takes from memory besides its own columns (the rows just above / below its tile, the pairs
    // left / right of it) would each need an interpolation of their own in every step -- measured: +100 us per pass at
    // 513^3, the edge waves hold up the whole workgroup at the barrier.  Instead the black points of the coarse cells those
    // values belong to (the set P: cell rows py % (WY R / 2) == 0, cell columns i > 0 with i % (64 WX) in {0, 64 WX - 1};
    // about 1/8 of the cells) are corrected IN PLACE by correct_pset3d_xs_kernel before this pass; own entries in P are
    // taken as they are.
    // (Round 3, end: only the ROWS are in P now.  The pair a tile reads left / right of itself is ONE value per row and step, in one
    // lane of the wave: that lane corrects it on the fly from the staged tile's outer columns -- one interpolation per wave and step,
    // hidden behind the loads -- and the column part of the pre-pass, 47 us at 513^3 for 12 MB of useful data in 128-byte lines, is gone.)
    bool own[R];   // does row r's own entry get the correction on the fly?
    bool rimc[R];  // does the value this lane takes from the neighbouring tile in row r (rimL: x = 2j - 1, rimR: x = 2j + 2) get one?
#pragma unroll
    for (int r = 0; r < R; r++) {
        own[r] = CORR && lane_on && y0 + r <= sy - 2;
        rimc[r] = CORR && lane_on && y0 + r <= sy - 2 && ((lane == 0 && wx == 0 && j > 0) || (lane == 63 && wx == WX - 1 && j + 1 < M - 1));
    }
    // ... and, last, the ROWS: the row a tile reads above / below itself (wave row 0: y0 - 1, the last wave row: y0 + R) is one value
    // per lane and step in the edge waves, corrected there from the staged rows (one more is staged for it); with that the set P is
    // empty and the pre-pass is gone for this kernel
    const bool edgeN = CORR && lane_on && wy == 0 && y0 - 1 >= 1, edgeS = CORR && lane_on && wy == WY - 1 && y0 + R <= sy - 2;
    // request coarse plane `plane` (kt), store what was requested into its ring slot
#define MGX_K_REQUEST(plane)                                                                    \
    do {                                                                                        \
        if (kload) {                                                                            \
            const real* c_ = coarse + (size_t)(plane) * CPL;                                    \
            _Pragma("unroll") for (int a = 0; a < WX; a++) kt[a] = c_[kg[a]];                   \
            if (klast) kt[WX] = c_[kg[WX]];                                                     \
        }                                                                                       \
    } while (0)
#define MGX_K_STORE(plane)                                                                      \
    do {                                                                                        \
        if (kload) {                                                                            \
            real* d_ = &sK[(plane) % 3][w][lane];                                               \
            _Pragma("unroll") for (int a = 0; a < WX; a++) d_[64 * a] = kt[a];                  \
            if (klast) d_[64 * WX] = kt[WX];                                                    \
        }                                                                                       \
    } while (0)
    // the corrections e0 / e1 of this lane's entries of row 0 / row 1 at plane zz (x = 2j + px0 in row 0, the other parity in
    // row 1) from the staged planes zz >> 1 (k0_) and (zz >> 1) + 1 (k1_).  Row 0 (odd y) lies between two coarse rows, row 1
    // on the second of them, so the parity class of both entries follows from (px0, zz & 1): ONE uniform branch, and in
    // every case interpolate3d_point with literal class arguments (the reference's association, N3/MultiGrid3D.cpp:216-329)
#define MGX_CORR_PAIR(px0, zz, e0, e1)                                                                              \
    do {                                                                                                            \
        const real* k0_ = &sK[0][0][0] + ((zz) >> 1) % 3 * (KR * KC) + kmy;                                         \
        const real* k1_ = &sK[0][0][0] + (((zz) >> 1) + 1) % 3 * (KR * KC) + kmy;                                   \
        auto g0_ = [&](int dx, int dy, int dz) { return (dz ? k1_ : k0_)[dy * KC + dx]; };                          \
        auto g1_ = [&](int dx, int dy, int dz) { return (dz ? k1_ : k0_)[KC + dy * KC + dx]; };                     \
        switch ((px0) * 2 + ((zz) & 1)) {                                                                           \
            case 0: e0 = interpolate3d_point<real>(0, 1, 0, g0_); e1 = interpolate3d_point<real>(1, 0, 0, g1_); break; \
            case 1: e0 = interpolate3d_point<real>(0, 1, 1, g0_); e1 = interpolate3d_point<real>(1, 0, 1, g1_); break; \
            case 2: e0 = interpolate3d_point<real>(1, 1, 0, g0_); e1 = interpolate3d_point<real>(0, 0, 0, g1_); break; \
            default: e0 = interpolate3d_point<real>(1, 1, 1, g0_); e1 = interpolate3d_point<real>(0, 0, 1, g1_); break; \
        }                                                                                                           \
    } while (0)

    // the correction e of the value the wave's rim lane takes from the neighbouring tile at plane zz, in the ONE row rr whose parity
    // asks for it (left rim, wave column 0: rows with q_r = 0, the point x = 2j - 1 of coarse column j - 1, odd; right rim, last wave
    // column: rows with q_r = 1, x = 2j + 2 = coarse column j + 1, even); all wave-uniform but the lane, so every lane computes it and
    // the rim lane uses it.  qq = the parity of row 0 at plane zz.
#define MGX_CORR_RIM(qq, zz, rr, e)                                                                                  \
    do {                                                                                                            \
        const real* k0_ = &sK[0][0][0] + ((zz) >> 1) % 3 * (KR * KC) + kmy;                                         \
        const real* k1_ = &sK[0][0][0] + (((zz) >> 1) + 1) % 3 * (KR * KC) + kmy;                                   \
        const bool left_ = wx == 0;                                                                                 \
        rr = left_ ? ((qq) & 1) : 1 - ((qq) & 1);  /* q_r = qq ^ (r & 1): 0 for the left rim, 1 for the right */     \
        const int co_ = (left_ ? -1 : 1) + (rr) * KC;                                                               \
        auto g_ = [&](int dx, int dy, int dz) { return (dz ? k1_ : k0_)[co_ + dy * KC + dx]; };                     \
        switch ((left_ ? 4 : 0) + (rr) * 2 + ((zz) & 1)) { /* (x parity, y parity = 1 - rr, z parity) as literals */  \
            case 0: e = interpolate3d_point<real>(0, 1, 0, g_); break;                                              \
            case 1: e = interpolate3d_point<real>(0, 1, 1, g_); break;                                              \
            case 2: e = interpolate3d_point<real>(0, 0, 0, g_); break;                                              \
            case 3: e = interpolate3d_point<real>(0, 0, 1, g_); break;                                              \
            case 4: e = interpolate3d_point<real>(1, 1, 0, g_); break;                                              \
            case 5: e = interpolate3d_point<real>(1, 1, 1, g_); break;                                              \
            case 6: e = interpolate3d_point<real>(1, 0, 0, g_); break;                                              \
            default: e = interpolate3d_point<real>(1, 0, 1, g_); break;                                             \
        }                                                                                                           \
    } while (0)

    // the correction e of the edge-row value of plane zz this lane reads (wave row 0: the row above, y0 - 1, even, the staged row of
    // the wave's first row; last wave row: the row below, y0 + R, odd, between the next two staged rows); qq = parity of row 0 at zz:
    // the entry is x = 2j + qq above, x = 2j + (qq ^ 1) below (R = 2)
#define MGX_CORR_EDGE(qq, zz, e)                                                                                    \
    do {                                                                                                            \
        const real* k0_ = &sK[0][0][0] + ((zz) >> 1) % 3 * (KR * KC) + kmy;                                         \
        const real* k1_ = &sK[0][0][0] + (((zz) >> 1) + 1) % 3 * (KR * KC) + kmy;                                   \
        const bool below_ = wy != 0;                                                                                \
        const int xp_ = below_ ? ((qq) ^ 1) & 1 : (qq) & 1;                                                         \
        const int ro_ = below_ ? KC : 0;                                                                            \
        auto g_ = [&](int dx, int dy, int dz) { return (dz ? k1_ : k0_)[ro_ + dy * KC + dx]; };                     \
        switch ((below_ ? 4 : 0) + xp_ * 2 + ((zz) & 1)) {                                                          \
            case 0: e = interpolate3d_point<real>(0, 0, 0, g_); break;                                              \
            case 1: e = interpolate3d_point<real>(0, 0, 1, g_); break;                                              \
            case 2: e = interpolate3d_point<real>(1, 0, 0, g_); break;                                              \
            case 3: e = interpolate3d_point<real>(1, 0, 1, g_); break;                                              \
            case 4: e = interpolate3d_point<real>(0, 1, 0, g_); break;                                              \
            case 5: e = interpolate3d_point<real>(0, 1, 1, g_); break;                                              \
            case 6: e = interpolate3d_point<real>(1, 1, 0, g_); break;                                              \
            default: e = interpolate3d_point<real>(1, 1, 1, g_); break;                                             \
        }                                                                                                           \
        if (!(xp_ | j)) e = 0; /* x = 0: a boundary entry */                                                        \
    } while (0)

    // everything that comes from memory besides the column itself, for the plane at offset dz from pv, row parity qq.
    // rim-right lanes need index j+1 of half 0 in q_r = 1 rows, rim-left lanes index j-1 of half 1 in q_r = 0 rows
    // (j = 0: x = 0, the result is discarded, index M-1 keeps the load inside the array); in the other rows the lane
    // re-loads its own entry (a cache hit) and the value is not used.  (A macro, not a lambda: scalars handed to a
    // lambda by reference end up in scratch memory here.)
#define MGX_LOAD_RIM(dz, qq, X, Nv, Sv)                                                        \
    do {                                                                                       \
        const real* p_ = pv + (dz) * sxy;                                                      \
        if (wy == 0) Nv = p_[roffN + (qq) * H + j];                                            \
        if (wy == WY - 1) Sv = p_[roffS + ((qq) ^ ((R - 1) & 1)) * H + j];                     \
        if (rimL || rimR) {                                                                    \
            _Pragma("unroll") for (int r = 0; r < R; r++) {                                    \
                const int qr_ = (qq) ^ (r & 1);                                                \
                const int d_ = qr_ ? (rimR ? 1 : 0) : (rimL ? (j ? -1 : M - 1) : 0);           \
                X[r] = p_[roff[r] + (1 - qr_) * H + j + d_];                                   \
            }                                                                                  \
        }                                                                                      \
    } while (0)
    auto publish = [&](int slot, const real (&c)[R]) __attribute__((always_inline)) {
        ey[slot][wy][wx][0][lane] = c[0];
        ey[slot][wy][wx][1][lane] = c[R - 1];
        if (lane == 0 || lane == 63) {
#pragma unroll
            for (int r = 0; r < R; r++) ex[slot][wy][wx][lane == 63][r] = c[r];
        }
    };
    auto store_plane = [&](int dz, int qq, const real (&O)[R]) __attribute__((always_inline)) {
        real* p = po + dz * sxy;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int qr = qq ^ (r & 1);
            if (lane_on && (qr | j) && r < nrows) __builtin_nontemporal_store(O[r], &p[roff[r] + qr * H + j]);
        }
    };

    // prologue: planes z0-1, z0, z0+1 of the column, f and rim of plane z0
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int qr = q ^ (r & 1);
        cp[r] = pv[roff[r] - sxy + qr * H + j];
        cc[r] = pv[roff[r] + (1 - qr) * H + j];
        cu[r] = pv[roff[r] + sxy + qr * H + j];
        fc[r] = (FNT ? __builtin_nontemporal_load(&pf[roff[r] + qr * H + j]) : pf[roff[r] + qr * H + j]);
        xc[r] = xn[r] = 0;
        op[r] = 0;
    }
    MGX_LOAD_RIM(0, q, xc, Nc, Sc);
    real er0 = 0, ee0 = 0;  // CORR: the corrections of the rim value (row rr0) and of the edge-row value of plane z0 + 1
    int rr0 = 0;
    if constexpr (CORR) {
        // own entries of the planes z0-1, z0, z0+1: the correction straight from the coarse array, once per run of planes
#pragma unroll
        for (int r = 0; r < R; r++)
            if (own[r]) {
                const int qr = q ^ (r & 1), y = y0 + r;
                if (z0 - 1 + zg0 >= 1 && (qr | j)) cp[r] = cp[r] + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * j + qr, y, z0 - 1);
                if ((1 - qr) | j) cc[r] = cc[r] + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * j + 1 - qr, y, z0);
                if (z0 + 1 <= szg - 2 && (qr | j)) cu[r] = cu[r] + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * j + qr, y, z0 + 1);
            }
#pragma unroll
        for (int r = 0; r < R; r++)
            if (rimc[r]) {  // the neighbouring tile's value of plane z0 (z0 >= 1 is an interior plane)
                const int qr = q ^ (r & 1);
                if (qr == 0 && lane == 0) xc[r] = xc[r] + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * j - 1, y0 + r, z0);
                if (qr == 1 && lane == 63) xc[r] = xc[r] + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * j + 2, y0 + r, z0);
            }
        if (edgeN && (q | j)) Nc = Nc + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * j + q, y0 - 1, z0);
        if (edgeS && ((q ^ 1) | j)) Sc = Sc + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * j + (q ^ 1), y0 + R, z0);
        if (z0 + 1 <= szg - 2) {
            if (edgeN && ((q ^ 1) | j)) ee0 = interp_xs_at<real>(coarse, CH, CP, CPL, 2 * j + (q ^ 1), y0 - 1, z0 + 1);
            if (edgeS && (q | j)) ee0 = interp_xs_at<real>(coarse, CH, CP, CPL, 2 * j + q, y0 + R, z0 + 1);
        }
        // ... and of plane z0 + 1, which arrives in the first step: one of its two coarse planes is not staged yet (z0 even)
        rr0 = wx == 0 ? ((q ^ 1) & 1) : 1 - ((q ^ 1) & 1);
        if (rimc[rr0] && z0 + 1 <= szg - 2)
            er0 = interp_xs_at<real>(coarse, CH, CP, CPL, wx == 0 ? 2 * j - 1 : 2 * j + 2, y0 + rr0, z0 + 1);
        // the coarse planes under the arrivals of the first three steps (the loop's requests start with the fourth)
        MGX_K_REQUEST(min((z0 + 2) >> 1, ckmax));
        MGX_K_STORE((z0 + 2) >> 1);
        MGX_K_REQUEST(min(((z0 + 2) >> 1) + 1, ckmax));
        MGX_K_STORE(((z0 + 2) >> 1) + 1);
        if (z0 & 1) {
            MGX_K_REQUEST(min(((z0 + 2) >> 1) + 2, ckmax));
            MGX_K_STORE(((z0 + 2) >> 1) + 2);
        }
    }
    // ZERO1: a loaded f value -> the red value at that place (0 on a face: x = 0 / x = sx - 1, a boundary row, a boundary plane)
    auto zred = [&](real x, bool face) __attribute__((always_inline)) {
        const real zero = (real)0;
        return face ? zero : relax3d_point_rd<real>(zero, zero, zero, zero, zero, zero, x, hx2, hy2, hz2, rd);
    };
    const bool x0 = j == 0;  // half 0 of the lane's pair is x = 0
    if constexpr (ZERO1) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int qr = q ^ (r & 1);
            const bool rowface = y0 + r >= sy - 1;
            cp[r] = zred(cp[r], rowface || z0 - 1 <= 0 || (qr == 0 && x0));
            cc[r] = zred(cc[r], rowface || (qr == 1 && x0));
            cu[r] = zred(cu[r], rowface || z0 + 1 >= szg - 1 || (qr == 0 && x0));
            xc[r] = zred(xc[r], qr == 1 && j == M - 2);
        }
        Nc = zred(Nc, y0 - 1 <= 0 || (q == 0 && x0));
        Sc = zred(Sc, y0 + R >= sy - 1 || ((q ^ ((R - 1) & 1)) == 0 && x0));
    }
    publish(z0 & 1, cc);
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if constexpr (UNR != 0) {
        // The same schedule with the loop unrolled four times and every register role fixed per step: the planes of the column
        // live in c[4][R] (step k: c[k & 3] = plane z - 1, c[(k + 1) & 3] = z, c[(k + 2) & 3] = z + 1, c[(k + 3) & 3] = the one on
        // its way), f / rim / edge rows / results in pairs of sets by step parity, and the row parity q is a literal: the 13 register
        // copies and ~25 parity selects of a rolled step are gone (the passes that are bound by instruction issue -- the correcting
        // pass, fp32 -- spend a fifth of their vector instructions on them).  Same loads, same stores, same arithmetic.
        // (UNR - 1) & 1 = the row parity q of the run's first plane: the host launches the instantiation that fits (every run of a
        // launch starts with the same parity: runs are an even number of planes long, and y0 is odd).  UNR >= 3: DEPTH 2 -- the column
        // and f are requested two steps ahead (mgx_pipe_step.inc), six steps per loop trip.
        static_assert(R % 2 == 0, "the unrolled loop takes y0 to be odd");
        constexpr int DEPTH = UNR >= 3 ? 2 : 1, Q0 = (UNR - 1) & 1, CR = DEPTH == 2 ? 6 : 4, FR = DEPTH + 1;
        real c[CR][R], fb[FR][R], xb[2][R], ob[2][R], nb2[2], sb2[2];
#pragma unroll
        for (int r = 0; r < R; r++) {
#pragma unroll
            for (int k = 3; k < CR; k++) c[k][r] = 0;
            c[0][r] = cp[r]; c[1][r] = cc[r]; c[2][r] = cu[r];
#pragma unroll
            for (int k = 1; k < FR; k++) fb[k][r] = 0;
            fb[0][r] = fc[r];
            xb[0][r] = xc[r]; xb[1][r] = 0;
            ob[0][r] = ob[1][r] = 0;
        }
        nb2[0] = Nc; nb2[1] = 0;
        sb2[0] = Sc; sb2[1] = 0;
        unsigned kgb[WX + 1];  // CORR: byte offsets of the coarse entries this thread stages
#pragma unroll
        for (int a = 0; a <= WX; a++) kgb[a] = (unsigned)kg[a] * (unsigned)sizeof(real);
        // MGX_HO(par, own): offset of a row's half inside the plane -- x-split: the half of x parity `par`; CSP: the half-plane of the
        // colour (own) or of the other colour; MGX_RO(off): the row's offset -- x-split: as computed (pitch P = 2 H); CSP: pitch H
#define MGX_HO(par, own) (CSP ? ((own) ? colour : 1 - colour) * (H * sy) : (par) * H)
#define MGX_RO(off) (CSP ? (off) / 2 : (off))
        const unsigned jb = (unsigned)j * (unsigned)sizeof(real);  // the lane's byte offset inside a half-row; the rim lanes': the pair right / left
        const unsigned jbR = (unsigned)(j + (rimR ? 1 : 0)) * (unsigned)sizeof(real), jbL = (unsigned)(j + (rimL ? (j ? -1 : M - 1) : 0)) * (unsigned)sizeof(real);
        if constexpr (DEPTH == 2) {  // what step z0 - 1 would have requested: the column of plane z0 + 2, f of plane z0 + 1 (clamped like the loop's)
            const auto rv0 = plane_rsrc<real>(pv, sxy, 3), rf0 = plane_rsrc<real>(pf, sxy, 2);
            const int e2 = min(2, z1 - z0) * sxy, e1 = min(1, z1 - z0) * sxy;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int qn = Q0 ^ 1 ^ (r & 1);
                c[3][r] = buf_load<real>(rv0, jb, roff[r] + e2 + qn * H);
                fb[1][r] = FNT ? buf_load_nt<real>(rf0, jb, roff[r] + e1 + qn * H) : buf_load<real>(rf0, jb, roff[r] + e1 + qn * H);
            }
        }
        {
            int z = z0;
            for (;;) {
#define MGX_K 0
#include "mgx_pipe_step.inc"
#undef MGX_K
                if (++z >= z1) break;
#define MGX_K 1
#include "mgx_pipe_step.inc"
#undef MGX_K
                if (++z >= z1) break;
#define MGX_K 2
#include "mgx_pipe_step.inc"
#undef MGX_K
                if (++z >= z1) break;
#define MGX_K 3
#include "mgx_pipe_step.inc"
#undef MGX_K
                if (++z >= z1) break;
                if constexpr (DEPTH == 2) {
#define MGX_K 4
#include "mgx_pipe_step.inc"
#undef MGX_K
                    if (++z >= z1) break;
#define MGX_K 5
#include "mgx_pipe_step.inc"
#undef MGX_K
                    if (++z >= z1) break;
                }
            }
        }
        const int kl = (z1 - z0 - 1) & 1;  // the last step: its results sit in ob[kl], its row parity is Q0 ^ kl
        if (kl) store_plane(-1, Q0 ^ 1, ob[1]);
        else store_plane(-1, Q0, ob[0]);
#undef MGX_HO
#undef MGX_RO
    } else {
        for (int z = z0; z < z1; z++) {
            const bool more = z + 1 < z1;
            // a wave that has passed the barrier issues its stores and next loads at raised priority: requests leave the CU
            // before the other waves' arithmetic (measured -1.3 % per pass, same-box A/B)
            __builtin_amdgcn_s_setprio(3);
            if (z > z0) store_plane(-1, q ^ 1, op);  // results of plane z-1
            if constexpr (ZERO1) {  // the red entries of the lane's own pairs at plane z (x = 0 is a boundary point)
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int qo = 1 - (q ^ (r & 1));
                    if (lane_on && (qo | j) && r < nrows) __builtin_nontemporal_store(cc[r], &po[roff[r] + qo * H + j]);
                }
            }
            if (more) {
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int qn = q ^ 1 ^ (r & 1);  // row parity in plane z+1
                    cn[r] = pv[roff[r] + 2 * sxy + qn * H + j];
                    fn[r] = (FNT ? __builtin_nontemporal_load(&pf[roff[r] + sxy + qn * H + j]) : pf[roff[r] + sxy + qn * H + j]);
                }
                MGX_LOAD_RIM(1, q ^ 1, xn, Nn, Sn);
                if constexpr (CORR) {
                    // the correction of the plane that arrives in step s is formed in step s itself, BEFORE its barrier, from the
                    // coarse planes (s + 2) >> 1 and, for odd s, (s + 3) / 2: that one is requested in step s - 3 (these are
                    // the LAST loads of the step: they stay in flight over the step's end), stored at the end of step s - 2
                    // and so visible from the barrier of step s - 1 on
                    if (!(z & 1) && z + 4 < z1) MGX_K_REQUEST(min((z >> 1) + 3, ckmax));
                }
                publish((z + 1) & 1, cu);
            }
            __builtin_amdgcn_s_setprio(0);
            const int slot = z & 1;
            const real Nl = ey[slot][wyN][wx][1][lane], Sl = ey[slot][wyS][wx][0][lane];
            const real Nedge = wy > 0 ? Nl : Nc;
            const real Sedge = wy < WY - 1 ? Sl : Sc;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int qr = q ^ (r & 1);
                const real fromR = ex[slot][wy][wxR][0][r], fromL = ex[slot][wy][wxL][1][r];
                real nb = qr ? __shfl_down(cc[r], 1, 64) : __shfl_up(cc[r], 1, 64);
                if (qr) {
                    if (lane == 63) nb = fromR;
                    if (rimR) nb = xc[r];
                } else {
                    if (lane == 0) nb = fromL;
                    if (rimL) nb = xc[r];
                }
                const real W = qr ? cc[r] : nb;
                const real E = qr ? nb : cc[r];
                const real N = r == 0 ? Nedge : cc[r - 1];
                const real S = r == R - 1 ? Sedge : cc[r + 1];
                oc[r] = relax3d_point_rd<real>(W, E, N, S, cp[r], cu[r], fc[r], hx2, hy2, hz2, rd);
            }
            real en[R];   // CORR: the correction of the entries that are on their way (plane z + 2, x = 2j + qn) ...
            bool dc[R];   // ... if they get one
#pragma unroll
            for (int r = 0; r < R; r++) {
                en[r] = 0;
                dc[r] = false;
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            real er = 0, ee = 0;  // CORR: the corrections of the rim value (row rrim) and of the edge-row value that are on their way (plane z + 1)
            int rrim = 0;
            if constexpr (CORR) {
                if (more) {
                    MGX_CORR_PAIR(q ^ 1, z + 2, en[0], en[1]);  // all lanes: the staged tile covers every lane's cell
#pragma unroll
                    for (int r = 0; r < R; r++) dc[r] = own[r] && z + 2 <= szg - 2 && ((q ^ 1 ^ (r & 1)) | j);
                    if (z == z0) {
                        er = er0;
                        rrim = rr0;
                        ee = ee0;
                    } else {
                        if (wx == 0 || wx == WX - 1) MGX_CORR_RIM(q ^ 1, z + 1, rrim, er);
                        if (wy == 0 || wy == WY - 1) MGX_CORR_EDGE(q ^ 1, z + 1, ee);
                    }
                    if (z + 1 > szg - 2) er = ee = 0;  // a boundary plane: no correction
                }
            }
            if (CORR && kload && more && !(z & 1) && z + 4 < z1) {
                // the staging loads issued last in this step may stay in flight (loads return in order: at most WX + 1
                // outstanding operations means everything issued before them has arrived); they are stored a step later
                if constexpr (WX == 2) __builtin_amdgcn_s_waitcnt(0x0F73);
                else __builtin_amdgcn_s_waitcnt(0x0F70);
            } else {
                __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this step's prefetch and stores have had the whole step
            }
#pragma unroll
            for (int r = 0; r < R; r++) {
                cp[r] = cc[r];
                cc[r] = cu[r];
                cu[r] = dc[r] ? cn[r] + en[r] : cn[r];
                fc[r] = fn[r];
                xc[r] = (CORR && rimc[r] && r == rrim) ? xn[r] + er : xn[r];
                op[r] = oc[r];
            }
            if constexpr (CORR) {
                if ((z & 1) && z > z0 && z + 3 < z1) MGX_K_STORE(((z - 1) >> 1) + 3);  // requested in step z - 1
            }
            Nc = (CORR && edgeN) ? Nn + ee : Nn;
            Sc = (CORR && edgeS) ? Sn + ee : Sn;
            if constexpr (ZERO1) {  // what arrived in this step was f: the red values at those places (plane z + 2 / the rim of z + 1)
                const int q1 = q ^ 1;  // the colour's half of row 0 at plane z + 1
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int qn = q1 ^ (r & 1);
                    cu[r] = zred(cu[r], y0 + r >= sy - 1 || z + 2 >= szg - 1 || (qn == 0 && x0));
                    xc[r] = zred(xc[r], qn == 1 && j == M - 2);
                }
                Nc = zred(Nc, y0 - 1 <= 0 || (q1 == 0 && x0));
                Sc = zred(Sc, y0 + R >= sy - 1 || ((q1 ^ ((R - 1) & 1)) == 0 && x0));
            }
            pv += sxy;
            pf += sxy;
            po += sxy;
            q ^= 1;
        }
        store_plane(-1, q ^ 1, op);  // the last plane
    }
#undef MGX_LOAD_RIM
#undef MGX_K_REQUEST
#undef MGX_K_STORE
#undef MGX_CORR_PAIR
#undef MGX_CORR_RIM
#undef MGX_CORR_EDGE
}

// ------------------------------------------------------------------ relax, one colour, XSplit, pipelined, TWO pairs per lane
// relax3d_xs_pipe_kernel for fp32: with one x-pair per lane a wave instruction moves only 256 bytes and every shape of
// that kernel stops at 0.64-0.66 of the HBM peak (profiles/r01_sweep_pipe_513_f32.txt: flat over shapes and run lengths).
// Here a lane owns the two consecutive pairs j0 = 2 l, j0 + 1 of each of its R rows: every load and store of the column is
// an 8-byte vector (512 bytes per wave instruction, as in fp64).  Same schedule (LDS hand-over of edge rows / edge lanes,
// loads one plane ahead, stores one plane behind, one barrier per plane), same per-point expression.  Of the two x
// neighbours of an updated point one is the lane's own other-colour entry, the other one is -- depending on the element --
// the lane's other element or the neighbouring lane's (wave shuffle; wave edge: LDS; tile edge: memory).

// VAR = 2: the correcting red pass of relax3d_xs_pipe_kernel (the black values read through v + Interpolate(coarse), coarse
// planes staged in LDS, the set P corrected in place beforehand) for two pairs per lane: the staged tile is 128 WX + 2 coarse
// columns wide, a lane interpolates for both of its pairs.
template <class real, int WX, int WY, int R, bool FNT = false, int VAR = 0, int UNR = 0>
__global__ void __launch_bounds__(64 * WX * WY)
    relax3d_xs_pipe_v2_kernel(const real* __restrict__ vin, real* __restrict__ vout, const real* __restrict__ f, int sx, int sy,
                              int zbeg, int zend, real hx2, real hy2, real hz2, int colour, int zchunk, int gx, int gy,
                              int xcd_mode, const real* __restrict__ coarse = nullptr, int cx = 0, int cy = 0, int szg = 0, int ckmax = 0, int zg0 = 0) {
    typedef typename Vec2T<real>::type vec2;
    constexpr bool CORR = VAR == 2;
    static_assert(!CORR || R == 2, "the correcting variant is written for 2 rows per lane");
    static_assert(!CORR || (WX * WY >= WY * R / 2 + 1 && WY > 1), "one wave per coarse row under the tile and its rim");
    // EDGEF (the unrolled form): the row a tile reads above / below itself is corrected on the fly by the edge waves, from one more
    // staged coarse row, as in relax3d_xs_pipe_kernel -- no set P, no pre-pass; the rolled form keeps the tile's first / last row in P
    constexpr bool EDGEF = CORR && UNR != 0;
    constexpr int KR = WY * R / 2 + 1 + (EDGEF ? 1 : 0), NK = 2 * WX, KC = 64 * NK + 2;  // coarse rows / columns staged per plane
    static_assert(!CORR || WX * WY >= KR, "one wave per staged coarse row");
    __shared__ vec2 ey[2][WY][WX][2][64];
    __shared__ real ex[2][WY][WX][2][R];  // [lane 0's element 0 / lane 63's element 1]
    __shared__ real sK[CORR ? 3 : 1][CORR ? KR : 1][CORR ? KC : 1];
    const Geo<XSplit, real> g(sx, sy);
    const int H = g.H;
    const int M = (sx + 1) >> 1;  // M - 1 pairs hold an interior point; M - 1 is even (the host: pipe_v2_takes)
    const double rd = relax3d_rd<real>(hx2, hy2, hz2);
    unsigned b = blockIdx.x;
    if (xcd_mode == 1) {
        const unsigned nb = gridDim.x, k = b & 7u, per = nb >> 3, rem = nb & 7u;
        b = k * per + (k < rem ? k : rem) + (b >> 3);
    }
    const int bx = b % gx, by = (b / gx) % gy, bz = b / (gx * gy);
    const int lane = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int wx = w % WX, wy = w / WX;
    const int jn = 2 * ((bx * WX + wx) * 64 + lane);  // nominal first pair of the lane
    const bool lane_on = jn < M - 1;                  // both pairs or none (M - 1 is even)
    const int j0 = lane_on ? jn : M - 3;
    const int y0 = 1 + (by * WY + wy) * R;
    const int nrows = max(0, min(R, sy - 1 - y0));
    const int z0 = zbeg + bz * zchunk;
    const int z1 = min(z0 + zchunk, zend);
    if (z0 >= z1) return;
    const int sxy = (int)g.PL;
    const bool rimR = j0 + 1 == M - 2 || (lane == 63 && wx == WX - 1);  // E side of element 1 (q_r = 1 rows) comes from memory
    const bool rimL = lane == 0 && wx == 0;                             // W side of element 0 (q_r = 0 rows) comes from memory
    const int wyN = wy > 0 ? wy - 1 : 0, wyS = wy < WY - 1 ? wy + 1 : WY - 1;
    const int wxL = wx > 0 ? wx - 1 : 0, wxR = wx < WX - 1 ? wx + 1 : WX - 1;
    int roff[R];
#pragma unroll
    for (int r = 0; r < R; r++) roff[r] = min(y0 + r, sy - 1) * g.P;
    const int roffN = (y0 - 1) * g.P, roffS = min(y0 + R, sy - 1) * g.P;
    const real* pv = vin + (size_t)z0 * g.PL;
    const real* pf = f + (size_t)z0 * g.PL;
    real* po = vout + (size_t)z0 * g.PL;
    int q = (colour + y0 + z0) & 1;
    vec2 cp[R], cc[R], cu[R], cn[R], fc[R], fn[R], oc[R], op[R];
    real xc[R], xn[R];
    vec2 Nc = {0, 0}, Sc = {0, 0}, Nn = {0, 0}, Sn = {0, 0};
    // CORR: as in relax3d_xs_pipe_kernel -- coarse geometry, this thread's share of the staging of one coarse plane (wave
    // w < KR: row w, columns lane + 64 a and, lanes 0 and 1, the last two), the lane's first coarse cell in the staged tile
    const Geo<XSplit, real> gcs(CORR ? cx : 3, CORR ? cy : 3);
    const int CH = gcs.H, CP = gcs.P;
    const size_t CPL = gcs.PL;
    const int cy0t = CORR ? (by * WY * R) / 2 : 0, cx0t = bx * WX * 128;
    int kg[NK + 1];
    const bool kload = CORR && w < KR, klast = kload && lane < 2;
#pragma unroll
    for (int a = 0; a <= NK; a++)
        kg[a] = CORR ? min(cy0t + w, cy - 1) * CP + XSplit::pos(min(max(cx0t - 1 + lane + 64 * a, 0), cx - 1), CH) : 0;
    real kt[NK + 1];
#pragma unroll
    for (int a = 0; a <= NK; a++) kt[a] = 0;
    const int kmy = wy * (R / 2) * KC + wx * 128 + 2 * lane + 1;  // coarse cell (column j0, row (y0 - 1) / 2); the second pair's: + 1
    bool own0[R], own1[R];  // does the entry of pair j0 / j0 + 1 in row r get its correction on the fly (not in the set P)?
    bool rimc[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const bool rowP = !EDGEF && ((wy == 0 && r == 0) || (wy == WY - 1 && r == R - 1));
        own0[r] = CORR && lane_on && !rowP && y0 + r <= sy - 2;
        own1[r] = CORR && lane_on && !rowP && y0 + r <= sy - 2;
        // the value taken from the neighbouring tile (left: x = 2 j0 - 1, right: x = 2 j0 + 4) is corrected by the lane that reads
        // it, as in relax3d_xs_pipe_kernel: no tile-edge columns in the set P
        rimc[r] = CORR && lane_on && !rowP && y0 + r <= sy - 2 && ((lane == 0 && wx == 0 && j0 > 0) || (lane == 63 && wx == WX - 1 && j0 + 2 < M - 1));
    }
    const bool edgeN = EDGEF && lane_on && wy == 0 && y0 - 1 >= 1, edgeS = EDGEF && lane_on && wy == WY - 1 && y0 + R <= sy - 2;
    // the corrections of the two edge-row values of plane zz this lane reads (wave row 0: the row above, y0 - 1, even: the staged row of
    // the wave's first row; last wave row: the row below, y0 + R, odd: between the next two staged rows); qq = parity of row 0 at zz:
    // the entries are x = 2 (j0 + p) + qq above, x = 2 (j0 + p) + (qq ^ 1) below (R = 2), p = 0, 1
#define MGX_CORR_EDGE2(qq, zz, e)                                                                                   \
    do {                                                                                                            \
        const real* k0_ = &sK[0][0][0] + ((zz) >> 1) % 3 * (KR * KC) + kmy;                                         \
        const real* k1_ = &sK[0][0][0] + (((zz) >> 1) + 1) % 3 * (KR * KC) + kmy;                                   \
        const bool below_ = wy != 0;                                                                                \
        const int xp_ = below_ ? ((qq) ^ 1) & 1 : (qq) & 1;                                                         \
        const int ro_ = below_ ? KC : 0;                                                                            \
        auto g0_ = [&](int dx, int dy, int dz) { return (dz ? k1_ : k0_)[ro_ + dy * KC + dx]; };                    \
        auto g1_ = [&](int dx, int dy, int dz) { return (dz ? k1_ : k0_)[ro_ + 1 + dy * KC + dx]; };                \
        switch ((below_ ? 4 : 0) + xp_ * 2 + ((zz) & 1)) {                                                          \
            case 0: e.x = interpolate3d_point<real>(0, 0, 0, g0_); e.y = interpolate3d_point<real>(0, 0, 0, g1_); break; \
            case 1: e.x = interpolate3d_point<real>(0, 0, 1, g0_); e.y = interpolate3d_point<real>(0, 0, 1, g1_); break; \
            case 2: e.x = interpolate3d_point<real>(1, 0, 0, g0_); e.y = interpolate3d_point<real>(1, 0, 0, g1_); break; \
            case 3: e.x = interpolate3d_point<real>(1, 0, 1, g0_); e.y = interpolate3d_point<real>(1, 0, 1, g1_); break; \
            case 4: e.x = interpolate3d_point<real>(0, 1, 0, g0_); e.y = interpolate3d_point<real>(0, 1, 0, g1_); break; \
            case 5: e.x = interpolate3d_point<real>(0, 1, 1, g0_); e.y = interpolate3d_point<real>(0, 1, 1, g1_); break; \
            case 6: e.x = interpolate3d_point<real>(1, 1, 0, g0_); e.y = interpolate3d_point<real>(1, 1, 0, g1_); break; \
            default: e.x = interpolate3d_point<real>(1, 1, 1, g0_); e.y = interpolate3d_point<real>(1, 1, 1, g1_); break; \
        }                                                                                                           \
        if (!(xp_ | j0)) e.x = 0; /* x = 0: a boundary entry */                                                     \
    } while (0)
#define MGX_K2_REQUEST(plane)                                                                   \
    do {                                                                                        \
        if (kload) {                                                                            \
            const real* c_ = coarse + (size_t)(plane) * CPL;                                    \
            _Pragma("unroll") for (int a = 0; a < NK; a++) kt[a] = c_[kg[a]];                   \
            if (klast) kt[NK] = c_[kg[NK]];                                                     \
        }                                                                                       \
    } while (0)
#define MGX_K2_STORE(plane)                                                                     \
    do {                                                                                        \
        if (kload) {                                                                            \
            real* d_ = &sK[(plane) % 3][w][lane];                                               \
            _Pragma("unroll") for (int a = 0; a < NK; a++) d_[64 * a] = kt[a];                  \
            if (klast) d_[64 * NK] = kt[NK];                                                    \
        }                                                                                       \
    } while (0)
#define MGX_CORR_PAIR2(kofs, px0, zz, e0, e1)                                                                       \
    do {                                                                                                            \
        const real* k0_ = &sK[0][0][0] + ((zz) >> 1) % 3 * (KR * KC) + (kofs);                                      \
        const real* k1_ = &sK[0][0][0] + (((zz) >> 1) + 1) % 3 * (KR * KC) + (kofs);                                \
        auto g0_ = [&](int dx, int dy, int dz) { return (dz ? k1_ : k0_)[dy * KC + dx]; };                          \
        auto g1_ = [&](int dx, int dy, int dz) { return (dz ? k1_ : k0_)[KC + dy * KC + dx]; };                     \
        switch ((px0) * 2 + ((zz) & 1)) {                                                                           \
            case 0: e0 = interpolate3d_point<real>(0, 1, 0, g0_); e1 = interpolate3d_point<real>(1, 0, 0, g1_); break; \
            case 1: e0 = interpolate3d_point<real>(0, 1, 1, g0_); e1 = interpolate3d_point<real>(1, 0, 1, g1_); break; \
            case 2: e0 = interpolate3d_point<real>(1, 1, 0, g0_); e1 = interpolate3d_point<real>(0, 0, 0, g1_); break; \
            default: e0 = interpolate3d_point<real>(1, 1, 1, g0_); e1 = interpolate3d_point<real>(0, 0, 1, g1_); break; \
        }                                                                                                           \
    } while (0)
#define MGX_CORR_RIM2(qq, zz, rr, e)                                                                                 \
    do {                                                                                                            \
        const real* k0_ = &sK[0][0][0] + ((zz) >> 1) % 3 * (KR * KC) + kmy;                                         \
        const real* k1_ = &sK[0][0][0] + (((zz) >> 1) + 1) % 3 * (KR * KC) + kmy;                                   \
        const bool left_ = wx == 0;                                                                                 \
        rr = left_ ? ((qq) & 1) : 1 - ((qq) & 1);                                                                   \
        const int co_ = (left_ ? -1 : 2) + (rr) * KC;                                                               \
        auto g_ = [&](int dx, int dy, int dz) { return (dz ? k1_ : k0_)[co_ + dy * KC + dx]; };                     \
        switch ((left_ ? 4 : 0) + (rr) * 2 + ((zz) & 1)) {                                                          \
            case 0: e = interpolate3d_point<real>(0, 1, 0, g_); break;                                              \
            case 1: e = interpolate3d_point<real>(0, 1, 1, g_); break;                                              \
            case 2: e = interpolate3d_point<real>(0, 0, 0, g_); break;                                              \
            case 3: e = interpolate3d_point<real>(0, 0, 1, g_); break;                                              \
            case 4: e = interpolate3d_point<real>(1, 1, 0, g_); break;                                              \
            case 5: e = interpolate3d_point<real>(1, 1, 1, g_); break;                                              \
            case 6: e = interpolate3d_point<real>(1, 0, 0, g_); break;                                              \
            default: e = interpolate3d_point<real>(1, 0, 1, g_); break;                                             \
        }                                                                                                           \
    } while (0)
#define MGX_LD2(p, i) (*(const vec2*)&(p)[(i)])
#define MGX_LOAD_RIM2(dz, qq, X, Nv, Sv)                                                       \
    do {                                                                                       \
        const real* p_ = pv + (dz) * sxy;                                                      \
        if (wy == 0) Nv = MGX_LD2(p_, roffN + (qq) * H + j0);                                  \
        if (wy == WY - 1) Sv = MGX_LD2(p_, roffS + ((qq) ^ ((R - 1) & 1)) * H + j0);           \
        if (rimL || rimR) {                                                                    \
            _Pragma("unroll") for (int r = 0; r < R; r++) {                                    \
                const int qr_ = (qq) ^ (r & 1);                                                \
                const int d_ = qr_ ? (rimR ? 2 : 0) : (rimL ? (j0 ? -1 : M - 1) : 0);          \
                X[r] = p_[roff[r] + (1 - qr_) * H + j0 + d_];                                  \
            }                                                                                  \
        }                                                                                      \
    } while (0)
    auto publish = [&](int slot, const vec2 (&c)[R]) __attribute__((always_inline)) {
        ey[slot][wy][wx][0][lane] = c[0];
        ey[slot][wy][wx][1][lane] = c[R - 1];
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < R; r++) ex[slot][wy][wx][0][r] = c[r].x;
        }
        if (lane == 63) {
#pragma unroll
            for (int r = 0; r < R; r++) ex[slot][wy][wx][1][r] = c[r].y;
        }
    };
    auto store_plane = [&](int dz, int qq, const vec2 (&O)[R]) __attribute__((always_inline)) {
        real* p = po + dz * sxy;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int qr = qq ^ (r & 1);
            if (lane_on && r < nrows) {
                real* d = &p[roff[r] + qr * H + j0];
                if (qr | j0) __builtin_nontemporal_store(O[r], (vec2*)d);  // both elements are interior points
                else __builtin_nontemporal_store(O[r].y, d + 1);          // x = 0 is a boundary point: element 1 only
            }
        }
    };

#pragma unroll
    for (int r = 0; r < R; r++) {
        const int qr = q ^ (r & 1);
        cp[r] = MGX_LD2(pv, roff[r] - sxy + qr * H + j0);
        cc[r] = MGX_LD2(pv, roff[r] + (1 - qr) * H + j0);
        cu[r] = MGX_LD2(pv, roff[r] + sxy + qr * H + j0);
        fc[r] = FNT ? __builtin_nontemporal_load((const vec2*)&pf[roff[r] + qr * H + j0]) : MGX_LD2(pf, roff[r] + qr * H + j0);
        xc[r] = xn[r] = 0;
        op[r] = vec2{0, 0};
        cn[r] = fn[r] = oc[r] = vec2{0, 0};
    }
    MGX_LOAD_RIM2(0, q, xc, Nc, Sc);
    real er0 = 0;
    vec2 ee0 = {0, 0};
    int rr0 = 0;
    if constexpr (CORR) {
        // own entries of the planes z0-1, z0, z0+1: the correction straight from the coarse array, once per run of planes
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int qr = q ^ (r & 1), y = y0 + r;
            if (rimc[r]) {
                if (qr == 0 && lane == 0) xc[r] = xc[r] + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * j0 - 1, y, z0);
                if (qr == 1 && lane == 63) xc[r] = xc[r] + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * j0 + 4, y, z0);
            }
            if (own0[r]) {
                if (z0 - 1 + zg0 >= 1 && (qr | j0)) cp[r].x = cp[r].x + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * j0 + qr, y, z0 - 1);
                if ((1 - qr) | j0) cc[r].x = cc[r].x + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * j0 + 1 - qr, y, z0);
                if (z0 + 1 <= szg - 2 && (qr | j0)) cu[r].x = cu[r].x + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * j0 + qr, y, z0 + 1);
            }
            if (own1[r]) {
                if (z0 - 1 + zg0 >= 1) cp[r].y = cp[r].y + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * (j0 + 1) + qr, y, z0 - 1);
                cc[r].y = cc[r].y + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * (j0 + 1) + 1 - qr, y, z0);
                if (z0 + 1 <= szg - 2) cu[r].y = cu[r].y + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * (j0 + 1) + qr, y, z0 + 1);
            }
        }
        rr0 = wx == 0 ? ((q ^ 1) & 1) : 1 - ((q ^ 1) & 1);
        if (rimc[rr0] && z0 + 1 <= szg - 2)
            er0 = interp_xs_at<real>(coarse, CH, CP, CPL, wx == 0 ? 2 * j0 - 1 : 2 * j0 + 4, y0 + rr0, z0 + 1);
        if constexpr (EDGEF) {  // the edge-row values of plane z0 (corrected here) and of plane z0 + 1 (ee0: added when they have arrived)
            if (edgeN) {
                if (q | j0) Nc.x = Nc.x + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * j0 + q, y0 - 1, z0);
                Nc.y = Nc.y + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * (j0 + 1) + q, y0 - 1, z0);
            }
            if (edgeS) {
                if ((q ^ 1) | j0) Sc.x = Sc.x + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * j0 + (q ^ 1), y0 + R, z0);
                Sc.y = Sc.y + interp_xs_at<real>(coarse, CH, CP, CPL, 2 * (j0 + 1) + (q ^ 1), y0 + R, z0);
            }
            if (z0 + 1 <= szg - 2) {
                if (edgeN) {
                    if ((q ^ 1) | j0) ee0.x = interp_xs_at<real>(coarse, CH, CP, CPL, 2 * j0 + (q ^ 1), y0 - 1, z0 + 1);
                    ee0.y = interp_xs_at<real>(coarse, CH, CP, CPL, 2 * (j0 + 1) + (q ^ 1), y0 - 1, z0 + 1);
                }
                if (edgeS) {
                    if (q | j0) ee0.x = interp_xs_at<real>(coarse, CH, CP, CPL, 2 * j0 + q, y0 + R, z0 + 1);
                    ee0.y = interp_xs_at<real>(coarse, CH, CP, CPL, 2 * (j0 + 1) + q, y0 + R, z0 + 1);
                }
            }
        }
        // the coarse planes under the arrivals of the first three steps (the loop's requests start with the fourth)
        MGX_K2_REQUEST(min((z0 + 2) >> 1, ckmax));
        MGX_K2_STORE((z0 + 2) >> 1);
        MGX_K2_REQUEST(min(((z0 + 2) >> 1) + 1, ckmax));
        MGX_K2_STORE(((z0 + 2) >> 1) + 1);
        if (z0 & 1) {
            MGX_K2_REQUEST(min(((z0 + 2) >> 1) + 2, ckmax));
            MGX_K2_STORE(((z0 + 2) >> 1) + 2);
        }
    }
    publish(z0 & 1, cc);
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if constexpr (UNR != 0) {
        // the step loop unrolled four times with fixed register roles, literal row parity, buffer-descriptor addressing and the two
        // points of a row as one vector expression: see relax3d_xs_pipe_kernel and mgx_pipe2_step.inc.  UNR - 1 = the row parity of
        // the run's first plane (runs are an even number of planes long, y0 is odd).
        static_assert(R % 2 == 0, "the unrolled loop takes y0 to be odd");
        vec2 c[4][R], fb[2][R], ob[2][R], nb2[2], sb2[2];
        real xb[2][R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            c[0][r] = cp[r]; c[1][r] = cc[r]; c[2][r] = cu[r]; c[3][r] = vec2{0, 0};
            fb[0][r] = fc[r]; fb[1][r] = vec2{0, 0};
            xb[0][r] = xc[r]; xb[1][r] = 0;
            ob[0][r] = ob[1][r] = vec2{0, 0};
        }
        nb2[0] = Nc; nb2[1] = vec2{0, 0};
        sb2[0] = Sc; sb2[1] = vec2{0, 0};
        unsigned kgb[NK + 1];
#pragma unroll
        for (int a = 0; a <= NK; a++) kgb[a] = (unsigned)kg[a] * (unsigned)sizeof(real);
        const unsigned jb = (unsigned)j0 * (unsigned)sizeof(real);  // the lane's byte offset inside a half-row; the rim lanes': the entry right / left
        const unsigned jbR = (unsigned)(j0 + (rimR ? 2 : 0)) * (unsigned)sizeof(real), jbL = (unsigned)(j0 + (rimL ? (j0 ? -1 : M - 1) : 0)) * (unsigned)sizeof(real);
        {
            int z = z0;
            for (;;) {
#define MGX_K 0
#include "mgx_pipe2_step.inc"
#undef MGX_K
                if (++z >= z1) break;
#define MGX_K 1
#include "mgx_pipe2_step.inc"
#undef MGX_K
                if (++z >= z1) break;
#define MGX_K 2
#include "mgx_pipe2_step.inc"
#undef MGX_K
                if (++z >= z1) break;
#define MGX_K 3
#include "mgx_pipe2_step.inc"
#undef MGX_K
                if (++z >= z1) break;
            }
        }
        const int kl = (z1 - z0 - 1) & 3;  // the last step: its results sit in ob[kl & 1], its row parity is (UNR - 1) ^ (kl & 1)
        if (kl & 1) store_plane(-1, (UNR - 1) ^ 1, ob[1]);
        else store_plane(-1, UNR - 1, ob[0]);
    } else {
        for (int z = z0; z < z1; z++) {
            const bool more = z + 1 < z1;
            if (z > z0) store_plane(-1, q ^ 1, op);
            if (more) {
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int qn = q ^ 1 ^ (r & 1);
                    cn[r] = MGX_LD2(pv, roff[r] + 2 * sxy + qn * H + j0);
                    fn[r] = FNT ? __builtin_nontemporal_load((const vec2*)&pf[roff[r] + sxy + qn * H + j0]) : MGX_LD2(pf, roff[r] + sxy + qn * H + j0);
                }
                MGX_LOAD_RIM2(1, q ^ 1, xn, Nn, Sn);
                if constexpr (CORR) {
                    if (!(z & 1) && z + 4 < z1) MGX_K2_REQUEST(min((z >> 1) + 3, ckmax));  // the LAST loads of the step (see relax3d_xs_pipe_kernel)
                }
                publish((z + 1) & 1, cu);
            }
            const int slot = z & 1;
            const vec2 Nl = ey[slot][wyN][wx][1][lane], Sl = ey[slot][wyS][wx][0][lane];
            const vec2 Nedge = wy > 0 ? Nl : Nc;
            const vec2 Sedge = wy < WY - 1 ? Sl : Sc;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int qr = q ^ (r & 1);
                const real fromR = ex[slot][wy][wxR][0][r], fromL = ex[slot][wy][wxL][1][r];
                // the x neighbour that is not the point's own pair: q_r = 1 -> E: element 0 takes the lane's element 1, element 1
                // the next lane's element 0; q_r = 0 -> W: element 1 takes the lane's element 0, element 0 the previous lane's 1
                real far;
                if (qr) {
                    far = __shfl_down(cc[r].x, 1, 64);
                    if (lane == 63) far = fromR;
                    if (rimR) far = xc[r];
                } else {
                    far = __shfl_up(cc[r].y, 1, 64);
                    if (lane == 0) far = fromL;
                    if (rimL) far = xc[r];
                }
                const vec2 N = r == 0 ? Nedge : cc[r > 0 ? r - 1 : 0];
                const vec2 S = r == R - 1 ? Sedge : cc[r < R - 1 ? r + 1 : r];
                const real W0 = qr ? cc[r].x : far, E0 = qr ? cc[r].y : cc[r].x;
                const real W1 = qr ? cc[r].y : cc[r].x, E1 = qr ? far : cc[r].y;
                oc[r].x = relax3d_point_rd<real>(W0, E0, N.x, S.x, cp[r].x, cu[r].x, fc[r].x, hx2, hy2, hz2, rd);
                oc[r].y = relax3d_point_rd<real>(W1, E1, N.y, S.y, cp[r].y, cu[r].y, fc[r].y, hx2, hy2, hz2, rd);
            }
            real en0[R], en1[R];  // CORR: the corrections of the entries that are on their way (plane z + 2) ...
            bool dc0[R], dc1[R];  // ... if they get one
#pragma unroll
            for (int r = 0; r < R; r++) {
                en0[r] = en1[r] = 0;
                dc0[r] = dc1[r] = false;
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            real er = 0;
            int rrim = 0;
            if constexpr (CORR) {
                if (more) {
                    MGX_CORR_PAIR2(kmy, q ^ 1, z + 2, en0[0], en0[1]);
                    MGX_CORR_PAIR2(kmy + 1, q ^ 1, z + 2, en1[0], en1[1]);
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        dc0[r] = own0[r] && z + 2 <= szg - 2 && ((q ^ 1 ^ (r & 1)) | j0);
                        dc1[r] = own1[r] && z + 2 <= szg - 2;
                    }
                    if (z == z0) {
                        er = er0;
                        rrim = rr0;
                    } else if (wx == 0 || wx == WX - 1) {
                        MGX_CORR_RIM2(q ^ 1, z + 1, rrim, er);
                    }
                    if (z + 1 > szg - 2) er = 0;
                }
            }
            if (CORR && kload && more && !(z & 1) && z + 4 < z1) {
                // the staging loads issued last in this step stay in flight (loads return in order: at most NK + 1 outstanding
                // operations means everything issued before them has arrived); they are stored a step later
                if constexpr (NK == 4) __builtin_amdgcn_s_waitcnt(0x0F75);
                else __builtin_amdgcn_s_waitcnt(0x0F70);
            } else {
                __builtin_amdgcn_s_waitcnt(0x0F70);
            }
#pragma unroll
            for (int r = 0; r < R; r++) {
                cp[r] = cc[r];
                cc[r] = cu[r];
                cu[r].x = dc0[r] ? cn[r].x + en0[r] : cn[r].x;
                cu[r].y = dc1[r] ? cn[r].y + en1[r] : cn[r].y;
                fc[r] = fn[r];
                xc[r] = (CORR && rimc[r] && r == rrim) ? xn[r] + er : xn[r];
                op[r] = oc[r];
            }
            if constexpr (CORR) {
                if ((z & 1) && z > z0 && z + 3 < z1) MGX_K2_STORE(((z - 1) >> 1) + 3);  // requested in step z - 1
            }
            Nc = Nn;
            Sc = Sn;
            pv += sxy;
            pf += sxy;
            po += sxy;
            q ^= 1;
        }
        store_plane(-1, q ^ 1, op);
    }
#undef MGX_LOAD_RIM2
#undef MGX_LD2
#undef MGX_K2_REQUEST
#undef MGX_K2_STORE
#undef MGX_CORR_PAIR2
#undef MGX_CORR_RIM2
#undef MGX_CORR_EDGE2
}

// ------------------------------------------------------------------ relax, whole small level in one workgroup
// Levels up to 17^3 (<= 4913 points) are pure launch latency with one launch per colour pass (about 5 us each;
// the thesis runs 3000 sweeps per level).  Here ONE workgroup keeps v and f of the whole level in LDS (2 x 38 KB
// in fp64) and runs all `ncycles` red-black sweeps with a barrier between colour passes.  Same per-point
// expression, same colour order: bit-identical to the multi-launch path.
constexpr int SMALL_MAX = 17;
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

// workgroup shapes 100*WX + 10*WY + R compiled into the library (diagnostic builds carry the whole sweep of round 1)
#ifdef MGX_DIAGNOSTICS
#define MGX_LDS_SHAPES(X)                                                                                          \
    X(4, 2, 4) X(4, 4, 4) X(4, 4, 2) X(4, 2, 2) X(2, 4, 4) X(2, 2, 4) X(1, 4, 4) X(1, 8, 4) X(2, 8, 2) X(2, 4, 2) \
    X(4, 2, 8) X(2, 2, 8) X(8, 2, 4) X(8, 1, 4) X(4, 1, 4) X(4, 1, 8)
#else
#define MGX_LDS_SHAPES(X) X(2, 8, 2) X(4, 4, 2) X(2, 4, 2) X(4, 2, 2) X(1, 8, 4) X(4, 2, 4)
#endif
bool relax3d_lds_shape_known(int shape) {
#define MGX_X(X, Y, RR) if (shape == 100 * X + 10 * Y + RR) return true;
    MGX_LDS_SHAPES(MGX_X)
#undef MGX_X
    return false;
}

// the shortest run of planes the automatic choice hands to the pipelined kernel.  Its launch has a floor (one workgroup per tile
// column filling and draining its pipeline: ~20 us at 1025-point rows, 17 us at 513, 11.5 us at 257) under which
// relax3d_xs_kernel's many small workgroups win; measured per plane size and run length with tools/slab_pass_time.py
// (profiles/r04_slab_pass_time.txt; fp64): 1025^2: pipelined from 9 planes on (21.9 against 26.9 us), 513^2: from ~24 (11 planes:
// 17.2 against 10.4 us, 32: 20.5 against 23.4), 257^2: from ~64 (38 planes: 12.3 against 9.4 us).  Whole levels have hundreds
// of planes; the short runs are the edge passes and thin slabs of the multi-GPU schedule.
template <class real>
static int pipe_min_planes(int sx) {
    const int M = (sx + 1) / 2;
    if (sizeof(real) == 4) return 8;
    return M - 1 >= 512 ? 8 : (M - 1 >= 256 ? 24 : 64);
}

// fp32 on wide levels: two x-pairs per lane (relax3d_xs_pipe_v2_kernel).  A lane of that kernel owns both pairs of its slot or
// none, so the level needs an even number of interior pairs: rows of 4k + 1 points (every 2^k + 1 >= 5).  Rows of 4k + 3 points
// (515, 771, 1023, ...) would have the last lane relax the boundary column x = sx - 1 and store into the odd half's pad: they
// take the one-pair kernel.
template <class real>
static bool pipe_v2_takes(const mgx_ctx* ctx, int sx) {
    if constexpr (sizeof(real) != 4) return false;  // the two-pair kernel exists in fp32 only
    const int pairs = (sx + 1) / 2 - 1;
    return ctx->relax_v2 && pairs >= 256 && pairs % 2 == 0;
}

// ---- the pipelined smoother, relax3d_xs_pipe_kernel and relax3d_xs_pipe_v2_kernel: pipe_plan decides how a pass launches,
// pipe_launch launches it
enum class PipePass { Plain, Zero, Corr };  // a colour pass; the first sweep from zero (VAR = 3); the correcting red pass (VAR = 2)

struct PipePlan {
    bool v2 = false;            // relax3d_xs_pipe_v2_kernel (two x-pairs per lane)
    int WX = 2, WY = 8, R = 2;  // waves across x and y, rows per wave
    bool fnt = false;           // non-temporal loads of f
    int unr = 0;                // 0: the rolled step loop; unrolled four times: 1 + q0 (entry row parity q0), 3 + q0 requesting two steps ahead
    int zchunk = 0;             // planes per run (even when unrolled)
    int gx = 0, gy = 0;         // tiles across x and y
    dim3 grid, block;
    int xcd = 0;
    // the correcting pass corrects every value it reads from a neighbouring tile itself: no set P beforehand
    bool corrects_edges() const { return !v2 || unr; }
};

// the shapes with an unrolled step loop: those of the automatic choice (2 x 8 and 2 x 4 waves of 2 rows) and, in diagnostic builds,
// tiles of 256 pairs x 8 rows (timing experiments only)
static constexpr bool pipe_shape_unrolls(int WX, int WY, int R) {
#ifdef MGX_DIAGNOSTICS
    if (WX == 4 && WY == 4 && R == 2) return true;
#endif
    return R == 2 && WX == 2 && (WY == 8 || WY == 4);
}

// The launch of a pass over the planes [zbeg, zend) of a level of sy rows of sx points, colour = the colour it updates.  Returns
// false when the pipelined kernels do not take the level (the correcting pass: the caller has asked corr_fused_takes).
template <class real>
static bool pipe_plan(const mgx_ctx* ctx, PipePass pass, int sx, int sy, int zbeg, int zend, int colour, PipePlan& p) {
    const int M = (sx + 1) / 2, planes = zend - zbeg, u = ctx->pipe_unroll;
    const bool fp64 = sizeof(real) == 8;
    // f is read exactly once per pass: load it non-temporally when the pass is too large to stay in the 256 MiB Infinity Cache
    // anyway (+1.5 % at 513^3 and 1025^3); a cache-resident level (257^3) is 5 % faster without
    const bool big = (size_t)sx * sy * (size_t)planes * sizeof(real) > ((size_t)256 << 20);
    int target = 0;       // > 0: runs of planes that make one resident round of `target` workgroups
    bool unroll = false;  // relax3d.unroll has the pass's bit set (one-pair fp32: and bit 8)
    p = PipePlan();
    p.fnt = big;
    if (pass == PipePass::Corr) {
        if (ctx->corr_v2 && pipe_v2_takes<real>(ctx, sx)) {  // fp32, wide level: two pairs per lane
            p.v2 = true;
            target = ctx->num_cus;
            unroll = u & 4;
        } else if (ctx->corr_low && fp64) {  // EXPERIMENT: 8-wave workgroups (tiles of 8 rows), two to a CU; rolled only
            p.WY = 4;
            target = 2 * ctx->num_cus;
        } else {
            target = ctx->num_cus * (fp64 ? 1 : 8);
            unroll = (u & 1) && (fp64 || (u & 8));
        }
    } else if (pass == PipePass::Plain && ctx->relax_lds < 0 && pipe_v2_takes<real>(ctx, sx)) {
        // fp32 on wide levels: two pairs per lane (8-byte loads), 2 x 8 waves of 2 rows over 256 pairs x 16 rows, one resident round
        // of workgroups as in fp64 (measured)
        if (sy - 2 < 64 || planes < 8) return false;
        p.v2 = true;
        target = ctx->num_cus;
        unroll = u & 4;
    } else if (pass == PipePass::Zero || ctx->relax_lds < 0) {
        // automatic (the default).  Measured on MI355X (tools/sweep_pipe.py, profiles/r01_sweep_pipe_*.txt): the
        // pipelined kernel with 2 x 8 waves of 2 rows wins from 257^3 up when the launch is ONE resident round of
        // workgroups -- about one 16-wave workgroup per CU, each streaming a long run of planes (fp32 moves half the
        // bytes per wave and wants 8 x as many, shorter runs); below 257^2 rows, or for runs of a few planes (the
        // edge planes of a z-slab), relax3d_xs_kernel is faster.  The first sweep from zero takes the same levels from 8 planes on,
        // except fp32 levels wide enough for the two-pairs-per-lane kernel.
        if (pass == PipePass::Zero ? !ctx->relax_zero_sweep || ctx->relax_lds != -1 || pipe_v2_takes<real>(ctx, sx) || planes < 8
                                   : planes < pipe_min_planes<real>(sx))
            return false;
        if (M - 1 < 128 || sy - 2 < 64) return false;
        // up to 257 rows (fp64): 2 x 4 waves over 8 rows, two 8-wave workgroups per CU -- twice the tiles, so runs of 16
        // instead of 8 planes (the three planes a run loads before its first result weigh half as much): 37.3 against
        // 39.4 us per pass at 257^3
        const bool low = fp64 && sy - 2 <= 256 && !big;
        if (low) p.WY = 4;
        target = ctx->num_cus * (fp64 ? (low ? 2 : 1) : 8);
        unroll = (u & 2) && (fp64 || (u & 8));
    } else {  // "relax3d.lds" = 1000 + 100*WX + 10*WY + R (+ 2000: non-temporal f; below 1000: relax3d_xs_lds_kernel, diagnostic builds)
        const int code = ctx->relax_lds % 1000;
        p.WX = code / 100;
        p.WY = (code / 10) % 10;
        p.R = code % 10;
        if (M - 1 < 64 * p.WX || sy - 2 < p.WY * p.R) return false;
        p.fnt = ctx->relax_lds >= 3000 && p.R == 2 && p.WX * p.WY == 16;
        unroll = ctx->relax_lds >= 1000 && pipe_shape_unrolls(p.WX, p.WY, p.R) && (u & 2) && (fp64 || (u & 8));
    }
    p.gx = ceil_div(M - 1, 64 * p.WX * (p.v2 ? 2 : 1));
    p.gy = ceil_div(sy - 2, p.WY * p.R);
    int zchunk = ctx->relax_zchunk;
    if (zchunk <= 0 && target > 0) {
        const int tiles = p.gx * p.gy;
        const int nchunks = max(1, (target + tiles / 2) / tiles);
        zchunk = max(8, ceil_div(planes, nchunks));
    } else if (zchunk <= 0) {  // shape codes: runs of 16 planes, halved while the launch has fewer than 32 waves per CU
        const long long tiles = (long long)p.gx * p.gy;
        zchunk = 16;
        while (zchunk > 2 && tiles * ceil_div(planes, zchunk) * p.WX * p.WY < 32LL * ctx->num_cus) zchunk >>= 1;
    }
    if (unroll && planes_fit_descriptor<real>(sx, sy)) {
        // the step loop unrolled four times, register roles and row parity fixed per step: runs of an even number of planes, so
        // that every run starts with the row parity q0 the instantiation is compiled for.  relax3d.unroll bit 16 (plain one-pair
        // passes): the column and f requested two steps ahead, twice the bytes in flight
        const int q0 = (colour + 1 + zbeg) & 1;
        zchunk += zchunk & 1;
        p.unr = 1 + q0 + (pass == PipePass::Plain && !p.v2 && (u & 16) ? 2 : 0);
        if (p.WY != 8) p.fnt = false;  // the unrolled 4 x 4 shape of diagnostic builds reads f through the caches
    }
    p.zchunk = zchunk;
    p.grid = dim3((unsigned)p.gx * p.gy * ceil_div(planes, zchunk));
    p.block = dim3(64, p.WX * p.WY, 1);
    p.xcd = ctx->relax_xcd == 1 ? 1 : 0;
    return true;
}

// The one launch of both kernels: the instantiation for the plan's FNT and UNR (those that exist are listed in unr_max and fnt_ok;
// a plan asks for no other).  Records the launch as the context's last_relax_kernel: the template arguments up to VAR, in the
// kernel's order (callers and tests read the pass kind from the end of the name; the rolled or unrolled form is not part of it).
template <class real, bool V2, int WX, int WY, int R, int VAR>
static void pipe_launch(mgx_ctx* ctx, const PipePlan& p, const real* vin, real* vout, const real* f, int sx, int sy, int zbeg, int zend,
                        real hx2, real hy2, real hz2, int colour, const real* coarse = nullptr, int cx = 0, int cy = 0, int szg = 0,
                        int ckmax = 0, int zg0 = 0) {
    // UNR 3 / 4: the plain one-pair pass only; the correcting pass in 8-wave workgroups: rolled only
    constexpr int unr_max = V2 || VAR == 3 ? 2 : VAR == 2 ? (WY == 8 ? 2 : 0) : (pipe_shape_unrolls(WX, WY, R) ? 4 : 0);
    constexpr bool fnt_ok = !(VAR == 3 && WY == 4);  // the first sweep from zero in 8-wave workgroups: cache-resident levels only
    snprintf(ctx->last_relax_kernel, sizeof ctx->last_relax_kernel, "%s<%s,%d,%d,%d,%s,%d>",
             V2 ? "relax3d_xs_pipe_v2_kernel" : "relax3d_xs_pipe_kernel", sizeof(real) == 8 ? "double" : "float", WX, WY, R,
             p.fnt ? "true" : "false", VAR);
    const auto launch = [&](auto fnt, auto unr) {
        constexpr bool F = decltype(fnt)::value;
        constexpr int U = decltype(unr)::value;
        if constexpr ((F && !fnt_ok) || U > unr_max) {
            return;
        } else if constexpr (V2) {
            MGX_LAUNCH((relax3d_xs_pipe_v2_kernel<real, WX, WY, R, F, VAR, U>), p.grid, p.block, 0, ctx->compute, vin, vout, f, sx, sy,
                       zbeg, zend, hx2, hy2, hz2, colour, p.zchunk, p.gx, p.gy, p.xcd, coarse, cx, cy, szg, ckmax, zg0);
        } else {  // non-temporal f is compiled for two rows per wave (a plan asks for it with R = 2 only)
            MGX_LAUNCH((relax3d_xs_pipe_kernel<real, WX, WY, F ? 2 : R, F, VAR, U>), p.grid, p.block, 0, ctx->compute, vin, vout, f, sx,
                       sy, zbeg, zend, hx2, hy2, hz2, colour, p.zchunk, p.gx, p.gy, p.xcd, coarse, cx, cy, szg, ckmax, zg0);
        }
    };
    const auto by_unr = [&](auto fnt) {
        switch (p.unr) {
            case 0: launch(fnt, std::integral_constant<int, 0>()); break;
            case 1: launch(fnt, std::integral_constant<int, 1>()); break;
            case 2: launch(fnt, std::integral_constant<int, 2>()); break;
            case 3: launch(fnt, std::integral_constant<int, 3>()); break;
            default: launch(fnt, std::integral_constant<int, 4>()); break;
        }
    };
    if (p.fnt) by_unr(std::true_type());
    else by_unr(std::false_type());
}

// a plain colour pass of relax3d_xs_pipe_kernel in the shape WX x WY x R (diagnostic builds: and its timing variants)
template <class real, int WX, int WY, int R>
static void pipe_pass_shape(mgx_ctx* ctx, PipePlan p, real* v, const real* f, int sx, int sy, int zbeg, int zend, real hx2, real hy2,
                            real hz2, int colour) {
#ifdef MGX_DIAGNOSTICS
    if (ctx->relax_lds > 0 && ctx->relax_lds < 1000) {  // relax3d_xs_lds_kernel: no software pipeline
        note_relax_kernel<real>(ctx, "relax3d_xs_lds_kernel", WX, WY, R);
        MGX_LAUNCH((relax3d_xs_lds_kernel<real, WX, WY, R>), p.grid, p.block, 0, ctx->compute, (const real*)v, v, f, sx, sy, zbeg, zend,
                   hx2, hy2, hz2, colour, p.zchunk, p.gx, p.gy, p.xcd);
        return;
    }
    if constexpr (pipe_shape_unrolls(WX, WY, R)) {
        if (p.unr && ctx->relax_ablate == 77) {  // TIMING ONLY: the access pattern of a colour-contiguous layout (wrong results)
            snprintf(ctx->last_relax_kernel, sizeof ctx->last_relax_kernel, "relax3d_xs_pipe_kernel<%s,%d,%d,2,%s,0,1,1>",
                     sizeof(real) == 8 ? "double" : "float", WX, WY, p.fnt ? "true" : "false");
            if (p.fnt)
                MGX_LAUNCH((relax3d_xs_pipe_kernel<real, WX, WY, 2, true, 0, 1, 1>), p.grid, p.block, 0, ctx->compute, (const real*)v, v,
                           f, sx, sy, zbeg, zend, hx2, hy2, hz2, colour, p.zchunk, p.gx, p.gy, p.xcd);
            else
                MGX_LAUNCH((relax3d_xs_pipe_kernel<real, WX, WY, 2, false, 0, 1, 1>), p.grid, p.block, 0, ctx->compute, (const real*)v, v,
                           f, sx, sy, zbeg, zend, hx2, hy2, hz2, colour, p.zchunk, p.gx, p.gy, p.xcd);
            return;
        }
    }
    if (p.unr) p.xcd |= (ctx->relax_ablate >= 100 ? ctx->relax_ablate - 100 : 0) << 4;  // "relax3d.ablate" = 100 + bits: see the kernel
#endif
    pipe_launch<real, false, WX, WY, R, 0>(ctx, p, v, v, f, sx, sy, zbeg, zend, hx2, hy2, hz2, colour);
}

// one colour pass on the pipelined kernels: the automatic choice, or the shape code "relax3d.lds".  Returns false when the level is
// not taken (the caller falls back to relax3d_xs_kernel).
template <class real>
static bool relax3d_xs_pass_lds(mgx_ctx* ctx, real* v, const real* f, int sx, int sy, int zbeg, int zend, real hx2, real hy2,
                                real hz2, int colour) {
    PipePlan p;
    if (!pipe_plan<real>(ctx, PipePass::Plain, sx, sy, zbeg, zend, colour, p)) return false;
    if (p.v2) {  // fp32 only (pipe_v2_takes)
        if constexpr (sizeof(real) == 4) pipe_launch<real, true, 2, 8, 2, 0>(ctx, p, v, v, f, sx, sy, zbeg, zend, hx2, hy2, hz2, colour);
        return true;
    }
#define MGX_X(X, Y, RR)                                                                                         \
    case 100 * X + 10 * Y + RR:                                                                                 \
        pipe_pass_shape<real, X, Y, RR>(ctx, p, v, f, sx, sy, zbeg, zend, hx2, hy2, hz2, colour); \
        return true;
    switch (100 * p.WX + 10 * p.WY + p.R) {
        MGX_LDS_SHAPES(MGX_X)
        default: return false;
    }
#undef MGX_X
}

// The FIRST SWEEP of a level that counts as all zeros (boundary entries zero in memory) in one launch: the black pass with the
// red pass folded in (relax3d_xs_pipe_kernel, VAR = 3: f in, red and black out).
template <class real>
static bool relax3d_xs_first_sweep_zero(mgx_ctx* ctx, real* v, const real* f, int sx, int sy, int sz, real hx2, real hy2, real hz2) {
    PipePlan p;
    if (!pipe_plan<real>(ctx, PipePass::Zero, sx, sy, 1, sz - 1, 1, p)) return false;
    if (p.WY == 4)
        pipe_launch<real, false, 2, 4, 2, 3>(ctx, p, f, v, f, sx, sy, 1, sz - 1, hx2, hy2, hz2, 1, nullptr, 0, 0, sz, 0);
    else
        pipe_launch<real, false, 2, 8, 2, 3>(ctx, p, f, v, f, sx, sy, 1, sz - 1, hx2, hy2, hz2, 1, nullptr, 0, 0, sz, 0);
    return true;
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
        MGX_LAUNCH((relax3d_small_kernel<real, L>), dim3(1), dim3(1024), 0, ctx->compute, v, f, n[0], n[1], n[2], hx2, hy2,
                           hz2, ncycles);
        MGX_LAUNCH_CHECK();
        return MGX_OK;
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
                               int czoff, int pzbeg, int pzend, int colour, bool add = true) {
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

// ---- the coarse-grid correction read on the fly by the first red pass of the post-smoothing (relax3d_xs_pipe_kernel, VAR = 2)
// does a level (rows of sx points, sy rows, `nplanes` planes to update) take it?
static bool corr_fused_takes(const mgx_ctx* ctx, int sx, int sy, int sz_global, int nplanes) {
    const bool small = sx <= SMALL_MAX && sy <= SMALL_MAX && sz_global <= SMALL_MAX && ctx->relax_small;
    return ctx->corr_fuse && !small && ctx->relax_lds < 0 && (sx + 1) / 2 - 1 >= 128 && sy - 2 >= 64 && nplanes >= 8;
}

// the set P (tile-edge cells of that pass) corrected in place: the coarse cells covering the GLOBAL fine planes [zmin, zmax),
// which are the only ones written.  v / coarse_v are local arrays starting at the global planes fzoff / czoff; every coarse
// plane a written fine plane interpolates from must exist locally.
template <class real>
static void corr_pset_launch(mgx_ctx* ctx, real* v, int sx, int sy, int fzoff, const real* coarse_v, const int cn[3], int czoff, int zmin,
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

// the red pass through the correction over the LOCAL planes [zb, ze) of v: `coarse_sh` = the coarse array shifted so that
// local fine plane z interpolates from its planes z >> 1 (+ 1), szl = global plane count - global index of local plane 0,
// ckmax = last plane of coarse_sh that exists; colour = 0 + parity of the slab's global offset.  vout != nullptr: the red
// interior points go there instead of into v (nothing else of vout is written, v is only read)
template <class real>
static void corr_red_launch(mgx_ctx* ctx, real* v, const real* f, int sx, int sy, int zb, int ze, real hx2, real hy2, real hz2, int colour,
                            const real* coarse_sh, int cx, int cy, int szl, int ckmax, int zg0 = 0, real* vout = nullptr) {
    real* const vo = vout ? vout : v;
    PipePlan p;
    pipe_plan<real>(ctx, PipePass::Corr, sx, sy, zb, ze, colour, p);
    if (p.v2) {  // fp32 only (pipe_v2_takes)
        if constexpr (sizeof(real) == 4)
            pipe_launch<real, true, 2, 8, 2, 2>(ctx, p, v, vo, f, sx, sy, zb, ze, hx2, hy2, hz2, colour, coarse_sh, cx, cy, szl, ckmax, zg0);
    } else if (p.WY == 4)
        pipe_launch<real, false, 2, 4, 2, 2>(ctx, p, v, vo, f, sx, sy, zb, ze, hx2, hy2, hz2, colour, coarse_sh, cx, cy, szl, ckmax, zg0);
    else
        pipe_launch<real, false, 2, 8, 2, 2>(ctx, p, v, vo, f, sx, sy, zb, ze, hx2, hy2, hz2, colour, coarse_sh, cx, cy, szl, ckmax, zg0);
    memcpy(ctx->last_corr_kernel, ctx->last_relax_kernel, sizeof ctx->last_corr_kernel);
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

// z-slab forms of the two pieces (multi-GPU post-smoothing, csrc/host/mg_dist3d.inc).  n / cn: GLOBAL sizes; v / f start at
// global plane fzoff (even), coarse_v at czoff <= fzoff / 2 and holds cplanes planes.
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
    corr_pset_launch<real>(ctx, v, n[0], n[1], fzoff, coarse_v, cn, czoff, zmin, zmax);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

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
    int PFX##jacobi_##SFX(mgx_ctx* ctx, real* v, real* tmp, const real* f, const int n[3], const real h[3],      \
                          real omega, int ncycles) {                                                             \
        return mgx::jacobi3d<real, L>(ctx, v, tmp, f, n, h, omega, ncycles);                                     \
    }                                                                                                            \
    int PFX##vcycle_tail_##SFX(mgx_ctx* ctx, int nlev, real* const* v, real* const* f, const int* n,             \
                               const real* h, int v1, int v2, int mode, int top_zero) {                          \
        return mgx::cycle3d_tail<real, L>(ctx, nlev, v, f, n, h, v1, v2, mode, top_zero);                        \
    }                                                                                                            \
    int PFX##vcycle_tail_fits_##SFX(const mgx_ctx* ctx, int nlev, const int* n) {                                \
        return ctx && ctx->relax_small && mgx::tail3_fits(nlev, n, sizeof(real));                                \
    }                                                                                                            \
    int PFX##diff_stats_##SFX(mgx_ctx* ctx, const real* v, const int n[3], const double* host_tx,                \
                              const double* host_ty, const double* host_tz, double host_out[4]) {                \
        return mgx::diff_stats3d<real, L>(ctx, v, n, host_tx, host_ty, host_tz, host_out);                       \
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
    int mgx3dxs_corr_fused_takes_##SFX(const mgx_ctx* ctx, const int n[3], int nplanes) {                        \
        return ctx && n && mgx::corr_fused_takes(ctx, n[0], n[1], n[2], nplanes);                                \
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
    int mgx3dxs_correct_pset_slab_##SFX(mgx_ctx* ctx, real* v, const int n[3], int fzoff, const real* coarse_v,  \
                                        const int cn[3], int czoff, int zmin, int zmax) {                        \
        return mgx::correct_pset3d_slab<real>(ctx, v, n, fzoff, coarse_v, cn, czoff, zmin, zmax);                \
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
