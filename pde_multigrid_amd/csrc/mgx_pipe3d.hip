// mgx_pipe3d.hip -- the pipelined smoothers: one colour of MultiGrid3D::Relax (N3/MultiGrid3D.cpp:489-567), x-split layout, on
// levels >= 257 rows wide, and everything that launches them.  Per-point expression, association order and rounding as in
// mgx_kernels3d.hip: bit-identical to the serial CPU loops.
//   relax3d_xs_pipe_kernel     THE hot kernel.  One workgroup per CU marches a long run of planes; neighbours' edge rows / lanes
//                              through LDS, loads one plane ahead, stores one plane behind, one barrier per plane.  VAR = 2: the
//                              red pass that reads black through the coarse-grid correction, VAR = 3: the first sweep from zero
//   relax3d_xs_pipe_v2_kernel  the same with two x-pairs per lane (fp32 on wide levels)
//   relax3d_xs_lds_kernel      LDS edges without the software pipeline (A/B, diagnostic builds only)
// The unrolled step loops are mgx_pipe_step.inc and mgx_pipe2_step.inc.  pipe_plan decides how a pass launches (PipePlan,
// mgx_host3d.hpp), pipe_launch is the one launch of both kernels; the other units reach them through relax3d_xs_pass_lds,
// relax3d_xs_first_sweep_zero and corr_red_launch.  No other unit names either kernel template.
#include <type_traits>

#include "mgx_host3d.hpp"

namespace mgx {

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

// =========================================================================== host side
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
int pipe_min_planes(int sx) {
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
// (PipePass and PipePlan: mgx_host3d.hpp)

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
bool pipe_plan(const mgx_ctx* ctx, PipePass pass, int sx, int sy, int zbeg, int zend, int colour, PipePlan& p) {
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
bool relax3d_xs_pass_lds(mgx_ctx* ctx, real* v, const real* f, int sx, int sy, int zbeg, int zend, real hx2, real hy2,
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
bool relax3d_xs_first_sweep_zero(mgx_ctx* ctx, real* v, const real* f, int sx, int sy, int sz, real hx2, real hy2, real hz2) {
    PipePlan p;
    if (!pipe_plan<real>(ctx, PipePass::Zero, sx, sy, 1, sz - 1, 1, p)) return false;
    if (p.WY == 4)
        pipe_launch<real, false, 2, 4, 2, 3>(ctx, p, f, v, f, sx, sy, 1, sz - 1, hx2, hy2, hz2, 1, nullptr, 0, 0, sz, 0);
    else
        pipe_launch<real, false, 2, 8, 2, 3>(ctx, p, f, v, f, sx, sy, 1, sz - 1, hx2, hy2, hz2, 1, nullptr, 0, 0, sz, 0);
    return true;
}

// ---- the coarse-grid correction read on the fly by the first red pass of the post-smoothing (relax3d_xs_pipe_kernel, VAR = 2)
// does a level (rows of sx points, sy rows, `nplanes` planes to update) take it?
bool corr_fused_takes(const mgx_ctx* ctx, int sx, int sy, int sz_global, int nplanes) {
    return corr_fused_level_takes(ctx, sx, sy, sz_global) && nplanes >= 8;
}

// the part of that rule that belongs to the level and the context's switches: the rows the kernel runs on.  The z-slab entries
// (mgx3dxs_relax_corr_colour_slab, mgx3dxs_correct_pset_slab) refuse a level it does not hold for; the number of planes is the
// caller's business (the slab driver hands the short edge ranges of an accepted level to the same kernel).
bool corr_fused_level_takes(const mgx_ctx* ctx, int sx, int sy, int sz_global) {
    const bool small = sx <= SMALL_MAX && sy <= SMALL_MAX && sz_global <= SMALL_MAX && ctx->relax_small;
    return ctx->corr_fuse && !small && ctx->relax_lds < 0 && (sx + 1) / 2 - 1 >= 128 && sy - 2 >= 64;
}

// the red pass through the correction over the LOCAL planes [zb, ze) of v: `coarse_sh` = the coarse array shifted so that
// local fine plane z interpolates from its planes z >> 1 (+ 1), szl = global plane count - global index of local plane 0,
// ckmax = last plane of coarse_sh that exists; colour = 0 + parity of the slab's global offset.  vout != nullptr: the red
// interior points go there instead of into v (nothing else of vout is written, v is only read)
template <class real>
void corr_red_launch(mgx_ctx* ctx, real* v, const real* f, int sx, int sy, int zb, int ze, real hx2, real hy2, real hz2, int colour,
                     const real* coarse_sh, int cx, int cy, int szl, int ckmax, int zg0, real* vout) {
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

#define MGX_X(real)                                                                                                              \
    template int pipe_min_planes<real>(int);                                                                                     \
    template bool pipe_plan<real>(const mgx_ctx*, PipePass, int, int, int, int, int, PipePlan&);                                 \
    template bool relax3d_xs_pass_lds<real>(mgx_ctx*, real*, const real*, int, int, int, int, real, real, real, int);            \
    template bool relax3d_xs_first_sweep_zero<real>(mgx_ctx*, real*, const real*, int, int, int, real, real, real);              \
    template void corr_red_launch<real>(mgx_ctx*, real*, const real*, int, int, int, int, real, real, real, int, const real*, int, int, \
                                        int, int, int, real*);
MGX_X(float) MGX_X(double)
#undef MGX_X

}  // namespace mgx

#define MGX_DEFINE_MISC3D(SFX, real)                                                                             \
    int mgx3dxs_corr_fused_takes_##SFX(const mgx_ctx* ctx, const int n[3], int nplanes) {                        \
        return ctx && n && mgx::corr_fused_takes(ctx, n[0], n[1], n[2], nplanes);                                \
    }

extern "C" {
MGX_DEFINE_MISC3D(f32, float)
MGX_DEFINE_MISC3D(f64, double)
}
