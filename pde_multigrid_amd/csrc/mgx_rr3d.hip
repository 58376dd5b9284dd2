// mgx_rr3d.hip -- CalculateResidual + Restrict in one launch (N3/MultiGrid3D.cpp:678-730, 50-184): no residual array.
//   residual_restrict3d_xs_pipe_kernel   pipelined, halos through LDS (x-split, large levels)
//   residual_restrict3d_xs_kernel        streaming register window (x-split)
//   residual_restrict3d_kernel           LDS rolling window (both layouts)
// rr_plan decides how a launch goes (also for the fused black pass of mgx_relax_rr3d.hip), rr_launch launches these three.

#include "mgx_host3d.hpp"

namespace mgx {

// ------------------------------------------------------------------ residual + restrict fused
// One block produces a CTX x CTY tile of coarse points for a chunk of coarse planes [pz0, pz1) and
// marches through them.  The fine residual lives only in an LDS ring of 4 planes of the
// (2*CTX+1) x (2*CTY+1) fine window the tile's 27-point stencils touch: every step adds the two new
// fine planes 2pz, 2pz+1 (plane 2pz-1 is the previous step's 2(pz-1)+1), boundary points -> 0 exactly
// like CalculateResidual, then applies the full-weighting formula.  The fine residual never goes to
// HBM and each fine plane's residual is evaluated once per tile (plus the one-point window overlap).
template <class real, class L, int MODE, int CTX, int CTY>
__global__ void __launch_bounds__(256) residual_restrict3d_kernel(const real* __restrict__ v, const real* __restrict__ f,
                                                                  int sx, int sy, int sz, real hx2, real hy2, real hz2,
                                                                  real* __restrict__ coarse, int cx, int cy, int cz,
                                                                  int pzchunk, int fzoff, int czoff, int pzbeg, int pzend) {
    // sz / cz are the GLOBAL plane counts; the fine arrays start at global plane fzoff and the coarse
    // array at global plane czoff (0 for whole grids); coarse planes [pzbeg, pzend) are produced.
    constexpr int FX = 2 * CTX + 1, FY = 2 * CTY + 1;
    __shared__ real res[4][FY][FX + 1];
    const int pz0 = pzbeg + blockIdx.z * pzchunk, pz1 = min(pz0 + pzchunk, pzend);
    const int px0 = blockIdx.x * CTX, py0 = blockIdx.y * CTY;
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    const int nthreads = blockDim.x * blockDim.y;
    const Geo<L, real> gf(sx, sy), gc(cx, cy);
    const int H = gf.H, P = gf.P;
    const size_t sxy = gf.PL;
    // fine window origin (may be -1 at the low edge: those entries are never read)
    const int gx0 = 2 * px0 - 1, gy0 = 2 * py0 - 1;
    // residual of fine plane gz into ring slot gz & 3.  The window is walked with a compile-time trip
    // count and all global loads of a thread's points are issued before the first division, so one
    // thread keeps NPT x 8 loads in flight instead of 8.
    constexpr int NPT = (FX * FY + 255) / 256;
    auto fill = [&](int gz) {
        const bool zin = gz >= 1 && gz < sz - 1;
        real O[NPT], E[NPT], N[NPT], S[NPT], D[NPT], U[NPT], C[NPT], F[NPT];
        bool in[NPT];
#pragma unroll
        for (int k = 0; k < NPT; k++) {
            const int t = tid + k * 256;
            const int ly = t / FX, lx = t - ly * FX;
            const int gx = gx0 + lx, gy = gy0 + ly;
            in[k] = zin && t < FX * FY && gx >= 1 && gx < sx - 1 && gy >= 1 && gy < sy - 1;
            if (in[k]) {
                const size_t row = (size_t)gy * P + (size_t)(gz - fzoff) * sxy;
                const size_t i = row + L::pos(gx, H);
                O[k] = v[row + L::pos(gx - 1, H)];
                E[k] = v[row + L::pos(gx + 1, H)];
                N[k] = v[i - P];
                S[k] = v[i + P];
                D[k] = v[i - sxy];
                U[k] = v[i + sxy];
                C[k] = v[i];
                F[k] = f[i];
            }
        }
#pragma unroll
        for (int k = 0; k < NPT; k++) {
            const int t = tid + k * 256;
            if (t < FX * FY) {
                const int ly = t / FX, lx = t - ly * FX;
                res[gz & 3][ly][lx] =
                    in[k] ? residual3d_point<real, MODE>(O[k], E[k], N[k], S[k], D[k], U[k], C[k], F[k], hx2, hy2, hz2) : (real)0;
            }
        }
    };
    if (pz0 > 0) fill(2 * pz0 - 1);
    for (int pz = pz0; pz < pz1; pz++) {
        const bool zinterior = pz > 0 && pz < cz - 1;
        if (pz < cz - 1) {  // planes 2pz and 2pz+1 exist
            fill(2 * pz);
            fill(2 * pz + 1);
        }
        __syncthreads();
        for (int t = tid; t < CTX * CTY; t += nthreads) {
            const int ty = t / CTX, tx = t - ty * CTX;
            const int px = px0 + tx, py = py0 + ty;
            if (px >= cx || py >= cy) continue;
            const size_t ci = gc.pos(px) + gc.row(py, pz - czoff);
            if (px == 0 || px == cx - 1 || py == 0 || py == cy - 1 || !zinterior) {
                coarse[ci] = (real)0;  // injection of a boundary residual, which is 0 (:704-705 then :113-119)
                continue;
            }
            const int lx = 2 * tx + 1, ly = 2 * ty + 1, g = 2 * pz;
            coarse[ci] = restrict3d_point<real>([&](int dx, int dy, int dz) { return res[(g + dz) & 3][ly + dy][lx + dx]; });
        }
        __syncthreads();  // slot (2pz-1)&3 is overwritten by the next step's plane 2pz+3
    }
}

// ------------------------------------------------------------------ residual + restrict, streaming (XSplit)
// Lane i of a wave owns the fine x-pair {2i, 2i+1} (= coarse column i) of the 2*CR+3 fine rows around CR
// consecutive coarse rows and marches through a chunk of coarse planes.  v is carried in registers along z
// (every v plane is loaded once), the y-neighbours are the thread's own rows, the x-neighbours come from the
// adjacent lanes by wave shuffle; no LDS, no barrier.  The full-weighting formula of the reference groups its 27
// terms by fine row (N3/MultiGrid3D.cpp:180: suffix _C / _N / _S = y, y-1, y+1), so each row contributes the
// three sub-sums  a = C,  b = ((N+E)+S)+O,  c = ((NE+SE)+SO)+NO  over its 3 x 3 (x, z) neighbourhood and
//   coarse = 1/8 a_C + 1/16 (b_C + (a_N + a_S)) + 1/32 ((c_C + b_N) + b_S) + 1/64 (c_N + c_S)
// is exactly the reference's expression, association included.  Lane 0 of every wave is a halo lane (it only
// supplies the x-1 residuals of lane 1), so a wave produces 63 coarse columns.  Boundary coarse points are not
// written: the host zeroes the output planes first (restricted residual = 0 there, :704-705 then :113-119).
template <class real, int MODE, int CR, int TYW>
__global__ void __launch_bounds__(64 * TYW)
    residual_restrict3d_xs_kernel(const real* __restrict__ v, const real* __restrict__ f, int sx, int sy, int szg, real hx2,
                                  real hy2, real hz2, real* __restrict__ coarse, int cx, int cy, int czg, int pzchunk,
                                  int fzoff, int czoff, int pzbeg, int pzend, int gx, int gy, int xcd_mode) {
    constexpr int NR = 2 * CR + 3;  // fine rows held per lane: residual rows 1 .. NR-2 plus one v-only row each side
    const Geo<XSplit, real> gf(sx, sy), gc(cx, cy);
    const int lane = threadIdx.x;
    int bx, by, bz;
    tile_of_block(xcd_mode, gx, gy, bx, by, bz);
    const int i = bx * 63 + lane;
    const int cyb = 1 + (by * TYW + __builtin_amdgcn_readfirstlane(threadIdx.y)) * CR;
    if (cyb > cy - 2 || i > cx - 1) return;
    int pz0 = pzbeg + bz * pzchunk;
    const int pz1 = min(min(pz0 + pzchunk, pzend), czg - 1);
    if (pz0 < 1) pz0 = 1;
    if (pz0 >= pz1) return;
    const bool hasB = i <= cx - 2;            // the odd-x entry 2i+1 exists
    const bool xinA = i >= 1 && i <= cx - 2;  // x = 2i is interior
    const bool lastlane = lane == 63;
    const int yf0 = 2 * cyb - 2;
    size_t roff[NR];
    bool yin[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const int y = yf0 + r;
        roff[r] = (size_t)min(y, sy - 1) * gf.P;
        yin[r] = y >= 1 && y <= sy - 2;
    }
    const size_t PL = gf.PL;
    auto loadA = [&](int g, real (&A)[NR]) {  // even-x entries of global fine plane g
        const size_t pb = (size_t)(g - fzoff) * PL + i;
#pragma unroll
        for (int r = 0; r < NR; r++) A[r] = v[pb + roff[r]];
    };
    auto loadB = [&](int g, real (&B)[NR]) {  // odd-x entries
        const size_t pb = (size_t)(g - fzoff) * PL + gf.H + (hasB ? i : 0);
#pragma unroll
        for (int r = 0; r < NR; r++) B[r] = v[pb + roff[r]];
    };
    // residuals of fine plane g on rows 1 .. NR-2 for x = 2i (rA) and x = 2i+1 (rB); 0 outside the interior
    auto resid = [&](int g, const real (&AP)[NR], const real (&BP)[NR], const real (&AC)[NR], const real (&BC)[NR],
                     const real (&AN)[NR], const real (&BN)[NR], real (&rA)[NR - 2], real (&rB)[NR - 2]) {
        const bool zin = g >= 1 && g <= szg - 2;
        const size_t pb = (size_t)(g - fzoff) * PL;
#pragma unroll
        for (int r = 1; r < NR - 1; r++) {
            const real fA = f[pb + roff[r] + i];
            const real fB = f[pb + roff[r] + gf.H + (hasB ? i : 0)];
            const real Bl = __shfl_up(BC[r], 1, 64);                                     // v(2i-1): odd entry of lane i-1
            real Ar = __shfl_down(AC[r], 1, 64);                                         // v(2i+2): even entry of lane i+1
            if (lastlane && hasB) Ar = v[pb + roff[r] + i + 1];                          // wave edge: load it
            const real a = residual3d_point<real, MODE>(Bl, BC[r], AC[r - 1], AC[r + 1], AP[r], AN[r], AC[r], fA, hx2, hy2, hz2);
            const real b = residual3d_point<real, MODE>(AC[r], Ar, BC[r - 1], BC[r + 1], BP[r], BN[r], BC[r], fB, hx2, hy2, hz2);
            rA[r - 1] = (zin && yin[r] && xinA && lane > 0) ? a : (real)0;
            rB[r - 1] = (zin && yin[r] && hasB) ? b : (real)0;
        }
    };
    real AP[NR], BP[NR], AC[NR], BC[NR], AN[NR], BN[NR];
    real rAm[NR - 2], rBm[NR - 2], rA0[NR - 2], rB0[NR - 2], rAp[NR - 2], rBp[NR - 2];
    // prologue: v planes 2pz0-2, 2pz0-1, 2pz0 and the residual of plane 2pz0-1
    loadA(2 * pz0 - 2, AP); loadB(2 * pz0 - 2, BP);
    loadA(2 * pz0 - 1, AC); loadB(2 * pz0 - 1, BC);
    loadA(2 * pz0, AN);     loadB(2 * pz0, BN);
    resid(2 * pz0 - 1, AP, BP, AC, BC, AN, BN, rAm, rBm);
    for (int pz = pz0; pz < pz1; pz++) {
        // plane 2pz: shift the v window, load plane 2pz+1
#pragma unroll
        for (int r = 0; r < NR; r++) { AP[r] = AC[r]; BP[r] = BC[r]; AC[r] = AN[r]; BC[r] = BN[r]; }
        loadA(2 * pz + 1, AN); loadB(2 * pz + 1, BN);
        resid(2 * pz, AP, BP, AC, BC, AN, BN, rA0, rB0);
        // plane 2pz+1: shift, load plane 2pz+2
#pragma unroll
        for (int r = 0; r < NR; r++) { AP[r] = AC[r]; BP[r] = BC[r]; AC[r] = AN[r]; BC[r] = BN[r]; }
        loadA(2 * pz + 2, AN); loadB(2 * pz + 2, BN);
        resid(2 * pz + 1, AP, BP, AC, BC, AN, BN, rAp, rBp);
        // per-row sub-sums a, b, c of residual rows 0 .. 2CR (x-1 values: rB of lane i-1)
        real sa[NR - 2], sb[NR - 2], sc[NR - 2];
#pragma unroll
        for (int r = 0; r < NR - 2; r++) {
            const real lm = __shfl_up(rBm[r], 1, 64), l0 = __shfl_up(rB0[r], 1, 64), lp = __shfl_up(rBp[r], 1, 64);
            sa[r] = rA0[r];
            sb[r] = ((rAp[r] + rB0[r]) + rAm[r]) + l0;      // (N + E + S + O): (x,z+1), (x+1,z), (x,z-1), (x-1,z)
            sc[r] = ((rBp[r] + rBm[r]) + lm) + lp;          // (NE + SE + SO + NO)
        }
        if (xinA && lane > 0) {
#pragma unroll
            for (int c = 0; c < CR; c++) {
                const int py = cyb + c;
                if (py <= cy - 2) {
                    const int rn = 2 * c, rc = 2 * c + 1, rs = 2 * c + 2;  // residual rows y-1, y, y+1 of this coarse row
                    coarse[gc.row(py, pz - czoff) + gc.pos(i)] =
                        (1 / 8.0f) * (sa[rc]) + (1 / 16.0f) * (sb[rc] + (sa[rn] + sa[rs])) +
                        (1 / 32.0f) * ((sc[rc] + sb[rn]) + sb[rs]) + (1 / 64.0f) * (sc[rn] + sc[rs]);
                }
            }
        }
        // plane 2pz+1 becomes the next step's plane 2(pz+1)-1
#pragma unroll
        for (int r = 0; r < NR - 2; r++) { rAm[r] = rAp[r]; rBm[r] = rBp[r]; }
    }
}

// ------------------------------------------------------------------ residual + restrict, pipelined, halos through LDS
// The recipe of relax3d_xs_pipe_kernel applied to residual+restrict.  residual_restrict3d_xs_kernel keeps a 7-row
// window per lane and re-reads three of the seven rows of v (and one of five of f) that the next row group also
// reads; those re-reads all reach the fabric (PMC: 3.76 GB for 2.16 GB of v and f at 513^3) as long as neighbouring
// workgroups sit on different XCDs (tile_of_block: with every XCD working on one contiguous run of tiles they meet in one
// L2).  Here a wave owns OWN fine rows (OWN / 2 coarse rows; OWN = 2: sixteen waves of 122 VGPRs, the default; OWN = 4:
// eight waves of 240) and loads nothing else: the row above and the row below its own come from the neighbouring waves of
// the workgroup through LDS (v of the current plane), and so does the residual row the last coarse row needs from
// below (the next wave's first row).  The last wave of a workgroup is a halo wave: it supplies those rows to the wave
// above it and produces no output (it loads two rows of v and one of f), so a workgroup of TYW waves produces
// (OWN / 2) (TYW-1) coarse rows.  MODE | 2: the residual multiplies by exact reciprocals (residual3d_point) -- with three
// IEEE divisions per point this kernel was bound by the VALU, not by memory.  Software pipeline as in the smoother: in the step of fine plane g a wave requests v of
// plane g+2 and f of plane g+1, publishes its edge rows of plane g+1, reads its neighbours' edge rows of plane g,
// computes the residual of plane g, publishes the residual of its first row, and meets the others at ONE barrier;
// what it requested is waited for only after the barrier.  The coarse plane pz is formed at the start of the step
// after its third residual plane (2pz+1), when the neighbour's residual rows are visible.  Lanes 0 and 63 are halo
// lanes (62 coarse columns per wave, nobody loads a foreign column).  Expressions and association: those of
// residual_restrict3d_xs_kernel.
template <class real, int MODE, int TYW, int OWN = 4>
__global__ void __launch_bounds__(64 * TYW)
    residual_restrict3d_xs_pipe_kernel(const real* __restrict__ v, const real* __restrict__ f, int sx, int sy, int szg,
                                       real hx2, real hy2, real hz2, real* __restrict__ coarse, int cx, int cy, int czg,
                                       int pzchunk, int fzoff, int czoff, int pzbeg, int pzend, int gx, int gy, int xcd_mode) {
    static_assert(OWN == 2 || OWN == 4, "a wave owns one or two coarse rows");
    __shared__ real hv[2][TYW][2][2][64];  // [plane & 1][wave][first / last own row][A / B][lane]: v
    __shared__ real hr[4][TYW][2][64];     // [plane & 3][wave][A / B][lane]: residual of the wave's first own row
    const Geo<XSplit, real> gf(sx, sy), gc(cx, cy);
    const int lane = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.y);
    int bx, by, bz;
    tile_of_block(xcd_mode, gx, gy, bx, by, bz);
    const int in = bx * 62 + lane;  // nominal coarse column; lanes past the row are clamped and masked
    const int i = min(in, cx - 1);
    const int cyb = 1 + (by * (TYW - 1) + w) * (OWN / 2);  // this wave's coarse rows: cyb (, cyb + 1)
    const bool halo_wave = w == TYW - 1;           // supplies rows to the wave above, produces nothing
    int pz0 = pzbeg + bz * pzchunk;
    const int pz1 = min(min(pz0 + pzchunk, pzend), czg - 1);
    if (pz0 < 1) pz0 = 1;
    if (pz0 >= pz1) return;  // uniform over the workgroup
    const bool hasB = i <= cx - 2;
    const bool xinA = in >= 1 && in <= cx - 2;
    const bool validB = in <= cx - 2 && lane < 63;
    const bool produces = !halo_wave && xinA && lane >= 1 && lane <= 62;
    const int Y0 = 2 * cyb - 1;  // first own fine row
    int roff[OWN];
    bool yin[OWN];
#pragma unroll
    for (int o = 0; o < OWN; o++) {
        roff[o] = min(Y0 + o, sy - 1) * gf.P;
        yin[o] = Y0 + o <= sy - 2;  // Y0 >= 1
    }
    const int roffU = min(Y0 - 1, sy - 1) * gf.P;  // the row above (loaded by the first wave of the workgroup only)
    const int nv = halo_wave ? 2 : OWN, nf = halo_wave ? 1 : OWN;  // rows of v / f this wave loads
    const int PL = (int)gf.PL;
    const int offA = i, offB = gf.H + (hasB ? i : 0);
    const int wU = w > 0 ? w - 1 : 0, wD = w < TYW - 1 ? w + 1 : TYW - 1;

    real AP[OWN], BP[OWN], AC[OWN], BC[OWN], AN[OWN], BN[OWN], AX[OWN], BX[OWN], fA[OWN], fB[OWN], fAX[OWN], fBX[OWN];
    real rAm[OWN], rBm[OWN], rA0[OWN], rB0[OWN], rAp[OWN], rBp[OWN];
    real tAc = 0, tBc = 0, tAx = 0, tBx = 0;  // the row above, planes g / g+1 (first wave only)
    const int g0 = 2 * pz0 - 1, glast = 2 * pz1 - 1;
    const real* pv = v + (size_t)(g0 - fzoff) * gf.PL;  // plane g of v and f, advanced with g
    const real* pf = f + (size_t)(g0 - fzoff) * gf.PL;
#pragma unroll
    for (int o = 0; o < OWN; o++) {
        AP[o] = BP[o] = AC[o] = BC[o] = AN[o] = BN[o] = AX[o] = BX[o] = fA[o] = fB[o] = fAX[o] = fBX[o] = 0;
        rAm[o] = rBm[o] = rA0[o] = rB0[o] = rAp[o] = rBp[o] = 0;
        if (o < nv) {
            AP[o] = pv[roff[o] - PL + offA];
            BP[o] = pv[roff[o] - PL + offB];
            AC[o] = pv[roff[o] + offA];
            BC[o] = pv[roff[o] + offB];
            AN[o] = pv[roff[o] + PL + offA];
            BN[o] = pv[roff[o] + PL + offB];
        }
        if (o < nf) {
            fA[o] = pf[roff[o] + offA];
            fB[o] = pf[roff[o] + offB];
        }
    }
    if (w == 0) {
        tAc = pv[roffU + offA];
        tBc = pv[roffU + offB];
    }
    hv[g0 & 1][w][0][0][lane] = AC[0];
    hv[g0 & 1][w][0][1][lane] = BC[0];
    hv[g0 & 1][w][1][0][lane] = AC[OWN - 1];
    hv[g0 & 1][w][1][1][lane] = BC[OWN - 1];
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // coarse plane pz from the residual planes 2pz-1, 2pz, 2pz+1 = (m, 0, p) and the next wave's first row (LDS ring)
    auto form_coarse = [&](int pz) __attribute__((always_inline)) {
        const int gm = 2 * pz - 1;
        real sa[OWN + 1], sb[OWN + 1], sc[OWN + 1];
#pragma unroll
        for (int o = 0; o < OWN; o++) {
            const real lm = wave_from_prev_lane<real>(rBm[o]), l0 = wave_from_prev_lane<real>(rB0[o]),
                       lp = wave_from_prev_lane<real>(rBp[o]);
            sa[o] = rA0[o];
            sb[o] = ((rAp[o] + rB0[o]) + rAm[o]) + l0;  // (N + E + S + O): (x,z+1), (x+1,z), (x,z-1), (x-1,z)
            sc[o] = ((rBp[o] + rBm[o]) + lm) + lp;      // (NE + SE + SO + NO)
        }
        {   // the row below my four: the first row of the next wave
            const int lm1 = lane > 0 ? lane - 1 : 0;
            const real eAm = hr[gm & 3][wD][0][lane], eBm = hr[gm & 3][wD][1][lane], elm = hr[gm & 3][wD][1][lm1];
            const real eA0 = hr[(gm + 1) & 3][wD][0][lane], eB0 = hr[(gm + 1) & 3][wD][1][lane], el0 = hr[(gm + 1) & 3][wD][1][lm1];
            const real eAp = hr[(gm + 2) & 3][wD][0][lane], eBp = hr[(gm + 2) & 3][wD][1][lane], elp = hr[(gm + 2) & 3][wD][1][lm1];
            sa[OWN] = eA0;
            sb[OWN] = ((eAp + eB0) + eAm) + el0;
            sc[OWN] = ((eBp + eBm) + elm) + elp;
        }
        if (produces) {
#pragma unroll
            for (int c = 0; c < OWN / 2; c++) {
                const int py = cyb + c;
                if (py <= cy - 2) {
                    const int rn = 2 * c, rc = 2 * c + 1, rs = 2 * c + 2;
                    coarse[gc.row(py, pz - czoff) + gc.pos(i)] =
                        (1 / 8.0f) * (sa[rc]) + (1 / 16.0f) * (sb[rc] + (sa[rn] + sa[rs])) +
                        (1 / 32.0f) * ((sc[rc] + sb[rn]) + sb[rs]) + (1 / 64.0f) * (sc[rn] + sc[rs]);
                }
            }
        }
    };

    for (int g = g0; g <= glast; g++) {
        const bool more = g < glast;
        if (more) {  // requests for the next step: v of plane g+2, f of plane g+1, the row above at plane g+1
#pragma unroll
            for (int o = 0; o < OWN; o++) {
                if (o < nv) {
                    AX[o] = pv[roff[o] + 2 * PL + offA];
                    BX[o] = pv[roff[o] + 2 * PL + offB];
                }
                if (o < nf) {
                    fAX[o] = pf[roff[o] + PL + offA];
                    fBX[o] = pf[roff[o] + PL + offB];
                }
            }
            if (w == 0) {
                tAx = pv[roffU + PL + offA];
                tBx = pv[roffU + PL + offB];
            }
            const int s1 = (g + 1) & 1;  // edge rows of plane g+1 for the neighbours' next step
            hv[s1][w][0][0][lane] = AN[0];
            hv[s1][w][0][1][lane] = BN[0];
            hv[s1][w][1][0][lane] = AN[OWN - 1];
            hv[s1][w][1][1][lane] = BN[OWN - 1];
        }
        if (!(g & 1) && g >= 2 * pz0 + 2) form_coarse(g / 2 - 1);  // its three residual planes are g-3, g-2, g-1
        // neighbours' edge rows of plane g
        const int s0 = g & 1;
        const real upA = w > 0 ? hv[s0][wU][1][0][lane] : tAc, upB = w > 0 ? hv[s0][wU][1][1][lane] : tBc;
        const real dnA = hv[s0][wD][0][0][lane], dnB = hv[s0][wD][0][1][lane];
        real rAn[OWN], rBn[OWN];
#pragma unroll
        for (int o = 0; o < OWN; o++) {
            const real Bl = wave_from_prev_lane<real>(BC[o]);  // v(2i-1): odd entry of lane i-1
            const real Ar = wave_from_next_lane<real>(AC[o]);  // v(2i+2): even entry of lane i+1
            const real An = o == 0 ? upA : AC[o > 0 ? o - 1 : 0], As = o == OWN - 1 ? dnA : AC[o < OWN - 1 ? o + 1 : o];
            const real Bn = o == 0 ? upB : BC[o > 0 ? o - 1 : 0], Bs = o == OWN - 1 ? dnB : BC[o < OWN - 1 ? o + 1 : o];
            const real a = residual3d_point<real, MODE>(Bl, BC[o], An, As, AP[o], AN[o], AC[o], fA[o], hx2, hy2, hz2);
            const real b = residual3d_point<real, MODE>(AC[o], Ar, Bn, Bs, BP[o], BN[o], BC[o], fB[o], hx2, hy2, hz2);
            rAn[o] = (yin[o] && xinA && lane > 0) ? a : (real)0;
            rBn[o] = (yin[o] && validB) ? b : (real)0;
        }
        hr[g & 3][w][0][lane] = rAn[0];
        hr[g & 3][w][1][lane] = rBn[0];
#pragma unroll
        for (int o = 0; o < OWN; o++) {
            rAm[o] = rA0[o]; rBm[o] = rB0[o];
            rA0[o] = rAp[o]; rB0[o] = rBp[o];
            rAp[o] = rAn[o]; rBp[o] = rBn[o];
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this step's requests have had the whole step
#pragma unroll
        for (int o = 0; o < OWN; o++) {
            AP[o] = AC[o]; BP[o] = BC[o];
            AC[o] = AN[o]; BC[o] = BN[o];
            AN[o] = AX[o]; BN[o] = BX[o];
            fA[o] = fAX[o]; fB[o] = fBX[o];
        }
        tAc = tAx;
        tBc = tBx;
        pv += PL;
        pf += PL;
    }
    form_coarse(pz1 - 1);  // the last coarse plane of the run (its third residual plane was the last step)
}

// =========================================================================== host side
// ---- residual+restrict: rr_plan decides how a launch over a run of coarse planes goes; rr_launch launches the window, shuffle
// and pipelined kernels, relax_rr3d_xs_launch (mgx_relax_rr3d.hip) the fused black one

// The launch over `planes` coarse planes of a level of n fine points (cn coarse): the fused black kernel, the window kernel (the
// natural layout, or residual_restrict3d.stream = 0) or the x-split kernel of residual_restrict3d.stream.  Returns false when
// there is nothing to launch: the x-split kernels on a level of fewer than 3 coarse points across x or y.
bool rr_plan(const mgx_ctx* ctx, bool xsplit, bool black, const int n[3], const int cn[3], int planes, RRPlan& p) {
    p = RRPlan();
    // runs of 8 coarse planes (residual_restrict3d.pzchunk), halved while the launch has fewer than four workgroups per CU
    const auto halved_runs = [&](long long tiles) {
        int pzc = ctx->rr_pzchunk > 0 ? ctx->rr_pzchunk : 8;
        while (pzc > 1 && tiles * ceil_div(planes, pzc) < 4LL * ctx->num_cus) pzc >>= 1;
        return pzc;
    };
    // rr_stream 3 (default): the pipelined kernel on levels of at least 129 x 65 rows and 8 coarse planes (with two rows per
    // wave it wins from 129^3 on: 18 against 25 us there, 75 against 97 us at 257^3; at 65^3 the streaming kernel's 6 us stand)
    const bool big = n[0] >= 129 && n[1] >= 65 && planes >= 8;
    p.kernel = black ? RRKernel::Black : !xsplit || !ctx->rr_stream ? RRKernel::Window
             : ctx->rr_stream == 2 || (ctx->rr_stream == 3 && big) ? RRKernel::Pipe : RRKernel::Shuffle;
    if (p.kernel == RRKernel::Window) {  // tiles of 32 x 8 coarse points (one extra fine plane per run)
        p.gx = ceil_div(cn[0], 32), p.gy = ceil_div(cn[1], 8);
        p.pzchunk = halved_runs((long long)p.gx * p.gy);
        p.grid = dim3(p.gx, p.gy, ceil_div(planes, p.pzchunk));
        p.block = blk();
        return true;
    }
    if (cn[0] < 3 || cn[1] < 3) return false;
    // XCD-aware tile order (residual_restrict3d.xcd): 1 = the pipelined and the fused kernel, 2 = the shuffle kernel too
    if (p.kernel == RRKernel::Black) {
        p.T = ctx->rr_black_waves == 12 ? 12 : ctx->rr_black_waves == 8 ? 8 : 16;
        p.gx = ceil_div(cn[0] - 2, 61);
        p.gy = ceil_div(cn[1] - 2, p.T - 2);
        // all workgroups take the same time and one fits a CU (two of 8 waves): the fewest runs that fill whole rounds to 90 %, runs
        // of at least 8 coarse planes (the two planes a run relaxes before its first residual)
        const int tiles = p.gx * p.gy;
        p.pzchunk = ctx->rr_pzchunk > 0 ? ctx->rr_pzchunk
                                        : ceil_div(planes, runs_filling_rounds(tiles, planes, (long long)ctx->num_cus * (p.T == 8 ? 2 : 1), 16, 8, 2));
        p.xcd = ctx->rr_xcd >= 1;
    } else if (p.kernel == RRKernel::Pipe) {
        // fine rows per wave: 2 (sixteen waves of <= 128 VGPRs per workgroup; 513^3: 474-486 us against 562-569 us with 4
        // rows = eight waves of 240 VGPRs; 1025^3: 3.49 against 3.76 ms -- once the runs fill whole rounds, see below)
        p.OWN = ctx->rr_rows ? ctx->rr_rows : 2;
        // two rows per wave: sixteen waves per workgroup, eight on levels of at most 257 rows (more tiles, so longer runs:
        // 69 against 76 us at 257^3)
        const bool by_level = ctx->rr_stream == 3;
        p.T = p.OWN == 2 ? ((by_level ? n[1] <= 257 : ctx->rr_tyw == 8) ? 8 : 16) : (by_level ? 8 : ctx->rr_tyw);
        p.gx = ceil_div(cn[0] - 2, 62);
        p.gy = ceil_div(cn[1] - 2, (p.OWN / 2) * (p.T - 1));  // the last wave is a halo wave
        const int tiles = p.gx * p.gy;
        // whole resident rounds of workgroups, because all workgroups take the same time: three rounds for the 8-wave
        // kernels; ONE for the 16-wave kernel (one workgroup per CU: 513^3 = 85 tiles x 3 runs of 85 coarse planes -- the
        // three planes a run loads before its first result then weigh 2 % instead of 5 %: 512 against 540 us)
        // T == 16: the fewest runs that fill whole rounds to 90 % (1025^3: 315 tiles x 3 = 945 of 1024 slots)
        const int runs = p.T == 16 ? runs_filling_rounds(tiles, planes, ctx->num_cus, 12, 0, 0) : max(1, (3 * ctx->num_cus + tiles / 2) / tiles);
        p.pzchunk = ctx->rr_pzchunk > 0 ? ctx->rr_pzchunk : max(4, ceil_div(planes, runs));
        p.xcd = ctx->rr_xcd >= 1;
    } else {
        // one coarse row per lane on the launch-bound levels (<= 65^3: 3-4 us faster, more waves), two above
        p.CR = ctx->rr_cr == 1 || (ctx->rr_cr == 0 && n[0] <= 65) ? 1 : 2;
        p.T = ctx->rr_tyw;
        p.gx = ceil_div(cn[0], 63);
        p.gy = ceil_div(cn[1] - 2, p.CR * p.T);
        p.pzchunk = halved_runs((long long)p.gx * p.gy);
        p.xcd = ctx->rr_xcd >= 2;
    }
    p.grid = dim3(p.gx * p.gy * ceil_div(planes, p.pzchunk), 1, 1);
    p.block = dim3(64, p.T, 1);
    return true;
}

// The one launch of the window, shuffle and pipelined kernels: the instantiation for the plan's shape and the MODE of s (the
// window kernel ignores rcp: MODE 0 / 1 with the squared spacings).  The coarse planes [pzbeg, pzend) are global; v / f start
// at global fine plane fzoff, coarse at global coarse plane czoff.  Returns false when no instantiation has the plan's shape.
template <class real, class L>
static bool rr_launch(mgx_ctx* ctx, const RRPlan& p, const ResidualScale<real>& s, const real* v, const real* f, const int n[3],
                      real* coarse, const int cn[3], int fzoff, int czoff, int pzbeg, int pzend) {
    const bool window = p.kernel == RRKernel::Window;
    bool done = false;
    with_value<0, 1, 2, 3>(window ? s.mode & 1 : s.mode, [&](auto m) {
        constexpr int M = decltype(m)::value;
        if (window) {
            if constexpr (M < 2) {
                MGX_LAUNCH((residual_restrict3d_kernel<real, L, M, 32, 8>), p.grid, p.block, 0, ctx->compute, v, f, n[0], n[1], n[2], s.hx2,
                           s.hy2, s.hz2, coarse, cn[0], cn[1], cn[2], p.pzchunk, fzoff, czoff, pzbeg, pzend);
                done = true;
            }
        } else if (p.kernel == RRKernel::Shuffle) {
            with_value<1, 2>(p.CR, [&](auto cr) {
                with_value<8, 2, 4>(p.T, [&](auto tyw) {
                    MGX_LAUNCH((residual_restrict3d_xs_kernel<real, M, decltype(cr)::value, decltype(tyw)::value>), p.grid, p.block, 0,
                               ctx->compute, v, f, n[0], n[1], n[2], s.qx, s.qy, s.qz, coarse, cn[0], cn[1], cn[2], p.pzchunk, fzoff,
                               czoff, pzbeg, pzend, p.gx, p.gy, p.xcd);
                    done = true;
                });
            });
        } else {  // the pipelined shapes: 16 waves of 2 rows, 8 of 2 or 4, 2 and 4 waves of 4 rows
            with_value<16, 8, 2, 4>(p.T, [&](auto tyw) {
                with_value<2, 4>(p.OWN, [&](auto own) {
                    constexpr int W = decltype(tyw)::value, OW = decltype(own)::value;
                    if constexpr (W == 8 || (W == 16) == (OW == 2)) {
                        MGX_LAUNCH((residual_restrict3d_xs_pipe_kernel<real, M, W, OW>), p.grid, p.block, 0, ctx->compute, v, f, n[0],
                                   n[1], n[2], s.qx, s.qy, s.qz, coarse, cn[0], cn[1], cn[2], p.pzchunk, fzoff, czoff, pzbeg, pzend, p.gx,
                                   p.gy, p.xcd);
                        done = true;
                    }
                });
            });
        }
    });
    return done;
}

// Residual+restrict into the GLOBAL coarse planes [pzbeg, pzend) (the whole grid: fzoff = czoff = pzbeg = 0, pzend = cn[2]).
// n / cn global sizes, v / f start at global fine plane fzoff, coarse_f at global coarse plane czoff.
template <class real, class L>
static int residual_restrict3d_range(mgx_ctx* ctx, const real* v, const real* f, const int n[3], int fzoff, const real h[3], int mode,
                                     real* coarse_f, const int cn[3], int czoff, int pzbeg, int pzend, bool rim_is_zero) {
    if (pzbeg == pzend) return MGX_OK;
    RRPlan p;
    const bool launch = rr_plan(ctx, L::xsplit, false, n, cn, pzend - pzbeg, p);
    // the x-split kernels write every interior coarse point of the planes and nothing else: boundary points and pad entries
    // are zeroed here unless the caller vouches that they already are (they stay zero from one cycle to the next)
    const Geo<XSplit, real> gc(cn[0], cn[1]);
    if (p.kernel != RRKernel::Window && !rim_is_zero)
        MGX_TRY_RET(fill_zero(ctx, coarse_f + gc.PL * (size_t)(pzbeg - czoff), gc.PL * (size_t)(pzend - pzbeg) * sizeof(real)));
    MGX_REQUIRE((!launch || rr_launch<real, L>(ctx, p, residual_scale<real>(ctx, h, mode), v, f, n, coarse_f, cn, fzoff, czoff, pzbeg, pzend)),
                MGX_ERR_INVALID, "residual_restrict: no kernel of the planned shape (T %d, CR %d, OWN %d)", p.T, p.CR, p.OWN);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

template <class real, class L>
int residual_restrict3d(mgx_ctx* ctx, const real* v, const real* f, const int n[3], const real h[3], int mode,
                        real* coarse_f, const int cn[3], bool rim_is_zero) {
    MGX_TRY_RET(check_rr_args(ctx, ctx && v && f && h && coarse_f, n, cn, "residual_restrict3d"));
    MGX_REQUIRE(mode == MGX_RESIDUAL_REF_COMPAT || mode == MGX_RESIDUAL_CORRECT, MGX_ERR_INVALID,
                "residual_restrict3d: bad mode %d", mode);
    return residual_restrict3d_range<real, L>(ctx, v, f, n, 0, h, mode, coarse_f, cn, 0, 0, cn[2], rim_is_zero);
}

template <class real>
int residual_restrict3d_slab(mgx_ctx* ctx, const real* v, const real* f, const int n[3], int fzoff, const real h[3],
                             int mode, real* coarse_f, const int cn[3], int czoff, int pzbeg, int pzend) {
    MGX_TRY_RET(check_rr_args(ctx, ctx && v && f && h && coarse_f, n, cn, "residual_restrict_slab"));
    MGX_REQUIRE(mode == MGX_RESIDUAL_REF_COMPAT || mode == MGX_RESIDUAL_CORRECT, MGX_ERR_INVALID, "bad residual mode %d", mode);
    MGX_REQUIRE(pzbeg >= 0 && pzend <= cn[2] && pzbeg <= pzend && fzoff >= 0 && czoff >= 0 && czoff <= pzbeg, MGX_ERR_INVALID,
                "residual_restrict_slab: bad plane range");
    return residual_restrict3d_range<real, XSplit>(ctx, v, f, n, fzoff, h, mode, coarse_f, cn, czoff, pzbeg, pzend, false);
}

#define MGX_X(real, L) \
    template int residual_restrict3d<real, L>(mgx_ctx*, const real*, const real*, const int[3], const real[3], int, real*, const int[3], bool);
MGX_X(float, Natural) MGX_X(double, Natural) MGX_X(float, XSplit) MGX_X(double, XSplit)
#undef MGX_X

}  // namespace mgx

#define MGX_DEFINE_OPS3D(PFX, L, SFX, real)                                                                      \
    int PFX##residual_restrict_##SFX(mgx_ctx* ctx, const real* v, const real* f, const int n[3], const real h[3], \
                                     int mode, real* coarse_f, const int cn[3]) {                                \
        return mgx::residual_restrict3d<real, L>(ctx, v, f, n, h, mode, coarse_f, cn);                           \
    }                                                                                                            \
    int PFX##residual_restrict_keep_rim_##SFX(mgx_ctx* ctx, const real* v, const real* f, const int n[3],        \
                                              const real h[3], int mode, real* coarse_f, const int cn[3]) {      \
        return mgx::residual_restrict3d<real, L>(ctx, v, f, n, h, mode, coarse_f, cn, true);                     \
    }

#define MGX_DEFINE_MISC3D(SFX, real)                                                                             \
    int mgx3dxs_residual_restrict_slab_##SFX(mgx_ctx* ctx, const real* v, const real* f, const int n[3],         \
                                             int fzoff, const real h[3], int mode, real* coarse_f,               \
                                             const int cn[3], int czoff, int pzbeg, int pzend) {                 \
        return mgx::residual_restrict3d_slab<real>(ctx, v, f, n, fzoff, h, mode, coarse_f, cn, czoff, pzbeg,     \
                                                   pzend);                                                       \
    }

extern "C" {
MGX_DEFINE_OPS3D(mgx3d_, mgx::Natural, f32, float)
MGX_DEFINE_OPS3D(mgx3d_, mgx::Natural, f64, double)
MGX_DEFINE_OPS3D(mgx3dxs_, mgx::XSplit, f32, float)
MGX_DEFINE_OPS3D(mgx3dxs_, mgx::XSplit, f64, double)
MGX_DEFINE_MISC3D(f32, float)
MGX_DEFINE_MISC3D(f64, double)
}
