// mgx_block3d.hip -- three colour passes X, Y, X of MultiGrid3D::Relax in ONE launch (x-split layout, fp64, HBM-bound levels).
//
// A colour pass overwrites every point of its colour from the other colour's values and f only; the old values of its own
// colour are never read.  So the three passes X, Y, X need colour Y's old values and f, nothing else: the launch reads Y from
// `vin` and f, and writes the final X (and, with STORE_BOTH, the Y of the middle pass) into `vout`.  Where the launch stores
// only X it may run in place (vin == vout): no workgroup ever reads an X value from memory, except the entries on a face of
// the grid, which no pass writes.  That is the argument that makes relax_rr3d_xs_kernel race-free.
//
// On the way down (smooth_residual_restrict3d_xs) the last three passes before relax_rr3d_xs_kernel are R, B, R.  The B values
// of the middle pass are overwritten by the rr kernel's own black pass, which reads only red: the launch stores red only and
// streams black 0.5 + f 1.0 + red 0.5 = 2.0 words per point instead of the 4.5 of three plain passes.
//
// On the way up (interpolate_correct_relax3d_xs with a partner array) the passes after the correcting red pass R' are B, R, B.
// R' stores red into the partner; the launch reads red and the faces from there and stores both colours into v: red 0.5 + f 1.0
// in, 1.0 out = 2.5 words per point.  Storing Y cannot be done in place: a neighbouring tile still reads the old Y as halo.
//
// A workgroup marches its (x, y) tile through a run of z-planes with the three stages lagged one plane each:
//
//   iteration t:   stage 1   X at plane t       from Y (loaded) of planes t - 1, t, t + 1 and f
//                  stage 2   Y at plane t - 1   from the stage-1 X of planes t - 2, t - 1, t and f
//                  stage 3   X at plane t - 2   from the stage-2 Y of planes t - 3, t - 2, t - 1 and f  -> stored
//
// Tile edges are recomputed, not exchanged: Y is loaded three deep around the tile, stage 1 is right two deep, stage 2 one
// deep, stage 3 on the tile.  A wave owns two rows and 64 x-pairs; lanes 0, 1, 62, 63 and the first three and last three rows
// of a workgroup are halo (60 pairs x (2 TW - 6) rows per tile).  A run of planes starts three planes early for the same
// reason.  Every value is computed from exactly the inputs of the separate passes with relax3d_point: bit-identical results.
//
// Rows of neighbouring waves go through LDS: every iteration publishes the first and last row of the Y of plane t + 1 (loaded
// one iteration earlier), of the stage-1 X and of the stage-2 Y, and reads those of the previous iteration -- ONE barrier per
// iteration, double-buffered.  Loads requested at the top of an iteration are waited for behind its barrier; the stores of the
// previous iteration's results go out at the top too.
//
// A run is head, steady state and tail.  The general iteration clamps every plane it addresses into the array, derives the range
// predicates of its stores and selects from t and builds its descriptors from scratch; it runs the iterations before the first
// store and those within three planes (CORR: six) of the far z-face.  In between, where none of that can bite, the steady iteration
// runs in pairs: the bases of the planes of vin, f, vout and coarse are kept as 64-bit scalars and advanced by the plane pitch, the
// range predicates are literals, and the lane masks of stores and selects, which do not depend on t, are formed once before the
// loop.  A third of the general iteration's scalar instructions, the same vector instructions.
//
// CORR (way up, in place, COL = 0, red stored only): the launch stands for R', B, R -- the first red pass reads black THROUGH
// the coarse-grid correction, as relax3d_xs_pipe_kernel<.., VAR = 2> does.  Every black value that arrives gets
// e = Interpolate(coarse)(x, y, z) added if it is an interior point of the grid, once, before it is published to sY; stages 2
// and 3 do not change.  The black values in memory stay uncorrected, which the plain black pass after the launch does not
// see: it rewrites every black interior point from red and f.  A wave's rows y (odd) and y + 1 lie on the coarse rows
// cr = y >> 1 and cr + 1, its lane's pair on coarse column p; column p + 1 is the next lane's (lane 63's odd entries, the only
// ones that have no next lane, are never read).  So the wave keeps those two rows of coarse planes K and K + 1 in registers
// (K = (t + 2) >> 1 for the plane t + 2 that arrives in iteration t), four values per lane, and asks for the rows of plane
// K + 2 every other iteration with the iteration's LAST two loads, which its wait leaves outstanding: they have until the end
// of the next iteration.  (`coarse` is deliberately not __restrict__: with it the compiler sinks those loads past the barrier
// into the next iteration, in front of that iteration's own requests.)
#include <type_traits>

#include "mgx_host3d.hpp"

namespace mgx {

template <class real, int COL, bool STORE_BOTH, int TW, bool CORR = false>
__global__ void __launch_bounds__(64 * TW, 4)  // four waves per SIMD: 128 VGPRs, one workgroup per CU
    relax3d_xs_block3_kernel(const real* vin, real* vout, const real* __restrict__ f, int sx, int sy, int sz, real hx2, real hy2,
                             real hz2, int zrun, int gx, int gy, int xcd_mode, const real* coarse = nullptr, int cx = 0,
                             int cy = 0) {
    constexpr int ROWS = 2 * TW, OUTR = ROWS - 6;  // rows of a tile, of which the middle OUTR are stored
    static_assert(OUTR % 2 == 0, "the colour parity of a wave's rows must not depend on the tile");
    static_assert(!CORR || (COL == 0 && !STORE_BOTH), "the correcting variant is R', B, R with red stored");
    __shared__ real sY[2][TW][2][64];  // [iteration & 1][wave][first / last row][lane]: loaded Y of plane t + 1
    __shared__ real sX[2][TW][2][64];  // stage-1 X of plane t
    __shared__ real sZ[2][TW][2][64];  // stage-2 Y of plane t - 1
    const Geo<XSplit, real> g(sx, sy);
    const int lane = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.y);
    int bx, by, bz;
    tile_of_block(xcd_mode, gx, gy, bx, by, bz);
    const int z0 = 1 + bz * zrun, z1 = min(z0 + zrun, sz - 1);  // planes [z0, z1) are this run's
    if (z0 >= z1) return;  // uniform over the workgroup
    const int PL = (int)g.PL;

    const int Hn = (sx + 1) >> 1;  // x-pairs of a row (the last one has its even entry only)
    const int pn = bx * 60 + lane - 2, p = min(max(pn, 0), Hn - 1);
    const unsigned off0 = (unsigned)p * (unsigned)sizeof(real), off1 = (unsigned)(g.H + (p <= Hn - 2 ? p : 0)) * (unsigned)sizeof(real);
    const bool xin0 = pn >= 1 && 2 * pn <= sx - 2, xin1 = pn >= 0 && 2 * pn + 1 <= sx - 2;  // 1 <= x <= sx - 2
    auto off = [&](int h) { return h ? off1 : off0; };  // byte offset of the lane's entry in half h (selects: no indexed arrays)
    auto xin = [&](int h) { return h ? xin1 : xin0; };
    const bool xface0 = pn <= 0 || pn >= Hn - 1;  // the even entry lies on (or beyond) an x-face
    const bool wxface = bx * 60 - 2 <= 0 || bx * 60 + 61 >= Hn - 1;  // some lane of the wave holds one (wave-uniform)
    const bool outlane = lane >= 2 && lane <= 61;
    int roff[2];
    bool yin[2], outrow[2];
#pragma unroll
    for (int o = 0; o < 2; o++) {
        const int y = by * OUTR - 3 + 2 * w + o;
        roff[o] = min(max(y, 0), sy - 1) * g.P;
        yin[o] = y >= 1 && y <= sy - 2;
        outrow[o] = 2 * w + o >= 3 && 2 * w + o < ROWS - 3;
    }
    // none of these depends on the plane: the lanes that store row o's entry of half h, the lanes whose entry there is an
    // interior point in x and y, the lanes whose even X entry is v on an x-face -- formed once, reused by every iteration
    bool stm[2][2], sel[2][2];
#pragma unroll
    for (int o = 0; o < 2; o++)
#pragma unroll
        for (int h = 0; h < 2; h++) {
            sel[o][h] = yin[o] && xin(h);
            stm[o][h] = outlane && outrow[o] && sel[o][h];
        }
    const bool xfm = wxface && xface0;
    const int wU = w > 0 ? w - 1 : 0, wD = w < TW - 1 ? w + 1 : TW - 1;
    auto zc = [&](int z) { return min(max(z, 0), sz - 1); };
    auto plane = [&](const real* a, int z) { return plane_rsrc<real>(a + (ptrdiff_t)zc(z) * (ptrdiff_t)g.PL, PL, 1); };
    // CORR: the coarse rows cr, cr + 1 under the wave's rows (row 0 is odd: y = 2 cr + 1), the lane's coarse column p, coarse plane k
    // (all clamped into the array: what a clamped request brings is only ever added to values that are no interior points)
    const Geo<XSplit, real> gc(CORR ? cx : 3, CORR ? cy : 3);
    const int cz = (sz + 1) >> 1;
    int croff[2];
#pragma unroll
    for (int i = 0; i < 2; i++) croff[i] = CORR ? min(max(by * (OUTR / 2) - 2 + w + i, 0), cy - 1) * gc.P : 0;
    const unsigned coff = (unsigned)XSplit::pos(p, gc.H) * (unsigned)sizeof(real);
    auto cplane = [&](int k) {
        return plane_rsrc<real>(coarse + (ptrdiff_t)min(max(k, 0), cz - 1) * (ptrdiff_t)gc.PL, (int)gc.PL, 1);
    };
    // e of the lane's black entry of row o (x parity ox, z parity oz) from the rows of coarse planes z >> 1 (k0) and (z >> 1) + 1 (k1)
    auto interp = [&](int ox, int oz, int o, const real (&k0)[2], const real (&k1)[2]) __attribute__((always_inline)) {
        return interpolate3d_point<real>(ox, 1 - o, oz, [&](int dx, int dy, int dz) __attribute__((always_inline)) {
            const real c = o + dy ? (dz ? k1[1] : k0[1]) : (dz ? k1[0] : k0[0]);  // row 1 is even: dy = 0
            return dx ? wave_from_next_lane<real>(c) : c;
        });
    };

    // per row: loaded Y of planes t-1, t, t+1, t+2 (in flight); f (or v on a face of the grid) of X at planes t, t-1, t-2, t+1 (in
    // flight, v of a y- / z-face); v of the even X entry at plane t+1 (in flight, x-face lanes: replaces f once it has arrived); f of Y at planes t-1, t (in flight); stage-1 X at t, t-1,
    // t-2; stage-2 Y at t-1, t-2, t-3; stage-3 X of plane t-2, stored in the next iteration
    real a_m[2], a_c[2], a_p[2], a_n[2], fx_c[2], fx_1[2], fx_2[2], fx_n[2], xv_n[2], fy_c[2], fy_n[2];
    real b_c[2], b_m[2], b_mm[2], d_c[2], d_m[2], d_mm[2], x3[2];
    // CORR: rows cr, cr + 1 of coarse planes K, K + 1, K + 2 (in flight); the correction of a_n
    real c_0[2], c_1[2], c_n[2], e_n[2];
#pragma unroll
    for (int o = 0; o < 2; o++)
        a_m[o] = a_c[o] = a_p[o] = a_n[o] = fx_c[o] = fx_1[o] = fx_2[o] = fx_n[o] = xv_n[o] = fy_c[o] = fy_n[o] = b_c[o] =
            b_m[o] = b_mm[o] = d_c[o] = d_m[o] = d_mm[o] = x3[o] = c_0[o] = c_1[o] = c_n[o] = e_n[o] = 0;

    const int t0 = z0 - 2, tlast = z1 + 1;
    // ---- set-up: Y of planes t0 - 1 .. t0 + 1, f / v of X at t0; the rows of Y at t0 published as if by iteration t0 - 1
    {
        const auto qm = plane(vin, t0 - 1), q0 = plane(vin, t0), qp = plane(vin, t0 + 1);
        const bool zf = t0 <= 0 || t0 >= sz - 1;
        const auto qf = plane(f, t0);
#pragma unroll
        for (int o = 0; o < 2; o++) {
            const int hx = (COL + 1 + o + t0) & 1;  // X half of row o at plane t0
            a_m[o] = buf_load<real>(qm, off(hx), roff[o]);
            a_c[o] = buf_load<real>(q0, off(hx ^ 1), roff[o]);
            a_p[o] = buf_load<real>(qp, off(hx), roff[o]);
            fx_c[o] = buf_load<real>(zf || !yin[o] ? q0 : qf, off(hx), roff[o]);
            if (wxface) xv_n[o] = buf_load<real>(q0, off(0), roff[o]);
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
#pragma unroll
        for (int o = 0; o < 2; o++)
            if (wxface && ((COL + 1 + o + t0) & 1) == 0 && xface0) fx_c[o] = xv_n[o];
        if constexpr (CORR) {
#pragma unroll
            for (int d = -1; d <= 1; d++) {
                const int z = t0 + d;
                const auto k0q = cplane(z >> 1), k1q = cplane((z >> 1) + 1);
                real k0[2], k1[2];
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    k0[i] = buf_load<real>(k0q, coff, croff[i]);
                    k1[i] = buf_load<real>(k1q, coff, croff[i]);
                }
                const bool zin = z >= 1 && z <= sz - 2;
#pragma unroll
                for (int o = 0; o < 2; o++) {
                    const int hb = (COL + o + z) & 1;  // the black half of row o at plane z
                    const real e = interp(hb, z & 1, o, k0, k1);
                    real& a = d < 0 ? a_m[o] : d == 0 ? a_c[o] : a_p[o];
                    if (zin && yin[o] && xin(hb)) a = a + e;
                }
            }
            // iteration t corrects plane t + 2 from coarse planes K = (t + 2) >> 1 and K + 1; an odd one ends by taking in K + 2
            const int K = (t0 + 2) >> 1;
            const auto q0c = cplane(K), q1c = cplane(K + 1), qnc = cplane(K + 2);
#pragma unroll
            for (int i = 0; i < 2; i++) {
                c_0[i] = buf_load<real>(q0c, coff, croff[i]);
                c_1[i] = buf_load<real>(q1c, coff, croff[i]);
                c_n[i] = buf_load<real>(qnc, coff, croff[i]);
            }
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
        }
        const int b = (t0 - 1) & 1;
        sY[b][w][0][lane] = a_c[0];
        sY[b][w][1][lane] = a_c[1];
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }

    // one relaxed point at half h of row o (stage with in-plane values `c` of the other colour, rows above / below through LDS)
    auto relax = [&](auto hc, int o, const real (&c)[2], real nb, real sb, real D, real U, real fv) __attribute__((always_inline)) {
        constexpr int h = decltype(hc)::value;
        real O, E;
        if (h == 0) {
            O = wave_from_prev_lane<real>(c[o]);
            E = c[o];
        } else {
            O = c[o];
            E = wave_from_next_lane<real>(c[o]);
        }
        const real N = o == 0 ? nb : c[0], S = o == 1 ? sb : c[1];
        return relax3d_point<real>(O, E, N, S, D, U, fv, hx2, hy2, hz2);
    };

    // the planes an iteration t addresses, as base pointers: vout at t - 3 and t - 2, vin at t + 2 and t + 1, f at t + 1 and t,
    // the coarse plane t / 2 + 3 (CORR, even t)
    struct Streams {
        real *o3, *o2;
        const real *y, *xv, *fx, *fy, *kc;
    };
    auto streams_at = [&](int t) {  // any iteration: every plane clamped into its array
        const ptrdiff_t pl = (ptrdiff_t)g.PL;
        return Streams{vout + (ptrdiff_t)zc(t - 3) * pl, vout + (ptrdiff_t)zc(t - 2) * pl, vin + (ptrdiff_t)zc(t + 2) * pl,
                       vin + (ptrdiff_t)zc(t + 1) * pl, f + (ptrdiff_t)zc(t + 1) * pl, f + (ptrdiff_t)zc(t) * pl,
                       CORR ? coarse + (ptrdiff_t)min(max((t >> 1) + 3, 0), cz - 1) * (ptrdiff_t)gc.PL : nullptr};
    };
    auto rsrc = [&](const real* a) { return plane_rsrc<real>(a, PL, 1); };

    // STEADY: the caller guarantees z0 + 3 <= t <= min(tlast, sz - 3) (CORR: sz - 6) -- every store is in its run, no plane of the iteration
    // is a z-face or clamped, and S holds the planes' bases as the caller advanced them: no range logic, no address arithmetic
    auto iteration = [&](auto parity, auto steady, int t, const Streams& S) __attribute__((always_inline)) {
        constexpr int PAR = decltype(parity)::value;  // t & 1
        constexpr int PB = PAR ^ 1;                  // LDS buffer written by the previous iteration
        constexpr bool STEADY = decltype(steady)::value;
        // ---- stores of the previous iteration's results: X of plane t - 3, Y of plane t - 2 (both in half hx ^ 1)
        const auto ro3 = rsrc(S.o3), ro2 = rsrc(S.o2);
        // ---- requests: Y of plane t + 2, f (v on a face) of X at t + 1, f of Y at t
        const auto rY = rsrc(S.y), rXv = rsrc(S.xv), rFy = rsrc(S.fy);
        const bool zf = STEADY ? false : t + 1 <= 0 || t + 1 >= sz - 1;
        const bool st3 = STEADY ? true : t - 3 >= z0 && t - 3 < z1, st2 = STEADY ? true : t - 2 >= z0 && t - 2 < z1;
        __builtin_amdgcn_s_setprio(3);
#pragma unroll
        for (int o = 0; o < 2; o++) {
            const int hx = (COL + 1 + o + PAR) & 1;  // X half of row o at plane t (compile-time)
            if (st3 && stm[o][hx ^ 1]) buf_store_nt<real>(x3[o], ro3, off(hx ^ 1), roff[o]);
            if (STORE_BOTH && st2 && stm[o][hx ^ 1]) buf_store_nt<real>(d_m[o], ro2, off(hx ^ 1), roff[o]);
            a_n[o] = buf_load<real>(rY, off(hx ^ 1), roff[o]);
            fx_n[o] = buf_load<real>(rsrc(zf || !yin[o] ? S.xv : S.fx), off(hx ^ 1), roff[o]);
            if ((hx ^ 1) == 0 && wxface) xv_n[o] = buf_load<real>(rXv, off(0), roff[o]);
            fy_n[o] = buf_load<real>(rFy, off(hx ^ 1), roff[o]);
        }
        if constexpr (CORR && PAR == 0) {  // coarse plane K + 2 = t / 2 + 3: the last requests, still on their way at the iteration's end
            const auto qnc = plane_rsrc<real>(S.kc, (int)gc.PL, 1);
            __builtin_amdgcn_sched_barrier(0);  // (the scheduler would move them up in front of the others)
#pragma unroll
            for (int i = 0; i < 2; i++) c_n[i] = buf_load<real>(qnc, coff, croff[i]);
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_s_setprio(0);
        // ---- stage 1: X at plane t (half hx) from the loaded Y
        const bool zin1 = STEADY ? true : t >= 1 && t <= sz - 2, zin2 = STEADY ? true : t - 1 >= 1 && t - 1 <= sz - 2;
        {
            const real nb = sY[PB][wU][1][lane], sb = sY[PB][wD][0][lane];
#pragma unroll
            for (int o = 0; o < 2; o++) {
                const real v1 = (((COL + 1 + PAR) & 1) ^ o) == 0
                                    ? relax(std::integral_constant<int, 0>{}, o, a_c, nb, sb, a_m[o], a_p[o], fx_c[o])
                                    : relax(std::integral_constant<int, 1>{}, o, a_c, nb, sb, a_m[o], a_p[o], fx_c[o]);
                const int hx = (COL + 1 + o + PAR) & 1;
                b_c[o] = zin1 && sel[o][hx] ? v1 : fx_c[o];
            }
        }
        // ---- stage 2: Y at plane t - 1 (half hx) from the stage-1 X
        {
            const real nb = sX[PB][wU][1][lane], sb = sX[PB][wD][0][lane];
#pragma unroll
            for (int o = 0; o < 2; o++) {
                const real v2 = (((COL + 1 + PAR) & 1) ^ o) == 0
                                    ? relax(std::integral_constant<int, 0>{}, o, b_m, nb, sb, b_mm[o], b_c[o], fy_c[o])
                                    : relax(std::integral_constant<int, 1>{}, o, b_m, nb, sb, b_mm[o], b_c[o], fy_c[o]);
                const int hx = (COL + 1 + o + PAR) & 1;
                d_c[o] = zin2 && sel[o][hx] ? v2 : a_m[o];
            }
        }
        // ---- stage 3: X at plane t - 2 (half hx) from the stage-2 Y; stored in the next iteration
        {
            const real nb = sZ[PB][wU][1][lane], sb = sZ[PB][wD][0][lane];
#pragma unroll
            for (int o = 0; o < 2; o++) {
                x3[o] = (((COL + 1 + PAR) & 1) ^ o) == 0
                            ? relax(std::integral_constant<int, 0>{}, o, d_m, nb, sb, d_mm[o], d_c[o], fx_2[o])
                            : relax(std::integral_constant<int, 1>{}, o, d_m, nb, sb, d_mm[o], d_c[o], fx_2[o]);
                // formed here: with a store mask that no longer depends on t the compiler would sink the whole stage into the next
                // iteration's store, between its s_setprio(3) and its requests
                asm volatile("" : "+v"(x3[o]));
            }
        }
        // ---- CORR: the correction of the Y of plane t + 2, formed while that Y is on its way
        if constexpr (CORR) {
#pragma unroll
            for (int o = 0; o < 2; o++) e_n[o] = interp((COL + o + PAR) & 1, PAR, o, c_0, c_1);
        }
        // ---- publish: Y of plane t + 1, stage-1 X of plane t, stage-2 Y of plane t - 1 (first and last row)
#pragma unroll
        for (int o = 0; o < 2; o++) {
            sY[PAR][w][o][lane] = a_p[o];
            sX[PAR][w][o][lane] = b_c[o];
            sZ[PAR][w][o][lane] = d_c[o];
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if constexpr (CORR && PAR == 0) __builtin_amdgcn_s_waitcnt(0x0F72);  // vmcnt(2): all but the two coarse requests
        else __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this iteration's requests have had the whole iteration
        const bool zin3 = STEADY ? true : t + 2 >= 1 && t + 2 <= sz - 2;
#pragma unroll
        for (int o = 0; o < 2; o++) {
            a_m[o] = a_c[o]; a_c[o] = a_p[o];
            a_p[o] = CORR && zin3 && sel[o][(COL + o + PAR) & 1] ? a_n[o] + e_n[o] : a_n[o];
            if constexpr (CORR && PAR == 1) { c_0[o] = c_1[o]; c_1[o] = c_n[o]; }
            fx_2[o] = fx_1[o]; fx_1[o] = fx_c[o];
            fx_c[o] = ((COL + 1 + o + PAR) & 1) == 1 && xfm ? xv_n[o] : fx_n[o];  // x-face lanes: v of the even X entry
            fy_c[o] = fy_n[o];
            b_mm[o] = b_m[o]; b_m[o] = b_c[o];
            d_mm[o] = d_m[o]; d_m[o] = d_c[o];
        }
    };

    // head (the iterations before the first store, up to an even t), steady state (pairs of iterations with the planes'
    // bases advanced by the plane pitch), tail (from three planes -- CORR: six -- before the far z-face, or the odd last one).
    // The general iteration exists once per parity and serves head and tail; the steady one once per parity.
    const int ts0 = (z0 + 4) & ~1, ts1 = min(tlast, sz - (CORR ? 6 : 3));  // steady: ts0 <= t <= ts1, begun at an even t
    constexpr std::integral_constant<int, 0> even{};
    constexpr std::integral_constant<int, 1> odd{};
    int t = t0;
#pragma nounroll
    for (int phase = 0;; phase++) {
        const int gend = phase == 0 ? min(ts0, tlast + 1) : tlast + 1;
#pragma nounroll
        for (; t < gend; t++) {
            if (t & 1) iteration(odd, std::false_type{}, t, streams_at(t));
            else iteration(even, std::false_type{}, t, streams_at(t));
        }
        if (phase == 1 || t > tlast) break;
        if (t + 1 <= ts1) {
            const ptrdiff_t pl = (ptrdiff_t)g.PL;
            real* pO = vout + (ptrdiff_t)(t - 3) * pl;                                            // vout at t - 3
            const real *pYm = vin + (ptrdiff_t)(t + 1) * pl, *pY = pYm + pl;                      // vin at t + 1, t + 2
            const real *pFm = f + (ptrdiff_t)t * pl, *pF = pFm + pl;                              // f at t, t + 1
            const real* pK = CORR ? coarse + (ptrdiff_t)((t >> 1) + 3) * (ptrdiff_t)gc.PL : nullptr;  // coarse at t / 2 + 3
#pragma nounroll
            for (; t + 1 <= ts1; t += 2) {
                real* const pO1 = pO + pl;
                real* const pO2 = pO1 + pl;
                const real* const pYn = pY + pl;
                const real* const pFn = pF + pl;
                iteration(even, std::true_type{}, t, Streams{pO, pO1, pY, pYm, pF, pFm, pK});
                iteration(odd, std::true_type{}, t + 1, Streams{pO1, pO2, pYn, pY, pFn, pF, pK});
                pO = pO2;
                pYm = pYn; pY = pYn + pl;
                pFm = pFn; pF = pFn + pl;
                if constexpr (CORR) pK += (ptrdiff_t)gc.PL;
            }
        }
    }
    // ---- the last X: plane z1 - 1 = tlast - 2
    {
        const auto ro3 = plane(vout, tlast - 2);
#pragma unroll
        for (int o = 0; o < 2; o++) {
            const int hx = (COL + 1 + o + tlast) & 1;
            if (stm[o][hx]) buf_store_nt<real>(x3[o], ro3, off(hx), roff[o]);
        }
    }
}

// Does the three-pass launch take the level?  The levels relax_rr3d_xs_kernel takes by its own rule (fp64 from 385-point rows
// on), not those forced into it by rr3d.black = 2; one plane addressed through a 32-bit buffer descriptor.  part: bit 0 the way
// down, bit 1 the way up's B, R, B after R', bit 2 the way up's R', B, R (switched by relax3d.block3 / relax3d.block3_up /
// relax3d.block3_corr).
bool relax_block3_takes(const mgx_ctx* ctx, const int n[3], size_t elem, int part) {
    if (!(ctx->block3 & part) || elem != 8) return false;
    if ((unsigned long long)Geo<XSplit, double>(n[0], n[1]).PL * 8ull >= (1ull << 31)) return false;
    return n[0] >= 385 && n[1] >= 129 && n[2] >= 65;
}

// colour passes first_colour, 1 - first_colour, first_colour over the interior of an (n[0], n[1], n[2]) level in one launch:
// reads the other colour and the faces of the grid from vin, f; writes first_colour's interior points (store_both: both
// colours') into vout.  Any size the smoother accepts.  coarse != nullptr (first_colour 0, red stored only, vin == vout): the
// first pass reads black through the correction from `coarse` (cn[0] x cn[1] x cn[2]).
template <class real>
void relax3d_xs_block3_launch(mgx_ctx* ctx, const real* vin, real* vout, const real* f, const int n[3], real hx2, real hy2, real hz2,
                              int first_colour, bool store_both, const real* coarse, const int* cn) {
    constexpr int TW = 16;
    const int gx = ceil_div((n[0] - 1) / 2, 60), gy = ceil_div(n[1] - 2, 2 * TW - 6);
    const int tiles = gx * gy, planes = n[2] - 2;
    // every workgroup takes the same time and has a CU to itself: the fewest runs that fill whole rounds to 90 %, counting the
    // three planes a run relaxes before its first store and the one after, runs of at least 16 planes
    const int zrun = ceil_div(planes, runs_filling_rounds(tiles, planes, ctx->num_cus, 64, 16, 4));
    const dim3 grid(tiles * ceil_div(planes, zrun), 1, 1), blk(64, TW, 1);
#define MGX_B3(C, S)                                                                                                          \
    MGX_LAUNCH((relax3d_xs_block3_kernel<real, C, S, TW>), grid, blk, 0, ctx->compute, vin, vout, f, n[0], n[1], n[2], hx2, hy2, \
               hz2, zrun, gx, gy, 1)
    if (coarse) {
        MGX_LAUNCH((relax3d_xs_block3_kernel<real, 0, false, TW, true>), grid, blk, 0, ctx->compute, vin, vout, f, n[0], n[1], n[2], hx2,
                   hy2, hz2, zrun, gx, gy, 1, coarse, cn[0], cn[1]);
    } else if (first_colour == 0) {
        if (store_both) MGX_B3(0, true); else MGX_B3(0, false);
    } else {
        if (store_both) MGX_B3(1, true); else MGX_B3(1, false);
    }
#undef MGX_B3
    snprintf(ctx->last_block3_kernel, sizeof ctx->last_block3_kernel, "relax3d_xs_block3_kernel<%s,%d,%s,%d%s>",
             sizeof(real) == 8 ? "double" : "float", first_colour, store_both ? "true" : "false", TW, coarse ? ",corr" : "");
}
template void relax3d_xs_block3_launch<double>(mgx_ctx*, const double*, double*, const double*, const int[3], double, double, double, int,
                                               bool, const double*, const int*);
template <>
void relax3d_xs_block3_launch<float>(mgx_ctx*, const float*, float*, const float*, const int[3], float, float, float, int, bool, const float*,
                                     const int*) {}  // fp64 only: never taken

}  // namespace mgx

extern "C" int mgx3dxs_relax_block3_f64(mgx_ctx* ctx, const double* vin, double* vout, const double* f, const int n[3], const double h[3],
                                        int first_colour, int store_both) {
    MGX_REQUIRE(ctx && vin && vout && f && n && h, MGX_ERR_INVALID, "relax_block3: NULL argument");
    MGX_USE(ctx);
    MGX_REQUIRE(mgx::valid_size(n[0]) && mgx::valid_size(n[1]) && mgx::valid_size(n[2]), MGX_ERR_SIZE,
                "relax_block3: sizes %d x %d x %d are not odd and >= 3", n[0], n[1], n[2]);
    MGX_REQUIRE(first_colour == 0 || first_colour == 1, MGX_ERR_INVALID, "relax_block3: first_colour = %d not in {0, 1}", first_colour);
    const unsigned long long plane_bytes = (unsigned long long)mgx::Geo<mgx::XSplit, double>(n[0], n[1]).PL * 8ull;
    MGX_REQUIRE(plane_bytes < (1ull << 31), MGX_ERR_SIZE,
                "relax_block3: a plane of %d x %d is too large", n[0], n[1]);
    MGX_REQUIRE(!store_both || vin != vout, MGX_ERR_INVALID, "relax_block3: store_both needs vout != vin");
    mgx::relax3d_xs_block3_launch<double>(ctx, vin, vout, f, n, h[0] * h[0], h[1] * h[1], h[2] * h[2], first_colour, store_both != 0, nullptr, nullptr);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}

// the correcting launch alone, in place: red = R(B(R'(v, coarse_v))) on the interior; nothing else of v is written
extern "C" int mgx3dxs_relax_block3_corr_f64(mgx_ctx* ctx, double* v, const double* f, const int n[3], const double h[3], const double* coarse_v,
                                             const int cn[3]) {
    MGX_REQUIRE(ctx && v && f && n && h && coarse_v && cn, MGX_ERR_INVALID, "relax_block3_corr: NULL argument");
    MGX_USE(ctx);
    MGX_REQUIRE(mgx::valid_size(n[0]) && mgx::valid_size(n[1]) && mgx::valid_size(n[2]), MGX_ERR_SIZE,
                "relax_block3_corr: sizes %d x %d x %d are not odd and >= 3", n[0], n[1], n[2]);
    for (int d = 0; d < 3; d++)
        MGX_REQUIRE(cn[d] == (n[d] - 1) / 2 + 1, MGX_ERR_SIZE, "relax_block3_corr: coarse size[%d] = %d != (%d-1)/2+1", d, cn[d], n[d]);
    const unsigned long long plane_bytes = (unsigned long long)mgx::Geo<mgx::XSplit, double>(n[0], n[1]).PL * 8ull;
    MGX_REQUIRE(plane_bytes < (1ull << 31), MGX_ERR_SIZE, "relax_block3_corr: a plane of %d x %d is too large", n[0], n[1]);
    mgx::relax3d_xs_block3_launch<double>(ctx, v, v, f, n, h[0] * h[0], h[1] * h[1], h[2] * h[2], 0, false, coarse_v, cn);
    MGX_LAUNCH_CHECK();
    return MGX_OK;
}
