// mgx_pipe_step.inc -- ONE step (plane z) of relax3d_xs_pipe_kernel's unrolled loop, included once per step of a loop trip with
// MGX_K = 0 ... 3 (DEPTH 1) or 0 ... 5 (DEPTH 2) (mgx_pipe3d.hip).  Register roles by step: the planes z - 1, z, z + 1 are c[K % CR],
// c[(K + 1) % CR], c[(K + 2) % CR]; c[(K + 3) % CR] is the plane that ARRIVES during this step (z + 2) and c[(K + 2 + DEPTH) % CR] the one
// REQUESTED in it -- the same set with DEPTH 1 (CR = 4: loads one step ahead, waited for with vmcnt(0) at the step's end), one further
// on with DEPTH 2 (CR = 6: the column and f are requested TWO steps ahead, the step's end waits for everything but the 2 R loads it
// has just issued: twice the bytes in flight per CU).  f in FR = DEPTH + 1 sets alike; rim / edge rows (always one step ahead) and
// results in pairs of sets by step parity; the row parity q = Q0 ^ (K & 1) is a literal.  An include file rather than a lambda: values
// handed to a lambda by reference end up in scratch memory here (the compiler then waits for a load right where it is issued), and a
// macro cannot carry #pragma unroll readably.
{
        constexpr int K = MGX_K;
        constexpr int q = Q0 ^ (K & 1);  // the colour's half of row 0 at plane z
        real (&cp)[R] = c[K % CR], (&cc)[R] = c[(K + 1) % CR], (&cu)[R] = c[(K + 2) % CR], (&cn)[R] = c[(K + 3) % CR], (&cl)[R] = c[(K + 2 + DEPTH) % CR];
        real (&fc)[R] = fb[K % FR], (&fl)[R] = fb[(K + DEPTH) % FR], (&xc)[R] = xb[K & 1], (&xn)[R] = xb[(K + 1) & 1];
        real (&oc)[R] = ob[K & 1], (&op)[R] = ob[(K + 1) & 1];
        real &Nc = nb2[K & 1], &Nn = nb2[(K + 1) & 1], &Sc = sb2[K & 1], &Sn = sb2[(K + 1) & 1];
        const bool more = z + 1 < z1;
        // plane descriptors: base in SGPRs + a uniform row offset + the lane's ONE byte offset -- no per-access address registers
        const auto rv = plane_rsrc<real>(pv, sxy, 2 + DEPTH), rf = plane_rsrc<real>(pf + sxy, sxy, DEPTH), ro = plane_rsrc<real>(po - sxy, sxy, 2);
        __builtin_amdgcn_s_setprio(3);
        if constexpr (CORR) {
            // the coarse plane under the arrivals of step z + 3, requested FIRST in this step and waited for with everything else at
            // its end (the rolled loop requests it last and leaves it in flight over the step's end, which the compiler cannot follow
            // through four step bodies: it then waits in mid-step); through a descriptor like the column loads -- a 64-bit address
            // formed in a register would need one to spare.  Stored into the ring at the end of the NEXT step as before.
            if (more && !(z & 1) && z + 4 < z1 && kload) {
                const auto rk = plane_rsrc<real>(coarse + (size_t)min((z >> 1) + 3, ckmax) * CPL, (int)CPL, 1);
#pragma unroll
                for (int a = 0; a < WX; a++) kt[a] = buf_load<real>(rk, kgb[a], 0);
                if (klast) kt[WX] = buf_load<real>(rk, kgb[WX], 0);
            }
        }
        if (z > z0 && !(ABLP & 4)) {  // results of plane z-1 (ABLP & 4: no stores)
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int qr = q ^ 1 ^ (r & 1);
                if (lane_on && (qr | j) && r < nrows) buf_store_nt<real>(op[r], ro, jb, MGX_RO(roff[r]) + MGX_HO(qr, 1));
            }
        }
        if constexpr (ZERO1) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                constexpr int qo_base = 1 - q;
                const int qo = qo_base ^ (r & 1);
                if (lane_on && (qo | j) && r < nrows) buf_store_nt<real>(cc[r], ro, jb, sxy + MGX_RO(roff[r]) + MGX_HO(qo, 0));
            }
        }
        if (more) {
            // everything else plane z + 1 needs from memory (MGX_LOAD_RIM): the rows above / below the tile, the pairs left / right of it
            if (wy == 0) Nn = buf_load<real>(rv, jb, sxy + MGX_RO(roffN) + MGX_HO(q ^ 1, 0));
            if (wy == WY - 1) Sn = buf_load<real>(rv, jb, sxy + MGX_RO(roffS) + MGX_HO(q ^ 1 ^ ((R - 1) & 1), 0));
            if (rimL || rimR) {
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int qr_ = q ^ 1 ^ (r & 1);
                    xn[r] = buf_load<real>(rv, qr_ ? jbR : jbL, sxy + MGX_RO(roff[r]) + MGX_HO(1 - qr_, 0));
                }
            }
        }
        if constexpr (DEPTH == 1) {
            if (more && !(ABLP & 8)) {  // ABLP & 8: no column / f loads
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int qn = q ^ 1 ^ (r & 1);
                    cl[r] = buf_load<real>(rv, jb, MGX_RO(roff[r]) + 2 * sxy + MGX_HO(qn, 0));
                    fl[r] = FNT ? buf_load_nt<real>(rf, jb, MGX_RO(roff[r]) + MGX_HO(qn, 1)) : buf_load<real>(rf, jb, MGX_RO(roff[r]) + MGX_HO(qn, 1));
                }
            }
        } else {
            // the LAST 2 R requests of the step, whatever the step: the wait at its end counts on that.  Planes past the run's end
            // are clamped onto plane z1 (valid memory; the values are never used)
            const int d3 = min(3, z1 - z) * sxy, d2 = (min(2, z1 - z) - 1) * sxy;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int qr = q ^ (r & 1);  // the other colour's half of the row at plane z + 3 = the colour's half at plane z + 2
                cl[r] = buf_load<real>(rv, jb, MGX_RO(roff[r]) + d3 + MGX_HO(qr, 0));
                fl[r] = FNT ? buf_load_nt<real>(rf, jb, MGX_RO(roff[r]) + d2 + MGX_HO(qr, 1)) : buf_load<real>(rf, jb, MGX_RO(roff[r]) + d2 + MGX_HO(qr, 1));
            }
        }
        if (more) publish((z + 1) & 1, cu);
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
            const real N = r == 0 ? Nedge : cc[r > 0 ? r - 1 : 0];
            const real S = r == R - 1 ? Sedge : cc[r < R - 1 ? r + 1 : r];
            oc[r] = (ABLP & 1) ? W + E + N + S + cp[r] + cu[r] + fc[r] : relax3d_point_rd<real>(W, E, N, S, cp[r], cu[r], fc[r], hx2, hy2, hz2, rd);  // ABLP & 1: seven additions instead of the update
        }
        real en[R];
        bool dc[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            en[r] = 0;
            dc[r] = false;
        }
        if (ABLP & 2) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // no barrier (the waves of a workgroup drift apart; stale neighbours)
        else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        real er = 0, ee = 0;
        int rrim = 0;
        if constexpr (CORR) {
            if (more) {
                MGX_CORR_PAIR(q ^ 1, z + 2, en[0], en[1]);
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
                if (z + 1 > szg - 2) er = ee = 0;
            }
        }
        if constexpr (DEPTH == 1) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this step's requests have had the whole step
        else if constexpr (R == 2) __builtin_amdgcn_s_waitcnt(0x0F74);   // vmcnt(2 R): everything but this step's column / f requests
        else __builtin_amdgcn_s_waitcnt(0x0F70);
        // what arrived becomes plane z + 2 of the next step in place (no copies: the roles move, not the values)
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (CORR) cn[r] = dc[r] ? cn[r] + en[r] : cn[r];
            if (CORR) xn[r] = (rimc[r] && r == rrim) ? xn[r] + er : xn[r];
        }
        if constexpr (CORR) {
            if ((z & 1) && z > z0 && z + 3 < z1) MGX_K_STORE(((z - 1) >> 1) + 3);
            if (edgeN) Nn = Nn + ee;
            if (edgeS) Sn = Sn + ee;
        }
        if constexpr (ZERO1) {
            constexpr int qx = q ^ 1;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int qn = qx ^ (r & 1);
                cn[r] = zred(cn[r], y0 + r >= sy - 1 || z + 2 >= szg - 1 || (qn == 0 && x0));
                xn[r] = zred(xn[r], qn == 1 && j == M - 2);
            }
            Nn = zred(Nn, y0 - 1 <= 0 || (qx == 0 && x0));
            Sn = zred(Sn, y0 + R >= sy - 1 || ((qx ^ ((R - 1) & 1)) == 0 && x0));
        }
        pv += sxy;
        pf += sxy;
        po += sxy;
}
