// mgx_pipe2_step.inc -- ONE step (plane z) of relax3d_xs_pipe_v2_kernel's unrolled loop (two x-pairs per lane), included four
// times with MGX_K = 0 ... 3 (mgx_pipe3d.hip).  Register roles by step as in mgx_pipe_step.inc: planes z - 1, z, z + 1 and the one
// on its way are c[K & 3], c[(K + 1) & 3], c[(K + 2) & 3], c[(K + 3) & 3]; f / rim / edge rows / results in pairs of sets by step
// parity; the row parity q = (UNR - 1) ^ (K & 1) is a literal.  The two points a lane updates per row are formed as ONE two-element
// vector expression (relax3d_num2: packed fp32 multiplies and adds, element-wise IEEE: the bits of the scalar form).
{
        constexpr int K = MGX_K;
        constexpr int q = (UNR - 1) ^ (K & 1);  // the colour's half of row 0 at plane z
        vec2 (&cp)[R] = c[K & 3], (&cc)[R] = c[(K + 1) & 3], (&cu)[R] = c[(K + 2) & 3], (&cn)[R] = c[(K + 3) & 3];
        vec2 (&fc)[R] = fb[K & 1], (&fn)[R] = fb[(K + 1) & 1], (&oc)[R] = ob[K & 1], (&op)[R] = ob[(K + 1) & 1];
        real (&xc)[R] = xb[K & 1], (&xn)[R] = xb[(K + 1) & 1];
        vec2 &Nc = nb2[K & 1], &Nn = nb2[(K + 1) & 1], &Sc = sb2[K & 1], &Sn = sb2[(K + 1) & 1];
        const bool more = z + 1 < z1;
        const auto rv = plane_rsrc<real>(pv, sxy, 3), rf = plane_rsrc<real>(pf + sxy, sxy, 1), ro = plane_rsrc<real>(po - sxy, sxy, 2);
        __builtin_amdgcn_s_setprio(3);
        if constexpr (CORR) {
            // the coarse plane under the arrivals of step z + 3: requested first in the step, waited for with everything else at its
            // end, stored into the ring at the end of the next step (see mgx_pipe_step.inc)
            if (more && !(z & 1) && z + 4 < z1 && kload) {
                const auto rk = plane_rsrc<real>(coarse + (size_t)min((z >> 1) + 3, ckmax) * CPL, (int)CPL, 1);
#pragma unroll
                for (int a = 0; a < NK; a++) kt[a] = buf_load<real>(rk, kgb[a], 0);
                if (klast) kt[NK] = buf_load<real>(rk, kgb[NK], 0);
            }
        }
        if (z > z0) {  // results of plane z-1
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int qr = q ^ 1 ^ (r & 1);
                if (lane_on && r < nrows) {
                    if (qr | j0) buf_store2_nt<real>(op[r], ro, jb, roff[r] + qr * H);  // both elements are interior points
                    else buf_store_nt<real>(op[r].y, ro, jb, roff[r] + qr * H + 1);    // x = 0 is a boundary point: element 1 only
                }
            }
        }
        if (more) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int qn = q ^ 1 ^ (r & 1);
                cn[r] = buf_load2<real>(rv, jb, roff[r] + 2 * sxy + qn * H);
                fn[r] = FNT ? buf_load2_nt<real>(rf, jb, roff[r] + qn * H) : buf_load2<real>(rf, jb, roff[r] + qn * H);
            }
            if (wy == 0) Nn = buf_load2<real>(rv, jb, sxy + roffN + (q ^ 1) * H);
            if (wy == WY - 1) Sn = buf_load2<real>(rv, jb, sxy + roffS + (q ^ 1 ^ ((R - 1) & 1)) * H);
            if (rimL || rimR) {
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int qr_ = q ^ 1 ^ (r & 1);
                    xn[r] = buf_load<real>(rv, qr_ ? jbR : jbL, sxy + roff[r] + (1 - qr_) * H);
                }
            }
            publish((z + 1) & 1, cu);
        }
        __builtin_amdgcn_s_setprio(0);
        const int slot = z & 1;
        const vec2 Nl = ey[slot][wyN][wx][1][lane], Sl = ey[slot][wyS][wx][0][lane];
        const vec2 Nedge = wy > 0 ? Nl : Nc;
        const vec2 Sedge = wy < WY - 1 ? Sl : Sc;
        real far[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int qr = q ^ (r & 1);
            const real fromR = ex[slot][wy][wxR][0][r], fromL = ex[slot][wy][wxL][1][r];
            if (qr) {
                far[r] = __shfl_down(cc[r].x, 1, 64);
                if (lane == 63) far[r] = fromR;
                if (rimR) far[r] = xc[r];
            } else {
                far[r] = __shfl_up(cc[r].y, 1, 64);
                if (lane == 0) far[r] = fromL;
                if (rimL) far[r] = xc[r];
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int qr = q ^ (r & 1);
            const vec2 N = r == 0 ? Nedge : cc[r > 0 ? r - 1 : 0];
            const vec2 S = r == R - 1 ? Sedge : cc[r < R - 1 ? r + 1 : r];
            // q_r = 1: W = the pair's own even entry, E = the next pair's; q_r = 0: W = the previous pair's odd entry, E = the own one
            const vec2 W = qr ? cc[r] : vec2{far[r], cc[r].x};
            const vec2 E = qr ? vec2{cc[r].y, far[r]} : cc[r];
            oc[r] = relax3d_point_rd2<real, vec2>(W, E, N, S, cp[r], cu[r], fc[r], hx2, hy2, hz2, rd);
        }
        real en0[R], en1[R];
        bool dc0[R], dc1[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            en0[r] = en1[r] = 0;
            dc0[r] = dc1[r] = false;
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        real er = 0;
        vec2 ee = {0, 0};  // the corrections of the edge-row values that are on their way (plane z + 1)
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
                    ee = ee0;
                } else {
                    if (wx == 0 || wx == WX - 1) MGX_CORR_RIM2(q ^ 1, z + 1, rrim, er);
                    if (wy == 0 || wy == WY - 1) MGX_CORR_EDGE2(q ^ 1, z + 1, ee);
                }
                if (z + 1 > szg - 2) {  // a boundary plane: no correction
                    er = 0;
                    ee = vec2{0, 0};
                }
            }
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this step's requests have had the whole step
        if constexpr (CORR) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                cn[r].x = dc0[r] ? cn[r].x + en0[r] : cn[r].x;
                cn[r].y = dc1[r] ? cn[r].y + en1[r] : cn[r].y;
                xn[r] = (rimc[r] && r == rrim) ? xn[r] + er : xn[r];
            }
            if ((z & 1) && z > z0 && z + 3 < z1) MGX_K2_STORE(((z - 1) >> 1) + 3);  // requested in step z - 1
            if (edgeN) Nn = Nn + ee;
            if (edgeS) Sn = Sn + ee;
        }
        pv += sxy;
        pf += sxy;
        po += sxy;
}
