/* mg_mixed3d.inc -- mgMultiGrid3D_f64_PCG_mixed: the solve of PCG with an fp32 preconditioner (an addition: the reference only
 * cycles).  Included once by mg_multigrid.c after both instantiations, so it calls the static helpers of either directly
 * (pcg_precond3_f32 on the twin, pcg_alloc3_f64 / pcg_true_sumsq3_f64 on the fp64 hierarchy).
 *
 * The iterate x, the right-hand side b, the residual r and the CG vectors p, q stay fp64; the preconditioner is one fp32
 * VCycle(0, v1, v2) from zero on a twin hierarchy, whose d_f[0] receives r32 = (float)(r s) and whose d_v[0] holds the result
 * z32, read back as z = (double)z32 / s.  s = 2^-floor(log2(rms)) with rms = sqrt(rr / interior points) of the last sum of
 * squares the host read: a power of two, so M(s r) / s = M(r) bit for bit (every operation of the V-cycle is linear and a power
 * of two scales IEEE results exactly); s only keeps fp32 out of underflow and overflow.  The kernels write the twin's d_f[0]
 * on interior points only and never write its d_v[0]: the twin's rim flags stay truthful without being touched. */

typedef struct mgMixed3D {
    mgMultiGrid3D_f32* tw; /* the fp32 twin hierarchy */
    double* work;          /* mgx3dxs_mixed_work_elems_f64 doubles of reduction scratch */
} mgMixed3D;

static void mg_mixed3d_free(mgx_ctx* ctx, void* state) {
    mgMixed3D* m = (mgMixed3D*)state;
    if (!m) return;
    mgMultiGrid3D_f32_destroy(m->tw);
    mgx_free(ctx, m->work);
    free(m);
}

/* the twin of mg: built on first use (same sizes, the range converted to float, x-split, CORRECT), rebuilt when mg's numGrids
 * exceeds its levels; given mg's numGrids and use_graph on every call */
static int mg_mixed3d_twin(mgMultiGrid3D_f64* mg, mgMixed3D** out) {
    mgMixed3D* m = (mgMixed3D*)mg->pcg_mixed;
    if (m && mg->numGrids > m->tw->maxGrids) {
        mg_mixed3d_free(mg->ctx, m);
        mg->pcg_mixed = m = NULL;
    }
    if (!m) {
        const mgGrid3D_f64* g = mg->grids3D[0];
        const float range[6] = {(float)g->x_a, (float)g->x_b, (float)g->y_a, (float)g->y_b, (float)g->z_a, (float)g->z_b};
        m = (mgMixed3D*)calloc(1, sizeof *m);
        MG_REQUIRE(m, MGX_ERR_NOMEM, "PCG_mixed: out of host memory");
        int st;
        if (semi_below3_f64(mg, 0)) { /* a semi-coarsened hierarchy: its plan copied, not recomputed in float */
            mgSemiPlan plan;
            plan_of3_f64(mg, &plan);
            st = create_plan3_f32(mg->ctx, &plan, range, &m->tw);
        } else {
            st = mgMultiGrid3D_f32_create_levels(mg->ctx, g->sizeXYZ, range, 1, mg->numGrids, &m->tw);
        }
        if (!st && m->tw->maxGrids < mg->numGrids)
            st = mg_fail(MGX_ERR_SIZE, "PCG_mixed: the fp32 twin has %d levels, numGrids is %d", m->tw->maxGrids, mg->numGrids);
        if (!st) st = mgx_malloc(mg->ctx, mgx3dxs_mixed_work_elems_f64(g->sizeXYZ) * sizeof(double), (void**)&m->work);
        if (st) {
            mg_mixed3d_free(mg->ctx, m);
            return st;
        }
        m->tw->residual_mode = MGX_RESIDUAL_CORRECT;
        mg->pcg_mixed = m;
    }
    m->tw->numGrids = mg->numGrids;
    m->tw->use_graph = mg->use_graph;
    *out = m;
    return MGX_OK;
}

/* s = 2^-floor(log2(rms)), rms = sqrt(rr / interior points); 1 when rr is 0 or not finite */
static double mg_mixed3d_scale(double rr, const int n[3]) {
    const double rms = sqrt(rr / ((double)(n[0] - 2) * (double)(n[1] - 2) * (double)(n[2] - 2)));
    if (!(rms > 0.0) || !isfinite(rms)) return 1.0;
    int e;
    frexp(rms, &e); /* rms = m 2^e with m in [0.5, 1): floor(log2(rms)) = e - 1 */
    if (e < -1000) e = -1000; /* s and 1 / s stay finite and normal */
    if (e > 1000) e = 1000;
    return ldexp(1.0, 1 - e);
}

/* krylov = 0: defect correction.  x ping-pongs between d_v[0] and pcg_x (the fused pass corrects out of place); b is d_f[0]
 * itself, which is only read.  Each step is one fp32 V-cycle and one pass x' = x + z32 / s_old, r = b - A x',
 * r32 = (float)(r s_new), <r, r>: the residual of every step is the true one of the stored x'. */
static int mg_mixed3d_ir(mgMultiGrid3D_f64* mg, mgMixed3D* m, int v1, int v2, double tol, int maxit, int* iters, double* rel_res,
                         int* converged, double* host_hist, int hist_cap) {
    mgx_ctx* ctx = mg->ctx;
    mgGrid3D_f64* g = mg->grids3D[0];
    mgGrid3D_f32* t = m->tw->grids3D[0];
    const int* n = g->sizeXYZ;
    const double h[3] = {g->h_x, g->h_y, g->h_z};
    const size_t bytes = mgx3dxs_elems_f64(n) * sizeof(double);
    double* xs[2] = {g->d_v, mg->pcg_x};
    double* rr_dev = mg->pcg_state + MGX_CG_RR;
    double rr0 = 0.0, rr = 0.0;
    MG_TRY(pcg_true_sumsq3_f64(mg, g->d_v, g->d_f, &rr0));
    if (rr0 == 0.0) {
        *converged = 1;
        return MGX_OK;
    }
    MG_TRY(mgx_memcpy_d2d(ctx, mg->pcg_x, g->d_v, bytes)); /* the partner's boundary (and zero pads) = the guess's */
    double s = mg_mixed3d_scale(rr0, n);
    int cur = 0;
    int st = mgx3dxs_correct_residual_demote_f64(ctx, xs[0], NULL, g->d_f, NULL, 1.0, t->d_f, s, n, h, m->work, rr_dev);
    for (int k = 1; !st && k <= maxit; k++) {
        st = pcg_precond3_f32(m->tw, v1, v2);
        const double s_new = mg_mixed3d_scale(k == 1 ? rr0 : rr, n);
        if (!st) st = mgx3dxs_correct_residual_demote_f64(ctx, xs[cur], xs[1 - cur], g->d_f, t->d_v, 1.0 / s, t->d_f, s_new, n, h, m->work, rr_dev);
        if (!st) st = mgx_memcpy_d2h(ctx, &rr, rr_dev, sizeof(double));
        if (st) break;
        cur = 1 - cur;
        s = s_new;
        const double rel = sqrt(rr / rr0);
        if (k - 1 < hist_cap) host_hist[k - 1] = rel;
        *iters = k;
        *rel_res = rel;
        if (rel < tol) {
            *converged = 1;
            break;
        }
        if (!isfinite(rel)) break;
    }
    /* the result into d_v[0]: the two arrays have the same boundary and pads, so d_v[0]'s rim flags stay as they are; d_e's
     * boundary copy is declared stale as PCG does */
    if (!st && cur) st = mgx_memcpy_d2d(ctx, g->d_v, xs[1], bytes);
    mg->e_rim_valid[0] = 0;
    if (!st) st = mgx_ctx_sync(ctx);
    return st;
}

/* krylov != 0: the flexible CG of pcg_krylov3_ with z = M32(r).  r lives in d_f[0] (fp64), x, the copy of b, p and q in PCG's
 * scratch; r32 / z32 are the twin's d_f[0] / d_v[0].  The demotion of r rides on the pass that updates it (cg_update_demote)
 * and the promotion of z on the passes that read it (dot2_mixed, cg_direction_mixed). */
static int mg_mixed3d_fcg(mgMultiGrid3D_f64* mg, mgMixed3D* m, int v1, int v2, double tol, int maxit, int* iters, double* rel_res,
                          int* converged, double* host_hist, int hist_cap) {
    mgx_ctx* ctx = mg->ctx;
    mgGrid3D_f64* g = mg->grids3D[0];
    mgGrid3D_f32* t = m->tw->grids3D[0];
    const int* n = g->sizeXYZ;
    const double h[3] = {g->h_x, g->h_y, g->h_z};
    const size_t bytes = mgx3dxs_elems_f64(n) * sizeof(double);
    double *x = mg->pcg_x, *b = mg->pcg_b, *p = mg->pcg_p, *q = mg->pcg_q, *r = g->d_f;
    float *r32 = t->d_f, *z32 = t->d_v;
    double *sv = mg->pcg_state, *w = m->work;
    const unsigned char v_rim0 = mg->v_rim_zero[0], f_rim0 = mg->f_rim_zero[0];
    MG_TRY(mgx_memcpy_d2d(ctx, x, g->d_v, bytes)); /* x: the guess with its Dirichlet boundary; pads are zero in both */
    MG_TRY(mgx_memcpy_d2d(ctx, b, g->d_f, bytes));
    int st = MGX_OK;
    double rr0 = 0.0, rr = 0.0, s = 1.0;
    int pending = 0; /* x still lacks alpha p of the last iteration */
    st = mgx3dxs_residual_f64(ctx, x, b, r, n, h, MGX_RESIDUAL_CORRECT);
    mg->f_rim_zero[0] = 0;
    if (!st) st = mgx3dxs_dot2_f64(ctx, r, r, NULL, n, w, sv + MGX_CG_RR);
    if (!st) st = mgx_memcpy_d2h(ctx, &rr0, sv + MGX_CG_RR, sizeof(double));
    if (!st && rr0 == 0.0) *converged = 1;
    rr = rr0; /* the last sum of squares read: the scale of the next demotion */
    int restart = 1; /* z = M r, p = z, rz = <r, z> */
    for (int k = 1; !st && !*converged && k <= maxit; k++) {
        if (restart) {
            s = mg_mixed3d_scale(rr, n);
            st = mgx3dxs_demote_f64(ctx, r, r32, s, n);
            if (!st) st = pcg_precond3_f32(m->tw, v1, v2);
            if (!st) st = mgx3dxs_dot2_mixed_f64(ctx, z32, 1.0 / s, r, NULL, n, w, sv + MGX_CG_ZR);
            if (!st) st = mgx_cg_scalars(ctx, sv, 2);
            if (!st) st = mgx3dxs_cg_direction_mixed_f64(ctx, NULL, p, z32, 1.0 / s, n, NULL, NULL);
            restart = 0;
        }
        /* q = A p, alpha = <r, z> / <p, q>; r -= alpha q, r32 = (float)(r s) */
        if (!st) st = mgx3dxs_laplace_dot_f64(ctx, p, q, n, h, w, sv + MGX_CG_PQ);
        if (!st) st = mgx_cg_scalars(ctx, sv, 0);
        s = mg_mixed3d_scale(rr, n);
        if (!st) st = mgx3dxs_cg_update_demote_f64(ctx, NULL, p, r, q, r32, s, n, sv + MGX_CG_ALPHA, w, sv + MGX_CG_RR);
        if (!st) st = mgx_memcpy_d2h(ctx, &rr, sv + MGX_CG_RR, sizeof(double)); /* the one host read of the iteration */
        if (st) break;
        *iters = k;
        if (!isfinite(rr)) break; /* breakdown: alpha was NaN; x is the previous iterate */
        pending = 1;
        const double rel = sqrt(rr / rr0);
        if (k - 1 < hist_cap) host_hist[k - 1] = rel;
        if (rel < tol) { /* the recursive residual may have drifted from b - A x: check the true one */
            st = mgx3dxs_cg_direction_f64(ctx, x, p, NULL, n, sv + MGX_CG_ALPHA, NULL);
            pending = 0;
            if (!st) st = mgx3dxs_residual_f64(ctx, x, b, r, n, h, MGX_RESIDUAL_CORRECT);
            if (!st) st = mgx3dxs_dot2_f64(ctx, r, r, NULL, n, w, sv + MGX_CG_RR);
            if (!st) st = mgx_memcpy_d2h(ctx, &rr, sv + MGX_CG_RR, sizeof(double));
            if (!st && sqrt(rr / rr0) < tol) *converged = 1;
            restart = 1; /* otherwise go on from the true residual */
            continue;
        }
        /* z = M r; beta = -alpha <z, q> / <r, z>_old; x += alpha p; p = z + beta p */
        st = pcg_precond3_f32(m->tw, v1, v2);
        if (!st) st = mgx3dxs_dot2_mixed_f64(ctx, z32, 1.0 / s, r, q, n, w, sv + MGX_CG_ZR);
        if (!st) st = mgx_cg_scalars(ctx, sv, 1);
        if (!st) st = mgx3dxs_cg_direction_mixed_f64(ctx, x, p, z32, 1.0 / s, n, sv + MGX_CG_ALPHA, sv + MGX_CG_BETA);
        pending = 0;
    }
    if (!st && pending) st = mgx3dxs_cg_direction_f64(ctx, x, p, NULL, n, sv + MGX_CG_ALPHA, NULL);
    /* the true relative residual of the result */
    if (!st && rr0 > 0.0) {
        double ss = 0.0;
        st = pcg_true_sumsq3_f64(mg, x, b, &ss);
        if (!st) *rel_res = sqrt(ss / rr0);
    } else if (!st && rr0 != 0.0) {
        *rel_res = rr0; /* NaN: the initial residual is not finite */
    }
    /* d_v[0] := x, d_f[0] := b, their flags as they were; d_e's boundary copy no longer matches d_v's */
    const int st2 = mgx_memcpy_d2d(ctx, g->d_v, x, bytes);
    const int st3 = mgx_memcpy_d2d(ctx, g->d_f, b, bytes);
    mg->v_rim_zero[0] = v_rim0;
    mg->f_rim_zero[0] = f_rim0;
    mg->e_rim_valid[0] = 0;
    if (!st) st = st2 ? st2 : st3;
    if (!st) st = mgx_ctx_sync(ctx);
    return st;
}

int mgMultiGrid3D_f64_PCG_mixed(mgMultiGrid3D_f64* mg, int v1, int v2, double tol, int maxit, int krylov, int* iters, double* rel_res,
                                int* converged, double* host_hist, int hist_cap) {
    MG_REQUIRE(mg && iters && rel_res && converged && (host_hist || hist_cap <= 0), MGX_ERR_INVALID, "PCG_mixed: NULL argument");
    MG_REQUIRE(mg->numGrids >= 1 && mg->numGrids <= mg->maxGrids, MGX_ERR_INVALID, "PCG_mixed: numGrids = %d outside [1,%d]",
               mg->numGrids, mg->maxGrids);
    MG_REQUIRE(!mg->cap, MGX_ERR_INVALID, "PCG_mixed: a hierarchy with a capacity is not supported");
    MG_REQUIRE(!mg->wall, MGX_ERR_INVALID, "PCG_mixed: a hierarchy with wall data (set_wall) is not supported");
    MG_REQUIRE(!mg->pin, MGX_ERR_INVALID, "PCG_mixed: a hierarchy with pinned nodes (set_pinned) is not supported: precond = f32 is not available");
    MG_REQUIRE(mg->shift == 0, MGX_ERR_INVALID, "PCG_mixed: a shifted hierarchy (shift = %g) is not supported", mg->shift);
    MG_REQUIRE(!(mg->grids3D && mg->grids3D[0] && mg->grids3D[0]->d_a), MGX_ERR_INVALID,
               "PCG_mixed: a hierarchy with a coefficient is not supported");
    MG_REQUIRE(mg->bc == 0, MGX_ERR_INVALID, "PCG_mixed: a hierarchy with Neumann faces (mask %d) is not supported", mg->bc);
    MG_REQUIRE(mg->layout == 1, MGX_ERR_INVALID, "PCG_mixed: needs the x-split layout (layout = 1)");
    MG_REQUIRE(mg->residual_mode == MGX_RESIDUAL_CORRECT, MGX_ERR_INVALID, "PCG_mixed: needs residual_mode = MGX_RESIDUAL_CORRECT");
    MG_REQUIRE(tol > 0 && maxit >= 1 && v1 >= 0 && v2 >= 0 && v1 + v2 >= 1, MGX_ERR_INVALID,
               "PCG_mixed: bad arguments (tol %g, maxit %d, v1 %d, v2 %d)", tol, maxit, v1, v2);
    *iters = 0;
    *rel_res = 0.0;
    *converged = 0;
    MG_TRY(pcg_alloc3_f64(mg));
    MG_TRY(mgx_memset_zero(mg->ctx, mg->pcg_state + MGX_CG_FMEAN, sizeof(double))); /* (no mean is removed here) */
    mgMixed3D* m = NULL;
    MG_TRY(mg_mixed3d_twin(mg, &m));
    if (!krylov) return mg_mixed3d_ir(mg, m, v1, v2, tol, maxit, iters, rel_res, converged, host_hist, hist_cap);
    return mg_mixed3d_fcg(mg, m, v1, v2, tol, maxit, iters, rel_res, converged, host_hist, hist_cap);
}

int mg3d_solve_pcg_mixed_f64(mgx_ctx* ctx, double* grid, const double* rhs, const int sizeXYZ[3], const double range[6], int nlevels,
                             int v1, int v2, double tol, int maxit, int krylov, int* iters, double* rel_res, int* converged) {
    MG_REQUIRE(ctx && grid && sizeXYZ && range, MGX_ERR_INVALID, "mg3d_solve_pcg_mixed: NULL argument");
    mgMultiGrid3D_f64* mg = NULL;
    MG_TRY(mgMultiGrid3D_f64_create_levels(ctx, sizeXYZ, range, 1, nlevels, &mg));
    int st = MGX_OK;
    if (nlevels > 0) {
        if (nlevels > mg->maxGrids) st = mg_fail(MGX_ERR_SIZE, "mg3d_solve_pcg_mixed: nlevels %d > %d", nlevels, mg->maxGrids);
        else mg->numGrids = nlevels;
    }
    mg->residual_mode = MGX_RESIDUAL_CORRECT;
    if (!st) st = mgMultiGrid3D_f64_upload_v(mg, 0, grid);
    if (!st && rhs) st = mgMultiGrid3D_f64_upload_f(mg, 0, rhs);
    if (!st) st = mgMultiGrid3D_f64_PCG_mixed(mg, v1, v2, tol, maxit, krylov, iters, rel_res, converged, NULL, 0);
    if (!st) st = mgMultiGrid3D_f64_download_v(mg, 0, grid);
    mgMultiGrid3D_f64_destroy(mg);
    return st;
}
