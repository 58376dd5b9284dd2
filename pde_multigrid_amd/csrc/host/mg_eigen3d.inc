/* mg_eigen3d.inc -- mgMultiGrid3D_f64_Eigen: the lowest eigenpairs of the hierarchy's operator by multigrid-preconditioned LOBPCG
 * (an addition: the reference only cycles; the contract is in mg_multigrid.h, the measurements in DESIGN.md 21), and its dense
 * solver mg_sym_geneig.  Included once by mg_multigrid.c after both instantiations, as mg_mixed3d.inc is: it calls the static helpers of the
 * fp64 one (op_ok3_f64, op_apply_dot3_f64, pcg_precond3_f64, put3_f64 / get3_f64).
 *
 * Device vectors: X, AX, T, AT, P, AP and two spare sets N1, N2, k arrays each.  An iteration:
 *   T_i := r_i = AX_i + mu_i c X_i (block_residual), T_i := M T_i (copy into d_f[0], the V-cycle, copy out of d_v[0]),
 *   AT_i := A T_i, the Gram matrices of [X, T, P] tile by tile (block_gram), the Rayleigh-Ritz problem on the host, then
 *   N1 := T Yt + P Yp, N2 := AT Yt + AP Yp, T := X Yx + N1, AT := AX Yx + N2 (block_combine, out of place), and the sets change
 *   names: X <-> T, AX <-> AT, P <-> N1, AP <-> N2. */

/* ---------------------------------------------------------------- the dense solver */
int mg_sym_geneig(int n, const double* G, const double* B, double* w, double* Y) {
    MG_REQUIRE(G && B && w && Y, MGX_ERR_INVALID, "mg_sym_geneig: NULL argument");
    MG_REQUIRE(n >= 1 && n <= MG_GENEIG_MAX, MGX_ERR_INVALID, "mg_sym_geneig: n = %d outside 1 .. %d", n, MG_GENEIG_MAX);
    enum { N = MG_GENEIG_MAX };
    static const double pivot_min = 64 * DBL_EPSILON; /* of the scaled B, whose diagonal is 1: below it B is singular to rounding */
    double d[N], L[N][N], A[N][N], Z[N][N];
    for (int i = 0; i < n; i++) {
        const double b = B[i * n + i];
        if (!(b > 0) || !isfinite(b)) return MG_GENEIG_NOT_SPD;
        d[i] = 1.0 / sqrt(b);
    }
    /* B' = D B D = L L^T */
    for (int j = 0; j < n; j++) {
        double s = (d[j] * B[j * n + j]) * d[j];
        for (int p = 0; p < j; p++) s -= L[j][p] * L[j][p];
        if (!(s > pivot_min) || !isfinite(s)) return MG_GENEIG_NOT_SPD;
        L[j][j] = sqrt(s);
        for (int i = j + 1; i < n; i++) {
            double t = (d[j] * B[j * n + i]) * d[i]; /* the upper triangle's entry (j, i) */
            for (int p = 0; p < j; p++) t -= L[i][p] * L[j][p];
            L[i][j] = t / L[j][j];
        }
    }
    /* A = L^-1 G' L^-T: column by column W = L^-1 G', then A^T = L^-1 W^T */
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            const double g = i <= j ? G[i * n + j] : G[j * n + i];
            if (!isfinite(g)) return MG_GENEIG_NOT_SPD;
            A[i][j] = (d[i] * g) * d[j];
        }
    for (int pass = 0; pass < 2; pass++) {
        for (int c = 0; c < n; c++)
            for (int i = 0; i < n; i++) {
                double t = A[i][c];
                for (int p = 0; p < i; p++) t -= L[i][p] * A[p][c];
                A[i][c] = t / L[i][i];
            }
        for (int i = 0; i < n; i++) /* transpose */
            for (int j = i + 1; j < n; j++) {
                const double t = A[i][j];
                A[i][j] = A[j][i];
                A[j][i] = t;
            }
    }
    for (int i = 0; i < n; i++) /* symmetric to the bit */
        for (int j = i + 1; j < n; j++) A[i][j] = A[j][i] = 0.5 * (A[i][j] + A[j][i]);
    /* cyclic Jacobi: rotations until no off-diagonal entry exceeds rounding relative to its two diagonal entries */
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) Z[i][j] = i == j;
    for (int sweep = 0; sweep < 64; sweep++) {
        int rotated = 0;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                const double apq = A[p][q], app = A[p][p], aqq = A[q][q];
                if (fabs(apq) <= 0.125 * DBL_EPSILON * sqrt(fabs(app) * fabs(aqq)) || fabs(apq) < DBL_MIN) {
                    A[p][q] = A[q][p] = 0.0;
                    continue;
                }
                rotated = 1;
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                A[p][p] = app - t * apq;
                A[q][q] = aqq + t * apq;
                A[p][q] = A[q][p] = 0.0;
                for (int r = 0; r < n; r++) {
                    if (r != p && r != q) {
                        const double arp = A[r][p], arq = A[r][q];
                        A[r][p] = A[p][r] = c * arp - s * arq;
                        A[r][q] = A[q][r] = s * arp + c * arq;
                    }
                    const double zrp = Z[r][p], zrq = Z[r][q];
                    Z[r][p] = c * zrp - s * zrq;
                    Z[r][q] = s * zrp + c * zrq;
                }
            }
        if (!rotated) break;
        if (sweep == 63) return MG_GENEIG_NO_CONVERGENCE; /* (quadratic convergence needs some ten sweeps at n = 24) */
    }
    /* ascending order (insertion sort of the column order: stable, so equal values keep their order) */
    int ord[N];
    for (int i = 0; i < n; i++) ord[i] = i;
    for (int i = 1; i < n; i++) {
        const int o = ord[i];
        int j = i;
        for (; j > 0 && A[ord[j - 1]][ord[j - 1]] > A[o][o]; j--) ord[j] = ord[j - 1];
        ord[j] = o;
    }
    /* Y = D L^-T Z */
    for (int c = 0; c < n; c++) {
        double y[N];
        for (int i = n - 1; i >= 0; i--) {
            double t = Z[i][ord[c]];
            for (int p = i + 1; p < n; p++) t -= L[p][i] * y[p];
            y[i] = t / L[i][i];
        }
        for (int i = 0; i < n; i++) Y[i * n + c] = d[i] * y[i];
        w[c] = A[ord[c]][ord[c]];
    }
    return MGX_OK;
}

/* ---------------------------------------------------------------- the eigensolver */
enum { EIG_K = MG_EIGEN_MAX_BLOCK, EIG_M = 3 * MG_EIGEN_MAX_BLOCK, EIG_SETS = 8, EIG_TILE = 64, EIG_OUT = 2048 };

typedef struct mgEigen3D {
    mgMultiGrid3D_f64* mg;
    mgGrid3D_f64* g;
    int k, bc;
    const double* c;        /* the capacity of level 0 or NULL */
    double* set[EIG_SETS][EIG_K]; /* X, AX, T, AT, P, AP, N1, N2 */
    double *save_v, *save_f; /* d_v[0] and d_f[0] as they were */
    double *work, *out;      /* partial sums; EIG_OUT device doubles of results */
    double mu[EIG_K], res[EIG_K];
} mgEigen3D;
enum { EIG_X = 0, EIG_AX, EIG_T, EIG_AT, EIG_P, EIG_AP, EIG_N1, EIG_N2 };

static void eig_free(mgEigen3D* E) {
    mgx_ctx* ctx = E->mg->ctx;
    for (int s = 0; s < EIG_SETS; s++)
        for (int i = 0; i < E->k; i++) mgx_free(ctx, E->set[s][i]);
    mgx_free(ctx, E->save_v);
    mgx_free(ctx, E->save_f);
    mgx_free(ctx, E->work);
    mgx_free(ctx, E->out);
}

static int eig_alloc(mgEigen3D* E) {
    mgx_ctx* ctx = E->mg->ctx;
    const int* n = E->g->sizeXYZ;
    const size_t bytes = mgx3dxs_elems_f64(n) * sizeof(double);
    size_t welems = mgx3dxs_block_work_elems_f64(n);
    const size_t kelems = mgx3dxs_krylov_work_elems_bc_f64(n); /* the operator's partials */
    MG_REQUIRE(welems, MGX_ERR_SIZE, "Eigen: the grid %d x %d x %d is too large for the block kernels", n[0], n[1], n[2]);
    if (kelems > welems) welems = kelems;
    /* every array zeroed once: pads and Dirichlet entries are never written by the kernels and are read by the operator as 0 */
    for (int s = 0; s < EIG_SETS; s++)
        for (int i = 0; i < E->k; i++) {
            MG_TRY(mgx_malloc(ctx, bytes, (void**)&E->set[s][i]));
            MG_TRY(mgx_memset_zero(ctx, E->set[s][i], bytes));
        }
    MG_TRY(mgx_malloc(ctx, bytes, (void**)&E->save_v));
    MG_TRY(mgx_malloc(ctx, bytes, (void**)&E->save_f));
    MG_TRY(mgx_malloc(ctx, welems * sizeof(double), (void**)&E->work));
    MG_TRY(mgx_malloc(ctx, EIG_OUT * sizeof(double), (void**)&E->out));
    return MGX_OK;
}

static void eig_swap(mgEigen3D* E, int a, int b) {
    for (int i = 0; i < E->k; i++) {
        double* t = E->set[a][i];
        E->set[a][i] = E->set[b][i];
        E->set[b][i] = t;
    }
}

/* out_i = [add_i +] sum_j Y[j * ldy + i] in_j for i < nout, j < nin, out of place (no out_i is an in_j or an add_j of another
 * group): output groups of four, and where a group's inputs exceed one launch the later launches add to the output */
static int eig_combine(mgEigen3D* E, int nin, double* const* in, const double* Y, int ldy, int nout, double* const* out, double* const* add) {
    const int* n = E->g->sizeXYZ;
    for (int o0 = 0; o0 < nout; o0 += 4) {
        const int no = nout - o0 < 4 ? nout - o0 : 4;
        int j0 = 0, first = 1;
        while (j0 < nin || first) {
            const double* S[12];
            double Yc[12 * 4];
            int m = 0;
            if (!first || add) /* what is there already: the group's add vectors, then the group's own partial results */
                for (int o = 0; o < no; o++, m++) {
                    S[m] = first ? add[o0 + o] : out[o0 + o];
                    for (int q = 0; q < no; q++) Yc[m * no + q] = q == o ? 1.0 : 0.0;
                }
            for (; m < 12 && j0 < nin; m++, j0++) {
                S[m] = in[j0];
                for (int q = 0; q < no; q++) Yc[m * no + q] = Y[j0 * ldy + o0 + q];
            }
            MG_TRY(mgx3dxs_block_combine_f64(E->mg->ctx, m, S, no, out + o0, Yc, n, E->bc));
            first = 0;
        }
    }
    return MGX_OK;
}

/* AV_i = A_s V_i, k operator applications (their dots are not used) */
static int eig_apply(mgEigen3D* E, int v, int av) {
    for (int i = 0; i < E->k; i++) MG_TRY(op_apply_dot3_f64(E->mg, E->g, E->set[v][i], E->set[av][i], E->work, E->out + EIG_OUT - 1));
    return MGX_OK;
}

/* T_i = r_i = AX_i + mu_i c X_i and res_i = ||r_i||_W / (mu_i ||x_i||_W); *all_ok: every res_i < tol */
static int eig_residual(mgEigen3D* E, double tol, int* all_ok) {
    const int k = E->k;
    double h[2 * EIG_K];
    for (int i0 = 0; i0 < k; i0 += 4) {
        const int nv = k - i0 < 4 ? k - i0 : 4;
        MG_TRY(mgx3dxs_block_residual_f64(E->mg->ctx, nv, (const double* const*)(E->set[EIG_AX] + i0), (const double* const*)(E->set[EIG_X] + i0),
                                          E->c, E->mu + i0, E->set[EIG_T] + i0, E->g->sizeXYZ, E->bc, E->work, E->out + 2 * i0));
    }
    MG_TRY(mgx_memcpy_d2h(E->mg->ctx, h, E->out, 2 * (size_t)k * sizeof(double)));
    *all_ok = 1;
    for (int i0 = 0; i0 < k; i0 += 4) {
        const int nv = k - i0 < 4 ? k - i0 : 4;
        for (int i = 0; i < nv; i++) {
            const double rr = h[2 * i0 + i], xx = h[2 * i0 + nv + i];
            E->res[i0 + i] = sqrt(rr) / (fabs(E->mu[i0 + i]) * sqrt(xx));
            if (!(E->res[i0 + i] < tol)) *all_ok = 0;
        }
    }
    return MGX_OK;
}

/* T_i := M T_i: one V(v1, v2) from zero per residual, d_f[0] its right-hand side and d_v[0] its result */
static int eig_precond(mgEigen3D* E, int v1, int v2) {
    mgx_ctx* ctx = E->mg->ctx;
    const size_t bytes = mgx3dxs_elems_f64(E->g->sizeXYZ) * sizeof(double);
    for (int i = 0; i < E->k; i++) {
        MG_TRY(mgx_memcpy_d2d(ctx, E->g->d_f, E->set[EIG_T][i], bytes));
        E->mg->f_rim_zero[0] = 0;
        MG_TRY(pcg_precond3_f64(E->mg, v1, v2));
        MG_TRY(mgx_memcpy_d2d(ctx, E->set[EIG_T][i], E->g->d_v, bytes));
    }
    return MGX_OK;
}

/* The Rayleigh-Ritz step on the first nsets of [X, T, P]: G = -S^T W A S and B = S^T W c S tile by tile (upper triangle), the k
 * lowest pairs into E->mu and Ysel (m x k, row-major).  *ok = 0: B is not positive definite to rounding. */
static int eig_ritz(mgEigen3D* E, int nsets, double* Ysel, int* ok) {
    static const int vs[3] = {EIG_X, EIG_T, EIG_P}, as[3] = {EIG_AX, EIG_AT, EIG_AP};
    mgx_ctx* ctx = E->mg->ctx;
    const int k = E->k, m = nsets * k, ng = (m + 3) / 4;
    const double *S[EIG_M], *AS[EIG_M];
    double G[EIG_M * EIG_M], B[EIG_M * EIG_M], w[EIG_M], Y[EIG_M * EIG_M], h[EIG_OUT];
    for (int s = 0; s < nsets; s++)
        for (int i = 0; i < k; i++) S[s * k + i] = E->set[vs[s]][i], AS[s * k + i] = E->set[as[s]][i];
    int tiles = 0;
    for (int a = 0; a < ng; a++)
        for (int b = a; b < ng; b++, tiles++) {
            const int nu = m - 4 * a < 4 ? m - 4 * a : 4, nv = m - 4 * b < 4 ? m - 4 * b : 4;
            double* o = E->out + (size_t)tiles * EIG_TILE;
            MG_TRY(mgx3dxs_block_gram_f64(ctx, nu, S + 4 * a, nv, AS + 4 * b, NULL, E->g->sizeXYZ, E->bc, E->work, o));
            MG_TRY(mgx3dxs_block_gram_f64(ctx, nu, S + 4 * a, nv, S + 4 * b, E->c, E->g->sizeXYZ, E->bc, E->work, o + 16));
        }
    MG_TRY(mgx_memcpy_d2h(ctx, h, E->out, (size_t)tiles * EIG_TILE * sizeof(double)));
    tiles = 0;
    for (int a = 0; a < ng; a++)
        for (int b = a; b < ng; b++, tiles++) {
            const int nu = m - 4 * a < 4 ? m - 4 * a : 4, nv = m - 4 * b < 4 ? m - 4 * b : 4;
            const double *hg = h + (size_t)tiles * EIG_TILE, *hb = hg + 16 + (E->c ? nu * nv : 0);
            for (int i = 0; i < nu; i++)
                for (int j = 0; j < nv; j++) {
                    const int r = 4 * a + i, c = 4 * b + j;
                    if (r > c) continue; /* (a diagonal tile: its upper triangle) */
                    G[r * m + c] = G[c * m + r] = -hg[i * nv + j];
                    B[r * m + c] = B[c * m + r] = hb[i * nv + j];
                }
        }
    const int st = mg_sym_geneig(m, G, B, w, Y);
    *ok = st == MGX_OK;
    if (st == MG_GENEIG_NOT_SPD || st == MG_GENEIG_NO_CONVERGENCE) return MGX_OK; /* no decomposition: the caller restarts or stops */
    MG_TRY(st);
    for (int i = 0; i < k; i++) {
        if (!(w[i] > 0) || !isfinite(w[i])) *ok = 0; /* -A_s is positive definite: anything else is a broken basis */
        for (int j = 0; j < m; j++) Ysel[j * k + i] = Y[j * m + i];
    }
    if (*ok) memcpy(E->mu, w, (size_t)k * sizeof(double));
    return MGX_OK;
}

/* X := X Y, AX := AX Y for the Rayleigh-Ritz step on X alone (through T and AT, which hold nothing then) */
static int eig_ritz_x(mgEigen3D* E, int* ok) {
    double Y[EIG_M * EIG_K];
    MG_TRY(eig_ritz(E, 1, Y, ok));
    if (!*ok) return MGX_OK;
    MG_TRY(eig_combine(E, E->k, E->set[EIG_X], Y, E->k, E->k, E->set[EIG_T], NULL));
    MG_TRY(eig_combine(E, E->k, E->set[EIG_AX], Y, E->k, E->k, E->set[EIG_AT], NULL));
    eig_swap(E, EIG_X, EIG_T);
    eig_swap(E, EIG_AX, EIG_AT);
    return MGX_OK;
}

static int eig_run(mgEigen3D* E, int v1, int v2, double tol, int maxit, int* iters, int* converged, const double* host_guess) {
    mgMultiGrid3D_f64* mg = E->mg;
    const int k = E->k;
    const size_t vol = vol3_f64(E->g);
    static const double one = 1.0;
    for (int i = 0; i < k; i++) {
        if (host_guess) { /* through T_i: X_i takes the unknowns only */
            MG_TRY(put3_f64(mg, E->g, E->set[EIG_T][i], host_guess + (size_t)i * vol));
            MG_TRY(eig_combine(E, 1, E->set[EIG_T] + i, &one, 1, 1, E->set[EIG_X] + i, NULL));
        } else {
            MG_TRY(mgx3dxs_eigen_start_f64(mg->ctx, E->set[EIG_X][i], i, E->g->sizeXYZ, E->bc));
        }
    }
    int ok = 0, all_ok = 0, have_p = 0, fresh = 1;
    MG_TRY(eig_apply(E, EIG_X, EIG_AX));
    MG_TRY(eig_ritz_x(E, &ok));
    MG_REQUIRE(ok, MGX_ERR_INVALID, "Eigen: the %d start vectors are not linearly independent in the c W inner product", k);
    for (int it = 0;; it++) {
        MG_TRY(eig_residual(E, tol, &all_ok));
        if (all_ok || it >= maxit) {
            if (!fresh) { /* confirm on a freshly applied A X, after a Rayleigh-Ritz step on X alone */
                MG_TRY(eig_apply(E, EIG_X, EIG_AX));
                MG_TRY(eig_ritz_x(E, &ok));
                if (!ok) break;
                fresh = 1;
                MG_TRY(eig_residual(E, tol, &all_ok));
            }
            if (all_ok) {
                *converged = 1;
                break;
            }
            if (it >= maxit) break;
        }
        MG_TRY(eig_precond(E, v1, v2));
        MG_TRY(eig_apply(E, EIG_T, EIG_AT));
        double Y[EIG_M * EIG_K];
        int nsets = have_p ? 3 : 2;
        MG_TRY(eig_ritz(E, nsets, Y, &ok));
        if (!ok && have_p) { /* a restart: the iteration again without P */
            nsets = 2;
            MG_TRY(eig_ritz(E, nsets, Y, &ok));
        }
        if (!ok) break; /* the last good iterate: X, mu and res of this iteration's start */
        /* N1 = T Yt + P Yp, N2 = AT Yt + AP Yp: one list of inputs each, the rows k .. of Y their coefficients (up to k = 6 one
         * launch per output group) */
        double *tp[2 * EIG_K], *atp[2 * EIG_K];
        for (int i = 0; i < k; i++) {
            tp[i] = E->set[EIG_T][i], tp[k + i] = E->set[EIG_P][i];
            atp[i] = E->set[EIG_AT][i], atp[k + i] = E->set[EIG_AP][i];
        }
        MG_TRY(eig_combine(E, (nsets - 1) * k, tp, Y + k * k, k, k, E->set[EIG_N1], NULL));
        MG_TRY(eig_combine(E, (nsets - 1) * k, atp, Y + k * k, k, k, E->set[EIG_N2], NULL));
        /* X' = X Yx + N1 into T, AX' = AX Yx + N2 into AT */
        MG_TRY(eig_combine(E, k, E->set[EIG_X], Y, k, k, E->set[EIG_T], E->set[EIG_N1]));
        MG_TRY(eig_combine(E, k, E->set[EIG_AX], Y, k, k, E->set[EIG_AT], E->set[EIG_N2]));
        eig_swap(E, EIG_X, EIG_T);
        eig_swap(E, EIG_AX, EIG_AT);
        eig_swap(E, EIG_P, EIG_N1);
        eig_swap(E, EIG_AP, EIG_N2);
        have_p = 1;
        fresh = 0;
        *iters = it + 1;
    }
    return MGX_OK;
}

int mgMultiGrid3D_f64_Eigen(mgMultiGrid3D_f64* mg, int k, int v1, int v2, double tol, int maxit, double* lambda, double* res, int* iters,
                            int* converged, double* host_vectors, const double* host_guess) {
    MG_REQUIRE(mg && lambda && res && iters && converged, MGX_ERR_INVALID, "Eigen: NULL argument");
    MG_REQUIRE(k >= 1 && k <= MG_EIGEN_MAX_BLOCK, MGX_ERR_INVALID, "Eigen: k = %d outside 1 .. %d", k, MG_EIGEN_MAX_BLOCK);
    MG_REQUIRE(tol > 0 && maxit >= 1 && v1 >= 0 && v2 >= 0 && v1 + v2 >= 1, MGX_ERR_INVALID,
               "Eigen: bad arguments (tol %g, maxit %d, v1 %d, v2 %d)", tol, maxit, v1, v2);
    MG_REQUIRE(mg->grids3D && mg->grids3D[0] && mg->ctx, MGX_ERR_INVALID, "Eigen: the hierarchy has no levels");
    MG_REQUIRE(mg->numGrids >= 1 && mg->numGrids <= mg->maxGrids, MGX_ERR_INVALID, "Eigen: numGrids = %d outside [1,%d]", mg->numGrids,
               mg->maxGrids);
    MG_REQUIRE(!mg->pin, MGX_ERR_INVALID, "Eigen: a hierarchy with pinned nodes (set_pinned) is not supported");
    MG_REQUIRE(mg->layout == 1, MGX_ERR_INVALID, "Eigen: needs the x-split layout (layout = 1)");
    MG_REQUIRE(mg->residual_mode == MGX_RESIDUAL_CORRECT, MGX_ERR_INVALID, "Eigen: needs residual_mode = MGX_RESIDUAL_CORRECT");
    mgGrid3D_f64* g = mg->grids3D[0];
    MG_TRY(op_ok3_f64(mg, g, "Eigen"));
    MG_REQUIRE((size_t)k < (size_t)(g->sizeX - 2) * (size_t)(g->sizeY - 2) * (size_t)(g->sizeZ - 2), MGX_ERR_SIZE,
               "Eigen: k = %d needs a grid with more interior points", k);
    *iters = 0;
    *converged = 0;
    for (int i = 0; i < k; i++) lambda[i] = res[i] = 0.0;
    mgx_ctx* ctx = mg->ctx;
    mgEigen3D E;
    memset(&E, 0, sizeof E);
    E.mg = mg, E.g = g, E.k = k, E.bc = mg->bc;
    E.c = has_cap3_f64(mg) ? cap_of3_f64(mg, g) : NULL;
    const size_t bytes = mgx3dxs_elems_f64(g->sizeXYZ) * sizeof(double);
    int st = eig_alloc(&E);
    if (st) {
        eig_free(&E);
        return st;
    }
    const unsigned char v_rim0 = mg->v_rim_zero[0], f_rim0 = mg->f_rim_zero[0];
    st = mgx_memcpy_d2d(ctx, E.save_v, g->d_v, bytes);
    if (!st) st = mgx_memcpy_d2d(ctx, E.save_f, g->d_f, bytes);
    if (st) {
        eig_free(&E);
        return st;
    }
    st = eig_run(&E, v1, v2, tol, maxit, iters, converged, host_guess);
    if (!st) {
        for (int i = 0; i < k; i++) lambda[i] = E.mu[i] - (double)mg->shift, res[i] = E.res[i];
        for (int i = 0; !st && host_vectors && i < k; i++) st = get3_f64(mg, g, E.set[EIG_X][i], host_vectors + (size_t)i * vol3_f64(g));
    }
    /* d_v[0] and d_f[0] as they were, boundary and flags included; d_e's boundary copy no longer matches d_v's history */
    const int st2 = mgx_memcpy_d2d(ctx, g->d_v, E.save_v, bytes);
    const int st3 = mgx_memcpy_d2d(ctx, g->d_f, E.save_f, bytes);
    mg->v_rim_zero[0] = v_rim0;
    mg->f_rim_zero[0] = f_rim0;
    mg->e_rim_valid[0] = 0;
    const int st4 = mgx_ctx_sync(ctx);
    eig_free(&E);
    return st ? st : st2 ? st2 : st3 ? st3 : st4;
}
