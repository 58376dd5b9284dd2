/* mg_multigrid2d.inc -- stamped once per real type (REAL, R) by mg_multigrid.c.
 * Control flow of MultiGrid2D / Grid2D (N2 = NOCUDA_TESI/PDE Lyapunov 2D/); arithmetic on grid
 * values happens in the HIP kernels behind mgx.h, except the boundary values of InitV which are
 * evaluated on the host in REAL exactly like Grid2D::InitV (N2/Grid2D.cpp:50-68). */

#define GRID MG_CAT(mgGrid2D_, R)
#define MGRID MG_CAT(mgMultiGrid2D_, R)
#define FN(name) MG_CAT3(mgMultiGrid2D_, R, _##name)
#define MGX(name) MG_CAT3(mgx2d_, name##_, R)

static size_t MG_CAT(vol2_, R)(const GRID* g) { return (size_t)g->sizeX * g->sizeY; }

/* Grid2D::Grid2D.                                                     N2/Grid2D.cpp:4-42 */
static int MG_CAT(grid2_new_, R)(mgx_ctx* ctx, const int sizeXY[2], const REAL range[4], GRID** out) {
    for (int d = 0; d < 2; d++)
        MG_REQUIRE(sizeXY[d] >= 3 && (sizeXY[d] - 1) % 2 == 0, MGX_ERR_SIZE, "Grid2D: size[%d] = %d is not odd and >= 3", d,
                   sizeXY[d]); /* :11-15 */
    MG_REQUIRE(range[1] > range[0] && range[3] > range[2], MGX_ERR_INVALID, "Grid2D: empty range"); /* :21-22 */
    GRID* g = (GRID*)calloc(1, sizeof(GRID));
    MG_REQUIRE(g, MGX_ERR_NOMEM, "Grid2D: out of host memory");
    g->sizeX = g->sizeXY[0] = sizeXY[0];
    g->sizeY = g->sizeXY[1] = sizeXY[1];
    REAL x_range = range[1] - range[0]; /* :24-25 */
    REAL y_range = range[3] - range[2];
    g->x_a = range[0]; g->x_b = range[1];
    g->y_a = range[2]; g->y_b = range[3];
    g->h_x = x_range / (REAL)(g->sizeX - 1); /* :34-35 */
    g->h_y = y_range / (REAL)(g->sizeY - 1);
    const size_t bytes = MG_CAT(vol2_, R)(g) * sizeof(REAL);
    int st;
    if ((st = mgx_malloc(ctx, bytes, (void**)&g->d_v)) || (st = mgx_malloc(ctx, bytes, (void**)&g->d_f)) ||
        (st = mgx_malloc(ctx, bytes, (void**)&g->d_r)) || (st = mgx_malloc(ctx, bytes, (void**)&g->d_e))) {
        mgx_free(ctx, g->d_v); mgx_free(ctx, g->d_f); mgx_free(ctx, g->d_r); mgx_free(ctx, g->d_e);
        free(g);
        return st;
    }
    *out = g;
    return MGX_OK;
}

static void MG_CAT(grid2_free_, R)(mgx_ctx* ctx, GRID* g) {
    if (!g) return;
    mgx_free(ctx, g->d_v); mgx_free(ctx, g->d_f); mgx_free(ctx, g->d_r); mgx_free(ctx, g->d_e);
    free(g->h_v); free(g->h_f);
    free(g);
}

/* Grid2D::InitV: boundary = 2*xj*xj-4*xj*yi+2*yi*yi in REAL, interior 0.   N2/Grid2D.cpp:50-68
 * On the device (mgx2d_init_v): products and sums only, same bits as the host loop, no O(n^2) host pass and no upload. */
int FN(InitV)(MGRID* mg, int gridID) {
    MG_REQUIRE(mg && gridID >= 0 && gridID < mg->maxGrids, MGX_ERR_INVALID, "InitV: bad gridID %d", gridID);
    GRID* g = mg->grids2D[gridID];
    const REAL h[2] = {g->h_x, g->h_y}, a[2] = {g->x_a, g->y_a};
    return MG_CAT(mgx2d_init_v_, R)(mg->ctx, g->d_v, g->sizeXY, h, a);
}

/* Grid2D::InitF: f = 0.                                               N2/Grid2D.cpp:70-80 */
int FN(InitF)(MGRID* mg, int gridID) {
    MG_REQUIRE(mg && gridID >= 0 && gridID < mg->maxGrids, MGX_ERR_INVALID, "InitF: bad gridID %d", gridID);
    GRID* g = mg->grids2D[gridID];
    return mgx_memset_zero(mg->ctx, g->d_f, MG_CAT(vol2_, R)(g) * sizeof(REAL));
}

/* MultiGrid2D::MultiGrid2D + InitGrids + InitA.                       N2/MultiGrid2D.cpp:5-60
 * A is the 2x2 matrix, row major (A_size must be 2; the reference copies A_size*A_size values). */
int FN(create)(mgx_ctx* ctx, const int finestGridSizeXY[2], const REAL range[4], const REAL* A, int A_size, int alfa,
               MGRID** out) {
    MG_REQUIRE(ctx && finestGridSizeXY && range && A && out, MGX_ERR_INVALID, "MultiGrid2D: NULL argument");
    MG_REQUIRE(A_size == 2, MGX_ERR_INVALID, "MultiGrid2D: A_size = %d (must be 2)", A_size);
    *out = NULL;
    int minSize = finestGridSizeXY[0]; /* :25-27 */
    if (finestGridSizeXY[1] < minSize) minSize = finestGridSizeXY[1];
    MG_REQUIRE(minSize >= 3, MGX_ERR_SIZE, "MultiGrid2D: finest grid %d too small", minSize);
    MGRID* mg = (MGRID*)calloc(1, sizeof(MGRID));
    MG_REQUIRE(mg, MGX_ERR_NOMEM, "MultiGrid2D: out of host memory");
    mg->ctx = ctx;
    mg->fuse = 2;
    mg->smoother = 0;
    mg->omega = (REAL)2 / (REAL)3;
    mg->alfa = alfa; /* InitA :47-59 */
    mg->sizeA = A_size;
    for (int i = 0; i < 4; i++) mg->matrixA[i] = A[i];
    mg->numGrids = mg->maxGrids = mg_num_grids(minSize); /* :29-30 */
    mg->grids2D = (GRID**)calloc((size_t)mg->maxGrids, sizeof(GRID*));
    if (!mg->grids2D) { free(mg); return mg_fail(MGX_ERR_NOMEM, "MultiGrid2D: out of host memory"); }
    int cur[2] = {finestGridSizeXY[0], finestGridSizeXY[1]};
    for (int i = 0; i < mg->maxGrids; i++) {
        int st = MG_CAT(grid2_new_, R)(ctx, cur, range, &mg->grids2D[i]);
        if (!st) st = FN(InitV)(mg, i);
        if (!st) st = FN(InitF)(mg, i);
        if (st) { FN(destroy)(mg); return st; }
        for (int d = 0; d < 2; d++) cur[d] = mg_coarse_size(cur[d]); /* :36-37 */
    }
    *out = mg;
    return MGX_OK;
}

void FN(destroy)(MGRID* mg) {
    if (!mg) return;
    for (int i = 0; i < MG_MAX_LEVELS; i++)
        if (mg->graph_exec[i]) mgx_graph_destroy(mg->ctx, mg->graph_exec[i]);
    if (mg->grids2D)
        for (int i = 0; i < mg->maxGrids; i++) MG_CAT(grid2_free_, R)(mg->ctx, mg->grids2D[i]);
    free(mg->grids2D);
    free(mg);
}

int FN(Restrict)(MGRID* mg, const REAL* fine, const int fsizeXY[2], REAL* coarse, const int csizeXY[2]) {
    MG_REQUIRE(mg, MGX_ERR_INVALID, "Restrict: NULL");
    return MGX(restrict)(mg->ctx, fine, fsizeXY, coarse, csizeXY);
}

int FN(Interpolate)(MGRID* mg, REAL* fine, const int fsizeXY[2], const REAL* coarse, const int csizeXY[2]) {
    MG_REQUIRE(mg, MGX_ERR_INVALID, "Interpolate: NULL");
    return MGX(interpolate)(mg->ctx, fine, fsizeXY, coarse, csizeXY);
}

int FN(Relax)(MGRID* mg, GRID* g, int ncycles) {
    MG_REQUIRE(mg && g, MGX_ERR_INVALID, "Relax: NULL");
    const REAL h[2] = {g->h_x, g->h_y}, a[2] = {g->x_a, g->y_a};
    if (mg->smoother == 1)
        return MGX(jacobi)(mg->ctx, g->d_v, g->d_e, g->d_f, g->sizeXY, h, a, mg->matrixA, mg->alfa, mg->omega, ncycles);
    if (mg->fuse >= 2 && ncycles >= 2 && (g->sizeX > 65 || g->sizeY > 65)) {
        /* long Relax calls on levels that do not fit one workgroup (the thesis runs FMG(2, 500, 500)): up to four sweeps
         * per launch through the tiled cache-resident kernel (out of place, d_v <-> d_e), in an EVEN number of launches so
         * that the result is back in d_v and no pointer changes hands (also under graph capture).  Bit-identical to the
         * launch-per-colour path (tests/test_gpu_parity.py). */
        int nl = (ncycles + 3) / 4;
        nl += nl & 1;
        REAL *src = g->d_v, *dst = g->d_e;
        int done = 0;
        for (int l = 0; l < nl; l++) {
            const int upto = (int)((long long)ncycles * (l + 1) / nl); /* sweeps finished after launch l: steps of <= 4 */
            MG_TRY(MGX(relax_residual_restrict)(mg->ctx, src, dst, g->d_f, g->sizeXY, h, a, mg->matrixA, mg->alfa, upto - done, 0, NULL,
                                                NULL));
            done = upto;
            REAL* t = src; src = dst; dst = t;
        }
        return MGX_OK;
    }
    return MGX(relax)(mg->ctx, g->d_v, g->d_f, g->sizeXY, h, a, mg->matrixA, mg->alfa, ncycles);
}

int FN(setToValue)(MGRID* mg, REAL* grid, const int sizeXY[2], REAL value, int modifyBoundaries) {
    MG_REQUIRE(mg, MGX_ERR_INVALID, "setToValue: NULL");
    return MGX(set)(mg->ctx, grid, sizeXY, value, modifyBoundaries);
}

int FN(CalculateResidual)(MGRID* mg, GRID* g, REAL** residual) {
    MG_REQUIRE(mg && g && residual, MGX_ERR_INVALID, "CalculateResidual: NULL");
    const REAL h[2] = {g->h_x, g->h_y}, a[2] = {g->x_a, g->y_a};
    MG_TRY(MGX(residual)(mg->ctx, g->d_v, g->d_f, g->d_r, g->sizeXY, h, a, mg->matrixA, mg->alfa));
    *residual = g->d_r;
    return MGX_OK;
}

int FN(ApplyCorrection)(MGRID* mg, REAL* fine, const int fsizeXY[2], const REAL* error, const int esizeXY[2]) {
    MG_REQUIRE(mg, MGX_ERR_INVALID, "ApplyCorrection: NULL");
    return MGX(apply_correction)(mg->ctx, fine, fsizeXY, error, esizeXY);
}

/* use_graph: see mg_multigrid3d.inc.  The body reads no rim flags in 2D. */
static int MG_CAT(vcycle_graph2_, R)(MGRID* mg, int gridID, int v1, int v2, int (*body)(MGRID*, int, int, int)) {
    mgGraphState s;
    memset(&s, 0, sizeof s);
    s.kind = MG_GRAPH_2D;
    s.gridID = gridID; s.v1 = v1; s.v2 = v2; s.numGrids = mg->numGrids;
    s.fuse = mg->fuse; s.smoother = mg->smoother; s.alfa = mg->alfa;
    s.omega_bits = mg_real_bits(&mg->omega, sizeof(REAL));
    for (int k = 0; k < 4; k++) s.matrixA_bits[k] = mg_real_bits(&mg->matrixA[k], sizeof(REAL));
    MG_TRY(mgx_ctx_generation(mg->ctx, &s.generation));
    mgGraphRec rec;
    mg_graph_record(&s, &rec);
    if (!mg->graph_exec[gridID] || !mg_graph_rec_equal(&mg->graph_rec[gridID], &rec)) {
        if (mg->graph_exec[gridID]) MG_TRY(mgx_graph_destroy(mg->ctx, mg->graph_exec[gridID]));
        mg->graph_exec[gridID] = NULL;
        MG_TRY(mgx_graph_begin(mg->ctx));
        mg->capturing = 1;
        const int st = body(mg, gridID, v1, v2);
        mg->capturing = 0;
        void* exec = NULL;
        const int st2 = mgx_graph_end(mg->ctx, &exec);
        if (st) {
            if (exec) mgx_graph_destroy(mg->ctx, exec);
            return st;
        }
        MG_TRY(st2);
        mg->graph_exec[gridID] = exec;
        mg->graph_rec[gridID] = rec;
    }
    return mgx_graph_launch(mg->ctx, mg->graph_exec[gridID]);
}

/* fuse == 2 (default): the cycle runs on the cache-resident kernels of mgx.h -- per level ONE launch on the way down
 * (Relax(v1) + CalculateResidual + Restrict, :317-323) and ONE on the way up (Interpolate + ApplyCorrection + Relax(v2),
 * :333-338), both out of place (d_v and the error scratch d_e of the level swap roles, twice per cycle), and ONE launch
 * for all levels that fit into the LDS of a workgroup together (65^2 and below).  The coarse error is never zeroed in
 * memory (:326): the way-down kernel of a coarse level takes its input as zeros (`v_zero`).  Bit-identical to fuse = 1 / 0. */
static int MG_CAT(vcycle_fast2_, R)(MGRID* mg, int gridID, int v1, int v2, int v_zero) {
    GRID* fine = mg->grids2D[gridID];
    const REAL a[2] = {fine->x_a, fine->y_a};
    const int nlev = mg->numGrids - gridID;
    if (nlev <= 8) { /* the rest of the hierarchy in one workgroup? */
        int n[16];
        REAL h[16];
        REAL *v[8], *f[8];
        for (int l = 0; l < nlev; l++) {
            GRID* g = mg->grids2D[gridID + l];
            n[2 * l] = g->sizeX; n[2 * l + 1] = g->sizeY;
            h[2 * l] = g->h_x; h[2 * l + 1] = g->h_y;
            v[l] = g->d_v; f[l] = g->d_f;
        }
        if (MGX(vcycle_tail_fits)(mg->ctx, nlev, n))
            return MGX(vcycle_tail)(mg->ctx, nlev, v, f, n, h, a, mg->matrixA, mg->alfa, v1, v2, v_zero);
    }
    const REAL h[2] = {fine->h_x, fine->h_y};
    if (gridID == mg->numGrids - 1) { /* the cycle ends on a level too large for the tail kernel: Relax(v1); Relax(v2) */
        MG_TRY(MGX(relax_residual_restrict)(mg->ctx, fine->d_v, fine->d_e, fine->d_f, fine->sizeXY, h, a, mg->matrixA, mg->alfa, v1,
                                            v_zero, NULL, NULL)); /* :317 */
        MG_TRY(MGX(relax_residual_restrict)(mg->ctx, fine->d_e, fine->d_v, fine->d_f, fine->sizeXY, h, a, mg->matrixA, mg->alfa, v2, 0,
                                            NULL, NULL)); /* :338 */
        return MGX_OK;
    }
    GRID* coarse = mg->grids2D[gridID + 1];
    REAL* t;
    MG_TRY(MGX(relax_residual_restrict)(mg->ctx, fine->d_v, fine->d_e, fine->d_f, fine->sizeXY, h, a, mg->matrixA, mg->alfa, v1, v_zero,
                                        coarse->d_f, coarse->sizeXY)); /* :317-323 */
    t = fine->d_v; fine->d_v = fine->d_e; fine->d_e = t;
    MG_TRY(MG_CAT(vcycle_fast2_, R)(mg, gridID + 1, v1, v2, 1)); /* :326-328 */
    MG_TRY(MGX(interpolate_correct_relax)(mg->ctx, fine->d_v, fine->d_e, fine->d_f, fine->sizeXY, h, a, mg->matrixA, mg->alfa,
                                          coarse->d_v, coarse->sizeXY, v2)); /* :333-338 */
    t = fine->d_v; fine->d_v = fine->d_e; fine->d_e = t;
    return MGX_OK;
}

/* MultiGrid2D::VCycle.                                                N2/MultiGrid2D.cpp:314-340 */
int FN(VCycle)(MGRID* mg, int gridID, int v1, int v2) {
    MG_REQUIRE(mg && mg->numGrids >= 1 && mg->numGrids <= mg->maxGrids, MGX_ERR_INVALID, "VCycle: numGrids = %d outside [1,%d]",
               mg ? mg->numGrids : -1, mg ? mg->maxGrids : -1);
    MG_REQUIRE(gridID >= 0 && gridID < mg->numGrids, MGX_ERR_INVALID, "VCycle: bad gridID %d", gridID);
    if (mg->use_graph && !mg->capturing) return MG_CAT(vcycle_graph2_, R)(mg, gridID, v1, v2, FN(VCycle));
    if (mg->fuse >= 2 && mg->smoother == 0 && v1 >= 0 && v2 >= 0 && v1 <= 4 && v2 <= 4) /* the tile halo covers 4 sweeps */
        return MG_CAT(vcycle_fast2_, R)(mg, gridID, v1, v2, 0);
    GRID* fine = mg->grids2D[gridID];
    MG_TRY(FN(Relax)(mg, fine, v1)); /* :317 */
    if (gridID != mg->numGrids - 1) {
        GRID* coarse = mg->grids2D[gridID + 1];
        if (mg->fuse) {
            const REAL h[2] = {fine->h_x, fine->h_y}, a[2] = {fine->x_a, fine->y_a};
            MG_TRY(MGX(residual_restrict)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXY, h, a, mg->matrixA, mg->alfa, coarse->d_f,
                                          coarse->sizeXY)); /* :320-323 */
        } else {
            REAL* residual = NULL;
            MG_TRY(FN(CalculateResidual)(mg, fine, &residual));                                   /* :320 */
            MG_TRY(FN(Restrict)(mg, residual, fine->sizeXY, coarse->d_f, coarse->sizeXY));        /* :323 */
        }
        MG_TRY(FN(setToValue)(mg, coarse->d_v, coarse->sizeXY, (REAL)0, 1));                  /* :326 */
        MG_TRY(FN(VCycle)(mg, gridID + 1, v1, v2));                                           /* :328 */
        if (mg->fuse) {
            MG_TRY(MGX(interpolate_correct)(mg->ctx, fine->d_v, fine->sizeXY, coarse->d_v, coarse->sizeXY)); /* :333-335 */
        } else {
            MG_TRY(FN(Interpolate)(mg, fine->d_e, fine->sizeXY, coarse->d_v, coarse->sizeXY));    /* :333 */
            MG_TRY(FN(ApplyCorrection)(mg, fine->d_v, fine->sizeXY, fine->d_e, fine->sizeXY));    /* :335 */
        }
    }
    return FN(Relax)(mg, fine, v2); /* :338 */
}

/* MultiGrid2D::FullMultiGridVCycle.                                   N2/MultiGrid2D.cpp:296-312 */
int FN(FullMultiGridVCycle)(MGRID* mg, int gridID, int v0, int v1, int v2) {
    MG_REQUIRE(mg && mg->numGrids >= 1 && mg->numGrids <= mg->maxGrids, MGX_ERR_INVALID, "FMG: numGrids = %d outside [1,%d]",
               mg ? mg->numGrids : -1, mg ? mg->maxGrids : -1);
    MG_REQUIRE(gridID >= 0 && gridID < mg->numGrids, MGX_ERR_INVALID, "FMG: bad gridID %d", gridID);
    GRID* fine = mg->grids2D[gridID];
    if (gridID != mg->numGrids - 1) {
        GRID* coarse = mg->grids2D[gridID + 1];
        MG_TRY(FN(Restrict)(mg, fine->d_f, fine->sizeXY, coarse->d_f, coarse->sizeXY));    /* :302 */
        MG_TRY(FN(FullMultiGridVCycle)(mg, gridID + 1, v0, v1, v2));                       /* :303 */
        MG_TRY(FN(Interpolate)(mg, fine->d_v, fine->sizeXY, coarse->d_v, coarse->sizeXY)); /* :304 */
    } else {
        MG_TRY(FN(setToValue)(mg, fine->d_v, fine->sizeXY, (REAL)0, 0)); /* :308 */
    }
    for (int i = 0; i < v0; i++) MG_TRY(FN(VCycle)(mg, gridID, v1, v2)); /* :310-311 */
    return MGX_OK;
}

static int MG_CAT(lvl2_, R)(MGRID* mg, int gridID, GRID** g) {
    MG_REQUIRE(mg && gridID >= 0 && gridID < mg->maxGrids, MGX_ERR_INVALID, "bad gridID %d", gridID);
    *g = mg->grids2D[gridID];
    return MGX_OK;
}

int FN(upload_v)(MGRID* mg, int gridID, const REAL* host) {
    GRID* g = NULL; MG_TRY(MG_CAT(lvl2_, R)(mg, gridID, &g));
    return mgx_memcpy_h2d(mg->ctx, g->d_v, host, MG_CAT(vol2_, R)(g) * sizeof(REAL));
}
int FN(upload_f)(MGRID* mg, int gridID, const REAL* host) {
    GRID* g = NULL; MG_TRY(MG_CAT(lvl2_, R)(mg, gridID, &g));
    return mgx_memcpy_h2d(mg->ctx, g->d_f, host, MG_CAT(vol2_, R)(g) * sizeof(REAL));
}
int FN(download_v)(MGRID* mg, int gridID, REAL* host) {
    GRID* g = NULL; MG_TRY(MG_CAT(lvl2_, R)(mg, gridID, &g));
    const size_t bytes = MG_CAT(vol2_, R)(g) * sizeof(REAL);
    if (!host) {
        if (!g->h_v) g->h_v = (REAL*)malloc(bytes);
        MG_REQUIRE(g->h_v, MGX_ERR_NOMEM, "download_v: out of host memory");
        host = g->h_v;
    }
    return mgx_memcpy_d2h(mg->ctx, host, g->d_v, bytes);
}
int FN(download_f)(MGRID* mg, int gridID, REAL* host) {
    GRID* g = NULL; MG_TRY(MG_CAT(lvl2_, R)(mg, gridID, &g));
    const size_t bytes = MG_CAT(vol2_, R)(g) * sizeof(REAL);
    if (!host) {
        if (!g->h_f) g->h_f = (REAL*)malloc(bytes);
        MG_REQUIRE(g->h_f, MGX_ERR_NOMEM, "download_f: out of host memory");
        host = g->h_f;
    }
    return mgx_memcpy_d2h(mg->ctx, host, g->d_f, bytes);
}

int FN(MeanAbsoluteError)(MGRID* mg, int gridID, double* mean) {
    GRID* g = NULL; MG_TRY(MG_CAT(lvl2_, R)(mg, gridID, &g));
    MG_REQUIRE(mean, MGX_ERR_INVALID, "MeanAbsoluteError: NULL");
    const REAL h[2] = {g->h_x, g->h_y}, a[2] = {g->x_a, g->y_a};
    return MGX(mean_abs_error)(mg->ctx, g->d_v, g->sizeXY, h, a, mean);
}

int MG_CAT(mg2d_solve_, R)(mgx_ctx* ctx, REAL* grid, const REAL* rhs, const int sizeXY[2], const REAL range[4],
                           const REAL A[4], int alfa, int nlevels, int fmg, int v0, int v1, int v2, int ncycles) {
    MG_REQUIRE(ctx && grid && rhs && sizeXY && range && A, MGX_ERR_INVALID, "mg2d_solve: NULL argument");
    MGRID* mg = NULL;
    MG_TRY(FN(create)(ctx, sizeXY, range, A, 2, alfa, &mg));
    int st = MGX_OK;
    if (nlevels > 0) {
        if (nlevels > mg->maxGrids) st = mg_fail(MGX_ERR_SIZE, "mg2d_solve: nlevels %d > %d", nlevels, mg->maxGrids);
        else mg->numGrids = nlevels;
    }
    if (!st) st = FN(upload_v)(mg, 0, grid);
    if (!st) st = FN(upload_f)(mg, 0, rhs);
    if (!st) {
        if (fmg) st = FN(FullMultiGridVCycle)(mg, 0, v0, v1, v2);
        else for (int i = 0; i < ncycles && !st; i++) st = FN(VCycle)(mg, 0, v1, v2);
    }
    if (!st) st = FN(download_v)(mg, 0, grid);
    FN(destroy)(mg);
    return st;
}

#undef GRID
#undef MGRID
#undef FN
#undef MGX
