/* mg_multigrid1d.inc -- stamped once per real type (REAL, R, MG_EXP) by mg_multigrid.c.
 * MultiGrid1D / Grid1D of the reference (N1 = NOCUDA_TESI/EQUAZIONE 1D/) as plain C on the host:
 * BASELINE.json configs[0] keeps the 1D ODE on the CPU ("plumbing, no GPU"); a 4097-point level
 * is 16-32 KB, far below anything worth a kernel launch.  This is product code (it does not use
 * oracle/); tests compare it with the oracle and the golden fixtures.
 * ODE: u' - u/(e^x+1) = f (relaxation, N1/MultiGrid1D.cpp:101); the residual keeps the
 * reference's sign quirk f - v' - v/(e^x+1) (:210, SURVEY.md fact 3). */

#define GRID MG_CAT(mgGrid1D_, R)
#define MGRID MG_CAT(mgMultiGrid1D_, R)
#define FN(name) MG_CAT3(mgMultiGrid1D_, R, _##name)

/* Grid1D::Grid1D + InitV + InitF.                                      N1/Grid1D.cpp:4-43 */
static int MG_CAT(grid1_new_, R)(int sizeX, const REAL range[2], GRID** out) {
    MG_REQUIRE(sizeX >= 3 && (sizeX - 1) % 2 == 0, MGX_ERR_SIZE, "Grid1D: size %d is not odd and >= 3", sizeX); /* :6-7 */
    MG_REQUIRE(range[1] > range[0], MGX_ERR_INVALID, "Grid1D: empty range");                              /* :10 */
    GRID* g = (GRID*)calloc(1, sizeof(GRID));
    MG_REQUIRE(g, MGX_ERR_NOMEM, "Grid1D: out of host memory");
    g->sizeX = sizeX;
    REAL x_range = range[1] - range[0];
    g->x_a = range[0];
    g->x_b = range[1];
    g->h_x = x_range / (REAL)(sizeX - 1); /* :15 */
    g->h_v = (REAL*)calloc((size_t)sizeX, sizeof(REAL)); /* reference: malloc, interior uninitialised */
    g->h_f = (REAL*)calloc((size_t)sizeX, sizeof(REAL));
    if (!g->h_v || !g->h_f) { free(g->h_v); free(g->h_f); free(g); return mg_fail(MGX_ERR_NOMEM, "Grid1D: out of host memory"); }
    g->h_v[0] = (MG_EXP(g->x_a) + g->x_a - 3) / (1 + MG_EXP(-g->x_a));          /* :32 */
    g->h_v[sizeX - 1] = (MG_EXP(g->x_b) + g->x_b - 3) / (1 + MG_EXP(-g->x_b));  /* :33 */
    for (int posX = 0; posX < sizeX; posX++) {                                   /* :38-42 */
        REAL xj = g->x_a + posX * g->h_x;
        g->h_f[posX] = MG_EXP(xj);
    }
    *out = g;
    return MGX_OK;
}

int FN(create)(int finestGridSize, const REAL range[2], MGRID** out) { /* N1/MultiGrid1D.cpp:5-31 */
    MG_REQUIRE(range && out, MGX_ERR_INVALID, "MultiGrid1D: NULL argument");
    *out = NULL;
    MG_REQUIRE(finestGridSize >= 3, MGX_ERR_SIZE, "MultiGrid1D: finest grid %d too small", finestGridSize);
    MGRID* mg = (MGRID*)calloc(1, sizeof(MGRID));
    MG_REQUIRE(mg, MGX_ERR_NOMEM, "MultiGrid1D: out of host memory");
    mg->numGrids = mg->maxGrids = mg_num_grids(finestGridSize); /* :21-22 */
    mg->grids1D = (GRID**)calloc((size_t)mg->maxGrids, sizeof(GRID*));
    if (!mg->grids1D) { free(mg); return mg_fail(MGX_ERR_NOMEM, "MultiGrid1D: out of host memory"); }
    int cur = finestGridSize;
    for (int i = 0; i < mg->maxGrids; i++) {
        int st = MG_CAT(grid1_new_, R)(cur, range, &mg->grids1D[i]);
        if (st) { FN(destroy)(mg); return st; }
        cur = mg_coarse_size(cur); /* :28 */
    }
    *out = mg;
    return MGX_OK;
}

void FN(destroy)(MGRID* mg) {
    if (!mg) return;
    if (mg->grids1D)
        for (int i = 0; i < mg->maxGrids; i++)
            if (mg->grids1D[i]) { free(mg->grids1D[i]->h_v); free(mg->grids1D[i]->h_f); free(mg->grids1D[i]); }
    free(mg->grids1D);
    free(mg);
}

int FN(Restrict)(MGRID* mg, const REAL* fine, int fsizeX, REAL* coarse, int csizeX) { /* N1/MultiGrid1D.cpp:34-58 */
    (void)mg;
    MG_REQUIRE(fine && coarse, MGX_ERR_INVALID, "Restrict: NULL");
    MG_REQUIRE(csizeX == ((fsizeX - 1) / 2 + 1), MGX_ERR_SIZE, "Restrict: coarse size %d != (%d-1)/2+1", csizeX, fsizeX); /* :36 */
    for (int cposX = 0; cposX < csizeX; cposX++) {
        if (cposX == 0 || cposX == csizeX - 1) { coarse[cposX] = fine[2 * cposX]; continue; } /* :45-49 */
        REAL C = fine[2 * cposX], E = fine[2 * cposX + 1], O = fine[2 * cposX - 1];
        coarse[cposX] = (1 / 4.0f) * (O + 2 * C + E); /* :56 */
    }
    return MGX_OK;
}

int FN(Interpolate)(MGRID* mg, REAL* fine, int fsizeX, const REAL* coarse, int csizeX) { /* N1/MultiGrid1D.cpp:60-77 */
    (void)mg;
    MG_REQUIRE(fine && coarse, MGX_ERR_INVALID, "Interpolate: NULL");
    MG_REQUIRE(csizeX == ((fsizeX - 1) / 2 + 1), MGX_ERR_SIZE, "Interpolate: coarse size %d != (%d-1)/2+1", csizeX, fsizeX);
    for (int fposX = 1; fposX < fsizeX - 1; fposX++) {
        int cposX = fposX / 2;
        if (fposX % 2 == 0) fine[fposX] = coarse[cposX];                                   /* :72 */
        else fine[fposX] = (1 / 2.0f) * (coarse[cposX] + coarse[cposX + 1]);               /* :74 */
    }
    return MGX_OK;
}

int FN(Relax)(MGRID* mg, GRID* g, int ncycles) { /* N1/MultiGrid1D.cpp:79-118 */
    (void)mg;
    MG_REQUIRE(g, MGX_ERR_INVALID, "Relax: NULL");
    REAL* h_v = g->h_v;
    const REAL* h_f = g->h_f;
    const REAL h_x = g->h_x, x_a = g->x_a;
    const int sizeX = g->sizeX;
    for (int k = 0; k < ncycles; k++)
        for (int colour = 0; colour < 2; colour++) /* red = even (:94), black = odd (:108) */
            for (int posX = 1 + (colour == 0); posX < sizeX - 1; posX += 2) {
                REAL xj = x_a + posX * h_x;
                h_v[posX] = (h_v[posX + 1] * (MG_EXP(xj) + 1) - h_f[posX] * h_x * (MG_EXP(xj) + 1)) / (MG_EXP(xj) + 1 + h_x); /* :101/:114 */
            }
    return MGX_OK;
}

int FN(setToValue)(MGRID* mg, REAL* grid, int sizeX, REAL value, int modifyBoundaries) { /* N1/MultiGrid1D.cpp:120-130 */
    (void)mg;
    MG_REQUIRE(grid, MGX_ERR_INVALID, "setToValue: NULL");
    const int lo = modifyBoundaries ? 0 : 1;
    for (int posX = lo; posX < sizeX - lo; posX++) grid[posX] = value;
    return MGX_OK;
}

/* writes into the caller's array (the reference returns a malloc it never frees, :199) */
int FN(CalculateResidual)(MGRID* mg, GRID* g, REAL* residual) { /* N1/MultiGrid1D.cpp:190-214 */
    (void)mg;
    MG_REQUIRE(g && residual, MGX_ERR_INVALID, "CalculateResidual: NULL");
    const int sizeX = g->sizeX;
    for (int posX = 0; posX < sizeX; posX++) {
        if (posX == 0 || posX == sizeX - 1) { residual[posX] = 0; continue; } /* :204-208 */
        REAL xj = g->x_a + posX * g->h_x;
        residual[posX] = g->h_f[posX] - (g->h_v[posX + 1] - g->h_v[posX]) / g->h_x - g->h_v[posX] / (MG_EXP(xj) + 1); /* :210 */
    }
    return MGX_OK;
}

int FN(ApplyCorrection)(MGRID* mg, REAL* fine, int fineSizeX, const REAL* fine_error, int errorSizeX) { /* N1/MultiGrid1D.cpp:177-188 */
    (void)mg;
    MG_REQUIRE(fine && fine_error, MGX_ERR_INVALID, "ApplyCorrection: NULL");
    MG_REQUIRE(fineSizeX == errorSizeX, MGX_ERR_SIZE, "ApplyCorrection: size %d != %d", fineSizeX, errorSizeX); /* :179 */
    for (int posX = 1; posX < fineSizeX - 1; posX++) fine[posX] = fine[posX] + fine_error[posX]; /* :186 */
    return MGX_OK;
}

int FN(VCycle)(MGRID* mg, int gridID, int v1, int v2) { /* N1/MultiGrid1D.cpp:150-175 */
    MG_REQUIRE(mg && mg->numGrids >= 1 && mg->numGrids <= mg->maxGrids, MGX_ERR_INVALID, "VCycle: numGrids = %d outside [1,%d]",
               mg ? mg->numGrids : -1, mg ? mg->maxGrids : -1);
    MG_REQUIRE(gridID >= 0 && gridID < mg->numGrids, MGX_ERR_INVALID, "VCycle: bad gridID %d", gridID);
    GRID* fine = mg->grids1D[gridID];
    MG_TRY(FN(Relax)(mg, fine, v1)); /* :153 */
    if (gridID != mg->numGrids - 1) {
        GRID* coarse = mg->grids1D[gridID + 1];
        REAL* scratch = (REAL*)malloc((size_t)fine->sizeX * sizeof(REAL));
        MG_REQUIRE(scratch, MGX_ERR_NOMEM, "VCycle: out of host memory");
        int st = FN(CalculateResidual)(mg, fine, scratch);                                  /* :156 */
        if (!st) st = FN(Restrict)(mg, scratch, fine->sizeX, coarse->h_f, coarse->sizeX);   /* :159 */
        if (!st) st = FN(setToValue)(mg, coarse->h_v, coarse->sizeX, (REAL)0, 1);           /* :162 */
        if (!st) st = FN(VCycle)(mg, gridID + 1, v1, v2);                                   /* :164 */
        if (!st) st = FN(Interpolate)(mg, scratch, fine->sizeX, coarse->h_v, coarse->sizeX);/* :170 */
        if (!st) st = FN(ApplyCorrection)(mg, fine->h_v, fine->sizeX, scratch, fine->sizeX);/* :172 */
        free(scratch);
        if (st) return st;
    }
    return FN(Relax)(mg, fine, v2); /* :174 */
}

int FN(FullMultiGridVCycle)(MGRID* mg, int gridID, int v0, int v1, int v2) { /* N1/MultiGrid1D.cpp:132-148 */
    MG_REQUIRE(mg && mg->numGrids >= 1 && mg->numGrids <= mg->maxGrids, MGX_ERR_INVALID, "FMG: numGrids = %d outside [1,%d]",
               mg ? mg->numGrids : -1, mg ? mg->maxGrids : -1);
    MG_REQUIRE(gridID >= 0 && gridID < mg->numGrids, MGX_ERR_INVALID, "FMG: bad gridID %d", gridID);
    GRID* fine = mg->grids1D[gridID];
    if (gridID != mg->numGrids - 1) {
        GRID* coarse = mg->grids1D[gridID + 1];
        MG_TRY(FN(Restrict)(mg, fine->h_f, fine->sizeX, coarse->h_f, coarse->sizeX));    /* :138 */
        MG_TRY(FN(FullMultiGridVCycle)(mg, gridID + 1, v0, v1, v2));                     /* :139 */
        MG_TRY(FN(Interpolate)(mg, fine->h_v, fine->sizeX, coarse->h_v, coarse->sizeX)); /* :140 */
    } else {
        MG_TRY(FN(setToValue)(mg, fine->h_v, fine->sizeX, (REAL)0, 0)); /* :144 */
    }
    for (int i = 0; i < v0; i++) MG_TRY(FN(VCycle)(mg, gridID, v1, v2)); /* :146-147 */
    return MGX_OK;
}

int MG_CAT(mg1d_solve_, R)(REAL* grid, const REAL* rhs, int sizeX, const REAL range[2], int nlevels, int fmg, int v0,
                           int v1, int v2, int ncycles) {
    MG_REQUIRE(grid && rhs && range, MGX_ERR_INVALID, "mg1d_solve: NULL argument");
    MGRID* mg = NULL;
    MG_TRY(FN(create)(sizeX, range, &mg));
    int st = MGX_OK;
    if (nlevels > 0) {
        if (nlevels > mg->maxGrids) st = mg_fail(MGX_ERR_SIZE, "mg1d_solve: nlevels %d > %d", nlevels, mg->maxGrids);
        else mg->numGrids = nlevels;
    }
    if (!st) {
        memcpy(mg->grids1D[0]->h_v, grid, (size_t)sizeX * sizeof(REAL));
        memcpy(mg->grids1D[0]->h_f, rhs, (size_t)sizeX * sizeof(REAL));
        if (fmg) st = FN(FullMultiGridVCycle)(mg, 0, v0, v1, v2);
        else for (int i = 0; i < ncycles && !st; i++) st = FN(VCycle)(mg, 0, v1, v2);
    }
    if (!st) memcpy(grid, mg->grids1D[0]->h_v, (size_t)sizeX * sizeof(REAL));
    FN(destroy)(mg);
    return st;
}

#undef GRID
#undef MGRID
#undef FN
