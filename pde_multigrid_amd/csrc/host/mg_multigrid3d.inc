/* mg_multigrid3d.inc -- stamped once per real type (REAL, R) by mg_multigrid.c.
 * C restatement of the CONTROL FLOW of MultiGrid3D / Grid3D (N3 = NOCUDA_TESI/POISSON_3D(TESI)/);
 * all arithmetic on grid values happens in the HIP kernels behind mgx.h. */

#define GRID MG_CAT(mgGrid3D_, R)
#define MGRID MG_CAT(mgMultiGrid3D_, R)
#define FN(name) MG_CAT3(mgMultiGrid3D_, R, _##name)
/* operator of the hierarchy's device layout (mg->layout: 0 = natural, 1 = x-split) */
#define MGXL(mg, name) ((mg)->layout ? MG_CAT3(mgx3dxs_, name##_, R) : MG_CAT3(mgx3d_, name##_, R))

static size_t MG_CAT(vol3_, R)(const GRID* g) { return (size_t)g->sizeX * g->sizeY * g->sizeZ; }
/* elements of one device array of the level: the x-split layout pads its rows to cache lines */
static size_t MG_CAT(dvol3_, R)(int layout, const GRID* g) {
    return layout ? MG_CAT(mgx3dxs_elems_, R)(g->sizeXYZ) : MG_CAT(vol3_, R)(g);
}

/* Grid3D::Grid3D geometry part.                                   N3/Grid3D.cpp:4-53 */
static int MG_CAT(grid3_new_, R)(mgx_ctx* ctx, int layout, const int sizeXYZ[3], const REAL range[6], GRID** out) {
    /* the reference asserts equal sizes (N3/Grid3D.cpp:10-11); the kernels do not need that, nor 2^k+1: every axis
     * has to be odd and >= 3 (every level of a hierarchy, so that it restricts onto the next one), nothing more. */
    for (int d = 0; d < 3; d++)
        MG_REQUIRE(sizeXYZ[d] >= 3 && (sizeXYZ[d] - 1) % 2 == 0, MGX_ERR_SIZE, "Grid3D: size[%d] = %d is not odd and >= 3", d,
                   sizeXYZ[d]); /* :13-20 */
    MG_REQUIRE(range[1] > range[0] && range[3] > range[2] && range[5] > range[4], MGX_ERR_INVALID,
               "Grid3D: empty range"); /* :27-29 */
    GRID* g = (GRID*)calloc(1, sizeof(GRID));
    MG_REQUIRE(g, MGX_ERR_NOMEM, "Grid3D: out of host memory");
    g->sizeX = g->sizeXYZ[0] = sizeXYZ[0];
    g->sizeY = g->sizeXYZ[1] = sizeXYZ[1];
    g->sizeZ = g->sizeXYZ[2] = sizeXYZ[2];
    REAL x_range = range[1] - range[0]; /* :31-33 */
    REAL y_range = range[3] - range[2];
    REAL z_range = range[5] - range[4];
    g->x_a = range[0]; g->x_b = range[1];
    g->y_a = range[2]; g->y_b = range[3];
    g->z_a = range[4]; g->z_b = range[5];
    g->h_x = x_range / (REAL)(g->sizeX - 1); /* :43-45 */
    g->h_y = y_range / (REAL)(g->sizeY - 1);
    g->h_z = z_range / (REAL)(g->sizeZ - 1);
    const size_t bytes = MG_CAT(dvol3_, R)(layout, g) * sizeof(REAL);
    int st;
    if ((st = mgx_malloc(ctx, bytes, (void**)&g->d_v)) || (st = mgx_malloc(ctx, bytes, (void**)&g->d_f)) ||
        (st = mgx_malloc(ctx, bytes, (void**)&g->d_r)) || (st = mgx_malloc(ctx, bytes, (void**)&g->d_e)) ||
        /* pad entries of the x-split layout are never written but by whole-array zero fills: zero them once */
        (st = mgx_memset_zero(ctx, g->d_v, bytes)) || (st = mgx_memset_zero(ctx, g->d_f, bytes)) ||
        (st = mgx_memset_zero(ctx, g->d_r, bytes)) || (st = mgx_memset_zero(ctx, g->d_e, bytes))) {
        mgx_free(ctx, g->d_v); mgx_free(ctx, g->d_f); mgx_free(ctx, g->d_r); mgx_free(ctx, g->d_e);
        free(g);
        return st;
    }
    *out = g;
    return MGX_OK;
}

static void MG_CAT(grid3_free_, R)(mgx_ctx* ctx, GRID* g) {
    if (!g) return;
    mgx_free(ctx, g->d_v); mgx_free(ctx, g->d_f); mgx_free(ctx, g->d_r); mgx_free(ctx, g->d_e);
    mgx_free(ctx, g->d_a);
    free(g->h_v); free(g->h_f);
    free(g);
}

/* Grid3D::InitV: v = 0 on the boundary.  The reference leaves the interior uninitialised
 * (malloc); here the whole array is zeroed.                           N3/Grid3D.cpp:61-76 */
int FN(InitV)(MGRID* mg, int gridID) {
    MG_REQUIRE(mg && gridID >= 0 && gridID < mg->maxGrids, MGX_ERR_INVALID, "InitV: bad gridID %d", gridID);
    GRID* g = mg->grids3D[gridID];
    MG_TRY(mgx_memset_zero(mg->ctx, g->d_v, MG_CAT(dvol3_, R)(mg->layout, g) * sizeof(REAL)));
    mg->v_rim_zero[gridID] = 1;
    mg->e_rim_valid[gridID] = 0;
    return MGX_OK;
}

/* Grid3D::InitF: f = -3*PI*PI*sin(PI*x)*sin(PI*y)*sin(PI*z) evaluated in double, left to right,
 * with x = x_a + posX*h_x in REAL (N3/Grid3D.cpp:88-92).  The three sines are tabulated on the
 * host (same libm as the reference) and the products are formed on the device in the same order. */
int FN(InitF)(MGRID* mg, int gridID) {
    MG_REQUIRE(mg && gridID >= 0 && gridID < mg->maxGrids, MGX_ERR_INVALID, "InitF: bad gridID %d", gridID);
    GRID* g = mg->grids3D[gridID];
    double* t = (double*)malloc(((size_t)g->sizeX + g->sizeY + g->sizeZ) * sizeof(double));
    MG_REQUIRE(t, MGX_ERR_NOMEM, "InitF: out of host memory");
    double *tx = t, *ty = t + g->sizeX, *tz = ty + g->sizeY;
    for (int i = 0; i < g->sizeX; i++) { REAL x = g->x_a + i * g->h_x; tx[i] = sin(MG_PI * x); }
    for (int i = 0; i < g->sizeY; i++) { REAL y = g->y_a + i * g->h_y; ty[i] = sin(MG_PI * y); }
    for (int i = 0; i < g->sizeZ; i++) { REAL z = g->z_a + i * g->h_z; tz[i] = sin(MG_PI * z); }
    int st = MGXL(mg, init_f)(mg->ctx, g->d_f, g->sizeXYZ, -3 * MG_PI * MG_PI, tx, ty, tz);
    mg->f_rim_zero[gridID] = 0;
    free(t);
    return st;
}

/* MultiGrid3D::MultiGrid3D + InitGrids.                               N3/MultiGrid3D.cpp:5-47 */
int FN(create)(mgx_ctx* ctx, const int finestGridSizeXYZ[3], const REAL range[6], MGRID** out) {
    return FN(create_levels)(ctx, finestGridSizeXYZ, range, 1, 0, out);
}

/* layout: 0 = device arrays in the reference layout, 1 = x-split (default of create(); faster smoother) */
int FN(create_layout)(mgx_ctx* ctx, const int finestGridSizeXYZ[3], const REAL range[6], int layout, MGRID** out) {
    return FN(create_levels)(ctx, finestGridSizeXYZ, range, layout, 0, out);
}

/* nlevels > 0: only the first nlevels levels will be used.  An odd extent that is not 2^k+1 reaches an even one further down
 * (97 -> 49 -> 25 -> 13 -> 7 -> 4): with the level count of the reference's rule that is MGX_ERR_SIZE, as the reference's Grid3D
 * asserts; levels past nlevels are not built, so such a grid runs with a shorter hierarchy. */
int FN(create_levels)(mgx_ctx* ctx, const int finestGridSizeXYZ[3], const REAL range[6], int layout, int nlevels, MGRID** out) {
    MG_REQUIRE(ctx && finestGridSizeXYZ && range && out, MGX_ERR_INVALID, "MultiGrid3D: NULL argument");
    *out = NULL;
    int minSize = finestGridSizeXYZ[0]; /* :25-30 */
    if (finestGridSizeXYZ[1] < minSize) minSize = finestGridSizeXYZ[1];
    if (finestGridSizeXYZ[2] < minSize) minSize = finestGridSizeXYZ[2];
    MG_REQUIRE(minSize >= 3, MGX_ERR_SIZE, "MultiGrid3D: finest grid %d too small", minSize);
    MG_TRY(mgx_ctx_prepare(ctx)); /* nothing is left to allocate inside a cycle (a cycle may be captured into a HIP graph) */
    MGRID* mg = (MGRID*)calloc(1, sizeof(MGRID));
    MG_REQUIRE(mg, MGX_ERR_NOMEM, "MultiGrid3D: out of host memory");
    mg->ctx = ctx;
    mg->residual_mode = MGX_RESIDUAL_REF_COMPAT;
    mg->fuse = 1;
    mg->layout = layout ? 1 : 0;
    mg->smoother = 0;
    mg->omega = (REAL)2 / (REAL)3;
    mg->numGrids = mg->maxGrids = mg_num_grids(minSize); /* :33-34 */
    memset(mg->coarsen, 7, sizeof mg->coarsen);
    mg->grids3D = (GRID**)calloc((size_t)mg->maxGrids, sizeof(GRID*));
    if (!mg->grids3D) { free(mg); return mg_fail(MGX_ERR_NOMEM, "MultiGrid3D: out of host memory"); }
    int cur[3] = {finestGridSizeXYZ[0], finestGridSizeXYZ[1], finestGridSizeXYZ[2]};
    for (int i = 0; i < mg->maxGrids; i++) {
        if (nlevels > 0 && i >= nlevels && (cur[0] % 2 == 0 || cur[1] % 2 == 0 || cur[2] % 2 == 0)) {
            mg->numGrids = mg->maxGrids = i; /* the levels from here on would never be visited */
            break;
        }
        int st = MG_CAT(grid3_new_, R)(ctx, mg->layout, cur, range, &mg->grids3D[i]);
        if (!st) st = FN(InitV)(mg, i);
        if (!st) st = FN(InitF)(mg, i);
        if (st) { FN(destroy)(mg); return st; }
        for (int d = 0; d < 3; d++) cur[d] = mg_coarse_size(cur[d]); /* :40-42 */
    }
    *out = mg;
    return MGX_OK;
}

/* the hierarchy of a plan (mg_semi_plan): x-split, one level per plan entry, the plan's masks */
static int MG_CAT(create_plan3_, R)(mgx_ctx* ctx, const mgSemiPlan* plan, const REAL range[6], MGRID** out) {
    MG_TRY(mgx_ctx_prepare(ctx));
    MGRID* mg = (MGRID*)calloc(1, sizeof(MGRID));
    MG_REQUIRE(mg, MGX_ERR_NOMEM, "MultiGrid3D: out of host memory");
    mg->ctx = ctx;
    mg->residual_mode = MGX_RESIDUAL_REF_COMPAT;
    mg->fuse = 1;
    mg->layout = 1;
    mg->smoother = 0;
    mg->omega = (REAL)2 / (REAL)3;
    mg->numGrids = mg->maxGrids = plan->nlevels;
    memset(mg->coarsen, 7, sizeof mg->coarsen);
    mg->grids3D = (GRID**)calloc((size_t)mg->maxGrids, sizeof(GRID*));
    if (!mg->grids3D) { free(mg); return mg_fail(MGX_ERR_NOMEM, "MultiGrid3D: out of host memory"); }
    for (int i = 0; i < mg->maxGrids; i++) {
        if (i + 1 < mg->maxGrids) mg->coarsen[i] = plan->mask[i];
        int st = MG_CAT(grid3_new_, R)(ctx, 1, plan->n[i], range, &mg->grids3D[i]);
        if (!st) st = FN(InitV)(mg, i);
        if (!st) st = FN(InitF)(mg, i);
        if (st) { FN(destroy)(mg); return st; }
    }
    *out = mg;
    return MGX_OK;
}

int FN(create_semi)(mgx_ctx* ctx, const int finestGridSizeXYZ[3], const REAL range[6], int nlevels, MGRID** out) {
    MG_REQUIRE(ctx && finestGridSizeXYZ && range && out, MGX_ERR_INVALID, "MultiGrid3D: NULL argument");
    *out = NULL;
    const double drange[6] = {(double)range[0], (double)range[1], (double)range[2], (double)range[3], (double)range[4], (double)range[5]};
    mgSemiPlan plan;
    MG_TRY(mg_semi_plan(finestGridSizeXYZ, drange, nlevels, &plan));
    return MG_CAT(create_plan3_, R)(ctx, &plan, range, out);
}

/* the plan a hierarchy was built from */
static __attribute__((unused)) void MG_CAT(plan_of3_, R)(const MGRID* mg, mgSemiPlan* plan) {
    memset(plan, 0, sizeof *plan);
    plan->nlevels = mg->maxGrids;
    for (int i = 0; i < mg->maxGrids; i++) {
        for (int d = 0; d < 3; d++) plan->n[i][d] = mg->grids3D[i]->sizeXYZ[d];
        plan->mask[i] = i + 1 < mg->maxGrids ? mg->coarsen[i] : 0;
    }
}

/* is some step of the levels [from, numGrids) not a halving of all three axes? */
static int MG_CAT(semi_below3_, R)(const MGRID* mg, int from) {
    for (int i = from; i + 1 < mg->numGrids; i++)
        if (mg->coarsen[i] != 7) return 1;
    return 0;
}

/* the capacity of div(a grad u) - (shift c) u = f: mg->cap points to this table, one device array per level (all maxGrids levels or
 * no table), and whether level 0 holds a positive entry (without one the operator has no zeroth-order term) */
typedef struct MG_CAT(mgCapTable3_, R) {
    REAL* d_c[MG_MAX_LEVELS];
    int positive;
} MG_CAT(mgCapTable3_, R);
#define CAPTAB MG_CAT(mgCapTable3_, R)

static void MG_CAT(cap_table_free3_, R)(MGRID* mg) {
    CAPTAB* t = (CAPTAB*)mg->cap;
    if (!t) return;
    for (int i = 0; i < MG_MAX_LEVELS; i++) mgx_free(mg->ctx, t->d_c[i]);
    free(t);
    mg->cap = NULL;
}

/* the walls of DESIGN.md 18: mg->wall points to this table, or is NULL (no face has a beta or a g other than 0).  beta and g in the
 * order of the mask's bits; lossy: some beta > 0 (the operator then has a zeroth-order term on a face: no closed box is singular),
 * flux: some g != 0 */
typedef struct MG_CAT(mgWallTable3_, R) {
    REAL beta[6], g[6];
    int lossy, flux;
} MG_CAT(mgWallTable3_, R);
#define WALLTAB MG_CAT(mgWallTable3_, R)

/* the betas of a hierarchy with a positive one, else NULL: the operators then pass six zeros, which is the _bc entry by another name */
static const REAL* MG_CAT(wall_beta3_, R)(const MGRID* mg) {
    const WALLTAB* t = (const WALLTAB*)mg->wall;
    return t && t->lossy ? t->beta : NULL;
}
static const REAL MG_CAT(no_wall3_, R)[6] = {0, 0, 0, 0, 0, 0};

/* the pinned interior nodes of DESIGN.md 22: mg->pin points to this table, or is NULL (no point is pinned).  Per level the list of
 * mgx.h (device: storage offsets, red first, and the values in list order; both NULL where the level has no pinned point), its two
 * counts, and the level's mask in the reference layout on the host (what _get_pinned returns) */
typedef struct MG_CAT(mgPinTable3_, R) {
    unsigned* d_idx[MG_MAX_LEVELS];
    REAL* d_val[MG_MAX_LEVELS];
    unsigned end[MG_MAX_LEVELS][2];
    unsigned char* h_mask[MG_MAX_LEVELS];
} MG_CAT(mgPinTable3_, R);
#define PINTAB MG_CAT(mgPinTable3_, R)

static void MG_CAT(pin_table_free3_, R)(MGRID* mg) {
    PINTAB* t = (PINTAB*)mg->pin;
    if (!t) return;
    for (int i = 0; i < MG_MAX_LEVELS; i++) {
        mgx_free(mg->ctx, t->d_idx[i]);
        mgx_free(mg->ctx, t->d_val[i]);
        free(t->h_mask[i]);
    }
    free(t);
    mg->pin = NULL;
}

/* the level of grid g, -1 where it is none of the hierarchy's */
static int MG_CAT(level_of3_, R)(const MGRID* mg, const GRID* g) {
    for (int i = 0; i < mg->maxGrids; i++)
        if (mg->grids3D[i] == g) return i;
    return -1;
}

/* dev (an array of level lvl) := the level's values (values != 0) or zeros at its pinned points; nothing without pins */
static int MG_CAT(pin_put3_, R)(MGRID* mg, int lvl, REAL* dev, int values) {
    const PINTAB* t = (const PINTAB*)mg->pin;
    if (!t || lvl < 0 || !t->end[lvl][1]) return MGX_OK;
    return MG_CAT(mgx3dxs_pin_put_, R)(mg->ctx, dev, t->d_idx[lvl], values ? t->d_val[lvl] : NULL, 0u, t->end[lvl][1]);
}

void FN(destroy)(MGRID* mg) {
    if (!mg) return;
    MG_CAT(pin_table_free3_, R)(mg);
    MG_CAT(cap_table_free3_, R)(mg);
    free(mg->wall);
    mg->wall = NULL;
    for (int i = 0; i < MG_MAX_LEVELS; i++)
        if (mg->graph_exec[i]) mgx_graph_destroy(mg->ctx, mg->graph_exec[i]);
    if (mg->pcg_graph_exec) mgx_graph_destroy(mg->ctx, mg->pcg_graph_exec);
    mgx_free(mg->ctx, mg->pcg_x); mgx_free(mg->ctx, mg->pcg_b); mgx_free(mg->ctx, mg->pcg_p); mgx_free(mg->ctx, mg->pcg_q);
    mgx_free(mg->ctx, mg->pcg_state); mgx_free(mg->ctx, mg->pcg_work); mgx_free(mg->ctx, mg->pcg_fproj);
    mg_mixed3d_free(mg->ctx, mg->pcg_mixed);
    if (mg->grids3D)
        for (int i = 0; i < mg->maxGrids; i++) MG_CAT(grid3_free_, R)(mg->ctx, mg->grids3D[i]);
    free(mg->grids3D);
    free(mg);
}

/* a write through the public operators into some level's d_f: its boundary entries are no longer known to be 0 */
static void MG_CAT(f_touched3_, R)(MGRID* mg, const REAL* dev) {
    for (int i = 0; i < mg->maxGrids; i++)
        if (mg->grids3D[i] && mg->grids3D[i]->d_f == dev) mg->f_rim_zero[i] = 0;
}

/* a write through the public operators that may change boundary entries of some level's d_v or d_e */
static void MG_CAT(v_touched3_, R)(MGRID* mg, const REAL* dev) {
    for (int i = 0; i < mg->maxGrids; i++)
        if (mg->grids3D[i] && (mg->grids3D[i]->d_v == dev || mg->grids3D[i]->d_e == dev)) {
            mg->e_rim_valid[i] = 0;
            if (mg->grids3D[i]->d_v == dev) mg->v_rim_zero[i] = 0;
        }
}

/* ---------------------------------------------------------------- the shifted operator (Laplacian - shift) u = f */
/* what a non-zero shift needs of the hierarchy (the members are public: checked where the shift is used, too) */
static int MG_CAT(shift_ok3_, R)(const MGRID* mg, REAL shift, const char* what) {
    MG_REQUIRE(isfinite((double)shift) && shift >= 0, MGX_ERR_INVALID, "%s: the shift %g is not finite and >= 0", what, (double)shift);
    if (shift == 0) return MGX_OK;
    MG_REQUIRE(mg->layout == 1, MGX_ERR_INVALID, "%s: a shifted hierarchy needs the x-split layout (layout = 1)", what);
    MG_REQUIRE(mg->smoother == 0, MGX_ERR_INVALID, "%s: a shifted hierarchy needs the red-black smoother (smoother = 0)", what);
    MG_REQUIRE(mg->residual_mode == MGX_RESIDUAL_CORRECT, MGX_ERR_INVALID, "%s: a shifted hierarchy needs residual_mode = MGX_RESIDUAL_CORRECT",
               what);
    return MGX_OK;
}

int FN(set_shift)(MGRID* mg, REAL shift) {
    MG_REQUIRE(mg, MGX_ERR_INVALID, "set_shift: NULL");
    MG_TRY(MG_CAT(shift_ok3_, R)(mg, shift, "set_shift"));
    mg->shift = shift;
    return MGX_OK;
}

size_t FN(sizeof)(void) { return sizeof(MGRID); }
size_t MG_CAT3(mgGrid3D_, R, _sizeof)(void) { return sizeof(GRID); }

/* ---------------------------------------------------------------- the variable-coefficient operator div(a grad u) - shift u = f */
/* "this hierarchy has a coefficient": level 0 holds one (set_coefficient allocates every level or none) */
static int MG_CAT(has_coef3_, R)(const MGRID* mg) { return mg->grids3D && mg->grids3D[0] && mg->grids3D[0]->d_a != NULL; }

/* "this hierarchy has a capacity" (set_capacity asks for a coefficient first), and the capacity array of grid g (NULL: none, or g
 * is no level of the hierarchy) */
static int MG_CAT(has_cap3_, R)(const MGRID* mg) { return mg->cap != NULL; }
static const REAL* MG_CAT(cap_of3_, R)(const MGRID* mg, const GRID* g) {
    const CAPTAB* t = (const CAPTAB*)mg->cap;
    for (int i = 0; t && i < mg->maxGrids; i++)
        if (mg->grids3D[i] == g) return t->d_c[i];
    return NULL;
}

/* "this hierarchy's faces carry the harmonic mean" (mg_multigrid.h _set_face_mean, DESIGN.md 19): the mode counts only where there
 * is a coefficient, and then every operator call takes the _hmean entries, with the capacity of the grid or NULL */
static int MG_CAT(harm3_, R)(const MGRID* mg) { return mg->face_mean == MG_FACE_MEAN_HARMONIC && MG_CAT(has_coef3_, R)(mg); }
static const REAL* MG_CAT(harm_cap3_, R)(const MGRID* mg, const GRID* g) { return MG_CAT(has_cap3_, R)(mg) ? MG_CAT(cap_of3_, R)(mg, g) : NULL; }

/* what the harmonic mean needs of a coefficient: the products aP * aQ normal and finite in REAL, that is, every square */
static int MG_CAT(harm_range3_, R)(const REAL* host_a, size_t vol, const char* what) {
    const REAL tiny = sizeof(REAL) == 4 ? (REAL)FLT_MIN : (REAL)DBL_MIN;
    for (size_t i = 0; i < vol; i++) {
        const REAL sq = host_a[i] * host_a[i];
        MG_REQUIRE(isfinite((double)sq) && sq >= tiny, MGX_ERR_INVALID,
                   "%s: a[%zu] = %g is outside the range of the harmonic face mean: its square %g is not a normal, finite number of this "
                   "precision", what, i, (double)host_a[i], (double)sq);
    }
    return MGX_OK;
}

/* what a coefficient needs of the hierarchy (the members are public: checked where the coefficient is used, too) */
static int MG_CAT(coef_ok3_, R)(const MGRID* mg, const char* what) {
    MG_REQUIRE(isfinite((double)mg->shift) && mg->shift >= 0, MGX_ERR_INVALID, "%s: the shift %g is not finite and >= 0", what, (double)mg->shift);
    MG_REQUIRE(mg->layout == 1, MGX_ERR_INVALID, "%s: a hierarchy with a coefficient needs the x-split layout (layout = 1)", what);
    MG_REQUIRE(mg->smoother == 0, MGX_ERR_INVALID, "%s: a hierarchy with a coefficient needs the red-black smoother (smoother = 0)", what);
    MG_REQUIRE(mg->residual_mode == MGX_RESIDUAL_CORRECT, MGX_ERR_INVALID,
               "%s: a hierarchy with a coefficient needs residual_mode = MGX_RESIDUAL_CORRECT", what);
    for (int i = 0; i < mg->maxGrids; i++)
        MG_REQUIRE(mg->grids3D[i]->d_a, MGX_ERR_INVALID, "%s: level %d has no coefficient array (set it through _set_coefficient)", what, i);
    return MGX_OK;
}

/* ---------------------------------------------------------------- homogeneous Neumann faces (the mask mg->bc) */
/* what the mask bc needs of the hierarchy (the members are public: checked by set_boundary and where the mask is used) */
static int MG_CAT(bc_ok3_, R)(const MGRID* mg, int bc, const char* what) {
    if (!bc) return MGX_OK;
    MG_REQUIRE(bc > 0 && bc <= 63, MGX_ERR_INVALID, "%s: the boundary mask %d is outside 0 .. 63", what, bc);
    MG_REQUIRE(mg->layout == 1, MGX_ERR_INVALID, "%s: a hierarchy with Neumann faces needs the x-split layout (layout = 1)", what);
    MG_REQUIRE(mg->smoother == 0, MGX_ERR_INVALID, "%s: a hierarchy with Neumann faces needs the red-black smoother (smoother = 0)", what);
    MG_REQUIRE(mg->residual_mode == MGX_RESIDUAL_CORRECT, MGX_ERR_INVALID,
               "%s: a hierarchy with Neumann faces needs residual_mode = MGX_RESIDUAL_CORRECT", what);
    for (int i = 0; i + 1 < mg->maxGrids; i++)
        MG_REQUIRE(mg->coarsen[i] == 7, MGX_ERR_INVALID, "%s: Neumann faces are not available on a semi-coarsened hierarchy", what);
    return MGX_OK;
}
/* ... and of the operator: a closed box without a shift has no unique solution (checked where the operator is used only: the
 * shift is a public member and may still change after set_boundary).  bc_reserved is set while PCG(krylov = 2) solves that
 * system in the projected sense: its preconditioner's Relax and residual then pass. */
static int MG_CAT(bc_singular3_, R)(const MGRID* mg, const char* what) {
    if (MG_CAT(wall_beta3_, R)(mg)) return MGX_OK; /* a wall that loses heat makes the closed box regular */
    MG_REQUIRE(!(mg->bc == 63 && mg->shift == 0) || mg->bc_reserved, MGX_ERR_INVALID,
               "%s: Neumann data on all six faces with shift = 0 is singular (set a shift > 0 or keep a Dirichlet face)", what);
    return MGX_OK;
}
/* ... nor has one whose capacity has no positive entry, whatever the shift: shift * c is zero everywhere */
static int MG_CAT(cap_singular3_, R)(const MGRID* mg, const char* what) {
    if (MG_CAT(wall_beta3_, R)(mg)) return MGX_OK;
    MG_REQUIRE(!(mg->bc == 63 && mg->cap && !((const CAPTAB*)mg->cap)->positive), MGX_ERR_INVALID,
               "%s: Neumann data on all six faces with a capacity that has no positive entry is singular (set a capacity with a "
               "positive entry or keep a Dirichlet face)", what);
    return MGX_OK;
}

/* The operators other than the plain Laplacian: the variable-coefficient one where the hierarchy has a coefficient (with any
 * shift), else the shifted one where shift != 0.  What the hierarchy's operator needs of the hierarchy and of the grid g it is
 * applied to (nothing for the plain one). */
/* what pinned nodes need of the hierarchy (the members are public: checked by set_pinned and where the pins are used).  The closed
 * box without a shift is refused whatever the pins: its projection would be wrong and a coarse level may lose the last pin. */
static int MG_CAT(pin_ok3_, R)(const MGRID* mg, const char* what) {
    if (!mg->pin) return MGX_OK;
    MG_REQUIRE(mg->layout == 1, MGX_ERR_INVALID, "%s: a hierarchy with pinned nodes needs the x-split layout (layout = 1, not natural)", what);
    MG_REQUIRE(mg->smoother == 0, MGX_ERR_INVALID,
               "%s: a hierarchy with pinned nodes needs the red-black smoother (smoother = 0): the Jacobi smoother is not available", what);
    MG_REQUIRE(mg->residual_mode == MGX_RESIDUAL_CORRECT, MGX_ERR_INVALID,
               "%s: a hierarchy with pinned nodes needs residual_mode = MGX_RESIDUAL_CORRECT", what);
    MG_REQUIRE(!(mg->bc == 63 && mg->shift == 0 && !MG_CAT(wall_beta3_, R)(mg)), MGX_ERR_INVALID,
               "%s: pinned nodes are not available in the closed box (walls on all six faces, shift = 0, no beta > 0), krylov = 2 "
               "included: keep a Dirichlet face, set a shift > 0 or a beta > 0", what);
    return MGX_OK;
}

static int MG_CAT(op_ok3_, R)(const MGRID* mg, const GRID* g, const char* what) {
    MG_TRY(MG_CAT(pin_ok3_, R)(mg, what));
    MG_TRY(MG_CAT(bc_ok3_, R)(mg, mg->bc, what));
    MG_TRY(MG_CAT(bc_singular3_, R)(mg, what));
    MG_TRY(MG_CAT(cap_singular3_, R)(mg, what));
    if (!MG_CAT(has_coef3_, R)(mg)) return MG_CAT(shift_ok3_, R)(mg, mg->shift, what);
    MG_TRY(MG_CAT(coef_ok3_, R)(mg, what));
    MG_REQUIRE(g->d_a, MGX_ERR_INVALID, "%s: the grid has no coefficient array", what);
    MG_REQUIRE(!MG_CAT(has_cap3_, R)(mg) || MG_CAT(cap_of3_, R)(mg, g), MGX_ERR_INVALID, "%s: the grid has no capacity array", what);
    return MGX_OK;
}

/* r = f - A v on grid g by the hierarchy's operator, 0 on the boundary (r == NULL: not stored), and its sum of squares into
 * *dev_sumsq (NULL: none; dev_work: the partials).  The plain operator takes mg->residual_mode and sums in a launch of its own. */
static int MG_CAT(op_residual_all3_, R)(MGRID* mg, const GRID* g, const REAL* v, const REAL* f, REAL* r, double* dev_work, double* dev_sumsq) {
    const REAL h[3] = {g->h_x, g->h_y, g->h_z};
    const REAL* wall = MG_CAT(wall_beta3_, R)(mg);
    const REAL* wb = wall ? wall : MG_CAT(no_wall3_, R); /* the _wall entries with the level's own spacings (DESIGN.md 18) */
    const int faces = mg->bc || wall || mg->pin;         /* (betas without a mask: the entry refuses them; pins: the op route) */
    if (MG_CAT(harm3_, R)(mg))
        return MG_CAT(mgx3dxs_residual_hmean_wall_, R)(mg->ctx, v, f, g->d_a, MG_CAT(harm_cap3_, R)(mg, g), r, g->sizeXYZ, h, mg->shift, dev_work,
                                                       dev_sumsq, mg->bc, wb);
    if (MG_CAT(has_cap3_, R)(mg))
        return MG_CAT(mgx3dxs_residual_cap_wall_, R)(mg->ctx, v, f, g->d_a, MG_CAT(cap_of3_, R)(mg, g), r, g->sizeXYZ, h, mg->shift, dev_work,
                                                     dev_sumsq, mg->bc, wb);
    if (MG_CAT(has_coef3_, R)(mg))
        return MG_CAT(mgx3dxs_residual_coef_wall_, R)(mg->ctx, v, f, g->d_a, r, g->sizeXYZ, h, mg->shift, dev_work, dev_sumsq, mg->bc, wb);
    if (mg->shift != 0 || faces) /* (with a mask the plain Laplacian is the shifted operator with s = 0) */
        return MG_CAT(mgx3dxs_residual_shift_wall_, R)(mg->ctx, v, f, r, g->sizeXYZ, h, mg->shift, dev_work, dev_sumsq, mg->bc, wb);
    MG_TRY(MGXL(mg, residual)(mg->ctx, v, f, r, g->sizeXYZ, h, mg->residual_mode));
    return dev_sumsq ? MG_CAT(mgx3dxs_dot2_, R)(mg->ctx, r, r, NULL, g->sizeXYZ, dev_work, dev_sumsq) : MGX_OK;
}

/* ... and with pinned nodes: the fused sum would include what the kernels compute at the pins, so the residual is stored (into the
 * level's d_r where the caller passes none), its pins zeroed, and the sum taken over the stored array in a pass of its own
 * (without a mask: mgx3dxs_dot2's bits) */
static int MG_CAT(op_residual3_, R)(MGRID* mg, const GRID* g, const REAL* v, const REAL* f, REAL* r, double* dev_work, double* dev_sumsq) {
    const int lvl = mg->pin ? MG_CAT(level_of3_, R)(mg, g) : -1;
    if (lvl < 0) return MG_CAT(op_residual_all3_, R)(mg, g, v, f, r, dev_work, dev_sumsq);
    if (!r) r = g->d_r;
    MG_TRY(MG_CAT(op_residual_all3_, R)(mg, g, v, f, r, NULL, NULL));
    MG_TRY(MG_CAT(pin_put3_, R)(mg, lvl, r, 0));
    return dev_sumsq ? MG_CAT(mgx3dxs_sumsq_bc_, R)(mg->ctx, r, g->sizeXYZ, dev_work, dev_sumsq, mg->bc) : MGX_OK;
}

/* q = A p on grid g by the hierarchy's operator (x-split, CORRECT mode), *dev_sum = <p, q>; with a mask at all unknowns and in the
 * weighted inner product (the plain Laplacian is then the shifted operator with s = 0).  With pinned nodes p is 0 there, so the
 * fused <p, q> is right as it is, and q's pins are zeroed afterwards */
static int MG_CAT(op_apply_dot_all3_, R)(MGRID* mg, const GRID* g, const REAL* p, REAL* q, double* dev_work, double* dev_sum);
static int MG_CAT(op_apply_dot3_, R)(MGRID* mg, const GRID* g, const REAL* p, REAL* q, double* dev_work, double* dev_sum) {
    MG_TRY(MG_CAT(op_apply_dot_all3_, R)(mg, g, p, q, dev_work, dev_sum));
    return mg->pin ? MG_CAT(pin_put3_, R)(mg, MG_CAT(level_of3_, R)(mg, g), q, 0) : MGX_OK;
}
static int MG_CAT(op_apply_dot_all3_, R)(MGRID* mg, const GRID* g, const REAL* p, REAL* q, double* dev_work, double* dev_sum) {
    const REAL h[3] = {g->h_x, g->h_y, g->h_z};
    const REAL* wall = MG_CAT(wall_beta3_, R)(mg);
    const REAL* wb = wall ? wall : MG_CAT(no_wall3_, R);
    const int faces = mg->bc || wall || mg->pin; /* (betas without a mask: the entry refuses them; pins: the op route, s = 0 too) */
    if (MG_CAT(harm3_, R)(mg)) /* (with bc = 0 the entry is the interior entry) */
        return MG_CAT(mgx3dxs_apply_hmean_dot_wall_, R)(mg->ctx, p, g->d_a, MG_CAT(harm_cap3_, R)(mg, g), q, g->sizeXYZ, h, mg->shift, dev_work,
                                                        dev_sum, mg->bc, wb);
    if (MG_CAT(has_cap3_, R)(mg)) /* (with bc = 0 the entry is the interior entry) */
        return MG_CAT(mgx3dxs_apply_cap_dot_wall_, R)(mg->ctx, p, g->d_a, MG_CAT(cap_of3_, R)(mg, g), q, g->sizeXYZ, h, mg->shift, dev_work,
                                                      dev_sum, mg->bc, wb);
    if (faces && MG_CAT(has_coef3_, R)(mg))
        return MG_CAT(mgx3dxs_apply_coef_dot_wall_, R)(mg->ctx, p, g->d_a, q, g->sizeXYZ, h, mg->shift, dev_work, dev_sum, mg->bc, wb);
    if (faces) return MG_CAT(mgx3dxs_laplace_dot_shift_wall_, R)(mg->ctx, p, q, g->sizeXYZ, h, mg->shift, dev_work, dev_sum, mg->bc, wb);
    if (MG_CAT(has_coef3_, R)(mg))
        return MG_CAT(mgx3dxs_apply_coef_dot_, R)(mg->ctx, p, g->d_a, q, g->sizeXYZ, h, mg->shift, dev_work, dev_sum);
    if (mg->shift != 0) return MG_CAT(mgx3dxs_laplace_dot_shift_, R)(mg->ctx, p, q, g->sizeXYZ, h, mg->shift, dev_work, dev_sum);
    return MG_CAT(mgx3dxs_laplace_dot_, R)(mg->ctx, p, q, g->sizeXYZ, h, dev_work, dev_sum);
}

/* The captured graphs hold the d_a pointers of every level, their records only level 0's: whenever the arrays are allocated or
 * freed the graphs are dropped, so that no replay can meet arrays other than those of its capture. */
static void MG_CAT(coef_drop_graphs3_, R)(MGRID* mg) {
    for (int i = 0; i < MG_MAX_LEVELS; i++) {
        if (mg->graph_exec[i]) mgx_graph_destroy(mg->ctx, mg->graph_exec[i]);
        mg->graph_exec[i] = NULL;
    }
    if (mg->pcg_graph_exec) mgx_graph_destroy(mg->ctx, mg->pcg_graph_exec);
    mg->pcg_graph_exec = NULL;
}

static void MG_CAT(coef_free3_, R)(MGRID* mg) {
    MG_CAT(coef_drop_graphs3_, R)(mg);
    for (int i = 0; i < mg->maxGrids; i++) {
        mgx_free(mg->ctx, mg->grids3D[i]->d_a);
        mg->grids3D[i]->d_a = NULL;
    }
}

static int MG_CAT(put3_, R)(MGRID* mg, GRID* g, REAL* dev, const REAL* host);
static int MG_CAT(get3_, R)(MGRID* mg, GRID* g, const REAL* dev, REAL* host);

int FN(set_coefficient)(MGRID* mg, const REAL* host_a) {
    MG_REQUIRE(mg && mg->grids3D && mg->maxGrids >= 1, MGX_ERR_INVALID, "set_coefficient: NULL");
    if (!host_a) { /* back to the constant-coefficient operators */
        MG_REQUIRE(!MG_CAT(has_cap3_, R)(mg), MGX_ERR_INVALID,
                   "set_coefficient: the hierarchy has a capacity, which needs a coefficient: clear it first (set_capacity(NULL))");
        MG_TRY(mgx_ctx_sync(mg->ctx));
        MG_CAT(coef_free3_, R)(mg);
        return MGX_OK;
    }
    MG_REQUIRE(mg->layout == 1, MGX_ERR_INVALID, "set_coefficient: a hierarchy with a coefficient needs the x-split layout (layout = 1)");
    MG_REQUIRE(mg->smoother == 0, MGX_ERR_INVALID, "set_coefficient: a hierarchy with a coefficient needs the red-black smoother (smoother = 0)");
    MG_REQUIRE(mg->residual_mode == MGX_RESIDUAL_CORRECT, MGX_ERR_INVALID,
               "set_coefficient: a hierarchy with a coefficient needs residual_mode = MGX_RESIDUAL_CORRECT");
    const size_t vol = MG_CAT(vol3_, R)(mg->grids3D[0]);
    for (size_t i = 0; i < vol; i++)
        MG_REQUIRE(isfinite((double)host_a[i]) && host_a[i] > 0, MGX_ERR_INVALID, "set_coefficient: a[%zu] = %g is not finite and > 0", i,
                   (double)host_a[i]);
    if (mg->face_mean == MG_FACE_MEAN_HARMONIC) MG_TRY(MG_CAT(harm_range3_, R)(host_a, vol, "set_coefficient"));
    const int had = MG_CAT(has_coef3_, R)(mg);
    int st = MGX_OK;
    if (!had) { /* (nothing of a captured cycle is in flight any more) */
        MG_TRY(mgx_ctx_sync(mg->ctx));
        MG_CAT(coef_drop_graphs3_, R)(mg);
    }
    for (int i = 0; !st && i < mg->maxGrids; i++) { /* first use: one array per level, pads zero */
        GRID* g = mg->grids3D[i];
        if (g->d_a) continue;
        const size_t bytes = MG_CAT(dvol3_, R)(mg->layout, g) * sizeof(REAL);
        st = mgx_malloc(mg->ctx, bytes, (void**)&g->d_a);
        if (!st) st = mgx_memset_zero(mg->ctx, g->d_a, bytes);
    }
    if (!st) st = MG_CAT(put3_, R)(mg, mg->grids3D[0], mg->grids3D[0]->d_a, host_a);
    for (int i = 0; !st && i + 1 < mg->maxGrids; i++) { /* a_{l+1} = Restrict(a_l) by the step's mask */
        GRID *fine = mg->grids3D[i], *coarse = mg->grids3D[i + 1];
        if (mg->coarsen[i] != 7) st = MG_CAT(mgx3dxs_restrict_axes_, R)(mg->ctx, fine->d_a, fine->sizeXYZ, coarse->d_a, coarse->sizeXYZ);
        else st = MG_CAT(mgx3dxs_restrict_, R)(mg->ctx, fine->d_a, fine->sizeXYZ, coarse->d_a, coarse->sizeXYZ);
    }
    if (!st) st = mgx_ctx_sync(mg->ctx);
    if (st && !had) MG_CAT(coef_free3_, R)(mg); /* nothing half-built stays behind */
    return st;
}

int FN(download_coefficient)(MGRID* mg, int gridID, REAL* host) {
    MG_REQUIRE(mg && gridID >= 0 && gridID < mg->maxGrids, MGX_ERR_INVALID, "download_coefficient: bad gridID %d", gridID);
    MG_REQUIRE(host, MGX_ERR_INVALID, "download_coefficient: NULL");
    GRID* g = mg->grids3D[gridID];
    MG_REQUIRE(g->d_a, MGX_ERR_INVALID, "download_coefficient: the hierarchy has no coefficient");
    return MG_CAT(get3_, R)(mg, g, g->d_a, host);
}

/* The mean of the face coefficients (mg_multigrid.h).  The captured graphs hold the kernels of the mean they were captured under:
 * a change of the mode drops them.  A coefficient the hierarchy already has is checked against the harmonic mean's range first. */
int FN(set_face_mean)(MGRID* mg, int mode) {
    MG_REQUIRE(mg && mg->grids3D && mg->maxGrids >= 1, MGX_ERR_INVALID, "set_face_mean: NULL");
    MG_REQUIRE(mode == MG_FACE_MEAN_ARITHMETIC || mode == MG_FACE_MEAN_HARMONIC, MGX_ERR_INVALID,
               "set_face_mean: the mode %d is neither MG_FACE_MEAN_ARITHMETIC (0) nor MG_FACE_MEAN_HARMONIC (1)", mode);
    if (mode == mg->face_mean) return MGX_OK;
    if (mode == MG_FACE_MEAN_HARMONIC && MG_CAT(has_coef3_, R)(mg)) {
        const size_t vol = MG_CAT(vol3_, R)(mg->grids3D[0]);
        REAL* host = (REAL*)malloc(vol * sizeof(REAL));
        MG_REQUIRE(host, MGX_ERR_NOMEM, "set_face_mean: out of host memory");
        int st = FN(download_coefficient)(mg, 0, host);
        if (!st) st = MG_CAT(harm_range3_, R)(host, vol, "set_face_mean");
        free(host);
        MG_TRY(st);
    }
    if (MG_CAT(has_coef3_, R)(mg)) { /* (a plain or shifted hierarchy captured nothing that depends on the mode) */
        MG_TRY(mgx_ctx_sync(mg->ctx)); /* (nothing of a captured cycle is in flight any more) */
        MG_CAT(coef_drop_graphs3_, R)(mg);
    }
    mg->face_mean = mode;
    return MGX_OK;
}

/* The capacity (mg_multigrid.h).  The captured graphs hold the arrays of every level: every call drops them. */
int FN(set_capacity)(MGRID* mg, const REAL* host_c) {
    MG_REQUIRE(mg && mg->grids3D && mg->maxGrids >= 1, MGX_ERR_INVALID, "set_capacity: NULL");
    if (!host_c) { /* back to the scalar-shift operators */
        if (!mg->cap) return MGX_OK;
        MG_TRY(mgx_ctx_sync(mg->ctx));
        MG_CAT(coef_drop_graphs3_, R)(mg);
        MG_CAT(cap_table_free3_, R)(mg);
        return MGX_OK;
    }
    MG_REQUIRE(MG_CAT(has_coef3_, R)(mg), MGX_ERR_INVALID,
               "set_capacity: a capacity needs a coefficient array: call set_coefficient first (an array of ones serves)");
    MG_TRY(MG_CAT(coef_ok3_, R)(mg, "set_capacity"));
    const size_t vol = MG_CAT(vol3_, R)(mg->grids3D[0]);
    int positive = 0;
    for (size_t i = 0; i < vol; i++) {
        MG_REQUIRE(isfinite((double)host_c[i]) && host_c[i] >= 0, MGX_ERR_INVALID, "set_capacity: c[%zu] = %g is not finite and >= 0", i,
                   (double)host_c[i]);
        if (host_c[i] > 0) positive = 1;
    }
    MG_TRY(mgx_ctx_sync(mg->ctx)); /* (nothing of a captured cycle is in flight any more) */
    MG_CAT(coef_drop_graphs3_, R)(mg);
    const int had = mg->cap != NULL;
    int st = MGX_OK;
    if (!had) { /* first use: one array per level, pads zero */
        mg->cap = calloc(1, sizeof(CAPTAB));
        MG_REQUIRE(mg->cap, MGX_ERR_NOMEM, "set_capacity: out of host memory");
        for (int i = 0; !st && i < mg->maxGrids; i++) {
            const size_t bytes = MG_CAT(dvol3_, R)(mg->layout, mg->grids3D[i]) * sizeof(REAL);
            st = mgx_malloc(mg->ctx, bytes, (void**)&((CAPTAB*)mg->cap)->d_c[i]);
            if (!st) st = mgx_memset_zero(mg->ctx, ((CAPTAB*)mg->cap)->d_c[i], bytes);
        }
    }
    CAPTAB* t = (CAPTAB*)mg->cap;
    if (!st) st = MG_CAT(put3_, R)(mg, mg->grids3D[0], t->d_c[0], host_c);
    for (int i = 0; !st && i + 1 < mg->maxGrids; i++) { /* c_{l+1} = Restrict(c_l) by the step's mask, as the coefficient goes down */
        GRID *fine = mg->grids3D[i], *coarse = mg->grids3D[i + 1];
        if (mg->coarsen[i] != 7) st = MG_CAT(mgx3dxs_restrict_axes_, R)(mg->ctx, t->d_c[i], fine->sizeXYZ, t->d_c[i + 1], coarse->sizeXYZ);
        else st = MG_CAT(mgx3dxs_restrict_, R)(mg->ctx, t->d_c[i], fine->sizeXYZ, t->d_c[i + 1], coarse->sizeXYZ);
    }
    if (!st) st = mgx_ctx_sync(mg->ctx);
    if (!st) t->positive = positive;
    if (st && !had) MG_CAT(cap_table_free3_, R)(mg); /* nothing half-built stays behind */
    return st;
}

int FN(download_capacity)(MGRID* mg, int gridID, REAL* host) {
    MG_REQUIRE(mg && gridID >= 0 && gridID < mg->maxGrids, MGX_ERR_INVALID, "download_capacity: bad gridID %d", gridID);
    MG_REQUIRE(host, MGX_ERR_INVALID, "download_capacity: NULL");
    MG_REQUIRE(mg->cap, MGX_ERR_INVALID, "download_capacity: the hierarchy has no capacity");
    return MG_CAT(get3_, R)(mg, mg->grids3D[gridID], ((CAPTAB*)mg->cap)->d_c[gridID], host);
}

/* the mask of the Neumann faces (mg_multigrid.h).  The captured graphs are dropped whenever it changes. */
int FN(set_boundary)(MGRID* mg, const int neumann[6]) {
    MG_REQUIRE(mg && mg->grids3D && neumann, MGX_ERR_INVALID, "set_boundary: NULL");
    int bc = 0;
    for (int k = 0; k < 6; k++)
        if (neumann[k]) bc |= 1 << k;
    if (bc == mg->bc) return MGX_OK;
    MG_TRY(MG_CAT(bc_ok3_, R)(mg, bc, "set_boundary"));
    for (int k = 0; mg->wall && k < 6; k++) {
        const WALLTAB* t = (const WALLTAB*)mg->wall;
        MG_REQUIRE(((bc >> k) & 1) || (t->beta[k] == 0 && t->g[k] == 0), MGX_ERR_INVALID,
                   "set_boundary: face %d still carries wall data (beta %g, g %g): clear them through set_wall first", k, (double)t->beta[k],
                   (double)t->g[k]);
    }
    MG_TRY(mgx_ctx_sync(mg->ctx)); /* (nothing of a captured cycle is in flight any more) */
    MG_CAT(coef_drop_graphs3_, R)(mg);
    /* below the finest level the entries the old mask made unknowns go back to the zeros they were before it */
    for (int i = 1; mg->bc && i < mg->maxGrids; i++) {
        GRID* g = mg->grids3D[i];
        MG_CAT(v_touched3_, R)(mg, g->d_v);
        MG_TRY(MG_CAT(mgx3dxs_set_rim_bc_, R)(mg->ctx, g->d_v, g->sizeXYZ, (REAL)0, mg->bc));
    }
    mg->bc = bc;
    return mgx_ctx_sync(mg->ctx);
}

int FN(get_boundary)(const MGRID* mg, int neumann[6]) {
    MG_REQUIRE(mg && neumann, MGX_ERR_INVALID, "get_boundary: NULL");
    for (int k = 0; k < 6; k++) neumann[k] = (mg->bc >> k) & 1;
    return MGX_OK;
}

/* the walls (mg_multigrid.h).  Every change drops the captured graphs: their launches hold the d_k by value. */
int FN(set_wall)(MGRID* mg, const REAL beta[6], const REAL g[6]) {
    MG_REQUIRE(mg && mg->grids3D && beta && g, MGX_ERR_INVALID, "set_wall: NULL");
    MG_TRY(MG_CAT(bc_ok3_, R)(mg, mg->bc, "set_wall"));
    int lossy = 0, flux = 0;
    for (int k = 0; k < 6; k++) {
        MG_REQUIRE(isfinite((double)beta[k]) && beta[k] >= 0, MGX_ERR_INVALID, "set_wall: beta[%d] = %g is not finite and >= 0", k,
                   (double)beta[k]);
        MG_REQUIRE(isfinite((double)g[k]), MGX_ERR_INVALID, "set_wall: g[%d] = %g is not finite", k, (double)g[k]);
        MG_REQUIRE(((mg->bc >> k) & 1) || (beta[k] == 0 && g[k] == 0), MGX_ERR_INVALID,
                   "set_wall: face %d has wall data (beta %g, g %g) but is not flagged in the mask %d (set_boundary first)", k, (double)beta[k],
                   (double)g[k], mg->bc);
        if (beta[k] > 0) lossy = 1;
        if (g[k] != 0) flux = 1;
        /* the terms the kernels work with, 2 beta / h on every level and 2 g / h on level 0, have to be finite in REAL */
        for (int i = 0; i < mg->maxGrids; i++) {
            const GRID* gl = mg->grids3D[i];
            const REAL hk = k < 2 ? gl->h_x : k < 4 ? gl->h_y : gl->h_z;
            MG_REQUIRE(isfinite((double)(((REAL)2 * beta[k]) / hk)), MGX_ERR_INVALID,
                       "set_wall: 2 * beta[%d] / h = 2 * %g / %g is not finite in this precision on level %d", k, (double)beta[k], (double)hk, i);
            MG_REQUIRE(i || isfinite((double)(((REAL)2 * g[k]) / hk)), MGX_ERR_INVALID,
                       "set_wall: 2 * g[%d] / h = 2 * %g / %g is not finite in this precision", k, (double)g[k], (double)hk);
        }
    }
    if (!lossy && !flux && !mg->wall) return MGX_OK;
    MG_TRY(mgx_ctx_sync(mg->ctx)); /* (nothing of a captured cycle is in flight any more) */
    MG_CAT(coef_drop_graphs3_, R)(mg);
    if (!lossy && !flux) { /* all zeros: the hierarchy is one that never had a wall */
        free(mg->wall);
        mg->wall = NULL;
        return MGX_OK;
    }
    if (!mg->wall) mg->wall = calloc(1, sizeof(WALLTAB));
    MG_REQUIRE(mg->wall, MGX_ERR_NOMEM, "set_wall: out of host memory");
    WALLTAB* t = (WALLTAB*)mg->wall;
    memcpy(t->beta, beta, sizeof t->beta);
    memcpy(t->g, g, sizeof t->g);
    t->lossy = lossy;
    t->flux = flux;
    return MGX_OK;
}

int FN(get_wall)(const MGRID* mg, REAL beta[6], REAL g[6]) {
    MG_REQUIRE(mg && beta && g, MGX_ERR_INVALID, "get_wall: NULL");
    const WALLTAB* t = (const WALLTAB*)mg->wall;
    for (int k = 0; k < 6; k++) {
        beta[k] = t ? t->beta[k] : (REAL)0;
        g[k] = t ? t->g[k] : (REAL)0;
    }
    return MGX_OK;
}

/* d_f[0] -= 2 g / h on the face unknowns (mgx3dxs_wall_rhs); without a flux nothing runs */
int FN(add_wall_flux)(MGRID* mg) {
    MG_REQUIRE(mg && mg->grids3D && mg->maxGrids >= 1, MGX_ERR_INVALID, "add_wall_flux: NULL");
    const WALLTAB* t = (const WALLTAB*)mg->wall;
    if (!t || !t->flux) return MGX_OK;
    MG_TRY(MG_CAT(bc_ok3_, R)(mg, mg->bc, "add_wall_flux"));
    GRID* g0 = mg->grids3D[0];
    const REAL h[3] = {g0->h_x, g0->h_y, g0->h_z};
    mg->f_rim_zero[0] = 0;
    return MG_CAT(mgx3dxs_wall_rhs_, R)(mg->ctx, g0->d_f, g0->sizeXYZ, h, t->g, mg->bc);
}

/* the pinned nodes (mg_multigrid.h).  Every call drops the captured graphs: their launches hold the lists. */
int FN(set_pinned)(MGRID* mg, const unsigned char* mask, const REAL* values) {
    MG_REQUIRE(mg && mg->grids3D && mg->maxGrids >= 1, MGX_ERR_INVALID, "set_pinned: NULL");
    const GRID* g0 = mg->grids3D[0];
    const size_t vol0 = MG_CAT(vol3_, R)(g0);
    size_t count0 = 0;
    for (size_t i = 0; mask && i < vol0; i++) count0 += mask[i] != 0;
    if (!count0) { /* no pins: the hierarchy is one that never had any */
        if (!mg->pin) return MGX_OK;
        MG_TRY(mgx_ctx_sync(mg->ctx));
        MG_CAT(coef_drop_graphs3_, R)(mg);
        MG_CAT(pin_table_free3_, R)(mg);
        return MGX_OK;
    }
    MG_REQUIRE(mg->layout == 1, MGX_ERR_INVALID, "set_pinned: pinned nodes need the x-split layout (layout = 1, not natural)");
    MG_REQUIRE(mg->smoother == 0, MGX_ERR_INVALID,
               "set_pinned: pinned nodes need the red-black smoother (smoother = 0): the Jacobi smoother is not available");
    MG_REQUIRE(mg->residual_mode == MGX_RESIDUAL_CORRECT, MGX_ERR_INVALID, "set_pinned: pinned nodes need residual_mode = MGX_RESIDUAL_CORRECT");
    for (size_t i = 0; values && i < vol0; i++)
        MG_REQUIRE(!mask[i] || isfinite((double)values[i]), MGX_ERR_INVALID, "set_pinned: values[%zu] = %g is not finite", i, (double)values[i]);
    unsigned end0[2];
    MG_TRY(MG_CAT(mgx3dxs_pin_list_, R)(g0->sizeXYZ, mask, NULL, NULL, NULL, end0)); /* refuses a boundary point, naming the first one */
    PINTAB* t = (PINTAB*)calloc(1, sizeof(PINTAB));
    MG_REQUIRE(t, MGX_ERR_NOMEM, "set_pinned: out of host memory");
    /* per level on the host: the mask by the coarse rule, the values by injection, the list; then the upload */
    int st = MGX_OK;
    REAL* val_f = NULL; /* the values of the level above at ALL its points */
    for (int l = 0; !st && l < mg->maxGrids; l++) {
        const GRID* g = mg->grids3D[l];
        const int sx = g->sizeX, sy = g->sizeY, sz = g->sizeZ;
        const size_t vol = MG_CAT(vol3_, R)(g);
        unsigned char* m = (unsigned char*)calloc(vol, 1);
        REAL* val = (REAL*)calloc(vol, sizeof(REAL));
        unsigned* idx = NULL;
        REAL* lv = NULL;
        if (!m || !val) st = mg_fail(MGX_ERR_NOMEM, "set_pinned: out of host memory");
        if (!st && l == 0) {
            for (size_t i = 0; i < vol; i++) m[i] = mask[i] != 0;
            if (values) memcpy(val, values, vol * sizeof(REAL));
        } else if (!st) {
            const GRID* gf = mg->grids3D[l - 1];
            const unsigned char* mf = t->h_mask[l - 1];
            const int ax = mg->coarsen[l - 1], fx = gf->sizeX, fy = gf->sizeY;
            const int kx = ax & 1 ? 2 : 1, ky = ax & 2 ? 2 : 1, kz = ax & 4 ? 2 : 1;
            for (int z = 0; z < sz; z++)
                for (int y = 0; y < sy; y++)
                    for (int x = 0; x < sx; x++) {
                        const size_t c = ((size_t)z * sy + y) * sx + x, f = ((size_t)(kz * z) * fy + (size_t)(ky * y)) * fx + (size_t)(kx * x);
                        val[c] = val_f[f];
                        if (x == 0 || x == sx - 1 || y == 0 || y == sy - 1 || z == 0 || z == sz - 1) continue; /* (an interior coarse */
                        int on = mf[f];                                          /* point's fine neighbours are inside the fine grid) */
                        if (ax & 1) on |= mf[f - 1] | mf[f + 1];
                        if (ax & 2) on |= mf[f - (size_t)fx] | mf[f + (size_t)fx];
                        if (ax & 4) on |= mf[f - (size_t)fx * fy] | mf[f + (size_t)fx * fy];
                        m[c] = on != 0;
                    }
        }
        if (!st) st = MG_CAT(mgx3dxs_pin_list_, R)(g->sizeXYZ, m, NULL, NULL, NULL, t->end[l]);
        const unsigned cnt = t->end[l][1];
        if (!st && cnt) {
            idx = (unsigned*)malloc((size_t)cnt * sizeof(unsigned));
            lv = (REAL*)malloc((size_t)cnt * sizeof(REAL));
            if (!idx || !lv) st = mg_fail(MGX_ERR_NOMEM, "set_pinned: out of host memory");
            if (!st) st = MG_CAT(mgx3dxs_pin_list_, R)(g->sizeXYZ, m, val, idx, lv, t->end[l]); /* (the values in list order) */
            if (!st) st = mgx_malloc(mg->ctx, (size_t)cnt * sizeof(unsigned), (void**)&t->d_idx[l]);
            if (!st) st = mgx_malloc(mg->ctx, (size_t)cnt * sizeof(REAL), (void**)&t->d_val[l]);
            if (!st) st = mgx_memcpy_h2d(mg->ctx, t->d_idx[l], idx, (size_t)cnt * sizeof(unsigned));
            if (!st) st = mgx_memcpy_h2d(mg->ctx, t->d_val[l], lv, (size_t)cnt * sizeof(REAL));
        }
        free(idx);
        free(lv);
        free(val_f);
        val_f = val;
        t->h_mask[l] = m;
    }
    free(val_f);
    if (!st) st = mgx_ctx_sync(mg->ctx); /* (nothing of a captured cycle is in flight any more; the uploads are done) */
    PINTAB* old = (PINTAB*)mg->pin;
    mg->pin = t;
    if (st) { /* nothing half-built stays behind: the hierarchy keeps the pins it had */
        MG_CAT(pin_table_free3_, R)(mg);
        mg->pin = old;
        return st;
    }
    MG_CAT(coef_drop_graphs3_, R)(mg);
    mg->pin = old;
    MG_CAT(pin_table_free3_, R)(mg);
    mg->pin = t;
    for (int l = 0; !st && l < mg->maxGrids; l++) st = MG_CAT(pin_put3_, R)(mg, l, mg->grids3D[l]->d_v, 1); /* v = g at the pins */
    if (!st) st = mgx_ctx_sync(mg->ctx);
    return st;
}

int FN(get_pinned)(const MGRID* mg, int gridID, unsigned char* mask) {
    MG_REQUIRE(mg && gridID >= 0 && gridID < mg->maxGrids, MGX_ERR_INVALID, "get_pinned: bad gridID %d", gridID);
    MG_REQUIRE(mask, MGX_ERR_INVALID, "get_pinned: NULL");
    const PINTAB* t = (const PINTAB*)mg->pin;
    const size_t vol = MG_CAT(vol3_, R)(mg->grids3D[gridID]);
    if (t) memcpy(mask, t->h_mask[gridID], vol);
    else memset(mask, 0, vol);
    return MGX_OK;
}

int FN(pinned_count)(const MGRID* mg, int gridID, size_t* count) {
    MG_REQUIRE(mg && gridID >= 0 && gridID < mg->maxGrids, MGX_ERR_INVALID, "pinned_count: bad gridID %d", gridID);
    MG_REQUIRE(count, MGX_ERR_INVALID, "pinned_count: NULL");
    const PINTAB* t = (const PINTAB*)mg->pin;
    *count = t ? (size_t)t->end[gridID][1] : 0;
    return MGX_OK;
}

int FN(Restrict)(MGRID* mg, const REAL* fine, const int fsizeXYZ[3], REAL* coarse, const int csizeXYZ[3]) {
    MG_REQUIRE(mg, MGX_ERR_INVALID, "Restrict: NULL");
    MG_CAT(f_touched3_, R)(mg, coarse); /* boundary = injection of the fine boundary (:113-119) */
    MG_CAT(v_touched3_, R)(mg, coarse);
    if (mg->bc) { /* the coarse unknowns on Neumann faces are restricted too */
        MG_TRY(MG_CAT(bc_ok3_, R)(mg, mg->bc, "Restrict"));
        return MG_CAT(mgx3dxs_restrict_bc_, R)(mg->ctx, fine, fsizeXYZ, coarse, csizeXYZ, mg->bc);
    }
    if (mg->layout && fsizeXYZ && csizeXYZ && (fsizeXYZ[0] == csizeXYZ[0] || fsizeXYZ[1] == csizeXYZ[1] || fsizeXYZ[2] == csizeXYZ[2]))
        return MG_CAT(mgx3dxs_restrict_axes_, R)(mg->ctx, fine, fsizeXYZ, coarse, csizeXYZ); /* a semi-coarsened step */
    return MGXL(mg, restrict)(mg->ctx, fine, fsizeXYZ, coarse, csizeXYZ);
}

int FN(Interpolate)(MGRID* mg, REAL* fine, const int fsizeXYZ[3], const REAL* coarse, const int csizeXYZ[3]) {
    MG_REQUIRE(mg, MGX_ERR_INVALID, "Interpolate: NULL");
    if (mg->bc) { /* ... and the fine unknowns on Neumann faces */
        MG_TRY(MG_CAT(bc_ok3_, R)(mg, mg->bc, "Interpolate"));
        MG_CAT(v_touched3_, R)(mg, fine);
        return MG_CAT(mgx3dxs_interpolate_bc_, R)(mg->ctx, fine, fsizeXYZ, coarse, csizeXYZ, mg->bc);
    }
    /* interior points only (:202-206): no boundary entry changes */
    if (mg->layout && fsizeXYZ && csizeXYZ && (fsizeXYZ[0] == csizeXYZ[0] || fsizeXYZ[1] == csizeXYZ[1] || fsizeXYZ[2] == csizeXYZ[2]))
        return MG_CAT(mgx3dxs_interpolate_axes_, R)(mg->ctx, fine, fsizeXYZ, coarse, csizeXYZ); /* a semi-coarsened step */
    return MGXL(mg, interpolate)(mg->ctx, fine, fsizeXYZ, coarse, csizeXYZ);
}

/* Relax on a hierarchy with pinned nodes: the hierarchy's operator through the _pin entries, which put the level's values (zeros:
 * the level holds a correction) back after every colour pass */
static int MG_CAT(relax_pin3_, R)(MGRID* mg, GRID* curGrid, int lvl, int ncycles, int zeros) {
    const PINTAB* t = (const PINTAB*)mg->pin;
    const REAL h[3] = {curGrid->h_x, curGrid->h_y, curGrid->h_z};
    const REAL* wall = MG_CAT(wall_beta3_, R)(mg);
    const REAL* wb = wall ? wall : MG_CAT(no_wall3_, R);
    const unsigned none[2] = {0, 0};
    const unsigned* idx = lvl >= 0 ? t->d_idx[lvl] : NULL;
    const unsigned* end = lvl >= 0 ? t->end[lvl] : none;
    const REAL* val = lvl >= 0 && !zeros ? t->d_val[lvl] : NULL;
    if (mg->bc) MG_CAT(v_touched3_, R)(mg, curGrid->d_v);
    if (MG_CAT(harm3_, R)(mg))
        return MG_CAT(mgx3dxs_relax_hmean_pin_, R)(mg->ctx, curGrid->d_v, curGrid->d_f, curGrid->d_a, MG_CAT(harm_cap3_, R)(mg, curGrid),
                                                   curGrid->sizeXYZ, h, mg->shift, ncycles, mg->bc, wb, idx, end, val);
    if (MG_CAT(has_cap3_, R)(mg))
        return MG_CAT(mgx3dxs_relax_cap_pin_, R)(mg->ctx, curGrid->d_v, curGrid->d_f, curGrid->d_a, MG_CAT(cap_of3_, R)(mg, curGrid),
                                                 curGrid->sizeXYZ, h, mg->shift, ncycles, mg->bc, wb, idx, end, val);
    if (MG_CAT(has_coef3_, R)(mg))
        return MG_CAT(mgx3dxs_relax_coef_pin_, R)(mg->ctx, curGrid->d_v, curGrid->d_f, curGrid->d_a, curGrid->sizeXYZ, h, mg->shift, ncycles,
                                                  mg->bc, wb, idx, end, val);
    return MG_CAT(mgx3dxs_relax_shift_pin_, R)(mg->ctx, curGrid->d_v, curGrid->d_f, curGrid->sizeXYZ, h, mg->shift, ncycles, mg->bc, wb, idx,
                                               end, val);
}

static int MG_CAT(relax_lvl3_, R)(MGRID* mg, GRID* curGrid, int ncycles, int zeros);

/* the public Relax: the level is the top of a cycle, its pinned points hold the stored values */
int FN(Relax)(MGRID* mg, GRID* curGrid, int ncycles) {
    MG_REQUIRE(mg && curGrid, MGX_ERR_INVALID, "Relax: NULL");
    if (mg->pin) MG_TRY(MG_CAT(pin_put3_, R)(mg, MG_CAT(level_of3_, R)(mg, curGrid), curGrid->d_v, 1)); /* (as VCycle does) */
    return MG_CAT(relax_lvl3_, R)(mg, curGrid, ncycles, 0);
}

/* zeros: the level holds a correction (its pinned points are zeros); counts only with pinned nodes */
static int MG_CAT(relax_lvl3_, R)(MGRID* mg, GRID* curGrid, int ncycles, int zeros) {
    MG_REQUIRE(mg && curGrid, MGX_ERR_INVALID, "Relax: NULL");
    const REAL h[3] = {curGrid->h_x, curGrid->h_y, curGrid->h_z};
    int lvl = -1;
    for (int i = 0; i < mg->maxGrids; i++)
        if (mg->grids3D[i] == curGrid) lvl = i;
    MG_TRY(MG_CAT(op_ok3_, R)(mg, curGrid, "Relax"));
    if (mg->pin) return MG_CAT(relax_pin3_, R)(mg, curGrid, lvl, ncycles, zeros);
    /* the coefficient and the shifted operator: one launch per colour pass; d_e is not used */
    if (mg->bc) MG_CAT(v_touched3_, R)(mg, curGrid->d_v); /* with a mask each colour pass is followed by its launch over the face unknowns */
    const REAL* wall = MG_CAT(wall_beta3_, R)(mg);
    const REAL* wb = wall ? wall : MG_CAT(no_wall3_, R);
    const int faces = mg->bc || wall; /* (betas without a mask: the entry refuses them) */
    if (MG_CAT(harm3_, R)(mg))
        return MG_CAT(mgx3dxs_relax_hmean_wall_, R)(mg->ctx, curGrid->d_v, curGrid->d_f, curGrid->d_a, MG_CAT(harm_cap3_, R)(mg, curGrid),
                                                    curGrid->sizeXYZ, h, mg->shift, ncycles, mg->bc, wb);
    if (MG_CAT(has_cap3_, R)(mg))
        return MG_CAT(mgx3dxs_relax_cap_wall_, R)(mg->ctx, curGrid->d_v, curGrid->d_f, curGrid->d_a, MG_CAT(cap_of3_, R)(mg, curGrid),
                                                  curGrid->sizeXYZ, h, mg->shift, ncycles, mg->bc, wb);
    if (MG_CAT(has_coef3_, R)(mg))
        return MG_CAT(mgx3dxs_relax_coef_wall_, R)(mg->ctx, curGrid->d_v, curGrid->d_f, curGrid->d_a, curGrid->sizeXYZ, h, mg->shift, ncycles,
                                                   mg->bc, wb);
    if (mg->shift != 0 || faces)
        return MG_CAT(mgx3dxs_relax_shift_wall_, R)(mg->ctx, curGrid->d_v, curGrid->d_f, curGrid->sizeXYZ, h, mg->shift, ncycles, mg->bc, wb);
    if (mg->smoother == 1) { /* weighted Jacobi: the error scratch doubles as the ping-pong array */
        if (lvl >= 0) mg->e_rim_valid[lvl] = 0;
        return MGXL(mg, jacobi)(mg->ctx, curGrid->d_v, curGrid->d_e, curGrid->d_f, curGrid->sizeXYZ, h, mg->omega, ncycles);
    }
    if (mg->layout && mg->fuse && lvl >= 0 && MG_CAT(mgx3dxs_relax_pp_takes_, R)(mg->ctx, curGrid->sizeXYZ, ncycles)) {
        /* one launch per red+black sweep, d_e as the ping-pong partner (its boundary is brought up to date once) */
        MG_TRY(MG_CAT(mgx3dxs_relax_pp_, R)(mg->ctx, curGrid->d_v, curGrid->d_e, curGrid->d_f, curGrid->sizeXYZ, h, ncycles,
                                            mg->e_rim_valid[lvl]));
        mg->e_rim_valid[lvl] = 1;
        return MGX_OK;
    }
    return MGXL(mg, relax)(mg->ctx, curGrid->d_v, curGrid->d_f, curGrid->sizeXYZ, h, ncycles);
}

int FN(setToValue)(MGRID* mg, REAL* grid, const int sizeXYZ[3], REAL value, int modifyBoundaries) {
    MG_REQUIRE(mg, MGX_ERR_INVALID, "setToValue: NULL");
    MG_CAT(f_touched3_, R)(mg, grid);
    if (modifyBoundaries) {
        MG_CAT(v_touched3_, R)(mg, grid);
        for (int i = 0; i < mg->maxGrids; i++)
            if (mg->grids3D[i] && mg->grids3D[i]->d_v == grid) mg->v_rim_zero[i] = value == (REAL)0;
    }
    return MGXL(mg, set)(mg->ctx, grid, sizeXYZ, value, modifyBoundaries);
}

/* returns the level-owned residual array (the reference returns a fresh malloc that is
 * never freed, N3/MultiGrid3D.cpp:695) */
int FN(CalculateResidual)(MGRID* mg, GRID* fine, REAL** residual) {
    MG_REQUIRE(mg && fine && residual, MGX_ERR_INVALID, "CalculateResidual: NULL");
    MG_TRY(MG_CAT(op_ok3_, R)(mg, fine, "CalculateResidual"));
    MG_TRY(MG_CAT(op_residual3_, R)(mg, fine, fine->d_v, fine->d_f, fine->d_r, NULL, NULL));
    *residual = fine->d_r;
    return MGX_OK;
}

int FN(ApplyCorrection)(MGRID* mg, REAL* fine, const int fsizeXYZ[3], const REAL* error, const int esizeXYZ[3]) {
    MG_REQUIRE(mg, MGX_ERR_INVALID, "ApplyCorrection: NULL"); /* interior points only (:664-672) */
    return MGXL(mg, apply_correction)(mg->ctx, fine, fsizeXYZ, error, esizeXYZ);
}

/* use_graph: the cycle that starts at gridID is captured once into a HIP graph and replayed while its record (mg_common.h)
 * is unchanged: every host-side input of the launch sequence, the rim flags of levels gridID .. numGrids-1 that pick kernel
 * forms and boundary copies, and the context's generation (its parameters) included.  The body also sets those flags; a
 * replay sets them as its capture did. */
static int MG_CAT(vcycle_graph3_, R)(MGRID* mg, int gridID, int v1, int v2, int (*body)(MGRID*, int, int, int), void** slot_exec,
                                     mgGraphRec* slot_rec, mgGraphFlags* slot_post, unsigned kind, unsigned long long extra) {
    unsigned char* const flags[3] = {mg->f_rim_zero, mg->v_rim_zero, mg->e_rim_valid};
    mgGraphState s;
    memset(&s, 0, sizeof s);
    s.kind = kind;
    s.gridID = gridID; s.v1 = v1; s.v2 = v2; s.numGrids = mg->numGrids;
    s.residual_mode = mg->residual_mode; s.fuse = mg->fuse; s.smoother = mg->smoother;
    s.omega_bits = mg_real_bits(&mg->omega, sizeof(REAL));
    s.extra = extra; /* what else the caller's body depends on */
    s.matrixA_bits[0] = mg_real_bits(&mg->shift, sizeof(REAL)); /* a 3D record has no matrix: the shift's bits (0 without one) */
    s.matrixA_bits[1] = (unsigned long long)(uintptr_t)mg->grids3D[0]->d_a; /* level 0's coefficient array (0 without one): setting or */
                                                                            /* clearing it captures again, new values in it are read  */
    s.matrixA_bits[2] = (unsigned long long)mg->bc; /* the mask of the Neumann faces (0 without one) */
    s.matrixA_bits[3] = (unsigned long long)(uintptr_t)(mg->cap ? ((CAPTAB*)mg->cap)->d_c[0] : NULL); /* level 0's capacity array */
    MG_TRY(mgx_ctx_generation(mg->ctx, &s.generation));
    for (int k = 0; k < 3; k++)
        for (int i = gridID; i < mg->numGrids; i++) s.flags.a[k][i] = flags[k][i];
    mgGraphRec rec;
    mg_graph_record(&s, &rec);
    if (!*slot_exec || !mg_graph_rec_equal(slot_rec, &rec)) {
        if (*slot_exec) MG_TRY(mgx_graph_destroy(mg->ctx, *slot_exec));
        *slot_exec = NULL;
        MG_TRY(mgx_graph_begin(mg->ctx));
        mg->capturing = 1;
        const int st = body(mg, gridID, v1, v2);
        mg->capturing = 0;
        void* exec = NULL;
        const int st2 = mgx_graph_end(mg->ctx, &exec); /* always end the capture, also after an error */
        if (st) {
            if (exec) mgx_graph_destroy(mg->ctx, exec);
            return st;
        }
        MG_TRY(st2);
        *slot_exec = exec;
        *slot_rec = rec;
        for (int k = 0; k < 3; k++) memcpy(slot_post->a[k], flags[k], MG_MAX_LEVELS);
    } else {
        for (int k = 0; k < 3; k++)
            for (int i = gridID; i < mg->numGrids; i++) flags[k][i] = slot_post->a[k][i];
    }
    return mgx_graph_launch(mg->ctx, *slot_exec);
}

static int MG_CAT(vcycle_body3_, R)(MGRID* mg, int gridID, int v1, int v2, int v_zero);

/* One level of the cycle whose step to the next level halves only some axes (coarsen[gridID] != 7): the smoother calls of the
 * other steps around the mgx3dxs_*_axes transfers, nothing fused across them.  Always x-split.  The rim flags as in
 * vcycle_body3_: the coarse f is written whole (boundary 0), the transfers write no boundary entry of v. */
static int MG_CAT(vcycle_semi_step3_, R)(MGRID* mg, int gridID, int v1, int v2, int v_zero) {
    GRID* fine = mg->grids3D[gridID];
    GRID* coarse = mg->grids3D[gridID + 1];
    const REAL h[3] = {fine->h_x, fine->h_y, fine->h_z};
    if (v_zero && mg->fuse && mg->smoother == 0 && v1 > 0) { /* :634 + :626: no fill, the first red pass does not read v */
        if (!mg->v_rim_zero[gridID]) mg->e_rim_valid[gridID] = 0; /* the zero fill changes v's boundary: d_e's copy is stale */
        MG_TRY(MG_CAT(mgx3dxs_relax_from_zero_pp_, R)(mg->ctx, fine->d_v, fine->d_e, fine->d_f, fine->sizeXYZ, h, v1, mg->v_rim_zero[gridID],
                                                      mg->e_rim_valid[gridID]));
        if (MG_CAT(mgx3dxs_relax_from_zero_pp_takes_, R)(mg->ctx, fine->sizeXYZ, v1, mg->v_rim_zero[gridID])) mg->e_rim_valid[gridID] = 1;
        mg->v_rim_zero[gridID] = 1;
    } else {
        if (v_zero) MG_TRY(FN(setToValue)(mg, fine->d_v, fine->sizeXYZ, (REAL)0, 1)); /* :634 */
        MG_TRY(FN(Relax)(mg, fine, v1));                                              /* :626 */
    }
    MG_TRY(MG_CAT(mgx3dxs_residual_restrict_axes_, R)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, h, mg->residual_mode, coarse->d_f,
                                                      coarse->sizeXYZ, mg->f_rim_zero[gridID + 1])); /* :629-632 */
    mg->f_rim_zero[gridID + 1] = 1;
    MG_TRY(MG_CAT(vcycle_body3_, R)(mg, gridID + 1, v1, v2, 1)); /* :634-635 */
    MG_TRY(MG_CAT(mgx3dxs_interpolate_correct_axes_, R)(mg->ctx, fine->d_v, fine->sizeXYZ, coarse->d_v, coarse->sizeXYZ)); /* :638-642 */
    return FN(Relax)(mg, fine, v2); /* :645 */
}

/* One level of the cycle of the shifted (shift != 0) or the variable-coefficient operator, on full and on semi-coarsened steps
 * alike: vcycle_semi_step3_ with the operator's smoother and residual around the plain transfers (the operator does not change
 * how grids are transferred).  The operator decides the settings check, the from-zero smoother and how the coarse f is formed:
 * the shifted one by the fused residual+restrict, the coefficient one by its residual stored into d_r and restricted by the
 * existing transfers (Restrict writes the coarse f whole: its boundary is the injected boundary of r, 0).  One launch per colour
 * pass: the one-launch tail and the fused routes are not taken.  The rim flags as in vcycle_semi_step3_; d_e is never used. */
static int MG_CAT(vcycle_op_step3_, R)(MGRID* mg, int gridID, int v1, int v2, int v_zero) {
    GRID* fine = mg->grids3D[gridID];
    MG_TRY(MG_CAT(op_ok3_, R)(mg, fine, "VCycle"));
    const int coef = MG_CAT(has_coef3_, R)(mg);
    const REAL h[3] = {fine->h_x, fine->h_y, fine->h_z};
    const int bc = mg->bc; /* Neumann faces: no from-zero shortcut (v := 0 on all points, then Relax), the stored-residual route */
    const int pins = mg->pin != NULL; /* pinned nodes: likewise; v_zero says whether the level's pins hold zeros or the values */
    if (!bc && !pins && v_zero && mg->fuse && v1 > 0) { /* :634 + :626: no fill, the first red pass does not read v */
        if (!mg->v_rim_zero[gridID]) mg->e_rim_valid[gridID] = 0; /* the zero fill changes v's boundary: d_e's copy is stale */
        if (MG_CAT(harm3_, R)(mg))
            MG_TRY(MG_CAT(mgx3dxs_relax_hmean_from_zero_, R)(mg->ctx, fine->d_v, fine->d_f, fine->d_a, MG_CAT(harm_cap3_, R)(mg, fine),
                                                             fine->sizeXYZ, h, mg->shift, v1, mg->v_rim_zero[gridID]));
        else if (MG_CAT(has_cap3_, R)(mg))
            MG_TRY(MG_CAT(mgx3dxs_relax_cap_from_zero_, R)(mg->ctx, fine->d_v, fine->d_f, fine->d_a, ((CAPTAB*)mg->cap)->d_c[gridID],
                                                           fine->sizeXYZ, h, mg->shift, v1, mg->v_rim_zero[gridID]));
        else if (coef)
            MG_TRY(MG_CAT(mgx3dxs_relax_coef_from_zero_, R)(mg->ctx, fine->d_v, fine->d_f, fine->d_a, fine->sizeXYZ, h, mg->shift, v1,
                                                            mg->v_rim_zero[gridID]));
        else
            MG_TRY(MG_CAT(mgx3dxs_relax_shift_from_zero_, R)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, h, mg->shift, v1, mg->v_rim_zero[gridID]));
        mg->v_rim_zero[gridID] = 1;
    } else {
        if (v_zero) MG_TRY(FN(setToValue)(mg, fine->d_v, fine->sizeXYZ, (REAL)0, 1)); /* :634 */
        MG_TRY(MG_CAT(relax_lvl3_, R)(mg, fine, v1, v_zero));                         /* :626 */
    }
    if (gridID != mg->numGrids - 1) {
        GRID* coarse = mg->grids3D[gridID + 1];
        const int semi = mg->coarsen[gridID] != 7;
        if (bc) { /* (with pinned nodes op_residual3_ zeroes d_r there before it is restricted) */
            MG_TRY(MG_CAT(op_residual3_, R)(mg, fine, fine->d_v, fine->d_f, fine->d_r, NULL, NULL)); /* :629 */
            MG_TRY(MG_CAT(mgx3dxs_restrict_bc_, R)(mg->ctx, fine->d_r, fine->sizeXYZ, coarse->d_f, coarse->sizeXYZ, bc)); /* :632 */
        } else if (coef || pins) {
            MG_TRY(MG_CAT(op_residual3_, R)(mg, fine, fine->d_v, fine->d_f, fine->d_r, NULL, NULL)); /* :629 */
            if (semi) MG_TRY(MG_CAT(mgx3dxs_restrict_axes_, R)(mg->ctx, fine->d_r, fine->sizeXYZ, coarse->d_f, coarse->sizeXYZ));
            else MG_TRY(MG_CAT(mgx3dxs_restrict_, R)(mg->ctx, fine->d_r, fine->sizeXYZ, coarse->d_f, coarse->sizeXYZ)); /* :632 */
        } else {
            MG_TRY(MG_CAT(mgx3dxs_residual_restrict_shift_, R)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, h, mg->shift, coarse->d_f,
                                                               coarse->sizeXYZ, mg->f_rim_zero[gridID + 1])); /* :629-632 */
        }
        mg->f_rim_zero[gridID + 1] = !bc; /* (the coarse unknowns on Neumann faces hold restricted residuals) */
        MG_TRY(MG_CAT(vcycle_body3_, R)(mg, gridID + 1, v1, v2, 1)); /* :634-635 */
        if (bc) {
            MG_CAT(v_touched3_, R)(mg, fine->d_v);
            MG_TRY(MG_CAT(mgx3dxs_interpolate_correct_bc_, R)(mg->ctx, fine->d_v, fine->sizeXYZ, coarse->d_v, coarse->sizeXYZ, bc));
        } else if (semi) MG_TRY(MG_CAT(mgx3dxs_interpolate_correct_axes_, R)(mg->ctx, fine->d_v, fine->sizeXYZ, coarse->d_v, coarse->sizeXYZ));
        else MG_TRY(MG_CAT(mgx3dxs_interpolate_correct_, R)(mg->ctx, fine->d_v, fine->sizeXYZ, coarse->d_v, coarse->sizeXYZ)); /* :638-642 */
        if (pins) MG_TRY(MG_CAT(pin_put3_, R)(mg, gridID, fine->d_v, !v_zero)); /* the correction has moved the pinned entries */
    }
    return MG_CAT(relax_lvl3_, R)(mg, fine, v2, v_zero); /* :645 */
}

/* VCycle from level gridID down.  v_zero: the level's v counts as all zeros (the coarse error of :634) but has not been
 * zeroed in memory yet -- the one-workgroup tail kernel never reads it, the other levels zero it first. */
static int MG_CAT(vcycle_body3_, R)(MGRID* mg, int gridID, int v1, int v2, int v_zero) {
    if (MG_CAT(has_coef3_, R)(mg) || mg->shift != 0 || mg->bc || mg->pin) return MG_CAT(vcycle_op_step3_, R)(mg, gridID, v1, v2, v_zero);
    GRID* fine = mg->grids3D[gridID];
    const int nlev = mg->numGrids - gridID;
    if (mg->fuse && mg->smoother == 0 && nlev <= 6 && !MG_CAT(semi_below3_, R)(mg, gridID)) { /* levels of at most 17^3: the rest of the cycle in ONE launch */
        int n[18];
        REAL h[18];
        REAL *v[6], *f[6];
        for (int l = 0; l < nlev; l++) {
            GRID* g = mg->grids3D[gridID + l];
            n[3 * l] = g->sizeX; n[3 * l + 1] = g->sizeY; n[3 * l + 2] = g->sizeZ;
            h[3 * l] = g->h_x; h[3 * l + 1] = g->h_y; h[3 * l + 2] = g->h_z;
            v[l] = g->d_v; f[l] = g->d_f;
        }
        if (MGXL(mg, vcycle_tail_fits)(mg->ctx, nlev, n)) {
            MG_TRY(MGXL(mg, vcycle_tail)(mg->ctx, nlev, v, f, n, h, v1, v2, mg->residual_mode, v_zero)); /* :623-647 */
            for (int l = 1; l < nlev; l++) mg->f_rim_zero[gridID + l] = 1; /* written whole, boundary 0 */
            return MGX_OK;
        }
    }
    if (gridID != mg->numGrids - 1 && mg->coarsen[gridID] != 7) return MG_CAT(vcycle_semi_step3_, R)(mg, gridID, v1, v2, v_zero);
    int down_done = 0;
    if (gridID != mg->numGrids - 1 && mg->fuse && mg->layout && mg->smoother == 0 && v1 > 0 &&
        !MG_CAT(mgx3dxs_relax_pp_takes_, R)(mg->ctx, fine->sizeXYZ, v1)) {
        /* :626-632 in one call: on the HBM-bound levels the last black pass runs inside the residual+restrict launch */
        GRID* coarse = mg->grids3D[gridID + 1];
        const REAL hh[3] = {fine->h_x, fine->h_y, fine->h_z};
        if (v_zero && !mg->v_rim_zero[gridID]) mg->e_rim_valid[gridID] = 0; /* the zero fill changes v's boundary: d_e's copy is stale */
        MG_TRY(MG_CAT(mgx3dxs_smooth_residual_restrict_, R)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, hh, v1, v_zero,
                                                            v_zero ? mg->v_rim_zero[gridID] : 0, mg->residual_mode, coarse->d_f,
                                                            coarse->sizeXYZ, mg->f_rim_zero[gridID + 1]));
        if (v_zero) mg->v_rim_zero[gridID] = 1;
        mg->f_rim_zero[gridID + 1] = 1;
        down_done = 1;
    } else if (v_zero && mg->fuse && mg->smoother == 0 && v1 > 0) { /* :634 + :626: no fill, the first red pass does not read v */
        const REAL hh[3] = {fine->h_x, fine->h_y, fine->h_z};
        if (!mg->v_rim_zero[gridID]) mg->e_rim_valid[gridID] = 0; /* the zero fill changes v's boundary: d_e's copy is stale */
        if (mg->layout) { /* d_e as the sweeps' ping-pong partner (one launch per sweep where the level takes it) */
            MG_TRY(MG_CAT(mgx3dxs_relax_from_zero_pp_, R)(mg->ctx, fine->d_v, fine->d_e, fine->d_f, fine->sizeXYZ, hh, v1,
                                                          mg->v_rim_zero[gridID], mg->e_rim_valid[gridID]));
            if (MG_CAT(mgx3dxs_relax_from_zero_pp_takes_, R)(mg->ctx, fine->sizeXYZ, v1, mg->v_rim_zero[gridID])) mg->e_rim_valid[gridID] = 1;
        } else {
            MG_TRY(MGXL(mg, relax_from_zero)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, hh, v1, mg->v_rim_zero[gridID]));
        }
        mg->v_rim_zero[gridID] = 1;
    } else {
        if (v_zero) MG_TRY(FN(setToValue)(mg, fine->d_v, fine->sizeXYZ, (REAL)0, 1)); /* :634 */
        MG_TRY(FN(Relax)(mg, fine, v1)); /* :626 */
    }
    if (gridID != mg->numGrids - 1) {
        GRID* coarse = mg->grids3D[gridID + 1];
        const REAL h[3] = {fine->h_x, fine->h_y, fine->h_z};
        if (down_done) {
            /* residual and restriction went with the pre-smoothing */
        } else if (mg->fuse && mg->f_rim_zero[gridID + 1]) {
            MG_TRY(MGXL(mg, residual_restrict_keep_rim)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, h, mg->residual_mode,
                                                        coarse->d_f, coarse->sizeXYZ)); /* :629-632 */
        } else if (mg->fuse) {
            MG_TRY(MGXL(mg, residual_restrict)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, h, mg->residual_mode, coarse->d_f,
                                          coarse->sizeXYZ)); /* :629-632 */
            mg->f_rim_zero[gridID + 1] = 1;
        } else {
            REAL* residual = NULL;
            MG_TRY(FN(CalculateResidual)(mg, fine, &residual));                                      /* :629 */
            MG_TRY(FN(Restrict)(mg, residual, fine->sizeXYZ, coarse->d_f, coarse->sizeXYZ));         /* :632 */
        }
        MG_TRY(MG_CAT(vcycle_body3_, R)(mg, gridID + 1, v1, v2, 1)); /* :634-635 */
        if (mg->fuse && mg->layout && mg->smoother == 0 && v2 > 0) {
            /* a red-black sweep follows (:645): its red pass rewrites every red interior point from black neighbours
             * alone, so only the black points need the correction, and only for that one pass: the correction and the
             * post-smoothing are one call (on large levels the corrected values are never stored) */
            if (MG_CAT(mgx3dxs_block3_corr_takes_, R)(mg->ctx, fine->sizeXYZ, v2)) {
                /* R', B, R as one in-place launch, then plain passes: neither v's faces nor d_e are touched */
                MG_TRY(MG_CAT(mgx3dxs_interpolate_correct_relax_block3_, R)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, h, coarse->d_v,
                                                                            coarse->sizeXYZ, v2)); /* :638-645 */
                return MGX_OK;
            }
            MG_TRY(MG_CAT(mgx3dxs_interpolate_correct_relax_pp_, R)(mg->ctx, fine->d_v, fine->d_e, fine->d_f, fine->sizeXYZ, h, coarse->d_v,
                                                                    coarse->sizeXYZ, v2, mg->e_rim_valid[gridID])); /* :638-645 */
            if (MG_CAT(mgx3dxs_relax_pp_takes_, R)(mg->ctx, fine->sizeXYZ, v2) && !MG_CAT(mgx3dxs_corr_fused_takes_, R)(mg->ctx, fine->sizeXYZ, fine->sizeZ - 2))
                mg->e_rim_valid[gridID] = 1; /* the sweeps ran on the partner array: its boundary was brought up to date */
            if (MG_CAT(mgx3dxs_block3_up_takes_, R)(mg->ctx, fine->sizeXYZ, v2))
                mg->e_rim_valid[gridID] = 1; /* so did the three-pass launch that reads the correcting pass's red from it */
            return MGX_OK;
        } else if (mg->fuse) {
            MG_TRY(MGXL(mg, interpolate_correct)(mg->ctx, fine->d_v, fine->sizeXYZ, coarse->d_v, coarse->sizeXYZ)); /* :638-642 */
        } else {
            MG_TRY(FN(Interpolate)(mg, fine->d_e, fine->sizeXYZ, coarse->d_v, coarse->sizeXYZ));      /* :640 */
            MG_TRY(FN(ApplyCorrection)(mg, fine->d_v, fine->sizeXYZ, fine->d_e, fine->sizeXYZ));      /* :642 */
        }
    }
    return FN(Relax)(mg, fine, v2); /* :645 */
}

/* MultiGrid3D::VCycle.                                                N3/MultiGrid3D.cpp:623-647 */
int FN(VCycle)(MGRID* mg, int gridID, int v1, int v2) {
    MG_REQUIRE(mg && mg->numGrids >= 1 && mg->numGrids <= mg->maxGrids, MGX_ERR_INVALID, "VCycle: numGrids = %d outside [1,%d]",
               mg ? mg->numGrids : -1, mg ? mg->maxGrids : -1);
    MG_REQUIRE(gridID >= 0 && gridID < mg->numGrids, MGX_ERR_INVALID, "VCycle: bad gridID %d", gridID);
    MG_REQUIRE(v1 >= 0 && v2 >= 0, MGX_ERR_INVALID, "VCycle: negative sweep count");
    if (mg->use_graph && !mg->capturing)
        return MG_CAT(vcycle_graph3_, R)(mg, gridID, v1, v2, FN(VCycle), &mg->graph_exec[gridID], &mg->graph_rec[gridID],
                                         &mg->graph_post[gridID], MG_GRAPH_3D, 0);
    /* the level is the top of a cycle: its pinned points hold the stored values, whatever an earlier cycle that used the level for a
     * correction has left there (nothing without pins) */
    MG_TRY(MG_CAT(pin_put3_, R)(mg, gridID, mg->grids3D[gridID]->d_v, 1));
    return MG_CAT(vcycle_body3_, R)(mg, gridID, v1, v2, 0);
}

/* MultiGrid3D::FullMultiGridVCycle.                                   N3/MultiGrid3D.cpp:569-585 */
int FN(FullMultiGridVCycle)(MGRID* mg, int gridID, int v0, int v1, int v2) {
    MG_REQUIRE(mg && mg->numGrids >= 1 && mg->numGrids <= mg->maxGrids, MGX_ERR_INVALID, "FMG: numGrids = %d outside [1,%d]",
               mg ? mg->numGrids : -1, mg ? mg->maxGrids : -1);
    MG_REQUIRE(gridID >= 0 && gridID < mg->numGrids, MGX_ERR_INVALID, "FMG: bad gridID %d", gridID);
    GRID* fine = mg->grids3D[gridID];
    if (gridID != mg->numGrids - 1) {
        GRID* coarse = mg->grids3D[gridID + 1];
        MG_TRY(FN(Restrict)(mg, fine->d_f, fine->sizeXYZ, coarse->d_f, coarse->sizeXYZ));    /* :575 */
        MG_TRY(FN(FullMultiGridVCycle)(mg, gridID + 1, v0, v1, v2));                         /* :576 */
        MG_TRY(FN(Interpolate)(mg, fine->d_v, fine->sizeXYZ, coarse->d_v, coarse->sizeXYZ)); /* :577 */
        MG_TRY(MG_CAT(pin_put3_, R)(mg, gridID, fine->d_v, 1)); /* the level's pinned values back (nothing without pins) */
    } else {
        MG_TRY(FN(setToValue)(mg, fine->d_v, fine->sizeXYZ, (REAL)0, 0)); /* :581 */
        if (mg->bc) { /* the unknowns on Neumann faces start from zero like the interior; Dirichlet entries stay */
            MG_TRY(MG_CAT(bc_ok3_, R)(mg, mg->bc, "FMG"));
            MG_CAT(v_touched3_, R)(mg, fine->d_v);
            MG_TRY(MG_CAT(mgx3dxs_set_rim_bc_, R)(mg->ctx, fine->d_v, fine->sizeXYZ, (REAL)0, mg->bc));
        }
        MG_TRY(MG_CAT(pin_put3_, R)(mg, gridID, fine->d_v, 1)); /* (the fill has zeroed them) */
    }
    for (int i = 0; i < v0; i++) MG_TRY(FN(VCycle)(mg, gridID, v1, v2)); /* :583-584 */
    return MGX_OK;
}

static int MG_CAT(lvl3_, R)(MGRID* mg, int gridID, GRID** g) {
    MG_REQUIRE(mg && gridID >= 0 && gridID < mg->maxGrids, MGX_ERR_INVALID, "bad gridID %d", gridID);
    *g = mg->grids3D[gridID];
    return MGX_OK;
}

/* host arrays are always in the reference layout (dense); x-split hierarchies convert on the device through
 * a transient dense buffer (not a hot path) */
static int MG_CAT(put3_, R)(MGRID* mg, GRID* g, REAL* dev, const REAL* host) {
    const size_t bytes = MG_CAT(vol3_, R)(g) * sizeof(REAL);
    if (!mg->layout) return mgx_memcpy_h2d(mg->ctx, dev, host, bytes);
    REAL* tmp = NULL;
    MG_TRY(mgx_malloc(mg->ctx, bytes, (void**)&tmp));
    int st = mgx_memcpy_h2d(mg->ctx, tmp, host, bytes);
    if (!st) st = MG_CAT(mgx3dxs_pack_, R)(mg->ctx, tmp, dev, g->sizeXYZ);
    if (!st) st = mgx_ctx_sync(mg->ctx);
    mgx_free(mg->ctx, tmp);
    return st;
}
static int MG_CAT(get3_, R)(MGRID* mg, GRID* g, const REAL* dev, REAL* host) {
    const size_t bytes = MG_CAT(vol3_, R)(g) * sizeof(REAL);
    if (!mg->layout) return mgx_memcpy_d2h(mg->ctx, host, dev, bytes);
    REAL* tmp = NULL;
    MG_TRY(mgx_malloc(mg->ctx, bytes, (void**)&tmp));
    int st = MG_CAT(mgx3dxs_unpack_, R)(mg->ctx, dev, tmp, g->sizeXYZ);
    if (!st) st = mgx_memcpy_d2h(mg->ctx, host, tmp, bytes);
    mgx_free(mg->ctx, tmp);
    return st;
}

int FN(upload_v)(MGRID* mg, int gridID, const REAL* host) {
    GRID* g = NULL; MG_TRY(MG_CAT(lvl3_, R)(mg, gridID, &g));
    MG_REQUIRE(host, MGX_ERR_INVALID, "upload_v: NULL");
    mg->v_rim_zero[gridID] = 0;
    mg->e_rim_valid[gridID] = 0;
    MG_TRY(MG_CAT(put3_, R)(mg, g, g->d_v, host));
    return MG_CAT(pin_put3_, R)(mg, gridID, g->d_v, 1); /* a pinned point keeps its value (nothing without pins) */
}
int FN(upload_f)(MGRID* mg, int gridID, const REAL* host) {
    GRID* g = NULL; MG_TRY(MG_CAT(lvl3_, R)(mg, gridID, &g));
    MG_REQUIRE(host, MGX_ERR_INVALID, "upload_f: NULL");
    mg->f_rim_zero[gridID] = 0;
    return MG_CAT(put3_, R)(mg, g, g->d_f, host);
}
/* host == NULL downloads into the level's own h_v / h_f mirror (allocated on first use) */
int FN(download_v)(MGRID* mg, int gridID, REAL* host) {
    GRID* g = NULL; MG_TRY(MG_CAT(lvl3_, R)(mg, gridID, &g));
    if (!host) {
        if (!g->h_v) g->h_v = (REAL*)malloc(MG_CAT(vol3_, R)(g) * sizeof(REAL));
        MG_REQUIRE(g->h_v, MGX_ERR_NOMEM, "download_v: out of host memory");
        host = g->h_v;
    }
    return MG_CAT(get3_, R)(mg, g, g->d_v, host);
}
int FN(download_f)(MGRID* mg, int gridID, REAL* host) {
    GRID* g = NULL; MG_TRY(MG_CAT(lvl3_, R)(mg, gridID, &g));
    if (!host) {
        if (!g->h_f) g->h_f = (REAL*)malloc(MG_CAT(vol3_, R)(g) * sizeof(REAL));
        MG_REQUIRE(g->h_f, MGX_ERR_NOMEM, "download_f: out of host memory");
        host = g->h_f;
    }
    return MG_CAT(get3_, R)(mg, g, g->d_f, host);
}
/* the residual of level gridID as a host array in the reference layout */
int FN(download_residual)(MGRID* mg, int gridID, REAL* host) {
    GRID* g = NULL; MG_TRY(MG_CAT(lvl3_, R)(mg, gridID, &g));
    MG_REQUIRE(host, MGX_ERR_INVALID, "download_residual: NULL");
    REAL* r = NULL;
    MG_TRY(FN(CalculateResidual)(mg, g, &r));
    return MG_CAT(get3_, R)(mg, g, r, host);
}

/* l2 norm of the residual of level gridID (an addition: the reference has no norm, SURVEY fact 9) */
int FN(ResidualNorm)(MGRID* mg, int gridID, double* l2) {
    GRID* g = NULL; MG_TRY(MG_CAT(lvl3_, R)(mg, gridID, &g));
    MG_REQUIRE(l2, MGX_ERR_INVALID, "ResidualNorm: NULL");
    REAL* r = NULL;
    MG_TRY(FN(CalculateResidual)(mg, g, &r));
    double ss = 0.0;
    MG_TRY(MG_CAT(mgx_norm2_, R)(mg->ctx, r, MG_CAT(dvol3_, R)(mg->layout, g), &ss)); /* pad entries are zero */
    *l2 = sqrt(ss);
    return MGX_OK;
}

int FN(DiffStats)(MGRID* mg, int gridID, double* mean_abs, double* max_abs, double* rel_l2) {
    GRID* g = NULL; MG_TRY(MG_CAT(lvl3_, R)(mg, gridID, &g));
    double* t = (double*)malloc(((size_t)g->sizeX + g->sizeY + g->sizeZ) * sizeof(double));
    MG_REQUIRE(t, MGX_ERR_NOMEM, "DiffStats: out of host memory");
    double *tx = t, *ty = t + g->sizeX, *tz = ty + g->sizeY;
    for (int i = 0; i < g->sizeX; i++) { REAL x = g->x_a + i * g->h_x; tx[i] = sin(MG_PI * x); } /* N3/Grid3D.cpp:146-150 */
    for (int i = 0; i < g->sizeY; i++) { REAL y = g->y_a + i * g->h_y; ty[i] = sin(MG_PI * y); }
    for (int i = 0; i < g->sizeZ; i++) { REAL z = g->z_a + i * g->h_z; tz[i] = sin(MG_PI * z); }
    double out[4] = {0, 0, 0, 0};
    int st = MGXL(mg, diff_stats)(mg->ctx, g->d_v, g->sizeXYZ, tx, ty, tz, out);
    free(t);
    if (st) return st;
    if (mean_abs) *mean_abs = out[0] / (double)MG_CAT(vol3_, R)(g);
    if (max_abs) *max_abs = out[1];
    if (rel_l2) *rel_l2 = out[3] > 0 ? sqrt(out[2] / out[3]) : sqrt(out[2]);
    return MGX_OK;
}

/* ---------------------------------------------------------------- PCG (an addition: the reference only cycles) */
/* preconditioner body: VCycle(gridID, v1, v2) with v[gridID] counting as zero (the graph helper's body signature) */
static int MG_CAT(pcg_vcycle_body3_, R)(MGRID* mg, int gridID, int v1, int v2) {
    return MG_CAT(vcycle_body3_, R)(mg, gridID, v1, v2, 1);
}

/* z = M r: d_v[0] := VCycle from zero with d_f[0] = r */
static int MG_CAT(pcg_precond3_, R)(MGRID* mg, int v1, int v2) {
    if (mg->use_graph)  /* the sequence also depends on whether d_v[0]'s boundary still has to be zeroed */
        return MG_CAT(vcycle_graph3_, R)(mg, 0, v1, v2, MG_CAT(pcg_vcycle_body3_, R), &mg->pcg_graph_exec, &mg->pcg_graph_rec,
                                         &mg->pcg_graph_post, MG_GRAPH_PCG3D, 1 + mg->v_rim_zero[0]);
    return MG_CAT(vcycle_body3_, R)(mg, 0, v1, v2, 1);
}

/* ||b - A x||^2 of level 0 into *ss (blocking, no residual array) */
static int MG_CAT(pcg_true_sumsq3_, R)(MGRID* mg, const REAL* x, const REAL* b, double* ss) {
    GRID* g = mg->grids3D[0];
    const REAL h[3] = {g->h_x, g->h_y, g->h_z};
    if (MG_CAT(wall_beta3_, R)(mg) || mg->pin) /* walls: the hierarchy's residual, not stored; pins: stored in d_r, over the unknowns only */
        MG_TRY(MG_CAT(op_residual3_, R)(mg, g, x, b, NULL, mg->pcg_work, mg->pcg_state + MGX_CG_RR));
    else if (MG_CAT(harm3_, R)(mg))
        MG_TRY(MG_CAT(mgx3dxs_residual_hmean_wall_, R)(mg->ctx, x, b, g->d_a, MG_CAT(harm_cap3_, R)(mg, g), NULL, g->sizeXYZ, h, mg->shift,
                                                       mg->pcg_work, mg->pcg_state + MGX_CG_RR, mg->bc, MG_CAT(no_wall3_, R)));
    else if (MG_CAT(has_cap3_, R)(mg))
        MG_TRY(MG_CAT(mgx3dxs_residual_cap_bc_, R)(mg->ctx, x, b, g->d_a, ((CAPTAB*)mg->cap)->d_c[0], NULL, g->sizeXYZ, h, mg->shift,
                                                   mg->pcg_work, mg->pcg_state + MGX_CG_RR, mg->bc));
    else if (g->d_a)
        MG_TRY(MG_CAT(mgx3dxs_residual_coef_bc_, R)(mg->ctx, x, b, g->d_a, NULL, g->sizeXYZ, h, mg->shift, mg->pcg_work,
                                                    mg->pcg_state + MGX_CG_RR, mg->bc));
    else if (mg->shift != 0 || mg->bc) /* (with a mask: over all unknowns, unweighted) */
        MG_TRY(MG_CAT(mgx3dxs_residual_shift_bc_, R)(mg->ctx, x, b, NULL, g->sizeXYZ, h, mg->shift, mg->pcg_work, mg->pcg_state + MGX_CG_RR,
                                                     mg->bc));
    else
        MG_TRY(MG_CAT(mgx3dxs_residual_sumsq_slab_, R)(mg->ctx, x, b, g->sizeX, g->sizeY, h, MGX_RESIDUAL_CORRECT, 1, g->sizeZ - 1,
                                                       mg->pcg_state + MGX_CG_RR));
    return mgx_memcpy_d2h(mg->ctx, ss, mg->pcg_state + MGX_CG_RR, sizeof(double));
}

/* krylov = 0: plain cycling of d_v[0] with the same stopping rule (the true residual after every cycle) */
static int MG_CAT(pcg_plain3_, R)(MGRID* mg, int v1, int v2, double tol, int maxit, int* iters, double* rel_res, int* converged,
                                  double* host_hist, int hist_cap) {
    GRID* g = mg->grids3D[0];
    double rr0 = 0.0, rr = 0.0;
    MG_TRY(MG_CAT(pcg_true_sumsq3_, R)(mg, g->d_v, g->d_f, &rr0));
    if (rr0 == 0.0) { *converged = 1; return MGX_OK; }
    for (int k = 1; k <= maxit; k++) {
        MG_TRY(FN(VCycle)(mg, 0, v1, v2));
        MG_TRY(MG_CAT(pcg_true_sumsq3_, R)(mg, g->d_v, g->d_f, &rr));
        const double rel = sqrt(rr / rr0);
        if (k - 1 < hist_cap) host_hist[k - 1] = rel;
        *iters = k;
        *rel_res = rel;
        if (rel < tol) { *converged = 1; break; }
        if (!isfinite(rel)) break;
    }
    return MGX_OK;
}

static int MG_CAT(pcg_alloc3_, R)(MGRID* mg) {
    if (mg->pcg_x) return MGX_OK;
    GRID* g = mg->grids3D[0];
    const size_t bytes = MG_CAT(dvol3_, R)(mg->layout, g) * sizeof(REAL);
    /* (the entries for all unknowns put the partials of the face unknowns behind those of the interior: the larger count) */
    const size_t wbytes = MG_CAT(mgx3dxs_krylov_work_elems_bc_, R)(g->sizeXYZ) * sizeof(double);
    int st;
    if ((st = mgx_malloc(mg->ctx, bytes, (void**)&mg->pcg_x)) || (st = mgx_malloc(mg->ctx, bytes, (void**)&mg->pcg_b)) ||
        (st = mgx_malloc(mg->ctx, bytes, (void**)&mg->pcg_p)) || (st = mgx_malloc(mg->ctx, bytes, (void**)&mg->pcg_q)) ||
        (st = mgx_malloc(mg->ctx, MGX_CG_STATE * sizeof(double), (void**)&mg->pcg_state)) ||
        (st = mgx_malloc(mg->ctx, wbytes, (void**)&mg->pcg_work)) ||
        /* p and q: their boundary and pad entries are never written by the kernels; zero them once (q's boundary is read */
        /* by nobody, p's by the Laplacian as zero Dirichlet data).  A solve with a mask writes the face unknowns of both and */
        /* zeroes them again before it returns. */
        (st = mgx_memset_zero(mg->ctx, mg->pcg_p, bytes)) || (st = mgx_memset_zero(mg->ctx, mg->pcg_q, bytes)) ||
        (st = mgx_memset_zero(mg->ctx, mg->pcg_state, MGX_CG_STATE * sizeof(double)))) {
        mgx_free(mg->ctx, mg->pcg_x); mgx_free(mg->ctx, mg->pcg_b); mgx_free(mg->ctx, mg->pcg_p); mgx_free(mg->ctx, mg->pcg_q);
        mgx_free(mg->ctx, mg->pcg_state); mgx_free(mg->ctx, mg->pcg_work);
        mg->pcg_x = mg->pcg_b = mg->pcg_p = mg->pcg_q = NULL;
        mg->pcg_state = mg->pcg_work = NULL;
        return st;
    }
    return MGX_OK;
}

/* flexible CG (the algorithm of mg_multigrid.h).  r lives in d_f[0] (the preconditioner's right-hand side), z in d_v[0] (its
 * result); x, a copy of b, p and q in the scratch.  The update of x by alpha p is deferred into the next direction pass
 * (x += alpha p; p = z + beta p in one pass over p), so an iteration streams 13 reals per point outside the V-cycle:
 * laplace_dot 2, cg_update 3 (r, q -> r), dot2 3 (z, r, q), cg_direction 5 (x, p, z -> x, p).
 * bc: the mask the vector kernels run with -- the hierarchy's (krylov = 2), where r, z, p, q and x live on all unknowns and the
 * dots that make alpha and beta are the weighted ones (DESIGN.md 16), while rr0, the recursive norm and the true-residual check
 * stay unweighted over all unknowns as pcg_plain3_ has them; 0 runs the interior entries and nothing else.
 * singular (the closed box without a shift): the system solved is A x = f - mean_W(f), the projected right-hand side in
 * pcg_fproj, every residual against it, and z := z - mean_W(z) after every preconditioner application, outside its graph. */
static int MG_CAT(pcg_krylov3_, R)(MGRID* mg, int v1, int v2, double tol, int maxit, int* iters, double* rel_res, int* converged,
                                   double* host_hist, int hist_cap, int bc, int singular) {
    mgx_ctx* ctx = mg->ctx;
    GRID* g = mg->grids3D[0];
    const int* n = g->sizeXYZ;
    const size_t bytes = MG_CAT(dvol3_, R)(mg->layout, g) * sizeof(REAL);
    REAL *x = mg->pcg_x, *b = mg->pcg_b, *p = mg->pcg_p, *q = mg->pcg_q, *r = g->d_f, *z = g->d_v;
    double *s = mg->pcg_state, *w = mg->pcg_work;
    const unsigned char v_rim0 = mg->v_rim_zero[0], f_rim0 = mg->f_rim_zero[0];
    MG_TRY(mgx_memcpy_d2d(ctx, x, g->d_v, bytes)); /* x: the guess with its Dirichlet boundary; pads are zero in both */
    MG_TRY(mgx_memcpy_d2d(ctx, b, g->d_f, bytes));
    const REAL* rhs = b;
    if (singular) { /* d_f[0] is restored from b, the caller's f; the removed mean stays in the state vector */
        if (!mg->pcg_fproj) MG_TRY(mgx_malloc(ctx, bytes, (void**)&mg->pcg_fproj));
        MG_TRY(mgx_memcpy_d2d(ctx, mg->pcg_fproj, b, bytes));
        MG_TRY(MG_CAT(mgx3dxs_project_bc_, R)(ctx, mg->pcg_fproj, n, w, s + MGX_CG_FMEAN, bc));
        rhs = mg->pcg_fproj;
    }
    int st = MGX_OK;
    double rr0 = 0.0, rr = 0.0;
    int pending = 0; /* x still lacks alpha p of the last iteration */
    /* r = b - A x (0 on the boundary), ||r0|| */
    st = MG_CAT(op_residual3_, R)(mg, g, x, rhs, r, w, s + MGX_CG_RR);
    mg->f_rim_zero[0] = 0;
    if (!st) st = mgx_memcpy_d2h(ctx, &rr0, s + MGX_CG_RR, sizeof(double));
    if (!st && rr0 == 0.0) *converged = 1;
    int restart = 1; /* z = M r, p = z, rz = <r, z> */
    for (int k = 1; !st && !*converged && k <= maxit; k++) {
        if (restart) {
            st = MG_CAT(pcg_precond3_, R)(mg, v1, v2); /* (ZR is dead until dot2 writes it: the projection's mean goes there) */
            if (!st && singular) st = MG_CAT(mgx3dxs_project_bc_, R)(ctx, z, n, w, s + MGX_CG_ZR, bc);
            if (!st) st = MG_CAT(mgx3dxs_dot2_bc_, R)(ctx, z, r, NULL, n, w, s + MGX_CG_ZR, bc);
            if (!st) st = mgx_cg_scalars(ctx, s, 2);
            if (!st) st = MG_CAT(mgx3dxs_cg_direction_bc_, R)(ctx, NULL, p, z, n, NULL, NULL, bc);
            restart = 0;
        }
        /* q = A p, alpha = <r, z> / <p, q>; r -= alpha q */
        if (!st) st = MG_CAT(op_apply_dot3_, R)(mg, g, p, q, w, s + MGX_CG_PQ);
        if (!st) st = mgx_cg_scalars(ctx, s, 0);
        if (!st) st = MG_CAT(mgx3dxs_cg_update_bc_, R)(ctx, NULL, p, r, q, n, s + MGX_CG_ALPHA, w, s + MGX_CG_RR, bc);
        if (!st) st = mgx_memcpy_d2h(ctx, &rr, s + MGX_CG_RR, sizeof(double)); /* the one host read of the iteration */
        if (st) break;
        *iters = k;
        if (!isfinite(rr)) break; /* breakdown: alpha was NaN; x is the previous iterate */
        pending = 1;
        const double rel = sqrt(rr / rr0);
        if (k - 1 < hist_cap) host_hist[k - 1] = rel;
        if (rel < tol) { /* the recursive residual may have drifted from b - A x: check the true one */
            st = MG_CAT(mgx3dxs_cg_direction_bc_, R)(ctx, x, p, NULL, n, s + MGX_CG_ALPHA, NULL, bc);
            pending = 0;
            if (!st) st = MG_CAT(op_residual3_, R)(mg, g, x, rhs, r, w, s + MGX_CG_RR);
            if (!st) st = mgx_memcpy_d2h(ctx, &rr, s + MGX_CG_RR, sizeof(double));
            if (!st && sqrt(rr / rr0) < tol) *converged = 1;
            restart = 1; /* otherwise go on from the true residual */
            continue;
        }
        /* z = M r; beta = -alpha <z, q> / <r, z>_old; x += alpha p; p = z + beta p */
        st = MG_CAT(pcg_precond3_, R)(mg, v1, v2);
        if (!st && singular) st = MG_CAT(mgx3dxs_project_bc_, R)(ctx, z, n, w, s + MGX_CG_ZR, bc);
        if (!st) st = MG_CAT(mgx3dxs_dot2_bc_, R)(ctx, z, r, q, n, w, s + MGX_CG_ZR, bc);
        if (!st) st = mgx_cg_scalars(ctx, s, 1);
        if (!st) st = MG_CAT(mgx3dxs_cg_direction_bc_, R)(ctx, x, p, z, n, s + MGX_CG_ALPHA, s + MGX_CG_BETA, bc);
        pending = 0;
    }
    if (!st && pending) st = MG_CAT(mgx3dxs_cg_direction_bc_, R)(ctx, x, p, NULL, n, s + MGX_CG_ALPHA, NULL, bc);
    /* the true relative residual of the result */
    if (!st && rr0 > 0.0) {
        double ss = 0.0;
        st = MG_CAT(pcg_true_sumsq3_, R)(mg, x, rhs, &ss);
        if (!st) *rel_res = sqrt(ss / rr0);
    } else if (!st && rr0 != 0.0) {
        *rel_res = rr0; /* NaN: the initial residual is not finite */
    }
    /* d_v[0] := x (its boundary is the guess's), d_f[0] := b; their flags as they were (same boundary contents) -- but with a */
    /* mask x's face unknowns are the solution's, not the guess's: v_rim_zero is then no longer known (a zero guess solved    */
    /* under a mask, the mask cleared, and the next preconditioner would take the rim of its correction for zeros); d_e's     */
    /* boundary copy no longer matches d_v's */
    const int st2 = mgx_memcpy_d2d(ctx, g->d_v, x, bytes);
    const int st3 = mgx_memcpy_d2d(ctx, g->d_f, b, bytes);
    /* the face unknowns of p and q back to the zeros a solve without a mask reads as Dirichlet data */
    const int st4 = MG_CAT(mgx3dxs_set_rim_bc_, R)(ctx, p, n, (REAL)0, bc);
    const int st5 = MG_CAT(mgx3dxs_set_rim_bc_, R)(ctx, q, n, (REAL)0, bc);
    mg->v_rim_zero[0] = bc ? 0 : v_rim0;
    mg->f_rim_zero[0] = f_rim0;
    mg->e_rim_valid[0] = 0;
    if (!st) st = st2 ? st2 : st3 ? st3 : st4 ? st4 : st5;
    if (!st) st = mgx_ctx_sync(ctx);
    return st;
}

int FN(PCG)(MGRID* mg, int v1, int v2, double tol, int maxit, int krylov, int* iters, double* rel_res, int* converged, double* host_hist,
            int hist_cap) {
    MG_REQUIRE(mg && iters && rel_res && converged && (host_hist || hist_cap <= 0), MGX_ERR_INVALID, "PCG: NULL argument");
    MG_REQUIRE(mg->numGrids >= 1 && mg->numGrids <= mg->maxGrids, MGX_ERR_INVALID, "PCG: numGrids = %d outside [1,%d]", mg->numGrids,
               mg->maxGrids);
    MG_REQUIRE(mg->layout == 1, MGX_ERR_INVALID, "PCG: needs the x-split layout (layout = 1)");
    MG_REQUIRE(mg->residual_mode == MGX_RESIDUAL_CORRECT, MGX_ERR_INVALID, "PCG: needs residual_mode = MGX_RESIDUAL_CORRECT");
    MG_REQUIRE(tol > 0 && maxit >= 1 && v1 >= 0 && v2 >= 0 && v1 + v2 >= 1, MGX_ERR_INVALID,
               "PCG: bad arguments (tol %g, maxit %d, v1 %d, v2 %d)", tol, maxit, v1, v2);
    MG_TRY(MG_CAT(shift_ok3_, R)(mg, mg->shift, "PCG"));
    if (MG_CAT(has_coef3_, R)(mg)) MG_TRY(MG_CAT(coef_ok3_, R)(mg, "PCG"));
    MG_REQUIRE(!MG_CAT(has_cap3_, R)(mg) || MG_CAT(has_coef3_, R)(mg), MGX_ERR_INVALID, "PCG: a capacity needs a coefficient (set_coefficient)");
    MG_TRY(MG_CAT(cap_singular3_, R)(mg, "PCG")); /* (not solved in the projected sense: its null space is not the shift's) */
    MG_TRY(MG_CAT(bc_ok3_, R)(mg, mg->bc, "PCG"));
    MG_TRY(MG_CAT(pin_ok3_, R)(mg, "PCG")); /* (the closed box is refused with pins, krylov = 2 included) */
    const int weighted = krylov == MG_KRYLOV_WEIGHTED;
    if (!weighted) MG_TRY(MG_CAT(bc_singular3_, R)(mg, "PCG")); /* (krylov = 2 solves the closed box without a shift, projected) */
    MG_REQUIRE(!mg->bc || !krylov || weighted, MGX_ERR_INVALID,
               "PCG: krylov = %d is not available with Neumann faces (its CG vector kernels are interior-only); use krylov = 2 "
               "(MG_KRYLOV_WEIGHTED: CG in the weighted inner product over all unknowns) or krylov = 0", krylov);
    *iters = 0;
    *rel_res = 0.0;
    *converged = 0;
    MG_TRY(MG_CAT(pcg_alloc3_, R)(mg));
    MG_TRY(mgx_memset_zero(mg->ctx, mg->pcg_state + MGX_CG_FMEAN, sizeof(double)));
    MG_TRY(MG_CAT(pin_put3_, R)(mg, 0, mg->grids3D[0]->d_v, 1)); /* the iterate holds the pinned values before the first residual */
    if (!krylov) return MG_CAT(pcg_plain3_, R)(mg, v1, v2, tol, maxit, iters, rel_res, converged, host_hist, hist_cap);
    const int singular = mg->bc == 63 && mg->shift == 0 && !MG_CAT(wall_beta3_, R)(mg); /* (a lossy wall: regular, nothing projected) */
    mg->bc_reserved = singular; /* "inside a projected solve": cleared on every way out */
    const int st = MG_CAT(pcg_krylov3_, R)(mg, v1, v2, tol, maxit, iters, rel_res, converged, host_hist, hist_cap, mg->bc, singular);
    mg->bc_reserved = 0;
    return st;
}

/* the weighted mean the last PCG removed from the right-hand side (0 unless it solved the closed box without a shift) */
int FN(pcg_removed_mean)(MGRID* mg, double* mean) {
    MG_REQUIRE(mg && mean, MGX_ERR_INVALID, "pcg_removed_mean: NULL argument");
    *mean = 0.0;
    if (!mg->pcg_state) return MGX_OK;
    return mgx_memcpy_d2h(mg->ctx, mean, mg->pcg_state + MGX_CG_FMEAN, sizeof(double));
}

/* implicit steps of u_t = kappa Laplacian(u) + q (an addition; mg_multigrid.h) */
int FN(BackwardEuler)(MGRID* mg, int nsteps, double dt, double kappa, const REAL* d_source, int v1, int v2, double tol, int maxit, int krylov,
                      int* iters_total, double* worst_rel_res, int* converged) {
    MG_REQUIRE(mg && iters_total && worst_rel_res && converged, MGX_ERR_INVALID, "BackwardEuler: NULL argument");
    MG_REQUIRE(nsteps >= 0 && dt > 0 && kappa > 0 && isfinite(dt) && isfinite(kappa), MGX_ERR_INVALID,
               "BackwardEuler: bad arguments (nsteps %d, dt %g, kappa %g)", nsteps, dt, kappa);
    const REAL s = (REAL)(1.0 / (kappa * dt)), qscale = (REAL)(1.0 / kappa);
    MG_REQUIRE(s > 0, MGX_ERR_INVALID, "BackwardEuler: 1 / (kappa dt) = %g is not a positive number of the hierarchy's precision", (double)s);
    MG_TRY(MG_CAT(bc_ok3_, R)(mg, mg->bc, "BackwardEuler"));
    MG_REQUIRE(!mg->bc || !krylov || krylov == MG_KRYLOV_WEIGHTED, MGX_ERR_INVALID,
               "BackwardEuler: krylov = %d is not available with Neumann faces (its CG vector kernels are interior-only); use krylov = 2 "
               "(MG_KRYLOV_WEIGHTED) or krylov = 0", krylov);
    MG_TRY(FN(set_shift)(mg, s)); /* stays set */
    *iters_total = 0;
    *worst_rel_res = 0.0;
    *converged = 1;
    GRID* g = mg->grids3D[0];
    for (int k = 0; k < nsteps; k++) {
        int it = 0, conv = 0;
        double rel = 0.0;
        /* the unknowns only: the Dirichlet entries of d_f[0] are read by nobody and stay as they are (f_rim_zero too, without a mask) */
        if (mg->bc) mg->f_rim_zero[0] = 0;
        if (MG_CAT(has_cap3_, R)(mg)) /* c u_t = kappa div(a grad u) + q: the old u enters weighted by the capacity */
            MG_TRY(MG_CAT(mgx3dxs_cap_rhs_bc_, R)(mg->ctx, g->d_v, ((CAPTAB*)mg->cap)->d_c[0], d_source, qscale, s, g->d_f, g->sizeXYZ, mg->bc));
        else
            MG_TRY(MG_CAT(mgx3dxs_shift_rhs_bc_, R)(mg->ctx, g->d_v, d_source, qscale, s, g->d_f, g->sizeXYZ, mg->bc));
        MG_TRY(FN(add_wall_flux)(mg)); /* the walls' g, in the units of div(a grad u) (nothing without one) */
        MG_TRY(FN(PCG)(mg, v1, v2, tol, maxit, krylov, &it, &rel, &conv, NULL, 0));
        *iters_total += it;
        if (rel > *worst_rel_res || !(rel == rel)) *worst_rel_res = rel;
        if (!conv) { *converged = 0; break; }
    }
    return MGX_OK;
}

int MG_CAT(mg3d_solve_pcg_, R)(mgx_ctx* ctx, REAL* grid, const REAL* rhs, const int sizeXYZ[3], const REAL range[6], int nlevels, int v1,
                               int v2, double tol, int maxit, int krylov, int* iters, double* rel_res, int* converged) {
    MG_REQUIRE(ctx && grid && sizeXYZ && range, MGX_ERR_INVALID, "mg3d_solve_pcg: NULL argument");
    MGRID* mg = NULL;
    MG_TRY(FN(create_levels)(ctx, sizeXYZ, range, 1, nlevels, &mg));
    int st = MGX_OK;
    if (nlevels > 0) {
        if (nlevels > mg->maxGrids) st = mg_fail(MGX_ERR_SIZE, "mg3d_solve_pcg: nlevels %d > %d", nlevels, mg->maxGrids);
        else mg->numGrids = nlevels;
    }
    mg->residual_mode = MGX_RESIDUAL_CORRECT;
    if (!st) st = FN(upload_v)(mg, 0, grid);
    if (!st && rhs) st = FN(upload_f)(mg, 0, rhs);
    if (!st) st = FN(PCG)(mg, v1, v2, tol, maxit, krylov, iters, rel_res, converged, NULL, 0);
    if (!st) st = FN(download_v)(mg, 0, grid);
    FN(destroy)(mg);
    return st;
}

static int MG_CAT(solve3_, R)(mgx_ctx* ctx, REAL* grid, const REAL* rhs, const int sizeXYZ[3], const REAL range[6], int nlevels,
                              int fmg, int v0, int v1, int v2, int ncycles, int residual_mode, int grid_is_zero) {
    MG_REQUIRE(ctx && grid && sizeXYZ && range, MGX_ERR_INVALID, "mg3d_solve: NULL argument");
    MGRID* mg = NULL;
    MG_TRY(FN(create_levels)(ctx, sizeXYZ, range, 1, nlevels, &mg)); /* InitV: v = 0; InitF: the reference's analytic right-hand side */
    int st = MGX_OK;
    if (nlevels > 0) {
        if (nlevels > mg->maxGrids) st = mg_fail(MGX_ERR_SIZE, "mg3d_solve: nlevels %d > %d", nlevels, mg->maxGrids);
        else mg->numGrids = nlevels;
    }
    mg->residual_mode = residual_mode;
    if (!st && !grid_is_zero) st = FN(upload_v)(mg, 0, grid);
    if (!st && rhs) st = FN(upload_f)(mg, 0, rhs);
    if (!st) {
        if (fmg) st = FN(FullMultiGridVCycle)(mg, 0, v0, v1, v2);
        else for (int i = 0; i < ncycles && !st; i++) st = FN(VCycle)(mg, 0, v1, v2);
    }
    if (!st) st = FN(download_v)(mg, 0, grid);
    FN(destroy)(mg);
    return st;
}

int MG_CAT(mg3d_solve_, R)(mgx_ctx* ctx, REAL* grid, const REAL* rhs, const int sizeXYZ[3], const REAL range[6],
                           int nlevels, int fmg, int v0, int v1, int v2, int ncycles, int residual_mode) {
    return MG_CAT(solve3_, R)(ctx, grid, rhs, sizeXYZ, range, nlevels, fmg, v0, v1, v2, ncycles, residual_mode, 0);
}

int MG_CAT(mg3d_solve_from_zero_, R)(mgx_ctx* ctx, REAL* grid_out, const REAL* rhs, const int sizeXYZ[3], const REAL range[6],
                                     int nlevels, int fmg, int v0, int v1, int v2, int ncycles, int residual_mode) {
    return MG_CAT(solve3_, R)(ctx, grid_out, rhs, sizeXYZ, range, nlevels, fmg, v0, v1, v2, ncycles, residual_mode, 1);
}

#undef CAPTAB
#undef PINTAB
#undef WALLTAB
#undef GRID
#undef MGRID
#undef FN
#undef MGXL
