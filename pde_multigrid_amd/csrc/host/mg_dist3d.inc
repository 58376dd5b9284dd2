/* mg_dist3d.inc -- stamped once per real type (REAL, R) by mg_multigrid.c.
 * z-slab decomposition of the 3D V-cycle over the ranks of one node (one process per GPU, RCCL over xGMI).
 * New work: the reference is single-device; its thesis names multi-GPU sub-grids as future work
 * (SURVEY.md section 2, 8e).  Per-point arithmetic is unchanged, so the result is bit-identical to one GPU.
 *
 * Level l (N = sizeZ-1 cells in z) is DISTRIBUTED while every rank still owns >= min_planes planes:
 *   rank r owns the global planes [r*N/P, (r+1)*N/P) (the last rank also the boundary plane N), so the
 *   owner of coarse plane k owns the fine planes 2k and 2k+1 and ownership commutes with coarsening.
 *   Its local array holds, in global z order: 2 ghost planes below (ranks > 0), the owned planes, 1 ghost
 *   plane above (ranks < P-1); x-split layout; planes are contiguous, so ghosts move without packing.
 *   Two ghosts below because the residual of fine plane 2k-1 (needed by the first owned coarse plane k) reads
 *   v at 2k-2.  After every change of v the two adjacent ghosts are refreshed (1 plane up, 1 down); the second
 *   plane below is refreshed once per cycle and level, right before residual+restrict.
 * Levels whose slabs have at least ca_min_planes planes (default 16) run the COMMUNICATION-AVOIDING schedule (the ca_*
 *   functions below): 6 ghost planes on either side, ONE exchange of v per Relax call (4 planes deep for two sweeps)
 *   instead of one per colour pass -- a rank relaxes the first ghost planes itself (the owner's expression on the
 *   owner's inputs: same bits), the region it may trust shrinking by one plane per colour pass.  Per V(2,2) cycle and
 *   level: one exchange of v behind the pre-smoothing, one behind the post-smoothing, one of f (coarse levels).
 * Coarser levels are REPLICATED: the restricted residual of the last distributed level is all-gathered and
 *   every rank runs the remaining levels redundantly with the single-GPU code (bit-identical replicas, no
 *   scatter on the way up). */

#ifndef MG_CA_ALL
#define MG_CA_ALL 99 /* gv / gf: every ghost plane of the level is current */
#endif
#define GRID MG_CAT(mgSlab3D_, R)
#define MGRID MG_CAT(mgDistMultiGrid3D_, R)
#define TAIL MG_CAT(mgMultiGrid3D_, R)
#define FN(name) MG_CAT3(mgDistMultiGrid3D_, R, _##name)
#define TFN(name) MG_CAT3(mgMultiGrid3D_, R, _##name)
#define XS(name) MG_CAT3(mgx3dxs_, name##_, R)

/* elements of one z-plane of the slab arrays (x-split layout: rows padded to cache lines) and of the host's
 * reference-layout arrays */
static size_t MG_CAT(plane3_, R)(const GRID* g) { return MG_CAT(mgx3dxs_plane_elems_, R)(g->sizeXYZ[0], g->sizeXYZ[1]); }
static size_t MG_CAT(hplane3_, R)(const GRID* g) { return (size_t)g->sizeXYZ[0] * g->sizeXYZ[1]; }

static void MG_CAT(slab_free_, R)(mgx_ctx* ctx, GRID* g) {
    if (!g) return;
    mgx_free(ctx, g->d_v);
    mgx_free(ctx, g->d_f);
    free(g);
}

/* Ghost planes of v on a distributed level.  The plane below the slab (zlo-1) and the plane above it (zhi) are
 * refreshed after every change of v: 1 plane up, 1 plane down.  The second plane below (zlo-2) is read only by the
 * residual of plane zlo-1 (restriction of the first owned coarse plane); it is refreshed right before
 * residual+restrict by _exchange2_.  _start_ enqueues the exchange on the comm stream (behind the work the
 * compute stream holds now); mgx_comm_wait makes the compute stream wait for it. */
/* Overlapped or inline?  An overlapped exchange costs two cross-stream dependencies (compute -> comm, comm -> compute:
 * 12.5 us each on MI355X, tools/probes/hop_latency.hip) and splits every pass into three launches; it pays when the interior
 * of a pass takes longer than that.  Levels whose slab (the same on every rank: N / nranks planes) has at most
 * `inline_bytes` of v run their collectives inline on the compute stream instead (mgx_comm_set_inline) with one launch
 * per pass.  Returns the mode in *inl; every rank takes the same decision at the same point. */
static int MG_CAT(slab_mode_, R)(MGRID* mg, const GRID* g, int* inl) {
    const long long bytes = (long long)((g->sizeXYZ[2] - 1) / mg->nranks) * g->sizeXYZ[0] * g->sizeXYZ[1] * (long long)sizeof(REAL);
    const int on = mg->nranks > 1 && mg->inline_bytes > 0 && bytes <= mg->inline_bytes;
    if (inl) *inl = on;
    return mgx_comm_set_inline(mg->ctx, on);
}

static int MG_CAT(slab_exchange_start_, R)(MGRID* mg, GRID* g) {
    if (mg->nranks == 1) return MGX_OK;
    MG_TRY(MG_CAT(slab_mode_, R)(mg, g, NULL));
    const mgSlabPlan* p = &g->plan;
    const size_t pl = MG_CAT(plane3_, R)(g);
    REAL* base = g->d_v;
    /* local index of global plane z is z - zoff */
    const int top = (mg->rank == mg->nranks - 1) ? p->zhi - 1 : p->zhi;           /* one past my top owned cell plane */
    const REAL* send_lo = base + (size_t)(p->zlo - p->zoff) * pl;                  /* my bottom owned plane */
    REAL* recv_lo = base + (size_t)(p->zlo - 1 - p->zoff) * pl;                    /* ghost zlo-1 (ranks > 0 only) */
    const REAL* send_up = base + (size_t)(top - 1 - p->zoff) * pl;                 /* my top owned plane */
    REAL* recv_up = base + (size_t)(p->zhi - p->zoff) * pl;                        /* ghost zhi */
    mg->gv[g->level] = 1;
    mg->n_exchanges++;
    return mgx_comm_halo_exchange(mg->ctx, send_lo, pl, mg->rank > 0 ? recv_lo : NULL, pl, send_up, pl, recv_up, pl,
                                  (int)sizeof(REAL));
}

/* The exchange behind a COLOUR PASS: the pass changed one colour, i.e. one half-row of every row of my bottom and my top owned
 * plane -- only those travel (packed into staging arrays on the compute stream, unpacked into the ghost planes on the stream
 * of the receive): half the bytes on the wire.  A ghost plane of the finest 1025^3 level is 8.4 MB, and its transfer takes as
 * long as the interior launch it hides behind (rehearsal, DESIGN.md section 6). */
static int MG_CAT(slab_exchange_colour_start_, R)(MGRID* mg, GRID* g, int colour) {
    if (mg->nranks == 1) return MGX_OK;
    if (!mg->pack_halos || !mg->d_stage || (colour != 0 && colour != 1)) return MG_CAT(slab_exchange_start_, R)(mg, g);
    MG_TRY(MG_CAT(slab_mode_, R)(mg, g, NULL));
    const mgSlabPlan* p = &g->plan;
    const size_t pl = MG_CAT(plane3_, R)(g);
    const int sx = g->sizeXYZ[0], sy = g->sizeXYZ[1];
    const size_t he = XS(halfplane_elems)(sx, sy);
    const int has_lo = mg->rank > 0, has_up = mg->rank < mg->nranks - 1;
    const int top = has_up ? p->zhi : p->zhi - 1; /* one past my top owned cell plane */
    REAL *s_lo = mg->d_stage, *s_up = s_lo + mg->stage_half, *r_lo = s_up + mg->stage_half, *r_up = r_lo + mg->stage_half;
    REAL* base = g->d_v;
    mg->gv[g->level] = 1;
    mg->n_exchanges++;
    MG_TRY(XS(halo_pack)(mg->ctx, has_lo ? base + (size_t)(p->zlo - p->zoff) * pl : NULL, p->zlo, s_lo,
                         has_up ? base + (size_t)(top - 1 - p->zoff) * pl : NULL, top - 1, s_up, sx, sy, colour));
    MG_TRY(mgx_comm_halo_exchange(mg->ctx, s_lo, he, has_lo ? r_lo : NULL, he, s_up, he, r_up, he, (int)sizeof(REAL)));
    return XS(halo_unpack)(mg->ctx, has_lo ? r_lo : NULL, has_lo ? base + (size_t)(p->zlo - 1 - p->zoff) * pl : NULL, p->zlo - 1,
                           has_up ? r_up : NULL, has_up ? base + (size_t)(p->zhi - p->zoff) * pl : NULL, p->zhi, sx, sy, colour);
}

/* second ghost plane below (zlo-2) <- the lower neighbour's plane top-2; enqueued on the comm stream, the caller
 * orders the compute stream behind it with mgx_comm_wait before the first kernel that reads the plane */
static int MG_CAT(slab_exchange2_start_, R)(MGRID* mg, GRID* g) {
    if (mg->nranks == 1) return MGX_OK;
    MG_TRY(MG_CAT(slab_mode_, R)(mg, g, NULL));
    const mgSlabPlan* p = &g->plan;
    const size_t pl = MG_CAT(plane3_, R)(g);
    const int top = (mg->rank == mg->nranks - 1) ? p->zhi - 1 : p->zhi;
    const REAL* send_up = g->d_v + (size_t)(top - 2 - p->zoff) * pl;
    REAL* recv_lo = mg->rank > 0 ? g->d_v + (size_t)(p->zlo - 2 - p->zoff) * pl : NULL; /* ghost zlo-2 */
    mg->n_exchanges++;
    return mgx_comm_halo_exchange(mg->ctx, NULL, 0, mg->rank > 0 ? recv_lo : NULL, pl, send_up, pl, NULL, 0, (int)sizeof(REAL));
}

/* residual+restrict of the coarse planes [czbeg, czend) of this rank, overlapped with the arrival of the second
 * lower ghost plane: only the first owned coarse plane reads it (its residual plane zlo-1 needs v at zlo-2) */
static int MG_CAT(slab_rr_overlapped_, R)(MGRID* mg, GRID* fine, const REAL h[3], REAL* coarse_f, const int cn[3], int czoff,
                                         int czbeg, int czend) {
    const mgSlabPlan* p = &fine->plan;
    int inl = 0;
    MG_TRY(MG_CAT(slab_mode_, R)(mg, fine, &inl));
    MG_TRY(MG_CAT(slab_exchange2_start_, R)(mg, fine));
    if (inl) { /* the ghost plane arrives in stream order: one launch */
        if (czend > czbeg)
            MG_TRY(XS(residual_restrict_slab)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, p->zoff, h, mg->residual_mode, coarse_f, cn,
                                              czoff, czbeg, czend)); /* :629-632 */
        return MGX_OK;
    }
    if (czend > czbeg + 1)
        MG_TRY(XS(residual_restrict_slab)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, p->zoff, h, mg->residual_mode, coarse_f, cn,
                                          czoff, czbeg + 1, czend)); /* :629-632 */
    MG_TRY(mgx_comm_wait(mg->ctx));
    if (czend > czbeg)
        MG_TRY(XS(residual_restrict_slab)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, p->zoff, h, mg->residual_mode, coarse_f, cn,
                                          czoff, czbeg, czbeg + 1));
    return MGX_OK;
}

/* v += Interpolate(coarse v) on the owned fine planes of the coarse cell-planes [czbeg, czend), then the ghost
 * exchange of v: the two cell-planes that produce the planes a neighbour needs (my bottom and my top owned plane)
 * go first, the exchange travels while the planes in between are corrected */
static int MG_CAT(slab_ic_overlapped_, R)(MGRID* mg, GRID* fine, const REAL* coarse_v, const int cn[3], int czoff, int czbeg,
                                         int czend, int colour) {
    const mgSlabPlan* p = &fine->plan;
    int b1 = czbeg, b2 = czend, inl = 0;
    MG_TRY(MG_CAT(slab_mode_, R)(mg, fine, &inl));
    if (mg->nranks > 1 && czend > czbeg && !inl) {
        b1 = czbeg + 1;
        b2 = czend - 1 > b1 ? czend - 1 : b1;
    }
    if (b1 > czbeg)
        MG_TRY(XS(interpolate_correct_colour_slab)(mg->ctx, fine->d_v, fine->sizeXYZ, p->zoff, coarse_v, cn, czoff, czbeg, b1,
                                                   colour)); /* :638-642 */
    if (czend > b2)
        MG_TRY(XS(interpolate_correct_colour_slab)(mg->ctx, fine->d_v, fine->sizeXYZ, p->zoff, coarse_v, cn, czoff, b2, czend,
                                                   colour));
    if (!inl) MG_TRY(MG_CAT(slab_exchange_colour_start_, R)(mg, fine, colour)); /* colour -1: whole planes */
    if (b2 > b1)
        MG_TRY(XS(interpolate_correct_colour_slab)(mg->ctx, fine->d_v, fine->sizeXYZ, p->zoff, coarse_v, cn, czoff, b1, b2,
                                                   colour));
    if (inl) MG_TRY(MG_CAT(slab_exchange_colour_start_, R)(mg, fine, colour));
    return mgx_comm_wait(mg->ctx);
}

int FN(InitF)(MGRID* mg, int gridID) {
    MG_REQUIRE(mg && gridID >= 0 && gridID < mg->numDist, MGX_ERR_INVALID, "InitF: level %d is not distributed", gridID);
    GRID* g = mg->slabs[gridID];
    const int sx = g->sizeXYZ[0], sy = g->sizeXYZ[1], sz = g->sizeXYZ[2];
    double* t = (double*)malloc(((size_t)sx + sy + sz) * sizeof(double));
    MG_REQUIRE(t, MGX_ERR_NOMEM, "InitF: out of host memory");
    double *tx = t, *ty = t + sx, *tz = ty + sy;
    for (int i = 0; i < sx; i++) { REAL x = g->x_a + i * g->h_x; tx[i] = sin(MG_PI * x); } /* N3/Grid3D.cpp:88-92 */
    for (int i = 0; i < sy; i++) { REAL y = g->y_a + i * g->h_y; ty[i] = sin(MG_PI * y); }
    for (int i = 0; i < sz; i++) { REAL z = g->z_a + i * g->h_z; tz[i] = sin(MG_PI * z); }
    /* init_f works plane by plane, so the slab is initialised in slices of 3 planes (a valid size: odd, >= 3) */
    const size_t pl = MG_CAT(plane3_, R)(g);
    int st = MGX_OK;
    for (int z = 0; z < g->plan.nzl && !st; z += 3) {
        const int z0 = z + 3 <= g->plan.nzl ? z : g->plan.nzl - 3;
        const int n3[3] = {sx, sy, 3};
        st = XS(init_f)(mg->ctx, g->d_f + pl * (size_t)z0, n3, -3 * MG_PI * MG_PI, tx, ty, tz + g->plan.zoff + z0);
    }
    free(t);
    mg->gf[gridID] = MG_CA_ALL;
    return st;
}

int FN(create)(mgx_ctx* ctx, const int finestGridSizeXYZ[3], const REAL range[6], int min_planes, MGRID** out) {
    MG_REQUIRE(ctx && finestGridSizeXYZ && range && out, MGX_ERR_INVALID, "DistMultiGrid3D: NULL argument");
    *out = NULL;
    for (int d = 0; d < 3; d++)
        MG_REQUIRE(finestGridSizeXYZ[d] >= 3 && (finestGridSizeXYZ[d] - 1) % 2 == 0, MGX_ERR_SIZE,
                   "DistMultiGrid3D: size[%d] = %d is not odd and >= 3", d, finestGridSizeXYZ[d]);
    MG_REQUIRE(range[1] > range[0] && range[3] > range[2] && range[5] > range[4], MGX_ERR_INVALID, "DistMultiGrid3D: empty range");
    int minSize = finestGridSizeXYZ[0];
    if (finestGridSizeXYZ[1] < minSize) minSize = finestGridSizeXYZ[1];
    if (finestGridSizeXYZ[2] < minSize) minSize = finestGridSizeXYZ[2];
    MGRID* mg = (MGRID*)calloc(1, sizeof(MGRID));
    MG_REQUIRE(mg, MGX_ERR_NOMEM, "DistMultiGrid3D: out of host memory");
    mg->ctx = ctx;
    mg->residual_mode = MGX_RESIDUAL_REF_COMPAT;
    mgx_comm_rank(ctx, &mg->rank, &mg->nranks);
    mg->numGrids = mg->maxGrids = mg_num_grids(minSize); /* N3/MultiGrid3D.cpp:33-34 */
    mg->numDist = mg_dist_num_levels(finestGridSizeXYZ[2], mg->nranks, mg->maxGrids, min_planes);
    mg->inline_bytes = 96LL << 20; /* slabs of v up to 96 MB: a pass takes less than an overlapped exchange costs */
    mg->ca_min_planes = 16;
    int st = MGX_OK;
    if (mg->numDist > 0) {
        mg->slabs = (GRID**)calloc((size_t)mg->numDist, sizeof(GRID*));
        if (!mg->slabs) { free(mg); return mg_fail(MGX_ERR_NOMEM, "DistMultiGrid3D: out of host memory"); }
    }
    int cur[3] = {finestGridSizeXYZ[0], finestGridSizeXYZ[1], finestGridSizeXYZ[2]};
    for (int l = 0; l < mg->numDist && !st; l++) {
        GRID* g = (GRID*)calloc(1, sizeof(GRID));
        if (!g) { st = mg_fail(MGX_ERR_NOMEM, "DistMultiGrid3D: out of host memory"); break; }
        mg->slabs[l] = g;
        g->level = l;
        mg->gv[l] = mg->gf[l] = MG_CA_ALL; /* zeros / InitF on every local plane */
        for (int d = 0; d < 3; d++) g->sizeXYZ[d] = cur[d];
        g->x_a = range[0]; g->y_a = range[2]; g->z_a = range[4];
        g->h_x = (range[1] - range[0]) / (REAL)(cur[0] - 1); /* N3/Grid3D.cpp:31-45 */
        g->h_y = (range[3] - range[2]) / (REAL)(cur[1] - 1);
        g->h_z = (range[5] - range[4]) / (REAL)(cur[2] - 1);
        st = mg_slab_plan(cur[2], mg->rank, mg->nranks, &g->plan);
        const size_t bytes = MG_CAT(plane3_, R)(g) * (size_t)g->plan.nzl * sizeof(REAL);
        if (!st) st = mgx_malloc(ctx, bytes, (void**)&g->d_v);
        if (!st) st = mgx_malloc(ctx, bytes, (void**)&g->d_f);
        if (!st) st = mgx_memset_zero(ctx, g->d_v, bytes); /* InitV: boundary 0 (interior: see mg_multigrid3d.inc) */
        if (!st) st = mgx_memset_zero(ctx, g->d_f, bytes); /* pad entries of the x-split rows stay zero */
        if (!st) st = FN(InitF)(mg, l);
        mg->v_rim_zero[l] = 1;
        for (int d = 0; d < 3; d++) cur[d] = mg_coarse_size(cur[d]);
    }
    if (!st && mg->numDist > 0 && mg->nranks > 1) { /* staging for the half-plane exchanges: 2 sends + 2 receives of the finest level */
        mg->stage_half = XS(halfplane_elems)(mg->slabs[0]->sizeXYZ[0], mg->slabs[0]->sizeXYZ[1]);
        st = mgx_malloc(ctx, 4 * mg->stage_half * sizeof(REAL), (void**)&mg->d_stage);
        mg->pack_halos = 0; /* measured (rehearsed rank 4 of 8 at 1025^3): 4.52 against 4.36 ms -- the two extra launches cost more than */
                            /* half a transfer that was hidden behind the interior launch anyway; for slabs thin enough that it is not */
    }
    if (!st && mg->numDist < mg->maxGrids) { /* replicated tail, starting at the first non-distributed level */
        st = TFN(create)(ctx, cur, range, &mg->tail);
        if (!st && mg->numDist > 0) {
            /* staging buffer for the all-gather of the tail's finest f: one rank's share of planes */
            const size_t share = MG_CAT(mgx3dxs_plane_elems_, R)(cur[0], cur[1]) * (size_t)((cur[2] - 1) / mg->nranks);
            st = mgx_malloc(ctx, share * sizeof(REAL), (void**)&mg->d_share);
        }
    }
    if (st) { FN(destroy)(mg); return st; }
    *out = mg;
    return MGX_OK;
}

void FN(destroy)(MGRID* mg) {
    if (!mg) return;
    if (mg->slabs)
        for (int l = 0; l < mg->numDist; l++) MG_CAT(slab_free_, R)(mg->ctx, mg->slabs[l]);
    free(mg->slabs);
    if (mg->tail) TFN(destroy)(mg->tail);
    if (mg->graph_exec) mgx_graph_destroy(mg->ctx, mg->graph_exec);
    mgx_free(mg->ctx, mg->d_share);
    mgx_free(mg->ctx, mg->d_stage);
    mgx_free(mg->ctx, mg->d_bplane);
    mgx_free(mg->ctx, mg->d_norm);
    free(mg);
}

/* Relax on a distributed level.                                                           N3/MultiGrid3D.cpp:489-567
 * Each colour pass is split so that the ghost exchange overlaps the bulk of the smoothing:
 *   1. the planes a neighbour needs (my bottom and my top owned plane) are smoothed first on the compute stream,
 *   2. the exchange is enqueued on the comm stream behind them (mgx_comm_halo_exchange orders itself after
 *      what the compute stream holds at that moment),
 *   3. the interior planes are smoothed on the compute stream while the planes travel over xGMI,
 *   4. the compute stream waits for the exchange before the next pass reads the ghosts.
 * A colour pass reads only the other colour, so the three launches are independent of each other. */
typedef struct MG_CAT(mgSlabCorr_, R) { /* the coarse-grid correction the first red pass reads on the fly (NULL: none) */
    const REAL* coarse_v;
    int cn[3], czoff, cplanes;
} MG_CAT(mgSlabCorr_, R);
static int MG_CAT(slab_relax_, R)(MGRID* mg, int gridID, int ncycles, int from_zero, const MG_CAT(mgSlabCorr_, R)* corr, int skip_last_black);
static int MG_CAT(ca_level_, R)(const MGRID* mg, int l);
static int MG_CAT(ca_relax_, R)(MGRID* mg, int l, int K, int kind0, const MG_CAT(mgSlabCorr_, R)* corr, int o, int x, int kint);
static int MG_CAT(ca_settle_, R)(MGRID* mg);
static int MG_CAT(ca_need_, R)(MGRID* mg, int l, int which, int d);
int FN(Relax)(MGRID* mg, int gridID, int ncycles) {
    MG_REQUIRE(mg && gridID >= 0 && gridID < mg->numDist, MGX_ERR_INVALID, "Relax: level %d is not distributed", gridID);
    MG_REQUIRE(ncycles >= 0, MGX_ERR_INVALID, "Relax: ncycles = %d < 0", ncycles);
    if (MG_CAT(ca_level_, R)(mg, gridID)) {
        MG_TRY(MG_CAT(ca_relax_, R)(mg, gridID, 2 * ncycles, 0, NULL, 0, 1, 2 * ncycles));
        return MG_CAT(ca_settle_, R)(mg);
    }
    return MG_CAT(slab_relax_, R)(mg, gridID, ncycles, 0, NULL, 0);
}

/* from_zero: v of the level counts as all zeros (the coarse error at the start of a cycle, :634) although the array has
 * not been zeroed: the first red pass does not read it (and needs no ghosts); it must be followed by a black pass, which
 * rewrites every black interior point (ncycles >= 1).  The caller checks v_rim_zero: the boundary entries of the slab
 * (ghost-plane rims included) must be zero in memory.
 * corr: the first red pass reads the black values through v + Interpolate(coarse) (mgx3dxs_relax_corr_colour_slab; the
 * caller has corrected the set P in place, ghost planes included): :638-645 without a stored correction.
 * skip_last_black: the final black pass is left to the caller (slab_black_rr_: it runs inside the residual+restrict launch). */
static int MG_CAT(slab_relax_, R)(MGRID* mg, int gridID, int ncycles, int from_zero, const MG_CAT(mgSlabCorr_, R)* corr, int skip_last_black) {
    MG_REQUIRE(mg && gridID >= 0 && gridID < mg->numDist, MGX_ERR_INVALID, "Relax: level %d is not distributed", gridID);
    GRID* g = mg->slabs[gridID];
    const REAL h[3] = {g->h_x, g->h_y, g->h_z};
    const mgSlabPlan* p = &g->plan;
    const int sx = g->sizeXYZ[0], sy = g->sizeXYZ[1];
    /* global plane ranges: [ubeg, b1) bottom edge, [b2, uend) top edge, [b1, b2) interior */
    int b1 = p->ubeg, b2 = p->uend, inl = 0;
    MG_TRY(MG_CAT(slab_mode_, R)(mg, g, &inl));
    if (mg->nranks > 1 && !inl) { /* inline mode: no edge planes, the whole slab is the "interior" launch */
        if (mg->rank > 0) b1 = p->ubeg + 1 < p->uend ? p->ubeg + 1 : p->uend;
        if (mg->rank < mg->nranks - 1) b2 = p->uend - 1 > b1 ? p->uend - 1 : b1;
    }
    for (int k = 0; k < ncycles; k++)
        for (int colour = 0; colour < 2; colour++) {
            if (skip_last_black && k == ncycles - 1 && colour == 1) break;
            if (from_zero && k == 0 && colour == 0) {
                MG_TRY(XS(relax_zero_colour_slab)(mg->ctx, g->d_v, g->d_f, sx, sy, h, 0, p->ubeg - p->zoff, p->uend - p->zoff, p->zoff));
                MG_TRY(MG_CAT(slab_exchange_colour_start_, R)(mg, g, 0));
                MG_TRY(mgx_comm_wait(mg->ctx));
                continue;
            }
            if (corr && k == 0 && colour == 0) { /* the three ranges are independent here too: the pass reads black, writes red */
                if (b1 > p->ubeg)
                    MG_TRY(XS(relax_corr_colour_slab)(mg->ctx, g->d_v, g->d_f, g->sizeXYZ, p->zoff, h, corr->coarse_v, corr->cn, corr->czoff,
                                                      corr->cplanes, p->ubeg - p->zoff, b1 - p->zoff));
                if (p->uend > b2)
                    MG_TRY(XS(relax_corr_colour_slab)(mg->ctx, g->d_v, g->d_f, g->sizeXYZ, p->zoff, h, corr->coarse_v, corr->cn, corr->czoff,
                                                      corr->cplanes, b2 - p->zoff, p->uend - p->zoff));
                if (!inl) MG_TRY(MG_CAT(slab_exchange_colour_start_, R)(mg, g, 0));
                if (b2 > b1)
                    MG_TRY(XS(relax_corr_colour_slab)(mg->ctx, g->d_v, g->d_f, g->sizeXYZ, p->zoff, h, corr->coarse_v, corr->cn, corr->czoff,
                                                      corr->cplanes, b1 - p->zoff, b2 - p->zoff));
                if (inl) MG_TRY(MG_CAT(slab_exchange_colour_start_, R)(mg, g, 0));
                MG_TRY(mgx_comm_wait(mg->ctx));
                continue;
            }
            if (b1 > p->ubeg && p->uend > b2) /* a middle rank: both edges in one launch */
                MG_TRY(XS(relax_colour_slab2)(mg->ctx, g->d_v, g->d_f, sx, sy, h, colour, p->ubeg - p->zoff, b1 - p->zoff, b2 - p->zoff,
                                              p->uend - p->zoff, p->zoff));
            else if (b1 > p->ubeg)
                MG_TRY(XS(relax_colour_slab)(mg->ctx, g->d_v, g->d_f, sx, sy, h, colour, p->ubeg - p->zoff, b1 - p->zoff, p->zoff));
            else if (p->uend > b2)
                MG_TRY(XS(relax_colour_slab)(mg->ctx, g->d_v, g->d_f, sx, sy, h, colour, b2 - p->zoff, p->uend - p->zoff, p->zoff));
            if (!inl) MG_TRY(MG_CAT(slab_exchange_colour_start_, R)(mg, g, colour));
            if (b2 > b1)
                MG_TRY(XS(relax_colour_slab)(mg->ctx, g->d_v, g->d_f, sx, sy, h, colour, b1 - p->zoff, b2 - p->zoff, p->zoff));
            if (inl) MG_TRY(MG_CAT(slab_exchange_colour_start_, R)(mg, g, colour));
            MG_TRY(mgx_comm_wait(mg->ctx));
        }
    return MGX_OK;
}

/* The last black pass of the pre-smoothing together with residual+restrict (mgx3dxs_relax_rr_slab, csrc/mgx_relax_rr3d.hip)
 * on a slab.  The fused launch reads red values only, two planes beyond the black planes it relaxes, so it takes the coarse
 * planes whose inputs are all here already -- everything but the first owned coarse plane (ranks > 0) and the last one
 * (ranks < P-1) -- and overlaps the ghost exchanges:
 *   1. the black points of the planes it leaves out (my bottom plane; my top two) by the colour-pass kernel,
 *   2. both ghost exchanges of v (1 up / 1 down, and the second plane below) start behind them on the comm stream,
 *   3. the fused launch: black points of the planes in between + the coarse planes [pA, pB),
 *   4. the compute stream waits for the ghosts; residual+restrict of the one or two coarse planes left (they read the ghosts
 *      and the black values of step 3: stream order).
 * coarse_f / czoff / [czbeg, czend): as slab_rr_overlapped_. */
static int MG_CAT(slab_black_rr_takes_, R)(MGRID* mg, const GRID* fine, const int cn[3], int czbeg, int czend, int v1) {
    int inl = 0;
    if (v1 < 1 || !MG_CAT(mgx3dxs_relax_rr_takes_, R)(mg->ctx, fine->sizeXYZ, cn)) return 0;
    if (MG_CAT(slab_mode_, R)((MGRID*)mg, fine, &inl) || inl) return 0;
    /* the same decision on every rank (the fused form has an exchange of its own): the run of coarse planes a MIDDLE rank would
     * hand to the fused launch, (cn[2] - 1) / nranks - 2, whatever this rank's own run is */
    (void)czbeg;
    (void)czend;
    return (cn[2] - 1) / mg->nranks - 2 >= 4;
}
static int MG_CAT(slab_black_rr_, R)(MGRID* mg, GRID* fine, const REAL h[3], REAL* coarse_f, const int cn[3], int czoff, int czbeg,
                                     int czend) {
    const mgSlabPlan* p = &fine->plan;
    const int sx = fine->sizeXYZ[0], sy = fine->sizeXYZ[1];
    const int pA = mg->rank > 0 ? czbeg + 1 : 1, pB = mg->rank < mg->nranks - 1 ? czend - 1 : cn[2] - 1;
    const int e1 = 2 * pA - 1, e2 = 2 * pB; /* the fused launch stores the black planes [e1, e2) */
    MG_TRY(MG_CAT(slab_mode_, R)(mg, fine, NULL));
    if (e1 > p->ubeg && p->uend > e2)
        MG_TRY(XS(relax_colour_slab2)(mg->ctx, fine->d_v, fine->d_f, sx, sy, h, 1, p->ubeg - p->zoff, e1 - p->zoff, e2 - p->zoff, p->uend - p->zoff,
                                      p->zoff));
    else if (e1 > p->ubeg) MG_TRY(XS(relax_colour_slab)(mg->ctx, fine->d_v, fine->d_f, sx, sy, h, 1, p->ubeg - p->zoff, e1 - p->zoff, p->zoff));
    else if (p->uend > e2) MG_TRY(XS(relax_colour_slab)(mg->ctx, fine->d_v, fine->d_f, sx, sy, h, 1, e2 - p->zoff, p->uend - p->zoff, p->zoff));
    MG_TRY(MG_CAT(slab_exchange_colour_start_, R)(mg, fine, 1));
    MG_TRY(MG_CAT(slab_exchange2_start_, R)(mg, fine));
    MG_TRY(XS(relax_rr_slab)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, p->zoff, h, mg->residual_mode, coarse_f, cn, czoff, pA, pB)); /* :626 (last black pass) + :629-632 */
    MG_TRY(mgx_comm_wait(mg->ctx));
    if (pA > czbeg)
        MG_TRY(XS(residual_restrict_slab)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, p->zoff, h, mg->residual_mode, coarse_f, cn, czoff,
                                          czbeg, pA));
    if (czend > pB)
        MG_TRY(XS(residual_restrict_slab)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, p->zoff, h, mg->residual_mode, coarse_f, cn, czoff,
                                          pB, czend));
    return MGX_OK;
}

/* send my top owned plane of f up: the upper neighbour needs f on its first lower ghost plane to evaluate the
 * residual there (restriction of its first owned coarse plane) */
static int MG_CAT(slab_exchange_f_, R)(MGRID* mg, GRID* g) {
    if (mg->nranks == 1) return MGX_OK;
    MG_TRY(MG_CAT(slab_mode_, R)(mg, g, NULL));
    const mgSlabPlan* p = &g->plan;
    const size_t pl = MG_CAT(plane3_, R)(g);
    const int top = (mg->rank == mg->nranks - 1) ? p->zhi - 1 : p->zhi;
    const REAL* send_up = g->d_f + (size_t)(top - 1 - p->zoff) * pl;
    REAL* recv_lo = g->d_f + (size_t)(p->zlo - 1 - p->zoff) * pl; /* only dereferenced on ranks > 0 */
    mg->n_exchanges++;
    /* No wait here: the plane is first read by the NEXT residual+restrict on this level, and every path to it goes
     * through a later exchange + mgx_comm_wait on the same (in-order) comm stream -- the smoother's, or at v1 = 0 the
     * second-ghost exchange of slab_rr_overlapped_.  Nothing on the compute stream touches the ghost plane of f
     * in between (the smoother reads f on owned planes only). */
    return mgx_comm_halo_exchange(mg->ctx, NULL, 0, mg->rank > 0 ? recv_lo : NULL, pl, send_up, pl, NULL, 0, (int)sizeof(REAL));
}

/* Interpolate + ApplyCorrection + Relax(v2) (:638-645) with the correction read on the fly by the first red pass, as the
 * single-GPU hierarchy does (mgx3dxs_interpolate_correct_relax): the set P is corrected in place on the planes the pass
 * touches -- the owned interior planes and the ghost plane on either side, whose coarse cells lie in the coarse slab's
 * own ghost planes (fresh after any operator of the coarse level) -- then the sweeps.  No corrected array is stored and
 * no exchange of corrected planes is needed: every rank forms the same corrections for the planes it shares. */
static int MG_CAT(slab_corr_takes_, R)(MGRID* mg, const GRID* fine, int v2) {
    /* EVERY rank must take the same decision (the two forms exchange different things): the plane count that decides is the smallest
     * any rank updates -- the last rank's, one less than the others' (found by tests/checkers/fuzz_dist.py: 17 planes on 2 ranks,
     * 8 and 7 planes against the kernel's minimum of 8) */
    const int nmin = (fine->sizeXYZ[2] - 1) / mg->nranks - (mg->nranks > 1 ? 1 : 0);
    return v2 > 0 && MG_CAT(mgx3dxs_corr_fused_takes_, R)(mg->ctx, fine->sizeXYZ, nmin < fine->plan.uend - fine->plan.ubeg ? nmin : fine->plan.uend - fine->plan.ubeg);
}
static int MG_CAT(slab_corr_relax_, R)(MGRID* mg, int gridID, int v2, const REAL* coarse_v, const int cn[3], int czoff, int cplanes) {
    GRID* fine = mg->slabs[gridID];
    const mgSlabPlan* p = &fine->plan;
    const int N = fine->sizeXYZ[2] - 1;
    const int zmin = p->ubeg - 1 > 1 ? p->ubeg - 1 : 1, zmax = p->uend + 1 < N ? p->uend + 1 : N;
    MG_TRY(MG_CAT(slab_mode_, R)(mg, fine, NULL));
    MG_TRY(XS(correct_pset_slab)(mg->ctx, fine->d_v, fine->sizeXYZ, p->zoff, coarse_v, cn, czoff, zmin, zmax));
    MG_CAT(mgSlabCorr_, R) corr;
    corr.coarse_v = coarse_v;
    corr.cn[0] = cn[0]; corr.cn[1] = cn[1]; corr.cn[2] = cn[2];
    corr.czoff = czoff;
    corr.cplanes = cplanes;
    return MG_CAT(slab_relax_, R)(mg, gridID, v2, 0, &corr, 0);
}

/* ====================================================================================================================
 * The communication-avoiding schedule.  N3/MultiGrid3D.cpp:489-567 (Relax) inside :623-647 (VCycle).
 *
 * A colour pass at plane z reads the other colour at z - 1, z, z + 1.  With ghost planes that are current d planes deep, a
 * rank can run k <= d passes without talking to anybody if pass j (0-based) covers the planes [zlo - (k - 1 - j), zhi + (k - 1 - j)):
 * what it computes on ghost planes is what the owner computes (same expression, same inputs, same bits), and what it can
 * no longer trust after pass j lies outside the range of pass j + 1.  So the ghosts are exchanged ONCE per Relax call, x
 * planes deep, where x is what the NEXT consumer of the level reads.
 * Overlap ("split"): the passes run first on the two EDGES of the slab -- the planes whose final values the neighbours
 * are waiting for, bottom edge pass j: [zlo - r, zlo + x + r), top edge: [zhi - x - r, zhi + r), r = k - 1 - j -- then the
 * exchange starts on the comm stream, then the same passes run on the INTERIOR [zlo + x + r, zhi - x - r), which reads
 * owned planes only.  In place and race-free: a pass never reads a plane of its own colour that a later pass of the other
 * region has overwritten (edge pass j + 1 ends one plane short of edge pass j, interior pass j + 1 starts one plane early).
 * gv[l] / gf[l] = how many ghost planes of v / f are current; every reader asks (ca_need_) and only a shortfall exchanges.
 * ==================================================================================================================== */
static int MG_CAT(ca_level_, R)(const MGRID* mg, int l) {
    if (mg->nranks <= 1 || mg->ca_min_planes <= 0 || l < 0 || l >= mg->numDist) return 0;
    const int planes = (mg->slabs[l]->sizeXYZ[2] - 1) / mg->nranks;
    return planes >= mg->ca_min_planes && planes >= 2 * MG_DEEP_MIN_PLANES && planes >= MG_DEEP_GHOSTS + 2;
}
/* ghost planes a level's slabs have on either side */
static int MG_CAT(ca_capacity_, R)(const MGRID* mg, int l) {
    return (mg->slabs[l]->sizeXYZ[2] - 1) / mg->nranks >= MG_DEEP_MIN_PLANES ? MG_DEEP_GHOSTS : 1;
}
/* the compute stream waits for the exchange in flight, if any */
static int MG_CAT(ca_settle_, R)(MGRID* mg) {
    if (!mg->comm_pending) return MGX_OK;
    mg->comm_pending = 0;
    if (mg_ca_trace()) fprintf(stderr, "[ca r%d] wait\n", mg->rank);
    return mgx_comm_wait(mg->ctx);
}
/* ghost planes of `arr` (d_v or d_f of the level), d deep on either side: my planes [zlo - d, zlo) from the lower neighbour's
 * top d planes, [zhi, zhi + d) from the upper neighbour's bottom d planes.  Enqueued behind what the compute stream holds. */
static int MG_CAT(ca_exchange_, R)(MGRID* mg, GRID* g, REAL* arr, int d) {
    const mgSlabPlan* p = &g->plan;
    const size_t pl = MG_CAT(plane3_, R)(g);
    const int has_lo = mg->rank > 0, has_up = mg->rank < mg->nranks - 1;
    MG_REQUIRE(d >= 1 && d <= MG_CAT(ca_capacity_, R)(mg, g->level) && d <= (g->sizeXYZ[2] - 1) / mg->nranks, MGX_ERR_INVALID,
               "ghost exchange: depth %d does not fit level %d", d, g->level);
    MG_TRY(MG_CAT(ca_settle_, R)(mg)); /* one exchange in flight at a time: the comm stream is in order anyway */
    int inl = 0;
    MG_TRY(MG_CAT(slab_mode_, R)(mg, g, &inl));
    const REAL* send_lo = has_lo ? arr + (size_t)(p->zlo - p->zoff) * pl : NULL;
    REAL* recv_lo = has_lo ? arr + (size_t)(p->zlo - d - p->zoff) * pl : NULL;
    const REAL* send_up = has_up ? arr + (size_t)(p->zhi - d - p->zoff) * pl : NULL;
    REAL* recv_up = has_up ? arr + (size_t)(p->zhi - p->zoff) * pl : NULL;
    mg->n_exchanges++;
    if (mg_ca_trace()) fprintf(stderr, "[ca r%d] L%d exchange %s depth %d %s\n", mg->rank, g->level, arr == g->d_v ? "v" : "f", d, inl ? "inline" : "overlapped");
    MG_TRY(mgx_comm_halo_exchange(mg->ctx, send_lo, pl * (size_t)d, recv_lo, pl * (size_t)d, send_up, pl * (size_t)d, recv_up, pl * (size_t)d,
                                  (int)sizeof(REAL)));
    mg->comm_pending = !inl;
    return MGX_OK;
}
/* at least d current ghost planes of v (which = 0) or f (1) on level l, the compute stream ordered behind their arrival */
static int MG_CAT(ca_need_, R)(MGRID* mg, int l, int which, int d) {
    signed char* st = which ? mg->gf : mg->gv;
    if (mg->nranks > 1 && d > 0 && st[l] < d) {
        GRID* g = mg->slabs[l];
        MG_TRY(MG_CAT(ca_exchange_, R)(mg, g, which ? g->d_f : g->d_v, d));
        st[l] = (signed char)d;
    }
    return MG_CAT(ca_settle_, R)(mg);
}

/* pass j of a Relax call (colour j & 1) on the global planes [za, zb) and [zc, zd), zb <= zc (either range may be empty).
 * kind0 (pass 0 only): 1 = the level counts as all zeros, v is not read; 2 = black is read through the correction `corr` */
static int MG_CAT(ca_pass_, R)(MGRID* mg, GRID* g, int j, int kind0, const MG_CAT(mgSlabCorr_, R)* corr, int za, int zb, int zc, int zd) {
    const mgSlabPlan* p = &g->plan;
    const REAL h[3] = {g->h_x, g->h_y, g->h_z};
    const int sx = g->sizeXYZ[0], sy = g->sizeXYZ[1], N = g->sizeXYZ[2] - 1, off = p->zoff;
    if (za < 1) za = 1;
    if (zc < 1) zc = 1;
    if (zb > N) zb = N;
    if (zd > N) zd = N;
    const int n1 = zb > za, n2 = zd > zc;
    if (mg_ca_trace()) fprintf(stderr, "[ca r%d] L%d pass %d kind %d  [%d,%d) [%d,%d)\n", mg->rank, g->level, j, j == 0 ? kind0 : 0, za, n1 ? zb : za, zc, n2 ? zd : zc);
    if (j == 0 && kind0 == 1) {
        if (n1) MG_TRY(XS(relax_zero_colour_slab)(mg->ctx, g->d_v, g->d_f, sx, sy, h, 0, za - off, zb - off, off));
        if (n2) MG_TRY(XS(relax_zero_colour_slab)(mg->ctx, g->d_v, g->d_f, sx, sy, h, 0, zc - off, zd - off, off));
        return MGX_OK;
    }
    if (j == 0 && kind0 == 2) {
        if (n1)
            MG_TRY(XS(relax_corr_colour_slab)(mg->ctx, g->d_v, g->d_f, g->sizeXYZ, off, h, corr->coarse_v, corr->cn, corr->czoff, corr->cplanes,
                                              za - off, zb - off));
        if (n2)
            MG_TRY(XS(relax_corr_colour_slab)(mg->ctx, g->d_v, g->d_f, g->sizeXYZ, off, h, corr->coarse_v, corr->cn, corr->czoff, corr->cplanes,
                                              zc - off, zd - off));
        return MGX_OK;
    }
    if (n1 && n2) return XS(relax_colour_slab2)(mg->ctx, g->d_v, g->d_f, sx, sy, h, j & 1, za - off, zb - off, zc - off, zd - off, off);
    if (n1) return XS(relax_colour_slab)(mg->ctx, g->d_v, g->d_f, sx, sy, h, j & 1, za - off, zb - off, off);
    if (n2) return XS(relax_colour_slab)(mg->ctx, g->d_v, g->d_f, sx, sy, h, j & 1, zc - off, zd - off, off);
    return MGX_OK;
}

/* can k passes followed by an exchange x planes deep run edges first, exchange in flight behind the interior? */
static int MG_CAT(ca_can_split_, R)(MGRID* mg, const GRID* g, int k, int x) {
    int inl = 0;
    if (mg->nranks <= 1 || x <= 0 || MG_CAT(slab_mode_, R)(mg, g, &inl) || inl) return 0;
    return (g->sizeXYZ[2] - 1) / mg->nranks >= 2 * x + 2 * (k - 1) + 3; /* every rank the same answer */
}

/* K colour passes of a CA level, starting with red (pass j: colour j & 1).
 *   kind0 / corr: the first pass, see ca_pass_ (the caller has the coarse ghosts and the set P ready)
 *   o: the LAST pass is to be right o planes beyond the owned ones by redundant work, without an exchange
 *   x: ghost depth to exchange afterwards (0 = none); left in flight in the split form (comm_pending)
 *   kint: passes the INTERIOR runs in the split form -- K, or K - 1 when the caller runs the interior's last black pass
 *         itself (inside the residual+restrict launch); the caller asks ca_can_split_ first.  The bottom edge is then one
 *         plane wider than the x planes that travel: the fused launch stores black values from an ODD plane on, and it
 *         must not store into a plane the exchange in flight is reading (ca_rr_)
 * More than MG_DEEP_GHOSTS passes run in chunks with an exchange in between. */
static int MG_CAT(ca_relax_, R)(MGRID* mg, int l, int K, int kind0, const MG_CAT(mgSlabCorr_, R)* corr, int o, int x, int kint) {
    GRID* g = mg->slabs[l];
    const mgSlabPlan* p = &g->plan;
    const int N = g->sizeXYZ[2] - 1, D = MG_DEEP_GHOSTS;
    const int has_lo = mg->rank > 0, has_up = mg->rank < mg->nranks - 1;
    if (K <= 0) {
        if (x > 0) MG_TRY(MG_CAT(ca_need_, R)(mg, l, 0, x));
        return MGX_OK;
    }
    for (int j0 = 0; j0 < K;) {
        int k, oc, xc;
        if (K - j0 + o <= D) { k = K - j0; oc = o; xc = x; }
        else { k = K - j0 < D ? K - j0 : D; oc = 0; xc = K - j0 - k > 0 ? (K - j0 - k + o <= D ? K - j0 - k + o : D) : (o > x ? o : x); }
        const int last = j0 + k == K;
        const int zero0 = j0 == 0 && kind0 == 1;
        if (zero0) mg->gv[l] = MG_CA_ALL; /* all zeros by contract: every ghost plane "holds" the right value */
        MG_TRY(MG_CAT(ca_need_, R)(mg, l, 1, k - 1 + oc)); /* f where the first pass of the chunk relaxes */
        MG_TRY(MG_CAT(ca_need_, R)(mg, l, 0, k + oc));
        const int split = MG_CAT(ca_can_split_, R)(mg, g, k, xc);
        MG_REQUIRE(split || !last || kint == K, MGX_ERR_INVALID, "ca_relax: the interior's last pass cannot be left out without the split form");
        mg->gv[l] = 0;
        if (split) {
            const int ki = last ? k - (K - kint) : k; /* the caller may keep the interior's very last pass for itself */
            const int wl = xc + (ki < k ? 1 : 0), wu = xc; /* planes of the bottom / top edge the passes finish */
            for (int jj = 0; jj < k; jj++) { /* the edges: what the neighbours wait for */
                const int r = k - 1 - jj;
                MG_TRY(MG_CAT(ca_pass_, R)(mg, g, j0 + jj, kind0, corr, has_lo ? p->zlo - (oc + r) : 0, has_lo ? p->zlo + wl + r : 0,
                                           has_up ? p->zhi - wu - r : N, has_up ? p->zhi + (oc + r) : N));
            }
            MG_TRY(MG_CAT(ca_exchange_, R)(mg, g, g->d_v, xc));
            for (int jj = 0; jj < ki; jj++) {
                const int r = k - 1 - jj;
                MG_TRY(MG_CAT(ca_pass_, R)(mg, g, j0 + jj, kind0, corr, has_lo ? p->zlo + wl + r : 1, has_up ? p->zhi - wu - r : N, N, N));
            }
            mg->gv[l] = (signed char)xc;
        } else {
            for (int jj = 0; jj < k; jj++) {
                const int r = k - 1 - jj;
                MG_TRY(MG_CAT(ca_pass_, R)(mg, g, j0 + jj, kind0, corr, has_lo ? p->zlo - (oc + r) : 1, has_up ? p->zhi + (oc + r) : N, N, N));
            }
            mg->gv[l] = (signed char)oc;
            if (xc > oc) {
                MG_TRY(MG_CAT(ca_exchange_, R)(mg, g, g->d_v, xc));
                mg->gv[l] = (signed char)xc;
            }
        }
        j0 += k;
    }
    return MGX_OK;
}

/* CalculateResidual + Restrict (:629-632) of a CA level into the coarse planes [czbeg, czend) of this rank.
 * black_inside: the interior's last black pass of the pre-smoothing was left out; it runs inside the fused launch
 * (mgx3dxs_relax_rr_slab), which reads red values of owned planes only -- so it runs while the exchange that follows the
 * pre-smoothing is still in flight; the two coarse planes at the bottom and the one at the top that read ghost planes follow
 * behind the wait.  Otherwise: the plain launch, main part first in the same way. */
static int MG_CAT(ca_rr_, R)(MGRID* mg, GRID* fine, const REAL h[3], REAL* coarse_f, const int cn[3], int czoff, int czbeg, int czend,
                            int black_inside, int x) {
    const mgSlabPlan* p = &fine->plan;
    const int has_lo = mg->rank > 0, has_up = mg->rank < mg->nranks - 1;
    const int cend = czend < cn[2] - 1 ? czend : cn[2] - 1; /* one past the last INTERIOR coarse plane of mine */
    int pA = czbeg, pB = czend;
    /* the residual of plane zlo - 1 (first owned coarse plane) reads f there: the pre-smoothing has asked for it unless it had no pass */
    if (mg->gf[fine->level] < 1) MG_TRY(MG_CAT(ca_need_, R)(mg, fine->level, 1, 1));
    if (black_inside) {
        /* the launch stores the black values of the fine planes [2 pA - 1, 2 pB - 1] and reads red from two planes further out:
         * it stays off the planes in flight, [zlo, zlo + x) and [zhi - x, zhi) (x even), whose black values the edge passes
         * have finished (bottom edge x + 1 planes wide, ca_relax_: the first plane the launch stores, zlo + x + 1, is odd) */
        pA = has_lo ? czbeg + x / 2 + 1 : 1;
        pB = has_up ? cend - x / 2 : cend;
        MG_TRY(XS(relax_rr_slab)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, p->zoff, h, mg->residual_mode, coarse_f, cn, czoff, pA, pB)); /* :626 end + :629-632 */
    } else if (mg->comm_pending) {
        pA = has_lo ? czbeg + 1 : czbeg;
        pB = has_up ? czend - 1 : czend;
        if (pB > pA)
            MG_TRY(XS(residual_restrict_slab)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, p->zoff, h, mg->residual_mode, coarse_f, cn, czoff, pA, pB));
    } else {
        pA = pB = czbeg; /* nothing done yet: one launch below */
    }
    MG_TRY(MG_CAT(ca_need_, R)(mg, fine->level, 0, 2));
    if (pA == pB && !black_inside) return czend > czbeg ? XS(residual_restrict_slab)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, p->zoff, h, mg->residual_mode,
                                                                                   coarse_f, cn, czoff, czbeg, czend)
                                                        : MGX_OK;
    if (pA > czbeg)
        MG_TRY(XS(residual_restrict_slab)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, p->zoff, h, mg->residual_mode, coarse_f, cn, czoff, czbeg, pA));
    if (czend > pB)
        MG_TRY(XS(residual_restrict_slab)(mg->ctx, fine->d_v, fine->d_f, fine->sizeXYZ, p->zoff, h, mg->residual_mode, coarse_f, cn, czoff, pB, czend));
    return MGX_OK;
}

/* ghost depth the level's next reader wants behind its post-smoothing: level 0 the next cycle's pre-smoothing (or its
 * residual), a coarser level the finer level's correction (coarse planes up to (zhi + k) / 2 for a first chunk of k passes) */
static int MG_CAT(ca_first_chunk_, R)(int sweeps) { return 2 * sweeps < MG_DEEP_GHOSTS ? 2 * sweeps : MG_DEEP_GHOSTS; }
static int MG_CAT(ca_x_post_, R)(int l, int v1, int v2) {
    if (l == 0) { const int k = MG_CAT(ca_first_chunk_, R)(v1); return k > 2 ? k : 2; }
    return v2 > 0 ? MG_CAT(ca_first_chunk_, R)(v2) / 2 + 1 : 1;
}

/* Relax(v1) (:626, from zero: :634 first) + residual + restrict of a CA level */
static int MG_CAT(ca_down_, R)(MGRID* mg, int l, int v1, int v2, int v_zero, REAL* coarse_f, const int cn[3], int czoff, int czbeg, int czend) {
    GRID* fine = mg->slabs[l];
    const REAL h[3] = {fine->h_x, fine->h_y, fine->h_z};
    int kind0 = 0;
    if (v_zero) {
        if (v1 > 0 && mg->v_rim_zero[l]) kind0 = 1;
        else MG_TRY(FN(zero_v)(mg, l)); /* :634 */
    }
    /* behind the pre-smoothing: what the way up reads (its first chunk of passes), at least the 2 planes of the residual */
    int x = v2 > 0 ? MG_CAT(ca_first_chunk_, R)(v2) : 2;
    if (x < 2) x = 2;
    const int K = 2 * v1;
    const int black_inside = K >= 2 && K <= MG_DEEP_GHOSTS && MG_CAT(ca_can_split_, R)(mg, fine, K, x) &&
                             MG_CAT(mgx3dxs_relax_rr_takes_, R)(mg->ctx, fine->sizeXYZ, cn) && (cn[2] - 1) / mg->nranks - (x + 1) >= 4 && x <= 4 && (x & 1) == 0;
    MG_TRY(MG_CAT(ca_relax_, R)(mg, l, K, kind0, NULL, 0, x, black_inside ? K - 1 : K));
    return MG_CAT(ca_rr_, R)(mg, fine, h, coarse_f, cn, czoff, czbeg, czend, black_inside, x);
}

/* Interpolate + ApplyCorrection + Relax(v2) (:638-645) of a CA level, v2 >= 1: the correction is formed on the ghost planes
 * too (their coarse cells lie in the coarse slab's ghost planes, or in the replicated level), so no corrected plane travels;
 * coarse_level: the coarse level's index if it is distributed, -1 if it is the replicated one */
static int MG_CAT(ca_up_, R)(MGRID* mg, int l, int v1, int v2, const REAL* coarse_v, const int cn[3], int czoff, int cplanes, int coarse_level) {
    GRID* fine = mg->slabs[l];
    const mgSlabPlan* p = &fine->plan;
    const int N = fine->sizeXYZ[2] - 1;
    const int K = 2 * v2, k0 = MG_CAT(ca_first_chunk_, R)(v2);
    const int has_lo = mg->rank > 0, has_up = mg->rank < mg->nranks - 1;
    MG_TRY(MG_CAT(ca_need_, R)(mg, l, 0, k0));
    if (coarse_level >= 0) MG_TRY(MG_CAT(ca_need_, R)(mg, coarse_level, 0, k0 / 2 + 1));
    /* the planes whose black points the first red pass reads: its own range and one plane either side */
    const int zmin = has_lo ? p->zlo - k0 : 1, zmax = has_up ? p->zhi + k0 : N;
    MG_CAT(mgSlabCorr_, R) corr;
    corr.coarse_v = coarse_v;
    corr.cn[0] = cn[0]; corr.cn[1] = cn[1]; corr.cn[2] = cn[2];
    corr.czoff = czoff;
    corr.cplanes = cplanes;
    int kind0 = 0;
    /* the correction read on the fly by the first red pass (no corrected array is stored) pays on thick slabs; the correcting
     * kernel is the pipelined one, whose launch floor (~17 us at 513-point rows, tools/slab_pass_time.py) the two edge launches
     * of a thin slab pay in full: below 96 planes per rank the black points are corrected in place by one launch and the passes
     * are plain ones (rehearsed rank 4 of 8 at 1025^3, 513-level: see DESIGN.md section 6) */
    if (MG_CAT(slab_corr_takes_, R)(mg, fine, v2) && (fine->sizeXYZ[2] - 1) / mg->nranks >= 96) {
        MG_TRY(XS(correct_pset_slab)(mg->ctx, fine->d_v, fine->sizeXYZ, p->zoff, coarse_v, cn, czoff, zmin > 1 ? zmin : 1, zmax));
        kind0 = 2;
    } else { /* the black points corrected in place (the red pass that follows rewrites every red point it covers) */
        MG_TRY(XS(interpolate_correct_colour_slab)(mg->ctx, fine->d_v, fine->sizeXYZ, p->zoff, coarse_v, cn, czoff, zmin / 2, zmax / 2, 1));
    }
    return MG_CAT(ca_relax_, R)(mg, l, K, kind0, &corr, 0, MG_CAT(ca_x_post_, R)(l, v1, v2), K);
}

/* VCycle with levels < numDist distributed and the rest replicated.                      N3/MultiGrid3D.cpp:623-647 */
static int MG_CAT(dist_vcycle_body_, R)(MGRID* mg, int gridID, int v1, int v2, int v_zero);
/* use_graph: the cycle from level 0 is captured once (compute and comm stream, collectives included) and replayed; the record
 * holds every host-side input of the launch sequence, as in mgMultiGrid3D (the flags that pick kernel forms change during the
 * first cycles: a changed record captures again, and a replay leaves the flags as its capture did) */
static int MG_CAT(dist_vcycle_graph_, R)(MGRID* mg, int v1, int v2) {
    MG_REQUIRE(mgx_comm_capturable(mg->ctx), MGX_ERR_INVALID, "VCycle: use_graph needs collectives that can be captured (RCCL or one rank)");
    if (!mg->graph_warm) { /* workspaces and the like are allocated on first use, which a capture does not allow */
        mg->graph_warm = 1;
        MG_TRY(MG_CAT(dist_vcycle_body_, R)(mg, 0, v1, v2, 0));
        return MG_CAT(ca_settle_, R)(mg);
    }
    unsigned char* const flags[6] = {mg->v_rim_zero, (unsigned char*)mg->gv, (unsigned char*)mg->gf,
                                     mg->tail ? mg->tail->f_rim_zero : NULL, mg->tail ? mg->tail->v_rim_zero : NULL,
                                     mg->tail ? mg->tail->e_rim_valid : NULL};
    mgGraphState s;
    memset(&s, 0, sizeof s);
    s.kind = MG_GRAPH_SLAB;
    s.v1 = v1; s.v2 = v2; s.numGrids = mg->numGrids; s.residual_mode = mg->residual_mode;
    s.ca_min_planes = mg->ca_min_planes;
    s.inline_bytes = (unsigned long long)mg->inline_bytes;
    s.extra = (unsigned)mg->pack_halos;
    if (mg->tail) {
        s.fuse = mg->tail->fuse; s.smoother = mg->tail->smoother;
        s.omega_bits = mg_real_bits(&mg->tail->omega, sizeof(REAL));
    }
    MG_TRY(mgx_ctx_generation(mg->ctx, &s.generation));
    for (int k = 0; k < 6; k++)
        if (flags[k]) memcpy(s.flags.a[k], flags[k], MG_MAX_LEVELS);
    mgGraphRec rec;
    mg_graph_record(&s, &rec);
    if (!mg->graph_exec || !mg_graph_rec_equal(&mg->graph_rec, &rec)) {
        if (mg->graph_exec) MG_TRY(mgx_graph_destroy(mg->ctx, mg->graph_exec));
        mg->graph_exec = NULL;
        MG_TRY(mgx_graph_begin(mg->ctx));
        int st = MG_CAT(dist_vcycle_body_, R)(mg, 0, v1, v2, 0);
        if (!st) st = MG_CAT(ca_settle_, R)(mg);
        void* exec = NULL;
        const int st2 = mgx_graph_end(mg->ctx, &exec); /* always end the capture, also after an error */
        if (st) {
            if (exec) mgx_graph_destroy(mg->ctx, exec);
            return st;
        }
        MG_TRY(st2);
        mg->graph_exec = exec;
        mg->graph_rec = rec;
        for (int k = 0; k < 6; k++)
            if (flags[k]) memcpy(mg->graph_post.a[k], flags[k], MG_MAX_LEVELS);
    } else { /* the flags as the captured cycle left them */
        for (int k = 0; k < 6; k++)
            if (flags[k]) memcpy(flags[k], mg->graph_post.a[k], MG_MAX_LEVELS);
        if (mg->tail && mg->numGrids > mg->numDist) {
            mg->tail->numGrids = mg->numGrids - mg->numDist;
            mg->tail->residual_mode = mg->residual_mode;
        }
    }
    return mgx_graph_launch(mg->ctx, mg->graph_exec);
}

int FN(VCycle)(MGRID* mg, int gridID, int v1, int v2) {
    MG_REQUIRE(mg && mg->numGrids >= 1 && mg->numGrids <= mg->maxGrids, MGX_ERR_INVALID, "VCycle: numGrids = %d outside [1,%d]",
               mg ? mg->numGrids : -1, mg ? mg->maxGrids : -1);
    MG_REQUIRE(gridID >= 0 && gridID < mg->numGrids, MGX_ERR_INVALID, "VCycle: bad gridID %d", gridID);
    MG_REQUIRE(!mg->tail || mg->tail->shift == 0, MGX_ERR_INVALID, "VCycle: a shifted hierarchy is not supported on slabs");
    MG_REQUIRE(v1 >= 0 && v2 >= 0, MGX_ERR_INVALID, "VCycle: negative sweep count");
    if (mg->use_graph && gridID == 0) return MG_CAT(dist_vcycle_graph_, R)(mg, v1, v2);
    MG_TRY(MG_CAT(dist_vcycle_body_, R)(mg, gridID, v1, v2, 0));
    return MG_CAT(ca_settle_, R)(mg); /* the exchange behind the last post-smoothing */
}

/* v_zero: the level's v counts as all zeros (:634) but has not been zeroed in memory yet */
static int MG_CAT(dist_vcycle_body_, R)(MGRID* mg, int gridID, int v1, int v2, int v_zero) {
    if (gridID >= mg->numDist) { /* fully replicated from here */
        mg->tail->numGrids = mg->numGrids - mg->numDist;
        mg->tail->residual_mode = mg->residual_mode;
        return MG_CAT(vcycle_body3_, R)(mg->tail, gridID - mg->numDist, v1, v2, v_zero);
    }
    GRID* fine = mg->slabs[gridID];
    const mgSlabPlan* p = &fine->plan;
    const REAL h[3] = {fine->h_x, fine->h_y, fine->h_z};
    const int N = fine->sizeXYZ[2] - 1;
    const int cn[3] = {mg_coarse_size(fine->sizeXYZ[0]), mg_coarse_size(fine->sizeXYZ[1]), mg_coarse_size(fine->sizeXYZ[2])};
    const int czlo = p->zlo / 2;                        /* first coarse plane this rank owns */
    const int pzint = (p->zhi < N ? p->zhi : N) / 2;    /* one past the last coarse cell-plane whose fine planes I own */
    /* the coarse planes this rank restricts into: its slab of the next level, or its share of the replicated level */
    const int rr_end = gridID + 1 < mg->numDist ? ((mg->rank == mg->nranks - 1) ? cn[2] : p->zhi / 2) : czlo + (cn[2] - 1) / mg->nranks;
    const int ca = MG_CAT(ca_level_, R)(mg, gridID); /* one exchange per Relax call instead of one per colour pass */
    if (ca && gridID == mg->numGrids - 1) { /* the coarsest level of this cycle: Relax(v1), Relax(v2) (:626, :645) */
        int kind0 = 0;
        if (v_zero) {
            if (v1 > 0 && mg->v_rim_zero[gridID]) kind0 = 1;
            else MG_TRY(FN(zero_v)(mg, gridID));
        }
        MG_TRY(MG_CAT(ca_relax_, R)(mg, gridID, 2 * v1, kind0, NULL, 0, 0, 2 * v1));
        return MG_CAT(ca_relax_, R)(mg, gridID, 2 * v2, 0, NULL, 0, MG_CAT(ca_x_post_, R)(gridID, v1, v2), 2 * v2);
    }
    const int black_rr = !ca && gridID != mg->numGrids - 1 && MG_CAT(slab_black_rr_takes_, R)(mg, fine, cn, czlo, rr_end, v1);
    if (ca) {
        /* pre-smoothing and residual+restrict together below (ca_down_) */
    } else if (v_zero && v1 > 0 && mg->v_rim_zero[gridID]) {
        MG_TRY(MG_CAT(slab_relax_, R)(mg, gridID, v1, 1, NULL, black_rr)); /* :634 + :626 without the zero fill */
    } else {
        if (v_zero) MG_TRY(FN(zero_v)(mg, gridID)); /* :634 */
        MG_TRY(MG_CAT(slab_relax_, R)(mg, gridID, v1, 0, NULL, black_rr)); /* :626 */
    }
    if (gridID != mg->numGrids - 1) {
        if (gridID + 1 < mg->numDist) {
            GRID* coarse = mg->slabs[gridID + 1];
            const int czhi = rr_end;
            if (ca) MG_TRY(MG_CAT(ca_down_, R)(mg, gridID, v1, v2, v_zero, coarse->d_f, cn, coarse->plan.zoff, czlo, czhi)); /* :626-632 */
            else if (black_rr) MG_TRY(MG_CAT(slab_black_rr_, R)(mg, fine, h, coarse->d_f, cn, coarse->plan.zoff, czlo, czhi)); /* :626 end + :629-632 */
            else MG_TRY(MG_CAT(slab_rr_overlapped_, R)(mg, fine, h, coarse->d_f, cn, coarse->plan.zoff, czlo, czhi)); /* :629-632 */
            mg->gf[gridID + 1] = 0; /* the coarse f has been rewritten on the owned planes only */
            if (!MG_CAT(ca_level_, R)(mg, gridID + 1)) MG_TRY(MG_CAT(slab_exchange_f_, R)(mg, coarse)); /* a CA level asks for what it reads */
            MG_TRY(MG_CAT(dist_vcycle_body_, R)(mg, gridID + 1, v1, v2, 1)); /* :634-635 */
            if (ca && v2 > 0) return MG_CAT(ca_up_, R)(mg, gridID, v1, v2, coarse->d_v, cn, coarse->plan.zoff, coarse->plan.nzl, gridID + 1); /* :638-645 */
            MG_TRY(MG_CAT(ca_settle_, R)(mg));
            if (MG_CAT(slab_corr_takes_, R)(mg, fine, v2))
                return MG_CAT(slab_corr_relax_, R)(mg, gridID, v2, coarse->d_v, cn, coarse->plan.zoff, coarse->plan.nzl); /* :638-645 */
            /* v2 > 0: black points only, the red pass that follows rewrites every red interior point (mg_multigrid3d.inc) */
            MG_TRY(MG_CAT(slab_ic_overlapped_, R)(mg, fine, coarse->d_v, cn, coarse->plan.zoff, czlo, pzint, v2 > 0 ? 1 : -1));
        } else {
            /* agglomeration: every rank restricts its share of coarse planes, the shares are all-gathered into
             * the replicated level's f (its last plane is a boundary plane: restricted residual = 0 there) and
             * every rank runs the rest of the cycle redundantly */
            TAIL* t = mg->tail;
            MG_REQUIRE(t, MGX_ERR_INVALID, "VCycle: no replicated tail");
            t->numGrids = mg->numGrids - mg->numDist;
            t->residual_mode = mg->residual_mode;
            const size_t cpl = MG_CAT(mgx3dxs_plane_elems_, R)(cn[0], cn[1]);
            const int share = (cn[2] - 1) / mg->nranks;
            REAL* tf = t->grids3D[0]->d_f;
            if (ca)
                MG_TRY(MG_CAT(ca_down_, R)(mg, gridID, v1, v2, v_zero, mg->nranks > 1 ? mg->d_share : tf, cn, mg->nranks > 1 ? czlo : 0, czlo, czlo + share));
            else if (black_rr)
                MG_TRY(MG_CAT(slab_black_rr_, R)(mg, fine, h, mg->nranks > 1 ? mg->d_share : tf, cn, mg->nranks > 1 ? czlo : 0, czlo, czlo + share));
            else
                MG_TRY(MG_CAT(slab_rr_overlapped_, R)(mg, fine, h, mg->nranks > 1 ? mg->d_share : tf, cn, mg->nranks > 1 ? czlo : 0,
                                                      czlo, czlo + share));
            if (mg->nranks > 1) {
                MG_TRY(MG_CAT(ca_settle_, R)(mg));
                mg->n_exchanges++;
                MG_TRY(mgx_comm_allgather(mg->ctx, mg->d_share, tf, cpl * (size_t)share, (int)sizeof(REAL)));
            }
            MG_TRY(mgx_memset_zero(mg->ctx, tf + cpl * (size_t)(cn[2] - 1), cpl * sizeof(REAL)));
            MG_TRY(mgx_comm_wait(mg->ctx));
            MG_TRY(MG_CAT(vcycle_body3_, R)(t, 0, v1, v2, 1)); /* :634-635 */
            if (ca && v2 > 0) return MG_CAT(ca_up_, R)(mg, gridID, v1, v2, t->grids3D[0]->d_v, cn, 0, cn[2], -1); /* :638-645 */
            MG_TRY(MG_CAT(ca_settle_, R)(mg));
            if (MG_CAT(slab_corr_takes_, R)(mg, fine, v2))
                return MG_CAT(slab_corr_relax_, R)(mg, gridID, v2, t->grids3D[0]->d_v, cn, 0, cn[2]); /* :638-645 */
            MG_TRY(MG_CAT(slab_ic_overlapped_, R)(mg, fine, t->grids3D[0]->d_v, cn, 0, czlo, pzint, v2 > 0 ? 1 : -1));
        }
    }
    return FN(Relax)(mg, gridID, v2); /* :645 */
}

/* MultiGrid3D::FullMultiGridVCycle on slabs.                                              N3/MultiGrid3D.cpp:569-585
 * Restrict(f) needs the fine f on the plane below the slab (the ghost every writer of f keeps fresh), Interpolate the
 * coarse v on the plane above the coarse slab (fresh after any Relax / Interpolate of that level). */
int FN(FullMultiGridVCycle)(MGRID* mg, int gridID, int v0, int v1, int v2) {
    MG_REQUIRE(mg && mg->numGrids >= 1 && mg->numGrids <= mg->maxGrids, MGX_ERR_INVALID, "FMG: numGrids = %d outside [1,%d]",
               mg ? mg->numGrids : -1, mg ? mg->maxGrids : -1);
    MG_REQUIRE(gridID >= 0 && gridID < mg->numGrids, MGX_ERR_INVALID, "FMG: bad gridID %d", gridID);
    MG_REQUIRE(!mg->tail || mg->tail->shift == 0, MGX_ERR_INVALID, "FMG: a shifted hierarchy is not supported on slabs");
    if (gridID >= mg->numDist) {
        mg->tail->numGrids = mg->numGrids - mg->numDist;
        mg->tail->residual_mode = mg->residual_mode;
        return TFN(FullMultiGridVCycle)(mg->tail, gridID - mg->numDist, v0, v1, v2);
    }
    GRID* fine = mg->slabs[gridID];
    const mgSlabPlan* p = &fine->plan;
    const int N = fine->sizeXYZ[2] - 1;
    if (gridID == mg->numGrids - 1) { /* the coarsest level of the cycle is a distributed one: v := 0 on the interior (:581) */
        const int zb = p->zlo > 1 ? p->zlo : 1, ze = p->zhi < N ? p->zhi : N; /* owned interior planes */
        MG_TRY(MG_CAT(ca_settle_, R)(mg));
        MG_TRY(XS(set_interior_slab)(mg->ctx, fine->d_v, fine->sizeXYZ[0], fine->sizeXYZ[1], zb - p->zoff, ze - p->zoff, (REAL)0));
        MG_TRY(MG_CAT(slab_exchange_start_, R)(mg, fine));
        MG_TRY(mgx_comm_wait(mg->ctx));
        for (int i = 0; i < v0; i++) MG_TRY(FN(VCycle)(mg, gridID, v1, v2)); /* :583-584 */
        return MGX_OK;
    }
    const int cn[3] = {mg_coarse_size(fine->sizeXYZ[0]), mg_coarse_size(fine->sizeXYZ[1]), mg_coarse_size(fine->sizeXYZ[2])};
    const int czlo = p->zlo / 2;
    const int pzint = (p->zhi < N ? p->zhi : N) / 2;
    const int last = mg->rank == mg->nranks - 1;
    const REAL* coarse_v = NULL;
    int coarse_zoff = 0;
    MG_TRY(MG_CAT(ca_need_, R)(mg, gridID, 1, MG_CAT(ca_capacity_, R)(mg, gridID) > 1 ? 1 : 0)); /* Restrict reads f on the plane below the slab */
    if (gridID + 1 < mg->numDist) {
        GRID* coarse = mg->slabs[gridID + 1];
        const int czhi = last ? cn[2] : p->zhi / 2;
        MG_TRY(XS(restrict_slab)(mg->ctx, fine->d_f, fine->sizeXYZ, p->zoff, coarse->d_f, cn, coarse->plan.zoff, czlo, czhi)); /* :575 */
        mg->gf[gridID + 1] = 0;
        if (MG_CAT(ca_capacity_, R)(mg, gridID + 1) > 1) {
            MG_TRY(MG_CAT(ca_need_, R)(mg, gridID + 1, 1, 1));
        } else {
            MG_TRY(MG_CAT(slab_exchange_f_, R)(mg, coarse));
            MG_TRY(mgx_comm_wait(mg->ctx)); /* the next level's Restrict reads the ghost right away */
        }
        coarse_v = coarse->d_v;
        coarse_zoff = coarse->plan.zoff;
    } else {
        TAIL* t = mg->tail;
        const size_t cpl = MG_CAT(mgx3dxs_plane_elems_, R)(cn[0], cn[1]);
        const int share = (cn[2] - 1) / mg->nranks;
        REAL* tf = t->grids3D[0]->d_f;
        if (mg->nranks > 1) {
            if (!mg->d_bplane) MG_TRY(mgx_malloc(mg->ctx, cpl * (size_t)(mg->nranks + 1) * sizeof(REAL), (void**)&mg->d_bplane));
            MG_TRY(XS(restrict_slab)(mg->ctx, fine->d_f, fine->sizeXYZ, p->zoff, mg->d_share, cn, czlo, czlo, czlo + share)); /* :575 */
            MG_TRY(mgx_comm_allgather(mg->ctx, mg->d_share, tf, cpl * (size_t)share, (int)sizeof(REAL)));
            /* the top boundary plane (injection of the fine boundary plane, :113-119) exists on the last rank only */
            REAL* mine = mg->d_bplane + cpl * (size_t)mg->nranks;
            if (last) MG_TRY(XS(restrict_slab)(mg->ctx, fine->d_f, fine->sizeXYZ, p->zoff, mine, cn, cn[2] - 1, cn[2] - 1, cn[2]));
            else MG_TRY(mgx_memset_zero(mg->ctx, mine, cpl * sizeof(REAL)));
            MG_TRY(mgx_comm_allgather(mg->ctx, mine, mg->d_bplane, cpl, (int)sizeof(REAL)));
            MG_TRY(mgx_comm_wait(mg->ctx));
            MG_TRY(mgx_memcpy_d2d(mg->ctx, tf + cpl * (size_t)(cn[2] - 1), mg->d_bplane + cpl * (size_t)(mg->nranks - 1),
                                  cpl * sizeof(REAL)));
        } else {
            MG_TRY(XS(restrict_slab)(mg->ctx, fine->d_f, fine->sizeXYZ, p->zoff, tf, cn, 0, 0, cn[2])); /* :575 */
        }
        coarse_v = t->grids3D[0]->d_v;
    }
    MG_TRY(FN(FullMultiGridVCycle)(mg, gridID + 1, v0, v1, v2));                                               /* :576 */
    if (gridID + 1 < mg->numDist) MG_TRY(MG_CAT(ca_need_, R)(mg, gridID + 1, 0, 1)); /* Interpolate reads the coarse plane above the coarse slab */
    MG_TRY(MG_CAT(ca_settle_, R)(mg));
    MG_TRY(XS(interpolate_slab)(mg->ctx, fine->d_v, fine->sizeXYZ, p->zoff, coarse_v, cn, coarse_zoff, czlo, pzint)); /* :577 */
    MG_TRY(MG_CAT(slab_exchange_start_, R)(mg, fine));
    MG_TRY(mgx_comm_wait(mg->ctx));
    for (int i = 0; i < v0; i++) MG_TRY(FN(VCycle)(mg, gridID, v1, v2)); /* :583-584 */
    return MGX_OK;
}

/* squared l2 norm of the residual of distributed level gridID over the whole grid -> d_norm[slot] on every rank:
 * the rank's own planes on the compute stream, then one all-reduce of one double on the comm stream.  The ghost
 * planes of v next to the owned planes are fresh after every operator of the cycle (Relax / correction end with
 * the exchange + wait). */
static int MG_CAT(slab_norm_, R)(MGRID* mg, int gridID, int slot) {
    MG_REQUIRE(mg && gridID >= 0 && gridID < mg->numDist, MGX_ERR_INVALID, "ResidualNorm: level %d is not distributed", gridID);
    if (!mg->d_norm) {
        MG_TRY(mgx_malloc(mg->ctx, (MG_NORM_HISTORY + 1) * sizeof(double), (void**)&mg->d_norm));
        MG_TRY(mgx_memset_zero(mg->ctx, mg->d_norm, (MG_NORM_HISTORY + 1) * sizeof(double)));
    }
    GRID* g = mg->slabs[gridID];
    const mgSlabPlan* p = &g->plan;
    const REAL h[3] = {g->h_x, g->h_y, g->h_z};
    MG_TRY(MG_CAT(ca_need_, R)(mg, gridID, 0, 1)); /* the planes next to the owned ones */
    MG_TRY(XS(residual_sumsq_slab)(mg->ctx, g->d_v, g->d_f, g->sizeXYZ[0], g->sizeXYZ[1], h, mg->residual_mode,
                                   p->ubeg - p->zoff, p->uend - p->zoff, mg->d_norm + slot)); /* N3/MultiGrid3D.cpp:723 */
    mg->n_exchanges++;
    MG_TRY(mgx_comm_allreduce_sum_f64(mg->ctx, mg->d_norm + slot, 1));
    return mgx_comm_wait(mg->ctx);
}

int FN(ResidualNorm)(MGRID* mg, int gridID, double* l2) {
    MG_REQUIRE(l2, MGX_ERR_INVALID, "ResidualNorm: NULL");
    MG_TRY(MG_CAT(slab_norm_, R)(mg, gridID, 0));
    double ss = 0.0;
    MG_TRY(mgx_memcpy_d2h(mg->ctx, &ss, mg->d_norm, sizeof ss)); /* blocking on the compute stream */
    *l2 = sqrt(ss);
    return MGX_OK;
}

int FN(ResidualNormRecord)(MGRID* mg, int gridID) {
    MG_REQUIRE(mg && mg->norm_count < MG_NORM_HISTORY, MGX_ERR_INVALID, "ResidualNormRecord: history full (%d entries)", MG_NORM_HISTORY);
    MG_TRY(MG_CAT(slab_norm_, R)(mg, gridID, 1 + mg->norm_count));
    mg->norm_count++;
    return MGX_OK;
}

int FN(ResidualNormHistory)(MGRID* mg, double* host_l2, int capacity, int* count) {
    MG_REQUIRE(mg && host_l2 && count && capacity >= 0, MGX_ERR_INVALID, "ResidualNormHistory: bad argument");
    const int n = mg->norm_count < capacity ? mg->norm_count : capacity;
    *count = n;
    if (n == 0) return MGX_OK;
    MG_TRY(mgx_memcpy_d2h(mg->ctx, host_l2, mg->d_norm + 1, (size_t)n * sizeof(double)));
    for (int i = 0; i < n; i++) host_l2[i] = sqrt(host_l2[i]);
    return MGX_OK;
}

/* v := 0 on a distributed level, ghosts included (setToValue(v, 0, true), N3/MultiGrid3D.cpp:634) */
int FN(zero_v)(MGRID* mg, int gridID) {
    MG_REQUIRE(mg && gridID >= 0 && gridID < mg->numDist, MGX_ERR_INVALID, "zero_v: level %d is not distributed", gridID);
    GRID* g = mg->slabs[gridID];
    mg->v_rim_zero[gridID] = 1;
    MG_TRY(MG_CAT(ca_settle_, R)(mg));
    mg->gv[gridID] = MG_CA_ALL;
    return mgx_memset_zero(mg->ctx, g->d_v, MG_CAT(plane3_, R)(g) * (size_t)g->plan.nzl * sizeof(REAL));
}

/* host <-> slab transfers.  Host arrays are FULL grids of the level in the reference layout; each rank moves
 * only its own planes (upload: owned + ghosts, download: owned), converting to / from x-split on the device. */
static int MG_CAT(slab_put_, R)(MGRID* mg, GRID* g, REAL* dev, const REAL* host_full) {
    const size_t pl = MG_CAT(plane3_, R)(g), hpl = MG_CAT(hplane3_, R)(g);
    REAL* tmp = NULL;
    MG_TRY(mgx_malloc(mg->ctx, hpl * (size_t)g->plan.nzl * sizeof(REAL), (void**)&tmp));
    int st = mgx_memcpy_h2d(mg->ctx, tmp, host_full + hpl * (size_t)g->plan.zoff, hpl * (size_t)g->plan.nzl * sizeof(REAL));
    /* pack works row by row, so a stack of planes can be converted in slices of 3 planes */
    for (int z = 0; z < g->plan.nzl && !st; z += 3) {
        const int z0 = z + 3 <= g->plan.nzl ? z : g->plan.nzl - 3;
        const int n3[3] = {g->sizeXYZ[0], g->sizeXYZ[1], 3};
        st = XS(pack)(mg->ctx, tmp + hpl * (size_t)z0, dev + pl * (size_t)z0, n3);
    }
    if (!st) st = mgx_ctx_sync(mg->ctx);
    mgx_free(mg->ctx, tmp);
    return st;
}

int FN(upload_v)(MGRID* mg, int gridID, const REAL* host_full) {
    MG_REQUIRE(mg && host_full && gridID >= 0 && gridID < mg->numDist, MGX_ERR_INVALID, "upload_v: level %d is not distributed", gridID);
    mg->v_rim_zero[gridID] = 0; /* the host array may carry non-zero boundary values */
    MG_TRY(MG_CAT(ca_settle_, R)(mg));
    mg->gv[gridID] = MG_CA_ALL; /* every local plane comes from the host array */
    return MG_CAT(slab_put_, R)(mg, mg->slabs[gridID], mg->slabs[gridID]->d_v, host_full);
}
int FN(upload_f)(MGRID* mg, int gridID, const REAL* host_full) {
    MG_REQUIRE(mg && host_full && gridID >= 0 && gridID < mg->numDist, MGX_ERR_INVALID, "upload_f: level %d is not distributed", gridID);
    MG_TRY(MG_CAT(ca_settle_, R)(mg));
    mg->gf[gridID] = MG_CA_ALL;
    return MG_CAT(slab_put_, R)(mg, mg->slabs[gridID], mg->slabs[gridID]->d_f, host_full);
}
/* writes the planes this rank owns into the full host array (other planes are left untouched) */
int FN(download_v)(MGRID* mg, int gridID, REAL* host_full) {
    MG_REQUIRE(mg && host_full && gridID >= 0 && gridID < mg->numDist, MGX_ERR_INVALID, "download_v: level %d is not distributed", gridID);
    GRID* g = mg->slabs[gridID];
    const size_t pl = MG_CAT(plane3_, R)(g), hpl = MG_CAT(hplane3_, R)(g);
    REAL* tmp = NULL;
    MG_TRY(MG_CAT(ca_settle_, R)(mg));
    MG_TRY(mgx_malloc(mg->ctx, hpl * (size_t)g->plan.nzl * sizeof(REAL), (void**)&tmp));
    int st = MGX_OK;
    for (int z = 0; z < g->plan.nzl && !st; z += 3) {
        const int z0 = z + 3 <= g->plan.nzl ? z : g->plan.nzl - 3;
        const int n3[3] = {g->sizeXYZ[0], g->sizeXYZ[1], 3};
        st = XS(unpack)(mg->ctx, g->d_v + pl * (size_t)z0, tmp + hpl * (size_t)z0, n3);
    }
    if (!st)
        st = mgx_memcpy_d2h(mg->ctx, host_full + hpl * (size_t)g->plan.zlo, tmp + hpl * (size_t)(g->plan.zlo - g->plan.zoff),
                            hpl * (size_t)(g->plan.zhi - g->plan.zlo) * sizeof(REAL));
    mgx_free(mg->ctx, tmp);
    return st;
}

#undef GRID
#undef MGRID
#undef TAIL
#undef FN
#undef TFN
#undef XS
