/* mg_multigrid.h -- C host layer: the reference's Grid{1,2,3}D / MultiGrid{1,2,3}D classes as C
 * structs + functions, driving the HIP kernels through the thin C-ABI of mgx.h.
 *
 * Mirrors, member for member, the public surface of the NOCUDA_TESI reference:
 *   class Grid3D        N3/Grid3D.h:4-38        -> struct mgGrid3D_<r>
 *   class MultiGrid3D   N3/MultiGrid3D.h:6-33   -> struct mgMultiGrid3D_<r> + mgMultiGrid3D_<r>_<Method>
 *   class Grid2D        N2/Grid2D.h:4-33        -> struct mgGrid2D_<r>
 *   class MultiGrid2D   N2/MultiGrid2D.h:6-37   -> struct mgMultiGrid2D_<r> + ...
 *   class Grid1D        N1/Grid1D.h:4-26        -> struct mgGrid1D_<r>      (CPU only: "plumbing")
 *   class MultiGrid1D   N1/MultiGrid1D.h:6-31   -> struct mgMultiGrid1D_<r> (CPU only)
 * with <r> = f32 (the reference's own type) or f64 (BASELINE.json's GPU configs).
 *
 * Same names, same argument meaning, same level-count rule (numGrids = (int)log2(minSize-1),
 * N3/MultiGrid3D.cpp:33-34; `numGrids` stays a public mutable field that may be lowered
 * after construction), same cycle control flow (VCycle N3/MultiGrid3D.cpp:623-647,
 * FullMultiGridVCycle :569-585).  Differences, all at the boundary:
 *   - every function returns an int status (mgx_status) instead of asserting/aborting;
 *   - d_v / d_f are device arrays; h_v / h_f are host mirrors (always the reference layout:
 *     dense, x fastest) filled by *_download_* and pushed by *_upload_*.  The 3D hierarchy keeps
 *     its device arrays in the x-split layout of mgx.h by default (`layout` = 1; rows
 *     de-interleaved by x parity so that each colour pass streams contiguous half-rows); raw
 *     device pointers handed to Restrict/Interpolate/... must use the hierarchy's layout;
 *   - residual / error scratch is owned by the level and preallocated (the reference mallocs
 *     both inside every VCycle call and never frees them, N3/MultiGrid3D.cpp:629,638);
 *   - `residual_mode` selects REF_COMPAT (default; reproduces the 3D residual sign quirk,
 *     N3/MultiGrid3D.cpp:723) or CORRECT;
 *   - `fuse` (default 1) runs CalculateResidual+Restrict and Interpolate+ApplyCorrection as
 *     one kernel each; results are bit-identical to the unfused sequence.
 * The 1D classes run entirely on the host in C (BASELINE.json configs[0]: CPU path, no GPU).
 */
#ifndef MG_MULTIGRID_H
#define MG_MULTIGRID_H

#include "mgx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Which planes of a level one rank of a z-slab decomposition holds (global plane indices).  Pure host
 * arithmetic; also used by the CPU emulation test of the decomposition. */
#define MG_DEEP_GHOSTS 6      /* ghost planes on either side of a slab of >= MG_DEEP_MIN_PLANES planes */
#define MG_DEEP_MIN_PLANES 8
typedef struct mgSlabPlan {
    int zlo, zhi;   /* owned planes [zlo, zhi); the last rank also owns the boundary plane sizeZ-1 */
    int glo, ghi;   /* ghost planes below (ranks > 0) and above (ranks < P-1): MG_DEEP_GHOSTS each on slabs of at least */
                    /* MG_DEEP_MIN_PLANES planes, otherwise 2 below and 1 above */
    int zoff, nzl;  /* local array = global planes [zoff, zoff + nzl), zoff = zlo - glo */
    int ubeg, uend; /* planes the smoother updates: owned and interior, [max(zlo,1), min(zhi, sizeZ-1)) */
} mgSlabPlan;
/* number of leading levels that stay distributed: every rank owns an even number >= min_planes of planes */
int mg_dist_num_levels(int sizeZ_finest, int nranks, int numGrids, int min_planes);
int mg_dist_num_levels_single(int sizeZ_finest, int numGrids, int min_planes);
int mg_slab_plan(int sizeZ_level, int rank, int nranks, mgSlabPlan* out);

#define MG_MAX_LEVELS 32 /* (int)log2(size-1) of any int size */
/* Levels of a SEMI-COARSENED 3D hierarchy (mgMultiGrid3D_<r>_create_semi): pure host arithmetic.  At a level with
 * sizes n, h[d] = (range[2d+1] - range[2d]) / (n[d] - 1) in double; axis d is coarsenable when n[d] >= 5 && n[d] % 4 == 1 (its
 * coarse size (n[d]-1)/2+1 is then odd and >= 3); hmin = the smallest h[d] over the coarsenable axes; mask[l] (bit 0 = x, 1 = y,
 * 2 = z) has bit d set when d is coarsenable and h[d] <= 1.5 hmin, and level l + 1 halves those axes and keeps the others.  The
 * plan ends at the first level without a coarsenable axis (its mask is 0), at max_levels levels when that is > 0, at
 * MG_MAX_LEVELS in any case.  Finest sizes must be odd and >= 3 (MGX_ERR_SIZE).  A cube of 2^k+1 points with equal spacings
 * gives the levels of _create: all masks 7, mg_num_grids levels. */
typedef struct mgSemiPlan {
    int nlevels;
    int n[MG_MAX_LEVELS][3];
    unsigned char mask[MG_MAX_LEVELS]; /* the step from level l to l + 1; 0 on the last level */
} mgSemiPlan;
int mg_semi_plan(const int finest[3], const double range[6], int max_levels, mgSemiPlan* out);
/* use_graph: a captured cycle is replayed only while every host-side input of its launch sequence is what it was at
 * capture time.  Those inputs are serialised (mg_graph_record, csrc/host/mg_common.h) into a fixed-size record of
 * unsigned words, and a replay needs the caller's record to equal the capture's word for word. */
#define MG_GRAPH_REC_WORDS 74
typedef struct mgGraphRec {
    unsigned int w[MG_GRAPH_REC_WORDS];
} mgGraphRec;
/* the rim flags a captured cycle reads and writes (3D: f_rim_zero, v_rim_zero, e_rim_valid; slab: v_rim_zero, gv, gf and
 * the replicated tail's three): a replay leaves them as the capture did */
#define MG_GRAPH_FLAG_ARRAYS 6
typedef struct mgGraphFlags {
    unsigned char a[MG_GRAPH_FLAG_ARRAYS][MG_MAX_LEVELS];
} mgGraphFlags;
/* the values of PCG's and BackwardEuler's `krylov`: plain cycling, flexible CG over the interior (any other non-zero value is taken
 * as this one), flexible CG in the weighted inner product over all unknowns -- the Krylov solver of a hierarchy with Neumann
 * faces; without a mask it is MG_KRYLOV_CG launch for launch */
#define MG_KRYLOV_NONE 0
#define MG_KRYLOV_CG 1
#define MG_KRYLOV_WEIGHTED 2
/* the face coefficients of the variable-coefficient operators (_set_face_mean): the arithmetic mean (aP + aQ) / 2 of the two
 * nodes' values -- a material boundary on a node plane -- or the harmonic mean 2 aP aQ / (aP + aQ) -- node-valued materials (voxel
 * data), the boundary midway between two nodes */
#define MG_FACE_MEAN_ARITHMETIC 0
#define MG_FACE_MEAN_HARMONIC 1
#define MG_NORM_HISTORY 255 /* residual-norm history entries a distributed hierarchy keeps on the device */
#define MG_DECLARE(R, real)                                                                              \
    /* ------------------------------------------------------------------ 3D ------ */                  \
    typedef struct mgGrid3D_##R {                                                                        \
        real* h_v; /* host mirror of the approximate solution (NULL until first download/upload) */     \
        real* h_f; /* host mirror of the right-hand side */                                              \
        real* d_v; /* device: approximate solution */                                                    \
        real* d_f; /* device: right-hand side */                                                         \
        real* d_r; /* device scratch: residual (unfused path) */                                         \
        real* d_e; /* device scratch: interpolated error (unfused path) */                               \
        int sizeX, sizeY, sizeZ;                                                                         \
        int sizeXYZ[3];                                                                                  \
        real h_x, h_y, h_z;                                                                              \
        real x_a, x_b, y_a, y_b, z_a, z_b;                                                               \
        /* device: the coefficient a of div(a grad u) - s u = f at ALL points of the level, or NULL (no */ \
        /* coefficient: the constant-coefficient operators).  Owned by mgMultiGrid3D_<r>_set_coefficient */ \
        /* and freed by _destroy.  Appended last: every older member keeps its offset.                   */ \
        real* d_a;                                                                                       \
    } mgGrid3D_##R;                                                                                      \
    size_t mgGrid3D_##R##_sizeof(void); /* sizeof(mgGrid3D_<r>): for mirrors of the struct */            \
    typedef struct mgMultiGrid3D_##R {                                                                   \
        mgGrid3D_##R** grids3D;                                                                          \
        int numGrids;    /* public and mutable like the reference's; 1 <= numGrids <= maxGrids */        \
        int maxGrids;    /* levels allocated = (int)log2(minSize-1) */                                   \
        mgx_ctx* ctx;                                                                                    \
        int residual_mode; /* mgx_residual_mode */                                                       \
        int fuse;                                                                                        \
        int layout; /* device layout of d_v/d_f/d_r/d_e: 0 = reference layout, 1 = x-split (mgx.h) */    \
        int smoother; /* 0 = red-black Gauss-Seidel (the reference), 1 = weighted Jacobi (addition) */   \
        real omega;   /* Jacobi weight, default 2/3 */                                                   \
        int use_graph; /* 1: VCycle(gridID, v1, v2) is captured into a HIP graph on first use and     */ \
                       /* replayed afterwards (re-captured when its arguments or the fields above     */ \
                       /* change, or the context's parameters, mgx_ctx_generation).  Default 0.       */ \
        int capturing;                                                                                   \
        void* graph_exec[MG_MAX_LEVELS];                                                                 \
        /* the mean the face coefficients of a hierarchy with a coefficient are formed by, MG_FACE_MEAN_* */\
        /* (default 0 = arithmetic: every call does what it did without this member).  Set it through    */\
        /* _set_face_mean, which validates.  It takes the first four bytes of the unused graph_key: every */\
        /* member keeps its offset and the struct its size, and `shift` stays the last member.           */\
        union {                                                                                          \
            long long graph_key[MG_MAX_LEVELS - 3]; /* unused */                                         \
            int face_mean;                                                                               \
            /* internal: the pinned interior nodes of _set_pinned (per level the list of their storage   */\
            /* offsets and their values, on the device), or NULL (none).  Owned by _set_pinned, freed by */\
            /* _destroy.  It takes the last eight bytes of the unused graph_key, in front of `wall`:     */\
            /* every member keeps its offset and the struct its size.                                    */\
            struct {                                                                                     \
                long long graph_key_head_[MG_MAX_LEVELS - 4]; /* (face_mean and unused words) */         \
                void* pin;                                                                               \
            };                                                                                           \
        };                                                                                               \
        /* internal: the walls of _set_wall (beta and g of the six faces), or NULL (none).  Owned by     */\
        /* _set_wall, freed by _destroy.  Like cap below it takes eight bytes of the unused graph_key:   */\
        /* every member keeps its offset and the struct its size.                                        */\
        void* wall;                                                                                      \
        /* internal: the capacity c of div(a grad u) - (shift c) u = f, a table of one device array     */ \
        /* per level, or NULL (no capacity: the scalar-shift operators).  Owned by _set_capacity,       */ \
        /* freed by _destroy.  Like pcg_fproj below it takes eight bytes of the unused graph_key:       */ \
        /* every member keeps its offset and the struct its size.                                       */ \
        void* cap;                                                                                       \
        /* internal: PCG's fifth level-0 scratch array, the projected right-hand side f - mean_W(f) of   */ \
        /* the closed box without a shift (krylov = 2; allocated by the first such call, freed by        */ \
        /* _destroy).  It takes the last eight bytes of the unused graph_key: every member keeps its     */ \
        /* offset and the struct its size.                                                               */ \
        real* pcg_fproj;                                                                                 \
        /* internal: 1 when the boundary entries of level l's d_f are known to be 0 (left so by the     */ \
        /* previous cycle's residual+restrict); cleared by InitF / upload_f / Restrict / setToValue.    */ \
        /* Those entries are never read by any operator; the flag only saves re-zeroing them.           */ \
        unsigned char f_rim_zero[MG_MAX_LEVELS];                                                         \
        /* internal: 1 when the boundary (and pad) entries of level l's d_v are known to be 0: the coarse */ \
        /* error then starts a cycle without a zero fill (relax_from_zero).  Cleared by upload_v and by  */ \
        /* setToValue(d_v, value != 0, true).                                                            */ \
        unsigned char v_rim_zero[MG_MAX_LEVELS];                                                         \
        /* internal: 1 when the boundary entries of level l's d_e equal those of its d_v: d_e is the      */ \
        /* ping-pong partner of the one-launch red+black sweeps (mgx3dxs_relax_pp), which never write     */ \
        /* boundary points.  Cleared by everything that may write either array's boundary.  External      */ \
        /* writers of d_v / d_e through the raw device pointers must clear it (and v_rim_zero) themselves. */ \
        unsigned char e_rim_valid[MG_MAX_LEVELS];                                                        \
        /* internal: scratch of PCG (level-0 arrays in the hierarchy's layout, allocated by the first    */ \
        /* call, freed by _destroy): the iterate x, a copy of the right-hand side b, the direction p,    */ \
        /* q = A p; the CG state (MGX_CG_STATE doubles) and the reduction scratch; the graph of its      */ \
        /* preconditioning V-cycle (kept apart from graph_exec[0], which holds VCycle's)                  */ \
        real* pcg_x;                                                                                     \
        real* pcg_b;                                                                                     \
        real* pcg_p;                                                                                     \
        real* pcg_q;                                                                                     \
        double* pcg_state;                                                                               \
        double* pcg_work;                                                                                \
        void* pcg_graph_exec;                                                                            \
        /* the mask of the homogeneous Neumann faces (an addition; bit 0 x-low, 1 x-high, 2 y-low,       */ \
        /* 3 y-high, 4 z-low, 5 z-high; default 0 = Dirichlet data on all six faces, and every call then */ \
        /* does what it did without it).  Set it through _set_boundary.  The two ints take the eight     */ \
        /* bytes of the unused pcg_graph_key that stood here: the struct keeps its size, every member    */ \
        /* its offset, and `shift` stays the last one.                                                   */ \
        int bc;                                                                                          \
        int bc_reserved; /* internal: 1 inside PCG's projected solve (krylov = 2, closed box, shift 0)   */ \
        /* internal: the record each graph was captured under and the rim flags its capture left behind  */ \
        /* (graph_key[] above is unused likewise)                                                        */ \
        mgGraphRec graph_rec[MG_MAX_LEVELS];                                                             \
        mgGraphFlags graph_post[MG_MAX_LEVELS];                                                          \
        mgGraphRec pcg_graph_rec;                                                                        \
        mgGraphFlags pcg_graph_post;                                                                     \
        /* internal: state of PCG_mixed (fp64 only; NULL until its first call, freed by _destroy): the  */ \
        /* fp32 twin hierarchy that runs the preconditioning V-cycle, and the mixed kernels' scratch     */ \
        void* pcg_mixed;                                                                                 \
        /* the axes halved between level l and l + 1 (bit 0 = x, 1 = y, 2 = z): 7 on every level but for */ \
        /* _create_semi, whose masks come from mg_semi_plan.  Fixed at creation.                         */ \
        unsigned char coarsen[MG_MAX_LEVELS];                                                            \
        /* the shift s >= 0 of the operator (Laplacian - s) u = f (an addition; default 0 = the          */ \
        /* reference's Poisson problem, and every call then does what it did without this member).       */ \
        /* Non-zero: Relax, CalculateResidual (ResidualNorm, download_residual), VCycle,                 */ \
        /* FullMultiGridVCycle and PCG use the shifted operators of mgx.h (mgx3dxs_*_shift) with this s  */ \
        /* on every level, on full and on semi-coarsened hierarchies: per level relax_shift(_from_zero), */ \
        /* residual_restrict_shift, the coarser levels, interpolate_correct(_axes), relax_shift -- one   */ \
        /* launch per colour pass, none of the fused routes.  That needs layout = 1, smoother = 0 and    */ \
        /* residual_mode = MGX_RESIDUAL_CORRECT (else MGX_ERR_INVALID); PCG_mixed and mgDistMultiGrid3D  */ \
        /* return MGX_ERR_INVALID on a shifted hierarchy.  Set it through _set_shift, which validates.   */ \
        /* Appended last: every older member keeps its offset.                                           */ \
        real shift;                                                                                      \
    } mgMultiGrid3D_##R;                                                                                 \
    /* Homogeneous Neumann faces (an addition; mgx3dxs_*_bc of mgx.h).  neumann[k] != 0   */ \
    /* makes face k (x-low, x-high, y-low, y-high, z-low, z-high) a wall with du/dn = 0 on EVERY level:  */ \
    /* its points, but for those on a Dirichlet face too, become unknowns, and d_v there is no longer    */ \
    /* data but part of the solution.  Relax, CalculateResidual (ResidualNorm, download_residual),       */ \
    /* Restrict, Interpolate, VCycle, FullMultiGridVCycle, PCG(krylov = 0) and BackwardEuler(krylov = 0) */ \
    /* then run the _bc kernels with the hierarchy's coefficient and shift (the plain Laplacian as the   */ \
    /* shifted kernels with s = 0): per level relax, the residual stored into d_r, restrict_bc into the  */ \
    /* coarse d_f, the coarser levels from a zero fill of all points, interpolate_correct_bc, relax --   */ \
    /* no from-zero shortcut, none of the fused routes.  ResidualNorm and PCG's stopping rule sum over   */ \
    /* all unknowns, unweighted.  That needs layout = 1, smoother = 0, residual_mode =                   */ \
    /* MGX_RESIDUAL_CORRECT and a hierarchy that is not semi-coarsened (else MGX_ERR_INVALID, here and   */ \
    /* where the mask is used); all six faces with shift == 0 is singular and MGX_ERR_INVALID where the  */ \
    /* operator is used -- but PCG(krylov = 2), CG in the weighted inner product over all unknowns,     */ \
    /* solves it in the projected sense (see PCG); PCG(krylov = 1), BackwardEuler(krylov = 1) and        */ \
    /* PCG_mixed return MGX_ERR_INVALID with a mask.  A prescribed flux or a                             */ \
    /* convective wall: _set_wall below.  All zeros: the                                                 */ \
    /* hierarchy is what it was without a mask.  A change of the mask drops the captured graphs and      */ \
    /* zeroes, on the levels below the finest, the entries of d_v the old mask made unknowns.  Blocking. */ \
    /* The mask is the member `bc` (bit k = neumann[k]).                                                 */ \
    int mgMultiGrid3D_##R##_set_boundary(mgMultiGrid3D_##R* mg, const int neumann[6]);                   \
    int mgMultiGrid3D_##R##_get_boundary(const mgMultiGrid3D_##R* mg, int neumann[6]);                   \
    /* Convective (Robin) and prescribed-flux walls (an addition; mgx3dxs_*_wall of mgx.h). */\
    /* On face k of the mask the wall law is a du/dn + beta[k] u = g[k] (n outward, beta >= 0), in the   */\
    /* units of the hierarchy's operator div(a grad u) (a = 1 without a coefficient): beta = g = 0 is   */\
    /* the insulated wall.  With BackwardEuler's kappa a physical kappa a du/dn + B u = G is beta = B /  */\
    /* kappa, g = G / kappa: nothing is rescaled here.  beta enters the operator of EVERY level as the   */\
    /* diagonal term 2 beta / h of that level's own spacing (never restricted): Relax, CalculateResidual */\
    /* (ResidualNorm, download_residual), VCycle, FullMultiGridVCycle, PCG with krylov = 0 and 2 and     */\
    /* BackwardEuler run the _wall entries where they ran the _bc entries.  g touches level 0's right-   */\
    /* hand side only: _add_wall_flux subtracts 2 g / h from d_f[0] at the face unknowns (once per      */\
    /* right-hand side: the caller's business after upload_f; BackwardEuler does it for every step).    */\
    /* A beta > 0 makes the closed box regular: all six faces with shift == 0 (or a capacity without a  */\
    /* positive entry) is then accepted everywhere and PCG(krylov = 2) projects nothing.  beta[k] not    */\
    /* finite or < 0, g[k] not finite, or either != 0 on a face the mask does not flag: MGX_ERR_INVALID, */\
    /* and _set_boundary refuses to clear a face that still carries either.  Every call syncs and drops */\
    /* the captured graphs; all zeros frees the table, and the hierarchy is then, launch for launch and */\
    /* bit for bit, one that never had a wall.  Everything the mask refuses stays refused; PCG_mixed     */\
    /* returns MGX_ERR_INVALID while walls are set.  Data that vary along a face: fold 2 g(P) / h into f */\
    /* by hand.                                                                                          */\
    int mgMultiGrid3D_##R##_set_wall(mgMultiGrid3D_##R* mg, const real beta[6], const real g[6]);        \
    int mgMultiGrid3D_##R##_get_wall(const mgMultiGrid3D_##R* mg, real beta[6], real g[6]);              \
    int mgMultiGrid3D_##R##_add_wall_flux(mgMultiGrid3D_##R* mg);                                        \
    /* Pinned interior nodes (an addition; csrc/mgx_pin3d.hip).  mask[x + y sx + z sx sy]  */\
    /* != 0 makes the interior point (x, y, z) of level 0 DATA with the value values[...] (values ==     */\
    /* NULL: 0): it is no unknown, its neighbours read it as they read a Dirichlet face point, the       */\
    /* smoother never changes it, and the residual, A p and every vector of PCG are exactly 0 there; the */\
    /* operator on the other unknowns is the old one with rows and columns struck out.  A coarse point   */\
    /* is pinned when its coincident fine point is, or one of that point's neighbours at +-1 along an    */\
    /* axis that the step halves; coarse boundary points never are.  The values go down by injection.    */\
    /* The level a cycle starts on (Relax, VCycle's gridID, every level in turn in FullMultiGridVCycle)  */\
    /* holds the stored values at its pins, every level that holds a correction (below the top; level 0  */\
    /* inside PCG's preconditioner) zeros.  Every level then takes the operator route (the plain         */\
    /* Laplacian as the shifted operator with s = 0), the residual is stored, its pins zeroed, then      */\
    /* restricted; ResidualNorm and PCG's stopping rule sum over the unknowns only, for one more read    */\
    /* pass.  _set_pinned validates (a true entry on the boundary of the box is MGX_ERR_INVALID and      */\
    /* names the first one), builds and uploads every level's list, puts the values into d_v of every    */\
    /* level and drops every captured graph.  Blocking.  mask == NULL or all zero: no pins, and the      */\
    /* hierarchy is launch for launch what it was without them.  Pins need layout = 1, smoother = 0,     */\
    /* residual_mode = MGX_RESIDUAL_CORRECT (else MGX_ERR_INVALID, here and where they are used);        */\
    /* PCG_mixed and Eigen return MGX_ERR_INVALID with pins, and so does every operator of a closed box  */\
    /* (all six faces walls, shift == 0, no beta > 0), PCG(krylov = 2) included.                         */\
    /* _get_pinned: level gridID's mask in the reference layout (0 / 1); _pinned_count: its count.       */\
    int mgMultiGrid3D_##R##_set_pinned(mgMultiGrid3D_##R* mg, const unsigned char* mask,                 \
                                       const real* values);                                              \
    int mgMultiGrid3D_##R##_get_pinned(const mgMultiGrid3D_##R* mg, int gridID, unsigned char* mask);    \
    int mgMultiGrid3D_##R##_pinned_count(const mgMultiGrid3D_##R* mg, int gridID, size_t* count);        \
    /* shift must be finite and >= 0, and a non-zero one needs the settings named at the member          */ \
    int mgMultiGrid3D_##R##_set_shift(mgMultiGrid3D_##R* mg, real shift);                                \
    size_t mgMultiGrid3D_##R##_sizeof(void); /* sizeof(mgMultiGrid3D_<r>): for mirrors of the struct */  \
    /* The variable-coefficient operator div(a grad u) - shift u = f (an addition; mgx3dxs_*_coef of     */ \
    /* mgx.h).  host_a: a at all points of level 0, reference layout, every value finite and > 0 (else  */ \
    /* MGX_ERR_INVALID, and the hierarchy stays as it was).  Level 0 is uploaded and a_{l+1} =          */ \
    /* Restrict(a_l) down all maxGrids levels with mgx3dxs_restrict (mask 7) / mgx3dxs_restrict_axes:    */ \
    /* full weighting inside, injection on the boundary, so a stays positive; the operator is           */ \
    /* re-discretised on every level.  The arrays (one per level, grids3D[l]->d_a) are allocated on the */ \
    /* first call and reused afterwards.  "Has a coefficient" means grids3D[0]->d_a != NULL: Relax,     */ \
    /* CalculateResidual (ResidualNorm, download_residual), VCycle, FullMultiGridVCycle, PCG and        */ \
    /* BackwardEuler (kappa then scales div(a grad u)) then use the _coef kernels with `shift` (0        */ \
    /* allowed), on full and semi-coarsened hierarchies: per level relax_coef(_from_zero), residual_coef */ \
    /* into d_r, Restrict into the coarse d_f, the coarser levels, interpolate_correct(_axes),           */ \
    /* relax_coef -- one launch per colour pass, none of the fused routes.  That needs layout = 1,       */ \
    /* smoother = 0 and residual_mode = MGX_RESIDUAL_CORRECT (else MGX_ERR_INVALID, here and where it   */ \
    /* is used); PCG_mixed returns MGX_ERR_INVALID.  host_a == NULL frees the arrays: the hierarchy is  */ \
    /* what it was without one.  use_graph: level 0's d_a is part of the record, so setting or clearing */ \
    /* re-captures (allocating or freeing the arrays drops the captured graphs) and new values in the    */ \
    /* same arrays are read by a replay.  Blocking.                                                      */ \
    int mgMultiGrid3D_##R##_set_coefficient(mgMultiGrid3D_##R* mg, const real* host_a);                  \
    /* the coefficient of level gridID as a host array in the reference layout                           */ \
    int mgMultiGrid3D_##R##_download_coefficient(mgMultiGrid3D_##R* mg, int gridID, real* host);         \
    /* The operator with a capacity, div(a grad u) - (shift c) u = f (an addition; mgx3dxs_*_cap of     */ \
    /* mgx.h).  host_c: c at all points of level 0, reference layout, every value finite  */ \
    /* and >= 0 (else MGX_ERR_INVALID, and the hierarchy stays as it was).  The hierarchy must have a   */ \
    /* coefficient (_set_coefficient first, an array of ones serves; else MGX_ERR_INVALID), and         */ \
    /* _set_coefficient(NULL) is MGX_ERR_INVALID while a capacity is set.  Level 0 is uploaded and c    */ \
    /* goes down all maxGrids levels exactly as the coefficient does (mgx3dxs_restrict /                */ \
    /* _restrict_axes by the step's mask: full weighting inside, injection on the boundary, so c stays  */ \
    /* >= 0).  The arrays are allocated by the first call and reused by later ones.  Relax,             */ \
    /* CalculateResidual (ResidualNorm, download_residual), VCycle, FullMultiGridVCycle and PCG         */ \
    /* (krylov 0, 1 and, with a mask, 2) then run the _cap entries on every level through the route     */ \
    /* the coefficient operator takes, on full and semi-coarsened hierarchies and with any mask;        */ \
    /* BackwardEuler steps c u_t = kappa div(a grad u) + q (s = 1 / (kappa dt) as before, the right-    */ \
    /* hand side by mgx3dxs_cap_rhs).  PCG_mixed returns MGX_ERR_INVALID.  All six faces Neumann with   */ \
    /* a capacity that has no positive entry is singular like shift == 0, and MGX_ERR_INVALID where     */ \
    /* the operator is used (PCG with krylov = 2 included). host_c == NULL frees the arrays: the        */ \
    /* hierarchy is what it was without one, bit for bit.  use_graph: level 0's array is part of the    */ \
    /* record, and every call drops the captured graphs.  Blocking.                                     */ \
    int mgMultiGrid3D_##R##_set_capacity(mgMultiGrid3D_##R* mg, const real* host_c);                     \
    /* the capacity of level gridID as a host array in the reference layout                              */ \
    int mgMultiGrid3D_##R##_download_capacity(mgMultiGrid3D_##R* mg, int gridID, real* host);            \
    /* Harmonic-mean face coefficients (an addition; mgx3dxs_*_hmean of mgx.h).  mode =    */ \
    /* MG_FACE_MEAN_HARMONIC: wherever the hierarchy's operator is the coefficient or the capacity one, */ \
    /* every level is discretised with the face coefficient 2 aP aQ / (aP + aQ) -- Relax,               */ \
    /* CalculateResidual (ResidualNorm, download_residual), VCycle, FullMultiGridVCycle, PCG (krylov 0, */ \
    /* 1 and, with a mask, 2), BackwardEuler, with walls, a capacity and use_graph, on full and semi-   */ \
    /* coarsened hierarchies, launch for launch the route of the arithmetic operator with the _hmean    */ \
    /* entries.  a goes down the levels exactly as before.  MG_FACE_MEAN_ARITHMETIC (the default): the  */ \
    /* operators of _set_coefficient.  Any other mode: MGX_ERR_INVALID.  It may be called before or     */ \
    /* after _set_coefficient and has an effect only while the hierarchy has a coefficient: a plain or  */ \
    /* shifted hierarchy runs what it ran, launch for launch.  The products aP * aQ have to be normal   */ \
    /* and finite in `real`: while the mode is harmonic _set_coefficient also refuses an a[i] whose     */ \
    /* square is below the smallest normal number or not finite, and _set_face_mean(HARMONIC) checks    */ \
    /* the coefficient a hierarchy already has (MGX_ERR_INVALID naming the value; the hierarchy stays   */ \
    /* as it was; full weighting keeps the coarse coefficients inside the fine range).  A change of the */ \
    /* mode syncs and drops the captured graphs.  Everything refused before stays refused (PCG_mixed    */ \
    /* with a coefficient among it).  Blocking.  The mode is the member `face_mean`.                    */ \
    int mgMultiGrid3D_##R##_set_face_mean(mgMultiGrid3D_##R* mg, int mode);                              \
    int mgMultiGrid3D_##R##_create(mgx_ctx* ctx, const int finestGridSizeXYZ[3], const real range[6],     \
                                   mgMultiGrid3D_##R** out);                                             \
    int mgMultiGrid3D_##R##_create_layout(mgx_ctx* ctx, const int finestGridSizeXYZ[3],                  \
                                          const real range[6], int layout, mgMultiGrid3D_##R** out);     \
    /* nlevels > 0: the caller will use only the first nlevels levels (numGrids <= nlevels); the levels */ \
    /* past them that would have an even extent are then not built (maxGrids stops before the first).  */ \
    int mgMultiGrid3D_##R##_create_levels(mgx_ctx* ctx, const int finestGridSizeXYZ[3],                  \
                                          const real range[6], int layout, int nlevels,                  \
                                          mgMultiGrid3D_##R** out);                                      \
    /* a semi-coarsened hierarchy: the levels of mg_semi_plan(finest, (double)range, nlevels), always    */ \
    /* x-split, numGrids = maxGrids = the plan's level count.  Every call above and below works on it;   */ \
    /* steps whose mask is not 7 run the mgx3dxs_*_axes transfers between the existing smoother calls.   */ \
    int mgMultiGrid3D_##R##_create_semi(mgx_ctx* ctx, const int finestGridSizeXYZ[3], const real range[6], \
                                        int nlevels, mgMultiGrid3D_##R** out);                           \
    void mgMultiGrid3D_##R##_destroy(mgMultiGrid3D_##R* mg);                                             \
    int mgMultiGrid3D_##R##_InitV(mgMultiGrid3D_##R* mg, int gridID);                                    \
    int mgMultiGrid3D_##R##_InitF(mgMultiGrid3D_##R* mg, int gridID);                                    \
    int mgMultiGrid3D_##R##_Restrict(mgMultiGrid3D_##R* mg, const real* fine, const int fsizeXYZ[3],     \
                                     real* coarse, const int csizeXYZ[3]);                               \
    int mgMultiGrid3D_##R##_Interpolate(mgMultiGrid3D_##R* mg, real* fine, const int fsizeXYZ[3],        \
                                        const real* coarse, const int csizeXYZ[3]);                      \
    int mgMultiGrid3D_##R##_Relax(mgMultiGrid3D_##R* mg, mgGrid3D_##R* curGrid, int ncycles);            \
    int mgMultiGrid3D_##R##_setToValue(mgMultiGrid3D_##R* mg, real* grid, const int sizeXYZ[3],          \
                                       real value, int modifyBoundaries);                                \
    int mgMultiGrid3D_##R##_CalculateResidual(mgMultiGrid3D_##R* mg, mgGrid3D_##R* fine,                 \
                                              real** residual);                                          \
    int mgMultiGrid3D_##R##_ApplyCorrection(mgMultiGrid3D_##R* mg, real* fine, const int fsizeXYZ[3],    \
                                            const real* error, const int esizeXYZ[3]);                   \
    int mgMultiGrid3D_##R##_VCycle(mgMultiGrid3D_##R* mg, int gridID, int v1, int v2);                   \
    int mgMultiGrid3D_##R##_FullMultiGridVCycle(mgMultiGrid3D_##R* mg, int gridID, int v0, int v1,       \
                                                int v2);                                                 \
    int mgMultiGrid3D_##R##_upload_v(mgMultiGrid3D_##R* mg, int gridID, const real* host);               \
    int mgMultiGrid3D_##R##_upload_f(mgMultiGrid3D_##R* mg, int gridID, const real* host);               \
    int mgMultiGrid3D_##R##_download_v(mgMultiGrid3D_##R* mg, int gridID, real* host);                   \
    int mgMultiGrid3D_##R##_download_f(mgMultiGrid3D_##R* mg, int gridID, real* host);                   \
    int mgMultiGrid3D_##R##_download_residual(mgMultiGrid3D_##R* mg, int gridID, real* host);            \
    int mgMultiGrid3D_##R##_ResidualNorm(mgMultiGrid3D_##R* mg, int gridID, double* l2);                 \
    /* PrintDiff (N3/MultiGrid3D.cpp:760-764 -> Grid3D::PrintDiff) as numbers: mean |diff|, max |diff| and  */ \
    /* relative L2 of diff = sin(pi x) sin(pi y) sin(pi z) - v over all points of level gridID              */ \
    int mgMultiGrid3D_##R##_DiffStats(mgMultiGrid3D_##R* mg, int gridID, double* mean_abs,               \
                                      double* max_abs, double* rel_l2);                                  \
    /* PCG (an addition: the reference only cycles): solves A v = f on level 0 to a relative residual   */ \
    /* ||f - A v|| / ||f - A v0|| < tol by flexible CG (Polak-Ribiere beta) preconditioned by one       */ \
    /* VCycle(0, v1, v2) from zero per iteration (krylov != 0), or by plain VCycle(0, v1, v2) cycling   */ \
    /* (krylov = 0).  Needs layout = 1 and residual_mode = MGX_RESIDUAL_CORRECT.  The initial guess is   */ \
    /* d_v[0], whose boundary holds the Dirichlet data and is never changed; on return d_v[0] holds the */ \
    /* solution and d_f[0] its old contents, bit for bit.  *iters = iterations (cycles) run; *rel_res = */ \
    /* the TRUE relative residual of the result (a recursive residual below tol is re-checked against  */ \
    /* f - A v, and the iteration goes on from the true residual when that is not below tol);          */ \
    /* host_hist[k] (k < hist_cap) = relative residual after iteration k + 1 (recursive for CG).  A     */ \
    /* breakdown (<p, q> zero or not finite) returns MGX_OK with *converged = 0.  use_graph captures   */ \
    /* the preconditioning V-cycle.  Blocking: the host reads one double per iteration.                */ \
    /* krylov = MG_KRYLOV_WEIGHTED (2): flexible CG in the inner product <a, b>_W = sum of W a b over all */ \
    /* unknowns, W = 1/2 per Neumann face an unknown lies on, in which the operator with a mask is        */ \
    /* symmetric.  Without a mask every weight is 1: the launches and the bits of          */ \
    /* krylov = 1.  With a mask it is the Krylov solver (krylov = 1 is then MGX_ERR_INVALID): the         */ \
    /* mgx3dxs_*_bc vector entries on all unknowns; rr0, the recursive norm, the true-residual check and  */ \
    /* *rel_res stay unweighted over all unknowns, as with krylov = 0.  All six faces Neumann with        */ \
    /* shift == 0 (singular: refused everywhere else) is solved in the projected sense: the system is     */ \
    /* A v = f - mean_W(f), every residual is taken against that right-hand side, the preconditioned      */ \
    /* residual loses its weighted mean after every V-cycle, so v keeps the weighted mean of the guess;   */ \
    /* d_f[0] is restored to f bit for bit and _pcg_removed_mean gives mean_W(f) (0 after any other       */ \
    /* solve).                                                                                            */ \
    int mgMultiGrid3D_##R##_pcg_removed_mean(mgMultiGrid3D_##R* mg, double* mean);                       \
    int mgMultiGrid3D_##R##_PCG(mgMultiGrid3D_##R* mg, int v1, int v2, double tol, int maxit, int krylov, \
                                int* iters, double* rel_res, int* converged, double* host_hist,          \
                                int hist_cap);                                                           \
    /* BackwardEuler (an addition): nsteps implicit steps of u_t = kappa Laplacian(u) + q on level 0,   */ \
    /* (I - kappa dt Laplacian) u' = u + dt q, solved as (Laplacian - s) u' = -s u - q / kappa with     */ \
    /* s = (real)(1 / (kappa dt)).  d_v[0] holds u; its boundary is the Dirichlet data, fixed in time.  */ \
    /* d_source: q as a device array in the hierarchy's layout, or NULL.  Per step mgx3dxs_shift_rhs    */ \
    /* writes d_f[0] (qscale = (real)(1 / kappa)) and PCG(v1, v2, tol, maxit, krylov) runs from the      */ \
    /* guess u.  *iters_total = PCG iterations of all steps, *worst_rel_res = the largest true relative  */ \
    /* residual of a step; it stops at the first step that does not converge, with *converged = 0.       */ \
    /* The shift it sets STAYS SET afterwards (and d_f[0] holds the last step's right-hand side).        */ \
    /* Needs dt > 0, kappa > 0, nsteps >= 0 and the settings of a shifted hierarchy.  krylov is PCG's:   */ \
    /* with a mask 0 or MG_KRYLOV_WEIGHTED.                                                              */ \
    int mgMultiGrid3D_##R##_BackwardEuler(mgMultiGrid3D_##R* mg, int nsteps, double dt, double kappa,    \
                                          const real* d_source, int v1, int v2, double tol, int maxit,   \
                                          int krylov, int* iters_total, double* worst_rel_res,           \
                                          int* converged);                                               \
    /* solve(grid, rhs, nlevels): host arrays in the reference layout; grid = initial guess incl.     */ \
    /* boundary values on input, solution on output; nlevels = 0 -> reference rule; ncycles V(v1,v2)  */ \
    /* cycles from the given guess, or one FullMultiGridVCycle(v0,v1,v2) when fmg != 0.               */ \
    /* rhs == NULL: the reference's own right-hand side (Grid3D::InitF) is built on the device, nothing is  */ \
    /* uploaded for it.  grid_is_zero != 0 (mg3d_solve_from_zero): the guess is the reference's InitV state */ \
    /* (all zeros); `grid` is output only and no guess is uploaded either -- with both, the call is the     */ \
    /* reference's whole driver (N3/Poisson3DSolver.cpp:6-51) with ONE transfer, the result.               */ \
    int mg3d_solve_##R(mgx_ctx* ctx, real* grid, const real* rhs, const int sizeXYZ[3],                  \
                       const real range[6], int nlevels, int fmg, int v0, int v1, int v2, int ncycles,   \
                       int residual_mode);                                                               \
    int mg3d_solve_from_zero_##R(mgx_ctx* ctx, real* grid_out, const real* rhs, const int sizeXYZ[3],    \
                                 const real range[6], int nlevels, int fmg, int v0, int v1, int v2,      \
                                 int ncycles, int residual_mode);                                        \
    /* solve_pcg: mgMultiGrid3D_<r>_PCG on a hierarchy built for the call (x-split, CORRECT residual);   */ \
    /* grid = initial guess with its Dirichlet boundary on input, solution on output; host arrays in    */ \
    /* the reference layout; rhs == NULL: the reference's own right-hand side; krylov as in PCG (the    */ \
    /* hierarchy has no mask: MG_KRYLOV_WEIGHTED gives the bits of 1)                                   */ \
    int mg3d_solve_pcg_##R(mgx_ctx* ctx, real* grid, const real* rhs, const int sizeXYZ[3],              \
                           const real range[6], int nlevels, int v1, int v2, double tol, int maxit,      \
                           int krylov, int* iters, double* rel_res, int* converged);                     \
    /* ---- z-slab decomposed 3D V-cycle (one process per GPU; csrc/host/mg_dist3d.inc) ---- */         \
    typedef struct mgSlab3D_##R {                                                                        \
        real* d_v; /* local planes [zoff, zoff+nzl) of the level, x-split layout, ghosts included */     \
        real* d_f;                                                                                       \
        int sizeXYZ[3]; /* GLOBAL sizes of the level */                                                  \
        mgSlabPlan plan;                                                                                 \
        real h_x, h_y, h_z;                                                                              \
        real x_a, y_a, z_a;                                                                              \
        int level;      /* its index in mgDistMultiGrid3D::slabs */                                      \
    } mgSlab3D_##R;                                                                                      \
    typedef struct mgDistMultiGrid3D_##R {                                                               \
        mgSlab3D_##R** slabs;      /* levels 0 .. numDist-1 */                                           \
        int numDist;               /* number of distributed levels (mg_dist_num_levels) */               \
        int numGrids;              /* total levels of the cycle, public and mutable like the reference */\
        int maxGrids;                                                                                    \
        mgMultiGrid3D_##R* tail;   /* replicated hierarchy for levels >= numDist */                      \
        mgx_ctx* ctx;                                                                                    \
        int rank, nranks;                                                                                \
        int residual_mode;                                                                               \
        real* d_share;             /* staging for the agglomeration all-gather */                        \
        real* d_bplane;            /* FMG: staging for the top boundary plane of the replicated f */     \
        double* d_norm;            /* device: [0] scratch of ResidualNorm, [1 ...] squared-norm history */ \
        int norm_count;            /* entries recorded by ResidualNormRecord (<= MG_NORM_HISTORY) */     \
        long long inline_bytes;    /* levels whose slab of v is at most this large exchange inline on the */ \
                                   /* compute stream, one launch per pass (0: always overlapped); public  */ \
        /* internal: 1 while the boundary entries (and ghost-plane rims) of distributed level l's v are  */ \
        /* known to be 0: the coarse error then starts a cycle without a zero fill.  Set by create and  */ \
        /* zero_v, cleared by upload_v.                                                                  */ \
        unsigned char v_rim_zero[MG_MAX_LEVELS];                                                         \
        /* use_graph != 0: VCycle(0, v1, v2) is captured into a HIP graph (both streams, the RCCL calls */ \
        /* included) and replayed, as mgMultiGrid3D does -- opt-in: it needs collectives that can be    */ \
        /* captured (RCCL or a single rank; mgx_comm_capturable), and RCCL under capture between        */ \
        /* different GPUs has not been run anywhere yet.  A failed capture is an error, not a fallback. */ \
        int use_graph;                                                                                   \
        void* graph_exec;                                                                                \
        long long graph_key;                                                                             \
        int graph_warm;            /* the first cycle runs eagerly: lazy allocations cannot be captured */ \
        /* pack_halos != 0: the ghost exchange behind a colour pass carries only the half-rows of the    */ \
        /* colour the pass changed (d_stage: 2 send + 2 receive arrays of stage_half elements); 0        */ \
        /* (default): whole planes -- at 1025^3 on 8 ranks a plane's transfer hides behind the interior  */ \
        /* launch and the pack / unpack launches only add latency (rehearsal: 4.52 against 4.36 ms)      */ \
        int pack_halos;                                                                                  \
        real* d_stage;                                                                                   \
        size_t stage_half;                                                                               \
        /* Communication-avoiding schedule (public knob): levels whose slabs have at least ca_min_planes */ \
        /* planes (default 16; 0 = never) exchange ghost planes of v ONCE PER Relax CALL (4 deep for two */ \
        /* sweeps) instead of once per colour pass: the first ghost planes are relaxed redundantly, the */ \
        /* owner's expression on the owner's inputs (same bits), the valid region shrinking by one plane */ \
        /* per pass.  Thinner levels keep one exchange per colour pass.                                  */ \
        int ca_min_planes;                                                                               \
        /* internal: how many ghost planes of v / f on either side of a level's slab hold current values */ \
        /* (the same number on every rank; >= MG_DEEP_GHOSTS: all of them); consumers ask for what they */ \
        /* read and an exchange happens only when that is not there                                     */ \
        signed char gv[MG_MAX_LEVELS], gf[MG_MAX_LEVELS];                                                \
        int comm_pending;          /* an exchange is in flight on the comm stream; nothing may touch ghost */ \
                                   /* planes before mgx_comm_wait                                       */ \
        /* halo exchanges + collectives enqueued since creation (bench.py: exchanges per cycle)          */ \
        long long n_exchanges;                                                                           \
        /* internal: the record graph_exec was captured under (graph_key above is unused) and the flags */ \
        /* its capture left behind                                                                      */ \
        mgGraphRec graph_rec;                                                                            \
        mgGraphFlags graph_post;                                                                         \
    } mgDistMultiGrid3D_##R;                                                                             \
    int mgDistMultiGrid3D_##R##_create(mgx_ctx* ctx, const int finestGridSizeXYZ[3], const real range[6], \
                                       int min_planes, mgDistMultiGrid3D_##R** out);                     \
    void mgDistMultiGrid3D_##R##_destroy(mgDistMultiGrid3D_##R* mg);                                     \
    int mgDistMultiGrid3D_##R##_InitF(mgDistMultiGrid3D_##R* mg, int gridID);                            \
    int mgDistMultiGrid3D_##R##_Relax(mgDistMultiGrid3D_##R* mg, int gridID, int ncycles);               \
    int mgDistMultiGrid3D_##R##_VCycle(mgDistMultiGrid3D_##R* mg, int gridID, int v1, int v2);           \
    /* FullMultiGridVCycle (N3/MultiGrid3D.cpp:569-585) on slabs                                        */ \
    int mgDistMultiGrid3D_##R##_FullMultiGridVCycle(mgDistMultiGrid3D_##R* mg, int gridID, int v0,       \
                                                    int v1, int v2);                                     \
    /* l2 norm of the residual of a distributed level over the WHOLE grid (ADDITION: the reference has  */ \
    /* no norm; parity unpinned): every rank reduces the squared residual of the planes  */ \
    /* it owns on the device (wavefront-wide shuffles, fixed order), the partial sums are all-reduced   */ \
    /* over RCCL (one double) and every rank returns the same value.  Blocking.  Uses residual_mode.    */ \
    int mgDistMultiGrid3D_##R##_ResidualNorm(mgDistMultiGrid3D_##R* mg, int gridID, double* l2);         \
    /* the same without a host round trip: the squared norm is appended to a history kept on the device */ \
    /* (at most MG_NORM_HISTORY entries, e.g. one per cycle); _History downloads sqrt of the entries.    */ \
    int mgDistMultiGrid3D_##R##_ResidualNormRecord(mgDistMultiGrid3D_##R* mg, int gridID);               \
    int mgDistMultiGrid3D_##R##_ResidualNormHistory(mgDistMultiGrid3D_##R* mg, double* host_l2,          \
                                                    int capacity, int* count);                          \
    int mgDistMultiGrid3D_##R##_zero_v(mgDistMultiGrid3D_##R* mg, int gridID);                           \
    int mgDistMultiGrid3D_##R##_upload_v(mgDistMultiGrid3D_##R* mg, int gridID, const real* host_full);  \
    int mgDistMultiGrid3D_##R##_upload_f(mgDistMultiGrid3D_##R* mg, int gridID, const real* host_full);  \
    int mgDistMultiGrid3D_##R##_download_v(mgDistMultiGrid3D_##R* mg, int gridID, real* host_full);      \
    /* ------------------------------------------------------------------ 2D ------ */                  \
    typedef struct mgGrid2D_##R {                                                                        \
        real* h_v;                                                                                       \
        real* h_f;                                                                                       \
        real* d_v;                                                                                       \
        real* d_f;                                                                                       \
        real* d_r;                                                                                       \
        real* d_e;                                                                                       \
        int sizeX, sizeY;                                                                                \
        int sizeXY[2];                                                                                   \
        real h_x, h_y;                                                                                   \
        real x_a, x_b, y_a, y_b;                                                                         \
    } mgGrid2D_##R;                                                                                      \
    typedef struct mgMultiGrid2D_##R {                                                                   \
        mgGrid2D_##R** grids2D;                                                                          \
        int numGrids;                                                                                    \
        int maxGrids;                                                                                    \
        real matrixA[4];                                                                                 \
        int sizeA;                                                                                       \
        int alfa;                                                                                        \
        mgx_ctx* ctx;                                                                                    \
        int fuse; /* 2 (default): VCycle on the cache-resident kernels (one launch per level and direction, */ \
                  /* one for all levels <= 65^2); 1: CalculateResidual+Restrict and Interpolate+             */ \
                  /* ApplyCorrection fused, one launch per colour pass; 0: one launch per reference call.    */ \
                  /* Results are bit-identical.                                                              */ \
        int smoother; /* 0 = red-black Gauss-Seidel (the reference), 1 = weighted Jacobi (addition) */   \
        real omega;                                                                                      \
        int use_graph; /* as in mgMultiGrid3D: the 1025^2 cycle is launch-bound */                       \
        int capturing;                                                                                   \
        void* graph_exec[MG_MAX_LEVELS];                                                                 \
        long long graph_key[MG_MAX_LEVELS]; /* unused: kept so that the members keep their offsets */   \
        mgGraphRec graph_rec[MG_MAX_LEVELS]; /* internal: the record each graph was captured under */  \
    } mgMultiGrid2D_##R;                                                                                 \
    int mgMultiGrid2D_##R##_create(mgx_ctx* ctx, const int finestGridSizeXY[2], const real range[4],     \
                                   const real* A, int A_size, int alfa, mgMultiGrid2D_##R** out);        \
    void mgMultiGrid2D_##R##_destroy(mgMultiGrid2D_##R* mg);                                             \
    int mgMultiGrid2D_##R##_InitV(mgMultiGrid2D_##R* mg, int gridID);                                    \
    int mgMultiGrid2D_##R##_InitF(mgMultiGrid2D_##R* mg, int gridID);                                    \
    int mgMultiGrid2D_##R##_Restrict(mgMultiGrid2D_##R* mg, const real* fine, const int fsizeXY[2],      \
                                     real* coarse, const int csizeXY[2]);                                \
    int mgMultiGrid2D_##R##_Interpolate(mgMultiGrid2D_##R* mg, real* fine, const int fsizeXY[2],         \
                                        const real* coarse, const int csizeXY[2]);                       \
    int mgMultiGrid2D_##R##_Relax(mgMultiGrid2D_##R* mg, mgGrid2D_##R* curGrid, int ncycles);            \
    int mgMultiGrid2D_##R##_setToValue(mgMultiGrid2D_##R* mg, real* grid, const int sizeXY[2],           \
                                       real value, int modifyBoundaries);                                \
    int mgMultiGrid2D_##R##_CalculateResidual(mgMultiGrid2D_##R* mg, mgGrid2D_##R* fine,                 \
                                              real** residual);                                          \
    int mgMultiGrid2D_##R##_ApplyCorrection(mgMultiGrid2D_##R* mg, real* fine, const int fsizeXY[2],     \
                                            const real* error, const int esizeXY[2]);                    \
    int mgMultiGrid2D_##R##_VCycle(mgMultiGrid2D_##R* mg, int gridID, int v1, int v2);                   \
    int mgMultiGrid2D_##R##_FullMultiGridVCycle(mgMultiGrid2D_##R* mg, int gridID, int v0, int v1,       \
                                                int v2);                                                 \
    int mgMultiGrid2D_##R##_upload_v(mgMultiGrid2D_##R* mg, int gridID, const real* host);               \
    int mgMultiGrid2D_##R##_upload_f(mgMultiGrid2D_##R* mg, int gridID, const real* host);               \
    int mgMultiGrid2D_##R##_download_v(mgMultiGrid2D_##R* mg, int gridID, real* host);                   \
    int mgMultiGrid2D_##R##_download_f(mgMultiGrid2D_##R* mg, int gridID, real* host);                   \
    /* mean over the interior of |v - (2x^2-4xy+2y^2)| on the finest level (thesis Fig. 4.3 metric,     */ \
    /* CUDA_TESI/CUDA Lyapunov 2D/Grid2D.cu:123-154)                                                    */ \
    int mgMultiGrid2D_##R##_MeanAbsoluteError(mgMultiGrid2D_##R* mg, int gridID, double* mean);          \
    int mg2d_solve_##R(mgx_ctx* ctx, real* grid, const real* rhs, const int sizeXY[2],                   \
                       const real range[4], const real A[4], int alfa, int nlevels, int fmg, int v0,     \
                       int v1, int v2, int ncycles);                                                     \
    /* ------------------------------------------------------------------ 1D (host only) */             \
    typedef struct mgGrid1D_##R {                                                                        \
        real* h_v;                                                                                       \
        real* h_f;                                                                                       \
        int sizeX;                                                                                       \
        real h_x;                                                                                        \
        real x_a, x_b;                                                                                   \
    } mgGrid1D_##R;                                                                                      \
    typedef struct mgMultiGrid1D_##R {                                                                   \
        mgGrid1D_##R** grids1D;                                                                          \
        int numGrids;                                                                                    \
        int maxGrids;                                                                                    \
    } mgMultiGrid1D_##R;                                                                                 \
    int mgMultiGrid1D_##R##_create(int finestGridSize, const real range[2], mgMultiGrid1D_##R** out);    \
    void mgMultiGrid1D_##R##_destroy(mgMultiGrid1D_##R* mg);                                             \
    int mgMultiGrid1D_##R##_Restrict(mgMultiGrid1D_##R* mg, const real* fine, int fsize, real* coarse,   \
                                     int csize);                                                         \
    int mgMultiGrid1D_##R##_Interpolate(mgMultiGrid1D_##R* mg, real* fine, int fsize,                    \
                                        const real* coarse, int csize);                                  \
    int mgMultiGrid1D_##R##_Relax(mgMultiGrid1D_##R* mg, mgGrid1D_##R* curGrid, int ncycles);            \
    int mgMultiGrid1D_##R##_setToValue(mgMultiGrid1D_##R* mg, real* grid, int sizeX, real value,         \
                                       int modifyBoundaries);                                            \
    int mgMultiGrid1D_##R##_CalculateResidual(mgMultiGrid1D_##R* mg, mgGrid1D_##R* fine,                 \
                                              real* residual);                                           \
    int mgMultiGrid1D_##R##_ApplyCorrection(mgMultiGrid1D_##R* mg, real* fine, int fineSize,             \
                                            const real* error, int errorSize);                           \
    int mgMultiGrid1D_##R##_VCycle(mgMultiGrid1D_##R* mg, int gridID, int v1, int v2);                   \
    int mgMultiGrid1D_##R##_FullMultiGridVCycle(mgMultiGrid1D_##R* mg, int gridID, int v0, int v1,       \
                                                int v2);                                                 \
    int mg1d_solve_##R(real* grid, const real* rhs, int sizeX, const real range[2], int nlevels,         \
                       int fmg, int v0, int v1, int v2, int ncycles);

MG_DECLARE(f32, float)
MG_DECLARE(f64, double)

/* PCG_mixed (an addition): mgMultiGrid3D_f64_PCG with the preconditioner in fp32.  The same contract in every respect -- arguments,
 * error codes, layout = 1 and MGX_RESIDUAL_CORRECT, d_v[0] the guess with its Dirichlet boundary, d_f[0] restored bit for bit,
 * *rel_res the TRUE fp64 relative residual of the result, a breakdown returns MGX_OK with *converged = 0, use_graph captures the
 * preconditioning cycle -- but the iterate, the residual and the stopping test stay fp64 while the preconditioner is one fp32
 * VCycle(0, v1, v2) from zero on an fp32 twin hierarchy (same sizes, the range converted to float, x-split, CORRECT), built on
 * the first call, given numGrids and use_graph of this hierarchy on every call, rebuilt when numGrids exceeds its levels and
 * freed by _destroy.  The twin is new device memory: four fp32 arrays per level, 2,645,596,160 bytes at 513^3.
 * krylov = 0: defect correction, x += M32(r) with r = b - A x, every residual of host_hist the true one; krylov != 0: the
 * flexible CG of PCG with z = M32(r).  M32(r) = (double)V32((float)(r s)) / s with s = 2^-floor(log2(rms of the last residual
 * read)), a power of two, so the scale changes no bits; it keeps fp32 out of underflow and overflow. */
int mgMultiGrid3D_f64_PCG_mixed(mgMultiGrid3D_f64* mg, int v1, int v2, double tol, int maxit, int krylov, int* iters,
                                double* rel_res, int* converged, double* host_hist, int hist_cap);
/* mg3d_solve_pcg_f64 with PCG_mixed */
int mg3d_solve_pcg_mixed_f64(mgx_ctx* ctx, double* grid, const double* rhs, const int sizeXYZ[3], const double range[6], int nlevels,
                             int v1, int v2, double tol, int maxit, int krylov, int* iters, double* rel_res, int* converged);

/* Eigen (an addition): the k smallest eigenvalues lambda_i and eigenvectors x_i of the hierarchy's operator,
 *     -(div(a grad x_i)) [+ the wall diagonal of set_wall]  =  lambda_i c x_i      on the unknowns of the mask
 * (a = 1, c = 1 where the hierarchy has none; the wall flux g is right-hand-side data and plays no part), by LOBPCG (Knyazev 2001)
 * with block size k, 1 <= k <= MG_EIGEN_MAX_BLOCK, preconditioned by one VCycle(0, v1, v2) from zero per residual (captured and
 * replayed with use_graph, the bits of the eager run).  It works in the inner product <u, v>_W = sum of W u v over the unknowns
 * (W = 1/2 per wall an unknown lies on), in which -A_s = -(div(a grad .) - s c) is symmetric positive definite.  The hierarchy's
 * shift s is a spectral shift only: the solver finds -A_s x = mu c x and returns lambda = mu - s, so the closed insulated box,
 * whose lambda_1 is 0, is solved with any s > 0.  Everything the operator refuses stays refused with its message (all six faces
 * walls with s = 0 and no lossy wall, Jacobi, ...), as do the natural layout and REF_COMPAT (MGX_ERR_INVALID); so are NULL
 * arguments, k outside its range, tol <= 0 and maxit < 1, before anything is touched.
 *   The basis of an iteration is [X, T, P]: T_i = M r_i the preconditioned residuals, P the T and P part of the previous Ritz
 * combination (none in the first iteration).  The Rayleigh-Ritz problem (at most 24 x 24) is solved on the host by
 * mg_sym_geneig, which scales every basis vector to unit c W norm; where its Cholesky factorization meets a non-positive pivot the
 * iteration is repeated without P, and if that fails too the call returns MGX_OK with *converged = 0 and the last good iterate.
 * A X and A P are carried along by the combination of X and P; only A T is applied: k operator applications per iteration.
 *   Stopping: res_i = ||A_s x_i + mu_i c x_i||_W / (mu_i ||x_i||_W) < tol for all i, confirmed on a freshly applied A X after a
 * Rayleigh-Ritz step on X alone (which also makes <x_i, c x_j>_W = delta_ij to rounding); if the confirmation fails the iteration
 * goes on from there.  The same confirmation runs before a return at maxit, so lambda, res and the vectors always belong together.
 *   lambda, res: k doubles each (ascending lambda); *iters: iterations done (each k V-cycles and k operator applications);
 * host_vectors: NULL or k * vol doubles, vector i at i * vol in the reference layout, 0 at the Dirichlet points, sign
 * unspecified; host_guess: NULL (pseudo-random start vectors from a fixed integer hash: a call gives the same bits on every
 * run) or k * vol doubles, read at the unknowns only.  Start vectors that are linearly dependent in the c W inner product (to
 * rounding: a pivot of their scaled mass Gram not above 64 eps) are MGX_ERR_INVALID: there is no iterate to return then.
 *   The workspace (8 k + 2 level-0 arrays -- the basis, its images, two spare sets, and the copies of d_v[0] and d_f[0] -- and
 * the partial sums) is allocated inside the call and freed before it returns on every
 * way out.  On return d_v[0] and d_f[0] hold the bits they held on entry and the rim flags are as they were, but for
 * e_rim_valid[0], cleared as PCG clears it; the coarser levels hold what the last V-cycle left, as after PCG. */
#define MG_EIGEN_MAX_BLOCK 8
int mgMultiGrid3D_f64_Eigen(mgMultiGrid3D_f64* mg, int k, int v1, int v2, double tol, int maxit, double* lambda, double* res, int* iters,
                            int* converged, double* host_vectors, const double* host_guess);
/* The dense solver of Eigen, pure host code: the n eigenpairs of G y = w B y for symmetric n x n G and symmetric positive definite
 * B (row-major; the upper triangles are read), 1 <= n <= 24.  w ascending, Y[i * n + j] = component i of vector j, Y^T B Y = I.
 * G and B are first scaled by D = diag(B)^(-1/2) (basis vectors of unit norm), then B = L L^T, a cyclic Jacobi eigensolver on
 * L^-1 G L^-T, Y = D L^-T Z.  Returns MGX_OK, MGX_ERR_INVALID for NULL arguments or n outside 1 .. 24, and
 * MG_GENEIG_NOT_SPD (w and Y untouched) when B has a non-positive or non-finite diagonal entry or a pivot of the scaled B not above
 * 64 eps, or G a non-finite entry, and MG_GENEIG_NO_CONVERGENCE (w and Y untouched) when 64 Jacobi sweeps have not brought every
 * off-diagonal entry below eps / 8 of its two diagonal entries (some ten sweeps do at n = 24).  Eigen treats both alike. */
#define MG_GENEIG_MAX 24
#define MG_GENEIG_NOT_SPD 100
#define MG_GENEIG_NO_CONVERGENCE 101
int mg_sym_geneig(int n, const double* G, const double* B, double* w, double* Y);

/* numGrids = (int)log2(minSize - 1)            N3/MultiGrid3D.cpp:33-34 */
int mg_num_grids(int minSize);
/* coarse size = ((size-1)/2)+1                 N3/MultiGrid3D.cpp:40-42 */
int mg_coarse_size(int size);

#ifdef __cplusplus
}
#endif
#endif /* MG_MULTIGRID_H */
