/* mgx.h -- thin C-ABI over the hand-written HIP (gfx950 / MI355X) multigrid kernels.
 *
 * This is the drop-in boundary of the hot path.  The reference
 * (MisterPup/PDE-MultiGrid, NOCUDA_TESI) has no FFI layer: its boundary is the public
 * C++ surface of MultiGrid{2,3}D.  Each entry point below replaces one of those member
 * functions and takes the same arguments as plain pointers and sizes (device pointers
 * instead of host `float*`; `real` = float or double chosen by the _f32/_f64 suffix;
 * the grid spacing / range members the reference reads from Grid3D* are passed
 * explicitly).  The C host layer in include/mg_multigrid.h is the only caller in the
 * product; tests and bench.py reach it through ctypes.
 *
 *   reference member function (file:line)                      replacement
 *   -------------------------------------------------------    -----------------------------
 *   MultiGrid3D::Relax            N3/MultiGrid3D.cpp:489-567   mgx3d_relax_{f32,f64}
 *   MultiGrid3D::CalculateResidual N3/MultiGrid3D.cpp:678-730  mgx3d_residual_*
 *   MultiGrid3D::Restrict         N3/MultiGrid3D.cpp:50-184    mgx3d_restrict_*
 *   MultiGrid3D::Interpolate      N3/MultiGrid3D.cpp:186-335   mgx3d_interpolate_*
 *   MultiGrid3D::ApplyCorrection  N3/MultiGrid3D.cpp:649-676   mgx3d_apply_correction_*
 *   MultiGrid3D::setToValue       N3/MultiGrid3D.cpp:587-621   mgx3d_set_*
 *   Grid3D::InitF                 N3/Grid3D.cpp:78-96          mgx3d_init_f_* (host sin tables)
 *   MultiGrid2D::Relax            N2/MultiGrid2D.cpp:199-273   mgx2d_relax_*
 *   MultiGrid2D::CalculateResidual N2/MultiGrid2D.cpp:367-408  mgx2d_residual_*
 *   MultiGrid2D::Restrict         N2/MultiGrid2D.cpp:63-126    mgx2d_restrict_*
 *   MultiGrid2D::Interpolate      N2/MultiGrid2D.cpp:128-196   mgx2d_interpolate_*
 *   MultiGrid2D::ApplyCorrection  N2/MultiGrid2D.cpp:343-366   mgx2d_apply_correction_*
 *   MultiGrid2D::setToValue       N2/MultiGrid2D.cpp:275-292   mgx2d_set_*
 *   (N3 = NOCUDA_TESI/POISSON_3D(TESI)/, N2 = NOCUDA_TESI/PDE Lyapunov 2D/)
 *
 * Fused forms (bit-identical to the two calls they replace):
 *   CalculateResidual + Restrict   (VCycle, N3/MultiGrid3D.cpp:629-632)  mgx3d_residual_restrict_*
 *   Interpolate + ApplyCorrection  (VCycle, N3/MultiGrid3D.cpp:638-642)  mgx3d_interpolate_correct_*
 *
 * Conventions
 *   - every function returns an int status (MGX_OK = 0); nothing aborts
 *     (the reference asserts, N3/MultiGrid3D.cpp:60-62).  mgx_last_error() gives text.
 *   - arrays are dense, unpadded, x fastest: idx = x + y*sx + z*sx*sy
 *     (N3/MultiGrid3D.cpp:531); sizes are int[dim] = {sx, sy(, sz)}, each odd and >= 3
 *     (2^k+1 is not required; a hierarchy needs every one of its levels odd).
 *   - all `real*` arguments are DEVICE pointers obtained from mgx_malloc unless the
 *     name starts with host_.
 *   - kernels run on the context's compute stream; calls are asynchronous with respect
 *     to the host unless stated; mgx_ctx_sync() waits.
 *   - one context per host thread; no global state.
 */
#ifndef MGX_H
#define MGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    MGX_OK = 0,
    MGX_ERR_INVALID = 1, /* NULL pointer, bad enum, negative count ...            */
    MGX_ERR_SIZE = 2,    /* size relation violated (the reference would assert)   */
    MGX_ERR_HIP = 3,     /* a HIP runtime call failed                             */
    MGX_ERR_NOMEM = 4,
    MGX_ERR_RCCL = 5,
    MGX_ERR_NOGPU = 6    /* no HIP device visible                                 */
} mgx_status;

/* Residual variants: REF_COMPAT reproduces the reference's
 * sign quirk ((N-2v-S)/hy2, (D-2v-U)/hz2, N3/MultiGrid3D.cpp:723); CORRECT uses +S, +U. */
typedef enum { MGX_RESIDUAL_REF_COMPAT = 0, MGX_RESIDUAL_CORRECT = 1 } mgx_residual_mode;

typedef struct mgx_ctx mgx_ctx;
typedef struct mgx_event mgx_event;

const char* mgx_status_string(int status);
const char* mgx_last_error(void); /* thread-local, valid until the next failing call */
void mgx_set_last_error(const char* msg); /* for layers above (include/mg_multigrid.h) */
const char* mgx_version(void);

/* ---- context / device ------------------------------------------------------------ */
int mgx_device_count(int* count);
int mgx_ctx_create(int device, mgx_ctx** out);
int mgx_ctx_destroy(mgx_ctx* ctx);
int mgx_ctx_sync(mgx_ctx* ctx);                 /* waits for the compute and comm streams, then mgx_ctx_check */
/* MGX_OK unless an inter-workgroup wait of a kernel whose workgroups hand data to each other (the one-launch red+black
 * sweep of mgx3dxs_relax_pp; the resident Relax kernel that runs all passes of a long Relax call on a cache-resident
 * level) has given up on this context -- its workgroups were not resident together; results of that launch are invalid
 * ("relax3d.fused" = 0 / "relax3d.resident" = 0 avoid the kernels).  Meaningful after a synchronisation. */
int mgx_ctx_check(mgx_ctx* ctx);
/* After mgx_ctx_check / mgx_ctx_sync reported a given-up wait: the context has stopped launching those kernels (it runs the
 * colour-pass kernels instead, same results) and keeps reporting the condition until this call clears it.  Synchronises,
 * resets the hand-off state on the device and the abort word; reenable != 0 also lets the context use the kernels again
 * (the caller vouches that whatever kept their workgroups from being resident together is gone).  Data written by the
 * aborted launch stays invalid: upload or recompute it.
 * These kernels ASSUME the context has the GPU to itself while they run (their grids are sized to be resident at once:
 * tiles <= CUs x occupancy).  A process that shares the GPU with other contexts or processes sets "gpu.exclusive" to 0
 * (mgx_ctx_set_param): they are then never launched.  "sync.spin_limit" (default 2^21 polls, ~2 s) bounds every wait. */
int mgx_ctx_clear_abort(mgx_ctx* ctx, int reenable);
/* *generation counts the changes to what the context launches: it grows with every mgx_ctx_set_param call, when
 * mgx_ctx_check finds a given-up wait (the context stops launching those kernels) and with every mgx_ctx_clear_abort.  A
 * captured cycle of the host layer (use_graph) is captured again when it has changed since the capture. */
int mgx_ctx_generation(const mgx_ctx* ctx, unsigned long long* generation);
/* allocates now what some kernels would allocate on first use (the progress words and exchange buffer of the kernels whose
 * workgroups hand data to each other, ~17 MB): the hierarchies call it when they are created, so that their first cycle can
 * be captured into a HIP graph */
int mgx_ctx_prepare(mgx_ctx* ctx);
int mgx_ctx_device(const mgx_ctx* ctx, int* device);
/* tuning knobs of the x-split smoother kernel (speed only, never results): "relax3d.ty" waves
 * per block and "relax3d.rows" consecutive rows per lane, each in {1,2,4,8}; "relax3d.zchunk"
 * planes per block (0 = automatic); "relax3d.xcd" 0/1/2 block-to-tile mapping (2 = every XCD owns a y-slab and walks z);
 * "relax3d.wave_planes" slab height of the time-skewed pass order (< 0 automatic, 0 = whole-grid passes);
 * "cycle2d.tile" tile edge of the cache-resident 2D kernels (0 = by level size, 16, 32, 64), "cycle2d.tail_points" largest
 * top level (in points, <= 5120) the one-workgroup tail kernel of the 2D cycle takes;
 * "relax3d.lds" kernel / shape code of the pipelined smoother (-1 automatic), "relax3d.corr_fuse", "relax3d.v2",
 * "relax3d.zero_first", "relax3d.small" 0/1 switches of the fused forms; "residual_restrict3d.stream" 0..3 kernel choice,
 * ".pzchunk" coarse planes per run (0 automatic), ".tyw" waves per workgroup, ".cr" coarse rows per lane, ".rows" fine rows
 * per wave of the pipelined kernel (0 = by level size, 2, 4), ".xcd" 0/1/2 XCD-aware block order, ".rcp" 0/1: with
 * power-of-two squared spacings the residual multiplies by the exact reciprocals instead of dividing (same bits);
 * "relax3d.zchunk" and "residual_restrict3d.pzchunk" also reach the operators of the shifted, the variable-coefficient and the
 * Neumann hierarchies: a value > 0 is the planes per run of their colour pass (mgx3dxs_relax_shift / _coef, their _from_zero and
 * _bc forms; any value >= 1, the same bits for each; the run length launched is the last number of mgx_ctx_last_relax_kernel's
 * name, relax_coef3d_xs_kernel<double,4,4,4> = runs of 4 planes), respectively the coarse planes per run of
 * mgx3dxs_residual_restrict_shift and mgx3dxs_residual_restrict_axes (any value >= 1, the same bits); 0 = by the size of the launch.
 * "relax3d.corr_v2" 0/1: fp32 on wide levels, the correcting red pass with two pairs per lane like the plain passes;
 * "relax3d.zero_sweep" 0/1: relax_from_zero on the pipelined levels runs its first red and black pass as one launch;
 * "relax3d.resident" 0 / 1 / 2 and "relax3d.resident_min" (sweeps per call, default 3): all colour passes of a Relax call on a level
 * of 33 ... 129 points per row in one launch (single-rank contexts only) -- off / the tiles exchange once per sweep (default) / once
 * per pass; "relax3d.resident_tile" 0 (by level) / 8: tiles of 8 x 8 lines always;
 * "rr3d.black" 0 / 1 / 2: the last black pass of the pre-smoothing inside the residual+restrict launch -- off / on the
 * HBM-bound levels / wherever the geometry allows (tests), "rr3d.black_waves" 0 (by precision), 8 (two workgroups per CU), 12, 16 waves per workgroup.
 * "relax3d.block3" 1 (default) / 0: on the levels the fused black pass takes by its own rule (fp64, from 385-point rows on), the
 * last three colour passes before it (R, B, R) run as one launch that stores red only (mgx3dxs_relax_block3_f64) -- or as three.
 * "relax3d.block3_up" 1 (default) / 0: on those levels (and where the correcting red pass runs), a post-smoothing call with a
 * partner array (mgx3dxs_interpolate_correct_relax_pp, two sweeps or more) stores the red of that pass into the partner and runs
 * the next three colour passes (B, R, B) as one launch that writes both colours back into v (mgx3dxs_block3_up_takes) -- or as three.
 * "relax3d.block3_corr" 1 (default) / 0: on those levels mgx3dxs_interpolate_correct_relax_block3 (two sweeps or more) runs the
 * correcting red pass and the next two passes (R', B, R) as one in-place launch that stores red only, then plain passes from B on
 * (mgx3dxs_block3_corr_takes); the cycle of the 3D hierarchy calls it where it takes the level.
 * "gpu.exclusive" 1 (default) / 0: 0 = the GPU is shared with other contexts or processes, so the kernels whose workgroups
 * wait for each other (resident Relax, one-launch sweep of 513-point rows) are never launched; "sync.spin_limit" polls (~1 us
 * each, default 2^21) before such a wait gives up (see mgx_ctx_check); "test.handoff_fault" != 0 is a TEST HOOK that makes
 * workgroup 0 of those kernels wait for tags nobody writes (the give-up path under test).
 * Unknown names and out-of-range values are rejected (MGX_ERR_INVALID). */
int mgx_ctx_set_param(mgx_ctx* ctx, const char* name, int value);
/* name (kernel<template arguments>) of the smoother kernel the most recent 3D x-split colour pass launched; "" if none.
 * bench.py reports it as roofline.kernel so that the PMC traffic figure is attached only to the kernel it was taken from */
const char* mgx_ctx_last_relax_kernel(const mgx_ctx* ctx);
/* name of the kernel that ran the last black pass together with residual + restrict in the most recent
 * mgx3dxs_smooth_residual_restrict_* call; "" when that call ran the operators one after the other */
const char* mgx_ctx_last_rr_kernel(const mgx_ctx* ctx);
/* name of the kernel that ran the correcting red pass (the correction read on the fly) in the most recent
 * mgx3dxs_interpolate_correct_relax_* call; "" when that call corrected in a pass of its own */
const char* mgx_ctx_last_corr_kernel(const mgx_ctx* ctx);
/* name of the three-pass kernel the most recent mgx3dxs_smooth_residual_restrict_*, mgx3dxs_interpolate_correct_relax(_pp)_* or
 * mgx3dxs_relax_block3_f64 call launched; "" when that call ran its colour passes one launch each */
const char* mgx_ctx_last_block3_kernel(const mgx_ctx* ctx);
/* colour passes first_colour, 1 - first_colour, first_colour of MultiGrid3D::Relax over the interior of an n[0] x n[1] x n[2]
 * x-split fp64 level, in one launch.  Reads colour 1 - first_colour and the faces of the grid from vin, f from f; writes the
 * interior points of first_colour into vout (store_both != 0: of both colours, the other one as the middle pass left it).
 * Nothing else of vout is written and no first_colour interior entry of vin is read, so vin == vout is allowed when
 * store_both == 0; store_both needs separate arrays.  Bit-identical to the three passes. */
int mgx3dxs_relax_block3_f64(mgx_ctx* ctx, const double* vin, double* vout, const double* f, const int n[3], const double h[3],
                             int first_colour, int store_both);
/* the way up's first three colour passes R', B, R in one in-place launch: R' reads every black interior value as
 * v + Interpolate(coarse_v) (cn[d] = (n[d] - 1) / 2 + 1), B and R follow; only the red interior points of v are written (the black
 * ones stay as they were, uncorrected: a black pass has to follow), and no red interior entry of v is read.  Bit-identical to
 * Interpolate + ApplyCorrection + the three passes at the red points.  Reports "relax3d_xs_block3_kernel<double,0,false,16,corr>". */
int mgx3dxs_relax_block3_corr_f64(mgx_ctx* ctx, double* v, const double* f, const int n[3], const double h[3], const double* coarse_v,
                                  const int cn[3]);
/* TEST HOOK, process-wide: on != 0 -> every kernel launch of the library is preceded by a launch that fills the LDS of every
 * CU with signalling-NaN patterns (a kernel that reads an LDS word before writing it then fails its parity test for certain
 * instead of depending on the previous launch's leftovers).  Costs ~15 us per launch; results are unchanged by contract. */
int mgx_test_set_lds_poison(int on);
/* self-test of the above: one workgroup per CU reads all of its LDS without writing any; *fraction = share of the words
 * that carry the poison pattern (1.0 with poisoning on: the launch is preceded by the poisoning launch like any other) */
int mgx_test_lds_probe(mgx_ctx* ctx, double* fraction);
/* raw hipStream_t of the compute stream (for callers that bring their own HIP code) */
int mgx_ctx_stream(const mgx_ctx* ctx, void** hip_stream);

/* ---- device memory ------------------------------------------------------------------ */
int mgx_malloc(mgx_ctx* ctx, size_t bytes, void** dptr);
int mgx_free(mgx_ctx* ctx, void* dptr);
int mgx_memcpy_h2d(mgx_ctx* ctx, void* dst, const void* host_src, size_t bytes); /* blocking */
int mgx_memcpy_d2h(mgx_ctx* ctx, void* host_dst, const void* src, size_t bytes); /* blocking */
int mgx_memcpy_d2d(mgx_ctx* ctx, void* dst, const void* src, size_t bytes);      /* async    */
int mgx_memset_zero(mgx_ctx* ctx, void* dst, size_t bytes);                      /* async    */

/* ---- timing on the compute stream (HIP events) ------------------------------------ */
/* HIP graphs for the launch-bound parts (2D cycles, coarse 3D levels): everything the calls between _begin and _end
 * enqueue on the context's compute stream is captured instead of executed and instantiated as one executable graph;
 * _launch replays it with a single launch.  The host layer's VCycle does this itself when `use_graph` is set. */
/* A captured graph freezes the launch sequence as it was at capture time, context parameters (mgx_ctx_set_param) included:
 * change a parameter -> capture again.  The host layer re-captures when the cycle's own arguments or fields change and when
 * the context's generation (mgx_ctx_generation) has changed. */
int mgx_graph_begin(mgx_ctx* ctx);
int mgx_graph_end(mgx_ctx* ctx, void** graph_exec);
int mgx_graph_launch(mgx_ctx* ctx, void* graph_exec);
int mgx_graph_destroy(mgx_ctx* ctx, void* graph_exec);
int mgx_event_create(mgx_ctx* ctx, mgx_event** out);
int mgx_event_destroy(mgx_ctx* ctx, mgx_event* ev);
int mgx_event_record(mgx_ctx* ctx, mgx_event* ev);
int mgx_event_elapsed_ms(mgx_ctx* ctx, mgx_event* start, mgx_event* stop, float* ms); /* syncs on stop */

/* ---- operators ------------------------------------------------------------------------
 * Declared once per real type through MGX_DECLARE_OPS(suffix, real).
 *
 * mgx3d_relax: `ncycles` red-black Gauss-Seidel sweeps, in place (one launch per colour).
 * mgx3d_residual: r = f - A v on the interior (mode selects the sign variant), 0 on the boundary.
 * mgx3d_restrict: 27-point full weighting, boundary = injection; cn must equal (fn-1)/2+1.
 * mgx3d_interpolate: trilinear, interior of `fine` only (boundary untouched).
 * mgx3d_apply_correction: fine += err on the interior.
 * mgx3d_set: fill; modify_boundaries = 0 leaves the boundary untouched.
 * mgx3d_residual_restrict: coarse_f = Restrict(CalculateResidual(v, f)) without storing
 *   the fine residual.
 * mgx3d_interpolate_correct: v += Interpolate(coarse_v) on the interior.
 * mgx3d_init_f: f[x,y,z] = (real)(c * tx[x] * ty[y] * tz[z]) evaluated in double, left to
 *   right (Grid3D::InitF with host-computed sin tables; tables are host pointers).
 * mgx3d_jacobi: ADDITION (north_star names weighted Jacobi; the reference has only red-black Gauss-Seidel):
 *   `ncycles` sweeps of v <- v + omega*(u - v), u = the Gauss-Seidel value from the OLD iterate; `tmp` is a
 *   second n-point array (ping-pong), the result always ends in v.  Parity unpinned by the reference.
 * mgx3d_diff_stats: Grid3D::PrintDiff (N3/Grid3D.cpp:136-159) as a device reduction: diff = realSol - v with
 *   realSol = (real)(tx[x]*ty[y]*tz[z]) (host sin tables); host_out = {sum|diff|, max|diff|, sum diff^2,
 *   sum realSol^2} over all points.
 * mgx2d_mean_abs_error: mean over the interior of |v - (2x^2-4xy+2y^2)| -- the accuracy metric of the thesis
 *   (PrintMeanAbsoluteError, CUDA_TESI/CUDA Lyapunov 2D/Grid2D.cu:123-154), reduced on the device.
 * mgx3dxs_*: the same operators on the device-internal "x-split" layout
 *   idx = (x>>1) + (x&1)*H + y*P + z*P*sy,  H = roundup((sx+1)/2, A), P = H + roundup(sx/2, A),
 *   A = 128/sizeof(real) elements
 *   (every x-row stored as its even-x half followed by its odd-x half, both starting on a 128-byte
 *   boundary; rows and planes in the reference order).  In row (y,z) the points of one colour are one
 *   contiguous, line-aligned half-row, so a red+black sweep moves the algorithmic minimum of 3 reals per
 *   point through HBM in full cache lines.  Results are bit-identical to the natural-layout operators;
 *   mgx3dxs_pack / _unpack convert (out of place); array sizes: mgx3dxs_elems.
 * mgx_norm2: sum of squares of `count` reals in double (wave-wide shuffle reduction +
 *   one atomic per block); host result, blocking.  An addition: the reference has no norm.
 */
#define MGX_DECLARE_OPS(SFX, real)                                                                      \
    int mgx3d_relax_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3],        \
                          int ncycles);                                                                 \
    /* relax_from_zero: v := 0 everywhere (setToValue(v, 0, true), N3/MultiGrid3D.cpp:634), then ncycles */ \
    /* sweeps (:626).  rim_is_zero != 0: the boundary (and pad) entries of v are zero already -- then      */ \
    /* nothing is filled and the first red pass does not read v; same bits either way.                   */ \
    int mgx3d_relax_from_zero_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], \
                                    int ncycles, int rim_is_zero);                                      \
    int mgx3d_residual_##SFX(mgx_ctx* ctx, const real* v, const real* f, real* r, const int n[3],       \
                             const real h[3], int mode);                                                \
    int mgx3d_restrict_##SFX(mgx_ctx* ctx, const real* fine, const int fn[3], real* coarse,             \
                             const int cn[3]);                                                          \
    int mgx3d_interpolate_##SFX(mgx_ctx* ctx, real* fine, const int fn[3], const real* coarse,          \
                                const int cn[3]);                                                       \
    int mgx3d_apply_correction_##SFX(mgx_ctx* ctx, real* fine, const int fn[3], const real* err,        \
                                     const int en[3]);                                                  \
    int mgx3d_set_##SFX(mgx_ctx* ctx, real* grid, const int n[3], real value, int modify_boundaries);   \
    int mgx3d_residual_restrict_##SFX(mgx_ctx* ctx, const real* v, const real* f, const int n[3],       \
                                      const real h[3], int mode, real* coarse_f, const int cn[3]);      \
    /* _keep_rim: the boundary entries of coarse_f are NOT rewritten (the caller knows they are 0,      */ \
    /* e.g. from the previous cycle); same interior results, one fill of the coarse array less.       */ \
    int mgx3d_residual_restrict_keep_rim_##SFX(mgx_ctx* ctx, const real* v, const real* f,              \
                                               const int n[3], const real h[3], int mode,               \
                                               real* coarse_f, const int cn[3]);                        \
    int mgx3d_interpolate_correct_##SFX(mgx_ctx* ctx, real* v, const int n[3], const real* coarse_v,    \
                                        const int cn[3]);                                               \
    int mgx3d_init_f_##SFX(mgx_ctx* ctx, real* f, const int n[3], double c, const double* host_tx,      \
                           const double* host_ty, const double* host_tz);                               \
    int mgx3d_jacobi_##SFX(mgx_ctx* ctx, real* v, real* tmp, const real* f, const int n[3],             \
                           const real h[3], real omega, int ncycles);                                   \
    /* vcycle_tail: the whole VCycle(v1, v2) (N3/MultiGrid3D.cpp:623-647) over levels[0 .. nlev), each  */ \
    /* at most 17 points per axis (n and h flattened {x0, y0, z0, x1, ...}; v / f HOST arrays of device  */ \
    /* pointers), in ONE workgroup with every level in LDS; top_zero != 0: v of levels[0] is taken as   */ \
    /* zeros without being read.  Leaves v of all levels and f of levels 1.. as the launch-per-operator */ \
    /* cycle does.  _fits: 1 when these levels can run that way ("relax3d.small" = 0 turns it off)      */ \
    int mgx3d_vcycle_tail_##SFX(mgx_ctx* ctx, int nlev, real* const* v, real* const* f, const int* n,   \
                                const real* h, int v1, int v2, int mode, int top_zero);                 \
    int mgx3d_vcycle_tail_fits_##SFX(const mgx_ctx* ctx, int nlev, const int* n);                       \
    int mgx3d_diff_stats_##SFX(mgx_ctx* ctx, const real* v, const int n[3], const double* host_tx,      \
                               const double* host_ty, const double* host_tz, double host_out[4]);       \
    /* x-split twins: same operators on arrays whose x-rows are de-interleaved (see below).  An        */ \
    /* x-split array of an (sx, sy, sz) grid has mgx3dxs_elems elements (rows are padded to cache      */ \
    /* lines), one z-plane has mgx3dxs_plane_elems; pad entries must be zero (mgx_memset_zero once).   */ \
    size_t mgx3dxs_elems_##SFX(const int n[3]);                                                         \
    size_t mgx3dxs_plane_elems_##SFX(int sx, int sy);                                                   \
    int mgx3dxs_pack_##SFX(mgx_ctx* ctx, const real* natural, real* xsplit, const int n[3]);            \
    int mgx3dxs_unpack_##SFX(mgx_ctx* ctx, const real* xsplit, real* natural, const int n[3]);          \
    int mgx3dxs_relax_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3],      \
                            int ncycles);                                                               \
    int mgx3dxs_relax_from_zero_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3],             \
                                      const real h[3], int ncycles, int rim_is_zero);                   \
    /* relax_pp: the same `ncycles` sweeps of v with a second array w (mgx3dxs_elems reals) as ping-pong */ \
    /* partner: on levels of 513-point rows every red+black sweep is ONE launch, out of place, that      */ \
    /* moves 2.5 instead of 3 reals per point (the black stage takes the new red values of its own tile  */ \
    /* from LDS and of the neighbouring tiles from memory, ordered by progress words; "relax3d.fused" = 0 */ \
    /* turns it off).  Result in v, bit-identical to mgx3dxs_relax; w is scratch.  w_rim_valid != 0: the  */ \
    /* caller vouches that the boundary entries of w equal those of v already.  _takes: 1 when a call    */ \
    /* with these sizes would run the one-launch sweeps (else it is mgx3dxs_relax).                      */ \
    int mgx3dxs_relax_pp_##SFX(mgx_ctx* ctx, real* v, real* w, const real* f, const int n[3],           \
                               const real h[3], int ncycles, int w_rim_valid);                          \
    int mgx3dxs_relax_pp_takes_##SFX(const mgx_ctx* ctx, const int n[3], int ncycles);                  \
    /* On cache-resident levels (33 ... 129 points per row) relax_pp also runs one launch per sweep      */ \
    /* (tile + halo in LDS, the neighbours' red values recomputed; "relax3d.fused_mid" = 0 turns it off). */ \
    /* relax_from_zero_pp / interpolate_correct_relax_pp: mgx3dxs_relax_from_zero /                      */ \
    /* mgx3dxs_interpolate_correct_relax with the same partner array for their sweeps; the first sweep of */ \
    /* relax_from_zero_pp does not read v on those levels (even ncycles, rim_is_zero).  Same bits.        */ \
    int mgx3dxs_relax_from_zero_pp_##SFX(mgx_ctx* ctx, real* v, real* w, const real* f, const int n[3], \
                                         const real h[3], int ncycles, int rim_is_zero, int w_rim_valid); \
    /* _takes: 1 when that call runs its sweeps on the partner array (and has brought w's boundary up to */ \
    /* date), 0 when it is plain mgx3dxs_relax_from_zero                                                 */ \
    /* sweep_once: ONE red+black sweep vin -> vout by the level's one-launch kernel (MGX_ERR_SIZE if it  */ \
    /* has none): interior points of vout are written, nothing else; zero != 0: vin counts as zeros and   */ \
    /* is not read (cache-resident levels).  The unit the _pp drivers are made of.                        */ \
    int mgx3dxs_sweep_once_##SFX(mgx_ctx* ctx, const real* vin, real* vout, const real* f,              \
                                 const int n[3], const real h[3], int zero);                            \
    int mgx3dxs_relax_from_zero_pp_takes_##SFX(const mgx_ctx* ctx, const int n[3], int ncycles,         \
                                               int rim_is_zero);                                        \
    int mgx3dxs_interpolate_correct_relax_pp_##SFX(mgx_ctx* ctx, real* v, real* w, const real* f,       \
                                                   const int n[3], const real h[3], const real* coarse_v, \
                                                   const int cn[3], int ncycles, int w_rim_valid);      \
    int mgx3dxs_residual_##SFX(mgx_ctx* ctx, const real* v, const real* f, real* r, const int n[3],     \
                               const real h[3], int mode);                                              \
    int mgx3dxs_restrict_##SFX(mgx_ctx* ctx, const real* fine, const int fn[3], real* coarse,           \
                               const int cn[3]);                                                        \
    int mgx3dxs_interpolate_##SFX(mgx_ctx* ctx, real* fine, const int fn[3], const real* coarse,        \
                                  const int cn[3]);                                                     \
    int mgx3dxs_apply_correction_##SFX(mgx_ctx* ctx, real* fine, const int fn[3], const real* err,      \
                                       const int en[3]);                                                \
    int mgx3dxs_set_##SFX(mgx_ctx* ctx, real* grid, const int n[3], real value, int modify_boundaries); \
    int mgx3dxs_residual_restrict_##SFX(mgx_ctx* ctx, const real* v, const real* f, const int n[3],     \
                                        const real h[3], int mode, real* coarse_f, const int cn[3]);    \
    int mgx3dxs_residual_restrict_keep_rim_##SFX(mgx_ctx* ctx, const real* v, const real* f,            \
                                                 const int n[3], const real h[3], int mode,             \
                                                 real* coarse_f, const int cn[3]);                      \
    int mgx3dxs_interpolate_correct_##SFX(mgx_ctx* ctx, real* v, const int n[3], const real* coarse_v,  \
                                          const int cn[3]);                                             \
    /* semi-coarsening (csrc/mgx_semi3d.hip): the same four transfers between levels of   */ \
    /* which only SOME axes are halved.  The axes are read off the sizes: axis d is kept when cn[d] ==   */ \
    /* fn[d] and halved when cn[d] == (fn[d]-1)/2+1; anything else, and no axis halved, is              */ \
    /* MGX_ERR_SIZE; all three halved forwards to the operator above.  One halved axis a: restriction    */ \
    /* (1/2) C + (1/4)(Ma + Pa); two, a < b: (1/4) C + (1/8)((Ma + Pa) + (Mb + Pb)) + (1/16)((MaMb +      */ \
    /* PaMb) + (MaPb + PaPb)).  Interpolation over the odd halved axes S: c[]; (1/2)(c[] + c[a]);        */ \
    /* (1/4)(((c[] + c[a]) + c[b]) + c[a,b]).  restrict_axes injects the coarse boundary;               */ \
    /* residual_restrict_axes writes it as 0 unless coarse_rim_is_zero != 0 (then it is left alone).    */ \
    int mgx3dxs_restrict_axes_##SFX(mgx_ctx* ctx, const real* fine, const int fn[3], real* coarse,      \
                                    const int cn[3]);                                                   \
    int mgx3dxs_interpolate_axes_##SFX(mgx_ctx* ctx, real* fine, const int fn[3], const real* coarse,   \
                                       const int cn[3]);                                                \
    int mgx3dxs_residual_restrict_axes_##SFX(mgx_ctx* ctx, const real* v, const real* f,                \
                                             const int n[3], const real h[3], int mode, real* coarse_f, \
                                             const int cn[3], int coarse_rim_is_zero);                  \
    int mgx3dxs_interpolate_correct_axes_##SFX(mgx_ctx* ctx, real* v, const int n[3],                   \
                                               const real* coarse_v, const int cn[3]);                  \
    int mgx3dxs_init_f_##SFX(mgx_ctx* ctx, real* f, const int n[3], double c, const double* host_tx,    \
                             const double* host_ty, const double* host_tz);                             \
    int mgx3dxs_jacobi_##SFX(mgx_ctx* ctx, real* v, real* tmp, const real* f, const int n[3],           \
                             const real h[3], real omega, int ncycles);                                 \
    int mgx3dxs_vcycle_tail_##SFX(mgx_ctx* ctx, int nlev, real* const* v, real* const* f, const int* n, \
                                  const real* h, int v1, int v2, int mode, int top_zero);               \
    int mgx3dxs_vcycle_tail_fits_##SFX(const mgx_ctx* ctx, int nlev, const int* n);                     \
    int mgx3dxs_diff_stats_##SFX(mgx_ctx* ctx, const real* v, const int n[3], const double* host_tx,    \
                                 const double* host_ty, const double* host_tz, double host_out[4]);     \
    /* z-slab forms for the multi-GPU decomposition.  A slab is a local x-split array of consecutive */ \
    /* z-planes of a level whose GLOBAL sizes are n[] (cn[] for the coarse level); it starts at       */ \
    /* global plane zoff.  relax_colour_slab: ONE colour pass (colour 0 = red: (x+y+z_global) even)   */ \
    /* over the local planes [zbeg, zend); the planes next to that range are read as ghosts.          */ \
    /* residual_restrict_slab / interpolate_correct_slab: global coarse planes [pzbeg, pzend);        */ \
    /* interpolate_correct writes the fine planes 2pz and 2pz+1 of every listed pz (z = 0 skipped).   */ \
    /* What the z-slab forms read and write (tests/test_gpu_slab_entries.py holds them to it; zoff,   */ \
    /* fzoff, czoff of either parity unless stated).  "Reads" = values that reach a result: a kernel   */ \
    /* may load more inside the planes listed, never outside the local array.  Every word not listed   */ \
    /* as written stays as it was, pad entries included.                                               */ \
    /*   relax_colour_slab(2): writes the colour's interior points of the listed planes; reads f at    */ \
    /*     those points and the OTHER colour of v on the planes [zbeg - 1, zend] (of either run) --     */ \
    /*     no point of the updated colour, in particular none in the two ghost planes.                */ \
    /*   relax_zero_colour_slab: the same writes; reads f at those points and nothing of v.            */ \
    /*   residual_restrict_slab: writes the coarse planes [pzbeg, pzend) whole (boundary and pad       */ \
    /*     entries as 0); with p0 = max(pzbeg, 1), p1 = min(pzend, cn[2] - 1) it reads v on the fine   */ \
    /*     planes [2 p0 - 2, 2 p1] and f on [2 p0 - 1, 2 p1 - 1]: fzoff <= 2 p0 - 2, czoff <= pzbeg.    */ \
    /*   residual_sumsq_slab: reads v on the local planes [zbeg - 1, zend], f on [zbeg, zend).         */ \
    /*   restrict_slab: writes the data entries of the coarse planes [pzbeg, pzend); reads the fine   */ \
    /*     planes 2 pz - 1 ... 2 pz + 1 of an interior pz and the plane 2 pz alone of pz = 0 and       */ \
    /*     cn[2] - 1 (injection).                                                                     */ \
    /*   interpolate_slab / interpolate_correct(_colour)_slab: pzend <= cn[2] - 1; write the interior  */ \
    /*     points (of the colour) of the fine planes 2 pz, 2 pz + 1 -- fzoff <= max(2 pzbeg, 1) -- and   */ \
    /*     read the coarse planes [pzbeg, pzend]; the _correct forms read what they write, plain       */ \
    /*     interpolate reads nothing of the fine array.                                               */ \
    /*   set_interior_slab: writes the (x, y)-interior of the local planes [zbeg, zend), zbeg >= 0.   */ \
    int mgx3dxs_relax_colour_slab_##SFX(mgx_ctx* ctx, real* v, const real* f, int sx, int sy,           \
                                        const real h[3], int colour, int zbeg, int zend, int zoff);     \
    /* relax_colour_slab2: the same pass over TWO runs of local planes [zb1, ze1) and [zb2, ze2), ze1   */ \
    /* <= zb2, in one launch where both are short (the bottom and the top edge of a slab)               */ \
    int mgx3dxs_relax_colour_slab2_##SFX(mgx_ctx* ctx, real* v, const real* f, int sx, int sy,          \
                                         const real h[3], int colour, int zb1, int ze1, int zb2,        \
                                         int ze2, int zoff);                                             \
    /* relax_zero_colour_slab: the same pass on a slab whose v counts as all zeros (the coarse error    */ \
    /* at the start of a cycle): v is not read, no ghost plane is needed; boundary entries must be 0   */ \
    int mgx3dxs_relax_zero_colour_slab_##SFX(mgx_ctx* ctx, real* v, const real* f, int sx, int sy,      \
                                             const real h[3], int colour, int zbeg, int zend, int zoff); \
    int mgx3dxs_residual_restrict_slab_##SFX(mgx_ctx* ctx, const real* v, const real* f,                \
                                             const int n[3], int fzoff, const real h[3], int mode,      \
                                             real* coarse_f, const int cn[3], int czoff, int pzbeg,     \
                                             int pzend);                                                \
    /* residual_sumsq_slab (ADDITION, the reference has no norm): sum of the squared residual over the */ \
    /* (x, y)-interior points of the local planes [zbeg, zend) -> *dev_out (device double), async on   */ \
    /* the compute stream, reduced in a fixed order (same bits on every run)                           */ \
    int mgx3dxs_residual_sumsq_slab_##SFX(mgx_ctx* ctx, const real* v, const real* f, int sx, int sy,   \
                                          const real h[3], int mode, int zbeg, int zend,                \
                                          double* dev_out);                                             \
    /* FMG on slabs: Restrict (coarse planes [pzbeg, pzend); boundary points by injection) and plain  */ \
    /* Interpolate (fine planes 2pz, 2pz+1 of every listed pz, interior points, z = 0 skipped).       */ \
    /* setToValue(.., false) on the LOCAL planes [zbeg, zend) of a slab: their (x, y)-interior points  */ \
    int mgx3dxs_set_interior_slab_##SFX(mgx_ctx* ctx, real* grid, int sx, int sy, int zbeg, int zend,   \
                                        real value);                                                    \
    int mgx3dxs_restrict_slab_##SFX(mgx_ctx* ctx, const real* fine, const int fn[3], int fzoff,         \
                                    real* coarse, const int cn[3], int czoff, int pzbeg, int pzend);    \
    int mgx3dxs_interpolate_slab_##SFX(mgx_ctx* ctx, real* fine, const int fn[3], int fzoff,            \
                                       const real* coarse, const int cn[3], int czoff, int pzbeg,       \
                                       int pzend);                                                      \
    int mgx3dxs_interpolate_correct_slab_##SFX(mgx_ctx* ctx, real* v, const int n[3], int fzoff,        \
                                               const real* coarse_v, const int cn[3], int czoff,        \
                                               int pzbeg, int pzend);                                   \
    /* interpolate_correct_relax: v += Interpolate(coarse_v) on the interior, then ncycles >= 1 sweeps   */ \
    /* (N3/MultiGrid3D.cpp:638-645 in one call).  On large levels the first red pass reads the black     */ \
    /* points THROUGH the correction instead of the correction being stored first ("relax3d.corr_fuse"  */ \
    /* = 0 turns that off); the result is bit-identical to interpolate_correct followed by relax.       */ \
    int mgx3dxs_interpolate_correct_relax_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3],   \
                                                const real h[3], const real* coarse_v, const int cn[3], \
                                                int ncycles);                                           \
    /* smooth_residual_restrict: the way down on one level in one call -- Relax(ncycles) (from_zero != 0: */ \
    /* on v = 0 as relax_from_zero, v_rim_is_zero as there), CalculateResidual, Restrict                  */ \
    /* (N3/MultiGrid3D.cpp:626-632; coarse_rim_is_zero as residual_restrict_keep_rim).  On the HBM-bound */ \
    /* levels the LAST BLACK PASS runs inside the residual+restrict launch (the black values are relaxed  */ \
    /* one plane ahead of the residual and stored on the way; "rr3d.black" = 0 turns that off); v and     */ \
    /* coarse_f are bit-identical to relax followed by residual_restrict.                                 */ \
    int mgx3dxs_smooth_residual_restrict_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3],    \
                                               const real h[3], int ncycles, int from_zero,             \
                                               int v_rim_is_zero, int mode, real* coarse_f,             \
                                               const int cn[3], int coarse_rim_is_zero);                \
    /* relax_rr_slab: that fused launch alone, on a z-slab (or the whole grid): the BLACK pass of the      */ \
    /* GLOBAL fine planes [2 pzbeg - 1, 2 pzend - 1] + residual + restrict into the GLOBAL coarse planes   */ \
    /* [pzbeg, pzend).  n / cn are global sizes, v / f start at global plane fzoff (even), coarse_f at     */ \
    /* global coarse plane czoff.  It reads only red values of v (fine planes 2 pzbeg - 3 ... 2 pzend + 1, */ \
    /* clipped to the grid: they must be present and current) and f (planes 2 pzbeg - 2 ... 2 pzend) --    */ \
    /* and, of the black points, only ones no pass writes: the face entries of the planes [2 pzbeg - 1,    */ \
    /* 2 pzend - 1] and the grid's planes 0 and n[2] - 1 where they lie next to that range.  No other      */ \
    /* black value reaches a result, inside or outside the range; the black interior points of the planes  */ \
    /* [2 pzbeg - 1, 2 pzend - 1] and the coarse planes (whole, boundary and pads 0) are all it writes.    */ \
    /* An odd fzoff is MGX_ERR_INVALID.  relax_rr_takes: 1 when a level of                                 */ \
    /* these global sizes has the kernel; otherwise relax_rr_slab fails with MGX_ERR_INVALID.              */ \
    int mgx3dxs_relax_rr_takes_##SFX(const mgx_ctx* ctx, const int n[3], const int cn[3]);              \
    int mgx3dxs_relax_rr_slab_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3], int fzoff,    \
                                    const real h[3], int mode, real* coarse_f, const int cn[3],         \
                                    int czoff, int pzbeg, int pzend);                                   \
    /* The same on a z-slab (the post-smoothing of the slab-decomposed cycle), in its two pieces.  n / cn */ \
    /* are GLOBAL sizes, v / f start at global plane fzoff (even), coarse_v at global plane czoff and     */ \
    /* holds cplanes planes.  corr_fused_takes: 1 when a level with these rows and `nplanes` planes to    */ \
    /* update runs the on-the-fly form.  correct_pset_slab: the tile-edge cells ("set P") of the GLOBAL   */ \
    /* fine planes [zmin, zmax) get v += Interpolate(coarse_v) in place (black points) -- list the ghost  */ \
    /* planes next to the updated range too, the red pass reads them.  (Since the end of round 3 the set   */ \
    /* is EMPTY for the one-pair-per-lane kernel -- fp64, and fp32 rows of < 513 points -- which corrects  */ \
    /* everything it reads itself: the call is then a no-op; the fp32 two-pair kernel keeps the cell rows.) */ \
    /* relax_corr_colour_slab: the RED                                                                    */ \
    /* pass over the LOCAL planes [zbeg, zend), every other black value read through the correction; the  */ \
    /* black pass that must follow rewrites every black interior point.                                  */ \
    /* Both refuse (MGX_ERR_INVALID) a level whose rows or switches the kernel does not run on -- the     */ \
    /* conditions of corr_fused_takes other than nplanes: a short range of an accepted level is fine --   */ \
    /* and relax_corr_colour_slab an odd fzoff.  correct_pset_slab writes black interior points of the    */ \
    /* planes [zmin, zmax) only, each either left alone or corrected.  relax_corr_colour_slab writes the  */ \
    /* red interior points of [zbeg, zend); it reads f there, the black values of v on the planes         */ \
    /* [zbeg - 1, zend] and the GLOBAL coarse planes (fzoff + zbeg - 1) / 2 ... (fzoff + zend + 1) / 2,    */ \
    /* all of which must lie within the cplanes planes handed in (the kernel clamps what it requests).     */ \
    int mgx3dxs_corr_fused_takes_##SFX(const mgx_ctx* ctx, const int n[3], int nplanes);                \
    /* block3_up_takes: 1 when mgx3dxs_interpolate_correct_relax_pp on a level of these sizes with      */ \
    /* `ncycles` sweeps runs its passes B, R, B in one launch ("relax3d.block3_up"); such a call brings   */ \
    /* w's boundary up to date (w's interior is scratch, as in relax_pp)                                  */ \
    int mgx3dxs_block3_up_takes_##SFX(const mgx_ctx* ctx, const int n[3], int ncycles);                 \
    /* interpolate_correct_relax_block3: interpolate_correct_relax whose passes R', B, R run as ONE       */ \
    /* in-place launch (mgx3dxs_relax_block3_corr_f64) followed by plain passes from B on, where           */ \
    /* block3_corr_takes says 1: fp64, `ncycles` >= 2, a level that corr_fused_takes and the three-pass    */ \
    /* launch's size rule accept, "relax3d.block3_corr" on.  Elsewhere it is interpolate_correct_relax.    */ \
    int mgx3dxs_block3_corr_takes_##SFX(const mgx_ctx* ctx, const int n[3], int ncycles);               \
    int mgx3dxs_interpolate_correct_relax_block3_##SFX(mgx_ctx* ctx, real* v, const real* f,            \
                                                       const int n[3], const real h[3],                 \
                                                       const real* coarse_v, const int cn[3],           \
                                                       int ncycles);                                    \
    int mgx3dxs_correct_pset_slab_##SFX(mgx_ctx* ctx, real* v, const int n[3], int fzoff,               \
                                        const real* coarse_v, const int cn[3], int czoff, int zmin,     \
                                        int zmax);                                                      \
    int mgx3dxs_relax_corr_colour_slab_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3],      \
                                             int fzoff, const real h[3], const real* coarse_v,          \
                                             const int cn[3], int czoff, int cplanes, int zbeg,         \
                                             int zend);                                                 \
    /* _colour forms: only the points with (x + y + z_global) % 2 == colour are corrected (-1 = all).  */ \
    /* The cycle passes colour 1 (black) when red-black sweeps follow: the red pass rewrites every red */ \
    /* interior point from black neighbours alone, so a corrected red value is never read.            */ \
    int mgx3dxs_interpolate_correct_colour_##SFX(mgx_ctx* ctx, real* v, const int n[3],                 \
                                                 const real* coarse_v, const int cn[3], int colour);    \
    int mgx3dxs_interpolate_correct_colour_slab_##SFX(mgx_ctx* ctx, real* v, const int n[3], int fzoff, \
                                                      const real* coarse_v, const int cn[3], int czoff, \
                                                      int pzbeg, int pzend, int colour);                \
    int mgx2d_relax_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[2], const real h[2],        \
                          const real a[2], const real A[4], int alfa, int ncycles);                     \
    int mgx2d_residual_##SFX(mgx_ctx* ctx, const real* v, const real* f, real* r, const int n[2],       \
                             const real h[2], const real a[2], const real A[4], int alfa);              \
    int mgx2d_restrict_##SFX(mgx_ctx* ctx, const real* fine, const int fn[2], real* coarse,             \
                             const int cn[2]);                                                          \
    /* fused forms of the cycle (N2/MultiGrid2D.cpp:320-323, 333-335): no residual / error array */    \
    int mgx2d_residual_restrict_##SFX(mgx_ctx* ctx, const real* v, const real* f, const int n[2],       \
                                      const real h[2], const real a[2], const real A[4], int alfa,      \
                                      real* coarse_f, const int cn[2]);                                 \
    int mgx2d_interpolate_correct_##SFX(mgx_ctx* ctx, real* v, const int n[2], const real* coarse_v,    \
                                        const int cn[2]);                                               \
    /* Cache-resident cycle kernels of the 2D path (the 1025^2 hierarchy never leaves L2 / Infinity     */ \
    /* Cache: the cycle is bound by launches, not HBM).  The upwind stencil {C, x+1, y+1} is one-sided, */ \
    /* so a workgroup that holds a tile plus a halo on the +x / +y side in LDS runs all colour passes   */ \
    /* of a Relax call on it, together with the operator next to it in VCycle -- bit-identical to the   */ \
    /* separate calls, OUT OF PLACE (tiles overlap: v_in != v_out), 0 <= ncycles <= 4:                  */ \
    /*   relax_residual_restrict: v_out = Relax(v_in, ncycles); coarse_f = Restrict(CalculateResidual(  */ \
    /*     v_out)) unless coarse_f is NULL (N2/MultiGrid2D.cpp:317-323); v_zero != 0: v_in is taken as  */ \
    /*     all zeros without being read (the coarse error after setToValue(v, 0, true), :326)           */ \
    /*   interpolate_correct_relax: v_out = Relax(v_in + Interpolate(coarse_v), ncycles)   (:333-338)   */ \
    /*   vcycle_tail: the whole VCycle(v1, v2) over levels[0 .. nlev) -- each at most 65^2, n and h     */ \
    /*     flattened {x0, y0, x1, y1, ...}, v / f HOST arrays of device pointers -- in ONE workgroup     */ \
    /*     with every level in LDS (:314-340); leaves v of all levels and f of levels 1.. as the        */ \
    /*     launch-per-operator cycle does.  _fits: may these levels run as one tail launch (they fit    */ \
    /*     into LDS and the top level has at most "cycle2d.tail_points" points: 1) or not (0)           */ \
    int mgx2d_relax_residual_restrict_##SFX(mgx_ctx* ctx, const real* v_in, real* v_out, const real* f, \
                                            const int n[2], const real h[2], const real a[2],           \
                                            const real A[4], int alfa, int ncycles, int v_zero,         \
                                            real* coarse_f, const int cn[2]);                           \
    int mgx2d_interpolate_correct_relax_##SFX(mgx_ctx* ctx, const real* v_in, real* v_out,              \
                                              const real* f, const int n[2], const real h[2],           \
                                              const real a[2], const real A[4], int alfa,               \
                                              const real* coarse_v, const int cn[2], int ncycles);      \
    int mgx2d_vcycle_tail_##SFX(mgx_ctx* ctx, int nlev, real* const* v, real* const* f, const int* n,   \
                                const real* h, const real a[2], const real A[4], int alfa, int v1,      \
                                int v2, int top_zero);                                                  \
    int mgx2d_vcycle_tail_fits_##SFX(const mgx_ctx* ctx, int nlev, const int* n);                       \
    int mgx2d_interpolate_##SFX(mgx_ctx* ctx, real* fine, const int fn[2], const real* coarse,          \
                                const int cn[2]);                                                       \
    int mgx2d_apply_correction_##SFX(mgx_ctx* ctx, real* fine, const int fn[2], const real* err,        \
                                     const int en[2]);                                                  \
    int mgx2d_set_##SFX(mgx_ctx* ctx, real* grid, const int n[2], real value, int modify_boundaries);   \
    int mgx2d_jacobi_##SFX(mgx_ctx* ctx, real* v, real* tmp, const real* f, const int n[2],             \
                           const real h[2], const real a[2], const real A[4], int alfa, real omega,     \
                           int ncycles);                                                                \
    /* init_v: Grid2D::InitV (N2/Grid2D.cpp:50-68) on the device: boundary 2*xj*xj-4*xj*yi+2*yi*yi with   */ \
    /* xj = a[0] + x*h[0], yi = a[1] + y*h[1] in `real`, interior 0; bit-identical to the host loop      */ \
    int mgx2d_init_v_##SFX(mgx_ctx* ctx, real* v, const int n[2], const real h[2], const real a[2]);    \
    int mgx2d_mean_abs_error_##SFX(mgx_ctx* ctx, const real* v, const int n[2], const real h[2],        \
                                   const real a[2], double* host_mean);                                 \
    int mgx_norm2_##SFX(mgx_ctx* ctx, const real* x, size_t count, double* host_sumsq);                \
    /* ---- vector kernels of the preconditioned CG solve (mgMultiGrid3D_<r>_PCG), x-split layout ----  */ \
    /* Interior points only: boundary and pad entries are neither read as data nor written.  Sums are  */ \
    /* accumulated in double in a fixed order (per-block partials in dev_work, then one final kernel), */ \
    /* so a call gives the same bits on every run.  dev_work: mgx3dxs_krylov_work_elems doubles of    */ \
    /* device scratch; dev_sum / dev_alpha / dev_beta: device doubles.  Asynchronous on the compute    */ \
    /* stream.  An addition: the reference has no Krylov solver.                                       */ \
    size_t mgx3dxs_krylov_work_elems_##SFX(const int n[3]);                                             \
    /* laplace_dot: q = A p with A the Laplacian of MGX_RESIDUAL_CORRECT (q is bit-identical to        */ \
    /* -mgx3dxs_residual(p, f = 0, CORRECT)); *dev_sum = <p, q>.  p's boundary is read, q's is not     */ \
    /* written.                                                                                         */ \
    int mgx3dxs_laplace_dot_##SFX(mgx_ctx* ctx, const real* p, real* q, const int n[3], const real h[3], \
                                  double* dev_work, double* dev_sum);                                   \
    /* cg_update: x += a p (skipped when x is NULL), r -= a q with a = (real)*dev_alpha;               */ \
    /* *dev_sum = <r, r> of the new r                                                                   */ \
    int mgx3dxs_cg_update_##SFX(mgx_ctx* ctx, real* x, const real* p, real* r, const real* q,           \
                                const int n[3], const double* dev_alpha, double* dev_work,              \
                                double* dev_sum);                                                       \
    /* dot2: dev_sum[0] = <a, b> and, unless c is NULL, dev_sum[1] = <a, c> (one pass over a)          */ \
    int mgx3dxs_dot2_##SFX(mgx_ctx* ctx, const real* a, const real* b, const real* c, const int n[3],   \
                           double* dev_work, double* dev_sum);                                          \
    /* cg_direction: x += (real)*dev_alpha * p with the old p (skipped when x is NULL), then, unless z  */ \
    /* is NULL, p = z + (real)*dev_beta * p, or p = z when dev_beta is NULL                             */ \
    int mgx3dxs_cg_direction_##SFX(mgx_ctx* ctx, real* x, real* p, const real* z, const int n[3],       \
                                   const double* dev_alpha, const double* dev_beta);                    \
    /* ---- the shifted operator (Laplacian - s) u = f, s >= 0, x-split layout (csrc/mgx_shift3d.hip) -- */ \
    /* An addition: the implicit step of diffusion and the screened Poisson equation.  Arithmetic, in   */ \
    /* `real`, left to right, nothing contracted (hx2 .. = squared spacings, c = the centre value):      */ \
    /*   smoother  v = num / den, num = the numerator of Relax's point update,                           */ \
    /*             den = 2*(hy2*hz2 + hx2*hz2 + hx2*hy2) + s*hx2*hy2*hz2                                 */ \
    /*   residual  r = (the MGX_RESIDUAL_CORRECT residual) + s*c on the interior, 0 on the boundary      */ \
    /*   operator  q = A p = -(residual of p with f = 0)                                                 */ \
    /* With s = 0 they give the bits of mgx3dxs_relax / _residual(CORRECT) / _laplace_dot.  Every entry  */ \
    /* returns MGX_ERR_INVALID unless s is finite and >= 0, MGX_ERR_SIZE for sizes that are not odd and  */ \
    /* >= 3; pad entries are neither written nor read as data.                                           */ \
    /* relax_shift: ncycles red-black sweeps in place, one launch per colour; mgx_ctx_last_relax_kernel  */ \
    /*   names the kernel.  relax_shift_from_zero: the contract of mgx3dxs_relax_from_zero (v counts as  */ \
    /*   zero; rim_is_zero != 0: its boundary and pad entries are zero in memory, nothing is filled and  */ \
    /*   the first red pass does not read v).                                                            */ \
    int mgx3dxs_relax_shift_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], \
                                  real s, int ncycles);                                                 \
    int mgx3dxs_relax_shift_from_zero_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3],       \
                                            const real h[3], real s, int ncycles, int rim_is_zero);     \
    /* residual_shift: r is stored unless it is NULL; unless dev_sumsq is NULL, *dev_sumsq = the sum of  */ \
    /*   the squared residuals in double, in a fixed order (the same bits on every run); dev_work:       */ \
    /*   mgx3dxs_krylov_work_elems doubles (unused without dev_sumsq).  Asynchronous.                    */ \
    int mgx3dxs_residual_shift_##SFX(mgx_ctx* ctx, const real* v, const real* f, real* r,               \
                                     const int n[3], const real h[3], real s, double* dev_work,         \
                                     double* dev_sumsq);                                                \
    /* residual_restrict_shift: coarse_f = Restrict(residual), the fine residual never stored; cn halves */ \
    /*   the axes of a mask in 1 .. 7 (as mgx3dxs_residual_restrict_axes reads it off n / cn; 7 = the    */ \
    /*   reference's full weighting).  The coarse boundary is set to 0 unless coarse_rim_is_zero != 0.   */ \
    int mgx3dxs_residual_restrict_shift_##SFX(mgx_ctx* ctx, const real* v, const real* f, const int n[3], \
                                              const real h[3], real s, real* coarse_f, const int cn[3], \
                                              int coarse_rim_is_zero);                                  \
    /* laplace_dot_shift: mgx3dxs_laplace_dot's contract with the shifted A                              */ \
    int mgx3dxs_laplace_dot_shift_##SFX(mgx_ctx* ctx, const real* p, real* q, const int n[3],           \
                                        const real h[3], real s, double* dev_work, double* dev_sum);    \
    /* shift_rhs: f = (-(s*u)) - qscale*q on the interior, f = -(s*u) when q is NULL: the right-hand     */ \
    /*   side of a backward Euler step.  The boundary and pad entries of f are not written.             */ \
    int mgx3dxs_shift_rhs_##SFX(mgx_ctx* ctx, const real* u, const real* q, real qscale, real s,        \
                                real* f, const int n[3]);                                               \
    /* ---- the variable-coefficient operator div(a grad u) - s u = f, a > 0 at the grid nodes, s >= 0, */ \
    /* x-split layout (csrc/mgx_coef3d.hip).  An addition: heterogeneous diffusion.  a is an array of   */ \
    /* the level's layout that holds ALL points (interior points next to a face read it on the          */ \
    /* boundary) and is never written.  Arithmetic, in `real`, left to right, nothing contracted        */ \
    /* (O/E = x-1/x+1, N/S = y-1/y+1, D/U = z-1/z+1, c the centre, aO .. aU, aC the coefficient there,  */ \
    /* qx = (real)0.5 / (h[0]*h[0]), likewise qy, qz):                                                  */ \
    /*   AW = aO + aC, AE = aE + aC, AN = aN + aC, AS = aS + aC, AD = aD + aC, AU = aU + aC             */ \
    /*   tx = qx*(AW*(O - c) + AE*(E - c)), ty = qy*(AN*(N - c) + AS*(S - c)),                          */ \
    /*   tz = qz*(AD*(D - c) + AU*(U - c))                                                              */ \
    /*   residual  r = (((f - tx) - ty) - tz) + s*c on the interior, 0 on the boundary                  */ \
    /*   operator  q = A p = -(residual of p with f = 0)                                                */ \
    /*   smoother  v = num / den, den = ((qx*(AW + AE) + qy*(AN + AS)) + qz*(AD + AU)) + s,             */ \
    /*             num = ((qx*(AW*O + AE*E) + qy*(AN*N + AS*S)) + qz*(AD*D + AU*U)) - f                 */ \
    /* Every entry returns MGX_ERR_INVALID for NULL arguments or an s that is not finite and >= 0,      */ \
    /* MGX_ERR_SIZE for sizes that are not odd and >= 3; pad entries are neither written nor read as    */ \
    /* data.  The values of a are not checked here (mgMultiGrid3D_<r>_set_coefficient does).            */ \
    /* relax_coef / relax_coef_from_zero: the contracts of relax_shift / relax_shift_from_zero (with    */ \
    /*   rim_is_zero the first red pass reads f and a only); mgx_ctx_last_relax_kernel reports the      */ \
    /*   name relax_coef3d_xs_kernel (the colour pass both operators share, instantiated for this       */ \
    /*   one).  residual_coef: residual_shift's contract (r and / or the sum of squares).               */ \
    /*   apply_coef_dot: laplace_dot_shift's contract (q = A p on the interior, <p, q>).                */ \
    int mgx3dxs_relax_coef_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const int n[3],   \
                                 const real h[3], real s, int ncycles);                                 \
    int mgx3dxs_relax_coef_from_zero_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a,         \
                                           const int n[3], const real h[3], real s, int ncycles,        \
                                           int rim_is_zero);                                            \
    int mgx3dxs_residual_coef_##SFX(mgx_ctx* ctx, const real* v, const real* f, const real* a, real* r, \
                                    const int n[3], const real h[3], real s, double* dev_work,          \
                                    double* dev_sumsq);                                                 \
    int mgx3dxs_apply_coef_dot_##SFX(mgx_ctx* ctx, const real* p, const real* a, real* q,               \
                                     const int n[3], const real h[3], real s, double* dev_work,         \
                                     double* dev_sum);                                                  \
    /* ---- homogeneous Neumann faces for the two operators above, x-split layout (csrc/mgx_rim3d.hip,  */ \
    /* DESIGN.md 15).  An addition.  bc is a mask of six bits -- bit 0 x-low, 1 x-high, 2 y-low,        */ \
    /* 3 y-high, 4 z-low, 5 z-high -- and a set bit makes that face homogeneous Neumann, du/dn = 0      */ \
    /* (a mirrored too).  A point is an UNKNOWN when it is interior, or lies on one or more Neumann     */ \
    /* faces and on no Dirichlet face (Dirichlet wins on shared edges and corners; Dirichlet entries    */ \
    /* of v are data and are never written).  At an unknown on a face every operator is the interior's  */ \
    /* point expression on a star whose out-of-range entry is replaced by the opposite one (x-low:      */ \
    /* O := E, for v and for a; edges and corners: on each axis).  A prescribed flux g enters through   */ \
    /* f, f -= 2 g a / h at the face for the outward derivative du/dn = g; no entry takes g.            */ \
    /* Each entry is the entry without _bc, argument for argument, plus the mask; with bc = 0 it does   */ \
    /* exactly what that entry does, bit for bit.  Otherwise the interior kernels run unchanged and     */ \
    /* each is followed by one launch over the face unknowns of all six faces (a colour pass: the       */ \
    /* interior launch, then the face launch of that colour).  MGX_ERR_INVALID for NULL arguments, a    */ \
    /* bc outside 0 .. 63 or a bad shift, MGX_ERR_SIZE for bad sizes; pads are neither written nor read */ \
    /* as data; f and a are never written.                                                              */ \
    /* residual_*_bc: r is stored at every unknown and is 0 at the Dirichlet points; *dev_sumsq = the   */ \
    /*   unweighted sum over ALL unknowns, in double, in a fixed order (the same bits on every run);    */ \
    /*   dev_work: mgx3dxs_krylov_work_elems doubles as before.                                         */ \
    /* restrict_bc: a coarse unknown on a face is the full weighting of the 27 reflected fine values;   */ \
    /*   coarse Dirichlet points keep injection.  interpolate(_correct)_bc: the interpolation formula   */ \
    /*   at the fine face unknowns too; it reads coarse points of the same face only.                   */ \
    /* shift_rhs_bc: shift_rhs on the face unknowns too.                                                */ \
    /* set_rim_bc: v := value on the face unknowns, nothing else (bc = 0: nothing at all).              */ \
    int mgx3dxs_relax_shift_bc_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3],              \
                                     const real h[3], real s, int ncycles, int bc);                     \
    int mgx3dxs_relax_coef_bc_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a,                \
                                    const int n[3], const real h[3], real s, int ncycles, int bc);      \
    int mgx3dxs_residual_shift_bc_##SFX(mgx_ctx* ctx, const real* v, const real* f, real* r,            \
                                        const int n[3], const real h[3], real s, double* dev_work,      \
                                        double* dev_sumsq, int bc);                                     \
    int mgx3dxs_residual_coef_bc_##SFX(mgx_ctx* ctx, const real* v, const real* f, const real* a,       \
                                       real* r, const int n[3], const real h[3], real s,                \
                                       double* dev_work, double* dev_sumsq, int bc);                    \
    int mgx3dxs_restrict_bc_##SFX(mgx_ctx* ctx, const real* fine, const int fn[3], real* coarse,        \
                                  const int cn[3], int bc);                                             \
    int mgx3dxs_interpolate_bc_##SFX(mgx_ctx* ctx, real* fine, const int fn[3], const real* coarse,     \
                                     const int cn[3], int bc);                                          \
    int mgx3dxs_interpolate_correct_bc_##SFX(mgx_ctx* ctx, real* v, const int n[3],                     \
                                             const real* coarse_v, const int cn[3], int bc);            \
    int mgx3dxs_shift_rhs_bc_##SFX(mgx_ctx* ctx, const real* u, const real* q, real qscale, real s,     \
                                   real* f, const int n[3], int bc);                                    \
    int mgx3dxs_set_rim_bc_##SFX(mgx_ctx* ctx, real* v, const int n[3], real value, int bc);            \
    /* The vector kernels of the solve over ALL unknowns (csrc/mgx_rim3d.hip): flexible CG */ \
    /* on a hierarchy with a mask works in the inner product <a, b>_W = sum of W a b over the unknowns, */ \
    /* W = 1/2 per Neumann face an unknown lies on (the trapezoid weights of section 15, in which A is */ \
    /* symmetric), 1 in the interior.  Each entry is the entry without _bc plus the mask; with bc = 0 it */ \
    /* calls that entry and nothing else.  Otherwise the interior launch runs unchanged, one launch over */ \
    /* the face unknowns follows it, its block partials go behind the interior launch's in dev_work and */ \
    /* one final sum adds both, in a fixed order: the same bits on every run.  Dirichlet entries are  */ \
    /* never written and pads neither read as data nor written.  MGX_ERR_INVALID for NULL arguments and */ \
    /* a bc outside 0 .. 63, checked before any argument is used; MGX_ERR_SIZE for bad sizes.         */ \
    /* krylov_work_elems_bc: the doubles of dev_work these entries need: two sums, each the interior  */ \
    /*   partials plus the most rim partials of any mask (mgx3dxs_krylov_work_elems keeps its value). */ \
    /* laplace_dot_shift_bc, apply_coef_dot_bc: q = A p at every unknown (at a face unknown the interior */ \
    /*   expression on the reflected star), *dev_sum = <p, q>_W.  The plain Laplacian is s = 0.       */ \
    /* cg_update_bc: [x += a p;] r -= a q at every unknown; *dev_sum = <r, r>, UNWEIGHTED over all    */ \
    /*   unknowns: the stopping rule's norm, that of residual_*_bc.                                   */ \
    /* dot2_bc: dev_sum[0] = <a, b>_W and, unless c is NULL, dev_sum[1] = <a, c>_W.                   */ \
    /* cg_direction_bc: the three forms of cg_direction at every unknown.                             */ \
    /* project_bc: *dev_mean = sum_W(a) / sum(W) in double, then a -= (real)*dev_mean at every unknown, */ \
    /*   with no host read in between (bc = 0: the interior and its plain mean).                      */ \
    size_t mgx3dxs_krylov_work_elems_bc_##SFX(const int n[3]);                                          \
    int mgx3dxs_laplace_dot_shift_bc_##SFX(mgx_ctx* ctx, const real* p, real* q, const int n[3],        \
                                           const real h[3], real s, double* dev_work, double* dev_sum,  \
                                           int bc);                                                     \
    int mgx3dxs_apply_coef_dot_bc_##SFX(mgx_ctx* ctx, const real* p, const real* a, real* q,            \
                                        const int n[3], const real h[3], real s, double* dev_work,      \
                                        double* dev_sum, int bc);                                       \
    int mgx3dxs_cg_update_bc_##SFX(mgx_ctx* ctx, real* x, const real* p, real* r, const real* q,        \
                                   const int n[3], const double* dev_alpha, double* dev_work,           \
                                   double* dev_sum, int bc);                                            \
    /* sumsq_bc: *dev_sum = the UNWEIGHTED sum of a^2 over all unknowns, the norm of a stored residual */ \
    /*   (bc = 0: mgx3dxs_dot2(a, a)'s bits); dev_work as for the entries above.                        */ \
    int mgx3dxs_sumsq_bc_##SFX(mgx_ctx* ctx, const real* a, const int n[3], double* dev_work,           \
                               double* dev_sum, int bc);                                                \
    int mgx3dxs_dot2_bc_##SFX(mgx_ctx* ctx, const real* a, const real* b, const real* c, const int n[3],\
                              double* dev_work, double* dev_sum, int bc);                               \
    int mgx3dxs_cg_direction_bc_##SFX(mgx_ctx* ctx, real* x, real* p, const real* z, const int n[3],    \
                                      const double* dev_alpha, const double* dev_beta, int bc);         \
    int mgx3dxs_project_bc_##SFX(mgx_ctx* ctx, real* a, const int n[3], double* dev_work, double* dev_mean, int bc);\
    /* ---- the operator with a capacity, div(a grad u) - (s c) u = f, c >= 0 at the grid nodes next to */ \
    /* the coefficient a, x-split layout (csrc/mgx_cap3d.hip).  An addition: the implicit */ \
    /* step of c u_t = kappa div(a grad u) + q, reaction terms that vary in space.  c is an array of    */ \
    /* the level's layout, read at the updated point only and never written.  Arithmetic: in `real`, sc */ \
    /* = s * c_P (one rounding), then the coefficient operator's expressions above with sc where they   */ \
    /* take s; with c == 1 every entry gives the bits of its _coef entry.  At an unknown on a Neumann   */ \
    /* face the capacity is that of the point itself.                                                   */ \
    /* Each entry is the _coef entry (cap_rhs: the shift_rhs entry), argument for argument, plus `const */ \
    /* real* c` after a (cap_rhs: after u), with that entry's contract: MGX_ERR_INVALID for NULL        */ \
    /* arguments, a bad s or a bc outside 0 .. 63, MGX_ERR_SIZE for bad sizes; f, a and c are never     */ \
    /* written, pads are neither read as data nor written, the sums give the same bits on every run.    */ \
    /* The values of c are not checked here (mgMultiGrid3D_<r>_set_capacity does).                      */ \
    /* mgx_ctx_last_relax_kernel reports relax_cap3d_xs_kernel / relax_cap_zero3d_xs_kernel.            */ \
    /* cap_rhs: f = (-((s*c)*u)) - qscale*q, f = -((s*c)*u) when q is NULL.                             */ \
    int mgx3dxs_relax_cap_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const real* c,     \
                                const int n[3], const real h[3], real s, int ncycles);                  \
    int mgx3dxs_relax_cap_from_zero_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a,          \
                                          const real* c, const int n[3], const real h[3], real s,       \
                                          int ncycles, int rim_is_zero);                                \
    int mgx3dxs_residual_cap_##SFX(mgx_ctx* ctx, const real* v, const real* f, const real* a,           \
                                   const real* c, real* r, const int n[3], const real h[3], real s,     \
                                   double* dev_work, double* dev_sumsq);                                \
    int mgx3dxs_apply_cap_dot_##SFX(mgx_ctx* ctx, const real* p, const real* a, const real* c, real* q, \
                                    const int n[3], const real h[3], real s, double* dev_work,          \
                                    double* dev_sum);                                                   \
    int mgx3dxs_cap_rhs_##SFX(mgx_ctx* ctx, const real* u, const real* c, const real* q, real qscale,   \
                              real s, real* f, const int n[3]);                                         \
    int mgx3dxs_relax_cap_bc_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const real* c,  \
                                   const int n[3], const real h[3], real s, int ncycles, int bc);       \
    int mgx3dxs_residual_cap_bc_##SFX(mgx_ctx* ctx, const real* v, const real* f, const real* a,        \
                                      const real* c, real* r, const int n[3], const real h[3], real s,  \
                                      double* dev_work, double* dev_sumsq, int bc);                     \
    int mgx3dxs_apply_cap_dot_bc_##SFX(mgx_ctx* ctx, const real* p, const real* a, const real* c,       \
                                       real* q, const int n[3], const real h[3], real s,                \
                                       double* dev_work, double* dev_sum, int bc);                      \
    int mgx3dxs_cap_rhs_bc_##SFX(mgx_ctx* ctx, const real* u, const real* c, const real* q, real qscale,\
                                 real s, real* f, const int n[3], int bc);                              \
    /* ---- convective (Robin) and prescribed-flux walls, x-split layout (csrc/mgx_wall3d.hip, DESIGN.md */\
    /* 18).  An addition.  On a face flagged in bc the wall law is a du/dn + beta u = g (n outward, beta */\
    /* >= 0 and g constants per face, in the units of the entry's operator div(a grad u); a = 1 for the */\
    /* shifted operator).  beta[k] and g[k] belong to the face of bit k (x-low, x-high, y-low, y-high,  */\
    /* z-low, z-high).  The half cell at a face unknown gains 2 (g - beta u_P) / h per wall face it     */\
    /* lies on, h the spacing along the face's axis: the operator a diagonal term, d_k = ((real)2 *     */\
    /* beta_k) / h_axis(k), summed over the point's faces in the order x, y, z into d(P); where d(P) != */\
    /* 0 the point is the operator's own expression with the effective shift s + d(P) (capacity: s *   */\
    /* c_P + d(P)), the shifted smoother a plain division in `real`; where d(P) == 0 it has the bits of */\
    /* the mirrored star alone.  Each _wall entry is the _bc entry of its name, argument for argument,  */\
    /* plus `const real beta[6]` last, with that entry's contract; beta NULL, a beta[k] negative or not */\
    /* finite, one != 0 on a face whose bit is clear, or one so large that 2 beta / h is not finite in  */\
    /* `real` (fp32: beyond about 1.7e38 h): MGX_ERR_INVALID.  A _bc entry and its _wall entry are two  */\
    /* names for one path: the _bc entry passes six zero betas, and one launch over the face unknowns   */\
    /* serves both.  bc = 63 with s = 0 is regular as soon as one beta[k] > 0.                          */\
    /* wall_rhs: f[P] = f[P] - ((real)2 * g[k]) / h_axis(k) at the face unknowns, successively for the  */\
    /* flagged faces of P with g[k] != 0 in the order x, y, z; nothing else of f is touched.  g[k] not  */\
    /* finite or != 0 on a face whose bit is clear: MGX_ERR_INVALID.  A g that varies along a face is   */\
    /* folded into f by the caller with the same formula, point by point.                               */\
    int mgx3dxs_relax_shift_wall_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3],            \
                                       const real h[3], real s, int ncycles, int bc, const real beta[6]);\
    int mgx3dxs_relax_coef_wall_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a,              \
                                      const int n[3], const real h[3], real s, int ncycles, int bc,     \
                                      const real beta[6]);                                              \
    int mgx3dxs_relax_cap_wall_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const real* c,\
                                     const int n[3], const real h[3], real s, int ncycles, int bc,      \
                                     const real beta[6]);                                               \
    int mgx3dxs_residual_shift_wall_##SFX(mgx_ctx* ctx, const real* v, const real* f, real* r,          \
                                          const int n[3], const real h[3], real s, double* dev_work,    \
                                          double* dev_sumsq, int bc, const real beta[6]);               \
    int mgx3dxs_residual_coef_wall_##SFX(mgx_ctx* ctx, const real* v, const real* f, const real* a,     \
                                         real* r, const int n[3], const real h[3], real s,              \
                                         double* dev_work, double* dev_sumsq, int bc, const real beta[6]);\
    int mgx3dxs_residual_cap_wall_##SFX(mgx_ctx* ctx, const real* v, const real* f, const real* a,      \
                                        const real* c, real* r, const int n[3], const real h[3], real s,\
                                        double* dev_work, double* dev_sumsq, int bc, const real beta[6]);\
    int mgx3dxs_laplace_dot_shift_wall_##SFX(mgx_ctx* ctx, const real* p, real* q, const int n[3],      \
                                             const real h[3], real s, double* dev_work, double* dev_sum,\
                                             int bc, const real beta[6]);                               \
    int mgx3dxs_apply_coef_dot_wall_##SFX(mgx_ctx* ctx, const real* p, const real* a, real* q,          \
                                          const int n[3], const real h[3], real s, double* dev_work,    \
                                          double* dev_sum, int bc, const real beta[6]);                 \
    int mgx3dxs_apply_cap_dot_wall_##SFX(mgx_ctx* ctx, const real* p, const real* a, const real* c,     \
                                         real* q, const int n[3], const real h[3], real s,              \
                                         double* dev_work, double* dev_sum, int bc, const real beta[6]);\
    int mgx3dxs_wall_rhs_##SFX(mgx_ctx* ctx, real* f, const int n[3], const real h[3], const real g[6], \
                               int bc);                                                                 \
    /* ---- harmonic-mean face coefficients for the coefficient and the capacity operator, x-split      */ \
    /* layout (csrc/mgx_hmean3d.hip).  An addition: the discretisation for a coefficient  */ \
    /* that belongs to the nodes (voxel data), where the interface lies midway between two nodes and a  */ \
    /* face carries the series conductance 2 aP aQ / (aP + aQ).  Arithmetic: the _coef / _cap           */ \
    /* expressions above with AW = (real)4 * ((aO * aC) / (aO + aC)) (likewise AE .. AU) where they     */ \
    /* form AW = aO + aC -- a plain division in `real`; nothing else differs.  A face has the same bits */ \
    /* seen from either node: the operator is symmetric bit for bit.  A constant coefficient 2^k gives  */ \
    /* the bits of the _coef / _cap entries.  One set of entries, in the _wall form: each is its        */ \
    /* _cap_wall namesake (relax_hmean_from_zero: relax_cap_from_zero), argument for argument and with  */ \
    /* that entry's contract, but c may be NULL: no capacity (the shift is s itself).  bc = 0 is the    */ \
    /* interior form, all betas zero the _bc form.  The values of a are not checked here: the products  */ \
    /* aP * aQ have to be normal and finite in `real` (mgMultiGrid3D_<r>_set_face_mean sees to it).     */ \
    /* mgx_ctx_last_relax_kernel reports relax_hmean3d_xs_kernel / relax_hmean_zero3d_xs_kernel, with a */ \
    /* capacity relax_hmean_cap3d_xs_kernel / relax_hmean_cap_zero3d_xs_kernel.                         */ \
    int mgx3dxs_relax_hmean_wall_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a,             \
                                       const real* c, const int n[3], const real h[3], real s,          \
                                       int ncycles, int bc, const real beta[6]);                        \
    int mgx3dxs_relax_hmean_from_zero_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a,        \
                                            const real* c, const int n[3], const real h[3], real s,     \
                                            int ncycles, int rim_is_zero);                              \
    int mgx3dxs_residual_hmean_wall_##SFX(mgx_ctx* ctx, const real* v, const real* f, const real* a,    \
                                          const real* c, real* r, const int n[3], const real h[3],      \
                                          real s, double* dev_work, double* dev_sumsq, int bc,          \
                                          const real beta[6]);                                          \
    int mgx3dxs_apply_hmean_dot_wall_##SFX(mgx_ctx* ctx, const real* p, const real* a, const real* c,   \
                                           real* q, const int n[3], const real h[3], real s,            \
                                           double* dev_work, double* dev_sum, int bc,                   \
                                           const real beta[6]);                                         \
    /* Pinned interior nodes (csrc/mgx_pin3d.hip; x-split only): interior points whose    */ \
    /* value is data.  A level's pinned points are a LIST of 32-bit storage offsets into the x-split    */ \
    /* array (device memory): the red points ((x + y + z) even) first, then the black ones, each colour */ \
    /* sorted by offset; end[0] = the number of red points, end[1] = the number of all; the values, one */ \
    /* per entry in list order, in a device array val (NULL: zeros).                                    */ \
    /* pin_list (host only, no launch): the list of a mask in the reference layout (mask[x + y sx +     */ \
    /*   z sx sy] != 0: pinned) into idx (host memory; NULL: only end[] is filled, to size it); with    */ \
    /*   val, val[t] = values[point t] (values: reference layout, all points; NULL: zeros).             */ \
    /*   MGX_ERR_INVALID for a true entry on the boundary of the box, naming the first one;             */ \
    /*   MGX_ERR_SIZE for bad sizes and for a level whose storage does not fit 32-bit offsets.          */ \
    /* pin_put: v[idx[t]] = val ? val[t] : 0 for t in [first, first + count): plain stores, one thread  */ \
    /*   per entry, nothing else of v is touched; count == 0 launches nothing.  The offsets are not     */ \
    /*   checked here: they have to lie inside v (pin_list's do).                                       */ \
    /* relax_*_pin: the _wall entry, argument for argument, plus the list: after the interior launch    */ \
    /*   (and the face launch) of a colour pass that colour's pinned entries of v are put back to val   */ \
    /*   (zeros), so that no pass ever reads an updated pinned point and v holds the data on return.    */ \
    /*   With end[1] == 0 it is the _wall entry, launch for launch.  v should hold the data at the pins */ \
    /*   on entry (the first red pass reads the black ones).  hmean: c == NULL means no capacity.       */ \
    int mgx3dxs_pin_list_##SFX(const int n[3], const unsigned char* mask, const real* values,           \
                               unsigned* idx, real* val, unsigned end[2]);                              \
    int mgx3dxs_pin_put_##SFX(mgx_ctx* ctx, real* v, const unsigned* idx, const real* val,              \
                              unsigned first, unsigned count);                                          \
    int mgx3dxs_relax_shift_pin_##SFX(mgx_ctx* ctx, real* v, const real* f, const int n[3],             \
                                      const real h[3], real s, int ncycles, int bc, const real beta[6], \
                                      const unsigned* idx, const unsigned end[2], const real* val);     \
    int mgx3dxs_relax_coef_pin_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a,               \
                                     const int n[3], const real h[3], real s, int ncycles, int bc,      \
                                     const real beta[6], const unsigned* idx, const unsigned end[2],    \
                                     const real* val);                                                  \
    int mgx3dxs_relax_cap_pin_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a, const real* c, \
                                    const int n[3], const real h[3], real s, int ncycles, int bc,       \
                                    const real beta[6], const unsigned* idx, const unsigned end[2],     \
                                    const real* val);                                                   \
    int mgx3dxs_relax_hmean_pin_##SFX(mgx_ctx* ctx, real* v, const real* f, const real* a,              \
                                      const real* c, const int n[3], const real h[3], real s,           \
                                      int ncycles, int bc, const real beta[6], const unsigned* idx,     \
                                      const unsigned end[2], const real* val);

MGX_DECLARE_OPS(f32, float)
MGX_DECLARE_OPS(f64, double)

/* ---- vector kernels of the mixed-precision solve (mgMultiGrid3D_f64_PCG_mixed), x-split layout ----------------------------
 * fp64 arrays (x, b, r, p, q) next to fp32 arrays of the same grid (r32, z32: the fp32 twin hierarchy's d_f[0] / d_v[0]), each in
 * the x-split geometry of its own precision.  The contract of the kernels above: interior points only, sums in double in a fixed
 * order, dev_work of mgx3dxs_mixed_work_elems_f64 doubles, asynchronous on the compute stream.  s (and inv_s = 1 / s) is meant to
 * be a power of two: r32 = (float)(r s) and z = (double)z32 * inv_s then rescale exactly.  An addition: the reference has no
 * Krylov solver.
 * mixed_work_elems: the most partials any of these kernels writes under any "mixed3d.*" setting -- the larger of the Krylov
 * kernels' 2 * ceil((sy - 2) / 4) * (sz - 2) and the z-marching pass's count at its smallest tiles ("mixed3d.rows" = 2,
 * "mixed3d.zchunk" = 1): ceil(((sx + 1) / 2 - 1) / 63) * ceil((sy - 2) / 8) * (sz - 2), which that setting writes exactly. */
size_t mgx3dxs_mixed_work_elems_f64(const int n[3]);
/* correct_residual_demote: with z32, xo = x + (double)z32 * inv_sz on the interior (xo != x: the pass is out of place, and xo's
 * boundary is left as it is), then r = b - A xo; without (z32 = NULL, xo unused) r = b - A x.  r (bit-identical to
 * mgx3dxs_residual_f64(..., MGX_RESIDUAL_CORRECT)) is not stored: r32 = (float)(r s) is, and *dev_sum = <r, r>.  One z-marching
 * launch, or two where the context's "mixed3d.fused" is 0 (a streaming correction into xo, then the pass on xo, which then
 * takes the boundary values from xo: the same bits when xo's boundary is x's). */
int mgx3dxs_correct_residual_demote_f64(mgx_ctx* ctx, const double* x, double* xo, const double* b, const float* z32, double inv_sz,
                                        float* r32, double s, const int n[3], const double h[3], double* dev_work, double* dev_sum);
/* correct_residual_demote_plan: what that call would launch on a level of these sizes and spacings with the context's present
 * "mixed3d.*" parameters, without launching: out = {rows per wave, planes per run, tiles across x, tiles across y, plane runs,
 * form of the residual (1: dividing, 3: exact reciprocals), launches (2: the streaming correction first; else 1)}.  The
 * z-marching launch writes tiles across x * tiles across y * plane runs partials. */
enum { MGX_CRD_ROWS = 0, MGX_CRD_ZCHUNK = 1, MGX_CRD_GX = 2, MGX_CRD_GY = 3, MGX_CRD_GZ = 4, MGX_CRD_MODE = 5, MGX_CRD_LAUNCHES = 6,
       MGX_CRD_PLAN = 7 };
int mgx3dxs_correct_residual_demote_plan_f64(const mgx_ctx* ctx, const int n[3], const double h[3], int with_correction,
                                             int out[MGX_CRD_PLAN]);
/* demote: r32 = (float)(r s) */
int mgx3dxs_demote_f64(mgx_ctx* ctx, const double* r, float* r32, double s, const int n[3]);
/* cg_update_demote: x += a p (skipped when x is NULL), r -= a q with a = *dev_alpha, r32 = (float)(r s); *dev_sum = <r, r> */
int mgx3dxs_cg_update_demote_f64(mgx_ctx* ctx, double* x, const double* p, double* r, const double* q, float* r32, double s,
                                 const int n[3], const double* dev_alpha, double* dev_work, double* dev_sum);
/* dot2_mixed: dev_sum[0] = <z, b> and, unless c is NULL, dev_sum[1] = <z, c>, with z = (double)z32 * inv_s */
int mgx3dxs_dot2_mixed_f64(mgx_ctx* ctx, const float* z32, double inv_s, const double* b, const double* c, const int n[3],
                           double* dev_work, double* dev_sum);
/* cg_direction_mixed: x += *dev_alpha * p with the old p (skipped when x is NULL), then p = z + *dev_beta * p, or p = z when
 * dev_beta is NULL, with z = (double)z32 * inv_s */
int mgx3dxs_cg_direction_mixed_f64(mgx_ctx* ctx, double* x, double* p, const float* z32, double inv_s, const int n[3],
                                   const double* dev_alpha, const double* dev_beta);

/* State vector of the flexible CG solve, MGX_CG_STATE device doubles, and its scalar steps (one thread, on the compute stream):
 *   step 0: alpha = RZ / PQ; NaN when PQ is 0 or alpha or PQ is not finite (a breakdown: the following cg_update then
 *           reports a NaN norm);
 *   step 1: beta = -alpha ZQ / RZ (Polak-Ribiere: = <z, r_new - r_old> / <r_old, z_old>), then RZ = ZR;
 *   step 2: RZ = ZR (restart).
 * FMEAN is no part of the iteration: the weighted mean mgMultiGrid3D_<r>_PCG removed from the right-hand side of a closed box
 * without a shift (mg_multigrid.h), 0 after every other solve. */
enum { MGX_CG_RZ = 0, MGX_CG_PQ = 1, MGX_CG_ALPHA = 2, MGX_CG_RR = 3, MGX_CG_ZR = 4, MGX_CG_ZQ = 5, MGX_CG_BETA = 6, MGX_CG_FMEAN = 7,
       MGX_CG_STATE = 8 };
int mgx_cg_scalars(mgx_ctx* ctx, double* dev_state, int step);

/* ---- block vector kernels of the eigensolver (mgMultiGrid3D_f64_Eigen), x-split layout, fp64 -------------------------------
 * An addition: the reference has no eigensolver.  Vectors come in groups: U, V, S, out, AX, X and R are HOST arrays of device
 * pointers, each to an array of mgx3dxs_elems_f64 doubles.  Every kernel runs over all grid points and forms a point's weight
 * from its position and the face mask bc (bit k = face k, x-low, x-high, y-low, y-high, z-low, z-high): 0 at a Dirichlet point (a
 * point on a face whose bit is clear), otherwise 1/2 per face it lies on -- the weights W of the _bc entries above, so one launch
 * serves every mask.  Entries of Dirichlet points and pads are never read as data, and pads are never written.  Sums are
 * accumulated in double in a fixed order (the same bits on every run); dev_work: mgx3dxs_block_work_elems_f64 doubles.
 * MGX_ERR_INVALID for NULL arguments (a NULL entry of a pointer array included), counts outside their ranges and a bc outside
 * 0 .. 63, checked before anything is launched; MGX_ERR_SIZE for bad sizes.  Asynchronous on the compute stream; the pointer
 * arrays, Y and mu are read before the call returns. */
size_t mgx3dxs_block_work_elems_f64(const int n[3]);
/* block_gram: for 1 <= nu, nv <= 4: dev_out[i * nv + j] = <U_i, V_j>_W and, unless c is NULL,
 * dev_out[nu * nv + i * nv + j] = <U_i, c V_j>_W (c: an array of the grid, the capacity) */
int mgx3dxs_block_gram_f64(mgx_ctx* ctx, int nu, const double* const* U, int nv, const double* const* V, const double* c,
                           const int n[3], int bc, double* dev_work, double* dev_out);
/* block_combine: out_i = ((Y[0][i] S_0 + Y[1][i] S_1) + Y[2][i] S_2) + ... at the unknowns, for 1 <= nin <= 12 inputs and
 * 1 <= nout <= 4 outputs; Y: nin x nout HOST doubles, row-major.  Products and sums are formed in exactly that order, none
 * contracted.  An output may be one of the inputs (a thread reads all inputs of a point before it writes); entries of
 * Dirichlet points and pads of the outputs stay as they are. */
int mgx3dxs_block_combine_f64(mgx_ctx* ctx, int nin, const double* const* S, int nout, double* const* out, const double* Y,
                              const int n[3], int bc);
/* block_residual: for 1 <= nvec <= 4: R_i = AX_i + mu_i * (c * X_i) (c NULL: mu_i * X_i) at the unknowns and 0 at the
 * Dirichlet points; dev_out[i] = <R_i, R_i>_W, dev_out[nvec + i] = <X_i, X_i>_W.  mu: nvec HOST doubles. */
int mgx3dxs_block_residual_f64(mgx_ctx* ctx, int nvec, const double* const* AX, const double* const* X, const double* c,
                               const double* mu, double* const* R, const int n[3], int bc, double* dev_work, double* dev_out);
/* eigen_start: v = pseudo-random values in (-1, 1) at the unknowns, from a fixed integer hash of (index, x, y, z), and 0 at the
 * Dirichlet points; index >= 0 */
int mgx3dxs_eigen_start_f64(mgx_ctx* ctx, double* v, int index, const int n[3], int bc);

/* ---- multi-GPU: z-slab halo exchange over RCCL (xGMI) ------------------------------
 * One process per GPU.  The unique id is created on rank 0 (mgx_comm_unique_id) and
 * handed to the other ranks by the launcher (bench.py broadcasts it with
 * torch.distributed); every rank then calls mgx_comm_init.  All communication runs on the
 * context's comm stream; mgx_comm_* functions that move planes take care of the
 * event ordering against the compute stream.
 */
#define MGX_UNIQUE_ID_BYTES 128
int mgx_comm_unique_id(void* host_id_bytes);
int mgx_comm_init(mgx_ctx* ctx, const void* host_id_bytes, int rank, int nranks);
/* rehearsal of ONE rank of a larger job on a single GPU (timing only, results are meaningless): a one-rank RCCL
 * communicator whose context reports (virtual_rank, virtual_nranks); every message keeps its size and its place in the
 * schedule but travels from this rank to itself */
int mgx_comm_init_rehearsal(mgx_ctx* ctx, const void* host_id_bytes, int virtual_rank, int virtual_nranks);
int mgx_comm_destroy(mgx_ctx* ctx);
int mgx_comm_rank(const mgx_ctx* ctx, int* rank, int* nranks);
/* 1 when the context's collectives can be captured into a HIP graph (an RCCL communicator, or a single rank without
 * one); 0 with the in-process test transport, whose exchanges are coordinated on the host */
int mgx_comm_capturable(const mgx_ctx* ctx);
/* the number of ranks the communicator itself reports (ncclCommCount) and the RCCL version in use (ncclGetVersion) */
int mgx_comm_info(const mgx_ctx* ctx, int* ranks_seen, int* rccl_version);
/* Test transport: `nranks` host threads of one process, one context each, all on the same device, so that the
 * slab-decomposed cycle AND the event ordering of its overlap schedule can be verified on a single-GPU box.  Same
 * stream semantics as RCCL: an exchange only enqueues device-to-device copies on the comm stream, ordered against
 * the peers by cross-context events; nothing is synchronised by the host; the compute stream sees the result only
 * through mgx_comm_wait.  Every rank's thread must take part in every exchange (as with RCCL).
 * _set_test_hooks: delay_us > 0 starts every transfer that late on the receiving comm stream (a missing wait then
 * reads stale ghosts for certain); drop_waits != 0 turns mgx_comm_wait into a no-op for the group's contexts (fault
 * injection: the tests must notice).  The hooks exist on this test transport only. */
typedef struct mgx_local_group mgx_local_group;
int mgx_local_group_create(int nranks, mgx_local_group** out);
int mgx_local_group_destroy(mgx_local_group* group);
int mgx_local_group_set_test_hooks(mgx_local_group* group, int delay_us, int drop_waits);
int mgx_comm_init_local(mgx_ctx* ctx, mgx_local_group* group, int rank);
/* Exchange ghost planes with the z-neighbours on a non-periodic chain of ranks (rank-1 = "lower",
 * rank+1 = "upper").  Counts are in elements of elem_bytes (4 or 8) and must match what the
 * neighbour passes for the opposite direction.  Buffers towards a missing neighbour are ignored.
 * Asynchronous on the comm stream: it first waits for everything enqueued so far on the compute
 * stream; mgx_comm_wait makes the compute stream wait for the exchange. */
int mgx_comm_halo_exchange(mgx_ctx* ctx, const void* send_to_lower, size_t count_to_lower, void* recv_from_lower,
                           size_t count_from_lower, const void* send_to_upper, size_t count_to_upper,
                           void* recv_from_upper, size_t count_from_upper, int elem_bytes);
int mgx_comm_wait(mgx_ctx* ctx);
/* Half planes for the ghost exchange behind a colour pass: only the half-rows that hold `colour` (even-x half where
 * colour + y + z is even, z = the plane's GLOBAL index) are packed into a staging array of mgx3dxs_halfplane_elems
 * elements (compute stream), exchanged with mgx_comm_halo_exchange, and unpacked into the ghost plane on the stream the
 * receive was enqueued on (mgx_comm_wait covers it).  Two planes per call (either may be NULL).
 * The staging array has one row of H = roundup((sx + 1) / 2, A) elements per row y of the plane (A, H, H2 as in the x-split
 * layout).  A row's half is copied WHOLE, pad entries included: H elements of an even-x half, H2 = roundup(sx / 2, A) of an
 * odd-x half, from / to the start of the staging row; the staging elements H2 ... H - 1 of such a row, everything behind
 * halfplane_elems, the other half of every row of the plane and every other plane are neither read nor written.  No-ops on a
 * context without a communicator. */
size_t mgx3dxs_halfplane_elems_f32(int sx, int sy);
size_t mgx3dxs_halfplane_elems_f64(int sx, int sy);
int mgx3dxs_halo_pack_f32(mgx_ctx* ctx, const float* plane_a, int z_a, float* stage_a, const float* plane_b, int z_b, float* stage_b, int sx,
                          int sy, int colour);
int mgx3dxs_halo_pack_f64(mgx_ctx* ctx, const double* plane_a, int z_a, double* stage_a, const double* plane_b, int z_b, double* stage_b,
                          int sx, int sy, int colour);
int mgx3dxs_halo_unpack_f32(mgx_ctx* ctx, const float* stage_a, float* plane_a, int z_a, const float* stage_b, float* plane_b, int z_b, int sx,
                            int sy, int colour);
int mgx3dxs_halo_unpack_f64(mgx_ctx* ctx, const double* stage_a, double* plane_a, int z_a, const double* stage_b, double* plane_b, int z_b,
                            int sx, int sy, int colour);
/* on != 0: from now on collectives are enqueued on the COMPUTE stream, in order with the kernels (no overlap, no
 * cross-stream events; mgx_comm_wait is then a no-op); 0: back to the comm stream.  Every rank switches at the same
 * points of its schedule.  The slab driver switches per level (mgDistMultiGrid3D_*: inline_bytes). */
int mgx_comm_set_inline(mgx_ctx* ctx, int on);
/* all-gather `count` reals per rank (agglomeration of a coarse level) and all-reduce (sum, in place) of `count`
 * doubles (residual norm; every rank receives the same bits).  Both enqueue on the comm stream with the same
 * ordering rules, on both transports. */
int mgx_comm_allgather(mgx_ctx* ctx, const void* send, void* recv, size_t count, int elem_bytes);
int mgx_comm_allreduce_sum_f64(mgx_ctx* ctx, double* dev_inout, size_t count);
/* RCCL plumbing check usable on a single-GPU box: this rank sends `count` doubles to itself with a grouped
 * ncclSend/ncclRecv on the comm stream (the exact call pattern of the halo exchange). */
int mgx_comm_selftest(mgx_ctx* ctx, const double* dev_src, double* dev_dst, size_t count);

#ifdef __cplusplus
}
#endif
#endif /* MGX_H */
