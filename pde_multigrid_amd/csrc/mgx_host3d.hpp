// mgx_host3d.hpp -- the host side the 3D translation units share: launch shapes, argument checks and the declaration of every
// host function that one 3D unit defines and another one calls.
//
// One home per kernel: the library is compiled with -fno-gpu-rdc, so a unit that launches a kernel template gets a copy of
// that kernel in its own code object.  A launch site in another unit therefore calls the host function declared here, which
// lives beside the kernel; it never names the kernel template itself.
#pragma once
#include "mgx_kernels3d.hpp"

namespace mgx {

// Everything below is shared by the files of the library, not part of its interface: hidden from the symbol table of the
// shared object.
#pragma GCC visibility push(hidden)

inline dim3 blk() { return dim3(64, 4, 1); }
inline dim3 grd(int nx, int ny, int nz) { return dim3(ceil_div(nx, 64), ceil_div(ny, 4), nz); }

inline int check_n3(const int n[3], const char* what) {
    MGX_REQUIRE(n, MGX_ERR_INVALID, "%s: size array is NULL", what);
    for (int d = 0; d < 3; d++)
        MGX_REQUIRE(valid_size(n[d]), MGX_ERR_SIZE, "%s: size[%d] = %d is not odd and >= 3", what, d, n[d]);
    MGX_REQUIRE((double)n[0] * n[1] * n[2] < 2147483647.0 * 4, MGX_ERR_SIZE, "%s: grid too large", what);
    return MGX_OK;
}

inline int check_coarse3(const int fn[3], const int cn[3], const char* what) {
    MGX_REQUIRE(fn && cn, MGX_ERR_INVALID, "%s: size array is NULL", what);
    for (int d = 0; d < 3; d++)  // the reference asserts this (N3/MultiGrid3D.cpp:60-62)
        MGX_REQUIRE(cn[d] == (fn[d] - 1) / 2 + 1, MGX_ERR_SIZE, "%s: coarse size[%d] = %d != (%d-1)/2+1", what, d, cn[d],
                    fn[d]);
    return MGX_OK;
}

// the checks every entry of the residual+restrict family begins with (each entry checks its residual mode itself)
inline int check_rr_args(mgx_ctx* ctx, bool nonnull, const int n[3], const int cn[3], const char* what) {
    MGX_REQUIRE(nonnull, MGX_ERR_INVALID, "%s: NULL argument", what);
    MGX_USE(ctx);
    MGX_TRY_RET(check_n3(n, what));
    return check_coarse3(n, cn, what);
}

// What one unit defines and others call.  The templates are instantiated explicitly, for float and double, in the unit named
// above them.

// the largest extent of a level that the one-workgroup kernels of mgx_small3d.hip keep in LDS (the `takes` predicates of the
// other units leave such levels to them)
constexpr int SMALL_MAX = 17;

// ---- mgx_kernels3d.hip
// the colour-pass smoother, x-split layout (mgx_sweep3d.hip falls back to it)
template <class real>
int relax3d_xs_colour_passes(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], int ncycles);
template <class real>
int relax3d_xs_from_zero(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], int ncycles, int rim_is_zero);

// ---- mgx_pipe3d.hip: the pipelined smoothers (relax3d_xs_pipe_kernel, relax3d_xs_pipe_v2_kernel)
bool relax3d_lds_shape_known(int shape);  // is "relax3d.lds" = 100*WX + 10*WY + R a compiled workgroup shape? (mgx_core.hip)
// the shortest run of planes the automatic choice hands to the pipelined kernel (relax3d_xs_pass2 merges shorter ones)
template <class real>
int pipe_min_planes(int sx);
// How a pass of the pipelined kernels launches (pipe_plan decides it; false: they do not take the level)
enum class PipePass { Plain, Zero, Corr };  // a colour pass; the first sweep from zero (VAR = 3); the correcting red pass (VAR = 2)

struct PipePlan {
    bool v2 = false;            // relax3d_xs_pipe_v2_kernel (two x-pairs per lane)
    int WX = 2, WY = 8, R = 2;  // waves across x and y, rows per wave
    bool fnt = false;           // non-temporal loads of f
    int unr = 0;                // 0: the rolled step loop; unrolled four times: 1 + q0 (entry row parity q0), 3 + q0 requesting two steps ahead
    int zchunk = 0;             // planes per run (even when unrolled)
    int gx = 0, gy = 0;         // tiles across x and y
    dim3 grid, block;
    int xcd = 0;
    // the correcting pass corrects every value it reads from a neighbouring tile itself: no set P beforehand
    bool corrects_edges() const { return !v2 || unr; }
};
template <class real>
bool pipe_plan(const mgx_ctx* ctx, PipePass pass, int sx, int sy, int zbeg, int zend, int colour, PipePlan& p);
// one colour pass / the first sweep of a zero level on the pipelined kernels; false: not taken, the caller uses relax3d_xs_kernel
template <class real>
bool relax3d_xs_pass_lds(mgx_ctx* ctx, real* v, const real* f, int sx, int sy, int zbeg, int zend, real hx2, real hy2,
                         real hz2, int colour);
template <class real>
bool relax3d_xs_first_sweep_zero(mgx_ctx* ctx, real* v, const real* f, int sx, int sy, int sz, real hx2, real hy2, real hz2);
// the red pass that reads black through the coarse-grid correction (VAR = 2): does a level take it; its launch
bool corr_fused_takes(const mgx_ctx* ctx, int sx, int sy, int sz_global, int nplanes);
// ... without the number of planes: the rows and switches alone (what the z-slab entries of that pass check)
bool corr_fused_level_takes(const mgx_ctx* ctx, int sx, int sy, int sz_global);
template <class real>
void corr_red_launch(mgx_ctx* ctx, real* v, const real* f, int sx, int sy, int zb, int ze, real hx2, real hy2, real hz2, int colour,
                     const real* coarse_sh, int cx, int cy, int szl, int ckmax, int zg0 = 0, real* vout = nullptr);

// ---- mgx_transfer3d.hip: the transfers between levels (the two the composites of mgx_kernels3d.hip call: v += Interpolate(coarse_v)
// on a run of coarse planes, one colour or both; the set P of the correcting red pass corrected in place)
template <class real>
int interpolate_correct3d_slab(mgx_ctx* ctx, real* v, const int n[3], int fzoff, const real* coarse_v, const int cn[3],
                               int czoff, int pzbeg, int pzend, int colour, bool add = true);
template <class real>
void corr_pset_launch(mgx_ctx* ctx, real* v, int sx, int sy, int fzoff, const real* coarse_v, const int cn[3], int czoff, int zmin,
                      int zmax);

// ---- mgx_small3d.hip: all sweeps of a Relax call on a level of at most SMALL_MAX points per axis in one workgroup
template <class real, class L>
int relax3d_small(mgx_ctx* ctx, real* v, const real* f, const int n[3], real hx2, real hy2, real hz2, int ncycles);

// ---- mgx_rr3d.hip: residual + restrict
// How a residual+restrict launch runs (rr_plan decides it).  The kernels: the LDS rolling window (residual_restrict3d_kernel),
// the streaming shuffle kernel (residual_restrict3d_xs_kernel), the pipelined kernel (residual_restrict3d_xs_pipe_kernel), all
// three in mgx_rr3d.hip, and the fused black pass + residual + restrict (relax_rr3d_xs_kernel, mgx_relax_rr3d.hip).
enum class RRKernel { Window, Shuffle, Pipe, Black };
struct RRPlan {
    RRKernel kernel = RRKernel::Window;
    int T = 4, CR = 1, OWN = 4;       // waves per workgroup (TYW, T); Shuffle: coarse rows per lane; Pipe: fine rows per wave
    int gx = 0, gy = 0, pzchunk = 0;  // tiles across x and y, coarse planes per run
    dim3 grid, block;
    int xcd = 0;
};
bool rr_plan(const mgx_ctx* ctx, bool xsplit, bool black, const int n[3], const int cn[3], int planes, RRPlan& p);
template <class real, class L>
int residual_restrict3d(mgx_ctx* ctx, const real* v, const real* f, const int n[3], const real h[3], int mode, real* coarse_f,
                        const int cn[3], bool rim_is_zero = false);

// ---- mgx_semi3d.hip
// boundary points of an x-split array := 0 (rim_zero3d_xs_kernel; pads are not touched)
template <class real>
void rim_zero3d_xs(mgx_ctx* ctx, real* a, const int n[3]);

// ---- mgx_relax_rr3d.hip: the last black pass inside the residual+restrict launch
bool relax_rr3d_xs_takes(const mgx_ctx* ctx, const int n[3], const int cn[3], size_t elem);
template <class real>
bool relax_rr3d_xs_launch(mgx_ctx* ctx, real* v, const real* f, const int n[3], const real h[3], int mode, real* coarse_f,
                          const int cn[3], int fzoff, int czoff, int pzbeg, int pzend);

// ---- mgx_block3d.hip: three colour passes in one launch (fp64; the float form is never taken and does nothing)
bool relax_block3_takes(const mgx_ctx* ctx, const int n[3], size_t elem, int part);
template <class real>
void relax3d_xs_block3_launch(mgx_ctx* ctx, const real* vin, real* vout, const real* f, const int n[3], real hx2, real hy2, real hz2,
                              int first_colour, bool store_both, const real* coarse = nullptr, const int* cn = nullptr);
template <>
void relax3d_xs_block3_launch<float>(mgx_ctx*, const float*, float*, const float*, const int[3], float, float, float, int, bool, const float*,
                                     const int*);

// ---- mgx_sweep3d.hip: one launch per red+black sweep with a ping-pong partner array
struct SweepSync;                                // mgx_sync.hpp
int sweep_state(mgx_ctx* ctx, SweepSync* out);  // the context's progress words (allocated on first use)
template <class real>
int relax3d_xs_pp(mgx_ctx* ctx, real* v, real* w, const real* f, const int n[3], const real h[3], int ncycles, int w_rim_valid);
template <class real>
void copy_rim3d_xs(mgx_ctx* ctx, const real* v, real* w, const int n[3]);

// ---- mgx_resident3d.hip: all colour passes of a Relax call on a cache-resident level in one launch
bool relax3d_resident_takes(const mgx_ctx* ctx, const int n[3], int ncycles);
template <class real>
int relax3d_resident(mgx_ctx* ctx, real* v, const real* f, const int n[3], real hx2, real hy2, real hz2, int ncycles, int zero_start);

// ---- mgx_krylov3d.hip
// dev_sum[s] = the sum of work[s * count .. (s + 1) * count) for s < nsums, in a fixed order (also used by mgx_stencil3d.hpp)
int krylov_final(mgx_ctx* ctx, const double* work, size_t count, int nsums, double* dev_sum);
// the interior launches of mgx3dxs_cg_update / _dot2 / _cg_direction.  finalize = false: no final sum, the partials stay in dev_work
// (count = the blocks of the row walk's grid; cg_update's and dot2's <a, b> in [0, count), dot2's <a, c> in [count, 2 count)) for
// a caller that adds partials of its own (mgx_rim3d.hip: the face unknowns)
template <class real>
int cg_update3d(mgx_ctx* ctx, real* x, const real* p, real* r, const real* q, const int n[3], const double* dev_alpha, double* dev_work,
                double* dev_sum, bool finalize);
template <class real>
int dot2_3d(mgx_ctx* ctx, const real* a, const real* b, const real* c, const int n[3], double* dev_work, double* dev_sum, bool finalize);
template <class real>
int cg_direction3d(mgx_ctx* ctx, real* x, real* p, const real* z, const int n[3], const double* dev_alpha, const double* dev_beta);

#pragma GCC visibility pop

}  // namespace mgx
