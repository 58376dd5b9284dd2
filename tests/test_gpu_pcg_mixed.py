"""GPU suite: the mixed-precision solve of the 3D hierarchy (mgMultiGrid3D_f64_PCG_mixed, PCG(precond="f32")) and its kernels.

The kernels are checked against numpy restatements bit for bit (the sums to 1e-13); defect correction against its restatement
with the oracle's fp32 V-cycle bit for bit (the scale s is a power of two, so M(s r) / s = M(r) and no scale appears in it);
flexible CG against the flexible CG of test_gpu_pcg.py with that preconditioner."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
import pde_multigrid_amd as P
from conftest import bits_equal
from odd_shapes import pack_poisoned
from solve_restated import boundary_mask as _boundary_mask
from solve_restated import check_out as _check_out
from solve_restated import close as _close
from solve_restated import fsum_dot as _fsum_dot
from solve_restated import interior as _interior
from solve_restated import ir_restated, m32
from solve_restated import problem as _problem
from solve_restated import true_rel as _true_rel
import solve_restated

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RG = [-1, 1, 0, 2, 0.5, 3]
UNIT = [0, 1, 0, 1, 0, 1]
# the shapes and grids of test_gpu_pcg.py: at (23, 19, 13), (259, 9, 7) and (515, 5, 5) the fp32 and fp64 pads differ
SHAPES = [(17, 17, 17), (33, 17, 9), (23, 19, 13), (259, 9, 7), (515, 5, 5)]
GRIDS = [((33, 33, 33), UNIT, 0), ((65, 65, 65), UNIT, 0), ((65, 65, 65), [0, 1, 0, 1, 0, 4], 0), ((65, 33, 129), UNIT, 0),
         ((49, 41, 57), [0, 1, 0, 2, 0, 1], 3)]
S, INV = 2.0 ** 7, 2.0 ** -5  # scales of the kernel tests (any doubles: the kernels apply them as given)


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


def _rand(n3, dtype, seed):
    return np.random.default_rng(seed).uniform(-1, 1, O.shape(n3)).astype(dtype)


def _on_interior(base, val):
    out = base.copy()
    _interior(out)[...] = _interior(val)
    return out


# ---------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("n3", SHAPES)
@pytest.mark.parametrize("rg", ["aniso", "unit"])
@pytest.mark.parametrize("corr", ["fused", "two launches", None])
def test_correct_residual_demote(ctx, n3, rg, corr):
    rng = RG if rg == "aniso" else UNIT  # the unit cube: the exact-reciprocal form of the residual, else the dividing one
    x, b, xo0 = _rand(n3, np.float64, 1), _rand(n3, np.float64, 2), _rand(n3, np.float64, 3)
    xo0[_boundary_mask(n3)] = x[_boundary_mask(n3)]  # xo has x's boundary, as the solver's two iterate arrays have
    z, r0 = _rand(n3, np.float32, 4), _rand(n3, np.float32, 5)
    ux, ub, uo, uz, ur = (pack_poisoned(a) for a in (x, b, xo0, z, r0))
    ctx.set_param("mixed3d.fused", int(corr == "fused"))
    try:
        outs = [P.ops3dxs.correct_residual_demote(ctx, ux, ub, ur, n3, rng, S, z=uz if corr else None, inv_sz=INV,
                                                  xo=uo if corr else None) for _ in range(2)]
    finally:
        ctx.set_param("mixed3d.fused", 0)
    xo_st, r_st, rr = outs[0]
    xc = _on_interior(x, x + z.astype(np.float64) * INV) if corr else x
    r = O.residual3d(n3, rng, xc, b, P.CORRECT, dtype=np.float64)
    _check_out(n3, ur, r_st, (r * S).astype(np.float32), r0)
    if corr:
        _check_out(n3, uo, xo_st, xc, xo0)
    else:
        assert xo_st is None
    assert _close(rr, _fsum_dot(r, r), 1e-13), (rr, _fsum_dot(r, r))
    assert outs[1][2] == rr and bits_equal(outs[1][1], r_st) and (not corr or bits_equal(outs[1][0], xo_st)), "not the same bits"


@pytest.mark.parametrize("n3", SHAPES)
def test_demote(ctx, n3):
    r, r0 = _rand(n3, np.float64, 6), _rand(n3, np.float32, 7)
    ur = pack_poisoned(r0)
    got = P.ops3dxs.demote(ctx, pack_poisoned(r), ur, n3, S)
    _check_out(n3, ur, got, (r * S).astype(np.float32), r0)


@pytest.mark.parametrize("n3", SHAPES)
@pytest.mark.parametrize("with_x", [True, False])
def test_cg_update_demote(ctx, n3, with_x):
    x, p, r, q = (_rand(n3, np.float64, s) for s in (8, 9, 10, 11))
    r0 = _rand(n3, np.float32, 12)
    alpha = 0.3141592653589793
    ups = [pack_poisoned(a) for a in (x, p, r, q, r0)]
    res = [P.ops3dxs.cg_update_demote(ctx, ups[0] if with_x else None, ups[1], ups[2], ups[3], ups[4], n3, alpha, S) for _ in range(2)]
    xo, ro, o32, rr = res[0]
    want_r = r - alpha * q
    _check_out(n3, ups[2], ro, want_r, r)
    _check_out(n3, ups[4], o32, (want_r * S).astype(np.float32), r0)
    if with_x:
        _check_out(n3, ups[0], xo, x + alpha * p, x)
    assert _close(rr, _fsum_dot(want_r, want_r), 1e-13)
    assert res[1][3] == rr and bits_equal(res[1][2], o32)


@pytest.mark.parametrize("n3", SHAPES)
def test_dot2_mixed(ctx, n3):
    z, b, c = _rand(n3, np.float32, 13), _rand(n3, np.float64, 14), _rand(n3, np.float64, 15)
    uz, ub, uc = (pack_poisoned(a) for a in (z, b, c))
    zb, zc = P.ops3dxs.dot2_mixed(ctx, uz, INV, ub, uc, n3)
    zb2, none = P.ops3dxs.dot2_mixed(ctx, uz, INV, ub, None, n3)
    assert none is None and zb2 == zb
    assert (zb, zc) == P.ops3dxs.dot2_mixed(ctx, uz, INV, ub, uc, n3)
    zd = z.astype(np.float64) * INV
    assert _close(zb, _fsum_dot(zd, b), 1e-13) and _close(zc, _fsum_dot(zd, c), 1e-13)


@pytest.mark.parametrize("n3", SHAPES)
@pytest.mark.parametrize("form", ["x+p", "p", "x+copy", "copy"])
def test_cg_direction_mixed(ctx, n3, form):
    x, p, z = _rand(n3, np.float64, 16), _rand(n3, np.float64, 17), _rand(n3, np.float32, 18)
    alpha, beta = -0.7071067811865476, 1.4142135623730951
    ux, up, uz = (pack_poisoned(a) for a in (x, p, z))
    use_x, use_b = form.startswith("x"), form in ("x+p", "p")
    xo, po = P.ops3dxs.cg_direction_mixed(ctx, ux if use_x else None, up, uz, INV, n3, alpha=alpha if use_x else None,
                                          beta=beta if use_b else None)
    zd = z.astype(np.float64) * INV
    _check_out(n3, up, po, zd + beta * p if use_b else zd, p)
    if use_x:
        _check_out(n3, ux, xo, x + alpha * p, x)


# ---------------------------------------------------------------------------------------------------------- solver
def _mg(ctx, n3, rng, f=None, v=None, **kw):
    mg = P.MultiGrid3D(ctx, n3, rng, np.float64, residual_mode=P.CORRECT, **kw)
    mg.upload_v(0, np.zeros(O.shape(n3)) if v is None else v)
    mg.upload_f(0, _problem(n3) if f is None else f)
    return mg


def fcg_restated(n3, rng, v0, f, v1, v2, tol, maxit, nlevels=0):
    """flexible CG of mg_multigrid.h in numpy (test_gpu_pcg.py's) with the fp32 preconditioner"""
    return solve_restated.fcg_restated(n3, rng, v0, f, m32(n3, rng, v1, v2, nlevels), tol, maxit)


@pytest.mark.parametrize("case", range(len(GRIDS)))
def test_defect_correction_matches_restatement(ctx, case):
    n3, rng, nlev = GRIDS[case]
    f = _problem(n3)
    want = ir_restated(n3, rng, np.zeros_like(f), f, 2, 2, 5, nlevels=nlev)
    for steps in (1, 2, 3, 5):
        mg = _mg(ctx, n3, rng, f=f, nlevels=nlev)
        k, rel, conv, hist = mg.PCG(2, 2, 1e-300, steps, krylov=False, precond="f32")
        x = mg.download_v(0)
        mg.close()
        assert k == steps and not conv and len(hist) == steps
        assert bits_equal(x, want[steps - 1]), (case, steps)
        assert _close(rel, _true_rel(n3, rng, x, f, np.zeros_like(f)), 1e-10)


@pytest.mark.parametrize("case", range(len(GRIDS)))
def test_flexible_cg_matches_restatement(ctx, case):
    n3, rng, nlev = GRIDS[case]
    f = _problem(n3)
    want_x, want_k, want_h, want_c = fcg_restated(n3, rng, np.zeros_like(f), f, 2, 2, 1e-10, 200, nlevels=nlev)
    mg = _mg(ctx, n3, rng, f=f, nlevels=nlev)
    k, rel, conv, hist = mg.PCG(2, 2, 1e-10, 200, precond="f32")
    x = mg.download_v(0)
    mg.close()
    assert conv and want_c and rel < 1e-10
    assert abs(k - want_k) <= 1, (k, want_k)
    m = min(len(hist), len(want_h))
    upto = want_h[:m] >= 1e-10
    assert np.allclose(hist[:m][upto], want_h[:m][upto], rtol=1e-6, atol=0), (hist[:m], want_h[:m])
    assert np.abs(x - want_x).max() <= 1e-9 * np.abs(want_x).max()


@pytest.mark.parametrize("krylov", [False, True])
def test_mixed_reaches_what_fp32_cannot(ctx, krylov):
    n3, rng = (65, 65, 65), [0, 1, 0, 1, 0, 4]  # test_pcg_fp32_is_honest: fp32 stalls far above 1e-9 here
    f = _problem(n3)
    its = {}
    for precond in ("f64", "f32"):
        mg = _mg(ctx, n3, rng, f=f)
        k, rel, conv, _ = mg.PCG(2, 2, 1e-10, 200, krylov=krylov, precond=precond)
        x = mg.download_v(0)
        mg.close()
        assert conv and rel < 1e-10, (precond, k, rel)
        assert _true_rel(n3, rng, x, f, np.zeros_like(f)) < 1e-10
        its[precond] = k
    assert its["f32"] <= its["f64"] + (2 if krylov else 1), its


@pytest.mark.parametrize("krylov", [False, True])
def test_scale_invariance(ctx, krylov):
    n3, rng = (33, 33, 33), [0, 1, 0, 2, 0, 1]
    f = _problem(n3, seed=7)
    runs = {}
    for e in (0, -140, 120):
        mg = _mg(ctx, n3, rng, f=np.ldexp(f, e))
        k, rel, conv, hist = mg.PCG(2, 2, 1e-10, 100, krylov=krylov, precond="f32")
        runs[e] = (k, conv, mg.download_v(0), hist)
        mg.close()
    k0, conv0, x0, h0 = runs[0]
    assert conv0
    for e in (-140, 120):
        k, conv, x, hist = runs[e]
        assert (k, conv) == (k0, conv0), (e, k, k0)
        assert bits_equal(x, np.ldexp(x0, e)), e
        assert bits_equal(hist, h0), e


@pytest.mark.parametrize("krylov", [False, True])
def test_hierarchy_contract(ctx, krylov):
    n3, rng = (65, 33, 129), [0, 1, 0, 0.5, 0, 2]  # isotropic spacing: plain cycling converges as fast as it can
    f, v0 = _problem(n3, seed=3), _rand(n3, np.float64, 4)
    results = []
    for use_graph in (False, True, True):
        mg = _mg(ctx, n3, rng, f=f, v=v0)
        mg.use_graph = use_graph
        k, rel, conv, hist = mg.PCG(1, 1, 1e-9, 100, krylov=krylov, precond="f32")
        assert conv
        assert bits_equal(mg.download_f(0), f), "d_f[0] not restored"
        v = mg.download_v(0)
        assert bits_equal(v[_boundary_mask(n3)], v0[_boundary_mask(n3)])
        # a second call behaves like the first: it starts from the solution, with its own initial residual
        k2, rel2, conv2, _ = mg.PCG(1, 1, 1e-3, 20, krylov=krylov, precond="f32")
        assert conv2 and rel2 < 1e-3
        assert bits_equal(mg.download_f(0), f)
        v2 = mg.download_v(0)
        results.append((k, rel, hist, v, k2, v2))
        # the hierarchy goes on working as a hierarchy
        mg.VCycle(0, 2, 2)
        want = O.cycle3d(n3, rng, mode=0, v0=1, v1=2, v2=2, v=v2, f=f, residual_mode=O.CORRECT, dtype=np.float64)
        assert bits_equal(mg.download_v(0), want)
        mg.close()
    for k, rel, hist, v, k2, v2 in results[1:]:
        r0 = results[0]
        assert (k, rel, k2) == (r0[0], r0[1], r0[4]) and bits_equal(hist, r0[2]) and bits_equal(v, r0[3]) and bits_equal(v2, r0[5])


def test_twin_follows_num_grids(ctx):
    n3, rng = (65, 33, 129), UNIT
    f = _problem(n3, seed=5)
    want3 = ir_restated(n3, rng, np.zeros_like(f), f, 2, 2, 2, nlevels=3)[-1]
    want = ir_restated(n3, rng, np.zeros_like(f), f, 2, 2, 2)[-1]
    mg = _mg(ctx, n3, rng, f=f)
    full = mg.numGrids
    mg.numGrids = 3
    mg.PCG(2, 2, 1e-300, 2, krylov=False, precond="f32")
    assert bits_equal(mg.download_v(0), want3)
    mg.numGrids = full
    mg.upload_v(0, np.zeros(O.shape(n3)))
    mg.PCG(2, 2, 1e-300, 2, krylov=False, precond="f32")
    assert bits_equal(mg.download_v(0), want)
    mg.close()


# ---------------------------------------------------------------------------------------------------------- interfaces
@pytest.mark.parametrize("krylov", [False, True])
def test_solve3d_pcg_mixed(ctx, krylov):
    n3, rng = (33, 25, 41), [-1, 1, 0, 2, 0.5, 3]
    f = _problem(n3, seed=9)
    v0 = _rand(n3, np.float64, 10)
    _interior(v0)[...] = 0
    mg = _mg(ctx, n3, rng, f=f, v=v0, nlevels=3)
    k, rel, conv, _ = mg.PCG(2, 2, 1e-11, 100, krylov=krylov, precond="f32")
    x = mg.download_v(0)
    mg.close()
    got, k2, rel2, conv2 = P.solve3d_pcg(ctx, v0, f, rng, nlevels=3, v1=2, v2=2, tol=1e-11, maxit=100, krylov=krylov, precond="f32")
    assert conv and (k2, conv2) == (k, conv) and rel2 == rel and bits_equal(got, x)


def test_mixed_rejects_invalid_arguments(ctx):
    n3 = (17, 17, 17)
    mg = _mg(ctx, n3, UNIT)
    for args in [dict(tol=0), dict(tol=-1), dict(maxit=0), dict(v1=0, v2=0)]:
        kw = dict(v1=1, v2=1, tol=1e-8, maxit=10, precond="f32")
        kw.update(args)
        with pytest.raises(P.MgxError) as e:
            mg.PCG(**kw)
        assert e.value.status == P.MGX_ERR_INVALID
    with pytest.raises(ValueError):
        mg.PCG(1, 1, 1e-8, 10, precond="f16")
    mg._mg.contents.residual_mode = P.REF_COMPAT
    with pytest.raises(P.MgxError) as e:
        mg.PCG(1, 1, 1e-8, 10, precond="f32")
    assert e.value.status == P.MGX_ERR_INVALID
    mg.close()
    mg = P.MultiGrid3D(ctx, n3, UNIT, np.float64, residual_mode=P.CORRECT, layout="natural")
    with pytest.raises(P.MgxError) as e:
        mg.PCG(1, 1, 1e-8, 10, precond="f32")
    assert e.value.status == P.MGX_ERR_INVALID
    mg.close()
    mg = P.MultiGrid3D(ctx, n3, UNIT, np.float32, residual_mode=P.CORRECT)
    with pytest.raises(ValueError):
        mg.PCG(1, 1, 1e-5, 10, precond="f32")
    mg.close()
    with pytest.raises(ValueError):
        P.solve3d_pcg(ctx, np.zeros(O.shape(n3), np.float32), None, UNIT, precond="f32")
    with pytest.raises(ValueError):
        P.solve3d_pcg(ctx, np.zeros(O.shape(n3)), None, UNIT, precond="bf16")


@pytest.mark.parametrize("krylov", [False, True])
def test_mixed_breakdown_is_not_success(ctx, krylov):
    n3 = (17, 17, 17)
    f = _problem(n3)
    f[8, 8, 8] = np.nan
    mg = _mg(ctx, n3, UNIT, f=f)
    k, rel, conv, _ = mg.PCG(1, 1, 1e-8, 10, krylov=krylov, precond="f32")
    assert not conv and k <= 1
    assert bits_equal(mg.download_f(0), f)
    mg.close()


C_SOLVE = r"""
#include "mg_multigrid.h"
#include <stdio.h>
#include <string.h>

int main(void) {
    enum { N = 17 };
    static double grid[N * N * N], rhs[N * N * N];
    const int n[3] = {N, N, N};
    const double range[6] = {0, 1, 0, 1, 0, 1};
    for (int z = 1; z < N - 1; z++)
        for (int y = 1; y < N - 1; y++)
            for (int x = 1; x < N - 1; x++) rhs[x + N * (y + N * z)] = (double)((x * 7 + y * 3 + z * 5) % 11) - 5.0;
    mgx_ctx* ctx;
    int iters = 0, converged = 0;
    double rel = 0;
    if (mgx_ctx_create(0, &ctx) ||
        mg3d_solve_pcg_mixed_f64(ctx, grid, rhs, n, range, 0, 2, 2, 1e-10, 50, 1, &iters, &rel, &converged)) {
        fprintf(stderr, "%s\n", mgx_last_error());
        return 1;
    }
    printf("iters %d\nrel %.17g\nconverged %d\n", iters, rel, converged);
    mgx_ctx_destroy(ctx);
    return 0;
}
"""


def test_c_caller_of_the_mixed_solve(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc on this box")
    src, exe = tmp_path / "mixed.c", tmp_path / "mixed"
    src.write_text(C_SOLVE)
    lib = os.path.join(ROOT, "pde_multigrid_amd", "lib")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lmgx",
                           "-Wl,-rpath," + lib, "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = dict(line.split(" ", 1) for line in p.stdout.strip().splitlines())
    assert out["converged"] == "1" and float(out["rel"]) < 1e-10 and 1 <= int(out["iters"]) <= 50, out


# ---------------------------------------------------------------------------------------------------------- scale
def test_mixed_scale_513(ctx):
    n3 = (513, 513, 513)
    mg = P.MultiGrid3D(ctx, n3, UNIT, np.float64, residual_mode=P.CORRECT)  # InitV / InitF: the reference's problem
    res = {}
    for krylov in (True, False):
        for precond in ("f64", "f32"):
            mg.setToValue_v(0, 0.0, True)
            k, rel, conv, _ = mg.PCG(2, 2, 1e-10, 40, krylov=krylov, precond=precond)
            res[krylov, precond] = (k, rel, conv, mg.DiffStats(0))
    mg.close()
    ds_ref = res[True, "f64"][3]
    for krylov in (True, False):
        k64, k32 = res[krylov, "f64"][0], res[krylov, "f32"][0]
        _, rel, conv, ds = res[krylov, "f32"]
        assert conv and rel < 1e-10 and k32 <= k64 + 1, (krylov, k32, k64, rel)
        for a, b in zip(ds, ds_ref):
            assert abs(a - b) <= 1e-4 * abs(b), (krylov, ds, ds_ref)
