"""GPU suite: the shifted operator (Laplacian - s) u = f (csrc/mgx_shift3d.hip), the hierarchy that cycles with it
(MultiGrid3D(shift=s)) and the implicit heat steps built on both (MultiGrid3D.BackwardEuler).

The six kernels are checked bit for bit against the numpy restatement of their arithmetic (tests/op_restated.py), with poisoned
pads; the cycles against the restated cycle, every level, bit for bit, eagerly and through captured graphs; the solver against the
restated iteration counts; the time stepping against the discrete eigenvalue of its initial state."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle as O
import pde_multigrid_amd as P
import semi_restated as S
import op_restated as OP
from conftest import bits_equal
from odd_shapes import pads_unchanged, run_poisoned
from pde_multigrid_amd.multigrid import _ct, _ip, _rp, grid_spacing, xs_unpack
from solve_restated import boundary_mask, close, fsum_dot, interior, problem

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]
UNIT = [0, 1, 0, 1, 0, 1]  # on 2^k + 1 points: the exact-reciprocal form of the residual
DTYPES = [np.float64, np.float32]
# 131 ends inside a tile; the rows of the last four span several waves
SHAPES = [(17, 17, 17), (21, 13, 29), (131, 7, 9), (257, 9, 5), (513, 5, 5), (513, 33, 9)]
SHIFTS = [0.0, 0.75, 1e4]
WORK_GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


def _rand(n3, dtype, seed):
    return np.random.default_rng(seed).uniform(-1, 1, O.shape(n3)).astype(dtype)


def _fn(name, dtype):
    s, ct = _ct(dtype)
    return getattr(P.lib, "mgx3dxs_%s_%s" % (name, s)), ct


def _h(n3, rng, dtype):
    return _rp(grid_spacing(n3, rng, dtype), _ct(dtype)[1])


class Work:
    """the reduction scratch of a call (mgx3dxs_krylov_work_elems doubles, NaN guards behind them) and its device sum"""

    def __init__(self, ctx, n3, dtype):
        fn = getattr(P.lib, "mgx3dxs_krylov_work_elems_" + _ct(dtype)[0])
        fn.restype = C.c_size_t
        self.ctx, self.elems = ctx, int(fn(_ip(n3)))
        host = np.zeros(self.elems + WORK_GUARD)
        host[self.elems:] = np.nan
        self.work, self.sum = ctx.to_device(host), ctx.to_device(np.full(1, np.nan))

    def result(self):
        tail = self.ctx.to_host(C.c_void_p(self.work.value + 8 * self.elems), (WORK_GUARD,), np.float64)
        assert np.isnan(tail).all(), "the work array was overrun"
        return float(self.ctx.to_host(self.sum, (1,), np.float64)[0])

    def close(self):
        self.ctx.free(self.work)
        self.ctx.free(self.sum)


# ---------------------------------------------------------------------------------------------------------- operators
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", SHIFTS)
@pytest.mark.parametrize("sweeps", [1, 3])
@pytest.mark.parametrize("n3", SHAPES)
def test_relax_shift(ctx, n3, sweeps, s, dtype):
    v, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    fn, ct = _fn("relax_shift", dtype)
    ups, outs = run_poisoned(ctx, [v, f], lambda a, b: fn(ctx._h, a, b, _ip(n3), _h(n3, RG, dtype), ct(s), C.c_int(sweeps)), dtype)
    assert ctx.last_relax_kernel().startswith("relax_shift3d_xs_kernel"), ctx.last_relax_kernel()
    want = OP.Op(n3, RG, dtype, s).relax(v, f, sweeps)
    got = xs_unpack(outs[0], n3[0])
    assert bits_equal(got, want), np.argwhere(got != want)[:5]  # the interior, and the boundary as it was
    assert pads_unchanged(ups[0], outs[0], n3[0]) and bits_equal(outs[1], ups[1])
    if s == 0:
        assert bits_equal(want, P.ops3dxs.relax(ctx, v, f, n3, RG, sweeps))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", SHIFTS)
@pytest.mark.parametrize("n3", SHAPES)
def test_relax_shift_from_zero(ctx, n3, s, dtype):
    v, f = _rand(n3, dtype, 3), _rand(n3, dtype, 4)
    f[1:-1:2, 1:-1, 1:-1] = 0  # zero right-hand sides too: the signs of the zeros the first pass stores
    fn, ct = _fn("relax_shift_from_zero", dtype)
    for sweeps in (1, 2):
        want = OP.Op(n3, RG, dtype, s).relax(np.zeros_like(v), f, sweeps)
        for rim_is_zero in (0, 1):
            v0 = v.copy()
            if rim_is_zero:  # the caller vouches for a zero boundary; the interior is stale
                v0[boundary_mask(n3)] = 0
            ups, outs = run_poisoned(ctx, [v0, f], lambda a, b: fn(ctx._h, a, b, _ip(n3), _h(n3, RG, dtype), ct(s), C.c_int(sweeps),
                                                                   C.c_int(rim_is_zero)), dtype)
            assert bits_equal(xs_unpack(outs[0], n3[0]), want), (sweeps, rim_is_zero)
            assert pads_unchanged(ups[0], outs[0], n3[0], zero_ok=not rim_is_zero) and bits_equal(outs[1], ups[1])
    assert ctx.last_relax_kernel().startswith("relax_shift3d_xs_kernel")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", SHIFTS)
@pytest.mark.parametrize("rg", ["aniso", "unit"])
@pytest.mark.parametrize("n3", SHAPES)
def test_residual_shift(ctx, n3, rg, s, dtype):
    rng = RG if rg == "aniso" else UNIT
    v, f, r0 = _rand(n3, dtype, 5), _rand(n3, dtype, 6), _rand(n3, dtype, 7)
    fn, ct = _fn("residual_shift", dtype)
    want = OP.Op(n3, rng, dtype, s).residual(v, f)
    want_ss = OP.fsum_sq(want)
    w = Work(ctx, n3, dtype)
    try:
        sums = []
        for rep in range(2):
            ups, outs = run_poisoned(ctx, [v, f, r0], lambda a, b, c: fn(ctx._h, a, b, c, _ip(n3), _h(n3, rng, dtype), ct(s), w.work, w.sum), dtype)
            assert bits_equal(xs_unpack(outs[2], n3[0]), want)  # the boundary written as 0
            assert bits_equal(outs[0], ups[0]) and bits_equal(outs[1], ups[1]) and pads_unchanged(ups[2], outs[2], n3[0])
            sums.append(w.result())
        assert sums[0] == sums[1], "two runs gave different sums"
        assert close(sums[0], want_ss, 1e-13), (sums[0], want_ss)
        # the sum alone (r = NULL), and r alone (no sum, no work array)
        ups, outs = run_poisoned(ctx, [v, f], lambda a, b: fn(ctx._h, a, b, None, _ip(n3), _h(n3, rng, dtype), ct(s), w.work, w.sum), dtype)
        assert w.result() == sums[0] and bits_equal(outs[0], ups[0]) and bits_equal(outs[1], ups[1])
        ups, outs = run_poisoned(ctx, [v, f, r0], lambda a, b, c: fn(ctx._h, a, b, c, _ip(n3), _h(n3, rng, dtype), ct(s), None, None), dtype)
        assert bits_equal(xs_unpack(outs[2], n3[0]), want) and pads_unchanged(ups[2], outs[2], n3[0])
    finally:
        w.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", SHIFTS)
@pytest.mark.parametrize("rg", ["aniso", "unit"])
@pytest.mark.parametrize("n3", SHAPES)
def test_laplace_dot_shift(ctx, n3, rg, s, dtype):
    rng = RG if rg == "aniso" else UNIT
    p, q0 = _rand(n3, dtype, 8), _rand(n3, dtype, 9)
    fn, ct = _fn("laplace_dot_shift", dtype)
    rfn, _ = _fn("residual_shift", dtype)
    want = OP.Op(n3, rng, dtype, s).apply_A(p)
    w = Work(ctx, n3, dtype)
    try:
        sums = []
        for rep in range(2):
            ups, outs = run_poisoned(ctx, [p, q0], lambda a, b: fn(ctx._h, a, b, _ip(n3), _h(n3, rng, dtype), ct(s), w.work, w.sum), dtype)
            q = xs_unpack(outs[1], n3[0])
            assert bits_equal(interior(q), interior(want))
            assert bits_equal(q[boundary_mask(n3)], q0[boundary_mask(n3)]), "a boundary entry of q was written"
            assert bits_equal(outs[0], ups[0]) and pads_unchanged(ups[1], outs[1], n3[0])
            sums.append(w.result())
        assert sums[0] == sums[1], "two runs gave different sums"
        assert close(sums[0], fsum_dot(p, want), 1e-13), (sums[0], fsum_dot(p, want))
        # q = -residual_shift(p, f = 0), the library's own
        _, outs = run_poisoned(ctx, [p, np.zeros_like(p), q0], lambda a, b, c: rfn(ctx._h, a, b, c, _ip(n3), _h(n3, rng, dtype), ct(s), None, None),
                               dtype)
        assert bits_equal(interior(q), interior(-xs_unpack(outs[2], n3[0])))
    finally:
        w.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", SHIFTS)
@pytest.mark.parametrize("n3", SHAPES)
def test_shift_rhs(ctx, n3, s, dtype):
    u, q, f0 = _rand(n3, dtype, 10), _rand(n3, dtype, 11), _rand(n3, dtype, 12)
    fn, ct = _fn("shift_rhs", dtype)
    rim = boundary_mask(n3)
    ups, outs = run_poisoned(ctx, [u, q, f0], lambda a, b, c: fn(ctx._h, a, b, ct(0.3), ct(s), c, _ip(n3)), dtype)
    got = xs_unpack(outs[2], n3[0])
    assert bits_equal(interior(got), interior(OP.Op(n3, UNIT, dtype, s).rhs(u, q, 0.3))) and bits_equal(got[rim], f0[rim])
    assert bits_equal(outs[0], ups[0]) and bits_equal(outs[1], ups[1]) and pads_unchanged(ups[2], outs[2], n3[0])
    ups, outs = run_poisoned(ctx, [u, f0], lambda a, c: fn(ctx._h, a, None, ct(0.3), ct(s), c, _ip(n3)), dtype)
    got = xs_unpack(outs[1], n3[0])
    assert bits_equal(interior(got), interior(OP.Op(n3, UNIT, dtype, s).rhs(u, None, 0.3))) and bits_equal(got[rim], f0[rim])
    assert bits_equal(outs[0], ups[0]) and pads_unchanged(ups[1], outs[1], n3[0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", SHIFTS)
@pytest.mark.parametrize("mask", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("rg", ["aniso", "unit"])
@pytest.mark.parametrize("n3", SHAPES)
def test_residual_restrict_shift(ctx, n3, rg, mask, s, dtype):
    rng = RG if rg == "aniso" else UNIT
    cn = S.coarse_size(n3, mask)
    v, f, c0 = _rand(n3, dtype, 13), _rand(n3, dtype, 14), _rand(cn, dtype, 15)
    fn, ct = _fn("residual_restrict_shift", dtype)
    want = OP.restrict(n3, OP.Op(n3, rng, dtype, s).residual(v, f), 0, dtype, mask)
    rim = boundary_mask(cn)
    assert not want[rim].any()
    for keep in (0, 1):
        ups, outs = run_poisoned(ctx, [v, f, c0], lambda a, b, c: fn(ctx._h, a, b, _ip(n3), _h(n3, rng, dtype), ct(s), c, _ip(cn), C.c_int(keep)),
                                 dtype)
        got = xs_unpack(outs[2], cn[0])
        assert bits_equal(interior(got), interior(want)), (keep, np.argwhere(interior(got) != interior(want))[:5])
        assert bits_equal(got[rim], c0[rim] if keep else np.zeros_like(c0)[rim]), keep  # left alone, or written as 0
        assert bits_equal(outs[0], ups[0]) and bits_equal(outs[1], ups[1]) and pads_unchanged(ups[2], outs[2], cn[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernels_reject_bad_shifts_and_sizes(ctx, dtype):
    n3 = (17, 9, 9)
    a = _rand(n3, dtype, 1)
    cn = S.coarse_size(n3, 7)
    for s in (-1.0, float("nan"), float("inf")):
        calls = [lambda: P.ops3dxs.relax_shift(ctx, a, a, n3, RG, s, 1), lambda: P.ops3dxs.relax_shift_from_zero(ctx, a, a, n3, RG, s, 1, False),
                 lambda: P.ops3dxs.residual_shift(ctx, a, a, n3, RG, s), lambda: P.ops3dxs.laplace_dot_shift(ctx, a, n3, RG, s),
                 lambda: P.ops3dxs.residual_restrict_shift(ctx, a, a, n3, RG, s, cn), lambda: P.ops3dxs.shift_rhs(ctx, a, a, 1.0, s, n3)]
        for call in calls:
            with pytest.raises(P.MgxError) as e:
                call()
            assert e.value.status == P.MGX_ERR_INVALID
    bad = (16, 9, 9)
    b = np.zeros(O.shape(bad), dtype)
    for call in (lambda: P.ops3dxs.relax_shift(ctx, b, b, bad, RG, 1.0, 1), lambda: P.ops3dxs.shift_rhs(ctx, b, b, 1.0, 1.0, bad),
                 lambda: P.ops3dxs.residual_restrict_shift(ctx, a, a, n3, RG, 1.0, (9, 9, 4))):
        with pytest.raises(P.MgxError) as e:
            call()
        assert e.value.status == P.MGX_ERR_SIZE


# ---------------------------------------------------------------------------------------------------------- hierarchy
GRIDS = [((33, 33, 33), UNIT, "full"), ((65, 33, 17), RG, "full"), (S.TABLE[0][0], S.TABLE[0][1], "semi")]
SHIFT = 0.75


def _mg(ctx, grid, dtype, s=SHIFT, v=None, f=None):
    n3, rng, how = GRIDS[grid]
    mg = P.MultiGrid3D(ctx, n3, rng, dtype, residual_mode=P.CORRECT, coarsening=how, shift=s)
    if v is not None:
        mg.upload_v(0, v)
    if f is not None:
        mg.upload_f(0, f)
    return mg


def _restated(grid, dtype, s, v, f):
    n3, rng, how = GRIDS[grid]
    H = OP.Hierarchy(OP.Op(n3, rng, dtype, s), how)
    H.v[0], H.f[0] = v.copy(), f.copy()
    return H


def _same_levels(mg, H, what):
    assert mg.maxGrids == len(H.sizes) and mg.masks == H.masks
    for l, n in enumerate(H.sizes):
        assert mg.size(l) == n
        assert bits_equal(mg.download_v(l), H.v[l]), (what, "v", l)
        if l > 0:
            assert bits_equal(mg.download_f(l), H.f[l]), (what, "f", l)


@pytest.fixture(scope="module")
def cycled():
    """the restated hierarchies after one and after two V(2,2) cycles, computed once per (grid, dtype, shift)"""
    import copy
    cache = {}

    def get(grid, dtype, s):
        key = (grid, np.dtype(dtype).name, s)
        if key not in cache:
            n3 = GRIDS[grid][0]
            H = _restated(grid, dtype, s, _rand(n3, dtype, 1), _rand(n3, dtype, 2))
            H.vcycle(0, 2, 2)
            first = copy.deepcopy(H)
            H.vcycle(0, 2, 2)
            cache[key] = (first, H)
        return cache[key]
    return get


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("grid", range(len(GRIDS)))
def test_vcycle_matches_restated_cycle(ctx, cycled, grid, dtype):
    n3 = GRIDS[grid][0]
    first, second = cycled(grid, dtype, SHIFT)
    mg = _mg(ctx, grid, dtype, v=_rand(n3, dtype, 1), f=_rand(n3, dtype, 2))
    assert mg.shift == SHIFT
    mg.VCycle(0, 2, 2)
    assert ctx.last_relax_kernel().startswith("relax_shift3d_xs_kernel")
    _same_levels(mg, first, "eager")
    mg.VCycle(0, 2, 2)  # starts from other rim flags (the coarse f's boundary is known to be zero now)
    _same_levels(mg, second, "second")
    mg.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("grid", range(len(GRIDS)))
def test_fmg_matches_restated_cycle(ctx, grid, dtype):
    n3 = GRIDS[grid][0]
    v, f = _rand(n3, dtype, 5), _rand(n3, dtype, 6)
    H = _restated(grid, dtype, SHIFT, v, f)
    H.fmg(0, 1, 2, 2)
    mg = _mg(ctx, grid, dtype, v=v, f=f)
    mg.FullMultiGridVCycle(0, 1, 2, 2)
    _same_levels(mg, H, "fmg")
    mg.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("grid", range(len(GRIDS)))
def test_graph_replay_and_recapture_on_a_new_shift(ctx, cycled, grid, dtype):
    n3 = GRIDS[grid][0]
    v, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    mg = _mg(ctx, grid, dtype, v=v, f=f)
    mg.use_graph = True
    execs = []
    for rep in range(4):  # capture; capture under the rim flags the first cycle left; replay; replay
        mg.upload_v(0, v)
        mg.VCycle(0, 2, 2)
        _same_levels(mg, cycled(grid, dtype, SHIFT)[0], rep)
        execs.append(mg._mg.contents.graph_exec[0])
    assert execs[2] and execs[3] == execs[2], "the last cycle was captured again instead of replayed"
    rec = bytes(mg._mg.contents.graph_rec[0])
    mg.shift = 100.0  # the shift's bits are part of the record: the next cycle is captured again
    mg.upload_v(0, v)
    mg.VCycle(0, 2, 2)
    assert bytes(mg._mg.contents.graph_rec[0]) != rec, "the record does not hold the shift"
    _same_levels(mg, cycled(grid, dtype, 100.0)[0], "new shift")
    mg.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_relax_residual_and_norm_through_the_hierarchy(ctx, dtype):
    n3, rng, _ = GRIDS[1]
    v, f = _rand(n3, dtype, 7), _rand(n3, dtype, 8)
    mg = _mg(ctx, 1, dtype, v=v, f=f)
    mg.Relax(0, 3)
    want = OP.Op(n3, rng, dtype, SHIFT).relax(v, f, 3)
    assert bits_equal(mg.download_v(0), want)
    r = OP.Op(n3, rng, dtype, SHIFT).residual(want, f)
    assert bits_equal(mg.CalculateResidual(0), r)
    assert close(mg.ResidualNorm(0), math.sqrt(OP.fsum_sq(r)), 1e-12)
    mg.shift = 0.0  # and back on the unshifted operators
    mg.upload_v(0, v)
    mg.Relax(0, 3)
    assert bits_equal(mg.download_v(0), O.relax3d(n3, rng, v, f, 3, dtype=dtype))
    mg.close()


@pytest.mark.parametrize("krylov", [True, False])
def test_pcg_matches_restatement(ctx, krylov):
    n3, s, tol = (33, 33, 33), 100.0, 1e-10
    f = problem(n3)
    v0 = np.zeros_like(f)
    v0[boundary_mask(n3)] = _rand(n3, np.float64, 9)[boundary_mask(n3)]  # Dirichlet data
    if krylov:
        want_x, want_k, _, want_c = OP.fcg(OP.Op(n3, UNIT, np.float64, s), v0, f, tol=tol, maxit=100)[:4]
    else:
        want_x, want_k, _, want_c = OP.cycles_to(OP.Op(n3, UNIT, np.float64, s), v0, f, 2, 2, tol, 100)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, shift=s)
    mg.upload_v(0, v0)
    mg.upload_f(0, f)
    k, rel, conv, hist = mg.PCG(2, 2, tol, 100, krylov=krylov)
    x = mg.download_v(0)
    assert bits_equal(mg.download_f(0), f), "d_f[0] was not restored"
    mg.close()
    r, r0 = OP.Op(n3, UNIT, np.float64, s).residual(x, f), OP.Op(n3, UNIT, np.float64, s).residual(v0, f)
    true_rel = math.sqrt(OP.fsum_sq(r) / OP.fsum_sq(r0))
    print("shifted PCG krylov=%s: %d iterations (restated %d), rel %.3e, restated residual of the result %.3e" % (krylov, k, want_k, rel, true_rel))
    assert k == want_k and conv == want_c and conv
    assert rel < tol and true_rel < tol and close(rel, true_rel, 1e-6)
    assert bits_equal(x[boundary_mask(n3)], v0[boundary_mask(n3)]), "the boundary was changed"
    assert np.abs(x - want_x).max() <= 1e-9 * np.abs(want_x).max()
    x2, k2, rel2, conv2 = P.solve3d_pcg(ctx, v0, f, UNIT, tol=tol, krylov=krylov, shift=s)
    assert (k2, conv2) == (k, conv) and bits_equal(x2, x)


# ---------------------------------------------------------------------------------------------------------- rejections
def test_bad_shifts_and_settings_are_rejected(ctx):
    n3 = (17, 17, 17)
    for s in (-0.5, float("nan"), float("inf")):
        with pytest.raises(P.MgxError) as e:
            P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, shift=s)
        assert e.value.status == P.MGX_ERR_INVALID
    with pytest.raises(P.MgxError) as e:
        P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, layout="natural", shift=1.0)
    assert e.value.status == P.MGX_ERR_INVALID and "layout" in str(e.value)
    with pytest.raises(P.MgxError) as e:
        P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.REF_COMPAT, shift=1.0)
    assert e.value.status == P.MGX_ERR_INVALID and "CORRECT" in str(e.value)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT)
    mg.set_smoother("jacobi")
    with pytest.raises(P.MgxError) as e:
        mg.shift = 1.0
    assert e.value.status == P.MGX_ERR_INVALID and "smoother" in str(e.value) and mg.shift == 0.0
    mg.set_smoother("rbgs")
    mg.shift = 1.0
    # the members are public: a setting changed after the shift is caught where the shift is used
    mg.set_smoother("jacobi")
    for call in (lambda: mg.VCycle(0, 2, 2), lambda: mg.Relax(0, 1), lambda: mg.ResidualNorm(0), lambda: mg.PCG(2, 2, 1e-8, 5),
                 lambda: mg.FullMultiGridVCycle(0, 1, 2, 2)):
        with pytest.raises(P.MgxError) as e:
            call()
        assert e.value.status == P.MGX_ERR_INVALID
    mg.set_smoother("rbgs")
    mg.VCycle(0, 2, 2)
    with pytest.raises(P.MgxError) as e:
        mg.PCG(2, 2, 1e-8, 5, precond="f32")
    assert e.value.status == P.MGX_ERR_INVALID and "shift" in str(e.value)
    mg.close()


# ---------------------------------------------------------------------------------------------------------- backward Euler
EULER_N = (33, 17, 17)


def _mode(n3):
    ax = [np.sin(np.pi * np.linspace(0.0, 1.0, k)) for k in n3]
    u = ax[2][:, None, None] * ax[1][None, :, None] * ax[0][None, None, :]
    u[boundary_mask(n3)] = 0.0
    return u


@pytest.mark.parametrize("kappa,dt", [(1.0, 1e-2), (0.5, 1e-4)])
def test_backward_euler_damps_the_discrete_eigenvector(ctx, kappa, dt):
    """u0 = sin(pi x) sin(pi y) sin(pi z) is an eigenvector of the discrete Laplacian with eigenvalue -lam, lam = sum_d (4 / h_d^2)
    sin^2(pi h_d / 2), so five steps give u0 / (1 + kappa dt lam)^5.  Every step stops at tol relative to its initial residual
    lam ||u||, i.e. within tol kappa dt lam (relative) of its exact result; ten times the sum over the steps bounds the error."""
    n3, steps, tol = EULER_N, 5, 1e-10
    u0 = _mode(n3)
    lam = sum(4.0 / (1.0 / (k - 1)) ** 2 * math.sin(math.pi / (k - 1) / 2) ** 2 for k in n3)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT)
    mg.upload_v(0, u0)
    its, worst, conv = mg.BackwardEuler(steps, dt, kappa, tol=tol)
    u = mg.download_v(0)
    assert mg.shift == 1.0 / (kappa * dt), "the shift of the steps stays set"
    mg.close()
    want = u0 / (1.0 + kappa * dt * lam) ** steps
    err = np.linalg.norm((u - want).ravel()) / np.linalg.norm(want.ravel())
    bound = 10 * steps * tol * max(1.0, kappa * dt * lam)
    print("backward Euler kappa %g dt %g: %d iterations, worst residual %.3e, relative L2 error %.3e (bound %.1e)" % (kappa, dt, its, worst, err, bound))
    assert conv and worst < tol and its >= 1
    assert err <= bound, (err, bound)
    assert not u[boundary_mask(n3)].any()


def test_backward_euler_step_with_a_source(ctx):
    n3, kappa, dt, tol = EULER_N, 0.7, 3e-3, 1e-10
    s = 1.0 / (kappa * dt)
    u0, q = _rand(n3, np.float64, 20), _rand(n3, np.float64, 21)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT)
    mg.upload_v(0, u0)
    its, worst, conv = mg.BackwardEuler(1, dt, kappa, source=q, tol=tol)
    u = mg.download_v(0)
    rhs_dev = mg.download_f(0)
    mg.close()
    f = OP.Op(n3, UNIT, np.float64, s).rhs(u0, q, 1.0 / kappa)
    assert bits_equal(interior(rhs_dev), interior(f)), "d_f[0] is not the step's right-hand side"
    rel = math.sqrt(OP.fsum_sq(OP.Op(n3, UNIT, np.float64, s).residual(u, f)) / OP.fsum_sq(OP.Op(n3, UNIT, np.float64, s).residual(u0, f)))
    print("backward Euler with a source: %d iterations, residual %.3e (restated %.3e)" % (its, worst, rel))
    assert conv and worst < tol and rel < tol
    assert bits_equal(u[boundary_mask(n3)], u0[boundary_mask(n3)]), "the Dirichlet data changed"
    # nothing to do, and a step that cannot converge
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT)
    mg.upload_v(0, u0)
    assert mg.BackwardEuler(0, dt, kappa) == (0, 0.0, True) and bits_equal(mg.download_v(0), u0)
    its, worst, conv = mg.BackwardEuler(3, dt, kappa, tol=1e-30, maxit=2)
    assert not conv and its == 2, "it did not stop at the first step that failed"
    for bad in ((1, -1.0, 1.0), (1, 1.0, 0.0), (-1, 1.0, 1.0)):
        with pytest.raises(P.MgxError) as e:
            mg.BackwardEuler(*bad)
        assert e.value.status == P.MGX_ERR_INVALID
    mg.close()
