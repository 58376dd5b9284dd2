"""GPU suite: the variable-coefficient operator div(a grad u) - s u = f (csrc/mgx_coef3d.hip), the hierarchy that cycles with it
(MultiGrid3D(coefficient=a), set_coefficient) and the solves and implicit heat steps on it.

The four kernels are checked bit for bit against the numpy restatement of their arithmetic (tests/op_restated.py), with poisoned
pads; the coefficient of every level against the restated restriction chain; the cycles against the restated cycle, every level,
bit for bit, eagerly and through captured graphs; the solver against the restated iteration counts; the time stepping against a
constant-coefficient hierarchy and against each step's own linear system."""
import ctypes as C
import copy
import math

import numpy as np
import pytest

import op_cases as OC
import op_restated as OP
import oracle as O
import pde_multigrid_amd as P
import semi_restated as S
from conftest import bits_equal
from odd_shapes import pads_unchanged, run_poisoned
from pde_multigrid_amd.multigrid import _ct, _ip, _rp, grid_spacing, xs_unpack
from solve_restated import boundary_mask, close, fsum_dot, interior, problem

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]
UNIT = [0, 1, 0, 1, 0, 1]
RANGES = {"aniso": RG, "unit": UNIT}
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


def _coef(n3, dtype, seed=100):
    """uniform in [0.5, 2] on all points, the boundary included"""
    return np.random.default_rng(seed).uniform(0.5, 2, O.shape(n3)).astype(dtype)


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
@pytest.mark.parametrize("rg", ["aniso", "unit"])
@pytest.mark.parametrize("sweeps", [1, 3])
@pytest.mark.parametrize("n3", SHAPES)
def test_relax_coef(ctx, n3, sweeps, rg, s, dtype):
    rng = RANGES[rg]
    v, f, a = _rand(n3, dtype, 1), _rand(n3, dtype, 2), _coef(n3, dtype)
    fn, ct = _fn("relax_coef", dtype)
    ups, outs = run_poisoned(ctx, [v, f, a], lambda x, b, c: fn(ctx._h, x, b, c, _ip(n3), _h(n3, rng, dtype), ct(s), C.c_int(sweeps)), dtype)
    assert ctx.last_relax_kernel().startswith("relax_coef3d_xs_kernel"), ctx.last_relax_kernel()
    want = OP.Op(n3, rng, dtype, s, a).relax(v, f, sweeps)
    got = xs_unpack(outs[0], n3[0])
    assert bits_equal(got, want), np.argwhere(got != want)[:5]  # the interior, and the boundary as it was
    assert pads_unchanged(ups[0], outs[0], n3[0]) and bits_equal(outs[1], ups[1]) and bits_equal(outs[2], ups[2])
    assert bits_equal(want, P.ops3dxs.relax_coef(ctx, v, f, a, n3, rng, s, sweeps))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", SHIFTS)
@pytest.mark.parametrize("rg", ["aniso", "unit"])
@pytest.mark.parametrize("n3", SHAPES)
def test_relax_coef_from_zero(ctx, n3, rg, s, dtype):
    rng = RANGES[rg]
    v, f, a = _rand(n3, dtype, 3), _rand(n3, dtype, 4), _coef(n3, dtype)
    f[1:-1:2, 1:-1, 1:-1] = 0  # zero right-hand sides too: the signs of the zeros the first pass stores
    fn, ct = _fn("relax_coef_from_zero", dtype)
    for sweeps in (1, 2):
        want = OP.Op(n3, rng, dtype, s, a).relax(np.zeros_like(v), f, sweeps)
        for rim_is_zero in (0, 1):
            v0 = v.copy()
            if rim_is_zero:  # the caller vouches for a zero boundary; the interior is stale
                v0[boundary_mask(n3)] = 0
            ups, outs = run_poisoned(ctx, [v0, f, a], lambda x, b, c: fn(ctx._h, x, b, c, _ip(n3), _h(n3, rng, dtype), ct(s), C.c_int(sweeps),
                                                                         C.c_int(rim_is_zero)), dtype)
            assert bits_equal(xs_unpack(outs[0], n3[0]), want), (sweeps, rim_is_zero)
            assert pads_unchanged(ups[0], outs[0], n3[0], zero_ok=not rim_is_zero)
            assert bits_equal(outs[1], ups[1]) and bits_equal(outs[2], ups[2])
    assert ctx.last_relax_kernel().startswith("relax_coef3d_xs_kernel")
    assert bits_equal(want, P.ops3dxs.relax_coef_from_zero(ctx, v, f, a, n3, rng, s, 2, False))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", SHIFTS)
@pytest.mark.parametrize("rg", ["aniso", "unit"])
@pytest.mark.parametrize("n3", SHAPES)
def test_residual_coef(ctx, n3, rg, s, dtype):
    rng = RANGES[rg]
    v, f, a, r0 = _rand(n3, dtype, 5), _rand(n3, dtype, 6), _coef(n3, dtype), _rand(n3, dtype, 7)
    fn, ct = _fn("residual_coef", dtype)
    want = OP.Op(n3, rng, dtype, s, a).residual(v, f)
    want_ss = OP.fsum_sq(want)
    w = Work(ctx, n3, dtype)
    try:
        sums = []
        for rep in range(2):
            ups, outs = run_poisoned(ctx, [v, f, a, r0],
                                     lambda x, b, c, d: fn(ctx._h, x, b, c, d, _ip(n3), _h(n3, rng, dtype), ct(s), w.work, w.sum), dtype)
            assert bits_equal(xs_unpack(outs[3], n3[0]), want)  # the boundary written as 0
            assert all(bits_equal(outs[i], ups[i]) for i in range(3)) and pads_unchanged(ups[3], outs[3], n3[0])
            sums.append(w.result())
        assert sums[0] == sums[1], "two runs gave different sums"
        assert close(sums[0], want_ss, 1e-13), (sums[0], want_ss)
        # the sum alone (r = NULL), and r alone (no sum, no work array)
        ups, outs = run_poisoned(ctx, [v, f, a], lambda x, b, c: fn(ctx._h, x, b, c, None, _ip(n3), _h(n3, rng, dtype), ct(s), w.work, w.sum), dtype)
        assert w.result() == sums[0] and all(bits_equal(outs[i], ups[i]) for i in range(3))
        ups, outs = run_poisoned(ctx, [v, f, a, r0], lambda x, b, c, d: fn(ctx._h, x, b, c, d, _ip(n3), _h(n3, rng, dtype), ct(s), None, None), dtype)
        assert bits_equal(xs_unpack(outs[3], n3[0]), want) and pads_unchanged(ups[3], outs[3], n3[0])
    finally:
        w.close()
    r, ss = P.ops3dxs.residual_coef(ctx, v, f, a, n3, rng, s)
    assert bits_equal(r, want) and ss == sums[0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", SHIFTS)
@pytest.mark.parametrize("rg", ["aniso", "unit"])
@pytest.mark.parametrize("n3", SHAPES)
def test_apply_coef_dot(ctx, n3, rg, s, dtype):
    rng = RANGES[rg]
    p, a, q0 = _rand(n3, dtype, 8), _coef(n3, dtype), _rand(n3, dtype, 9)
    fn, ct = _fn("apply_coef_dot", dtype)
    want = OP.Op(n3, rng, dtype, s, a).apply_A(p)
    w = Work(ctx, n3, dtype)
    try:
        sums = []
        for rep in range(2):
            ups, outs = run_poisoned(ctx, [p, a, q0], lambda x, c, b: fn(ctx._h, x, c, b, _ip(n3), _h(n3, rng, dtype), ct(s), w.work, w.sum), dtype)
            q = xs_unpack(outs[2], n3[0])
            assert bits_equal(interior(q), interior(want))
            assert bits_equal(q[boundary_mask(n3)], q0[boundary_mask(n3)]), "a boundary entry of q was written"
            assert bits_equal(outs[0], ups[0]) and bits_equal(outs[1], ups[1]) and pads_unchanged(ups[2], outs[2], n3[0])
            sums.append(w.result())
        assert sums[0] == sums[1], "two runs gave different sums"
        assert close(sums[0], fsum_dot(p, want), 1e-13), (sums[0], fsum_dot(p, want))
    finally:
        w.close()
    q, pq = P.ops3dxs.apply_coef_dot(ctx, p, a, n3, rng, s)
    assert bits_equal(interior(q), interior(want)) and pq == sums[0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", [(21, 13, 29), (131, 7, 9), (513, 33, 9)])
def test_relax_rows_knob_lowers_the_coefficient_pass_only(ctx, n3, dtype):
    """"relax3d.rows" below 4 lowers the rows per lane of the coefficient's colour pass (same bits) and is not read by the shifted
    one.  The pass then halves its rows while four waves of them exceed the level's interior rows, as with the default: 11
    interior rows take at most 2 rows per lane, 5 take 1, and only the 31 of the last shape take every value as set."""
    s, rng = 0.75, RG
    v, f, a = _rand(n3, dtype, 1), _rand(n3, dtype, 2), _coef(n3, dtype)
    coef, ct = _fn("relax_coef", dtype)
    shift, _ = _fn("relax_shift", dtype)
    want, want_shift = OP.Op(n3, rng, dtype, s, a).relax(v, f, 1), OP.Op(n3, rng, dtype, s).relax(v, f, 1)
    ups, outs = run_poisoned(ctx, [v, f], lambda x, b: shift(ctx._h, x, b, _ip(n3), _h(n3, rng, dtype), ct(s), C.c_int(1)), dtype)
    default_shift = ctx.last_relax_kernel()
    assert default_shift.startswith("relax_shift3d_xs_kernel") and bits_equal(xs_unpack(outs[0], n3[0]), want_shift)
    try:
        for knob in (1, 2):
            ctx.set_param("relax3d.rows", knob)
            rows = knob
            while rows > 1 and 4 * rows > n3[1] - 2:
                rows //= 2
            ups, outs = run_poisoned(ctx, [v, f, a], lambda x, b, c: coef(ctx._h, x, b, c, _ip(n3), _h(n3, rng, dtype), ct(s), C.c_int(1)), dtype)
            name = ctx.last_relax_kernel()
            assert name.startswith("relax_coef3d_xs_kernel") and int(name.rstrip(">").split(",")[2]) == rows, (knob, rows, name)
            assert bits_equal(xs_unpack(outs[0], n3[0]), want), knob
            assert pads_unchanged(ups[0], outs[0], n3[0]) and bits_equal(outs[1], ups[1]) and bits_equal(outs[2], ups[2])
            ups, outs = run_poisoned(ctx, [v, f], lambda x, b: shift(ctx._h, x, b, _ip(n3), _h(n3, rng, dtype), ct(s), C.c_int(1)), dtype)
            assert ctx.last_relax_kernel() == default_shift, (knob, ctx.last_relax_kernel(), default_shift)
            assert bits_equal(xs_unpack(outs[0], n3[0]), want_shift), knob
    finally:
        ctx.set_param("relax3d.rows", 4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernels_reject_bad_shifts_and_sizes(ctx, dtype):
    n3 = (17, 9, 9)
    a = _coef(n3, dtype)
    for s in (-1.0, float("nan"), float("inf")):
        calls = [lambda: P.ops3dxs.relax_coef(ctx, a, a, a, n3, RG, s, 1), lambda: P.ops3dxs.relax_coef_from_zero(ctx, a, a, a, n3, RG, s, 1, False),
                 lambda: P.ops3dxs.residual_coef(ctx, a, a, a, n3, RG, s), lambda: P.ops3dxs.apply_coef_dot(ctx, a, a, n3, RG, s)]
        for call in calls:
            with pytest.raises(P.MgxError) as e:
                call()
            assert e.value.status == P.MGX_ERR_INVALID
    bad = (16, 9, 9)
    b = np.ones(O.shape(bad), dtype)
    for call in (lambda: P.ops3dxs.relax_coef(ctx, b, b, b, bad, RG, 1.0, 1), lambda: P.ops3dxs.residual_coef(ctx, b, b, b, bad, RG, 1.0),
                 lambda: P.ops3dxs.apply_coef_dot(ctx, b, b, bad, RG, 1.0)):
        with pytest.raises(P.MgxError) as e:
            call()
        assert e.value.status == P.MGX_ERR_SIZE


# ---------------------------------------------------------------------------------------------------------- hierarchy
GRIDS = [((33, 33, 33), UNIT, "full"), ((65, 33, 17), RG, "full"), (S.TABLE[0][0], S.TABLE[0][1], "semi")]
CYCLE_SHIFTS = [0.0, 100.0]


def _mg(ctx, grid, dtype, s, a, v=None, f=None):
    n3, rng, how = GRIDS[grid]
    mg = P.MultiGrid3D(ctx, n3, rng, dtype, residual_mode=P.CORRECT, coarsening=how, shift=s, coefficient=a)
    if v is not None:
        mg.upload_v(0, v)
    if f is not None:
        mg.upload_f(0, f)
    return mg


def _restated(grid, dtype, s, a, v, f):
    n3, rng, how = GRIDS[grid]
    H = OP.Hierarchy(OP.Op(n3, rng, dtype, s, a), how)
    H.v[0], H.f[0] = v.copy(), f.copy()
    return H


def _same_levels(mg, H, what):
    assert mg.maxGrids == len(H.sizes) and mg.masks == H.masks
    for l, n in enumerate(H.sizes):
        assert mg.size(l) == n
        assert bits_equal(mg.download_v(l), H.v[l]), (what, "v", l)
        if l > 0:
            assert bits_equal(mg.download_f(l), H.f[l]), (what, "f", l)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("grid", [0, 2])
def test_set_coefficient_restricts_down_the_levels(ctx, grid, dtype):
    n3, rng, how = GRIDS[grid]
    a = _coef(n3, dtype)
    mg = P.MultiGrid3D(ctx, n3, rng, dtype, residual_mode=P.CORRECT, coarsening=how)
    assert not mg.has_coefficient
    mg.set_coefficient(a)
    assert mg.has_coefficient
    sizes, masks = S.plan(n3, rng) if how == "semi" else OP.full_plan(n3)
    assert mg.masks == masks
    ptrs = [mg.grid(l).d_a for l in range(mg.maxGrids)]
    for l, want in enumerate(OP.coarse_coefficients(sizes, masks, a, dtype)):
        assert bits_equal(mg.download_coefficient(l), want), l
        assert want.min() >= 0.5
    b = _coef(n3, dtype, 101)  # new values: the same arrays
    mg.set_coefficient(b)
    assert [mg.grid(l).d_a for l in range(mg.maxGrids)] == ptrs
    for l, want in enumerate(OP.coarse_coefficients(sizes, masks, b, dtype)):
        assert bits_equal(mg.download_coefficient(l), want), l
    mg.set_coefficient(None)
    assert not mg.has_coefficient and all(not mg.grid(l).d_a for l in range(mg.maxGrids))
    with pytest.raises(P.MgxError) as e:
        mg.download_coefficient(0)
    assert e.value.status == P.MGX_ERR_INVALID
    mg.close()


@pytest.fixture(scope="module")
def cycled():
    """the restated hierarchies after one and after two V(2,2) cycles, computed once per (grid, dtype, shift, coefficient seed)"""
    cache = {}

    def get(grid, dtype, s, seed=100):
        key = (grid, np.dtype(dtype).name, s, seed)
        if key not in cache:
            n3 = GRIDS[grid][0]
            H = _restated(grid, dtype, s, _coef(n3, dtype, seed), _rand(n3, dtype, 1), _rand(n3, dtype, 2))
            H.vcycle(0, 2, 2)
            first = copy.deepcopy(H)
            if seed == 100:
                H.vcycle(0, 2, 2)
            cache[key] = (first, H)
        return cache[key]
    return get


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", CYCLE_SHIFTS)
@pytest.mark.parametrize("grid", range(len(GRIDS)))
def test_vcycle_matches_restated_cycle(ctx, cycled, grid, s, dtype):
    n3 = GRIDS[grid][0]
    first, second = cycled(grid, dtype, s)
    mg = _mg(ctx, grid, dtype, s, _coef(n3, dtype), v=_rand(n3, dtype, 1), f=_rand(n3, dtype, 2))
    assert mg.shift == s and mg.has_coefficient
    mg.VCycle(0, 2, 2)
    assert ctx.last_relax_kernel().startswith("relax_coef3d_xs_kernel")
    _same_levels(mg, first, "eager")
    mg.VCycle(0, 2, 2)  # starts from other rim flags (the coarse f's boundary is known to be zero now)
    _same_levels(mg, second, "second")
    mg.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", CYCLE_SHIFTS)
@pytest.mark.parametrize("grid", range(len(GRIDS)))
def test_fmg_matches_restated_cycle(ctx, grid, s, dtype):
    n3 = GRIDS[grid][0]
    v, f, a = _rand(n3, dtype, 5), _rand(n3, dtype, 6), _coef(n3, dtype)
    H = _restated(grid, dtype, s, a, v, f)
    H.fmg(0, 1, 2, 2)
    for graph in (False, True):
        mg = _mg(ctx, grid, dtype, s, a, v=v, f=f)
        mg.use_graph = graph
        mg.FullMultiGridVCycle(0, 1, 2, 2)
        _same_levels(mg, H, "fmg graph=%s" % graph)
        mg.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", CYCLE_SHIFTS)
@pytest.mark.parametrize("grid", range(len(GRIDS)))
def test_graph_replay_new_values_and_clearing(ctx, cycled, grid, s, dtype):
    n3, rng, how = GRIDS[grid]
    v, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    mg = _mg(ctx, grid, dtype, s, _coef(n3, dtype), v=v, f=f)
    mg.use_graph = True
    execs = []
    for rep in range(4):  # capture; capture under the rim flags the first cycle left; replay; replay
        mg.upload_v(0, v)
        mg.VCycle(0, 2, 2)
        _same_levels(mg, cycled(grid, dtype, s)[0], rep)  # the eager cycle's bits (test_vcycle_matches_restated_cycle)
        execs.append(mg._mg.contents.graph_exec[0])
    assert execs[2] and execs[3] == execs[2], "the last cycle was captured again instead of replayed"
    rec = bytes(mg._mg.contents.graph_rec[0])
    mg.set_coefficient(_coef(n3, dtype, 101))  # new values in the same arrays: a replay reads them
    mg.upload_v(0, v)
    mg.VCycle(0, 2, 2)
    assert mg._mg.contents.graph_exec[0] == execs[3] and bytes(mg._mg.contents.graph_rec[0]) == rec, "new values captured again"
    _same_levels(mg, cycled(grid, dtype, s, 101)[0], "new values")
    mg.set_coefficient(None)  # the record holds the array: cleared, the next cycle is captured again -- the plain cycle
    mg.upload_v(0, v)
    mg.VCycle(0, 2, 2)
    assert bytes(mg._mg.contents.graph_rec[0]) != rec, "the record does not hold the coefficient"
    plain = P.MultiGrid3D(ctx, n3, rng, dtype, residual_mode=P.CORRECT, coarsening=how, shift=s)
    plain.upload_v(0, v)
    plain.upload_f(0, f)
    plain.VCycle(0, 2, 2)
    for l in range(mg.maxGrids):
        assert bits_equal(mg.download_v(l), plain.download_v(l)), ("cleared", l)
    plain.close()
    # set, cleared and set again with no cycle in between: the arrays are new ones (level 0's may even come back at its old
    # address), and no graph of the earlier arrays may be replayed
    mg.set_coefficient(_coef(n3, dtype))
    mg.upload_v(0, v)
    mg.VCycle(0, 2, 2)
    mg.set_coefficient(None)
    mg.set_coefficient(_coef(n3, dtype, 101))
    assert not mg._mg.contents.graph_exec[0], "a graph of freed coefficient arrays was kept"
    mg.upload_v(0, v)
    mg.VCycle(0, 2, 2)
    _same_levels(mg, cycled(grid, dtype, s, 101)[0], "set again")
    mg.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_relax_residual_and_norm_through_the_hierarchy(ctx, dtype):
    n3, rng, _ = GRIDS[1]
    s = 0.75
    v, f, a = _rand(n3, dtype, 7), _rand(n3, dtype, 8), _coef(n3, dtype)
    mg = _mg(ctx, 1, dtype, s, a, v=v, f=f)
    mg.Relax(0, 3)
    want = OP.Op(n3, rng, dtype, s, a).relax(v, f, 3)
    assert bits_equal(mg.download_v(0), want)
    r = OP.Op(n3, rng, dtype, s, a).residual(want, f)
    assert bits_equal(mg.CalculateResidual(0), r)
    assert close(mg.ResidualNorm(0), math.sqrt(OP.fsum_sq(r)), 1e-12)
    mg.close()


# ---------------------------------------------------------------------------------------------------------- solves
PCG_N = (33, 33, 33)
COEFS = {"smooth": lambda: OC.smooth_coefficient(PCG_N), "jump10": lambda: OC.jump_coefficient(PCG_N, 10)}


@pytest.mark.parametrize("krylov", [True, False])
@pytest.mark.parametrize("s", CYCLE_SHIFTS)
@pytest.mark.parametrize("which", ["smooth", "jump10"])
def test_pcg_matches_restatement(ctx, which, s, krylov):
    n3, tol = PCG_N, 1e-10
    a, f = COEFS[which](), problem(n3)
    v0 = np.zeros_like(f)
    v0[boundary_mask(n3)] = _rand(n3, np.float64, 9)[boundary_mask(n3)]  # Dirichlet data
    if krylov:
        want_x, want_k, _, want_c = OP.fcg(OP.Op(n3, UNIT, np.float64, s, a), v0, f, tol=tol, maxit=100)[:4]
    else:
        want_x, want_k, _, want_c = OP.cycles_to(OP.Op(n3, UNIT, np.float64, s, a), v0, f, 2, 2, tol, 100)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, shift=s, coefficient=a)
    mg.upload_v(0, v0)
    mg.upload_f(0, f)
    k, rel, conv, hist = mg.PCG(2, 2, tol, 100, krylov=krylov)
    x = mg.download_v(0)
    assert bits_equal(mg.download_f(0), f), "d_f[0] was not restored"
    mg.close()
    r, r0 = OP.Op(n3, UNIT, np.float64, s, a).residual(x, f), OP.Op(n3, UNIT, np.float64, s, a).residual(v0, f)
    true_rel = math.sqrt(OP.fsum_sq(r) / OP.fsum_sq(r0))
    print("PCG %s s=%g krylov=%s: %d iterations (restated %d), rel %.3e, restated residual of the result %.3e"
          % (which, s, krylov, k, want_k, rel, true_rel))
    assert k == want_k and conv == want_c and conv
    assert rel < tol and true_rel < tol and close(rel, true_rel, 1e-6)
    assert bits_equal(x[boundary_mask(n3)], v0[boundary_mask(n3)]), "the boundary was changed"
    if krylov and which == "smooth":
        x2, k2, rel2, conv2 = P.solve3d_pcg(ctx, v0, f, UNIT, tol=tol, krylov=krylov, shift=s, coefficient=a)
        assert (k2, conv2) == (k, conv) and bits_equal(x2, x)


# ---------------------------------------------------------------------------------------------------------- backward Euler
EULER_N = (33, 17, 17)


def _mode(n3):
    ax = [np.sin(np.pi * np.linspace(0.0, 1.0, k)) for k in n3]
    u = ax[2][:, None, None] * ax[1][None, :, None] * ax[0][None, None, :]
    u[boundary_mask(n3)] = 0.0
    return u


def test_backward_euler_with_a_constant_coefficient_is_kappa(ctx):
    """a = 2 everywhere with kappa = 1 is the coefficient-free hierarchy with kappa = 2: five steps agree to 1e-9 (relative, max
    norm).  The bound is from the solver tolerance 1e-12 of either run times the conditioning of a step (1 + kappa dt lam_max,
    about 120 here) times the steps, not measured."""
    n3, steps, dt, tol = EULER_N, 5, 1e-2, 1e-12
    u0 = _mode(n3)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, coefficient=np.full(O.shape(n3), 2.0))
    mg.upload_v(0, u0)
    its, worst, conv = mg.BackwardEuler(steps, dt, 1.0, tol=tol)
    u = mg.download_v(0)
    assert mg.shift == 1.0 / dt and mg.has_coefficient
    mg.close()
    ref = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT)
    ref.upload_v(0, u0)
    its2, worst2, conv2 = ref.BackwardEuler(steps, dt, 2.0, tol=tol)
    want = ref.download_v(0)
    ref.close()
    diff = np.abs(u - want).max() / np.abs(want).max()
    print("backward Euler a = 2, kappa = 1 against kappa = 2: %d and %d iterations, worst residuals %.3e and %.3e, relative difference %.3e"
          % (its, its2, worst, worst2, diff))
    assert conv and conv2 and worst < tol and worst2 < tol
    assert diff <= 1e-9, diff


def test_backward_euler_steps_solve_their_own_systems(ctx):
    n3, kappa, dt, tol = EULER_N, 0.7, 3e-3, 1e-10
    s = 1.0 / (kappa * dt)
    a = OC.smooth_coefficient(n3)
    u = _rand(n3, np.float64, 20)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, coefficient=a)
    mg.upload_v(0, u)
    for step in range(5):
        its, worst, conv = mg.BackwardEuler(1, dt, kappa, tol=tol)
        new = mg.download_v(0)
        f = OP.Op(n3, UNIT, np.float64, mg.shift).rhs(u, None, 1.0 / kappa)
        assert bits_equal(interior(mg.download_f(0)), interior(f)), "d_f[0] is not the step's right-hand side"
        rel = math.sqrt(OP.fsum_sq(OP.Op(n3, UNIT, np.float64, mg.shift, a).residual(new, f)) /
                        OP.fsum_sq(OP.Op(n3, UNIT, np.float64, mg.shift, a).residual(u, f)))
        print("backward Euler, smooth coefficient, step %d: %d iterations, residual %.3e (restated %.3e)" % (step, its, worst, rel))
        assert conv and worst < tol and rel < tol
        assert bits_equal(new[boundary_mask(n3)], u[boundary_mask(n3)]), "the Dirichlet data changed"
        u = new
    assert close(mg.shift, s, 1e-15)
    mg.close()


# ---------------------------------------------------------------------------------------------------------- rejections
def test_bad_coefficients_and_settings_are_rejected(ctx):
    n3 = (17, 17, 17)
    good = _coef(n3, np.float64)
    v, f = _rand(n3, np.float64, 1), _rand(n3, np.float64, 2)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT)
    mg.upload_v(0, v)
    mg.upload_f(0, f)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        a = good.copy()
        a[0, 3, 5] = bad  # a boundary point: the coefficient is read there too
        with pytest.raises(P.MgxError) as e:
            mg.set_coefficient(a)
        assert e.value.status == P.MGX_ERR_INVALID and not mg.has_coefficient
    mg.VCycle(0, 2, 2)  # still the plain hierarchy
    assert bits_equal(mg.download_v(0), O.cycle3d(n3, UNIT, nlevels=0, mode=0, v0=1, v1=2, v2=2, v=v, f=f, residual_mode=O.CORRECT,
                                                  dtype=np.float64))
    mg.set_coefficient(good)
    a = good.copy()
    a[8, 8, 8] = -3.0
    with pytest.raises(P.MgxError):
        mg.set_coefficient(a)
    assert bits_equal(mg.download_coefficient(0), good), "a rejected coefficient changed the hierarchy"
    mg.close()
    with pytest.raises(P.MgxError) as e:
        P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, layout="natural", coefficient=good)
    assert e.value.status == P.MGX_ERR_INVALID and "layout" in str(e.value)
    with pytest.raises(P.MgxError) as e:
        P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.REF_COMPAT, coefficient=good)
    assert e.value.status == P.MGX_ERR_INVALID and "CORRECT" in str(e.value)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT)
    mg.set_smoother("jacobi")
    with pytest.raises(P.MgxError) as e:
        mg.set_coefficient(good)
    assert e.value.status == P.MGX_ERR_INVALID and "smoother" in str(e.value) and not mg.has_coefficient
    mg.set_smoother("rbgs")
    mg.set_coefficient(good)
    # the members are public: a setting changed after the coefficient is caught where the coefficient is used
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
    assert e.value.status == P.MGX_ERR_INVALID and "coefficient" in str(e.value)
    k, rel, conv, _ = mg.PCG(2, 2, 1e-8, 30)  # and usable afterwards
    assert conv and rel < 1e-8
    mg.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_coefficient_is_the_old_hierarchy(dtype):
    n3 = (33, 33, 33)
    v, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    c = P.Context(0)  # a context of its own: the kernel name it reports is this hierarchy's
    try:
        mg = P.MultiGrid3D(c, n3, UNIT, dtype, residual_mode=P.CORRECT)
        assert not mg.has_coefficient and not mg.grid(0).d_a
        mg.upload_v(0, v)
        mg.upload_f(0, f)
        mg.VCycle(0, 2, 2)
        assert "coef" not in c.last_relax_kernel() and "shift" not in c.last_relax_kernel(), c.last_relax_kernel()
        assert bits_equal(mg.download_v(0), O.cycle3d(n3, UNIT, nlevels=0, mode=0, v0=1, v1=2, v2=2, v=v, f=f, residual_mode=O.CORRECT,
                                                      dtype=dtype))
        mg.close()
    finally:
        c.close()
