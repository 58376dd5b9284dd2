"""GPU suite: homogeneous Neumann faces (csrc/mgx_rim3d.hip), the hierarchy that cycles with a face mask
(MultiGrid3D(neumann=...)) and the plain-cycling solve and implicit heat steps on it.

The eight _bc kernel entries are checked bit for bit against the numpy restatement (tests/op_restated.py), with poisoned
pads, on rows longer than a wave, rows that end inside a tile and three-point axes (both mirrors of an axis are then the same
point); mask 0 against the existing entries too.  The cycles against the restated cycle, every level, bit for bit, eagerly and
through captured graphs, with the mask changed and cleared in between; the solver against the restated cycle counts; the time
stepping in a closed box against the heat content it must keep."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

import op_cases as OC
import op_restated as OP
import oracle as O
import pde_multigrid_amd as P
from conftest import bits_equal
from op_cases import VCYCLE_CASES, gaussian, vcycle_case
from odd_shapes import pads_unchanged, run_poisoned
from pde_multigrid_amd.multigrid import _ct, _ip, _rp, grid_spacing, xs_unpack
from solve_restated import close

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]
UNIT = [0, 1, 0, 1, 0, 1]
DTYPES = [np.float64, np.float32]
# 131 ends inside a tile; the rows of 257 and 513 span several waves; on a three-point axis both mirrors are the middle point
SHAPES = [(17, 17, 17), (21, 13, 29), (131, 7, 9), (257, 9, 5), (513, 5, 5), (3, 3, 3), (3, 5, 9), (5, 3, 3)]
MASKS = [0, 1, 2, 12, 48, 21, 42, 37, 63]
WORK_GUARD = 64


def shifts(bc):
    return [0.75, 1e4] if bc == 63 else [0.0, 0.75, 1e4]  # a closed box without a shift is singular


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


def _rand(n3, dtype, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, O.shape(n3)).astype(dtype)


def _fn(name, dtype):
    s, ct = _ct(dtype)
    return getattr(P.lib, "mgx3dxs_%s_%s" % (name, s)), ct


def _h(n3, rng, dtype):
    return _rp(grid_spacing(n3, rng, dtype), _ct(dtype)[1])


def _rng(n3):
    return UNIT if n3 == (17, 17, 17) else RG  # the unit cube on 2^k + 1 points: the exact-reciprocal form of the residual


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


# ---------------------------------------------------------------------------------------------------------- kernel entries
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("coef", [False, True])
@pytest.mark.parametrize("n3", SHAPES)
def test_relax_bc(ctx, n3, coef, dtype):
    rng = _rng(n3)
    v, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    a = _rand(n3, dtype, 3, 0.5, 2.0) if coef else None
    fn, ct = _fn("relax_coef_bc" if coef else "relax_shift_bc", dtype)
    for bc in MASKS:
        unk = OP.unknown_mask(n3, bc)
        for s in shifts(bc):
            for sweeps in (1, 3):
                if coef:
                    ups, outs = run_poisoned(ctx, [v, f, a], lambda x, b, c: fn(ctx._h, x, b, c, _ip(n3), _h(n3, rng, dtype), ct(s), C.c_int(sweeps),
                                                                                C.c_int(bc)), dtype)
                else:
                    ups, outs = run_poisoned(ctx, [v, f], lambda x, b: fn(ctx._h, x, b, _ip(n3), _h(n3, rng, dtype), ct(s), C.c_int(sweeps),
                                                                          C.c_int(bc)), dtype)
                got = xs_unpack(outs[0], n3[0])
                want = OP.Op(n3, rng, dtype, s, a, bc=bc).relax(v, f, sweeps)
                assert bits_equal(got, want), (bc, s, sweeps, np.argwhere(got != want)[:5])
                assert bits_equal(got[~unk], v[~unk]), "a Dirichlet entry of v was written"
                assert pads_unchanged(ups[0], outs[0], n3[0]) and all(bits_equal(o, u) for o, u in zip(outs[1:], ups[1:])), (bc, s, sweeps)
                if bc == 0:  # ... and the existing entry's bits
                    old = P.ops3dxs.relax_coef(ctx, v, f, a, n3, rng, s, sweeps) if coef else P.ops3dxs.relax_shift(ctx, v, f, n3, rng, s, sweeps)
                    assert bits_equal(got, old), (s, sweeps)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("coef", [False, True])
@pytest.mark.parametrize("n3", SHAPES)
def test_residual_bc(ctx, n3, coef, dtype):
    rng = _rng(n3)
    v, f, r0 = _rand(n3, dtype, 5), _rand(n3, dtype, 6), _rand(n3, dtype, 7)
    a = _rand(n3, dtype, 8, 0.5, 2.0) if coef else None
    fn, ct = _fn("residual_coef_bc" if coef else "residual_shift_bc", dtype)
    ins = [v, f, a] if coef else [v, f]
    w = Work(ctx, n3, dtype)

    def run(arrays, store, summed, s, bc):
        def call(*p):
            r = p[len(ins)] if store else None
            return fn(ctx._h, *p[:len(ins)], r, _ip(n3), _h(n3, rng, dtype), ct(s), w.work if summed else None, w.sum if summed else None,
                      C.c_int(bc))
        return run_poisoned(ctx, arrays, call, dtype)

    try:
        for bc in MASKS:
            for s in shifts(bc):
                want = OP.Op(n3, rng, dtype, s, a, bc=bc).residual(v, f)
                want_ss = OP.fsum_sq(want)
                sums = []
                for rep in range(2):
                    ups, outs = run(ins + [r0], True, True, s, bc)
                    got = xs_unpack(outs[-1], n3[0])
                    assert bits_equal(got, want), (bc, s, np.argwhere(got != want)[:5])  # the Dirichlet points written as 0
                    assert all(bits_equal(o, u) for o, u in zip(outs[:-1], ups[:-1])) and pads_unchanged(ups[-1], outs[-1], n3[0])
                    sums.append(w.result())
                assert sums[0] == sums[1], "two runs gave different sums"
                assert close(sums[0], want_ss, 1e-13), (bc, s, sums[0], want_ss)
                ups, outs = run(ins, False, True, s, bc)  # the sum alone
                assert w.result() == sums[0] and all(bits_equal(o, u) for o, u in zip(outs, ups))
                ups, outs = run(ins + [r0], True, False, s, bc)  # r alone
                assert bits_equal(xs_unpack(outs[-1], n3[0]), want) and pads_unchanged(ups[-1], outs[-1], n3[0])
                if bc == 0:
                    old = (P.ops3dxs.residual_coef(ctx, v, f, a, n3, rng, s) if coef else P.ops3dxs.residual_shift(ctx, v, f, n3, rng, s))
                    assert bits_equal(got, old[0]) and sums[0] == old[1], s
    finally:
        w.close()


def _pairs(n3):
    """(fine, coarse) size pairs around a listed shape: the shape as the coarse grid, and as the fine one where its coarse grid is a
    level of its own (odd extents of at least 3)"""
    out = [(tuple(2 * k - 1 for k in n3), n3)]
    cn = O.csize(n3)
    if all(k >= 3 and k % 2 == 1 for k in cn):
        out.append((n3, cn))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", SHAPES)
def test_transfers_bc(ctx, n3, dtype):
    rfn, _ = _fn("restrict_bc", dtype)
    ifn, _ = _fn("interpolate_bc", dtype)
    cfn, _ = _fn("interpolate_correct_bc", dtype)
    for fn3, cn3 in _pairs(n3):
        fine, coarse = _rand(fn3, dtype, 11), _rand(cn3, dtype, 12)
        for bc in MASKS:
            ups, outs = run_poisoned(ctx, [fine, coarse], lambda a, b: rfn(ctx._h, a, _ip(fn3), b, _ip(cn3), C.c_int(bc)), dtype)
            got = xs_unpack(outs[1], cn3[0])
            assert bits_equal(got, OP.restrict(fn3, fine, bc, dtype)), ("restrict", fn3, bc)
            assert bits_equal(outs[0], ups[0]) and pads_unchanged(ups[1], outs[1], cn3[0])
            if bc == 0:
                assert bits_equal(got, P.ops3dxs.restrict(ctx, fine, fn3))
            for add, kfn in ((False, ifn), (True, cfn)):
                ups, outs = run_poisoned(ctx, [fine, coarse], lambda a, b: kfn(ctx._h, a, _ip(fn3), b, _ip(cn3), C.c_int(bc)), dtype)
                got = xs_unpack(outs[0], fn3[0])
                assert bits_equal(got, OP.interpolate(fn3, fine, coarse, bc, dtype, add=add)), ("interpolate", add, fn3, bc)
                unk = OP.unknown_mask(fn3, bc)
                assert bits_equal(got[~unk], fine[~unk]), "a Dirichlet entry was written"
                assert bits_equal(outs[1], ups[1]) and pads_unchanged(ups[0], outs[0], fn3[0])
                if bc == 0:
                    old = P.ops3dxs.interpolate_correct(ctx, fine, fn3, coarse) if add else P.ops3dxs.interpolate(ctx, fine, fn3, coarse)
                    assert bits_equal(got, old)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", SHAPES)
def test_shift_rhs_bc(ctx, n3, dtype):
    u, q, f0 = _rand(n3, dtype, 13), _rand(n3, dtype, 14), _rand(n3, dtype, 15)
    fn, ct = _fn("shift_rhs_bc", dtype)
    for bc in MASKS:
        for s in (0.75, 1e4):
            ups, outs = run_poisoned(ctx, [u, q, f0], lambda a, b, c: fn(ctx._h, a, b, ct(0.3), ct(s), c, _ip(n3), C.c_int(bc)), dtype)
            got = xs_unpack(outs[2], n3[0])
            assert bits_equal(got, OP.Op(n3, UNIT, dtype, s, bc=bc).rhs(u, q, 0.3, f=f0)), (bc, s)  # the Dirichlet entries of f as they were
            assert bits_equal(outs[0], ups[0]) and bits_equal(outs[1], ups[1]) and pads_unchanged(ups[2], outs[2], n3[0])
            ups, outs = run_poisoned(ctx, [u, f0], lambda a, c: fn(ctx._h, a, None, ct(0.3), ct(s), c, _ip(n3), C.c_int(bc)), dtype)
            assert bits_equal(xs_unpack(outs[1], n3[0]), OP.Op(n3, UNIT, dtype, s, bc=bc).rhs(u, None, 0.3, f=f0)), (bc, s)
            if bc == 0:
                assert bits_equal(got, P.ops3dxs.shift_rhs(ctx, u, q, 0.3, s, n3, f=f0))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", SHAPES)
def test_set_rim_bc(ctx, n3, dtype):
    v = _rand(n3, dtype, 16)
    fn, ct = _fn("set_rim_bc", dtype)
    for bc in MASKS:
        for value in (0.0, -2.5):
            ups, outs = run_poisoned(ctx, [v], lambda a: fn(ctx._h, a, _ip(n3), ct(value), C.c_int(bc)), dtype)
            want = v.copy()
            want[OP.face_unknowns(n3, bc)] = value  # the interior and the Dirichlet entries as they were
            assert bits_equal(xs_unpack(outs[0], n3[0]), want), (bc, value)
            assert pads_unchanged(ups[0], outs[0], n3[0])
            assert bits_equal(P.ops3dxs.set_rim_bc(ctx, v, n3, value, bc), want)
    with pytest.raises(P.MgxError) as e:
        P.ops3dxs.set_rim_bc(ctx, v, n3, 0.0, 64)
    assert e.value.status == P.MGX_ERR_INVALID


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernels_reject_bad_masks_shifts_and_sizes(ctx, dtype):
    n3 = (17, 9, 9)
    a = _rand(n3, dtype, 1, 0.5, 2.0)
    ops = P.ops3dxs

    def calls(s, bc, n=n3, x=a):
        return [lambda: ops.relax_shift_bc(ctx, x, x, n, RG, s, 1, bc), lambda: ops.relax_coef_bc(ctx, x, x, x, n, RG, s, 1, bc),
                lambda: ops.residual_shift_bc(ctx, x, x, n, RG, s, bc), lambda: ops.residual_coef_bc(ctx, x, x, x, n, RG, s, bc),
                lambda: ops.shift_rhs_bc(ctx, x, x, 1.0, s, n, bc)]

    transfers = lambda bc: [lambda: ops.restrict_bc(ctx, a, n3, bc), lambda: ops.interpolate_bc(ctx, a, n3, np.zeros(O.shape(O.csize(n3)), dtype), bc),
                            lambda: ops.interpolate_correct_bc(ctx, a, n3, np.zeros(O.shape(O.csize(n3)), dtype), bc)]
    for call in calls(1.0, 64) + calls(1.0, -1) + transfers(64) + calls(-1.0, 5) + calls(float("nan"), 5) + calls(float("inf"), 5):
        with pytest.raises(P.MgxError) as e:
            call()
        assert e.value.status == P.MGX_ERR_INVALID
    bad = (16, 9, 9)
    b = np.ones(O.shape(bad), dtype)
    for call in calls(1.0, 5, bad, b):
        with pytest.raises(P.MgxError) as e:
            call()
        assert e.value.status == P.MGX_ERR_SIZE
    # a coarse grid that is no level of its own (131 -> 66) takes no mask
    fine = _rand((131, 7, 9), dtype, 2)
    with pytest.raises(P.MgxError) as e:
        ops.restrict_bc(ctx, fine, (131, 7, 9), 5)
    assert e.value.status == P.MGX_ERR_SIZE


# ---------------------------------------------------------------------------------------------------------- hierarchy
GRIDS = [((33, 33, 33), UNIT), ((65, 33, 17), RG)]
FACES = lambda bc: [bool((bc >> k) & 1) for k in range(6)]


def _mg(ctx, grid, dtype, bc, s, coef, v=None, f=None):
    n3, rng = GRIDS[grid]
    mg = P.MultiGrid3D(ctx, n3, rng, dtype, residual_mode=P.CORRECT, shift=s, coefficient=OC.smooth_coefficient(n3, dtype) if coef else None,
                       neumann=FACES(bc))
    if v is not None:
        mg.upload_v(0, v)
    if f is not None:
        mg.upload_f(0, f)
    return mg


def _restated(grid, dtype, bc, s, coef, v, f):
    n3, rng = GRIDS[grid]
    H = OP.Hierarchy(OP.Op(n3, rng, dtype, s, OC.smooth_coefficient(n3, dtype) if coef else None, bc=bc))
    H.v[0], H.f[0] = v.copy(), f.copy()
    return H


def _same_levels(mg, H, what):
    assert mg.maxGrids == len(H.sizes)
    for l, n in enumerate(H.sizes):
        assert mg.size(l) == n
        assert bits_equal(mg.download_v(l), H.v[l]), (what, "v", l)
        if l > 0:
            assert bits_equal(mg.download_f(l), H.f[l]), (what, "f", l)


@pytest.fixture(scope="module")
def cycled():
    """the restated hierarchies after one and after two V(2,2) cycles, computed once per case"""
    cache = {}

    def get(grid, dtype, bc, s, coef):
        key = (grid, np.dtype(dtype).name, bc, s, coef)
        if key not in cache:
            n3 = GRIDS[grid][0]
            H = _restated(grid, dtype, bc, s, coef, _rand(n3, dtype, 1), _rand(n3, dtype, 2))
            H.vcycle(0, 2, 2)
            first = copy.deepcopy(H)
            H.vcycle(0, 2, 2)
            cache[key] = (first, H)
        return cache[key]
    return get


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("coef", [False, True])
@pytest.mark.parametrize("s", [0.75, 100.0])
@pytest.mark.parametrize("bc", [1, 37, 63])
@pytest.mark.parametrize("grid", range(len(GRIDS)))
def test_vcycles_match_restated_cycles_eagerly_and_through_graphs(ctx, cycled, grid, bc, s, coef, dtype):
    n3 = GRIDS[grid][0]
    v, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    first, second = cycled(grid, dtype, bc, s, coef)
    mg = _mg(ctx, grid, dtype, bc, s, coef, v=v, f=f)
    assert mg.neumann == tuple(FACES(bc))
    mg.VCycle(0, 2, 2)
    _same_levels(mg, first, "eager")
    mg.VCycle(0, 2, 2)
    _same_levels(mg, second, "second")
    mg.use_graph = True
    execs = []
    for rep in range(3):  # capture, then replays
        mg.upload_v(0, v)
        mg.VCycle(0, 2, 2)
        _same_levels(mg, first, ("graph", rep))
        execs.append(mg._mg.contents.graph_exec[0])
    assert execs[1] and execs[2] == execs[1], "the last cycle was captured again instead of replayed"
    mg.close()


@pytest.fixture(scope="module")
def fmg_restated():
    """the restated hierarchies after FMG(1,2,2), computed once per case (the eager and the captured runs share them)"""
    cache = {}

    def get(grid, dtype, bc, s, coef):
        key = (grid, np.dtype(dtype).name, bc, s, coef)
        if key not in cache:
            n3 = GRIDS[grid][0]
            H = _restated(grid, dtype, bc, s, coef, _rand(n3, dtype, 5), _rand(n3, dtype, 6))
            H.fmg(0, 1, 2, 2)
            cache[key] = H
        return cache[key]
    return get


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("coef", [False, True])
@pytest.mark.parametrize("s", [0.75, 100.0])
@pytest.mark.parametrize("bc", [1, 37, 63])
@pytest.mark.parametrize("grid", range(len(GRIDS)))
def test_fmg_matches_restated_cycle(ctx, fmg_restated, grid, bc, s, coef, graph, dtype):
    """FMG(1,2,2), every level downloaded; with use_graph FMG's VCycle of every starting level is captured by the first run, captured
    again under the rim flags it left or replayed by the second, and replayed by the third"""
    n3 = GRIDS[grid][0]
    v, f = _rand(n3, dtype, 5), _rand(n3, dtype, 6)
    H = fmg_restated(grid, dtype, bc, s, coef)
    mg = _mg(ctx, grid, dtype, bc, s, coef, v=v, f=f)
    mg.use_graph = graph
    execs = []
    for rep in range(3 if graph else 1):
        mg.upload_v(0, v)
        mg.FullMultiGridVCycle(0, 1, 2, 2)
        _same_levels(mg, H, ("fmg", graph, rep))
        execs.append([mg._mg.contents.graph_exec[l] for l in range(mg.maxGrids)])
    if graph:
        assert all(execs[1]) and execs[2] == execs[1], "a level's cycle was captured again instead of replayed"
    else:
        assert not any(execs[0])
    mg.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", [False, True])
def test_mask_changed_between_cycles_then_cleared(ctx, cycled, graph, dtype):
    """a cycle under mask 1, one under mask 37 from the same start, then the mask cleared: the cycles of a hierarchy that never had
    one, bit for bit on every level"""
    grid, s = 0, 0.75
    n3, rng = GRIDS[grid]
    v, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    mg = _mg(ctx, grid, dtype, 1, s, False, v=v, f=f)
    mg.use_graph = graph
    mg.VCycle(0, 2, 2)
    _same_levels(mg, cycled(grid, dtype, 1, s, False)[0], "mask 1")
    rec = bytes(mg._mg.contents.graph_rec[0])
    mg.set_neumann(FACES(37))
    assert not graph or not mg._mg.contents.graph_exec[0], "the captured graph outlived the mask"
    mg.upload_v(0, v)
    mg.VCycle(0, 2, 2)
    _same_levels(mg, cycled(grid, dtype, 37, s, False)[0], "mask 37")
    assert not graph or bytes(mg._mg.contents.graph_rec[0]) != rec, "the record does not hold the mask"
    mg.set_neumann(None)
    assert mg.neumann == (False,) * 6
    parent = P.MultiGrid3D(ctx, n3, rng, dtype, residual_mode=P.CORRECT, shift=s)
    parent.use_graph = graph
    for m in (mg, parent):
        m.upload_v(0, v)
        m.upload_f(0, f)
    for rep in range(2):
        mg.VCycle(0, 2, 2)
        parent.VCycle(0, 2, 2)
        for l in range(mg.maxGrids):
            assert bits_equal(mg.download_v(l), parent.download_v(l)), (rep, "v", l)
            assert l == 0 or bits_equal(mg.download_f(l), parent.download_f(l)), (rep, "f", l)
    mg.FullMultiGridVCycle(0, 1, 2, 2)
    parent.FullMultiGridVCycle(0, 1, 2, 2)
    for l in range(mg.maxGrids):
        assert bits_equal(mg.download_v(l), parent.download_v(l)), ("fmg", l)
    mg.close()
    parent.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_mask_never_set_against_the_oracle(ctx, dtype):
    n3, rng = GRIDS[1]
    v, f = _rand(n3, dtype, 7), _rand(n3, dtype, 8)
    mg = P.MultiGrid3D(ctx, n3, rng, dtype, residual_mode=P.CORRECT)
    assert mg.neumann == (False,) * 6
    mg.upload_v(0, v)
    mg.upload_f(0, f)
    mg.VCycle(0, 2, 2)
    mg.VCycle(0, 2, 2)
    want = O.cycle3d(n3, rng, mode=0, v1=2, v2=2, reps=2, v=v, f=f, residual_mode=O.CORRECT, dtype=dtype)
    assert bits_equal(mg.download_v(0), want)
    mg.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_relax_residual_and_norm_through_the_hierarchy(ctx, dtype):
    n3, rng = GRIDS[1]
    bc, s = 37, 0.0  # the plain Laplacian with walls: the shifted kernels with s = 0
    v, f = _rand(n3, dtype, 7), _rand(n3, dtype, 8)
    mg = _mg(ctx, 1, dtype, bc, s, False, v=v, f=f)
    mg.Relax(0, 3)
    want = OP.Op(n3, rng, dtype, s, bc=bc).relax(v, f, 3)
    assert bits_equal(mg.download_v(0), want)
    r = OP.Op(n3, rng, dtype, s, bc=bc).residual(want, f)
    assert bits_equal(mg.CalculateResidual(0), r)
    assert close(mg.ResidualNorm(0), math.sqrt(OP.fsum_sq(r)), 1e-12)  # all unknowns, unweighted
    mg.close()


@pytest.mark.parametrize("bc,s,coef", VCYCLE_CASES)
def test_plain_cycling_counts_match_the_restatement(ctx, bc, s, coef):
    tol = 1e-10
    H = vcycle_case(bc, s, coef)
    n3, v0, f = H.sizes[0], H.v[0].copy(), H.f[0].copy()
    want_k, want_rel, want_c = H.cycle_to(2, 2, tol, 100)
    a = OC.smooth_coefficient(n3) if coef else None
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, shift=s, coefficient=a, neumann=FACES(bc))
    mg.upload_v(0, v0)
    mg.upload_f(0, f)
    k, rel, conv, hist = mg.PCG(2, 2, tol, 100, krylov=False)
    x = mg.download_v(0)
    assert bits_equal(mg.download_f(0), f), "d_f[0] was not restored"
    mg.close()
    print("bc %d s %g coef %d: %d cycles (restated %d), rel %.3e (restated %.3e)" % (bc, s, coef, k, want_k, rel, want_rel))
    assert (k, conv) == (want_k, want_c) and conv and rel < tol and close(rel, want_rel, 1e-6)
    unk = OP.unknown_mask(n3, bc)
    assert bits_equal(x[~unk], v0[~unk]), "the boundary data were changed"
    assert bits_equal(x, H.v[0])
    x2, k2, rel2, conv2 = P.solve3d_pcg(ctx, v0, f, UNIT, tol=tol, krylov=False, shift=s, coefficient=a, neumann=FACES(bc))
    assert (k2, conv2) == (k, conv) and bits_equal(x2, x)


# ---------------------------------------------------------------------------------------------------------- backward Euler
@pytest.mark.parametrize("kdt", [1e-2, 5e-5])
def test_backward_euler_in_a_closed_box_keeps_the_heat_content(ctx, kdt):
    """test_neumann_cpu's conservation case on the device: 17^3, all six faces walls, the smooth coefficient, Gaussian initial data,
    five steps solved to 1e-10: the relative drift of sum(w u) stays below 1e-9"""
    n3 = (17, 17, 17)
    u0 = gaussian(n3)
    W = OP.weights(n3, 63)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, coefficient=OC.smooth_coefficient(n3), neumann=[1] * 6)
    mg.upload_v(0, u0)
    its, worst, conv = mg.BackwardEuler(5, kdt, 1.0, tol=1e-10, maxit=50, krylov=False)
    u = mg.download_v(0)
    mg.close()
    heat0, heat = math.fsum((W * u0).ravel()), math.fsum((W * u).ravel())
    drift = abs(heat - heat0) / abs(heat0)
    print("kappa dt %g: %d cycles, worst relative residual %.3e, relative drift of the heat content %.3e" % (kdt, its, worst, drift))
    assert conv and worst < 1e-10
    assert drift < 1e-9, drift
    H = OP.Hierarchy(OP.Op(n3, UNIT, np.float64, 0.0, OC.smooth_coefficient(n3), bc=63))
    H.v[0] = u0.copy()
    want_its, _, _ = H.backward_euler(5, kdt, 1.0, 2, 2, 1e-10, 50)
    assert its == want_its and bits_equal(u, H.v[0])


def test_backward_euler_step_against_its_own_linear_system(ctx):
    n3, rng, bc, kappa, dt, tol = (33, 17, 17), UNIT, 37, 0.7, 3e-3, 1e-10
    s = 1.0 / (kappa * dt)
    u0, q, f0 = _rand(n3, np.float64, 20), _rand(n3, np.float64, 21), _rand(n3, np.float64, 22)
    mg = P.MultiGrid3D(ctx, n3, rng, residual_mode=P.CORRECT, neumann=FACES(bc))
    mg.upload_v(0, u0)
    mg.upload_f(0, f0)
    its, worst, conv = mg.BackwardEuler(1, dt, kappa, source=q, tol=tol, krylov=False)
    u, rhs_dev = mg.download_v(0), mg.download_f(0)
    assert mg.shift == s
    mg.close()
    f = OP.Op(n3, UNIT, np.float64, s, bc=bc).rhs(u0, q, 1.0 / kappa, f=f0)
    assert bits_equal(rhs_dev, f), "d_f[0] is not the step's right-hand side on the unknowns and what it was elsewhere"
    res = lambda x: OP.fsum_sq(OP.Op(n3, rng, np.float64, s, bc=bc).residual(x, f))
    rel = math.sqrt(res(u) / res(u0))
    print("one step, bc %d: %d cycles, residual %.3e (restated %.3e)" % (bc, its, worst, rel))
    assert conv and worst < tol and rel < tol and close(worst, rel, 1e-6)
    unk = OP.unknown_mask(n3, bc)
    assert bits_equal(u[~unk], u0[~unk]), "the Dirichlet data changed"


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_hierarchy_usable(ctx):
    n3 = (17, 17, 17)
    I = P.MGX_ERR_INVALID

    def refused(call, word):
        with pytest.raises(P.MgxError) as e:
            call()
        assert e.value.status == I and word in str(e.value), str(e.value)

    refused(lambda: P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, layout="natural", neumann=[1, 0, 0, 0, 0, 0]), "layout")
    refused(lambda: P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.REF_COMPAT, neumann=[1, 0, 0, 0, 0, 0]), "CORRECT")
    refused(lambda: P.MultiGrid3D(ctx, (33, 17, 9), RG, residual_mode=P.CORRECT, coarsening="semi", neumann=[1, 0, 0, 0, 0, 0]), "semi")
    with pytest.raises(ValueError):
        P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, neumann=[1, 0])
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT)
    mg.set_smoother("jacobi")
    refused(lambda: mg.set_neumann([1, 0, 0, 0, 0, 0]), "smoother")
    assert mg.neumann == (False,) * 6
    mg.set_smoother("rbgs")
    mg.set_neumann([1, 0, 0, 0, 1, 0])
    v, f = _rand(n3, np.float64, 1), _rand(n3, np.float64, 2)
    mg.upload_v(0, v)
    mg.upload_f(0, f)
    refused(lambda: mg.PCG(2, 2, 1e-8, 5, krylov=True), "Neumann")
    refused(lambda: mg.BackwardEuler(1, 1e-2, 1.0, krylov=True), "Neumann")
    refused(lambda: mg.PCG(2, 2, 1e-8, 5, krylov=False, precond="f32"), "Neumann")
    mg.shift = 0.0
    # the members are public: a setting changed after the mask is caught where the mask is used
    mg.set_smoother("jacobi")
    for call in (lambda: mg.VCycle(0, 2, 2), lambda: mg.Relax(0, 1), lambda: mg.ResidualNorm(0), lambda: mg.PCG(2, 2, 1e-8, 5, krylov=False),
                 lambda: mg.FullMultiGridVCycle(0, 1, 2, 2)):
        refused(call, "smoother")
    mg.set_smoother("rbgs")
    # all six faces without a shift: singular, caught where the operator is used
    mg.set_neumann([1] * 6)
    for call in (lambda: mg.VCycle(0, 2, 2), lambda: mg.Relax(0, 1), lambda: mg.ResidualNorm(0), lambda: mg.PCG(2, 2, 1e-8, 5, krylov=False)):
        refused(call, "singular")
    mg.shift = 0.75
    mg.upload_v(0, v)
    mg.VCycle(0, 2, 2)  # still usable
    H = OP.Hierarchy(OP.Op(n3, UNIT, np.float64, 0.75, bc=63))
    H.v[0], H.f[0] = v.copy(), f.copy()
    H.vcycle(0, 2, 2)
    assert bits_equal(mg.download_v(0), H.v[0])
    mg.close()
