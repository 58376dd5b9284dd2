"""The operator with a capacity, div(a grad u) - (s c) u = f, on the GPU: the mgx3dxs_*_cap kernels and their _bc forms
(csrc/mgx_cap3d.hip), the hierarchy that holds a capacity array per level (MultiGrid3D(capacity=c), set_capacity) and the solves and
implicit heat steps on it.

Every kernel is checked bit for bit against the numpy restatement of its arithmetic (tests/op_restated.py), with poisoned pads and
with both row counts of the colour pass; with c == 1 against the _coef entry on the same inputs; the capacity of every level against
the restated restriction chain; the cycles against the restated cycle, every level, eager and replayed from a graph."""
import ctypes as C
import math

import numpy as np
import pytest

import op_cases as OC
import op_restated as OP
import oracle as O
import pde_multigrid_amd as P
from conftest import bits_equal
from odd_shapes import pads_unchanged, run_poisoned
from pde_multigrid_amd.multigrid import _ct, _ip, _rp, grid_spacing, xs_unpack
from solve_restated import boundary_mask, close

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]
UNIT = [0, 1, 0, 1, 0, 1]
DTYPES = [np.float64, np.float32]
# (21,13,29): rows end inside a tile, several plane runs; (131,7,9): a row longer than a wave; (35,21,7): the smallest with 16
# interior rows, below which the colour pass lowers its rows per lane by itself, and a last tile of three rows; the last two of
# BC_SHAPES: the _bc forms' smallest
SHAPES = [(17, 17, 17), (21, 13, 29), (131, 7, 9), (257, 9, 5), (513, 5, 5), (35, 21, 7)]
BC_SHAPES = SHAPES + [(3, 3, 3), (3, 5, 9)]
MASKS = [0, 1, 12, 37, 63]
SHIFTS = [0.0, 0.75, 1e4]
WORK_GUARD = 64


def _cases(shapes):
    """(n3, bc, s): every shape with every mask and shift, but s = 0 in a closed box; the smallest shapes with a mask only"""
    return [(n3, bc, s) for n3 in shapes for bc in MASKS for s in SHIFTS if not (bc == 63 and s == 0) and (bc or min(n3) > 3 or n3 == (3, 5, 9))]


CASES = _cases(BC_SHAPES)


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


def _rand(n3, dtype, seed):
    return np.random.default_rng(seed).uniform(-1, 1, O.shape(n3)).astype(dtype)


def _coef(n3, dtype, seed=100):
    return np.random.default_rng(seed).uniform(0.5, 2, O.shape(n3)).astype(dtype)


def _cap(n3, dtype, seed=200):
    return OC.random_capacity(n3, dtype, seed)


def _fn(name, dtype):
    s, ct = _ct(dtype)
    return getattr(P.lib, "mgx3dxs_%s_%s" % (name, s)), ct


def _h(n3, dtype):
    return _rp(grid_spacing(n3, RG, dtype), _ct(dtype)[1])


def _forms(name, bc):
    """the entries that answer for a mask: the _bc form, and for mask 0 the plain entry too; each as (entry name, trailing arguments)"""
    return ([(name, [])] if bc == 0 else []) + [(name + "_bc", [C.c_int(bc)])]


class Work:
    """the reduction scratch of a call (mgx3dxs_krylov_work_elems_bc doubles, NaN guards behind them) and its device sum"""

    def __init__(self, ctx, n3, dtype):
        fn = getattr(P.lib, "mgx3dxs_krylov_work_elems_bc_" + _ct(dtype)[0])
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


def _unchanged(ups, outs, idx):
    return all(bits_equal(outs[i], ups[i]) for i in idx)


# ---------------------------------------------------------------------------------------------------------- operators
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3,bc,s", CASES)
def test_relax_cap(ctx, n3, bc, s, dtype):
    """1 and 3 sweeps, two and four rows per lane: the restatement's bits; f, a, c, the Dirichlet entries and the pads as they were"""
    v, f, a, c = _rand(n3, dtype, 1), _rand(n3, dtype, 2), _coef(n3, dtype), _cap(n3, dtype)
    assert (c == 0).any() and c.max() > 1
    try:
        for sweeps in (1, 3):
            want = OP.Op(n3, RG, dtype, s, a, c, bc).relax(v, f, sweeps)
            assert bits_equal(want[~OP.unknown_mask(n3, bc)], v[~OP.unknown_mask(n3, bc)])
            for knob in (2, 4):
                ctx.set_param("relax3d.rows", knob)
                rows = knob
                while rows > 1 and 4 * rows > n3[1] - 2:  # (the pass halves them while four waves of them exceed the interior rows)
                    rows //= 2
                for name, tail in _forms("relax_cap", bc):
                    fn, ct = _fn(name, dtype)
                    ups, outs = run_poisoned(ctx, [v, f, a, c], lambda x, b, aa, cc: fn(ctx._h, x, b, aa, cc, _ip(n3), _h(n3, dtype), ct(s),
                                                                                        C.c_int(sweeps), *tail), dtype)
                    kernel = ctx.last_relax_kernel()
                    assert kernel.startswith("relax_cap3d_xs_kernel") and int(kernel.rstrip(">").split(",")[2]) == rows, (knob, rows, kernel)
                    got = xs_unpack(outs[0], n3[0])
                    assert bits_equal(got, want), (name, sweeps, knob, np.argwhere(got != want)[:5])
                    assert pads_unchanged(ups[0], outs[0], n3[0]) and _unchanged(ups, outs, (1, 2, 3)), (name, sweeps, knob)
    finally:
        ctx.set_param("relax3d.rows", 4)
    assert bits_equal(want, P.ops3dxs.relax_cap(ctx, v, f, a, c, n3, RG, s, 3, bc if bc else None))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", SHIFTS)
@pytest.mark.parametrize("n3", SHAPES)
def test_relax_cap_from_zero(ctx, n3, s, dtype):
    v, f, a, c = _rand(n3, dtype, 3), _rand(n3, dtype, 4), _coef(n3, dtype), _cap(n3, dtype)
    f[1:-1:2, 1:-1, 1:-1] = 0  # zero right-hand sides too: the signs of the zeros the first pass stores
    fn, ct = _fn("relax_cap_from_zero", dtype)
    for sweeps in (1, 2):
        want = OP.Op(n3, RG, dtype, s, a, c).relax(np.zeros_like(v), f, sweeps)
        for rim_is_zero in (0, 1):
            v0 = v.copy()
            if rim_is_zero:  # the caller vouches for a zero boundary; the interior is stale
                v0[boundary_mask(n3)] = 0
            ups, outs = run_poisoned(ctx, [v0, f, a, c], lambda x, b, aa, cc: fn(ctx._h, x, b, aa, cc, _ip(n3), _h(n3, dtype), ct(s),
                                                                                 C.c_int(sweeps), C.c_int(rim_is_zero)), dtype)
            assert bits_equal(xs_unpack(outs[0], n3[0]), want), (sweeps, rim_is_zero)
            assert pads_unchanged(ups[0], outs[0], n3[0], zero_ok=not rim_is_zero) and _unchanged(ups, outs, (1, 2, 3))
    assert ctx.last_relax_kernel().startswith("relax_cap3d_xs_kernel")
    assert bits_equal(want, P.ops3dxs.relax_cap_from_zero(ctx, v, f, a, c, n3, RG, s, 2, False))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3,bc,s", CASES)
def test_residual_cap(ctx, n3, bc, s, dtype):
    v, f, a, c, r0 = _rand(n3, dtype, 5), _rand(n3, dtype, 6), _coef(n3, dtype), _cap(n3, dtype), _rand(n3, dtype, 7)
    want = OP.Op(n3, RG, dtype, s, a, c, bc).residual(v, f)
    want_ss = OP.fsum_sq(want)
    w = Work(ctx, n3, dtype)
    try:
        for name, tail in _forms("residual_cap", bc):
            fn, ct = _fn(name, dtype)
            sums = []
            for rep in range(2):
                ups, outs = run_poisoned(ctx, [v, f, a, c, r0], lambda x, b, aa, cc, d: fn(ctx._h, x, b, aa, cc, d, _ip(n3), _h(n3, dtype), ct(s),
                                                                                           w.work, w.sum, *tail), dtype)
                assert bits_equal(xs_unpack(outs[4], n3[0]), want), name  # 0 at the Dirichlet points
                assert _unchanged(ups, outs, (0, 1, 2, 3)) and pads_unchanged(ups[4], outs[4], n3[0]), name
                sums.append(w.result())
            assert sums[0] == sums[1], "two runs gave different sums"
            assert close(sums[0], want_ss, 1e-13), (name, sums[0], want_ss)
            # the sum alone (r = NULL), and r alone (no sum, no work array)
            ups, outs = run_poisoned(ctx, [v, f, a, c], lambda x, b, aa, cc: fn(ctx._h, x, b, aa, cc, None, _ip(n3), _h(n3, dtype), ct(s),
                                                                                w.work, w.sum, *tail), dtype)
            assert w.result() == sums[0] and _unchanged(ups, outs, (0, 1, 2, 3))
            ups, outs = run_poisoned(ctx, [v, f, a, c, r0], lambda x, b, aa, cc, d: fn(ctx._h, x, b, aa, cc, d, _ip(n3), _h(n3, dtype), ct(s),
                                                                                       None, None, *tail), dtype)
            assert bits_equal(xs_unpack(outs[4], n3[0]), want) and pads_unchanged(ups[4], outs[4], n3[0])
    finally:
        w.close()
    r, ss = P.ops3dxs.residual_cap(ctx, v, f, a, c, n3, RG, s, bc if bc else None)
    assert bits_equal(r, want) and ss == sums[0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3,bc,s", CASES)
def test_apply_cap_dot(ctx, n3, bc, s, dtype):
    p, a, c, q0 = _rand(n3, dtype, 8), _coef(n3, dtype), _cap(n3, dtype), _rand(n3, dtype, 9)
    unk = OP.unknown_mask(n3, bc)
    want = OP.Op(n3, RG, dtype, s, a, c, bc).apply_A(p)
    want_pq = OP.wdot(OP.weights(n3, bc), p, want)
    w = Work(ctx, n3, dtype)
    try:
        for name, tail in _forms("apply_cap_dot", bc):
            fn, ct = _fn(name, dtype)
            sums = []
            for rep in range(2):
                ups, outs = run_poisoned(ctx, [p, a, c, q0], lambda x, aa, cc, b: fn(ctx._h, x, aa, cc, b, _ip(n3), _h(n3, dtype), ct(s),
                                                                                     w.work, w.sum, *tail), dtype)
                q = xs_unpack(outs[3], n3[0])
                assert bits_equal(q[unk], want[unk]), name
                assert bits_equal(q[~unk], q0[~unk]), "a Dirichlet entry of q was written"
                assert _unchanged(ups, outs, (0, 1, 2)) and pads_unchanged(ups[3], outs[3], n3[0]), name
                sums.append(w.result())
            assert sums[0] == sums[1], "two runs gave different sums"
            assert close(sums[0], want_pq, 1e-13), (name, sums[0], want_pq)
    finally:
        w.close()
    q, pq = P.ops3dxs.apply_cap_dot(ctx, p, a, c, n3, RG, s, bc if bc else None)
    assert bits_equal(q[unk], want[unk]) and pq == sums[0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3,bc,s", CASES)
def test_cap_rhs(ctx, n3, bc, s, dtype):
    u, c, q, f0 = _rand(n3, dtype, 10), _cap(n3, dtype), _rand(n3, dtype, 11), _rand(n3, dtype, 12)
    ct = _ct(dtype)[1]
    for name, tail in _forms("cap_rhs", bc):
        fn = _fn(name, dtype)[0]
        for src in (q, None):
            want = OP.Op(n3, UNIT, dtype, s, c=c, bc=bc).rhs(u, src, 0.3, f=f0)
            arrays = [u, c, f0] + ([q] if src is not None else [])
            ups, outs = run_poisoned(ctx, arrays, lambda x, cc, d, qq=None: fn(ctx._h, x, cc, qq, ct(0.3), ct(s), d, _ip(n3), *tail), dtype)
            assert bits_equal(xs_unpack(outs[2], n3[0]), want), (name, src is None)  # the Dirichlet entries of f as they were
            assert pads_unchanged(ups[2], outs[2], n3[0]) and _unchanged(ups, outs, [0, 1] + ([3] if src is not None else []))
    assert bits_equal(P.ops3dxs.cap_rhs(ctx, u, c, None, 0.3, s, n3, bc if bc else None, f=f0), want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bc", MASKS)
@pytest.mark.parametrize("n3", SHAPES)
def test_unit_capacity_gives_the_bits_of_the_coefficient_entries(ctx, n3, bc, dtype):
    """c == 1: s * 1 = s, so every _cap entry returns what its _coef entry returns on the same inputs"""
    s = 0.75
    v, f, a = _rand(n3, dtype, 13), _rand(n3, dtype, 14), _coef(n3, dtype)
    one = np.ones(O.shape(n3), dtype)
    X, m = P.ops3dxs, (bc if bc else None)
    if bc:
        assert bits_equal(X.relax_cap(ctx, v, f, a, one, n3, RG, s, 2, bc), X.relax_coef_bc(ctx, v, f, a, n3, RG, s, 2, bc))
        r1, s1 = X.residual_cap(ctx, v, f, a, one, n3, RG, s, bc)
        r2, s2 = X.residual_coef_bc(ctx, v, f, a, n3, RG, s, bc)
        q1, d1 = X.apply_cap_dot(ctx, v, a, one, n3, RG, s, bc)
        q2, d2 = X.apply_coef_dot_bc(ctx, v, a, n3, RG, s, bc)
        assert bits_equal(X.cap_rhs(ctx, v, one, f, 0.3, s, n3, bc), X.shift_rhs_bc(ctx, v, f, 0.3, s, n3, bc))
    else:
        assert bits_equal(X.relax_cap(ctx, v, f, a, one, n3, RG, s, 2), X.relax_coef(ctx, v, f, a, n3, RG, s, 2))
        assert bits_equal(X.relax_cap_from_zero(ctx, v, f, a, one, n3, RG, s, 2, False), X.relax_coef_from_zero(ctx, v, f, a, n3, RG, s, 2, False))
        r1, s1 = X.residual_cap(ctx, v, f, a, one, n3, RG, s)
        r2, s2 = X.residual_coef(ctx, v, f, a, n3, RG, s)
        q1, d1 = X.apply_cap_dot(ctx, v, a, one, n3, RG, s)
        q2, d2 = X.apply_coef_dot(ctx, v, a, n3, RG, s)
        assert bits_equal(X.cap_rhs(ctx, v, one, f, 0.3, s, n3), X.shift_rhs(ctx, v, f, 0.3, s, n3))
    assert bits_equal(r1, r2) and s1 == s2 and bits_equal(q1, q2) and d1 == d2


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernels_reject_bad_shifts_and_sizes(ctx, dtype):
    n3 = (17, 17, 17)
    v, f, a, c = _rand(n3, dtype, 1), _rand(n3, dtype, 2), _coef(n3, dtype), _cap(n3, dtype)
    for s in (-1.0, float("nan"), float("inf")):
        with pytest.raises(P.MgxError) as e:
            P.ops3dxs.relax_cap(ctx, v, f, a, c, n3, RG, s, 1)
        assert e.value.status == P.MGX_ERR_INVALID and "shift" in str(e.value)
        with pytest.raises(P.MgxError) as e:
            P.ops3dxs.cap_rhs(ctx, v, c, None, 1.0, s, n3, 5)
        assert e.value.status == P.MGX_ERR_INVALID
    fn, ct = _fn("residual_cap_bc", dtype)
    buf = ctx.to_device(np.zeros(64))
    try:
        st = fn(ctx._h, buf, buf, buf, buf, buf, _ip((16, 17, 17)), _h(n3, dtype), ct(1.0), None, None, C.c_int(1))
        assert st == P.MGX_ERR_SIZE
    finally:
        ctx.free(buf)


# ---------------------------------------------------------------------------------------------------------- hierarchy
GRIDS = [((33, 33, 33), UNIT, "full"), ((65, 33, 17), RG, "full"), ((65, 33, 17), UNIT, "semi")]
HIER = [(g, bc) for g in range(len(GRIDS)) for bc in (0, 37, 63) if not (bc and GRIDS[g][2] == "semi")]  # (walls need full coarsening)
S_CYCLE = 100.0


def _faces(bc):
    return [(bc >> k) & 1 for k in range(6)]


def _mg(ctx, grid, bc, dtype, a, c, v=None, f=None, s=S_CYCLE):
    n3, rng, how = GRIDS[grid]
    mg = P.MultiGrid3D(ctx, n3, rng, dtype, residual_mode=P.CORRECT, coarsening=how, shift=s, coefficient=a, neumann=_faces(bc), capacity=c)
    if v is not None:
        mg.upload_v(0, v)
    if f is not None:
        mg.upload_f(0, f)
    return mg


def _restated(grid, bc, dtype, a, c, v, f, s=S_CYCLE):
    n3, rng, how = GRIDS[grid]
    H = OP.Hierarchy(OP.Op(n3, rng, dtype, s, a, c, bc), how)
    H.v[0], H.f[0] = v.copy(), f.copy()
    return H


def _same_levels(mg, H, what):
    assert mg.maxGrids == len(H.sizes) and mg.masks == H.masks
    for l, n in enumerate(H.sizes):
        assert mg.size(l) == n
        assert bits_equal(mg.download_v(l), H.v[l]), (what, "v", l)
        assert bits_equal(mg.download_capacity(l), H.c[l]) and bits_equal(mg.download_coefficient(l), H.a[l]), (what, "c / a", l)
        if l > 0:
            assert bits_equal(mg.download_f(l), H.f[l]), (what, "f", l)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("grid,bc", HIER)
def test_cycles_eager_and_replayed_match_the_restated_cycle(ctx, grid, bc, dtype):
    """two V(2,2) eagerly, then three through use_graph, the last of them a replay: the restated hierarchy after every cycle, every
    level, the capacity arrays included"""
    n3 = GRIDS[grid][0]
    v, f, a, c = _rand(n3, dtype, 1), _rand(n3, dtype, 2), _coef(n3, dtype), _cap(n3, dtype)
    H = _restated(grid, bc, dtype, a, c, v, f)
    mg = _mg(ctx, grid, bc, dtype, a, c, v=v, f=f)
    assert mg.has_capacity and mg.has_coefficient and mg.shift == S_CYCLE
    execs = []
    for k in range(5):
        mg.use_graph = k >= 2
        mg.VCycle(0, 2, 2)
        H.vcycle(0, 2, 2)
        _same_levels(mg, H, "cycle %d" % k)
        execs.append(mg._mg.contents.graph_exec[0])
    assert ctx.last_relax_kernel().startswith("relax_cap3d_xs_kernel"), ctx.last_relax_kernel()
    assert not execs[1] and execs[4] and execs[4] == execs[3], "the last cycle was captured again instead of replayed"
    mg.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("grid,bc", HIER)
def test_fmg_matches_the_restated_cycle(ctx, grid, bc, dtype):
    n3 = GRIDS[grid][0]
    v, f, a, c = _rand(n3, dtype, 5), _rand(n3, dtype, 6), _coef(n3, dtype), _cap(n3, dtype)
    H = _restated(grid, bc, dtype, a, c, v, f)
    H.fmg(0, 1, 2, 2)
    for graph in (False, True):
        mg = _mg(ctx, grid, bc, dtype, a, c, v=v, f=f)
        mg.use_graph = graph
        mg.FullMultiGridVCycle(0, 1, 2, 2)
        _same_levels(mg, H, "fmg graph=%s" % graph)
        mg.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("grid,bc", HIER)
def test_capacity_replaced_and_cleared_between_cycles(ctx, grid, bc, dtype):
    """through use_graph: new values reuse the arrays and are what the next cycle reads; cleared, the hierarchy gives the bits of
    one that never had a capacity; every change drops the captured graphs"""
    n3, rng, how = GRIDS[grid]
    v, f, a = _rand(n3, dtype, 1), _rand(n3, dtype, 2), _coef(n3, dtype)
    c1, c2 = _cap(n3, dtype), _cap(n3, dtype, 201)
    mg = _mg(ctx, grid, bc, dtype, a, c1, v=v, f=f)
    mg.use_graph = True
    mg.VCycle(0, 2, 2)
    assert mg._mg.contents.graph_exec[0]
    rec = bytes(mg._mg.contents.graph_rec[0])
    table = mg._mg.contents.cap
    mg.set_capacity(c2)
    assert mg._mg.contents.cap == table and not mg._mg.contents.graph_exec[0], "replacing kept a captured graph"
    mg.upload_v(0, v)
    mg.VCycle(0, 2, 2)
    H = _restated(grid, bc, dtype, a, c2, v, f)
    H.vcycle(0, 2, 2)
    _same_levels(mg, H, "replaced")
    mg.set_capacity(None)
    assert not mg.has_capacity and not mg._mg.contents.graph_exec[0]
    with pytest.raises(P.MgxError) as e:
        mg.download_capacity(0)
    assert e.value.status == P.MGX_ERR_INVALID
    mg.upload_v(0, v)
    mg.VCycle(0, 2, 2)
    assert bytes(mg._mg.contents.graph_rec[0]) != rec, "the record does not hold the capacity"
    assert "coef" in ctx.last_relax_kernel(), ctx.last_relax_kernel()
    never = P.MultiGrid3D(ctx, n3, rng, dtype, residual_mode=P.CORRECT, coarsening=how, shift=S_CYCLE, coefficient=a, neumann=_faces(bc))
    never.upload_v(0, v)
    never.upload_f(0, f)
    never.VCycle(0, 2, 2)
    for l in range(mg.maxGrids):
        assert bits_equal(mg.download_v(l), never.download_v(l)), ("cleared", l)
        if l:
            assert bits_equal(mg.download_f(l), never.download_f(l)), ("cleared f", l)
    never.close()
    mg.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bc", [0, 37])
def test_relax_residual_and_norm_through_the_hierarchy(ctx, bc, dtype):
    n3, rng, _ = GRIDS[1]
    s = 0.75
    v, f, a, c = _rand(n3, dtype, 7), _rand(n3, dtype, 8), _coef(n3, dtype), _cap(n3, dtype)
    mg = _mg(ctx, 1, bc, dtype, a, c, v=v, f=f, s=s)
    mg.Relax(0, 3)
    want = OP.Op(n3, rng, dtype, s, a, c, bc).relax(v, f, 3)
    assert bits_equal(mg.download_v(0), want)
    r = OP.Op(n3, rng, dtype, s, a, c, bc).residual(want, f)
    assert bits_equal(mg.CalculateResidual(0), r)
    assert close(mg.ResidualNorm(0), math.sqrt(OP.fsum_sq(r)), 1e-12)
    mg.close()


# ---------------------------------------------------------------------------------------------------------- solves
PCG_N = (33, 33, 33)


@pytest.fixture(scope="module")
def pcg_problem():
    n3 = PCG_N
    f = _rand(n3, np.float64, 5)
    v0 = np.zeros_like(f)
    v0[boundary_mask(n3)] = _rand(n3, np.float64, 9)[boundary_mask(n3)]  # Dirichlet data where a face is no wall
    return OC.smooth_coefficient(n3), OC.block_capacity(n3, 100, 1), f, v0


@pytest.mark.parametrize("krylov,bc", [(False, 0), (True, 0), ("weighted", 0), (False, 37), ("weighted", 37), ("weighted", 63)])
def test_pcg_matches_the_restatement(ctx, pcg_problem, krylov, bc):
    """smooth a, c = 100 in the centred block, s = 100: the restatement's iteration count.  The device sums differ from fsum in the
    last bits, so the tolerance is one the restated history keeps a factor 1.5 from on both sides of the deciding iteration:
    1e-10 with walls, 5e-11 without (there the restatement passes 1.08e-10 and 1.29e-10 on its way)"""
    n3, s, tol = PCG_N, 100.0, (1e-10 if bc else 5e-11)
    a, c, f, v0 = pcg_problem
    if krylov:
        _, want_k, hist, want_c, _ = OP.fcg(OP.Op(n3, UNIT, np.float64, s, a, c, bc), v0, f, tol=tol, maxit=60)[:5]
    else:
        H = OP.Hierarchy(OP.Op(n3, UNIT, np.float64, s, a, c, bc))
        H.v[0], H.f[0] = v0.copy(), f.copy()
        rr0, hist = OP.fsum_sq(H.residual(0)), []
        while not hist or (hist[-1] >= tol and len(hist) < 60):
            H.vcycle(0, 2, 2)
            hist.append(math.sqrt(OP.fsum_sq(H.residual(0)) / rr0))
        want_k, want_c = len(hist), hist[-1] < tol
    assert want_c and OC.decisive(hist, tol), hist[-2:]
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, shift=s, coefficient=a, neumann=_faces(bc), capacity=c)
    mg.upload_v(0, v0)
    mg.upload_f(0, f)
    k, rel, conv, _ = mg.PCG(2, 2, tol, 60, krylov=krylov)
    x = mg.download_v(0)
    assert bits_equal(mg.download_f(0), f), "d_f[0] was not restored"
    mg.close()
    unk = OP.unknown_mask(n3, bc)
    op = OP.Op(n3, UNIT, np.float64, s, a, c, bc)
    true_rel = math.sqrt(OP.fsum_sq(op.residual(x, f)) / OP.fsum_sq(op.residual(v0, f)))
    print("PCG krylov=%s bc=%d: %d iterations (restated %d), rel %.3e, restated residual of the result %.3e" % (krylov, bc, k, want_k, rel, true_rel))
    assert k == want_k and conv
    assert rel < tol and true_rel < tol and close(rel, true_rel, 1e-6)
    assert bits_equal(x[~unk], v0[~unk]), "the Dirichlet data changed"
    if krylov is True:
        x2, k2, rel2, conv2 = P.solve3d_pcg(ctx, v0, f, UNIT, tol=tol, krylov=True, shift=s, coefficient=a, capacity=c)
        assert (k2, conv2) == (k, conv) and bits_equal(x2, x)


@pytest.mark.parametrize("krylov", [False, "weighted"])
def test_backward_euler_in_a_closed_box_keeps_the_heat_content(ctx, krylov):
    """17^3, all six faces walls, smooth a, c jumping by 100, five steps of c u_t = div(a grad u) with kappa dt = 1e-2 to 1e-10: the
    first step's right-hand side is the restated one, and sum(w c u) drifts by less than 1e-9 (relative)"""
    n3 = (17, 17, 17)
    a, c, u0 = OC.smooth_coefficient(n3), OC.block_capacity(n3, 100, 1), OC.gaussian(n3)
    W = OP.weights(n3, 63)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, coefficient=a, neumann=[1] * 6, capacity=c)
    mg.upload_v(0, u0)
    its, worst, conv = mg.BackwardEuler(1, 1e-2, 1.0, tol=1e-10, krylov=krylov)
    assert conv and mg.shift == 100.0
    assert bits_equal(mg.download_f(0), OP.Op(n3, UNIT, np.float64, 100.0, c=c, bc=63).rhs(u0, None, 1.0, f=mg.download_f(0)))
    its4, worst4, conv4 = mg.BackwardEuler(4, 1e-2, 1.0, tol=1e-10, krylov=krylov)
    u = mg.download_v(0)
    mg.close()
    heat0, heat = math.fsum((W * c * u0).ravel()), math.fsum((W * c * u).ravel())
    drift = abs(heat - heat0) / abs(heat0)
    print("closed box, krylov=%s: %d iterations, worst residual %.3e, drift of sum(w c u) %.3e" % (krylov, its + its4, max(worst, worst4), drift))
    assert conv4 and max(worst, worst4) < 1e-10 and np.abs(u - u0).max() > 1e-3
    assert drift < 1e-9, drift


# ---------------------------------------------------------------------------------------------------------- refusals
def _refused(call, *words):
    with pytest.raises(P.MgxError) as e:
        call()
    assert e.value.status == P.MGX_ERR_INVALID and all(w in str(e.value) for w in words), str(e.value)


def test_capacity_needs_a_coefficient(ctx):
    n3 = (17, 17, 17)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT)
    _refused(lambda: mg.set_capacity(_cap(n3, np.float64)), "set_coefficient")
    assert not mg.has_capacity
    mg.close()


def test_coefficient_cannot_be_cleared_under_a_capacity(ctx):
    n3 = (17, 17, 17)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, coefficient=_coef(n3, np.float64), capacity=_cap(n3, np.float64))
    _refused(lambda: mg.set_coefficient(None), "set_capacity")
    assert mg.has_coefficient and mg.has_capacity
    mg.set_capacity(None)
    mg.set_coefficient(None)
    assert not mg.has_coefficient
    mg.close()


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_bad_capacity_values_leave_the_hierarchy_as_it_was(ctx, bad):
    n3 = (17, 17, 17)
    good = _cap(n3, np.float64)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, coefficient=_coef(n3, np.float64))
    c = good.copy()
    c[0, 3, 5] = bad  # a boundary point: every point of level 0 is validated
    _refused(lambda: mg.set_capacity(c), "set_capacity")
    assert not mg.has_capacity
    mg.set_capacity(good)
    _refused(lambda: mg.set_capacity(c), "set_capacity")
    assert bits_equal(mg.download_capacity(0), good), "a rejected capacity changed the hierarchy"
    with pytest.raises(ValueError):
        mg.set_capacity(good[1:])
    mg.close()


def test_pcg_mixed_is_refused(ctx):
    n3 = (17, 17, 17)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, coefficient=_coef(n3, np.float64), capacity=_cap(n3, np.float64))
    _refused(lambda: mg.PCG(2, 2, 1e-8, 5, precond="f32"), "capacity")
    mg.close()


def test_closed_box_needs_a_zeroth_order_term(ctx):
    """all six faces walls: singular with s == 0 (as before) and with a capacity that has no positive entry, whatever s"""
    n3 = (17, 17, 17)
    a, v, f = _coef(n3, np.float64), _rand(n3, np.float64, 1), _rand(n3, np.float64, 2)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, shift=100.0, coefficient=a, neumann=[1] * 6, capacity=np.zeros(O.shape(n3)))
    mg.upload_v(0, v)
    mg.upload_f(0, f)
    for call in (lambda: mg.VCycle(0, 2, 2), lambda: mg.Relax(0, 1), lambda: mg.ResidualNorm(0), lambda: mg.PCG(2, 2, 1e-8, 5, krylov=False),
                 lambda: mg.PCG(2, 2, 1e-8, 5, krylov="weighted")):
        _refused(call, "capacity", "singular")
    mg.set_capacity(_cap(n3, np.float64))
    mg.VCycle(0, 2, 2)
    mg.shift = 0.0
    _refused(lambda: mg.VCycle(0, 2, 2), "shift = 0", "singular")
    mg.set_neumann([1, 1, 1, 1, 1, 0])  # a Dirichlet face: an all-zero capacity is the coefficient operator without a shift
    mg.set_capacity(np.zeros(O.shape(n3)))
    mg.upload_v(0, v)
    mg.VCycle(0, 2, 2)
    plain = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, coefficient=a, neumann=[1, 1, 1, 1, 1, 0])
    plain.upload_v(0, v)
    plain.upload_f(0, f)
    plain.VCycle(0, 2, 2)
    assert bits_equal(mg.download_v(0), plain.download_v(0))
    plain.close()
    mg.close()
