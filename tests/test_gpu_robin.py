"""Convective (Robin) and prescribed-flux walls on the GPU: the mgx3dxs_*_wall kernels and wall_rhs (csrc/mgx_wall3d.hip), the
hierarchy that carries the walls (MultiGrid3D(robin=, wall_flux=), set_wall, add_wall_flux) and the solves and implicit heat steps
on it.  DESIGN.md 18.

Every kernel is checked bit for bit against the numpy restatement of its arithmetic (tests/op_restated.py) with poisoned pads,
with all betas zero against the _bc entry on the same inputs too; the cycles against the restated cycle, every level, eager and
replayed from a graph; the solves against the restated iteration counts."""
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
from solve_restated import close

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]
UNIT = [0, 1, 0, 1, 0, 1]
DTYPES = [np.float64, np.float32]
# (21,13,29), (131,7,9): rows end inside a tile; (257,9,5): a row longer than a wave; the last three: the smallest grids, on which a
# face is a single point or a single line
SHAPES = [(17, 17, 17), (21, 13, 29), (131, 7, 9), (257, 9, 5), (3, 3, 3), (3, 5, 9), (5, 3, 3)]
MASKS = [1, 2, 12, 48, 37, 63]
SHIFTS = [0.0, 0.75]
KINDS = ["shift", "coef", "cap"]
# the parametrised cases: the larger shapes and the smallest ones (every shape runs with every mask inside its case)
SHAPE_GROUPS = [tuple(SHAPES[:2]), tuple(SHAPES[2:4]), tuple(SHAPES[4:])]
WORK_GUARD = 64


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
    c = OC.random_capacity(n3, dtype, seed)
    c[-1, 0, :] = 0  # zeros on face unknowns too
    return c


def _fn(name, dtype):
    s, ct = _ct(dtype)
    return getattr(P.lib, "mgx3dxs_%s_%s" % (name, s)), ct


def _h(n3, dtype):
    return _rp(grid_spacing(n3, RG, dtype), _ct(dtype)[1])


def _faces(bc):
    return [(bc >> k) & 1 for k in range(6)]


def _beta_sets(bc):
    """all zero; a mixed set that leaves some flagged faces at 0 (where the mask has more than one); 1e6 on every flagged face"""
    return [OP.ZERO, OC.mixed_betas(bc), tuple(1e6 * b for b in _faces(bc))]


def _operands(kind, n3, dtype):
    """(a, c) of the operator kind"""
    return (None if kind == "shift" else _coef(n3, dtype)), (_cap(n3, dtype) if kind == "cap" else None)


def _entry(base, kind, form):
    """the C entry of an operator kind: form = "wall" or "bc" """
    dot = {"shift": "laplace_dot_shift", "coef": "apply_coef_dot", "cap": "apply_cap_dot"}[kind]
    return {"relax": "relax_%s_%s" % (kind, form), "residual": "residual_%s_%s" % (kind, form), "dot": "%s_%s" % (dot, form)}[base]


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


# ---------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shapes", SHAPE_GROUPS)
def test_relax_wall(ctx, shapes, dtype):
    """every shape of the group with every mask (one case per group and precision: the suite's count of cases stays small)"""
    for n3 in shapes:
        for bc in MASKS:
            _relax_wall(ctx, n3, bc, dtype)


def _relax_wall(ctx, n3, bc, dtype):
    """1 and 3 sweeps of every operator, every beta set and shift: the restatement's bits (all betas zero: the _bc entry's too); f,
    a, c, the Dirichlet entries of v and the pads as they were"""
    v, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    dirichlet = ~OP.unknown_mask(n3, bc)
    for kind in KINDS:
        a, c = _operands(kind, n3, dtype)
        ops = [x for x in (a, c) if x is not None]
        for bi, beta in enumerate(_beta_sets(bc)):
            for s in SHIFTS:
                for sweeps in (1, 3):
                    want = OP.Op(n3, RG, dtype, s, a, c, bc, beta).relax(v, f, sweeps)
                    fn, ct = _fn(_entry("relax", kind, "wall"), dtype)
                    ups, outs = run_poisoned(ctx, [v, f] + ops, lambda x, b, *ac: fn(ctx._h, x, b, *ac, _ip(n3), _h(n3, dtype), ct(s),
                                                                                     C.c_int(sweeps), C.c_int(bc), _rp(beta, ct)), dtype)
                    got = xs_unpack(outs[0], n3[0])
                    assert bits_equal(got, want), (kind, beta, s, sweeps, np.argwhere(got != want)[:5])
                    assert bits_equal(got[dirichlet], v[dirichlet])
                    assert pads_unchanged(ups[0], outs[0], n3[0]) and _unchanged(ups, outs, range(1, 2 + len(ops))), (kind, beta, s)
                    if bi == 0:
                        fb, _ = _fn(_entry("relax", kind, "bc"), dtype)
                        _, outb = run_poisoned(ctx, [v, f] + ops, lambda x, b, *ac: fb(ctx._h, x, b, *ac, _ip(n3), _h(n3, dtype), ct(s),
                                                                                       C.c_int(sweeps), C.c_int(bc)), dtype)
                        assert bits_equal(outb[0], outs[0]), (kind, s, sweeps)
                if bi and not np.isinf(want).any():
                    assert not bits_equal(want, OP.Op(n3, RG, dtype, s, a, c, bc).relax(v, f, 3)), "the wall changed nothing"
    # the Python wrapper, on a call of its own: the capacity operator, the mixed betas, three sweeps
    a, c = _operands("cap", n3, dtype)
    beta = OC.mixed_betas(bc)
    assert bits_equal(P.ops3dxs.relax_wall(ctx, v, f, a, c, n3, RG, 0.75, 3, bc, beta), OP.Op(n3, RG, dtype, 0.75, a, c, bc, beta).relax(v, f, 3))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shapes", SHAPE_GROUPS)
def test_residual_wall(ctx, shapes, dtype):
    """every shape of the group with every mask (one case per group and precision: the suite's count of cases stays small)"""
    for n3 in shapes:
        for bc in MASKS:
            _residual_wall(ctx, n3, bc, dtype)


def _residual_wall(ctx, n3, bc, dtype):
    """r and its sum of squares (against math.fsum to 1e-13, equal on two runs); the sum alone; r alone"""
    v, f, r0 = _rand(n3, dtype, 5), _rand(n3, dtype, 6), _rand(n3, dtype, 7)
    w = Work(ctx, n3, dtype)
    try:
        for kind in KINDS:
            a, c = _operands(kind, n3, dtype)
            ops = [x for x in (a, c) if x is not None]
            keep = range(0, 2 + len(ops))
            for bi, beta in enumerate(_beta_sets(bc)):
                for s in SHIFTS:
                    want = OP.Op(n3, RG, dtype, s, a, c, bc, beta).residual(v, f)
                    want_ss = OP.fsum_sq(want)
                    fn, ct = _fn(_entry("residual", kind, "wall"), dtype)
                    tail = (C.c_int(bc), _rp(beta, ct))
                    sums = []
                    for rep in range(2):
                        ups, outs = run_poisoned(ctx, [v, f] + ops + [r0], lambda x, b, *rest: fn(ctx._h, x, b, *rest, _ip(n3), _h(n3, dtype), ct(s),
                                                                                                 w.work, w.sum, *tail), dtype)
                        assert bits_equal(xs_unpack(outs[-1], n3[0]), want), (kind, beta, s)  # 0 at the Dirichlet points
                        assert _unchanged(ups, outs, keep) and pads_unchanged(ups[-1], outs[-1], n3[0]), (kind, beta, s)
                        sums.append(w.result())
                    assert sums[0] == sums[1], "two runs gave different sums"
                    assert close(sums[0], want_ss, 1e-13), (kind, beta, s, sums[0], want_ss)
                    ups, outs = run_poisoned(ctx, [v, f] + ops, lambda x, b, *rest: fn(ctx._h, x, b, *rest, None, _ip(n3), _h(n3, dtype), ct(s),
                                                                                       w.work, w.sum, *tail), dtype)
                    assert w.result() == sums[0] and _unchanged(ups, outs, keep)
                    ups, outs = run_poisoned(ctx, [v, f] + ops + [r0], lambda x, b, *rest: fn(ctx._h, x, b, *rest, _ip(n3), _h(n3, dtype), ct(s),
                                                                                             None, None, *tail), dtype)
                    assert bits_equal(xs_unpack(outs[-1], n3[0]), want) and pads_unchanged(ups[-1], outs[-1], n3[0])
                    if bi == 0:
                        fb, _ = _fn(_entry("residual", kind, "bc"), dtype)
                        _, outb = run_poisoned(ctx, [v, f] + ops + [r0], lambda x, b, *rest: fb(ctx._h, x, b, *rest, _ip(n3), _h(n3, dtype), ct(s),
                                                                                               w.work, w.sum, C.c_int(bc)), dtype)
                        assert bits_equal(outb[-1], outs[-1]) and w.result() == sums[0], (kind, s)
    finally:
        w.close()
    # the Python wrapper, on a call of its own: the capacity operator, the mixed betas
    a, c = _operands("cap", n3, dtype)
    beta = OC.mixed_betas(bc)
    want = OP.Op(n3, RG, dtype, 0.75, a, c, bc, beta).residual(v, f)
    r, ss = P.ops3dxs.residual_wall(ctx, v, f, a, c, n3, RG, 0.75, bc, beta)
    assert bits_equal(r, want) and close(ss, OP.fsum_sq(want), 1e-13)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shapes", SHAPE_GROUPS)
def test_apply_dot_wall(ctx, shapes, dtype):
    """every shape of the group with every mask (one case per group and precision: the suite's count of cases stays small)"""
    for n3 in shapes:
        for bc in MASKS:
            _apply_dot_wall(ctx, n3, bc, dtype)


def _apply_dot_wall(ctx, n3, bc, dtype):
    """q = A p at the unknowns and <p, q>_W"""
    p, q0 = _rand(n3, dtype, 8), _rand(n3, dtype, 9)
    unk = OP.unknown_mask(n3, bc)
    W = OP.weights(n3, bc)
    w = Work(ctx, n3, dtype)
    try:
        for kind in KINDS:
            a, c = _operands(kind, n3, dtype)
            ops = [x for x in (a, c) if x is not None]
            for bi, beta in enumerate(_beta_sets(bc)):
                for s in SHIFTS:
                    want = OP.Op(n3, RG, dtype, s, a, c, bc, beta).apply_A(p)
                    want_pq = OP.wdot(W, p, want)
                    fn, ct = _fn(_entry("dot", kind, "wall"), dtype)
                    sums = []
                    for rep in range(2):
                        ups, outs = run_poisoned(ctx, [p] + ops + [q0], lambda x, *rest: fn(ctx._h, x, *rest, _ip(n3), _h(n3, dtype), ct(s), w.work,
                                                                                           w.sum, C.c_int(bc), _rp(beta, ct)), dtype)
                        q = xs_unpack(outs[-1], n3[0])
                        assert bits_equal(q[unk], want[unk]), (kind, beta, s)
                        assert bits_equal(q[~unk], q0[~unk]), "a Dirichlet entry of q was written"
                        assert _unchanged(ups, outs, range(0, 1 + len(ops))) and pads_unchanged(ups[-1], outs[-1], n3[0]), (kind, beta, s)
                        sums.append(w.result())
                    assert sums[0] == sums[1], "two runs gave different sums"
                    assert close(sums[0], want_pq, 1e-13), (kind, beta, s, sums[0], want_pq)
                    if bi == 0:
                        fb, _ = _fn(_entry("dot", kind, "bc"), dtype)
                        _, outb = run_poisoned(ctx, [p] + ops + [q0], lambda x, *rest: fb(ctx._h, x, *rest, _ip(n3), _h(n3, dtype), ct(s), w.work,
                                                                                         w.sum, C.c_int(bc)), dtype)
                        assert bits_equal(outb[-1], outs[-1]) and w.result() == sums[0], (kind, s)
    finally:
        w.close()
    # the Python wrapper, on a call of its own: the capacity operator, the mixed betas
    a, c = _operands("cap", n3, dtype)
    beta = OC.mixed_betas(bc)
    want = OP.Op(n3, RG, dtype, 0.75, a, c, bc, beta).apply_A(p)
    q, pq = P.ops3dxs.apply_dot_wall(ctx, p, a, c, n3, RG, 0.75, bc, beta)
    assert bits_equal(q[unk], want[unk]) and close(pq, OP.wdot(W, p, want), 1e-13)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shapes", SHAPE_GROUPS)
def test_wall_rhs(ctx, shapes, dtype):
    """every shape of the group with every mask (one case per group and precision: the suite's count of cases stays small)"""
    for n3 in shapes:
        for bc in MASKS:
            _wall_rhs(ctx, n3, bc, dtype)


def _wall_rhs(ctx, n3, bc, dtype):
    """f -= 2 g / h at the face unknowns of the faces with a flux, nothing else of f; all zeros: f as it was"""
    f0 = _rand(n3, dtype, 12)
    fn, ct = _fn("wall_rhs", dtype)
    fluxes = [OP.ZERO, tuple(-x for x in OC.mixed_betas(bc)), tuple((-1) ** k * 1e6 * b for k, b in enumerate(_faces(bc)))]
    for g in fluxes:
        want = OP.Op(n3, RG, dtype, 0.0, bc=bc).add_flux(f0, g)
        ups, outs = run_poisoned(ctx, [f0], lambda x: fn(ctx._h, x, _ip(n3), _h(n3, dtype), _rp(g, ct), C.c_int(bc)), dtype)
        got = xs_unpack(outs[0], n3[0])
        assert bits_equal(got, want), (g, np.argwhere(got != want)[:5])
        assert pads_unchanged(ups[0], outs[0], n3[0])
        changed = got != f0
        assert (changed <= OP.face_unknowns(n3, bc)).all() and changed.any() == any(g), g
    # the Python wrapper, on a call of its own
    g = fluxes[1]
    assert bits_equal(P.ops3dxs.wall_rhs(ctx, f0, n3, RG, g, bc), OP.Op(n3, RG, dtype, 0.0, bc=bc).add_flux(f0, g))


# ---------------------------------------------------------------------------------------------------------- hierarchy
GRIDS = [((33, 33, 33), UNIT), ((65, 33, 17), RG)]
# (grid, mask, operator kind, s): s = 0 in the closed box, which a lossy wall makes regular
HIER = [(g, bc, kind, 0.0 if bc == 63 else 0.75) for g in (0, 1) for bc in (37, 63) for kind in ("shift", "coef")] + [(1, 63, "cap", 0.0)]


# ... and the rows of the test that clears the walls again: a shift everywhere, so that the closed box without a wall is regular
# too and can be compared level by level -- the rows of HIER with a shift, and the closed box shifted, with the coefficient and
# with the capacity
CLEARED = [h for h in HIER if h[3]] + [(0, 63, "shift", 0.75), (1, 63, "coef", 0.75), (1, 63, "cap", 0.75), (0, 63, "cap", 0.75)]


def _problem(grid, kind, dtype):
    n3 = GRIDS[grid][0]
    a = None if kind == "shift" else OC.smooth_coefficient(n3, dtype)
    c = _cap(n3, dtype) if kind == "cap" else None
    return _rand(n3, dtype, 1), _rand(n3, dtype, 2), a, c


def _mg(ctx, grid, bc, dtype, a, c, s, beta, g=None, v=None, f=None):
    n3, rng = GRIDS[grid]
    mg = P.MultiGrid3D(ctx, n3, rng, dtype, residual_mode=P.CORRECT, shift=s, coefficient=a, neumann=_faces(bc), capacity=c, robin=beta,
                       wall_flux=g)
    if v is not None:
        mg.upload_v(0, v)
    if f is not None:
        mg.upload_f(0, f)
    return mg


def _restated(grid, bc, dtype, a, c, s, beta, g, v, f):
    n3, rng = GRIDS[grid]
    H = OP.Hierarchy(OP.Op(n3, rng, dtype, s, a, c, bc, beta), g=g or OP.ZERO)
    H.v[0], H.f[0] = v.copy(), f.copy()
    return H


def _same_levels(mg, H, what, f0=False):
    assert mg.maxGrids == len(H.sizes)
    for l, n in enumerate(H.sizes):
        assert mg.size(l) == n
        assert bits_equal(mg.download_v(l), H.v[l]), (what, "v", l)
        if l > 0 or f0:
            assert bits_equal(mg.download_f(l), H.f[l]), (what, "f", l)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cycles_eager_and_replayed_match_the_restated_cycle(ctx, dtype):
    for grid, bc, kind, s in HIER:
        _cycles_eager_and_replayed_match_the_restated_cycle(ctx, grid, bc, kind, s, dtype)


def _cycles_eager_and_replayed_match_the_restated_cycle(ctx, grid, bc, kind, s, dtype):
    """two V(2,2) eagerly, then three through use_graph (a capture and two runs, the last a replay): the restated hierarchy after
    every cycle, every level"""
    v, f, a, c = _problem(grid, kind, dtype)
    beta = OC.mixed_betas(bc)
    H = _restated(grid, bc, dtype, a, c, s, beta, None, v, f)
    mg = _mg(ctx, grid, bc, dtype, a, c, s, beta, v=v, f=f)
    assert mg.wall == (tuple(float(_ct(dtype)[1](b).value) for b in beta), OP.ZERO)
    execs = []
    for k in range(5):
        mg.use_graph = k >= 2
        mg.VCycle(0, 2, 2)
        H.vcycle(0, 2, 2)
        _same_levels(mg, H, "cycle %d" % k)
        execs.append(mg._mg.contents.graph_exec[0])
    assert not execs[1] and execs[4] and execs[4] == execs[3], "the last cycle was captured again instead of replayed"
    r = H.residual(0)
    assert bits_equal(mg.CalculateResidual(0), r) and close(mg.ResidualNorm(0), math.sqrt(OP.fsum_sq(r)), 1e-12)
    mg.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_fmg_with_a_flux_matches_the_restated_cycle(ctx, dtype):
    for grid, bc, kind, s in HIER:
        _fmg_with_a_flux_matches_the_restated_cycle(ctx, grid, bc, kind, s, dtype)


def _fmg_with_a_flux_matches_the_restated_cycle(ctx, grid, bc, kind, s, dtype):
    """add_wall_flux, then FMG(1,2,2): f of level 0 included"""
    v, f, a, c = _problem(grid, kind, dtype)
    beta, g = OC.mixed_betas(bc), tuple((0.5 - 0.3 * k) if (bc >> k) & 1 else 0.0 for k in range(6))
    H = _restated(grid, bc, dtype, a, c, s, beta, g, v, f)
    H.add_wall_flux()
    assert not bits_equal(H.f[0], f)
    H.fmg(0, 1, 2, 2)
    for graph in (False, True):
        mg = _mg(ctx, grid, bc, dtype, a, c, s, beta, g, v=v, f=f)
        mg.use_graph = graph
        mg.add_wall_flux()
        mg.FullMultiGridVCycle(0, 1, 2, 2)
        _same_levels(mg, H, "fmg graph=%s" % graph, f0=True)
        mg.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_walls_set_between_cycles_and_cleared(ctx, dtype):
    for grid, bc, kind, s in CLEARED:
        _walls_set_between_cycles_and_cleared(ctx, grid, bc, kind, s, dtype)


def _walls_set_between_cycles_and_cleared(ctx, grid, bc, kind, s, dtype):
    """through use_graph: set_wall drops the captured graph and the next cycle runs with the new betas; with zeros the hierarchy
    gives the bits of one that never had a wall"""
    v, f, a, c = _problem(grid, kind, dtype)
    b1, b2 = OC.mixed_betas(bc), tuple(2.5 * b for b in _faces(bc))
    mg = _mg(ctx, grid, bc, dtype, a, c, s, b1, v=v, f=f)
    mg.use_graph = True
    mg.VCycle(0, 2, 2)
    assert mg._mg.contents.graph_exec[0] and mg._mg.contents.wall
    mg.set_wall(b2, None)
    assert not mg._mg.contents.graph_exec[0], "set_wall kept a captured graph"
    mg.upload_v(0, v)
    mg.VCycle(0, 2, 2)
    H = _restated(grid, bc, dtype, a, c, s, b2, None, v, f)
    H.vcycle(0, 2, 2)
    _same_levels(mg, H, "replaced")
    mg.set_wall(None, None)
    assert not mg._mg.contents.wall and not mg._mg.contents.graph_exec[0] and mg.wall == (OP.ZERO, OP.ZERO)
    mg.upload_v(0, v)
    mg.VCycle(0, 2, 2)
    never = _mg(ctx, grid, bc, dtype, a, c, s, None, v=v, f=f)
    assert not never._mg.contents.wall
    never.use_graph = True
    never.VCycle(0, 2, 2)
    for l in range(mg.maxGrids):
        assert bits_equal(mg.download_v(l), never.download_v(l)), ("cleared", l)
        if l:
            assert bits_equal(mg.download_f(l), never.download_f(l)), ("cleared f", l)
    never.close()
    mg.close()


# ---------------------------------------------------------------------------------------------------------- solves
PCG_N = (17, 17, 17)
# (mask, s, smooth coefficient?, betas, krylov, tol): tolerances the restated history keeps a factor 1.5 from on both sides of the
# deciding iteration (the device sums differ from fsum in the last bits); the second and third rows: the closed box without a shift
PCG_CASES = [(37, 0.0, True, (3, 0, 10, 0, 0, 0.5), False, 1e-10), (37, 0.0, True, (3, 0, 10, 0, 0, 0.5), "weighted", 5e-10),
             (63, 0.0, False, (1, 0, 0, 0, 0, 0), "weighted", 1.4e-10), (63, 0.0, True, (5, 0, 0, 0, 0, 2), False, 1e-10),
             (63, 0.0, True, (5, 0, 0, 0, 0, 2), "weighted", 1e-10)]


def pcg_restated(case):
    """(iterations, converged, history) of the restatement, the start and the operands"""
    bc, s, coef, beta, krylov, tol = PCG_CASES[case]
    n3 = PCG_N
    g = np.random.default_rng(5)
    f, v0 = g.uniform(-1, 1, O.shape(n3)), g.uniform(-1, 1, O.shape(n3))
    a = OC.smooth_coefficient(n3) if coef else None
    if krylov:
        _, k, hist, conv, _ = OP.fcg(OP.Op(n3, UNIT, np.float64, s, a, bc=bc, beta=beta), v0, f, tol=tol, maxit=60)[:5]
    else:
        H = OP.Hierarchy(OP.Op(n3, UNIT, np.float64, s, a, bc=bc, beta=beta))
        H.v[0], H.f[0] = v0.copy(), f.copy()
        rr0, hist = OP.fsum_sq(H.residual(0)), []
        while not hist or (hist[-1] >= tol and len(hist) < 60):
            H.vcycle(0, 2, 2)
            hist.append(math.sqrt(OP.fsum_sq(H.residual(0)) / rr0))
        k, conv = len(hist), hist[-1] < tol
    return k, conv, list(hist), a, v0, f


def test_pcg_matches_the_restatement(ctx):
    for case in range(len(PCG_CASES)):
        _pcg_matches_the_restatement(ctx, case)


def _pcg_matches_the_restatement(ctx, case):
    bc, s, coef, beta, krylov, tol = PCG_CASES[case]
    n3 = PCG_N
    want_k, want_c, hist, a, v0, f = pcg_restated(case)
    assert want_c and OC.decisive(hist, tol), hist[-2:]
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, shift=s, coefficient=a, neumann=_faces(bc), robin=beta)
    mg.upload_v(0, v0)
    mg.upload_f(0, f)
    k, rel, conv, _ = mg.PCG(2, 2, tol, 60, krylov=krylov)
    x = mg.download_v(0)
    assert bits_equal(mg.download_f(0), f), "d_f[0] was not restored"
    assert mg.pcg_removed_mean == 0.0 and mg._mg.contents.bc_reserved == 0
    mg.close()
    unk = OP.unknown_mask(n3, bc)
    res = lambda u: OP.fsum_sq(OP.Op(n3, UNIT, np.float64, s, a, bc=bc, beta=beta).residual(u, f))
    true_rel = math.sqrt(res(x) / res(v0))
    print("PCG case %d: %d iterations (restated %d), rel %.3e, restated residual of the result %.3e" % (case, k, want_k, rel, true_rel))
    assert k == want_k and conv
    assert rel < tol and true_rel < tol and close(rel, true_rel, 1e-6)
    assert bits_equal(x[~unk], v0[~unk]), "the Dirichlet data changed"


def test_the_constant_state_is_the_solution(ctx):
    """mask 63, s = 0, f = 0, g = 7 beta: u = 7, found by solve3d_pcg (which folds the flux into its right-hand side) to 1e-10 from a
    zero guess.  The bound on the error: r0 = the flux terms, 2 * 7 beta / h <= 14 * 4 * 16 on fewer than 6 * 17^2 points, so
    |r0| < 4e4 and |r| < 4e-6; the operator's smallest eigenvalue in the weighted product is that of a box losing heat through
    walls with beta >= 0.25, above 0.25 (the Rayleigh quotient of the constant is sum_W(d) / sum(W) > 1), and the weights are at
    least 1/8: max |u - 7| <= 8 * 4e-6 / 0.25 < 2e-4."""
    n3, beta = (17, 17, 17), (1.0, 0.5, 0.25, 2.0, 0.25, 4.0)
    g = tuple(7 * b for b in beta)
    zero = np.zeros(O.shape(n3))
    for coef in (None, OC.smooth_coefficient(n3)):
        u, k, rel, conv = P.solve3d_pcg(ctx, zero, zero, UNIT, tol=1e-10, krylov="weighted", coefficient=coef, neumann=[1] * 6, robin=beta,
                                        wall_flux=g)
        err = float(np.abs(u - 7).max())
        print("constant state: %d iterations, rel %.3e, max |u - 7| = %.3e" % (k, rel, err))
        assert conv and rel < 1e-10 and err < 2e-4
    # ... and it is a fixed point of the cycle: the residual at u = 7 is exactly 0
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, neumann=[1] * 6, robin=beta, wall_flux=g)
    mg.upload_v(0, zero + 7)
    mg.upload_f(0, zero)
    mg.add_wall_flux()
    assert not mg.CalculateResidual(0).any() and mg.ResidualNorm(0) == 0.0
    mg.close()


def test_one_backward_euler_step_solves_its_own_system(ctx):
    for cap in (False, True):
        for krylov in (False, "weighted"):
            _one_backward_euler_step(ctx, cap, krylov)


def _one_backward_euler_step(ctx, cap, krylov):
    """the step's right-hand side is the restated one, flux included, and u' solves (A - s c - d) u' = rhs to the tolerance"""
    n3, dt, kappa = (17, 17, 17), 1e-2, 2.0
    beta, g = (2.0, 0.0, 0.5, 0.0, 0.0, 1.0), (0.0, 1.5, 0.0, 0.0, -0.5, 1.0)
    a, c, u0, q = OC.smooth_coefficient(n3), (OC.smooth_capacity(n3) if cap else None), OC.gaussian(n3), _rand(n3, np.float64, 3)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, coefficient=a, neumann=[1] * 6, capacity=c, robin=beta, wall_flux=g)
    mg.upload_v(0, u0)
    its, worst, conv = mg.BackwardEuler(1, dt, kappa, source=q, tol=1e-10, krylov=krylov)
    s = 1.0 / (kappa * dt)
    assert conv and worst < 1e-10 and mg.shift == s
    rhs = OP.Op(n3, UNIT, np.float64, s, c=c, bc=63).rhs(u0, q, 1.0 / kappa) if cap else OP.Op(n3, UNIT, np.float64, s, bc=63).rhs(u0, q, 1.0 / kappa)
    rhs = OP.Op(n3, UNIT, np.float64, 0.0, bc=63).add_flux(rhs, g)
    assert bits_equal(mg.download_f(0), rhs)
    u = mg.download_v(0)
    mg.close()
    res = lambda x: OP.fsum_sq(OP.Op(n3, UNIT, np.float64, s, a, c, 63, beta).residual(x, rhs))
    rel = math.sqrt(res(u) / res(u0))
    print("one step, cap=%s krylov=%s: %d iterations, rel %.3e (restated %.3e)" % (cap, krylov, its, worst, rel))
    assert rel < 1e-10 and np.abs(u - u0).max() > 1e-3


def test_heat_balance_in_a_closed_box(ctx):
    for krylov in (False, "weighted"):
        _heat_balance_in_a_closed_box(ctx, krylov)


def _heat_balance_in_a_closed_box(ctx, krylov):
    """five steps of test_robin_cpu's closed 17^3 box with a capacity: per step the change of sum_W(c u) is kappa dt times the
    weighted sum of the wall terms of the new u, to ten times the bound the restatement meets on the CPU (op_cases.heat_bound)"""
    k = OC.HEAT_CASE
    n3 = k["n3"]
    c = OC.smooth_capacity(n3)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, coefficient=OC.smooth_coefficient(n3), neumann=[1] * 6, capacity=c, robin=k["beta"],
                       wall_flux=k["g"])
    us = [OC.gaussian(n3)]
    mg.upload_v(0, us[0])
    for _ in range(k["steps"]):
        its, worst, conv = mg.BackwardEuler(1, k["dt"], k["kappa"], tol=1e-10, krylov=krylov)
        assert conv and worst < 1e-10
        us.append(mg.download_v(0))
    mg.close()
    worst, heat = OC.heat_balance(n3, c, us, k["beta"], k["g"], k["dt"], k["kappa"])
    bound = 10 * OC.heat_bound(n3, OC.smooth_coefficient(n3), c, us, k["beta"], k["g"], k["dt"], k["kappa"], 1e-10)
    print("closed box, krylov=%s: worst relative imbalance of a step %.3e (bound %.1e), heat %.6e -> %.6e" % (krylov, worst, bound,
                                                                                                             heat[0], heat[-1]))
    assert abs(heat[-1] - heat[0]) > 1e-4 * abs(heat[0])
    assert worst <= bound, worst


# ---------------------------------------------------------------------------------------------------------- refusals
def _refused(call, *words):
    with pytest.raises(P.MgxError) as e:
        call()
    assert e.value.status == P.MGX_ERR_INVALID and all(w in str(e.value) for w in words), str(e.value)


def test_refusals_leave_the_hierarchy_usable(ctx):
    n3, bc, beta = (17, 17, 17), 37, (3.0, 0, 10.0, 0, 0, 0.5)
    v, f = _rand(n3, np.float64, 1), _rand(n3, np.float64, 2)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, shift=0.75, neumann=_faces(bc), robin=beta)
    mg.upload_v(0, v)
    mg.upload_f(0, f)
    H = OP.Hierarchy(OP.Op(n3, UNIT, np.float64, 0.75, bc=bc, beta=beta))
    H.v[0], H.f[0] = v.copy(), f.copy()
    for call, words in [(lambda: mg.set_wall((-1, 0, 0, 0, 0, 0), None), ("beta",)),
                        (lambda: mg.set_wall((float("nan"), 0, 0, 0, 0, 0), None), ("beta",)),
                        (lambda: mg.set_wall(None, (float("inf"), 0, 0, 0, 0, 0)), ("g[",)),
                        (lambda: mg.set_wall((0, 1, 0, 0, 0, 0), None), ("mask",)),
                        (lambda: mg.set_wall(None, (0, 0, 0, 2, 0, 0)), ("mask",)),
                        (lambda: mg.set_neumann([0, 0, 1, 0, 0, 1]), ("set_wall",)),
                        (lambda: mg.PCG(2, 2, 1e-8, 5, krylov=True), ("krylov",)),
                        (lambda: mg.PCG(2, 2, 1e-8, 5, precond="f32"), ("wall",)),
                        (lambda: mg.BackwardEuler(1, 1e-2, 1.0, krylov=True), ("krylov",))]:
        _refused(call, *words)
        assert mg.wall == (tuple(float(b) for b in beta), OP.ZERO) and mg.neumann == tuple(bool(b) for b in _faces(bc))
    with pytest.raises(ValueError):
        mg.set_wall((1, 2, 3), None)
    mg.VCycle(0, 2, 2)
    H.vcycle(0, 2, 2)
    _same_levels(mg, H, "after the refusals")
    mg.set_wall((3.0, 0, 10.0, 0, 0, 0), None)  # the face to be cleared carries nothing any more
    mg.set_neumann([1, 0, 1, 0, 0, 0])
    mg.close()


def test_the_mask_still_refuses_what_it_refused(ctx):
    """a semi-coarsened hierarchy takes no mask, so no wall either; the closed box with s = 0 stays singular until a beta > 0"""
    n3 = (17, 17, 17)
    semi = P.MultiGrid3D(ctx, (65, 33, 17), RG, residual_mode=P.CORRECT, coarsening="semi")
    _refused(lambda: semi.set_neumann([1, 0, 0, 0, 0, 0]), "semi")
    _refused(lambda: semi.set_wall((1, 0, 0, 0, 0, 0), None), "mask")
    semi.VCycle(0, 2, 2)
    semi.close()
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, neumann=[1] * 6, wall_flux=(1, 0, 0, 0, 0, 0))
    mg.upload_f(0, _rand(n3, np.float64, 2))
    for call in (lambda: mg.VCycle(0, 2, 2), lambda: mg.Relax(0, 1), lambda: mg.ResidualNorm(0), lambda: mg.PCG(2, 2, 1e-8, 5, krylov=False)):
        _refused(call, "singular")  # a flux alone loses no heat
    mg.set_wall((0, 0, 0, 0.5, 0, 0), (1, 0, 0, 0, 0, 0))
    mg.VCycle(0, 2, 2)
    assert mg.ResidualNorm(0) > 0
    mg.set_wall(None, None)
    _refused(lambda: mg.VCycle(0, 2, 2), "singular")
    mg.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_wall_data_too_large_for_the_precision_are_refused(ctx, dtype):
    """2 beta / h and 2 g / h have to be finite in the hierarchy's precision on every level: the largest finite number is refused by
    set_wall (and by the kernels' entries: test_robin_cpu.py), the hierarchy stays as it was"""
    big = float(np.finfo(dtype).max)
    mg = P.MultiGrid3D(ctx, (17, 17, 17), UNIT, dtype, residual_mode=P.CORRECT, shift=0.75, neumann=[1, 0, 0, 0, 0, 0], robin=(2, 0, 0, 0, 0, 0))
    _refused(lambda: mg.set_wall((big, 0, 0, 0, 0, 0), None), "beta", "not finite in this precision")
    _refused(lambda: mg.set_wall(None, (-big, 0, 0, 0, 0, 0)), "g[", "not finite in this precision")
    assert mg.wall == ((2.0, 0, 0, 0, 0, 0), OP.ZERO)
    mg.set_wall((big / 64, 0, 0, 0, 0, 0), None)  # 2 beta / h with h = 1/16 on level 0 is finite, on every coarser level too
    mg.VCycle(0, 1, 1)
    assert np.isfinite(mg.download_v(0)).all()
    mg.close()
