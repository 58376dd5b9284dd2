"""GPU suite: pinned interior nodes (csrc/mgx_pin3d.hip) against the restatement tests/pin_restated.py.

The list kernel alone (every other entry of the stored array, pads included, untouched bit for bit; a list longer than one launch
covers), the smoother entries with a pin list for every operator with and without walls, the hierarchy's calls bit for bit against
PinHierarchy on x-rows that end inside a tile and on non-cubic grids, the solves, graphs against eager runs, a hierarchy without
pins against one that never heard of them, and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import op_restated as R
import oracle as O
import pde_multigrid_amd as P
import pin_restated as PR
from conftest import bits_equal
from odd_shapes import bits, run_poisoned
from pde_multigrid_amd.multigrid import _ct

pytestmark = pytest.mark.gpu
UNIT = [0, 1, 0, 1, 0, 1]
RG = [-1, 1, 0, 2, 0.5, 3]
DTYPES = [np.float64, np.float32]
SHAPES = [(9, 9, 9), (33, 17, 9), (9, 9, 65), (17, 33, 17)]
FACES = lambda bc: [bool((bc >> k) & 1) for k in range(6)]
WALL_BC, WALL_BETA = 0b100101, (0.0, 0.0, 1.5, 0.0, 0.0, 0.0)  # x-low and z-high insulated, y-low convective


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


def _rand(n3, dtype, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, O.shape(n3)).astype(dtype)


def _rng(n3):
    return UNIT if len(set(n3)) == 1 else RG


def _sets(n3):
    """the pinned sets of the issue: one red point, one black point, the first and last storage positions of a row, a plate on an
    odd plane, a ball, the complement of a ball"""
    sx, sy, sz = n3
    ends = PR.point(n3, (1, sy // 2, sz // 2)) | PR.point(n3, (sx - 2, sy // 2, sz // 2)) | PR.point(n3, (2, 1, 1)) | PR.point(n3, (sx - 3, 1, 1))
    return {"red": PR.point(n3, (2, 3, 3)), "black": PR.point(n3, (2, 3, 4)), "row ends": ends, "odd plate": PR.plate(n3, (sz // 2) | 1),
            "ball": PR.ball(n3), "outside": PR.outside_ball(n3)}


SETS = list(_sets((9, 9, 9)))


# ------------------------------------------------------------------------------------------ the list kernel alone
def _put_case(ctx, n3, mask, dtype, first, count, with_values):
    v, g = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    idx, val, end = P.ops3dxs.pin_list(n3, mask, g, dtype)
    fn = getattr(P.lib, "mgx3dxs_pin_put_" + _ct(dtype)[0])
    di, dv = ctx.to_device(idx), ctx.to_device(val)
    try:
        ups, outs = run_poisoned(ctx, [v], lambda a: fn(ctx._h, a, di, dv if with_values else None, C.c_uint(first), C.c_uint(count)), dtype)
    finally:
        ctx.free(di)
        ctx.free(dv)
    want = ups[0].copy().ravel()
    sel = idx[first:first + count].astype(np.int64)
    want[sel] = val[first:first + count] if with_values else 0
    return np.array_equal(bits(outs[0].ravel()), bits(want)), end


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", [(9, 9, 9), (33, 17, 9)])
def test_pin_put_counts(ctx, n3, dtype):
    """ranges of 0, 1, 63, 64, 65 and 257 entries, from the start, from inside the red part and across the colours: the listed
    entries hold the values (or zeros), every other entry of the stored array, pads included, keeps its bits"""
    mask = PR.random_set(n3, 0.95, seed=3)
    end = P.ops3dxs.pin_list(n3, mask, None, dtype)[2]
    assert end[1] >= 257 + 70 and 0 < end[0] < end[1]
    for count in (0, 1, 63, 64, 65, 257):
        for first in (0, 7, end[0] - 1, end[1] - count):
            if first + count > end[1]:
                continue
            for with_values in (True, False):
                ok, _ = _put_case(ctx, n3, mask, dtype, first, count, with_values)
                assert ok, (count, first, with_values)
    for first, count in ((0, end[0]), (end[0], end[1] - end[0]), (0, end[1])):  # one colour, the other, both
        assert _put_case(ctx, n3, mask, dtype, first, count, True)[0], (first, count)


def test_pin_put_list_longer_than_one_launch_covers(ctx):
    """129^3 with every interior point but a few pinned: 2 048 000 entries, more than the 4096 blocks of 256 threads cover at once"""
    n3 = (129, 129, 129)
    mask = np.zeros(O.shape(n3), bool)
    mask[1:-1, 1:-1, 1:-1] = True
    mask[5, 6, 7] = mask[64, 64, 64] = mask[127, 127, 1] = False
    ok, end = _put_case(ctx, n3, mask, np.float64, 0, 127 ** 3 - 3, True)
    assert end[1] == 127 ** 3 - 3 > 4096 * 256 and ok
    assert _put_case(ctx, n3, mask, np.float64, end[0], end[1] - end[0], False)[0]


# ------------------------------------------------------------------------------------------ the smoother entries
def _fields(n3, kind, dtype):
    """(a, c, mean) of an operator kind"""
    a = np.exp(_rand(n3, dtype, 21)).astype(dtype) if kind != "shift" else None
    c = _rand(n3, dtype, 22, 0.5, 2.0) if kind in ("cap", "hmean+cap") else None
    return a, c, "harmonic" if kind.startswith("hmean") else "arithmetic"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("walls", [False, True])
@pytest.mark.parametrize("kind", ["shift", "coef", "cap", "hmean", "hmean+cap"])
def test_relax_pin(ctx, kind, walls, dtype):
    """1 and 3 sweeps of every operator, with and without a wall mask, on every shape and set in turn: PinOp.relax's bits, and the
    pins hold g exactly"""
    for i, n3 in enumerate(SHAPES):
        name = SETS[(i + len(kind) + walls) % len(SETS)]
        pin = _sets(n3)[name]
        a, c, mean = _fields(n3, kind, dtype)
        bc, beta = (WALL_BC, WALL_BETA) if walls else (0, R.ZERO)
        s = 0.75
        op = PR.PinOp(n3, _rng(n3), dtype, s, a, c, bc, beta, mean, pin=pin)
        v, f, g = _rand(n3, dtype, 1), _rand(n3, dtype, 2), _rand(n3, dtype, 3)
        v[pin] = g[pin]
        for sweeps in (1, 3):
            got = P.ops3dxs.relax_pin(ctx, v, f, n3, _rng(n3), s, sweeps, pin, g, a=a, c=c, mean=mean, bc=bc, beta=beta)
            assert bits_equal(got, op.relax(v, f, sweeps)), (n3, name, sweeps, np.argwhere(got != op.relax(v, f, sweeps))[:4])
            assert bits_equal(got[pin], g[pin])
    # an empty list is the _wall entry
    none = np.zeros(O.shape(n3), bool)
    got = P.ops3dxs.relax_pin(ctx, v, f, n3, _rng(n3), s, 2, none, None, a=a, c=c, mean=mean, bc=bc, beta=beta)
    assert bits_equal(got, R.Op(n3, _rng(n3), dtype, s, a, c, bc, beta, mean).relax(v, f, 2))


def test_relax_pin_with_zeros(ctx):
    n3 = (33, 17, 9)
    pin = PR.ball(n3)
    v, f = _rand(n3, np.float64, 1), _rand(n3, np.float64, 2)
    v[pin] = 0
    got = P.ops3dxs.relax_pin(ctx, v, f, n3, RG, 0.0, 2, pin, None)
    assert bits_equal(got, PR.PinOp(n3, RG, np.float64, 0.0, pin=pin).relax(v, f, 2)) and not got[pin].any()


# ------------------------------------------------------------------------------------------ the hierarchy
HIER = [  # (shape, kind, shift, coarsening, walls)
    ((9, 9, 9), "shift", 0.0, "full", False), ((33, 17, 9), "shift", 0.0, "full", False), ((9, 9, 65), "shift", 2.5, "full", False),
    ((17, 33, 17), "coef", 0.0, "full", False), ((33, 17, 9), "hmean", 1.0, "full", False), ((17, 33, 17), "cap", 3.0, "full", False),
    ((33, 17, 9), "shift", 0.0, "semi", False), ((9, 9, 65), "coef", 0.5, "semi", False), ((17, 33, 17), "shift", 0.0, "full", True),
    ((33, 17, 9), "hmean+cap", 2.0, "full", True)]


def _pair(ctx, n3, kind, s, how, walls, dtype, pin, g, v0, f, use_graph=False):
    """the library's hierarchy and the restated one, both holding v0 and f on level 0"""
    a, c, mean = _fields(n3, kind, dtype)
    bc, beta = (WALL_BC, WALL_BETA) if walls else (0, R.ZERO)
    rng = _rng(n3)
    kw = dict(neumann=FACES(bc), robin=beta) if walls else {}
    mg = P.MultiGrid3D(ctx, n3, rng, dtype, residual_mode=P.CORRECT, coarsening=how, shift=s, coefficient=a, capacity=c, face_mean=mean,
                       pinned=pin, pinned_values=g, **kw)
    mg.use_graph = use_graph
    H = PR.PinHierarchy(R.Op(n3, rng, dtype, s, a, c, bc, beta, mean), pin, g, how)
    if v0 is not None:
        mg.upload_v(0, v0)
        H.set_v(v0)
    if f is not None:
        mg.upload_f(0, f)
        H.f[0] = np.array(f, dtype)
    return mg, H


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(HIER)))
def test_hierarchy_calls_match_the_restatement(ctx, case, dtype):
    """the masks and values of every level, then Relax, CalculateResidual, ResidualNorm, VCycle(2, 2) and FullMultiGridVCycle(1, 2, 2)
    bit for bit; v = g at the pins after every call"""
    n3, kind, s, how, walls = HIER[case]
    name = SETS[case % len(SETS)]
    pin, g = _sets(n3)[name], _rand(n3, dtype, 5)
    v0, f = _rand(n3, dtype, 6), _rand(n3, dtype, 7)
    mg, H = _pair(ctx, n3, kind, s, how, walls, dtype, pin, g, v0, f)
    try:
        assert mg.maxGrids == len(H.sizes) and list(mg.masks) == list(H.masks)
        for l in range(mg.maxGrids):
            assert np.array_equal(mg.pinned(l), H.pins[l]) and mg.pinned_count(l) == int(H.pins[l].sum()), l
            assert bits_equal(mg.download_v(l)[H.pins[l]], H.gs[l][H.pins[l]]), l
        assert bits_equal(mg.download_v(0), H.v[0])  # upload_v kept the pinned values
        mg.Relax(0, 2)
        H.relax(0, 2)
        assert bits_equal(mg.download_v(0), H.v[0]), "Relax"
        r = H.residual(0)
        assert bits_equal(mg.CalculateResidual(0), r) and not r[pin].any()
        norm = math.sqrt(R.fsum_sq(r))
        assert abs(mg.ResidualNorm(0) - norm) <= 1e-12 * norm
        mg.VCycle(0, 2, 2)
        H.vcycle(0, 2, 2)
        assert bits_equal(mg.download_v(0), H.v[0]), ("VCycle", name)
        for l in range(1, mg.maxGrids):
            assert bits_equal(mg.download_v(l), H.v[l]) and bits_equal(mg.download_f(l), H.f[l]), l
        mg.FullMultiGridVCycle(0, 1, 2, 2)
        H.fmg(0, 1, 2, 2)
        for l in range(mg.maxGrids):
            assert bits_equal(mg.download_v(l), H.v[l]), ("FMG", l)
        assert bits_equal(mg.download_v(0)[pin], g[pin])
        if mg.maxGrids > 1:  # a cycle that starts further down: that level holds its own values
            mg.VCycle(1, 1, 1)
            H.vcycle(1, 1, 1)
            assert bits_equal(mg.download_v(1), H.v[1])
    finally:
        mg.close()


# ------------------------------------------------------------------------------------------ the solves
SOLVES = [((17, 17, 17), "shift", 0.0, False, "ball"), ((17, 33, 17), "coef", 1.0, False, "odd plate"), ((17, 17, 17), "shift", 0.0, True, "outside"),
          ((33, 17, 9), "hmean", 0.5, True, "row ends")]


# (krylov = True is refused with walls: test_refusals)
SOLVE_MODES = [(i, k) for i, c in enumerate(SOLVES) for k in (False, True, "weighted") if not (c[3] and k is True)]


@pytest.mark.parametrize("case,krylov", SOLVE_MODES)
def test_pcg_matches_the_restated_solver(ctx, case, krylov):
    """iterations and iterate against the restatement, as tests/test_gpu_neumann_krylov.py compares its cases: converged, the true
    residual below tol and the restated one of the downloaded x next to it, the count the restated one where its history is
    decisive (within 2 where not); plain cycling bit for bit.  Pins hold g, the residual is exactly 0 there, d_f[0] is restored"""
    n3, kind, s, walls, name = SOLVES[case]
    dtype, tol = np.float64, 1e-10
    pin, g = _sets(n3)[name], _rand(n3, dtype, 5)
    v0, f = _rand(n3, dtype, 6), _rand(n3, dtype, 7)
    mg, H = _pair(ctx, n3, kind, s, "full", walls, dtype, pin, g, v0, f)
    try:
        k, rel, conv, hist = mg.PCG(2, 2, tol, 60, krylov=krylov)
        x = mg.download_v(0)
        assert bits_equal(mg.download_f(0), f), "d_f[0] was not restored"
        assert bits_equal(x[pin], g[pin]) and not mg.CalculateResidual(0)[pin].any()
        top = H.ops[0]
        x0 = H.v[0].copy()
        want = math.sqrt(R.fsum_sq(top.residual(x, f)) / R.fsum_sq(top.residual(x0, f)))
        if krylov is False:
            k_r, rel_r, conv_r = H.cycle_to(2, 2, tol, 60)
            assert (k, conv) == (k_r, conv_r) and bits_equal(x, H.v[0])
            hist_r = None
        else:
            a, c, mean = _fields(n3, kind, dtype)
            bc, beta = (WALL_BC, WALL_BETA) if walls else (0, R.ZERO)
            x_r, k_r, hist_r, conv_r, rel_r = PR.pin_fcg(R.Op(n3, _rng(n3), dtype, s, a, c, bc, beta, mean), pin, g, v0, f, tol, 60)
            decisive = len(hist_r) >= 1 and hist_r[-1] * 1.5 < tol and (len(hist_r) < 2 or hist_r[-2] > tol * 1.5)
            assert k == k_r if decisive else abs(k - k_r) <= 2
            assert np.abs(x - x_r).max() <= 1e3 * tol * max(1.0, np.abs(x_r).max())
        print("%s %s %s krylov=%r: %d iterations (restated %d), rel %.3e (restated of x %.3e)" % (n3, kind, name, krylov, k, k_r, rel, want))
        assert conv and conv_r and rel < tol and want < tol and abs(rel - want) <= 1e-6 * want
        unk = top.unk
        assert bits_equal(x[~unk & ~pin], v0[~unk & ~pin]), "the Dirichlet data were changed"
    finally:
        mg.close()


def test_solve3d_pcg_takes_pins(ctx):
    n3 = (17, 17, 17)
    pin, g = PR.ball(n3), _rand(n3, np.float32, 5)
    v0, f = _rand(n3, np.float32, 6), _rand(n3, np.float32, 7)
    x, k, rel, conv = P.solve3d_pcg(ctx, v0, f, UNIT, tol=2e-5, maxit=40, pinned=pin, pinned_values=g)
    assert conv and rel < 2e-5 and bits_equal(x[pin], g[pin])
    top = PR.PinOp(n3, UNIT, np.float32, 0.0, pin=pin)
    w0 = v0.copy()
    w0[pin] = g[pin]
    assert math.sqrt(R.fsum_sq(top.residual(x, f)) / R.fsum_sq(top.residual(w0, f))) < 2e-5


@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_euler_with_a_pinned_hot_plate(ctx, dtype):
    """three implicit steps, plain cycling: PinHierarchy.backward_euler's bits; the plate keeps its temperature"""
    n3 = (17, 33, 17)
    pin = PR.plate(n3, 9)
    g = np.full(O.shape(n3), 2.0, dtype)
    u0 = np.zeros(O.shape(n3), dtype)
    tol = 1e-9 if dtype == np.float64 else 1e-4
    mg, H = _pair(ctx, n3, "shift", 0.0, "full", False, dtype, pin, g, u0, None)
    try:
        mg.upload_f(0, np.zeros(O.shape(n3), dtype))
        got = mg.BackwardEuler(3, 0.01, 0.5, None, 2, 2, tol, 40, krylov=False)
        want = H.backward_euler(3, 0.01, 0.5, 2, 2, tol, 40)
        u = mg.download_v(0)
        assert got[0] == want[0] and got[2] and want[2] and bits_equal(u, H.v[0])
        assert bits_equal(u[pin], g[pin]) and u[H.ops[0].unk].max() > 0
        kk, worst, conv = mg.BackwardEuler(1, 0.01, 0.5, None, 2, 2, tol, 40, krylov=True)
        assert conv and worst < tol and bits_equal(mg.download_v(0)[pin], g[pin])
    finally:
        mg.close()


# ------------------------------------------------------------------------------------------ graphs
@pytest.mark.parametrize("case", [1, 4, 8])
def test_graph_replay_gives_the_eager_bits(ctx, case):
    """VCycle and PCG, replayed against eager, before and after set_pinned changes the set and after set_pinned(None)"""
    n3, kind, s, how, walls = HIER[case]
    dtype = np.float64
    sets = _sets(n3)
    g = _rand(n3, dtype, 5)
    v0, f = _rand(n3, dtype, 6), _rand(n3, dtype, 7)
    pair = [_pair(ctx, n3, kind, s, how, walls, dtype, sets["ball"], g, v0, f, use_graph=ug)[0] for ug in (True, False)]
    try:
        for step, pin in enumerate((sets["ball"], sets["odd plate"], None, sets["black"])):
            if step:
                for mg in pair:
                    mg.set_pinned(pin, g)
                    assert not mg._mg.contents.graph_exec[0] and not mg._mg.contents.pcg_graph_exec, "set_pinned kept a captured graph"
            for rep in range(3):
                for mg in pair:
                    mg.VCycle(0, 2, 2)
                assert bits_equal(pair[0].download_v(0), pair[1].download_v(0)), (step, rep)
            assert pair[0]._mg.contents.graph_exec[0]
            res = []
            for mg in pair:
                mg.upload_v(0, v0)
                k, rel, conv, hist = mg.PCG(2, 2, 1e-9, 30, krylov="weighted")
                res.append((k, rel, conv, hist, mg.download_v(0)))
            assert res[0][:3] == res[1][:3] and np.array_equal(res[0][3], res[1][3]) and bits_equal(res[0][4], res[1][4]), step
            assert res[0][2]
            if pin is not None:
                assert bits_equal(res[0][4][pin], g[pin])
    finally:
        for mg in pair:
            mg.close()


# ------------------------------------------------------------------------------------------ no pins
@pytest.mark.parametrize("how", ["never set, then cleared", "all False"])
@pytest.mark.parametrize("kind,walls", [("shift", False), ("coef", False), ("shift", True)])
def test_without_pins_the_hierarchy_is_what_it_was(ctx, kind, walls, how):
    """set_pinned(None) after a pinned cycle, and an all-False mask: VCycle and PCG bit for bit those of a hierarchy that never
    heard of pins; the plain one still reports its fused kernels"""
    n3, dtype = (33, 33, 33), np.float64
    a, c, mean = _fields(n3, kind, dtype)
    kw = dict(neumann=FACES(WALL_BC), robin=WALL_BETA) if walls else {}
    v0, f = _rand(n3, dtype, 6), _rand(n3, dtype, 7)
    out = []
    for pinned in (False, True):
        mg = P.MultiGrid3D(ctx, n3, UNIT, dtype, residual_mode=P.CORRECT, coefficient=a, **kw)
        try:
            if pinned and how == "all False":
                mg.set_pinned(np.zeros(O.shape(n3), bool))
            elif pinned:
                mg.set_pinned(PR.ball(n3), _rand(n3, dtype, 5))
                mg.upload_v(0, v0)
                mg.upload_f(0, f)
                mg.VCycle(0, 2, 2)
                mg.set_pinned(None)  # (the values the pins left in the coarse v are zeroed by every cycle before it reads them)
            assert mg.pinned_count(0) == 0 and not mg.pinned(0).any() and not mg._mg.contents.pin
            mg.upload_v(0, v0)
            mg.upload_f(0, f)
            mg.VCycle(0, 2, 2)
            names = (ctx.last_relax_kernel(), ctx.last_rr_kernel(), ctx.last_corr_kernel(), ctx.last_block3_kernel())
            x1 = mg.download_v(0)
            res = mg.PCG(2, 2, 1e-10, 30, krylov="weighted")
            out.append((x1, res, mg.download_v(0), names))
        finally:
            mg.close()
    (x1, res, x2, names), (y1, resy, y2, namesy) = out
    assert bits_equal(x1, y1) and bits_equal(x2, y2) and res[:3] == resy[:3] and np.array_equal(res[3], resy[3]) and res[2]
    assert names == namesy
    if kind == "shift" and not walls:
        assert names[0] and "relax_shift" not in names[0], names  # (the operator route, which pins take, reports relax_shift3d_xs_kernel)


# ------------------------------------------------------------------------------------------ refusals
def _refused(call, *words):
    with pytest.raises(P.MgxError) as e:
        call()
    assert e.value.status == P.MGX_ERR_INVALID, e.value
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_refusals(ctx):
    n3 = (17, 17, 17)
    pin, g = PR.ball(n3), _rand(n3, np.float64, 5)
    # a True on the boundary names the first offending point
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT)
    bad = pin.copy()
    bad[4, 0, 3] = bad[9, 16, 2] = True
    _refused(lambda: mg.set_pinned(bad), "(3, 0, 4)", "boundary")
    assert mg.pinned_count(0) == 0
    with pytest.raises(ValueError):
        mg.set_pinned(np.zeros((3, 3, 3), bool))
    nan = g.copy()
    nan[pin] = np.nan
    _refused(lambda: mg.set_pinned(pin, nan), "finite")
    mg.set_pinned(pin, g)
    # the Jacobi smoother, residual_mode, precond = f32, Eigen
    mg.set_smoother("jacobi")
    _refused(lambda: mg.Relax(0, 1), "Jacobi")
    _refused(lambda: mg.VCycle(0, 1, 1), "Jacobi")
    mg.set_smoother("rbgs")
    mg._mg.contents.residual_mode = P.REF_COMPAT
    _refused(lambda: mg.VCycle(0, 1, 1), "residual_mode")
    _refused(lambda: mg.CalculateResidual(0), "residual_mode")
    mg._mg.contents.residual_mode = P.CORRECT
    _refused(lambda: mg.PCG(2, 2, 1e-8, 5, precond="f32"), "pinned", "f32")
    _refused(lambda: mg.Eigen(2), "Eigen", "pinned")
    mg.VCycle(0, 1, 1)  # and it still works
    mg.close()
    for kw, word in ((dict(residual_mode=P.REF_COMPAT), "residual_mode"), (dict(residual_mode=P.CORRECT, layout="natural"), "natural")):
        mg = P.MultiGrid3D(ctx, n3, UNIT, **kw)
        _refused(lambda: mg.set_pinned(pin, g), word)
        mg.close()
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT)
    mg.set_smoother("jacobi")
    _refused(lambda: mg.set_pinned(pin, g), "Jacobi")
    mg.close()
    with pytest.raises(P.MgxError) as e:
        P.MultiGrid3D(ctx, n3, UNIT, layout="natural", residual_mode=P.CORRECT, pinned=pin)
    assert "natural" in str(e.value)
    # the closed box, whatever the pins, krylov = "weighted" included; a shift or a beta > 0 opens it
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, neumann=[1] * 6, pinned=pin, pinned_values=g)
    for call in (lambda: mg.VCycle(0, 2, 2), lambda: mg.Relax(0, 1), lambda: mg.ResidualNorm(0), lambda: mg.PCG(2, 2, 1e-8, 5, krylov=False),
                 lambda: mg.PCG(2, 2, 1e-8, 5, krylov="weighted")):
        _refused(call, "closed box")
    mg.shift = 1.0
    assert mg.PCG(2, 2, 1e-8, 30, krylov="weighted")[2]
    mg.shift = 0.0
    mg.set_wall([0, 0, 0, 0, 0, 2.0])
    assert mg.PCG(2, 2, 1e-8, 30, krylov="weighted")[2]
    mg.close()
