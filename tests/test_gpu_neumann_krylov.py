"""GPU suite: flexible CG in the weighted inner product on hierarchies with Neumann faces (PCG(krylov="weighted")).

The vector entries for all unknowns (mgx3dxs_*_bc of csrc/mgx_rim3d.hip: laplace_dot_shift, apply_coef_dot, cg_update, dot2,
cg_direction, project) are checked on test_gpu_neumann.py's shapes and masks: the arrays bit for bit against numpy with poisoned
pads, Dirichlet entries and read-only arguments unchanged, the sums against math.fsum to 1e-13 of the sum of the absolute terms
and equal on two runs with NaN guards behind the work array, mask 0 against the existing entries.  The solves against the
restatement (tests/op_restated.py): iteration counts, residuals, what a solve leaves behind, graphs against eager
runs, the closed box without a shift."""
import ctypes as C
import math

import numpy as np
import pytest

import op_cases as OC
import op_restated as OP
import oracle as O
import pde_multigrid_amd as P
from conftest import bits_equal
from op_cases import CASES, TOL, UNIT, gaussian
from odd_shapes import pads_unchanged, run_poisoned
from pde_multigrid_amd.multigrid import _ct, _ip, _rp, grid_spacing, xs_unpack

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]
DTYPES = [np.float64, np.float32]
SHAPES = [(17, 17, 17), (21, 13, 29), (131, 7, 9), (257, 9, 5), (513, 5, 5), (3, 3, 3), (3, 5, 9), (5, 3, 3)]
MASKS = [0, 1, 2, 12, 48, 21, 42, 37, 63]
WORK_GUARD = 64
FACES = lambda bc: [bool((bc >> k) & 1) for k in range(6)]


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


def fsum_close(got, terms, rtol=1e-13):
    """got against math.fsum(terms), to rtol of the sum of the absolute terms"""
    terms = np.asarray(terms, np.float64).ravel()
    return abs(got - math.fsum(terms)) <= rtol * math.fsum(np.abs(terms))


class Work:
    """the reduction scratch of a call (mgx3dxs_krylov_work_elems_bc doubles, NaN guards behind them), `nsums` device sums and
    two device scalars"""

    def __init__(self, ctx, n3, dtype, scalars=(0.0, 0.0)):
        fn = getattr(P.lib, "mgx3dxs_krylov_work_elems_bc_" + _ct(dtype)[0])
        fn.restype = C.c_size_t
        self.ctx, self.elems = ctx, int(fn(_ip(n3)))
        host = np.zeros(self.elems + WORK_GUARD)
        host[self.elems:] = np.nan
        self.work, self.sum = ctx.to_device(host), ctx.to_device(np.full(2, np.nan))
        self.scal = ctx.to_device(np.array(scalars, np.float64))
        self.alpha, self.beta = self.scal, C.c_void_p(self.scal.value + 8)

    def result(self, nsums=1):
        tail = self.ctx.to_host(C.c_void_p(self.work.value + 8 * self.elems), (WORK_GUARD,), np.float64)
        assert np.isnan(tail).all(), "the work array was overrun"
        out = self.ctx.to_host(self.sum, (2,), np.float64)
        return float(out[0]) if nsums == 1 else (float(out[0]), float(out[1]))

    def close(self):
        for p in (self.work, self.sum, self.scal):
            self.ctx.free(p)


def _same(outs, ups):
    return all(bits_equal(o, u) for o, u in zip(outs, ups))


# ---------------------------------------------------------------------------------------------------------- kernel entries
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("coef", [False, True])
@pytest.mark.parametrize("n3", SHAPES)
def test_apply_dot_bc(ctx, n3, coef, dtype):
    rng = _rng(n3)
    p, q0 = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    a = _rand(n3, dtype, 3, 0.5, 2.0) if coef else None
    fn, ct = _fn("apply_coef_dot_bc" if coef else "laplace_dot_shift_bc", dtype)
    ins = [p, a] if coef else [p]
    w = Work(ctx, n3, dtype)
    try:
        for bc in MASKS:
            unk, W = OP.unknown_mask(n3, bc), OP.weights(n3, bc)
            for s in (0.0, 0.75):
                want = q0.copy()
                want[unk] = OP.Op(n3, rng, dtype, s, a, bc=bc).apply_A(p)[unk]  # the Dirichlet entries of q are not written
                sums = []
                for rep in range(2):
                    ups, outs = run_poisoned(ctx, ins + [q0], lambda *d: fn(ctx._h, *d, _ip(n3), _h(n3, rng, dtype), ct(s), w.work, w.sum,
                                                                           C.c_int(bc)), dtype)
                    got = xs_unpack(outs[-1], n3[0])
                    assert bits_equal(got, want), (bc, s, np.argwhere(got != want)[:5])
                    assert _same(outs[:-1], ups[:-1]) and pads_unchanged(ups[-1], outs[-1], n3[0])
                    sums.append(w.result())
                assert sums[0] == sums[1], "two runs gave different sums"
                assert fsum_close(sums[0], W * p.astype(np.float64) * want.astype(np.float64)), (bc, s, sums[0])
                if bc == 0:
                    old = P.ops3dxs.apply_coef_dot(ctx, p, a, n3, rng, s, q=q0) if coef else P.ops3dxs.laplace_dot_shift(ctx, p, n3, rng, s, q=q0)
                    assert bits_equal(got, old[0]) and sums[0] == old[1], s
    finally:
        w.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", SHAPES)
def test_cg_update_bc(ctx, n3, dtype):
    x, p, r, q = (_rand(n3, dtype, k) for k in (4, 5, 6, 7))
    alpha = 0.37
    al = dtype(alpha)
    fn, _ = _fn("cg_update_bc", dtype)
    w = Work(ctx, n3, dtype, (alpha, 0.0))
    try:
        for bc in MASKS:
            unk = OP.unknown_mask(n3, bc)
            wx, wr = x.copy(), r.copy()
            wx[unk] = (x + al * p)[unk]
            wr[unk] = (r - al * q)[unk]
            for with_x in (True, False):
                sums = []
                for rep in range(2):
                    ups, outs = run_poisoned(ctx, [x, p, r, q], lambda xd, pd, rd, qd: fn(ctx._h, xd if with_x else None, pd, rd, qd, _ip(n3), w.alpha,
                                                                                           w.work, w.sum, C.c_int(bc)), dtype)
                    assert bits_equal(xs_unpack(outs[0], n3[0]), wx if with_x else x), (bc, with_x)
                    assert bits_equal(xs_unpack(outs[2], n3[0]), wr), (bc, with_x)
                    assert bits_equal(outs[1], ups[1]) and bits_equal(outs[3], ups[3])
                    assert pads_unchanged(ups[0], outs[0], n3[0]) and pads_unchanged(ups[2], outs[2], n3[0])
                    sums.append(w.result())
                assert sums[0] == sums[1], "two runs gave different sums"
                assert fsum_close(sums[0], wr[unk].astype(np.float64) ** 2), (bc, with_x, sums[0])  # unweighted
                if bc == 0:
                    xo, ro, ss = P.ops3dxs.cg_update(ctx, P.xs_pack(x) if with_x else None, P.xs_pack(p), P.xs_pack(r), P.xs_pack(q), n3, alpha)
                    assert bits_equal(xs_unpack(ro, n3[0]), wr) and ss == sums[0] and (not with_x or bits_equal(xs_unpack(xo, n3[0]), wx))
    finally:
        w.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", SHAPES)
def test_dot2_bc(ctx, n3, dtype):
    a, b, c = (_rand(n3, dtype, k) for k in (8, 9, 10))
    fn, _ = _fn("dot2_bc", dtype)
    w = Work(ctx, n3, dtype)
    a64, b64, c64 = (t.astype(np.float64) for t in (a, b, c))
    try:
        for bc in MASKS:
            W = OP.weights(n3, bc)
            for two in (True, False):
                sums = []
                for rep in range(2):
                    ups, outs = run_poisoned(ctx, [a, b, c], lambda ad, bd, cd: fn(ctx._h, ad, bd, cd if two else None, _ip(n3), w.work, w.sum,
                                                                                  C.c_int(bc)), dtype)
                    assert _same(outs, ups)
                    sums.append(w.result(2))
                assert sums[0][0] == sums[1][0] and (not two or sums[0][1] == sums[1][1]), "two runs gave different sums"
                assert fsum_close(sums[0][0], W * a64 * b64), (bc, two)
                assert not two or fsum_close(sums[0][1], W * a64 * c64), (bc, two)
                if bc == 0:
                    old = P.ops3dxs.dot2(ctx, P.xs_pack(a), P.xs_pack(b), P.xs_pack(c) if two else None, n3)
                    assert old[0] == sums[0][0] and (not two or old[1] == sums[0][1])
    finally:
        w.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", SHAPES)
def test_cg_direction_bc(ctx, n3, dtype):
    x, p, z = (_rand(n3, dtype, k) for k in (11, 12, 13))
    alpha, beta = 0.37, -0.21
    al, be = dtype(alpha), dtype(beta)
    fn, _ = _fn("cg_direction_bc", dtype)
    w = Work(ctx, n3, dtype, (alpha, beta))
    # (x updated?, z given?, beta given?): the three forms of the solver and the two the entry takes besides
    forms = [(False, True, False), (True, True, True), (True, False, False), (True, True, False), (False, True, True)]
    try:
        for bc in MASKS:
            unk = OP.unknown_mask(n3, bc)
            for fx, fz, fb in forms:
                wx, wp = x.copy(), p.copy()
                if fx:
                    wx[unk] = (x + al * p)[unk]
                if fz:
                    wp[unk] = (z + be * p)[unk] if fb else z[unk]
                ups, outs = run_poisoned(ctx, [x, p, z], lambda xd, pd, zd: fn(ctx._h, xd if fx else None, pd, zd if fz else None, _ip(n3),
                                                                              w.alpha if fx else None, w.beta if fb else None, C.c_int(bc)), dtype)
                assert bits_equal(xs_unpack(outs[0], n3[0]), wx) and bits_equal(xs_unpack(outs[1], n3[0]), wp), (bc, fx, fz, fb)
                assert bits_equal(outs[2], ups[2]) and pads_unchanged(ups[0], outs[0], n3[0]) and pads_unchanged(ups[1], outs[1], n3[0])
                if bc == 0:
                    xo, po = P.ops3dxs.cg_direction(ctx, P.xs_pack(x) if fx else None, P.xs_pack(p), P.xs_pack(z) if fz else None, n3,
                                                    alpha if fx else None, beta if fb else None)
                    assert bits_equal(xs_unpack(po, n3[0]), wp) and (not fx or bits_equal(xs_unpack(xo, n3[0]), wx))
    finally:
        w.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", SHAPES)
def test_project_bc(ctx, n3, dtype):
    a = _rand(n3, dtype, 14, -0.5, 1.5)
    fn, _ = _fn("project_bc", dtype)
    w = Work(ctx, n3, dtype)
    try:
        for bc in MASKS:
            unk, W = OP.unknown_mask(n3, bc), OP.weights(n3, bc)
            sw = OP.sum_weights(n3, bc)
            means = []
            for rep in range(2):
                ups, outs = run_poisoned(ctx, [a], lambda ad: fn(ctx._h, ad, _ip(n3), w.work, w.sum, C.c_int(bc)), dtype)
                mean = w.result()
                want = a.copy()
                want[unk] = (a - dtype(mean))[unk]  # the downloaded mean, rounded to the arrays' precision
                assert bits_equal(xs_unpack(outs[0], n3[0]), want), bc
                assert pads_unchanged(ups[0], outs[0], n3[0])
                means.append(mean)
            assert means[0] == means[1], "two runs gave different means"
            assert fsum_close(means[0] * sw, W * a.astype(np.float64)), (bc, means[0])
    finally:
        w.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_entries_reject_bad_masks_and_sizes(ctx, dtype):
    n3, bad = (17, 9, 9), (16, 9, 9)
    a, b = _rand(n3, dtype, 1, 0.5, 2.0), np.ones(O.shape(bad), dtype)
    ops = P.ops3dxs

    def calls(bc, n=n3, x=a):
        return [lambda: ops.laplace_dot_shift_bc(ctx, x, n, RG, 1.0, bc), lambda: ops.apply_coef_dot_bc(ctx, x, x, n, RG, 1.0, bc),
                lambda: ops.cg_update_bc(ctx, x, x, x, x, n, 0.5, bc), lambda: ops.dot2_bc(ctx, x, x, x, n, bc),
                lambda: ops.cg_direction_bc(ctx, x, x, x, n, bc, 0.5, 0.5), lambda: ops.project_bc(ctx, x, n, bc)]
    for bc in (64, -1):
        for call in calls(bc):
            with pytest.raises(P.MgxError) as e:
                call()
            assert e.value.status == P.MGX_ERR_INVALID
    for call in calls(5, bad, b):
        with pytest.raises(P.MgxError) as e:
            call()
        assert e.value.status == P.MGX_ERR_SIZE
    q, pq = ops.laplace_dot_shift_bc(ctx, a, n3, RG, 1.0, 37)  # the wrappers themselves
    want = OP.Op(n3, RG, dtype, 1.0, bc=37).apply_A(a)
    want[~OP.unknown_mask(n3, 37)] = 0.0  # the Dirichlet entries of the wrapper's zero-filled q, unwritten
    assert bits_equal(q, want)
    got, mean = ops.project_bc(ctx, a, n3, 63)
    assert bits_equal(got, a - dtype(mean))


# ---------------------------------------------------------------------------------------------------------- solves
def _mg(ctx, n3, bc, s, kind, v0, f, dtype=np.float64):
    mg = P.MultiGrid3D(ctx, n3, UNIT, dtype, residual_mode=P.CORRECT, shift=s, coefficient=OC.coefficient(n3, kind, dtype), neumann=FACES(bc))
    mg.upload_v(0, v0)
    mg.upload_f(0, f)
    return mg


def _true_rel(n3, bc, s, kind, x, v0, f, removed=0.0, dtype=np.float64):
    """the restated true relative residual of x against f - removed"""
    a = OC.coefficient(n3, kind, dtype)
    fp = (f - dtype(removed)).astype(dtype) if removed else f
    res = lambda y: OP.fsum_sq(OP.Op(n3, UNIT, dtype, s, a, bc=bc).residual(y, fp))
    return math.sqrt(res(x) / res(v0))


@pytest.mark.parametrize("size", [17, 33])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_table_cases_match_the_restated_solver(ctx, case, size):
    """every row of DESIGN.md 16's table: converged, the true residual below tol and the restated one of the downloaded x next to
    it, d_f[0] restored, the Dirichlet data unchanged; the iteration count is the restated one where the restated history keeps
    a factor 1.5 from tol on both sides of the deciding iteration (within 2 where it does not: a count may then flip)"""
    bc, s, kind = CASES[case][:3]
    n3 = (size,) * 3
    v0, f = OC.table_start(case, n3)
    x_r, k_r, hist_r, conv_r, rel_r, removed_r = OC.solved(case, size)
    mg = _mg(ctx, n3, bc, s, kind, v0, f)
    k, rel, conv, hist = mg.PCG(2, 2, TOL, 60, krylov="weighted")
    x, removed = mg.download_v(0), mg.pcg_removed_mean
    assert bits_equal(mg.download_f(0), f), "d_f[0] was not restored"
    mg.close()
    want = _true_rel(n3, bc, s, kind, x, v0, f, removed)
    print("case %r at %d^3: %d iterations (restated %d, decisive %s), rel %.3e (restated of x %.3e)" % (CASES[case][:3], size, k, k_r,
                                                                                                          OC.decisive(hist_r), rel, want))
    assert conv and conv_r and rel < TOL and want < TOL and abs(rel - want) <= 1e-6 * want
    if OC.decisive(hist_r):
        assert k == k_r == CASES[case][3 + (size == 33)]
    else:
        assert abs(k - k_r) <= 2
    unk = OP.unknown_mask(n3, bc)
    assert bits_equal(x[~unk], v0[~unk]), "the Dirichlet data were changed"
    if not (bc == 63 and s == 0):
        assert removed == 0.0


@pytest.mark.parametrize("case", [3, 4])
def test_jump_1000_converges_where_plain_cycling_does_not(ctx, case):
    bc, s, kind = CASES[case][:3]
    n3 = (33, 33, 33)
    v0, f = OC.start(n3)
    k_r, conv_r = OC.solved(case, 33)[1], OC.solved(case, 33)[3]
    mg = _mg(ctx, n3, bc, s, kind, v0, f)
    k, rel, conv, _ = mg.PCG(2, 2, TOL, 60, krylov="weighted")
    mg.upload_v(0, v0)
    kp, relp, convp, _ = mg.PCG(2, 2, TOL, 60, krylov=False)
    mg.close()
    print("case %r: weighted CG %d iterations (restated %d), rel %.3e; plain cycling %d cycles, rel %.3e" % (CASES[case][:3], k, k_r, rel, kp, relp))
    assert conv and conv_r and rel < TOL and abs(k - k_r) <= 2
    assert not convp and kp == 60


def test_fp32_solve_in_the_closed_box(ctx):
    n3, bc, s, tol, dt = (17, 17, 17), 63, 100.0, 1e-4, np.float32
    v0, f = OC.start(n3, dt)
    x_r, k_r, hist_r, conv_r, rel_r, _ = OP.fcg(OP.Op(n3, UNIT, dt, s, bc=bc), v0, f, tol=tol)
    mg = _mg(ctx, n3, bc, s, None, v0, f, dt)
    k, rel, conv, _ = mg.PCG(2, 2, tol, 60, krylov=2)
    x = mg.download_v(0)
    assert bits_equal(mg.download_f(0), f)
    mg.close()
    want = _true_rel(n3, bc, s, None, x, v0, f, dtype=dt)
    print("fp32: %d iterations (restated %d), rel %.3e (restated of x %.3e)" % (k, k_r, rel, want))
    assert conv and conv_r and abs(k - k_r) <= 1 and rel < tol and want < tol


@pytest.mark.parametrize("case", [3, 7])
def test_graph_replay_gives_the_eager_bits(ctx, case):
    bc, s, kind = CASES[case][:3]
    n3 = (17, 17, 17)
    v0, f = OC.start(n3)
    mg = _mg(ctx, n3, bc, s, kind, v0, f)
    k0, rel0, conv0, hist0 = mg.PCG(2, 2, TOL, 60, krylov="weighted")
    x0 = mg.download_v(0)
    assert not mg._mg.contents.pcg_graph_exec
    mg.use_graph = True
    execs = []
    for rep in range(2):  # the first call captures the preconditioning cycle, the second replays it
        mg.upload_v(0, v0)
        k, rel, conv, hist = mg.PCG(2, 2, TOL, 60, krylov="weighted")
        assert (k, conv) == (k0, conv0) and rel == rel0 and np.array_equal(hist, hist0), rep
        assert bits_equal(mg.download_v(0), x0), rep
        execs.append(mg._mg.contents.pcg_graph_exec)
    assert execs[0] and execs[1] == execs[0], "the cycle was captured again instead of replayed"
    assert mg._mg.contents.bc_reserved == 0
    mg.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s,kind", [(0.0, None), (0.75, None), (0.0, "smooth")])
def test_weighted_without_a_mask_is_krylov_1(ctx, s, kind, dtype):
    n3, tol = (33, 17, 17), 1e-8 if dtype == np.float64 else 1e-4
    v0, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    out = []
    for krylov in (True, "weighted"):
        mg = P.MultiGrid3D(ctx, n3, RG, dtype, residual_mode=P.CORRECT, shift=s, coefficient=OC.coefficient(n3, kind, dtype))
        mg.upload_v(0, v0)
        mg.upload_f(0, f)
        k, rel, conv, hist = mg.PCG(2, 2, tol, 50, krylov=krylov)
        out.append((k, rel, conv, hist, mg.download_v(0), mg.pcg_removed_mean))
        mg.close()
    (k1, rel1, conv1, hist1, x1, m1), (k2, rel2, conv2, hist2, x2, m2) = out
    assert conv1 and (k1, rel1, conv1) == (k2, rel2, conv2) and np.array_equal(hist1, hist2) and bits_equal(x1, x2) and m1 == m2 == 0.0


def test_mask_cleared_after_a_masked_solve(ctx):
    """p and q hold values on the face unknowns during a solve with a mask and krylov = 1 reads p's boundary as zero Dirichlet
    data: after the mask is cleared it gives the bits of a hierarchy that never had one"""
    n3, tol = (17, 17, 17), 1e-10
    v0, f = OC.start(n3)
    mg = _mg(ctx, n3, 63, 0.0, None, v0, f)
    k, rel, conv, _ = mg.PCG(2, 2, tol, 60, krylov="weighted")  # the singular solve: the projections too
    assert conv and mg.pcg_removed_mean != 0.0
    mg.set_neumann(None)
    mg.upload_v(0, v0)
    assert mg.PCG(2, 2, tol, 60, krylov=True, precond="f32")[2] and mg.pcg_removed_mean == 0.0  # written as 0 by every other solve
    mg.set_neumann([1] * 6)
    mg.shift = 1.0
    mg.upload_v(0, v0)
    assert mg.PCG(2, 2, tol, 60, krylov="weighted")[2]
    mg.shift = 0.0
    mg.set_neumann(None)
    fresh = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT)
    res = []
    for m in (mg, fresh):
        m.upload_v(0, v0)
        m.upload_f(0, f)
        res.append(m.PCG(2, 2, tol, 60, krylov=True)[:3] + (m.download_v(0),))
        m.close()
    assert res[0][2] and res[0][:3] == res[1][:3] and bits_equal(res[0][3], res[1][3])


def test_krylov_1_with_a_mask_names_krylov_2(ctx):
    n3 = (17, 17, 17)
    v0, f = OC.start(n3)
    mg = _mg(ctx, n3, 17, 0.0, None, v0, f)
    for call in (lambda: mg.PCG(2, 2, 1e-8, 5, krylov=True), lambda: mg.BackwardEuler(1, 1e-2, 1.0, krylov=True)):
        with pytest.raises(P.MgxError) as e:
            call()
        assert e.value.status == P.MGX_ERR_INVALID and "Neumann" in str(e.value) and "krylov = 2" in str(e.value)
    with pytest.raises(P.MgxError) as e:
        mg.PCG(2, 2, 1e-8, 5, krylov="weighted", precond="f32")
    assert "Neumann" in str(e.value)
    mg.close()


# ---------------------------------------------------------------------------------------------------------- backward Euler
@pytest.mark.parametrize("kdt", [1e-2, 5e-5])
def test_backward_euler_in_a_closed_box_keeps_the_heat_content(ctx, kdt):
    """test_gpu_neumann's conservation case with krylov = 2: 17^3, all six faces walls, the smooth coefficient, Gaussian initial
    data, five steps solved to 1e-10: the relative drift of sum(w u) stays below 1e-9"""
    n3 = (17, 17, 17)
    u0 = gaussian(n3)
    W = OP.weights(n3, 63)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, coefficient=OC.smooth_coefficient(n3), neumann=[1] * 6)
    mg.upload_v(0, u0)
    its, worst, conv = mg.BackwardEuler(5, kdt, 1.0, tol=1e-10, maxit=50, krylov="weighted")
    u = mg.download_v(0)
    mg.close()
    heat0, heat = math.fsum((W * u0).ravel()), math.fsum((W * u).ravel())
    drift = abs(heat - heat0) / abs(heat0)
    print("kappa dt %g: %d iterations, worst relative residual %.3e, relative drift of the heat content %.3e" % (kdt, its, worst, drift))
    assert conv and worst < 1e-10
    assert drift < 1e-9, drift


def test_backward_euler_step_against_its_own_linear_system(ctx):
    n3, bc, kappa, dt, tol = (33, 17, 17), 37, 0.7, 3e-3, 1e-10
    s = 1.0 / (kappa * dt)
    u0, q, f0 = _rand(n3, np.float64, 20), _rand(n3, np.float64, 21), _rand(n3, np.float64, 22)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, neumann=FACES(bc))
    mg.upload_v(0, u0)
    mg.upload_f(0, f0)
    its, worst, conv = mg.BackwardEuler(1, dt, kappa, source=q, tol=tol, krylov=2)
    u, rhs_dev = mg.download_v(0), mg.download_f(0)
    assert mg.shift == s
    mg.close()
    f = OP.Op(n3, UNIT, np.float64, s, bc=bc).rhs(u0, q, 1.0 / kappa, f=f0)
    assert bits_equal(rhs_dev, f), "d_f[0] is not the step's right-hand side on the unknowns and what it was elsewhere"
    res = lambda x: OP.fsum_sq(OP.Op(n3, UNIT, np.float64, s, bc=bc).residual(x, f))
    rel = math.sqrt(res(u) / res(u0))
    print("one step, bc %d: %d iterations, residual %.3e (restated %.3e)" % (bc, its, worst, rel))
    assert conv and worst < tol and rel < tol and abs(worst - rel) <= 1e-6 * rel
    unk = OP.unknown_mask(n3, bc)
    assert bits_equal(u[~unk], u0[~unk]), "the Dirichlet data changed"


@pytest.mark.parametrize("case", [1, 5, 7])
def test_solve3d_pcg_equals_the_hierarchy_call(ctx, case):
    bc, s, kind = CASES[case][:3]
    n3 = (17, 17, 17)
    v0, f = OC.start(n3)
    mg = _mg(ctx, n3, bc, s, kind, v0, f)
    k, rel, conv, _ = mg.PCG(2, 2, TOL, 60, krylov="weighted")
    x = mg.download_v(0)
    mg.close()
    x2, k2, rel2, conv2 = P.solve3d_pcg(ctx, v0, f, UNIT, tol=TOL, maxit=60, krylov="weighted", shift=s, coefficient=OC.coefficient(n3, kind),
                                        neumann=FACES(bc))
    assert conv and (k2, rel2, conv2) == (k, rel, conv) and bits_equal(x2, x)


# ---------------------------------------------------------------------------------------------------------- the closed box, no shift
@pytest.mark.parametrize("size", [17, 33])
@pytest.mark.parametrize("case", [6, 7, 8])
def test_singular_solve(ctx, case, size):
    """the projected solve from the table's zero guess: the table's count, which is the restated one (where decisive), and the
    removed mean; from the random guess the weighted mean of the guess is kept; afterwards the hierarchy refuses the singular
    operator as before, and cycles with a shift like any other"""
    bc, s, kind = CASES[case][:3]
    n3 = (size,) * 3
    v0, f = OC.start(n3)
    x_r, k_r, hist_r, conv_r, rel_r, removed_r = OC.solved(case, size)
    W = OP.weights(n3, 63)
    mg = _mg(ctx, n3, bc, s, kind, np.zeros_like(v0), f)
    k, rel, conv, _ = mg.PCG(2, 2, TOL, 60, krylov="weighted")
    x0, removed = mg.download_v(0), mg.pcg_removed_mean
    assert conv and rel < TOL and abs(OP.wmean(W, x0)) <= 1e-12 * np.abs(x0).max()
    mg.upload_v(0, v0)
    k_rand, rel_rand, conv_rand, _ = mg.PCG(2, 2, TOL, 60, krylov="weighted")
    x = mg.download_v(0)
    assert conv_rand and rel_rand < TOL and mg.pcg_removed_mean == removed
    print("case %r at %d^3: %d iterations (restated %d, decisive %s), removed mean %.17g" % (CASES[case][:3], size, k, k_r, OC.decisive(hist_r),
                                                                                             removed))
    assert k == k_r == CASES[case][3 + (size == 33)] if OC.decisive(hist_r) else abs(k - k_r) <= 2
    want = math.fsum((W * f).ravel()) / OP.sum_weights(n3, 63)
    assert removed_r == want and abs(removed - want) <= 1e-12 * abs(want)
    assert abs(OP.wmean(W, x) - OP.wmean(W, v0)) <= 1e-12 * np.abs(x).max()
    assert mg._mg.contents.bc_reserved == 0
    for call in (lambda: mg.VCycle(0, 2, 2), lambda: mg.Relax(0, 1), lambda: mg.ResidualNorm(0), lambda: mg.PCG(2, 2, TOL, 5, krylov=False),
                 lambda: mg.PCG(2, 2, TOL, 5, krylov=True)):
        with pytest.raises(P.MgxError) as e:
            call()
        assert e.value.status == P.MGX_ERR_INVALID and ("singular" in str(e.value) or "Neumann" in str(e.value)), str(e.value)
    with pytest.raises(P.MgxError) as e:
        mg.VCycle(0, 2, 2)
    assert "singular" in str(e.value)
    mg.shift = 0.75
    mg.upload_v(0, v0)
    mg.VCycle(0, 2, 2)
    assert mg.PCG(2, 2, TOL, 60, krylov="weighted")[2] and mg.pcg_removed_mean == 0.0  # written as 0 by every other solve
    H = OP.Hierarchy(OP.Op(n3, UNIT, np.float64, 0.75, OC.coefficient(n3, kind), bc=63))
    H.v[0], H.f[0] = v0.copy(), f.copy()
    H.vcycle(0, 2, 2)
    mg.upload_v(0, v0)
    mg.VCycle(0, 2, 2)
    assert bits_equal(mg.download_v(0), H.v[0])
    mg.close()
