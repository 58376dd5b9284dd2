"""GPU suite: the vector kernels of the solve (csrc/mgx_krylov3d.hip) and the solves themselves at the sizes the solver is run at.

test_gpu_pcg.py and test_gpu_pcg_mixed.py compare these kernels with numpy on arrays whose launches have at most 1016
workgroup partial sums and whose z-marching pass (correct_residual_demote) runs in runs of 2 planes.  Here every entry point is
compared with the same numpy expressions on shapes where cg_final_kernel takes several trips over the partials, where the
z-marching pass takes runs of 4, 8 and 16 planes with a shorter last run over several x-blocks and many y-blocks, and with the
knobs "mixed3d.rows" / "mixed3d.zchunk" set; every case asserts the launch geometry it exists for (asked of the library,
mgx3dxs_correct_residual_demote_plan_f64, and compared with the rule written out here).  The solves are compared with their
numpy restatements where the geometry is the production one (257^3, 513^3, an odd hierarchy).

Element-wise outputs: bit for bit.  Sums: against math.fsum over the same terms (each term is one rounded double product that
numpy forms identically, so fsum is the exact sum of what the kernel adds):
  sums of squares  |got - ref| <= 1e-13 |ref| (the project's bound; L u below it), L u |ref| where a knob setting makes L u larger
  signed sums      |got - ref| <= L u sum(|terms|): the forward error bound of any fixed order of additions, u = 2^-53, L = the
                   longest chain of additions one term passes through, counted per launch in _stream_L / _crd_L below
Every work array the wrappers upload carries 1024 sentinel doubles behind it which are looked at after each call (_Ops3D._work_check)."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle as O
import pde_multigrid_amd as P
import solve_restated as R
from conftest import bits_equal
from odd_shapes import POISON, bits, hierarchy_ok, levels, pack_poisoned, pads_unchanged
from pde_multigrid_amd.multigrid import _ip, _rp, grid_spacing, xs_geometry, xs_unpack

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]
UNIT = [0, 1, 0, 1, 0, 1]
DTYPES = [np.float64, np.float32]
S, INV = 2.0 ** 7, 2.0 ** -5  # scales of the kernel tests (any doubles: the kernels apply them as given)
U = 2.0 ** -53
# shape: (Krylov partials, (tiles across x, tiles across y, planes per run, plane runs) of correct_residual_demote at its defaults)
BIG = {
    (33, 131, 67): (2145, (1, 9, 2, 33)),      # more than 1024 partials on a small array; 2145 is no multiple of 1024
    (259, 131, 67): (2145, (3, 9, 2, 33)),     # the same with 3 x-blocks; rows end inside a block; fp32 and fp64 pads differ
    (387, 131, 69): (2211, (4, 9, 2, 34)),     # 4 x-blocks, 4 columns in the last; odd but not 2^k + 1
    (771, 69, 41): (663, (7, 5, 2, 20)),       # 7 x-blocks; rows of 4 steps of a wave
    (513, 513, 35): (4224, (5, 32, 4, 9)),     # runs of 4: 33 planes = 8 runs + 1 plane
    (1025, 257, 67): (4160, (9, 16, 8, 9)),    # runs of 8: 65 planes = 8 runs + 1 plane; 9 x-blocks
    (513, 513, 99): (12416, (5, 32, 16, 7)),   # runs of 16: 97 planes = 6 runs + 1 plane
}
KNOB_SHAPES = [(259, 131, 67), (387, 131, 69)]
ZCHUNKS = [1, 2, 3, 5, 16, 64, 128, 0]  # 65 and 67 planes: 64 leaves a last run of 1 and 3 planes, 128 is longer than the level


def _ceil(a, b):
    return -(-a // b)


def _id(n3):
    return "x".join(str(k) for k in n3)


def _pow2_box(n3):
    """a box whose three spacings are (different) powers of two: the exact-reciprocal form of the residual"""
    return [0, (n3[0] - 1) * 2.0 ** -10, 0, (n3[1] - 1) * 2.0 ** -9, 0, (n3[2] - 1) * 2.0 ** -11]


# ---------------------------------------------------------------------------------------------------------- geometry, L
def _krylov_partials(n3, dtype=np.float64):
    fn = getattr(P.lib, "mgx3dxs_krylov_work_elems_" + ("f64" if dtype == np.float64 else "f32"))
    fn.restype = C.c_size_t
    return int(fn(_ip(n3))) // 2  # room for the two sums of dot2


def _crd_rule(n3, rows=4, zchunk=0):
    """the launch rule of correct_residual_demote as the issue states it: (gx, gy, planes per run, plane runs)"""
    gx, gy, planes = _ceil(max((n3[0] + 1) // 2 - 1, 1), 63), _ceil(n3[1] - 2, 4 * rows), n3[2] - 2
    if zchunk == 0:
        zchunk = 16
        while zchunk > 2 and gx * gy * _ceil(planes, zchunk) < 1024:
            zchunk //= 2
    return gx, gy, zchunk, _ceil(planes, zchunk)


def _crd_plan(ctx, n3, rng, corr=False):
    p = P.ops3dxs.correct_residual_demote_plan(ctx, n3, rng, corr)
    return (p["gx"], p["gy"], p["zchunk"], p["gz"]), p


def _final_L(count):
    """cg_final_kernel: a thread adds ceil(count / 1024) partials, then 10 levels of the tree over 1024 threads"""
    return _ceil(count, 1024) + 10


def _stream_L(n3, dtype, count):
    """a streaming kernel: a lane adds KJ = 4 terms per step of 256 positions of its row (pitch P), then 6 shuffle levels, 2
    additions across the block's four waves, then the final kernel.  + 2: the rounding of fsum itself and the 1 / (1 - L u) of
    the bound.  An over-estimate: the first addition of every chain is onto 0.0 and exact."""
    return _ceil(xs_geometry(n3[0], np.dtype(dtype).itemsize)[1], 256) * 4 + 6 + 2 + _final_L(count) + 2


def _crd_L(n3, rows, zchunk, count):
    """the z-marching pass: a lane adds 2 terms (its x-pair) for each of its `rows` rows on each plane of its run, then 6
    shuffle levels, TYW - 1 = 3 additions across the waves, then the final kernel; + 2 as above"""
    return 2 * rows * min(zchunk, n3[2] - 2) + 6 + 3 + _final_L(count) + 2


# ---------------------------------------------------------------------------------------------------------- helpers
@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


def _interior(a):
    return a[1:-1, 1:-1, 1:-1]


def _terms(a, b):
    return (_interior(a).astype(np.float64) * _interior(b).astype(np.float64)).ravel()


def _fsum(t):
    return math.fsum(t.tolist())


class Pool:
    """random arrays of one shape (host, and as stored with poisoned pads) and references computed once per shape"""

    def __init__(self, n3):
        self.n3, self._arr, self._memo = n3, {}, {}

    def get(self, dtype, seed):
        key = (np.dtype(dtype).name, seed)
        if key not in self._arr:
            a = np.random.default_rng(seed).uniform(-1, 1, O.shape(self.n3)).astype(dtype)
            self._arr[key] = (a, pack_poisoned(a))
        return self._arr[key]

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def sums(self, key, a, b):
        """(fsum of the terms of <a, b>, sum of their magnitudes)"""
        def f():
            t = _terms(a, b)
            return _fsum(t), float(np.abs(t).sum())
        return self.memo(("sum",) + tuple(key), f)


@pytest.fixture(scope="module", params=list(BIG), ids=_id)
def pool(request):
    p = Pool(request.param)
    yield p
    p._arr.clear()
    p._memo.clear()


def _where(got, want):
    d = np.argwhere(bits(got) != bits(want))
    if not len(d):
        return "equal"
    lo, hi = d.min(axis=0), d.max(axis=0)
    return "%d entries differ: z %d..%d (%d planes), y %d..%d, x %d..%d; first at z, y, x = %s" % (
        len(d), lo[0], hi[0], len(np.unique(d[:, 0])), lo[1], hi[1], lo[2], hi[2], d[0].tolist())


def _check_out(n3, up, got_stored, want, was):
    """interior = want bit for bit, boundary = was, pads as uploaded"""
    got = xs_unpack(got_stored, n3[0])
    assert bits_equal(_interior(got), _interior(want)), _where(_interior(got), _interior(want))
    full = was.copy()
    _interior(full)[...] = _interior(got)
    assert bits_equal(got, full), "a boundary entry was written: " + _where(got, full)
    assert pads_unchanged(up, got_stored, n3[0])


def _stored(want, was):
    """the array as it has to be stored: want on the interior, was on the boundary, the poison on the pads"""
    full = was.copy()
    _interior(full)[...] = _interior(want)
    return pack_poisoned(full)


def _signed_ok(got, ref_mag, L):
    ref, mag = ref_mag
    return abs(got - ref) <= L * U * mag


def _squares_ok(got, ref, L):
    return abs(got - ref) <= max(1e-13, L * U) * abs(ref)  # L u only where a knob setting puts it above the project's 1e-13


# ---------------------------------------------------------------------------------------------------------- Krylov kernels
@pytest.mark.parametrize("dtype", DTYPES)
def test_laplace_dot(ctx, pool, dtype):
    n3, count = pool.n3, BIG[pool.n3][0]
    assert _krylov_partials(n3, dtype) == count == _ceil(n3[1] - 2, 4) * (n3[2] - 2)
    (p, pp), (q0, qp) = pool.get(dtype, 1), pool.get(dtype, 2)
    outs = [P.ops3dxs.laplace_dot(ctx, pp, n3, RG, q=qp, packed=True, dtype=dtype) for _ in range(2)]
    q_st, pq = outs[0]
    want = pool.memo(("Ap", np.dtype(dtype).name), lambda: -O.residual3d(n3, RG, p, np.zeros_like(p), P.CORRECT, dtype=dtype))
    _check_out(n3, qp, q_st, want, q0)
    ref = pool.sums(("pAp", np.dtype(dtype).name), p, want)
    assert _signed_ok(pq, ref, _stream_L(n3, dtype, count)), (pq, ref)
    assert outs[1][1] == pq and bits_equal(outs[1][0], q_st), "not the same bits on every call"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_x", [True, False])
def test_cg_update(ctx, pool, dtype, with_x):
    n3, count = pool.n3, BIG[pool.n3][0]
    assert _krylov_partials(n3, dtype) == count
    (x, ux), (p, up), (r, ur), (q, uq) = (pool.get(dtype, s) for s in (1, 2, 3, 4))
    alpha = 0.3141592653589793
    res = [P.ops3dxs.cg_update(ctx, ux if with_x else None, up, ur, uq, n3, alpha, dtype=dtype) for _ in range(2)]
    xo, ro, rr = res[0]
    a = dtype(alpha)
    want_r = pool.memo(("r-aq", np.dtype(dtype).name), lambda: r - a * q)
    _check_out(n3, ur, ro, want_r, r)
    if with_x:
        _check_out(n3, ux, xo, x + a * p, x)
    ref = pool.sums(("rr", np.dtype(dtype).name), want_r, want_r)[0]
    assert _squares_ok(rr, ref, _stream_L(n3, dtype, count)), (rr, ref)
    assert res[1][2] == rr and bits_equal(res[1][1], ro)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dot2(ctx, pool, dtype):
    n3, count = pool.n3, BIG[pool.n3][0]
    assert _krylov_partials(n3, dtype) == count
    (a, pa), (b, pb), (c, pc) = (pool.get(dtype, s) for s in (1, 2, 3))
    ab, ac = P.ops3dxs.dot2(ctx, pa, pb, pc, n3, dtype=dtype)
    ab2, none = P.ops3dxs.dot2(ctx, pa, pb, None, n3, dtype=dtype)
    assert none is None and ab2 == ab
    assert (ab, ac) == P.ops3dxs.dot2(ctx, pa, pb, pc, n3, dtype=dtype)
    L = _stream_L(n3, dtype, count)
    name = np.dtype(dtype).name
    assert _signed_ok(ab, pool.sums(("ab", name), a, b), L), (ab, pool.sums(("ab", name), a, b))
    assert _signed_ok(ac, pool.sums(("ac", name), a, c), L), (ac, pool.sums(("ac", name), a, c))  # the second set of partials


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["x+p", "copy"])
def test_cg_direction(ctx, pool, dtype, form):
    n3 = pool.n3
    (x, ux), (p, up), (z, uz) = (pool.get(dtype, s) for s in (1, 2, 3))
    alpha, beta = -0.7071067811865476, 1.4142135623730951
    use_x = form == "x+p"
    (xo, po), (xo2, po2) = (P.ops3dxs.cg_direction(ctx, ux if use_x else None, up, uz, n3, alpha=alpha if use_x else None,
                                                   beta=beta if use_x else None, dtype=dtype) for _ in range(2))
    _check_out(n3, up, po, z + dtype(beta) * p if use_x else z, p)
    if use_x:
        _check_out(n3, ux, xo, x + dtype(alpha) * p, x)
    assert bits_equal(po2, po) and (not use_x or bits_equal(xo2, xo)), "not the same bits on every call"


# ---------------------------------------------------------------------------------------------------------- mixed kernels
def test_demote(ctx, pool):
    n3 = pool.n3
    (r, ur64), (r0, ur) = pool.get(np.float64, 1), pool.get(np.float32, 2)
    got, again = (P.ops3dxs.demote(ctx, ur64, ur, n3, S) for _ in range(2))
    _check_out(n3, ur, got, (r * S).astype(np.float32), r0)
    assert bits_equal(again, got), "not the same bits on every call"


@pytest.mark.parametrize("with_x", [True, False])
def test_cg_update_demote(ctx, pool, with_x):
    n3, count = pool.n3, BIG[pool.n3][0]
    assert _krylov_partials(n3) == count
    (x, ux), (p, up), (r, ur), (q, uq) = (pool.get(np.float64, s) for s in (1, 2, 3, 4))
    r0, u32 = pool.get(np.float32, 2)
    alpha = 0.3141592653589793
    res = [P.ops3dxs.cg_update_demote(ctx, ux if with_x else None, up, ur, uq, u32, n3, alpha, S) for _ in range(2)]
    xo, ro, o32, rr = res[0]
    want_r = pool.memo(("r-aq", "float64"), lambda: r - alpha * q)
    _check_out(n3, ur, ro, want_r, r)
    _check_out(n3, u32, o32, (want_r * S).astype(np.float32), r0)
    if with_x:
        _check_out(n3, ux, xo, x + alpha * p, x)
    ref = pool.sums(("rr", "float64"), want_r, want_r)[0]
    assert _squares_ok(rr, ref, _stream_L(n3, np.float64, count)), (rr, ref)
    assert res[1][3] == rr and bits_equal(res[1][2], o32) and bits_equal(res[1][1], ro)


def test_dot2_mixed(ctx, pool):
    n3, count = pool.n3, BIG[pool.n3][0]
    assert _krylov_partials(n3) == count
    (z, uz), (b, ub), (c, uc) = pool.get(np.float32, 1), pool.get(np.float64, 2), pool.get(np.float64, 3)
    zb, zc = P.ops3dxs.dot2_mixed(ctx, uz, INV, ub, uc, n3)
    zb2, none = P.ops3dxs.dot2_mixed(ctx, uz, INV, ub, None, n3)
    assert none is None and zb2 == zb
    assert (zb, zc) == P.ops3dxs.dot2_mixed(ctx, uz, INV, ub, uc, n3)
    zd = pool.memo("zd", lambda: z.astype(np.float64) * INV)
    L = _stream_L(n3, np.float64, count)
    assert _signed_ok(zb, pool.sums(("zb",), zd, b), L), (zb, pool.sums(("zb",), zd, b))
    assert _signed_ok(zc, pool.sums(("zc",), zd, c), L), (zc, pool.sums(("zc",), zd, c))


@pytest.mark.parametrize("form", ["x+p", "copy"])
def test_cg_direction_mixed(ctx, pool, form):
    n3 = pool.n3
    (x, ux), (p, up), (z, uz) = pool.get(np.float64, 1), pool.get(np.float64, 2), pool.get(np.float32, 1)
    alpha, beta = -0.7071067811865476, 1.4142135623730951
    use_x = form == "x+p"
    (xo, po), (xo2, po2) = (P.ops3dxs.cg_direction_mixed(ctx, ux if use_x else None, up, uz, INV, n3, alpha=alpha if use_x else None,
                                                         beta=beta if use_x else None) for _ in range(2))
    zd = pool.memo("zd", lambda: z.astype(np.float64) * INV)
    _check_out(n3, up, po, zd + beta * p if use_x else zd, p)
    if use_x:
        _check_out(n3, ux, xo, x + alpha * p, x)
    assert bits_equal(po2, po) and (not use_x or bits_equal(xo2, xo)), "not the same bits on every call"


def _crd_case(pool, rng, corr):
    """inputs and numpy results of correct_residual_demote on the pool's shape: (uploads, hosts, r, corrected x)"""
    n3 = pool.n3
    (x, ux), (b, ub), (z, uz), (r0, ur) = pool.get(np.float64, 1), pool.get(np.float64, 2), pool.get(np.float32, 1), pool.get(np.float32, 2)

    def xo_start():  # xo has x's boundary, as the solver's two iterate arrays have
        xo0 = x.copy()
        _interior(xo0)[...] = _interior(pool.get(np.float64, 3)[0])
        return xo0, pack_poisoned(xo0)
    xo0, uo = pool.memo("xo0", xo_start)

    def reference():
        xc = x.copy()
        if corr:
            _interior(xc)[...] = _interior(x + z.astype(np.float64) * INV)
        r = O.residual3d(n3, rng, xc, b, P.CORRECT, dtype=np.float64)
        return xc, r, (r * S).astype(np.float32), _fsum(_terms(r, r))
    xc, r, r32, rr = pool.memo(("crd", tuple(rng), bool(corr)), reference)
    return (ux, ub, uo, uz, ur), (x, xo0, r0), (xc, r, r32, rr)


def _crd_run(ctx, n3, rng, ups, corr):
    ux, ub, uo, uz, ur = ups
    return P.ops3dxs.correct_residual_demote(ctx, ux, ub, ur, n3, rng, S, z=uz if corr else None, inv_sz=INV, xo=uo if corr else None)


@pytest.mark.parametrize("corr,box", [(None, "aniso"), ("two launches", "aniso"), ("fused", "aniso"), ("fused", "pow2")])
def test_correct_residual_demote(ctx, pool, corr, box):
    n3, want_plan = pool.n3, BIG[pool.n3][1]
    rng = RG if box == "aniso" else _pow2_box(n3)
    ups, (x, xo0, r0), (xc, r, r32, rr_ref) = _crd_case(pool, rng, corr)
    ctx.set_param("mixed3d.fused", int(corr == "fused"))
    try:
        plan, p = _crd_plan(ctx, n3, rng, bool(corr))
        assert plan == want_plan == _crd_rule(n3), (plan, want_plan)
        assert p["rows"] == 4 and p["mode"] == (1 if box == "aniso" else 3) and p["launches"] == (2 if corr == "two launches" else 1)
        outs = [_crd_run(ctx, n3, rng, ups, corr) for _ in range(2)]
    finally:
        ctx.set_param("mixed3d.fused", 0)
    xo_st, r_st, rr = outs[0]
    _check_out(n3, ups[4], r_st, r32, r0)
    if corr:
        _check_out(n3, ups[2], xo_st, xc, xo0)
    else:
        assert xo_st is None
    assert _squares_ok(rr, rr_ref, _crd_L(n3, 4, plan[2], plan[0] * plan[1] * plan[3])), (rr, rr_ref)
    assert outs[1][2] == rr and bits_equal(outs[1][1], r_st) and (not corr or bits_equal(outs[1][0], xo_st)), "not the same bits"


# ---------------------------------------------------------------------------------------------------------- knobs
@pytest.fixture(scope="module")
def knob_pools():
    pools = {n3: Pool(n3) for n3 in KNOB_SHAPES}
    yield pools
    pools.clear()


@pytest.mark.parametrize("n3", KNOB_SHAPES, ids=_id)
@pytest.mark.parametrize("box", ["aniso", "pow2"])
@pytest.mark.parametrize("rows", [2, 4, 8])
def test_correct_residual_demote_knobs(ctx, knob_pools, n3, box, rows):
    """every run length (one plane, not dividing the plane count, longer than the level) with every row count: r32 and xo
    are the same bits for every setting, namely numpy's"""
    pool = knob_pools[n3]
    rng = RG if box == "aniso" else _pow2_box(n3)
    seen = set()
    try:
        ctx.set_param("mixed3d.rows", rows)
        for zchunk in ZCHUNKS:
            ctx.set_param("mixed3d.zchunk", zchunk)
            for corr in (None, "fused", "two launches"):
                ctx.set_param("mixed3d.fused", int(corr == "fused"))
                ups, (x, xo0, r0), (xc, r, r32, rr_ref) = _crd_case(pool, rng, corr)
                plan, p = _crd_plan(ctx, n3, rng, bool(corr))
                assert plan == _crd_rule(n3, rows, zchunk), (plan, rows, zchunk)
                # a chosen run length is taken as given; the automatic one (2 here, 4 at 2 rows per wave on the 4 x-blocks
                # of 387 x 131 x 69) is the rule's, compared above
                assert (plan[2] == zchunk if zchunk else plan[2] in (2, 4)) and p["rows"] == rows
                assert p["mode"] == (1 if box == "aniso" else 3)
                assert p["launches"] == (2 if corr == "two launches" else 1)
                xo_st, r_st, rr = _crd_run(ctx, n3, rng, ups, corr)
                what = (rows, zchunk, corr)
                if not bits_equal(r_st, pool.memo(("r32 stored", box, bool(corr)), lambda: _stored(r32, r0))):
                    _check_out(n3, ups[4], r_st, r32, r0)
                    raise AssertionError(what)
                if corr and not bits_equal(xo_st, pool.memo(("xo stored", box), lambda: _stored(xc, xo0))):
                    _check_out(n3, ups[2], xo_st, xc, xo0)
                    raise AssertionError(what)
                L = _crd_L(n3, rows, plan[2], plan[0] * plan[1] * plan[3])
                assert _squares_ok(rr, rr_ref, L), (what, rr, rr_ref, L)
                seen.add(plan[2:])
    finally:
        for name, value in (("mixed3d.rows", 4), ("mixed3d.zchunk", 0), ("mixed3d.fused", 0)):
            ctx.set_param(name, value)
    planes = n3[2] - 2
    auto = _crd_rule(n3, rows, 0)[2:]
    assert seen == {(1, planes), (2, _ceil(planes, 2)), (3, _ceil(planes, 3)), (5, _ceil(planes, 5)), (16, _ceil(planes, 16)), (64, 2), (128, 1), auto}


def test_knobs_refuse_what_has_no_kernel(ctx):
    n3 = KNOB_SHAPES[0]
    before = _crd_plan(ctx, n3, RG)
    for name, value in (("mixed3d.rows", 3), ("mixed3d.rows", 0), ("mixed3d.rows", 16), ("mixed3d.zchunk", -1)):
        with pytest.raises(P.MgxError) as e:
            ctx.set_param(name, value)
        assert e.value.status == P.MGX_ERR_INVALID, (name, value)
    assert _crd_plan(ctx, n3, RG) == before


# ---------------------------------------------------------------------------------------------------------- work arrays
def _mixed_work_elems(n3):
    fn = P.lib.mgx3dxs_mixed_work_elems_f64
    fn.restype = C.c_size_t
    return int(fn(_ip(n3)))


def test_work_guard_notices_one_double(ctx):
    ops = P.ops3dxs
    work, elems = ops._work_alloc(ctx, 7)
    try:
        ops._work_check(ctx, work, elems)
        one = np.array([1.0])
        P.check(P.lib.mgx_memcpy_h2d(ctx._h, C.c_void_p(work.value + 8 * elems), one.ctypes.data_as(C.c_void_p), C.c_size_t(8)))
        with pytest.raises(AssertionError):
            ops._work_check(ctx, work, elems)
    finally:
        ctx.free(work)


@pytest.mark.parametrize("n3", [(387, 131, 69), (771, 69, 41)], ids=_id)
def test_work_array_is_sized_for_the_smallest_tiles(ctx, n3):
    """2 rows per wave and one plane per run is the setting mgx3dxs_mixed_work_elems_f64 is sized for: on these shapes (4 and 7
    x-blocks) the z-marching pass then writes exactly that many partials, more than any Krylov kernel, and none behind them
    (the wrappers' guard); no other setting writes more"""
    pool = Pool(n3)
    krylov = 2 * _ceil(n3[1] - 2, 4) * (n3[2] - 2)
    try:
        for rows, zchunk in ((2, 1), (4, 0), (2, 0), (4, 1), (8, 1)):
            ctx.set_param("mixed3d.rows", rows)
            ctx.set_param("mixed3d.zchunk", zchunk)
            for corr in (None, "two launches"):
                ups, (x, xo0, r0), (xc, r, r32, rr_ref) = _crd_case(pool, RG, corr)
                plan, _ = _crd_plan(ctx, n3, RG, bool(corr))
                assert plan == _crd_rule(n3, rows, zchunk), (plan, rows, zchunk)
                count = plan[0] * plan[1] * plan[3]
                assert count <= _mixed_work_elems(n3)
                if (rows, zchunk) == (2, 1):
                    assert count == _ceil((n3[0] + 1) // 2 - 1, 63) * _ceil(n3[1] - 2, 8) * (n3[2] - 2) == _mixed_work_elems(n3) > krylov
                xo_st, r_st, rr = _crd_run(ctx, n3, RG, ups, corr)  # raises when a sentinel behind the work array was written
                assert bits_equal(r_st, pool.memo(("r32 stored", bool(corr)), lambda: _stored(r32, r0))), (rows, zchunk, corr)
                assert _squares_ok(rr, rr_ref, _crd_L(n3, rows, plan[2], count))
    finally:
        ctx.set_param("mixed3d.rows", 4)
        ctx.set_param("mixed3d.zchunk", 0)


# ---------------------------------------------------------------------------------------------------------- plane limit
def test_too_many_planes_are_refused_by_every_entry(ctx):
    """gridDim.y holds 65535 planes: 65537 interior planes are MGX_ERR_SIZE from every entry, and nothing is launched (arrays
    of the full size, the work array and the scalars all keep their bits)"""
    n3 = (5, 3, 65539)
    n = _ip(n3)
    assert _krylov_partials(n3) == 0 and _krylov_partials(n3, np.float32) == 0 and _mixed_work_elems(n3) == 0
    host = {dt: pack_poisoned(np.full(O.shape(n3), POISON[np.dtype(dt)], dt)) for dt in DTYPES}
    dev = {dt: [ctx.to_device(host[dt]) for _ in range(4)] for dt in DTYPES}
    wh = np.full(4096, POISON[np.dtype(np.float64)])
    sh = np.array([0.5, 0.25, 7.0, 7.0])
    work, sc = ctx.to_device(wh), ctx.to_device(sh)
    al, be, s0 = sc, C.c_void_p(sc.value + 8), C.c_void_p(sc.value + 16)
    L = P.lib
    h = ctx._h
    try:
        calls = []
        for sfx, dt, ct in (("f64", np.float64, C.c_double), ("f32", np.float32, C.c_float)):
            a, b, c, d = dev[dt]
            hh = _rp(grid_spacing(n3, RG, dt), ct)
            calls += [("laplace_dot_" + sfx, getattr(L, "mgx3dxs_laplace_dot_" + sfx)(h, a, b, n, hh, work, s0)),
                      ("cg_update_" + sfx, getattr(L, "mgx3dxs_cg_update_" + sfx)(h, a, b, c, d, n, al, work, s0)),
                      ("dot2_" + sfx, getattr(L, "mgx3dxs_dot2_" + sfx)(h, a, b, c, n, work, s0)),
                      ("cg_direction_" + sfx, getattr(L, "mgx3dxs_cg_direction_" + sfx)(h, a, b, c, n, al, be))]
        a, b, c, d = dev[np.float64]
        z32, r32 = dev[np.float32][:2]
        hh = _rp(grid_spacing(n3, RG, np.float64), C.c_double)
        s, inv = C.c_double(S), C.c_double(INV)
        calls += [("demote", L.mgx3dxs_demote_f64(h, a, r32, s, n)),
                  ("cg_update_demote", L.mgx3dxs_cg_update_demote_f64(h, a, b, c, d, r32, s, n, al, work, s0)),
                  ("dot2_mixed", L.mgx3dxs_dot2_mixed_f64(h, z32, inv, a, b, n, work, s0)),
                  ("cg_direction_mixed", L.mgx3dxs_cg_direction_mixed_f64(h, a, b, z32, inv, n, al, be)),
                  ("correct_residual_demote", L.mgx3dxs_correct_residual_demote_f64(h, a, b, c, z32, inv, r32, s, n, hh, work, s0)),
                  ("correct_residual_demote, no correction", L.mgx3dxs_correct_residual_demote_f64(h, a, None, c, None, inv, r32, s, n, hh, work, s0)),
                  ("correct_residual_demote_plan", L.mgx3dxs_correct_residual_demote_plan_f64(h, n, hh, 0, (C.c_int * 7)()))]
        assert [name for name, st in calls if st != P.MGX_ERR_SIZE] == [], calls
        assert b"planes" in P.lib.mgx_last_error()
        ctx.sync()
        for dt in DTYPES:
            for p in dev[dt]:
                assert bits_equal(ctx.to_host(p, host[dt].shape, dt), host[dt]), "an array was written"
        assert bits_equal(ctx.to_host(work, wh.shape, np.float64), wh) and bits_equal(ctx.to_host(sc, sh.shape, np.float64), sh)
    finally:
        for p in dev[np.float64] + dev[np.float32] + [work, sc]:
            ctx.free(p)


@pytest.mark.parametrize("zchunk", [0, 1])
def test_the_most_planes_accepted(ctx, zchunk):
    """65535 interior planes, the most gridDim.y (and, with one plane per run, gridDim.z) holds"""
    n3 = (5, 3, 65537)
    pool = Pool(n3)
    count = 65535
    assert _krylov_partials(n3) == count and _mixed_work_elems(n3) == 2 * count
    if zchunk == 0:
        for dtype in DTYPES:
            name = np.dtype(dtype).name
            (p, pp), (q0, qp), (r, ur), (q, uq) = (pool.get(dtype, s) for s in (1, 2, 3, 4))
            q_st, pq = P.ops3dxs.laplace_dot(ctx, pp, n3, RG, q=qp, packed=True, dtype=dtype)
            want = -O.residual3d(n3, RG, p, np.zeros_like(p), P.CORRECT, dtype=dtype)
            _check_out(n3, qp, q_st, want, q0)
            assert _signed_ok(pq, pool.sums(("pAp", name), p, want), _stream_L(n3, dtype, count))
            alpha = 0.3141592653589793
            xo, ro, rr = P.ops3dxs.cg_update(ctx, pp, qp, ur, uq, n3, alpha, dtype=dtype)
            want_r = r - dtype(alpha) * q
            _check_out(n3, ur, ro, want_r, r)
            _check_out(n3, pp, xo, p + dtype(alpha) * q0, p)
            assert _squares_ok(rr, pool.sums(("rr", name), want_r, want_r)[0], _stream_L(n3, dtype, count))
    try:
        ctx.set_param("mixed3d.zchunk", zchunk)
        for corr in (None, "fused"):
            ctx.set_param("mixed3d.fused", int(corr == "fused"))
            ups, (x, xo0, r0), (xc, r, r32, rr_ref) = _crd_case(pool, RG, corr)
            plan, _ = _crd_plan(ctx, n3, RG, bool(corr))
            assert plan == ((1, 1, 16, 4096) if zchunk == 0 else (1, 1, 1, 65535)) == _crd_rule(n3, 4, zchunk)
            xo_st, r_st, rr = _crd_run(ctx, n3, RG, ups, corr)
            _check_out(n3, ups[4], r_st, r32, r0)
            if corr:
                _check_out(n3, ups[2], xo_st, xc, xo0)
            assert _squares_ok(rr, rr_ref, _crd_L(n3, 4, plan[2], plan[3]))
    finally:
        ctx.set_param("mixed3d.zchunk", 0)
        ctx.set_param("mixed3d.fused", 0)


# ---------------------------------------------------------------------------------------------------------- solves
_WANT = {}


def _mg(ctx, n3, rng, f):
    mg = P.MultiGrid3D(ctx, n3, rng, np.float64, residual_mode=P.CORRECT)
    mg.upload_v(0, np.zeros(O.shape(n3)))
    mg.upload_f(0, f)
    return mg


def _ir_want(n3, rng, steps):
    key = (n3, tuple(rng))
    if key not in _WANT or len(_WANT[key][1]) < steps:
        _WANT.clear()  # one size at a time: these are large
        f = R.problem(n3)
        _WANT[key] = (f, R.ir_restated(n3, rng, np.zeros_like(f), f, 2, 2, steps))
    return _WANT[key]


def _defect_correction(ctx, n3, rng, fused, steps_list):
    f, want = _ir_want(n3, rng, max(steps_list))
    ctx.set_param("mixed3d.fused", fused)
    try:
        for steps in steps_list:
            mg = _mg(ctx, n3, rng, f)
            k, rel, conv, hist = mg.PCG(2, 2, 1e-300, steps, krylov=False, precond="f32")
            x = mg.download_v(0)
            mg.close()
            assert k == steps and not conv and len(hist) == steps
            assert bits_equal(x, want[steps - 1]), (steps, _where(x, want[steps - 1]))
            assert R.close(rel, R.true_rel(n3, rng, x, f, np.zeros_like(f)), 1e-10)
    finally:
        ctx.set_param("mixed3d.fused", 0)


@pytest.mark.parametrize("fused", [0, 1])
def test_defect_correction_257(ctx, fused):
    n3 = (257, 257, 257)
    assert _krylov_partials(n3) == 16320 and _crd_plan(ctx, n3, UNIT)[0] == (3, 16, 8, 32)
    _defect_correction(ctx, n3, UNIT, fused, (1, 2))


@pytest.mark.timeout(600)
def test_defect_correction_step_513(ctx):
    """the headline size of the mixed solve: x after one step = x0 + M(b - A x0) with the oracle's fp32 V-cycle, bit for bit"""
    n3 = (513, 513, 513)
    assert _krylov_partials(n3) == 65408 and _crd_plan(ctx, n3, UNIT)[0] == (5, 32, 16, 32)
    _defect_correction(ctx, n3, UNIT, 0, (1,))
    _WANT.clear()


def test_defect_correction_odd_hierarchy(ctx):
    """rows of 192 pairs; the fp32 twin and the fp64 hierarchy have different pads on the three finest levels (385, 193 and 97
    points per row), all six levels are odd"""
    n3 = (385, 129, 65)
    assert hierarchy_ok(n3) and len(levels(n3)) == 6
    assert all(xs_geometry(k[0], 8) != xs_geometry(k[0], 4) for k in levels(n3)[:3])
    _defect_correction(ctx, n3, RG, 0, (2,))
    _WANT.clear()


@pytest.mark.parametrize("precond", ["f64", "f32"])
def test_flexible_cg_257(ctx, precond):
    """the Krylov kernels and cg_final_kernel at 4064 partials under a comparison of the whole history"""
    n3, rng = (257, 129, 129), [0, 1, 0, 1, 0, 2]
    assert _krylov_partials(n3) == 4064
    f = R.problem(n3)
    M = R.m_cycle(n3, rng, 2, 2) if precond == "f64" else R.m32(n3, rng, 2, 2)
    want_x, want_k, want_h, want_c = R.fcg_restated(n3, rng, np.zeros_like(f), f, M, 1e-10, 200)
    mg = _mg(ctx, n3, rng, f)
    k, rel, conv, hist = mg.PCG(2, 2, 1e-10, 200, precond=precond)
    x = mg.download_v(0)
    mg.close()
    assert conv and want_c and rel < 1e-10
    assert abs(k - want_k) <= 1, (k, want_k)
    m = min(len(hist), len(want_h))
    upto = want_h[:m] >= 1e-10
    assert np.allclose(hist[:m][upto], want_h[:m][upto], rtol=1e-6, atol=0), (hist[:m], want_h[:m])
    assert np.abs(x - want_x).max() <= 1e-9 * np.abs(want_x).max()
