"""GPU suite: the face-unknown kernels on lists that one launch does not cover.

Every operation on the face unknowns runs through RIM_FOR_EACH_POINT (csrc/mgx_rim3d.hpp): at most 4096 blocks of 256 threads that
stride over the list of face points.  The other files' longest list has 8,466 entries: there the loop body runs once per thread.
The solver's own sizes stride -- the closed box at 513^3 lists 1.6 M entries -- so the colour passes, residuals, operator
applications, transfers and vector entries are run here on the thin shapes of tests/long_lists.py, whose lists take two, three and
five rounds (test_long_lists_cpu.py proves that without a GPU), and compared as at the small shapes: arrays bit for bit against
tests/op_restated.py with poisoned pads, read-only arguments and Dirichlet entries unchanged, sums to 1e-13 of the sum of the
absolute terms, equal on two runs, with NaN guards behind the work array (the rim launch writes up to 4096 partials behind the
interior launch's 384).  A failure names the lowest round of the list in which a wrong point lies (long_lists.diagnose): round 0
is the loop body, a later one the stride or what a thread carries between rounds.

A case is one shape in one precision, its masks in a loop; the operators behind the wrappers (walls, a capacity, harmonic-mean
faces) have cases of their own, so that no case takes more than a few seconds in its numpy references."""
import ctypes as C
import math

import numpy as np
import pytest

import long_lists as LL
import op_cases as OC
import op_restated as OP
import oracle as O
import pde_multigrid_amd as P
from conftest import bits_equal
from odd_shapes import pads_unchanged, run_poisoned
from pde_multigrid_amd.multigrid import _ct, _ip, _rp, xs_unpack
from test_gpu_neumann_krylov import FACES, Work, _fn, _h, _rand

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]
UNIT = [0, 1, 0, 1, 0, 1]
S = 0.75
DTYPES = LL.DTYPES
VEC_MASKS = {"A": [48, 63], "B": [63]}


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


def same(got, want, n3, bc, dtype, what):
    """got has want's bits; else the failure names the lowest round of the list of (n3, bc) with a wrong point"""
    d = LL.diagnose(got, want, LL.round_of(n3, bc, dtype))
    assert d is None, (what, "mask %d" % bc, d)


def fsum_ref(terms):
    """(math.fsum(terms), math.fsum(|terms|)): a sum's reference and its scale, computed once per sum"""
    terms = np.asarray(terms, np.float64).ravel()
    return math.fsum(terms), math.fsum(np.abs(terms))


def near(got, ref, rtol=1e-13):
    return abs(got - ref[0]) <= rtol * ref[1]


def _unchanged(ups, outs, idx):
    return all(bits_equal(outs[i], ups[i]) for i in idx)


def _coef(n3, dtype):
    return _rand(n3, dtype, 3, 0.5, 2.0)


def _cap(n3, dtype):
    return OC.random_capacity(n3, dtype, 200)


def test_the_lists_of_this_file_take_more_than_one_round():
    for name, n3, bc, entries, rounds in LL.TABLE:
        for k, dtype in enumerate(DTYPES):
            assert LL.rounds(n3, bc, dtype) == rounds[k] >= 2


# ---------------------------------------------------------------------------------------------------------- colour passes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", "ABY")
def test_relax_bc(ctx, name, dtype):
    """relax_shift_bc and relax_coef_bc as stored, with poisoned pads: one sweep, on A two as well (the second sweep reads what the
    first one's later rounds wrote)"""
    for bc in LL.MASKS[name]:
        _relax_bc(ctx, name, bc, dtype)


def _relax_bc(ctx, name, bc, dtype):
    n3 = LL.SHAPES[name]
    v, f, a = _rand(n3, dtype, 1), _rand(n3, dtype, 2), _coef(n3, dtype)
    unk = OP.unknown_mask(n3, bc)
    for coef in (False, True):
        fn, ct = _fn("relax_coef_bc" if coef else "relax_shift_bc", dtype)
        op = OP.Op(n3, RG, dtype, S, a if coef else None, bc=bc)
        for sweeps in ((1, 2) if name == "A" else (1,)):
            tail = lambda: (_ip(n3), _h(n3, RG, dtype), ct(S), C.c_int(sweeps), C.c_int(bc))
            if coef:
                ups, outs = run_poisoned(ctx, [v, f, a], lambda x, b, c: fn(ctx._h, x, b, c, *tail()), dtype)
            else:
                ups, outs = run_poisoned(ctx, [v, f], lambda x, b: fn(ctx._h, x, b, *tail()), dtype)
            got = xs_unpack(outs[0], n3[0])
            same(got, op.relax(v, f, sweeps), n3, bc, dtype, (coef, sweeps))
            assert bits_equal(got[~unk], v[~unk]), "a Dirichlet entry of v was written"
            assert pads_unchanged(ups[0], outs[0], n3[0]) and _unchanged(ups, outs, range(1, len(ups))), (coef, sweeps)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", "ABY")
def test_relax_wall_and_hmean(ctx, name, dtype):
    """all six faces with every second one a convective wall: the capacity operator, and harmonic-mean faces with and without a
    capacity, through the wrappers"""
    n3, bc = LL.SHAPES[name], 63
    beta = OC.mixed_betas(bc)
    v, f, a, c = _rand(n3, dtype, 1), _rand(n3, dtype, 2), _coef(n3, dtype), _cap(n3, dtype)
    got = P.ops3dxs.relax_wall(ctx, v, f, a, c, n3, RG, S, 1, bc, beta)
    same(got, OP.Op(n3, RG, dtype, S, a, c, bc, beta).relax(v, f, 1), n3, bc, dtype, "relax_wall, capacity")
    for cc in (None, c):
        got = P.ops3dxs.relax_hmean(ctx, v, f, a, n3, RG, S, 1, c=cc, bc=bc, beta=beta)
        same(got, OP.Op(n3, RG, dtype, S, a, cc, bc, beta, "harmonic").relax(v, f, 1), n3, bc, dtype, ("relax_hmean", cc is not None))


# ---------------------------------------------------------------------------------------------------------- residual
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", "ABY")
def test_residual_bc(ctx, name, dtype):
    """stored and summed (twice), the sum alone, r alone.  With a sum the face launch is clamped to the interior launch's block
    count (384 on A and B, 511 on Y): every thread strides about eleven times"""
    for bc in LL.MASKS[name]:
        _residual_bc(ctx, name, bc, dtype)


def _residual_bc(ctx, name, bc, dtype):
    n3 = LL.SHAPES[name]
    v, f, r0, a = _rand(n3, dtype, 5), _rand(n3, dtype, 6), _rand(n3, dtype, 7), _coef(n3, dtype)
    w = Work(ctx, n3, dtype)
    try:
        for coef in (False, True):
            fn, ct = _fn("residual_coef_bc" if coef else "residual_shift_bc", dtype)
            ins = [v, f, a] if coef else [v, f]

            def run(store, summed):
                def call(*p):
                    return fn(ctx._h, *p[:len(ins)], p[len(ins)] if store else None, _ip(n3), _h(n3, RG, dtype), ct(S), w.work if summed else None,
                              w.sum if summed else None, C.c_int(bc))
                return run_poisoned(ctx, ins + [r0] if store else ins, call, dtype)

            want = OP.Op(n3, RG, dtype, S, a if coef else None, bc=bc).residual(v, f)
            ref = fsum_ref(want.astype(np.float64) ** 2)
            sums = []
            for rep in range(2):
                ups, outs = run(True, True)
                same(xs_unpack(outs[-1], n3[0]), want, n3, bc, dtype, (coef, rep))  # the Dirichlet points written as 0
                assert _unchanged(ups, outs, range(len(ins))) and pads_unchanged(ups[-1], outs[-1], n3[0])
                sums.append(w.result())
            assert sums[0] == sums[1], "two runs gave different sums"
            assert near(sums[0], ref), (coef, sums[0], ref)
            ups, outs = run(False, True)  # the sum alone
            assert w.result() == sums[0] and _unchanged(ups, outs, range(len(ins)))
            ups, outs = run(True, False)  # r alone: the full launch
            same(xs_unpack(outs[-1], n3[0]), want, n3, bc, dtype, (coef, "r alone"))
            assert pads_unchanged(ups[-1], outs[-1], n3[0])
    finally:
        w.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", "ABY")
def test_residual_wall_and_hmean(ctx, name, dtype):
    n3, bc = LL.SHAPES[name], 63
    beta = OC.mixed_betas(bc)
    v, f, a, c = _rand(n3, dtype, 5), _rand(n3, dtype, 6), _coef(n3, dtype), _cap(n3, dtype)
    X = P.ops3dxs
    cases = [("residual_wall, capacity", OP.Op(n3, RG, dtype, S, a, c, bc, beta), lambda **k: X.residual_wall(ctx, v, f, a, c, n3, RG, S, bc, beta, **k))]
    for cc in (None, c):
        cases.append((("residual_hmean", cc is not None), OP.Op(n3, RG, dtype, S, a, cc, bc, beta, "harmonic"),
                      lambda cc=cc, **k: X.residual_hmean(ctx, v, f, a, n3, RG, S, c=cc, bc=bc, beta=beta, **k)))
    for what, op, call in cases:
        want = op.residual(v, f)
        ref = fsum_ref(want.astype(np.float64) ** 2)
        r, ss = call()
        same(r, want, n3, bc, dtype, what)
        assert near(ss, ref), (what, ss, ref)
        assert call(store=False) == (None, ss), (what, "the sum alone")
        r2, none = call(want_sum=False)
        same(r2, want, n3, bc, dtype, (what, "r alone"))
        assert none is None and call()[1] == ss, (what, "two runs gave different sums")


# ---------------------------------------------------------------------------------------------------------- q = A p and <p, q>_W
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", "AB")
def test_apply_dot_bc(ctx, name, dtype):
    for bc in LL.MASKS[name]:
        _apply_dot_bc(ctx, name, bc, dtype)


def _apply_dot_bc(ctx, name, bc, dtype):
    n3 = LL.SHAPES[name]
    p, q0, a = _rand(n3, dtype, 1), _rand(n3, dtype, 2), _coef(n3, dtype)
    unk, W = OP.unknown_mask(n3, bc), OP.weights(n3, bc)
    w = Work(ctx, n3, dtype)
    try:
        for coef in (False, True):
            fn, ct = _fn("apply_coef_dot_bc" if coef else "laplace_dot_shift_bc", dtype)
            ins = [p, a] if coef else [p]
            want = q0.copy()
            want[unk] = OP.Op(n3, RG, dtype, S, a if coef else None, bc=bc).apply_A(p)[unk]  # the Dirichlet entries of q are not written
            ref = fsum_ref(W * p.astype(np.float64) * want.astype(np.float64))
            sums = []
            for rep in range(2):
                ups, outs = run_poisoned(ctx, ins + [q0], lambda *d: fn(ctx._h, *d, _ip(n3), _h(n3, RG, dtype), ct(S), w.work, w.sum, C.c_int(bc)),
                                         dtype)
                same(xs_unpack(outs[-1], n3[0]), want, n3, bc, dtype, (coef, rep))
                assert _unchanged(ups, outs, range(len(ins))) and pads_unchanged(ups[-1], outs[-1], n3[0])
                sums.append(w.result())  # ... and the guards behind the work array are intact
            assert sums[0] == sums[1], "two runs gave different sums"
            assert near(sums[0], ref), (coef, sums[0], ref)
    finally:
        w.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", "AB")
def test_apply_dot_wall_and_hmean(ctx, name, dtype):
    n3, bc = LL.SHAPES[name], 63
    beta = OC.mixed_betas(bc)
    p, a, c = _rand(n3, dtype, 8), _coef(n3, dtype), _cap(n3, dtype)
    unk, W = OP.unknown_mask(n3, bc), OP.weights(n3, bc)
    X = P.ops3dxs
    cases = [("apply_dot_wall, capacity", OP.Op(n3, RG, dtype, S, a, c, bc, beta), lambda: X.apply_dot_wall(ctx, p, a, c, n3, RG, S, bc, beta)),
             ("apply_hmean_dot", OP.Op(n3, RG, dtype, S, a, None, bc, beta, "harmonic"),
              lambda: X.apply_hmean_dot(ctx, p, a, n3, RG, S, bc=bc, beta=beta))]
    for what, op, call in cases:
        want = np.zeros(O.shape(n3), dtype)
        want[unk] = op.apply_A(p)[unk]  # the wrapper's zero-filled q, its Dirichlet entries unwritten
        q, pq = call()  # (the wrapper looks at its own guards behind the work array)
        same(q, want, n3, bc, dtype, what)
        assert near(pq, fsum_ref(W * p.astype(np.float64) * want.astype(np.float64))), (what, pq)
        q2, pq2 = call()
        assert bits_equal(q2, q) and pq2 == pq, (what, "two runs differ")


# ---------------------------------------------------------------------------------------------------------- transfers
@pytest.mark.parametrize("dtype", DTYPES)
def test_transfers_bc(ctx, dtype):
    """restrict_bc lists the coarse grid C (two rounds), interpolate_bc and interpolate_correct_bc the fine grid F (five)"""
    for bc in LL.MASKS["F"]:
        _transfers_bc(ctx, bc, dtype)


def _transfers_bc(ctx, bc, dtype):
    fn3, cn3 = LL.F, LL.C
    fine, coarse = _rand(fn3, dtype, 11), _rand(cn3, dtype, 12)
    rfn, _ = _fn("restrict_bc", dtype)
    ups, outs = run_poisoned(ctx, [fine, coarse], lambda a, b: rfn(ctx._h, a, _ip(fn3), b, _ip(cn3), C.c_int(bc)), dtype)
    same(xs_unpack(outs[1], cn3[0]), OP.restrict(fn3, fine, bc, dtype), cn3, bc, dtype, "restrict")
    assert bits_equal(outs[0], ups[0]) and pads_unchanged(ups[1], outs[1], cn3[0])
    unk = OP.unknown_mask(fn3, bc)
    for add, name in ((False, "interpolate_bc"), (True, "interpolate_correct_bc")):
        kfn, _ = _fn(name, dtype)
        ups, outs = run_poisoned(ctx, [fine, coarse], lambda a, b: kfn(ctx._h, a, _ip(fn3), b, _ip(cn3), C.c_int(bc)), dtype)
        got = xs_unpack(outs[0], fn3[0])
        same(got, OP.interpolate(fn3, fine, coarse, bc, dtype, add=add), fn3, bc, dtype, name)
        assert bits_equal(got[~unk], fine[~unk]), "a Dirichlet entry was written"
        assert bits_equal(outs[1], ups[1]) and pads_unchanged(ups[0], outs[0], fn3[0])


# ---------------------------------------------------------------------------------------------------------- vector entries
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", "AB")
def test_vector_entries_that_write(ctx, name, dtype):
    """set_rim_bc, shift_rhs_bc, cap_rhs_bc, wall_rhs and the five forms of cg_direction_bc"""
    for bc in VEC_MASKS[name]:
        _vector_entries_that_write(ctx, name, bc, dtype)


def _vector_entries_that_write(ctx, name, bc, dtype):
    n3 = LL.SHAPES[name]
    ct = _ct(dtype)[1]
    unk, rim = OP.unknown_mask(n3, bc), OP.face_unknowns(n3, bc)
    u, q, f0, c = _rand(n3, dtype, 13), _rand(n3, dtype, 14), _rand(n3, dtype, 15), _cap(n3, dtype)
    # set_rim_bc: the interior and the Dirichlet entries as they were
    fn = _fn("set_rim_bc", dtype)[0]
    for value in (0.0, -2.5):
        ups, outs = run_poisoned(ctx, [u], lambda a: fn(ctx._h, a, _ip(n3), ct(value), C.c_int(bc)), dtype)
        want = u.copy()
        want[rim] = value
        same(xs_unpack(outs[0], n3[0]), want, n3, bc, dtype, ("set_rim_bc", value))
        assert pads_unchanged(ups[0], outs[0], n3[0])
    # shift_rhs_bc and cap_rhs_bc, with and without q: the Dirichlet entries of f as they were
    fn = _fn("shift_rhs_bc", dtype)[0]
    op = OP.Op(n3, UNIT, dtype, S, bc=bc)
    ups, outs = run_poisoned(ctx, [u, q, f0], lambda a, b, d: fn(ctx._h, a, b, ct(0.3), ct(S), d, _ip(n3), C.c_int(bc)), dtype)
    same(xs_unpack(outs[2], n3[0]), op.rhs(u, q, 0.3, f=f0), n3, bc, dtype, "shift_rhs_bc")
    assert _unchanged(ups, outs, [0, 1]) and pads_unchanged(ups[2], outs[2], n3[0])
    ups, outs = run_poisoned(ctx, [u, f0], lambda a, d: fn(ctx._h, a, None, ct(0.3), ct(S), d, _ip(n3), C.c_int(bc)), dtype)
    same(xs_unpack(outs[1], n3[0]), op.rhs(u, None, 0.3, f=f0), n3, bc, dtype, "shift_rhs_bc without q")
    assert _unchanged(ups, outs, [0]) and pads_unchanged(ups[1], outs[1], n3[0])
    fn = _fn("cap_rhs_bc", dtype)[0]
    op = OP.Op(n3, UNIT, dtype, S, c=c, bc=bc)
    ups, outs = run_poisoned(ctx, [u, c, f0, q], lambda a, cc, d, b: fn(ctx._h, a, cc, b, ct(0.3), ct(S), d, _ip(n3), C.c_int(bc)), dtype)
    same(xs_unpack(outs[2], n3[0]), op.rhs(u, q, 0.3, f=f0), n3, bc, dtype, "cap_rhs_bc")
    assert _unchanged(ups, outs, [0, 1, 3]) and pads_unchanged(ups[2], outs[2], n3[0])
    ups, outs = run_poisoned(ctx, [u, c, f0], lambda a, cc, d: fn(ctx._h, a, cc, None, ct(0.3), ct(S), d, _ip(n3), C.c_int(bc)), dtype)
    same(xs_unpack(outs[2], n3[0]), op.rhs(u, None, 0.3, f=f0), n3, bc, dtype, "cap_rhs_bc without q")
    assert _unchanged(ups, outs, [0, 1]) and pads_unchanged(ups[2], outs[2], n3[0])
    # wall_rhs with fluxes on every second flagged face: nothing else of f
    fn = _fn("wall_rhs", dtype)[0]
    g = tuple(-x for x in OC.mixed_betas(bc))
    ups, outs = run_poisoned(ctx, [f0], lambda a: fn(ctx._h, a, _ip(n3), _h(n3, RG, dtype), _rp(g, ct), C.c_int(bc)), dtype)
    got = xs_unpack(outs[0], n3[0])
    same(got, OP.Op(n3, RG, dtype, 0.0, bc=bc).add_flux(f0, g), n3, bc, dtype, "wall_rhs")
    changed = got != f0
    assert pads_unchanged(ups[0], outs[0], n3[0]) and (changed <= rim).all() and changed.any()
    # cg_direction_bc (x updated?, z given?, beta given?): the three forms of the solver and the two the entry takes besides
    x, p, z = (_rand(n3, dtype, k) for k in (11, 12, 13))
    alpha, beta = 0.37, -0.21
    al, be = dtype(alpha), dtype(beta)
    fn = _fn("cg_direction_bc", dtype)[0]
    w = Work(ctx, n3, dtype, (alpha, beta))
    try:
        for fx, fz, fb in [(False, True, False), (True, True, True), (True, False, False), (True, True, False), (False, True, True)]:
            wx, wp = x.copy(), p.copy()
            if fx:
                wx[unk] = (x + al * p)[unk]
            if fz:
                wp[unk] = (z + be * p)[unk] if fb else z[unk]
            ups, outs = run_poisoned(ctx, [x, p, z], lambda xd, pd, zd: fn(ctx._h, xd if fx else None, pd, zd if fz else None, _ip(n3),
                                                                          w.alpha if fx else None, w.beta if fb else None, C.c_int(bc)), dtype)
            same(xs_unpack(outs[0], n3[0]), wx, n3, bc, dtype, ("cg_direction_bc x", fx, fz, fb))
            same(xs_unpack(outs[1], n3[0]), wp, n3, bc, dtype, ("cg_direction_bc p", fx, fz, fb))
            assert bits_equal(outs[2], ups[2]) and pads_unchanged(ups[0], outs[0], n3[0]) and pads_unchanged(ups[1], outs[1], n3[0])
    finally:
        w.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", "AB")
def test_vector_entries_that_sum(ctx, name, dtype):
    """cg_update_bc with and without x, dot2_bc with one and two sums (the two sums' rim partials lie behind both interior sums and
    have a final of their own) and project_bc"""
    for bc in VEC_MASKS[name]:
        _vector_entries_that_sum(ctx, name, bc, dtype)


def _vector_entries_that_sum(ctx, name, bc, dtype):
    n3 = LL.SHAPES[name]
    unk, W = OP.unknown_mask(n3, bc), OP.weights(n3, bc)
    x, p, r, q = (_rand(n3, dtype, k) for k in (4, 5, 6, 7))
    alpha = 0.37
    al = dtype(alpha)
    fn = _fn("cg_update_bc", dtype)[0]
    w = Work(ctx, n3, dtype, (alpha, 0.0))
    try:
        wx, wr = x.copy(), r.copy()
        wx[unk] = (x + al * p)[unk]
        wr[unk] = (r - al * q)[unk]
        ref = fsum_ref(wr[unk].astype(np.float64) ** 2)  # unweighted
        for with_x in (True, False):
            sums = []
            for rep in range(2):
                ups, outs = run_poisoned(ctx, [x, p, r, q], lambda xd, pd, rd, qd: fn(ctx._h, xd if with_x else None, pd, rd, qd, _ip(n3), w.alpha,
                                                                                       w.work, w.sum, C.c_int(bc)), dtype)
                same(xs_unpack(outs[0], n3[0]), wx if with_x else x, n3, bc, dtype, ("cg_update_bc x", with_x))
                same(xs_unpack(outs[2], n3[0]), wr, n3, bc, dtype, ("cg_update_bc r", with_x))
                assert _unchanged(ups, outs, [1, 3]) and pads_unchanged(ups[0], outs[0], n3[0]) and pads_unchanged(ups[2], outs[2], n3[0])
                sums.append(w.result())
            assert sums[0] == sums[1], "two runs gave different sums"
            assert near(sums[0], ref), (with_x, sums[0], ref)
        # dot2_bc
        fn = _fn("dot2_bc", dtype)[0]
        a64, b64, c64 = (t.astype(np.float64) for t in (x, p, r))
        ref_ab, ref_ac = fsum_ref(W * a64 * b64), fsum_ref(W * a64 * c64)
        for two in (True, False):
            sums = []
            for rep in range(2):
                ups, outs = run_poisoned(ctx, [x, p, r], lambda ad, bd, cd: fn(ctx._h, ad, bd, cd if two else None, _ip(n3), w.work, w.sum,
                                                                              C.c_int(bc)), dtype)
                assert _unchanged(ups, outs, range(3))
                sums.append(w.result(2))
            assert sums[0][0] == sums[1][0] and (not two or sums[0][1] == sums[1][1]), "two runs gave different sums"
            assert near(sums[0][0], ref_ab), (two, sums[0], ref_ab)
            assert not two or near(sums[0][1], ref_ac), (two, sums[0], ref_ac)
        # project_bc: the downloaded mean, rounded to the arrays' precision, is subtracted at every unknown
        fn = _fn("project_bc", dtype)[0]
        a = _rand(n3, dtype, 14, -0.5, 1.5)
        ref = fsum_ref(W * a.astype(np.float64))
        sw = OP.sum_weights(n3, bc)
        means = []
        for rep in range(2):
            ups, outs = run_poisoned(ctx, [a], lambda ad: fn(ctx._h, ad, _ip(n3), w.work, w.sum, C.c_int(bc)), dtype)
            mean = w.result()
            want = a.copy()
            want[unk] = (a - dtype(mean))[unk]
            same(xs_unpack(outs[0], n3[0]), want, n3, bc, dtype, "project_bc")
            assert pads_unchanged(ups[0], outs[0], n3[0])
            means.append(mean)
        assert means[0] == means[1], "two runs gave different means"
        assert near(means[0] * sw, ref), (means[0], ref)
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------------------- hierarchy
def _mg(ctx, dtype, coef, v, f):
    n3 = LL.A
    mg = P.MultiGrid3D(ctx, n3, RG, dtype, residual_mode=P.CORRECT, shift=S, coefficient=OC.smooth_coefficient(n3, dtype) if coef else None,
                       neumann=FACES(63))
    mg.upload_v(0, v)
    mg.upload_f(0, f)
    return mg


def _same_levels(mg, H, dtype, what):
    assert mg.maxGrids == len(H.sizes) == 2
    for l, n in enumerate(H.sizes):
        assert mg.size(l) == n
        same(mg.download_v(l), H.v[l], n, 63, dtype, (what, "v", l))
        if l > 0:
            same(mg.download_f(l), H.f[l], n, 63, dtype, (what, "f", l))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("coef", [False, True])
def test_vcycles_on_two_levels_eagerly_and_through_a_graph(ctx, coef, dtype):
    """the closed box on A: the levels (1025, 513, 5) and (513, 257, 3); level 0's lists take two rounds in every colour pass,
    residual and transfer of the cycle"""
    n3 = LL.A
    v, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    H = OP.Hierarchy(OP.Op(n3, RG, dtype, S, OC.smooth_coefficient(n3, dtype) if coef else None, bc=63))
    assert H.sizes == [n3, (513, 257, 3)]
    H.v[0], H.f[0] = v.copy(), f.copy()
    mg = _mg(ctx, dtype, coef, v, f)
    try:
        H.vcycle(0, 2, 2)
        mg.VCycle(0, 2, 2)
        _same_levels(mg, H, dtype, "eager")
        first = [H.v[0].copy(), H.v[1].copy(), H.f[1].copy()]
        H.vcycle(0, 2, 2)
        mg.VCycle(0, 2, 2)
        _same_levels(mg, H, dtype, "second")
        H.v[0], H.v[1], H.f[1] = first
        mg.use_graph = True
        execs = []
        for rep in range(2):  # capture, then replay
            mg.upload_v(0, v)
            mg.VCycle(0, 2, 2)
            _same_levels(mg, H, dtype, ("graph", rep))
            execs.append(mg._mg.contents.graph_exec[0])
        assert execs[0] and execs[1] == execs[0], "the cycle was captured again instead of replayed"
    finally:
        mg.close()


def test_three_iterations_of_weighted_cg(ctx):
    """PCG(2, 2, 1e-10, 3, krylov="weighted") from a random guess: three iterations do not converge on two levels; the reported
    relative residual is the restated true one of the downloaded x, d_f[0] is restored"""
    n3, bc, dtype = LL.A, 63, np.float64
    v0, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    mg = _mg(ctx, dtype, False, v0, f)
    try:
        k, rel, conv, hist = mg.PCG(2, 2, 1e-10, 3, krylov="weighted")
        x = mg.download_v(0)
        assert bits_equal(mg.download_f(0), f), "d_f[0] was not restored"
        assert mg.pcg_removed_mean == 0.0
    finally:
        mg.close()
    op = OP.Op(n3, RG, dtype, S, bc=bc)
    want = math.sqrt(OP.fsum_sq(op.residual(x, f)) / OP.fsum_sq(op.residual(v0, f)))
    print("A, closed box: %d iterations, rel %.6e (restated of x %.6e), history %s" % (k, rel, want, hist))
    assert k == 3 and not conv and rel >= 1e-10
    assert abs(rel - want) <= 1e-6 * want, (rel, want)
    unk = OP.unknown_mask(n3, bc)
    assert bits_equal(x[~unk], v0[~unk]), "the Dirichlet data were changed"
    assert np.isfinite(x).all() and not bits_equal(x, v0)
