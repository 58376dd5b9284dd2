"""CPU suite: pinned interior nodes in the restatement tests/pin_restated.py -- the coarse rule on hand-made masks,
the struck-out operator, a solve that is right only with the pins, and the convergence table that chose the rule -- and what of the
library can be checked without a device: the entry points' argument checks, the list a mask becomes, the struct mirror."""
import ctypes as C

import numpy as np
import pytest

import op_restated as R
import oracle as O
import pde_multigrid_amd as P
import pin_restated as PR
from conftest import bits_equal
from pde_multigrid_amd.multigrid import _grid3_struct, _ip, xs_geometry

UNIT = [0, 1, 0, 1, 0, 1]


def _rand(n3, dtype, seed):
    return np.random.default_rng(seed).uniform(-1, 1, O.shape(n3)).astype(dtype)


def _where(m):
    """the true points of a mask as (x, y, z)"""
    return sorted((int(x), int(y), int(z)) for z, y, x in np.argwhere(m))


# ------------------------------------------------------------------------------------------ the coarse rule
def test_coarse_rule_single_point_at_an_odd_index():
    """(3, 5, 7) of 17^3 coincides with no coarse point: its 6 axis neighbours do -- (1 or 2, ...) -- and only those that differ
    from it along ONE axis have a coincident coarse point, which is none (all three coordinates are odd)"""
    assert not PR.coarse_pin(PR.point((17,) * 3, (3, 5, 7))).any()
    # odd along x alone: the neighbours at x -+ 1 are the coarse points (1, 2, 3) and (2, 2, 3)
    assert _where(PR.coarse_pin(PR.point((17,) * 3, (3, 4, 6)))) == [(1, 2, 3), (2, 2, 3)]
    # injection loses it, any of the 27 neighbours spreads it further
    assert not PR.coarse_pin(PR.point((17,) * 3, (3, 4, 6)), rule="injection").any()
    assert len(_where(PR.coarse_pin(PR.point((17,) * 3, (3, 5, 7)), rule="any27"))) == 8


def test_coarse_rule_single_point_at_an_even_index():
    for rule in ("axis", "injection", "any27"):
        assert _where(PR.coarse_pin(PR.point((17,) * 3, (4, 6, 8)), rule=rule)) == [(2, 3, 4)], rule
    # (a lone point's full weight at its coarse point is 1/8: the weighted rule loses it)
    assert not PR.coarse_pin(PR.point((17,) * 3, (4, 6, 8)), rule="weighted").any()


def test_coarse_rule_keeps_the_coarse_boundary_unpinned():
    """(1, 8, 8) of 17^3: its neighbour (0, 8, 8) is a boundary point and stays unpinned, (2, 8, 8) is the coarse (1, 4, 4)"""
    assert _where(PR.coarse_pin(PR.point((17,) * 3, (1, 8, 8)))) == [(1, 4, 4)]
    assert _where(PR.coarse_pin(PR.point((17,) * 3, (15, 8, 8)))) == [(7, 4, 4)]
    full = np.zeros(O.shape((9, 9, 9)), bool)
    full[1:-1, 1:-1, 1:-1] = True
    c = PR.coarse_pin(full)
    assert c.shape == O.shape((5, 5, 5)) and c[1:-1, 1:-1, 1:-1].all() and c.sum() == 27


def test_coarse_rule_on_a_semi_coarsened_step():
    """only the halved axes fatten: a step that halves x and y (axes = 3) on 17 x 17 x 9"""
    n3 = (17, 17, 9)
    got = PR.coarse_pin(PR.point(n3, (5, 6, 3)), axes=3)
    assert got.shape == O.shape((9, 9, 9)) and _where(got) == [(2, 3, 3), (3, 3, 3)]
    assert not PR.coarse_pin(PR.point(n3, (5, 7, 3)), axes=3).any()  # odd along both halved axes
    assert _where(PR.coarse_pin(PR.point(n3, (6, 6, 3)), axes=3)) == [(3, 3, 3)]  # z is kept: 3 stays 3, no neighbour along z
    assert _where(PR.coarse_pin(PR.point(n3, (6, 6, 4)), axes=4)) == [(6, 6, 2)]
    assert _where(PR.coarse_pin(PR.point(n3, (6, 6, 3)), axes=4)) == [(6, 6, 1), (6, 6, 2)]


def test_hierarchy_masks_values_and_operators():
    n3 = (17, 17, 17)
    g = _rand(n3, np.float64, 3)
    H = PR.PinHierarchy(R.Op(n3, UNIT, np.float64, 0.0), PR.ball(n3), g)
    assert [p.shape for p in H.pins] == [O.shape(n) for n in H.sizes]
    assert bits_equal(H.gs[1], g[::2, ::2, ::2]) and bits_equal(H.gs[2], g[::4, ::4, ::4])
    for l, (p, op) in enumerate(zip(H.pins, H.ops)):
        assert not (p & (R.on_faces(H.sizes[l]) != 0)).any() and not (op.unk & p).any()
        assert bits_equal(H.v[l][p], H.gs[l][p])
    with pytest.raises(AssertionError):
        PR.PinHierarchy(R.Op(n3, UNIT, np.float64, 0.0), PR.point(n3, (0, 3, 3)))


# ------------------------------------------------------------------------------------------ the struck-out operator
@pytest.mark.parametrize("kind", ["shift", "coef", "walls"])
def test_struck_out_operator_is_symmetric(kind):
    """A from apply_A on unit vectors at 9^3: rows and columns of the pins are zero, the rest is symmetric bit for bit (with walls:
    in the weighted product, W A symmetric; W is a power of two).  The operator acts on vectors that are 0 at the pins and at the
    Dirichlet points -- every CG vector is -- so a unit vector there is the zero vector: its column is struck out, not read as data"""
    n3 = (9, 9, 9)
    a = np.exp(_rand(n3, np.float64, 2)) if kind != "shift" else None
    bc = 0b010001 if kind == "walls" else 0
    pin = PR.ball(n3) | PR.point(n3, (1, 7, 2))
    op = PR.PinOp(n3, UNIT, np.float64, 3.0, a, bc=bc, pin=pin)
    N = int(np.prod(n3))
    A = np.zeros((N, N))
    for j in range(N):
        e = np.zeros(N)
        e[j] = 1.0
        A[:, j] = op.apply_A(np.where(op.unk, e.reshape(O.shape(n3)), 0.0)).ravel()
    pf, unk = pin.ravel(), op.unk.ravel()
    assert pf.any() and not A[pf, :].any() and not A[:, pf].any()
    assert not A[~unk, :].any()
    WA = R.weights(n3, bc).ravel()[:, None] * A
    sub = WA[np.ix_(unk, unk)]
    assert np.array_equal(sub, sub.T) and np.abs(sub).sum() > 0


def test_relax_never_moves_a_pin_and_residual_is_zero_there():
    n3 = (9, 17, 9)
    pin = PR.plate(n3, 3) | PR.point(n3, (1, 1, 1))
    op = PR.PinOp(n3, UNIT, np.float32, 0.5, pin=pin)
    v, f = _rand(n3, np.float32, 1), _rand(n3, np.float32, 2)
    out = op.relax(v, f, 3)
    assert bits_equal(out[pin], v[pin]) and not bits_equal(out[op.unk], v[op.unk])
    assert not op.residual(out, f)[pin].any()
    # "update everything, then put back": the same bits
    plain = R.Op(n3, UNIT, np.float32, 0.5)
    w = v.copy()
    for _ in range(3):
        for colour in (0, 1):
            m = plain._colour[colour]
            full = _one_pass(plain, w, f, m)
            full[pin] = v[pin]
            w = full
    assert bits_equal(w, out)


def _one_pass(op, v, f, m):
    """one colour pass of op_restated.Op.relax on the mask m"""
    o, e, n, so, d, u, _c = R._nb(R.mirror(v))
    hx2, hy2, hz2 = op._stencil
    fi = np.ascontiguousarray(f, op.dtype)
    num = o * (hy2 * hz2) + e * (hy2 * hz2) + n * (hx2 * hz2) + so * (hx2 * hz2) + d * (hx2 * hy2) + u * (hx2 * hy2) - fi * hx2 * hy2 * hz2
    out = v.copy()
    out[m] = (num / op._den)[m]
    return out


# ------------------------------------------------------------------------------------------ a solve that needs the pins
@pytest.mark.parametrize("n3,dtype,tol", [((17, 17, 17), np.float64, 1e-12), ((9, 17, 9), np.float32, 2e-6)])
def test_pinned_solve_returns_the_unpinned_solution(n3, dtype, tol):
    """u* solves the Dirichlet problem; with a set pinned to u*'s values and a random start the pinned flexible CG must return u*.
    The bound: the error of a second unpinned solve from another random start, times 10 -- both are stopped at the same relative
    residual, so that is what the tolerance alone allows"""
    op = R.Op(n3, UNIT, dtype, 0.0)
    f = _rand(n3, dtype, 1)
    starts = [_rand(n3, dtype, s) for s in (2, 3, 4)]
    bnd = starts[0].copy()
    for s in starts[1:]:  # the same Dirichlet data
        edge = R.on_faces(n3) != 0
        s[edge] = bnd[edge]
    ustar, k1, _, conv1 = R.fcg(op, starts[0], f, tol=tol, maxit=60)[:4]
    second, k2, _, conv2 = R.fcg(op, starts[1], f, tol=tol, maxit=60)[:4]
    assert conv1 and conv2
    allowed = 10 * float(np.abs(second.astype(np.float64) - ustar).max())
    pin = PR.ball(n3) | PR.point(n3, (1, 1, 1))
    x, k, hist, conv, rel = PR.pin_fcg(op, pin, ustar, starts[2], f, tol=tol, maxit=60)
    err = float(np.abs(x.astype(np.float64) - ustar).max())
    print("%s %s: unpinned %d and %d iterations, pinned %d; error %.3e, allowed %.3e" % (n3, np.dtype(dtype).name, k1, k2, k, err, allowed))
    assert conv and rel < tol and bits_equal(x[pin], ustar[pin])
    assert allowed > 0 and err <= allowed
    # without the pins' values (pinned to zeros) the answer is another one: the pins matter
    y = PR.pin_fcg(op, pin, None, starts[2], f, tol=tol, maxit=60)[0]
    assert float(np.abs(y.astype(np.float64) - ustar).max()) > 100 * allowed


# ------------------------------------------------------------------------------------------ the table that chose the rule
def _cycles(n3, pin, rule, maxit=60, tol=1e-10):
    op = R.Op(n3, UNIT, np.float64, 0.0)
    H = PR.PinHierarchy(op, pin, _rand(n3, np.float64, 7), rule=rule)
    H.set_v(_rand(n3, np.float64, 8))
    H.f[0] = _rand(n3, np.float64, 9)
    with np.errstate(all="ignore"):
        return H.cycle_to(2, 2, tol, maxit)


@pytest.mark.parametrize("name", list(PR.table_sets((17,) * 3)))
def test_plain_cycling_converges_with_the_chosen_rule(name):
    """V(2,2) to 1e-10 within 60 cycles for every set of DESIGN.md 22's table at 17^3"""
    k, rel, conv = _cycles((17,) * 3, PR.table_sets((17,) * 3)[name], "axis")
    print("%s: %d cycles, rel %.2e" % (name, k, rel))
    assert conv and k <= 60


def test_injection_only_fails_for_the_odd_plane_plate():
    """the guard of the rule: with the coincident point alone the plate on an odd plane vanishes from the coarse levels and plain
    cycling does not reach 1e-10 within 60 cycles at 33^3 (the chosen rule does)"""
    n3 = (33,) * 3
    pin = PR.table_sets(n3)["plate, odd plane"]
    k, rel, conv = _cycles(n3, pin, "injection")
    k_a, rel_a, conv_a = _cycles(n3, pin, "axis")
    print("injection: rel %.2e after %d cycles; axis rule: %d cycles" % (rel, k, k_a))
    assert not conv and k == 60
    assert conv_a


# ------------------------------------------------------------------------------------------ the library without a device
@pytest.mark.parametrize("sfx,ct", [("f32", C.c_float), ("f64", C.c_double)])
def test_the_mirror_holds_the_pin_table(sfx, ct):
    """pin takes the last eight bytes of the unused graph_key, in front of wall: no member moved, the struct kept its size"""
    G, M = _grid3_struct(ct)
    fn = getattr(P.lib, "mgMultiGrid3D_%s_sizeof" % sfx)
    fn.restype = C.c_size_t
    assert C.sizeof(M) == fn()
    assert M.pin.offset == M.graph_key.offset + 28 * 8 and M.pin.size == 8 and M.wall.offset == M.pin.offset + 8
    assert M.face_mean.offset == M.graph_key.offset and M._fields_[-1][0] == "shift"
    for name in ("set_pinned", "get_pinned", "pinned_count"):
        assert hasattr(P.lib, "mgMultiGrid3D_%s_%s" % (sfx, name))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_pin_list_orders_red_then_black_by_offset(dtype):
    n3 = (9, 7, 5)
    mask = PR.random_set(n3, 0.5, seed=2)
    g = _rand(n3, dtype, 4)
    idx, val, end = P.ops3dxs.pin_list(n3, mask, g, dtype)
    H, Pp = xs_geometry(n3[0], np.dtype(dtype).itemsize)
    want = [[], []]
    for z, y, x in np.argwhere(mask):
        want[(x + y + z) & 1].append(((y + z * n3[1]) * Pp + (x >> 1) + (x & 1) * H, g[z, y, x]))
    want = [sorted(w) for w in want]
    assert end == (len(want[0]), len(want[0]) + len(want[1])) and end[1] == mask.sum()
    assert [int(i) for i in idx] == [o for w in want for o, _ in w]
    assert bits_equal(val, np.array([t for w in want for _, t in w], dtype))
    assert P.ops3dxs.pin_list(n3, np.zeros(O.shape(n3), bool), None, dtype)[2] == (0, 0)


@pytest.mark.parametrize("sfx,ct", [("f32", C.c_float), ("f64", C.c_double)])
def test_entries_check_their_arguments(sfx, ct):
    L, I = P.lib, P.MGX_ERR_INVALID
    n3 = (9, 9, 9)
    end = (C.c_uint * 2)()
    fn = getattr(L, "mgx3dxs_pin_list_" + sfx)
    bad = PR.point(n3, (0, 4, 5)).astype(np.uint8)
    assert fn(_ip(n3), bad.ctypes.data_as(C.c_void_p), None, None, None, end) == I
    assert b"(0, 4, 5)" in L.mgx_last_error() and b"boundary" in L.mgx_last_error()
    assert fn(_ip(n3), None, None, None, None, end) == I and b"NULL" in L.mgx_last_error()
    assert fn(_ip((8, 9, 9)), bad.ctypes.data_as(C.c_void_p), None, None, None, end) == P.MGX_ERR_SIZE
    huge = (4097, 4097, 513)  # 4224 * 4097 * 513 > 2^32 storage positions of doubles; the mask is not read before the check
    assert fn(_ip(huge), bad.ctypes.data_as(C.c_void_p), None, None, None, end) == P.MGX_ERR_SIZE and b"32-bit" in L.mgx_last_error()
    assert getattr(L, "mgx3dxs_pin_put_" + sfx)(None, None, None, None, C.c_uint(0), C.c_uint(1)) == I
    for k in ("shift", "coef", "cap", "hmean"):
        assert hasattr(L, "mgx3dxs_relax_%s_pin_%s" % (k, sfx)), k
    N = None
    assert getattr(L, "mgMultiGrid3D_%s_set_pinned" % sfx)(N, N, N) == I
    assert getattr(L, "mgMultiGrid3D_%s_get_pinned" % sfx)(N, 0, N) == I
    assert getattr(L, "mgMultiGrid3D_%s_pinned_count" % sfx)(N, 0, N) == I
