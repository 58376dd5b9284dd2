"""Harmonic-mean face coefficients without a GPU: the restatement of the arithmetic (tests/op_restated.py) is
exact for a layered medium whose interface lies midway between two node planes, where the arithmetic mean is wrong by the order
of the flux itself; its matrix is symmetric bit for bit; with a constant power-of-two coefficient it has the bits of the
arithmetic restatement; and the library exports the new entries, rejects NULL arguments and bad masks before it touches the
device and keeps the sizes and offsets of the struct mirror."""
import ctypes as C
import math

import numpy as np
import pytest

import op_cases as OC
import op_restated as OP
import oracle as O
import pde_multigrid_amd as P
from conftest import bits_equal
from pde_multigrid_amd.multigrid import _grid3_struct

UNIT = [0, 1, 0, 1, 0, 1]
RG = [-1, 1, 0, 2, 0.5, 3]
N = None
ENTRIES = ("relax_hmean_wall", "relax_hmean_from_zero", "residual_hmean_wall", "apply_hmean_dot_wall")


# ------------------------------------------------------------------------------------------ the layered medium
# The bound on the harmonic residual of the analytic nodal values.  Only the z terms are not exactly zero (u does not depend on x, y):
#   tz = qz * (AD * (D - c) + AU * (U - c)),  qz = 0.5 / h^2,  AD, AU <= 2 max|a| (1 + 3 eps)
# The nodal values carry eps/2 max|u| each from their rounding to `dtype`, so each difference is off its exact value by at most
# eps max|u| (the subtraction of neighbours is exact or adds another eps/2 of a smaller number); the two products, their sum and the
# scaling add three more roundings of terms of size <= 2 max|a| max|du|, du <= max|u|.  Per term that is below
# (0.5 / h^2) * 2 max|a| * max|u| * (1 + 3 + 3) eps = 7 eps max|a| max|u| / h^2, twice for the two terms, plus the cancelling
# subtraction f - tz: the multiple 16 of eps * max|a| * max|u| / h^2 covers it.
SLAB_MULTIPLE = 16


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("jump", [10, 1000])
def test_the_harmonic_restatement_is_exact_for_a_layered_medium(jump, dtype):
    n3, rng = OC.SLAB_N3, OC.SLAB_RNG
    a, u, q = OC.slab(jump, dtype)
    h = (rng[5] - rng[4]) / (n3[2] - 1)
    f = np.zeros(O.shape(n3), dtype)
    r = OP.Op(n3, rng, dtype, 0.0, a, mean="harmonic").residual(u, f)
    bound = SLAB_MULTIPLE * np.finfo(dtype).eps * float(a.max()) * float(np.abs(u).max()) / h ** 2
    worst = float(np.abs(r).max())
    print("jump %g %s: harmonic residual %.3e (bound %.3e)" % (jump, np.dtype(dtype).name, worst, bound))
    assert worst <= bound, (worst, bound)
    # the arithmetic faces put the interface on node plane K: the same field leaves a residual of the order of the flux itself
    ra = OP.Op(n3, rng, dtype, 0.0, a).residual(u, f)
    flux = abs(q)  # max |a grad u|: the same in both layers
    print("jump %g %s: arithmetic residual %.3e against flux / h = %.3e" % (jump, np.dtype(dtype).name, float(np.abs(ra).max()), flux / h))
    assert float(np.abs(ra).max()) > 1e-2 * flux / h


@pytest.mark.parametrize("jump", [10, 1000])
def test_the_restated_solve_of_the_slab_is_the_analytic_profile(jump):
    """flexible CG on the slab with insulated x/y faces reproduces the series-resistance profile: to 1e-12 in the residual, and
    in the solution to that times the jump, which the problem's condition grows with (measured: 3.7e-13 for the jump of 10 in 12
    iterations, 4.6e-11 for 1000 in 60 -- the cycle is a weak preconditioner across a sheet the coarse levels smear); the
    arithmetic operator's solution is off by 0.036 and 0.059 of the unit drop: the test_gpu_hmean.py slab test holds ten times
    the harmonic figures"""
    n3, rng = OC.SLAB_N3, OC.SLAB_RNG
    a, u, _ = OC.slab(jump)
    v0 = u.copy()
    v0[1:-1] = 0.0  # the Dirichlet planes z-low and z-high keep the data; every other point is an unknown
    f = np.zeros(O.shape(n3))
    x, it, _, conv, rel = OP.fcg(OP.Op(n3, rng, np.float64, 0.0, a, bc=15, mean="harmonic"), v0, f, tol=1e-12, maxit=100)[:5]
    assert conv and rel < 1e-12, (it, rel)
    err = float(np.abs(x - u).max())
    print("jump %g: harmonic CG %d iterations, error %.3e" % (jump, it, err))
    assert err < 1e-12 * jump
    xa, _, _, conva, _ = OP.fcg(OP.Op(n3, rng, np.float64, 0.0, a, bc=15), v0, f, tol=1e-12, maxit=100)[:5]
    assert conva and float(np.abs(xa - u).max()) > 1e-2


# ------------------------------------------------------------------------------------------ symmetry, bit for bit
def _matrix(n3, rng, a, s, dtype, c, bc, beta):
    """A column by column over all points: A[:, j] = apply_A(e_j)"""
    vol = n3[0] * n3[1] * n3[2]
    A = np.zeros((vol, vol), dtype)
    for j in range(vol):
        e = np.zeros(vol, dtype)
        e[j] = 1
        A[:, j] = OP.Op(n3, rng, dtype, s, a, c, bc, beta, "harmonic").apply_A(e.reshape(O.shape(n3))).ravel()
    return A


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("bc,beta", [(0, OP.ZERO), (63, OP.ZERO), (0b101010, (0, 1.5, 0, 0.25, 0, 3.0))])
def test_apply_A_is_symmetric_bit_for_bit(bc, beta, dtype):
    """<x, A y> == <y, A x> through math.fsum for x = e_i, y = e_j: an entry of the matrix is one face coefficient times q*, and a
    face has the same bits seen from either node (the inner product of the mask weighs by powers of two, exactly).  For general
    x, y the two sides agree to rounding only, whatever the mean: A y is rounded."""
    n3 = (5, 7, 5)
    g = np.random.default_rng(5)
    a = g.uniform(0.5, 2, O.shape(n3)).astype(dtype)
    a[1:3, 2:5, 1:4] *= dtype(1000)
    c = g.uniform(0, 2, O.shape(n3)).astype(dtype)
    A = _matrix(n3, RG, a, 3.0, dtype, c, bc, beta)
    unk = OP.unknown_mask(n3, bc).ravel()
    W = OP.weights(n3, bc).ravel()
    WA = (W[:, None] * A.astype(np.float64))[np.ix_(unk, unk)]
    assert np.count_nonzero(WA) > 3 * unk.sum()  # (the matrix was formed)
    for i, j in zip(*np.nonzero(WA)):  # <e_i, A e_j>_W and <e_j, A e_i>_W
        assert math.fsum([WA[i, j]]) == math.fsum([WA[j, i]]), (i, j)
    assert np.array_equal(WA.view(np.uint64), WA.T.copy().view(np.uint64))


def test_general_vectors_agree_to_rounding():
    n3 = (9, 7, 5)
    g = np.random.default_rng(6)
    a = g.uniform(0.5, 2, O.shape(n3))
    a[1:3, 2:5, 3:6] *= 1000.0
    x, y = g.uniform(-1, 1, O.shape(n3)), g.uniform(-1, 1, O.shape(n3))
    for v in (x, y):
        v[0], v[-1], v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1] = 0, 0, 0, 0, 0, 0
    xAy = math.fsum((x * OP.Op(n3, RG, np.float64, 2.0, a, mean="harmonic").apply_A(y)).ravel())
    yAx = math.fsum((y * OP.Op(n3, RG, np.float64, 2.0, a, mean="harmonic").apply_A(x)).ravel())
    assert abs(xAy - yAx) <= 1e-12 * abs(xAy)
    assert math.fsum((x * OP.Op(n3, RG, np.float64, 2.0, a, mean="harmonic").apply_A(x)).ravel()) < 0  # negative definite


# ------------------------------------------------------------------------------------------ the bits of the arithmetic operator
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("k", [-3, 0, 5])
def test_a_constant_power_of_two_gives_the_bits_of_the_arithmetic_restatement(k, dtype):
    """a == 2^k at every node: 4 * ((a * a) / (a + a)) = 4 * (a / 2) = 2 a = a + a exactly, so every restated operation has the
    arithmetic restatement's bits (two different powers of two do not: 4 * (2 / 3) is not 3 -- the two means differ)"""
    n3 = (17, 9, 9)
    g = np.random.default_rng(7)
    a = np.full(O.shape(n3), 2.0 ** k, dtype)
    c = g.uniform(0, 2, O.shape(n3)).astype(dtype)
    v, f = g.uniform(-1, 1, O.shape(n3)).astype(dtype), g.uniform(-1, 1, O.shape(n3)).astype(dtype)
    for cc, bc, beta in ((None, 0, OP.ZERO), (c, 0, OP.ZERO), (c, 0b010101, (2.0, 0, 0.5, 0, 0, 0))):
        hm, ar = (OP.Op(n3, RG, dtype, 3.0, a, cc, bc, beta, mean) for mean in ("harmonic", "arithmetic"))
        assert bits_equal(hm.relax(v, f, 2), ar.relax(v, f, 2))
        assert bits_equal(hm.residual(v, f), ar.residual(v, f))
        assert bits_equal(hm.apply_A(v), ar.apply_A(v))
    outs = []
    for mean in ("harmonic", "arithmetic"):
        for coarsening in ("full", "semi"):
            H = OP.Hierarchy(OP.Op(n3, RG, dtype, 3.0, a, mean=mean), coarsening)
            H.v[0], H.f[0] = v.copy(), f.copy()
            H.vcycle(0, 2, 2)
            H.fmg(0, 1, 1, 1)
            outs.append(H.v[0])
    assert bits_equal(outs[0], outs[2]) and bits_equal(outs[1], outs[3])
    a2 = a.copy()
    a2[::2] *= dtype(2)  # two powers of two: the means differ
    assert not bits_equal(OP.Op(n3, RG, dtype, 3.0, a2, mean="harmonic").residual(v, f), OP.Op(n3, RG, dtype, 3.0, a2).residual(v, f))


def test_restated_cg_solves_the_jump():
    """the block jump of 1000 at 17^3: flexible CG around the harmonic V(2,2) converges to 1e-10 (plain cycling is slow on jumps for
    either mean -- the transfers do not see the coefficient; DESIGN.md 19 has the counts at 33^3)"""
    n3 = (17, 17, 17)
    g = np.random.default_rng(9)
    a = OC.jump_coefficient(n3, 1000.0)
    f = g.uniform(-1, 1, O.shape(n3))
    _, it, hist, conv, rel = OP.fcg(OP.Op(n3, UNIT, np.float64, 0.0, a, mean="harmonic"), np.zeros(O.shape(n3)), f, tol=1e-10, maxit=40)[:5]
    print("harmonic CG on the jump of 1000 at 17^3: %d iterations to %.2e" % (it, rel))
    assert conv and rel < 1e-10


# ------------------------------------------------------------------------------------------ the library's new surface
def _calls(ct, buf, n, h, bc, beta, c):
    """every entry with all arguments given (host buffers stand in: the checks come before any use)"""
    s = ct(0.5)
    return {"relax_hmean_wall": (buf, buf, buf, buf, c, n, h, s, 1, bc, beta), "relax_hmean_from_zero": (buf, buf, buf, buf, c, n, h, s, 1, 0),
            "residual_hmean_wall": (buf, buf, buf, buf, c, buf, n, h, s, buf, buf, bc, beta),
            "apply_hmean_dot_wall": (buf, buf, buf, c, buf, n, h, s, buf, buf, bc, beta)}


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_new_symbols_are_exported_and_reject_null(sfx):
    ct = C.c_float if sfx == "f32" else C.c_double
    L, I = P.lib, P.MGX_ERR_INVALID
    buf = (C.c_double * 64)()
    n, h, beta = (C.c_int * 3)(5, 5, 5), (ct * 3)(0.25, 0.25, 0.25), (ct * 6)(1, 0, 0, 0, 0, 0)
    for c in (buf, N):  # with a capacity and without one
        full = _calls(ct, buf, n, h, 1, beta, c)
        assert set(full) == set(ENTRIES)
        for k, args in full.items():
            fn = getattr(L, "mgx3dxs_%s_%s" % (k, sfx))
            assert fn(*[None if isinstance(x, C.Array) else x for x in args]) == I, k
            assert b"NULL" in L.mgx_last_error(), k
            for miss in range(1, 4):  # v / p, f / a, a / ... alone missing (the capacity may be missing: no capacity)
                if args[miss] is c:
                    continue
                one = list(args)
                one[miss] = None
                assert fn(*one) == I and b"NULL" in L.mgx_last_error(), (k, miss)
            if k != "relax_hmean_from_zero":
                assert fn(*args[:-1], None) == I and b"NULL" in L.mgx_last_error(), k  # beta alone missing
                for bc in (64, -1):
                    assert fn(*args[:-2], bc, (ct * 6)()) == I, (k, bc)
                    assert b"bc" in L.mgx_last_error(), (k, L.mgx_last_error())
                assert fn(*args[:-2], 2, beta) == I and b"mask" in L.mgx_last_error(), k  # a beta on a face the mask does not flag
                assert fn(*args[:-1], (ct * 6)(-1, 0, 0, 0, 0, 0)) == I and b"beta" in L.mgx_last_error(), k
    assert hasattr(L, "mgMultiGrid3D_%s_set_face_mean" % sfx)
    assert getattr(L, "mgMultiGrid3D_%s_set_face_mean" % sfx)(N, 1) == I


@pytest.mark.parametrize("sfx,ct", [("f32", C.c_float), ("f64", C.c_double)])
def test_the_mirror_still_has_the_library_size(sfx, ct):
    """face_mean takes the first four bytes of the unused graph_key: no member moved, the struct kept its size, shift stays last"""
    G, M = _grid3_struct(ct)
    fn = getattr(P.lib, "mgMultiGrid3D_%s_sizeof" % sfx)
    fn.restype = C.c_size_t
    assert C.sizeof(M) == fn()
    assert M.face_mean.offset == M.graph_key.offset and M.face_mean.size == 4 and M.graph_key.size == 29 * 8
    assert M.wall.offset == M.graph_key.offset + 29 * 8 and M._fields_[-1][0] == "shift"
    assert P.multigrid.FACE_MEANS == {"arithmetic": 0, "harmonic": 1}
    for bad in ("geometric", "", None, 1):
        with pytest.raises(ValueError):
            P.multigrid.face_mean_mode(bad)
