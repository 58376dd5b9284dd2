"""The variable-coefficient operator div(a grad u) - s u = f without a GPU: the restatement of its arithmetic
(tests/op_restated.py) is exact where the discretisation is, symmetric and negative definite, anchored to the pinned
constant-coefficient operators at a = 1, and its cycle is a solver; the library exports the new entries, rejects NULL arguments and
reports the size of the struct the Python mirror restates."""
import ctypes as C
import math

import numpy as np
import pytest

import op_cases as OC
import op_restated as OP
import oracle as O
import pde_multigrid_amd as P
from pde_multigrid_amd.multigrid import _grid3_struct
from solve_restated import boundary_mask, problem

RG = [-1, 1, 0, 2, 0.5, 3]
UNIT = [0, 1, 0, 1, 0, 1]
KERNELS = ("relax_coef", "relax_coef_from_zero", "residual_coef", "apply_coef_dot")


def test_exact_for_linear_a_times_quadratic_u():
    """a = 1 + x + 2y, u = x^2 + y z, f = div(a grad u) = 2(1 + x + 2y) + 2x + 2z on 17^3: the arithmetic-mean faces are exact for
    a linear a, the differences for a quadratic u (measured: a residual of 0.0 or a few ulps of |f|; the bound is the issue's)"""
    n3 = (17, 17, 17)
    x, y, z = OC.nodes(n3)
    a, u, f = 1 + x + 2 * y, x * x + y * z, 2 * (1 + x + 2 * y) + 2 * x + 2 * z
    r = OP.Op(n3, UNIT, np.float64, 0.0, a).residual(u, f)
    print("exactness: max |residual| = %.3e" % np.abs(r).max())
    assert np.abs(r).max() <= 1e-10


def test_operator_is_symmetric_and_negative_definite():
    n3, s = (9, 9, 9), 0.7
    g = np.random.default_rng(5)
    a = g.uniform(0.5, 2, O.shape(n3))
    p, w = g.uniform(-1, 1, O.shape(n3)), g.uniform(-1, 1, O.shape(n3))
    p[boundary_mask(n3)] = 0
    w[boundary_mask(n3)] = 0
    Ap, Aw = OP.Op(n3, RG, np.float64, s, a).apply_A(p), OP.Op(n3, RG, np.float64, s, a).apply_A(w)
    wAp, pAw, pAp = float((w * Ap).sum()), float((p * Aw).sum()), float((p * Ap).sum())
    print("symmetry: <w, A p> = %.15e, <p, A w> = %.15e, <p, A p> = %.6e" % (wAp, pAw, pAp))
    assert abs(wAp - pAw) <= 1e-12 * abs(wAp)
    assert pAp < 0


# the largest differences this test showed on the CPU, in units of eps(dtype) * max |want| (relax, residual), per
# (precision, grid, s); the test asserts 8 times them
ANCHOR_SEEN = {("float32", 0, 0): (1.500, 1.136), ("float32", 0, 100): (0.875, 1.024), ("float32", 1, 0): (0.500, 0.820),
               ("float32", 1, 100): (0.500, 0.790), ("float64", 0, 0): (0.750, 1.136), ("float64", 0, 100): (0.500, 1.024),
               ("float64", 1, 0): (0.750, 0.820), ("float64", 1, 100): (0.500, 0.790)}
ANCHOR_GRIDS = [((21, 13, 29), RG), ((17, 17, 17), UNIT)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("s", [0, 100])
@pytest.mark.parametrize("grid", [0, 1])
def test_unit_coefficient_is_the_pinned_operator_in_value(grid, s, dtype):
    """a = 1: relax (two sweeps) and residual agree with the shifted operator's in value -- other associations, so not in bits.  The
    differences seen on the CPU, in units of eps * max |want| (relax, residual), are ANCHOR_SEEN -- between 0.5 and 1.5 for the
    two sweeps, between 0.79 and 1.14 for the residual; the bound is 8 times them."""
    n3, rng = ANCHOR_GRIDS[grid]
    g = np.random.default_rng(3)
    v, f = g.uniform(-1, 1, O.shape(n3)).astype(dtype), g.uniform(-1, 1, O.shape(n3)).astype(dtype)
    one = np.ones(O.shape(n3), dtype)
    eps = float(np.finfo(dtype).eps)
    seen = ANCHOR_SEEN[(np.dtype(dtype).name, grid, s)]
    pairs = [("relax", OP.Op(n3, rng, dtype, s, one).relax(v, f, 2), OP.Op(n3, rng, dtype, s).relax(v, f, 2)),
             ("residual", OP.Op(n3, rng, dtype, s, one).residual(v, f), OP.Op(n3, rng, dtype, s).residual(v, f))]
    for (what, got, want), bound in zip(pairs, seen):
        got, want = got.astype(np.float64), want.astype(np.float64)
        units = np.abs(got - want).max() / (eps * np.abs(want).max())
        print("anchor %s %s grid %d s %g: %.3f eps * max|want| (seen %.3f)" % (np.dtype(dtype).name, what, grid, s, units, bound))
        assert units <= 8 * bound, (what, units, bound)


@pytest.mark.parametrize("s", [0.0, 100.0])
def test_restated_cycle_converges_with_a_smooth_coefficient(s):
    """fp64 V(2,2) on 33^3, unit cube, random interior f, a = 1 + 0.5 sin(2 pi x) cos(pi y) + 0.25 z: relative residual below 1e-8
    after 8 cycles (the issue's prototype: 8.2e-10 and 9.5e-11; the bound is the shift test's)"""
    n3 = (33, 33, 33)
    H = OP.Hierarchy(OP.Op(n3, UNIT, np.float64, s, OC.smooth_coefficient(n3)))
    H.f[0] = problem(n3)
    r0 = math.sqrt(OP.fsum_sq(H.residual(0)))
    for _ in range(8):
        H.vcycle(0, 2, 2)
    rel = math.sqrt(OP.fsum_sq(H.residual(0))) / r0
    print("smooth coefficient, shift %g: relative residual %.3e after 8 V(2,2)" % (s, rel))
    assert rel < 1e-8, rel


def test_restated_fcg_solves_a_jump_of_ten():
    """a = 10 inside the centred cube of edge 1/2, 1 outside, s = 0: flexible CG + V(2,2) to 1e-10 in at most 20 iterations (the
    issue's prototype: 12), and the restricted coefficients never fall below the smallest fine one (positive weights)"""
    n3 = (33, 33, 33)
    a, f = OC.jump_coefficient(n3, 10), problem(n3)
    H = OP.Hierarchy(OP.Op(n3, UNIT, np.float64, 0.0, a))
    for l, al in enumerate(H.a):
        assert al.min() >= 1.0, (l, al.min())
    _, k, hist, conv = OP.fcg(OP.Op(n3, UNIT, np.float64, 0.0, a), np.zeros_like(f), f, tol=1e-10, maxit=50)[:4]
    print("jump 10: %d iterations, last relative residual %.3e" % (k, hist[-1]))
    assert conv and k <= 20, k


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_new_symbols_are_exported_and_reject_null(sfx):
    for k in KERNELS:
        assert hasattr(P.lib, "mgx3dxs_%s_%s" % (k, sfx)), k
    for k in ("set_coefficient", "download_coefficient"):
        assert hasattr(P.lib, "mgMultiGrid3D_%s_%s" % (sfx, k)), k
    assert hasattr(P.lib, "mgGrid3D_%s_sizeof" % sfx)
    ct = C.c_float if sfx == "f32" else C.c_double
    L, I = P.lib, P.MGX_ERR_INVALID
    assert getattr(L, "mgx3dxs_relax_coef_" + sfx)(None, None, None, None, None, None, ct(1), 1) == I
    assert b"NULL" in L.mgx_last_error()
    assert getattr(L, "mgx3dxs_relax_coef_from_zero_" + sfx)(None, None, None, None, None, None, ct(1), 1, 0) == I
    assert getattr(L, "mgx3dxs_residual_coef_" + sfx)(None, None, None, None, None, None, None, ct(1), None, None) == I
    assert getattr(L, "mgx3dxs_apply_coef_dot_" + sfx)(None, None, None, None, None, None, ct(1), None, None) == I
    assert getattr(L, "mgMultiGrid3D_%s_set_coefficient" % sfx)(None, None) == I
    assert getattr(L, "mgMultiGrid3D_%s_download_coefficient" % sfx)(None, 0, None) == I


@pytest.mark.parametrize("sfx,ct", [("f32", C.c_float), ("f64", C.c_double)])
def test_grid_mirror_has_the_library_size(sfx, ct):
    fn = getattr(P.lib, "mgGrid3D_%s_sizeof" % sfx)
    fn.restype = C.c_size_t
    G = _grid3_struct(ct)[0]
    assert C.sizeof(G) == fn()
    assert G._fields_[-1][0] == "d_a" and G.d_a.offset + C.sizeof(C.c_void_p) == fn()
