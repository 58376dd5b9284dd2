"""Homogeneous Neumann faces without a GPU: the library exports the new entries, rejects NULL arguments and masks outside 0 .. 63
and reports the size of the struct the Python mirror restates; the restatement of the arithmetic (tests/op_restated.py) is
exact where the discretisation is, symmetric under the trapezoid weights and negative definite, second order, its cycle is a solver
and its implicit steps in a closed box keep the heat content."""
import ctypes as C
import math

import numpy as np
import pytest

import op_cases as OC
import op_restated as OP
import oracle as O
import pde_multigrid_amd as P
from op_cases import VCYCLE_CASES, gaussian, vcycle_case
from pde_multigrid_amd.multigrid import _grid3_struct

UNIT = [0, 1, 0, 1, 0, 1]
KERNELS = ("relax_shift_bc", "relax_coef_bc", "residual_shift_bc", "residual_coef_bc", "restrict_bc", "interpolate_bc",
           "interpolate_correct_bc", "shift_rhs_bc")


# ------------------------------------------------------------------------------------------ the library's new surface
@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_new_symbols_are_exported_and_reject_null_and_bad_masks(sfx):
    for k in KERNELS:
        assert hasattr(P.lib, "mgx3dxs_%s_%s" % (k, sfx)), k
    for k in ("set_boundary", "get_boundary"):
        assert hasattr(P.lib, "mgMultiGrid3D_%s_%s" % (sfx, k)), k
    ct = C.c_float if sfx == "f32" else C.c_double
    L, I = P.lib, P.MGX_ERR_INVALID
    fn = lambda k: getattr(L, "mgx3dxs_%s_%s" % (k, sfx))
    N = None
    null_calls = {"relax_shift_bc": (N, N, N, N, N, ct(1), 1, 1), "relax_coef_bc": (N, N, N, N, N, N, ct(1), 1, 1),
                  "residual_shift_bc": (N, N, N, N, N, N, ct(1), N, N, 1), "residual_coef_bc": (N, N, N, N, N, N, N, ct(1), N, N, 1),
                  "restrict_bc": (N, N, N, N, N, 1), "interpolate_bc": (N, N, N, N, N, 1), "interpolate_correct_bc": (N, N, N, N, N, 1),
                  "shift_rhs_bc": (N, N, N, ct(1), ct(1), N, N, 1)}
    for k in KERNELS:
        assert fn(k)(*null_calls[k]) == I, k
        assert b"NULL" in L.mgx_last_error(), k
    # bc = 64 (and -1): the mask is looked at before any argument is used, so host buffers stand in for the context and the arrays
    buf = (C.c_double * 64)()
    n, h = (C.c_int * 3)(5, 5, 5), (ct * 3)(0.25, 0.25, 0.25)
    cn = (C.c_int * 3)(3, 3, 3)
    for bc in (64, -1):
        bad = {"relax_shift_bc": (buf, buf, buf, n, h, ct(1), 1, bc), "relax_coef_bc": (buf, buf, buf, buf, n, h, ct(1), 1, bc),
               "residual_shift_bc": (buf, buf, buf, buf, n, h, ct(1), buf, buf, bc),
               "residual_coef_bc": (buf, buf, buf, buf, buf, n, h, ct(1), buf, buf, bc), "restrict_bc": (buf, buf, n, buf, cn, bc),
               "interpolate_bc": (buf, buf, n, buf, cn, bc), "interpolate_correct_bc": (buf, buf, n, buf, cn, bc),
               "shift_rhs_bc": (buf, buf, buf, ct(1), ct(1), buf, n, bc)}
        for k in KERNELS:
            assert fn(k)(*bad[k]) == I, (k, bc)
            assert b"bc" in L.mgx_last_error(), (k, L.mgx_last_error())
    assert getattr(L, "mgx3dxs_set_rim_bc_" + sfx)(None, None, None, ct(0), 1) == I and b"NULL" in L.mgx_last_error()
    assert getattr(L, "mgx3dxs_set_rim_bc_" + sfx)(buf, buf, n, ct(0), 64) == I and b"bc" in L.mgx_last_error()
    assert getattr(L, "mgMultiGrid3D_%s_set_boundary" % sfx)(None, None) == I
    assert getattr(L, "mgMultiGrid3D_%s_get_boundary" % sfx)(None, None) == I


@pytest.mark.parametrize("sfx,ct", [("f32", C.c_float), ("f64", C.c_double)])
def test_hierarchy_mirror_has_the_library_size(sfx, ct):
    fn = getattr(P.lib, "mgMultiGrid3D_%s_sizeof" % sfx)
    fn.restype = C.c_size_t
    M = _grid3_struct(ct)[1]
    assert C.sizeof(M) == fn()
    # the mask stands where the unused eight bytes behind pcg_graph_exec stood: no member moved, `shift` is still the last one
    assert M.bc.offset == M.pcg_graph_exec.offset + C.sizeof(C.c_void_p) and M.graph_rec.offset == M.bc.offset + 8
    assert M._fields_[-1][0] == "shift" and M.shift.offset + C.sizeof(ct) <= fn()


# ------------------------------------------------------------------------------------------ the restated arithmetic
def test_unknowns_and_weights():
    n3 = (5, 7, 9)
    assert OP.unknown_mask(n3, 0).sum() == 3 * 5 * 7 and OP.unknown_mask(n3, 63).all()
    m = OP.unknown_mask(n3, 1)  # x-low: the open face only, its edges are Dirichlet
    assert m[1:-1, 1:-1, 0].all() and not m[0, :, 0].any() and not m[:, 0, 0].any() and not m[:, :, -1].any()
    w = OP.weights(n3, 63)
    assert w[0, 0, 0] == 0.125 and w[0, 0, 3] == 0.25 and w[0, 3, 3] == 0.5 and w[4, 3, 2] == 1.0
    assert math.isclose(w.sum(), 4 * 6 * 8)  # the trapezoid rule of 1 over the box, in cells


@pytest.mark.parametrize("case", [1, 17])
def test_exact_for_quadratic_u_with_linear_a(case):
    """17^3, unit cube, a = 1 + 2y.  bc = 1: u = x^2 + y z (u_x = 0 at x = 0), f = 2a + 2z.  bc = 17: u = x^2 + y z^2 (u_x = 0 at
    x = 0, u_z = 0 at z = 0), f = 2a + 2 a y + 2 z^2.  The mirrored differences and the arithmetic-mean faces are exact for them:
    the restated residual is exactly 0.0 at every unknown."""
    n3 = (17, 17, 17)
    x, y, z = OC.nodes(n3)
    a = 1 + 2 * y
    if case == 1:
        u, f = x * x + y * z, 2 * a + 2 * z
    else:
        u, f = x * x + y * z * z, 2 * a + 2 * a * y + 2 * z * z
    r = OP.Op(n3, UNIT, np.float64, 0.0, a, bc=case).residual(u, f)
    print("exactness, bc = %d: max |residual| = %.3e over %d unknowns" % (case, np.abs(r).max(), OP.unknown_mask(n3, case).sum()))
    assert OP.face_unknowns(n3, case).sum() > 0
    assert np.abs(r).max() == 0.0


@pytest.mark.parametrize("coef", [False, True])
@pytest.mark.parametrize("bc", [1, 21, 63])
def test_weighted_operator_is_symmetric_and_negative_definite(bc, coef):
    n3, s = (9, 9, 9), 0.75
    g = np.random.default_rng(5)
    a = g.uniform(0.5, 2, O.shape(n3)) if coef else None
    p, w = g.uniform(-1, 1, O.shape(n3)), g.uniform(-1, 1, O.shape(n3))
    unk = OP.unknown_mask(n3, bc)
    p[~unk] = 0
    w[~unk] = 0
    W = OP.weights(n3, bc)
    Ap, Aw = OP.Op(n3, UNIT, np.float64, s, a, bc=bc).apply_A(p), OP.Op(n3, UNIT, np.float64, s, a, bc=bc).apply_A(w)
    wAp, pAw, pAp = float((W * w * Ap).sum()), float((W * p * Aw).sum()), float((W * p * Ap).sum())
    print("bc %d coef %d: <w, A p>_W = %.15e, <p, A w>_W = %.15e, <p, A p>_W = %.6e" % (bc, coef, wAp, pAw, pAp))
    assert abs(wAp - pAw) <= 1e-12 * abs(wAp)
    assert pAp < 0


def test_second_order_in_a_closed_box():
    """u = cos(pi x) cos(pi y) cos(pi z), bc = 63, s = 100, f = -(3 pi^2 + s) u, cycled to 1e-10 on 9^3, 17^3, 33^3: both ratios of
    the maximum errors in [3.5, 4.5] (measured: 3.99 and 4.00)"""
    s, errs = 100.0, []
    for k in (9, 17, 33):
        n3 = (k, k, k)
        x, y, z = OC.nodes(n3)
        u = np.cos(np.pi * x) * np.cos(np.pi * y) * np.cos(np.pi * z)
        H = OP.Hierarchy(OP.Op(n3, UNIT, np.float64, s, bc=63))
        H.f[0] = -(3 * np.pi ** 2 + s) * u
        cycles, rel, conv = H.cycle_to(2, 2, 1e-10, 50)
        assert conv, (k, cycles, rel)
        errs.append(float(np.abs(H.v[0] - u).max()))
    ratios = [errs[0] / errs[1], errs[1] / errs[2]]
    print("second order: errors %s, ratios %.3f %.3f" % (["%.3e" % e for e in errs], ratios[0], ratios[1]))
    assert all(3.5 <= q <= 4.5 for q in ratios), ratios


@pytest.mark.parametrize("bc,s,coef", VCYCLE_CASES)
def test_restated_cycle_converges(bc, s, coef):
    """fp64 V(2,2) on 33^3 from random v and f: the weighted residual falls below 1e-9 of its start in eight cycles (measured:
    4.3e-11 to 6.2e-11 on the first three cases, 8.3e-12 and 9.8e-12 on the last two)"""
    H = vcycle_case(bc, s, coef)
    W = OP.weights(H.sizes[0], bc)
    wnorm = lambda r: math.sqrt(math.fsum((W * r * r).ravel()))
    r0 = wnorm(H.residual(0))
    for _ in range(8):
        H.vcycle(0, 2, 2)
    rel = wnorm(H.residual(0)) / r0
    print("bc %d, s %g, coefficient %d: weighted relative residual %.3e after 8 V(2,2)" % (bc, s, coef, rel))
    assert rel < 1e-9, rel


@pytest.mark.parametrize("kdt", [1e-2, 5e-5])
def test_backward_euler_in_a_closed_box_keeps_the_heat_content(kdt):
    """17^3, bc = 63, the smooth coefficient, Gaussian initial data, five restated steps with kappa dt = kdt solved to 1e-10: the
    relative drift of sum(w u) stays below 1e-9 (measured: 4.2e-14 and 0.0)"""
    n3 = (17, 17, 17)
    H = OP.Hierarchy(OP.Op(n3, UNIT, np.float64, 0.0, OC.smooth_coefficient(n3), bc=63))
    H.v[0] = gaussian(n3)
    W = OP.weights(n3, 63)
    heat0 = math.fsum((W * H.v[0]).ravel())
    cycles, worst, conv = H.backward_euler(5, kdt, 1.0, 2, 2, 1e-10, 50)
    assert conv, (cycles, worst)
    drift = abs(math.fsum((W * H.v[0]).ravel()) - heat0) / abs(heat0)
    print("kappa dt %g: %d cycles, worst relative residual %.3e, relative drift of the heat content %.3e" % (kdt, cycles, worst, drift))
    assert drift < 1e-9, drift
