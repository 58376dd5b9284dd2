"""Convective (Robin) and prescribed-flux walls without a GPU: the library exports the new entries, rejects NULL arguments and bad
wall data before it touches the device and keeps the sizes and offsets of both struct mirrors; the restatement of the arithmetic
(tests/op_restated.py) is symmetric under the trapezoid
weights and negative definite, second-order accurate, exact on the constant state, and its cycle is a solver."""
import ctypes as C
import math

import numpy as np
import pytest

import op_cases as OC
import op_restated as OP
import oracle as O
import pde_multigrid_amd as P
from pde_multigrid_amd.multigrid import _grid3_struct

UNIT = [0, 1, 0, 1, 0, 1]
RG = [-1, 1, 0, 2, 0.5, 3]
N = None
WALL_ENTRIES = ("relax_shift_wall", "relax_coef_wall", "relax_cap_wall", "residual_shift_wall", "residual_coef_wall", "residual_cap_wall",
                "laplace_dot_shift_wall", "apply_coef_dot_wall", "apply_cap_dot_wall")


# ------------------------------------------------------------------------------------------ the library's new surface
def _calls(ct, buf, n, h, bc, beta):
    """every _wall entry with all arguments given (host buffers stand in: the checks come before any use)"""
    s = ct(0.5)
    return {"relax_shift_wall": (buf, buf, buf, n, h, s, 1, bc, beta), "relax_coef_wall": (buf, buf, buf, buf, n, h, s, 1, bc, beta),
            "relax_cap_wall": (buf, buf, buf, buf, buf, n, h, s, 1, bc, beta),
            "residual_shift_wall": (buf, buf, buf, buf, n, h, s, buf, buf, bc, beta),
            "residual_coef_wall": (buf, buf, buf, buf, buf, n, h, s, buf, buf, bc, beta),
            "residual_cap_wall": (buf, buf, buf, buf, buf, buf, n, h, s, buf, buf, bc, beta),
            "laplace_dot_shift_wall": (buf, buf, buf, n, h, s, buf, buf, bc, beta),
            "apply_coef_dot_wall": (buf, buf, buf, buf, n, h, s, buf, buf, bc, beta),
            "apply_cap_dot_wall": (buf, buf, buf, buf, buf, n, h, s, buf, buf, bc, beta)}


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_new_symbols_are_exported_and_reject_null(sfx):
    ct = C.c_float if sfx == "f32" else C.c_double
    L, I = P.lib, P.MGX_ERR_INVALID
    buf = (C.c_double * 64)()
    n, h, beta = (C.c_int * 3)(5, 5, 5), (ct * 3)(0.25, 0.25, 0.25), (ct * 6)(1, 0, 0, 0, 0, 0)
    full = _calls(ct, buf, n, h, 1, beta)
    assert set(full) == set(WALL_ENTRIES)
    for k, args in full.items():
        fn = getattr(L, "mgx3dxs_%s_%s" % (k, sfx))
        assert fn(*[None if isinstance(a, C.Array) else a for a in args]) == I, k
        assert b"NULL" in L.mgx_last_error(), k
        assert fn(*args[:-1], None) == I, k  # beta alone missing
        assert b"NULL" in L.mgx_last_error(), k
    rhs = getattr(L, "mgx3dxs_wall_rhs_" + sfx)
    assert rhs(N, N, N, N, N, 1) == I and b"NULL" in L.mgx_last_error()
    assert rhs(buf, buf, n, h, N, 1) == I and b"NULL" in L.mgx_last_error()
    for k in ("set_wall", "get_wall", "add_wall_flux"):
        assert hasattr(L, "mgMultiGrid3D_%s_%s" % (sfx, k)), k
    assert getattr(L, "mgMultiGrid3D_%s_set_wall" % sfx)(N, N, N) == I
    assert getattr(L, "mgMultiGrid3D_%s_get_wall" % sfx)(N, N, N) == I
    assert getattr(L, "mgMultiGrid3D_%s_add_wall_flux" % sfx)(N) == I


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_bad_wall_data_is_refused_before_anything_runs(sfx):
    """a beta that is negative or not finite, a g that is not finite, either on a face whose bit is clear, a mask outside 0 .. 63"""
    ct = C.c_float if sfx == "f32" else C.c_double
    L, I = P.lib, P.MGX_ERR_INVALID
    buf = (C.c_double * 64)()
    n, h = (C.c_int * 3)(5, 5, 5), (ct * 3)(0.25, 0.25, 0.25)
    big = float(np.finfo(np.float32 if sfx == "f32" else np.float64).max)
    bad = [(1, (-1, 0, 0, 0, 0, 0), b"beta"), (1, (float("nan"), 0, 0, 0, 0, 0), b"beta"), (1, (float("inf"), 0, 0, 0, 0, 0), b"beta"),
           (1, (1, 2, 0, 0, 0, 0), b"mask"), (0, (0, 0, 0, 1, 0, 0), b"mask"), (64, (0,) * 6, b"bc"), (-1, (0,) * 6, b"bc"),
           (1, (big, 0, 0, 0, 0, 0), b"not finite in this precision")]  # (finite, but 2 beta / h is not)
    for bc, beta, word in bad:
        for k, args in _calls(ct, buf, n, h, bc, (ct * 6)(*beta)).items():
            assert getattr(L, "mgx3dxs_%s_%s" % (k, sfx))(*args) == I, (k, bc, beta)
            assert word in L.mgx_last_error(), (k, L.mgx_last_error())
    rhs = getattr(L, "mgx3dxs_wall_rhs_" + sfx)
    for bc, g, word in [(1, (float("nan"), 0, 0, 0, 0, 0), b"g["), (1, (float("-inf"), 0, 0, 0, 0, 0), b"g["), (1, (0, -3, 0, 0, 0, 0), b"mask"),
                        (64, (0,) * 6, b"bc"), (1, (-big, 0, 0, 0, 0, 0), b"not finite in this precision")]:
        assert rhs(buf, buf, n, h, (ct * 6)(*g), bc) == I, (bc, g)
        assert word in L.mgx_last_error(), L.mgx_last_error()


@pytest.mark.parametrize("sfx,ct", [("f32", C.c_float), ("f64", C.c_double)])
def test_both_mirrors_still_have_the_library_sizes(sfx, ct):
    """the wall table takes the eight bytes of graph_key[29] in front of cap: no member moved, the struct kept its size"""
    G, M = _grid3_struct(ct)
    for S_, name in ((G, "mgGrid3D_%s_sizeof"), (M, "mgMultiGrid3D_%s_sizeof")):
        fn = getattr(P.lib, name % sfx)
        fn.restype = C.c_size_t
        assert C.sizeof(S_) == fn(), name
    assert G._fields_[-1][0] == "d_a" and M._fields_[-1][0] == "shift"
    assert M.wall.offset == M.graph_key.offset + 29 * 8 and M.graph_key.size == 29 * 8
    assert M.cap.offset == M.graph_key.offset + 30 * 8 and M.pcg_fproj.offset == M.graph_key.offset + 31 * 8
    assert M.f_rim_zero.offset == M.graph_key.offset + 32 * 8
    assert M.bc.offset == M.pcg_graph_exec.offset + C.sizeof(C.c_void_p)
    assert M.graph_exec.offset + 32 * 8 == M.graph_key.offset


# ------------------------------------------------------------------------------------------ the restated arithmetic
def test_a_wall_changes_the_points_with_a_diagonal_and_no_others():
    """mask 37 with a beta on x-low only: the residual differs from the insulated one exactly at the unknowns of that face, by
    d u_P up to rounding"""
    n3, bc, beta = (9, 7, 5), 37, (3.0, 0, 0, 0, 0, 0)
    g = np.random.default_rng(4)
    v, f = g.uniform(-1, 1, O.shape(n3)), g.uniform(-1, 1, O.shape(n3))
    r0 = OP.Op(n3, RG, np.float64, 0.75, bc=bc).residual(v, f)
    r1 = OP.Op(n3, RG, np.float64, 0.75, bc=bc, beta=beta).residual(v, f)
    d = OP.Op(n3, RG, np.float64, 0.0, bc=bc, beta=beta).diagonal()
    unk = OP.unknown_mask(n3, bc)
    assert ((r0 != r1) <= ((d != 0) & unk)).all() and (r0 != r1).sum() > 0
    assert d[:, :, 0].min() == 2 * 3.0 / (2.0 / 8) and (d[:, :, 1:] == 0).all()
    assert np.abs((r1 - r0)[unk] - (d * v)[unk]).max() < 1e-12 * 30


@pytest.mark.parametrize("bc,s,beta", [(63, 0.75, (1.5, 0, 0.25, 4, 0, 2)), (37, 0.75, (3, 0, 10, 0, 0, 0.5)), (63, 0.0, (0, 0, 0, 2, 0, 0))])
@pytest.mark.parametrize("cap", [False, True])
def test_weighted_operator_is_symmetric_and_negative_definite(bc, s, beta, cap):
    n3 = (9, 9, 9)
    g = np.random.default_rng(5)
    a = OC.smooth_coefficient(n3)
    c = OC.random_capacity(n3, np.float64, 6) if cap else None
    p, w = g.uniform(-1, 1, O.shape(n3)), g.uniform(-1, 1, O.shape(n3))
    unk = OP.unknown_mask(n3, bc)
    p[~unk] = 0
    w[~unk] = 0
    W = OP.weights(n3, bc)
    Ap, Aw = (OP.Op(n3, UNIT, np.float64, s, a, c, bc, beta).apply_A(x) for x in (p, w))
    wAp, pAw, pAp = float((W * w * Ap).sum()), float((W * p * Aw).sum()), float((W * p * Ap).sum())
    print("bc %d: <w, A p>_W = %.15e, <p, A w>_W = %.15e, <p, A p>_W = %.6e" % (bc, wAp, pAw, pAp))
    assert abs(wAp - pAw) <= 1e-12 * abs(wAp)
    assert pAp < 0
    one = unk.astype(np.float64)  # the constant is no null vector any more: a wall loses heat
    assert float((W * one * OP.Op(n3, UNIT, np.float64, s, a, c, bc, beta).apply_A(one)).sum()) < 0


def _accuracy_case(n):
    """u = exp(x + y/2) cos z, a = 1 + x/2 + yz/4, s = 2, mask 62, betas (0, 2, 0.5, 0, 3, 1) on n^3; g = a du/dn + beta u varies
    along each face and is folded into f with the documented formula, f -= 2 g(P) / h.  Returns the maximum error of the
    solution of the discrete system at the unknowns."""
    n3, s, bc, beta = (n,) * 3, 2.0, 62, (0, 2, 0.5, 0, 3, 1)
    x, y, z = OC.nodes(n3)
    e = np.exp(x + y / 2)
    u, a = e * np.cos(z), 1 + x / 2 + y * z / 4
    grad = (u, u / 2, -e * np.sin(z))
    f = a * (u + u / 4 - u) + 0.5 * grad[0] + (z / 4) * grad[1] + (y / 4) * grad[2] - s * u
    h = 1.0 / (n - 1)
    unk = OP.unknown_mask(n3, bc)
    for k in range(6):
        if not (bc >> k) & 1:
            continue
        axis, high = k >> 1, k & 1
        idx = [slice(None)] * 3
        idx[2 - axis] = -1 if high else 0
        idx = tuple(idx)
        gP = (1 if high else -1) * a[idx] * grad[axis][idx] + beta[k] * u[idx]
        f[idx] = np.where(unk[idx], f[idx] - 2 * gP / h, f[idx])
    H = OP.Hierarchy(OP.Op(n3, UNIT, np.float64, s, a, bc=bc, beta=beta))
    H.v[0] = np.where(unk, 0.0, u)
    H.f[0] = f
    cycles, rel, conv = H.cycle_to(2, 2, 1e-11, 40)
    assert conv, (n, cycles, rel)
    return float(np.abs(H.v[0] - u)[unk].max())


def test_second_order():
    """the issue's case: both error ratios in [3.5, 4.5]"""
    err = [_accuracy_case(n) for n in (9, 17, 33)]
    print("max errors %.3e %.3e %.3e, ratios %.3f %.3f" % (*err, err[0] / err[1], err[1] / err[2]))
    assert 3.5 <= err[0] / err[1] <= 4.5 and 3.5 <= err[1] / err[2] <= 4.5, err


@pytest.mark.parametrize("coef", [False, True])
def test_the_constant_state_has_a_residual_of_exactly_zero(coef):
    """mask 63, s = 0, f = 0, g_k = beta_k * 7: u = 7 balances every wall, and the residual is exactly 0 (the betas are dyadic and
    the spacings powers of two, so that 2 (7 beta) / h and 7 (2 beta / h) are the same number)"""
    n3, beta = (17, 9, 5), (1.0, 0.5, 0.0, 2.0, 0.25, 4.0)
    g = tuple(b * 7 for b in beta)
    H = OP.Hierarchy(OP.Op(n3, UNIT, np.float64, 0.0, OC.smooth_coefficient(n3) if coef else None, bc=63, beta=beta), g=g)
    H.v[0][:] = 7.0
    H.add_wall_flux()
    r = H.residual(0)
    assert (H.f[0] != 0).any() and not r.any(), np.abs(r).max()


@pytest.mark.parametrize("case", range(len(OC.WALL_VCYCLE_CASES)))
def test_restated_vcycle_converges_within_the_recorded_count(case):
    """V(2,2) from a random start at 33^3: below 1e-9 of the initial residual within the count recorded in DESIGN.md 18 (to 1e-10)
    plus two"""
    recorded = OC.WALL_VCYCLE_CASES[case][4]
    H = OC.vcycle_case(*OC.WALL_VCYCLE_CASES[case][:4])
    cycles, rel, conv = H.cycle_to(2, 2, 1e-10, 40)
    print("case %d %r: %d cycles to 1e-10 (relative residual %.3e)" % (case, OC.WALL_VCYCLE_CASES[case][:4], cycles, rel))
    H = OC.vcycle_case(*OC.WALL_VCYCLE_CASES[case][:4])
    k9, rel9, conv9 = H.cycle_to(2, 2, 1e-9, recorded + 2)
    assert conv and cycles == recorded, (cycles, recorded)
    assert conv9 and k9 <= recorded + 2, (k9, rel9)


def test_restated_heat_balance_in_a_closed_box():
    """five backward Euler steps in a closed 17^3 box with a capacity and walls that lose and feed heat: per step
    sum_W(c u') - sum_W(c u) = kappa dt sum_W(2 (g - beta u') / h), up to the solves' tolerance"""
    worst, _, bound = OC.heat_balance_restated()
    print("worst relative imbalance of a step %.3e (bound %.3e)" % (worst, bound))
    assert worst <= bound
