"""Convective (Robin) and prescribed-flux walls restated (a plain module, imported by test_robin_cpu.py and test_gpu_robin.py):
what csrc/mgx_wall3d.hip adds to the shifted, the variable-coefficient and the capacity operator, in numpy, colour by colour and in
`dtype`, on top of neumann_restated, coef_restated and cap_restated.

On a face flagged in the mask bc the wall law is  a du/dn + beta u = g  (n outward).  The half cell at a face unknown gains
2 (g - beta u_P) / h per wall face it lies on, so
  d_k  = (t(2) * t(beta_k)) / h_axis(k)           once per level, in `dtype`, from that level's own spacing
  d(P) = ((dx + dy) + dz)                          the d_k of the faces P lies on, 0 for an axis on whose faces P does not lie
  se   = base + d(P) where d(P) != 0, else base    base = t(s), with a capacity t(s) * c_P
and every point expression is the base module's with se where it takes the shift: where d(P) == 0 the bits of neumann_restated /
cap_restated, elsewhere the wall's.  g touches the right-hand side of level 0 only: f -= (t(2) * t(g_k)) / h_axis(k), face by face
in the order x, y, z.  a = None means the shifted operator, c = None no capacity.  Arrays are in the reference layout, shape
(sz, sy, sx); beta and g in the order of the mask's bits (x-low, x-high, y-low, y-high, z-low, z-high)."""
import math

import numpy as np

import cap_restated as CA
import coef_restated as CO
import neumann_krylov_restated as NK
import neumann_restated as NR
import oracle as O
from shift_restated import _nb, fsum_sq, full_plan, squares

ZERO = (0.0,) * 6


def spacings(n3, rng, dtype):
    """h as Grid3D forms it: range / (real)(size - 1) in `dtype`"""
    t = np.dtype(dtype).type
    return [t(t(rng[2 * d + 1]) - t(rng[2 * d])) / t(int(n3[d]) - 1) for d in range(3)]


def face_terms(n3, rng, val, bc, dtype):
    """(t(2) * t(val_k)) / h_axis(k) for the six faces; a value other than 0 on a face the mask does not flag is an error"""
    t = np.dtype(dtype).type
    h = spacings(n3, rng, dtype)
    assert all(v == 0 or (int(bc) >> k) & 1 for k, v in enumerate(val)), (val, bc)
    return [t((t(2) * t(val[k])) / h[k >> 1]) for k in range(6)]


def per_axis(n3, terms, dtype):
    """the three arrays of the x-, y- and z-face term of every point (0 off that axis's faces)"""
    sx, sy, sz = (int(k) for k in n3)
    z, y, x = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    t = np.dtype(dtype).type
    out = []
    for d, (i, m) in enumerate(((x, sx), (y, sy), (z, sz))):
        out.append(np.where(i == 0, terms[2 * d], np.where(i == m - 1, terms[2 * d + 1], t(0))).astype(dtype))
    return out


def diagonal(n3, rng, beta, bc, dtype):
    """d(P) at every point"""
    dx, dy, dz = per_axis(n3, face_terms(n3, rng, beta, bc, dtype), dtype)
    return (dx + dy) + dz


def _se(n3, rng, c, s, bc, beta, dtype):
    """the effective shift of every point: an array, or the scalar t(s) without a capacity and without a wall"""
    t = np.dtype(dtype).type
    base = t(s) if c is None else t(s) * np.ascontiguousarray(c, dtype)
    d = diagonal(n3, rng, beta, bc, dtype)
    return np.where(d != 0, base + d, base).astype(dtype)


def relax(n3, rng, v, f, a, c, s, ncycles, bc, beta, dtype):
    """ncycles red-black sweeps over the unknowns"""
    t = np.dtype(dtype).type
    v = np.array(v, dtype=dtype, order="C", copy=True)
    fi = np.ascontiguousarray(f, dtype)
    unk, col = NR.unknown_mask(n3, bc), NR.colours(n3)
    se = _se(n3, rng, c, s, bc, beta, dtype)
    if a is None:
        hx2, hy2, hz2 = squares(n3, rng, dtype)
        den = t(2) * (hy2 * hz2 + hx2 * hz2 + hx2 * hy2) + se * hx2 * hy2 * hz2
    else:
        qx, qy, qz = CO.scales(n3, rng, dtype)
        AW, AE, AN, AS, AD, AU = CO._faces(NR.mirror(np.ascontiguousarray(a, dtype)))
        den = ((qx * (AW + AE) + qy * (AN + AS)) + qz * (AD + AU)) + se
    for _ in range(ncycles):
        for colour in (0, 1):
            o, e, n, so, d, u, _c = _nb(NR.mirror(v))
            if a is None:
                num = o * (hy2 * hz2) + e * (hy2 * hz2) + n * (hx2 * hz2) + so * (hx2 * hz2) + d * (hx2 * hy2) + u * (hx2 * hy2) - fi * hx2 * hy2 * hz2
            else:
                num = ((qx * (AW * o + AE * e) + qy * (AN * n + AS * so)) + qz * (AD * d + AU * u)) - fi
            new = num / den
            m = unk & (col == colour)
            v[m] = new[m]
    return v


def residual(n3, rng, v, f, a, c, s, bc, beta, dtype):
    """r at the unknowns, 0 at the Dirichlet points"""
    t = np.dtype(dtype).type
    fi = np.ascontiguousarray(f, dtype)
    o, e, n, so, d, u, cc = _nb(NR.mirror(np.ascontiguousarray(v, dtype)))
    se = _se(n3, rng, c, s, bc, beta, dtype)
    if a is None:
        hx2, hy2, hz2 = squares(n3, rng, dtype)
        full = (fi - ((o - t(2) * cc + e) / hx2) - ((n - t(2) * cc + so) / hy2) - ((d - t(2) * cc + u) / hz2)) + se * cc
    else:
        qx, qy, qz = CO.scales(n3, rng, dtype)
        AW, AE, AN, AS, AD, AU = CO._faces(NR.mirror(np.ascontiguousarray(a, dtype)))
        tx = qx * (AW * (o - cc) + AE * (e - cc))
        ty = qy * (AN * (n - cc) + AS * (so - cc))
        tz = qz * (AD * (d - cc) + AU * (u - cc))
        full = (((fi - tx) - ty) - tz) + se * cc
    r = np.zeros(O.shape(n3), dtype)
    unk = NR.unknown_mask(n3, bc)
    r[unk] = full[unk]
    return r


def apply_A(n3, rng, p, a, c, s, bc, beta, dtype):
    """q = A p = -(residual with f = 0) at the unknowns"""
    return -residual(n3, rng, p, np.zeros(O.shape(n3), dtype), a, c, s, bc, beta, dtype)


def add_flux(n3, rng, f, g, bc, dtype):
    """f - 2 g / h at the face unknowns: successively for the x-, the y- and the z-face of a point whose term is not 0"""
    out = np.array(f, dtype)
    m = NR.face_unknowns(n3, bc)
    for term in per_axis(n3, face_terms(n3, rng, g, bc, dtype), dtype):
        mk = m & (term != 0)
        out[mk] = out[mk] - term[mk]
    return out


def wall_sum(n3, rng, u, beta, g, bc):
    """sum_W of the wall terms 2 (g - beta u_P) / h over the unknowns, in double: what the walls feed into the box"""
    W = NR.weights(n3, bc)
    gq = sum(per_axis(n3, face_terms(n3, rng, g, bc, np.float64), np.float64))
    d = diagonal(n3, rng, beta, bc, np.float64)
    return math.fsum((W * (gq - d * np.asarray(u, np.float64))).ravel())


class Hierarchy:
    """v, f (a, c) of every level and the cycles of mg_multigrid3d.inc on a hierarchy with the mask bc and the walls (beta, g):
    neumann_restated.Hierarchy's cycles around this module's smoother and residual, d_k formed on every level from its own spacing;
    g enters f[0] through add_wall_flux()"""

    def __init__(self, n3, rng, a, c, s, bc, beta=ZERO, g=ZERO, dtype=np.float64):
        self.rng, self.s, self.bc, self.dtype = list(rng), s, int(bc), dtype
        self.beta, self.g = tuple(beta), tuple(g)
        self.sizes, self.masks = full_plan(n3)
        self.v = [np.zeros(O.shape(n), dtype) for n in self.sizes]
        self.f = [np.zeros(O.shape(n), dtype) for n in self.sizes]
        self.a = CO.coarse_coefficients(self.sizes, self.masks, a, dtype) if a is not None else [None] * len(self.sizes)
        self.c = CA.coarse_capacities(self.sizes, self.masks, c, dtype) if c is not None else [None] * len(self.sizes)

    def relax(self, l, k):
        self.v[l] = relax(self.sizes[l], self.rng, self.v[l], self.f[l], self.a[l], self.c[l], self.s, k, self.bc, self.beta, self.dtype)

    def residual(self, l):
        return residual(self.sizes[l], self.rng, self.v[l], self.f[l], self.a[l], self.c[l], self.s, self.bc, self.beta, self.dtype)

    def add_wall_flux(self):
        self.f[0] = add_flux(self.sizes[0], self.rng, self.f[0], self.g, self.bc, self.dtype)

    vcycle = NR.Hierarchy.vcycle
    fmg = NR.Hierarchy.fmg
    cycle_to = NR.Hierarchy.cycle_to

    def backward_euler(self, nsteps, dt, kappa, v1, v2, tol, maxit, source=None):
        """mgMultiGrid3D_<r>_BackwardEuler(krylov = 0): (cycles of all steps, worst relative residual, converged)"""
        t = np.dtype(self.dtype).type
        self.s = t(1.0 / (kappa * dt))
        total, worst = 0, 0.0
        for _ in range(nsteps):
            if self.c[0] is not None:
                self.f[0] = CA.rhs(self.v[0], self.c[0], source, t(1.0 / kappa), self.s, self.dtype, self.bc, f=self.f[0])
            else:
                self.f[0] = NR.rhs(self.v[0], source, t(1.0 / kappa), self.s, self.bc, self.dtype, f=self.f[0])
            self.add_wall_flux()
            k, rel, conv = self.cycle_to(v1, v2, tol, maxit)
            total, worst = total + k, max(worst, rel)
            if not conv:
                return total, worst, False
        return total, worst, True


def m_cycle(n3, rng, a, c, s, bc, beta, v1, v2, dtype=np.float64):
    """the preconditioner of PCG: the V(v1, v2) cycle from zero on all points"""
    H = Hierarchy(n3, rng, a, c, s, bc, beta, ZERO, dtype)

    def M(r):
        for l in range(len(H.sizes)):
            H.v[l] = np.zeros(O.shape(H.sizes[l]), dtype)
        H.f[0] = np.ascontiguousarray(r, dtype)
        H.vcycle(0, v1, v2)
        return H.v[0].copy()
    return M


def wfcg(n3, rng, a, c, s, bc, beta, v0, f, tol=1e-10, maxit=60, v1=2, v2=2, dtype=np.float64):
    """PCG(v1, v2, tol, maxit, krylov = 2) with a lossy wall (some beta > 0: regular, nothing is projected), with the associations
    of neumann_krylov_restated.wfcg: (x, iterations, history, converged, true relative residual)"""
    assert any(b > 0 for b in beta)
    return _wfcg(n3, rng, a, c, s, bc, beta, v0, f, tol, maxit, v1, v2, dtype)


def _wfcg(n3, rng, a, c, s, bc, beta, v0, f, tol, maxit, v1, v2, dtype):
    """the iteration of wfcg for any betas: with all of them zero (and a regular system) it is neumann_krylov_restated.wfcg's, bit
    for bit -- test_robin_cpu.py holds the two copies of the loop together that way"""
    dtype = np.dtype(dtype).type
    unk = NR.unknown_mask(n3, bc)
    W = NR.weights(n3, bc)
    M = m_cycle(n3, rng, a, c, s, bc, beta, v1, v2, dtype)
    f = np.ascontiguousarray(f, dtype)

    def res(x):
        return residual(n3, rng, x, f, a, c, s, bc, beta, dtype)

    x = np.array(v0, dtype)
    r = res(x)
    rr0 = fsum_sq(r)
    hist, k, restart, conv = [], 0, True, False
    if rr0 == 0.0:
        return x, 0, np.array(hist), True, 0.0
    while k < maxit:
        if restart:
            z = M(r)
            p, rz, restart = z.copy(), NK.wdot(W, r, z), False
        k += 1
        q = apply_A(n3, rng, p, a, c, s, bc, beta, dtype)
        alpha = rz / NK.wdot(W, p, q)
        x[unk] = x[unk] + dtype(alpha) * p[unk]
        r = r - dtype(alpha) * q
        rel = math.sqrt(fsum_sq(r) / rr0)
        hist.append(rel)
        if rel < tol:
            r = res(x)
            if math.sqrt(fsum_sq(r) / rr0) < tol:
                conv = True
                break
            restart = True
            continue
        z = M(r)
        beta_cg = -alpha * NK.wdot(W, z, q) / rz
        rz = NK.wdot(W, r, z)
        p = z + dtype(beta_cg) * p
    return x, k, np.array(hist), conv, math.sqrt(fsum_sq(res(x)) / rr0)


# ---- the cases the CPU and the GPU tests share
# the five regular V(2,2) cases of DESIGN.md 18 at 33^3, unit cube: (mask, s, smooth coefficient?, betas, recorded cycles to 1e-10)
VCYCLE_CASES = [
    (63, 0.0, False, (1.0,) * 6, 8),
    (37, 0.0, True, (3.0, 0.0, 10.0, 0.0, 0.0, 0.5), 8),
    (63, 100.0, True, (1e3,) * 6, 7),
    (1, 0.0, False, (1e6, 0.0, 0.0, 0.0, 0.0, 0.0), 5),
    (63, 0.0, True, (5.0, 0.0, 0.0, 0.0, 0.0, 2.0), 10),
]


def vcycle_case(case, seed=11, n3=(33, 33, 33)):
    """the hierarchy of VCYCLE_CASES[case] from a random start (v drawn first) and a random f"""
    bc, s, coef, beta, _ = VCYCLE_CASES[case]
    g = np.random.default_rng(seed)
    H = Hierarchy(n3, NK.UNIT, CO.smooth_coefficient(n3) if coef else None, None, s, bc, beta)
    H.v[0], H.f[0] = g.uniform(-1, 1, O.shape(n3)), g.uniform(-1, 1, O.shape(n3))
    return H


def mixed_betas(bc):
    """a set that leaves some flagged faces at 0: every second flagged face gets a beta"""
    out, take = [], True
    for k in range(6):
        if (bc >> k) & 1:
            out.append((0.5 + 0.75 * k) if take else 0.0)
            take = not take
        else:
            out.append(0.0)
    return tuple(out)


# ---- the heat balance of a closed box whose walls lose and feed heat (test_robin_cpu.py, test_gpu_robin.py)
# The bound on the imbalance of a step.  The step solves  A u' - s c u' - d u' = rhs  to a residual r with |r|_2 < tol |r_0|_2,
# r_0 the residual of the old u against the step's right-hand side.  Summed with the weights W the operator's flux terms cancel in
# a closed box, which leaves  sum_W(c u') - sum_W(c u) - kappa dt sum_W(wall terms) = -kappa dt sum_W(r),  and by Cauchy-Schwarz
# |sum_W(r)| <= |W|_2 |r|_2 < |W|_2 tol |r_0|_2.  heat_bound() evaluates that, relative to sum_W(c u_0) as heat_balance() reports
# it: what the restatement has to meet on the CPU (it measures 2.3e-11 where the bound is 1.0e-9: the residuals of a converged cycle
# are far from aligned with W); the GPU test holds ten times the bound.
HEAT_CASE = dict(n3=(17, 17, 17), beta=(2.0, 0.0, 0.5, 0.0, 0.0, 1.0), g=(0.0, 1.5, 0.0, 0.0, -0.5, 1.0), dt=1e-2, kappa=1.0, steps=5)


def heat_balance(n3, c, u_steps, beta, g, dt, kappa):
    """the worst |change of sum_W(c u) - kappa dt sum_W(wall terms of the new u)| of a step, relative to sum_W(c u_0)"""
    W = NR.weights(n3, 63)
    heat = [math.fsum((W * c * u).ravel()) for u in u_steps]
    worst = 0.0
    for k in range(1, len(u_steps)):
        wall = kappa * dt * wall_sum(n3, NK.UNIT, u_steps[k], beta, g, 63)
        worst = max(worst, abs((heat[k] - heat[k - 1]) - wall) / abs(heat[0]))
    return worst, heat


def heat_bound(n3, a, c, u_steps, beta, g, dt, kappa, tol):
    """kappa dt |W|_2 tol max_k |r_0 of step k|_2 / |sum_W(c u_0)| (the derivation above)"""
    W = NR.weights(n3, 63)
    s = 1.0 / (kappa * dt)
    r0 = 0.0
    for k in range(1, len(u_steps)):
        rhs = add_flux(n3, NK.UNIT, CA.rhs(u_steps[k - 1], c, None, 1.0 / kappa, s, np.float64, 63), g, 63, np.float64)
        r0 = max(r0, math.sqrt(fsum_sq(residual(n3, NK.UNIT, u_steps[k - 1], rhs, a, c, s, 63, beta, np.float64))))
    return kappa * dt * math.sqrt(float((W * W).sum())) * tol * r0 / abs(math.fsum((W * c * u_steps[0]).ravel()))


def heat_balance_restated():
    k = HEAT_CASE
    n3 = k["n3"]
    c = CA.smooth_capacity(n3)
    H = Hierarchy(n3, NK.UNIT, CO.smooth_coefficient(n3), c, 0.0, 63, k["beta"], k["g"])
    H.v[0] = NR.gaussian(n3)
    us = [H.v[0].copy()]
    for _ in range(k["steps"]):
        cycles, worst, conv = H.backward_euler(1, k["dt"], k["kappa"], 2, 2, 1e-10, 60)
        assert conv, (cycles, worst)
        us.append(H.v[0].copy())
    worst, heat = heat_balance(n3, c, us, k["beta"], k["g"], k["dt"], k["kappa"])
    assert abs(heat[-1] - heat[0]) > 1e-4 * abs(heat[0]), heat  # the walls did move heat
    return worst, heat, heat_bound(n3, CO.smooth_coefficient(n3), c, us, k["beta"], k["g"], k["dt"], k["kappa"], 1e-10)
