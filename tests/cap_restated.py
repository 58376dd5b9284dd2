"""The operator with a capacity, div(a grad u) - (s c) u = f, restated (a plain module, imported by test_cap_cpu.py and
test_gpu_cap.py): the arithmetic of csrc/mgx_cap3d.hip in numpy, colour by colour and in `dtype` -- coef_restated's expressions
with sc = s * c_P, one rounding, where they take s -- the capacity's restriction chain, the Neumann form through
neumann_restated's reflection (bc = 0: the interior alone, and then the reflected layer is never used), the cycles of
mg_multigrid3d.inc on such a hierarchy, plain cycling, flexible CG and backward Euler steps of c u_t = kappa div(a grad u) + q.
Arrays are in the reference layout, shape (sz, sy, sx); a and c hold all points.  Only the capacity of the updated point enters:
nothing of c is mirrored."""
import math

import numpy as np

import coef_restated as CO
import neumann_krylov_restated as NK
import neumann_restated as NR
import oracle as O
import semi_restated as S
from shift_restated import _nb, fsum_sq, full_plan


def _sc(s, c, dtype):
    return np.dtype(dtype).type(s) * np.ascontiguousarray(c, dtype)


def relax(n3, rng, v, f, a, c, s, ncycles, dtype, bc=0):
    """ncycles red-black sweeps over the unknowns: v = num / den with coef_restated.relax's num and den = (...) + s*c_P"""
    qx, qy, qz = CO.scales(n3, rng, dtype)
    v = np.array(v, dtype=dtype, order="C", copy=True)
    fi = np.ascontiguousarray(f, dtype)
    unk, col = NR.unknown_mask(n3, bc), NR.colours(n3)
    AW, AE, AN, AS, AD, AU = CO._faces(NR.mirror(np.ascontiguousarray(a, dtype)))
    den = ((qx * (AW + AE) + qy * (AN + AS)) + qz * (AD + AU)) + _sc(s, c, dtype)
    for _ in range(ncycles):
        for colour in (0, 1):
            o, e, n, so, d, u, _c = _nb(NR.mirror(v))
            num = ((qx * (AW * o + AE * e) + qy * (AN * n + AS * so)) + qz * (AD * d + AU * u)) - fi
            new = num / den
            m = unk & (col == colour)
            v[m] = new[m]
    return v


def residual(n3, rng, v, f, a, c, s, dtype, bc=0):
    """r = (((f - tx) - ty) - tz) + (s*c_P)*u_P at the unknowns, 0 at the Dirichlet points"""
    qx, qy, qz = CO.scales(n3, rng, dtype)
    fi = np.ascontiguousarray(f, dtype)
    o, e, n, so, d, u, cc = _nb(NR.mirror(np.ascontiguousarray(v, dtype)))
    AW, AE, AN, AS, AD, AU = CO._faces(NR.mirror(np.ascontiguousarray(a, dtype)))
    tx = qx * (AW * (o - cc) + AE * (e - cc))
    ty = qy * (AN * (n - cc) + AS * (so - cc))
    tz = qz * (AD * (d - cc) + AU * (u - cc))
    full = (((fi - tx) - ty) - tz) + _sc(s, c, dtype) * cc
    r = np.zeros(O.shape(n3), dtype)
    unk = NR.unknown_mask(n3, bc)
    r[unk] = full[unk]
    return r


def apply_A(n3, rng, p, a, c, s, dtype, bc=0):
    """q = A p = -(residual with f = 0) = div(a grad p) - (s c) p at the unknowns"""
    return -residual(n3, rng, p, np.zeros(O.shape(n3), dtype), a, c, s, dtype, bc)


def rhs(u, c, q, qscale, s, dtype, bc=0, f=None):
    """f = (-((s*c)*u)) - qscale*q at the unknowns; the other entries are those of `f` (default zeros)"""
    t = np.dtype(dtype).type
    u = np.ascontiguousarray(u, dtype)
    out = np.zeros(u.shape, dtype) if f is None else np.array(f, dtype)
    val = -(_sc(s, c, dtype) * u)
    if q is not None:
        val = val - t(qscale) * np.ascontiguousarray(q, dtype)
    m = NR.unknown_mask(tuple(reversed(u.shape)), bc)
    out[m] = val[m]
    return out


def coarse_capacities(sizes, masks, c, dtype):
    """c on every level: c_{l+1} = Restrict(c_l) by the step's mask, exactly as the coefficient goes down (c stays >= 0)"""
    return CO.coarse_coefficients(sizes, masks, c, dtype)


class Hierarchy:
    """v, f, a and c of every level and the cycles of mg_multigrid3d.inc: coef_restated.Hierarchy's without a mask (full or
    semi-coarsened), neumann_restated.Hierarchy's with one, around this operator's smoother and residual"""

    def __init__(self, n3, rng, a, c, s, bc=0, dtype=np.float64, coarsening="full"):
        self.rng, self.s, self.bc, self.dtype = list(rng), s, int(bc), dtype
        self.sizes, self.masks = S.plan(n3, rng) if coarsening == "semi" else full_plan(n3)
        assert not (self.bc and coarsening == "semi")
        self.v = [np.zeros(O.shape(n), dtype) for n in self.sizes]
        self.f = [np.zeros(O.shape(n), dtype) for n in self.sizes]
        self.a = CO.coarse_coefficients(self.sizes, self.masks, a, dtype)
        self.c = coarse_capacities(self.sizes, self.masks, c, dtype)

    def relax(self, l, k):
        self.v[l] = relax(self.sizes[l], self.rng, self.v[l], self.f[l], self.a[l], self.c[l], self.s, k, self.dtype, self.bc)

    def residual(self, l):
        return residual(self.sizes[l], self.rng, self.v[l], self.f[l], self.a[l], self.c[l], self.s, self.dtype, self.bc)

    def vcycle(self, l, v1, v2):
        (NR.Hierarchy.vcycle if self.bc else CO.Hierarchy.vcycle)(self, l, v1, v2)

    def fmg(self, l, v0, v1, v2):
        (NR.Hierarchy.fmg if self.bc else CO.Hierarchy.fmg)(self, l, v0, v1, v2)

    cycle_to = NR.Hierarchy.cycle_to

    def backward_euler(self, nsteps, dt, kappa, v1, v2, tol, maxit, source=None):
        """mgMultiGrid3D_<r>_BackwardEuler(krylov = 0): (cycles of all steps, worst relative residual, converged)"""
        t = np.dtype(self.dtype).type
        self.s = t(1.0 / (kappa * dt))
        total, worst = 0, 0.0
        for _ in range(nsteps):
            self.f[0] = rhs(self.v[0], self.c[0], source, t(1.0 / kappa), self.s, self.dtype, self.bc, f=self.f[0])
            k, rel, conv = self.cycle_to(v1, v2, tol, maxit)
            total, worst = total + k, max(worst, rel)
            if not conv:
                return total, worst, False
        return total, worst, True


def m_cycle(n3, rng, a, c, s, bc, v1, v2, dtype=np.float64, coarsening="full"):
    """the preconditioner of PCG: the V(v1, v2) cycle from zero on all points"""
    H = Hierarchy(n3, rng, a, c, s, bc, dtype, coarsening)

    def M(r):
        for l in range(len(H.sizes)):
            H.v[l] = np.zeros(O.shape(H.sizes[l]), dtype)
        H.f[0] = np.ascontiguousarray(r, dtype)
        H.vcycle(0, v1, v2)
        return H.v[0].copy()
    return M


def fcg(n3, rng, a, c, s, bc, v0, f, tol=1e-10, maxit=60, v1=2, v2=2, dtype=np.float64, coarsening="full"):
    """PCG(v1, v2, tol, maxit, krylov = 1 or 2): neumann_krylov_restated.wfcg with this operator (without a mask every weight is 1;
    a singular system is refused by the library, not restated): (x, iterations, history, converged, true relative residual)"""
    dtype = np.dtype(dtype).type
    unk = NR.unknown_mask(n3, bc)
    W = NR.weights(n3, bc)
    M = m_cycle(n3, rng, a, c, s, bc, v1, v2, dtype, coarsening)
    f = np.ascontiguousarray(f, dtype)

    def res(x):
        return residual(n3, rng, x, f, a, c, s, dtype, bc)

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
        q = apply_A(n3, rng, p, a, c, s, dtype, bc)
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
        beta = -alpha * NK.wdot(W, z, q) / rz
        rz = NK.wdot(W, r, z)
        p = z + dtype(beta) * p
    return x, k, np.array(hist), conv, math.sqrt(fsum_sq(res(x)) / rr0)


# ---- the capacities of the issue's table, on the nodes of the unit cube
def smooth_capacity(n3, dtype=np.float64):
    """1 + 0.5 cos(2 pi x) sin(pi z) + 0.25 y"""
    x, y, z = CO._nodes(n3)
    return (1.0 + 0.5 * np.cos(2 * np.pi * x) * np.sin(np.pi * z) + 0.25 * y).astype(dtype)


def block_capacity(n3, inside, outside, dtype=np.float64):
    """`inside` in the cube |x-.5|, |y-.5|, |z-.5| < .25, `outside` elsewhere"""
    x, y, z = CO._nodes(n3)
    m = (np.abs(x - 0.5) < 0.25) & (np.abs(y - 0.5) < 0.25) & (np.abs(z - 0.5) < 0.25)
    return np.where(m, float(inside), float(outside)).astype(dtype)


def random_capacity(n3, dtype, seed):
    """uniform in [0, 2] with a block of zeros (the operator is purely elliptic there)"""
    c = np.random.default_rng(seed).uniform(0, 2, O.shape(n3)).astype(dtype)
    sz, sy, sx = c.shape
    c[: max(1, sz // 2), sy // 3:, : max(2, sx // 2)] = 0
    return c
