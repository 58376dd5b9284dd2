"""Harmonic-mean face coefficients restated (a plain module, imported by test_hmean_cpu.py and test_gpu_hmean.py): the arithmetic
of csrc/mgx_hmean3d.hip in numpy, colour by colour and in `dtype`.  The operators are those of coef_restated / cap_restated /
robin_restated with ONE function swapped: where coef_restated._faces forms AW = aO + aC (likewise AE .. AU) the harmonic operator
forms the doubled harmonic mean
  AW = t(4) * ((aO * aC) / (aO + aC))
and everything after it -- den, num, tx, ty, tz, the effective shift of a capacity and of the walls, the restriction chains, the
cycles, flexible CG and the backward Euler steps -- is those modules' code, run while the swap is in place (`harmonic()`).  Product
and sum commute, so a face has the same bits seen from either of its two nodes.  mean="arithmetic" runs the same code without the
swap: the bits of the base modules.  a holds all points; c = None means no capacity, bc = 0 no mask, beta = ZERO no wall.  Arrays
are in the reference layout, shape (sz, sy, sx)."""
import contextlib
import math

import numpy as np

import cap_restated as CA
import coef_restated as CO
import neumann_krylov_restated as NK
import neumann_restated as NR
import oracle as O
import robin_restated as RB
import semi_restated as S
from robin_restated import ZERO
from shift_restated import _nb, fsum_sq


def faces(a):
    """AW, AE, AN, AS, AD, AU of every interior point of `a`: the doubled harmonic means, in a's dtype"""
    o, e, n, so, d, u, c = _nb(a)
    t = a.dtype.type
    return tuple(t(4) * ((q * c) / (q + c)) for q in (o, e, n, so, d, u))


@contextlib.contextmanager
def harmonic(mean="harmonic"):
    """while it is open the restated operators of coef_restated, cap_restated and robin_restated form harmonic faces"""
    assert mean in ("harmonic", "arithmetic"), mean
    old = CO._faces
    if mean == "harmonic":
        CO._faces = faces
    try:
        yield
    finally:
        CO._faces = old


def relax(n3, rng, v, f, a, s, ncycles, dtype, c=None, bc=0, beta=ZERO, mean="harmonic"):
    """ncycles red-black sweeps over the unknowns"""
    with harmonic(mean):
        return RB.relax(n3, rng, v, f, a, c, s, ncycles, bc, beta, dtype)


def relax_from_zero(n3, rng, f, a, s, ncycles, dtype, c=None, mean="harmonic"):
    """the sweeps from v = 0 (interior entries; no mask)"""
    return relax(n3, rng, np.zeros(O.shape(n3), dtype), f, a, s, ncycles, dtype, c, mean=mean)


def residual(n3, rng, v, f, a, s, dtype, c=None, bc=0, beta=ZERO, mean="harmonic"):
    """r at the unknowns, 0 at the Dirichlet points"""
    with harmonic(mean):
        return RB.residual(n3, rng, v, f, a, c, s, bc, beta, dtype)


def apply_A(n3, rng, p, a, s, dtype, c=None, bc=0, beta=ZERO, mean="harmonic"):
    """q = A p = -(residual with f = 0) at the unknowns"""
    with harmonic(mean):
        return RB.apply_A(n3, rng, p, a, c, s, bc, beta, dtype)


class Hierarchy(RB.Hierarchy):
    """robin_restated.Hierarchy (v, f, a, c of every level, the walls) with the hierarchy's mean, and -- without a mask -- on full or
    semi-coarsened levels with coef_restated.Hierarchy's cycles, as cap_restated.Hierarchy picks them; a goes down the levels as it
    always did"""

    def __init__(self, n3, rng, a, s, c=None, bc=0, beta=ZERO, g=ZERO, dtype=np.float64, coarsening="full", mean="harmonic"):
        assert not (bc and coarsening == "semi")
        RB.Hierarchy.__init__(self, n3, rng, a, c, s, bc, beta, g, dtype)
        self.mean = mean
        if coarsening == "semi":
            self.sizes, self.masks = S.plan(n3, rng)
            self.v = [np.zeros(O.shape(n), dtype) for n in self.sizes]
            self.f = [np.zeros(O.shape(n), dtype) for n in self.sizes]
            self.a = CO.coarse_coefficients(self.sizes, self.masks, a, dtype)
            self.c = CA.coarse_capacities(self.sizes, self.masks, c, dtype) if c is not None else [None] * len(self.sizes)

    def relax(self, l, k):
        with harmonic(self.mean):
            RB.Hierarchy.relax(self, l, k)

    def residual(self, l):
        with harmonic(self.mean):
            return RB.Hierarchy.residual(self, l)

    def vcycle(self, l, v1, v2):
        (NR.Hierarchy.vcycle if self.bc else CO.Hierarchy.vcycle)(self, l, v1, v2)

    def fmg(self, l, v0, v1, v2):
        (NR.Hierarchy.fmg if self.bc else CO.Hierarchy.fmg)(self, l, v0, v1, v2)


def m_cycle(n3, rng, a, s, v1, v2, c=None, bc=0, beta=ZERO, dtype=np.float64, coarsening="full", mean="harmonic"):
    """the preconditioner of PCG: the V(v1, v2) cycle from zero on all points"""
    H = Hierarchy(n3, rng, a, s, c, bc, beta, ZERO, dtype, coarsening, mean)

    def M(r):
        for l in range(len(H.sizes)):
            H.v[l] = np.zeros(O.shape(H.sizes[l]), dtype)
        H.f[0] = np.ascontiguousarray(r, dtype)
        H.vcycle(0, v1, v2)
        return H.v[0].copy()
    return M


def fcg(n3, rng, a, s, v0, f, c=None, bc=0, beta=ZERO, tol=1e-10, maxit=60, v1=2, v2=2, dtype=np.float64, coarsening="full", mean="harmonic"):
    """PCG(v1, v2, tol, maxit, krylov = 1 or 2): the iteration of cap_restated.fcg / robin_restated._wfcg (without a mask every weight
    is 1) with this module's operator: (x, iterations, history, converged, true relative residual)"""
    dtype = np.dtype(dtype).type
    unk = NR.unknown_mask(n3, bc)
    W = NR.weights(n3, bc)
    M = m_cycle(n3, rng, a, s, v1, v2, c, bc, beta, dtype, coarsening, mean)
    f = np.ascontiguousarray(f, dtype)

    def res(x):
        return residual(n3, rng, x, f, a, s, dtype, c, bc, beta, mean)

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
        q = apply_A(n3, rng, p, a, s, dtype, c, bc, beta, mean)
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


# ---- the layered slab (test_hmean_cpu.py, test_gpu_hmean.py): two materials stacked in z, the interface midway between the node
# planes K and K + 1 -- what a node-valued (voxel) material means.  With u = 0 at z = zlo and u = 1 at z = zhi and no source the flux
# q is the same in both layers (series resistance) and u is piecewise linear in z with its kink at the interface:
#   below: u = q (z - zlo) / a1,   above: u = 1 - q (zhi - z) / a2,   q = 1 / (L1 / a1 + L2 / a2)
SLAB_N3, SLAB_K, SLAB_RNG = (9, 9, 17), 8, [0.0, 1.0, 0.0, 1.0, 0.0, 2.0]


def slab(jump, dtype=np.float64, n3=SLAB_N3, K=SLAB_K, rng=SLAB_RNG, a1=1.0):
    """(a, u, q): the coefficient (a1 for k <= K, a1 * jump above), the analytic nodal values (the Dirichlet data among them) and the
    flux, all computed in double and rounded once to `dtype`"""
    sx, sy, sz = n3
    zlo, zhi = float(rng[4]), float(rng[5])
    h = (zhi - zlo) / (sz - 1)
    z = zlo + h * np.arange(sz)
    zi = zlo + h * (K + 0.5)
    a2 = a1 * float(jump)
    q = 1.0 / ((zi - zlo) / a1 + (zhi - zi) / a2)
    uz = np.where(np.arange(sz) <= K, q * (z - zlo) / a1, 1.0 - q * (zhi - z) / a2)
    az = np.where(np.arange(sz) <= K, a1, a2)
    shape = (sz, sy, sx)
    a = np.broadcast_to(az[:, None, None], shape).astype(dtype)
    u = np.broadcast_to(uz[:, None, None], shape).astype(dtype)
    return a, u, q
