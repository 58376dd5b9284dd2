"""Homogeneous Neumann faces restated (a plain module, imported by test_neumann_cpu.py and test_gpu_neumann.py): what
csrc/mgx_rim3d.hip adds to the shifted and the variable-coefficient operator, in numpy, colour by colour and in `dtype`, with the
associations of shift_restated / coef_restated and the oracle's transfers; the cycles of mg_multigrid3d.inc on a hierarchy with a
face mask; plain cycling to a tolerance and backward Euler steps built on it.

bc is the mask of mgx.h: bit 0 x-low, 1 x-high, 2 y-low, 3 y-high, 4 z-low, 5 z-high; a set bit makes that face homogeneous
Neumann.  A point is an unknown when it is interior, or lies on one or more Neumann faces and on no Dirichlet face.  At an unknown
on a face every operator is the interior's expression on a star whose out-of-range entry is the opposite one -- numpy's "reflect"
padding, for v and for a -- so every function here pads, evaluates the interior expression of the padded array (which is then
every point of the grid) and keeps the values at the unknowns.  a = None means the shifted operator.  Arrays are in the reference
layout, shape (sz, sy, sx)."""
import math

import numpy as np

import coef_restated as CO
import oracle as O
from shift_restated import _nb, fsum_sq, full_plan, squares


def on_faces(n3):
    """the bits of the faces every point lies on (0 in the interior)"""
    sx, sy, sz = (int(k) for k in n3)
    z, y, x = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    return ((x == 0) * 1 | (x == sx - 1) * 2 | (y == 0) * 4 | (y == sy - 1) * 8 | (z == 0) * 16 | (z == sz - 1) * 32).astype(np.int64)


def unknown_mask(n3, bc):
    """True at the unknowns: the interior, and the points on Neumann faces that lie on no Dirichlet face"""
    return (on_faces(n3) & ~int(bc)) == 0


def face_unknowns(n3, bc):
    """the unknowns that lie on a face"""
    on = on_faces(n3)
    return (on != 0) & ((on & ~int(bc)) == 0)


def weights(n3, bc):
    """1/2 per Neumann face an unknown lies on (the trapezoid weights), 0 at the Dirichlet points"""
    on = on_faces(n3)
    count = sum((on >> k) & 1 for k in range(6))
    return np.where(unknown_mask(n3, bc), 0.5 ** count, 0.0)


def colours(n3):
    sx, sy, sz = (int(k) for k in n3)
    z, y, x = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    return (x + y + z) % 2


def mirror(v, k=1):
    """k reflected layers around v: entry -1 is entry 1, entry n is entry n - 2 (with three points both are the middle one)"""
    return np.pad(v, k, mode="reflect")


def relax(n3, rng, v, f, a, s, ncycles, bc, dtype):
    """ncycles red-black sweeps over the unknowns with shift_restated.relax's (a None) or coef_restated.relax's point expression"""
    t = np.dtype(dtype).type
    v = np.array(v, dtype=dtype, order="C", copy=True)
    fi = np.ascontiguousarray(f, dtype)
    unk, col = unknown_mask(n3, bc), colours(n3)
    if a is None:
        hx2, hy2, hz2 = squares(n3, rng, dtype)
        den = t(2) * (hy2 * hz2 + hx2 * hz2 + hx2 * hy2) + t(s) * hx2 * hy2 * hz2
    else:
        qx, qy, qz = CO.scales(n3, rng, dtype)
        AW, AE, AN, AS, AD, AU = CO._faces(mirror(np.ascontiguousarray(a, dtype)))
        den = ((qx * (AW + AE) + qy * (AN + AS)) + qz * (AD + AU)) + t(s)
    for _ in range(ncycles):
        for colour in (0, 1):
            o, e, n, so, d, u, _c = _nb(mirror(v))
            if a is None:
                num = o * (hy2 * hz2) + e * (hy2 * hz2) + n * (hx2 * hz2) + so * (hx2 * hz2) + d * (hx2 * hy2) + u * (hx2 * hy2) - fi * hx2 * hy2 * hz2
            else:
                num = ((qx * (AW * o + AE * e) + qy * (AN * n + AS * so)) + qz * (AD * d + AU * u)) - fi
            new = num / den
            m = unk & (col == colour)
            v[m] = new[m]
    return v


def residual(n3, rng, v, f, a, s, bc, dtype):
    """r at the unknowns, 0 at the Dirichlet points"""
    t = np.dtype(dtype).type
    fi = np.ascontiguousarray(f, dtype)
    o, e, n, so, d, u, c = _nb(mirror(np.ascontiguousarray(v, dtype)))
    if a is None:
        hx2, hy2, hz2 = squares(n3, rng, dtype)
        full = (fi - ((o - t(2) * c + e) / hx2) - ((n - t(2) * c + so) / hy2) - ((d - t(2) * c + u) / hz2)) + t(s) * c
    else:
        qx, qy, qz = CO.scales(n3, rng, dtype)
        AW, AE, AN, AS, AD, AU = CO._faces(mirror(np.ascontiguousarray(a, dtype)))
        tx = qx * (AW * (o - c) + AE * (e - c))
        ty = qy * (AN * (n - c) + AS * (so - c))
        tz = qz * (AD * (d - c) + AU * (u - c))
        full = (((fi - tx) - ty) - tz) + t(s) * c
    r = np.zeros(O.shape(n3), dtype)
    unk = unknown_mask(n3, bc)
    r[unk] = full[unk]
    return r


def apply_A(n3, rng, p, a, s, bc, dtype):
    """q = A p = -(residual with f = 0) at the unknowns"""
    return -residual(n3, rng, p, np.zeros(O.shape(n3), dtype), a, s, bc, dtype)


def restrict(n3, fine, bc, dtype):
    """the oracle's restriction; a coarse unknown on a face is its full weighting of the 27 reflected fine values"""
    coarse = O.restrict3d(n3, fine, dtype=dtype)
    if bc:
        padded = tuple(int(k) + 4 for k in n3)  # two layers: the fine point 2c is the padded point 2 (c + 1)
        fw = O.restrict3d(padded, np.ascontiguousarray(mirror(np.ascontiguousarray(fine, dtype), 2)), dtype=dtype)[1:-1, 1:-1, 1:-1]
        m = face_unknowns(O.csize(n3), bc)
        coarse[m] = fw[m]
    return coarse


def interpolate(n3, fine, coarse, bc, dtype, add=False):
    """the oracle's interpolation (add: and correction) on the interior, and its formula at the fine face unknowns"""
    fine, coarse = np.ascontiguousarray(fine, dtype), np.ascontiguousarray(coarse, dtype)
    if add:
        out = O.correct3d(n3, fine.copy(), O.interpolate3d(n3, np.zeros_like(fine), coarse, dtype=dtype), dtype=dtype)
    else:
        out = O.interpolate3d(n3, fine.copy(), coarse, dtype=dtype)
    if bc:
        padded = tuple(int(k) + 4 for k in n3)  # the coarse point c is the padded coarse point c + 1
        full = O.interpolate3d(padded, np.zeros(O.shape(padded), dtype), np.ascontiguousarray(mirror(coarse, 1)), dtype=dtype)[2:-2, 2:-2, 2:-2]
        m = face_unknowns(n3, bc)
        out[m] = (fine[m] + full[m]) if add else full[m]
    return out


def rhs(u, q, qscale, s, bc, dtype, f=None):
    """f = (-(s*u)) - qscale*q at the unknowns; the other entries are those of `f` (default zeros)"""
    t = np.dtype(dtype).type
    u = np.ascontiguousarray(u, dtype)
    out = np.zeros(u.shape, dtype) if f is None else np.array(f, dtype)
    val = -(t(s) * u)
    if q is not None:
        val = val - t(qscale) * np.ascontiguousarray(q, dtype)
    m = unknown_mask(tuple(reversed(u.shape)), bc)
    out[m] = val[m]
    return out


class Hierarchy:
    """v, f (and a) of every level and the cycles of mg_multigrid3d.inc on a hierarchy with the face mask bc: the stored residual,
    restricted; the coarse levels from zero on all points; interpolate + correct; a coefficient's own restriction chain unchanged"""

    def __init__(self, n3, rng, a, s, bc, dtype=np.float64):
        self.rng, self.s, self.bc, self.dtype = list(rng), s, int(bc), dtype
        self.sizes, masks = full_plan(n3)
        self.v = [np.zeros(O.shape(n), dtype) for n in self.sizes]
        self.f = [np.zeros(O.shape(n), dtype) for n in self.sizes]
        self.a = CO.coarse_coefficients(self.sizes, masks, a, dtype) if a is not None else [None] * len(self.sizes)

    def relax(self, l, k):
        self.v[l] = relax(self.sizes[l], self.rng, self.v[l], self.f[l], self.a[l], self.s, k, self.bc, self.dtype)

    def residual(self, l):
        return residual(self.sizes[l], self.rng, self.v[l], self.f[l], self.a[l], self.s, self.bc, self.dtype)

    def vcycle(self, l, v1, v2):
        n, dt = self.sizes[l], self.dtype
        self.relax(l, v1)
        if l != len(self.sizes) - 1:
            self.f[l + 1] = restrict(n, self.residual(l), self.bc, dt)
            self.v[l + 1] = np.zeros(O.shape(self.sizes[l + 1]), dt)
            self.vcycle(l + 1, v1, v2)
            self.v[l] = interpolate(n, self.v[l], self.v[l + 1], self.bc, dt, add=True)
        self.relax(l, v2)

    def fmg(self, l, v0, v1, v2):
        n, dt = self.sizes[l], self.dtype
        if l != len(self.sizes) - 1:
            self.f[l + 1] = restrict(n, self.f[l], self.bc, dt)
            self.fmg(l + 1, v0, v1, v2)
            self.v[l] = interpolate(n, self.v[l], self.v[l + 1], self.bc, dt)
        else:
            self.v[l] = O.set3d(n, self.v[l], 0, False, dtype=dt)
            self.v[l][face_unknowns(n, self.bc)] = 0
        for _ in range(v0):
            self.vcycle(l, v1, v2)

    def cycle_to(self, v1, v2, tol, maxit):
        """plain cycling of level 0 (PCG with krylov = 0): (cycles, true relative residual, converged); the sums run over all
        unknowns, unweighted"""
        rr0 = fsum_sq(self.residual(0))
        k, rel = 0, 0.0
        if rr0 == 0.0:
            return 0, 0.0, True
        for k in range(1, maxit + 1):
            self.vcycle(0, v1, v2)
            rel = math.sqrt(fsum_sq(self.residual(0)) / rr0)
            if rel < tol:
                return k, rel, True
        return k, rel, False

    def backward_euler(self, nsteps, dt, kappa, v1, v2, tol, maxit, source=None):
        """mgMultiGrid3D_<r>_BackwardEuler(krylov = 0): (cycles of all steps, worst relative residual, converged)"""
        t = np.dtype(self.dtype).type
        self.s = t(1.0 / (kappa * dt))
        total, worst = 0, 0.0
        for _ in range(nsteps):
            self.f[0] = rhs(self.v[0], source, t(1.0 / kappa), self.s, self.bc, self.dtype, f=self.f[0])
            k, rel, conv = self.cycle_to(v1, v2, tol, maxit)
            total, worst = total + k, max(worst, rel)
            if not conv:
                return total, worst, False
        return total, worst, True


# ---- the cases the CPU and the GPU tests share
# (bc, s, smooth coefficient?): the V(2,2) convergence cases, also those of the plain-cycling counts
VCYCLE_CASES = [(1, 0.0, False), (3, 0.0, False), (37, 0.0, True), (63, 100.0, False), (63, 100.0, True)]


def vcycle_case(bc, s, coef, seed=11):
    n3 = (33, 33, 33)
    g = np.random.default_rng(seed)
    H = Hierarchy(n3, [0, 1, 0, 1, 0, 1], CO.smooth_coefficient(n3) if coef else None, s, bc)
    H.v[0], H.f[0] = g.uniform(-1, 1, O.shape(n3)), g.uniform(-1, 1, O.shape(n3))
    return H


def gaussian(n3):
    x, y, z = CO._nodes(n3)
    return np.exp(-40 * ((x - 0.4) ** 2 + (y - 0.55) ** 2 + (z - 0.3) ** 2))
