"""The shifted operator (Laplacian - s) u = f restated (a plain module, imported by test_shift_cpu.py and test_gpu_shift.py): the
arithmetic of csrc/mgx_shift3d.hip in numpy, colour by colour and in `dtype`, with the same association; the cycles of
mg_multigrid3d.inc built from it, from the oracle's restrict3d / interpolate3d / correct3d / set3d and from semi_restated's
transfers; and flexible CG with the shifted operator.  Arrays are in the reference layout, shape (sz, sy, sx)."""
import math

import numpy as np

import oracle as O
import semi_restated as S


def squares(n3, rng, dtype):
    """hx2, hy2, hz2 as Grid3D forms the spacings (range / (real)(size - 1) in `dtype`) and Relax squares them"""
    t = np.dtype(dtype).type
    h = [t(t(rng[2 * d + 1]) - t(rng[2 * d])) / t(int(n3[d]) - 1) for d in range(3)]
    return [t(x * x) for x in h]


def _nb(v):
    """O, E (x -/+ 1), N, S (y -/+ 1), D, U (z -/+ 1) and the centre of every interior point"""
    return (v[1:-1, 1:-1, :-2], v[1:-1, 1:-1, 2:], v[1:-1, :-2, 1:-1], v[1:-1, 2:, 1:-1], v[:-2, 1:-1, 1:-1], v[2:, 1:-1, 1:-1],
            v[1:-1, 1:-1, 1:-1])


def colour_mask(n3, colour):
    z, y, x = np.meshgrid(*(np.arange(1, k - 1) for k in n3[::-1]), indexing="ij")
    return (x + y + z) % 2 == colour


def relax(n3, rng, v, f, s, ncycles, dtype):
    """ncycles red-black sweeps: v = num / den with relax3d_point's numerator and den = 2*(hy2*hz2 + hx2*hz2 + hx2*hy2) + s*hx2*hy2*hz2"""
    t = np.dtype(dtype).type
    hx2, hy2, hz2 = squares(n3, rng, dtype)
    den = t(2) * (hy2 * hz2 + hx2 * hz2 + hx2 * hy2) + t(s) * hx2 * hy2 * hz2
    v = np.array(v, dtype=dtype, order="C", copy=True)
    fi = np.ascontiguousarray(f, dtype)[1:-1, 1:-1, 1:-1]
    masks = [colour_mask(n3, c) for c in (0, 1)]
    for _ in range(ncycles):
        for colour in (0, 1):
            o, e, n, so, d, u, c = _nb(v)
            num = o * (hy2 * hz2) + e * (hy2 * hz2) + n * (hx2 * hz2) + so * (hx2 * hz2) + d * (hx2 * hy2) + u * (hx2 * hy2) - fi * hx2 * hy2 * hz2
            new = num / den
            c[masks[colour]] = new[masks[colour]]
    return v


def residual(n3, rng, v, f, s, dtype):
    """r = residual3d_point<real, 1>(...) + s*c on the interior, 0 on the boundary"""
    t = np.dtype(dtype).type
    hx2, hy2, hz2 = squares(n3, rng, dtype)
    v = np.ascontiguousarray(v, dtype)
    fi = np.ascontiguousarray(f, dtype)[1:-1, 1:-1, 1:-1]
    o, e, n, so, d, u, c = _nb(v)
    r = np.zeros(O.shape(n3), dtype)
    r[1:-1, 1:-1, 1:-1] = (fi - ((o - t(2) * c + e) / hx2) - ((n - t(2) * c + so) / hy2) - ((d - t(2) * c + u) / hz2)) + t(s) * c
    return r


def apply_A(n3, rng, p, s, dtype):
    """q = A p = -(residual with f = 0) = Laplacian p - s p"""
    return -residual(n3, rng, p, np.zeros(O.shape(n3), dtype), s, dtype)


def restrict_residual(n3, r, mask, dtype):
    """Restrict over the axes of mask in 1 .. 7 of a residual (0 on the boundary, so the injected coarse boundary is 0)"""
    return O.restrict3d(n3, r, dtype=dtype) if mask == 7 else S.restrict_axes(r, mask)


def rhs(u, q, qscale, s, dtype):
    """f = (-(s*u)) - qscale*q on the interior, 0 elsewhere (the library leaves the boundary of f alone)"""
    t = np.dtype(dtype).type
    out = np.zeros(u.shape, dtype)
    val = -(t(s) * np.ascontiguousarray(u, dtype)[1:-1, 1:-1, 1:-1])
    if q is not None:
        val = val - t(qscale) * np.ascontiguousarray(q, dtype)[1:-1, 1:-1, 1:-1]
    out[1:-1, 1:-1, 1:-1] = val
    return out


def full_plan(n3):
    """sizes and masks of mgMultiGrid3D_create: floor(log2(min - 1)) levels, every step halves all axes"""
    sizes = [tuple(int(k) for k in n3)]
    while len(sizes) < int(math.log2(min(n3) - 1)):
        sizes.append(S.coarse_size(sizes[-1], 7))
    return sizes, (7,) * (len(sizes) - 1) + (0,)


class Hierarchy:
    """v and f of every level and the cycles of mg_multigrid3d.inc with the shifted smoother and residual"""

    def __init__(self, n3, rng, s, dtype=np.float64, coarsening="full"):
        self.rng, self.s, self.dtype = list(rng), s, dtype
        self.sizes, self.masks = S.plan(n3, rng) if coarsening == "semi" else full_plan(n3)
        self.v = [np.zeros(O.shape(n), dtype) for n in self.sizes]
        self.f = [np.zeros(O.shape(n), dtype) for n in self.sizes]

    def relax(self, l, k):
        self.v[l] = relax(self.sizes[l], self.rng, self.v[l], self.f[l], self.s, k, self.dtype)

    def residual(self, l):
        return residual(self.sizes[l], self.rng, self.v[l], self.f[l], self.s, self.dtype)

    def vcycle(self, l, v1, v2):
        n, dt = self.sizes[l], self.dtype
        self.relax(l, v1)
        if l != len(self.sizes) - 1:
            m = self.masks[l]
            self.f[l + 1] = restrict_residual(n, self.residual(l), m, dt)
            self.v[l + 1] = O.set3d(self.sizes[l + 1], self.v[l + 1], 0, True, dtype=dt)
            self.vcycle(l + 1, v1, v2)
            if m == 7:
                e = O.interpolate3d(n, np.zeros_like(self.v[l]), self.v[l + 1], dtype=dt)
                self.v[l] = O.correct3d(n, self.v[l], e, dtype=dt)
            else:
                self.v[l] = S.interpolate_correct_axes(self.v[l], self.v[l + 1], m)
        self.relax(l, v2)

    def fmg(self, l, v0, v1, v2):
        n, dt = self.sizes[l], self.dtype
        if l != len(self.sizes) - 1:
            m = self.masks[l]
            self.f[l + 1] = O.restrict3d(n, self.f[l], dtype=dt) if m == 7 else S.restrict_axes(self.f[l], m)
            self.fmg(l + 1, v0, v1, v2)
            self.v[l] = O.interpolate3d(n, self.v[l], self.v[l + 1], dtype=dt) if m == 7 else S.interpolate_axes(self.v[l], self.v[l + 1], m)
        else:
            self.v[l] = O.set3d(n, self.v[l], 0, False, dtype=dt)
        for _ in range(v0):
            self.vcycle(l, v1, v2)


def fsum_sq(r):
    return math.fsum((np.asarray(r, np.float64) ** 2).ravel())


def m_cycle(n3, rng, s, v1, v2, dtype=np.float64, coarsening="full"):
    """the preconditioner of PCG: the shifted V-cycle from zero"""
    def M(r):
        H = Hierarchy(n3, rng, s, dtype, coarsening)
        H.f[0] = np.ascontiguousarray(r, dtype)
        H.vcycle(0, v1, v2)
        return H.v[0]
    return M


def cycles_to(n3, rng, s, v0, f, v1, v2, tol, maxit, dtype=np.float64):
    """plain cycling from the guess v0 (PCG with krylov = 0): (x, cycles, true relative residual, converged)"""
    H = Hierarchy(n3, rng, s, dtype)
    H.v[0], H.f[0] = np.array(v0, dtype), np.ascontiguousarray(f, dtype)
    rr0 = fsum_sq(H.residual(0))
    k, rel = 0, 0.0
    if rr0 == 0.0:
        return H.v[0], 0, 0.0, True
    for k in range(1, maxit + 1):
        H.vcycle(0, v1, v2)
        rel = math.sqrt(fsum_sq(H.residual(0)) / rr0)
        if rel < tol:
            return H.v[0], k, rel, True
    return H.v[0], k, rel, False


def fcg_restated(n3, rng, s, v0, f, M, tol, maxit, dtype=np.float64):
    """solve_restated.fcg_restated with the shifted operator and residual: (x, iterations, history, converged)"""
    def dot(a, b):
        return math.fsum((a.astype(np.float64) * b.astype(np.float64)).ravel())

    x = np.array(v0, dtype)
    r = residual(n3, rng, x, f, s, dtype)
    rr0 = dot(r, r)
    hist, k, restart, conv = [], 0, True, False
    while k < maxit:
        if restart:
            z = M(r)
            p, rz, restart = z.copy(), dot(r, z), False
        k += 1
        q = apply_A(n3, rng, p, s, dtype)
        alpha = rz / dot(p, q)
        x = x + dtype(alpha) * p
        r = r - dtype(alpha) * q
        rel = math.sqrt(dot(r, r) / rr0)
        hist.append(rel)
        if rel < tol:
            r = residual(n3, rng, x, f, s, dtype)
            if math.sqrt(dot(r, r) / rr0) < tol:
                conv = True
                break
            restart = True
            continue
        z = M(r)
        beta = -alpha * dot(z, q) / rz
        rz = dot(r, z)
        p = z + dtype(beta) * p
    return x, k, np.array(hist), conv
