"""The variable-coefficient operator div(a grad u) - s u = f restated (a plain module, imported by test_coef_cpu.py and
test_gpu_coef.py): the arithmetic of csrc/mgx_coef3d.hip in numpy, colour by colour and in `dtype`, with the same association; the
coefficient's restriction chain; the cycles of mg_multigrid3d.inc built from them, from the oracle's restrict3d / interpolate3d /
correct3d / set3d and from semi_restated's transfers; and flexible CG with this operator.  Arrays are in the reference layout,
shape (sz, sy, sx); `a` holds all points, the boundary included."""
import math

import numpy as np

import oracle as O
import semi_restated as S
from shift_restated import _nb, colour_mask, fsum_sq, full_plan, squares


def scales(n3, rng, dtype):
    """qx, qy, qz = (real)0.5 / hx2 .. as the host forms them once per call"""
    t = np.dtype(dtype).type
    return [t(t(0.5) / h2) for h2 in squares(n3, rng, dtype)]


def _faces(a):
    """AW, AE, AN, AS, AD, AU of every interior point"""
    o, e, n, so, d, u, c = _nb(a)
    return o + c, e + c, n + c, so + c, d + c, u + c


def relax(n3, rng, v, f, a, s, ncycles, dtype):
    """ncycles red-black sweeps: v = num / den,
    den = ((qx*(AW + AE) + qy*(AN + AS)) + qz*(AD + AU)) + s, num = ((qx*(AW*O + AE*E) + qy*(AN*N + AS*S)) + qz*(AD*D + AU*U)) - f"""
    t = np.dtype(dtype).type
    qx, qy, qz = scales(n3, rng, dtype)
    v = np.array(v, dtype=dtype, order="C", copy=True)
    fi = np.ascontiguousarray(f, dtype)[1:-1, 1:-1, 1:-1]
    AW, AE, AN, AS, AD, AU = _faces(np.ascontiguousarray(a, dtype))
    den = ((qx * (AW + AE) + qy * (AN + AS)) + qz * (AD + AU)) + t(s)
    masks = [colour_mask(n3, c) for c in (0, 1)]
    for _ in range(ncycles):
        for colour in (0, 1):
            o, e, n, so, d, u, c = _nb(v)
            num = ((qx * (AW * o + AE * e) + qy * (AN * n + AS * so)) + qz * (AD * d + AU * u)) - fi
            new = num / den
            c[masks[colour]] = new[masks[colour]]
    return v


def residual(n3, rng, v, f, a, s, dtype):
    """r = (((f - tx) - ty) - tz) + s*c on the interior, 0 on the boundary"""
    t = np.dtype(dtype).type
    qx, qy, qz = scales(n3, rng, dtype)
    v = np.ascontiguousarray(v, dtype)
    fi = np.ascontiguousarray(f, dtype)[1:-1, 1:-1, 1:-1]
    AW, AE, AN, AS, AD, AU = _faces(np.ascontiguousarray(a, dtype))
    o, e, n, so, d, u, c = _nb(v)
    tx = qx * (AW * (o - c) + AE * (e - c))
    ty = qy * (AN * (n - c) + AS * (so - c))
    tz = qz * (AD * (d - c) + AU * (u - c))
    r = np.zeros(O.shape(n3), dtype)
    r[1:-1, 1:-1, 1:-1] = (((fi - tx) - ty) - tz) + t(s) * c
    return r


def apply_A(n3, rng, p, a, s, dtype):
    """q = A p = -(residual with f = 0) = div(a grad p) - s p"""
    return -residual(n3, rng, p, np.zeros(O.shape(n3), dtype), a, s, dtype)


def restrict(n3, fine, mask, dtype):
    """the library's restriction over the axes of mask in 1 .. 7: full weighting inside, injection on the boundary"""
    return O.restrict3d(n3, fine, dtype=dtype) if mask == 7 else S.restrict_axes(fine, mask)


def coarse_coefficients(sizes, masks, a, dtype):
    """a on every level: a_{l+1} = Restrict(a_l) by the step's mask"""
    out = [np.ascontiguousarray(a, dtype)]
    for l in range(len(sizes) - 1):
        out.append(np.ascontiguousarray(restrict(sizes[l], out[-1], masks[l], dtype), dtype))
    return out


class Hierarchy:
    """v, f and a of every level and the cycles of mg_multigrid3d.inc with the variable-coefficient smoother and residual"""

    def __init__(self, n3, rng, a, s, dtype=np.float64, coarsening="full"):
        self.rng, self.s, self.dtype = list(rng), s, dtype
        self.sizes, self.masks = S.plan(n3, rng) if coarsening == "semi" else full_plan(n3)
        self.v = [np.zeros(O.shape(n), dtype) for n in self.sizes]
        self.f = [np.zeros(O.shape(n), dtype) for n in self.sizes]
        self.a = coarse_coefficients(self.sizes, self.masks, a, dtype)

    def relax(self, l, k):
        self.v[l] = relax(self.sizes[l], self.rng, self.v[l], self.f[l], self.a[l], self.s, k, self.dtype)

    def residual(self, l):
        return residual(self.sizes[l], self.rng, self.v[l], self.f[l], self.a[l], self.s, self.dtype)

    def vcycle(self, l, v1, v2):
        n, dt = self.sizes[l], self.dtype
        self.relax(l, v1)
        if l != len(self.sizes) - 1:
            m = self.masks[l]
            self.f[l + 1] = restrict(n, self.residual(l), m, dt)
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
            self.f[l + 1] = restrict(n, self.f[l], m, dt)
            self.fmg(l + 1, v0, v1, v2)
            self.v[l] = O.interpolate3d(n, self.v[l], self.v[l + 1], dtype=dt) if m == 7 else S.interpolate_axes(self.v[l], self.v[l + 1], m)
        else:
            self.v[l] = O.set3d(n, self.v[l], 0, False, dtype=dt)
        for _ in range(v0):
            self.vcycle(l, v1, v2)


def m_cycle(n3, rng, a, s, v1, v2, dtype=np.float64, coarsening="full"):
    """the preconditioner of PCG: the variable-coefficient V-cycle from zero (the coefficients are restricted once)"""
    H = Hierarchy(n3, rng, a, s, dtype, coarsening)

    def M(r):
        for l in range(len(H.sizes)):
            H.v[l] = np.zeros(O.shape(H.sizes[l]), dtype)
        H.f[0] = np.ascontiguousarray(r, dtype)
        H.vcycle(0, v1, v2)
        return H.v[0].copy()
    return M


def cycles_to(n3, rng, a, s, v0, f, v1, v2, tol, maxit, dtype=np.float64):
    """plain cycling from the guess v0 (PCG with krylov = 0): (x, cycles, true relative residual, converged)"""
    H = Hierarchy(n3, rng, a, s, dtype)
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


def fcg_restated(n3, rng, a, s, v0, f, M, tol, maxit, dtype=np.float64):
    """shift_restated.fcg_restated with this operator and residual: (x, iterations, history, converged)"""
    def dot(x, y):
        return math.fsum((x.astype(np.float64) * y.astype(np.float64)).ravel())

    x = np.array(v0, dtype)
    r = residual(n3, rng, x, f, a, s, dtype)
    rr0 = dot(r, r)
    hist, k, restart, conv = [], 0, True, False
    while k < maxit:
        if restart:
            z = M(r)
            p, rz, restart = z.copy(), dot(r, z), False
        k += 1
        q = apply_A(n3, rng, p, a, s, dtype)
        alpha = rz / dot(p, q)
        x = x + dtype(alpha) * p
        r = r - dtype(alpha) * q
        rel = math.sqrt(dot(r, r) / rr0)
        hist.append(rel)
        if rel < tol:
            r = residual(n3, rng, x, f, a, s, dtype)
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


# ---- the coefficients of the issue's table, on the nodes of the unit cube
def _nodes(n3):
    z, y, x = np.meshgrid(*(np.linspace(0.0, 1.0, k) for k in n3[::-1]), indexing="ij")
    return x, y, z


def smooth_coefficient(n3, dtype=np.float64):
    """1 + 0.5 sin(2 pi x) cos(pi y) + 0.25 z"""
    x, y, z = _nodes(n3)
    return (1.0 + 0.5 * np.sin(2 * np.pi * x) * np.cos(np.pi * y) + 0.25 * z).astype(dtype)


def jump_coefficient(n3, jump, dtype=np.float64):
    """`jump` in the cube |x-.5|, |y-.5|, |z-.5| < .25, 1 outside"""
    x, y, z = _nodes(n3)
    inside = (np.abs(x - 0.5) < 0.25) & (np.abs(y - 0.5) < 0.25) & (np.abs(z - 0.5) < 0.25)
    return np.where(inside, float(jump), 1.0).astype(dtype)
