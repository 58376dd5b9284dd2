"""The 3D operators restated, once (a plain module, imported by the *_cpu.py tests and their test_gpu_* twins): the arithmetic of
csrc/mgx_shift3d.hip, mgx_coef3d.hip, mgx_cap3d.hip, mgx_rim3d.hip, mgx_wall3d.hip and mgx_hmean3d.hip in numpy, colour by colour
and in `dtype`, with the kernels' associations; the cycles of mg_multigrid3d.inc built from it, from the oracle's restrict3d /
interpolate3d / correct3d / set3d and from semi_restated's transfers; plain cycling, flexible CG and backward Euler steps.

An operator is an `Op` value:  div(a grad u) - s c u = f  with faces of a as `mean` forms them, on the unknowns of the mask bc, with
the wall law  a du/dn + beta u = g  on the flagged faces.  a = None is the shifted Laplacian in the squared-spacings form, c = None
no capacity, bc = 0 Dirichlet faces all round, beta = ZERO insulated walls: the absent options cost no rounding, so every simpler
operator's bits are this one's.

bc is the mask of mgx.h: bit 0 x-low, 1 x-high, 2 y-low, 3 y-high, 4 z-low, 5 z-high; beta and g are in the order of its bits.  A
point is an unknown when it is interior, or lies on one or more flagged faces and on no Dirichlet face.  At an unknown on a face
every expression is the interior's on a star whose out-of-range entry is the opposite one -- numpy's "reflect" padding, for v and
for a -- so every function pads, evaluates the interior expression of the padded array (which is then every point of the grid) and
keeps the values at the unknowns.  A wall adds 2 (g - beta u_P) / h per wall face to the half cell of a face unknown:
  d_k  = (t(2) * t(beta_k)) / h_axis(k)           once per level, in `dtype`, from that level's own spacing
  d(P) = ((dx + dy) + dz)                          the d_k of the faces P lies on, 0 for an axis on whose faces P does not lie
  se   = base + d(P) where d(P) != 0, else base    base = t(s), with a capacity t(s) * c_P (only the updated point's c enters)
and g touches the right-hand side of level 0 only.  Arrays are in the reference layout, shape (sz, sy, sx); a and c hold all points."""
import dataclasses
import functools
import math

import numpy as np

import oracle as O
import semi_restated as S

ZERO = (0.0,) * 6


# ------------------------------------------------------------------------------------------ geometry
def on_faces(n3):
    """the bits of the faces every point lies on (0 in the interior)"""
    sx, sy, sz = (int(k) for k in n3)
    z, y, x = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    return ((x == 0) * 1 | (x == sx - 1) * 2 | (y == 0) * 4 | (y == sy - 1) * 8 | (z == 0) * 16 | (z == sz - 1) * 32).astype(np.int64)


def unknown_mask(n3, bc):
    """True at the unknowns: the interior, and the points on flagged faces that lie on no Dirichlet face"""
    return (on_faces(n3) & ~int(bc)) == 0


def face_unknowns(n3, bc):
    """the unknowns that lie on a face"""
    on = on_faces(n3)
    return (on != 0) & ((on & ~int(bc)) == 0)


def weights(n3, bc):
    """1/2 per flagged face an unknown lies on (the trapezoid weights), 0 at the Dirichlet points"""
    on = on_faces(n3)
    count = sum((on >> k) & 1 for k in range(6))
    return np.where(unknown_mask(n3, bc), 0.5 ** count, 0.0)


def sum_weights(n3, bc):
    """sum(W), separable: per axis the interior points plus half a point per flagged end"""
    return math.prod((int(k) - 2) + 0.5 * (((bc >> (2 * d)) & 1) + ((bc >> (2 * d + 1)) & 1)) for d, k in enumerate(n3))


def colours(n3):
    sx, sy, sz = (int(k) for k in n3)
    z, y, x = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    return (x + y + z) % 2


def mirror(v, k=1):
    """k reflected layers around v: entry -1 is entry 1, entry n is entry n - 2 (with three points both are the middle one)"""
    return np.pad(v, k, mode="reflect")


def spacings(n3, rng, dtype):
    """h as Grid3D forms it: range / (real)(size - 1) in `dtype`"""
    t = np.dtype(dtype).type
    return [t(t(rng[2 * d + 1]) - t(rng[2 * d])) / t(int(n3[d]) - 1) for d in range(3)]


def squares(n3, rng, dtype):
    """hx2, hy2, hz2 as Relax squares the spacings"""
    t = np.dtype(dtype).type
    return [t(x * x) for x in spacings(n3, rng, dtype)]


def scales(n3, rng, dtype):
    """qx, qy, qz = (real)0.5 / hx2 .. as the host forms them once per call"""
    t = np.dtype(dtype).type
    return [t(t(0.5) / h2) for h2 in squares(n3, rng, dtype)]


def _nb(v):
    """O, E (x -/+ 1), N, S (y -/+ 1), D, U (z -/+ 1) and the centre of every interior point"""
    return (v[1:-1, 1:-1, :-2], v[1:-1, 1:-1, 2:], v[1:-1, :-2, 1:-1], v[1:-1, 2:, 1:-1], v[:-2, 1:-1, 1:-1], v[2:, 1:-1, 1:-1],
            v[1:-1, 1:-1, 1:-1])


def faces(a, mean):
    """AW, AE, AN, AS, AD, AU of every interior point of `a`, in a's dtype: aO + aC (the mean's factor 1/2 is in scales()), or the
    doubled harmonic mean t(4) * ((aO * aC) / (aO + aC)).  Product and sum commute, so a face has the same bits from both its nodes"""
    assert mean in ("arithmetic", "harmonic"), mean
    o, e, n, so, d, u, c = _nb(a)
    if mean == "arithmetic":
        return tuple(q + c for q in (o, e, n, so, d, u))
    t = a.dtype.type
    return tuple(t(4) * ((q * c) / (q + c)) for q in (o, e, n, so, d, u))


def fsum_sq(r):
    return math.fsum((np.asarray(r, np.float64) ** 2).ravel())


def wdot(W, x, y):
    return math.fsum((W * x.astype(np.float64) * y.astype(np.float64)).ravel())


def wmean(W, x):
    """sum_W(x) / sum(W); sum(W) is exact in double"""
    return math.fsum((W * x.astype(np.float64)).ravel()) / float(W.sum())


def project(W, unk, x, dtype):
    """(x - (dtype)mean_W(x) at the unknowns, the mean)"""
    m = wmean(W, x)
    out = np.array(x, dtype)
    out[unk] = out[unk] - dtype(m)
    return out, m


# ------------------------------------------------------------------------------------------ the operator
@dataclasses.dataclass(frozen=True, eq=False)
class Op:
    """one operator on one grid; what depends on the grid and the fields alone is formed once per value"""
    n3: tuple
    rng: list
    dtype: type
    s: float
    a: np.ndarray = None
    c: np.ndarray = None
    bc: int = 0
    beta: tuple = ZERO
    mean: str = "arithmetic"

    @property
    def t(self):
        return np.dtype(self.dtype).type

    @functools.cached_property
    def unk(self):
        return unknown_mask(self.n3, self.bc)

    @functools.cached_property
    def _colour(self):
        col = colours(self.n3)
        return [self.unk & (col == colour) for colour in (0, 1)]

    def wall_terms(self, val):
        """(t(2) * t(val_k)) / h_axis(k) of the x-, y- and z-face of every point (0 off that axis's faces); a value other than 0 on a
        face the mask does not flag is an error"""
        t = self.t
        h = spacings(self.n3, self.rng, self.dtype)
        assert all(v == 0 or (int(self.bc) >> k) & 1 for k, v in enumerate(val)), (val, self.bc)
        terms = [t((t(2) * t(val[k])) / h[k >> 1]) for k in range(6)]
        sx, sy, sz = (int(k) for k in self.n3)
        z, y, x = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
        return [np.where(i == 0, terms[2 * d], np.where(i == m - 1, terms[2 * d + 1], t(0))).astype(self.dtype)
                for d, (i, m) in enumerate(((x, sx), (y, sy), (z, sz)))]

    def diagonal(self):
        """d(P) at every point"""
        dx, dy, dz = self.wall_terms(self.beta)
        return (dx + dy) + dz

    @functools.cached_property
    def _sc(self):
        """t(s), with a capacity t(s) * c_P: one rounding"""
        return self.t(self.s) if self.c is None else self.t(self.s) * np.ascontiguousarray(self.c, self.dtype)

    @functools.cached_property
    def _se(self):
        """the effective shift of every point"""
        d = self.diagonal()
        return np.where(d != 0, self._sc + d, self._sc).astype(self.dtype)

    @functools.cached_property
    def _stencil(self):
        """(hx2, hy2, hz2) without a coefficient, else (qx, qy, qz) and the six face arrays"""
        if self.a is None:
            return squares(self.n3, self.rng, self.dtype)
        return scales(self.n3, self.rng, self.dtype) + list(faces(mirror(np.ascontiguousarray(self.a, self.dtype)), self.mean))

    @functools.cached_property
    def _den(self):
        """the smoother's denominator at every point"""
        if self.a is None:
            hx2, hy2, hz2 = self._stencil
            return self.t(2) * (hy2 * hz2 + hx2 * hz2 + hx2 * hy2) + self._se * hx2 * hy2 * hz2
        qx, qy, qz, AW, AE, AN, AS, AD, AU = self._stencil
        return ((qx * (AW + AE) + qy * (AN + AS)) + qz * (AD + AU)) + self._se

    def relax(self, v, f, ncycles):
        """ncycles red-black sweeps over the unknowns: v = num / den"""
        v = np.array(v, dtype=self.dtype, order="C", copy=True)
        fi = np.ascontiguousarray(f, self.dtype)
        den = self._den
        if self.a is None:
            hx2, hy2, hz2 = self._stencil
        else:
            qx, qy, qz, AW, AE, AN, AS, AD, AU = self._stencil
        for _ in range(ncycles):
            for m in self._colour:
                o, e, n, so, d, u, _c = _nb(mirror(v))
                if self.a is None:
                    num = o * (hy2 * hz2) + e * (hy2 * hz2) + n * (hx2 * hz2) + so * (hx2 * hz2) + d * (hx2 * hy2) + u * (hx2 * hy2) - fi * hx2 * hy2 * hz2
                else:
                    num = ((qx * (AW * o + AE * e) + qy * (AN * n + AS * so)) + qz * (AD * d + AU * u)) - fi
                new = num / den
                v[m] = new[m]
        return v

    def residual(self, v, f):
        """r at the unknowns, 0 at the Dirichlet points"""
        t = self.t
        fi = np.ascontiguousarray(f, self.dtype)
        o, e, n, so, d, u, cc = _nb(mirror(np.ascontiguousarray(v, self.dtype)))
        se = self._se
        if self.a is None:
            hx2, hy2, hz2 = self._stencil
            full = (fi - ((o - t(2) * cc + e) / hx2) - ((n - t(2) * cc + so) / hy2) - ((d - t(2) * cc + u) / hz2)) + se * cc
        else:
            qx, qy, qz, AW, AE, AN, AS, AD, AU = self._stencil
            tx = qx * (AW * (o - cc) + AE * (e - cc))
            ty = qy * (AN * (n - cc) + AS * (so - cc))
            tz = qz * (AD * (d - cc) + AU * (u - cc))
            full = (((fi - tx) - ty) - tz) + se * cc
        r = np.zeros(O.shape(self.n3), self.dtype)
        r[self.unk] = full[self.unk]
        return r

    def apply_A(self, p):
        """q = A p = -(residual with f = 0) at the unknowns"""
        return -self.residual(p, np.zeros(O.shape(self.n3), self.dtype))

    def rhs(self, u, q, qscale, f=None):
        """f = (-((s*c)*u)) - qscale*q at the unknowns; the other entries are those of `f` (default zeros: the library leaves them
        alone)"""
        u = np.ascontiguousarray(u, self.dtype)
        out = np.zeros(u.shape, self.dtype) if f is None else np.array(f, self.dtype)
        val = -(self._sc * u)
        if q is not None:
            val = val - self.t(qscale) * np.ascontiguousarray(q, self.dtype)
        out[self.unk] = val[self.unk]
        return out

    def add_flux(self, f, g):
        """f - 2 g / h at the face unknowns: successively for the x-, the y- and the z-face of a point whose term is not 0"""
        out = np.array(f, self.dtype)
        m = face_unknowns(self.n3, self.bc)
        for term in self.wall_terms(g):
            mk = m & (term != 0)
            out[mk] = out[mk] - term[mk]
        return out


# ------------------------------------------------------------------------------------------ transfers and levels
def restrict(n3, fine, bc, dtype, axes=7):
    """the library's restriction (full weighting inside, injection on the boundary) over the halved axes: the oracle's, or
    semi_restated's for axes in 1 .. 6; a coarse unknown on a face is its full weighting of the 27 reflected fine values"""
    if axes != 7:
        assert not bc
        return S.restrict_axes(fine, axes)
    coarse = O.restrict3d(n3, fine, dtype=dtype)
    if bc:
        padded = tuple(int(k) + 4 for k in n3)  # two layers: the fine point 2c is the padded point 2 (c + 1)
        fw = O.restrict3d(padded, np.ascontiguousarray(mirror(np.ascontiguousarray(fine, dtype), 2)), dtype=dtype)[1:-1, 1:-1, 1:-1]
        m = face_unknowns(O.csize(n3), bc)
        coarse[m] = fw[m]
    return coarse


def interpolate(n3, fine, coarse, bc, dtype, add=False, axes=7):
    """the oracle's interpolation (add: and correction) on the interior, and its formula at the fine face unknowns"""
    fine, coarse = np.ascontiguousarray(fine, dtype), np.ascontiguousarray(coarse, dtype)
    if axes != 7:
        assert not bc
        return (S.interpolate_correct_axes if add else S.interpolate_axes)(fine, coarse, axes)
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


def full_plan(n3):
    """sizes and masks of mgMultiGrid3D_create: floor(log2(min - 1)) levels, every step halves all axes"""
    sizes = [tuple(int(k) for k in n3)]
    while len(sizes) < int(math.log2(min(n3) - 1)):
        sizes.append(S.coarse_size(sizes[-1], 7))
    return sizes, (7,) * (len(sizes) - 1) + (0,)


def coarse_coefficients(sizes, masks, a, dtype):
    """a (or c: it stays >= 0) on every level: a_{l+1} = Restrict(a_l) by the step's mask, whatever the faces' mask"""
    out = [np.ascontiguousarray(a, dtype)]
    for l in range(len(sizes) - 1):
        out.append(np.ascontiguousarray(restrict(sizes[l], out[-1], 0, dtype, masks[l]), dtype))
    return out


class Hierarchy:
    """v, f, a, c and the operator of every level, and the cycles of mg_multigrid3d.inc: the stored residual, restricted; the coarse
    levels from zero on all points; interpolate + correct.  coarsening="semi" takes semi_restated's plan (refused with a mask).  The
    wall fluxes g enter f[0] through add_wall_flux().  The shift, the mean and the walls live in the operators: replace() changes
    them, and the slots keep a stray `H.s = ...` from passing silently"""
    __slots__ = ("g", "sizes", "masks", "v", "f", "a", "c", "ops")

    def __init__(self, op, coarsening="full", g=ZERO):
        assert not (op.bc and coarsening == "semi")
        self.g = tuple(g)
        self.sizes, self.masks = S.plan(op.n3, op.rng) if coarsening == "semi" else full_plan(op.n3)
        self.v = [np.zeros(O.shape(n), op.dtype) for n in self.sizes]
        self.f = [np.zeros(O.shape(n), op.dtype) for n in self.sizes]
        self.a = coarse_coefficients(self.sizes, self.masks, op.a, op.dtype) if op.a is not None else [None] * len(self.sizes)
        self.c = coarse_coefficients(self.sizes, self.masks, op.c, op.dtype) if op.c is not None else [None] * len(self.sizes)
        self.ops = [dataclasses.replace(op, n3=n, a=a, c=c) for n, a, c in zip(self.sizes, self.a, self.c)]

    def replace(self, **changes):
        """another shift, mean or wall: new operator values on every level"""
        self.ops = [dataclasses.replace(op, **changes) for op in self.ops]

    def relax(self, l, k):
        self.v[l] = self.ops[l].relax(self.v[l], self.f[l], k)

    def residual(self, l):
        return self.ops[l].residual(self.v[l], self.f[l])

    def add_wall_flux(self):
        self.f[0] = self.ops[0].add_flux(self.f[0], self.g)

    def vcycle(self, l, v1, v2):
        op = self.ops[l]
        self.relax(l, v1)
        if l != len(self.sizes) - 1:
            self.f[l + 1] = restrict(op.n3, self.residual(l), op.bc, op.dtype, self.masks[l])
            self.v[l + 1] = np.zeros(O.shape(self.sizes[l + 1]), op.dtype)
            self.vcycle(l + 1, v1, v2)
            self.v[l] = interpolate(op.n3, self.v[l], self.v[l + 1], op.bc, op.dtype, True, self.masks[l])
        self.relax(l, v2)

    def fmg(self, l, v0, v1, v2):
        op = self.ops[l]
        if l != len(self.sizes) - 1:
            self.f[l + 1] = restrict(op.n3, self.f[l], op.bc, op.dtype, self.masks[l])
            self.fmg(l + 1, v0, v1, v2)
            self.v[l] = interpolate(op.n3, self.v[l], self.v[l + 1], op.bc, op.dtype, False, self.masks[l])
        else:
            self.v[l] = O.set3d(op.n3, self.v[l], 0, False, dtype=op.dtype)
            self.v[l][face_unknowns(op.n3, op.bc)] = 0
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
        t = self.ops[0].t
        self.replace(s=t(1.0 / (kappa * dt)))
        total, worst = 0, 0.0
        for _ in range(nsteps):
            self.f[0] = self.ops[0].rhs(self.v[0], source, t(1.0 / kappa), f=self.f[0])
            self.add_wall_flux()
            k, rel, conv = self.cycle_to(v1, v2, tol, maxit)
            total, worst = total + k, max(worst, rel)
            if not conv:
                return total, worst, False
        return total, worst, True


# ------------------------------------------------------------------------------------------ solves
def m_cycle(hierarchy, v1, v2):
    """the preconditioner of PCG: the V(v1, v2) cycle from zero on all points (the fields are restricted once)"""
    H = hierarchy

    def M(r):
        for l in range(len(H.sizes)):
            H.v[l] = np.zeros(O.shape(H.sizes[l]), H.ops[l].dtype)
        H.f[0] = np.ascontiguousarray(r, H.ops[0].dtype)
        H.vcycle(0, v1, v2)
        return H.v[0].copy()
    return M


def cycles_to(op, v0, f, v1, v2, tol, maxit):
    """plain cycling from the guess v0 (PCG with krylov = 0): (x, cycles, true relative residual, converged)"""
    H = Hierarchy(op)
    H.v[0], H.f[0] = np.array(v0, op.dtype), np.ascontiguousarray(f, op.dtype)
    k, rel, conv = H.cycle_to(v1, v2, tol, maxit)
    return H.v[0], k, rel, conv


def fcg(op, v0, f, tol=1e-10, maxit=60, v1=2, v2=2, coarsening="full", weighted=True):
    """PCG(v1, v2, tol, maxit, krylov = 1 or 2): flexible CG preconditioned by the operator's V(v1, v2) cycle, returning
    (x, iterations, history, converged, true relative residual, removed mean).  The dots that make alpha and beta are math.fsum of
    W x y, W the trapezoid weights (every weight 1 without a mask; weighted=False: plain Euclidean sums over the unknowns, the
    comparison column of DESIGN.md 16); the stopping norm is fsum_sq over the unknowns, unweighted.  The closed, insulated box
    without a shift is solved in the projected sense: the right-hand side and, after every preconditioner application, z lose
    their weighted mean"""
    dtype = op.t
    unk = op.unk
    W = weights(op.n3, op.bc) if weighted else unk.astype(np.float64)
    singular = op.bc == 63 and op.s == 0 and not any(op.beta)
    M = m_cycle(Hierarchy(op, coarsening), v1, v2)
    f = np.ascontiguousarray(f, dtype)
    removed = 0.0
    if singular:
        f, removed = project(W, unk, f, dtype)

    def precond(r):
        z = M(r)
        return project(W, unk, z, dtype)[0] if singular else z

    x = np.array(v0, dtype)
    r = op.residual(x, f)
    rr0 = fsum_sq(r)
    hist, k, restart, conv = [], 0, True, False
    if rr0 == 0.0:
        return x, 0, np.array(hist), True, 0.0, removed
    while k < maxit:
        if restart:
            z = precond(r)
            p, rz, restart = z.copy(), wdot(W, r, z), False
        k += 1
        q = op.apply_A(p)
        alpha = rz / wdot(W, p, q)
        x[unk] = x[unk] + dtype(alpha) * p[unk]
        r = r - dtype(alpha) * q
        rel = math.sqrt(fsum_sq(r) / rr0)
        hist.append(rel)
        if rel < tol:
            r = op.residual(x, f)
            if math.sqrt(fsum_sq(r) / rr0) < tol:
                conv = True
                break
            restart = True
            continue
        z = precond(r)
        beta = -alpha * wdot(W, z, q) / rz
        rz = wdot(W, r, z)
        p = z + dtype(beta) * p
    return x, k, np.array(hist), conv, math.sqrt(fsum_sq(op.residual(x, f)) / rr0), removed
