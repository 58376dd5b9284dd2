"""Pinned interior nodes restated (a plain module, imported by test_pin_cpu.py and test_gpu_zzzz_pin.py): op_restated's
operator with a smaller set of unknowns, the coarse rule, the cycles that keep the pinned entries, and the flexible CG on them.

A pinned point is no unknown: its value is data on every level, its neighbours read it as they read a Dirichlet face point, and the
residual, A p and every CG vector are 0 there.  `PinOp.unk` is `unknown_mask & ~pin`; relax, residual, apply_A and rhs of
op_restated.Op work on `unk` alone, so they skip the pins -- bit for bit what the library does when it updates every interior point
and puts the pinned values back, because a pinned value never changes.

The coarse rule: a coarse point is pinned when its coincident fine point is, or one of that point's neighbours at +-1 along an axis
the step halves; boundary points of the coarse grid never are.  The values go down by injection (the array g sampled at the
coincident fine points, whatever the mask there).  The level a cycle starts on holds g at its pins, every level below zeros."""
import dataclasses
import functools
import math

import numpy as np

import op_restated as R
import oracle as O

RULES = ("injection", "weighted", "any27", "axis")


@dataclasses.dataclass(frozen=True, eq=False)
class PinOp(R.Op):
    pin: np.ndarray = None

    @functools.cached_property
    def unk(self):
        return R.unknown_mask(self.n3, self.bc) & ~np.asarray(self.pin, bool)


def _sample(a, axes):
    """the entries of `a` at the fine points that coincide with coarse ones (numpy's axes are z, y, x; bit 0 of `axes` is x)"""
    return a[tuple(slice(None, None, 2) if axes & bit else slice(None) for bit in (4, 2, 1))]


def _interior(m):
    out = np.zeros_like(m)
    out[1:-1, 1:-1, 1:-1] = m[1:-1, 1:-1, 1:-1]
    return out


def _shifted(m, axis, d):
    """m moved by d along axis, False shifted in"""
    out = np.zeros_like(m)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    src[axis], dst[axis] = (slice(None, -1), slice(1, None)) if d > 0 else (slice(1, None), slice(None, -1))
    out[tuple(dst)] = m[tuple(src)]
    return out


def coarse_pin(pin, axes=7, rule="axis"):
    """the coarse mask of a step that halves `axes`.  rule "axis" is the library's; the others are the candidates of DESIGN.md 22's
    table (full coarsening only): "injection" the coincident point alone, "weighted" the full-weighted mask >= 1/4, "any27" any of
    the 27 fine neighbours"""
    pin = np.asarray(pin, bool)
    assert rule in RULES and (rule == "axis" or axes == 7)
    if rule == "injection":
        fat = pin
    elif rule == "axis":
        fat = pin.copy()
        for bit, axis in ((1, 2), (2, 1), (4, 0)):
            if axes & bit:
                fat = fat | _shifted(pin, axis, 1) | _shifted(pin, axis, -1)
    else:
        w = pin.astype(np.float64)
        for axis in range(3):  # the tensor product (1/4, 1/2, 1/4), or any neighbour
            lo, hi = _shifted(w, axis, 1), _shifted(w, axis, -1)
            w = 0.25 * lo + 0.5 * w + 0.25 * hi if rule == "weighted" else np.maximum(np.maximum(lo, hi), w)
        fat = w >= 0.25 if rule == "weighted" else w > 0
    return _interior(_sample(fat, axes))


class PinHierarchy(R.Hierarchy):
    """op_restated.Hierarchy with the points of `pin` (level 0, booleans) pinned to the entries of `g` (an array over level 0;
    None: zeros).  pins[l] and gs[l] are the levels' masks and values; v[l] holds gs[l] at pins[l] from the start"""
    __slots__ = ("pins", "gs", "rule")

    def __init__(self, op, pin, g=None, coarsening="full", wall_g=R.ZERO, rule="axis"):
        super().__init__(op, coarsening, wall_g)
        pin = np.asarray(pin, bool)
        assert pin.shape == O.shape(op.n3) and not (pin & (R.on_faces(op.n3) != 0)).any(), "only interior points can be pinned"
        self.rule = rule
        self.pins = [pin]
        self.gs = [np.zeros(O.shape(op.n3), op.dtype) if g is None else np.ascontiguousarray(g, op.dtype)]
        for l in range(len(self.sizes) - 1):
            self.pins.append(coarse_pin(self.pins[-1], self.masks[l], rule))
            self.gs.append(np.ascontiguousarray(_sample(self.gs[-1], self.masks[l])))
        self.ops = [PinOp(**{f.name: getattr(o, f.name) for f in dataclasses.fields(o)}, pin=p) for o, p in zip(self.ops, self.pins)]
        for l in range(len(self.sizes)):
            self.put(l)

    def put(self, l):
        """v[l] = g_l at the level's pins"""
        self.v[l][self.pins[l]] = self.gs[l][self.pins[l]]

    def set_v(self, v0):
        """level 0's iterate: v0 with the pinned values"""
        self.v[0] = np.array(v0, self.ops[0].dtype)
        self.put(0)

    def relax(self, l, k, top=True):
        """the public Relax is the top of a cycle: the level's pins hold g_l whatever an earlier cycle left there"""
        if top:
            self.put(l)
        super().relax(l, k)

    def vcycle(self, l, v1, v2, top=True):
        """the base cycle; top: the level the cycle starts on, whose pins hold g_l (the levels below and, with top=False, the level
        of a preconditioner hold zeros there: a correction); the pinned entries of v[l] survive the correction"""
        op = self.ops[l]
        if top:
            self.put(l)
        self.relax(l, v1, False)
        if l != len(self.sizes) - 1:
            self.f[l + 1] = R.restrict(op.n3, self.residual(l), op.bc, op.dtype, self.masks[l])  # (the residual is 0 at the pins)
            self.v[l + 1] = np.zeros(O.shape(self.sizes[l + 1]), op.dtype)
            self.vcycle(l + 1, v1, v2, False)
            keep = self.v[l][self.pins[l]].copy()
            self.v[l] = R.interpolate(op.n3, self.v[l], self.v[l + 1], op.bc, op.dtype, True, self.masks[l])
            self.v[l][self.pins[l]] = keep
        self.relax(l, v2, False)

    def fmg(self, l, v0, v1, v2):
        op = self.ops[l]
        if l != len(self.sizes) - 1:
            self.f[l + 1] = R.restrict(op.n3, self.f[l], op.bc, op.dtype, self.masks[l])
            self.fmg(l + 1, v0, v1, v2)
            self.v[l] = R.interpolate(op.n3, self.v[l], self.v[l + 1], op.bc, op.dtype, False, self.masks[l])
        else:
            self.v[l] = O.set3d(op.n3, self.v[l], 0, False, dtype=op.dtype)
            self.v[l][R.face_unknowns(op.n3, op.bc)] = 0
        self.put(l)
        for _ in range(v0):
            self.vcycle(l, v1, v2)


def pin_fcg(op, pin, g, v0, f, tol=1e-10, maxit=60, v1=2, v2=2, coarsening="full", rule="axis"):
    """op_restated.fcg's algorithm on a PinHierarchy: (x, iterations, history, converged, true relative residual).  x holds g at the
    pins; r, z, p and q are 0 there, so the weights there do not matter; the closed box is not solved with pins"""
    assert not (op.bc == 63 and op.s == 0 and not any(op.beta))
    H = PinHierarchy(op, pin, g, coarsening, rule=rule)
    top = H.ops[0]
    dtype, unk = top.t, top.unk
    W = R.weights(op.n3, op.bc) * unk

    def M(r):  # op_restated.m_cycle with level 0 as a correction
        for l in range(len(H.sizes)):
            H.v[l] = np.zeros(O.shape(H.sizes[l]), H.ops[l].dtype)
        H.f[0] = np.ascontiguousarray(r, dtype)
        H.vcycle(0, v1, v2, False)
        return H.v[0].copy()

    f = np.ascontiguousarray(f, dtype)
    x = np.array(v0, dtype)
    x[H.pins[0]] = H.gs[0][H.pins[0]]
    r = top.residual(x, f)
    rr0 = R.fsum_sq(r)
    hist, k, restart, conv = [], 0, True, False
    if rr0 == 0.0:
        return x, 0, np.array(hist), True, 0.0
    while k < maxit:
        if restart:
            z = M(r)
            p, rz, restart = z.copy(), R.wdot(W, r, z), False
        k += 1
        q = top.apply_A(p)
        alpha = rz / R.wdot(W, p, q)
        x[unk] = x[unk] + dtype(alpha) * p[unk]
        r = r - dtype(alpha) * q
        rel = math.sqrt(R.fsum_sq(r) / rr0)
        hist.append(rel)
        if rel < tol:
            r = top.residual(x, f)
            if math.sqrt(R.fsum_sq(r) / rr0) < tol:
                conv = True
                break
            restart = True
            continue
        z = M(r)
        beta = -alpha * R.wdot(W, z, q) / rz
        rz = R.wdot(W, r, z)
        p = z + dtype(beta) * p
    return x, k, np.array(hist), conv, math.sqrt(R.fsum_sq(top.residual(x, f)) / rr0)


# ------------------------------------------------------------------------------------------ the pinned sets of the tests
def coords(n3):
    sx, sy, sz = (int(k) for k in n3)
    return np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")


def ball(n3, frac=0.3):
    """the interior points within frac * (the smallest extent) of the centre"""
    z, y, x = coords(n3)
    c = [(int(k) - 1) / 2 for k in n3]
    rad = frac * (min(n3) - 1)
    return _interior((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= rad * rad)


def outside_ball(n3, frac=0.4):
    m = np.ones(O.shape(n3), bool)
    return _interior(m & ~ball(n3, frac))


def plate(n3, z0):
    """part of the plane z = z0: the interior points with x and y in the middle half"""
    z, y, x = coords(n3)
    sx, sy = int(n3[0]), int(n3[1])
    return _interior((z == z0) & (x >= sx // 4) & (x <= 3 * sx // 4) & (y >= sy // 4) & (y <= 3 * sy // 4))


def wire(n3):
    """a line along x at odd y and z"""
    z, y, x = coords(n3)
    oy, oz = (int(n3[1]) // 2) | 1, (int(n3[2]) // 2) | 1
    return _interior((y == oy) & (z == oz))


def point(n3, xyz):
    m = np.zeros(O.shape(n3), bool)
    m[xyz[2], xyz[1], xyz[0]] = True
    return m


def random_set(n3, frac=0.1, seed=5):
    return _interior(np.random.default_rng(seed).uniform(size=O.shape(n3)) < frac)


def table_sets(n3):
    """the seven sets of DESIGN.md 22's table"""
    h = int(n3[2]) // 2
    even, odd = h - (h & 1), h | 1
    return {"ball": ball(n3), "outside a ball": outside_ball(n3), "plate, even plane": plate(n3, even), "plate, odd plane": plate(n3, odd),
            "wire, odd coordinates": wire(n3), "one point": point(n3, tuple(int(k) // 2 for k in n3)), "10 % at random": random_set(n3)}
