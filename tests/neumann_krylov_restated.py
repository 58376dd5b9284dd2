"""Flexible CG in the weighted inner product restated (a plain module, imported by test_neumann_krylov_cpu.py and
test_gpu_neumann_krylov.py): PCG(krylov = 2) of mg_multigrid3d.inc on a hierarchy with a face mask, on neumann_restated's operators
and cycle, with the associations of coef_restated.fcg_restated.  The dots that make alpha and beta are math.fsum of W x y, W the
trapezoid weights of neumann_restated.weights (1/2 per Neumann face an unknown lies on); the stopping norm is fsum_sq over the
unknowns, unweighted.  The closed box without a shift (mask 63, s = 0) is solved in the projected sense: the right-hand side and,
after every preconditioner application, z lose their weighted mean.  Arrays are in the reference layout, shape (sz, sy, sx)."""
import math

import numpy as np

import coef_restated as CO
import neumann_restated as NR
import oracle as O
from shift_restated import fsum_sq

UNIT = [0, 1, 0, 1, 0, 1]
TOL = 1e-10


def wdot(W, x, y):
    return math.fsum((W * x.astype(np.float64) * y.astype(np.float64)).ravel())


def wmean(W, x):
    """sum_W(x) / sum(W); sum(W) is exact in double"""
    return math.fsum((W * x.astype(np.float64)).ravel()) / float(W.sum())


def sum_weights(n3, bc):
    """sum(W), separable: per axis the interior points plus half a point per Neumann end"""
    return math.prod((int(k) - 2) + 0.5 * (((bc >> (2 * d)) & 1) + ((bc >> (2 * d + 1)) & 1)) for d, k in enumerate(n3))


def m_cycle(n3, rng, a, s, bc, v1, v2, dtype=np.float64):
    """the preconditioner: the V(v1, v2) cycle of a hierarchy with the mask from zero on all points"""
    H = NR.Hierarchy(n3, rng, a, s, bc, dtype)

    def M(r):
        for l in range(len(H.sizes)):
            H.v[l] = np.zeros(O.shape(H.sizes[l]), dtype)
        H.f[0] = np.ascontiguousarray(r, dtype)
        H.vcycle(0, v1, v2)
        return H.v[0].copy()
    return M


def project(W, unk, x, dtype):
    """(x - (dtype)mean_W(x) at the unknowns, the mean)"""
    m = wmean(W, x)
    out = np.array(x, dtype)
    out[unk] = out[unk] - dtype(m)
    return out, m


def wfcg(n3, rng, a, s, bc, v0, f, tol=TOL, maxit=60, v1=2, v2=2, dtype=np.float64, weighted=True):
    """PCG(v1, v2, tol, maxit, krylov = 2): (x, iterations, history, converged, true relative residual, removed mean).
    weighted=False: the dots as plain Euclidean sums over the unknowns (the comparison column of DESIGN.md 16)."""
    dtype = np.dtype(dtype).type
    unk = NR.unknown_mask(n3, bc)
    W = NR.weights(n3, bc) if weighted else unk.astype(np.float64)
    singular = bc == 63 and s == 0
    M = m_cycle(n3, rng, a, s, bc, v1, v2, dtype)
    f = np.ascontiguousarray(f, dtype)
    removed = 0.0
    if singular:
        f, removed = project(W, unk, f, dtype)

    def res(x):
        return NR.residual(n3, rng, x, f, a, s, bc, dtype)

    def precond(r):
        z = M(r)
        return project(W, unk, z, dtype)[0] if singular else z

    x = np.array(v0, dtype)
    r = res(x)
    rr0 = fsum_sq(r)
    hist, k, restart, conv = [], 0, True, False
    if rr0 == 0.0:
        return x, 0, np.array(hist), True, 0.0, removed
    while k < maxit:
        if restart:
            z = precond(r)
            p, rz, restart = z.copy(), wdot(W, r, z), False
        k += 1
        q = NR.apply_A(n3, rng, p, a, s, bc, dtype)
        alpha = rz / wdot(W, p, q)
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
        z = precond(r)
        beta = -alpha * wdot(W, z, q) / rz
        rz = wdot(W, r, z)
        p = z + dtype(beta) * p
    return x, k, np.array(hist), conv, math.sqrt(fsum_sq(res(x)) / rr0), removed


def decisive(hist, tol=TOL, factor=1.5):
    """does the history keep `factor` from tol on both sides of the deciding iteration (the count is then safe to compare)"""
    return len(hist) >= 1 and hist[-1] * factor < tol and (len(hist) < 2 or hist[-2] > tol * factor)


# ---- the case table of DESIGN.md 16: (mask, shift, coefficient) -> weighted CG iterations at 17^3 and at 33^3 (V(2,2), fp64, unit
# cube, tol 1e-10, the start of table_start); coefficient: None, "smooth" or the jump of coef_restated.  The three rows of the
# closed box without a shift are counted from the zero guess with the same f: from there the restated solver takes all six of their
# figures, from the random guess it takes 7, 7, 14 at 17^3 and 7, 7, 16 at 33^3 (A v0 of a random v0 is rough and large, so rr0 is
# larger and tol is met earlier).
CASES = [
    (62, 0.0, None, 7, 7),
    (63, 1.0, None, 9, 8),
    (63, 100.0, 100, 9, 12),
    (63, 1.0, 1000, 29, 30),
    (37, 0.0, 1000, 23, 28),
    (37, 0.0, "smooth", 7, 7),
    (63, 0.0, None, 7, 7),
    (63, 0.0, "smooth", 8, 8),
    (63, 0.0, 100, 18, 20),
]
# the cases whose count is compared exactly at 17^3 (their histories are decisive there)
EXACT_17 = [0, 2, 5, 6, 7]


def coefficient(n3, kind, dtype=np.float64):
    if kind is None:
        return None
    return CO.smooth_coefficient(n3, dtype) if kind == "smooth" else CO.jump_coefficient(n3, kind, dtype)


def start(n3, dtype=np.float64, seed=11):
    """(v0, f): uniform in (-1, 1), v0 drawn first, as vcycle_case draws them"""
    g = np.random.default_rng(seed)
    return g.uniform(-1, 1, O.shape(n3)).astype(dtype), g.uniform(-1, 1, O.shape(n3)).astype(dtype)


def table_start(case, n3, dtype=np.float64):
    """(v0, f) of table row `case`: start(), with the zero guess in the rows of the closed box without a shift"""
    v0, f = start(n3, dtype)
    bc, s = CASES[case][:2]
    return (np.zeros_like(v0) if bc == 63 and s == 0 else v0), f


_solved = {}


def solved(case, size, dtype=np.float64, tol=TOL, random_guess=False):
    """wfcg of table case `case` on size^3 from table_start() (random_guess: from start() in every row), computed once and shared
    (do not modify the arrays)"""
    key = (case, size, np.dtype(dtype).name, tol, bool(random_guess))
    if key not in _solved:
        bc, s, kind = CASES[case][:3]
        n3 = (size,) * 3
        v0, f = start(n3, dtype) if random_guess else table_start(case, n3, dtype)
        _solved[key] = wfcg(n3, UNIT, coefficient(n3, kind, dtype), s, bc, v0, f, tol=tol, dtype=dtype)
    return _solved[key]
