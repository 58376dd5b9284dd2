"""What the eigensolver's tests share (a plain module, imported by test_eigen_cpu.py and test_gpu_zz_eigen.py): the closed-form
spectrum of the constant-coefficient operator on a box, the dense reference built from the restated operator (op_restated.Op),
the bound the computed eigenvalues are held to, and the cases.

The problem: -(div(a grad x)) [+ the walls' diagonal] = lambda c x on the unknowns of the mask bc.  With the shift s the operator
of the hierarchy is A_s = div(a grad .) - s c, so -A_s x = mu c x with mu = lambda + s; in the inner product <u, v>_W = sum W u v
(W = 1/2 per wall an unknown lies on) -A_s is symmetric positive definite."""
import functools
import math

import numpy as np

import op_restated as OP
import oracle as O

EPS = float(np.finfo(np.float64).eps)
BOX = [0, 1, 0, 1.25, 0, 1.5]  # no eigenvalue among the first eight of a cube-shaped grid is degenerate on it


def axis_values(n, h, lo_wall, hi_wall):
    """the eigenvalues (2 - 2 cos(kappa pi / (n - 1))) / h^2 of one axis: Dirichlet-Dirichlet kappa = 1 .. n-2, wall-wall
    kappa = 0 .. n-1, mixed kappa = 1/2, 3/2, .. (n - 1 of them)"""
    if lo_wall and hi_wall:
        kappa = np.arange(0, n, dtype=np.float64)
    elif lo_wall or hi_wall:
        kappa = np.arange(0, n - 1, dtype=np.float64) + 0.5
    else:
        kappa = np.arange(1, n - 1, dtype=np.float64)
    return (2.0 - 2.0 * np.cos(kappa * math.pi / (n - 1))) / (h * h)


def closed_form(n3, rng, bc):
    """every eigenvalue of the constant-coefficient operator with insulated walls on the faces of bc, ascending"""
    ax = []
    for d in range(3):
        h = (float(rng[2 * d + 1]) - float(rng[2 * d])) / (int(n3[d]) - 1)
        ax.append(axis_values(int(n3[d]), h, (bc >> (2 * d)) & 1, (bc >> (2 * d + 1)) & 1))
    return np.sort((ax[0][:, None, None] + ax[1][None, :, None] + ax[2][None, None, :]).ravel())


def norm_A(n3, rng):
    """||A|| <= 4 sum_d 1 / h_d^2"""
    return 4.0 * sum(((int(n3[d]) - 1) / (float(rng[2 * d + 1]) - float(rng[2 * d]))) ** 2 for d in range(3))


def bound(exact, k, tol, s, n3, rng):
    """|lambda_i - exact_i| <= (tol mu_i)^2 / gap_i + 64 eps ||A|| for i < k: the Kato-Temple bound of a vector whose residual is
    tol mu_i (gap_i: the distance to the nearest other exact eigenvalue) plus the rounding of a Rayleigh quotient"""
    exact = np.asarray(exact, np.float64)
    out = np.empty(k)
    for i in range(k):
        gap = min(abs(exact[i] - exact[j]) for j in (i - 1, i + 1) if 0 <= j < len(exact))  # (exact is ascending)
        out[i] = (tol * (exact[i] + s)) ** 2 / gap + 64 * EPS * norm_A(n3, rng)
    return out


def dense(op):
    """(S, unk): S = diag(W) K with K = -A_s on the unknowns, column by column from op.apply_A on unit vectors, and the unknowns'
    mask.  S is symmetric to the bit (test_eigen_cpu.py)."""
    unk = op.unk
    idx = np.flatnonzero(unk.ravel())
    W = OP.weights(op.n3, op.bc).ravel()[idx]
    K = np.empty((idx.size, idx.size))
    e = np.zeros(O.shape(op.n3), np.float64)
    for j, p in enumerate(idx):
        e.ravel()[p] = 1.0
        K[:, j] = -op.apply_A(e).ravel()[idx]
        e.ravel()[p] = 0.0
    return W[:, None] * K, unk


def dense_spectrum(op):
    """every lambda of the dense problem S x = mu diag(W c) x, ascending, lambda = mu - s, and the eigenvectors (columns, on the
    unknowns) with x^T diag(W c) x = 1"""
    S, unk = dense(op)
    idx = np.flatnonzero(unk.ravel())
    d = OP.weights(op.n3, op.bc).ravel()[idx]
    if op.c is not None:
        d = d * np.asarray(op.c, np.float64).ravel()[idx]
    r = 1.0 / np.sqrt(d)
    M = r[:, None] * (0.5 * (S + S.T)) * r[None, :]
    mu, Z = np.linalg.eigh(M)
    return mu - float(op.s), r[:, None] * Z


def wc(op):
    """W c at every point (W where there is no capacity)"""
    W = OP.weights(op.n3, op.bc)
    return W if op.c is None else W * np.asarray(op.c, np.float64)


def residuals(op, lam, X):
    """res_i = ||A_s x_i + mu_i c x_i||_W / (mu_i ||x_i||_W) recomputed in numpy from the restated operator"""
    W = OP.weights(op.n3, op.bc)
    c = 1.0 if op.c is None else np.asarray(op.c, np.float64)
    out = []
    for l, x in zip(lam, X):
        mu = l + float(op.s)
        r = np.where(op.unk, op.apply_A(x) + mu * (c * x), 0.0)
        out.append(math.sqrt(OP.wdot(W, r, r)) / (mu * math.sqrt(OP.wdot(W, x, x))))
    return np.array(out)


# ---- the materials case: 17 x 9 x 9 on [0,2] x [0,1] x [0,1]; a jumps by 100 across x = 0.9 and varies smoothly in y, c jumps by 10
# across z = 0.5; walls x-low, y-low, z-high (mask 37), convective on x-low and y-low; s = 2
MAT_N, MAT_RNG, MAT_BC, MAT_BETA, MAT_S = (17, 9, 9), [0, 2, 0, 1, 0, 1], 37, (0.7, 0.0, 3.0, 0.0, 0.0, 0.0), 2.0


def materials():
    sx, sy, sz = MAT_N
    z, y, x = np.meshgrid(np.linspace(0, 1, sz), np.linspace(0, 1, sy), np.linspace(0, 2, sx), indexing="ij")
    a = (1.0 + 0.5 * np.sin(math.pi * y)) * np.where(x < 0.9, 1.0, 100.0)
    c = np.where(z < 0.5, 1.0, 10.0)
    return np.ascontiguousarray(a), np.ascontiguousarray(c)


@functools.lru_cache(maxsize=None)
def materials_op(mean):
    a, c = materials()
    return OP.Op(MAT_N, MAT_RNG, np.float64, MAT_S, a=a, c=c, bc=MAT_BC, beta=MAT_BETA, mean=mean)


@functools.lru_cache(maxsize=None)
def materials_spectrum(mean):
    return dense_spectrum(materials_op(mean))[0]
