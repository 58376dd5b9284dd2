"""Shared helpers of the solve tests (a plain module, imported by test_gpu_pcg.py, test_gpu_pcg_mixed.py and
test_gpu_solve_scale.py): the numpy restatements of flexible CG and of defect correction, their preconditioners (the oracle's
V-cycle from zero, in the hierarchy's precision or in fp32), and the protocol the kernel tests share."""
import math

import numpy as np

import oracle as O
import pde_multigrid_amd as P
from conftest import bits_equal
from odd_shapes import pads_unchanged
from pde_multigrid_amd.multigrid import xs_unpack


def interior(a):
    return a[1:-1, 1:-1, 1:-1]


def boundary_mask(n3):
    m = np.ones(O.shape(n3), bool)
    m[1:-1, 1:-1, 1:-1] = False
    return m


def fsum_dot(a, b):
    return math.fsum((interior(a).astype(np.float64) * interior(b).astype(np.float64)).ravel())


def close(got, want, rtol):
    return abs(got - want) <= rtol * max(abs(want), 1e-300)


def check_out(n3, up, got_stored, want, was):
    """interior = want bit for bit, boundary = was, pads as uploaded"""
    got = xs_unpack(got_stored, n3[0])
    assert bits_equal(interior(got), interior(want))
    assert bits_equal(got[boundary_mask(n3)], was[boundary_mask(n3)]), "a boundary entry was written"
    assert pads_unchanged(up, got_stored, n3[0])


def problem(n3, dtype=np.float64, seed=0):
    f = np.zeros(O.shape(n3), dtype)
    interior(f)[...] = np.random.default_rng(seed).uniform(-1, 1, interior(f).shape)
    return f


def m_cycle(n3, rng, v1, v2, nlevels=0, dtype=np.float64):
    """the preconditioner of PCG: the oracle's V-cycle from zero in the hierarchy's precision"""
    def M(r):
        return O.cycle3d(n3, rng, nlevels=nlevels, mode=0, v0=1, v1=v1, v2=v2, v=np.zeros_like(r), f=r, residual_mode=O.CORRECT,
                         dtype=dtype)
    return M


def m32(n3, rng, v1, v2, nlevels=0):
    """the preconditioner of the mixed solve: the oracle's fp32 V-cycle from zero on float32(r), promoted"""
    def M(r):
        r32 = r.astype(np.float32)
        return O.cycle3d(n3, rng, nlevels=nlevels, mode=0, v0=1, v1=v1, v2=v2, v=np.zeros_like(r32), f=r32, residual_mode=O.CORRECT,
                         dtype=np.float32).astype(np.float64)
    return M


def ir_restated(n3, rng, v0, f, v1, v2, steps, nlevels=0):
    """defect correction: x after each of `steps` steps x += M(b - A x)"""
    M = m32(n3, rng, v1, v2, nlevels)
    x, out = v0.copy(), []
    for _ in range(steps):
        x = x + M(O.residual3d(n3, rng, x, f, P.CORRECT, dtype=np.float64))
        out.append(x)
    return out


def fcg_restated(n3, rng, v0, f, M, tol, maxit, dtype=np.float64):
    """flexible CG of mg_multigrid.h in numpy: A p = -residual(p, 0, CORRECT), z = M(r)"""
    def A(p):
        return -O.residual3d(n3, rng, p, np.zeros_like(p), P.CORRECT, dtype=dtype)

    def dot(a, b):
        return math.fsum((a.astype(np.float64) * b.astype(np.float64)).ravel())

    x = v0.copy()
    r = O.residual3d(n3, rng, x, f, P.CORRECT, dtype=dtype)
    rr0 = dot(r, r)
    hist, k, restart, conv = [], 0, True, False
    while k < maxit:
        if restart:
            z = M(r)
            p, rz, restart = z.copy(), dot(r, z), False
        k += 1
        q = A(p)
        alpha = rz / dot(p, q)
        x = x + dtype(alpha) * p
        r = r - dtype(alpha) * q
        rel = math.sqrt(dot(r, r) / rr0)
        hist.append(rel)
        if rel < tol:
            r = O.residual3d(n3, rng, x, f, P.CORRECT, dtype=dtype)
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


def true_rel(n3, rng, x, f, v0):
    r = O.residual3d(n3, rng, x, f, P.CORRECT, dtype=np.float64)
    r0 = O.residual3d(n3, rng, v0, f, P.CORRECT, dtype=np.float64)
    return np.linalg.norm(interior(r)) / np.linalg.norm(interior(r0))
