"""The semi-coarsened 3D hierarchy restated (a plain module, imported by test_semi_cpu.py and test_gpu_semi.py): the level
rule of mg_semi_plan in Python, the transfer operators of csrc/mgx_semi3d.hip in numpy with the same association, and the cycle
built from them and from the oracle's relax3d / residual3d / set3d -- VCycle and FullMultiGridVCycle of mg_multigrid3d.inc with
the transfers swapped.  Arrays are in the reference layout, shape (sz, sy, sx); axis d (0 = x, 1 = y, 2 = z) is numpy axis 2 - d;
bit d of a mask = axis d is halved on the way to the next level."""
import math

import numpy as np

import oracle as O

MAX_LEVELS = 32

# the grids of the issue's table: (sizes, range, masks by level)
TABLE = [((65, 65, 65), [0, 1, 0, 1, 0, 4], (3, 3, 7, 7, 7, 4, 4)),
         ((65, 33, 129), [0, 1, 0, 1, 0, 1], (4, 5, 7, 7, 7, 7)),
         ((129, 129, 33), [0, 1, 0, 1, 0, 4], (3, 3, 3, 3, 7, 7, 4, 4)),
         ((33, 129, 65), [0, 8, 0, 1, 0, 2], (2, 2, 6, 6, 6, 7, 5, 1, 1)),
         ((257, 257, 65), [0, 1, 0, 1, 0, 4], (3, 3, 3, 3, 7, 7, 7, 4, 4)),
         ((513, 513, 257), [0, 1, 0, 1, 0, 4], (3, 3, 3, 7, 7, 7, 7, 7, 4, 4))]
ODD = ((49, 41, 57), [0, 1, 0, 2, 0, 1], (5, 7, 3))  # ends at 7 x 11 x 15


def plan(n3, rng, max_levels=0):
    """(sizes, masks) by the rule of mg_semi_plan: one (sx, sy, sz) and one mask per level, the last mask 0"""
    if any(k < 3 or k % 2 == 0 for k in n3):
        raise ValueError("sizes must be odd and >= 3")
    cap = max_levels if 0 < max_levels < MAX_LEVELS else MAX_LEVELS
    n, sizes, masks = [int(k) for k in n3], [], []
    while True:
        sizes.append(tuple(n))
        masks.append(0)
        if len(sizes) >= cap:
            break
        h = [(float(rng[2 * d + 1]) - float(rng[2 * d])) / float(n[d] - 1) for d in range(3)]
        can = [n[d] >= 5 and n[d] % 4 == 1 for d in range(3)]
        if not any(can):
            break
        hmin = min(h[d] for d in range(3) if can[d])
        for d in range(3):
            if can[d] and h[d] <= 1.5 * hmin:
                masks[-1] |= 1 << d
                n[d] = (n[d] - 1) // 2 + 1
    return sizes, tuple(masks)


def coarse_size(n3, mask):
    return tuple((n3[d] - 1) // 2 + 1 if mask >> d & 1 else n3[d] for d in range(3))


def _axes(mask):
    return [d for d in range(3) if mask >> d & 1]


def restrict_axes(fine, mask):
    """Restrict over the halved axes of mask in 1..6; the coarse boundary is injected"""
    assert 1 <= mask <= 6
    w = fine.dtype.type
    n3 = fine.shape[::-1]
    cn = coarse_size(n3, mask)
    coarse = np.ascontiguousarray(fine[tuple(slice(None, None, 2) if mask >> (2 - ax) & 1 else slice(None) for ax in range(3))]).copy()
    assert coarse.shape == cn[::-1]

    def at(off):  # fine values at offset off[d] along axis d from the fine centre of every coarse interior point
        sl = []
        for ax in range(3):
            d = 2 - ax
            if mask >> d & 1:
                sl.append(slice(2 + off.get(d, 0), 2 * (cn[d] - 2) + off.get(d, 0) + 1, 2))
            else:
                assert off.get(d, 0) == 0
                sl.append(slice(1, n3[d] - 1))
        return fine[tuple(sl)]

    ax = _axes(mask)
    C = at({})
    if len(ax) == 1:
        a = ax[0]
        val = w(0.5) * C + w(0.25) * (at({a: -1}) + at({a: 1}))
    else:
        a, b = ax
        val = (w(0.25) * C + w(0.125) * ((at({a: -1}) + at({a: 1})) + (at({b: -1}) + at({b: 1}))) +
               w(0.0625) * ((at({a: -1, b: -1}) + at({a: 1, b: -1})) + (at({a: -1, b: 1}) + at({a: 1, b: 1}))))
    coarse[1:-1, 1:-1, 1:-1] = val
    return coarse


def interpolate_values(coarse, n3, mask):
    """the interpolated value at every fine point (only the interior ones are used)"""
    assert 1 <= mask <= 6
    w = coarse.dtype.type
    out = np.zeros(n3[::-1], coarse.dtype)
    halved = _axes(mask)
    for cls in range(1 << len(halved)):
        odd = {d: cls >> k & 1 for k, d in enumerate(halved)}
        fsl, count = [], {}
        for ax in range(3):
            d = 2 - ax
            if d in odd:
                fsl.append(slice(odd[d], None, 2))
                count[d] = len(range(odd[d], n3[d], 2))
            else:
                fsl.append(slice(None))

        def c(*plus):  # coarse value at the base plus 1 along the listed axes
            sl = []
            for ax in range(3):
                d = 2 - ax
                if d in odd:
                    sl.append(slice(1, count[d] + 1) if d in plus else slice(0, count[d]))
                else:
                    sl.append(slice(None))
            return coarse[tuple(sl)]

        S = [d for d in halved if odd[d]]
        if not S:
            val = c()
        elif len(S) == 1:
            val = w(0.5) * (c() + c(S[0]))
        else:
            a, b = S
            val = w(0.25) * (((c() + c(a)) + c(b)) + c(a, b))
        out[tuple(fsl)] = val
    return out


def interpolate_axes(fine, coarse, mask):
    out = fine.copy()
    out[1:-1, 1:-1, 1:-1] = interpolate_values(coarse, fine.shape[::-1], mask)[1:-1, 1:-1, 1:-1]
    return out


def interpolate_correct_axes(v, coarse, mask):
    out = v.copy()
    out[1:-1, 1:-1, 1:-1] = v[1:-1, 1:-1, 1:-1] + interpolate_values(coarse, v.shape[::-1], mask)[1:-1, 1:-1, 1:-1]
    return out


def residual_restrict_axes(n3, rng, v, f, mask, mode, dtype):
    """the restricted residual: 0 on the coarse boundary (the residual is 0 on the fine one)"""
    return restrict_axes(O.residual3d(n3, rng, v, f, mode, dtype=dtype), mask)


class Hierarchy:
    """v and f of every level of a semi-coarsened hierarchy and the cycles of mg_multigrid3d.inc on them"""

    def __init__(self, n3, rng, dtype=np.float64, mode=O.CORRECT, max_levels=0):
        self.rng, self.dtype, self.mode = list(rng), dtype, mode
        self.sizes, self.masks = plan(n3, rng, max_levels)
        self.v = [np.zeros(O.shape(n), dtype) for n in self.sizes]
        self.f = [np.zeros(O.shape(n), dtype) for n in self.sizes]

    def relax(self, l, k):
        self.v[l] = O.relax3d(self.sizes[l], self.rng, self.v[l], self.f[l], k, dtype=self.dtype)

    def vcycle(self, l, v1, v2):
        n, dt = self.sizes[l], self.dtype
        self.relax(l, v1)
        if l != len(self.sizes) - 1:
            r = O.residual3d(n, self.rng, self.v[l], self.f[l], self.mode, dtype=dt)
            m = self.masks[l]
            self.f[l + 1] = O.restrict3d(n, r, dtype=dt) if m == 7 else restrict_axes(r, m)
            self.v[l + 1] = O.set3d(self.sizes[l + 1], self.v[l + 1], 0, True, dtype=dt)
            self.vcycle(l + 1, v1, v2)
            if m == 7:
                e = O.interpolate3d(n, np.zeros_like(self.v[l]), self.v[l + 1], dtype=dt)
                self.v[l] = O.correct3d(n, self.v[l], e, dtype=dt)
            else:
                self.v[l] = interpolate_correct_axes(self.v[l], self.v[l + 1], m)
        self.relax(l, v2)

    def fmg(self, l, v0, v1, v2):
        n, dt = self.sizes[l], self.dtype
        if l != len(self.sizes) - 1:
            m = self.masks[l]
            self.f[l + 1] = O.restrict3d(n, self.f[l], dtype=dt) if m == 7 else restrict_axes(self.f[l], m)
            self.fmg(l + 1, v0, v1, v2)
            self.v[l] = O.interpolate3d(n, self.v[l], self.v[l + 1], dtype=dt) if m == 7 else interpolate_axes(self.v[l], self.v[l + 1], m)
        else:
            self.v[l] = O.set3d(n, self.v[l], 0, False, dtype=dt)
        for _ in range(v0):
            self.vcycle(l, v1, v2)


def m_cycle(n3, rng, v1, v2, dtype=np.float64):
    """the preconditioner of PCG on a semi-coarsened hierarchy: its V-cycle from zero"""
    def M(r):
        H = Hierarchy(n3, rng, dtype)
        H.f[0] = np.ascontiguousarray(r, dtype)
        H.vcycle(0, v1, v2)
        return H.v[0]
    return M


def cycles_to(n3, rng, f, v1, v2, tol, maxit, dtype=np.float64):
    """plain cycling from a zero guess: (cycles, true relative residual) at the first cycle below tol, or after maxit"""
    H = Hierarchy(n3, rng, dtype)
    H.f[0] = np.ascontiguousarray(f, dtype)

    def norm():
        r = O.residual3d(n3, rng, H.v[0], H.f[0], O.CORRECT, dtype=dtype)
        return math.sqrt(math.fsum((r.astype(np.float64) ** 2).ravel()))

    r0, rel = norm(), float("inf")
    for k in range(1, maxit + 1):
        H.vcycle(0, v1, v2)
        rel = norm() / r0
        if rel < tol:
            return k, rel
    return maxit, rel
