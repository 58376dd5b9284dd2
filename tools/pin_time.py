#!/usr/bin/python3
"""Wall time of cycles and solves with pinned interior nodes against the same hierarchy without pins, fp64, on the
unit cube at 257^3 and 513^3: the shifted operator (s = 1), whose route is the one a hierarchy with pins takes, so that the
difference is the list launches and the stored-residual route alone --

  V(2,2)          VCycle(0, 2, 2), best of `reps` after a warm-up
  PCG             PCG(2, 2, tol = 1e-8, krylov = True) from a zero guess with a random right-hand side: time and iterations
  ResidualNorm    the residual, its pins zeroed, and the norm (with pins the sum is a read pass of its own)

-- for three pinned sets: a plate (the interior points of an odd plane next to the middle: a surface-sized set, 2.6e5 points at
513^3), a ball of radius 0.3, and the complement of a ball of radius 0.4 (a bulk set, about 70 % of the grid).  Reported only:
nothing is asserted.

    python tools/pin_time.py [--sizes 257 513] [--reps 3]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pde_multigrid_amd as P  # noqa: E402

RNG = [0, 1, 0, 1, 0, 1]


def timed(ctx, fn, reps):
    best, out = 1e9, None
    for rep in range(1 + reps):
        ctx.sync()
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        if rep:
            best = min(best, time.perf_counter() - t0)
    return best, out


def sets(n):
    ax = np.arange(n)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij", sparse=True)
    c = (n - 1) / 2
    r2 = (x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2
    inner = (x > 0) & (x < n - 1) & (y > 0) & (y < n - 1) & (z > 0) & (z < n - 1)
    plate = inner & (z == (n // 2) | 1)  # the interior of an odd plane: 2.6e5 points at 513^3
    return {"none": None, "plate": plate, "ball": inner & (r2 <= (0.3 * (n - 1)) ** 2), "outside a ball": inner & (r2 > (0.4 * (n - 1)) ** 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[257, 513])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    ctx = P.Context(0)
    for n in args.sizes:
        n3 = (n, n, n)
        rng = np.random.default_rng(1)
        f = rng.uniform(-1, 1, (n, n, n))
        g = rng.uniform(-1, 1, (n, n, n))
        zero = np.zeros((n, n, n))
        mg = P.MultiGrid3D(ctx, n3, RNG, np.float64, residual_mode=P.CORRECT, shift=1.0)
        base = None
        for name, mask in sets(n).items():
            mg.set_pinned(mask, g)
            mg.upload_v(0, zero)
            mg.upload_f(0, f)
            t_v, _ = timed(ctx, lambda: mg.VCycle(0, 2, 2), args.reps)
            t_n, _ = timed(ctx, lambda: mg.ResidualNorm(0), args.reps)

            def solve():
                mg.upload_v(0, zero)
                return mg.PCG(2, 2, 1e-8, 60, krylov=True)
            t_up, _ = timed(ctx, lambda: mg.upload_v(0, zero), args.reps)
            t_p, res = timed(ctx, solve, args.reps)
            t_p -= t_up
            cnt = mg.pinned_count(0)
            row = (t_v, t_p, t_n)
            base = base or row
            print("%d^3 %-15s %9d pins (%5.2f %%): V(2,2) %7.2f ms (x%.3f)   PCG %2d it %8.2f ms (x%.3f, %6.2f ms/it)   ResidualNorm %6.2f ms (x%.3f)"
                  % (n, name, cnt, 100.0 * cnt / n ** 3, 1e3 * t_v, t_v / base[0], res[0], 1e3 * t_p, t_p / base[1], 1e3 * t_p / max(res[0], 1),
                     1e3 * t_n, t_n / base[2]), flush=True)
        mg.close()
    ctx.close()


if __name__ == "__main__":
    main()
