#!/usr/bin/python3
"""Wall time of MultiGrid3D.PCG against plain V(2,2) cycling (krylov=False), both to a true relative residual of 1e-10, fp64,
on the isotropic 513^3 unit cube and on 513x513x257 with z in [0, 4] (random interior right-hand side, zero guess).  Each
solve runs once untimed (allocations, first-use paths) and is then timed from a synchronised start to its return.

    python tools/pcg_time.py [--only iso|aniso] [--reps N]

Under rocprofv3 --kernel-trace --stats the kernel table gives each PCG kernel's time per launch; the launches per solve are
(iterations) x (1 laplace_dot + 1 cg_update + 1 dot2 + 1 cg_direction) plus a few around the loop."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pde_multigrid_amd as P  # noqa: E402

CASES = {"iso": ((513, 513, 513), [0, 1, 0, 1, 0, 1]), "aniso": ((513, 513, 257), [0, 1, 0, 1, 0, 4])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    ctx = P.Context(0)
    for name, (n3, rng) in CASES.items():
        if args.only and name != args.only:
            continue
        f = np.zeros(n3[::-1])
        f[1:-1, 1:-1, 1:-1] = np.random.default_rng(0).uniform(-1, 1, (n3[2] - 2, n3[1] - 2, n3[0] - 2))
        mg = P.MultiGrid3D(ctx, n3, rng, np.float64, residual_mode=P.CORRECT)
        mg.upload_f(0, f)
        zero = np.zeros_like(f)
        for krylov in (True, False):
            best, res = 1e9, None
            for rep in range(1 + args.reps):
                mg.upload_v(0, zero)
                ctx.sync()
                t0 = time.perf_counter()
                res = mg.PCG(2, 2, 1e-10, 400, krylov=krylov)
                dt = time.perf_counter() - t0
                if rep:
                    best = min(best, dt)
            k, rel, conv, _ = res
            print("%-5s %s %s: %3d %s, true rel. residual %.2e, converged %d, %.1f ms (%.2f ms per iteration)" % (
                name, "x".join(map(str, n3)), "PCG  " if krylov else "plain", k, "iterations" if krylov else "cycles    ", rel,
                conv, best * 1e3, best * 1e3 / max(k, 1)), flush=True)
        mg.close()
    ctx.close()


if __name__ == "__main__":
    main()
