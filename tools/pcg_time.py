#!/usr/bin/python3
"""Wall time of MultiGrid3D.PCG against plain V(2,2) cycling (krylov=False), both to a true relative residual of 1e-10, fp64,
on the isotropic 513^3 unit cube and on 513x513x257 with z in [0, 4] (random interior right-hand side, zero guess).  Each
solve runs once untimed (allocations, first-use paths) and is then timed from a synchronised start to its return.

    python tools/pcg_time.py [--only iso|aniso] [--reps N] [--precond f64|f32|both] [--semi]

--precond f32 times the mixed-precision solves (fp32 V-cycle, PCG(precond="f32")) instead, both times fp64 and mixed
alternately in one process (each repetition runs every variant once, so drifts of the clock hit all of them alike).

--semi runs every solve on the semi-coarsened hierarchy too (MultiGrid3D(coarsening="semi")), after the
full-coarsening one in the same process, and prints the device memory both hierarchies' level arrays take.

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
    ap.add_argument("--precond", choices=["f64", "f32", "both"], default="f64")
    ap.add_argument("--semi", action="store_true", help="also the semi-coarsened hierarchy")
    args = ap.parse_args()
    ctx = P.Context(0)
    for name, (n3, rng) in CASES.items():
        if args.only and name != args.only:
            continue
        f = np.zeros(n3[::-1])
        f[1:-1, 1:-1, 1:-1] = np.random.default_rng(0).uniform(-1, 1, (n3[2] - 2, n3[1] - 2, n3[0] - 2))
        zero = np.zeros_like(f)
        precs = {"f64": ["f64"], "f32": ["f32"], "both": ["f64", "f32"]}[args.precond]
        for how in (("full", "semi") if args.semi else ("full",)):
            mg = P.MultiGrid3D(ctx, n3, rng, np.float64, residual_mode=P.CORRECT, coarsening=how)
            mg.upload_f(0, f)
            if args.semi:
                elems = sum(4 * P.xs_geometry(mg.size(l)[0], 8)[1] * mg.size(l)[1] * mg.size(l)[2] for l in range(mg.maxGrids))
                print("%-5s %s %s coarsening: %d levels, masks %s, level arrays %.1f MiB" % (
                    name, "x".join(map(str, n3)), how, mg.maxGrids, " ".join(map(str, mg.masks[:-1])), elems * 8 / 2**20), flush=True)
            time_solves(ctx, mg, name + ("/" + how if args.semi else ""), n3, zero, precs, args.reps)
            mg.close()
    ctx.close()


def time_solves(ctx, mg, name, n3, zero, precs, reps):
    for krylov in (True, False):
        best, res = {p: 1e9 for p in precs}, {}
        for rep in range(1 + reps):
            for prec in precs:
                mg.upload_v(0, zero)
                ctx.sync()
                t0 = time.perf_counter()
                res[prec] = mg.PCG(2, 2, 1e-10, 400, krylov=krylov, precond=prec)
                dt = time.perf_counter() - t0
                if rep:
                    best[prec] = min(best[prec], dt)
        for prec in precs:
            k, rel, conv, _ = res[prec]
            label = ("PCG  " if krylov else "plain") if prec == "f64" else ("mixed PCG" if krylov else "mixed IR ")
            print("%-5s %s %s: %3d %s, true rel. residual %.2e, converged %d, %.1f ms (%.2f ms per iteration)" % (
                name, "x".join(map(str, n3)), label, k, "iterations" if krylov or prec == "f32" else "cycles    ", rel,
                conv, best[prec] * 1e3, best[prec] * 1e3 / max(k, 1)), flush=True)
        if len(precs) == 2:
            print("%-5s %s: mixed / fp64 wall time %.3f" % (name, "PCG  " if krylov else "plain", best["f32"] / best["f64"]), flush=True)


if __name__ == "__main__":
    main()
