#!/usr/bin/python3
"""Workloads behind DESIGN.md 19 (harmonic-mean face coefficients), on the unit cube; device events, profiler off.

--mode passes: a hierarchy with harmonic and one with arithmetic faces of the same --n^3 size, coefficient (the smooth one of
DESIGN.md 14), shift and right-hand side, in one process, alternating, --reps times each after --warmup rounds: one Relax(0, 1)
(two launches of the colour pass: the reported time is per pass) and one VCycle(0, 2, 2), in fp64 and in fp32.  The colour passes
are relax_op3d_xs_kernel<real, mgx::HarmOp<real>, 4, R> and <real, mgx::CoefOp<real>, 4, R> of csrc/mgx_stencil3d.hpp.

--mode counts: at --n^3 (33 for the table of section 19), fp64, shift 0, a random right-hand side from a zero guess, the block that
jumps by 10 and by 1000: the V(2,2) cycles (PCG with krylov = 0) and the CG iterations (krylov = 1) to 1e-10 with either mean.

Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pde_multigrid_amd as P  # noqa: E402

UNIT = [0, 1, 0, 1, 0, 1]
MEANS = ("harmonic", "arithmetic")


def interior_random(n, seed, dtype=np.float64):
    a = np.zeros((n, n, n), dtype)
    a[1:-1, 1:-1, 1:-1] = np.random.default_rng(seed).uniform(-1, 1, (n - 2,) * 3)
    return a


def smooth_coefficient(n):
    t = np.linspace(0.0, 1.0, n)
    return 1.0 + 0.5 * np.sin(2 * np.pi * t)[None, None, :] * np.cos(np.pi * t)[None, :, None] + 0.25 * t[:, None, None]


def jump_coefficient(n, jump):
    inside = np.abs(np.linspace(0.0, 1.0, n) - 0.5) < 0.25
    return np.where(inside[:, None, None] & inside[None, :, None] & inside[None, None, :], float(jump), 1.0)


def passes(args):
    n = args.n
    n3 = (n,) * 3
    ctx = P.Context(0)
    out = {"mode": "passes", "n": n, "shift": args.shift, "warmup": args.warmup, "reps": args.reps}
    e0, e1 = ctx.event(), ctx.event()
    for dtype in (np.float64, np.float32):
        name = np.dtype(dtype).name
        f, a = interior_random(n, 1, dtype), smooth_coefficient(n).astype(dtype)
        mgs = {m: P.MultiGrid3D(ctx, n3, UNIT, dtype, residual_mode=P.CORRECT, shift=args.shift, coefficient=a, face_mean=m) for m in MEANS}
        for mg in mgs.values():
            mg.upload_f(0, f)
        ms = {(m, what): [] for m in MEANS for what in ("pass", "vcycle22")}
        kernels = {}
        for rep in range(args.warmup + args.reps):
            for what, run in (("pass", lambda mg: mg.Relax(0, 1)), ("vcycle22", lambda mg: mg.VCycle(0, 2, 2))):
                for m in MEANS:
                    ctx.record(e0)
                    run(mgs[m])
                    ctx.record(e1)
                    ctx.sync()
                    if what == "pass":
                        kernels[m] = ctx.last_relax_kernel()
                    if rep >= args.warmup:
                        ms[(m, what)].append(ctx.elapsed_ms(e0, e1) / (2 if what == "pass" else 1))
        for m in MEANS:
            out["%s_%s_kernel" % (name, m)] = kernels[m]
            for what in ("pass", "vcycle22"):
                t = ms[(m, what)]
                out["%s_%s_%s_ms" % (name, m, what)] = {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))}
        for mg in mgs.values():
            mg.close()
    ctx.close()
    print(json.dumps(out))


def counts(args):
    n = args.n
    n3 = (n,) * 3
    ctx = P.Context(0)
    f = interior_random(n, 3)
    out = {"mode": "counts", "n": n, "tol": 1e-10, "maxit": args.maxit}
    for jump in (10, 1000):
        a = jump_coefficient(n, jump)
        for m in MEANS:
            for krylov in (False, True):
                mg = P.MultiGrid3D(ctx, n3, UNIT, np.float64, residual_mode=P.CORRECT, coefficient=a, face_mean=m)
                mg.upload_f(0, f)
                k, rel, conv, _ = mg.PCG(2, 2, 1e-10, args.maxit, krylov=krylov)
                out["jump%d_%s_%s" % (jump, m, "cg" if krylov else "vcycles")] = {"iterations": k, "rel_res": rel, "converged": conv}
                mg.close()
    ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("passes", "counts"), default="passes")
    ap.add_argument("--n", type=int, default=513)
    ap.add_argument("--shift", type=float, default=100.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--maxit", type=int, default=100)
    args = ap.parse_args()
    (passes if args.mode == "passes" else counts)(args)


if __name__ == "__main__":
    main()
