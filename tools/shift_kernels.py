#!/usr/bin/python3
"""Workloads behind DESIGN.md 13 (the shifted operator), fp64 on the unit cube.

--mode kernels (for rocprofv3, counters off): on the same --n^3 arrays, in one process, alternating, --reps times each after
--warmup rounds: one sweep of mgx3dxs_relax_shift (two launches of the colour pass of csrc/mgx_stencil3d.hpp, which the
profiler lists as relax_op3d_xs_kernel<double, mgx::ShiftOp<double>, 4, 4>) against one sweep of the plain mgx3dxs_relax (two
colour passes of whichever kernel the level takes), and mgx3dxs_residual_restrict_shift against
mgx3dxs_residual_restrict_keep_rim.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/shift_kernels.py --mode kernels

--mode cycles (profiler off; device events): V(2,2) of one hierarchy with shift 100 and with shift 0, alternating, and one
BackwardEuler step (kappa = 1, dt = 1e-2, tol 1e-10) from u = sin(pi x) sin(pi y) sin(pi z).  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pde_multigrid_amd as P  # noqa: E402
from pde_multigrid_amd.multigrid import _ip, _rp, grid_spacing  # noqa: E402

UNIT = [0, 1, 0, 1, 0, 1]


def interior_random(n, seed):
    a = np.zeros((n, n, n))
    a[1:-1, 1:-1, 1:-1] = np.random.default_rng(seed).uniform(-1, 1, (n - 2,) * 3)  # zero boundary: the coarse rim may be kept
    return a


def kernels(args):
    n, cn = args.n, (args.n - 1) // 2 + 1
    n3, c3 = (n,) * 3, (cn,) * 3
    ctx = P.Context(0)
    dev = {name: ctx.to_device(P.xs_pack(interior_random(k, seed))) for seed, (name, k) in enumerate((("v", n), ("f", n), ("c", cn)))}
    h = _rp(grid_spacing(n3, UNIT, np.float64), C.c_double)
    L, s = P.lib, C.c_double(args.shift)
    for _ in range(args.warmup + args.reps):
        P.check(L.mgx3dxs_relax_shift_f64(ctx._h, dev["v"], dev["f"], _ip(n3), h, s, C.c_int(1)))
        P.check(L.mgx3dxs_relax_f64(ctx._h, dev["v"], dev["f"], _ip(n3), h, C.c_int(1)))
        P.check(L.mgx3dxs_residual_restrict_shift_f64(ctx._h, dev["v"], dev["f"], _ip(n3), h, s, dev["c"], _ip(c3), C.c_int(1)))
        P.check(L.mgx3dxs_residual_restrict_keep_rim_f64(ctx._h, dev["v"], dev["f"], _ip(n3), h, C.c_int(P.CORRECT), dev["c"], _ip(c3)))
    ctx.sync()
    print(json.dumps({"mode": "kernels", "n": n, "shift": args.shift, "warmup": args.warmup, "reps": args.reps,
                      "plain_relax_kernel": ctx.last_relax_kernel()}))
    for p in dev.values():
        ctx.free(p)
    ctx.close()


def cycles(args):
    n = args.n
    n3 = (n,) * 3
    ctx = P.Context(0)
    mg = P.MultiGrid3D(ctx, n3, UNIT, np.float64, residual_mode=P.CORRECT)
    mg.upload_f(0, interior_random(n, 1))
    e0, e1 = ctx.event(), ctx.event()
    ms = {100.0: [], 0.0: []}
    for rep in range(args.warmup + args.reps):
        for s in (100.0, 0.0):
            mg.shift = s
            ctx.record(e0)
            mg.VCycle(0, 2, 2)
            ctx.record(e1)
            ctx.sync()
            if rep >= args.warmup:
                ms[s].append(ctx.elapsed_ms(e0, e1))
    ax = np.sin(np.pi * np.linspace(0.0, 1.0, n))
    u = ax[:, None, None] * ax[None, :, None] * ax[None, None, :]
    u[0], u[-1], u[:, 0], u[:, -1], u[:, :, 0], u[:, :, -1] = 0, 0, 0, 0, 0, 0
    steps = []
    for rep in range(1 + args.steps):  # the first step allocates the solver's scratch
        mg.upload_v(0, u)
        ctx.sync()
        ctx.record(e0)
        its, worst, conv = mg.BackwardEuler(1, 1e-2, 1.0, tol=1e-10)
        ctx.record(e1)
        ctx.sync()
        if rep:
            steps.append({"ms": ctx.elapsed_ms(e0, e1), "iterations": its, "rel_res": worst, "converged": conv})
    print(json.dumps({"mode": "cycles", "n": n, "reps": args.reps, "vcycle22_ms_shift100": float(np.mean(ms[100.0])),
                      "vcycle22_ms_shift0": float(np.mean(ms[0.0])), "vcycle22_ms_shift100_all": ms[100.0], "vcycle22_ms_shift0_all": ms[0.0],
                      "backward_euler_steps": steps}))
    mg.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernels", "cycles"), default="kernels")
    ap.add_argument("--n", type=int, default=513)
    ap.add_argument("--shift", type=float, default=100.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=2)
    args = ap.parse_args()
    (kernels if args.mode == "kernels" else cycles)(args)


if __name__ == "__main__":
    main()
