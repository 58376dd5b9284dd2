#!/usr/bin/python3
"""Workloads behind DESIGN.md 15 (homogeneous Neumann faces), fp64 on the unit cube.

--mode kernels (for rocprofv3, counters off): on the same --n^3 arrays, in one process, alternating, --reps times each after
--warmup rounds: one sweep of mgx3dxs_relax_shift_bc with bc = 63 (per colour the interior launch relax_op3d_xs_kernel<double,
ShiftOp, 4, 4> and the face launch face_relax3d_xs_kernel<double, ShiftOp>), one with bc = 0 (the interior launches alone),
the same two with mgx3dxs_relax_coef_bc, and residual_shift_bc / restrict_bc / interpolate_correct_bc with bc = 63.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/neumann_kernels.py --mode kernels

--mode cycles (profiler off; device events): V(2,2) of one hierarchy with shift 100 in a closed box (all six faces Neumann) and
with the mask cleared, alternating, the same with the smooth coefficient, and one BackwardEuler step (kappa = 1, dt = 1e-2, tol
1e-10, plain cycling) in the closed box from a Gaussian.  Prints one JSON line."""
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


def nodes(n):
    z, y, x = np.meshgrid(*(np.linspace(0.0, 1.0, n),) * 3, indexing="ij")
    return x, y, z


def smooth_coefficient(n):
    x, y, z = nodes(n)
    return 1.0 + 0.5 * np.sin(2 * np.pi * x) * np.cos(np.pi * y) + 0.25 * z


def kernels(args):
    n, cn = args.n, (args.n - 1) // 2 + 1
    n3, c3 = (n,) * 3, (cn,) * 3
    ctx = P.Context(0)
    g = np.random.default_rng(0)
    dev = {name: ctx.to_device(P.xs_pack(g.uniform(-1, 1, (k,) * 3))) for name, k in (("v", n), ("f", n), ("r", n), ("c", cn))}
    dev["a"] = ctx.to_device(P.xs_pack(smooth_coefficient(n)))
    wfn = P.lib.mgx3dxs_krylov_work_elems_f64
    wfn.restype = C.c_size_t
    work, ssum = ctx.malloc(8 * int(wfn(_ip(n3)))), ctx.malloc(8)
    h = _rp(grid_spacing(n3, UNIT, np.float64), C.c_double)
    L, s = P.lib, C.c_double(args.shift)
    for _ in range(args.warmup + args.reps):
        for bc in (63, 0):
            P.check(L.mgx3dxs_relax_shift_bc_f64(ctx._h, dev["v"], dev["f"], _ip(n3), h, s, C.c_int(1), C.c_int(bc)))
            P.check(L.mgx3dxs_relax_coef_bc_f64(ctx._h, dev["v"], dev["f"], dev["a"], _ip(n3), h, s, C.c_int(1), C.c_int(bc)))
        P.check(L.mgx3dxs_residual_shift_bc_f64(ctx._h, dev["v"], dev["f"], dev["r"], _ip(n3), h, s, work, ssum, C.c_int(63)))
        P.check(L.mgx3dxs_restrict_bc_f64(ctx._h, dev["r"], _ip(n3), dev["c"], _ip(c3), C.c_int(63)))
        P.check(L.mgx3dxs_interpolate_correct_bc_f64(ctx._h, dev["v"], _ip(n3), dev["c"], _ip(c3), C.c_int(63)))
    ctx.sync()
    print(json.dumps({"mode": "kernels", "n": n, "shift": args.shift, "warmup": args.warmup, "reps": args.reps,
                      "face_points_share": 6.0 * n * n / n ** 3}))
    for p in list(dev.values()) + [work, ssum]:
        ctx.free(p)
    ctx.close()


def cycles(args):
    n = args.n
    n3 = (n,) * 3
    ctx = P.Context(0)
    f = np.random.default_rng(1).uniform(-1, 1, (n,) * 3)
    e0, e1 = ctx.event(), ctx.event()
    out = {"mode": "cycles", "n": n, "reps": args.reps}
    for name, a in (("shift", None), ("coef", smooth_coefficient(n))):
        mg = P.MultiGrid3D(ctx, n3, UNIT, np.float64, residual_mode=P.CORRECT, shift=100.0, coefficient=a)
        mg.upload_f(0, f)
        ms = {63: [], 0: []}
        for rep in range(args.warmup + args.reps):
            for bc in (63, 0):
                mg.set_neumann([(bc >> k) & 1 for k in range(6)])
                ctx.record(e0)
                mg.VCycle(0, 2, 2)
                ctx.record(e1)
                ctx.sync()
                if rep >= args.warmup:
                    ms[bc].append(ctx.elapsed_ms(e0, e1))
        out["vcycle22_ms_%s_bc63" % name] = float(np.mean(ms[63]))
        out["vcycle22_ms_%s_bc0" % name] = float(np.mean(ms[0]))
        out["vcycle22_ms_%s_bc63_all" % name], out["vcycle22_ms_%s_bc0_all" % name] = ms[63], ms[0]
        if a is None:
            x, y, z = nodes(n)
            u = np.exp(-40 * ((x - 0.4) ** 2 + (y - 0.55) ** 2 + (z - 0.3) ** 2))
            mg.set_neumann([1] * 6)
            steps = []
            for rep in range(1 + args.steps):  # the first step allocates the solver's scratch
                mg.upload_v(0, u)
                ctx.sync()
                ctx.record(e0)
                its, worst, conv = mg.BackwardEuler(1, 1e-2, 1.0, tol=1e-10, krylov=False)
                ctx.record(e1)
                ctx.sync()
                if rep:
                    steps.append({"ms": ctx.elapsed_ms(e0, e1), "cycles": its, "rel_res": worst, "converged": conv})
            out["backward_euler_steps"] = steps
        mg.close()
    print(json.dumps(out))
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
