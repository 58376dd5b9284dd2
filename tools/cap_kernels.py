#!/usr/bin/python3
"""Workloads behind DESIGN.md 17 (the operator with a capacity), fp64 on the unit cube.

--mode kernels (for rocprofv3, counters off): on the same --n^3 arrays, in one process, alternating, --reps times each after
--warmup rounds: one sweep of mgx3dxs_relax_cap with four and with two rows per lane ("relax3d.rows": relax_op3d_xs_kernel<double,
CapOp, 4, 4> and <.., 4, 2>), the same two of mgx3dxs_relax_coef, and residual_cap / residual_coef with the sum.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/cap_kernels.py --mode kernels

--mode cycles (profiler off; device events): V(2,2) of one hierarchy with the smooth coefficient and shift 100, without a capacity,
with a smooth one and with one that jumps by 100, alternating; then one BackwardEuler step (kappa = 1, dt = 1e-2, tol 1e-10,
flexible CG) from a Gaussian for each of the three.  Prints one JSON line."""
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


def smooth_capacity(n):
    x, y, z = nodes(n)
    return 1.0 + 0.5 * np.cos(2 * np.pi * x) * np.sin(np.pi * z) + 0.25 * y


def block_capacity(n, inside):
    x, y, z = nodes(n)
    m = (np.abs(x - 0.5) < 0.25) & (np.abs(y - 0.5) < 0.25) & (np.abs(z - 0.5) < 0.25)
    return np.where(m, float(inside), 1.0)


def kernels(args):
    n = args.n
    n3 = (n,) * 3
    ctx = P.Context(0)
    g = np.random.default_rng(0)
    dev = {name: ctx.to_device(P.xs_pack(g.uniform(-1, 1, (n,) * 3))) for name in ("v", "f", "r")}
    dev["a"] = ctx.to_device(P.xs_pack(smooth_coefficient(n)))
    dev["c"] = ctx.to_device(P.xs_pack(smooth_capacity(n)))
    wfn = P.lib.mgx3dxs_krylov_work_elems_f64
    wfn.restype = C.c_size_t
    work, ssum = ctx.malloc(8 * int(wfn(_ip(n3)))), ctx.malloc(8)
    h = _rp(grid_spacing(n3, UNIT, np.float64), C.c_double)
    L, s = P.lib, C.c_double(args.shift)
    for _ in range(args.warmup + args.reps):
        for rows in (4, 2):
            ctx.set_param("relax3d.rows", rows)
            P.check(L.mgx3dxs_relax_cap_f64(ctx._h, dev["v"], dev["f"], dev["a"], dev["c"], _ip(n3), h, s, C.c_int(1)))
            P.check(L.mgx3dxs_relax_coef_f64(ctx._h, dev["v"], dev["f"], dev["a"], _ip(n3), h, s, C.c_int(1)))
        P.check(L.mgx3dxs_residual_cap_f64(ctx._h, dev["v"], dev["f"], dev["a"], dev["c"], dev["r"], _ip(n3), h, s, work, ssum))
        P.check(L.mgx3dxs_residual_coef_f64(ctx._h, dev["v"], dev["f"], dev["a"], dev["r"], _ip(n3), h, s, work, ssum))
    ctx.sync()
    print(json.dumps({"mode": "kernels", "n": n, "shift": args.shift, "warmup": args.warmup, "reps": args.reps}))
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
    caps = {"coef": None, "cap_smooth": smooth_capacity(n), "cap_jump100": block_capacity(n, 100)}
    mg = P.MultiGrid3D(ctx, n3, UNIT, np.float64, residual_mode=P.CORRECT, shift=100.0, coefficient=smooth_coefficient(n))
    mg.upload_f(0, f)
    ms = {k: [] for k in caps}
    for rep in range(args.warmup + args.reps):
        for name, c in caps.items():
            mg.set_capacity(c)
            ctx.sync()
            ctx.record(e0)
            mg.VCycle(0, 2, 2)
            ctx.record(e1)
            ctx.sync()
            if rep >= args.warmup:
                ms[name].append(ctx.elapsed_ms(e0, e1))
    for name in caps:
        out["vcycle22_ms_" + name], out["vcycle22_ms_%s_all" % name] = float(np.mean(ms[name])), ms[name]
    x, y, z = nodes(n)
    u = np.exp(-40 * ((x - 0.4) ** 2 + (y - 0.55) ** 2 + (z - 0.3) ** 2))
    u[0], u[-1], u[:, 0], u[:, -1], u[:, :, 0], u[:, :, -1] = 0, 0, 0, 0, 0, 0
    for name, c in caps.items():
        mg.set_capacity(c)
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
        out["backward_euler_" + name] = steps
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
