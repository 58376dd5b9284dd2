#!/usr/bin/python3
"""Workloads behind DESIGN.md 18 (convective and prescribed-flux walls), fp64 on the unit cube, mask 63.

--mode kernels (for rocprofv3, counters off): on the same --n^3 arrays, in one process, alternating, --reps times each after
--warmup rounds: one sweep of mgx3dxs_relax_shift_wall with beta = 1 on every face (per colour the interior launch and the launch
over the face unknowns, face_relax3d_xs_kernel<double, ShiftOp>) and one of mgx3dxs_relax_shift_bc (the same two launches with
six zero diagonals); the same pair with the coefficient entries; residual_shift_wall and residual_shift_bc
(face_residual3d_xs_kernel); and wall_rhs.  One kernel serves a round's _wall call and its _bc call: in the trace the launches
of a colour pass alternate in pairs, _wall first, those of the residual one by one.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/wall_kernels.py --mode kernels

--mode cycles (profiler off; device events): V(2,2) of one hierarchy with shift 100 in the closed box with beta = 1 on every face
and with beta = 0, alternating (set_wall between them), the same with the smooth coefficient, and BackwardEuler steps (kappa = 1,
dt = 1e-2, tol 1e-10, plain cycling) from a Gaussian with beta = 1, g = 1 and with neither.  Prints one JSON line."""
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
ONES, ZEROS = (1.0,) * 6, (0.0,) * 6


def nodes(n):
    z, y, x = np.meshgrid(*(np.linspace(0.0, 1.0, n),) * 3, indexing="ij")
    return x, y, z


def smooth_coefficient(n):
    x, y, z = nodes(n)
    return 1.0 + 0.5 * np.sin(2 * np.pi * x) * np.cos(np.pi * y) + 0.25 * z


def kernels(args):
    n = args.n
    n3 = (n,) * 3
    ctx = P.Context(0)
    g = np.random.default_rng(0)
    dev = {name: ctx.to_device(P.xs_pack(g.uniform(-1, 1, n3))) for name in ("v", "f", "r")}
    dev["a"] = ctx.to_device(P.xs_pack(smooth_coefficient(n)))
    wfn = P.lib.mgx3dxs_krylov_work_elems_bc_f64
    wfn.restype = C.c_size_t
    work, ssum = ctx.malloc(8 * int(wfn(_ip(n3)))), ctx.malloc(8)
    h = _rp(grid_spacing(n3, UNIT, np.float64), C.c_double)
    L, s, bc, one = P.lib, C.c_double(args.shift), C.c_int(63), C.c_int(1)
    beta, flux = _rp(ONES, C.c_double), _rp((1e-3,) * 6, C.c_double)
    for _ in range(args.warmup + args.reps):
        P.check(L.mgx3dxs_relax_shift_wall_f64(ctx._h, dev["v"], dev["f"], _ip(n3), h, s, one, bc, beta))
        P.check(L.mgx3dxs_relax_shift_bc_f64(ctx._h, dev["v"], dev["f"], _ip(n3), h, s, one, bc))
        P.check(L.mgx3dxs_relax_coef_wall_f64(ctx._h, dev["v"], dev["f"], dev["a"], _ip(n3), h, s, one, bc, beta))
        P.check(L.mgx3dxs_relax_coef_bc_f64(ctx._h, dev["v"], dev["f"], dev["a"], _ip(n3), h, s, one, bc))
        P.check(L.mgx3dxs_residual_shift_wall_f64(ctx._h, dev["v"], dev["f"], dev["r"], _ip(n3), h, s, work, ssum, bc, beta))
        P.check(L.mgx3dxs_residual_shift_bc_f64(ctx._h, dev["v"], dev["f"], dev["r"], _ip(n3), h, s, work, ssum, bc))
        P.check(L.mgx3dxs_wall_rhs_f64(ctx._h, dev["f"], _ip(n3), h, flux, bc))
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
    f = np.random.default_rng(1).uniform(-1, 1, n3)
    e0, e1 = ctx.event(), ctx.event()
    out = {"mode": "cycles", "n": n, "reps": args.reps}
    for name, a in (("shift", None), ("coef", smooth_coefficient(n))):
        mg = P.MultiGrid3D(ctx, n3, UNIT, np.float64, residual_mode=P.CORRECT, shift=100.0, coefficient=a, neumann=[1] * 6)
        mg.upload_f(0, f)
        ms = {"wall": [], "bc": []}
        for rep in range(args.warmup + args.reps):
            for key, beta in (("wall", ONES), ("bc", ZEROS)):
                mg.set_wall(beta, None)
                ctx.record(e0)
                mg.VCycle(0, 2, 2)
                ctx.record(e1)
                ctx.sync()
                if rep >= args.warmup:
                    ms[key].append(ctx.elapsed_ms(e0, e1))
        for key in ms:
            out["vcycle22_ms_%s_%s" % (name, key)] = float(np.mean(ms[key]))
            out["vcycle22_ms_%s_%s_all" % (name, key)] = ms[key]
        if a is None:
            x, y, z = nodes(n)
            u = np.exp(-40 * ((x - 0.4) ** 2 + (y - 0.55) ** 2 + (z - 0.3) ** 2))
            for key, beta, g in (("wall", ONES, ONES), ("bc", ZEROS, ZEROS)):
                mg.set_wall(beta, g)
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
                out["backward_euler_steps_%s" % key] = steps
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
