#!/usr/bin/python3
"""Workloads behind DESIGN.md 14 (the variable-coefficient operator), fp64 on the unit cube, the smooth coefficient
a = 1 + 0.5 sin(2 pi x) cos(pi y) + 0.25 z.

--mode kernels (for rocprofv3, counters off): on the same --n^3 arrays, in one process, alternating, --reps times each after
--warmup rounds: one sweep of mgx3dxs_relax_coef (two launches of the colour pass) with four and with two rows per lane
("relax3d.rows") against one sweep of mgx3dxs_relax_shift (two launches of the colour pass), then mgx3dxs_residual_coef
(r and the sum) and mgx3dxs_apply_coef_dot.  The kernels are the shared templates of csrc/mgx_stencil3d.hpp; the profiler lists
them as relax_op3d_xs_kernel<double, mgx::CoefOp<double>, 4, R> and <double, mgx::ShiftOp<double>, 4, 4>, and
residual_op3d_xs_kernel<double, mgx::CoefOp<double>, 1, false> (residual_coef) and <..., 1, true> (apply_coef_dot).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/coef_kernels.py --mode kernels

--mode cycles (profiler off; device events): V(2,2) of a hierarchy with the coefficient and of a shifted hierarchy of the same
size, shift and right-hand side, alternating; one BackwardEuler step (kappa = 1, dt = 1e-2, tol 1e-10) from
u = sin(pi x) sin(pi y) sin(pi z) with the smooth coefficient and with a jump of 10; the device memory the coefficient takes.
Prints one JSON line."""
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
    a[1:-1, 1:-1, 1:-1] = np.random.default_rng(seed).uniform(-1, 1, (n - 2,) * 3)
    return a


def smooth_coefficient(n):
    t = np.linspace(0.0, 1.0, n)
    return 1.0 + 0.5 * np.sin(2 * np.pi * t)[None, None, :] * np.cos(np.pi * t)[None, :, None] + 0.25 * t[:, None, None]


def jump_coefficient(n, jump):
    inside = np.abs(np.linspace(0.0, 1.0, n) - 0.5) < 0.25
    return np.where(inside[:, None, None] & inside[None, :, None] & inside[None, None, :], float(jump), 1.0)


def device_free_bytes():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


def kernels(args):
    n = args.n
    n3 = (n,) * 3
    ctx = P.Context(0)
    dev = {"v": ctx.to_device(P.xs_pack(interior_random(n, 0))), "f": ctx.to_device(P.xs_pack(interior_random(n, 1))),
           "a": ctx.to_device(P.xs_pack(smooth_coefficient(n))), "r": ctx.to_device(P.xs_pack(np.zeros((n, n, n))))}
    elems = P.lib.mgx3dxs_krylov_work_elems_f64
    elems.restype = C.c_size_t
    work, total = ctx.to_device(np.zeros(int(elems(_ip(n3))))), ctx.to_device(np.zeros(1))
    h = _rp(grid_spacing(n3, UNIT, np.float64), C.c_double)
    L, s = P.lib, C.c_double(args.shift)
    names = {}
    for _ in range(args.warmup + args.reps):
        for rows in (4, 2):
            ctx.set_param("relax3d.rows", rows)
            P.check(L.mgx3dxs_relax_coef_f64(ctx._h, dev["v"], dev["f"], dev["a"], _ip(n3), h, s, C.c_int(1)))
            names[rows] = ctx.last_relax_kernel()
        ctx.set_param("relax3d.rows", 4)
        P.check(L.mgx3dxs_relax_shift_f64(ctx._h, dev["v"], dev["f"], _ip(n3), h, s, C.c_int(1)))
        P.check(L.mgx3dxs_residual_coef_f64(ctx._h, dev["v"], dev["f"], dev["a"], dev["r"], _ip(n3), h, s, work, total))
        P.check(L.mgx3dxs_apply_coef_dot_f64(ctx._h, dev["v"], dev["a"], dev["r"], _ip(n3), h, s, work, total))
    ctx.sync()
    print(json.dumps({"mode": "kernels", "n": n, "shift": args.shift, "warmup": args.warmup, "reps": args.reps,
                      "coef_kernel_rows4": names[4], "coef_kernel_rows2": names[2], "shift_kernel": ctx.last_relax_kernel()}))
    for p in list(dev.values()) + [work, total]:
        ctx.free(p)
    ctx.close()


def cycles(args):
    n = args.n
    n3 = (n,) * 3
    ctx = P.Context(0)
    f = interior_random(n, 1)
    free0 = device_free_bytes()
    coef = P.MultiGrid3D(ctx, n3, UNIT, np.float64, residual_mode=P.CORRECT, shift=args.shift)
    free1 = device_free_bytes()
    coef.set_coefficient(smooth_coefficient(n))
    free2 = device_free_bytes()
    shifted = P.MultiGrid3D(ctx, n3, UNIT, np.float64, residual_mode=P.CORRECT, shift=args.shift)
    e0, e1 = ctx.event(), ctx.event()
    ms = {"coef": [], "shift": []}
    for mg in (coef, shifted):
        mg.upload_f(0, f)
    for rep in range(args.warmup + args.reps):
        for name, mg in (("coef", coef), ("shift", shifted)):
            ctx.record(e0)
            mg.VCycle(0, 2, 2)
            ctx.record(e1)
            ctx.sync()
            if rep >= args.warmup:
                ms[name].append(ctx.elapsed_ms(e0, e1))
    shifted.close()
    ax = np.sin(np.pi * np.linspace(0.0, 1.0, n))
    u = ax[:, None, None] * ax[None, :, None] * ax[None, None, :]
    u[0], u[-1], u[:, 0], u[:, -1], u[:, :, 0], u[:, :, -1] = 0, 0, 0, 0, 0, 0
    steps = {}
    for which, a in (("smooth", None), ("jump10", jump_coefficient(n, 10))):
        if a is not None:
            coef.set_coefficient(a)
        steps[which] = []
        for rep in range(1 + args.steps):  # the first step allocates the solver's scratch
            coef.upload_v(0, u)
            ctx.sync()
            ctx.record(e0)
            its, worst, conv = coef.BackwardEuler(1, 1e-2, 1.0, tol=1e-10)
            ctx.record(e1)
            ctx.sync()
            if rep:
                steps[which].append({"ms": ctx.elapsed_ms(e0, e1), "iterations": its, "rel_res": worst, "converged": conv})
    print(json.dumps({"mode": "cycles", "n": n, "shift": args.shift, "reps": args.reps, "vcycle22_ms_coef": float(np.mean(ms["coef"])),
                      "vcycle22_ms_shift": float(np.mean(ms["shift"])), "vcycle22_ms_coef_all": ms["coef"], "vcycle22_ms_shift_all": ms["shift"],
                      "backward_euler_steps": steps, "hierarchy_bytes": free0 - free1, "coefficient_bytes": free1 - free2}))
    coef.close()
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
