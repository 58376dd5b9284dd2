#!/usr/bin/python3
"""Workloads behind DESIGN.md 16 (flexible CG in the weighted inner product on hierarchies with Neumann faces), fp64, unit cube.

--mode kernels (for rocprofv3, counters off): on the same --n^3 arrays, in one process, --reps rounds after --warmup: the vector
entries of one CG iteration with bc = 63 -- laplace_dot_shift_bc, apply_coef_dot_bc, cg_update_bc, dot2_bc (two sums),
cg_direction_bc (x and p) -- and project_bc; each is its interior launch followed by its launch over the face unknowns.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/neumann_krylov.py --mode kernels

--mode solves (profiler off): at --n^3 from a random guess and right-hand side, V(2,2), tol 1e-10: PCG(krylov = 2) against
PCG(krylov = 0, at most 60 cycles) in the closed box with shift 1, without a coefficient and with a jump of 1000; the closed box
without a shift (the projected solve); and the vector entries of one iteration outside the V-cycle (apply, update, two dots,
direction) with bc = 63 and with bc = 0, by device events.  Every solve runs twice, the second is reported.  One JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

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


def jump_coefficient(n, jump):
    x, y, z = nodes(n)
    return np.where((np.abs(x - 0.5) < 0.25) & (np.abs(y - 0.5) < 0.25) & (np.abs(z - 0.5) < 0.25), float(jump), 1.0)


class Vectors:
    """the device arrays, work array and scalars of the vector entries on an n^3 grid"""

    def __init__(self, ctx, n, coef):
        self.ctx, self.n3 = ctx, (n,) * 3
        g = np.random.default_rng(0)
        self.dev = {name: ctx.to_device(P.xs_pack(g.uniform(-1, 1, (n,) * 3))) for name in ("x", "p", "q", "r", "z")}
        if coef:
            self.dev["a"] = ctx.to_device(P.xs_pack(smooth_coefficient(n)))
        wfn = P.lib.mgx3dxs_krylov_work_elems_bc_f64
        wfn.restype = C.c_size_t
        self.work, self.sums = ctx.malloc(8 * int(wfn(_ip(self.n3)))), ctx.malloc(16)
        self.scal = ctx.to_device(np.array([1e-3, 0.5]))
        self.alpha, self.beta = self.scal, C.c_void_p(self.scal.value + 8)
        self.h = _rp(grid_spacing(self.n3, UNIT, np.float64), C.c_double)

    def iteration(self, bc, s):
        """the vector entries of one iteration outside the V-cycle, as pcg_krylov3_ calls them"""
        L, d, n, b = P.lib, self.dev, _ip(self.n3), C.c_int(bc)
        P.check(L.mgx3dxs_laplace_dot_shift_bc_f64(self.ctx._h, d["p"], d["q"], n, self.h, C.c_double(s), self.work, self.sums, b))
        P.check(L.mgx3dxs_cg_update_bc_f64(self.ctx._h, None, d["p"], d["r"], d["q"], n, self.alpha, self.work, self.sums, b))
        P.check(L.mgx3dxs_dot2_bc_f64(self.ctx._h, d["z"], d["r"], d["q"], n, self.work, self.sums, b))
        P.check(L.mgx3dxs_cg_direction_bc_f64(self.ctx._h, d["x"], d["p"], d["z"], n, self.alpha, self.beta, b))

    def close(self):
        for p in list(self.dev.values()) + [self.work, self.sums, self.scal]:
            self.ctx.free(p)


def kernels(args):
    ctx = P.Context(0)
    v = Vectors(ctx, args.n, True)
    L, d, n = P.lib, v.dev, _ip(v.n3)
    for _ in range(args.warmup + args.reps):
        v.iteration(63, args.shift)
        P.check(L.mgx3dxs_apply_coef_dot_bc_f64(ctx._h, d["p"], d["a"], d["q"], n, v.h, C.c_double(args.shift), v.work, v.sums, C.c_int(63)))
        P.check(L.mgx3dxs_project_bc_f64(ctx._h, d["z"], n, v.work, v.sums, C.c_int(63)))
    ctx.sync()
    print(json.dumps({"mode": "kernels", "n": args.n, "shift": args.shift, "warmup": args.warmup, "reps": args.reps,
                      "face_points_share": 6.0 * args.n ** 2 / args.n ** 3}))
    v.close()
    ctx.close()


def solves(args):
    n = args.n
    n3 = (n,) * 3
    ctx = P.Context(0)
    g = np.random.default_rng(11)
    v0, f = g.uniform(-1, 1, (n,) * 3), g.uniform(-1, 1, (n,) * 3)
    out = {"mode": "solves", "n": n, "tol": 1e-10, "cycle": "V(2,2)"}

    def solve(mg, krylov, maxit):
        res = None
        for rep in range(2):  # the first call allocates the solver's scratch
            mg.upload_v(0, v0)
            ctx.sync()
            t0 = time.perf_counter()
            k, rel, conv, _ = mg.PCG(2, 2, 1e-10, maxit, krylov=krylov)  # blocking
            res = {"ms": 1e3 * (time.perf_counter() - t0), "iterations": k, "rel_res": rel, "converged": conv}
        return res

    for name, s, a in (("closed_s1", 1.0, None), ("closed_s1_jump1000", 1.0, jump_coefficient(n, 1000)), ("closed_s0_singular", 0.0, None)):
        mg = P.MultiGrid3D(ctx, n3, UNIT, np.float64, residual_mode=P.CORRECT, shift=s, coefficient=a, neumann=[1] * 6)
        mg.upload_f(0, f)
        out[name + "_weighted_cg"] = solve(mg, "weighted", 100)
        if s:
            out[name + "_plain_cycling"] = solve(mg, False, 60)
        else:
            out[name + "_removed_mean"] = mg.pcg_removed_mean
        mg.close()
    # the same solve without walls: krylov = 2 runs krylov = 1's launches
    mg = P.MultiGrid3D(ctx, n3, UNIT, np.float64, residual_mode=P.CORRECT, shift=1.0)
    mg.upload_f(0, f)
    out["dirichlet_s1_cg"] = solve(mg, "weighted", 100)
    mg.close()
    v = Vectors(ctx, n, False)
    e0, e1 = ctx.event(), ctx.event()
    for bc in (63, 0):
        ms = []
        for rep in range(args.warmup + args.reps):
            ctx.record(e0)
            v.iteration(bc, 1.0)
            ctx.record(e1)
            ctx.sync()
            if rep >= args.warmup:
                ms.append(ctx.elapsed_ms(e0, e1))
        out["iteration_outside_vcycle_ms_bc%d" % bc] = float(np.mean(ms))
        out["iteration_outside_vcycle_ms_bc%d_all" % bc] = ms
    v.close()
    print(json.dumps(out))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernels", "solves"), default="kernels")
    ap.add_argument("--n", type=int, default=513)
    ap.add_argument("--shift", type=float, default=100.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    (kernels if args.mode == "kernels" else solves)(args)


if __name__ == "__main__":
    main()
