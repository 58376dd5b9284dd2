#!/usr/bin/python3
"""Device time of the vector passes of the mixed-precision solve (MultiGrid3D.PCG(precond="f32")) at 513^3, next to the fp64
passes they stand in for: CUDA-style events around N back-to-back launches each, the best of three rounds.  The arrays are
the levels-0 arrays of an fp64 and an fp32 hierarchy (x-split), so every pass streams the real geometry.  The fused
correction + residual + demote pass is timed for every rows-per-wave choice and against its two-launch form
(mixed3d.fused = 0, the default: a streaming correction, then the z-marching residual + demote).

    python tools/mixed_pass_time.py [--n 513] [--launches 20]

Algorithmic bytes per interior point are what the pass must move at least; TB/s and the share of 8 TB/s follow from them."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pde_multigrid_amd as P  # noqa: E402
from pde_multigrid_amd._lib import lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=513)
    ap.add_argument("--launches", type=int, default=20)
    args = ap.parse_args()
    n3 = (args.n,) * 3
    ctx = P.Context(0)
    m64 = P.MultiGrid3D(ctx, n3, [0, 1, 0, 1, 0, 1], np.float64, nlevels=1, residual_mode=P.CORRECT)
    m32 = P.MultiGrid3D(ctx, n3, [0, 1, 0, 1, 0, 1], np.float32, nlevels=1, residual_mode=P.CORRECT)
    g, t = m64.grid(0), m32.grid(0)
    x, xo, b, q = (C.c_void_p(a) for a in (g.d_v, g.d_e, g.d_f, g.d_r))
    z32, r32 = C.c_void_p(t.d_v), C.c_void_p(t.d_f)
    n = (C.c_int * 3)(*n3)
    h = (C.c_double * 3)(*([1.0 / (args.n - 1)] * 3))
    fn = lib.mgx3dxs_mixed_work_elems_f64
    fn.restype = C.c_size_t
    work = ctx.to_device(np.zeros(int(fn(n)), np.float64))
    dev = ctx.to_device(np.array([0.5, 0.25, 0, 0, 0, 0, 0, 0], np.float64))  # alpha, beta, sums
    alpha, beta, s0 = (C.c_void_p(dev.value + 8 * i) for i in (0, 1, 2))
    pts = float(args.n - 2) ** 3
    S, INV = C.c_double(2.0 ** 10), C.c_double(2.0 ** -10)
    passes = [
        ("correct_residual_demote (fused)", 32, [("mixed3d.fused", 1)], lambda: lib.mgx3dxs_correct_residual_demote_f64(ctx._h, x, xo, b, z32, INV, r32, S, n, h, work, s0)),
        ("correct_residual_demote (two launches)", 40, [],
         lambda: lib.mgx3dxs_correct_residual_demote_f64(ctx._h, x, xo, b, z32, INV, r32, S, n, h, work, s0)),
        ("residual_demote (no correction)", 20, None, lambda: lib.mgx3dxs_correct_residual_demote_f64(ctx._h, x, None, b, None, INV, r32, S, n, h, work, s0)),
        ("demote", 12, None, lambda: lib.mgx3dxs_demote_f64(ctx._h, b, r32, S, n)),
        ("cg_update_demote", 28, None, lambda: lib.mgx3dxs_cg_update_demote_f64(ctx._h, None, None, b, q, r32, S, n, alpha, work, s0)),
        ("dot2_mixed (two sums)", 20, None, lambda: lib.mgx3dxs_dot2_mixed_f64(ctx._h, z32, INV, b, q, n, work, s0)),
        ("cg_direction_mixed (x, beta)", 36, None, lambda: lib.mgx3dxs_cg_direction_mixed_f64(ctx._h, x, q, z32, INV, n, alpha, beta)),
        ("fp64 cg_update", 24, None, lambda: lib.mgx3dxs_cg_update_f64(ctx._h, None, None, b, q, n, alpha, work, s0)),
        ("fp64 dot2 (two sums)", 24, None, lambda: lib.mgx3dxs_dot2_f64(ctx._h, x, b, q, n, work, s0)),
        ("fp64 cg_direction (x, beta)", 40, None, lambda: lib.mgx3dxs_cg_direction_f64(ctx._h, x, q, xo, n, alpha, beta)),
        ("fp64 laplace_dot", 16, None, lambda: lib.mgx3dxs_laplace_dot_f64(ctx._h, x, q, n, h, work, s0)),
    ]
    for rows in (2, 8):
        passes.insert(1, ("correct_residual_demote (fused, %d rows per wave)" % rows, 32, [("mixed3d.fused", 1), ("mixed3d.rows", rows)],
                          lambda: lib.mgx3dxs_correct_residual_demote_f64(ctx._h, x, xo, b, z32, INV, r32, S, n, h, work, s0)))
    e0, e1 = ctx.event(), ctx.event()
    print("%d^3, %d launches per round, best of 3 rounds; %.4g interior points" % (args.n, args.launches, pts))
    for name, bpp, param, call in passes:
        for kv in param or []:
            ctx.set_param(*kv)
        P.check(call())
        best = 1e30
        for _ in range(3):
            ctx.record(e0)
            for _ in range(args.launches):
                P.check(call())
            ctx.record(e1)
            ctx.sync()
            best = min(best, ctx.elapsed_ms(e0, e1) / args.launches)
        for k, _ in param or []:
            ctx.set_param(k, {"mixed3d.fused": 0, "mixed3d.rows": 4}[k])  # the defaults
        tbs = bpp * pts / (best * 1e-3) / 1e12
        print("%-50s %7.3f ms  %2d B/pt  %5.2f GB  %5.2f TB/s  %.2f of 8 TB/s" % (name, best, bpp, bpp * pts / 1e9, tbs, tbs / 8), flush=True)
    ctx.free(work)
    ctx.free(dev)
    m64.close()
    m32.close()
    ctx.close()


if __name__ == "__main__":
    main()
