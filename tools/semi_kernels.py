#!/usr/bin/python3
"""Workload for rocprofv3: the two hot transfers of a semi-coarsened step with mask 3 (x and y halved, z kept) on a
513 x 513 x 257 fp64 fine level -- mgx3dxs_residual_restrict_axes / mgx3dxs_interpolate_correct_axes onto 257 x 257 x 257 --
against the full-coarsening pair on the same fine arrays in the same process (mgx3dxs_residual_restrict_keep_rim /
mgx3dxs_interpolate_correct onto 257 x 257 x 129), alternating, --reps times each.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/semi_kernels.py [--reps N] [--unit]

--unit: z in [0, 1] instead of [0, 4] (all spacings powers of two: the exact-reciprocal form of the residual)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pde_multigrid_amd as P  # noqa: E402
from pde_multigrid_amd.multigrid import _ip, _rp, grid_spacing  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--unit", action="store_true")
    args = ap.parse_args()
    n3, semi, full = (513, 513, 257), (257, 257, 257), (257, 257, 129)
    rng = [0, 1, 0, 1, 0, 1 if args.unit else 4]
    ctx = P.Context(0)
    r = np.random.default_rng(0)
    dev = {}
    for name, n in (("v", n3), ("f", n3), ("cs", semi), ("cf", full)):
        a = np.zeros(n[::-1])
        a[1:-1, 1:-1, 1:-1] = r.uniform(-1, 1, (n[2] - 2, n[1] - 2, n[0] - 2))  # zero boundary: the rim may be kept
        dev[name] = ctx.to_device(P.xs_pack(a))
    h = _rp(grid_spacing(n3, rng, np.float64), C.c_double)
    L = P.lib
    for _ in range(args.reps):
        P.check(L.mgx3dxs_residual_restrict_axes_f64(ctx._h, dev["v"], dev["f"], _ip(n3), h, C.c_int(P.CORRECT), dev["cs"], _ip(semi), C.c_int(1)))
        P.check(L.mgx3dxs_residual_restrict_keep_rim_f64(ctx._h, dev["v"], dev["f"], _ip(n3), h, C.c_int(P.CORRECT), dev["cf"], _ip(full)))
        P.check(L.mgx3dxs_interpolate_correct_axes_f64(ctx._h, dev["v"], _ip(n3), dev["cs"], _ip(semi)))
        P.check(L.mgx3dxs_interpolate_correct_f64(ctx._h, dev["v"], _ip(n3), dev["cf"], _ip(full)))
    ctx.sync()
    for p in dev.values():
        ctx.free(p)
    ctx.close()


if __name__ == "__main__":
    main()
