#!/usr/bin/python3
"""Wall time of MultiGrid3D.Eigen (LOBPCG preconditioned by V(2,2)) on the unit cube, fp64, k = 4, tol = 1e-8, at
257^3 and 513^3: iterations, time per iteration, and that time split into its three parts, each timed on its own with the launches
an iteration makes --

  the k V-cycles             k x VCycle(0, 2, 2) of the hierarchy
  the k operator applications  k x mgx3dxs_laplace_dot_f64 on level-0 arrays
  the block kernels          the Gram tiles of the 3k-vector basis (block_gram), the combinations (block_combine), the residuals
                             (block_residual) and the 2k array copies in and out of the preconditioner

-- with the words per point the block kernels stream (distinct arrays per launch: a diagonal tile of S^T W c S passes one group
twice, as the solver does) and their rate, printed next to the 2R+1W streaming ceiling `tools/membench` measures on the device
(5.9 TB/s).  Reported only: nothing is asserted.

    python tools/eigen_time.py [--sizes 257 513] [--k 4] [--reps 2] [--graph]

Under rocprofv3 --kernel-trace --stats the kernel table gives each kernel's time per launch."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pde_multigrid_amd as P  # noqa: E402
from pde_multigrid_amd.multigrid import _ip, _rp, grid_spacing  # noqa: E402

RNG = [0, 1, 0, 1, 0, 1]
TRIAD_TBS = 5.9  # the 2R+1W triad of tools/membench on an MI355X (profiles/r01_membench_hbm_ceilings.txt)
lib = P.lib


def timed(ctx, fn, reps):
    best = 1e9
    for rep in range(1 + reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        if rep:
            best = min(best, time.perf_counter() - t0)
    return best


def block_launches(k):
    """the block launches of one iteration with P in the basis: (gram pairs (nu, nv), combinations (nin, nout), residual groups)"""
    m = 3 * k
    groups = [min(4, m - 4 * g) for g in range((m + 3) // 4)]
    # S^T W A S: a group of S against a group of A S; S^T W c S: two groups of S, the same one twice on the diagonal tiles
    pairs = [(a, b) for a in range(len(groups)) for b in range(a, len(groups))]
    grams = [(groups[a], groups[b], False) for a, b in pairs] + [(groups[a], groups[b], a == b) for a, b in pairs]
    outs = [min(4, k - o) for o in range(0, k, 4)]
    combos = []
    for no in outs:
        for _ in range(2):  # the vectors and their images
            combos += chunks(2 * k, no, False) + chunks(k, no, True)  # N1 = [T, P] [Yt; Yp]; X Yx + N1
    return grams, combos, outs


def chunks(nin, no, add):
    """the launches of one output group: at most 12 inputs each, the group's own partial results among them"""
    out, first = [], True
    while nin > 0 or first:
        own = no if (add or not first) else 0
        take = min(nin, 12 - own)
        out.append((own + take, no))
        nin -= take
        first = False
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[257, 513])
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--graph", action="store_true", help="replay the preconditioning cycle as a captured graph")
    args = ap.parse_args()
    k = args.k
    ctx = P.Context(0)
    for n in args.sizes:
        n3 = (n, n, n)
        mg = P.MultiGrid3D(ctx, n3, RNG, np.float64, residual_mode=P.CORRECT)
        mg.use_graph = args.graph
        out = {}

        def solve():
            out["r"] = mg.Eigen(k, tol=1e-8, vectors=False)
        t_solve = timed(ctx, solve, 1)
        lam, _, info = out["r"]
        it = max(info["iterations"], 1)
        print("%d^3 k=%d: %d iterations, converged %d, lambda %s, worst residual %.2e, %.1f ms, %.2f ms per iteration" % (
            n, k, info["iterations"], info["converged"], np.array2string(lam, precision=10), info["residuals"].max(), t_solve * 1e3,
            t_solve * 1e3 / it), flush=True)
        if info["iterations"] > 1:  # a call that stops after one iteration pays the same workspace, start and confirmation
            t_one = timed(ctx, lambda: mg.Eigen(k, tol=1e-8, maxit=1, vectors=False), 1)
            print("%d^3 k=%d: a call with maxit=1 takes %.1f ms (the workspace of %d level-0 arrays, the start, one iteration, the "
                  "confirmation): %.2f ms per further iteration" % (n, k, t_one * 1e3, 8 * k + 2, (t_solve - t_one) * 1e3 / (it - 1)), flush=True)
        t_cycles = timed(ctx, lambda: [mg.VCycle(0, 2, 2) for _ in range(k)], args.reps)
        # level-0 arrays for the raw entries, filled with the start vectors
        fn = lib.mgx3dxs_elems_f64
        fn.restype = C.c_size_t
        elems = int(fn(_ip(n3)))
        fw = lib.mgx3dxs_block_work_elems_f64
        fw.restype = C.c_size_t
        fk = lib.mgx3dxs_krylov_work_elems_bc_f64
        fk.restype = C.c_size_t
        work = ctx.malloc(8 * max(int(fw(_ip(n3))), int(fk(_ip(n3)))))
        sums = ctx.malloc(8 * 64)
        vec = [ctx.malloc(8 * elems) for _ in range(max(8 * k, 20))]  # (the solver's 8k arrays; 20 serve the launches below)
        for i, p in enumerate(vec):
            P.check(lib.mgx_memset_zero(ctx._h, p, C.c_size_t(8 * elems)))
            P.check(lib.mgx3dxs_eigen_start_f64(ctx._h, p, C.c_int(i), _ip(n3), C.c_int(0)))
        h = _rp(grid_spacing(n3, RNG, np.float64), C.c_double)
        t_apply = timed(ctx, lambda: [P.check(lib.mgx3dxs_laplace_dot_f64(ctx._h, vec[i], vec[k + i], _ip(n3), h, work, sums)) for i in range(k)],
                        args.reps)
        grams, combos, outs = block_launches(k)
        pp = lambda ps: (C.c_void_p * len(ps))(*[p.value for p in ps])
        Y = np.full(48, 0.25)
        mu = np.ones(4)

        def blocks():
            for nu, nv, same in grams:
                V = vec[:nv] if same else vec[4:4 + nv]
                P.check(lib.mgx3dxs_block_gram_f64(ctx._h, C.c_int(nu), pp(vec[:nu]), C.c_int(nv), pp(V), None, _ip(n3), C.c_int(0), work, sums))
            for nin, no in combos:
                P.check(lib.mgx3dxs_block_combine_f64(ctx._h, C.c_int(nin), pp(vec[:nin]), C.c_int(no), pp(vec[16:16 + no]),
                                                      Y.ctypes.data_as(C.c_void_p), _ip(n3), C.c_int(0)))
            for no in outs:
                P.check(lib.mgx3dxs_block_residual_f64(ctx._h, C.c_int(no), pp(vec[:no]), pp(vec[4:4 + no]), None, mu.ctypes.data_as(C.c_void_p),
                                                       pp(vec[16:16 + no]), _ip(n3), C.c_int(0), work, sums))
            for i in range(2 * k):
                P.check(lib.mgx_memcpy_d2d(ctx._h, vec[16 + i % 4], vec[i % 4], C.c_size_t(8 * elems)))
        t_block = timed(ctx, blocks, args.reps)
        gram_words = sum(nu if same else nu + nv for nu, nv, same in grams)  # (distinct arrays a launch reads)
        words = gram_words + sum(nin + no for nin, no in combos) + sum(3 * no for no in outs) + 2 * 2 * k
        print("%d^3 k=%d per iteration: %d V-cycles %.2f ms, %d operator applications %.2f ms, block kernels %.2f ms "
              "(%d launches, %d words per point of which the Gram tiles read %d: %.2f TB/s over the %d points of the padded arrays)" % (
                  n, k, k, t_cycles * 1e3, k, t_apply * 1e3, t_block * 1e3, len(grams) + len(combos) + len(outs) + 2 * k, words, gram_words,
                  words * 8 * elems / t_block / 1e12, elems), flush=True)
        print("%d^3 k=%d: the 2R+1W streaming ceiling of this device (tools/membench, DESIGN.md 5) is %.1f TB/s: the block kernels run at "
              "%.2f of it" % (n, k, TRIAD_TBS, words * 8 * elems / t_block / 1e12 / TRIAD_TBS), flush=True)
        print("%d^3 k=%d: the parts add up to %.2f ms of the %.2f ms an iteration of the solve takes" % (
            n, k, (t_cycles + t_apply + t_block) * 1e3, t_solve * 1e3 / it), flush=True)
        for p in vec + [work, sums]:
            ctx.free(p)
        mg.close()
    ctx.close()


if __name__ == "__main__":
    main()
