"""Harmonic-mean face coefficients on the GPU: the mgx3dxs_*_hmean entries (csrc/mgx_hmean3d.hip, the face
unknowns in csrc/mgx_wall3d.hip), the hierarchy's switch (MultiGrid3D(face_mean="harmonic"), set_face_mean) and the solves on it.

Every kernel is checked bit for bit against the numpy restatement of its arithmetic (tests/op_restated.py), with poisoned pads,
with and without a capacity, with masks and walls; the cycles against the restated cycle; the layered slab against its analytic
series-resistance profile, which the arithmetic faces miss by orders of magnitude.

The cases are looped over inside two tests, not parametrised: the 488 of them take 5 s together, a few milliseconds each, and
would otherwise be a tenth of the GPU suite's test ids.  Every assertion names its case."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import op_cases as OC
import op_restated as OP
import oracle as O
import pde_multigrid_amd as P
from conftest import bits_equal
from odd_shapes import pads_unchanged, run_poisoned
from pde_multigrid_amd.multigrid import _ct, _ip, _rp, grid_spacing, xs_unpack
from op_restated import ZERO
from solve_restated import boundary_mask, close

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]
UNIT = [0, 1, 0, 1, 0, 1]
DTYPES = [np.float64, np.float32]
# the shapes of test_gpu_pcg_mixed.py: the last three end x-rows inside a tile and have differing fp32 / fp64 pads
SHAPES = [(17, 17, 17), (33, 17, 9), (23, 19, 13), (259, 9, 7), (515, 5, 5)]
# (mask, s): no mask, one face, one face per axis, the closed box (which needs s > 0)
MASK_SHIFT = [(0, 0.0), (0, 100.0), (1, 0.0), (1, 100.0), (0b101010, 0.0), (0b101010, 100.0), (63, 100.0)]
# per mask: all betas zero (homogeneous Neumann faces) and one non-zero beta per flagged axis
BETAS = {0: [ZERO], 1: [ZERO, (1.5, 0, 0, 0, 0, 0)], 0b101010: [ZERO, (0, 1.5, 0, 0.25, 0, 3.0)], 63: [ZERO, (2.0, 0, 0, 0.5, 1.25, 0)]}
WORK_GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


def _rand(n3, dtype, seed):
    return np.random.default_rng(seed).uniform(-1, 1, O.shape(n3)).astype(dtype)


def _coef(n3, dtype, seed=100):
    """random in [0.5, 2] with a block that jumps by 1000"""
    a = np.random.default_rng(seed).uniform(0.5, 2, O.shape(n3)).astype(dtype)
    sz, sy, sx = a.shape
    a[sz // 3: sz // 3 + max(2, sz // 3), 1: max(3, sy // 2), sx // 4: sx // 4 + max(3, sx // 3)] *= dtype(1000)
    return a


def _cap(n3, dtype, use):
    return OC.random_capacity(n3, dtype, 200) if use else None


def _fn(name, dtype):
    s, ct = _ct(dtype)
    return getattr(P.lib, "mgx3dxs_%s_%s" % (name, s)), ct


def _h(n3, dtype):
    return _rp(grid_spacing(n3, RG, dtype), _ct(dtype)[1])


def _b(beta, dtype):
    return _rp(list(beta), _ct(dtype)[1])


class Work:
    """the reduction scratch of a call (mgx3dxs_krylov_work_elems_bc doubles, NaN guards behind them) and its device sum"""

    def __init__(self, ctx, n3, dtype):
        fn = getattr(P.lib, "mgx3dxs_krylov_work_elems_bc_" + _ct(dtype)[0])
        fn.restype = C.c_size_t
        self.ctx, self.elems = ctx, int(fn(_ip(n3)))
        host = np.zeros(self.elems + WORK_GUARD)
        host[self.elems:] = np.nan
        self.work, self.sum = ctx.to_device(host), ctx.to_device(np.full(1, np.nan))

    def result(self):
        tail = self.ctx.to_host(C.c_void_p(self.work.value + 8 * self.elems), (WORK_GUARD,), np.float64)
        assert np.isnan(tail).all(), "the work array was overrun"
        return float(self.ctx.to_host(self.sum, (1,), np.float64)[0])

    def close(self):
        self.ctx.free(self.work)
        self.ctx.free(self.sum)


def _unchanged(ups, outs, idx):
    return all(bits_equal(outs[i], ups[i]) for i in idx)


def _run(ctx, given, call, dtype):
    """run_poisoned over the arrays that are given (the capacity may be None); call gets a pointer or None per entry of `given`"""
    present = [x for x in given if x is not None]

    def inner(*ptrs):
        it = iter(ptrs)
        return call(*[next(it) if x is not None else None for x in given])
    return run_poisoned(ctx, present, inner, dtype)


# ---------------------------------------------------------------------------------------------------------- kernels
def _check_relax_hmean(ctx, n3, bc, s, dtype, cap):
    """1 and 3 sweeps: the restatement's bits; f, a, c, the Dirichlet entries and the pads as they were; twice, the same bits"""
    v, f, a, c = _rand(n3, dtype, 1), _rand(n3, dtype, 2), _coef(n3, dtype), _cap(n3, dtype, cap)
    fn, ct = _fn("relax_hmean_wall", dtype)
    unk = OP.unknown_mask(n3, bc)
    for beta in BETAS[bc]:
        for sweeps in (1, 3):
            want = OP.Op(n3, RG, dtype, s, a, c, bc, beta, "harmonic").relax(v, f, sweeps)
            assert bits_equal(want[~unk], v[~unk])
            got = []
            for rep in range(2):
                ups, outs = _run(ctx, [v, f, a, c], lambda x, b, aa, cc: fn(ctx._h, x, b, aa, cc, _ip(n3), _h(n3, dtype), ct(s), C.c_int(sweeps),
                                                                            C.c_int(bc), _b(beta, dtype)), dtype)
                got.append(xs_unpack(outs[0], n3[0]))
                assert pads_unchanged(ups[0], outs[0], n3[0]) and _unchanged(ups, outs, range(1, len(ups))), (beta, sweeps)
            kernel = ctx.last_relax_kernel()
            assert kernel.startswith("relax_hmean_cap3d_xs_kernel" if cap else "relax_hmean3d_xs_kernel"), kernel
            assert bits_equal(got[0], want), (beta, sweeps, np.argwhere(got[0] != want)[:5])
            assert bits_equal(got[0], got[1])
    assert bits_equal(want, P.ops3dxs.relax_hmean(ctx, v, f, a, n3, RG, s, 3, c=c, bc=bc if bc else None, beta=beta if bc else None))
    if not cap and not bc:  # the faces are not the arithmetic ones
        assert not bits_equal(want, OP.Op(n3, RG, dtype, s, a).relax(v, f, 3))


def _check_relax_hmean_from_zero(ctx, n3, s, dtype, cap):
    v, f, a, c = _rand(n3, dtype, 3), _rand(n3, dtype, 4), _coef(n3, dtype), _cap(n3, dtype, cap)
    f[1:-1:2, 1:-1, 1:-1] = 0  # zero right-hand sides too: the signs of the zeros the first pass stores
    fn, ct = _fn("relax_hmean_from_zero", dtype)
    for sweeps in (1, 3):
        want = OP.Op(n3, RG, dtype, s, a, c, mean="harmonic").relax(np.zeros(O.shape(n3), dtype), f, sweeps)
        for rim_is_zero in (0, 1):
            v0 = v.copy()
            if rim_is_zero:  # the caller vouches for a zero boundary; the interior is stale
                v0[boundary_mask(n3)] = 0
            for rep in range(2):
                ups, outs = _run(ctx, [v0, f, a, c], lambda x, b, aa, cc: fn(ctx._h, x, b, aa, cc, _ip(n3), _h(n3, dtype), ct(s), C.c_int(sweeps),
                                                                             C.c_int(rim_is_zero)), dtype)
                assert bits_equal(xs_unpack(outs[0], n3[0]), want), (sweeps, rim_is_zero, rep)
                assert pads_unchanged(ups[0], outs[0], n3[0], zero_ok=not rim_is_zero) and _unchanged(ups, outs, range(1, len(ups)))
    assert ctx.last_relax_kernel().startswith("relax_hmean_cap3d_xs_kernel" if cap else "relax_hmean3d_xs_kernel")
    assert bits_equal(want, P.ops3dxs.relax_hmean_from_zero(ctx, v, f, a, n3, RG, s, 3, False, c=c))


def _check_residual_hmean(ctx, n3, bc, s, dtype, cap):
    v, f, a, c, r0 = _rand(n3, dtype, 5), _rand(n3, dtype, 6), _coef(n3, dtype), _cap(n3, dtype, cap), _rand(n3, dtype, 7)
    fn, ct = _fn("residual_hmean_wall", dtype)
    w = Work(ctx, n3, dtype)
    try:
        for beta in BETAS[bc]:
            want = OP.Op(n3, RG, dtype, s, a, c, bc, beta, "harmonic").residual(v, f)
            want_ss = OP.fsum_sq(want)
            sums = []
            for rep in range(2):
                ups, outs = _run(ctx, [v, f, a, c, r0], lambda x, b, aa, cc, d: fn(ctx._h, x, b, aa, cc, d, _ip(n3), _h(n3, dtype), ct(s), w.work, w.sum,
                                                                                   C.c_int(bc), _b(beta, dtype)), dtype)
                assert bits_equal(xs_unpack(outs[-1], n3[0]), want), beta  # 0 at the Dirichlet points
                assert _unchanged(ups, outs, range(len(ups) - 1)) and pads_unchanged(ups[-1], outs[-1], n3[0]), beta
                sums.append(w.result())
            assert sums[0] == sums[1], "two runs gave different sums"
            assert close(sums[0], want_ss, 1e-13), (beta, sums[0], want_ss)
            # the sum alone (r = NULL), and r alone (no sum, no work array)
            ups, outs = _run(ctx, [v, f, a, c], lambda x, b, aa, cc: fn(ctx._h, x, b, aa, cc, None, _ip(n3), _h(n3, dtype), ct(s), w.work, w.sum,
                                                                        C.c_int(bc), _b(beta, dtype)), dtype)
            assert w.result() == sums[0] and _unchanged(ups, outs, range(len(ups)))
            ups, outs = _run(ctx, [v, f, a, c, r0], lambda x, b, aa, cc, d: fn(ctx._h, x, b, aa, cc, d, _ip(n3), _h(n3, dtype), ct(s), None, None,
                                                                               C.c_int(bc), _b(beta, dtype)), dtype)
            assert bits_equal(xs_unpack(outs[-1], n3[0]), want) and pads_unchanged(ups[-1], outs[-1], n3[0])
    finally:
        w.close()
    r, ss = P.ops3dxs.residual_hmean(ctx, v, f, a, n3, RG, s, c=c, bc=bc if bc else None, beta=beta if bc else None)
    assert bits_equal(r, want) and ss == sums[0]


def _check_apply_hmean_dot(ctx, n3, bc, s, dtype, cap):
    p, a, c, q0 = _rand(n3, dtype, 8), _coef(n3, dtype), _cap(n3, dtype, cap), _rand(n3, dtype, 9)
    unk = OP.unknown_mask(n3, bc)
    fn, ct = _fn("apply_hmean_dot_wall", dtype)
    w = Work(ctx, n3, dtype)
    try:
        for beta in BETAS[bc]:
            want = OP.Op(n3, RG, dtype, s, a, c, bc, beta, "harmonic").apply_A(p)
            want_pq = OP.wdot(OP.weights(n3, bc), p, want)
            sums = []
            for rep in range(2):
                ups, outs = _run(ctx, [p, a, c, q0], lambda x, aa, cc, b: fn(ctx._h, x, aa, cc, b, _ip(n3), _h(n3, dtype), ct(s), w.work, w.sum,
                                                                             C.c_int(bc), _b(beta, dtype)), dtype)
                q = xs_unpack(outs[-1], n3[0])
                assert bits_equal(q[unk], want[unk]), beta
                assert bits_equal(q[~unk], q0[~unk]), "a Dirichlet entry of q was written"
                assert _unchanged(ups, outs, range(len(ups) - 1)) and pads_unchanged(ups[-1], outs[-1], n3[0]), beta
                sums.append(w.result())
            assert sums[0] == sums[1], "two runs gave different sums"
            assert close(sums[0], want_pq, 1e-13), (beta, sums[0], want_pq)
    finally:
        w.close()
    q, pq = P.ops3dxs.apply_hmean_dot(ctx, p, a, n3, RG, s, c=c, bc=bc if bc else None, beta=beta if bc else None)
    assert bits_equal(q[unk], want[unk]) and pq == sums[0]


def _check_a_constant_power_of_two_gives_the_bits_of_the_arithmetic_entries(ctx, dtype, cap):
    n3 = (23, 19, 13)
    v, f, c = _rand(n3, dtype, 1), _rand(n3, dtype, 2), _cap(n3, dtype, cap)
    for k in (0, -2):
        a = np.full(O.shape(n3), 2.0 ** k, dtype)
        for bc, beta in ((0, ZERO), (0b101010, BETAS[0b101010][1])):
            h = P.ops3dxs.relax_hmean(ctx, v, f, a, n3, RG, 100.0, 2, c=c, bc=bc, beta=beta)
            assert bits_equal(h, P.ops3dxs.relax_wall(ctx, v, f, a, c, n3, RG, 100.0, 2, bc, beta))
            r, ss = P.ops3dxs.residual_hmean(ctx, v, f, a, n3, RG, 100.0, c=c, bc=bc, beta=beta)
            r2, ss2 = P.ops3dxs.residual_wall(ctx, v, f, a, c, n3, RG, 100.0, bc, beta)
            assert bits_equal(r, r2) and ss == ss2


# ---------------------------------------------------------------------------------------------------------- hierarchy
GRIDS = [((33, 33, 33), UNIT, "full"), ((33, 17, 9), UNIT, "semi")]
S_CYCLE = 100.0


def _mg(ctx, grid, dtype, a, v=None, f=None, s=S_CYCLE, mean="harmonic", **kw):
    n3, rng, how = GRIDS[grid]
    mg = P.MultiGrid3D(ctx, n3, rng, dtype, residual_mode=P.CORRECT, coarsening=how, shift=s, coefficient=a, face_mean=mean, **kw)
    if v is not None:
        mg.upload_v(0, v)
    if f is not None:
        mg.upload_f(0, f)
    return mg


def _same_levels(mg, H, what):
    assert mg.maxGrids == len(H.sizes) and mg.masks == H.masks
    for l, n in enumerate(H.sizes):
        assert mg.size(l) == n
        assert bits_equal(mg.download_v(l), H.v[l]), (what, "v", l)
        assert bits_equal(mg.download_coefficient(l), H.a[l]), (what, "a", l)
        if l > 0:
            assert bits_equal(mg.download_f(l), H.f[l]), (what, "f", l)


def _check_cycles_match_the_restated_hierarchy(ctx, grid, dtype):
    """VCycle(0, 2, 2) and FullMultiGridVCycle(0, 1, 2, 2): the restated hierarchy on every level; the coefficients of every level are
    those of the arithmetic hierarchy (a goes down the levels as it always did)"""
    n3, rng, how = GRIDS[grid]
    v, f, a = _rand(n3, dtype, 1), _rand(n3, dtype, 2), _coef(n3, dtype)
    H = OP.Hierarchy(OP.Op(n3, rng, dtype, S_CYCLE, a, mean="harmonic"), how)
    H.v[0], H.f[0] = v.copy(), f.copy()
    mg = _mg(ctx, grid, dtype, a, v, f)
    assert mg.face_mean == "harmonic" and mg.has_coefficient
    mg.VCycle(0, 2, 2)
    H.vcycle(0, 2, 2)
    _same_levels(mg, H, "vcycle")
    assert ctx.last_relax_kernel().startswith("relax_hmean3d_xs_kernel"), ctx.last_relax_kernel()
    arith = _mg(ctx, grid, dtype, a, v, f, mean="arithmetic")
    assert arith.face_mean == "arithmetic"
    arith.VCycle(0, 2, 2)
    for l in range(mg.maxGrids):
        assert bits_equal(mg.download_coefficient(l), arith.download_coefficient(l)), l
    assert not bits_equal(mg.download_v(0), arith.download_v(0))
    arith.close()
    mg.upload_v(0, v)
    H.v[0] = v.copy()
    mg.FullMultiGridVCycle(0, 1, 2, 2)
    H.fmg(0, 1, 2, 2)
    _same_levels(mg, H, "fmg")
    mg.close()


def _check_cycles_with_walls_and_a_capacity_match_the_restated_hierarchy(ctx, dtype):
    n3, rng, _ = GRIDS[0]
    bc, beta, g = 0b100101, (1.5, 0, 0.25, 0, 0, 0), (0, 0, -0.5, 0, 0, 2.0)
    v, f, a, c = _rand(n3, dtype, 1), _rand(n3, dtype, 2), _coef(n3, dtype), OC.random_capacity(n3, dtype, 200)
    H = OP.Hierarchy(OP.Op(n3, rng, dtype, S_CYCLE, a, c, bc, beta, "harmonic"), g=g)
    H.v[0], H.f[0] = v.copy(), f.copy()
    H.add_wall_flux()
    mg = _mg(ctx, 0, dtype, a, v, f, neumann=[(bc >> k) & 1 for k in range(6)], capacity=c, robin=beta, wall_flux=g)
    mg.add_wall_flux()
    for k in range(2):
        mg.use_graph = bool(k)
        mg.VCycle(0, 2, 2)
        H.vcycle(0, 2, 2)
        _same_levels(mg, H, "cycle %d" % k)
    mg.Relax(0, 1)
    H.relax(0, 1)
    r = H.residual(0)
    assert bits_equal(mg.CalculateResidual(0), r)
    assert close(mg.ResidualNorm(0), math.sqrt(OP.fsum_sq(r)), 1e-12)
    mg.close()


# ---------------------------------------------------------------------------------------------------------- solves
PCG_N = (17, 17, 17)


def _pcg_problem():
    n3 = PCG_N
    f = _rand(n3, np.float64, 5)
    v0 = np.zeros_like(f)
    v0[boundary_mask(n3)] = _rand(n3, np.float64, 9)[boundary_mask(n3)]  # Dirichlet data where a face is no wall
    return OC.jump_coefficient(n3, 1000.0), f, v0


# (krylov, mask, the restatement's count on this problem from a CPU run, maxit with room above it)
PCG_CASES = [(False, 0, 80, 100), (True, 0, 15, 30), ("weighted", 5, 19, 30)]


def _check_pcg_on_the_jump_of_1000(ctx, krylov, bc, count, maxit):
    """17^3, the block that jumps by 1000, s = 0, to 1e-10: the iteration count is within 1 of the restatement's (the device sums
    differ from fsum in the last bits)"""
    n3, tol = PCG_N, 1e-10
    a, f, v0 = _pcg_problem()
    if krylov:
        _, want_k, hist, want_c, _ = OP.fcg(OP.Op(n3, UNIT, np.float64, 0.0, a, bc=bc, mean="harmonic"), v0, f, tol=tol, maxit=maxit)[:5]
    else:
        H = OP.Hierarchy(OP.Op(n3, UNIT, np.float64, 0.0, a, bc=bc, mean="harmonic"))
        H.v[0], H.f[0] = v0.copy(), f.copy()
        want_k, _, want_c = H.cycle_to(2, 2, tol, maxit)
    assert want_c and want_k == count, (want_k, count)
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, coefficient=a, neumann=[(bc >> k) & 1 for k in range(6)], face_mean="harmonic")
    mg.upload_v(0, v0)
    mg.upload_f(0, f)
    k, rel, conv, _ = mg.PCG(2, 2, tol, maxit, krylov=krylov)
    x = mg.download_v(0)
    mg.close()
    unk = OP.unknown_mask(n3, bc)
    op = OP.Op(n3, UNIT, np.float64, 0.0, a, bc=bc, mean="harmonic")
    true_rel = math.sqrt(OP.fsum_sq(op.residual(x, f)) / OP.fsum_sq(op.residual(v0, f)))
    print("PCG krylov=%s bc=%d: %d iterations (restated %d), rel %.3e, restated residual of the result %.3e" % (krylov, bc, k, want_k, rel, true_rel))
    assert conv and abs(k - want_k) <= 1, (k, want_k)
    assert rel < tol and true_rel < tol and close(rel, true_rel, 1e-6)
    assert bits_equal(x[~unk], v0[~unk]), "the Dirichlet data changed"
    if krylov is True:
        x2, k2, rel2, conv2 = P.solve3d_pcg(ctx, v0, f, UNIT, tol=tol, maxit=maxit, krylov=True, coefficient=a, face_mean="harmonic")
        assert (k2, conv2) == (k, conv) and bits_equal(x2, x)


def _check_backward_euler_with_a_jumping_capacity(ctx):
    """two steps of c u_t = div(a grad u), a jumping by 1000 and c by 100 in the block, kappa dt = 1e-2, plain cycling to 1e-10 (the
    restatement takes 25 cycles): the first step's right-hand side is the restated one, the result the restated steps' to 1e-9 --
    the bound test_gpu_cap.py holds its own backward Euler test to -- and bit for bit where the cycle counts agree"""
    n3 = PCG_N
    a, c = OC.jump_coefficient(n3, 1000.0), OC.block_capacity(n3, 100, 1)
    u0 = OC.gaussian(n3)
    u0[boundary_mask(n3)] = 0
    H = OP.Hierarchy(OP.Op(n3, UNIT, np.float64, 0.0, a, c, mean="harmonic"))
    H.v[0] = u0.copy()
    want_its, want_worst, want_conv = H.backward_euler(2, 1e-2, 1.0, 2, 2, 1e-10, 100)
    assert want_conv and want_its == 25, want_its
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, coefficient=a, capacity=c, face_mean="harmonic")
    mg.upload_v(0, u0)
    its, worst, conv = mg.BackwardEuler(1, 1e-2, 1.0, tol=1e-10, krylov=False)
    assert conv and mg.shift == 100.0
    assert bits_equal(mg.download_f(0)[~boundary_mask(n3)], OP.Op(n3, UNIT, np.float64, 100.0, c=c).rhs(u0, None, 1.0)[~boundary_mask(n3)])
    its2, worst2, conv2 = mg.BackwardEuler(1, 1e-2, 1.0, tol=1e-10, krylov=False)
    u = mg.download_v(0)
    mg.close()
    print("backward Euler: %d cycles (restated %d), worst residual %.3e (restated %.3e)" % (its + its2, want_its, max(worst, worst2), want_worst))
    assert conv2 and max(worst, worst2) < 1e-10 and abs(its + its2 - want_its) <= 2
    assert np.abs(u - H.v[0]).max() <= 1e-9 * np.abs(H.v[0]).max()
    if its + its2 == want_its:
        assert bits_equal(u, H.v[0])


# ---------------------------------------------------------------------------------------------------------- physics
# the error the CPU restatement leaves on the slab (test_hmean_cpu.py: flexible CG to 1e-12): 3.678e-13 for the jump of 10 and
# 4.635e-11 for 1000; the GPU holds ten times that (the sums round differently).  Measured on the GPU: 3.678e-13 (12 iterations) and
# 2.307e-11 (61 iterations); with arithmetic faces 3.585e-2 and 5.853e-2.
SLAB_RESTATED_ERROR = {10: 3.678e-13, 1000: 4.635e-11}


def _check_the_layered_slab_matches_the_series_resistance_profile(ctx, jump):
    """9 x 9 x 17, a1 below the interface midway between planes 8 and 9, a1 * jump above; insulated x/y faces, u = 0 and 1 on the z
    faces, f = 0: PCG(krylov="weighted") to 1e-12 gives the analytic piecewise-linear profile with harmonic faces; with
    arithmetic faces the same call is off by orders of magnitude more (0.036 and 0.059 of the unit drop in the restatement)"""
    n3, rng = OC.SLAB_N3, OC.SLAB_RNG
    a, u, _ = OC.slab(jump)
    v0 = u.copy()
    v0[1:-1] = 0.0
    bound = 10 * SLAB_RESTATED_ERROR[jump]
    errs = {}
    for mean in ("harmonic", "arithmetic"):
        x, k, rel, conv = P.solve3d_pcg(ctx, v0, np.zeros_like(u), rng, tol=1e-12, maxit=100, krylov="weighted", coefficient=a,
                                        neumann=[1, 1, 1, 1, 0, 0], face_mean=mean)
        errs[mean] = float(np.abs(x - u).max())
        print("slab, jump %g, %s faces: %d iterations to %.2e, error %.3e (bound %.3e)" % (jump, mean, k, rel, errs[mean], bound))
        assert conv, (mean, k, rel)
    assert errs["harmonic"] <= bound, errs
    assert errs["arithmetic"] > 1e6 * bound, errs


# ---------------------------------------------------------------------------------------------------------- switching
def _check_switching_the_mean_between_replayed_cycles(ctx, dtype):
    """use_graph: cycle arithmetic, switch to harmonic, cycle, switch back, cycle -- every cycle has the bits of an eager hierarchy
    taken through the same switches and of the restated hierarchy of that mean"""
    n3, rng, how = GRIDS[0]
    v, f, a = _rand(n3, dtype, 1), _rand(n3, dtype, 2), _coef(n3, dtype)
    mg, eager = _mg(ctx, 0, dtype, a, v, f, mean="arithmetic"), _mg(ctx, 0, dtype, a, v, f, mean="arithmetic")
    mg.use_graph = True
    H = OP.Hierarchy(OP.Op(n3, rng, dtype, S_CYCLE, a))
    H.v[0], H.f[0] = v.copy(), f.copy()
    for step, mean in enumerate(("arithmetic", "arithmetic", "harmonic", "harmonic", "arithmetic")):
        if mean != mg.face_mean:
            assert mg._mg.contents.graph_exec[0], "nothing was captured before the switch"
            mg.set_face_mean(mean)
            eager.set_face_mean(mean)
            assert not mg._mg.contents.graph_exec[0], "the switch kept a captured graph"
        H.replace(mean=mean)
        assert mg.face_mean == eager.face_mean == mean
        mg.VCycle(0, 2, 2)
        eager.VCycle(0, 2, 2)
        H.vcycle(0, 2, 2)
        assert ("hmean" in ctx.last_relax_kernel()) == (mean == "harmonic"), ctx.last_relax_kernel()
        for l in range(mg.maxGrids):
            assert bits_equal(mg.download_v(l), eager.download_v(l)) and bits_equal(mg.download_v(l), H.v[l]), (step, mean, l)
    mg.close()
    eager.close()


def _check_unit_coefficient_gives_the_same_bits_under_both_means(ctx, dtype):
    n3, rng, _ = GRIDS[0]
    v, f, a = _rand(n3, dtype, 1), _rand(n3, dtype, 2), np.ones(O.shape(n3), dtype)
    out = []
    for mean in ("harmonic", "arithmetic"):
        mg = _mg(ctx, 0, dtype, a, v, f, mean=mean)
        mg.VCycle(0, 2, 2)
        out.append([mg.download_v(l) for l in range(mg.maxGrids)])
        mg.close()
    assert all(bits_equal(x, y) for x, y in zip(*out))


# ---------------------------------------------------------------------------------------------------------- refusals
def _refused(call, *words):
    with pytest.raises(P.MgxError) as e:
        call()
    assert e.value.status == P.MGX_ERR_INVALID and all(w in str(e.value) for w in words), str(e.value)


def _check_a_bad_mode_is_refused(ctx):
    n3 = (17, 17, 17)
    with pytest.raises(ValueError):
        P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, face_mean="geometric")
    with pytest.raises(ValueError):
        P.solve3d_pcg(ctx, np.zeros(O.shape(n3)), None, UNIT, face_mean="geometric")
    mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, coefficient=_coef(n3, np.float64))
    with pytest.raises(ValueError):
        mg.set_face_mean("geometric")
    for mode in (2, -1):
        _refused(lambda: mg._call("set_face_mean", C.c_int(mode)), "set_face_mean", str(mode))
    assert mg.face_mean == "arithmetic"
    mg.set_face_mean("harmonic")
    _refused(lambda: mg._call("set_face_mean", C.c_int(7)), "set_face_mean")
    assert mg.face_mean == "harmonic"
    mg.close()


# a * a leaves the normal range: fp32 and fp64, below and above
RANGE_CASES = [(np.float32, 1e-25), (np.float32, 1e25), (np.float64, 1e-160), (np.float64, 1e160)]


def _check_coefficients_outside_the_range_of_the_product_are_refused(ctx, dtype, bad):
    """a * a has to be normal and finite: refused on either order of set_face_mean / set_coefficient, with the value named and the
    hierarchy as it was"""
    n3 = (17, 17, 17)
    good = _coef(n3, dtype)
    a = good.copy()
    a[0, 3, 5] = bad  # a boundary point: every point of level 0 is checked
    v, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    word = "%g" % float(dtype(bad))
    # the mode first
    mg = P.MultiGrid3D(ctx, n3, UNIT, dtype, residual_mode=P.CORRECT, face_mean="harmonic")
    _refused(lambda: mg.set_coefficient(a), "set_coefficient", word)
    assert not mg.has_coefficient and mg.face_mean == "harmonic"
    mg.set_coefficient(good)
    _refused(lambda: mg.set_coefficient(a), "set_coefficient", word)
    assert bits_equal(mg.download_coefficient(0), good), "a refused coefficient changed the hierarchy"
    mg.close()
    with pytest.raises(P.MgxError):
        P.MultiGrid3D(ctx, n3, UNIT, dtype, residual_mode=P.CORRECT, coefficient=a, face_mean="harmonic")
    # the coefficient first: fine for the arithmetic faces, and the switch is refused
    mg = P.MultiGrid3D(ctx, n3, UNIT, dtype, residual_mode=P.CORRECT, coefficient=a)
    mg.upload_v(0, v)
    mg.upload_f(0, f)
    _refused(lambda: mg.set_face_mean("harmonic"), "set_face_mean", word)
    assert mg.face_mean == "arithmetic" and bits_equal(mg.download_coefficient(0), a)
    mg.VCycle(0, 1, 1)
    assert "coef" in ctx.last_relax_kernel()
    mg.set_coefficient(good)
    mg.set_face_mean("harmonic")
    assert mg.face_mean == "harmonic" and bits_equal(mg.download_coefficient(0), good)
    mg.close()


def _check_pcg_mixed_is_still_refused(ctx):
    n3 = (17, 17, 17)
    words = {}
    for mean in ("arithmetic", "harmonic"):
        mg = P.MultiGrid3D(ctx, n3, UNIT, residual_mode=P.CORRECT, coefficient=_coef(n3, np.float64), face_mean=mean)
        with pytest.raises(P.MgxError) as e:
            mg.PCG(2, 2, 1e-8, 5, precond="f32")
        assert e.value.status == P.MGX_ERR_INVALID
        words[mean] = str(e.value)
        mg.close()
    assert words["harmonic"] == words["arithmetic"]  # refused with the same words


def _check_the_mode_changes_no_bit_of_a_hierarchy_without_a_coefficient(ctx, dtype):
    n3, rng, _ = GRIDS[0]
    v, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    out = []
    for mean in ("arithmetic", "harmonic"):
        mg = P.MultiGrid3D(ctx, n3, rng, dtype, residual_mode=P.CORRECT, shift=S_CYCLE)
        mg.use_graph = True
        mg.upload_v(0, v)
        mg.upload_f(0, f)
        mg.VCycle(0, 2, 2)
        graph = mg._mg.contents.graph_exec[0]
        mg.set_face_mean(mean)
        assert mg.face_mean == mean and mg._mg.contents.graph_exec[0] == graph, "a hierarchy without a coefficient dropped its graph"
        mg.VCycle(0, 2, 2)
        assert "shift" in ctx.last_relax_kernel(), ctx.last_relax_kernel()
        out.append([mg.download_v(l) for l in range(mg.maxGrids)])
        mg.close()
    assert all(bits_equal(x, y) for x, y in zip(*out))


# ---------------------------------------------------------------------------------------------------------- the two tests
def _each(check, ctx, *axes):
    """check(ctx, *case) for every case of the product of the axes (the last axis varies fastest); a failure names the case"""
    for case in itertools.product(*axes):
        try:
            check(ctx, *case)
        except Exception as e:
            raise AssertionError("%s%r: %s" % (check.__name__, case, e)) from e


def test_hmean_kernels_match_the_restatement(ctx):
    """the four entries on every shape, mask, shift and precision, with and without a capacity; the constant power of two"""
    for check in (_check_relax_hmean, _check_residual_hmean, _check_apply_hmean_dot):
        for bc, s in MASK_SHIFT:
            _each(check, ctx, SHAPES, [bc], [s], DTYPES, [False, True])
    _each(_check_relax_hmean_from_zero, ctx, SHAPES, [0.0, 100.0], DTYPES, [False, True])
    _each(_check_a_constant_power_of_two_gives_the_bits_of_the_arithmetic_entries, ctx, DTYPES, [False, True])


def test_hmean_hierarchy_solves_switch_and_refusals(ctx):
    """the hierarchy with harmonic faces: cycles, walls and a capacity, PCG, backward Euler, the layered slab, switching the mean
    between replayed cycles, and everything that is refused"""
    _each(_check_cycles_match_the_restated_hierarchy, ctx, [0, 1], DTYPES)
    _each(_check_cycles_with_walls_and_a_capacity_match_the_restated_hierarchy, ctx, DTYPES)
    for case in PCG_CASES:
        _each(_check_pcg_on_the_jump_of_1000, ctx, *([x] for x in case))
    _each(_check_backward_euler_with_a_jumping_capacity, ctx)
    _each(_check_the_layered_slab_matches_the_series_resistance_profile, ctx, [10, 1000])
    _each(_check_switching_the_mean_between_replayed_cycles, ctx, DTYPES)
    _each(_check_unit_coefficient_gives_the_same_bits_under_both_means, ctx, DTYPES)
    _each(_check_a_bad_mode_is_refused, ctx)
    for dtype, bad in RANGE_CASES:
        _each(_check_coefficients_outside_the_range_of_the_product_are_refused, ctx, [dtype], [bad])
    _each(_check_pcg_mixed_is_still_refused, ctx)
    _each(_check_the_mode_changes_no_bit_of_a_hierarchy_without_a_coefficient, ctx, DTYPES)
