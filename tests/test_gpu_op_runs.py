"""GPU suite: the z-marching kernels of the shifted, the variable-coefficient and the Neumann operators on runs of MORE THAN ONE
plane.

The colour pass relax_op3d_xs_kernel (csrc/mgx_stencil3d.hpp) gives a workgroup a run of planes and carries v (and, with a
coefficient, a) from plane to plane in registers; residual_restrict_axes3d_xs_kernel (csrc/mgx_semi3d.hpp) does the same with
its three v planes and a row of residuals over a run of coarse planes.  The host picks the run lengths by the size of the launch,
and on every shape small enough for a test it picks the shortest one: 1 plane for the colour pass (what is carried is then never
read), 2 coarse planes for the transfers.  "relax3d.zchunk" and "residual_restrict3d.pzchunk" set the run lengths here, so that
the carried values, runs that do not divide the planes and runs longer than the grid are all exercised; one test uses grids long enough along z for the host's own rule to choose runs of 4 and of 2 planes.

Everything is compared bit for bit with the numpy restatements (op_restated,
semi_restated), computed once per case and shared by all run lengths: the run length never changes a result.  All arrays are
random, the coefficient included, so that they vary along z."""
import copy
import ctypes as C
import functools
import subprocess
import sys

import numpy as np
import pytest

import op_cases as OC
import op_restated as OP
import oracle as O
import pde_multigrid_amd as P
import semi_restated as S
from conftest import bits_equal
from odd_shapes import pads_unchanged, run_poisoned
from pde_multigrid_amd.multigrid import _ct, _ip, _rp, grid_spacing, xs_unpack
from solve_restated import boundary_mask, interior

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]
UNIT = [0, 1, 0, 1, 0, 1]
DTYPES = [np.float64, np.float32]
ZCHUNK, PZCHUNK = "relax3d.zchunk", "residual_restrict3d.pzchunk"
# (21,13,29): 27 planes, 11 interior rows -- two rows per lane, and the last wave of the second row tile has one row (nrows < R);
# (131,7,9): 66 x-pairs, the second x-block has one active lane, one row per lane; (513,33,9): rows longer than a wave, four rows
# per lane, a last tile of three rows, 7 planes; (3,5,9) and (5,3,3): minimal axes
SHAPES = [(21, 13, 29), (131, 7, 9), (513, 33, 9), (3, 5, 9), (5, 3, 3)]
# 0 = the host's rule; runs that do not divide the planes (a shorter last run) and runs longer than the grid
RUNS = [0, 1, 2, 3, 4, 5, 8, 64]


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def num_cus():
    """the device's CU count from torch's device properties.  Asked in a process of its own, once per module: torch brings its own
    copy of the HIP runtime, which a process that has loaded libmgx first must not load as well (pde_multigrid_amd/_lib.py)"""
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         check=True, capture_output=True, text=True, timeout=120).stdout
    return int(out.split()[-1])


def _rand(n3, dtype, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, O.shape(n3)).astype(dtype)


def _coef(n3, dtype, seed=100):
    return _rand(n3, dtype, seed, 0.5, 2.0)


def _fn(name, dtype):
    s, ct = _ct(dtype)
    return getattr(P.lib, "mgx3dxs_%s_%s" % (name, s)), ct


def _h(n3, rng, dtype):
    return _rp(grid_spacing(n3, rng, dtype), _ct(dtype)[1])


def _ceil(a, b):
    return -(-a // b)


def launch_rule(n3, rows, cus):
    """relax_op3d_pass's choice restated: (waves per workgroup, rows per lane, planes per run) with no "relax3d.zchunk" set.  Four
    waves of `rows` rows, both halved while they exceed the interior rows; runs of four planes, halved while the launch has fewer
    than eight workgroups per CU"""
    sx, sy, sz = n3
    ty = 4
    while rows > 1 and rows * ty > sy - 2:
        rows //= 2
    while ty > 1 and rows * ty > sy - 2:
        ty //= 2
    gx, gy = _ceil((sx + 1) // 2 - 1, 64), _ceil(sy - 2, ty * rows)
    zchunk = 4
    while zchunk > 1 and gx * gy * _ceil(sz - 2, zchunk) < 8 * cus:
        zchunk //= 2
    return ty, rows, zchunk


def kernel_name(kernel, dtype, n3, rows, cus, knob):
    """what last_relax_kernel() reports for a colour pass: name<type, waves, rows per lane, planes per run as launched>"""
    ty, rows, auto = launch_rule(n3, rows, cus)
    return "%s<%s,%d,%d,%d>" % (kernel, "double" if np.dtype(dtype) == np.float64 else "float", ty, rows, knob or auto)


class knobs:
    """context parameters set inside a `with` block and put back to their defaults at its end, whatever happens in it"""
    DEFAULTS = {ZCHUNK: 0, PZCHUNK: 0, "relax3d.rows": 4}

    def __init__(self, ctx):
        self.ctx, self.touched = ctx, set()

    def __enter__(self):
        return self

    def set(self, name, value):
        self.touched.add(name)
        self.ctx.set_param(name, value)

    def __exit__(self, *exc):
        for name in self.touched:
            self.ctx.set_param(name, self.DEFAULTS[name])


# ------------------------------------------------------------------------------------------- a. forced runs, the colour pass
def _relax_call(ctx, entry, dtype, n3, arrays, s, sweeps, extra):
    """one call of a relax entry on poisoned arrays: (v as stored before, every array as stored after)"""
    fn, ct = _fn(entry, dtype)
    ups, outs = run_poisoned(ctx, arrays, lambda *p: fn(ctx._h, *p, _ip(n3), _h(n3, RG, dtype), ct(s), C.c_int(sweeps),
                                                        *[C.c_int(e) for e in extra]), dtype)
    return ups, outs


def _check_relax(ctx, entry, kernel, dtype, n3, arrays, s, sweeps, extra, want, untouched, rows, cus, what, zero_ok=False):
    """every run length of RUNS: the restatement's bits, pads and inputs as they were, the entries under the mask `untouched` (those
    that are no unknowns) as they were, and the run length launched as the last field of last_relax_kernel()"""
    v = arrays[0]
    with knobs(ctx) as k:
        for run in RUNS:
            k.set(ZCHUNK, run)
            ups, outs = _relax_call(ctx, entry, dtype, n3, arrays, s, sweeps, extra)
            name = ctx.last_relax_kernel()
            assert name == kernel_name(kernel, dtype, n3, rows, cus, run), (what, run, name)
            got = xs_unpack(outs[0], n3[0])
            assert bits_equal(got, want), (what, run, np.argwhere(got != want)[:5])
            assert bits_equal(got[untouched], v[untouched]), (what, run, "an entry that is no unknown was written")
            assert pads_unchanged(ups[0], outs[0], n3[0], zero_ok=zero_ok), (what, run)
            assert all(bits_equal(o, u) for o, u in zip(outs[1:], ups[1:])), (what, run, "an input was written")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", SHAPES)
def test_relax_shift_runs(ctx, num_cus, n3, dtype):
    v, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    rim = boundary_mask(n3)
    for s in (0.0, 0.75):
        for sweeps in (1, 2):
            want = OP.Op(n3, RG, dtype, s).relax(v, f, sweeps)
            _check_relax(ctx, "relax_shift", "relax_shift3d_xs_kernel", dtype, n3, [v, f], s, sweeps, (), want, rim, 4, num_cus, (s, sweeps))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [4, 2, 1])
@pytest.mark.parametrize("n3", SHAPES)
def test_relax_coef_runs(ctx, num_cus, n3, rows, dtype):
    v, f, a = _rand(n3, dtype, 1), _rand(n3, dtype, 2), _coef(n3, dtype)
    rim = boundary_mask(n3)
    with knobs(ctx) as k:
        k.set("relax3d.rows", rows)
        for s in (0.0, 0.75):
            for sweeps in (1, 2):
                want = OP.Op(n3, RG, dtype, s, a).relax(v, f, sweeps)
                _check_relax(ctx, "relax_coef", "relax_coef3d_xs_kernel", dtype, n3, [v, f, a], s, sweeps, (), want, rim, rows, num_cus,
                             (rows, s, sweeps))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("coef", [False, True])
@pytest.mark.parametrize("n3", SHAPES)
def test_relax_from_zero_runs(ctx, num_cus, n3, coef, dtype):
    """two sweeps from zero: with rim_is_zero the first red pass is the from-zero kernel and three generic passes follow it,
    without it the array is filled and four generic passes run"""
    v, f = _rand(n3, dtype, 3), _rand(n3, dtype, 4)
    f[1:-1:2, 1:-1, 1:-1] = 0  # zero right-hand sides too: the signs of the zeros the first pass stores
    a = _coef(n3, dtype) if coef else None
    entry, kernel = ("relax_coef_from_zero", "relax_coef3d_xs_kernel") if coef else ("relax_shift_from_zero", "relax_shift3d_xs_kernel")
    rim = boundary_mask(n3)
    for s in (0.0, 0.75):
        zero = np.zeros_like(v)
        want = OP.Op(n3, RG, dtype, s, a).relax(zero, f, 2) if coef else OP.Op(n3, RG, dtype, s).relax(zero, f, 2)
        for rim_is_zero in (0, 1):
            v0 = v.copy()
            if rim_is_zero:  # the caller vouches for a zero boundary, which then stays as it is; the interior is stale
                v0[rim] = 0
            untouched = rim if rim_is_zero else np.zeros_like(rim)  # (without it the fill writes every entry)
            _check_relax(ctx, entry, kernel, dtype, n3, [v0, f] + ([a] if coef else []), s, 2, (rim_is_zero,), want, untouched, 4, num_cus,
                         (s, rim_is_zero), zero_ok=not rim_is_zero)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("coef", [False, True])
@pytest.mark.parametrize("n3", SHAPES)
def test_relax_bc_runs(ctx, num_cus, n3, coef, dtype):
    """Neumann faces: the rim launch of a colour sits between the interior passes, which march runs of several planes"""
    v, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    a = _coef(n3, dtype, 3) if coef else None
    entry, kernel = ("relax_coef_bc", "relax_coef3d_xs_kernel") if coef else ("relax_shift_bc", "relax_shift3d_xs_kernel")
    for bc, shifts in ((37, (0.0, 0.75)), (63, (0.75,))):  # a closed box without a shift is singular
        unk = OP.unknown_mask(n3, bc)
        for s in shifts:
            for sweeps in (1, 2):
                want = OP.Op(n3, RG, dtype, s, a, bc=bc).relax(v, f, sweeps)
                _check_relax(ctx, entry, kernel, dtype, n3, [v, f] + ([a] if coef else []), s, sweeps, (bc,), want, ~unk, 4, num_cus,
                             (bc, s, sweeps))


# ------------------------------------------------------------------------------------------- b. the host's own rule
def _smallest_sz(n2, rows, cus, zchunk):
    """the smallest odd sz for which the restated rule gives runs of `zchunk` planes on (n2[0], n2[1], sz), found by bisection:
    the run length does not shrink as sz grows"""
    lo, hi = 1, 1 << 16  # in units of sz = 2k + 1
    while lo < hi:
        mid = (lo + hi) // 2
        if launch_rule((n2[0], n2[1], 2 * mid + 1), rows, cus)[2] >= zchunk:
            hi = mid
        else:
            lo = mid + 1
    return 2 * lo + 1


AUTO_N2 = (21, 19)  # one x-block; 17 interior rows: two row tiles of four waves of four rows, three of two rows
AUTO_CASES = [("relax_shift", 4), ("relax_coef", 4), ("relax_coef", 2), ("relax_coef_bc", 4)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("zchunk", [4, 2])
@pytest.mark.parametrize("entry,rows", AUTO_CASES)
def test_the_hosts_rule_chooses_multi_plane_runs(ctx, num_cus, entry, rows, zchunk, dtype):
    """no knob set: on a grid long enough along z, relax_op3d_pass itself launches runs of 4 (of 2) planes, and the result is the
    restatement's.  The smallest such sz under the rule as restated above; on 256 CUs, for four rows per lane, 4095 and 2049."""
    sz = _smallest_sz(AUTO_N2, rows, num_cus, zchunk)
    if num_cus == 256 and rows == 4:
        assert sz == {4: 4095, 2: 2049}[zchunk]
    if sz > 16387:
        pytest.skip("%d CUs: runs of %d planes need sz = %d, more than 16387 (a device of over 1000 CUs)" % (num_cus, zchunk, sz))
    n3 = AUTO_N2 + (sz,)
    assert launch_rule(n3, rows, num_cus)[2] == zchunk and launch_rule(AUTO_N2 + (sz - 2,), rows, num_cus)[2] < zchunk
    v, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    s, extra, a = 0.75, (), None
    if entry == "relax_shift":
        kernel, want, keep = "relax_shift3d_xs_kernel", OP.Op(n3, RG, dtype, s).relax(v, f, 1), boundary_mask(n3)
    else:
        a = _coef(n3, dtype)
        kernel = "relax_coef3d_xs_kernel"
        if entry == "relax_coef":
            want, keep = OP.Op(n3, RG, dtype, s, a).relax(v, f, 1), boundary_mask(n3)
        else:
            extra = (63,)
            want, keep = OP.Op(n3, RG, dtype, s, a, bc=63).relax(v, f, 1), ~OP.unknown_mask(n3, 63)
    with knobs(ctx) as k:
        k.set("relax3d.rows", rows)
        ups, outs = _relax_call(ctx, entry, dtype, n3, [v, f] + ([] if a is None else [a]), s, 1, extra)
        name = ctx.last_relax_kernel()
    assert name == kernel_name(kernel, dtype, n3, rows, num_cus, 0) and name.endswith(",%d>" % zchunk), name
    got = xs_unpack(outs[0], n3[0])
    assert bits_equal(got, want), np.argwhere(got != want)[:5]
    assert bits_equal(got[keep], v[keep]), "an entry that is no unknown was written"
    assert pads_unchanged(ups[0], outs[0], n3[0]) and all(bits_equal(o, u) for o, u in zip(outs[1:], ups[1:]))


# ------------------------------------------------------------------------------------------- c. cycles on multi-plane runs
CYCLE_S, CYCLE_BC = 0.75, 37
CYCLE_GRIDS = [((33, 33, 33), UNIT, "full"), ((65, 33, 17), RG, "full"), (S.TABLE[0][0], S.TABLE[0][1], "semi")]
CYCLES = [("shift", 0), ("shift", 1), ("shift", 2), ("coef", 0), ("coef", 1), ("neumann", 0), ("neumann", 1)]
FACES = [bool((CYCLE_BC >> k) & 1) for k in range(6)]


def _restated(op, grid, dtype):
    n3, rng, how = CYCLE_GRIDS[grid]
    if op == "shift":
        return OP.Hierarchy(OP.Op(n3, rng, dtype, CYCLE_S), how)
    if op == "coef":
        return OP.Hierarchy(OP.Op(n3, rng, dtype, CYCLE_S, OC.smooth_coefficient(n3, dtype)), how)
    return OP.Hierarchy(OP.Op(n3, rng, dtype, CYCLE_S, OC.smooth_coefficient(n3, dtype), bc=CYCLE_BC))


def _mg(ctx, op, grid, dtype, v, f):
    n3, rng, how = CYCLE_GRIDS[grid]
    mg = P.MultiGrid3D(ctx, n3, rng, dtype, residual_mode=P.CORRECT, coarsening=how, shift=CYCLE_S,
                       coefficient=None if op == "shift" else OC.smooth_coefficient(n3, dtype), neumann=FACES if op == "neumann" else None)
    mg.upload_v(0, v)
    mg.upload_f(0, f)
    return mg


@functools.lru_cache(maxsize=None)
def _cycled(op, grid, dtype):
    """the restated hierarchy after one and after two V(2,2) cycles, and after FMG(1,2,2) (from other data), once per case"""
    n3 = CYCLE_GRIDS[grid][0]
    H = _restated(op, grid, dtype)
    H.v[0], H.f[0] = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    H.vcycle(0, 2, 2)
    first = copy.deepcopy(H)
    H.vcycle(0, 2, 2)
    F = _restated(op, grid, dtype)
    F.v[0], F.f[0] = _rand(n3, dtype, 5), _rand(n3, dtype, 6)
    F.fmg(0, 1, 2, 2)
    return first, H, F


def _same_levels(mg, H, what):
    assert mg.maxGrids == len(H.sizes)
    for l, n in enumerate(H.sizes):
        assert mg.size(l) == n
        assert bits_equal(mg.download_v(l), H.v[l]), (what, "v", l)
        if l > 0:
            assert bits_equal(mg.download_f(l), H.f[l]), (what, "f", l)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op,grid", CYCLES)
def test_cycles_on_runs_of_three_planes(ctx, op, grid, dtype):
    """V(2,2) twice and FMG(1,2,2) with every colour pass on runs of 3 planes and residual_restrict_shift on runs of 3 coarse planes:
    every level's v and f against the restated hierarchy, eagerly and through use_graph (capture, then replays)"""
    n3 = CYCLE_GRIDS[grid][0]
    first, second, fmg = _cycled(op, grid, dtype)
    with knobs(ctx) as k:
        k.set(ZCHUNK, 3)
        k.set(PZCHUNK, 3)
        v, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
        mg = _mg(ctx, op, grid, dtype, v, f)
        mg.VCycle(0, 2, 2)
        assert ctx.last_relax_kernel().endswith(",3>"), ctx.last_relax_kernel()
        _same_levels(mg, first, "eager")
        mg.VCycle(0, 2, 2)
        _same_levels(mg, second, "second")
        mg.use_graph = True
        execs = []
        for rep in range(4):  # capture (perhaps once more under the rim flags that cycle left), then replays: two at the least
            mg.upload_v(0, v)
            mg.VCycle(0, 2, 2)
            _same_levels(mg, first, ("graph", rep))
            execs.append(mg._mg.contents.graph_exec[0])
        assert execs[1] and execs[2] == execs[1] and execs[3] == execs[1], "the last cycles were captured again instead of replayed"
        mg.close()
        v, f = _rand(n3, dtype, 5), _rand(n3, dtype, 6)
        for graph in (False, True):
            mg = _mg(ctx, op, grid, dtype, v, f)
            mg.use_graph = graph
            execs = []
            for rep in range(4 if graph else 1):
                mg.upload_v(0, v)
                mg.FullMultiGridVCycle(0, 1, 2, 2)
                _same_levels(mg, fmg, ("fmg", graph, rep))
                execs.append([mg._mg.contents.graph_exec[l] for l in range(mg.maxGrids)])
            if graph:
                assert all(execs[1]) and execs[2] == execs[1] and execs[3] == execs[1], "a level's cycle was captured again instead of replayed"
            mg.close()


# ------------------------------------------------------------------------------------------- d. forced runs, the transfers
# 0 = the host's rule (2 on every shape here); the runs large levels get (4, 8, 16), runs that do not divide the planes, and 31
PRUNS = [0, 1, 2, 3, 4, 8, 16, 31]
# (9,9,67): with z halved 32 interior coarse planes -- two full runs of 16, or a run of 31 and a run of 1; (9,67,9): 7 planes where
# z is kept; the others are the kinds of shape the transfers are tested on elsewhere
RR_SHAPES = [(21, 13, 29), (513, 33, 9), (33, 17, 9), (9, 9, 67), (9, 67, 9)]


def _rr_rng(n3):
    return UNIT if n3 == (33, 17, 9) else RG  # the unit cube on 2^k + 1 points: the exact-reciprocal form of the residual


def _check_transfer(ctx, call, dtype, n3, cn, v, f, want, what):
    c0 = _rand(cn, dtype, 15)
    rim = boundary_mask(cn)
    assert not want[rim].any()
    with knobs(ctx) as k:
        for run in PRUNS:
            k.set(PZCHUNK, run)
            for keep in (0, 1):
                ups, outs = run_poisoned(ctx, [v, f, c0], lambda a, b, c: call(a, b, c, keep), dtype)
                got = xs_unpack(outs[2], cn[0])
                assert bits_equal(interior(got), interior(want)), (what, run, keep, np.argwhere(interior(got) != interior(want))[:5])
                assert bits_equal(got[rim], c0[rim] if keep else np.zeros_like(c0)[rim]), (what, run, keep)  # left alone, or written as 0
                assert bits_equal(outs[0], ups[0]) and bits_equal(outs[1], ups[1]) and pads_unchanged(ups[2], outs[2], cn[0]), (what, run, keep)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mask", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("n3", RR_SHAPES)
def test_residual_restrict_shift_runs(ctx, n3, mask, dtype):
    rng, cn = _rr_rng(n3), S.coarse_size(n3, mask)
    v, f = _rand(n3, dtype, 13), _rand(n3, dtype, 14)
    fn, ct = _fn("residual_restrict_shift", dtype)
    for s in (0.0, 0.75):
        want = OP.restrict(n3, OP.Op(n3, rng, dtype, s).residual(v, f), 0, dtype, mask)
        _check_transfer(ctx, lambda a, b, c, keep: fn(ctx._h, a, b, _ip(n3), _h(n3, rng, dtype), ct(s), c, _ip(cn), C.c_int(keep)), dtype, n3, cn,
                        v, f, want, s)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mask", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("n3", RR_SHAPES)
def test_residual_restrict_axes_runs(ctx, n3, mask, dtype):
    rng, cn = _rr_rng(n3), S.coarse_size(n3, mask)
    v, f = _rand(n3, dtype, 5), _rand(n3, dtype, 6)
    fn, _ = _fn("residual_restrict_axes", dtype)
    for mode in (P.REF_COMPAT, P.CORRECT):
        want = S.residual_restrict_axes(n3, rng, v, f, mask, mode, dtype)
        _check_transfer(ctx, lambda a, b, c, keep: fn(ctx._h, a, b, _ip(n3), _h(n3, rng, dtype), C.c_int(mode), c, _ip(cn), C.c_int(keep)), dtype,
                        n3, cn, v, f, want, mode)
