"""GPU suite: the way up's passes R', B, R as one in-place launch that reads black through the coarse-grid correction and stores
red only (relax3d_xs_block3_kernel, CORR, csrc/mgx_block3d.hip), against the oracle's Interpolate + ApplyCorrection + Relax
(N3/MultiGrid3D.cpp:638-645), bit for bit.

The launch alone (mgx3dxs_relax_block3_corr_f64) at sizes that end inside a tile and at one whose runs of planes start on planes
of both parities; the cycle-level entry (mgx3dxs_interpolate_correct_relax_block3) with "relax3d.block3_corr" on and off; whole
cycles of a hierarchy under both way-up knobs, eager against captured and replayed, and PCG."""
import numpy as np
import pytest

import oracle as O
import pde_multigrid_amd as P
from conftest import bits_equal

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]  # anisotropic box, spacings that are no powers of two
R3 = [0, 1, 0, 1, 0, 1]
B3C = "relax3d_xs_block3_kernel<double,0,false,16,corr>"
GEOMS = [(385, 129, 65), (387, 131, 67), (513, 129, 69), (449, 133, 71)]
# one x-tile of 60 pairs, y-tiles of 26 + 1 rows; a second x-tile of one pair; three x-tiles, three y-tiles; several runs of planes
SMALL = [(121, 29, 9), (123, 31, 13), (245, 59, 37), (385, 129, 69)]
KNOBS = ("relax3d.block3_corr", "relax3d.block3_up", "relax3d.block3")


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


def _reset(ctx):
    for k in KNOBS:
        ctx.set_param(k, 1)


def _data(n3, seed, dtype=np.float64):
    r = np.random.default_rng(seed)
    shape, cshape = tuple(reversed(n3)), tuple(reversed(P.coarse_size(n3)))
    return tuple(r.uniform(-1, 1, s).astype(dtype) for s in (shape, shape, cshape))


def _red_interior(n3):
    z, y, x = np.ogrid[:n3[2], :n3[1], :n3[0]]
    m = (x + y + z) % 2 == 0
    m[[0, -1], :, :] = False
    m[:, [0, -1], :] = False
    m[:, :, [0, -1]] = False
    return m


def _want_launch(n3, rg, v, f, c):
    """red interior points: R(B(R(v + Interpolate(c)))); everything else: v as it was"""
    w = O.correct3d(n3, v, O.interpolate3d(n3, v, c, dtype=np.float64), dtype=np.float64)
    for colour in (0, 1, 0):
        w = O.relax_colour3d(n3, rg, w, f, colour, dtype=np.float64)
    red = _red_interior(n3)
    out = v.copy()
    out[red] = w[red]
    return out


def _want(n3, rg, v, f, c, ncycles, dtype=np.float64):
    return O.relax3d(n3, rg, O.correct3d(n3, v, O.interpolate3d(n3, v, c, dtype=dtype), dtype=dtype), f, ncycles, dtype=dtype)


def _run_starts(n3, cus):
    """first planes of the launch's runs: relax3d_xs_block3_launch's geometry (tiles of 60 pairs x 26 rows, runs_filling_rounds)"""
    tiles, planes = -(-((n3[0] - 1) // 2) // 60) * -(-(n3[1] - 2) // 26), n3[2] - 2
    runs, best, c = 1, 0.0, 1
    while c <= 64 and (c == 1 or planes // c >= 16):
        wgs = tiles * c
        eff = wgs / (-(-wgs // cus) * cus) * planes / (planes + 4 * c)
        if eff > best + 1e-9:
            best, runs = eff, c
        if eff >= 0.9:
            break
        c += 1
    zrun = -(-planes // runs)
    return list(range(1, n3[2] - 1, zrun))


def test_the_largest_small_size_starts_runs_on_both_parities():
    """(385, 129, 69) is 20 tiles x 67 planes: four runs of 17 planes on every device of 80 CUs or more (MI355X: 256)"""
    for cus in (80, 128, 256, 304):
        starts = _run_starts(SMALL[3], cus)
        assert starts == [1, 18, 35, 52], (cus, starts)
        assert {s & 1 for s in starts} == {0, 1}


@pytest.fixture(scope="module")
def small_cases():
    out = {}
    for n3 in SMALL:
        v, f, c = _data(n3, 7 + n3[0] + n3[2])
        out[n3] = (v, f, c, _want_launch(n3, RG, v, f, c))
    return out


@pytest.mark.parametrize("n3", SMALL)
def test_launch_alone(ctx, small_cases, n3):
    v, f, c, want = small_cases[n3]
    got = P.ops3dxs.relax_block3_corr(ctx, v, f, n3, RG, c)
    assert ctx.last_block3_kernel() == B3C
    red = _red_interior(n3)
    assert bits_equal(got[red], want[red])
    assert bits_equal(got[~red], v[~red])  # black interior points and the faces stay as they were
    assert bits_equal(got, want)


def test_launch_reads_no_red_interior_value(ctx, small_cases):
    n3 = (245, 59, 37)
    v, f, c, want = small_cases[n3]
    vn = v.copy()
    vn[_red_interior(n3)] = np.nan
    got = P.ops3dxs.relax_block3_corr(ctx, vn, f, n3, RG, c)
    assert np.isfinite(got).all()
    assert bits_equal(got, want)


@pytest.mark.parametrize("n3", GEOMS)
@pytest.mark.parametrize("ncycles", [1, 2, 3, 4])
def test_cycle_entry_knob_on_and_off(ctx, n3, ncycles):
    rg = R3 if n3[0] == 513 else RG
    v, f, c = _data(n3, 13 * ncycles + n3[0])
    want = _want(n3, rg, v, f, c, ncycles)
    try:
        for knob in (1, 0):
            ctx.set_param("relax3d.block3_corr", knob)
            assert P.ops3dxs.block3_corr_takes(ctx, n3, ncycles) == (knob == 1 and ncycles >= 2)
            got = P.ops3dxs.interpolate_correct_relax_block3(ctx, v, f, n3, rg, c, ncycles)
            name = ctx.last_block3_kernel()
            assert bits_equal(got, want), (knob, ncycles)
            assert name == (B3C if knob == 1 and ncycles >= 2 else ""), (knob, ncycles, name)
    finally:
        _reset(ctx)


def test_not_taken_in_fp32(ctx):
    n3 = (513, 129, 65)
    v, f, c = _data(n3, 5, np.float32)
    assert not P.ops3dxs.block3_corr_takes(ctx, n3, 2, np.float32)
    got = P.ops3dxs.interpolate_correct_relax_block3(ctx, v, f, n3, R3, c, 2)
    assert ctx.last_block3_kernel() == ""
    assert bits_equal(got, _want(n3, R3, v, f, c, 2, np.float32))


def _hierarchy(ctx, n3, seed, use_graph=False):
    v, f, _ = _data(n3, seed)
    mg = P.MultiGrid3D(ctx, n3, RG, np.float64, residual_mode=P.CORRECT)
    mg.upload_v(0, v)
    mg.upload_f(0, f)
    mg.use_graph = use_graph
    return mg, v, f


def test_vcycles_under_both_way_up_knobs(ctx):
    n3 = (385, 129, 65)
    out = []
    try:
        for corr in (1, 0):
            for up in (1, 0):
                ctx.set_param("relax3d.block3_corr", corr)
                ctx.set_param("relax3d.block3_up", up)
                mg, v, f = _hierarchy(ctx, n3, 31)
                for _ in range(3):
                    mg.VCycle(0, 2, 2)
                out.append(mg.download_v(0))
                mg.close()
    finally:
        _reset(ctx)
    want = O.cycle3d(n3, RG, mode=0, v1=2, v2=2, reps=3, v=v, f=f, residual_mode=O.CORRECT, dtype=np.float64)
    assert np.isfinite(want).all()
    for i, got in enumerate(out):
        assert bits_equal(got, want), i


def test_graph_twin_with_the_knob_flipped(ctx):
    """captured and replayed cycles against eager ones, the knob flipped between cycles (each flip re-captures)"""
    n3 = (385, 129, 65)
    g, _, _ = _hierarchy(ctx, n3, 32, use_graph=True)
    e, _, _ = _hierarchy(ctx, n3, 32)
    try:
        for step, knob in enumerate((1, 1, 1, 0, 0, 1, 1, 0, 1)):
            ctx.set_param("relax3d.block3_corr", knob)
            g.VCycle(0, 2, 2)
            e.VCycle(0, 2, 2)
            ve = e.download_v(0)
            assert np.isfinite(ve).all(), step
            assert bits_equal(g.download_v(0), ve), (step, knob)
    finally:
        _reset(ctx)
        g.close()
        e.close()


def test_pcg_knob_on_and_off(ctx):
    n3 = (385, 129, 65)
    res = []
    try:
        for knob in (1, 0):
            ctx.set_param("relax3d.block3_corr", knob)
            mg, _, _ = _hierarchy(ctx, n3, 33)
            k, rel, conv, hist = mg.PCG(2, 2, 1e-9, 30)
            mg.VCycle(0, 2, 2)  # a cycle after PCG, on the path the knob chooses
            res.append((k, rel, conv, hist, mg.download_v(0)))
            mg.close()
    finally:
        _reset(ctx)
    (k1, r1, c1, h1, v1), (k0, r0, c0, h0, v0) = res
    assert k1 == k0 and r1 == r0 and c1 == c0
    assert bits_equal(h1, h0)
    assert bits_equal(v1, v0)


def test_knob_values(ctx):
    n3 = (385, 129, 65)
    try:
        for val in (0, 1):
            ctx.set_param("relax3d.block3_corr", val)
        with pytest.raises(P.MgxError):
            ctx.set_param("relax3d.block3_corr", 2)
        # three separate bits: the new switch leaves the way up's B, R, B launch and the way down's launch alone
        ctx.set_param("relax3d.block3_corr", 0)
        assert not P.ops3dxs.block3_corr_takes(ctx, n3, 2)
        assert P.ops3dxs.block3_up_takes(ctx, n3, 2)
        v, f, _ = _data(n3, 41)
        P.ops3dxs.smooth_residual_restrict(ctx, v, f, n3, RG, 2)
        assert ctx.last_block3_kernel() == "relax3d_xs_block3_kernel<double,0,false,16>"
        ctx.set_param("relax3d.block3_corr", 1)
        for other in ("relax3d.block3", "relax3d.block3_up"):
            ctx.set_param(other, 0)
            assert P.ops3dxs.block3_corr_takes(ctx, n3, 2)
            ctx.set_param(other, 1)
    finally:
        _reset(ctx)
