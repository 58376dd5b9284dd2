"""GPU suite: the way up's passes B, R, B after the correcting red pass R' as one launch (relax3d_xs_block3_kernel with both
colours stored, csrc/mgx_block3d.hip), against the oracle's Interpolate + ApplyCorrection + Relax (N3/MultiGrid3D.cpp:638-645),
bit for bit.

With a partner array w, R' reads black from v and writes red into w; the launch reads red and the faces from w and writes every
interior point of both colours into v.  Through mgx3dxs_interpolate_correct_relax_pp with a NaN partner (its faces copied
first) and with a partner whose faces the caller vouches for (w_rim_valid = 1, NaN interior); with "relax3d.block3_up" on and
off, every form of R' the fp64 path can take, and whole cycles of a hierarchy: eager against captured and replayed, and PCG."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import pde_multigrid_amd as P
from conftest import bits_equal
from pde_multigrid_amd._lib import check, lib
from pde_multigrid_amd.multigrid import _ip, _rp, grid_spacing, xs_pack, xs_unpack, xs_geometry

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]  # anisotropic box, spacings that are no powers of two
R3 = [0, 1, 0, 1, 0, 1]
B3 = "relax3d_xs_block3_kernel<double,1,true,16>"
# x-rows of 192 / 193 / 256 pairs; 224 pairs = 3 tiles of 60 + 44: the rows end inside a tile
GEOMS = [(385, 129, 65), (387, 131, 67), (513, 129, 69), (449, 133, 71)]


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


def _data(n3, seed, dtype=np.float64):
    r = np.random.default_rng(seed)
    shape, cshape = tuple(reversed(n3)), tuple(reversed(P.coarse_size(n3)))
    return tuple(r.uniform(-1, 1, s).astype(dtype) for s in (shape, shape, cshape))


def _want(n3, rg, v, f, c, ncycles, dtype=np.float64):
    return O.relax3d(n3, rg, O.correct3d(n3, v, O.interpolate3d(n3, v, c, dtype=dtype), dtype=dtype), f, ncycles, dtype=dtype)


def _with(ctx, params, fn):
    try:
        for k, val in params.items():
            ctx.set_param(k, val)
        return fn()
    finally:
        ctx.set_param("relax3d.block3_up", 1)
        ctx.set_param("relax3d.unroll", 7)
        ctx.set_param("relax3d.corr_low", 0)


@pytest.mark.parametrize("n3", GEOMS)
@pytest.mark.parametrize("ncycles", [1, 2, 3, 4])
def test_pp_knob_on_and_off(ctx, n3, ncycles):
    rg = R3 if n3[0] == 513 else RG
    v, f, c = _data(n3, 11 * ncycles + n3[0])
    want = _want(n3, rg, v, f, c, ncycles)
    for knob in (1, 0):
        got, name, corr = _with(ctx, {"relax3d.block3_up": knob},
                                lambda: (P.ops3dxs.interpolate_correct_relax_pp(ctx, v, f, n3, rg, c, ncycles), ctx.last_block3_kernel(),
                                         ctx.last_corr_kernel()))
        assert bits_equal(got, want), (knob, ncycles)
        taken = knob == 1 and ncycles >= 2
        assert name == (B3 if taken else ""), (knob, ncycles, name)
        assert corr.startswith("relax3d_xs_pipe_kernel<double,2,8,2,") and corr.endswith(",2>"), corr
        assert P.ops3dxs.block3_up_takes(ctx, n3, ncycles) == (ncycles >= 2)


@pytest.mark.parametrize("params", [{"relax3d.unroll": 6}, {"relax3d.corr_low": 1}], ids=["rolled", "corr_low"])
def test_pp_other_forms_of_the_correcting_pass(ctx, params):
    """R' out of place in its rolled form (pipe_unroll bit 0 off) and in 8-wave workgroups"""
    n3 = (387, 131, 67)
    v, f, c = _data(n3, 3)
    got, name, corr = _with(ctx, params, lambda: (P.ops3dxs.interpolate_correct_relax_pp(ctx, v, f, n3, RG, c, 2), ctx.last_block3_kernel(),
                                                  ctx.last_corr_kernel()))
    assert name == B3
    assert corr.startswith("relax3d_xs_pipe_kernel<double,2,%d,2," % (4 if "relax3d.corr_low" in params else 8)), corr
    assert bits_equal(got, _want(n3, RG, v, f, c, 2))


def test_pp_with_valid_rim(ctx):
    """w_rim_valid = 1: no boundary copy; w carries v's faces and NaN everywhere inside, pads NaN too"""
    n3 = (449, 133, 71)
    v, f, c = _data(n3, 9)
    w = v.copy()
    w[1:-1, 1:-1, 1:-1] = np.nan
    pads = xs_pack(np.ones(v.shape)) == 0
    pw = xs_pack(w)
    pw[pads] = np.nan
    h = _rp(grid_spacing(n3, RG, np.float64), C.c_double)
    cn = P.coarse_size(n3)
    ptrs = [ctx.to_device(a) for a in (xs_pack(v), pw, xs_pack(f), xs_pack(c))]
    try:
        check(lib.mgx3dxs_interpolate_correct_relax_pp_f64(ctx._h, ptrs[0], ptrs[1], ptrs[2], _ip(n3), h, ptrs[3], _ip(cn), C.c_int(3),
                                                           C.c_int(1)))
        assert ctx.last_block3_kernel() == B3
        P_ = xs_geometry(n3[0], 8)[1]
        got = xs_unpack(ctx.to_host(ptrs[0], tuple(reversed(n3))[:-1] + (P_,), np.float64), n3[0])
    finally:
        for p in ptrs:
            ctx.free(p)
    assert bits_equal(got, _want(n3, RG, v, f, c, 3))


def test_not_taken(ctx):
    """fp32, and the call without a partner array, keep the passes one launch each"""
    n3 = (513, 129, 65)
    v, f, c = _data(n3, 5, np.float32)
    got = P.ops3dxs.interpolate_correct_relax_pp(ctx, v, f, n3, R3, c, 2)
    assert ctx.last_block3_kernel() == ""
    assert not P.ops3dxs.block3_up_takes(ctx, n3, 2, np.float32)
    assert bits_equal(got, _want(n3, R3, v, f, c, 2, np.float32))
    v, f, c = _data(n3, 6)
    got = P.ops3dxs.interpolate_correct_relax(ctx, v, f, n3, R3, c, 2)
    assert ctx.last_block3_kernel() == ""
    assert bits_equal(got, _want(n3, R3, v, f, c, 2))


def _hierarchy(ctx, n3, seed, use_graph=False):
    v, f, _ = _data(n3, seed)
    mg = P.MultiGrid3D(ctx, n3, RG, np.float64, residual_mode=P.CORRECT)
    mg.upload_v(0, v)
    mg.upload_f(0, f)
    mg.use_graph = use_graph
    return mg, v, f


def test_vcycles_knob_on_and_off(ctx):
    n3 = (385, 129, 65)
    out = []
    for knob in (1, 0):
        ctx.set_param("relax3d.block3_up", knob)
        try:
            mg, v, f = _hierarchy(ctx, n3, 21)
            for _ in range(3):
                mg.VCycle(0, 2, 2)
            out.append(mg.download_v(0))
            mg.close()
        finally:
            ctx.set_param("relax3d.block3_up", 1)
    assert np.isfinite(out[0]).all()
    assert bits_equal(out[0], out[1])
    want = O.cycle3d(n3, RG, mode=0, v1=2, v2=2, reps=3, v=v, f=f, residual_mode=O.CORRECT, dtype=np.float64)
    assert bits_equal(out[0], want)


def test_graph_twin_with_the_knob_flipped(ctx):
    """captured and replayed cycles against eager ones, the knob flipped between cycles (each flip re-captures)"""
    n3 = (385, 129, 65)
    g, _, _ = _hierarchy(ctx, n3, 22, use_graph=True)
    e, _, _ = _hierarchy(ctx, n3, 22)
    try:
        for step, knob in enumerate((1, 1, 1, 0, 0, 1, 1, 0, 1)):
            ctx.set_param("relax3d.block3_up", knob)
            g.VCycle(0, 2, 2)
            e.VCycle(0, 2, 2)
            ve = e.download_v(0)
            assert np.isfinite(ve).all(), step
            assert bits_equal(g.download_v(0), ve), (step, knob)
    finally:
        ctx.set_param("relax3d.block3_up", 1)
        g.close()
        e.close()


def test_pcg_knob_on_and_off(ctx):
    n3 = (385, 129, 65)
    res = []
    for knob in (1, 0):
        ctx.set_param("relax3d.block3_up", knob)
        try:
            mg, _, _ = _hierarchy(ctx, n3, 23)
            k, rel, conv, hist = mg.PCG(2, 2, 1e-9, 30)
            mg.VCycle(0, 2, 2)  # a cycle after PCG (whose end invalidates the partner's faces)
            res.append((k, rel, conv, hist, mg.download_v(0)))
            mg.close()
        finally:
            ctx.set_param("relax3d.block3_up", 1)
    (k1, r1, c1, h1, v1), (k0, r0, c0, h0, v0) = res
    assert k1 == k0 and r1 == r0 and c1 == c0
    assert bits_equal(h1, h0)
    assert bits_equal(v1, v0)


def test_knob_values(ctx):
    for val in (0, 1):
        ctx.set_param("relax3d.block3_up", val)
    with pytest.raises(P.MgxError):
        ctx.set_param("relax3d.block3_up", 2)
    ctx.set_param("relax3d.block3_up", 1)
    # the two knobs are separate bits: the way down's switch leaves the way up's alone
    ctx.set_param("relax3d.block3", 0)
    try:
        assert P.ops3dxs.block3_up_takes(ctx, (385, 129, 65), 2)
    finally:
        ctx.set_param("relax3d.block3", 1)
