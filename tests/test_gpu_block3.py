"""GPU suite: three colour passes in one launch (csrc/mgx_block3d.hip, relax3d_xs_block3_kernel) against the oracle's colour
passes (MultiGrid3D::Relax, N3/MultiGrid3D.cpp:489-567), bit for bit.

Through mgx3dxs_relax_block3_f64 alone: x-rows whose last tile of 60 pairs is partly filled, y-tiles of 26 rows, runs of planes
of every length mod 4, random Dirichlet faces -- with every interior entry of the colour the launch writes set to NaN in its
input, which proves it never reads one (what makes the in-place launch of the way down race-free), and pads checked unchanged.
Through mgx3dxs_smooth_residual_restrict (the way down: R, B, R in one launch before the fused black pass + residual + restrict)
with "relax3d.block3" on and off, against Relax + CalculateResidual + Restrict."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import pde_multigrid_amd as P
from conftest import bits_equal
from pde_multigrid_amd._lib import check, lib
from pde_multigrid_amd.multigrid import _ip, _rp, grid_spacing, xs_geometry, xs_pack, xs_unpack

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]  # anisotropic box, spacings that are no powers of two: the residual divides
R3 = [0, 1, 0, 1, 0, 1]     # unit cube on 2^k + 1 points: the residual multiplies by exact reciprocals


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


def _data(n3, seed):
    r = np.random.default_rng(seed)
    shape = tuple(reversed(n3))
    return r.uniform(-1, 1, shape), r.uniform(-1, 1, shape)


def _colour_mask(n3, colour):
    """interior points of `colour`: (x + y + z) % 2 == colour"""
    z, y, x = np.indices(tuple(reversed(n3)))
    m = (x + y + z) % 2 == colour
    m[0], m[-1], m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = False, False, False, False, False, False
    return m


def _passes(n3, rg, v, f, colours):
    for c in colours:
        v = O.relax_colour3d(n3, rg, v, f, c, dtype=np.float64)
    return v


def _run_raw(ctx, n3, rg, vin, f, vout, first, store_both):
    """the launch on packed arrays whose pads hold a sentinel; returns (vout unpacked, its pads unchanged?)"""
    P_ = xs_geometry(n3[0], 8)[1]
    pads = xs_pack(np.ones(tuple(reversed(n3)))) == 0
    pi, pf = xs_pack(vin), xs_pack(f)
    pi[pads] = 7.0
    pv = ctx.to_device(pi)
    pff = ctx.to_device(pf)
    po = pv
    if vout is not None:
        q = xs_pack(vout)
        q[pads] = 7.0
        po = ctx.to_device(q)
    try:
        h = _rp(grid_spacing(n3, rg, np.float64), C.c_double)
        check(lib.mgx3dxs_relax_block3_f64(ctx._h, pv, po, pff, _ip(n3), h, C.c_int(first), C.c_int(int(store_both))))
        raw = ctx.to_host(po, tuple(reversed(n3))[:-1] + (P_,), np.float64)
        return xs_unpack(raw, n3[0]), bool(np.all(raw[pads] == 7.0))
    finally:
        for q in {pv.value: pv, pff.value: pff, po.value: po}.values():
            ctx.free(q)


GEOMS = [(9, 9, 9), (17, 33, 11), (129, 27, 13), (385, 129, 65), (387, 131, 67), (513, 35, 69), (515, 61, 71), (771, 29, 21),
         (1023, 33, 19)]


@pytest.mark.parametrize("n3", GEOMS)
@pytest.mark.parametrize("first", [0, 1])
def test_entry_in_place_never_reads_its_colour(ctx, n3, first):
    """store X only, in place: X interior of the input is NaN, Y and the faces stay as they were"""
    v, f = _data(n3, n3[0] + n3[2] + first)
    want = _passes(n3, RG, v, f, [first, 1 - first, first])
    want[_colour_mask(n3, 1 - first)] = v[_colour_mask(n3, 1 - first)]  # the middle pass's colour is not stored
    vin = v.copy()
    vin[_colour_mask(n3, first)] = np.nan
    got, pads_ok = _run_raw(ctx, n3, RG, vin, f, None, first, False)
    assert ctx.last_block3_kernel().startswith("relax3d_xs_block3_kernel<double,%d,false" % first), ctx.last_block3_kernel()
    assert pads_ok
    assert bits_equal(got, want)


@pytest.mark.parametrize("n3", GEOMS)
@pytest.mark.parametrize("first", [0, 1])
def test_entry_store_both(ctx, n3, first):
    """store both colours into a second array: vin's X interior and vout's interior are NaN; vout's faces are left alone"""
    v, f = _data(n3, 7 * n3[1] + first)
    want = _passes(n3, R3, v, f, [first, 1 - first, first])
    vin = v.copy()
    vin[_colour_mask(n3, first)] = np.nan
    vout = np.random.default_rng(1).uniform(-1, 1, v.shape)
    interior = _colour_mask(n3, 0) | _colour_mask(n3, 1)
    vout[interior] = np.nan
    want[~interior] = vout[~interior]
    got, pads_ok = _run_raw(ctx, n3, R3, vin, f, vout, first, True)
    assert pads_ok
    assert bits_equal(got, want)


def _way_down(ctx, n3, rg, v1, mode, block3):
    ctx.set_param("relax3d.block3", block3)
    try:
        v, f = _data(n3, v1 + 3 * mode)
        got_v, got_c = P.ops3dxs.smooth_residual_restrict(ctx, v, f, n3, rg, v1, False, False, mode)
        name = ctx.last_block3_kernel()
    finally:
        ctx.set_param("relax3d.block3", 1)
    want_v = O.relax3d(n3, rg, v, f, v1, dtype=np.float64)
    want_c = O.restrict3d(n3, O.residual3d(n3, rg, want_v, f, mode, dtype=np.float64), dtype=np.float64)
    assert bits_equal(got_v, want_v)
    assert bits_equal(got_c, want_c)
    return name


@pytest.mark.parametrize("n3", [(385, 129, 65), (387, 131, 67), (513, 129, 69)])
@pytest.mark.parametrize("v1", [1, 2, 3])
@pytest.mark.parametrize("mode", [P.REF_COMPAT, P.CORRECT])
def test_way_down_knob_on_and_off(ctx, n3, v1, mode):
    rg = R3 if n3[0] == 513 else RG
    name = _way_down(ctx, n3, rg, v1, mode, 1)
    assert name.startswith("relax3d_xs_block3_kernel<double,0,false") == (v1 >= 2), name
    assert ctx.last_rr_kernel().startswith("relax_rr3d_xs_kernel"), ctx.last_rr_kernel()
    assert _way_down(ctx, n3, rg, v1, mode, 0) == ""


def test_forced_rr_level_is_not_taken(ctx):
    """a level the fused black pass takes only under rr3d.black = 2 keeps its plain passes"""
    ctx.set_param("rr3d.black", 2)
    try:
        assert _way_down(ctx, (385, 35, 17), RG, 2, P.REF_COMPAT, 1) == ""
    finally:
        ctx.set_param("rr3d.black", 1)


def test_fp32_keeps_its_passes(ctx):
    n3 = (513, 129, 65)
    v, f = _data(n3, 5)
    v, f = v.astype(np.float32), f.astype(np.float32)
    got_v, _ = P.ops3dxs.smooth_residual_restrict(ctx, v, f, n3, R3, 2)
    assert ctx.last_block3_kernel() == ""
    assert bits_equal(got_v, O.relax3d(n3, R3, v, f, 2, dtype=np.float32))


def test_knob_values(ctx):
    with pytest.raises(P.MgxError):
        ctx.set_param("relax3d.block3", 2)
    ctx.set_param("relax3d.block3", 1)
