"""GPU suite: where the head, the steady state and the tail of a run of planes meet or vanish in the three-pass launch
(csrc/mgx_block3d.hip, relax3d_xs_block3_kernel), against the oracle's colour passes, bit for bit.

A run relaxes three planes before its first store (head: general iterations up to an even plane), then pairs of iterations whose
plane bases advance by the pitch and that carry no range logic (steady state), then general iterations again from three planes
(the correcting launch: six) before the far z-face, or for an odd last plane (tail).  The shapes: 1, 3, 5 and 7 interior planes
(no steady state at all, then a few steady iterations, both z-faces inside head and tail); one tile and 65 planes in four runs
of 17, 17, 17 and 14 planes (first planes of both parities, interior run boundaries, a shorter last run); two x-tiles with a
partly filled last one and two y-tiles (the store and select masks formed once, on tile edges).

The launches alone: mgx3dxs_relax_block3_f64 with both first colours, in place (red or black stored) and out of place (both
stored), and mgx3dxs_relax_block3_corr_f64 -- anisotropic spacings that are no powers of two, random Dirichlet faces, every
interior entry of the stored colour NaN on input, pads checked unchanged."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import pde_multigrid_amd as P
from conftest import bits_equal
from pde_multigrid_amd._lib import check, lib
from pde_multigrid_amd.multigrid import _ip, _rp, grid_spacing, xs_geometry, xs_pack, xs_unpack

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]  # anisotropic box, spacings that are no powers of two
SHAPES = [(9, 9, 3), (9, 9, 5), (9, 9, 7), (9, 9, 9), (9, 9, 67), (131, 35, 21)]
PAD = 7.0


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


def _colour_mask(n3, colour):
    """interior points of `colour`: (x + y + z) % 2 == colour"""
    z, y, x = np.indices(tuple(reversed(n3)))
    m = (x + y + z) % 2 == colour
    m[0], m[-1], m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = False, False, False, False, False, False
    return m


def _passes(n3, v, f, colours):
    for c in colours:
        v = O.relax_colour3d(n3, RG, v, f, c, dtype=np.float64)
    return v


@pytest.fixture(scope="module")
def cases():
    """per shape: v, f, the coarse correction, and the three references (computed once, never written to)"""
    out = {}
    for n3 in SHAPES:
        r = np.random.default_rng(11 + n3[0] + 3 * n3[2])
        shape, cshape = tuple(reversed(n3)), tuple(reversed(P.coarse_size(n3)))
        v, f, c = r.uniform(-1, 1, shape), r.uniform(-1, 1, shape), r.uniform(-1, 1, cshape)
        w = O.correct3d(n3, v, O.interpolate3d(n3, v, c, dtype=np.float64), dtype=np.float64)
        out[n3] = dict(v=v, f=f, c=c, rbr=_passes(n3, v, f, [0, 1, 0]), brb=_passes(n3, v, f, [1, 0, 1]), corr=_passes(n3, w, f, [0, 1, 0]))
        for a in out[n3].values():
            a.setflags(write=False)
    return out


def _pads(n3):
    return xs_pack(np.ones(tuple(reversed(n3)))) == 0


def _device(ctx, a, n3):
    q = xs_pack(a)
    q[_pads(n3)] = PAD
    return ctx.to_device(q)


def _host(ctx, p, n3):
    """(the array unpacked, its pads unchanged?)"""
    raw = ctx.to_host(p, tuple(reversed(n3))[:-1] + (xs_geometry(n3[0], 8)[1],), np.float64)
    return xs_unpack(raw, n3[0]), bool(np.all(raw[_pads(n3)] == PAD))


def _launch(ctx, n3, vin, f, vout, first, store_both):
    h = _rp(grid_spacing(n3, RG, np.float64), C.c_double)
    ps = [_device(ctx, vin, n3), _device(ctx, f, n3)] + ([_device(ctx, vout, n3)] if vout is not None else [])
    try:
        check(lib.mgx3dxs_relax_block3_f64(ctx._h, ps[0], ps[-1] if vout is not None else ps[0], ps[1], _ip(n3), h, C.c_int(first),
                                           C.c_int(int(store_both))))
        return _host(ctx, ps[-1] if vout is not None else ps[0], n3)
    finally:
        for p in ps:
            ctx.free(p)


def _launch_corr(ctx, n3, v, f, c):
    h = _rp(grid_spacing(n3, RG, np.float64), C.c_double)
    cn = P.coarse_size(n3)
    ps = [_device(ctx, v, n3), _device(ctx, f, n3), _device(ctx, c, cn)]
    try:
        check(lib.mgx3dxs_relax_block3_corr_f64(ctx._h, ps[0], ps[1], _ip(n3), h, ps[2], _ip(cn)))
        got = _host(ctx, ps[0], n3)
        coarse_after, coarse_pads = _host(ctx, ps[2], cn)
        return got[0], got[1] and coarse_pads and bits_equal(coarse_after, c)
    finally:
        for p in ps:
            ctx.free(p)


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


def test_the_shapes_are_the_runs_they_are_meant_to_be():
    """one run everywhere but at 65 planes, where one tile gives four runs of 17, 17, 17 and 14 planes, on any device of 8 CUs or more"""
    for cus in (8, 80, 256, 304):
        for n3 in SHAPES:
            assert _run_starts(n3, cus) == ([1, 18, 35, 52] if n3[2] == 67 else [1]), (cus, n3)


@pytest.mark.parametrize("n3", SHAPES)
@pytest.mark.parametrize("first", [0, 1])
def test_in_place(ctx, cases, n3, first):
    """one colour stored, in place: its interior entries are NaN on input; the other colour and the faces stay as they were"""
    k = cases[n3]
    X, Y = _colour_mask(n3, first), _colour_mask(n3, 1 - first)
    want = np.array(k["rbr" if first == 0 else "brb"])
    want[Y] = k["v"][Y]  # the middle pass's colour is not stored
    vin = np.array(k["v"])
    vin[X] = np.nan
    got, pads_ok = _launch(ctx, n3, vin, k["f"], None, first, False)
    assert ctx.last_block3_kernel() == "relax3d_xs_block3_kernel<double,%d,false,16>" % first
    assert pads_ok
    assert bits_equal(got, want)


@pytest.mark.parametrize("n3", SHAPES)
@pytest.mark.parametrize("first", [0, 1])
def test_store_both_out_of_place(ctx, cases, n3, first):
    """both colours stored into a second array whose interior is NaN and whose faces are left alone"""
    k = cases[n3]
    interior = _colour_mask(n3, 0) | _colour_mask(n3, 1)
    vin = np.array(k["v"])
    vin[_colour_mask(n3, first)] = np.nan
    vout = np.random.default_rng(1).uniform(-1, 1, vin.shape)
    vout[interior] = np.nan
    want = np.array(k["rbr" if first == 0 else "brb"])
    want[~interior] = vout[~interior]
    got, pads_ok = _launch(ctx, n3, vin, k["f"], vout, first, True)
    assert ctx.last_block3_kernel() == "relax3d_xs_block3_kernel<double,%d,true,16>" % first
    assert pads_ok
    assert bits_equal(got, want)


@pytest.mark.parametrize("n3", SHAPES)
def test_correcting_launch(ctx, cases, n3):
    """R', B, R in place: red interior NaN on input; black, the faces, the pads and the coarse array stay as they were"""
    k = cases[n3]
    red = _colour_mask(n3, 0)
    want = np.array(k["v"])
    want[red] = k["corr"][red]
    vin = np.array(k["v"])
    vin[red] = np.nan
    got, untouched = _launch_corr(ctx, n3, vin, k["f"], np.array(k["c"]))
    assert ctx.last_block3_kernel() == "relax3d_xs_block3_kernel<double,0,false,16,corr>"
    assert untouched
    assert bits_equal(got, want)
