"""GPU suite: odd extents that are not 2^k + 1, against the oracle, bit for bit.

The library accepts every odd extent of at least 3 per axis.  On rows of 2^k + 1 points the number of x-pairs (sx - 1) / 2 is a
power of two and fills every x-tile of every kernel; on the rows here the LAST x-tile of a row is partly filled (the remainder
of each case is in its comment), the lanes past the row end are masked and the odd-x half of a row has pad entries.  Every case
names the kernel it is about (ctx.last_*_kernel), so a quiet fall-back to another kernel cannot pass for it.  The pad contract
(tests/odd_shapes.py): pads are never read as data, and a call writes them only when it zero-fills a whole array."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import pde_multigrid_amd as P
from conftest import bits_equal
from odd_shapes import hierarchy_ok, levels, pads_unchanged, run_poisoned
from pde_multigrid_amd.multigrid import _ip, _rp, xs_pack, xs_unpack

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]  # anisotropic box: no spacing is a power of two, the kernels divide
DTYPES = [np.float64, np.float32]
TNAME = {np.float64: "double", np.float32: "float"}
# the x-tiles: 128 pairs (fp64 pipelined smoother, 2 x 8 waves) ...
PIPE_X = [259, 383, 385, 387, 511]    # 129, 191, 192, 193, 255 pairs: 1, 63, 64, 65, 127 in the last tile
# ... and 256 pairs (fp32 two pairs per lane)
V2_X = [515, 517, 769, 771, 1023]     # 257, 258, 384, 385, 511 pairs: 1, 2, 128, 129, 255 in the last tile
LDS_SHAPES = [1282, 1442, 1242, 1422, 1184, 1424]  # MGX_LDS_SHAPES of the product build: 1000 + 100 WX + 10 WY + R


def pow2_box(n3):
    """a box on which every spacing is a power of two again (axis lengths (n - 1) / 2^j): the exact-reciprocal forms run"""
    return [0, (n3[0] - 1) / 256, 0, (n3[1] - 1) / 64, 0, (n3[2] - 1) / 32]


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


def _data(n3, dtype, seed):
    r = np.random.default_rng(seed)
    return r.uniform(-1, 1, O.shape(n3)).astype(dtype), r.uniform(-1, 1, O.shape(n3)).astype(dtype)


def _coarse(n3, dtype, seed):
    return np.random.default_rng(seed + 1).uniform(-1, 1, O.shape(O.csize(n3))).astype(dtype)


def _sweeps(n3, rg, v, f, kmax, dtype):
    """the oracle's Relax(1), Relax(2), ... Relax(kmax) of v (one sweep after the other)"""
    out, w = [v], v
    for _ in range(kmax):
        w = O.relax3d(n3, rg, w, f, 1, dtype=dtype)
        out.append(w)
    return out


def _pairs(sx):
    return (sx + 1) // 2 - 1


def _v2_takes(sx):
    """fp32 levels of >= 256 pairs run relax3d_xs_pipe_v2_kernel only when the pair count is even (csrc: pipe_v2_takes)"""
    return _pairs(sx) >= 256 and _pairs(sx) % 2 == 0


def _set(ctx, params):
    for k, v in params.items():
        ctx.set_param(k, v)


DEFAULTS = {"relax3d.zchunk": 0, "relax3d.unroll": 7, "relax3d.lds": -1, "relax3d.v2": 1, "relax3d.corr_fuse": 1, "relax3d.corr_v2": 1,
            "relax3d.corr_low": 0, "relax3d.zero_sweep": 1, "relax3d.resident": 1, "relax3d.resident_min": 3, "relax3d.resident_tile": 0,
            "relax3d.fused": 0, "relax3d.fused_mid": 1, "residual_restrict3d.stream": 3, "rr3d.black": 1}


@pytest.fixture
def knobs(ctx):
    """set_param for one test; everything it may touch is put back to the library defaults afterwards"""
    yield functools.partial(_set, ctx)
    _set(ctx, DEFAULTS)


# ------------------------------------------------------------------ colour passes and Relax(k): the pipelined smoothers
@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sx", PIPE_X)
def test_pipelined_smoother_partial_last_tile(ctx, knobs, sx, dtype):
    """relax3d_xs_pipe_kernel, 128-pair tiles: 65 rows (a partial y-tile too) and 65 planes (>= pipe_min_planes)"""
    n3 = (sx, 67, 67)
    v, f = _data(n3, dtype, sx)
    want = _sweeps(n3, RG, v, f, 3, dtype)
    name = "relax3d_xs_pipe_kernel<%s" % TNAME[dtype]
    for k in (1, 2, 3):
        assert bits_equal(P.ops3dxs.relax(ctx, v, f, n3, RG, k), want[k]), k
        assert ctx.last_relax_kernel().startswith(name), ctx.last_relax_kernel()
        assert bits_equal(P.ops3dxs.relax_pp(ctx, v, f, n3, RG, k), want[k]), ("pp", k)
    for zchunk in (0, 3, 8):
        for unroll in (7, 15, 31):
            knobs({"relax3d.zchunk": zchunk, "relax3d.unroll": unroll})
            assert bits_equal(P.ops3dxs.relax(ctx, v, f, n3, RG, 2), want[2]), (zchunk, unroll)
            assert ctx.last_relax_kernel().startswith(name), ctx.last_relax_kernel()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("code", LDS_SHAPES)
def test_pipelined_smoother_every_product_shape(ctx, knobs, code):
    """every workgroup shape of the product build: tiles of 64, 128 and 256 pairs, each left partly filled"""
    WX, WY, R = code // 100 % 10, code // 10 % 10, code % 10
    for n3, dtype in (((385, 67, 19), np.float64), ((771, 35, 11), np.float64), ((387, 35, 13), np.float32)):
        v, f = _data(n3, dtype, code + n3[0])
        want = O.relax3d(n3, RG, v, f, 2, dtype=dtype)
        takes = _pairs(n3[0]) >= 64 * WX and n3[1] - 2 >= WY * R
        for zchunk in (0, 3):
            knobs({"relax3d.lds": code, "relax3d.zchunk": zchunk})
            assert bits_equal(P.ops3dxs.relax(ctx, v, f, n3, RG, 2), want), (n3, zchunk)
            name = "relax3d_xs_pipe_kernel<%s,%d,%d,%d" % (TNAME[dtype], WX, WY, R) if takes else "relax3d_xs_kernel"
            assert ctx.last_relax_kernel().startswith(name), (n3, ctx.last_relax_kernel())


@pytest.mark.timeout(300)
@pytest.mark.parametrize("sx", V2_X)
def test_fp32_two_pairs_per_lane_partial_last_tile(ctx, knobs, sx):
    """relax3d_xs_pipe_v2_kernel, 256-pair tiles.  A lane owns two pairs or none: rows with an odd pair count (515, 771, 1023)
    run the one-pair kernel instead, which is asserted by name"""
    n3 = (sx, 67, 11)
    v, f = _data(n3, np.float32, sx)
    want = _sweeps(n3, RG, v, f, 3, np.float32)
    v2 = "relax3d_xs_pipe_v2_kernel<float" if _v2_takes(sx) else "relax3d_xs_pipe_kernel<float"
    for k in (1, 2, 3):
        assert bits_equal(P.ops3dxs.relax(ctx, v, f, n3, RG, k), want[k]), k
        assert ctx.last_relax_kernel().startswith(v2), ctx.last_relax_kernel()
    for on in (1, 0):
        for zchunk in (0, 3, 8):
            for unroll in (7, 15, 31):
                knobs({"relax3d.v2": on, "relax3d.zchunk": zchunk, "relax3d.unroll": unroll})
                assert bits_equal(P.ops3dxs.relax(ctx, v, f, n3, RG, 2), want[2]), (on, zchunk, unroll)
                name = v2 if on else "relax3d_xs_pipe_kernel<float"
                assert ctx.last_relax_kernel().startswith(name), (on, ctx.last_relax_kernel())


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n3,dtype", [((385, 67, 67), np.float64), ((387, 67, 67), np.float32), ((771, 67, 11), np.float32),
                                      ((517, 67, 11), np.float32), ((1023, 67, 27), np.float64)])
def test_relax_from_zero_and_zero_sweep(ctx, knobs, n3, dtype):
    """relax_from_zero with and without a zero rim; the first sweep as one launch (relax3d.zero_sweep, VAR 3 of the pipelined
    kernel) where the level takes it -- fp32 levels that run the two-pair kernel do not"""
    _, f = _data(n3, dtype, n3[0] + 5)
    zeros = np.zeros(O.shape(n3), dtype)
    garbage = np.full(O.shape(n3), np.nan, dtype)
    rim0 = garbage.copy()
    rim0[0], rim0[-1], rim0[:, 0], rim0[:, -1], rim0[:, :, 0], rim0[:, :, -1] = 0, 0, 0, 0, 0, 0
    want = _sweeps(n3, RG, zeros, f, 2, dtype)
    one_launch = _pairs(n3[0]) >= 128 and not (dtype == np.float32 and _v2_takes(n3[0]))
    for zs in (1, 0):
        knobs({"relax3d.zero_sweep": zs})
        for k in (1, 2):
            assert bits_equal(P.ops3dxs.relax_from_zero(ctx, garbage, f, n3, RG, k, False), want[k]), (zs, k)
            assert bits_equal(P.ops3dxs.relax_from_zero(ctx, rim0, f, n3, RG, k, True), want[k]), (zs, k, "rim")
            if k == 1:
                assert ctx.last_relax_kernel().endswith(",3>") == bool(zs and one_launch), ctx.last_relax_kernel()
        assert bits_equal(P.ops3d.relax_from_zero(ctx, rim0, f, n3, RG, 2, True), want[2]), (zs, "natural")


# ------------------------------------------------------------------ the correcting pass (Interpolate + ApplyCorrection + Relax)
@pytest.mark.timeout(300)
@pytest.mark.parametrize("n3,dtype", [((387, 67, 19), np.float64), ((259, 67, 13), np.float64), ((771, 67, 19), np.float32),
                                      ((517, 67, 19), np.float32), ((1023, 67, 11), np.float32)])
def test_interpolate_correct_relax(ctx, knobs, n3, dtype):
    v, f = _data(n3, dtype, n3[0] + 7)
    c = _coarse(n3, dtype, n3[0])
    corrected = O.correct3d(n3, v, O.interpolate3d(n3, np.zeros(O.shape(n3), dtype), c, dtype=dtype), dtype=dtype)
    want = _sweeps(n3, RG, corrected, f, 2, dtype)
    for fuse in (1, 0):
        for cv2 in (1, 0):
            for low in (0, 1):
                knobs({"relax3d.corr_fuse": fuse, "relax3d.corr_v2": cv2, "relax3d.corr_low": low})
                for k in (1, 2):
                    assert bits_equal(P.ops3dxs.interpolate_correct_relax(ctx, v, f, n3, RG, c, k), want[k]), (fuse, cv2, low, k)
                    if not fuse:
                        name = ""
                    elif dtype == np.float32 and cv2 and _v2_takes(n3[0]):
                        name = "relax3d_xs_pipe_v2_kernel<float,2,8,2"
                    elif dtype == np.float64 and low:
                        name = "relax3d_xs_pipe_kernel<double,2,4,2"
                    else:
                        name = "relax3d_xs_pipe_kernel<%s,2,8,2" % TNAME[dtype]
                    got = ctx.last_corr_kernel()
                    assert got.startswith(name) and (name or got == ""), (fuse, cv2, low, got)
    assert bits_equal(P.ops3d.interpolate_correct(ctx, v, n3, c), corrected)


# ------------------------------------------------------------------ the way down: residual + restrict, and the fused last black pass
@pytest.mark.timeout(300)
@pytest.mark.parametrize("n3", [(385, 67, 19), (771, 35, 11), (1023, 33, 9), (259, 131, 13)])
def test_residual_restrict_streams(ctx, knobs, n3):
    for rg in (RG, pow2_box(n3)):
        for dtype in DTYPES:
            v, f = _data(n3, dtype, n3[0] + 11)
            for mode in (P.REF_COMPAT, P.CORRECT):
                r = O.residual3d(n3, rg, v, f, mode, dtype=dtype)
                want = O.restrict3d(n3, r, dtype=dtype)
                assert bits_equal(P.ops3dxs.residual(ctx, v, f, n3, rg, mode), r), (rg, dtype, mode)
                assert bits_equal(P.ops3d.residual_restrict(ctx, v, f, n3, rg, mode), want), (rg, dtype, mode, "natural")
                for stream in (0, 1, 2, 3):
                    knobs({"residual_restrict3d.stream": stream})
                    assert bits_equal(P.ops3dxs.residual_restrict(ctx, v, f, n3, rg, mode), want), (rg, dtype, mode, stream)


def _check_rr(ctx, n3, rg, k, mode, dtype, fused):
    v, f = _data(n3, dtype, n3[0] + k)
    got_v, got_c = P.ops3dxs.smooth_residual_restrict(ctx, v, f, n3, rg, k, False, False, mode)
    assert ctx.last_rr_kernel().startswith("relax_rr3d_xs_kernel<%s" % TNAME[dtype]) == fused, ctx.last_rr_kernel()
    want_v = O.relax3d(n3, rg, v, f, k, dtype=dtype)
    assert bits_equal(got_v, want_v)
    assert bits_equal(got_c, O.restrict3d(n3, O.residual3d(n3, rg, want_v, f, mode, dtype=dtype), dtype=dtype))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", [(259, 67, 19), (385, 35, 17), (387, 67, 13), (515, 33, 11), (771, 35, 9)])
def test_smooth_residual_restrict_every_geometry(ctx, knobs, n3, dtype):
    """relax_rr3d_xs_kernel taking every geometry (rr3d.black = 2): tiles of 61 coarse columns, the row end moved around"""
    knobs({"rr3d.black": 2})
    for mode in (P.REF_COMPAT, P.CORRECT):
        for rg in (RG, pow2_box(n3)):
            _check_rr(ctx, n3, rg, 2, mode, dtype, True)
    _check_rr(ctx, n3, RG, 1, P.REF_COMPAT, dtype, True)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n3", [(385, 129, 65), (387, 131, 67)])
def test_smooth_residual_restrict_default_choice(ctx, n3):
    """the automatic choice takes the fused kernel on fp64 levels of x >= 385, y >= 129, z >= 65"""
    _check_rr(ctx, n3, RG, 1, P.REF_COMPAT, np.float64, True)
    _check_rr(ctx, n3, pow2_box(n3), 2, P.CORRECT, np.float64, True)


# ------------------------------------------------------------------ cache-resident levels: resident kernels, mid sweep
RESIDENT = [(75, 33, 129), (81, 129, 33), (97, 65, 67), (101, 41, 35), (131, 67, 45)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", RESIDENT)
def test_resident_and_mid_sweep(ctx, knobs, n3, dtype):
    """rows of 33 ... 129 points: the resident kernels (one lane per pair, the lanes past the row masked) and sweep3d_xs_mid_kernel;
    131-point rows are beyond both and take the colour passes"""
    v, f = _data(n3, dtype, n3[0] + 3)
    want = _sweeps(n3, RG, v, f, 3, dtype)
    fits = n3[0] <= 129
    for tile in (0, 8):
        knobs({"relax3d.resident": 1, "relax3d.resident_min": 1, "relax3d.resident_tile": tile})
        for k in (1, 2, 3):
            assert bits_equal(P.ops3dxs.relax(ctx, v, f, n3, RG, k), want[k]), (tile, k)
            assert ctx.last_relax_kernel().startswith("relax3d_xs_resident") == fits, ctx.last_relax_kernel()
            ctx.sync()
    knobs({"relax3d.resident": 0, "relax3d.fused_mid": 2})
    assert P.ops3dxs.relax_pp_takes(ctx, n3, 2, dtype) == fits
    for k in (2, 3):  # ping-pong sweeps (an odd count starts with one sweep of colour passes)
        assert bits_equal(P.ops3dxs.relax_pp(ctx, v, f, n3, RG, k), want[k]), ("mid", k)
        assert ctx.last_relax_kernel().startswith("sweep3d_xs_mid_kernel") == fits, ctx.last_relax_kernel()
    _, f2 = _data(n3, dtype, 1)
    zeros = np.zeros(O.shape(n3), dtype)
    assert bits_equal(P.ops3dxs.relax_from_zero(ctx, zeros, f2, n3, RG, 2, True), O.relax3d(n3, RG, zeros, f2, 2, dtype=dtype))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_launch_sweep_keeps_to_513_point_rows(ctx, knobs, dtype):
    """sweep3d_xs_kernel spans the whole x-extent with 256 pairs: wide rows of another length take the colour passes"""
    knobs({"relax3d.fused": 1, "relax3d.resident": 0})
    for n3 in ((515, 67, 67), (511, 67, 67)):
        v, f = _data(n3, dtype, n3[0])
        assert not P.ops3dxs.relax_pp_takes(ctx, n3, 2, dtype)
        assert bits_equal(P.ops3dxs.relax_pp(ctx, v, f, n3, RG, 2), O.relax3d(n3, RG, v, f, 2, dtype=dtype))
        assert not ctx.last_relax_kernel().startswith("sweep3d"), ctx.last_relax_kernel()


# ------------------------------------------------------------------ transfers, set, layout conversion
@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", [(259, 35, 9), (385, 17, 11), (515, 9, 13), (771, 11, 9), (1023, 13, 5), (99, 99, 99)])
def test_transfer_operators_and_layout(ctx, n3, dtype):
    v, f = _data(n3, dtype, n3[0] + 13)
    c = _coarse(n3, dtype, n3[0])
    for ops in (P.ops3d, P.ops3dxs):
        assert bits_equal(ops.restrict(ctx, v, n3), O.restrict3d(n3, v, dtype=dtype))
        assert bits_equal(ops.interpolate(ctx, v, n3, c), O.interpolate3d(n3, v, c, dtype=dtype))
        assert bits_equal(ops.apply_correction(ctx, v, n3, f), O.correct3d(n3, v, f, dtype=dtype))
        assert bits_equal(ops.interpolate_correct(ctx, v, n3, c),
                          O.correct3d(n3, v, O.interpolate3d(n3, v, c, dtype=dtype), dtype=dtype))
        for b in (0, 1):
            assert bits_equal(ops.set(ctx, v, n3, -7.25, b), O.set3d(n3, v, -7.25, b, dtype=dtype))
    assert bits_equal(P.ops3d.pack(ctx, v), xs_pack(v))
    assert bits_equal(P.ops3d.unpack(ctx, xs_pack(v), n3[0]), v)
    assert bits_equal(xs_unpack(xs_pack(v), n3[0]), v)


# ------------------------------------------------------------------ the pad contract
def _fn(name, dtype):
    return getattr(P.lib, "mgx3dxs_%s_%s" % (name, "f64" if dtype == np.float64 else "f32"))


def _h(n3, rg, dtype):
    return _rp(P.grid_spacing(n3, rg, dtype), C.c_double if dtype == np.float64 else C.c_float)


PAD_CASES = [((385, 67, 67), np.float64), ((771, 67, 11), np.float32), ((517, 67, 11), np.float32), ((97, 65, 67), np.float64),
             ((75, 33, 35), np.float32), ((387, 131, 67), np.float64)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n3,dtype", PAD_CASES)
def test_pads_are_never_read_nor_written(ctx, n3, dtype):
    """every array handed in with NaN pads: the data entries equal the oracle's, and the pads come back bit-identical -- or
    +0.0 where a call zero-fills a whole array (relax_from_zero without a zero rim, the coarse array of the way down)"""
    v, f = _data(n3, dtype, n3[0] + 17)
    cn = O.csize(n3)
    c = _coarse(n3, dtype, n3[0])
    ct = C.c_double if dtype == np.float64 else C.c_float
    h, N, CN = _h(n3, RG, dtype), _ip(n3), _ip(cn)
    sx, cx = n3[0], cn[0]

    def run(arrays, call, sxs, zero_ok=()):
        ups, outs = run_poisoned(ctx, arrays, call, dtype)
        for i, (u, o) in enumerate(zip(ups, outs)):
            assert pads_unchanged(u, o, sxs[i], zero_ok=i in zero_ok), i
        return [xs_unpack(o, s) for o, s in zip(outs, sxs)]

    want2 = O.relax3d(n3, RG, v, f, 2, dtype=dtype)
    got = run([v, f], lambda a, b: _fn("relax", dtype)(ctx._h, a, b, N, h, C.c_int(2)), [sx, sx])
    assert bits_equal(got[0], want2), ctx.last_relax_kernel()
    assert bits_equal(got[1], f)
    got = run([np.full_like(v, np.nan), f], lambda a, b: _fn("relax_from_zero", dtype)(ctx._h, a, b, N, h, C.c_int(2), C.c_int(0)),
              [sx, sx], zero_ok=(0,))
    assert bits_equal(got[0], O.relax3d(n3, RG, np.zeros_like(v), f, 2, dtype=dtype))
    corrected = O.correct3d(n3, v, O.interpolate3d(n3, np.zeros_like(v), c, dtype=dtype), dtype=dtype)
    got = run([v, f, c], lambda a, b, cc: _fn("interpolate_correct_relax", dtype)(ctx._h, a, b, N, h, cc, CN, C.c_int(1)), [sx, sx, cx])
    assert bits_equal(got[0], O.relax3d(n3, RG, corrected, f, 1, dtype=dtype)), ctx.last_corr_kernel()
    for mode in (P.REF_COMPAT, P.CORRECT):
        r = O.residual3d(n3, RG, v, f, mode, dtype=dtype)
        got = run([v, f, np.zeros_like(v)], lambda a, b, rr: _fn("residual", dtype)(ctx._h, a, b, rr, N, h, C.c_int(mode)), [sx, sx, sx])
        assert bits_equal(got[2], r)
        got = run([v, f, np.zeros_like(c)], lambda a, b, cc: _fn("residual_restrict", dtype)(ctx._h, a, b, N, h, C.c_int(mode), cc, CN),
                  [sx, sx, cx], zero_ok=(2,))
        assert bits_equal(got[2], O.restrict3d(n3, r, dtype=dtype))
        got = run([v, f, np.full_like(c, np.nan)],
                  lambda a, b, cc: _fn("smooth_residual_restrict", dtype)(ctx._h, a, b, N, h, C.c_int(2), C.c_int(0), C.c_int(0), C.c_int(mode),
                                                                          cc, CN, C.c_int(0)), [sx, sx, cx], zero_ok=(2,))
        assert bits_equal(got[0], want2), ctx.last_rr_kernel()
        assert bits_equal(got[2], O.restrict3d(n3, O.residual3d(n3, RG, want2, f, mode, dtype=dtype), dtype=dtype)), ctx.last_rr_kernel()
    got = run([v, np.zeros_like(c)], lambda a, cc: _fn("restrict", dtype)(ctx._h, a, N, cc, CN), [sx, cx], zero_ok=(1,))
    assert bits_equal(got[1], O.restrict3d(n3, v, dtype=dtype))
    got = run([v, c], lambda a, cc: _fn("interpolate", dtype)(ctx._h, a, N, cc, CN), [sx, cx])
    assert bits_equal(got[0], O.interpolate3d(n3, v, c, dtype=dtype))
    got = run([v, f], lambda a, b: _fn("apply_correction", dtype)(ctx._h, a, N, b, N), [sx, sx])
    assert bits_equal(got[0], O.correct3d(n3, v, f, dtype=dtype))
    for b in (0, 1):
        got = run([v], lambda a: _fn("set", dtype)(ctx._h, a, N, ct(-7.25), C.c_int(b)), [sx])
        assert bits_equal(got[0], O.set3d(n3, v, -7.25, b, dtype=dtype))


# ------------------------------------------------------------------ cycles on hierarchies that are odd at every level
CYCLES3 = [((385, 129, 65), DTYPES, (P.REF_COMPAT, P.CORRECT)), ((769, 129, 65), [np.float64], (P.REF_COMPAT,)),
           ((769, 129, 65), [np.float32], (P.CORRECT,)), ((1281, 129, 65), [np.float64], (P.CORRECT,)),
           ((1281, 129, 65), [np.float32], (P.REF_COMPAT,)), ((641, 257, 129), [np.float64], (P.REF_COMPAT,)),
           ((641, 257, 129), [np.float32], (P.CORRECT,))]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("n3,dtypes,modes", CYCLES3, ids=["%dx%dx%d-%d" % (c[0] + (i,)) for i, c in enumerate(CYCLES3)])
def test_3d_cycles_bit_identical(ctx, n3, dtypes, modes):
    assert hierarchy_ok(n3)
    for dtype in dtypes:
        v, f = _data(n3, dtype, sum(n3))
        for mode in modes:
            mg = P.MultiGrid3D(ctx, n3, RG, dtype, residual_mode=mode)
            assert [mg.size(i) for i in range(mg.numGrids)] == levels(n3)
            mg.upload_v(0, v)
            mg.upload_f(0, f)
            mg.VCycle(0, 2, 2)
            mg.VCycle(0, 2, 2)
            want = O.cycle3d(n3, RG, mode=0, v1=2, v2=2, reps=2, v=v, f=f, residual_mode=mode, dtype=dtype)
            assert bits_equal(mg.download_v(0), want), (dtype, mode, "V")
            mg.close()
            mg = P.MultiGrid3D(ctx, n3, RG, dtype, residual_mode=mode)
            mg.upload_v(0, v)
            mg.upload_f(0, f)
            mg.FullMultiGridVCycle(0, 1, 2, 2)
            want = O.cycle3d(n3, RG, mode=1, v0=1, v1=2, v2=2, v=v, f=f, residual_mode=mode, dtype=dtype)
            assert bits_equal(mg.download_v(0), want), (dtype, mode, "FMG")
            mg.close()


@pytest.mark.timeout(300)
def test_3d_cycle_graph_replay(ctx):
    n3, dtype = (385, 129, 65), np.float64
    v, f = _data(n3, dtype, 5)
    mg = P.MultiGrid3D(ctx, n3, RG, dtype)
    mg.use_graph = True
    mg.upload_v(0, v)
    mg.upload_f(0, f)
    for _ in range(3):  # the first cycle runs eagerly and is captured, the others replay the graph
        mg.VCycle(0, 2, 2)
    want = O.cycle3d(n3, RG, mode=0, v1=2, v2=2, reps=3, v=v, f=f, dtype=dtype)
    assert bits_equal(mg.download_v(0), want)
    mg.close()


A2 = [-1.0, -2.0, 0.0, -3.0]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n2", [(193, 65), (385, 129), (1537, 513)])
def test_2d_cycles_bit_identical(ctx, n2, dtype):
    """2D hierarchies odd at every level: cache-resident cycle tiles of 16 / 32 / 64 and the one-workgroup tail"""
    assert hierarchy_ok(n2)
    rg = [0, 1, 0, 2]
    r = np.random.default_rng(sum(n2))
    v, f = r.uniform(-1, 1, O.shape(n2)).astype(dtype), r.uniform(-1, 1, O.shape(n2)).astype(dtype)
    for fuse in (True, 1, 0):
        mg = P.MultiGrid2D(ctx, n2, rg, A2, 2, dtype, fuse=fuse)
        mg.upload_v(0, v)
        mg.upload_f(0, f)
        mg.VCycle(0, 2, 2)
        mg.VCycle(0, 2, 2)
        assert bits_equal(mg.download_v(0), O.cycle2d(n2, rg, A2, 2, mode=0, v1=2, v2=2, reps=2, v=v, f=f, dtype=dtype)), (fuse, "V")
        mg.close()
    mg = P.MultiGrid2D(ctx, n2, rg, A2, 2, dtype)
    mg.upload_v(0, v)
    mg.upload_f(0, f)
    mg.FullMultiGridVCycle(0, 1, 2, 2)
    assert bits_equal(mg.download_v(0), O.cycle2d(n2, rg, A2, 2, mode=1, v0=1, v1=2, v2=2, v=v, f=f, dtype=dtype)), "FMG"
    mg.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n2", [(131, 67), (259, 35), (515, 19)])
def test_2d_operators(ctx, n2, dtype):
    rg = [0, 1, 0, 2]
    r = np.random.default_rng(sum(n2))
    v, f = r.uniform(-1, 1, O.shape(n2)).astype(dtype), r.uniform(-1, 1, O.shape(n2)).astype(dtype)
    c = r.uniform(-1, 1, O.shape(O.csize(n2))).astype(dtype)
    for k in (1, 2):
        assert bits_equal(P.ops2d.relax(ctx, v, f, n2, rg, A2, 2, k), O.relax2d(n2, rg, A2, 2, v, f, k, dtype=dtype))
    res = O.residual2d(n2, rg, A2, 2, v, f, dtype=dtype)
    assert bits_equal(P.ops2d.residual(ctx, v, f, n2, rg, A2, 2), res)
    assert bits_equal(P.ops2d.residual_restrict(ctx, v, f, n2, rg, A2, 2), O.restrict2d(n2, res, dtype=dtype))
    assert bits_equal(P.ops2d.restrict(ctx, v, n2), O.restrict2d(n2, v, dtype=dtype))
    assert bits_equal(P.ops2d.interpolate(ctx, v, n2, c), O.interpolate2d(n2, v, c, dtype=dtype))
    assert bits_equal(P.ops2d.interpolate_correct(ctx, v, n2, c), O.correct2d(n2, v, O.interpolate2d(n2, v, c, dtype=dtype), dtype=dtype))
    for k in (1, 2):
        w = O.relax2d(n2, rg, A2, 2, v, f, k, dtype=dtype)
        got_v, got_c = P.ops2d.relax_residual_restrict(ctx, v, f, n2, rg, A2, 2, k)
        assert bits_equal(got_v, w), k
        assert bits_equal(got_c, O.restrict2d(n2, O.residual2d(n2, rg, A2, 2, w, f, dtype=dtype), dtype=dtype)), k
        corrected = O.correct2d(n2, v, O.interpolate2d(n2, np.zeros_like(v), c, dtype=dtype), dtype=dtype)
        assert bits_equal(P.ops2d.interpolate_correct_relax(ctx, v, f, n2, rg, A2, 2, c, k),
                          O.relax2d(n2, rg, A2, 2, corrected, f, k, dtype=dtype)), k


# ------------------------------------------------------------------ the slab driver
@functools.lru_cache(maxsize=None)
def _dist_case(dtype):
    n3 = (769, 129, 129)
    v, f = _data(n3, dtype, 769)
    return n3, v, f, O.cycle3d(n3, RG, mode=0, v1=2, v2=2, reps=2, v=v, f=f, dtype=dtype)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("nranks,dtype,ca", [(2, np.float64, None), (4, np.float64, None), (2, np.float64, 0), (4, np.float64, 0),
                                             (4, np.float32, None)])
def test_slab_driver_bit_identical(nranks, dtype, ca):
    from test_gpu_dist import run_ranks
    n3, v, f, want = _dist_case(dtype)
    assert hierarchy_ok(n3)
    got, info = run_ranks(nranks, n3, RG, dtype, 2, 2, 2, 4, v0=v, f0=f, inline_bytes=None, ca_min_planes=ca)
    assert all(nd >= 1 for nd, _ in info.values()), info
    assert bits_equal(got, want)


# ------------------------------------------------------------------ the size contract
@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", DTYPES)
def test_hierarchy_that_reaches_an_even_extent(ctx, dtype):
    """97 -> 49 -> 25 -> 13 -> 7 -> 4: six levels by the reference's rule, the last one even.  The constructor refuses that
    (as the reference's Grid3D asserts) and builds the five odd levels when only those are asked for"""
    n3 = (97, 97, 97)
    assert not hierarchy_ok(n3) and hierarchy_ok(n3, 5)
    with pytest.raises(P.MgxError) as e:
        P.MultiGrid3D(ctx, n3, RG, dtype)
    assert e.value.status == P.MGX_ERR_SIZE
    v, f = _data(n3, dtype, 97)
    for mode in (P.REF_COMPAT, P.CORRECT):
        mg = P.MultiGrid3D(ctx, n3, RG, dtype, nlevels=5, residual_mode=mode)
        assert mg.numGrids == 5
        mg.upload_v(0, v)
        mg.upload_f(0, f)
        mg.VCycle(0, 2, 2)
        mg.VCycle(0, 2, 2)
        assert bits_equal(mg.download_v(0), O.cycle3d(n3, RG, nlevels=5, mode=0, v1=2, v2=2, reps=2, v=v, f=f, residual_mode=mode, dtype=dtype))
        mg.close()
        mg = P.MultiGrid3D(ctx, n3, RG, dtype, nlevels=5, residual_mode=mode)
        mg.upload_v(0, v)
        mg.upload_f(0, f)
        mg.FullMultiGridVCycle(0, 1, 2, 2)
        assert bits_equal(mg.download_v(0), O.cycle3d(n3, RG, nlevels=5, mode=1, v0=1, v1=2, v2=2, v=v, f=f, residual_mode=mode, dtype=dtype))
        mg.close()
    got = P.solve3d(ctx, v, f, RG, nlevels=5)
    assert bits_equal(got, O.cycle3d(n3, RG, nlevels=5, mode=0, v1=2, v2=2, v=v, f=f, dtype=dtype))
    with pytest.raises(P.MgxError) as e:
        P.solve3d(ctx, v, f, RG)
    assert e.value.status == P.MGX_ERR_SIZE
