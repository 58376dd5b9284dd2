"""GPU suite: the z-slab entries of include/mgx.h, one by one, against whole-grid results of the oracle, bit for bit.

The slab driver (csrc/host/mg_dist3d.inc) is the only caller of these entries in the product, and the cycle tests see them only
through it: even offsets, the ranges of its schedule, a few cube-like sizes.  Here every entry runs on WINDOWS of a global array
(tests/slab_cases.py): offsets of either parity, windows that end on the grid's last plane, ranges that are empty, one plane next
to a ghost plane, the whole window, a part of it.  On the planes an entry says it writes it must give the bits of the whole-grid
operator on the global array; every other word of the window, pad entries included, must come back as it went in.  What an entry
may not read is poisoned (whole surplus planes on either side of its read set, and within the read planes the points its
comment in mgx.h excludes), so a NaN in a result is a read outside the contract -- the contract the overlap schedule of the
driver relies on when it launches an entry while a neighbour's ghost plane is still in flight.  Kernel names are asserted where
the context reports them, so that each launch path (relax3d_xs_kernel, its merged two-range launch, the pipelined smoothers, the
correcting pass, the fused black pass) provably ran on a slab whose end planes are ghosts."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import oracle as O
import pde_multigrid_amd as P
import slab_cases as S
from conftest import bits_equal
from odd_shapes import POISON, bits, pack_poisoned
from pde_multigrid_amd.multigrid import _ip, _rp, grid_spacing, xs_geometry
from solve_restated import close

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]  # anisotropic box: no spacing is a power of two, the residual divides
R3 = [0, 1, 0, 1, 0, 1]     # unit cube on 2^k + 1 points: the residual multiplies by exact reciprocals
DTYPES = [np.float64, np.float32]
TNAME = {np.float64: "double", np.float32: "float"}
L = P.lib
# every entry by name, (fp64, fp32)
ENTRIES = {
    "relax_colour_slab": (L.mgx3dxs_relax_colour_slab_f64, L.mgx3dxs_relax_colour_slab_f32),
    "relax_colour_slab2": (L.mgx3dxs_relax_colour_slab2_f64, L.mgx3dxs_relax_colour_slab2_f32),
    "relax_zero_colour_slab": (L.mgx3dxs_relax_zero_colour_slab_f64, L.mgx3dxs_relax_zero_colour_slab_f32),
    "residual_restrict_slab": (L.mgx3dxs_residual_restrict_slab_f64, L.mgx3dxs_residual_restrict_slab_f32),
    "residual_sumsq_slab": (L.mgx3dxs_residual_sumsq_slab_f64, L.mgx3dxs_residual_sumsq_slab_f32),
    "relax_rr_slab": (L.mgx3dxs_relax_rr_slab_f64, L.mgx3dxs_relax_rr_slab_f32),
    "relax_rr_takes": (L.mgx3dxs_relax_rr_takes_f64, L.mgx3dxs_relax_rr_takes_f32),
    "set_interior_slab": (L.mgx3dxs_set_interior_slab_f64, L.mgx3dxs_set_interior_slab_f32),
    "restrict_slab": (L.mgx3dxs_restrict_slab_f64, L.mgx3dxs_restrict_slab_f32),
    "interpolate_slab": (L.mgx3dxs_interpolate_slab_f64, L.mgx3dxs_interpolate_slab_f32),
    "interpolate_correct_slab": (L.mgx3dxs_interpolate_correct_slab_f64, L.mgx3dxs_interpolate_correct_slab_f32),
    "interpolate_correct_colour_slab": (L.mgx3dxs_interpolate_correct_colour_slab_f64, L.mgx3dxs_interpolate_correct_colour_slab_f32),
    "correct_pset_slab": (L.mgx3dxs_correct_pset_slab_f64, L.mgx3dxs_correct_pset_slab_f32),
    "relax_corr_colour_slab": (L.mgx3dxs_relax_corr_colour_slab_f64, L.mgx3dxs_relax_corr_colour_slab_f32),
    "corr_fused_takes": (L.mgx3dxs_corr_fused_takes_f64, L.mgx3dxs_corr_fused_takes_f32),
    "halo_pack": (L.mgx3dxs_halo_pack_f64, L.mgx3dxs_halo_pack_f32),
    "halo_unpack": (L.mgx3dxs_halo_unpack_f64, L.mgx3dxs_halo_unpack_f32),
    "halfplane_elems": (L.mgx3dxs_halfplane_elems_f64, L.mgx3dxs_halfplane_elems_f32),
}
for _f in ENTRIES["halfplane_elems"]:
    _f.restype = C.c_size_t


def E(name, dtype):
    return ENTRIES[name][0 if dtype == np.float64 else 1]


def _ct(dtype):
    return C.c_double if dtype == np.float64 else C.c_float


def _h(n3, rg, dtype):
    return _rp(grid_spacing(n3, rg, dtype), _ct(dtype))


def _i(*a):
    return [C.c_int(int(k)) for k in a]


def _rand(n3, dtype, seed):
    a = np.random.default_rng(seed).uniform(-1, 1, O.shape(n3)).astype(dtype)
    a.setflags(write=False)
    return a


def _pow2(n3):
    return all((k - 1) & (k - 2) == 0 for k in n3)


@functools.lru_cache(maxsize=None)
def _masks(n3):
    inside = S.interior_mask(n3)
    return inside, S.colour_mask(n3, 0), S.colour_mask(n3, 1)


def _set(ctx, params):
    for k, val in params.items():
        ctx.set_param(k, val)


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_rr():
    c = P.Context(0)
    c.set_param("rr3d.black", 2)  # the fused black pass takes every geometry
    yield c
    c.close()


def _windows(sz):
    """(off, nplanes): offsets 0, 1, 2, an even and an odd one in the middle, and a window that ends on the grid's last plane"""
    me = (sz // 2) & ~1
    out = {(sz - 5, 5)}
    for off in (0, 1, 2, me, me | 1):
        if min(sz - off, 6) >= 3:
            out.add((off, min(sz - off, 6)))
    return sorted(out)


def _ranges(npl):
    """local [zbeg, zend): empty, one plane next to the bottom ghost, one next to the top ghost, the whole window, the middle"""
    out = [(2, 2), (1, 2), (npl - 2, npl - 1), (1, npl - 1)]
    if npl >= 5:
        out.append((2, npl - 2))
    return out


# =================================================================================================== a. colour passes
@functools.lru_cache(maxsize=None)
def _colour_case(n3, dtype):
    v, f = _rand(n3, dtype, n3[0]), _rand(n3, dtype, n3[0] + 1)
    want = [O.relax_colour3d(n3, RG, v, f, c, dtype=dtype) for c in (0, 1)]
    zero = [O.relax_colour3d(n3, RG, np.zeros_like(v), f, c, dtype=dtype) for c in (0, 1)]
    return v, f, want, zero


def _colour_windows(n3, v, f, off, npl, runs, colour, zero):
    """the windows of v and f for a pass of `colour` over the local runs [zb, ze): what the pass may not read is poison"""
    inside, red, black = _masks(n3)
    upd = (red, black)[colour]
    updated = {off + z for zb, ze in runs for z in range(zb, ze)}
    readv = {off + z for zb, ze in runs if ze > zb for z in range(zb - 1, ze + 1)}
    vw, fw = S.window(v, off, npl), S.window(f, off, npl)
    if zero:  # garbage but for the boundary entries, which must be 0
        vw[...] = POISON[vw.dtype]
        for k in range(npl):
            vw[k][~inside[off + k]] = 0
    else:
        S.poison_planes(vw, off, readv)
        S.poison_points(vw, off, upd, planes=readv)  # no point of the updated colour is read, in the ghost planes or between them
    S.poison_planes(fw, off, updated)
    S.poison_points(fw, off, ~(upd & inside), planes=updated)  # f is read at the points the pass writes
    return vw, fw, sorted(updated), upd & inside


def _check_colour(ctx, n3, dtype, off, npl, runs, colour, zero=False, kernel=None, entry=None):
    v, f, want, wzero = _colour_case(n3, dtype)
    vw, fw, planes, mask = _colour_windows(n3, v, f, off, npl, runs, colour, zero)
    h = _h(n3, RG, dtype)
    name = entry or ("relax_zero_colour_slab" if zero else "relax_colour_slab")
    flat = [z for r in runs for z in r] if name == "relax_colour_slab2" else list(runs[0])
    got = S.run_slab(ctx, [vw, fw], lambda a, b: E(name, dtype)(ctx._h, a, b, *_i(n3[0], n3[1]), h, *_i(colour, *flat, off)), dtype)
    tag = (name, n3, off, npl, runs, colour)
    assert bits_equal(got[0], S.expected(vw, (wzero if zero else want)[colour], off, planes, mask)), tag
    assert bits_equal(got[1], fw), tag
    if kernel and planes:
        assert ctx.last_relax_kernel().startswith(kernel), (tag, ctx.last_relax_kernel())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", [(3, 5, 9), (21, 13, 29), (131, 7, 19), (513, 5, 11)])
def test_colour_pass_on_windows(ctx, n3, dtype):
    """relax3d_xs_kernel and relax3d_zero_colour_kernel: minimal axes, rows that end inside a tile, rows longer than a wave; the
    colour is folded from an offset of either parity"""
    for off, npl in _windows(n3[2]):
        for zb, ze in _ranges(npl):
            for colour in (0, 1):
                _check_colour(ctx, n3, dtype, off, npl, [(zb, ze)], colour, kernel="relax3d_xs_kernel<")
                _check_colour(ctx, n3, dtype, off, npl, [(zb, ze)], colour, zero=True)


PIPE = [((257, 67, 21), np.float32, 8), ((513, 67, 41), np.float64, 24)]  # pipe_min_planes of the rows


@pytest.mark.parametrize("n3,dtype,pmin", PIPE)
def test_colour_pass_both_sides_of_the_pipelined_switch(ctx, n3, dtype, pmin):
    """a run of pipe_min_planes planes takes the pipelined kernel, one plane less relax3d_xs_kernel; both ends of the run are
    ghost planes inside the grid, the offset odd and even"""
    for off in (1, 2):
        for run, kernel in ((pmin, "relax3d_xs_pipe_kernel<" + TNAME[dtype]), (pmin - 1, "relax3d_xs_kernel<")):
            for colour in (0, 1):
                _check_colour(ctx, n3, dtype, off, run + 2, [(1, run + 1)], colour, kernel=kernel)


SLAB2 = [((21, 13, 29), np.float64, None), ((21, 13, 29), np.float32, 8), ((131, 7, 19), np.float64, None), ((131, 7, 19), np.float32, 8),
         ((513, 67, 41), np.float64, 24), ((257, 67, 21), np.float32, 8)]


@pytest.mark.parametrize("n3,dtype,pmin", SLAB2)
def test_colour_pass_two_runs(ctx, n3, dtype, pmin):
    """relax_colour_slab2: runs that touch, runs apart, either run empty, a run long enough for the two-pass fallback; merged or
    not ("slab.edges_merged"), the same bits"""
    small = n3[1] - 2 < 16  # relax3d_xs_pass then launches fewer than 4 x 4 rows per workgroup: the merged launch shows in the name
    cases = [([(1, 3), (3, 5)], True), ([(1, 3), (6, 8)], True), ([(2, 2), (5, 8)], False), ([(1, 4), (7, 7)], False)]
    if pmin:
        cases.append(([(1, 1 + pmin), (2 + pmin, 4 + pmin)], False))  # the first run is one the pipelined kernel may take
    try:
        for off in (1, 2):
            for runs, mergeable in cases:
                npl = max(runs[1][1], runs[0][1]) + 1
                if off + npl > n3[2]:
                    continue
                for merged in (1, 0):
                    ctx.set_param("slab.edges_merged", merged)
                    for colour in (0, 1):
                        _check_colour(ctx, n3, dtype, off, npl, runs, colour, entry="relax_colour_slab2")
                        one_launch = ctx.last_relax_kernel().startswith("relax3d_xs_kernel<%s,4,4,0>" % TNAME[dtype])
                        if small:
                            assert one_launch == bool(merged and mergeable), (runs, merged, ctx.last_relax_kernel())
    finally:
        ctx.set_param("slab.edges_merged", 1)


# =================================================================================================== b. transfers
TRANSFER = [(133, 13, 29), (21, 13, 29), (17, 17, 17), (513, 9, 9), (129, 65, 33)]


def _coarse_ranges(cz, last):
    """[pzbeg, pzend) within [0, last): the first plane, the last, all, empty, one interior plane at either end, the interior"""
    out = [(0, 1), (last - 1, last), (0, last), (2, 2), (1, 2), (1, last - 1)]
    if last >= 5:
        out.append((2, last - 2))
    return out


@functools.lru_cache(maxsize=None)
def _transfer_case(n3, dtype):
    v, c = _rand(n3, dtype, n3[0] + 2), _rand(O.csize(n3), dtype, n3[0] + 3)
    zeros = np.zeros_like(v)
    return (v, c, O.restrict3d(n3, v, dtype=dtype), O.interpolate3d(n3, v, c, dtype=dtype),
            O.correct3d(n3, v, O.interpolate3d(n3, zeros, c, dtype=dtype), dtype=dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", TRANSFER)
def test_restrict_slab(ctx, n3, dtype):
    v, c, want = _transfer_case(n3, dtype)[:3]
    cn, sz = O.csize(n3), n3[2]
    for k, (pb, pe) in enumerate(_coarse_ranges(cn[2], cn[2])):
        lo = 2 * pb - 1 if pb >= 1 else 0
        hi = min(2 * pe - 1, sz - 1) if pe > pb else lo
        read = range(lo, hi + 1) if pe > pb else ()
        for below in (1, 2):  # fine offsets of either parity
            off, npl = S.span(lo, hi, sz, below, 2)
            coff, cnpl = S.span(pb, max(pe - 1, pb), cn[2], (k + below) & 1, 1)
            fw = S.poison_planes(S.window(v, off, npl), off, read)
            cw = S.poison_planes(S.window(c, coff, cnpl), coff, range(pb, pe))
            got = S.run_slab(ctx, [fw, cw], lambda a, b: E("restrict_slab", dtype)(ctx._h, a, _ip(n3), *_i(off), b, _ip(cn), *_i(coff, pb, pe)),
                             dtype)
            assert bits_equal(got[1], S.expected(cw, want, coff, range(pb, pe))), (n3, pb, pe, off, coff)
            assert bits_equal(got[0], fw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", TRANSFER)
def test_interpolate_slabs(ctx, n3, dtype):
    """interpolate_slab, interpolate_correct_slab and its colour forms over runs of cells; pz = 0 leaves fine plane 0 alone"""
    v, c, _, inter, corr = _transfer_case(n3, dtype)
    cn, sz = O.csize(n3), n3[2]
    inside, red, black = _masks(n3)
    variants = [("interpolate_slab", None, inter, inside), ("interpolate_correct_slab", None, corr, inside),
                ("interpolate_correct_colour_slab", -1, corr, inside), ("interpolate_correct_colour_slab", 0, corr, inside & red),
                ("interpolate_correct_colour_slab", 1, corr, inside & black)]
    for k, (pb, pe) in enumerate(_coarse_ranges(cn[2], cn[2] - 1)):
        planes = [z for pz in range(pb, pe) for z in (2 * pz, 2 * pz + 1) if z >= 1]
        lo, hi = (planes[0], planes[-1]) if planes else (2 * pb, 2 * pb)
        for below in (1, 2):
            off, npl = S.span(lo, hi, sz, below, 2)
            coff, cnpl = S.span(pb, pe, cn[2], (k + below) & 1, 1)
            cw = S.poison_planes(S.window(c, coff, cnpl), coff, range(pb, pe + 1) if pe > pb else ())
            for name, colour, want, mask in variants:
                vw = S.poison_planes(S.window(v, off, npl), off, planes)
                # plain Interpolate reads nothing of the fine array, a colour form nothing of the other colour
                S.poison_points(vw, off, inside if name == "interpolate_slab" else inside & ~mask, planes=set(planes))
                extra = [] if colour is None else _i(colour)
                got = S.run_slab(ctx, [vw, cw], lambda a, b: E(name, dtype)(ctx._h, a, _ip(n3), *_i(off), b, _ip(cn), *_i(coff, pb, pe), *extra),
                                 dtype)
                assert bits_equal(got[0], S.expected(vw, want, off, planes, mask)), (n3, name, colour, pb, pe, off, coff)
                assert bits_equal(got[1], cw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", TRANSFER)
def test_set_interior_slab(ctx, n3, dtype):
    g = _transfer_case(n3, dtype)[0]
    whole = O.set3d(n3, g, -7.25, 0, dtype=dtype)
    for off, npl in _windows(n3[2]):
        for zb, ze in [(0, 1), (0, npl), (npl - 1, npl)] + _ranges(npl):
            gw = S.window(g, off, npl)
            want = gw.copy()
            want[zb:ze, 1:-1, 1:-1] = -7.25
            for z in range(zb, ze):  # ... which on an interior plane of the grid is setToValue(.., false)
                if 1 <= off + z <= n3[2] - 2:
                    assert bits_equal(want[z], whole[off + z])
            got = S.run_slab(ctx, [gw], lambda a: E("set_interior_slab", dtype)(ctx._h, a, *_i(n3[0], n3[1], zb, ze), _ct(dtype)(-7.25)), dtype)
            assert bits_equal(got[0], want), (n3, off, npl, zb, ze)


@functools.lru_cache(maxsize=None)
def _residual_case(n3, dtype, unit):
    rg = R3 if unit else RG
    v, f = _rand(n3, dtype, n3[0] + 4), _rand(n3, dtype, n3[0] + 5)
    res = [O.residual3d(n3, rg, v, f, mode, dtype=dtype) for mode in (P.REF_COMPAT, P.CORRECT)]
    return rg, v, f, res, [O.restrict3d(n3, r, dtype=dtype) for r in res]


def _check_rr(ctx, n3, dtype, unit, mode, pb, pe, below, cbelow):
    rg, v, f, _, want = _residual_case(n3, dtype, unit)
    cn, sz = O.csize(n3), n3[2]
    p0, p1 = max(pb, 1), min(pe, cn[2] - 1)
    readv = range(2 * p0 - 2, 2 * p1 + 1) if p1 > p0 else ()
    readf = range(2 * p0 - 1, 2 * p1) if p1 > p0 else ()
    lo, hi = (readv[0], readv[-1]) if readv else (min(2 * pb, sz - 1), min(2 * pb, sz - 1))
    off, npl = S.span(lo, hi, sz, below, 2)
    coff, cnpl = S.span(pb, max(pe - 1, pb), cn[2], cbelow, 1)
    vw = S.poison_planes(S.window(v, off, npl), off, readv)
    fw = S.poison_planes(S.window(f, off, npl), off, readf)
    cw = S.poison_planes(S.window(_rand(cn, dtype, 9), coff, cnpl), coff, ())  # garbage everywhere: the entry writes the planes whole
    got = S.run_slab(ctx, [vw, fw, cw], lambda a, b, cc: E("residual_restrict_slab", dtype)(ctx._h, a, b, _ip(n3), *_i(off), _h(n3, rg, dtype),
                                                                                           *_i(mode), cc, _ip(cn), *_i(coff, pb, pe)),
                     dtype, zero_ok=(2,))
    assert bits_equal(got[2], S.expected(cw, want[mode], coff, range(pb, pe))), (n3, unit, mode, pb, pe, off, coff)
    assert bits_equal(got[0], vw) and bits_equal(got[1], fw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", TRANSFER)
def test_residual_restrict_slab(ctx, n3, dtype):
    """the kernel the level takes by itself ((129,65,33) with >= 8 coarse planes: the pipelined one), then the shuffle (stream 1) and
    the pipelined kernel (stream 2) forced, with runs of coarse planes that do not divide the range or exceed it"""
    cz = O.csize(n3)[2]
    ranges = _coarse_ranges(cz, cz)
    try:
        for unit in ([False, True] if _pow2(n3) else [False]):
            for k, (pb, pe) in enumerate(ranges):
                for mode in (P.REF_COMPAT, P.CORRECT):
                    _check_rr(ctx, n3, dtype, unit, mode, pb, pe, 1 + (k & 1), (k >> 1) & 1)
            for stream in (1, 2):
                for j, pzchunk in enumerate((1, 2, 3, 5, 8, 64)):
                    _set(ctx, {"residual_restrict3d.stream": stream, "residual_restrict3d.pzchunk": pzchunk})
                    for k, (pb, pe) in enumerate(((0, cz), (1, cz - 2), (2, 3))):
                        _check_rr(ctx, n3, dtype, unit, (j + k + stream) & 1, pb, pe, 1 + ((j + k) & 1), k & 1)
            _set(ctx, {"residual_restrict3d.stream": 3, "residual_restrict3d.pzchunk": 0})
    finally:
        _set(ctx, {"residual_restrict3d.stream": 3, "residual_restrict3d.pzchunk": 0})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", TRANSFER)
def test_residual_sumsq_slab(ctx, n3, dtype):
    """against math.fsum over the oracle's residual, to the relative 1e-13 of the whole-grid and _bc sum tests (test_gpu_shift.py,
    test_gpu_neumann.py); the same bits on a second run; exactly 0.0 for an empty range"""
    out = ctx.to_device(np.full(1, np.nan))
    try:
        for unit in ([False, True] if _pow2(n3) else [False]):
            rg, v, f, res, _ = _residual_case(n3, dtype, unit)
            for off, npl in _windows(n3[2]):
                for zb, ze in _ranges(npl):
                    for mode in (P.REF_COMPAT, P.CORRECT):
                        vw = S.poison_planes(S.window(v, off, npl), off, range(off + zb - 1, off + ze + 1) if ze > zb else ())
                        fw = S.poison_planes(S.window(f, off, npl), off, range(off + zb, off + ze))
                        sums = []
                        for rep in range(2):
                            got = S.run_slab(ctx, [vw, fw], lambda a, b: E("residual_sumsq_slab", dtype)(
                                ctx._h, a, b, *_i(n3[0], n3[1]), _h(n3, rg, dtype), *_i(mode, zb, ze), out), dtype)
                            assert bits_equal(got[0], vw) and bits_equal(got[1], fw)
                            sums.append(float(ctx.to_host(out, (1,), np.float64)[0]))
                        want = math.fsum((res[mode][off + zb:off + ze, 1:-1, 1:-1].astype(np.float64) ** 2).ravel())
                        print("sumsq", n3, np.dtype(dtype).name, unit, mode, off, zb, ze, sums[0], want)
                        assert bits_equal(np.array(sums[:1]), np.array(sums[1:])), "two runs gave different sums"
                        if ze == zb:
                            assert bits_equal(np.array(sums[:1]), np.zeros(1)), sums
                        else:
                            assert close(sums[0], want, 1e-13), (n3, unit, mode, off, zb, ze, sums[0], want)
    finally:
        ctx.free(out)


# =================================================================================================== c. relax_rr_slab
@functools.lru_cache(maxsize=None)
def _rr_case(n3, dtype, unit):
    rg = R3 if unit else RG
    v, f = _rand(n3, dtype, n3[0] + 6), _rand(n3, dtype, n3[0] + 7)
    blackpass = O.relax_colour3d(n3, rg, v, f, 1, dtype=dtype)
    coarse = [O.restrict3d(n3, O.residual3d(n3, rg, blackpass, f, mode, dtype=dtype), dtype=dtype) for mode in (P.REF_COMPAT, P.CORRECT)]
    return rg, v, f, blackpass, coarse


def _rr_windows(n3, v, f, pb, pe, fz, coff, dtype):
    cn, sz = O.csize(n3), n3[2]
    inside, red, black = _masks(n3)
    lo, hi = max(2 * pb - 3, 0), min(2 * pe + 1, sz - 1)
    npl = min(hi + 2, sz - 1) - fz + 1
    written = set(range(2 * pb - 1, 2 * pe))
    vw = S.poison_planes(S.window(v, fz, npl), fz, range(lo, hi + 1))
    # outside the planes it writes the entry reads red values only -- and the grid's planes 0 and sz - 1, which no pass writes
    zin = np.zeros_like(inside)
    zin[1:-1] = True
    S.poison_points(vw, fz, black & zin, planes=set(range(lo, hi + 1)) - written)
    fw = S.poison_planes(S.window(f, fz, npl), fz, range(max(2 * pb - 2, 0), min(2 * pe, sz - 1) + 1))
    cnpl = min(pe + 1, cn[2]) - coff
    cw = S.poison_planes(S.window(_rand(cn, dtype, 11), coff, cnpl), coff, range(pb, pe))
    return vw, fw, cw, sorted(written), black & inside


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", [(17, 9, 33), (129, 65, 65), (257, 65, 33)])
def test_relax_rr_slab(ctx_rr, n3, dtype):
    """the fused black pass + residual + restrict over one coarse plane, the first, the last, all: v gets the whole grid's black pass
    on the fine planes [2 pzbeg - 1, 2 pzend - 1] and nothing else, the black points outside them are never read"""
    ctx = ctx_rr
    cn = O.csize(n3)
    assert E("relax_rr_takes", dtype)(ctx._h, _ip(n3), _ip(cn)) == 1
    mid = cn[2] // 2
    for unit in (False, True):
        rg, v, f, blackpass, coarse = _rr_case(n3, dtype, unit)
        for k, (pb, pe) in enumerate([(mid, mid + 1), (1, 2), (cn[2] - 2, cn[2] - 1), (1, cn[2] - 1)]):
            lo = max(2 * pb - 3, 0)
            for j, fz in enumerate(sorted({lo - (lo & 1), max(lo - (lo & 1) - 2, 0)})):
                mode, coff = (k + j) & 1, max(pb - ((k + j) & 1), 0)
                vw, fw, cw, written, mask = _rr_windows(n3, v, f, pb, pe, fz, coff, dtype)
                got = S.run_slab(ctx, [vw, fw, cw], lambda a, b, cc: E("relax_rr_slab", dtype)(
                    ctx._h, a, b, _ip(n3), *_i(fz), _h(n3, rg, dtype), *_i(mode), cc, _ip(cn), *_i(coff, pb, pe)), dtype, zero_ok=(2,))
                tag = (n3, unit, mode, pb, pe, fz, coff)
                assert ctx.last_rr_kernel().startswith("relax_rr3d_xs_kernel<" + TNAME[dtype]), ctx.last_rr_kernel()
                assert bits_equal(got[0], S.expected(vw, blackpass, fz, written, mask)), tag
                assert bits_equal(got[2], S.expected(cw, coarse[mode], coff, range(pb, pe))), tag
                assert bits_equal(got[1], fw), tag


def test_relax_rr_slab_refusals(ctx_rr):
    """an odd fzoff, and a level relax_rr_takes does not take ("rr3d.black" = 1: fp32 never), are MGX_ERR_INVALID"""
    ctx, n3 = ctx_rr, (17, 9, 33)
    cn = O.csize(n3)

    def call(dtype, fz):
        v, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
        st = []
        S.run_slab(ctx, [v, f, np.zeros(O.shape(cn), dtype)], lambda a, b, cc: st.append(E("relax_rr_slab", dtype)(
            ctx._h, a, b, _ip(n3), *_i(fz), _h(n3, RG, dtype), *_i(0), cc, _ip(cn), *_i(0, 4, 6))) or 0, dtype)
        return st[0]

    for dtype in DTYPES:
        assert call(dtype, 1) == P.MGX_ERR_INVALID and call(dtype, 3) == P.MGX_ERR_INVALID
    ctx.set_param("rr3d.black", 1)
    try:
        assert E("relax_rr_takes", np.float32)(ctx._h, _ip(n3), _ip(cn)) == 0
        assert call(np.float32, 0) == P.MGX_ERR_INVALID
    finally:
        ctx.set_param("rr3d.black", 2)


# =================================================================================================== d. the correcting red pass
@functools.lru_cache(maxsize=None)
def _corr_case(n3, dtype):
    v, f, c = _rand(n3, dtype, n3[0] + 8), _rand(n3, dtype, n3[0] + 9), _rand(O.csize(n3), dtype, n3[0] + 10)
    vc = O.correct3d(n3, v, O.interpolate3d(n3, np.zeros_like(v), c, dtype=dtype), dtype=dtype)
    redpass = O.relax_colour3d(n3, RG, vc, f, 0, dtype=dtype)
    sweep = O.relax3d(n3, RG, vc, f, 1, dtype=dtype)
    assert bits_equal(sweep, O.relax_colour3d(n3, RG, redpass, f, 1, dtype=dtype))
    return v, f, c, vc, redpass, sweep


# (fzoff, zbeg, zend) on 21 planes: a run of 8 planes between two interior ghosts; short runs (the edge ranges of the driver), one with
# the grid's plane 0 as its lower ghost; a run whose upper ghost is the grid's last plane
CORR_RUNS = [(2, 1, 9), (0, 1, 4), (4, 2, 5), (10, 1, 10)]
CORR = [((257, 67, 21), np.float64, 7, "relax3d_xs_pipe_kernel<double,2,8,2", False),
        ((257, 67, 21), np.float32, 7, "relax3d_xs_pipe_kernel<float,2,8,2", False),
        ((513, 67, 21), np.float32, 7, "relax3d_xs_pipe_v2_kernel<float,2,8,2", False),  # unrolled: corrects its tile edges itself
        ((513, 67, 21), np.float32, 3, "relax3d_xs_pipe_v2_kernel<float,2,8,2", True)]   # rolled two-pair kernel: the set P is not empty


@pytest.mark.parametrize("n3,dtype,unroll,kernel,pset", CORR)
def test_correcting_red_pass_on_a_slab(ctx, n3, dtype, unroll, kernel, pset):
    """correct_pset_slab over the range and its ghost planes, then relax_corr_colour_slab, as the driver calls them; then the
    black pass: the planes equal the oracle's sweep on v + Interpolate(coarse_v)"""
    v, f, c, vc, redpass, sweep = _corr_case(n3, dtype)
    cn, sz = O.csize(n3), n3[2]
    inside, red, black = _masks(n3)
    h = _h(n3, RG, dtype)
    ctx.set_param("relax3d.unroll", unroll)
    try:
        for k, (fz, zb, ze) in enumerate(CORR_RUNS):
            assert E("corr_fused_takes", dtype)(ctx._h, _ip(n3), *_i(ze - zb)) == int(ze - zb >= 8)
            gb, ge = fz + zb, fz + ze
            npl = min(ge + 2, sz - 1) - fz + 1
            zmin, zmax = max(gb - 1, 1), min(ge + 1, sz - 1)
            clo, chi = (gb - 1) // 2, min((ge + 1) // 2, cn[2] - 1)
            coff = max(fz // 2 - (k & 1), 0)
            cw = S.poison_planes(S.window(c, coff, min(chi + 2, cn[2] - 1) - coff + 1), coff, range(clo, chi + 1))
            cplanes = chi - coff + 1  # the planes beyond ckmax are poison
            vw = S.poison_planes(S.window(v, fz, npl), fz, range(gb - 1, ge + 1))
            S.poison_points(vw, fz, red, planes=set(range(gb - 1, ge + 1)))  # neither entry reads a red value, on any plane
            fw = S.poison_planes(S.window(f, fz, npl), fz, range(gb, ge))
            vcw = S.window(vc, fz, npl)
            tag = (n3, fz, zb, ze, coff)

            def pset_call(a, cc):
                return E("correct_pset_slab", dtype)(ctx._h, a, _ip(n3), *_i(fz), cc, _ip(cn), *_i(coff, zmin, zmax))

            def red_call(a, b, cc):
                return E("relax_corr_colour_slab", dtype)(ctx._h, a, b, _ip(n3), *_i(fz), h, cc, _ip(cn), *_i(coff, cplanes, zb, ze))

            # the set P alone
            v1 = S.run_slab(ctx, [vw, cw], pset_call, dtype)[0]
            old, new = bits(v1) == bits(vw), bits(v1) == bits(vcw)
            may = np.zeros(vw.shape, bool)
            may[zmin - fz:zmax - fz] = (black & inside)[zmin:zmax]
            assert (old | (new & may)).all(), tag
            assert bool((~old).any()) == pset, (tag, int((~old).sum()))
            # both, back to back
            got = S.run_slab(ctx, [vw, fw, cw], lambda a, b, cc: pset_call(a, cc) or red_call(a, b, cc), dtype)
            assert ctx.last_corr_kernel().startswith(kernel) and ctx.last_corr_kernel().endswith(",2>"), ctx.last_corr_kernel()
            assert bits_equal(got[0], S.expected(v1, redpass, fz, range(gb, ge), red & inside)), tag  # 1. red, 2. black as the set P left it
            assert bits_equal(got[1], fw) and bits_equal(got[2], cw), tag
            # the ghost exchange brings the neighbours' new red values; then the black pass over the same range
            v3 = S.expected(got[0], redpass, fz, range(gb - 1, ge + 1), red)  # (on a face of the grid the red pass leaves v as it is)
            fb = S.poison_planes(S.window(f, fz, npl), fz, range(gb, ge))
            out = S.run_slab(ctx, [v3, fb], lambda a, b: E("relax_colour_slab", dtype)(ctx._h, a, b, *_i(n3[0], n3[1]), h, *_i(1, zb, ze, fz)),
                             dtype)
            want = S.expected(v3, sweep, fz, range(gb, ge), inside)
            assert bits_equal(out[0], want), tag
            assert bits_equal(want[zb:ze][:, 1:-1, 1:-1], sweep[gb:ge, 1:-1, 1:-1])  # 3. whole planes of the oracle's sweep
    finally:
        ctx.set_param("relax3d.unroll", 7)


@pytest.mark.parametrize("dtype", DTYPES)
def test_correcting_entries_refuse_a_level_the_kernel_does_not_run_on(ctx, dtype):
    """rows too short or too few, the switch off, an odd fzoff: MGX_ERR_INVALID and nothing launched; a short range of an accepted
    level is not refused (test_correcting_red_pass_on_a_slab runs them)"""
    def calls(n3, fz=2):
        cn = O.csize(n3)
        v, f, c = _rand(n3, dtype, 1), _rand(n3, dtype, 2), _rand(cn, dtype, 3)
        st = []
        out = S.run_slab(ctx, [v, f, c], lambda a, b, cc: st.extend([
            E("correct_pset_slab", dtype)(ctx._h, a, _ip(n3), *_i(fz), cc, _ip(cn), *_i(0, 3, 13)),
            E("relax_corr_colour_slab", dtype)(ctx._h, a, b, _ip(n3), *_i(fz), _h(n3, RG, dtype), cc, _ip(cn), *_i(0, cn[2], 2, 10))]) or 0, dtype)
        assert bits_equal(out[0], v)
        return st

    assert calls((131, 67, 21)) == [P.MGX_ERR_INVALID] * 2   # 65 pairs per row
    assert calls((257, 65, 21)) == [P.MGX_ERR_INVALID] * 2   # 63 interior rows
    assert E("corr_fused_takes", dtype)(ctx._h, _ip((257, 67, 21)), *_i(8)) == 1
    assert calls((257, 67, 21), fz=3)[1] == P.MGX_ERR_INVALID  # the slab must start on an even plane
    ctx.set_param("relax3d.corr_fuse", 0)
    try:
        assert E("corr_fused_takes", dtype)(ctx._h, _ip((257, 67, 21)), *_i(8)) == 0
        assert calls((257, 67, 21)) == [P.MGX_ERR_INVALID] * 2
    finally:
        ctx.set_param("relax3d.corr_fuse", 1)


# =================================================================================================== e. half planes
GUARD = 64


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sx,sy", [(131, 7), (515, 5), (257, 67), (3, 3)])
def test_halo_pack_unpack(sx, sy, dtype):
    """plane -> staging array -> a second plane, on both ranks of a LocalGroup(2) (no exchange is made): the colour's half-rows
    arrive whole, pads included, and nothing else of the staging array or the second plane is touched"""
    w = np.uint64 if dtype == np.float64 else np.uint32
    other = (bits(POISON[np.dtype(dtype)]) + w(1)).view(dtype)  # what the second plane holds before: a NaN of its own
    H, Pt = xs_geometry(sx, np.dtype(dtype).itemsize)
    elems = int(E("halfplane_elems", dtype)(*_i(sx, sy)))
    assert elems == sy * H
    ctxs = [P.Context(0), P.Context(0)]
    group = P.LocalGroup(2)
    try:
        for r, c in enumerate(ctxs):
            group.attach(c, r)
        rng = np.random.default_rng(sx + sy)
        for case, (ctx, z, colour, which) in enumerate((c, z, col, wh) for c in ctxs for z in (4, 7) for col in (0, 1) for wh in ("a", "b", "ab")):
            zs = {"a": z, "b": z + 1}
            src = {k: pack_poisoned(rng.uniform(-1, 1, (sy, sx)).astype(dtype)) for k in which}
            d_src = {k: ctx.to_device(src[k]) for k in which}
            d_stage = {k: ctx.to_device(np.full(elems + GUARD, POISON[np.dtype(dtype)], dtype)) for k in which}
            d_dst = {k: ctx.to_device(np.full((sy, Pt), other, dtype)) for k in which}
            try:
                P.check(E("halo_pack", dtype)(ctx._h, d_src.get("a"), *_i(zs["a"]), d_stage.get("a"), d_src.get("b"), *_i(zs["b"]), d_stage.get("b"),
                                              *_i(sx, sy, colour)))
                ctx.sync()  # the unpacking runs on the communication stream
                P.check(E("halo_unpack", dtype)(ctx._h, d_stage.get("a"), d_dst.get("a"), *_i(zs["a"]), d_stage.get("b"), d_dst.get("b"),
                                                *_i(zs["b"]), *_i(sx, sy, colour)))
                P.check(L.mgx_comm_wait(ctx._h))
                ctx.sync()
                for k in which:
                    want_stage = np.full(elems + GUARD, POISON[np.dtype(dtype)], dtype)
                    want_dst = np.full((sy, Pt), other, dtype)
                    for y in range(sy):
                        q = (colour + y + zs[k]) & 1
                        base, n = (H, Pt - H) if q else (0, H)
                        want_stage[y * H:y * H + n] = src[k][y, base:base + n]
                        want_dst[y, base:base + n] = src[k][y, base:base + n]  # the half whole: the colour's data entries and its pads
                    tag = (sx, sy, z, colour, which, k, case)
                    assert bits_equal(ctx.to_host(d_stage[k], (elems + GUARD,), dtype), want_stage), tag
                    assert bits_equal(ctx.to_host(d_dst[k], (sy, Pt), dtype), want_dst), tag
                    assert bits_equal(ctx.to_host(d_src[k], (sy, Pt), dtype), src[k]), tag
            finally:
                for d in (d_src, d_stage, d_dst):
                    for p in d.values():
                        ctx.free(p)
    finally:
        for c in ctxs:
            c.close()
        group.close()


def test_halo_entries_without_a_communicator_do_nothing(ctx):
    dtype, sx, sy = np.float64, 21, 5
    H, Pt = xs_geometry(sx, 8)
    src = pack_poisoned(np.random.default_rng(0).uniform(-1, 1, (sy, sx)))
    stage = np.full(sy * H, POISON[np.dtype(dtype)])
    d_src, d_stage = ctx.to_device(src), ctx.to_device(stage)
    try:
        P.check(E("halo_pack", dtype)(ctx._h, d_src, *_i(4), d_stage, None, *_i(5), None, *_i(sx, sy, 0)))
        P.check(E("halo_unpack", dtype)(ctx._h, d_stage, d_src, *_i(4), None, None, *_i(5), *_i(sx, sy, 0)))
        ctx.sync()
        assert bits_equal(ctx.to_host(d_stage, stage.shape, dtype), stage) and bits_equal(ctx.to_host(d_src, src.shape, dtype), src)
    finally:
        ctx.free(d_src)
        ctx.free(d_stage)
