"""CPU suite: the harness of the z-slab entry tests (tests/slab_cases.py) on the oracle alone.  What test_gpu_slab_entries.py
expects of an entry is the whole-grid operator's result stitched into a window; stitched over a partition of the planes, the
windows must give back the whole-grid result, for any partition."""
import numpy as np
import pytest

import oracle as O
import slab_cases as S
from conftest import bits_equal
from odd_shapes import POISON
from solve_restated import boundary_mask

RG = [-1, 1, 0, 2, 0.5, 3]
DTYPES = [np.float64, np.float32]
SHAPES = [(9, 5, 13), (21, 13, 29), (5, 7, 9)]


def _rand(n3, dtype, seed):
    return np.random.default_rng(seed).uniform(-1, 1, O.shape(n3)).astype(dtype)


def _partitions(lo, hi):
    """[lo, hi) as one range, as single planes, and cut at uneven places (an empty range among them)"""
    yield [(lo, hi)]
    yield [(z, z + 1) for z in range(lo, hi)]
    a, b = lo + (hi - lo) // 3, lo + (hi - lo) // 3
    yield [(lo, a), (a, b), (b, hi - 1), (hi - 1, hi)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", SHAPES)
def test_colour_pass_stitched_over_a_partition(n3, dtype):
    v, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    sz = n3[2]
    for colour in (0, 1):
        want = O.relax_colour3d(n3, RG, v, f, colour, dtype=dtype)
        mask = S.colour_mask(n3, colour) & S.interior_mask(n3)
        assert bits_equal(want[~mask], v[~mask])  # the oracle's pass writes the colour's interior points and nothing else
        for parts in _partitions(1, sz - 1):
            got = v.copy()
            for zb, ze in parts:
                off, npl = S.span(zb - 1, ze, sz) if ze > zb else (zb, 1)
                w = S.expected(S.window(v, off, npl), want, off, range(zb, ze), mask)
                got[zb:ze] = w[zb - off:ze - off]  # a rank keeps the planes it updated
                rest = np.ones(npl, bool)
                rest[zb - off:ze - off] = False
                assert bits_equal(w[rest], v[off:off + npl][rest]), "a plane outside the range changed"
            assert bits_equal(got, want), (colour, parts)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", SHAPES)
def test_restrict_stitched_over_a_partition(n3, dtype):
    fine = _rand(n3, dtype, 3)
    cn = O.csize(n3)
    want = O.restrict3d(n3, fine, dtype=dtype)
    before = _rand(cn, dtype, 4)
    for parts in _partitions(0, cn[2]):
        got = before.copy()
        for pb, pe in parts:
            off, npl = S.span(pb, max(pe - 1, pb), cn[2])
            w = S.expected(S.window(before, off, npl), want, off, range(pb, pe))
            got[pb:pe] = w[pb - off:pe - off]
        assert bits_equal(got, want), parts


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n3", SHAPES)
def test_interpolate_and_correct_stitched_over_a_partition(n3, dtype):
    v, c = _rand(n3, dtype, 5), _rand(O.csize(n3), dtype, 6)
    cn = O.csize(n3)
    inter = O.interpolate3d(n3, v, c, dtype=dtype)
    corr = O.correct3d(n3, v, O.interpolate3d(n3, np.zeros_like(v), c, dtype=dtype), dtype=dtype)
    inside = S.interior_mask(n3)
    for want, mask in ((inter, inside), (corr, inside), (corr, inside & S.colour_mask(n3, 1))):
        for parts in _partitions(0, cn[2] - 1):  # the cells pz: fine planes 2 pz and 2 pz + 1
            got = v.copy()
            for pb, pe in parts:
                planes = [z for pz in range(pb, pe) for z in (2 * pz, 2 * pz + 1) if z >= 1]
                if not planes:
                    continue
                off, npl = S.span(planes[0], planes[-1], n3[2])
                w = S.expected(S.window(v, off, npl), want, off, planes, mask)
                got[planes[0]:planes[-1] + 1] = w[planes[0] - off:planes[-1] + 1 - off]
            full = v.copy()
            full[mask] = want[mask]
            assert bits_equal(got, full), parts
    assert bits_equal(inter[~inside], v[~inside]) and bits_equal(corr[~inside], v[~inside])


@pytest.mark.parametrize("n3", SHAPES + [(3, 3, 3)])
def test_masks(n3):
    assert np.array_equal(S.interior_mask(n3), ~boundary_mask(n3))
    red, black = S.colour_mask(n3, 0), S.colour_mask(n3, 1)
    assert red.shape == O.shape(n3) and np.array_equal(red, ~black)
    assert red[0, 0, 0] and black[0, 0, 1] and black[0, 1, 0] and black[1, 0, 0] and red[1, 1, 0]
    xy = S.xy_interior_mask(n3)
    assert np.array_equal(xy[1:-1], S.interior_mask(n3)[1:-1]) and xy[0, 1:-1, 1:-1].all() and not xy[:, 0].any() and not xy[:, :, -1].any()
    # a colour pass of the oracle changes the colour's interior points only
    v = np.random.default_rng(0).uniform(-1, 1, O.shape(n3))
    for colour, m in ((0, red), (1, black)):
        w = O.relax_colour3d(n3, RG, v, v, colour, dtype=np.float64)
        assert bits_equal(w[~(m & S.interior_mask(n3))], v[~(m & S.interior_mask(n3))])


@pytest.mark.parametrize("dtype", DTYPES)
def test_poison_survives_expected(dtype):
    n3 = (9, 5, 13)
    v, res = _rand(n3, dtype, 7), _rand(n3, dtype, 8)
    off, npl = S.span(4, 6, n3[2], below=2, above=2)
    assert (off, npl) == (2, 7)
    win = S.poison_planes(S.window(v, off, npl), off, keep=range(4, 7))
    red = S.colour_mask(n3, 0)
    S.poison_points(win, off, red, planes={4, 6})
    w = S.expected(win, res, off, [5], red & S.interior_mask(n3))
    assert S.is_poison(w[[0, 1, 5, 6]]).all()                       # the surplus planes, whole
    assert S.is_poison(w[2][red[4]]).all() and S.is_poison(w[4][red[6]]).all()
    assert bits_equal(w[2][~red[4]], v[4][~red[4]]) and not np.isnan(w[3][~red[5]]).any()
    m5 = (red & S.interior_mask(n3))[5]
    assert bits_equal(w[3][m5], res[5][m5]) and bits_equal(w[3][~m5], v[5][~m5])
    assert np.isnan(POISON[np.dtype(dtype)]) and S.span(0, 12, 13) == (0, 13)
