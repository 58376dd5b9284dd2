"""CPU suite: the oracle itself on odd extents that are not 2^k + 1.

tests/test_oracle_vs_ref.py pins the oracle to the compiled reference on cubic 2^k + 1 grids only (the reference builds no other
hierarchy).  Here a small vectorised numpy model of the 3D operators, restated from oracle/mg_oracle.hpp and evaluated in
np.longdouble, checks the oracle's fp64 instantiation on anisotropic odd shapes, so that the GPU tests on such shapes compare
the kernels with something that is right there too."""
import numpy as np
import pytest

import oracle as O

LD = np.longdouble
SHAPES = [(11, 7, 9), (23, 13, 5), (35, 19, 27), (5, 3, 7)]
RANGES = [[-1, 1, 0, 2, 0.5, 3], [0, 1, 0, 1, 0, 1]]


def _h2(n, rng):
    # h = range / (size - 1) in the oracle's real type (fp64 here); squared in high precision
    return [LD((np.float64(rng[2 * d + 1]) - np.float64(rng[2 * d])) / np.float64(n[d] - 1)) ** 2 for d in range(3)]


def _interior(n):
    s = [slice(1, k - 1) for k in reversed(n)]
    return tuple(s)


def _parity(n):
    z, y, x = np.meshgrid(*[np.arange(k) for k in reversed(n)], indexing="ij")
    return (x + y + z) % 2


def model_relax(n, rng, v, f, ncycles):
    """ncycles x (red pass: interior points with (x + y + z) even, black pass: odd), each a Gauss-Seidel update from the
    other colour only, so a whole colour is one vectorised step"""
    hx2, hy2, hz2 = _h2(n, rng)
    v = v.astype(LD).copy()
    f = f.astype(LD)
    I = _interior(n)
    par = _parity(n)[I]
    for _ in range(ncycles):
        for colour in (0, 1):
            O_, E_ = v[1:-1, 1:-1, :-2], v[1:-1, 1:-1, 2:]
            N_, S_ = v[1:-1, :-2, 1:-1], v[1:-1, 2:, 1:-1]
            D_, U_ = v[:-2, 1:-1, 1:-1], v[2:, 1:-1, 1:-1]
            new = ((O_ + E_) * (hy2 * hz2) + (N_ + S_) * (hx2 * hz2) + (D_ + U_) * (hx2 * hy2) - f[I] * hx2 * hy2 * hz2) / (
                2 * (hy2 * hz2 + hx2 * hz2 + hx2 * hy2))
            v[I] = np.where(par == colour, new, v[I])
    return v


def model_residual(n, rng, v, f, mode):
    """f - Laplacian(v) on the interior, 0 on the boundary.  REF_COMPAT keeps the reference's sign quirk: the y and z terms
    are (N - 2v - S) / hy2 and (D - 2v - U) / hz2 (oracle/mg_oracle.hpp, residual3)"""
    hx2, hy2, hz2 = _h2(n, rng)
    v = v.astype(LD)
    r = np.zeros(v.shape, LD)
    I = _interior(n)
    c = v[I]
    O_, E_ = v[1:-1, 1:-1, :-2], v[1:-1, 1:-1, 2:]
    N_, S_ = v[1:-1, :-2, 1:-1], v[1:-1, 2:, 1:-1]
    D_, U_ = v[:-2, 1:-1, 1:-1], v[2:, 1:-1, 1:-1]
    s = -1 if mode == O.REF_COMPAT else 1
    r[I] = f[I].astype(LD) - (O_ - 2 * c + E_) / hx2 - (N_ - 2 * c + s * S_) / hy2 - (D_ - 2 * c + s * U_) / hz2
    return r


def model_restrict(n, fine):
    """27-point full weighting (1/8 centre, 1/16 faces, 1/32 edges, 1/64 corners) on the interior, injection on the boundary"""
    fine = fine.astype(LD)
    w1 = np.array([0.25, 0.5, 0.25], LD)
    cn = O.csize(n)
    coarse = fine[::2, ::2, ::2].copy()
    pz, py, px = np.meshgrid(*[np.arange(1, k - 1) for k in reversed(cn)], indexing="ij")
    acc = np.zeros(pz.shape, LD)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                acc += w1[dz + 1] * w1[dy + 1] * w1[dx + 1] * fine[2 * pz + dz, 2 * py + dy, 2 * px + dx]
    coarse[1:-1, 1:-1, 1:-1] = acc
    return coarse


def _lin(a, axis, m):
    """linear interpolation along `axis` onto m = 2 (len - 1) + 1 points"""
    a = np.moveaxis(a, axis, 0)
    out = np.empty((m,) + a.shape[1:], LD)
    out[0::2] = a
    out[1::2] = (a[:-1] + a[1:]) / 2
    return np.moveaxis(out, 0, axis)


def model_interpolate(n, fine, coarse):
    """trilinear interpolation of the coarse grid onto the interior points; the fine boundary is kept"""
    e = coarse.astype(LD)
    for axis, k in ((0, n[2]), (1, n[1]), (2, n[0])):
        e = _lin(e, axis, k)
    out = fine.astype(LD).copy()
    I = _interior(n)
    out[I] = e[I]
    return out


def model_correct(n, fine, err):
    out = fine.astype(LD).copy()
    I = _interior(n)
    out[I] += err.astype(LD)[I]
    return out


def _close(got, want, tol=1e-13):
    want = np.asarray(want, LD)
    scale = np.max(np.abs(want))
    return float(np.max(np.abs(np.asarray(got, LD) - want)) / scale) <= tol


@pytest.mark.parametrize("rng", RANGES, ids=["box", "unit"])
@pytest.mark.parametrize("n", SHAPES)
def test_oracle_fp64_matches_the_high_precision_model(n, rng):
    r = np.random.default_rng(sum(n))
    v, f = r.uniform(-1, 1, O.shape(n)), r.uniform(-1, 1, O.shape(n))
    c = r.uniform(-1, 1, O.shape(O.csize(n)))
    for k in (1, 2, 3):
        assert _close(O.relax3d(n, rng, v, f, k, dtype=np.float64), model_relax(n, rng, v, f, k)), k
    red = O.relax_colour3d(n, rng, v, f, 0, dtype=np.float64)
    assert np.array_equal(red[_parity(n) == 1], v[_parity(n) == 1])  # a red pass leaves the black points alone
    assert _close(O.relax_colour3d(n, rng, red, f, 1, dtype=np.float64), model_relax(n, rng, v, f, 1))
    for mode in (O.REF_COMPAT, O.CORRECT):
        assert _close(O.residual3d(n, rng, v, f, mode, dtype=np.float64), model_residual(n, rng, v, f, mode)), mode
    assert _close(O.restrict3d(n, v, dtype=np.float64), model_restrict(n, v))
    assert _close(O.interpolate3d(n, v, c, dtype=np.float64), model_interpolate(n, v, c))
    assert _close(O.correct3d(n, v, f, dtype=np.float64), model_correct(n, v, f))


def test_the_model_tells_the_residual_modes_apart():
    """the sign quirk matters on these shapes: a model without it would not pass for REF_COMPAT"""
    n, rng = (23, 13, 5), RANGES[0]
    r = np.random.default_rng(1)
    v, f = r.uniform(-1, 1, O.shape(n)), r.uniform(-1, 1, O.shape(n))
    assert not _close(O.residual3d(n, rng, v, f, O.REF_COMPAT, dtype=np.float64), model_residual(n, rng, v, f, O.CORRECT))


def test_hierarchy_rule_of_the_helper():
    from odd_shapes import hierarchy_ok, levels
    assert levels((385, 129, 65)) == [(385, 129, 65), (193, 65, 33), (97, 33, 17), (49, 17, 9), (25, 9, 5), (13, 5, 3)]
    assert hierarchy_ok((385, 129, 65)) and hierarchy_ok((1537, 513)) and hierarchy_ok((641, 257, 129))
    assert not hierarchy_ok((97, 97, 97)) and hierarchy_ok((97, 97, 97), 5)
    assert levels((97, 97, 97))[-1] == (4, 4, 4)
