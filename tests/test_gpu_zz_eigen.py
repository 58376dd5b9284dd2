"""GPU suite of the eigensolver (MultiGrid3D.Eigen / mgMultiGrid3D_f64_Eigen).

The block vector kernels (csrc/mgx_eigen3d.hip) through their raw entries on test_gpu_neumann.py's shapes and masks, with NaN in
every pad and Dirichlet entry of the inputs and NaN guards behind the work array: Gram entries and norms against math.fsum of the
restated W-weighted products to 1e-13 of the sum of the absolute terms and equal on two runs, block_combine and block_residual
bit for bit against numpy evaluated left to right (the order the kernels document), an output aliasing an input, pads and Dirichlet
entries of the outputs unchanged.  The solver against the closed-form spectrum of the box (eigen_cases.bound: Kato-Temple plus the
rounding of a Rayleigh quotient), against a dense eigh of the restated operator with materials and convective walls, on a
semi-coarsened hierarchy; what a call leaves behind, determinism, graphs against eager runs, and the refusals.

Iterations seen on an MI355X (nothing asserts them): see DESIGN.md 21.

The file's name sorts it behind every other GPU file: the suite's existing files keep their places in the order of a run."""
import ctypes as C
import math

import numpy as np
import pytest

import eigen_cases as EC
import op_restated as OP
import oracle as O
import pde_multigrid_amd as P
from conftest import bits_equal

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]
SHAPES = [(3, 3, 3), (5, 3, 3), (3, 5, 9), (17, 17, 17), (21, 13, 29), (131, 7, 9), (257, 9, 5), (513, 5, 5)]
MASKS = [0, 1, 2, 12, 48, 21, 42, 37, 63]
TOL = 1e-8
FACES = lambda bc: [bool((bc >> k) & 1) for k in range(6)]


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------ the block kernels
def _pads(n3):
    return P.xs_pack(np.ones(O.shape(n3))) == 0


def _vec(n3, bc, seed, lo=-1.0, hi=1.0):
    """(the array in the reference layout with 0 off the unknowns, the same as stored with NaN in pads and Dirichlet entries)"""
    unk = OP.unknown_mask(n3, bc)
    a = np.random.default_rng(seed).uniform(lo, hi, O.shape(n3))
    stored = P.xs_pack(np.where(unk, a, np.nan))
    stored[_pads(n3)] = np.nan
    return np.where(unk, a, 0.0), stored


def fsum_close(got, terms, rtol=1e-13):
    terms = np.asarray(terms, np.float64).ravel()
    return abs(got - math.fsum(terms)) <= rtol * math.fsum(np.abs(terms))


@pytest.mark.parametrize("bc", MASKS)
@pytest.mark.parametrize("n3", SHAPES)
def test_block_gram(ctx, n3, bc):
    W = OP.weights(n3, bc)
    U = [_vec(n3, bc, 10 + i) for i in range(3)]
    V = [_vec(n3, bc, 20 + i) for i in range(4)]
    c, cs = _vec(n3, bc, 30, 0.5, 2.0)
    for cap in (None, cs):
        plain, cw = P.ops3dxs.block_gram(ctx, [u[1] for u in U], [v[1] for v in V], cap, n3, bc)
        again = P.ops3dxs.block_gram(ctx, [u[1] for u in U], [v[1] for v in V], cap, n3, bc)
        assert bits_equal(plain, again[0]) and (cap is None or bits_equal(cw, again[1]))
        assert (cw is None) == (cap is None)
        for i in range(3):
            for j in range(4):
                assert fsum_close(plain[i, j], W * U[i][0] * V[j][0]), (i, j)
                if cap is not None:
                    assert fsum_close(cw[i, j], W * U[i][0] * c * V[j][0]), (i, j)


def test_block_gram_every_group_size(ctx):
    n3, bc = (21, 13, 29), 37
    W = OP.weights(n3, bc)
    U = [_vec(n3, bc, 40 + i) for i in range(4)]
    c, cs = _vec(n3, bc, 31, 0.5, 2.0)
    for nu in range(1, 5):
        for nv in range(1, 5):
            plain, cw = P.ops3dxs.block_gram(ctx, [u[1] for u in U[:nu]], [u[1] for u in U[4 - nv:]], cs, n3, bc)
            for i in range(nu):
                for j in range(nv):
                    assert fsum_close(plain[i, j], W * U[i][0] * U[4 - nv + j][0]) and fsum_close(cw[i, j], W * U[i][0] * c * U[4 - nv + j][0])
            if nu == nv == 4:  # a group with itself: symmetric to the bit (W is a power of two, products commute, one order of the sums)
                assert bits_equal(plain, plain.T.copy())


def _combine_ref(S, Y, i):
    t = Y[0, i] * S[0]
    for j in range(1, len(S)):
        t = t + Y[j, i] * S[j]
    return t


@pytest.mark.parametrize("bc", MASKS)
@pytest.mark.parametrize("n3", SHAPES)
def test_block_combine(ctx, n3, bc):
    unk, pads = OP.unknown_mask(n3, bc), _pads(n3)
    S = [_vec(n3, bc, 50 + i) for i in range(5)]
    Y = np.random.default_rng(7).uniform(-2, 2, (5, 3))
    fill = P.xs_pack(np.full(O.shape(n3), 7.25))
    fill[pads] = -3.5
    # output 1 IS input 2 on the device; outputs 0 and 2 are arrays of their own
    out = P.ops3dxs.block_combine(ctx, [s[1] for s in S], Y, n3, bc, out=[fill, None, fill], alias={1: 2})
    for i in range(3):
        got = P.xs_unpack(out[i], n3[0])
        want = _combine_ref([s[0] for s in S], Y, i)
        assert bits_equal(got[unk], want[unk]), i  # left to right in double: exact
        before = S[2][1] if i == 1 else fill
        keep = pads | (P.xs_pack((~unk).astype(np.float64)) != 0)
        assert bits_equal(out[i][keep], before[keep]), i  # pads and Dirichlet entries as they were (NaN where the input had NaN)


def test_block_combine_every_count(ctx):
    n3, bc = (5, 3, 3), 21
    unk = OP.unknown_mask(n3, bc)
    S = [_vec(n3, bc, 70 + i) for i in range(12)]
    rng = np.random.default_rng(8)
    for nin in range(1, 13):
        for nout in range(1, 5):
            Y = rng.uniform(-2, 2, (nin, nout))
            out = P.ops3dxs.block_combine(ctx, [s[1] for s in S[:nin]], Y, n3, bc)
            for i in range(nout):
                assert bits_equal(P.xs_unpack(out[i], n3[0])[unk], _combine_ref([s[0] for s in S[:nin]], Y, i)[unk]), (nin, nout, i)
    p = ctx.to_device(S[0][1])
    ptrs, y = (C.c_void_p * 13)(*([p.value] * 13)), np.ones(13 * 5)
    for nin, nout, mask in ((0, 1, 0), (13, 1, 0), (1, 0, 0), (1, 5, 0), (1, 1, 64), (1, 1, -1)):  # counts and masks outside their ranges
        st = P.lib.mgx3dxs_block_combine_f64(ctx._h, C.c_int(nin), ptrs, C.c_int(nout), ptrs, y.ctypes.data_as(C.c_void_p),
                                             (C.c_int * 3)(*n3), C.c_int(mask))
        assert st == P.MGX_ERR_INVALID, (nin, nout, mask)
    # ... and of the other three entries, every argument but the one under test valid
    fn = P.lib.mgx3dxs_block_work_elems_f64
    fn.restype = C.c_size_t
    work, sums = ctx.malloc(8 * int(fn((C.c_int * 3)(*n3)))), ctx.malloc(8 * 32)
    nn, mu = (C.c_int * 3)(*n3), np.ones(4)
    for nu, nv, mask in ((0, 1, 0), (5, 1, 0), (1, 0, 0), (1, 5, 0), (-1, 1, 0), (1, 1, 64), (1, 1, -1)):
        st = P.lib.mgx3dxs_block_gram_f64(ctx._h, C.c_int(nu), ptrs, C.c_int(nv), ptrs, None, nn, C.c_int(mask), work, sums)
        assert st == P.MGX_ERR_INVALID, (nu, nv, mask)
    for nvec, mask in ((0, 0), (5, 0), (-1, 0), (1, 64), (1, -1)):
        st = P.lib.mgx3dxs_block_residual_f64(ctx._h, C.c_int(nvec), ptrs, ptrs, None, mu.ctypes.data_as(C.c_void_p), ptrs, nn, C.c_int(mask),
                                              work, sums)
        assert st == P.MGX_ERR_INVALID, (nvec, mask)
    for index, mask in ((-1, 0), (0, 64), (0, -1)):
        assert P.lib.mgx3dxs_eigen_start_f64(ctx._h, p, C.c_int(index), nn, C.c_int(mask)) == P.MGX_ERR_INVALID, (index, mask)
    null = (C.c_void_p * 4)(p.value, None, p.value, p.value)  # a NULL entry of a pointer array
    assert P.lib.mgx3dxs_block_gram_f64(ctx._h, C.c_int(2), null, C.c_int(1), ptrs, None, nn, C.c_int(0), work, sums) == P.MGX_ERR_INVALID
    assert P.lib.mgx3dxs_block_gram_f64(ctx._h, C.c_int(1), ptrs, C.c_int(1), ptrs, None, (C.c_int * 3)(4, 3, 3), C.c_int(0), work,
                                        sums) == P.MGX_ERR_SIZE
    assert bits_equal(ctx.to_host(p, S[0][1].shape, np.float64), S[0][1])  # nothing was launched
    for q in (p, work, sums):
        ctx.free(q)


@pytest.mark.parametrize("bc", MASKS)
@pytest.mark.parametrize("n3", SHAPES)
def test_block_residual(ctx, n3, bc):
    unk, pads, W = OP.unknown_mask(n3, bc), _pads(n3), OP.weights(n3, bc)
    AX = [_vec(n3, bc, 80 + i) for i in range(3)]
    X = [_vec(n3, bc, 90 + i) for i in range(3)]
    c, cs = _vec(n3, bc, 32, 0.5, 2.0)
    mu = np.array([0.75, 3.0, 11.5])
    fill = P.xs_pack(np.full(O.shape(n3), 7.25))
    fill[pads] = -3.5
    for cap in (None, cs):
        R, rr, xx = P.ops3dxs.block_residual(ctx, [a[1] for a in AX], [x[1] for x in X], cap, mu, n3, bc, R=[fill] * 3)
        again = P.ops3dxs.block_residual(ctx, [a[1] for a in AX], [x[1] for x in X], cap, mu, n3, bc, R=[fill] * 3)
        assert bits_equal(rr, again[1]) and bits_equal(xx, again[2])
        for i in range(3):
            want = AX[i][0] + mu[i] * ((c * X[i][0]) if cap is not None else X[i][0])
            got = P.xs_unpack(R[i], n3[0])
            assert bits_equal(got[unk], want[unk]) and not got[~unk].any() and bits_equal(R[i][pads], fill[pads]), i
            r = np.where(unk, want, 0.0)
            assert fsum_close(rr[i], W * r * r) and fsum_close(xx[i], W * X[i][0] * X[i][0]), i


@pytest.mark.parametrize("bc", MASKS)
@pytest.mark.parametrize("n3", SHAPES)
def test_eigen_start(ctx, n3, bc):
    unk, pads = OP.unknown_mask(n3, bc), _pads(n3)
    fill = P.xs_pack(np.full(O.shape(n3), np.nan))
    fill[pads] = -3.5
    a, b, other = (P.ops3dxs.eigen_start(ctx, i, n3, bc, v=fill) for i in (2, 2, 3))
    assert bits_equal(a, b) and bits_equal(a[pads], fill[pads])
    v, w = P.xs_unpack(a, n3[0]), P.xs_unpack(other, n3[0])
    assert not v[~unk].any() and np.all(np.abs(v[unk]) < 1.0) and np.all(np.isfinite(v))
    if unk.sum() > 4:
        assert len(np.unique(v[unk])) > unk.sum() // 2 and not np.array_equal(v, w)


# ------------------------------------------------------------------------------------------ the solver
def _box(ctx, n3, rng, bc, s, **kw):
    return P.MultiGrid3D(ctx, list(n3), rng, np.float64, residual_mode=P.CORRECT, shift=s, neumann=FACES(bc) if bc else None, **kw)


def _check_closed_form(mg, n3, rng, bc, s, k):
    lam, X, info = mg.Eigen(k, tol=TOL)
    exact = EC.closed_form(n3, rng, bc)
    b = EC.bound(exact, k, TOL, s, n3, rng)
    print("Eigen %s mask %d s %g k %d: %d iterations, residuals %s, errors %s, bound %s" % (
        n3, bc, s, k, info["iterations"], info["residuals"], np.abs(lam - exact[:k]), b))
    assert info["converged"] and np.all(info["residuals"] < TOL)
    assert np.all(np.abs(lam - exact[:k]) <= b), (lam - exact[:k], b)
    Wc = OP.weights(n3, bc)
    gram = np.array([[OP.wdot(Wc, X[i], X[j]) for j in range(k)] for i in range(k)])
    assert np.max(np.abs(gram - np.eye(k))) <= 1e-10
    assert not X[:, ~OP.unknown_mask(n3, bc)].any()
    return lam, X, info, b


N33 = (33, 33, 33)


@pytest.mark.parametrize("bc,s,kw", [(0, 0.0, {"fuse": False}), (21, 0.0, {}), (63, 1.0, {}), (0, 0.0, {})],
                         ids=["mask0-unfused", "mask21", "closed-box-shift1", "mask0-plain-tuned"])
def test_closed_form(ctx, bc, s, kw):
    mg = _box(ctx, N33, EC.BOX, bc, s, **kw)
    lam, X, info, b = _check_closed_form(mg, N33, EC.BOX, bc, s, 6)
    if bc == 63:  # lambda_1 = 0 and x_1 is constant
        assert abs(lam[0]) <= b[0]
        assert np.max(np.abs(X[0] - X[0].mean())) <= 1e-8 * abs(X[0].mean())
    mg.close()


def test_shift_independence(ctx):
    lams, bounds = [], []
    for s in (0.5, 4.0):
        mg = _box(ctx, N33, EC.BOX, 21, s)
        lam, _, _, b = _check_closed_form(mg, N33, EC.BOX, 21, s, 6)
        lams.append(lam)
        bounds.append(b)
        mg.close()
    assert np.all(np.abs(lams[0] - lams[1]) <= 2 * np.maximum(bounds[0], bounds[1]))


@pytest.mark.parametrize("mean", ["arithmetic", "harmonic"])
def test_materials_and_walls_against_dense(ctx, mean):
    a, c = EC.materials()
    mg = P.MultiGrid3D(ctx, list(EC.MAT_N), EC.MAT_RNG, np.float64, residual_mode=P.CORRECT, shift=EC.MAT_S, coefficient=a, capacity=c,
                       neumann=FACES(EC.MAT_BC), robin=EC.MAT_BETA, face_mean=mean)
    lam, X, info = mg.Eigen(5, tol=TOL)
    want = EC.materials_spectrum(mean)[:5]
    print("Eigen materials %s: %d iterations, residuals %s, relative errors %s" % (mean, info["iterations"], info["residuals"],
                                                                                   np.abs(lam - want) / want))
    assert info["converged"] and np.all(info["residuals"] < TOL)
    assert np.max(np.abs(lam - want) / want) <= 1e-9
    op = EC.materials_op(mean)
    assert np.all(EC.residuals(op, lam, X) < 2 * TOL)  # the residual equation, recomputed from the restated operator
    Wc = EC.wc(op)
    gram = np.array([[OP.wdot(Wc, X[i], X[j]) for j in range(5)] for i in range(5)])
    assert np.max(np.abs(gram - np.eye(5))) <= 1e-10
    mg.close()


def test_semi_coarsened(ctx):
    n3, rng = (33, 33, 17), [0, 1, 0, 1, 0, 4]
    mg = P.MultiGrid3D(ctx, list(n3), rng, np.float64, residual_mode=P.CORRECT, coarsening="semi")
    assert any(m != 7 for m in mg.masks[:-1])
    lam = _check_closed_form(mg, n3, rng, 0, 0.0, 4)[0]
    mg.close()
    full = P.MultiGrid3D(ctx, list(n3), rng, np.float64, residual_mode=P.CORRECT)  # the same grid, every axis halved: a weaker
    lam_full, _, _, b = _check_closed_form(full, n3, rng, 0, 0.0, 4)              # preconditioner, the same eigenvalues
    assert np.all(np.abs(lam - lam_full) <= 2 * b)
    full.close()


def _stored(ctx, mg, which):
    g = mg.grid(0)
    shape = P.xs_pack(np.zeros(O.shape(mg.size(0)))).shape
    return ctx.to_host(C.c_void_p(getattr(g, which)), shape, np.float64)


def _flags(mg):
    m = mg._mg.contents
    return (m.v_rim_zero[0], m.f_rim_zero[0])


def test_state_and_determinism(ctx):
    n3, bc, s = (17, 17, 17), 21, 0.5
    r = np.random.default_rng(3)
    v0, f0 = r.uniform(-1, 1, O.shape(n3)), r.uniform(-1, 1, O.shape(n3))

    def fresh(graph=False):
        mg = _box(ctx, n3, EC.BOX, bc, s)
        mg.upload_v(0, v0)
        mg.upload_f(0, f0)
        mg.use_graph = graph
        return mg

    mg = fresh()
    before = (_stored(ctx, mg, "d_v"), _stored(ctx, mg, "d_f"), _flags(mg))
    lam, X, info = mg.Eigen(4, tol=TOL)
    assert info["converged"]
    after = (_stored(ctx, mg, "d_v"), _stored(ctx, mg, "d_f"), _flags(mg))
    assert bits_equal(before[0], after[0]) and bits_equal(before[1], after[1]) and before[2] == after[2]
    assert mg._mg.contents.e_rim_valid[0] == 0
    lam2, X2, info2 = mg.Eigen(4, tol=TOL)  # two calls: the same bits
    assert bits_equal(lam, lam2) and bits_equal(X, X2) and info["iterations"] == info2["iterations"]
    assert bits_equal(info["residuals"], info2["residuals"])
    mg.VCycle(0, 2, 2)  # a cycle afterwards: the bits of one on a hierarchy that never called Eigen
    other = fresh()
    other.VCycle(0, 2, 2)
    assert bits_equal(mg.download_v(0), other.download_v(0))
    other.close()
    g = fresh(graph=True)  # capture, run and replay: the eager bits
    for _ in range(2):
        lam3, X3, info3 = g.Eigen(4, tol=TOL)
        assert bits_equal(lam, lam3) and bits_equal(X, X3) and info3["iterations"] == info["iterations"]
    assert bits_equal(_stored(ctx, g, "d_v"), before[0]) and bits_equal(_stored(ctx, g, "d_f"), before[1])
    g.close()
    lam4, X4, info4 = mg.Eigen(4, tol=TOL, guess=X)  # the converged vectors as the guess
    assert info4["converged"] and info4["iterations"] <= 2
    exact = EC.closed_form(n3, EC.BOX, bc)[:4]
    assert np.all(np.abs(lam4 - exact) <= EC.bound(EC.closed_form(n3, EC.BOX, bc), 4, TOL, s, n3, EC.BOX))
    lam5, none, _ = mg.Eigen(2, tol=TOL, vectors=False)
    assert none is None and np.all(np.abs(lam5 - exact[:2]) <= 1e-9)
    mg.close()


def test_refusals_leave_the_hierarchy_usable(ctx):
    n3 = (17, 17, 17)
    mg32 = P.MultiGrid3D(ctx, list(n3), EC.BOX, np.float32, residual_mode=P.CORRECT)
    with pytest.raises(ValueError, match="fp64"):
        mg32.Eigen(2)
    mg32.VCycle(0, 2, 2)
    mg32.close()
    mg = _box(ctx, n3, EC.BOX, 0, 0.0)
    for k in (0, 9, -1):
        with pytest.raises(P.MgxError) as e:
            mg.Eigen(k)
        assert e.value.status == P.MGX_ERR_INVALID
    with pytest.raises(ValueError, match="shape"):
        mg.Eigen(2, guess=np.zeros((2, 17, 17, 16)))
    with pytest.raises(ValueError, match="shape"):
        mg.Eigen(2, guess=np.zeros((3,) + O.shape(n3)))
    with pytest.raises(P.MgxError):  # twice the same start vector: no basis
        mg.Eigen(2, guess=np.ones((2,) + O.shape(n3)))
    lam, _, info = mg.Eigen(2, tol=TOL)
    assert info["converged"] and np.all(np.abs(lam - EC.closed_form(n3, EC.BOX, 0)[:2]) <= 1e-9)
    mg.close()
    closed = _box(ctx, n3, EC.BOX, 63, 0.0)
    with pytest.raises(P.MgxError, match="singular"):
        closed.Eigen(2)
    closed.shift = 1.0
    lam, _, info = closed.Eigen(2, tol=TOL)
    assert info["converged"] and abs(lam[0]) <= 1e-9
    closed.close()
    nat = P.MultiGrid3D(ctx, list(n3), EC.BOX, np.float64, residual_mode=P.CORRECT, layout="natural")
    with pytest.raises(P.MgxError, match="x-split"):
        nat.Eigen(2)
    nat.VCycle(0, 2, 2)
    nat.close()
    ref = P.MultiGrid3D(ctx, list(n3), EC.BOX, np.float64)  # REF_COMPAT
    with pytest.raises(P.MgxError, match="CORRECT"):
        ref.Eigen(2)
    ref.VCycle(0, 2, 2)
    ref.close()


def test_maxit_one_on_a_hard_case(ctx):
    a, c = EC.materials()
    mg = P.MultiGrid3D(ctx, list(EC.MAT_N), EC.MAT_RNG, np.float64, residual_mode=P.CORRECT, shift=EC.MAT_S, coefficient=a, capacity=c,
                       neumann=FACES(EC.MAT_BC), robin=EC.MAT_BETA)
    lam, X, info = mg.Eigen(5, tol=TOL, maxit=1)
    assert not info["converged"] and info["iterations"] == 1
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(X)) and np.all(np.isfinite(info["residuals"])) and np.all(info["residuals"] > TOL)
    lam, _, info = mg.Eigen(5, tol=TOL)  # and the hierarchy goes on working
    assert info["converged"]
    mg.close()
