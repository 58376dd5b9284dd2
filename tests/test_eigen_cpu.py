"""CPU suite of the eigensolver (mgMultiGrid3D_f64_Eigen): the exports and the refusals that need no GPU, the dense
solver mg_sym_geneig against numpy, and the references of test_gpu_zz_eigen.py themselves -- the closed-form spectrum against a
dense eigh of the restated operator, whose weighted matrix is symmetric to the bit."""
import ctypes as C

import numpy as np
import pytest

import eigen_cases as EC
import op_restated as OP
import pde_multigrid_amd as P

NOT_SPD = 100  # MG_GENEIG_NOT_SPD


def _dp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_exports():
    for name in ("mgMultiGrid3D_f64_Eigen", "mg_sym_geneig", "mgx3dxs_block_work_elems_f64", "mgx3dxs_block_gram_f64",
                 "mgx3dxs_block_combine_f64", "mgx3dxs_block_residual_f64", "mgx3dxs_eigen_start_f64"):
        assert hasattr(P.lib, name), name
    assert callable(P.MultiGrid3D.Eigen)
    for name in ("block_gram", "block_combine", "block_residual", "eigen_start"):
        assert callable(getattr(P.ops3dxs, name)), name


def test_eigen_refuses_bad_arguments_before_touching_anything():
    fn = P.lib.mgMultiGrid3D_f64_Eigen
    lam, res = np.full(9, 7.0), np.full(9, 7.0)
    it, conv = C.c_int(-5), C.c_int(-5)
    mg = (C.c_ubyte * 65536)()  # a hierarchy of zeros: anything read from it beyond the argument checks would be a NULL

    def call(mgp, k, tol, maxit, lamp=_dp(lam), resp=_dp(res), itp=C.byref(it), convp=C.byref(conv)):
        return fn(mgp, C.c_int(k), C.c_int(2), C.c_int(2), C.c_double(tol), C.c_int(maxit), lamp, resp, itp, convp, None, None)

    assert call(None, 2, 1e-8, 10) == P.MGX_ERR_INVALID
    assert b"NULL" in P.lib.mgx_last_error()
    assert call(mg, 2, 1e-8, 10, lamp=None) == P.MGX_ERR_INVALID
    assert call(mg, 2, 1e-8, 10, resp=None) == P.MGX_ERR_INVALID
    assert call(mg, 2, 1e-8, 10, itp=None) == P.MGX_ERR_INVALID
    assert call(mg, 2, 1e-8, 10, convp=None) == P.MGX_ERR_INVALID
    for k, tol, maxit in ((0, 1e-8, 10), (9, 1e-8, 10), (-1, 1e-8, 10), (2, 0.0, 10), (2, -1e-8, 10), (2, float("nan"), 10), (2, 1e-8, 0),
                          (2, 1e-8, -3)):
        assert call(mg, k, tol, maxit) == P.MGX_ERR_INVALID, (k, tol, maxit)
    assert call(mg, 2, 1e-8, 10) == P.MGX_ERR_INVALID  # (no levels)
    assert bytes(mg) == bytes(65536) and (lam == 7.0).all() and (res == 7.0).all() and it.value == -5 and conv.value == -5


def test_block_entries_refuse_null():
    n = (C.c_int * 3)(5, 5, 5)
    one = (C.c_void_p * 1)(None)
    assert P.lib.mgx3dxs_block_gram_f64(None, 1, one, 1, one, None, n, 0, None, None) == P.MGX_ERR_INVALID
    assert P.lib.mgx3dxs_block_combine_f64(None, 1, one, 1, one, None, n, 0) == P.MGX_ERR_INVALID
    assert P.lib.mgx3dxs_block_residual_f64(None, 1, one, one, None, None, one, n, 0, None, None) == P.MGX_ERR_INVALID
    assert P.lib.mgx3dxs_eigen_start_f64(None, None, 0, n, 0) == P.MGX_ERR_INVALID
    fn = P.lib.mgx3dxs_block_work_elems_f64
    fn.restype = C.c_size_t
    assert fn(n) == 32 * 1 * 5 and fn((C.c_int * 3)(4, 5, 5)) == 0  # 2 * 16 sums per block of 16 rows and plane; bad sizes: 0


# ------------------------------------------------------------------------------------------ mg_sym_geneig
def _geneig(G, B):
    n = G.shape[0]
    G, B = np.ascontiguousarray(G, np.float64), np.ascontiguousarray(B, np.float64)
    w, Y = np.full(n, np.nan), np.full((n, n), np.nan)
    st = P.lib.mg_sym_geneig(C.c_int(n), _dp(G), _dp(B), _dp(w), _dp(Y))
    return st, w, Y


def _numpy_geneig(G, B):
    """eigh after a Cholesky reduction"""
    L = np.linalg.cholesky(B)
    Li = np.linalg.inv(L)
    Cm = Li @ G @ Li.T
    return np.linalg.eigvalsh(0.5 * (Cm + Cm.T))


def _spd(rng, n, lo=1.0, hi=10.0):
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    return (Q * rng.uniform(lo, hi, n)) @ Q.T


def _check_pair(G, B):
    st, w, Y = _geneig(G, B)
    assert st == P.MGX_OK
    want = _numpy_geneig(G, B)
    assert np.all(np.diff(w) >= 0)
    assert np.max(np.abs(w - want) / np.abs(want)) <= 1e-10, np.max(np.abs(w - want) / np.abs(want))
    assert np.max(np.abs(Y.T @ B @ Y - np.eye(len(w)))) <= 1e-10
    assert np.max(np.abs(G @ Y - (B @ Y) * w)) <= 1e-9 * np.max(np.abs(G))


@pytest.mark.parametrize("n", [1, 2, 7, 24])
def test_geneig_random_spd_pairs(n):
    rng = np.random.default_rng(100 + n)
    G, B = _spd(rng, n, 0.1, 50.0), _spd(rng, n)
    G, B = 0.5 * (G + G.T), 0.5 * (B + B.T)
    _check_pair(G, B)


def test_geneig_only_the_upper_triangles_are_read():
    rng = np.random.default_rng(5)
    G, B = _spd(rng, 6), _spd(rng, 6)
    G, B = 0.5 * (G + G.T), 0.5 * (B + B.T)
    _, w0, Y0 = _geneig(G, B)
    G2, B2 = np.triu(G) + np.tril(np.full((6, 6), np.nan), -1), np.triu(B) + np.tril(np.full((6, 6), np.nan), -1)
    _, w1, Y1 = _geneig(G2, B2)
    assert np.array_equal(w0, w1) and np.array_equal(Y0, Y1)


def test_geneig_mass_matrix_of_condition_1e10():
    """The pair of a badly scaled basis, the one the solver meets: S = Q D with Q of condition 3 and column norms D from 1 down to
    1e-5, B = S^T S of condition 1e10, G = S^T K S.  Both Cholesky reductions are invariant under the scaling of the basis to
    rounding, so numpy's is a reference to 1e-10 here; a B of that condition with no such structure would leave numpy's own
    reduction with an error of eps cond(B), far above the bound."""
    rng = np.random.default_rng(11)
    n = 12
    Q = np.linalg.qr(rng.standard_normal((40, n)))[0] @ _spd(rng, n, 1.0, 3.0)
    S = Q * np.logspace(0, -5, n)
    K = _spd(rng, 40, 1.0, 1e3)
    B, G = S.T @ S, S.T @ K @ S
    B, G = 0.5 * (B + B.T), 0.5 * (G + G.T)
    assert 1e9 < np.linalg.cond(B) < 1e12
    _check_pair(G, B)


def test_geneig_failure_status():
    rng = np.random.default_rng(3)
    G = _spd(rng, 5)
    B = _spd(rng, 5)
    Bi = B - 5.5 * np.eye(5)  # indefinite: eigenvalues on both sides of 0
    assert np.linalg.eigvalsh(Bi)[0] < 0 < np.linalg.eigvalsh(Bi)[-1]
    st, w, Y = _geneig(G, Bi)
    assert st == NOT_SPD and np.isnan(w).all() and np.isnan(Y).all()
    Bn = B.copy()
    Bn[2, 2] = -1.0
    assert _geneig(G, Bn)[0] == NOT_SPD
    Bs = np.ones((3, 3))  # singular: three times the same vector
    assert _geneig(np.eye(3), Bs)[0] == NOT_SPD
    w, Y = np.zeros(25), np.zeros(625)
    assert P.lib.mg_sym_geneig(C.c_int(0), _dp(G), _dp(B), _dp(w), _dp(Y)) == P.MGX_ERR_INVALID
    assert P.lib.mg_sym_geneig(C.c_int(25), _dp(G), _dp(B), _dp(w), _dp(Y)) == P.MGX_ERR_INVALID
    assert P.lib.mg_sym_geneig(C.c_int(5), None, _dp(B), _dp(w), _dp(Y)) == P.MGX_ERR_INVALID


# ------------------------------------------------------------------------------------------ the references of the GPU tests
def test_axis_values_count_and_order():
    for lo, hi, cnt in ((0, 0, 7), (1, 1, 9), (1, 0, 8), (0, 1, 8)):
        v = EC.axis_values(9, 0.125, lo, hi)
        assert len(v) == cnt and np.all(np.diff(v) > 0)
    assert EC.axis_values(9, 0.125, 1, 1)[0] == 0.0


@pytest.mark.parametrize("bc", [0, 21, 37, 63])
def test_closed_form_against_dense_eigh(bc):
    n3 = (9, 9, 9)
    s = 1.0 if bc == 63 else 0.0
    op = OP.Op(n3, EC.BOX, np.float64, s, bc=bc)
    S, unk = EC.dense(op)
    assert np.max(np.abs(S - S.T)) == 0.0  # symmetric to the bit in the weighted inner product
    lam = EC.dense_spectrum(op)[0]
    want = EC.closed_form(n3, EC.BOX, bc)
    assert len(lam) == len(want) == int(unk.sum())
    scale = np.maximum(np.abs(want), 1.0) if bc == 63 else np.abs(want)  # (the closed box: lambda_1 = 0, absolute there)
    assert np.max(np.abs(lam - want) / scale) <= 1e-11, np.max(np.abs(lam - want) / scale)


@pytest.mark.parametrize("mean", ["arithmetic", "harmonic"])
def test_materials_case_is_symmetric_definite_and_separated(mean):
    op = EC.materials_op(mean)
    S, unk = EC.dense(op)
    assert np.max(np.abs(S - S.T)) == 0.0
    lam = EC.materials_spectrum(mean)
    assert lam[0] > 0 and np.all(np.diff(lam[:6]) > 1e-3 * lam[:6].max())  # the five pairs asked for are simple
    X = EC.dense_spectrum(op)[1][:, :3]
    full = np.zeros((3,) + unk.shape)
    for i in range(3):
        full[i][unk] = X[:, i]
    assert np.max(EC.residuals(op, lam[:3], full)) < 1e-10  # residuals() recomputes what the solver reports


def test_bound_is_about_1e_minus_10():
    n3 = (33, 33, 33)
    b = EC.bound(EC.closed_form(n3, EC.BOX, 0), 6, 1e-8, 0.0, n3, EC.BOX)
    assert np.all(b < 5e-10) and np.all(b > 64 * EC.EPS * EC.norm_A(n3, EC.BOX) * 0.999)
