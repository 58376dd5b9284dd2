"""GPU suite: semi-coarsened 3D hierarchies (MultiGrid3D(coarsening="semi")) and their transfer kernels (csrc/mgx_semi3d.hip).

The four operators are checked bit for bit against the numpy restatement of their formulas (tests/semi_restated.py), for every
mask, with poisoned pads; the cycles against the restated cycle (the oracle's smoother and residual around those transfers),
every level, bit for bit; the solver against the restated iteration counts and against the full-coarsening hierarchy."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import pde_multigrid_amd as P
import semi_restated as S
from conftest import bits_equal
from odd_shapes import pads_unchanged, run_poisoned
from pde_multigrid_amd.multigrid import _ct, _ip, _rp, grid_spacing, xs_unpack
from solve_restated import boundary_mask, fcg_restated, interior, problem

pytestmark = pytest.mark.gpu
RG = [-1, 1, 0, 2, 0.5, 3]
UNIT = [0, 1, 0, 1, 0, 1]  # on 2^k + 1 points: the exact-reciprocal form of the residual
DTYPES = [np.float64, np.float32]
# every axis of every shape is coarsenable (n >= 5, n % 4 == 1); 257- and 513-point rows span several waves
SHAPES = [(17, 17, 17), (33, 17, 9), (21, 13, 29), (257, 9, 5), (513, 5, 5), (513, 33, 9)]
MASKS = [1, 2, 3, 4, 5, 6]
CYCLE_GRIDS = [(n3, rng) for n3, rng, _ in S.TABLE[:4]] + [S.ODD[:2]]


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


def _rand(n3, dtype, seed):
    return np.random.default_rng(seed).uniform(-1, 1, O.shape(n3)).astype(dtype)


def _fn(name, dtype):
    s, ct = _ct(dtype)
    return getattr(P.lib, "mgx3dxs_%s_%s" % (name, s)), ct


# ---------------------------------------------------------------------------------------------------------- operators
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("n3", SHAPES)
def test_restrict_axes(ctx, n3, mask, dtype):
    cn = S.coarse_size(n3, mask)
    fine, c0 = _rand(n3, dtype, 1), _rand(cn, dtype, 2)
    fn, _ = _fn("restrict_axes", dtype)
    ups, outs = run_poisoned(ctx, [fine, c0], lambda a, c: fn(ctx._h, a, _ip(n3), c, _ip(cn)), dtype)
    assert bits_equal(xs_unpack(outs[1], cn[0]), S.restrict_axes(fine, mask))  # the boundary injected
    assert bits_equal(outs[0], ups[0]) and pads_unchanged(ups[1], outs[1], cn[0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("n3", SHAPES)
@pytest.mark.parametrize("add", [False, True])
def test_interpolate_axes(ctx, add, n3, mask, dtype):
    cn = S.coarse_size(n3, mask)
    fine, coarse = _rand(n3, dtype, 3), _rand(cn, dtype, 4)
    fn, _ = _fn("interpolate_correct_axes" if add else "interpolate_axes", dtype)
    ups, outs = run_poisoned(ctx, [fine, coarse], lambda a, c: fn(ctx._h, a, _ip(n3), c, _ip(cn)), dtype)
    want = (S.interpolate_correct_axes if add else S.interpolate_axes)(fine, coarse, mask)
    assert bits_equal(xs_unpack(outs[0], n3[0]), want)  # the interior, and the boundary as it was
    assert pads_unchanged(ups[0], outs[0], n3[0]) and bits_equal(outs[1], ups[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("n3", SHAPES)
@pytest.mark.parametrize("rg", ["aniso", "unit"])
@pytest.mark.parametrize("mode", [P.REF_COMPAT, P.CORRECT])
def test_residual_restrict_axes(ctx, mode, rg, n3, mask, dtype):
    rng = RG if rg == "aniso" else UNIT
    cn = S.coarse_size(n3, mask)
    v, f, c0 = _rand(n3, dtype, 5), _rand(n3, dtype, 6), _rand(cn, dtype, 7)
    fn, ct = _fn("residual_restrict_axes", dtype)
    h = _rp(grid_spacing(n3, rng, dtype), ct)
    want = S.residual_restrict_axes(n3, rng, v, f, mask, mode, dtype)
    assert not want[boundary_mask(cn)].any()
    for keep in (0, 1):
        ups, outs = run_poisoned(ctx, [v, f, c0], lambda a, b, c: fn(ctx._h, a, b, _ip(n3), h, C.c_int(mode), c, _ip(cn), C.c_int(keep)), dtype)
        got = xs_unpack(outs[2], cn[0])
        assert bits_equal(interior(got), interior(want)), (keep, np.argwhere(interior(got) != interior(want))[:5])
        rim = boundary_mask(cn)
        assert bits_equal(got[rim], c0[rim] if keep else np.zeros_like(c0)[rim]), keep  # left alone, or written as 0
        assert bits_equal(outs[0], ups[0]) and bits_equal(outs[1], ups[1]) and pads_unchanged(ups[2], outs[2], cn[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_axes_halved_forwards_to_the_existing_operators(ctx, dtype):
    n3 = (33, 17, 9)
    cn = S.coarse_size(n3, 7)
    v, f, c = _rand(n3, dtype, 1), _rand(n3, dtype, 2), _rand(cn, dtype, 3)
    assert bits_equal(P.ops3dxs.restrict_axes(ctx, v, n3, cn), P.ops3dxs.restrict(ctx, v, n3))
    assert bits_equal(P.ops3dxs.interpolate_axes(ctx, v, n3, c, cn), P.ops3dxs.interpolate(ctx, v, n3, c))
    assert bits_equal(P.ops3dxs.interpolate_correct_axes(ctx, v, n3, c, cn), P.ops3dxs.interpolate_correct(ctx, v, n3, c))
    assert bits_equal(P.ops3dxs.residual_restrict_axes(ctx, v, f, n3, RG, cn), P.ops3dxs.residual_restrict(ctx, v, f, n3, RG))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cn", [(17, 17, 17), (8, 17, 17), (9, 17, 10), (9, 9, 33), (17, 5, 17)])
def test_bad_size_pairs(ctx, cn, dtype):
    """no axis halved, a size that is neither kept nor halved"""
    n3 = (17, 17, 17)
    a, c = _rand(n3, dtype, 1), np.zeros(O.shape(cn), dtype)
    calls = [lambda: P.ops3dxs.restrict_axes(ctx, a, n3, cn), lambda: P.ops3dxs.interpolate_axes(ctx, a, n3, c, cn),
             lambda: P.ops3dxs.interpolate_correct_axes(ctx, a, n3, c, cn), lambda: P.ops3dxs.residual_restrict_axes(ctx, a, a, n3, RG, cn)]
    for call in calls:
        with pytest.raises(P.MgxError) as e:
            call()
        assert e.value.status == P.MGX_ERR_SIZE


# ---------------------------------------------------------------------------------------------------------- cycles
def _semi(ctx, n3, rng, dtype=np.float64, mode=P.CORRECT, v=None, f=None):
    mg = P.MultiGrid3D(ctx, n3, rng, dtype, residual_mode=mode, coarsening="semi")
    if v is not None:
        mg.upload_v(0, v)
    if f is not None:
        mg.upload_f(0, f)
    return mg


def _same_levels(mg, H, what):
    assert mg.maxGrids == len(H.sizes) and mg.masks == H.masks
    for l, n in enumerate(H.sizes):
        assert mg.size(l) == n
        assert bits_equal(mg.download_v(l), H.v[l]), (what, "v", l)
        if l > 0:
            assert bits_equal(mg.download_f(l), H.f[l]), (what, "f", l)


CYCLES = [(np.float64, 2, 2, P.CORRECT), (np.float64, 1, 1, P.REF_COMPAT), (np.float64, 0, 2, P.CORRECT), (np.float64, 2, 0, P.CORRECT),
          (np.float32, 2, 2, P.CORRECT)]


@pytest.mark.parametrize("dtype,v1,v2,mode", CYCLES)
@pytest.mark.parametrize("grid", range(len(CYCLE_GRIDS)))
def test_vcycle_matches_restated_cycle(ctx, grid, dtype, v1, v2, mode):
    n3, rng = CYCLE_GRIDS[grid]
    v, f = _rand(n3, dtype, 1), _rand(n3, dtype, 2)
    H = S.Hierarchy(n3, rng, dtype, mode)
    H.v[0], H.f[0] = v.copy(), f.copy()
    H.vcycle(0, v1, v2)
    mg = _semi(ctx, n3, rng, dtype, mode, v, f)
    mg.VCycle(0, v1, v2)
    _same_levels(mg, H, "eager")
    # a second cycle starts from other rim flags (the coarse f's boundary is known to be zero now)
    H.vcycle(0, v1, v2)
    mg.VCycle(0, v1, v2)
    _same_levels(mg, H, "second")
    mg.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("grid", range(len(CYCLE_GRIDS)))
def test_graph_capture_and_replay_give_the_eager_bits(ctx, grid, dtype):
    """the masks are fixed at creation, so the graph record needs no word for them: a captured and a replayed cycle of a
    semi-coarsened hierarchy give the bits of the restated cycle"""
    n3, rng = CYCLE_GRIDS[grid]
    v, f = _rand(n3, dtype, 3), _rand(n3, dtype, 4)
    H = S.Hierarchy(n3, rng, dtype)
    H.v[0], H.f[0] = v.copy(), f.copy()
    H.vcycle(0, 2, 2)
    mg = _semi(ctx, n3, rng, dtype, P.CORRECT, v, f)
    mg.use_graph = True
    execs = []
    for rep in range(4):  # capture; capture under the rim flags the first cycle left; replay; replay
        mg.upload_v(0, v)
        mg.VCycle(0, 2, 2)
        _same_levels(mg, H, rep)
        execs.append(mg._mg.contents.graph_exec[0])
    assert execs[2] and execs[3] == execs[2], "the last cycle was captured again instead of replayed"
    mg.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("grid", range(len(CYCLE_GRIDS)))
def test_fmg_matches_restated_cycle(ctx, grid, dtype):
    n3, rng = CYCLE_GRIDS[grid]
    v, f = _rand(n3, dtype, 5), _rand(n3, dtype, 6)
    H = S.Hierarchy(n3, rng, dtype)
    H.v[0], H.f[0] = v.copy(), f.copy()
    H.fmg(0, 1, 2, 2)
    mg = _semi(ctx, n3, rng, dtype, P.CORRECT, v, f)
    mg.FullMultiGridVCycle(0, 1, 2, 2)
    _same_levels(mg, H, "fmg")
    mg.close()


def test_relax_and_transfers_through_the_hierarchy(ctx):
    n3, rng = CYCLE_GRIDS[0]
    v, f = _rand(n3, np.float64, 7), _rand(n3, np.float64, 8)
    mg = _semi(ctx, n3, rng, v=v, f=f)
    mg.Relax(0, 3)
    assert bits_equal(mg.download_v(0), O.relax3d(n3, rng, v, f, 3, dtype=np.float64))
    mg.close()


def test_natural_layout_is_refused(ctx):
    with pytest.raises(ValueError):
        P.MultiGrid3D(ctx, (65, 65, 65), [0, 1, 0, 1, 0, 4], coarsening="semi", layout="natural")
    with pytest.raises(ValueError):
        P.MultiGrid3D(ctx, (65, 65, 65), UNIT, coarsening="other")


# ---------------------------------------------------------------------------------------------------------- degenerate case
@pytest.mark.parametrize("dtype", DTYPES)
def test_cube_is_the_existing_hierarchy(ctx, dtype):
    n3 = (33, 33, 33)
    v, f = _rand(n3, dtype, 1), problem(n3, dtype)
    out = {}
    for how in ("full", "semi"):
        mg = P.MultiGrid3D(ctx, n3, UNIT, dtype, residual_mode=P.CORRECT, coarsening=how)
        assert mg.masks == (7, 7, 7, 7, 0) and [mg.size(l)[0] for l in range(mg.maxGrids)] == [33, 17, 9, 5, 3]
        mg.upload_v(0, v)
        mg.upload_f(0, f)
        mg.VCycle(0, 2, 2)
        cyc = [mg.download_v(l) for l in range(mg.maxGrids)]
        mg.upload_v(0, np.zeros_like(v))
        res = mg.PCG(2, 2, 1e-10 if dtype == np.float64 else 1e-4, 50)
        out[how] = (cyc, res, mg.download_v(0))
        mg.close()
    for a, b in zip(out["full"][0], out["semi"][0]):
        assert bits_equal(a, b)
    assert out["full"][1][:3] == out["semi"][1][:3] and bits_equal(out["full"][1][3], out["semi"][1][3])
    assert out["full"][1][2] and bits_equal(out["full"][2], out["semi"][2])


# ---------------------------------------------------------------------------------------------------------- solver
@pytest.mark.parametrize("grid", range(4))
def test_plain_cycling_converges_where_full_coarsening_does_not(ctx, grid):
    n3, rng, _ = S.TABLE[grid]
    f = problem(n3)
    want_k, _ = S.cycles_to(n3, rng, f, 2, 2, 1e-10, 12)
    mg = _semi(ctx, n3, rng, f=f)
    k, rel, conv, hist = mg.PCG(2, 2, 1e-10, 300, krylov=False)
    x = mg.download_v(0)
    assert bits_equal(mg.download_f(0), f), "d_f[0] was not restored"
    mg.close()
    full = P.MultiGrid3D(ctx, n3, rng, residual_mode=P.CORRECT)  # the existing hierarchy on the same grid
    full.upload_f(0, f)
    k_full, rel_full, conv_full, _ = full.PCG(2, 2, 1e-10, 300, krylov=False)
    full.close()
    print("%s: semi %d cycles (restated %d, rel %.3e), full %d%s" % (n3, k, want_k, rel, k_full, "" if conv_full else " (not converged)"))
    assert conv and rel < 1e-10 and len(hist) == k
    assert abs(k - want_k) <= 1 and k <= 10, (k, want_k)
    assert 4 * k <= k_full, (k, k_full)
    assert not x[boundary_mask(n3)].any()


@pytest.mark.parametrize("grid", range(4))
def test_pcg_matches_restatement(ctx, grid):
    n3, rng, _ = S.TABLE[grid]
    f = problem(n3)
    want_x, want_k, want_h, want_c = fcg_restated(n3, rng, np.zeros_like(f), f, S.m_cycle(n3, rng, 2, 2), 1e-10, 200)
    mg = _semi(ctx, n3, rng, f=f)
    k, rel, conv, hist = mg.PCG(2, 2, 1e-10, 200)
    x = mg.download_v(0)
    assert bits_equal(mg.download_f(0), f), "d_f[0] was not restored"
    mg.close()
    assert conv and want_c and rel < 1e-10
    assert abs(k - want_k) <= 1, (k, want_k)
    m = min(len(hist), len(want_h))
    upto = want_h[:m] >= 1e-10
    assert np.allclose(hist[:m][upto], want_h[:m][upto], rtol=1e-6, atol=0), (hist[:m], want_h[:m])
    assert np.abs(x - want_x).max() <= 1e-9 * np.abs(want_x).max()


@pytest.mark.parametrize("krylov", [True, False])
@pytest.mark.parametrize("grid", range(4))
def test_mixed_precision_on_a_semi_hierarchy(ctx, grid, krylov):
    """the fp32 twin copies the plan: same levels, and the fp64 iteration count to within one"""
    n3, rng, _ = S.TABLE[grid]
    f = problem(n3)
    v0 = np.zeros_like(f)
    v0[boundary_mask(n3)] = _rand(n3, np.float64, 9)[boundary_mask(n3)]  # Dirichlet data
    its = {}
    for precond in ("f64", "f32"):
        mg = _semi(ctx, n3, rng, v=v0, f=f)
        k, rel, conv, _ = mg.PCG(2, 2, 1e-10, 100, krylov=krylov, precond=precond)
        x = mg.download_v(0)
        assert conv and rel < 1e-10, (precond, k, rel)
        assert bits_equal(mg.download_f(0), f), "d_f[0] was not restored"
        assert bits_equal(x[boundary_mask(n3)], v0[boundary_mask(n3)]), "the boundary was changed"
        its[precond] = k
        mg.close()
    assert abs(its["f32"] - its["f64"]) <= 1, its


def test_solve3d_pcg_semi(ctx):
    n3, rng, _ = S.TABLE[0]
    f = problem(n3)
    x, k, rel, conv = P.solve3d_pcg(ctx, np.zeros_like(f), f, rng, krylov=False, coarsening="semi")
    assert conv and rel < 1e-10 and k <= 10
    mg = _semi(ctx, n3, rng, f=f)
    k2, _, _, _ = mg.PCG(2, 2, 1e-10, 100, krylov=False)
    assert k2 == k and bits_equal(mg.download_v(0), x)
    mg.close()
