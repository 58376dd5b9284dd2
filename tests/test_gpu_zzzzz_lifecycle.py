"""GPU suite: long-lived 3D hierarchies against fresh ones after every setter (the walks, the disturbances and the probe
are tests/lifecycle_cases.py, checked without a GPU by test_lifecycle_cpu.py).

One hierarchy lives through a whole walk.  After every step -- the setter, then a disturbance: a call that documents what it leaves
behind or claims to leave nothing -- the same probe runs on the long-lived hierarchy, on one created for the step with the settings
the record says the long-lived one now has, and on the restated hierarchy of those settings:
  long-lived against fresh   bit for bit: every array the probe records, the residual, PCG's k, conv, history and x (the same code
                             from the same state); ResidualNorm by the tolerance of the operator's own test;
  fresh against restated     bit for bit: Relax, the residual, the three V-cycles, FullMultiGridVCycle and the cycle from level 1 on
                             every level (PCG against the restated solver is the feature files' business).
A failure names the walk, the step, the setter and the one before it, the disturbance, the first item that differs and whether fresh
and restated agree: if they do, the long-lived hierarchy holds stale state; if not, a kernel or the restatement is wrong."""
import numpy as np
import pytest

import lifecycle_cases as LC
import pde_multigrid_amd as P

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
WALK_IDS = [w.name for w in LC.WALKS]


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


def snapshot(mg):
    """everything a refused call must leave alone: the settings, and every array of every level"""
    m = mg._mg.contents
    out = {"shift": mg.shift, "mask": int(m.bc), "wall": mg.wall, "mean": mg.face_mean, "numGrids": mg.numGrids, "use_graph": mg.use_graph,
           "coefficient": mg.has_coefficient, "capacity": mg.has_capacity, "graph": bool(m.graph_exec[0]), "pcg graph": bool(m.pcg_graph_exec)}
    for l in range(mg.maxGrids):
        out["v[%d]" % l], out["f[%d]" % l], out["pins[%d]" % l] = mg.download_v(l), mg.download_f(l), mg.pinned(l)
        if mg.has_coefficient:
            out["a[%d]" % l] = mg.download_coefficient(l)
        if mg.has_capacity:
            out["c[%d]" % l] = mg.download_capacity(l)
    return out


def changed(before, after):
    return [k for k in before if not LC._same(before[k], after[k])]


def refused(call):
    with pytest.raises(P.MgxError) as e:
        call()
    assert e.value.status == P.MGX_ERR_INVALID, e.value


def solve_f32(mg, s):
    mg.upload_v(0, LC.field(s, "v0"))
    mg.upload_f(0, LC.field(s, "f"))
    k, rel, conv, hist = mg.PCG(2, 2, LC.pcg_tol(s.dtype), LC.PCG_MAXIT, krylov=True, precond="f32")
    return k, conv, hist, mg.download_v(0)


def f32_matches_a_fresh_hierarchy(ctx, mg, s):
    """PCG(precond='f32') on a plain hierarchy, whatever fp32 twin it has kept, against one that builds its twin now"""
    got = solve_f32(mg, s)
    fr = LC.fresh(ctx, s)
    try:
        want = solve_f32(fr, s)
    finally:
        fr.close()
    assert got[1] and want[1], "PCG(precond='f32') did not converge"
    assert got[:2] == want[:2] and LC._same(got[2], want[2]) and LC._same(got[3], want[3]), \
        "PCG(precond='f32'): %d iterations on the long-lived hierarchy, %d on a fresh one, or other bits" % (got[0], want[0])


def disturb(ctx, mg, walk, st):
    """the call between the setter and the probe; the record after it is st.now"""
    s, name, tol = st.set, st.disturbance, LC.pcg_tol(st.set.dtype)
    if name == "Eigen(2)":  # "v[0] and f[0] are left as they were" (MultiGrid3D.Eigen)
        v, f = mg.download_v(0), mg.download_f(0)
        mg.Eigen(2, tol=1e-6, maxit=30)
        assert LC._same(v, mg.download_v(0)) and LC._same(f, mg.download_f(0)), "Eigen changed v[0] or f[0]"
    elif name == "PCG in every krylov mode":
        for mode in LC.krylov_modes(s):
            mg.PCG(2, 2, tol, 3, krylov=mode)
    elif name == "PCG(precond='f32')":
        if s.plain:
            f32_matches_a_fresh_hierarchy(ctx, mg, s)
        else:  # refused with any feature set, and nothing changes
            before = snapshot(mg)
            refused(lambda: mg.PCG(2, 2, tol, 3, precond="f32"))
            assert not changed(before, snapshot(mg)), ("the refused PCG(precond='f32') changed", changed(before, snapshot(mg)))
    elif name == "BackwardEuler(1)":  # "The shift it sets STAYS SET afterwards" (mg_multigrid.h)
        mg.BackwardEuler(1, LC.BE_DT, LC.BE_KAPPA, None, 2, 2, tol, LC.PCG_MAXIT, krylov="weighted" if s.bc else True)
        assert mg.shift == st.now.shift, (mg.shift, st.now.shift)
    elif name == "VCycle(1, 1, 1)":
        mg.VCycle(1, 1, 1)
    elif name == "upload_v(1)":  # a non-zero rim on a level that the cycles from level 0 use for corrections
        mg.upload_v(1, LC.field(s, "v1", LC.plan(s)[0][1]))
    elif name == "setToValue_v":
        mg.setToValue_v(0, 0.25, True)
        mg.setToValue_v(1, 0.5, True)
    else:
        assert name == "a refused setter", name
        calls = LC.refusals(s)
        what, call = calls[(walk.rot + st.index) % len(calls)]
        before = snapshot(mg)
        refused(lambda: call(mg))
        assert not changed(before, snapshot(mg)), ("the refused setter (%s) changed" % what, changed(before, snapshot(mg)))


def graphs_left(mg):
    m = mg._mg.contents
    return [l for l in range(mg.maxGrids) if m.graph_exec[l]] + (["PCG"] if m.pcg_graph_exec else [])


def check_step(st, long, fresh, rest):
    """the assertions of one step, as a list of what failed"""
    s, out = st.now, []
    agree = LC.first_difference(fresh, rest, calls={it[0] for it in rest.items})
    verdict = ("fresh and restated agree: stale state in the long-lived hierarchy" if agree is None else
               "fresh and restated differ too (%s): a wrong kernel or a wrong restatement" % agree)
    d = LC.first_difference(long, fresh, skip=("norm",))
    if d is not None:
        out.append("long-lived against fresh: %s; %s" % (d, verdict))
    if agree is not None:
        out.append("fresh against restated: %s" % agree)
    want = LC.item(rest, "ResidualNorm(0)", 0, "norm")
    tol = 1e-5 if s.plain else 1e-12  # the plain route's tolerance is test_gpu_graph_replay.py's, the operators' their own files'
    for who, p in (("long-lived", long), ("fresh", fresh)):
        got = LC.item(p, "ResidualNorm(0)", 0, "norm")
        if not abs(got - want) <= tol * want:
            out.append("ResidualNorm on the %s hierarchy: %r, restated %r (tolerance %g)" % (who, got, want, tol))
        if not p.pcg[2]:
            out.append("PCG on the %s hierarchy did not converge: %d iterations, rel %g" % (who, p.pcg[0], p.pcg[1]))
        if not LC._same(LC.item(p, "PCG", 0, "f"), LC.item(p, "upload + add_wall_flux", 0, "f")):
            out.append("PCG on the %s hierarchy did not restore f[0]" % who)
        if s.pin:
            pin, g = LC.field(s, s.pin), LC.field(s, s.pin_values)
            for it in p.items:
                if it[1] == 0 and it[2] in ("v", "x") and not LC._same(it[3][pin], g[pin]):
                    out.append("%s hierarchy, %s: the pins do not hold their values" % (who, it[0]))
                    break
            if LC.item(p, "CalculateResidual(0)", 0, "r")[pin].any():
                out.append("%s hierarchy: the residual is not 0 at the pins" % who)
    if st.use_graph:
        before, after = long.replay
        if not (after[0] and before == after):
            out.append("use_graph: the third V-cycle captured again instead of replaying (or there is no graph)")
    return out


def run_walk(ctx, walk, dtype, target=lambda st: st.now):
    """the whole walk on one hierarchy; returns what failed, step by step.  target: the settings the comparison hierarchy of a step is
    created with -- the record's; anything else must be reported at every step that changes the operator"""
    failures = []
    mg = LC.fresh(ctx, LC.start(walk.n3, walk.rng, dtype, walk.coarsening))
    mg.use_graph = walk.graph
    long = fresh = None
    try:
        for st in LC.states(walk, dtype):
            where = "walk %r (%s), step %d: %r after %r, then %s" % (walk.name, np.dtype(dtype).name, st.index, st.step, st.prev_step, st.disturbance)
            try:
                had = graphs_left(mg)
                LC.apply(mg, st.before, st.step)
                if LC.drops_graphs(st.before, st.step) and graphs_left(mg):
                    failures.append("%s: the setter kept the captured graphs %r (of %r)" % (where, graphs_left(mg), had))
                assert mg.use_graph == st.use_graph
                disturb(ctx, mg, walk, st)
                long = LC.probe(LC.Lib(mg, ctx), st.now)
                fr = LC.fresh(ctx, target(st))
                try:
                    fresh = LC.probe(LC.Lib(fr, ctx), target(st))
                finally:
                    fr.close()
                rest = LC.probe(LC.Rest(LC.restated(st.now)), st.now)
                failures += ["%s: %s" % (where, what) for what in check_step(st, long, fresh, rest)]
            except (P.MgxError, AssertionError) as e:  # the state is no longer the record's: the walk ends here
                failures.append("%s: %s: %s" % (where, type(e).__name__, e))
                return failures
        if walk.ends_plain:  # (fresh is then a hierarchy that never had a setting: the constructor's defaults)
            assert st.now.cleared
            if long.kernels != fresh.kernels or any("relax_shift" in k for k in long.kernels):
                failures.append("walk %r: back to plain, the first V-cycle ran %r; a hierarchy that never had a setting runs %r" %
                                (walk.name, long.kernels, fresh.kernels))
            if np.dtype(dtype) == np.float64:
                try:
                    f32_matches_a_fresh_hierarchy(ctx, mg, st.now)
                except (P.MgxError, AssertionError) as e:
                    failures.append("walk %r: back to plain: %s" % (walk.name, e))
    finally:
        mg.close()
    return failures


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_zero_guess_solved_under_a_mask_then_the_mask_cleared(ctx, dtype):
    """What the probe cannot reach, because it uploads v[0] first: level 0's v_rim_zero.  A hierarchy is created with walls (v = 0,
    the flag set), PCG(krylov="weighted") solves from that zero guess -- the solution's face unknowns are not 0 --, the mask is
    cleared, and the next right-hand side is solved from the iterate as it stands: the bits of a fresh hierarchy given that iterate
    (whose preconditioner zeroes the rim of its correction).  DESIGN.md 23: the flag PCG used to put back."""
    s = LC.advance(LC.advance(LC.start((33, 17, 9), LC.RG, dtype), ("shift", 0.75)), ("neumann", 0b100101))
    plain = LC.advance(s, ("neumann", 0))
    f, f2, tol = LC.field(s, "f"), LC.field(s, "g1"), LC.pcg_tol(dtype)
    mg, fr = LC.fresh(ctx, s), LC.fresh(ctx, plain)
    try:
        mg.upload_f(0, f)
        assert mg.PCG(2, 2, tol, LC.PCG_MAXIT, krylov="weighted")[2]
        x = mg.download_v(0)
        assert x[:, :, 0].any() and not x[:, :, -1].any()  # x-low is a wall, x-high Dirichlet data (zeros)
        mg.set_neumann(None)
        got, want = [], []
        for h, out in ((mg, got), (fr, want)):
            if h is fr:
                h.upload_v(0, x)
            h.upload_f(0, f2)
            k, rel, conv, hist = h.PCG(2, 2, tol, LC.PCG_MAXIT, krylov=True)
            out += [k, conv, hist, h.download_v(0)]
        print("after the mask was cleared: %d iterations on the long-lived hierarchy, %d on a fresh one" % (got[0], want[0]))
        assert want[1] and got[:2] == want[:2] and LC._same(got[2], want[2]) and LC._same(got[3], want[3])
    finally:
        mg.close()
        fr.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", WALK_IDS)
def test_walk(ctx, name, dtype):
    failures = run_walk(ctx, LC.WALKS[WALK_IDS.index(name)], dtype)
    assert not failures, "%d failures:\n%s" % (len(failures), "\n".join(failures))
