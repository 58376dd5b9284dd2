"""The walks of tests/lifecycle_cases.py checked without a GPU: that they cover what they claim and are legal, that
every step can be seen by the probe -- on level 0, and through the coarse levels alone --, that the restated solver converges from
every state the GPU test solves from, and that the probe's adapter runs the call sequence the feature files write out.  Run with -s
for the coverage table and the observability result per step."""
import dataclasses
import functools

import numpy as np
import pytest

import lifecycle_cases as LC
import op_restated as R
import pin_restated as PR
from conftest import bits_equal

DTYPES = [np.float64, np.float32]
WALK_IDS = [w.name for w in LC.WALKS]


# ------------------------------------------------------------------------------------------ coverage
def test_every_ordered_pair_of_kinds_and_every_self_pair():
    got = LC.pairs()
    print("\n" + LC.coverage_table())
    print("\n".join("%d = %s (%s, %s, %d steps)" % (i, w.name, "x".join(map(str, w.n3)), w.coarsening, len(w.steps)) for i, w in enumerate(LC.WALKS)))
    missing = [(a, b) for a in LC.KINDS for b in LC.KINDS if (a, b) not in got]
    assert not missing, missing


def test_the_walks_have_the_shapes_and_lengths_of_the_issue():
    assert len({w.name for w in LC.WALKS}) == len(LC.WALKS)
    assert all(1 <= len(w.steps) <= 16 for w in LC.WALKS)
    shapes = {(w.n3, w.coarsening) for w in LC.WALKS}
    assert shapes == {((33, 17, 9), "full"), ((17, 33, 17), "full"), ((9, 9, 65), "semi"), ((33, 33, 33), "full")}
    assert all(w.rng == (LC.UNIT if w.n3 == (33, 33, 33) else LC.RG) for w in LC.WALKS)
    levels = {w.n3: LC.max_grids(LC.start(w.n3, w.rng, np.float64, w.coarsening)) for w in LC.WALKS}
    assert levels[(33, 17, 9)] == 3 and levels[(17, 33, 17)] == 4
    graph = sum(w.graph for w in LC.WALKS)
    assert graph * 2 == len(LC.WALKS), "half the walks start with use_graph"
    assert sum(w.ends_plain for w in LC.WALKS) >= 2
    assert any(w.ends_plain and w.n3 == (33, 33, 33) for w in LC.WALKS)
    assert all(k == "use_graph" or v is not True for w in LC.WALKS for k, v in w.steps)


@pytest.mark.parametrize("name", WALK_IDS)
def test_every_step_is_legal(name):
    """by the rules of mg_multigrid.h, as LC.legal states them: a capacity needs a coefficient, a face is cleared only without wall
    data, a semi-coarsened hierarchy refuses masks, the closed box needs a shift or a beta > 0 (pins or not); BackwardEuler's shift
    is part of the record the next step meets.  A semi-coarsened walk has no mask and no wall at all"""
    w = LC.WALKS[WALK_IDS.index(name)]
    for dtype in DTYPES:
        for st in LC.states(w, dtype):
            why = LC.legal(st.before, st.step)
            assert why is None, (st.index, st.step, why)
            assert st.now.regular and (w.coarsening != "semi" or st.step[0] not in ("neumann", "wall")), (st.index, st.step)
            if st.step[0] == "pinned" and st.step[1]:
                assert not (LC.field(st.now, st.now.pin) & (R.on_faces(w.n3) != 0)).any()
                assert LC.field(st.now, st.now.pin).any()
            if st.step[0] != "use_graph":
                assert LC.changes_operator(st.before, st.step), (st.index, st.step, "sets what is set already")
            else:
                assert st.use_graph != (LC.states(w, dtype)[st.index - 1].use_graph if st.index else w.graph), (st.index, "use_graph stays")


def test_the_walks_that_end_plain_do():
    for w in LC.WALKS:
        for dtype in DTYPES:
            end = LC.states(w, dtype)[-1].now
            assert end.cleared == w.ends_plain, (w.name, end)


def test_mask_63_is_made_regular_by_a_shift_and_by_a_beta():
    seen = set()
    for w in LC.WALKS:
        for st in LC.states(w, np.float64):
            if st.now.bc == 63:
                seen.add(("shift", st.now.shift > 0) + ("beta", any(b > 0 for b in st.now.beta)))
    assert ("shift", True, "beta", False) in seen and ("shift", False, "beta", True) in seen, seen


def test_every_disturbance_runs_and_the_rotation_is_the_records():
    seen = set()
    for w in LC.WALKS:
        for dtype in DTYPES:
            for st in LC.states(w, dtype):
                seen.add(st.disturbance)
                if st.disturbance == "BackwardEuler(1)":  # the shift stays set: the record carries it on
                    assert st.set.shift != 0 and st.now == dataclasses.replace(st.set, shift=1.0 / (LC.BE_KAPPA * LC.BE_DT))
                else:
                    assert st.now == st.set
                assert len(LC.refusals(st.set)) >= 4
    assert seen == set(LC.DISTURBANCES)
    # PCG(precond='f32') meets a plain fp64 state (it runs and builds the twin) and, later in the same walk, states with a feature (it
    # is refused); the GPU test runs it once more when that walk is back to plain
    w = [w for w in LC.WALKS if w.ends_plain and w.n3 == (33, 33, 33)][0]
    f32 = [st.set.plain for st in LC.states(w, np.float64) if st.disturbance == "PCG(precond='f32')"]
    assert f32[0] is True and False in f32[1:], f32


# ------------------------------------------------------------------------------------------ observability
@functools.lru_cache(maxsize=None)
def _probe(s):
    return LC.probe(LC.Rest(LC.restated(s)), s)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", WALK_IDS)
def test_every_step_is_observable(name, dtype):
    """a step the probe cannot see tests nothing: the restated probe of the settings the step leaves (st.now, what the GPU test
    probes) and that of the settings it met (with the after-effect of the step's disturbance, which the long-lived hierarchy has in
    any case) differ in the bits of a level-0 array, and so does one whose coarse levels (operators, coefficients, pin sets, pin
    values) are still the old ones"""
    w = LC.WALKS[WALK_IDS.index(name)]
    for st in LC.states(w, dtype):
        if st.step[0] == "use_graph":
            print("%-44s step %2d %-50r no operator change" % (w.name, st.index, st.step))
            continue
        now, old = _probe(st.now), LC.after_disturbance(st.before, st.disturbance)
        d0 = LC.first_difference(_probe(old), now, level0=True)
        assert d0 is not None, (st.index, st.step, "the probe cannot tell the settings before the step from those after it")
        d1 = "exempt"
        if LC.reaches_coarse_levels(st.before, st.step):
            hyb = LC.probe(LC.Rest(LC.hybrid(old, st.now)), st.now)
            d1 = LC.first_difference(hyb, LC.probe(LC.Rest(LC.restated(st.now, True)), st.now), level0=True)
            assert d1 is not None, (st.index, st.step, "the probe cannot tell stale coarse levels from current ones")
        print("%-44s step %2d %-50r level 0: %s | stale coarse levels: %s" % (w.name, st.index, st.step, d0.split(",")[0], d1.split(",")[0]))


def test_an_empty_pin_set_is_the_plain_restatement():
    """(the hybrid builds PinHierarchy with an empty set where the settings have no pins)"""
    s = LC.advance(LC.advance(LC.start((33, 17, 9), LC.RG, np.float32), ("shift", 0.75)), ("coefficient", "a1"))
    assert LC.first_difference(LC.probe(LC.Rest(LC.restated(s, True)), s), _probe(s)) is None


# ------------------------------------------------------------------------------------------ convergence
def _distinct_states():
    out = {}
    for w in LC.WALKS:
        for st in LC.states(w, np.float64):
            out.setdefault(st.now, (w.name, st.index))
    return out


def test_the_restated_solver_converges_from_every_state():
    """fp64, every distinct record a probe meets: within 20 of PCG's 30 iterations, so that the GPU test can assert `conv` outright"""
    worst = 0
    for s, where in _distinct_states().items():
        k, conv, rel = LC.restated_solve(s)
        worst = max(worst, k)
        assert conv and k <= 20 and rel < LC.pcg_tol(s.dtype), (where, k, rel)
    print("\n%d distinct states, at most %d iterations" % (len(_distinct_states()), worst))


# ------------------------------------------------------------------------------------------ the adapter
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,index", [(WALK_IDS[0], 11), (WALK_IDS[3], 4), (WALK_IDS[6], 5)])
def test_the_adapter_runs_the_call_sequence_of_the_feature_files(name, index, dtype):
    """probe(restated(S)) against H.relax / residual / vcycle / fmg written out as test_gpu_zzzz_pin.py and test_gpu_robin.py do"""
    s = LC.states(LC.WALKS[WALK_IDS.index(name)], dtype)[index].now
    p = _probe(s)
    H = LC.restated(s)
    v0, f = LC.field(s, "v0"), LC.field(s, "f")
    if s.pin:
        assert isinstance(H, PR.PinHierarchy)
        H.set_v(v0)
    else:
        assert type(H) is R.Hierarchy
        H.v[0] = np.array(v0, s.dtype)
    H.f[0] = np.array(f, s.dtype)
    if any(s.g):
        H.add_wall_flux()
    H.relax(0, 1)
    assert bits_equal(LC.item(p, "Relax(0, 1)", 0, "v"), H.v[0])
    assert bits_equal(LC.item(p, "CalculateResidual(0)", 0, "r"), H.residual(0))
    for i in range(3):
        H.vcycle(0, 2, 2)
        for l in range(s.numGrids):
            assert bits_equal(LC.item(p, "VCycle(0, 2, 2) #%d" % (i + 1), l, "v"), H.v[l]), (i, l)
            assert bits_equal(LC.item(p, "VCycle(0, 2, 2) #%d" % (i + 1), l, "f"), H.f[l]), (i, l)
    H.fmg(0, 1, 2, 2)
    for l in range(s.numGrids):
        assert bits_equal(LC.item(p, "FullMultiGridVCycle(0, 1, 2, 2)", l, "v"), H.v[l]), l
    H.vcycle(1, 1, 1)
    assert bits_equal(LC.item(p, "VCycle(1, 1, 1)", 1, "v"), H.v[1]) and bits_equal(LC.item(p, "VCycle(1, 1, 1)", 0, "v"), H.v[0])
    assert len(H.sizes) == s.numGrids
