"""Semi-coarsening without a GPU: the level rule of the library (mg_semi_plan, host arithmetic) against its Python restatement
and the issue's table, and the restated cycle (tests/semi_restated.py: the oracle's smoother and residual, numpy transfers) as a
solver on the anisotropic grids that full coarsening cannot handle."""
import numpy as np
import pytest

import oracle as O
import pde_multigrid_amd as P
import semi_restated as S
from solve_restated import problem


@pytest.mark.parametrize("case", range(len(S.TABLE) + 1))
def test_plan_matches_rule_and_table(case):
    n3, rng, masks = (S.TABLE + [S.ODD])[case]
    sizes, got = P.semi_plan(n3, rng)
    want_sizes, want = S.plan(n3, rng)
    assert sizes == want_sizes and got == want
    assert got[:-1] == masks and got[-1] == 0, (got, masks)
    assert len(sizes) == len(masks) + 1
    for l, m in enumerate(got[:-1]):
        assert sizes[l + 1] == S.coarse_size(sizes[l], m)
    if case == len(S.TABLE):
        assert sizes[-1] == (7, 11, 15)


def test_plan_max_levels():
    n3, rng, masks = S.TABLE[0]
    for k in (1, 2, 5, 40):
        sizes, got = P.semi_plan(n3, rng, k)
        assert (sizes, got) == S.plan(n3, rng, k)
        assert len(sizes) == min(k, len(masks) + 1) and got[-1] == 0


@pytest.mark.parametrize("n", [5, 17, 33, 129])
def test_plan_of_a_cube_is_full_coarsening(n):
    sizes, masks = P.semi_plan((n, n, n), [0, 1, 0, 1, 0, 1])
    assert len(sizes) == P.num_grids(n)
    assert masks == (7,) * (len(sizes) - 1) + (0,)
    want = [(n, n, n)]
    while len(want) < len(sizes):
        want.append(tuple(P.coarse_size(want[-1])))
    assert sizes == want


@pytest.mark.parametrize("n3", [(64, 65, 65), (65, 65, 34), (65, 1, 65)])
def test_plan_rejects_even_and_small_sizes(n3):
    with pytest.raises(P.MgxError) as e:
        P.semi_plan(n3, [0, 1, 0, 1, 0, 1])
    assert e.value.status == P.MGX_ERR_SIZE
    with pytest.raises(ValueError):
        S.plan(n3, [0, 1, 0, 1, 0, 1])


def test_restated_transfers_are_transposes_on_constants():
    """a constant is interpolated to itself, and restriction of a constant gives it back (the weights sum to 1)"""
    for mask in range(1, 7):
        n3 = (17, 9, 13)
        cn = S.coarse_size(n3, mask)
        fine = np.full(O.shape(n3), 3.0)
        assert np.array_equal(S.restrict_axes(fine, mask), np.full(O.shape(cn), 3.0))
        got = S.interpolate_axes(np.zeros(O.shape(n3)), np.full(O.shape(cn), 3.0), mask)
        assert np.array_equal(got[1:-1, 1:-1, 1:-1], fine[1:-1, 1:-1, 1:-1]) and not got[0].any()


@pytest.mark.parametrize("case", range(4))
def test_restated_cycle_converges_within_10_cycles(case):
    """fp64 V(2,2) from a zero guess on a random interior right-hand side to a true relative residual below 1e-10.
    Counts with this summation: 9, 9, 8, 8; the cap of 10 is the issue's."""
    n3, rng, _ = S.TABLE[case]
    k, rel = S.cycles_to(n3, rng, problem(n3), 2, 2, 1e-10, 10)
    print("semi V(2,2) on %s: %d cycles, rel %.3e" % (n3, k, rel))
    assert rel < 1e-10 and k <= 10, (k, rel)
