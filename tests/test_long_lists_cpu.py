"""The inputs of test_gpu_zzz_long_face_lists.py reach what they are chosen for, without a GPU: on every shape of long_lists.TABLE the
list of face points is longer than one rim launch covers (4096 blocks of 256 threads), in the tabulated number of rounds; the points
visited after the first round are of both colours and, on A with all six faces, of all three kinds of face; the restated list visits
exactly the face unknowns of op_restated, every one once; and the library itself says that the launch is capped there.  Should the
row pitch or the cap change, this file fails and the GPU tests do not quietly lose their purpose."""
import ctypes as C

import numpy as np
import pytest

import long_lists as LL
import op_restated as OP
import oracle as O
import pde_multigrid_amd as P

IDS = ["%s-%d" % (name, bc) for name, _, bc, _, _ in LL.TABLE]


@pytest.mark.parametrize("dtype", LL.DTYPES)
@pytest.mark.parametrize("row", LL.TABLE, ids=IDS)
def test_tabulated_lengths_and_rounds(row, dtype):
    name, n3, bc, entries, rounds = row
    k = LL.DTYPES.index(dtype)
    assert LL.listed(n3, bc, dtype) == entries[k]
    assert LL.rounds(n3, bc, dtype) == rounds[k] >= 2
    assert LL.round_of(n3, bc, dtype).max() == rounds[k] - 1, "the last round visits no unknown"


@pytest.mark.parametrize("dtype", LL.DTYPES)
@pytest.mark.parametrize("row", LL.TABLE, ids=IDS)
def test_later_rounds_hold_both_colours_and_the_list_is_the_face_unknowns(row, dtype):
    name, n3, bc, entries, rounds = row
    rnd, count = LL.visits(n3, bc, dtype)
    later = rnd >= 1
    col = OP.colours(n3)
    assert (later & (col == 0)).any() and (later & (col == 1)).any()
    m = OP.face_unknowns(n3, bc)
    assert np.array_equal(rnd >= 0, m), "the restated list does not visit exactly the face unknowns"
    assert np.array_equal(count, m.astype(np.int64)), "a face unknown is listed more than once"
    on = OP.on_faces(n3)
    if name == "A" and bc == 63:  # the second round: the last rows of z-high and ALL y- and x-face points
        assert (later & (on == 32)).any() and not (later & ((on & 16) != 0)).any()
        for face in (4, 8, 1, 2):
            assert np.array_equal(later & (on == face), on == face), face
        assert ((rnd == 0) & ((on & 32) != 0)).any(), "z-high lies in both rounds"
    if name == "Y" and bc == 12:  # the tail in rows of y-high
        assert np.array_equal(on[later] & 8, np.full(int(later.sum()), 8))


@pytest.mark.parametrize("sfx,dtype", [("f64", np.float64), ("f32", np.float32)])
def test_the_library_caps_the_launch_on_these_shapes(sfx, dtype):
    """mgx3dxs_krylov_work_elems_bc: two sums, each the interior partials plus the rim partials of all six faces -- 4096 here"""
    fn = getattr(P.lib, "mgx3dxs_krylov_work_elems_bc_" + sfx)
    fn.restype = C.c_size_t
    for name, n3 in LL.SHAPES.items():
        interior = -(-(n3[1] - 2) // 4) * (n3[2] - 2)
        assert fn((C.c_int * 3)(*n3)) == 2 * (interior + LL.RIM_MAX_BLOCKS), name
        assert LL.listed(n3, 63, dtype) > LL.CAP, name
    for n3 in LL.CONTROLS:
        interior = -(-(n3[1] - 2) // 4) * (n3[2] - 2)
        assert fn((C.c_int * 3)(*n3)) == 2 * (interior + -(-LL.listed(n3, 63, dtype) // LL.RIM_THREADS)) < 2 * (interior + LL.RIM_MAX_BLOCKS)


@pytest.mark.parametrize("dtype", LL.DTYPES)
def test_the_shapes_of_the_other_files_never_stride(dtype):
    for n3 in LL.CONTROLS:
        assert LL.rounds(n3, 63, dtype) == 1
        assert LL.round_of(n3, 63, dtype).max() == 0
        assert LL.all_face_unknowns_listed_once(n3, 63, dtype)
    assert LL.listed((513, 5, 5), 63, dtype) == (8466 if dtype == np.float64 else 8722)  # the longest list the other files build


def test_the_sizes_the_solver_is_built_for_stride():
    """the closed box at 513^3 and a single flagged z-face at 1025^3"""
    assert LL.listed((513,) * 3, 63, np.float64) == 1603586 and LL.listed((513,) * 3, 63, np.float32) == 1636354
    assert LL.rounds((513,) * 3, 63, np.float64) == LL.rounds((513,) * 3, 63, np.float32) == 2
    for dtype in LL.DTYPES:
        assert LL.rounds((1025,) * 3, 16, dtype) == LL.rounds((1025,) * 3, 4, dtype) == 2
        assert LL.listed((1025,) * 3, 1, dtype) == 1023 ** 2 < LL.CAP  # an x-face alone stays just below the cap


def test_the_hierarchy_of_shape_a_has_two_levels():
    assert OP.full_plan(LL.A)[0] == [LL.A, (513, 257, 3)]
    assert O.csize(LL.F) == LL.C


def test_diagnose_names_the_lowest_round():
    n3, bc = (33, 9, 5), 63
    rnd = LL.round_of(n3, bc, np.float64).copy()
    want = np.random.default_rng(0).uniform(-1, 1, O.shape(n3))
    assert LL.diagnose(want.copy(), want, rnd) is None
    nan = want.copy()
    nan[0, 0, 0] = np.nan
    assert LL.diagnose(nan, nan.copy(), rnd) is None, "NaNs of the same bits are equal"
    rnd[rnd >= 0] = 0
    rnd[4, 3:, :] = 1  # a made-up second round
    got = want.copy()
    got[4, 5, 7] += 1.0
    got[2, 4, 9] += 1.0  # interior: off the list
    text = LL.diagnose(got, want, rnd)
    assert "2 points differ" in text and "1 on the list, the lowest round 1" in text and "1 off the list" in text, text
    got[0, 1, 1] -= 1.0
    assert "the lowest round 0 (per round [1, 1])" in LL.diagnose(got, want, rnd)
    neg = want.copy()
    neg[2, 2, 2] = 0.0
    z = neg.copy()
    z[2, 2, 2] = -0.0
    assert LL.diagnose(z, neg, rnd) is not None, "zeros of different signs differ"
