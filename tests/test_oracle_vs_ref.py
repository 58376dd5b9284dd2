"""CPU suite: oracle<float> against the UNMODIFIED compiled reference, bit for bit, on seeded inputs with anisotropic
ranges (the cases: oracle/ref_cases.py).

tests/golden/ref_digests.json holds the SHA-256, shape and dtype of every reference output, so the restatement is
pinned to the reference on every machine.  Where the reference was compiled as well (oracle/_ref/libmgref.so,
`make -C oracle ref`), the two are also compared directly and the stored digests are checked against the reference."""
import json
import os

import pytest

import oracle as O
import ref_cases as RC
import refshim as R
from conftest import GOLDEN, bits_equal

with open(os.path.join(GOLDEN, "ref_digests.json")) as _fh:
    DIGESTS = json.load(_fh)


def _check(name):
    case, want = RC.CASES[name], DIGESTS[name]
    got = case(O)
    assert sorted(got) == sorted(want), name
    if R.available():
        ref = case(R)
        for label in got:
            assert bits_equal(ref[label], got[label]), (name, label)
            assert RC.digest(ref[label]) == want[label], (name, label, "stored digest differs from the compiled reference")
    for label, a in got.items():
        assert RC.digest(a) == want[label], (name, label)


@pytest.mark.parametrize("n,seed", RC.OPS3D)
def test_3d_ops(n, seed):
    _check("3d_ops_n%d_seed%d" % (n, seed))


@pytest.mark.parametrize("n,nlev", RC.ANALYTIC3D)
def test_3d_analytic_cycles(n, nlev):
    _check("3d_analytic_n%d_nlev%d" % (n, nlev))


@pytest.mark.parametrize("n,seed", RC.OPS2D)
def test_2d_ops(n, seed):
    _check("2d_ops_n%d_seed%d" % (n, seed))


def test_2d_thesis_range_analytic():
    _check("2d_thesis_range_analytic")


@pytest.mark.parametrize("n,seed", RC.OPS1D)
def test_1d_ops(n, seed):
    _check("1d_ops_n%d_seed%d" % (n, seed))
