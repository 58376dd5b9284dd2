"""CPU suite: bench.py --dump-outputs without a GPU.  What one rank writes for a whole finest v is what three ranks write
for z-slabs of it (joined by rank 0 through the bench's control plane); a v too large for 64 MB is written as the seeded
sample and the centre plane."""
import os
import threading

import numpy as np
import pytest

import bench


def _dump(path, v, cuts):
    """bench.dump_outputs of `v` cut into z-slabs at `cuts`, one thread per rank"""
    n, world = v.shape[0], len(cuts) - 1
    if world == 1:
        bench.dump_outputs(str(path), v, 0, n, 0, 1, None)
        return
    launch, errors = bench.load_launch(), []

    def rank(r):
        try:
            rdzv = launch.Rendezvous(r, world, key="dump_test_%d_%s" % (os.getpid(), path.name), timeout=60)
            bench.dump_outputs(str(path), np.ascontiguousarray(v[cuts[r]:cuts[r + 1]]), cuts[r], n, r, world, rdzv)
            rdzv.close()
        except Exception as e:  # noqa: BLE001  (re-raised below, in the test's thread)
            errors.append(e)
    ts = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not errors, errors


@pytest.mark.parametrize("n,dtype", [(129, np.float64), (257, np.float64), (257, np.float32)])
def test_slabs_join_to_the_one_rank_dump(tmp_path, n, dtype):
    v = np.random.default_rng(n).uniform(-1, 1, (n, n, n)).astype(dtype)
    one, three = tmp_path / "one", tmp_path / "three"
    _dump(one, v, [0, n])
    _dump(three, v, [0, n // 5, n // 2 + 3, n])
    files = sorted(os.listdir(one))
    assert sorted(os.listdir(three)) == files
    assert sum(os.path.getsize(one / f) for f in files) <= 64_000_000
    if v.nbytes <= 60_000_000:
        want = {"v.npy": v}
    else:
        want = {"v_sample.npy": v.reshape(-1)[bench.dump_sample_index(n)], "v_centre_plane.npy": v[n // 2]}
    assert files == sorted(want)
    for f, a in want.items():
        for d in (one, three):
            got = np.load(d / f)
            assert got.dtype == dtype and np.array_equal(got, a), (d, f)
    idx = bench.dump_sample_index(n)
    assert np.array_equal(idx, bench.dump_sample_index(n)) and np.all(np.diff(idx) > 0) and idx[-1] < n ** 3
