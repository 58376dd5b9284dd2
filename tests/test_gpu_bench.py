"""GPU suite: bench.py itself.  The slab-decomposed branch with one rank (MGX_BENCH_FORCE_DIST=1: rendezvous, RCCL
communicator, slab hierarchy) must pass its result check WITHOUT PyTorch in the process, report what the communicator
says about itself, and the default N = 1 line must carry the contract's fields, the batch statistics and the secondary
configurations with their own result checks."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, env_extra=None, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MGX_RDZV_KEY")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.timeout(900)
def test_forced_slab_branch_one_rank_without_torch():
    out = _bench(["--gpus", "1", "--size", "257", "--steps", "3", "--warmup", "1", "--batches", "2", "--no-cpu-baseline"],
                 {"MGX_BENCH_FORCE_DIST": "1"})
    assert out["result_check"]["status"] == "ok"
    comm = out["config"]["communicator"]
    assert comm["ranks_seen"] == 1 and comm["rccl_version"] > 20000 and comm["torch_imported"] is False
    assert out["n_gpus"] == 1 and out["steps"] == 3 and len(out["batches"]["ms_per_step"]) == 2


@pytest.mark.timeout(900)
def test_default_line_contract_and_secondary_configs():
    out = _bench(["--steps", "5", "--warmup", "2", "--batches", "3", "--no-cpu-baseline"])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline"):
        assert key in out
    assert out["result_check"]["status"] == "ok"
    assert out["batches"]["min"] <= out["batches"]["median"] == out["ms_per_step"]
    assert 0.3 < out["roofline"]["frac"] < 1.0 and out["roofline"]["bound"] == "hbm"
    down = out["roofline_down"]  # the fused last black pass + residual + restrict launch of the finest level
    assert down["kernel"].startswith("relax_rr3d_xs_kernel<double") and 0.2 < down["frac"] < 1.0 and down["avg_launch_us"] > 100
    sec = out["secondary"]
    assert len(sec) == 5 and all(c["result_check"] == "ok" for c in sec.values()), sec  # configs[1], [2], fp32, the two published workloads
    pub = [c for k, c in sec.items() if k.startswith("published workload")][0]
    assert 0.05 < pub["seconds"] < 5.0 and pub["known_answer"] == "3d_n129_fmg_2_3000_3000_f32"


@pytest.mark.timeout(900)
@pytest.mark.parametrize("n", [65, 513])
def test_dump_outputs_are_the_last_timed_step(tmp_path, n):
    """--dump-outputs: the finest v after W + 1 + K cycles from v = 0 (v.npy whole when it fits into 64 MB, else the
    seeded sample and the centre plane), bit for bit what the same cycles give in this process; --steps K times K steps"""
    import numpy as np

    import bench
    import pde_multigrid_amd as P

    w, k = 2, 3
    out = _bench(["--size", str(n), "--steps", str(k), "--warmup", str(w), "--batches", "2", "--no-secondary", "--no-cpu-baseline",
                  "--dump-outputs", str(tmp_path)])
    assert out["steps"] == k and len(out["batches"]["ms_per_step"]) == 2
    files = sorted(os.listdir(tmp_path))
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in files) <= 64_000_000
    ctx = P.Context(0)
    mg = P.MultiGrid3D(ctx, [n] * 3, [0, 1, 0, 1, 0, 1], np.float64)
    mg.setToValue_v(0, 0.0, True)
    for _ in range(w + 1 + k):
        mg.VCycle(0, 2, 2)
    want = mg.download_v(0)
    mg.close()
    ctx.close()
    if n == 65:
        assert files == ["v.npy"]
        parts = {"v": want}
    else:
        assert files == ["v_centre_plane.npy", "v_sample.npy"]
        parts = {"v_sample": want.reshape(-1)[bench.dump_sample_index(n)], "v_centre_plane": want[n // 2]}
    for name, a in parts.items():
        got = np.load(os.path.join(tmp_path, name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), a.view(np.uint64)), name
