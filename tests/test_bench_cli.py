"""bench.py's command line: a plain run is the headline alone, --full adds the rest, --dump-outputs writes what the timed path
computed in its last step (float64 .npy files, a fixed sample of the envs, under 64 MB)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from pomcpp_amd.state import new_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_full_and_dump_outputs_are_off_by_default():
    import bench
    a = bench.parse_args([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3", "--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d" and a.steps == 7 and a.warmup == 3


class _FakeEnv:
    """the three reads dump_outputs makes of a BatchEnvironment, over host arrays"""

    def __init__(self, n):
        self.n = n
        rng = np.random.default_rng(3)
        self.states = new_states(n)
        self.states["board"] = rng.integers(0, 1 << 24, size=(n, 11, 11)) + (1 << 24)  # AGENT0..: beyond float32's integers
        self.states["timeStep"] = np.arange(n)
        self.states["agents"]["pad"] = 7  # padding is not part of the State's value

    def episodes(self):
        return np.arange(self.n, dtype=np.uint32) % 5

    def get_state(self):
        return self.states.copy()

    def policy_memory(self):
        return np.arange(self.n * 64, dtype=np.int32).reshape(self.n, 4, 16)


def test_dump_outputs_writes_exact_float64_of_a_fixed_sample(tmp_path):
    import bench
    n = 65536
    env = _FakeEnv(n)
    counters = np.array([n * 20, 17, 0, 0], dtype=np.int64)
    total = bench.dump_outputs(str(tmp_path / "a"), env, counters, with_policy_memory=True)
    assert total <= 64 * 2**20
    files = sorted(os.listdir(tmp_path / "a"))
    assert all(f.endswith(".npy") for f in files) and "state_agents_pad.npy" not in files
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) == total
    idx = got["env_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE_ENVS and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(got["counters"], counters.astype(np.float64))
    assert np.array_equal(got["state_board"], env.states["board"][idx].astype(np.float64))  # exact, not rounded to float32
    assert np.array_equal(got["state_timeStep"], idx.astype(np.float64))
    assert np.array_equal(got["episodes"], (idx % 5).astype(np.float64))
    assert got["policy_memory"].shape == (len(idx), 4, 16)
    # every value of the State but the agents' padding: 1004 bytes = 251 dwords, less 4 x 2 pad bytes, the 4 x 2 flag bytes widened
    per_env = sum(a[0].size for k, a in got.items() if k.startswith("state_"))
    assert per_env == 121 + 2 + 4 * 7 + 20 + 2 + 20 * 4 + 2
    # the same sample, run after run
    bench.dump_outputs(str(tmp_path / "b"), _FakeEnv(n), counters, with_policy_memory=False)
    assert np.array_equal(np.load(tmp_path / "b" / "env_index.npy"), got["env_index"])
    assert not (tmp_path / "b" / "policy_memory.npy").exists()


def test_dump_outputs_takes_every_env_of_a_small_batch(tmp_path):
    import bench
    bench.dump_outputs(str(tmp_path), _FakeEnv(100), np.zeros(4, dtype=np.int64), with_policy_memory=False)
    assert np.array_equal(np.load(tmp_path / "env_index.npy"), np.arange(100.0))
    assert np.load(tmp_path / "state_board.npy").shape == (100, 11, 11)


def _plain_run(out_dir):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs", "4096", "--steps", "12", "--warmup", "3",
                          "--burn-in", "40", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_bench_run_is_the_headline_and_dumps_the_same_outputs_every_run(hip_lib, oracle, tmp_path):
    """two plain runs with the same arguments: the headline's fields, none of --full's, and bit-identical dumped outputs that equal
    the oracle's restatement of the same 40 + 3 + 12 ticks"""
    import pomcpp_amd as pa
    from pomcpp_amd.batch import DIST_RANDOM
    r1 = _plain_run(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in r1, k
    assert r1["metric"] == "env_steps_per_sec" and r1["higher_is_better"] is True and r1["steps"] == 12
    assert abs(r1["value"] * r1["ms_per_step"] * 1e-3 - 4096) < 1.0
    assert "other_configs" not in r1 and "cpu_baseline" not in r1 and "config3_simple_agent" not in r1
    assert r1["roofline"]["step_ms_hip_events"] is None and r1["config"]["full"] is False
    _plain_run(tmp_path / "b")
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and "state_board.npy" in files
    total = 0
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b), f
        total += a.nbytes
    assert total == r1["config"]["dumped_output_bytes"] <= 64 * 2**20
    assert np.load(tmp_path / "a" / "counters.npy")[0] == 4096 * 12
    # what the GPU computed is what the oracle computes from the same boards and move stream (bench.py: seed 1, rank 0)
    start = pa.make_boards(4096, seed=1 * 1000003, kind="ffa")
    want = start.copy()
    oracle.run_random(want, start, 40 + 3 + 12, 1, 0, 0, DIST_RANDOM, 800)
    import bench
    for name, col in bench._state_columns(want):
        assert np.array_equal(np.load(tmp_path / "a" / (name + ".npy")), col.astype(np.float64)), name
