"""bench.py's command line: a plain run measures the headline only, `--steps` sets the timed
rounds, and `--dump-outputs` writes the sampled final state as float32 / float64 arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MEMBERS, STEPS = 100_000, 3


def test_plain_run_headline_and_dump(tmp_path):
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "1", "--members", str(MEMBERS), "--dump-outputs", str(out)],
                       capture_output=True, text=True, cwd=ROOT, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == "gossip node-rounds/s" and line["unit"] == "node-rounds/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u64" and line["steps"] == STEPS
    # value = members x steps / wall and ms_per_step = wall / steps: one timed step's milliseconds
    assert line["ms_per_step"] > 0
    assert line["value"] * line["ms_per_step"] / 1e3 == pytest.approx(MEMBERS, rel=1e-9)
    # what --full adds is not measured in a plain run
    assert line["cpu_baseline"] is None
    assert not {"vivaldi", "model_points_q64", "configs2_shard_regime"} & set(line)
    assert line["error_members"] == 0 and line["cub_canaries_intact"] is True
    arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert all(f.endswith(".npy") for f in os.listdir(out))
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert 0 < sum(a.nbytes for a in arrays.values()) <= 64 << 20
    ids = arrays["member_ids"].astype(np.int64)
    assert np.all(np.diff(ids) > 0) and ids[0] >= 0 and ids[-1] < MEMBERS
    for k in ("clock", "event_clock", "query_clock", "digest_lo", "digest_hi", "err"):
        assert arrays[k].shape == ids.shape
    assert arrays["clock"].min() >= 1 and np.all(arrays["err"] == 0)
    assert arrays["view_ltime"].shape == (len(arrays["view_rows"]), 4096)
    assert arrays["queue_rumor"].shape[:2] == (len(arrays["queue_rows"]), 3)
    assert arrays["merged_total"][0] > 0


def _vivaldi_run(out, *extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "vivaldi",
                        "--members", "200000", "--steps", "7", "--warmup", "2", "--dump-outputs", str(out), *extra],
                       capture_output=True, text=True, cwd=ROOT, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["metric"] == "Vivaldi updates/s" and line["steps"] == 7 and line["ms_per_step"] > 0
    assert line["value"] * line["ms_per_step"] / 1e3 == pytest.approx(200000, rel=1e-9)
    return {f: np.load(out / f) for f in sorted(os.listdir(out))}


def test_vivaldi_long_run_in_segments_computes_the_same(tmp_path):
    """A run whose probe inputs do not fit HBM at once is timed in segments, the inputs of the
    next rounds generated between them: 2 + 7 rounds with 3 resident at a time (the timed rounds
    in segments of 3, 3 and 1, the input buffers reused) give bit for bit the coordinates of
    the same rounds with every input generated up front."""
    whole = _vivaldi_run(tmp_path / "whole")
    parts = _vivaldi_run(tmp_path / "parts", "--probe-rounds", "3")
    assert sorted(whole) == sorted(parts) == ["vivaldi_first_members.npy", "vivaldi_rows.npy"]
    assert whole["vivaldi_rows.npy"].dtype == np.float64 and np.all(np.isfinite(whole["vivaldi_rows.npy"]))
    for f in whole:
        assert np.array_equal(whole[f].view(np.uint64), parts[f].view(np.uint64)), f
