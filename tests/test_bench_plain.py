"""bench.py's plain run and its --dump-outputs: the line carries the headline
fields and none of the --full legs, and the dumped words are the filter the
timed build computes (against the oracle's build of the same keys)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import keygen
import lsmbloom

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_timed_filter(oracle, tmp_path):
    n = 300_000  # many workgroups; the whole filter (44 847 words) fits the dump's sample
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--global-keys", str(n), "--dump-outputs", str(tmp_path / "dump"),
           "--detail-out", str(tmp_path / "detail.json")]
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["unit"] == "Mkeys/s" and out["higher_is_better"] is True
    # ms_per_step is rounded to 1e-4 ms; a step of this size takes well over 0.01 ms
    assert abs(out["value"] - n / (out["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * out["value"]
    for k in ("legs", "roofline", "cpu_baseline", "words_equal_oracle_fixture"):
        assert k not in out, k
    nb, k = lsmbloom.params(n, 0.01)
    ref = oracle.build_fixed(keygen.key16(bench.SEED_MEMBERS, 0, n), 16, nb, k)
    s = np.load(tmp_path / "dump" / "words_sample_u16.npy")
    pc = np.load(tmp_path / "dump" / "words_popcount.npy")
    assert s.shape == (ref.size, 5)
    q = s[:, :4].astype(np.uint64)
    assert np.array_equal(q[:, 0] | q[:, 1] << 16 | q[:, 2] << 32 | q[:, 3] << 48, ref)
    assert pc.sum(dtype=np.float64) == np.bitwise_count(ref).sum()
