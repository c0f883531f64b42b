"""bench.py's plain run on the device: the headline alone, and --dump-outputs'
files against the oracle on the stripes the same seed gives this process.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_what_the_last_step_computed(gpu, oracle, tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` on a small
    ragged batch (RS(12,4), S = 87382, 37 stripes, fused digests): one line
    with K steps and their ms_per_step, no extras and no CPU baseline, and
    float32 files that hold the parity and the digests the oracle computes
    from the seeded stripes."""
    import torch
    k, m, n = 12, 4, 37
    S = -(-(1 << 20) // k)
    out = tmp_path / "dump"
    env = {x: v for x, v in os.environ.items() if x not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--warm-seconds", "0", "--k", str(k), "--m", str(m), "--batch", str(n), "--digests",
           "--dump-outputs", str(out)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "GiB/s" and line["dtype"] == "u8"
    assert line["value"] == pytest.approx(n * k * S / (line["ms_per_step"] * 1e-3) / bench.GiB, rel=1e-3)
    assert line["extras"] == {} and line["cpu_baseline"] is None

    plan = bench.dump_plan(k, m, S, n, True)
    assert sorted(os.listdir(out)) == sorted(name + ".npy" for name in plan)
    # the run's inputs again: the same seed on the same device
    st = bench.random_stripes(torch.device("cuda", 0), k, m, S, n, 1000)
    st[:, k:] = 0
    ref = st.cpu().numpy()
    for s in range(n):
        oracle.encode(k, m, ref[s])
    got = {name: np.load(out / (name + ".npy")) for name in plan}
    assert all(g.dtype == np.float32 for g in got.values())
    assert sum(g.nbytes for g in got.values()) <= 64 * 1000 * 1000
    rows, _ = plan["parity_stripes"]
    assert np.array_equal(got["parity_stripes"], ref[rows, k:].astype(np.float32))
    rows, cols = plan["parity_columns"]
    assert np.array_equal(got["parity_columns"], ref[rows, k:][:, :, cols].astype(np.float32))
    rows, _ = plan["digests"]
    assert got["digests"].shape == (len(rows), k + m, 32)
    for j, s in enumerate(rows):
        for i in range(k + m):
            assert got["digests"][j, i].astype(np.uint8).tobytes() == oracle.hh256s(ref[s, i]), (s, i)
