"""Measurements of the mixed-length batch encode (rsg_encode_mixed_*).

(a) host path: N objects with seeded log-uniform sizes in 1 KiB - 1 MiB, one
    Erasure.encode_inline_shards_many call against the loop of
    Erasure.encode_inline_shards over the same objects (what there was before
    the mixed-length call), alternated in one process after a warm-up;
    objects/s and payload GiB/s as median of --reps with min/max, and the
    ratio of the medians beside the loop's own run-to-run spread.
(b) device-resident: one rsg_encode_mixed_dev over the same objects, HIP
    events, against algorithmic bytes sum((k+m)*S_j + 32*(k+m)); then a uniform
    batch (S = 131072, n = 4096, RS(8,4)) through the mixed kernel and through
    rsg_encode_batch_dev with RSG_FUSED_KIND=packed, alternated.

Prints one JSON document (and writes it to --out).  bench.py is the project's
benchmark; this tool only records the numbers of profiles/r07/mixed/.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

GiB = float(1 << 30)
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def sizes_for(n: int, seed: int = 2024):
    rng = np.random.default_rng(seed)
    return [int(x) for x in np.exp(rng.uniform(np.log(1 << 10), np.log(1 << 20), n))]


def host_part(k: int, m: int, sizes, reps: int) -> dict:
    from rustfs_amd import Erasure
    e = Erasure(k, m, 1 << 20)
    pool = np.random.default_rng(1).integers(0, 256, max(sizes) + 4096, dtype=np.uint8)
    datas = [pool[(37 * j) % 4096:(37 * j) % 4096 + s] for j, s in enumerate(sizes)]
    payload = float(sum(sizes))
    few = datas[:: max(1, len(datas) // 64)]
    many = e.encode_inline_shards_many(few)  # warm-up of both paths, and a spot check that they agree
    assert many == [e.encode_inline_shards(d) for d in few]
    e.encode_inline_shards_many(datas)
    t_many, t_loop = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        e.encode_inline_shards_many(datas)
        t_many.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for d in datas:
            e.encode_inline_shards(d)
        t_loop.append(time.perf_counter() - t0)

    def rates(ts):
        return {"seconds": summary(ts), "objects_per_s": summary([len(sizes) / t for t in ts]),
                "payload_gib_per_s": summary([payload / t / GiB for t in ts])}
    ml, mm = statistics.median(t_loop), statistics.median(t_many)
    return {"k": k, "m": m, "objects": len(sizes), "payload_bytes": int(payload), "many": rates(t_many),
            "loop": rates(t_loop), "ratio_loop_over_many": ml / mm,
            "loop_spread_max_over_min": max(t_loop) / min(t_loop),
            "many_beats_loop_beyond_spread": max(t_many) < min(t_loop)}


def event_ms(fn, reps: int):
    import torch
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def device_mixed(k: int, m: int, sizes, reps: int) -> dict:
    import torch
    from rustfs_amd import Erasure
    e = Erasure(k, m, 1 << 20)
    S = np.array([-(-s // k) for s in sizes], dtype=np.uint64)
    n, t = len(sizes), k + m
    desc = np.zeros((n, 3), dtype=np.uint64)
    desc[:, 2] = S
    desc[1:, 0] = np.cumsum(S[:-1] * np.uint64(k))
    desc[1:, 1] = np.cumsum(S[:-1] * np.uint64(m))
    total = int(S.sum())
    data = torch.randint(0, 256, (total * k,), dtype=torch.uint8, device="cuda")
    parity = torch.zeros(total * m, dtype=torch.uint8, device="cuda")
    dig = torch.zeros((n, t, 32), dtype=torch.uint8, device="cuda")
    run = lambda: e.encode_mixed(data, parity, desc, dig)  # noqa: E731
    event_ms(run, 3)
    ms = event_ms(run, reps)
    alg = float(total * t + 32 * t * n)
    return {"k": k, "m": m, "stripes": n, "algorithmic_bytes": int(alg), "ms": summary(ms),
            "gb_per_s": summary([alg / (x * 1e-3) / 1e9 for x in ms]),
            "hbm_fraction_median": alg / (statistics.median(ms) * 1e-3) / 1e9 / HBM_PEAK_GBS}


def device_uniform(reps: int, n: int = 4096, S: int = 131072, k: int = 8, m: int = 4) -> dict:
    import torch
    from rustfs_amd import Erasure, _lib
    e = Erasure(k, m, k * S)
    t = k + m
    st = torch.zeros((n, t, S), dtype=torch.uint8, device="cuda")
    st[:, :k] = torch.randint(0, 256, (n, k, S), dtype=torch.uint8, device="cuda")
    dig = torch.zeros((n, t, 32), dtype=torch.uint8, device="cuda")
    dig2 = torch.zeros_like(dig)
    flat = st.view(-1)
    desc = np.zeros((n, 3), dtype=np.uint64)
    desc[:, 0] = np.arange(n, dtype=np.uint64) * np.uint64(t * S)
    desc[:, 1] = desc[:, 0] + np.uint64(k * S)
    desc[:, 2] = S
    mixed = lambda: e.encode_mixed(flat, flat, desc, dig)  # noqa: E731
    packed = lambda: e.encode_batch(st, dig2)  # noqa: E731
    ms_mixed, ms_packed = [], []
    with _lib.tuned(RSG_FUSED_KIND="packed"):
        event_ms(mixed, 2)
        event_ms(packed, 2)
        torch.cuda.synchronize()
        same = bool(torch.equal(dig, dig2))
        for _ in range(reps):
            ms_mixed += event_ms(mixed, 1)
            ms_packed += event_ms(packed, 1)
    alg = float(n * t * S + 32 * t * n)
    gbs = lambda ms: summary([alg / (x * 1e-3) / 1e9 for x in ms])  # noqa: E731
    return {"k": k, "m": m, "stripes": n, "shard_len": S, "algorithmic_bytes": int(alg), "digests_equal": same,
            "mixed_ms": summary(ms_mixed), "packed_ms": summary(ms_packed), "mixed_gb_per_s": gbs(ms_mixed),
            "packed_gb_per_s": gbs(ms_packed),
            "mixed_over_packed_median": statistics.median(ms_mixed) / statistics.median(ms_packed),
            "packed_spread_max_over_min": max(ms_packed) / min(ms_packed)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--geometries", default="8,4;12,4")
    ap.add_argument("--part", choices=["a", "b", "ab"], default="ab")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    geos = [tuple(int(x) for x in g.split(",")) for g in a.geometries.split(";")]
    sizes = sizes_for(a.objects)
    doc = {"objects": a.objects, "size_range": [1 << 10, 1 << 20], "reps": a.reps}
    if "a" in a.part:
        doc["host"] = [host_part(k, m, sizes, a.reps) for k, m in geos]
    if "b" in a.part:
        doc["device_mixed"] = [device_mixed(k, m, sizes, a.reps) for k, m in geos]
        doc["device_uniform"] = device_uniform(a.reps)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
