"""Measurements of the mixed-length batch GET (rsg_decode_mixed_*).

(a) host path: N objects with seeded log-uniform sizes in 1 KiB - 1 MiB (the
    set tools/mixed_bench.py uses), healthy and with one data disk absent: one
    Erasure.decode_inline_shards_many call against the per-object loop there
    was before it (hash_encode per shard for verify-before-use, then
    decode_data_with_reconstruction_verification: the short-block code of
    pipeline.get_stream), alternated in one process after a warm-up; seconds as
    median of --reps with min/max, the ratio of the medians beside the loop's
    own run-to-run spread.
(b) device-resident, HIP events: the same batch in one rsg_decode_mixed_dev
    against algorithmic bytes (records read plus shards written); then a
    uniform batch (RS(8,4), S = 131072, n = 4096, two data shards absent)
    through the mixed kernel and through rsg_decode_records_into_dev on the
    same records, alternated, outputs compared.

Prints one JSON document (and writes it to --out).  bench.py is the project's
benchmark; this tool only records the numbers of profiles/r07/mixed_get/.
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

from tools.mixed_bench import event_ms, sizes_for, summary  # noqa: E402

GiB = float(1 << 30)
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec


def note(msg: str) -> None:
    print(msg, file=sys.stderr, flush=True)


def loop_get(e, algo, objs, sizes):
    """The per-object GET there was before the batched call."""
    k = e.data_shards
    out = []
    for shards, size in zip(objs, sizes):
        got = [None if r is None or algo.hash_encode(r[32:]) != r[:32] else r[32:] for r in shards]
        e.decode_data_with_reconstruction_verification(got)
        out.append(b"".join(bytes(got[i]) for i in range(k))[:size])
    return out


def host_part(k: int, m: int, sizes, reps: int, objs, datas) -> list:
    from rustfs_amd import Erasure
    from rustfs_amd.bitrot import HashAlgorithm
    e = Erasure(k, m, 1 << 20)
    algo = HashAlgorithm.HighwayHash256S
    payload = float(sum(sizes))
    res = []
    for name, lose in (("healthy", None), ("one data disk absent", 1)):
        cur = [[None if i == lose else r for i, r in enumerate(o)] for o in objs]
        step = max(1, len(cur) // 64)  # warm-up of both paths, and a spot check against the bodies
        assert e.decode_inline_shards_many(cur[::step], sizes[::step]) == datas[::step]
        assert loop_get(e, algo, cur[::step], sizes[::step]) == datas[::step]
        assert e.decode_inline_shards_many(cur, sizes) == datas
        t_many, t_loop = [], []
        for r in range(reps):
            t0 = time.perf_counter()
            e.decode_inline_shards_many(cur, sizes)
            t_many.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            loop_get(e, algo, cur, sizes)
            t_loop.append(time.perf_counter() - t0)
            note(f"host RS({k},{m}) {name} rep {r}: many {t_many[-1]:.3f} s, loop {t_loop[-1]:.3f} s")

        def rates(ts):
            return {"seconds": summary(ts), "objects_per_s": summary([len(sizes) / t for t in ts]),
                    "payload_gib_per_s": summary([payload / t / GiB for t in ts])}
        res.append({"k": k, "m": m, "case": name, "objects": len(sizes), "payload_bytes": int(payload),
                    "many": rates(t_many), "loop": rates(t_loop),
                    "ratio_loop_over_many": statistics.median(t_loop) / statistics.median(t_many),
                    "loop_spread_max_over_min": max(t_loop) / min(t_loop),
                    "slowest_many_faster_than_fastest_loop": max(t_many) < min(t_loop)})
    return res


def device_mixed(k: int, m: int, sizes, reps: int, objs) -> list:
    import torch
    from rustfs_amd import Erasure, _lib
    e = Erasure(k, m, 1 << 20)
    t, n = k + m, len(sizes)
    S = np.array([-(-s // k) for s in sizes], dtype=np.uint64)
    desc = np.zeros(n, dtype=np.dtype(list(_lib.RECORD_DESC_FIELDS)))
    desc["shard_len"] = S
    desc["rec_off"][1:] = np.cumsum(S[:-1] + np.uint64(32))
    desc["out_off"][1:] = np.cumsum(S[:-1] * np.uint64(k))
    files = [torch.from_numpy(np.frombuffer(b"".join(o[i] for o in objs), dtype=np.uint8).copy()).cuda()
             for i in range(t)]
    out = torch.zeros(int(S.sum()) * k, dtype=torch.uint8, device="cuda")
    total = int(S.sum())
    res = []
    for name, gone in (("healthy", ()), ("one data disk absent", (1,))):
        desc["present"] = ((1 << t) - 1) & ~sum(1 << i for i in gone)
        run = lambda: e.decode_mixed(files, desc, out)  # noqa: E731
        status, _ = run()
        assert not any(status)
        event_ms(run, 2)
        ms = event_ms(run, reps)
        read = k if not gone else t - len(gone)  # records read per stripe (sources + surplus)
        alg = float(read * (total + 32 * n) + len(gone) * total)
        res.append({"k": k, "m": m, "case": name, "stripes": n, "algorithmic_bytes": int(alg), "ms": summary(ms),
                    "gb_per_s": summary([alg / (x * 1e-3) / 1e9 for x in ms]),
                    "hbm_fraction_median": alg / (statistics.median(ms) * 1e-3) / 1e9 / HBM_PEAK_GBS})
    return res


def device_uniform(reps: int, n: int = 4096, S: int = 131072, k: int = 8, m: int = 4, gone=(0, 1)) -> dict:
    import torch
    from rustfs_amd import Erasure, _lib
    e = Erasure(k, m, k * S)
    t = k + m
    st = torch.zeros((n, t, S), dtype=torch.uint8, device="cuda")
    st[:, :k] = torch.randint(0, 256, (n, k, S), dtype=torch.uint8, device="cuda")
    dig = torch.zeros((n, t, 32), dtype=torch.uint8, device="cuda")
    e.encode_batch(st, dig)
    files = [torch.cat([dig[:, i], st[:, i]], dim=1).contiguous().view(-1) for i in range(t)]
    want = st[:, list(gone)].clone()
    del st
    desc = np.zeros(n, dtype=np.dtype(list(_lib.RECORD_DESC_FIELDS)))
    desc["shard_len"] = S
    desc["rec_off"] = np.arange(n, dtype=np.uint64) * np.uint64(32 + S)
    desc["out_off"] = np.arange(n, dtype=np.uint64) * np.uint64(k * S)
    desc["present"] = ((1 << t) - 1) & ~sum(1 << i for i in gone)
    out = torch.zeros((n, k * S), dtype=torch.uint8, device="cuda")
    slots = torch.zeros((n, k * S), dtype=torch.uint8, device="cuda")
    engine_files = [None if i in gone else f for i, f in enumerate(files)]
    mixed = lambda: e.decode_mixed(files, desc, out.view(-1))  # noqa: E731
    engine = lambda: e.decode_records_into_batch(engine_files, S, n, targets=slots)  # noqa: E731
    event_ms(mixed, 2)
    event_ms(engine, 2)
    torch.cuda.synchronize()
    same = all(bool(torch.equal(out[:, c * S:(c + 1) * S], slots[:, c * S:(c + 1) * S]) and
                    torch.equal(out[:, c * S:(c + 1) * S], want[:, j])) for j, c in enumerate(gone))
    ms_mixed, ms_engine = [], []
    for _ in range(reps):
        ms_mixed += event_ms(mixed, 1)
        ms_engine += event_ms(engine, 1)
    alg = float(n * ((t - len(gone)) * (32 + S) + len(gone) * S))
    gbs = lambda ms: summary([alg / (x * 1e-3) / 1e9 for x in ms])  # noqa: E731
    return {"k": k, "m": m, "stripes": n, "shard_len": S, "absent": list(gone), "algorithmic_bytes": int(alg),
            "outputs_equal": same, "mixed_ms": summary(ms_mixed), "engine_ms": summary(ms_engine),
            "mixed_gb_per_s": gbs(ms_mixed), "engine_gb_per_s": gbs(ms_engine),
            "mixed_over_engine_median": statistics.median(ms_mixed) / statistics.median(ms_engine),
            "engine_spread_max_over_min": max(ms_engine) / min(ms_engine)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--geometries", default="8,4;12,4")
    ap.add_argument("--part", choices=["a", "b", "ab"], default="ab")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    from rustfs_amd import Erasure
    geos = [tuple(int(x) for x in g.split(",")) for g in a.geometries.split(";")]
    sizes = sizes_for(a.objects)
    pool = np.random.default_rng(1).integers(0, 256, max(sizes) + 4096, dtype=np.uint8)
    datas = [pool[(37 * j) % 4096:(37 * j) % 4096 + s].tobytes() for j, s in enumerate(sizes)]
    doc = {"objects": a.objects, "size_range": [1 << 10, 1 << 20], "reps": a.reps}
    for k, m in geos:
        objs = Erasure(k, m, 1 << 20).encode_inline_shards_many(datas)
        note(f"RS({k},{m}): {len(objs)} objects encoded")
        if "a" in a.part:
            doc.setdefault("host", []).extend(host_part(k, m, sizes, a.reps, objs, datas))
        if "b" in a.part:
            doc.setdefault("device_mixed", []).extend(device_mixed(k, m, sizes, a.reps, objs))
    if "b" in a.part:
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
