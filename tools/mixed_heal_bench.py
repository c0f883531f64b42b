"""Measurements of the mixed-length batch heal (rsg_heal_mixed_*).

(a) loopback set: N objects with seeded log-uniform sizes in 1 KiB - 1 MiB
    (the set tools/mixed_bench.py uses) written with put_objects into a
    LocalErasureSet of 1 MiB blocks in a temporary directory, one data disk
    the heal target: one LocalErasureSet.heal_objects call against the loop
    of heal_object over the same files (full blocks through
    rsg_heal_records_dev, the short block verified, decoded and hashed on the
    host), alternated in one process after a warm-up; seconds as median of
    --reps with min/max, the ratio of the medians beside the loop's own
    run-to-run spread.  The target's part files are compared with what PUT
    wrote after each path.
(b) device-resident, HIP events: a uniform batch (RS(8,4), S = 131072,
    n = 4096, data shard 1 the target) through rsg_heal_mixed_dev and through
    rsg_heal_records_dev on the same records, alternated, target records
    compared.

Prints one JSON document (and writes it to --out).  bench.py is the project's
benchmark; this tool only records the numbers of profiles/r09/mixed_heal/.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tools.mixed_bench import event_ms, sizes_for, summary  # noqa: E402

GiB = float(1 << 30)


def note(msg: str) -> None:
    print(msg, file=sys.stderr, flush=True)


def loopback_part(k: int, m: int, sizes, reps: int, datas, target: int, put_batch: int = 256) -> dict:
    from rustfs_amd.loopback import LocalErasureSet
    root = tempfile.mkdtemp(prefix="mixed_heal_bench_")
    try:
        dirs = [os.path.join(root, f"d{i}") for i in range(k + m)]
        for d in dirs:
            os.makedirs(d)
        s = LocalErasureSet(dirs, k, m, block_size=1 << 20)
        names = [f"o{j}" for j in range(len(sizes))]
        for j0 in range(0, len(names), put_batch):
            s.put_objects(list(zip(names[j0:j0 + put_batch], datas[j0:j0 + put_batch])))
        note(f"RS({k},{m}): {len(names)} objects written")
        paths = [s.part_file(target, n) for n in names]
        wrote = [open(p, "rb").read() for p in paths]

        def same():
            return all(open(p, "rb").read() == w for p, w in zip(paths, wrote))

        def loop():
            for n in names:
                s.heal_object(n, [target])

        step = max(1, len(names) // 64)  # warm-up of both paths
        s.heal_objects(names[::step], [target])
        for n in names[::step]:
            s.heal_object(n, [target])
        t_many, t_loop, equal = [], [], True
        for r in range(reps):
            t0 = time.perf_counter()
            s.heal_objects(names, [target])
            t_many.append(time.perf_counter() - t0)
            equal = equal and same()
            t0 = time.perf_counter()
            loop()
            t_loop.append(time.perf_counter() - t0)
            equal = equal and same()
            note(f"RS({k},{m}) rep {r}: heal_objects {t_many[-1]:.3f} s, heal_object loop {t_loop[-1]:.3f} s")
        s.close()
        payload = float(sum(sizes))

        def rates(ts):
            return {"seconds": summary(ts), "objects_per_s": summary([len(sizes) / t for t in ts]),
                    "payload_gib_per_s": summary([payload / t / GiB for t in ts])}
        return {"k": k, "m": m, "target_disk": target, "objects": len(sizes), "payload_bytes": int(payload),
                "healed_files_equal_put": equal, "many": rates(t_many), "loop": rates(t_loop),
                "ratio_loop_over_many": statistics.median(t_loop) / statistics.median(t_many),
                "loop_spread_max_over_min": max(t_loop) / min(t_loop),
                "slowest_many_faster_than_fastest_loop": max(t_many) < min(t_loop)}
    finally:
        shutil.rmtree(root, ignore_errors=True)


def device_uniform(reps: int, n: int = 4096, S: int = 131072, k: int = 8, m: int = 4, target: int = 1) -> dict:
    import torch
    from rustfs_amd import Erasure, _lib
    e = Erasure(k, m, k * S)
    t = k + m
    st = torch.zeros((n, t, S), dtype=torch.uint8, device="cuda")
    st[:, :k] = torch.randint(0, 256, (n, k, S), dtype=torch.uint8, device="cuda")
    dig = torch.zeros((n, t, 32), dtype=torch.uint8, device="cuda")
    e.encode_batch(st, dig)
    files = [torch.cat([dig[:, i], st[:, i]], dim=1).contiguous().view(-1) for i in range(t)]
    del st
    want = files[target]
    src = [None if i == target else f for i, f in enumerate(files)]
    desc = np.zeros(n, dtype=np.dtype(list(_lib.RECORD_DESC_FIELDS)))
    desc["shard_len"] = S
    desc["rec_off"] = np.arange(n, dtype=np.uint64) * np.uint64(32 + S)
    desc["out_off"] = desc["rec_off"]
    desc["present"] = ((1 << t) - 1) & ~(1 << target)
    out_mixed = torch.zeros(n * (32 + S), dtype=torch.uint8, device="cuda")
    out_engine = torch.zeros(n * (32 + S), dtype=torch.uint8, device="cuda")
    tg_mixed = [out_mixed if i == target else None for i in range(t)]
    tg_engine = [out_engine if i == target else None for i in range(t)]
    mixed = lambda: e.heal_mixed(src, tg_mixed, desc)  # noqa: E731
    engine = lambda: e.heal_records_batch(src, tg_engine, S, n)  # noqa: E731
    assert not any(mixed())
    event_ms(mixed, 2)
    event_ms(engine, 2)
    torch.cuda.synchronize()
    same = bool(torch.equal(out_mixed, want)) and bool(torch.equal(out_engine, want))
    ms_mixed, ms_engine = [], []
    for _ in range(reps):
        ms_mixed += event_ms(mixed, 1)
        ms_engine += event_ms(engine, 1)
    alg = float(n * ((t - 1) * (32 + S) + 32 + S))  # every other record read, the target's written
    gbs = lambda ms: summary([alg / (x * 1e-3) / 1e9 for x in ms])  # noqa: E731
    return {"k": k, "m": m, "stripes": n, "shard_len": S, "target": target, "algorithmic_bytes": int(alg),
            "targets_equal_encode": same, "mixed_ms": summary(ms_mixed), "engine_ms": summary(ms_engine),
            "mixed_gb_per_s": gbs(ms_mixed), "engine_gb_per_s": gbs(ms_engine),
            "mixed_over_engine_median": statistics.median(ms_mixed) / statistics.median(ms_engine),
            "engine_spread_max_over_min": max(ms_engine) / min(ms_engine)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--geometries", default="8,4;12,4")
    ap.add_argument("--target", type=int, default=1)
    ap.add_argument("--part", choices=["a", "b", "ab"], default="ab")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    geos = [tuple(int(x) for x in g.split(",")) for g in a.geometries.split(";")]
    sizes = sizes_for(a.objects)
    pool = np.random.default_rng(1).integers(0, 256, max(sizes) + 4096, dtype=np.uint8)
    datas = [pool[(37 * j) % 4096:(37 * j) % 4096 + s].tobytes() for j, s in enumerate(sizes)]
    doc = {"objects": a.objects, "size_range": [1 << 10, 1 << 20], "reps": a.reps}
    if "a" in a.part:
        for k, m in geos:
            doc.setdefault("loopback", []).append(loopback_part(k, m, sizes, a.reps, datas, a.target))
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
