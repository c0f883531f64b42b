"""Measurements of the mixed-length batch deep scan (rsg_bitrot_verify_mixed_*).

(a) loopback set: N objects with seeded log-uniform sizes in 1 KiB - 1 MiB
    (the set tools/mixed_bench.py uses) written with put_objects into a
    LocalErasureSet of 1 MiB blocks in a temporary directory: one
    LocalErasureSet.verify_objects call against the loop of verify_object over
    the same files (one rsg_bitrot_verify_dev call per object, a file read and
    one H2D copy per shard file), alternated in one process after a warm-up;
    seconds as median of --reps with min/max, the ratio of the medians beside
    the loop's own run-to-run spread.  Both paths' statuses are compared (all
    files healthy).
(b) device-resident, HIP events: the 12 shard files of a uniform part (RS(8,4),
    1 MiB blocks, S = 131072, 4096 stripes) through
    rsg_bitrot_verify_mixed_dev and through rsg_bitrot_verify_dev on the same
    buffers, alternated; the event time spans the whole call (planning and the
    table copy included), the library's own kernel timing
    (rsg_set_kernel_timing) is recorded beside it.

Prints one JSON document (and writes it to --out).  bench.py is the project's
benchmark; this tool only records the numbers of profiles/r10/mixed_verify/.
"""
from __future__ import annotations

import argparse
import ctypes
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


def loopback_part(k: int, m: int, sizes, reps: int, datas, put_batch: int = 256) -> dict:
    from rustfs_amd.loopback import LocalErasureSet
    root = tempfile.mkdtemp(prefix="mixed_verify_bench_")
    try:
        dirs = [os.path.join(root, f"d{i}") for i in range(k + m)]
        for d in dirs:
            os.makedirs(d)
        s = LocalErasureSet(dirs, k, m, block_size=1 << 20)
        names = [f"o{j}" for j in range(len(sizes))]
        for j0 in range(0, len(names), put_batch):
            s.put_objects(list(zip(names[j0:j0 + put_batch], datas[j0:j0 + put_batch])))
        note(f"RS({k},{m}): {len(names)} objects written")
        healthy = [[0] * (k + m) for _ in names]
        file_bytes = sum(os.path.getsize(s.part_file(i, n)) for n in names for i in range(k + m))

        def loop():
            return [s.verify_object(n) for n in names]

        step = max(1, len(names) // 64)  # warm-up of both paths
        s.verify_objects(names[::step])
        for n in names[::step]:
            s.verify_object(n)
        t_many, t_loop, equal = [], [], True
        for r in range(reps):
            t0 = time.perf_counter()
            got = s.verify_objects(names)
            t_many.append(time.perf_counter() - t0)
            equal = equal and got == healthy
            t0 = time.perf_counter()
            got = loop()
            t_loop.append(time.perf_counter() - t0)
            equal = equal and got == healthy
            note(f"RS({k},{m}) rep {r}: verify_objects {t_many[-1]:.3f} s, verify_object loop {t_loop[-1]:.3f} s")
        s.close()

        def rates(ts):
            return {"seconds": summary(ts), "objects_per_s": summary([len(sizes) / t for t in ts]),
                    "file_gib_per_s": summary([file_bytes / t / GiB for t in ts])}
        return {"k": k, "m": m, "objects": len(sizes), "shard_files": len(sizes) * (k + m),
                "file_bytes": int(file_bytes), "all_files_healthy_both_paths": equal,
                "many": rates(t_many), "loop": rates(t_loop),
                "ratio_loop_over_many": statistics.median(t_loop) / statistics.median(t_many),
                "loop_spread_max_over_min": max(t_loop) / min(t_loop),
                "slowest_many_faster_than_fastest_loop": max(t_many) < min(t_loop)}
    finally:
        shutil.rmtree(root, ignore_errors=True)


def device_uniform(reps: int, n: int = 4096, S: int = 131072, k: int = 8, m: int = 4) -> dict:
    import torch
    from rustfs_amd import Erasure, _lib
    from rustfs_amd.bitrot import HashAlgorithm, bitrot_verify_batch, bitrot_verify_many
    e = Erasure(k, m, k * S)
    t = k + m
    st = torch.zeros((n, t, S), dtype=torch.uint8, device="cuda")
    st[:, :k] = torch.randint(0, 256, (n, k, S), dtype=torch.uint8, device="cuda")
    dig = torch.zeros((n, t, 32), dtype=torch.uint8, device="cuda")
    e.encode_batch(st, dig)
    files = [torch.cat([dig[:, i], st[:, i]], dim=1).contiguous().view(-1) for i in range(t)]
    del st
    rec = 32 + S
    desc = np.zeros(t, dtype=np.dtype(list(_lib.FILE_DESC_FIELDS)))
    desc["file_len"] = n * rec
    desc["want_size"] = n * rec
    desc["part_size"] = n * S
    desc["shard_size"] = S
    desc["arena"] = np.arange(t)
    algo = HashAlgorithm.HighwayHash256S
    mixed = lambda: bitrot_verify_many(files, desc, algo)  # noqa: E731
    part = lambda: bitrot_verify_batch(files, n * rec, n * S, algo, S)  # noqa: E731
    ok = mixed() == [0] * t and part() == [0] * t
    # one flipped byte: both calls must name the same file
    files[5][7 * rec + 40] ^= 1
    ok = ok and mixed() == part() == [11 if i == 5 else 0 for i in range(t)]
    files[5][7 * rec + 40] ^= 1
    event_ms(mixed, 2)
    event_ms(part, 2)
    ctx, lib = _lib.context(0).handle, _lib.load()
    kms = ctypes.c_float(-1.0)

    def kernel_ms(fn):
        fn()
        lib.rsg_last_kernel_ms(ctx, ctypes.byref(kms))
        return float(kms.value)
    ms_mixed, ms_part, k_mixed, k_part = [], [], [], []
    for _ in range(reps):
        ms_mixed += event_ms(mixed, 1)
        ms_part += event_ms(part, 1)
    lib.rsg_set_kernel_timing(ctx, 1)
    try:
        for _ in range(reps):
            k_mixed.append(kernel_ms(mixed))
            k_part.append(kernel_ms(part))
    finally:
        lib.rsg_set_kernel_timing(ctx, 0)
    alg = float(t * n * rec)  # every byte of every file read once
    gbs = lambda ms: summary([alg / (x * 1e-3) / 1e9 for x in ms])  # noqa: E731
    return {"k": k, "m": m, "stripes": n, "shard_size": S, "files": t, "algorithmic_bytes": int(alg),
            "statuses_agree": bool(ok), "mixed_ms": summary(ms_mixed), "per_part_ms": summary(ms_part),
            "mixed_gb_per_s": gbs(ms_mixed), "per_part_gb_per_s": gbs(ms_part),
            "mixed_kernel_ms": summary(k_mixed), "per_part_kernel_ms": summary(k_part),
            "mixed_over_per_part_median": statistics.median(ms_mixed) / statistics.median(ms_part),
            "mixed_over_per_part_kernel_median": statistics.median(k_mixed) / statistics.median(k_part),
            "per_part_spread_max_over_min": max(ms_part) / min(ms_part)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--geometries", default="8,4;12,4")
    ap.add_argument("--part", choices=["a", "b", "ab"], default="ab")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    geos = [tuple(int(x) for x in g.split(",")) for g in a.geometries.split(";")]
    doc = {"objects": a.objects, "size_range": [1 << 10, 1 << 20], "reps": a.reps}
    if "a" in a.part:
        sizes = sizes_for(a.objects)
        pool = np.random.default_rng(1).integers(0, 256, max(sizes) + 4096, dtype=np.uint8)
        datas = [pool[(37 * j) % 4096:(37 * j) % 4096 + s].tobytes() for j, s in enumerate(sizes)]
        for k, m in geos:
            doc.setdefault("loopback", []).append(loopback_part(k, m, sizes, a.reps, datas))
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
