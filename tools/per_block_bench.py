"""Per-block encode calls, the reference's call pattern (one
ReedSolomonEncoder::encode per 1 MiB block from many workers, encode.rs:504-530,
then BitrotWriter's hash of every shard): what tools/pcie_bench.py's
per_block_calls measures, extended to rsg_encode_hashed.

Shapes RS(8,4) and RS(12,4) 1 MiB blocks; layouts "pinned" (the block in
page-locked memory), "block" (shards back to back in one pageable buffer) and
"separate" (one pageable buffer per shard); with and without HH256S; 1, 8 and
16 callers.  Every point is warmed, then timed over windows of --window
seconds (default 2), --repeats times (default 5); reported per window: median
and p99 us per call and the aggregate GiB/s of payload (k * S bytes per call).

--baseline uses only entries every earlier library has (rsg_encode, and k+m
rsg_hash calls for the hashed variant), so it also runs against another
build: --lib PATH.  --cpu records the CPU oracle's
rate over --threads threads instead (oracle.encode_batch_mt, as bench.py's
cpu_baseline).  One JSON line per point on stdout."""
import argparse
import ctypes
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

GiB = float(1 << 30)
HH = 1


def load(path):
    import torch  # noqa: F401  (one HIP runtime in the process, see rustfs_amd/_lib.py)
    L = ctypes.CDLL(path)
    P, I, S = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    L.rsg_create.argtypes = [I, ctypes.POINTER(P)]
    L.rsg_destroy.argtypes = [P]
    L.rsg_destroy.restype = None
    L.rsg_encode.argtypes = [P, I, I, S, P]
    L.rsg_hash.argtypes = [P, I, P, S, P]
    if hasattr(L, "rsg_encode_hashed"):
        L.rsg_encode_hashed.argtypes = [P, I, I, S, P, P, I]
    return L


class Caller:
    """One worker's block and the call it repeats."""

    def __init__(self, L, ctx, k, m, S, layout, hashed, baseline, seed):
        import torch
        t = k + m
        rng = np.random.default_rng(seed)
        if layout == "separate":
            self.sh = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)] + [np.zeros(S, np.uint8) for _ in range(m)]
        else:
            blk = (torch.zeros(t * S, dtype=torch.uint8).pin_memory().numpy() if layout == "pinned"
                   else np.zeros(t * S, np.uint8)).reshape(t, S)
            blk[:k] = rng.integers(0, 256, (k, S), dtype=np.uint8)
            self.sh = [blk[i] for i in range(t)]
        self.dig = (torch.zeros(t * 32, dtype=torch.uint8).pin_memory().numpy() if layout == "pinned"
                    else np.zeros(t * 32, np.uint8))
        self.ptrs = (ctypes.c_void_p * t)(*[a.ctypes.data for a in self.sh])
        self.L, self.ctx, self.k, self.m, self.S, self.hashed, self.baseline = L, ctx, k, m, S, hashed, baseline

    def call(self):
        L, k, m, S = self.L, self.k, self.m, self.S
        if not self.hashed:
            st = L.rsg_encode(self.ctx, k, m, S, self.ptrs)
        elif self.baseline:
            st = L.rsg_encode(self.ctx, k, m, S, self.ptrs)
            for i in range(k + m):
                st = st or L.rsg_hash(self.ctx, HH, self.ptrs[i], S, self.dig.ctypes.data + 32 * i)
        else:
            st = L.rsg_encode_hashed(self.ctx, k, m, S, self.ptrs, self.dig.ctypes.data, HH)
        if st:
            raise RuntimeError(f"status {st}")


def window(callers, seconds):
    """All callers call for `seconds`; per-call latencies and the aggregate rate."""
    lat = [[] for _ in callers]
    start = threading.Barrier(len(callers) + 1)
    stop = [False]
    errors = []

    def work(i):
        c = callers[i]
        start.wait()
        try:
            while not stop[0]:
                t0 = time.perf_counter()
                c.call()
                lat[i].append(time.perf_counter() - t0)
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(len(callers))]
    for t in th:
        t.start()
    start.wait()
    t0 = time.perf_counter()
    time.sleep(seconds)
    stop[0] = True
    for t in th:
        t.join()
    el = time.perf_counter() - t0
    if errors:
        raise errors[0]
    flat = sorted(x for l in lat for x in l)
    c = callers[0]
    return {"calls": len(flat), "median_us": round(flat[len(flat) // 2] * 1e6, 1),
            "p99_us": round(flat[min(len(flat) - 1, int(len(flat) * 0.99))] * 1e6, 1),
            "GiB_s": round(len(flat) * c.k * c.S / el / GiB, 2)}


def cpu_rate(k, m, S, threads, hashed, seconds, repeats):
    from oracle import oracle as O
    n = 256
    st = np.zeros((n, k + m, S), np.uint8)
    st[:, :k] = np.random.default_rng(0).integers(0, 256, (n, k, S), dtype=np.uint8)
    dig = np.zeros((n, k + m, 32), np.uint8) if hashed else None
    O.encode_batch_mt(k, m, S, st, dig, threads)
    out = []
    for _ in range(repeats):
        t0, reps = time.perf_counter(), 0
        while time.perf_counter() - t0 < seconds:
            O.encode_batch_mt(k, m, S, st, dig, threads)
            reps += 1
        out.append(round(reps * n * k * S / (time.perf_counter() - t0) / GiB, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "rustfs_amd", "librsgpu.so"))
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--shapes", default="8,4 12,4")
    ap.add_argument("--layouts", default="pinned block separate")
    ap.add_argument("--callers", default="1 8 16")
    ap.add_argument("--hashed", default="0 1")
    ap.add_argument("--window", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--block", type=int, default=1 << 20)
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(",")) for s in a.shapes.split()]
    if a.cpu:
        for k, m in shapes:
            S = -(-a.block // k)
            for hashed in (int(h) for h in a.hashed.split()):
                print(json.dumps({"cpu_oracle": True, "k": k, "m": m, "S": S, "threads": a.threads, "hashed": hashed,
                                  "GiB_s": cpu_rate(k, m, S, a.threads, bool(hashed), a.window, a.repeats)}), flush=True)
        return
    L = load(a.lib)
    ctx = ctypes.c_void_p()
    assert L.rsg_create(0, ctypes.byref(ctx)) == 0
    for k, m in shapes:
        S = -(-a.block // k)
        for layout in a.layouts.split():
            for hashed in (int(h) for h in a.hashed.split()):
                for nc in (int(c) for c in a.callers.split()):
                    callers = [Caller(L, ctx, k, m, S, layout, bool(hashed), a.baseline, seed=i) for i in range(nc)]
                    window(callers, min(0.3, a.window))  # warm
                    res = [window(callers, a.window) for _ in range(a.repeats)]
                    print(json.dumps({"baseline": a.baseline, "k": k, "m": m, "S": S, "layout": layout, "hashed": hashed,
                                      "callers": nc, "window_s": a.window, "windows": res}), flush=True)
    L.rsg_destroy(ctx)


if __name__ == "__main__":
    main()
