"""Per-block degraded reads, the reference's call pattern (BitrotReader::read
hashes each shard it reads, bitrot.rs:139-244, then one
ReedSolomonEncoder::reconstruct_data per 1 MiB block, erasure.rs:411-422, from
many workers), against rsg_reconstruct_blocks: tools/per_block_bench.py's
measurement for the read half of the seam.

Shapes RS(8,4) and RS(12,4), 1 MiB blocks with data shards 0 and 1 lost, mode
RSG_RECONSTRUCT_DATA; layouts "pinned" (the block in page-locked memory) and
"pageable" (shards back to back in one pageable buffer); with and without
HH256S verification; n = 1, 16 and 64 blocks per call; 1, 8 and 16 callers.
Every point is warmed, then timed over windows of --window seconds (default
2), --repeats times (default 5); reported per window: median and p99 us per
call, the median us per block, and the aggregate GiB/s of payload (k * S bytes
per block).

--baseline uses only entries every earlier library has: per block one
rsg_reconstruct, and for the verified form one rsg_hash per survivor with the
digest compared on the host first; so it also runs against another build:
--lib PATH.  (Its cost per block does not depend on n: --blocks 1 suffices.)
One JSON line per point on stdout."""
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
HH, NONE, DATA = 1, 0, 0
LOST = (0, 1)


class rsg_rblock(ctypes.Structure):
    _fields_ = [("shards", ctypes.POINTER(ctypes.c_void_p)), ("shard_len", ctypes.c_uint64), ("present", ctypes.c_void_p),
                ("digests", ctypes.c_void_p), ("bad", ctypes.c_void_p)]


def load(path):
    import torch  # noqa: F401  (one HIP runtime in the process, see rustfs_amd/_lib.py)
    L = ctypes.CDLL(path)
    P, I, S = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    L.rsg_create.argtypes = [I, ctypes.POINTER(P)]
    L.rsg_destroy.argtypes = [P]
    L.rsg_destroy.restype = None
    L.rsg_reconstruct.argtypes = [P, I, I, S, P, P, I]
    L.rsg_hash.argtypes = [P, I, P, S, P]
    if hasattr(L, "rsg_reconstruct_blocks"):
        L.rsg_reconstruct_blocks.argtypes = [P, I, I, S, P, I, I, P]
    return L


def template(k, m, S):
    """One encoded block and its shards' HH256S digests (every block of a run
    holds the same bytes: the time does not depend on them)."""
    from oracle import oracle as O
    st = np.zeros((k + m, S), np.uint8)
    st[:k] = np.random.default_rng(0).integers(0, 256, (k, S), dtype=np.uint8)
    O.encode(k, m, st)
    return st, np.frombuffer(b"".join(O.hh256s(st[i]) for i in range(k + m)), dtype=np.uint8).copy()


class Caller:
    """One worker's n degraded blocks and the call it repeats."""

    def __init__(self, L, ctx, k, m, S, layout, verified, baseline, n, tmpl):
        import torch
        t = k + m
        st, dig = tmpl
        buf = (torch.zeros(n * t * S, dtype=torch.uint8).pin_memory().numpy() if layout == "pinned"
               else np.zeros(n * t * S, np.uint8)).reshape(n, t, S)
        buf[:] = st
        buf[:, list(LOST)] = 0
        self.buf, self.dig = buf, dig
        self.present = np.array([s not in LOST for s in range(t)], dtype=np.uint8)
        self.bad = np.zeros((n, t), np.uint8)
        self.status = (ctypes.c_int * n)()
        self.ptrs = [(ctypes.c_void_p * t)(*[buf[i, s].ctypes.data for s in range(t)]) for i in range(n)]
        self.descs = (rsg_rblock * n)()
        for i in range(n):
            self.descs[i] = rsg_rblock(ctypes.cast(self.ptrs[i], ctypes.POINTER(ctypes.c_void_p)), S, self.present.ctypes.data,
                                       dig.ctypes.data if verified else None, self.bad[i].ctypes.data)
        self.out = np.zeros(32, np.uint8)
        self.survivors = [s for s in range(t) if s not in LOST][:k]
        self.L, self.ctx, self.k, self.m, self.S, self.n = L, ctx, k, m, S, n
        self.verified, self.baseline = verified, baseline

    def call(self):
        L, k, m, S = self.L, self.k, self.m, self.S
        if not self.baseline:
            st = L.rsg_reconstruct_blocks(self.ctx, k, m, self.n, self.descs, DATA, HH if self.verified else NONE, self.status)
            if st or any(self.status):
                raise RuntimeError(f"status {st} {list(self.status)}")
            return
        for i in range(self.n):
            if self.verified:
                for s in self.survivors:
                    st = L.rsg_hash(self.ctx, HH, self.ptrs[i][s], S, self.out.ctypes.data)
                    if st or self.out.tobytes() != self.dig[32 * s: 32 * s + 32].tobytes():
                        raise RuntimeError(f"hash: status {st} or mismatch")
            st = L.rsg_reconstruct(self.ctx, k, m, S, self.ptrs[i], self.present.ctypes.data, DATA)
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
    med = flat[len(flat) // 2] * 1e6
    return {"calls": len(flat), "median_us": round(med, 1), "us_per_block": round(med / c.n, 1),
            "p99_us": round(flat[min(len(flat) - 1, int(len(flat) * 0.99))] * 1e6, 1),
            "GiB_s": round(len(flat) * c.n * c.k * c.S / el / GiB, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "rustfs_amd", "librsgpu.so"))
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--shapes", default="8,4 12,4")
    ap.add_argument("--layouts", default="pinned pageable")
    ap.add_argument("--callers", default="1 8 16")
    ap.add_argument("--blocks", default="1 16 64")
    ap.add_argument("--verified", default="0 1")
    ap.add_argument("--window", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--block", type=int, default=1 << 20)
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(",")) for s in a.shapes.split()]
    L = load(a.lib)
    ctx = ctypes.c_void_p()
    assert L.rsg_create(0, ctypes.byref(ctx)) == 0
    for k, m in shapes:
        S = -(-a.block // k)
        tmpl = template(k, m, S)
        for layout in a.layouts.split():
            for verified in (int(h) for h in a.verified.split()):
                for n in (int(b) for b in a.blocks.split()):
                    for nc in (int(c) for c in a.callers.split()):
                        callers = [Caller(L, ctx, k, m, S, layout, bool(verified), a.baseline, n, tmpl) for _ in range(nc)]
                        window(callers, min(0.3, a.window))  # warm
                        res = [window(callers, a.window) for _ in range(a.repeats)]
                        print(json.dumps({"baseline": a.baseline, "k": k, "m": m, "S": S, "layout": layout,
                                          "verified": verified, "blocks": n, "callers": nc, "window_s": a.window,
                                          "windows": res}), flush=True)
                        del callers
    L.rsg_destroy(ctx)


if __name__ == "__main__":
    main()
