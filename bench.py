"""Benchmark of the erasure hot path (BASELINE.json metric).

Default workload = BASELINE configs[1]: RS(k=8,m=4) encode of device-resident
1 MiB stripes (S = 131072 B per shard), batch 4096 per GPU.  One step = one
encode pass over the whole batch (one rsg_encode_batch_dev call).  value =
payload (data) GiB/s over all ranks, the reference benches' convention
(crates/ecstore/benches/erasure_benchmark.rs:112 Throughput::Bytes(data_size)).

Multi-GPU: one process per GPU, independent stripes, no data-path collective
("scaling": "weak"); a gloo barrier brackets the timed region and the elapsed
time is the max over ranks.  `python bench.py --gpus N` starts the N rank
processes itself (before anything touches the GPU) and relays rank 0's line;
under torch.distributed.run the ranks come from the environment and must
number exactly --gpus.  Ranks never share a device unless
--allow-shared-device (a rehearsal on a smaller box) says so.

A plain run does what the headline needs and no more: set up, warm up, time
the K steps, write the outputs if --dump-outputs is given, print the line
(extras empty, no CPU baseline).

With --full the line's extras also time, in the same process:
config 3 (reconstruct with 1-4 lost data shards), config 4 (RS(8,4) encode +
fused HighwayHash-256 digests, the PUT path's kernel, encode.rs:601-628),
config 5's per-GPU share (RS(16,4) encode, S = 65536, 8192 stripes) and the
GET / heal / bitrot_verify engines — each with its kernel time, algorithmic
bytes and roofline fraction — then the RS(12,4) and host-memory extras and the
CPU baseline (the --no-* options trim a --full run).

--dump-outputs DIR writes what the last timed step computed, as float32 .npy
files (dump_outputs): the stripes are seeded, so two builds run with the same
arguments can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

GiB = float(1 << 30)
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec, /opt/skills/guides/MI355X_MICROARCH.md


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    # --data-shards / --parity-shards: the same as --k / --m, for launches
    # through torch.distributed.run, whose parser takes "--m" for its own
    # options (ambiguous abbreviation)
    ap.add_argument("--k", "--data-shards", dest="k", type=int, default=8)
    ap.add_argument("--m", "--parity-shards", dest="m", type=int, default=4)
    ap.add_argument("--stripe-bytes", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=4096, help="stripes per GPU (weak scaling)")
    ap.add_argument("--total-batch", type=int, default=0,
                    help="stripes over ALL GPUs, split evenly (strong scaling, BASELINE config 5)")
    ap.add_argument("--digests", action="store_true", help="fused HH256S digests (config 4)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline also measure the extras (reconstruct, config 4 / 5, engines, RS(12,4), "
                         "host path) and the CPU baseline; off: the headline alone")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32, a seeded sample, "
                         "under 64 MB in all; rank 0's share)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample-stripes", type=int, default=256)
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="CPU baseline threads (default: every CPU this process may use: affinity and cgroup quota)")
    ap.add_argument("--no-extras", action="store_true", help="skip the reconstruct / GET / heal measurements")
    ap.add_argument("--no-engines", action="store_true", help="skip the GET / heal / bitrot_verify measurements")
    ap.add_argument("--warm-seconds", type=float, default=0.5,
                    help="keep warming (untimed) until the device has been busy this long (clock ramp)")
    ap.add_argument("--allow-shared-device", action="store_true",
                    help="rehearsal only: let ranks share GPUs when fewer are visible than ranks")
    ap.add_argument("--no-config-extras", action="store_true",
                    help="skip the config 4 (fused digests) and config 5 (RS(16,4)) encode extras")
    ap.add_argument("--config4-batch", type=int, default=4096, help="config 4 extra: stripes per GPU")
    ap.add_argument("--config5-total", type=int, default=32768,
                    help="config 5 extra: RS(16,4) stripes split over all GPUs (one GPU: its 1/8 share)")
    ap.add_argument("--no-rs12", action="store_true", help="skip the RS(12,4) (16-drive default) extras")
    ap.add_argument("--rs12-batch", type=int, default=4096, help="RS(12,4) extras: stripes")
    ap.add_argument("--no-host-path", action="store_true",
                    help="skip extras.host_path (host memory at both ends: pinned copies, host-batch encode, "
                         "streamed GET / PUT)")
    ap.add_argument("--host-path-blocks", type=int, default=1024, help="extras.host_path: 1 MiB blocks per call")
    ap.add_argument("--record-engine", choices=["auto", "one-pass", "two-pass"], default="auto",
                    help="GET/heal engine path for the engine extras (rsg_set_record_engine)")
    return ap.parse_args(argv)


def free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(a, argv, script=None, devices=None) -> int:
    """`bench.py --gpus N` without a launcher: start N rank processes of this
    script (rank r on device r), relay rank 0's JSON line, return the first
    failing rank's exit code.  Nothing here touches the GPU: counting devices
    with torch.cuda.device_count() does not initialise it on this image, and
    the ranks are fresh child processes, not an exec of this one.  (`script`
    and `devices` let the CPU tests drive the launcher with a stand-in rank.)"""
    import subprocess
    from rustfs_amd.dispatch import check_world, rank_plan
    if devices is None:
        import torch
        devices = torch.cuda.device_count()
    why = check_world(a.gpus, a.gpus, devices, a.allow_shared_device)
    if why:
        print(f"bench.py: {why}", file=sys.stderr, flush=True)
        return 2
    import signal

    def stop(signum, frame):  # a launcher killed by its caller takes its ranks along
        raise SystemExit(128 + signum)

    for sig in (signal.SIGTERM, signal.SIGINT, signal.SIGHUP):
        signal.signal(sig, stop)
    procs = []
    script = script or os.path.abspath(__file__)
    for r, env in enumerate(rank_plan(a.gpus, free_port(), os.environ)):
        # rank 0's stdout is this process's (its JSON line); the others' go to stderr
        procs.append(subprocess.Popen([sys.executable, "-u", script] + list(argv), env=env,
                                      stdout=None if r == 0 else sys.stderr))
    rc = 0
    try:
        live = list(procs)
        while live:
            for p in list(live):
                code = p.poll()
                if code is None:
                    continue
                live.remove(p)
                if code != 0 and rc == 0:
                    rc = code if code > 0 else 1
                    print(f"bench.py: rank {procs.index(p)} exited with {code}; stopping the others",
                          file=sys.stderr, flush=True)
                    for o in live:
                        o.kill()
            time.sleep(0.05)
    finally:
        for p in procs:  # exact PIDs this launcher started
            if p.poll() is None:
                p.kill()
                p.wait()
    return rc


def dist_init(a):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    return rank, world, local


def barrier(world):
    if world > 1:
        import torch.distributed as dist
        dist.barrier()


def max_over_ranks(x: float, world: int) -> float:
    if world == 1:
        return x
    import torch
    import torch.distributed as dist
    t = torch.tensor([x], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def host_cpu_info():
    """What the CPU baseline ran on: the machine's logical CPUs, the ones this
    process may use (affinity), the cgroup CPU quota if any, the model."""
    info = {"nproc_machine": os.cpu_count()}
    try:
        info["affinity_cpus"] = len(os.sched_getaffinity(0))
    except Exception:
        pass
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        info["cgroup_cpu_quota"] = None if q == "max" else round(int(q) / int(per), 2)
    except Exception:
        pass
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                info["model"] = line.split(":", 1)[1].strip()
                break
    except Exception:
        pass
    return info


def usable_cpus():
    """Logical CPUs this process can actually run on: the affinity mask,
    capped by the cgroup CPU quota (the GPU box shows its whole machine,
    e.g. 256 CPUs, to a job limited to 16 by its cgroup; 256 threads there
    measure the throttling, not the CPU: 29 GiB/s against 85 GiB/s)."""
    info = host_cpu_info()
    n = info.get("affinity_cpus") or info.get("nproc_machine") or 1
    q = info.get("cgroup_cpu_quota")
    if q:
        n = min(n, max(1, int(q + 0.999)))
    return n


def cpu_baseline(k, m, S, stripes, threads):
    """Restated reference algorithm (oracle/rs_oracle_simd.c: split-nibble
    pshufb GF MAC, one stripe per thread) on a bounded sample of the workload:
    ~10 s on `threads` host threads (default: every CPU the process may use,
    SURVEY.md §8d; the host's CPU count, quota and model are reported), then
    ~4 s on one core (the reference quotes ~110 us per
    1 MiB block on one core, encode.rs:512)."""
    import numpy as np
    from oracle import oracle as O
    threads = max(1, min(threads, 512))
    buf = np.zeros((stripes, k + m, S), dtype=np.uint8)
    buf[:, :k] = np.random.default_rng(0).integers(0, 256, (stripes, k, S), dtype=np.uint8)

    def timed(nthreads, nstripes, budget_s):
        view = buf[:nstripes]
        O.encode_batch_mt(k, m, S, view, None, nthreads)  # warm-up
        reps, t0 = 0, time.perf_counter()
        while True:  # a fixed amount of wall time regardless of the host's speed
            O.encode_batch_mt(k, m, S, view, None, nthreads)
            reps += 1
            el = time.perf_counter() - t0
            if el > budget_s:
                return reps, el, reps * nstripes * k * S / el / GiB

    reps, el, gibs = timed(threads, stripes, 10.0)
    n1 = min(stripes, 16)
    reps1, el1, gibs1 = timed(1, n1, 4.0)
    return {"value": round(gibs, 3), "unit": "GiB/s", "cores": threads, "kind": "port",
            "sample": f"{reps} passes x {stripes} stripes RS({k},{m}) S={S} on {threads} threads ({el:.1f}s), "
                      f"AVX2={'yes' if O.lib().ro_simd_level() >= 2 else 'no'}",
            "host": host_cpu_info(),
            "value_1core": round(gibs1, 3),
            "sample_1core": f"{reps1} passes x {n1} stripes on 1 thread ({el1:.1f}s); "
                            f"{el1 / (reps1 * n1) * 1e6 * (1 << 20) / (k * S):.1f} us per 1 MiB of payload "
                            f"(reference: ~110 us per 1 MiB block on one core, encode.rs:512)"}


def random_stripes(dev, k, m, S, n, seed):
    """n synthetic stripes in the a3 layout (n, k+m, S), data bytes uniform
    random, resident in HBM."""
    import torch
    st = torch.empty((n, k + m, S), dtype=torch.uint8, device=dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    step = max(1, (384 << 20) // (k * S))
    for s0 in range(0, n, step):
        s1 = min(n, s0 + step)
        st[s0:s1, :k] = torch.randint(0, 256, (s1 - s0, k, S), dtype=torch.uint8, device=dev, generator=g)
    return st


DUMP_MAX_BYTES = 64 * 1000 * 1000  # --dump-outputs: every file together, as float32
DUMP_SEED = 5150


def dump_plan(k, m, S, n, digests, max_bytes=DUMP_MAX_BYTES, seed=DUMP_SEED):
    """What --dump-outputs keeps of one encode pass over (n, k+m, S) stripes,
    the same for every run with the same geometry: {file name: (stripe
    indices, byte columns or None for a whole row)}.  The parity is 2 GiB on
    the default line, so the dump is a seeded sample of it in float32 elements
    (4 bytes each): at most half the budget for the whole parity of a few
    stripes ("parity_stripes"), a quarter for a few byte columns of every
    stripe's parity, or of as many stripes as fit ("parity_columns"), and an
    eighth for the fused digests of as many stripes as fit ("digests")."""
    import numpy as np
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    budget = max_bytes // 4 - 3 * 64  # elements, less the three .npy headers
    plan = {}
    ns = min(n, (budget // 2) // (m * S))
    if ns:
        plan["parity_stripes"] = (np.sort(perm[:ns]), None)
    nr = min(n, (budget // 4) // m)
    nc = min(S, (budget // 4) // (nr * m))
    plan["parity_columns"] = (np.sort(perm[:nr]), np.sort(rng.permutation(S)[:nc]))
    if digests:
        nd = min(n, (budget // 8) // ((k + m) * 32))
        if nd:
            plan["digests"] = (np.sort(perm[:nd]), None)
    return plan


def dump_outputs(out_dir, stripes, digests, k, m):
    """--dump-outputs: what a caller of the timed path holds after its last
    step — the parity shards the encode wrote into the stripes (and the
    digests of --digests) — sampled by dump_plan, gathered on the device and
    written as float32 out_dir/<name>.npy."""
    import numpy as np
    import torch
    n, t, S = stripes.shape
    dev = stripes.device
    os.makedirs(out_dir, exist_ok=True)

    def index(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)

    shard = torch.arange(k, t, device=dev)
    for name, (rows, cols) in dump_plan(k, m, S, n, digests is not None).items():
        if name == "digests":
            got = digests[index(rows)]
        elif cols is None:
            got = stripes[index(rows), k:]
        else:
            got = stripes[index(rows)[:, None, None], shard[None, :, None], index(cols)[None, None, :]]
        np.save(os.path.join(out_dir, name + ".npy"), got.cpu().numpy().astype(np.float32))


PMC_TRAFFIC = os.path.join(ROOT, "tools", "pmc_traffic.json")


def pmc_lookup(key):
    """HBM bytes per call of one measured configuration from the committed
    PMC passes (tools/pmc_traffic.json, shipped with the tree: FETCH_SIZE x 2
    + WRITE_SIZE, the microarch guide's gfx950 correction; tools/pmc.sh,
    tools/pmc_engine.sh, tools/pmc_traffic.py), or None when no pass covered it."""
    try:
        return json.load(open(PMC_TRAFFIC)).get(key, {}).get("bytes_per_launch")
    except Exception:
        return None


def pmc_traffic(k, m, S, n, digests):
    return pmc_lookup(f"rs{k}{m}_S{S}_n{n}{'_hash' if digests else ''}")


def time_encode(e, stripes, digests, stream, reps, warm=3, warm_seconds=0.5):
    """Average device time (ms) of one rsg_encode_batch_dev over `reps`
    launches: HIP events on the launch stream around each, after `warm`
    untimed launches continued until the device has been busy with this
    kernel for `warm_seconds` (clock ramp after the previous extras)."""
    import torch
    for _ in range(warm):
        e.encode_batch(stripes, digests, stream=stream)
    torch.cuda.synchronize()
    t_w = time.perf_counter()
    while time.perf_counter() - t_w < warm_seconds:
        for _ in range(4):
            e.encode_batch(stripes, digests, stream=stream)
        torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, t in ev:
        s.record(stream)
        e.encode_batch(stripes, digests, stream=stream)
        t.record(stream)
    torch.cuda.synchronize()
    ms = [s.elapsed_time(t) for s, t in ev]
    return sum(ms) / len(ms), min(ms)


def encode_extra(name_workload, e, stripes, digests, k, m, S, n, stream, reps, timed=None):
    """One encode configuration priced like the headline: algorithmic bytes =
    k*S read + m*S written per stripe (+ 32*(k+m) digest bytes with fused
    digests), over the average launch time (`timed`: already measured)."""
    avg, mn = timed if timed else time_encode(e, stripes, digests, stream, reps)
    alg = n * (k + m) * S + (n * (k + m) * 32 if digests is not None else 0)
    return {"workload": name_workload, "k": k, "m": m, "shard_bytes": S, "stripes": n,
            "traffic": pmc_traffic(k, m, S, n, digests is not None),
            "kernel_ms": round(avg, 4), "kernel_ms_min": round(mn, 4), "launches": reps,
            "GiB_s_payload": round(n * k * S / (avg * 1e-3) / GiB, 2),
            "alg_bytes": alg, "achieved_GB_s": round(alg / (avg * 1e-3) / 1e9, 1),
            "frac": round(alg / (avg * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}


def config5_plan(world: int, rank: int, total: int):
    """BASELINE config 5 (RS(16,4), 1 MiB stripes, a batch split across the
    node's GPUs): (first stripe, stripes this rank encodes, stripes timed over
    all ranks).  One GPU runs its share of the 8-GPU split (total / 8); N > 1
    ranks split the whole batch contiguously (dispatch.split_batch: the
    stripes are independent, encode.rs:795-919, so no collective)."""
    from rustfs_amd.dispatch import split_batch
    if world == 1:
        return 0, total // 8, total // 8
    s0, cnt = split_batch(total, world, rank)
    return s0, cnt, total


def gather_ranks(x, world: int):
    if world == 1:
        return [x]
    import torch.distributed as dist
    out = [None] * world
    dist.all_gather_object(out, x)
    return out


def config_extras(a, e_main, stripes, k, m, dev, stream, rank, world=1):
    """BASELINE configs 4 and 5 timed beside the headline so the driver's
    default run carries them, at every N: config 4 (RS(8,4) encode + fused
    HH256S, 4096 stripes per rank, weak) and config 5 (RS(16,4), S = 65536,
    --config5-total stripes split over the ranks, strong; one GPU runs its
    share of the 8-way split).  With N > 1 each is bracketed by a barrier and
    its wall time is the max over ranks; every rank's kernel time, fraction
    and device are reported."""
    import torch
    from rustfs_amd import Erasure
    out = {}
    reps = max(10, a.steps)

    def timed_ranks(name, e, st, dig, kk, mm, S, n, total):
        torch.cuda.synchronize()
        t_w = time.perf_counter()  # untimed warm-up (clock ramp after the previous extras)
        while time.perf_counter() - t_w < 0.5:
            for _ in range(4):
                e.encode_batch(st, dig, stream=stream)
            torch.cuda.synchronize()
        barrier(world)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        avg, mn = time_encode(e, st, dig, stream, reps, warm=0, warm_seconds=0.0)
        el = max_over_ranks(time.perf_counter() - t0, world)
        alg = n * (kk + mm) * S + (n * (kk + mm) * 32 if dig is not None else 0)
        res = encode_extra(name, e, st, dig, kk, mm, S, n, stream, reps, timed=(avg, mn))
        mine = {"kernel_ms": res["kernel_ms"], "frac": res["frac"], "stripes": n, "device": dev.index}
        ranks = gather_ranks(mine, world)
        if world > 1:
            res.update({"n_gpus": world, "total_stripes": total,
                        "GiB_s_payload_all_ranks": round(reps * total * kk * S / el / GiB, 2),
                        "wall_ms_max_over_ranks": round(el * 1e3, 3),
                        "per_rank_kernel_ms": [r["kernel_ms"] for r in ranks],
                        "per_rank_frac": [r["frac"] for r in ranks],
                        "per_rank_stripes": [r["stripes"] for r in ranks],
                        "per_rank_device": [r["device"] for r in ranks],
                        "alg_bytes_per_launch_this_rank": alg})
        return res

    # config 4: RS(8,4) 1 MiB stripes, parity + all 12 HH256S digests in one
    # pass (the PUT path's kernel, bitrot.rs:496-502), a.config4_batch per rank
    n4, k4, m4 = a.config4_batch, 8, 4
    S4 = -(-(1 << 20) // k4)
    if (k, m, a.stripe_bytes, stripes.shape[0]) == (k4, m4, 1 << 20, n4):
        st4, e4 = stripes, e_main
    else:
        st4, e4 = random_stripes(dev, k4, m4, S4, n4, 2000 + rank), Erasure(k4, m4, 1 << 20, device=dev.index)
    dig = torch.empty((n4, k4 + m4, 32), dtype=torch.uint8, device=dev)
    out["encode_fused_hh256s"] = timed_ranks(
        f"RS(8,4) encode + fused HighwayHash-256S digests, 1 MiB stripes, batch {n4} per GPU (config 4)",
        e4, st4, dig, k4, m4, S4, n4, n4 * world)
    del dig, st4
    # config 5: RS(16,4), S = 65536, the batch split over the ranks
    k5, m5 = 16, 4
    S5 = -(-(1 << 20) // k5)
    _, n5, total5 = config5_plan(world, rank, a.config5_total)
    st5 = random_stripes(dev, k5, m5, S5, n5, 3000 + rank)
    e5 = Erasure(k5, m5, 1 << 20, device=dev.index)
    what = (f"RS(16,4) encode, 1 MiB stripes, {total5} stripes split over {world} GPUs (config 5)" if world > 1 else
            f"RS(16,4) encode, 1 MiB stripes, {n5} stripes: one GPU's share of the 8-GPU split of "
            f"{a.config5_total} (config 5)")
    out["encode_rs16_4"] = timed_ranks(what, e5, st5, None, k5, m5, S5, n5, total5)
    del st5
    torch.cuda.empty_cache()
    return out


ENGINE_WARM_S = 0.5  # each engine loop: back-to-back calls until the device has been busy this long
ENGINE_REPS = 20     # then this many timed calls (kernel median / min / max from the in-call hook)


def engine_plan(k, m, S, n, full=True):
    """The engine extras one geometry's line carries: (name, algorithmic bytes
    per call, PMC lookup key or None).  Algorithmic bytes are what the call's
    contract moves at minimum: every record it must verify read once (t - e
    present files of 32 + S bytes per stripe), every output byte written once.
    full (the RS(8,4) headline's geometry): also the asynchronous GET / heal."""
    t, rec = k + m, 32 + S
    g = f"rs{k}{m}_S{S}_n{n}"
    plan = [("get_all_present", n * k * rec, f"get_into0_{g}"),
            ("get_2_data_lost", n * ((t - 2) * rec + 2 * S), f"get_into2_{g}"),
            ("heal_1data_1parity", n * ((t - 2) * rec + 2 * rec), f"heal_1d1p_{g}"),
            ("bitrot_verify_all_files", t * n * rec, f"verify_all_{g}")]
    if full:
        plan += [("get_all_present_async", n * k * rec, None),
                 ("get_2_data_lost_async", n * ((t - 2) * rec + 2 * S), None),
                 ("heal_1data_1parity_async", n * ((t - 2) * rec + 2 * rec), None)]
    return plan


def steady_loop(fn, warm_s):
    """Back-to-back calls of fn until the device has been busy for warm_s
    (the clock the chip holds under this load, not the first calls after an
    idle or a different kernel); returns the last result."""
    import torch
    r = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_s:
        for _ in range(4):
            r = fn()
        torch.cuda.synchronize()
    return r


def engine_extras(e, stripes, k, m, S, n, stream, record_engine="auto", full=True, reps=ENGINE_REPS,
                  warm_s=ENGINE_WARM_S):
    """SURVEY §8(f) engines on the same device-resident batch, as BitrotWriter
    record files ([HH256S][S bytes] per block): GET all present, GET with two
    data disks lost (in place, reconstruct_into's contract), heal of one data
    + one parity disk, whole-file bitrot_verify (engine_plan).  Every entry is
    timed in steady state, the headline's protocol: warm-up calls until the
    device has been busy for warm_s, then `reps` calls; the kernel time of each
    comes from HIP events recorded inside the call (rsg_set_kernel_timing) —
    median, min and max — and the whole calls' time from HIP events on the
    stream around all of them.  The roofline is priced on engine_plan's
    algorithmic bytes."""
    import torch
    from rustfs_amd.bitrot import HashAlgorithm, bitrot_verify_batch
    t, rec = k + m, 32 + S
    plan = {name: (alg, key) for name, alg, key in engine_plan(k, m, S, n, full)}
    dig = torch.empty((n, t, 32), dtype=torch.uint8, device=stripes.device)
    e.encode_batch(stripes, dig, stream=stream)
    files = []
    for i in range(t):
        f = torch.empty((n, rec), dtype=torch.uint8, device=stripes.device)
        f[:, :32] = dig[:, i]
        f[:, 32:] = stripes[:, i]
        files.append(f.reshape(-1))
    del dig
    res = {}

    import ctypes
    from rustfs_amd import _lib
    L, ctx = _lib.load(), _lib.context(stripes.device.index or 0).handle

    def timed(name, fn, check):
        alg, key = plan[name]
        steady_loop(fn, warm_s)
        kms = []
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        _lib.check(L.rsg_set_kernel_timing(ctx, 1))
        try:
            ev[0].record(stream)
            for _ in range(reps):
                r = fn()
                v = ctypes.c_float(-1)
                _lib.check(L.rsg_last_kernel_ms(ctx, ctypes.byref(v)))
                kms.append(v.value)
            ev[1].record(stream)
            torch.cuda.synchronize()
        finally:
            _lib.check(L.rsg_set_kernel_timing(ctx, 0))
        check(r)
        ms = ev[0].elapsed_time(ev[1]) / reps
        res[name] = {"call_ms": round(ms, 4), "calls": reps, "warm_s": warm_s,
                     "GiB_s_payload": round(n * k * S / (ms * 1e-3) / GiB, 1),
                     "alg_bytes": alg, "achieved_GB_s": round(alg / (ms * 1e-3) / 1e9, 1),
                     "frac_call": round(alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                     "traffic": pmc_lookup(key) if key else None}
        if kms and min(kms) > 0:
            km = sorted(kms)[len(kms) // 2]  # the median
            res[name].update({"kernel_ms": round(km, 4), "kernel_ms_min": round(min(kms), 4),
                              "kernel_ms_max": round(max(kms), 4), "max_over_min": round(max(kms) / min(kms), 3),
                              "kernel_ms_each": [round(x, 4) for x in kms],
                              "frac": round(alg / (km * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)})
        else:
            res[name]["frac"] = res[name]["frac_call"]

    def timed_pipelined(name, submit, check):
        """`reps` calls, each submitted before the previous one is waited on
        (the asynchronous ABI), after the same steady-state warm-up, timed
        with HIP events on the stream around all of them: the device never
        idles while the host reads a batch's verdicts."""
        alg, _ = plan[name]
        steady_loop(lambda: submit().wait(), warm_s)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(stream)
        tk = submit()
        for _ in range(reps - 1):
            nxt = submit()
            r = tk.wait()
            tk = nxt
        r = tk.wait()
        ev[1].record(stream)
        torch.cuda.synchronize()
        ms = ev[0].elapsed_time(ev[1]) / reps
        check(r)
        res[name] = {"call_ms": round(ms, 4), "calls": reps, "warm_s": warm_s,
                     "GiB_s_payload": round(n * k * S / (ms * 1e-3) / GiB, 1),
                     "alg_bytes": alg, "frac_call": round(alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}

    _lib.check(L.rsg_set_record_engine(ctx, {"auto": _lib.RSG_RECORD_ENGINE_AUTO,
                                              "one-pass": _lib.RSG_RECORD_ENGINE_ONE_PASS,
                                              "two-pass": _lib.RSG_RECORD_ENGINE_TWO_PASS}[record_engine]))
    res["record_engine"] = record_engine
    res["protocol"] = (f"steady state: back-to-back calls until the device has been busy {warm_s} s, then "
                       f"{reps} timed calls; kernel_ms = median of the in-call HIP-event kernel times")

    # GET, in-place form (rsg_decode_records_into_dev, reconstruct_into's
    # contract, bridge.rs:274-307): present data served from the verified
    # records, only the lost shards written into their slots — all present:
    # the k data records read once; two data disks lost: t-2 records read, two
    # shards written
    slots = torch.empty((n, k * S), dtype=torch.uint8, device=stripes.device)

    def ok_into(lost):  # every stripe's rebuilt shards against the encoded data (on the device)
        def check(r):
            sl, src, status = r
            assert all(x == 0 for x in status)
            for i in range(k):
                assert (not src[i].any()) if i in lost else src[i].all(), i
            for i in lost:
                assert torch.equal(sl.view(n, k, S)[:, i], stripes[:, i]), i
        return check

    lost = [None if i in (0, 3) else files[i] for i in range(t)]
    timed("get_all_present", lambda: e.decode_records_into_batch(files, S, n, targets=slots, stream=stream),
          ok_into(()))
    if full:  # submitted back to back (rsg_decode_records_submit): the host's verdict reading overlapped
        timed_pipelined("get_all_present_async",
                        lambda: e.decode_records_submit(files, S, n, targets=slots, inplace=True, stream=stream),
                        ok_into(()))
    timed("get_2_data_lost", lambda: e.decode_records_into_batch(lost, S, n, targets=slots, stream=stream),
          ok_into((0, 3)))
    if full:  # the same GETs submitted back to back (rsg_decode_records_submit)
        timed_pipelined("get_2_data_lost_async",
                        lambda: e.decode_records_submit(lost, S, n, targets=slots, inplace=True, stream=stream),
                        ok_into((0, 3)))
    tg = [torch.empty(n * rec, dtype=torch.uint8, device=stripes.device) if i in (1, k) else None for i in range(t)]
    src = [None if i in (1, k) else files[i] for i in range(t)]

    def ok_heal(status):
        assert all(x == 0 for x in status) and torch.equal(tg[1], files[1]) and torch.equal(tg[k], files[k])

    def ok_verify(status):
        assert status == [0] * t

    timed("heal_1data_1parity", lambda: e.heal_records_batch(src, tg, S, n, stream=stream), ok_heal)
    if full:
        timed_pipelined("heal_1data_1parity_async", lambda: e.heal_records_submit(src, tg, S, n, stream=stream),
                        ok_heal)
    timed("bitrot_verify_all_files",
          lambda: bitrot_verify_batch(files, n * rec, n * S, HashAlgorithm.HighwayHash256S, S, stream=stream),
          ok_verify)
    del files, lost, tg, src, slots
    torch.cuda.empty_cache()
    return res


def rs12_4_extras(a, dev, stream):
    """rustfs's 16-drive default, RS(12,4) (storageclass.rs:24-31), at 1 MiB
    blocks (S = 87382: ragged walks, records at 2 mod 8) on the driver's line:
    encode, encode + fused HH256S (the PUT path's kernel), and the engines of
    engine_plan(12, 4, ...) — each with kernel_ms, frac and traffic."""
    import torch
    from rustfs_amd import Erasure
    k, m, n = 12, 4, a.rs12_batch
    S = -(-(1 << 20) // k)
    st = random_stripes(dev, k, m, S, n, 4000)
    e = Erasure(k, m, 1 << 20, device=dev.index)
    out = {"workload": f"RS(12,4), 1 MiB blocks (S={S}), {n} stripes (16-drive default set, storageclass.rs:24-31)"}
    reps = max(10, a.steps)
    out["encode"] = encode_extra(f"RS(12,4) encode, S={S}, n={n}", e, st, None, k, m, S, n, stream, reps)
    dig = torch.empty((n, k + m, 32), dtype=torch.uint8, device=dev)
    out["encode_fused_hh256s"] = encode_extra(f"RS(12,4) encode + fused HH256S, S={S}, n={n}", e, st, dig,
                                              k, m, S, n, stream, reps)
    del dig
    out["engines"] = engine_extras(e, st, k, m, S, n, stream, full=False)
    del st
    torch.cuda.empty_cache()
    return out


def link_bound_ms(in_bytes, out_bytes, h2d_gbs, d2h_gbs):
    """The fastest a host-memory call can run on the link: its bytes in at the
    measured pinned H2D rate and its bytes out at the D2H rate, the two
    directions overlapped (PCIe is full duplex), so the larger of the two."""
    return max(in_bytes / (h2d_gbs * 1e9), out_bytes / (d2h_gbs * 1e9)) * 1e3


def host_path_plan(k, m, S, n):
    """The host-memory (PCIe-inclusive) entries of extras.host_path, north_star's
    "the rate including pinned hipMemcpyAsync to and from the GPU": (name, bytes
    in over the link, bytes out, payload bytes) per call.  Encode moves the k
    data shards in and the m parity shards (+ all digests) out
    (rsg_encode_batch_host, encode_batched's dispatch, encode.rs:795-919); the
    streamed GET (pipeline.get_stream, decode_inner, decode.rs:1702-1968) moves
    every present record in and only the rebuilt data shards out (the
    in-place GET: present data are served from the host stage they were read
    into); the streamed PUT moves the data in and every record's parity +
    digests out."""
    t, rec = k + m, 32 + S
    return [("encode_batch_host", n * k * S, n * m * S, n * k * S),
            ("encode_batch_host_hh256s", n * k * S, n * m * S + n * t * 32, n * k * S),
            ("get_stream_all_present", n * t * rec, 0, n * k * S),
            ("get_stream_2_data_lost", n * (t - 2) * rec, n * 2 * S, n * k * S),
            ("get_stream_bytes_all_present", n * t * rec, 0, n * k * S),
            ("get_stream_data_shards_only_all_present", n * k * rec, 0, n * k * S),
            ("put_stream_hh256s", n * k * S, n * m * S + n * t * 32, n * k * S)]


def host_path_extras(dev, stream, n=1024, reps=5):
    """extras.host_path: the path as the reference runs it, starting and
    ending in host memory (north_star; SURVEY §8(d)'s pinned hipMemcpyAsync
    rate).  RS(8,4), 1 MiB blocks, n blocks (1 GiB of payload):
    - raw page-locked copy rates, H2D, D2H and both at once (two streams);
    - rsg_encode_batch_host on page-locked stripes, without and with the fused
      HH256S digests (H2D -> encode -> D2H pipelined inside the library);
    - pipeline.get_stream over BitrotWriter shard files in tmpfs, all present
      and with two data disks lost (pread into page-locked stages, H2D,
      verify + rebuild on the GPU, rebuilt shards D2H, the range's bytes
      yielded block by block);
    - pipeline.put_stream of the same object from a tmpfs body file (pread
      into page-locked batches, encode + digests on the GPU, one writev per
      shard file).
    Each entry: ms per call (best of `reps` after a warm-up call), payload
    GiB/s, bytes over the link, the link-bound time at the measured copy
    rates (link_bound_ms) and frac_link = that bound / the measured time."""
    import shutil
    import numpy as np
    import torch
    from rustfs_amd import Erasure
    from rustfs_amd import pipeline
    from rustfs_amd.pipeline import _pinned
    k, m = 8, 4
    bs = 1 << 20
    S, t, rec = bs // k, k + m, 32 + bs // k
    out = {"workload": f"RS(8,4), 1 MiB blocks (S={S}), {n} blocks = {n * bs / GiB:.2f} GiB of payload, "
                       f"host memory at both ends"}

    def copy_gbs(nbytes):
        h = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        h2 = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        d = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        d2 = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        s2 = torch.cuda.Stream(dev)
        res = {}
        for name, fn in (("h2d", lambda: d.copy_(h, non_blocking=True)),
                         ("d2h", lambda: h.copy_(d, non_blocking=True))):
            fn()
            torch.cuda.synchronize()
            best = None
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                el = time.perf_counter() - t0
                best = el if best is None else min(best, el)
            res[name] = nbytes / best / 1e9
        best = None
        for _ in range(reps):  # both directions at once, one copy per stream
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.copy_(h, non_blocking=True)
            with torch.cuda.stream(s2):
                h2.copy_(d2, non_blocking=True)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            best = el if best is None else min(best, el)
        res["both"] = 2 * nbytes / best / 1e9
        return res

    link = copy_gbs(1 << 30)
    out["pinned_copy_GB_s"] = {"h2d": round(link["h2d"], 2), "d2h": round(link["d2h"], 2),
                               "h2d_plus_d2h_concurrent": round(link["both"], 2), "bytes_per_copy": 1 << 30}
    plan = {name: (bi, bo, pay) for name, bi, bo, pay in host_path_plan(k, m, S, n)}

    def entry(name, ms, extra=None):
        bi, bo, pay = plan[name]
        bound = link_bound_ms(bi, bo, link["h2d"], link["d2h"])
        r = {"ms": round(ms, 3), "GiB_s_payload": round(pay / (ms * 1e-3) / GiB, 2),
             "link_bytes_in": bi, "link_bytes_out": bo, "link_bound_ms": round(bound, 3),
             "frac_link": round(bound / ms, 4)}
        if extra:
            r.update(extra)
        out[name] = r

    e = Erasure(k, m, bs, device=dev.index)
    st = _pinned((n, t, S))
    g = torch.Generator(device=dev).manual_seed(77)
    for s0 in range(0, n, 256):  # random data made on the device, copied into the page-locked stripes
        s1 = min(n, s0 + 256)
        torch.from_numpy(st[s0:s1, :k]).copy_(
            torch.randint(0, 256, (s1 - s0, k, S), dtype=torch.uint8, device=dev, generator=g))
    dg = _pinned((n, t, 32))

    def best_ms(fn):
        fn()  # warm-up: staging allocation, clock ramp
        b = None
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            el = (time.perf_counter() - t0) * 1e3
            b = el if b is None else min(b, el)
        return b

    entry("encode_batch_host", best_ms(lambda: e.encode_batch_host(st)))
    entry("encode_batch_host_hh256s", best_ms(lambda: e.encode_batch_host(st, dg)))
    # the records of the encoded object, checked against the device path once
    chk = torch.from_numpy(st[:4].copy()).to(dev)
    cd = torch.empty((4, t, 32), dtype=torch.uint8, device=dev)
    e.encode_batch(chk, cd)
    torch.cuda.synchronize()
    assert torch.equal(chk.cpu(), torch.from_numpy(st[:4])) and torch.equal(cd.cpu(), torch.from_numpy(dg[:4]))
    del chk, cd

    need = int(n * bs * (1 + 2 * t / k) * 1.1)  # body + GET files + PUT files
    root = None
    try:
        sv = os.statvfs("/dev/shm")
        if sv.f_bavail * sv.f_frsize > need + (2 << 30):
            root = os.path.join("/dev/shm", f"rsg_bench_{os.getpid()}")
    except OSError:
        pass
    if root is None:
        out["streams"] = "skipped: /dev/shm lacks room for the shard files (tmpfs keeps the figures the host pipeline's)"
        return out
    os.makedirs(root)
    try:
        paths = [os.path.join(root, f"part.{i}") for i in range(t)]
        for i in range(t):  # BitrotWriter records [HH256S][shard] per block (bitrot.rs:464-510)
            recs = np.empty((n, rec), dtype=np.uint8)
            recs[:, :32] = dg[:, i]
            recs[:, 32:] = st[:, i]
            with open(paths[i], "wb") as f:
                f.write(recs.data)
            del recs
        size = n * bs
        stage = pipeline.GetStage()

        def get(lost, views=True, data_only=False):
            fds = [None if i in lost else os.open(paths[i], os.O_RDONLY) for i in range(t)]
            try:
                got = 0
                for chunk in pipeline.get_stream(e, fds, size, stage=stage, views=views, data_shards_only=data_only):
                    got += sum(len(v) for v in chunk) if views else len(chunk)
                assert got == size
            finally:
                for fd in fds:
                    if fd is not None:
                        os.close(fd)

        for lost in ((), (0, 3)):  # untimed correctness pass: every block against the stripes
            fds = [None if i in lost else os.open(paths[i], os.O_RDONLY) for i in range(t)]
            try:
                for b, chunk in enumerate(pipeline.get_stream(e, fds, size, stage=stage, views=True)):
                    assert b"".join(chunk) == st[b, :k].tobytes(), f"get_stream block {b} (lost {lost})"
            finally:
                for fd in fds:
                    if fd is not None:
                        os.close(fd)
        form = {"batch_blocks": pipeline.DEFAULT_BATCH_BLOCKS,
                "yields": "views: each block as memoryviews of the shard buffers (write_data_blocks' form, "
                          "decode.rs:1390)"}
        entry("get_stream_all_present", best_ms(lambda: get(())), form)
        entry("get_stream_2_data_lost", best_ms(lambda: get((0, 3))), form)
        entry("get_stream_bytes_all_present", best_ms(lambda: get((), views=False)),
              {"batch_blocks": pipeline.DEFAULT_BATCH_BLOCKS, "yields": "bytes: each block joined into one object"})
        entry("get_stream_data_shards_only_all_present", best_ms(lambda: get((), data_only=True)),
              dict(form, reads="the k data files only (RUSTFS_GET_LOCKSTEP_DATA_SHARDS_ONLY_ENABLE, "
                                "decode.rs:125-143; off by default in the reference)"))
        stage.close()
        body = os.path.join(root, "body")
        with open(body, "wb") as f:  # the object: block b is stripe b's k data shards
            f.write(np.ascontiguousarray(st[:, :k]).data)
        wpaths = [os.path.join(root, f"put.{i}") for i in range(t)]
        pstage = {}

        def put():
            for p_ in wpaths:  # a new part's files (not a truncation of the last call's)
                if os.path.exists(p_):
                    os.remove(p_)
            fds = [os.open(p_, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for p_ in wpaths]
            try:
                t0 = time.perf_counter()
                with open(body, "rb", buffering=0) as f:
                    r = pipeline.put_stream(e, f, size, fds, stage=pstage.get("s"))
                el = (time.perf_counter() - t0) * 1e3
                pstage["s"] = r["stage"]
                if el < pstage.get("best", 1e30):
                    pstage["best"] = el
                    pstage["clock"] = {x: round(r[x] * 1e3, 2) for x in ("read_s", "submit_s", "wait_s", "write_s")}
            finally:
                for fd in fds:
                    os.close(fd)

        put()
        for _ in range(reps):
            put()
        ms = pstage["best"]
        for i in range(t):  # the PUT's shard files equal the records the GET read
            with open(wpaths[i], "rb") as a_, open(paths[i], "rb") as b_:
                assert a_.read() == b_.read(), f"put_stream shard file {i}"
        entry("put_stream_hh256s", ms, {"batch_blocks": pipeline.DEFAULT_BATCH_BLOCKS,
                                        "inflight_batches": pipeline.DEFAULT_INFLIGHT_BATCHES,
                                        "clock_ms": pstage["clock"]})
        out["files"] = "shard files and object body in tmpfs (/dev/shm): the host pipeline's rate, not a disk's"
    finally:
        shutil.rmtree(root, ignore_errors=True)
    return out


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    a = parse(argv)
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        return launch_ranks(a, argv)  # before anything touches the GPU
    import torch
    from rustfs_amd.dispatch import check_world, device_for_rank
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    why = check_world(a.gpus, world_env, torch.cuda.device_count(), a.allow_shared_device)
    if why:
        print(f"bench.py: {why}", file=sys.stderr, flush=True)
        return 2
    rank, world, local = dist_init(a)
    from rustfs_amd import Erasure, RSG_RECONSTRUCT_MISSING, _lib  # noqa: F401

    # one process per GPU: rank r on device LOCAL_RANK (shared only in a
    # --allow-shared-device rehearsal)
    local = device_for_rank(local, torch.cuda.device_count(), a.allow_shared_device)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    k, m = a.k, a.m
    S = -(-a.stripe_bytes // k)
    n = a.batch
    if a.total_batch:
        from rustfs_amd.dispatch import split_batch
        _, n = split_batch(a.total_batch, world, rank)  # contiguous stripe split, no collective
    e = Erasure(k, m, a.stripe_bytes, device=local)

    # synthetic stripes, a3 layout (n, k+m, S), data random, resident in HBM
    stripes = random_stripes(dev, k, m, S, n, 1000 + rank)
    digests = torch.empty((n, k + m, 32), dtype=torch.uint8, device=dev) if a.digests else None
    stream = torch.cuda.current_stream(dev)

    def step():
        e.encode_batch(stripes, digests, stream=stream)

    # W untimed warm-up steps, continued (still untimed) until the device has
    # been busy for --warm-seconds: after an idle period the first ~25 launches
    # run ~12 % slower while the clocks ramp (tools/kbench/lib_encode.cpp:
    # 1.21 ms, then 1.07 ms per RS(8,4) n=4096 encode), and the metric is the
    # steady-state rate of a busy engine.  The timed region is unchanged:
    # exactly K full steps.
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t_w = time.perf_counter()
    while time.perf_counter() - t_w < a.warm_seconds:
        for _ in range(8):
            step()
        torch.cuda.synchronize()

    # per-launch device time with HIP events on the launch stream
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
    barrier(world)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        ev[i][0].record(stream)
        step()
        ev[i][1].record(stream)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    barrier(world)
    elapsed = max_over_ranks(elapsed, world)
    kern_ms = sorted(s.elapsed_time(t) for s, t in ev)
    avg_ms = sum(kern_ms) / len(kern_ms)
    mine = {"rank": rank, "device": local, "pci_bus": None, "kernel_ms": avg_ms}
    try:
        mine["pci_bus"] = torch.cuda.get_device_properties(local).pci_bus_id
    except Exception:
        pass
    ranks = [mine]
    if world > 1:
        import torch.distributed as dist
        ranks = [None] * world
        dist.all_gather_object(ranks, mine)
    rank_ms = [r["kernel_ms"] for r in ranks]

    payload = n * k * S
    total_stripes = a.total_batch if a.total_batch else n * world
    value = a.steps * total_stripes * k * S / elapsed / GiB
    alg_bytes = n * (k + m) * S + (n * (k + m) * 32 if a.digests else 0)
    achieved = alg_bytes / (avg_ms * 1e-3) / 1e9

    if a.dump_outputs and rank == 0:  # before the extras: config 3 rebuilds shards of this buffer
        dump_outputs(a.dump_outputs, stripes, digests, k, m)

    extras = {}
    if a.full and not a.no_extras:
        # config 3: reconstruct with 1-4 missing data shards (same buffer)
        for miss in ((0,), (0, 3), (0, 3, 5), (0, 3, 5, 7)):
            present = [i not in miss for i in range(k + m)]
            for _ in range(2):
                e.reconstruct_batch(stripes, present, RSG_RECONSTRUCT_MISSING, stream=stream)
            torch.cuda.synchronize()
            reps = max(3, a.steps // 4)
            s_ev, t_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s_ev.record(stream)
            for _ in range(reps):
                e.reconstruct_batch(stripes, present, RSG_RECONSTRUCT_MISSING, stream=stream)
            t_ev.record(stream)
            torch.cuda.synchronize()
            ms = s_ev.elapsed_time(t_ev) / reps
            rb = n * (k + len(miss)) * S
            extras[f"reconstruct_e{len(miss)}"] = {
                "GiB_s_payload": round(payload / (ms * 1e-3) / GiB, 2),
                "kernel_ms": round(ms, 4), "alg_bytes": rb,
                "traffic": pmc_lookup(f"reconstruct_e{len(miss)}_rs{k}{m}_S{S}_n{n}"),
                "hbm_GB_s": round(rb / (ms * 1e-3) / 1e9, 1),
                "frac": round(rb / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        # round trip correctness of the last pattern (cheap, on device)
        ok = e.verify_batch(stripes, stream=stream)
        torch.cuda.synchronize()
        extras["verify_all_ok_after_reconstruct"] = bool(ok.all().item())
        if not a.no_engines and world == 1 and not a.digests:
            extras["engines"] = engine_extras(e, stripes, k, m, S, n, stream, a.record_engine)
        if not a.no_engines and not a.no_rs12 and world == 1 and (k, m) != (12, 4):
            extras["rs12_4"] = rs12_4_extras(a, dev, stream)
        if not a.no_config_extras:
            extras.update(config_extras(a, e, stripes, k, m, dev, stream, rank, world))
        if not a.no_host_path and world == 1:
            extras["host_path"] = host_path_extras(dev, stream, a.host_path_blocks)

    traffic = pmc_traffic(k, m, S, n, a.digests)

    cpu = None
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
        cpu = cpu_baseline(k, m, S, min(a.cpu_sample_stripes, n), a.cpu_threads or usable_cpus())

    if rank == 0:
        line = {
            "metric": "GiB/s RS(8,4) encode+reconstruct, device-resident 1 MiB stripes, 1/2/4/8 GPU",
            "value": round(value, 3),
            "unit": "GiB/s",
            "n_gpus": world,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": round(elapsed / a.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "strong" if a.total_batch else "weak",
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic (uniform random bytes, torch generator), device-resident",
            "config": {"workload": f"RS(k={k},m={m}) encode{' + fused HH256S' if a.digests else ''}, "
                                   f"{a.stripe_bytes} B stripes (S={S}), batch {n} per GPU",
                       "timed": "value and roofline: the encode pass (one rsg_encode_batch_dev per step); "
                                "reconstruct with 1-4 missing shards and the GET/heal engines: extras",
                       "k": k, "m": m, "shard_bytes": S, "stripes_per_gpu": n, "total_stripes": total_stripes,
                       "parallelism": f"stripe-split x{world}"},
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                         "kernel_ms_avg": round(avg_ms, 4), "kernel_ms_min": round(kern_ms[0], 4),
                         "alg_bytes_per_launch": alg_bytes,
                         "per_rank_kernel_ms": [round(x, 4) for x in rank_ms],
                         "per_rank_frac": [round(alg_bytes / (x * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) for x in rank_ms],
                         "per_rank_device": [r["device"] for r in ranks],
                         "per_rank_pci_bus": [r["pci_bus"] for r in ranks],
                         "shared_device": len(set(r["device"] for r in ranks)) < world},
            "cpu_baseline": cpu,
            "extras": extras,
        }
        print(json.dumps(line), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
