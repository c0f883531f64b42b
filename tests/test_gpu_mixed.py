"""Mixed-length batch encode + HH256S on the GPU (rsg_encode_mixed_dev / _host,
k_encode_hash_mixed): parity and all k+m digests of n stripes with different
shard lengths, always against the CPU oracle (oracle.encode, oracle.hh256s,
oracle.hh256s_legacy)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from mixed_shapes import SMALL_PERM, sweep_params

pytestmark = pytest.mark.gpu

FILL = 0xA5
LENGTHS = [0, 1, 7, 8, 31, 32, 33, 511, 512, 513, 1023, 1024, 1025, 87382]
GEOMETRIES = [(2, 2), (3, 1), (4, 2), (5, 3), (8, 4), (12, 4), (16, 4)]
HH, LEGACY = 1, 2  # RSG_HASH_HIGHWAY256S, RSG_HASH_HIGHWAY256S_LEGACY

_REF = {}


def spw_for(t):
    """Stripes per workgroup of the kernel (rs_fused.h fused_spw_for)."""
    return 1 if t % 16 == 0 else 2 if t % 8 == 0 else 4 if (t % 4 == 0 or t <= 6) else 2


def ref_stripe(O, k, m, S):
    """Oracle stripe of shard length S: ((k+m, S) shards, {algo: k+m digests});
    computed once per (k, m, S) and shared, never modified."""
    key = (k, m, S)
    if key not in _REF:
        st = np.zeros((k + m, S), dtype=np.uint8)
        st[:k] = np.random.default_rng(7919 * k + 31 * m + S).integers(0, 256, (k, S), dtype=np.uint8)
        if m and S:
            O.encode(k, m, st)
        st.setflags(write=False)
        digs = {HH: b"".join(O.hh256s(st[i]) for i in range(k + m)),
                LEGACY: b"".join(O.hh256s_legacy(st[i]) for i in range(k + m))}
        _REF[key] = (st, digs)
    return _REF[key]


class Batch:
    """n stripes of the given lengths packed at odd byte offsets with 1-3 byte
    gaps into a data arena and a parity arena (separate, or one a3 arena),
    every gap and 64 bytes after each arena filled with FILL; plus what the
    arenas and digests must hold afterwards."""

    def __init__(self, O, k, m, lens, aliased=False, seed=0):
        self.k, self.m, self.n, self.lens = k, m, len(lens), list(lens)
        rng = np.random.default_rng(seed)
        desc = np.zeros((self.n, 3), dtype=np.uint64)
        doff, poff = 1, 3  # odd starts
        for j, S in enumerate(lens):
            if aliased:
                desc[j] = (doff, doff + k * S, S)
                doff += (k + m) * S
            else:
                gap = int(rng.integers(1, 4))
                desc[j] = (doff, poff, S)
                doff += k * S + gap
                poff += m * S + gap
        self.desc = desc
        self.data = np.full(doff + 64, FILL, dtype=np.uint8)
        self.parity = self.data if aliased else np.full(poff + 64, FILL, dtype=np.uint8)
        self.want = {HH: [], LEGACY: []}
        for j, S in enumerate(lens):
            st, digs = ref_stripe(O, k, m, S)
            d0 = int(desc[j, 0])
            self.data[d0:d0 + k * S] = st[:k].reshape(-1)
            for a in (HH, LEGACY):
                self.want[a].append(digs[a])
        self.data_in = self.data.copy()
        self.parity_want = self.data_in.copy() if aliased else self.parity.copy()
        for j, S in enumerate(lens):
            st, _ = ref_stripe(O, k, m, S)
            p0 = int(desc[j, 1])
            self.parity_want[p0:p0 + m * S] = st[k:].reshape(-1)

    def digests_want(self, algo):
        return np.frombuffer(b"".join(self.want[algo]), dtype=np.uint8).reshape(self.n, self.k + self.m, 32)


def run_dev(b, algo=HH, digests=True):
    """One rsg_encode_mixed_dev over a Batch; returns (data, parity, digests) back on the host."""
    import torch
    from rustfs_amd import Erasure
    e = Erasure(b.k, b.m, 1 << 20)
    d = torch.from_numpy(b.data_in.copy()).cuda()
    p = d if b.parity is b.data else torch.from_numpy(b.parity.copy()).cuda()
    dig = torch.full((b.n, b.k + b.m, 32), FILL, dtype=torch.uint8, device="cuda") if digests else None
    e.encode_mixed(d, p, b.desc, dig, algo=algo)
    torch.cuda.synchronize()
    return d.cpu().numpy(), p.cpu().numpy(), (dig.cpu().numpy() if digests else None)


def check_dev(b, algos=(HH, LEGACY)):
    for algo in algos:
        d, p, dig = run_dev(b, algo)
        if b.parity is not b.data:
            assert np.array_equal(d, b.data_in), "data arena changed"
        bad = np.flatnonzero(p != b.parity_want)
        assert bad.size == 0, f"parity arena differs at {bad[:8]} (gaps and tail must stay {FILL:#x})"
        want = b.digests_want(algo)
        for j in range(b.n):
            assert np.array_equal(dig[j], want[j]), f"digests of stripe {j} (len {b.lens[j]}), algo {algo}"


def ordered(lens, how):
    up = sorted(lens)
    if how == "ascending":
        return up
    if how == "descending":
        return up[::-1]
    out = []  # long / short alternating
    lo, hi = 0, len(up) - 1
    while lo <= hi:
        out.append(up[hi])
        if lo < hi:
            out.append(up[lo])
        lo, hi = lo + 1, hi - 1
    return out


# -- 2 (first: the smallest launch of the kernel) --------------------------------

def test_single_stripe(gpu, oracle):
    """n = 1: one workgroup, one live encoder wave."""
    check_dev(Batch(oracle, 4, 2, [1025]), algos=(HH,))


@pytest.mark.parametrize("k,m", [(4, 2), (8, 4), (12, 4), (5, 3)])
def test_degenerate_batches(gpu, oracle, k, m):
    spw = spw_for(k + m)
    check_dev(Batch(oracle, k, m, [1025] + [0] * spw))  # n = SPW + 1: a workgroup of one long and empty stripes
    check_dev(Batch(oracle, k, m, [0] * (2 * spw + 1)))  # every workgroup has zero steps
    check_dev(Batch(oracle, k, m, [0]))


# -- 1 -----------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["ascending", "descending", "alternating"])
@pytest.mark.parametrize("k,m", GEOMETRIES)
def test_lengths_and_geometries(gpu, oracle, k, m, order):
    """All 14 lengths in one batch, separate arenas, stripes at odd offsets
    with 1-3 byte gaps: parity and digests (both keys) equal the oracle's,
    every gap, the bytes after each arena and the data arena come back
    untouched."""
    lens = ordered(LENGTHS, order)
    assert sorted(lens) == sorted(LENGTHS)
    check_dev(Batch(oracle, k, m, lens, seed=len(order)))


@pytest.mark.parametrize("k,m", sweep_params(1))
def test_every_shape(gpu, oracle, k, m):
    """Every instantiation of the kernel, k = 1..16 by m = 1..4, over the
    small length set (mixed_shapes.py): HH256S, the guard layout of
    test_lengths_and_geometries, whole arenas compared
    (test_mixed_shapes.py: the parameters are all 64 built shapes)."""
    check_dev(Batch(oracle, k, m, SMALL_PERM, seed=m), algos=(HH,))


# -- 3 -----------------------------------------------------------------------------

@pytest.mark.parametrize("k,m,S", [(8, 4, 1536), (12, 4, 87382), (4, 2, 100)])
def test_aliased_a3_layout(gpu, oracle, k, m, S):
    """d_parity == d_data with parity_off = data_off + k*S: uniform lengths
    equal rsg_encode_batch_dev and the oracle; RSG_HASH_NONE and a null digest
    pointer give the same parity."""
    import torch
    from rustfs_amd import Erasure, _lib
    n = 9
    b = Batch(oracle, k, m, [S] * n, aliased=True)
    check_dev(b)
    _, p_nodig, none = run_dev(b, digests=False)
    assert none is None and np.array_equal(p_nodig, b.parity_want)
    # a digest array with algo NONE
    e = Erasure(k, m, 1 << 20)
    d = torch.from_numpy(b.data_in.copy()).cuda()
    dig = torch.full((n, k + m, 32), FILL, dtype=torch.uint8, device="cuda")
    e.encode_mixed(d, d, b.desc, dig, algo=_lib.RSG_HASH_NONE)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), b.parity_want) and (dig.cpu().numpy() == FILL).all()
    # the uniform batch entry on the same bytes
    st = torch.from_numpy(b.data_in[1:1 + n * (k + m) * S].copy()).cuda().view(n, k + m, S)
    dg = torch.zeros((n, k + m, 32), dtype=torch.uint8, device="cuda")
    e.encode_batch(st, dg)
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy().reshape(-1), b.parity_want[1:1 + n * (k + m) * S])
    assert np.array_equal(dg.cpu().numpy(), b.digests_want(HH))


def test_aliased_mixed_lengths(gpu, oracle):
    check_dev(Batch(oracle, 8, 4, ordered(LENGTHS, "alternating"), aliased=True))


def test_offsets_past_2g_and_4g(gpu, oracle):
    """Stripes whose offsets have bit 31 set and whose offsets need more than
    32 bits (arenas of 4 GiB + a little, only the stripes' ranges filled and
    read back): 64-bit addressing end to end."""
    import torch
    from rustfs_amd import Erasure
    k, m = 4, 2
    lens = [1025, 700, 513]
    doffs = [5, (1 << 31) + 7, (1 << 32) + 9]
    poffs = [(1 << 31) - 1, (1 << 31) + 4099, (1 << 32) + 3]
    size = (1 << 32) + (1 << 16)
    data = torch.empty(size, dtype=torch.uint8, device="cuda")
    parity = torch.empty(size, dtype=torch.uint8, device="cuda")
    desc = np.array([[d, p, S] for d, p, S in zip(doffs, poffs, lens)], dtype=np.uint64)
    for d, p, S in zip(doffs, poffs, lens):
        st, _ = ref_stripe(oracle, k, m, S)
        data[d:d + k * S] = torch.from_numpy(st[:k].reshape(-1).copy()).cuda()
        parity[p - 8:p + m * S + 8] = FILL
    dig = torch.zeros((3, k + m, 32), dtype=torch.uint8, device="cuda")
    Erasure(k, m, 1 << 20).encode_mixed(data, parity, desc, dig)
    torch.cuda.synchronize()
    for j, (d, p, S) in enumerate(zip(doffs, poffs, lens)):
        st, digs = ref_stripe(oracle, k, m, S)
        got = parity[p - 8:p + m * S + 8].cpu().numpy()
        assert (got[:8] == FILL).all() and (got[-8:] == FILL).all()
        assert np.array_equal(got[8:-8], st[k:].reshape(-1)), f"parity of stripe {j}"
        assert dig[j].cpu().numpy().tobytes() == digs[HH]
        assert np.array_equal(data[d:d + k * S].cpu().numpy(), st[:k].reshape(-1))


# -- 4 -----------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(4, 0), (10, 6), (17, 3)])
def test_fallback_geometries(gpu, oracle, k, m):
    """Digests only (m = 0), m > 4 and k > 16: the same results through the
    per-length kernels."""
    check_dev(Batch(oracle, k, m, [0, 1, 33, 513, 1025, 4097, 0, 700]))


# -- 5 -----------------------------------------------------------------------------

def host_arrays(b, pinned):
    """A Batch's arenas and a digest array in pinned or pageable host memory."""
    import torch
    def mk(a):
        if not pinned:
            return a.copy()
        t = torch.empty(a.size, dtype=torch.uint8).pin_memory().numpy()
        t[:] = a
        return t
    dig = mk(np.full(b.n * (b.k + b.m) * 32, FILL, dtype=np.uint8)).reshape(b.n, b.k + b.m, 32)
    return mk(b.data_in), mk(b.parity), dig


def check_host(b, data, parity, dig, algo=HH):
    """Host form: data untouched, every parity range and digest right, bytes
    outside the call's parity span untouched (the gaps inside the span come
    back unspecified: include/rsgpu.h)."""
    assert np.array_equal(data, b.data_in)
    lo = min(int(b.desc[j, 1]) for j in range(b.n) if b.lens[j])
    hi = max(int(b.desc[j, 1]) + b.m * b.lens[j] for j in range(b.n) if b.lens[j])
    assert (parity[:lo] == FILL).all() and (parity[hi:] == FILL).all()
    for j, S in enumerate(b.lens):
        p0 = int(b.desc[j, 1])
        assert np.array_equal(parity[p0:p0 + b.m * S], b.parity_want[p0:p0 + b.m * S]), f"parity of stripe {j}"
    assert np.array_equal(dig, b.digests_want(algo))


@pytest.mark.parametrize("pinned", [True, False])
def test_host_sync_submit_and_jobs_in_flight(gpu, oracle, pinned):
    from rustfs_amd import Erasure
    e = Erasure(8, 4, 1 << 20)
    b1 = Batch(oracle, 8, 4, ordered(LENGTHS, "alternating"), seed=1)
    b2 = Batch(oracle, 8, 4, ordered(LENGTHS, "descending"), seed=2)
    d, p, g = host_arrays(b1, pinned)
    e.encode_mixed_host(d, p, b1.desc, g)
    check_host(b1, d, p, g)
    d, p, g = host_arrays(b1, pinned)
    e.encode_mixed_host(d, p, b1.desc, g, algo=LEGACY)
    check_host(b1, d, p, g, LEGACY)
    # submit / poll / wait, two jobs in flight
    a1, a2 = host_arrays(b1, pinned), host_arrays(b2, pinned)
    t1 = e.encode_mixed_host_submit(a1[0], a1[1], b1.desc, a1[2])
    t2 = e.encode_mixed_host_submit(a2[0], a2[1], b2.desc, a2[2])
    t2.wait()
    while not t1.poll():
        pass
    assert t1.poll() and t2.poll()
    check_host(b1, *a1)
    check_host(b2, *a2)
    # n = 0: a ticket that is already complete
    z = np.zeros(0, np.uint8)
    t0 = e.encode_mixed_host_submit(z, z.copy(), np.zeros((0, 3), np.uint64), None)
    assert t0.poll()
    # parity only
    d, p, _ = host_arrays(b1, pinned)
    e.encode_mixed_host(d, p, b1.desc, None)
    for j, S in enumerate(b1.lens):
        p0 = int(b1.desc[j, 1])
        assert np.array_equal(p[p0:p0 + 4 * S], b1.parity_want[p0:p0 + 4 * S])


def stage_bytes():
    import re
    src = open(os.path.join(ROOT, "include", "rsgpu.h")).read()
    m = re.search(r"#define\s+RSG_MIXED_STAGE_BYTES\s+\((\d+)u\s*<<\s*(\d+)\)", src)
    return int(m.group(1)) << int(m.group(2))


def test_host_three_sub_batches(gpu, oracle):
    """Seeded lengths up to 128 KiB, enough of them that their data spans
    alone exceed twice the staging size: at least three sub-batches, a few
    distinct lengths so that the oracle work stays small."""
    from rustfs_amd import Erasure
    k, m = 4, 2
    rng = np.random.default_rng(5)
    pool = [int(x) for x in rng.integers(1, (128 << 10) + 1, 6)] + [128 << 10]
    lens, total = [], 0
    while total <= 2 * stage_bytes():
        lens.append(pool[int(rng.integers(0, len(pool)))])
        total += k * lens[-1]
    b = Batch(oracle, k, m, lens, seed=3)
    d, p, g = host_arrays(b, pinned=True)
    t = Erasure(k, m, 1 << 20).encode_mixed_host_submit(d, p, b.desc, g)
    t.wait()
    check_host(b, d, p, g)


def test_host_intersecting_spans_rejected(gpu, oracle):
    """One host arena holding data and parity interleaved (a3): the spans
    intersect, RSG_ERR_INVALID_ARG, nothing written."""
    from rustfs_amd import _lib
    b = Batch(oracle, 4, 2, [100, 200, 300], aliased=True)
    arena = b.data_in.copy()
    tk = ctypes.c_uint64(5)
    L = _lib.load()
    rc = L.rsg_encode_mixed_host_submit(gpu.handle, 4, 2, b.n, b.desc.ctypes.data, arena.ctypes.data,
                                        arena.ctypes.data, None, 0, ctypes.byref(tk))
    assert rc == _lib.RSG_ERR_INVALID_ARG and tk.value == 0
    assert np.array_equal(arena, b.data_in)
    # two arenas whose spans do not intersect are fine in one allocation: parity after data
    sep = Batch(oracle, 4, 2, [100, 200, 300])
    one = np.full(sep.data.size + sep.parity.size, FILL, dtype=np.uint8)
    one[:sep.data.size] = sep.data_in
    assert L.rsg_encode_mixed_host(gpu.handle, 4, 2, sep.n, sep.desc.ctypes.data, one.ctypes.data,
                                   one.ctypes.data + sep.data.size, None, 0) == _lib.RSG_OK
    for j, S in enumerate(sep.lens):
        p0 = int(sep.desc[j, 1])
        assert np.array_equal(one[sep.data.size + p0:sep.data.size + p0 + 2 * S], sep.parity_want[p0:p0 + 2 * S])


# -- 6 -----------------------------------------------------------------------------

def test_failed_submit_drains(tmp_path):
    """rsg_encode_mixed_host_submit failing on its second sub-batch (the
    test-only rsg_test_fail_subbatch(1), in a child process): no ticket, the
    first sub-batch has landed when the call returns, the buffers can be freed
    at once and a following call is correct."""
    script = tmp_path / "child.py"
    script.write_text(f'''
import ctypes, gc, re, sys
sys.path.insert(0, {ROOT!r})
import numpy as np, torch
from oracle import oracle as O
from rustfs_amd import _lib
L = _lib.load(); ctx = _lib.context(0).handle
src = open({os.path.join(ROOT, "include", "rsgpu.h")!r}).read()
mm = re.search(r"#define\\s+RSG_MIXED_STAGE_BYTES\\s+\\((\\d+)u\\s*<<\\s*(\\d+)\\)", src)
stage = int(mm.group(1)) << int(mm.group(2))
k, m, S = 4, 2, 65536
n = 2 * (stage // (k * S)) + 2   # at least three sub-batches
desc = np.zeros((n, 3), dtype=np.uint64)
desc[:, 0] = np.arange(n) * k * S; desc[:, 1] = np.arange(n) * m * S; desc[:, 2] = S
def arenas():
    d = torch.empty(n * k * S, dtype=torch.uint8).pin_memory().numpy()
    d[:] = np.tile(np.random.default_rng(4).integers(0, 256, k * S, dtype=np.uint8), n)
    p = torch.empty(n * m * S, dtype=torch.uint8).pin_memory().numpy(); p[:] = 0xEE
    g = torch.empty(n * (k + m) * 32, dtype=torch.uint8).pin_memory().numpy(); g[:] = 0xEE
    return d, p, g
ref = np.zeros((k + m, S), dtype=np.uint8); ref[:k] = arenas()[0][:k * S].reshape(k, S); O.encode(k, m, ref)
refd = b"".join(O.hh256s(ref[i]) for i in range(k + m))
assert L.rsg_test_fail_subbatch(ctx, 1) == _lib.RSG_OK
d, p, g = arenas()
t = ctypes.c_uint64(77)
rc = L.rsg_encode_mixed_host_submit(ctx, k, m, n, desc.ctypes.data, d.ctypes.data, p.ctypes.data, g.ctypes.data,
                                    _lib.RSG_HASH_HIGHWAY256S, ctypes.byref(t))
assert rc == _lib.RSG_ERR_DEVICE and t.value == 0, (rc, t.value)
# sub-batch 0 landed before the call returned: no synchronisation here
assert np.array_equal(p[:m * S], ref[k:].reshape(-1)) and g[:(k + m) * 32].tobytes() == refd
assert (p[-m * S:] == 0xEE).all() and (g[-32:] == 0xEE).all()  # the failed and later sub-batches wrote nothing
del d, p, g; gc.collect()  # nothing is in flight: the buffers can go
assert L.rsg_test_fail_subbatch(ctx, -1) == _lib.RSG_OK
d, p, g = arenas()
assert L.rsg_encode_mixed_host(ctx, k, m, n, desc.ctypes.data, d.ctypes.data, p.ctypes.data, g.ctypes.data,
                               _lib.RSG_HASH_HIGHWAY256S) == _lib.RSG_OK
assert np.array_equal(p.reshape(n, m * S), np.tile(ref[k:].reshape(-1), (n, 1)))
assert g.tobytes() == refd * n
print("child ok")
''')
    p = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=150)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stderr[-3000:]


# -- 7 -----------------------------------------------------------------------------

def test_validation_leaves_parity_untouched(gpu, oracle):
    """Every invalid call returns RSG_ERR_INVALID_ARG (geometry errors as
    rsg_check_geometry) and writes nothing into a FILL-ed parity arena."""
    import torch
    from rustfs_amd import _lib
    L = _lib.load()
    k, m = 4, 2
    data = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    parity = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    dig = torch.full((4, k + m, 32), FILL, dtype=torch.uint8, device="cuda")

    def call(desc, d=data, p=parity, g=dig, algo=HH, kk=k, mm=m, n=None, null_desc=False):
        a = np.ascontiguousarray(np.asarray(desc, dtype=np.uint64).reshape(-1, 3))
        return L.rsg_encode_mixed_dev(gpu.handle, kk, mm, a.shape[0] if n is None else n,
                                      None if null_desc else a.ctypes.data, d.data_ptr() if d is not None else None,
                                      p.data_ptr() if p is not None else None,
                                      g.data_ptr() if g is not None else None, algo, None)

    ok = [[0, 0, 10], [40, 20, 10]]
    bad = [
        call([[0, 0, 10], [0, 20, 10]]),            # data_off not strictly ascending
        call([[0, 0, 10], [39, 20, 10]]),           # data ranges overlap
        call([[0, 20, 10], [40, 20, 10]]),          # parity_off not strictly ascending
        call([[0, 0, 10], [40, 19, 10]]),           # parity ranges overlap
        call([[0, 0, 1 << 32]]),                    # shard_len above 0xffffffff
        call([[0, 39, 10]], p=data),                # aliased: parity on data
        call([[0, 40, 10], [59, 100, 10]], p=data),
        call(ok, d=None), call(ok, p=None), call(ok, null_desc=True),
        call(ok, algo=3), call(ok, algo=-1),
    ]
    assert bad == [_lib.RSG_ERR_INVALID_ARG] * len(bad)
    assert call(ok, kk=0) == _lib.RSG_ERR_ZERO_DATA_SHARDS
    assert call(ok, kk=255, mm=2) == _lib.RSG_ERR_TOO_MANY_SHARDS
    assert call(ok, mm=-1) == _lib.RSG_ERR_INVALID_ARG
    assert call([], n=0, d=None, p=None, g=None) == _lib.RSG_OK  # n == 0
    torch.cuda.synchronize()
    assert bool((parity == FILL).all()) and bool((dig == FILL).all()) and not bool(data.any())
    assert call(ok) == _lib.RSG_OK  # and the valid table goes through
    torch.cuda.synchronize()
    assert not bool(parity[:40].any()) and bool((parity[40:] == FILL).all())


# -- 8 -----------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(8, 4), (12, 4), (5, 0)])
def test_encode_inline_shards_many(gpu, oracle, k, m):
    from rustfs_amd import Erasure
    e = Erasure(k, m, 1 << 20)
    rng = np.random.default_rng(40)
    sizes = [0, 1, k - 1, k, k + 1, 1 << 20] + [int(x) for x in np.exp(rng.uniform(np.log(2), np.log(300000), 34))]
    assert len(sizes) == 40
    rng.shuffle(sizes)
    datas = [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]
    many = e.encode_inline_shards_many(datas)
    again = e.encode_inline_shards_many([bytes(d) for d in datas[:7]])  # the reused arenas, smaller
    assert again == many[:7]
    assert len(many) == 40
    for j, d in enumerate(datas):
        if d.size == 0:
            assert many[j] == []
            continue
        S = -(-d.size // k)
        st = np.zeros((k + m, S), dtype=np.uint8)
        st.reshape(-1)[:d.size] = d
        if m:
            oracle.encode(k, m, st)
        assert many[j] == [oracle.hh256s(st[i]) + st[i].tobytes() for i in range(k + m)], f"object {j} ({d.size} B)"
        if j % 8 == 0 or d.size <= k + 1:
            assert many[j] == e.encode_inline_shards(d)


def test_put_objects_matches_put_object(gpu, oracle, tmp_path):
    from rustfs_amd.loopback import LocalErasureSet
    k, m = 4, 2
    sets = []
    for tag in ("many", "one"):
        dirs = [str(tmp_path / tag / f"d{i}") for i in range(k + m)]
        for d in dirs:
            os.makedirs(d)
        sets.append(LocalErasureSet(dirs, k, m, block_size=1 << 20))
    many, one = sets
    rng = np.random.default_rng(12)
    sizes = [0, 1, k, 1000, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 2 << 20, int(2.5 * (1 << 20)), 77777, 3, 1500000]
    items = [(f"obj{j}", rng.integers(0, 256, s, dtype=np.uint8).tobytes()) for j, s in enumerate(sizes)]
    metas = many.put_objects(items)
    assert [mt["size"] for mt in metas] == sizes
    for name, body in items:
        one.put_object(name, body)
    for name, body in items:
        for i in range(k + m):
            with open(many.part_file(i, name), "rb") as f, open(one.part_file(i, name), "rb") as g:
                assert f.read() == g.read(), f"{name} shard {i}"
        assert bytes(many.get_object(name)) == body
        assert many.verify_object(name) == [0] * (k + m), name
    many.close()
    one.close()
