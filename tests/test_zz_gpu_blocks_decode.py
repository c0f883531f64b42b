"""Gathered block reconstruct (rsg_reconstruct_blocks) on the GPU, against the
CPU oracle.

Every buffer the library may touch is a window in a larger array filled with
0xA5, and a whole array is compared with what it must hold afterwards: the
oracle's shard inside the window of a shard the call rebuilds, the bytes it
held before everywhere else (present shards, the 0xA5 windows of absent shards
the mode does not rebuild, the expected digests, the guard bytes).

The file's name sorts after test_zz_gpu_blocks.py, so these tests are
collected last and the run order of the suite before them is unchanged."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, compat_data

pytestmark = pytest.mark.gpu

FILL = 0xA5
OFFS = (0, 1, 3, 8, 13)  # shard starts, bytes past a 16-byte boundary
HH, LEGACY, NONE = 1, 2, 0
DATA, MISSING, REENCODE = 0, 1, 2
MODES = (DATA, MISSING, REENCODE)
OK, TOO_FEW = 0, 8


def _ktile():
    src = open(os.path.join(ROOT, "rustfs_amd", "csrc", "rs_blocks_plan.h")).read()
    return int(re.search(r"constexpr\s+uint32_t\s+kTile\s*=\s*(\d+)\s*;", src).group(1))


KT = _ktile()
LENS = (1, 15, 16, 17, 255, KT - 1, KT, KT + 1, 2 * KT + 3, 87382)


def _arena(nbytes, pinned):
    """A 0xA5-filled uint8 array and the index of a 16-byte boundary at least
    16 bytes into it: every window has 0xA5 guard bytes below and above it."""
    if pinned:
        import torch
        a = torch.empty(nbytes + 64, dtype=torch.uint8).pin_memory().numpy()
    else:
        a = np.empty(nbytes + 64, dtype=np.uint8)
    a[:] = FILL
    return a, 16 + (-a.ctypes.data) % 16


def targets_of(k, t, usable, mode):
    """The shards a reconstruct in `mode` writes, restated: lost data always,
    lost parity under MISSING, every parity shard that is not one of the
    first k usable shards under REENCODE."""
    surv = [s for s in range(t) if usable[s]][:k]
    tg = [s for s in range(k) if not usable[s]]
    if mode == MISSING:
        tg += [s for s in range(k, t) if not usable[s]]
    if mode == REENCODE:
        tg += [s for s in range(k, t) if s not in surv]
    return tg


class RBlk:
    """One degraded block: its arrays, the windows in them, and what they must
    hold after a call.  present: k+m truth values; rot: {shard: byte index}
    of present shards with one flipped byte; digests: None or the algo whose
    expected digests the block carries; wrong_absent: the digest entries of
    absent shards are garbage."""

    def __init__(self, oracle, k, m, S, layout, pinned, seed, present, rot=None, digests=None, wrong_absent=False,
                 with_bad=True, data=None):
        self.k, self.m, self.S, self.t = k, m, S, k + m
        t = k + m
        self.present = [bool(p) for p in present]
        self.rot = dict(rot or {})
        self.algo = digests
        rng = np.random.default_rng(seed)
        self.full = np.zeros((t, S), dtype=np.uint8)
        self.full[:k] = rng.integers(0, 256, (k, S), dtype=np.uint8) if data is None else data
        if m:
            oracle.encode(k, m, self.full)
        self.arrays, self.shards = [], []
        kinds = pinned if isinstance(pinned, (list, tuple)) else [pinned] * t
        if layout == "packed":  # shards back to back in one buffer
            a, z = _arena(t * S + 16, kinds[0])
            z += OFFS[seed % 5]
            self.arrays.append(a)
            self.shards = [a[z + s * S: z + (s + 1) * S] for s in range(t)]
        else:  # one buffer per shard, each at its own offset
            for s in range(t):
                a, z = _arena(S + 16, kinds[s])
                z += OFFS[(seed + s) % 5]
                self.arrays.append(a)
                self.shards.append(a[z: z + S])
        for s in range(t):
            if self.present[s]:
                self.shards[s][:] = self.full[s]
                if s in self.rot:
                    self.shards[s][self.rot[s]] ^= 0x40
        a, z = _arena(t * 32 + t + 32, False)
        self.arrays.append(a)
        self.dig = a[z + OFFS[(seed + 2) % 5]:][:t * 32]
        self.bad = a[z + t * 32 + 16:][:t]
        self.with_bad = with_bad
        if digests is not None:
            h = oracle.hh256s if digests == HH else oracle.hh256s_legacy
            for s in range(t):
                if self.present[s] or not wrong_absent:
                    self.dig[32 * s: 32 * s + 32] = np.frombuffer(h(self.full[s]), dtype=np.uint8)
                else:
                    self.dig[32 * s: 32 * s + 32] = 0x11
        self.pres = np.array([3 if p else 0 for p in self.present], dtype=np.uint8)
        self.before = [x.copy() for x in self.arrays]
        self.ptrs = (ctypes.c_void_p * t)(*[s.ctypes.data for s in self.shards])

    def desc(self, d):
        d.shards = ctypes.cast(self.ptrs, ctypes.POINTER(ctypes.c_void_p))
        d.shard_len = self.S
        d.present = self.pres.ctypes.data
        d.digests = self.dig.ctypes.data if self.algo is not None else None
        d.bad = self.bad.ctypes.data if self.with_bad else None

    def reset(self):
        for a, b in zip(self.arrays, self.before):
            a[:] = b

    def check_untouched(self):
        for a, b in zip(self.arrays, self.before):
            assert (a == b).all()

    def expected(self, mode, algo):
        """(status, bad bytes, targets) of a call in `mode` with `algo`."""
        verified = algo != NONE and self.algo is not None
        assert not verified or algo == self.algo
        bad = [1 if (verified and self.present[s] and s in self.rot) else 0 for s in range(self.t)]
        usable = [self.present[s] and not bad[s] for s in range(self.t)]
        if sum(usable) < self.k:
            return TOO_FEW, bad, []
        # (a rotten shard that goes unnoticed must not be a survivor: the test would expect garbage)
        assert not any(s in self.rot for s in [s for s in range(self.t) if usable[s]][:self.k])
        return OK, bad, targets_of(self.k, self.t, usable, mode)

    def check(self, mode, algo, status, tag=""):
        """Every array holds exactly what it must."""
        want_status, bad, tg = self.expected(mode, algo)
        assert status == want_status, (tag, "status", status, want_status)
        for s in tg:
            assert (self.shards[s] == self.full[s]).all(), (tag, "shard", s, self.S, mode)
        if self.with_bad:
            assert self.bad.tolist() == bad, (tag, "bad", self.bad.tolist(), bad)
        # put the written windows back: the arrays must then equal their earlier copies
        keep = [a.copy() for a in self.arrays]
        for s in tg:
            self.shards[s][:] = self.full[s] if self.present[s] else FILL
            if self.present[s] and s in self.rot:
                self.shards[s][self.rot[s]] ^= 0x40
        if self.with_bad:
            self.bad[:] = FILL
        try:
            self.check_untouched()
        finally:
            for a, b in zip(self.arrays, keep):
                a[:] = b


def recon_blocks(lib, ctx, k, m, blks, mode, algo, want_status=True):
    from rustfs_amd import _lib
    descs = (_lib.rsg_rblock * max(len(blks), 1))()
    for i, b in enumerate(blks):
        b.desc(descs[i])
    status = (ctypes.c_int * max(len(blks), 1))(*([0x5A5A] * max(len(blks), 1)))
    rc = lib.rsg_reconstruct_blocks(ctx.handle, k, m, len(blks), ctypes.byref(descs), mode, algo,
                                    status if want_status else None)
    return rc, list(status)[:len(blks)]


def run_and_check(lib, ctx, k, m, blks, mode, algo, tag=""):
    for b in blks:
        b.reset()
    rc, status = recon_blocks(lib, ctx, k, m, blks, mode, algo)
    assert rc == 0, (tag, rc)
    for i, b in enumerate(blks):
        b.check(mode, algo, status[i], (tag, i))


def all_masks(k, m):
    t = k + m
    return [[(x >> s) & 1 for s in range(t)] for x in range(1 << t) if bin(x).count("1") >= k]


_pattern_blocks = {}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,m", [(8, 4), (4, 2)])
def test_every_pattern_in_one_call(gpu, rsgpu_lib, oracle, k, m, mode):
    """Every loss pattern the geometry can rebuild as one block each of one
    call: per-block tables and every row count.  (No pattern has more than m
    targets: under REENCODE a parity shard among the survivors re-encodes to
    itself and is not written, so a block never needs a second row group.)"""
    if (k, m) not in _pattern_blocks:
        masks = all_masks(k, m)
        assert len(masks) == {(8, 4): 794, (4, 2): 22}[(k, m)]
        _pattern_blocks[(k, m)] = [RBlk(oracle, k, m, 33, "packed", False, seed=i, present=p) for i, p in enumerate(masks)]
    blks = _pattern_blocks[(k, m)]
    run_and_check(rsgpu_lib, gpu, k, m, blks, mode, NONE)
    assert {len(b.expected(mode, NONE)[2]) for b in blks} == set(range(0 if mode != REENCODE else m, m + 1))


GEOMS = [(1, 1), (2, 2), (4, 2), (8, 4), (9, 4), (12, 4), (13, 3), (16, 4)]


def _random_present(rng, k, m):
    lost = rng.choice(k + m, size=int(rng.integers(0, m + 1)), replace=False)
    return [s not in lost for s in range(k + m)]


@pytest.mark.parametrize("k,m", GEOMS)
def test_lengths_alignments_geometries(gpu, rsgpu_lib, oracle, k, m):
    """n = 17 blocks of mixed lengths and mixed loss patterns in one call,
    every shard pointer at its own offset from a 16-byte boundary, both
    layouts, three modes; a third of the blocks verified when an algo is
    given.  Covers the unrolled kernels and both group sizes of the rolled
    one, with partial groups."""
    g = GEOMS.index((k, m))
    rng = np.random.default_rng(1000 + g)
    lens = [LENS[(g + i) % len(LENS)] for i in range(17)]
    for layout in ("packed", "separate"):
        blks = [RBlk(oracle, k, m, S, layout, False, seed=g * 100 + i, present=_random_present(rng, k, m),
                     digests=HH if i % 3 == 0 else None) for i, S in enumerate(lens)]
        assert any(not all(b.present) for b in blks)
        for mode in MODES:
            for algo in (NONE, HH):
                run_and_check(rsgpu_lib, gpu, k, m, blks, mode, algo, (layout, mode, algo))


@pytest.mark.parametrize("zero_copy", ["0", "1"])
def test_memory_kinds(gpu, rsgpu_lib, oracle, zero_copy):
    """Pageable arrays, one page-locked buffer per block, separately
    page-locked shards, and blocks whose shards alternate between the two:
    each kind alone and all in one call, verified and not, staged
    (RSG_ZERO_COPY=0) and in place."""
    from rustfs_amd import _lib
    k, m = 8, 4
    t = k + m
    lens = (131072, KT + 1, 33, 1025, 87382, 17, 4097, 255)
    kinds = [("packed", False), ("packed", True), ("separate", True), ("separate", [s % 2 == 0 for s in range(t)])]
    present = [[s not in lost for s in range(t)] for lost in ((1, 6), (0,), (3, 9, 11), (7, 8), (2, 5, 10), (4, 11), (0, 1, 2, 3), ())]
    blks = [RBlk(oracle, k, m, S, *kinds[i % 4], seed=40 + i, present=present[i], digests=HH) for i, S in enumerate(lens)]
    with _lib.tuned(RSG_ZERO_COPY=zero_copy):
        for algo in (NONE, HH):
            for mode in (DATA, REENCODE):
                for group in (blks[0::4], blks[1::4], blks[2::4], blks[3::4], blks):
                    run_and_check(rsgpu_lib, gpu, k, m, group, mode, algo, (zero_copy, algo, mode))


@pytest.mark.parametrize("algo", [HH, LEGACY])
def test_verification(gpu, rsgpu_lib, oracle, algo):
    """One flipped byte in a present data, parity or surplus shard, at the
    first, middle and last byte: `bad` exact, the rotten shard rebuilt (a
    rotten parity shard under DATA only marked); a block driven below k usable
    shards is TOO_FEW with its buffers untouched while its neighbours are
    rebuilt; blocks with and without digests in one call; a wrong digest
    entry of an absent shard is ignored."""
    k, m = 8, 4
    t = k + m
    S = KT + 37
    where = (0, S // 2, S - 1)
    cases = []
    for lost, rot_shard in [((1,), 4),         # a data shard among the survivors
                            ((1,), 9),         # a surplus parity shard
                            ((0, 2), 8),       # a parity shard among the survivors
                            ((0, 2), 11),      # a surplus parity shard, two data shards lost
                            ((), 5),           # nothing lost, one rotten data shard
                            ((3, 9), 10),      # one data and one parity shard lost, surplus parity rotten
                            ((0, 1, 2), 5)]:   # exactly k usable shards left
        for w in where:
            cases.append(dict(present=[s not in lost for s in range(t)], rot={rot_shard: w}, digests=algo))
    blks = [RBlk(oracle, k, m, S, ("packed", "separate")[i % 2], i % 3 == 0, seed=300 + i, wrong_absent=True, **c)
            for i, c in enumerate(cases)]
    # below k usable: 4 lost and one rotten; 3 lost and two rotten
    few = [RBlk(oracle, k, m, S, "packed", False, seed=390, present=[s >= 4 for s in range(t)], rot={6: 5}, digests=algo),
           RBlk(oracle, k, m, 100, "separate", True, seed=391, present=[s not in (0, 5, 10) for s in range(t)],
                rot={1: 0, 11: 99}, digests=algo)]
    blks.insert(3, few[0])
    blks.insert(9, few[1])
    # not verified: its flipped byte, in a surplus shard, goes unnoticed (the block behaves as rsg_reconstruct's)
    blks.insert(5, RBlk(oracle, k, m, 257, "packed", False, seed=392, present=[s != 2 for s in range(t)], rot={9: 3}, digests=None))
    # verified, no `bad` array
    blks.append(RBlk(oracle, k, m, 33, "packed", False, seed=393, present=[s != 7 for s in range(t)], rot={0: 32}, digests=algo,
                     with_bad=False))
    for mode in MODES:
        assert all(b.expected(mode, algo)[0] == TOO_FEW for b in few)
        run_and_check(rsgpu_lib, gpu, k, m, blks, mode, algo, ("verify", mode))


def test_validation_errors_write_nothing(gpu, rsgpu_lib, oracle):
    from rustfs_amd import _lib
    k, m = 4, 2
    t = k + m
    blks = [RBlk(oracle, k, m, S, "packed", False, seed=70 + i, present=[s != i for s in range(t)], digests=HH)
            for i, S in enumerate((100, 4097, 33))]

    def expect(status, algo=HH, mode=DATA, k_=k, m_=m, want_status=True):
        rc, st = recon_blocks(rsgpu_lib, gpu, k_, m_, blks, mode, algo, want_status)
        assert rc == status, (rc, status)
        assert st == [0x5A5A] * len(blks)
        for b in blks:
            b.check_untouched()

    for s in (0, 2, k):  # a NULL pointer of a present, an absent and a parity shard, in the last block
        blks[2].ptrs[s] = None
        expect(_lib.RSG_ERR_INVALID_ARG)
        blks[2].ptrs[s] = blks[2].shards[s].ctypes.data
    blks[1].S = 0
    expect(_lib.RSG_ERR_EMPTY_SHARD)
    blks[1].S = 1 << 32
    expect(_lib.RSG_ERR_INVALID_ARG)
    blks[1].S = 4097
    expect(_lib.RSG_ERR_INVALID_ARG, mode=3)
    expect(_lib.RSG_ERR_INVALID_ARG, mode=-1)
    expect(_lib.RSG_ERR_INVALID_ARG, algo=9)
    expect(_lib.RSG_ERR_INVALID_ARG, want_status=False)  # verified blocks need the status array
    # fewer than k present in one block fails the call
    keep = blks[1].pres.copy()
    blks[1].pres[:3] = 0
    expect(_lib.RSG_ERR_TOO_FEW_SHARDS)
    expect(_lib.RSG_ERR_TOO_FEW_SHARDS, algo=NONE)
    blks[1].pres[:] = keep
    # a shard of block 2 over one byte of a shard of block 0
    blks[2].ptrs[1] = blks[0].shards[3].ctypes.data + 99
    expect(_lib.RSG_ERR_INVALID_ARG)
    expect(_lib.RSG_ERR_INVALID_ARG, algo=NONE)
    blks[2].ptrs[1] = blks[2].shards[1].ctypes.data
    # `bad` of block 0 inside a shard of block 1
    keep = blks[0].bad
    blks[0].bad = blks[1].shards[2][5:5 + t]
    expect(_lib.RSG_ERR_INVALID_ARG)
    expect(_lib.RSG_ERR_INVALID_ARG, algo=NONE)
    blks[0].bad = keep
    # a shard of block 1 inside the digests of block 0: only with an algo
    blks[1].ptrs[0] = blks[0].dig.ctypes.data + 20
    expect(_lib.RSG_ERR_INVALID_ARG)
    blks[1].ptrs[0] = blks[1].shards[0].ctypes.data
    # geometry errors are rsg_reconstruct's
    expect(_lib.RSG_ERR_ZERO_DATA_SHARDS, k_=0, m_=2)
    expect(_lib.RSG_ERR_TOO_MANY_SHARDS, k_=200, m_=57)
    assert rsgpu_lib.rsg_reconstruct_blocks(gpu.handle, k, m, 0, None, DATA, HH, None) == 0
    assert rsgpu_lib.rsg_reconstruct_blocks(gpu.handle, k, m, 2, None, DATA, HH, None) == _lib.RSG_ERR_INVALID_ARG
    # two blocks may share their expected digests: they are only read
    blks[1].dig, keep = blks[0].dig, blks[1].dig
    rc, st = recon_blocks(rsgpu_lib, gpu, k, m, blks[:2], DATA, HH)
    assert rc == 0 and st == [OK, TOO_FEW]  # (block 0's digests are not block 1's)
    blks[1].dig = keep


def test_no_parity_geometry(gpu, rsgpu_lib, oracle):
    """m == 0: RSG_OK, `bad` and status zeroed, nothing else written."""
    k = 4
    b = RBlk(oracle, k, 0, 100, "separate", False, seed=5, present=[True] * k, rot={1: 3}, digests=HH)
    rc, st = recon_blocks(rsgpu_lib, gpu, k, 0, [b], DATA, HH)
    assert rc == 0 and st == [OK] and b.bad.tolist() == [0] * k
    b.bad[:] = FILL
    b.check_untouched()


@pytest.mark.parametrize("k,m", [(5, 5), (17, 3)])
def test_other_geometries_fall_back(gpu, rsgpu_lib, oracle, k, m):
    t = k + m
    blks = [RBlk(oracle, k, m, S, lay, False, seed=90 + i, present=[s not in lost for s in range(t)], rot=rot, digests=dg)
            for i, (S, lay, lost, rot, dg) in enumerate(((1025, "packed", (0, k), {2: 7}, HH),
                                                         (33, "separate", (1,), {}, None),
                                                         (KT + 1, "packed", (0, 1, 2), {3: 0}, HH),
                                                         (255, "separate", (2, k + 1), {}, HH)))]
    for mode in MODES:
        run_and_check(rsgpu_lib, gpu, k, m, blks, mode, HH, (mode, HH))
        run_and_check(rsgpu_lib, gpu, k, m, [b for b in blks if not b.rot], mode, NONE, (mode, NONE))
    if m == 3:
        assert blks[2].expected(DATA, HH)[0] == TOO_FEW


def test_block_larger_than_the_stage(gpu, rsgpu_lib, oracle):
    """RS(2,1) with 3 shards just over a third of the stage each: that block
    goes alone through the per-block path, its neighbours through the kernels."""
    from rustfs_amd import _lib
    k, m = 2, 1
    big = _lib.RSG_BLOCKS_STAGE_BYTES // 3 + 4096
    blks = [RBlk(oracle, k, m, S, "packed", False, seed=95 + i, present=[s != i % 3 for s in range(3)], digests=HH)
            for i, S in enumerate((1025, big, 33))]
    run_and_check(rsgpu_lib, gpu, k, m, blks, MISSING, HH)


@pytest.mark.parametrize("mode", MODES)
def test_same_as_rsg_reconstruct(gpu, rsgpu_lib, oracle, mode):
    """The same block through rsg_reconstruct and through
    rsg_reconstruct_blocks leaves identical arrays."""
    k, m = 8, 4
    t = k + m
    for S, lost in ((KT + 5, (0, 3, 9)), (33, (10,)), (4096, ())):
        a, b = (RBlk(oracle, k, m, S, "separate", False, seed=S, present=[s not in lost for s in range(t)]) for _ in range(2))
        assert rsgpu_lib.rsg_reconstruct(gpu.handle, k, m, S, a.ptrs, a.pres.ctypes.data, mode) == 0
        rc, st = recon_blocks(rsgpu_lib, gpu, k, m, [b], mode, NONE)
        assert rc == 0 and st == [OK]
        for x, y in zip(a.arrays[:t], b.arrays[:t]):
            assert (x == y).all()
        b.check(mode, NONE, st[0])


def test_rs42_compat_vector(gpu, rsgpu_lib, oracle, ref_vectors):
    """The reference's MinIO-compat vector (erasure.rs:2496-2545): its shards,
    whose digests are the reference's, with two dropped and rebuilt under
    verification; the oracle's reconstruct agrees."""
    v = ref_vectors["rs42_compat"]
    data = np.frombuffer(compat_data(v["len"]), dtype=np.uint8)
    S = -(-data.size // 4)
    flat = np.zeros(4 * S, dtype=np.uint8)
    flat[:data.size] = data
    for lost in ((0, 3), (1, 4), (4, 5)):
        b = RBlk(oracle, 4, 2, S, "packed", False, seed=1, present=[s not in lost for s in range(6)], digests=HH,
                 data=flat.reshape(4, S))
        assert [b.dig[32 * i: 32 * i + 32].tobytes().hex() for i in range(6)] == v["shard_hh256s"]
        ref = b.full.copy()
        for s in lost:
            ref[s] = 0
        oracle.reconstruct(4, 2, ref, b.present)
        assert (ref == b.full).all()
        run_and_check(rsgpu_lib, gpu, 4, 2, [b], MISSING, HH)
        for s in lost:
            assert oracle.hh256s(b.shards[s]).hex() == v["shard_hh256s"][s]


def test_python_surface(gpu, oracle):
    """Erasure.decode_blocks end to end, with None shards."""
    from rustfs_amd import Erasure, _lib
    k, m = 4, 2
    t = k + m
    src = [RBlk(oracle, k, m, S, "separate", False, seed=400 + i, present=[True] * t) for i, S in enumerate((33, KT + 1, 1025))]
    e = Erasure(k, m, 1 << 20)
    lost = ((0, 5), (2,), (1, 4))
    blocks = [[None if s in lost[i] else b.full[s].copy() for s in range(t)] for i, b in enumerate(src)]
    out = e.decode_blocks(blocks)
    for i, b in enumerate(src):
        assert out[i][0] == _lib.RSG_OK and out[i][1].tolist() == [0] * t
        for s in range(t):
            if s >= k and s in lost[i]:
                assert blocks[i][s] is None  # parity stays None under DATA
            else:
                assert bytes(blocks[i][s]) == b.full[s].tobytes()
    # verified, every missing shard rebuilt; block 1 has a rotten shard, block 2 too few usable
    blocks = [[None if s in lost[i] else b.full[s].copy() for s in range(t)] for i, b in enumerate(src)]
    blocks[1][0][7] ^= 1
    blocks[2][0][0] ^= 1
    digs = [np.frombuffer(b"".join(oracle.hh256s(b.full[s]) for s in range(t)), dtype=np.uint8).reshape(t, 32) for b in src]
    out = e.decode_blocks(blocks, digests=digs, mode=_lib.RSG_RECONSTRUCT_MISSING)
    assert [o[0] for o in out] == [_lib.RSG_OK, _lib.RSG_OK, _lib.RSG_ERR_TOO_FEW_SHARDS]
    assert out[0][1].tolist() == [0] * t and out[1][1].tolist() == [1] + [0] * (t - 1) and out[2][1].tolist() == [1] + [0] * (t - 1)
    for i in (0, 1):
        for s in range(t):
            assert bytes(blocks[i][s]) == src[i].full[s].tobytes()
