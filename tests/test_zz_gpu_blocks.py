"""Gathered block encode (rsg_encode_blocks, rsg_encode_hashed) on the GPU,
against the CPU oracle.

Every buffer the library may write is a window in a larger array filled with
0xA5, and a whole array is compared with what it must hold afterwards: the
oracle's parity and digests inside the windows, the bytes it held before
everywhere else (data included).

The file's name sorts after every other test file, so these tests are
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


def _ktile():
    src = open(os.path.join(ROOT, "rustfs_amd", "csrc", "rs_blocks_plan.h")).read()
    return int(re.search(r"constexpr\s+uint32_t\s+kTile\s*=\s*(\d+)\s*;", src).group(1))


KT = _ktile()
LENS = (1, 7, 8, 9, 15, 16, 17, 31, 33, 255, 1023, 1024, 1025, KT - 1, KT, KT + 1, 2 * KT + 3, 87382, 131072)


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


class Blk:
    """One block: its arrays, the windows in them, and what they must hold."""

    def __init__(self, k, m, S, layout, pinned, seed, with_digests=True, pinned_digests=None):
        self.k, self.m, self.S = k, m, S
        t = k + m
        rng = np.random.default_rng(seed)
        self.arrays, self.shards = [], []
        if layout == "packed":  # encode_buffer's layout: shards back to back in one buffer
            a, z = _arena(t * S + 16, pinned)
            z += OFFS[seed % 5]
            self.arrays.append(a)
            self.shards = [a[z + s * S: z + (s + 1) * S] for s in range(t)]
        else:  # one buffer per shard, each at its own offset
            for s in range(t):
                a, z = _arena(S + 16, pinned)
                z += OFFS[(seed + s) % 5]
                self.arrays.append(a)
                self.shards.append(a[z: z + S])
        for s in range(k):
            self.shards[s][:] = rng.integers(0, 256, S, dtype=np.uint8)
        a, z = _arena(t * 32 + 16, pinned if pinned_digests is None else pinned_digests)
        z += OFFS[(seed + 2) % 5]
        self.arrays.append(a)
        self.dig = a[z: z + t * 32]
        self.with_digests = with_digests
        self.before = [x.copy() for x in self.arrays]
        self.ptrs = (ctypes.c_void_p * t)(*[s.ctypes.data for s in self.shards])

    def desc(self, d):
        d.shards = ctypes.cast(self.ptrs, ctypes.POINTER(ctypes.c_void_p))
        d.shard_len = self.S
        d.digests = self.dig.ctypes.data if self.with_digests else None

    def reference(self, oracle):
        """(parity (m, S), digests per algo {HH, LEGACY}: (k+m)*32 bytes), computed once."""
        if not hasattr(self, "_ref"):
            st = np.zeros((self.k + self.m, self.S), dtype=np.uint8)
            for s in range(self.k):
                st[s] = self.shards[s]
            oracle.encode(self.k, self.m, st)
            self._ref = (st[self.k:].copy(),
                         {HH: b"".join(oracle.hh256s(st[i]) for i in range(self.k + self.m)),
                          LEGACY: b"".join(oracle.hh256s_legacy(st[i]) for i in range(self.k + self.m))})
        return self._ref

    def reset(self):
        for a, b in zip(self.arrays, self.before):
            a[:] = b

    def check_untouched(self):
        for a, b in zip(self.arrays, self.before):
            assert (a == b).all()

    def check(self, oracle, algo, tag=""):
        """Every array holds exactly what it must: parity and (with an algo
        and a digest pointer) digests in their windows, everything else as
        before."""
        parity, digs = self.reference(oracle)
        for r in range(self.m):
            assert (self.shards[self.k + r] == parity[r]).all(), (tag, "parity", r, self.S)
        if algo != NONE and self.with_digests:
            assert self.dig.tobytes() == digs[algo], (tag, "digests", self.S)
        # now put the windows back: the arrays must equal their earlier copies
        keep = [s.copy() for s in self.shards[self.k:]], self.dig.copy()
        for r in range(self.m):
            self.shards[self.k + r][:] = FILL
        if algo != NONE and self.with_digests:  # else the digest window must still hold 0xA5
            self.dig[:] = FILL
        try:
            self.check_untouched()
        finally:
            for r in range(self.m):
                self.shards[self.k + r][:] = keep[0][r]
            self.dig[:] = keep[1]


def encode_blocks(lib, ctx, k, m, blks, algo):
    descs = (_rsg_block() * max(len(blks), 1))()
    for i, b in enumerate(blks):
        b.desc(descs[i])
    return lib.rsg_encode_blocks(ctx.handle, k, m, len(blks), ctypes.byref(descs), algo)


def _rsg_block():
    from rustfs_amd import _lib
    return _lib.rsg_block


GEOMS = [(1, 1), (2, 2), (4, 2), (8, 4), (12, 4), (16, 4)]


@pytest.mark.parametrize("n", [1, 2, 17])
@pytest.mark.parametrize("k,m", GEOMS)
def test_parity_and_digests_bit_exact(gpu, rsgpu_lib, oracle, k, m, n):
    """Mixed lengths in one call, every shard pointer at its own offset from a
    16-byte boundary, both layouts, both Highway algos, algo NONE, and NULL
    digests on some blocks.  Over n = 17, 2 and 1 a geometry sees every length
    of LENS."""
    g = GEOMS.index((k, m))
    rot = LENS[g * 3 % len(LENS):] + LENS[:g * 3 % len(LENS)]
    lens = {17: rot[:17], 2: rot[17:], 1: rot[18 - g % 2:][:1]}[n]
    for layout in ("packed", "separate"):
        blks = [Blk(k, m, S, layout, False, seed=g * 100 + i, with_digests=(i % 4 != 3)) for i, S in enumerate(lens)]
        for algo in (HH, LEGACY, NONE):
            for b in blks:
                b.reset()
            assert encode_blocks(rsgpu_lib, gpu, k, m, blks, algo) == 0
            for b in blks:
                b.check(oracle, algo, (layout, algo))


def test_rs42_compat_vector(gpu, rsgpu_lib, ref_vectors):
    """The reference's MinIO-compat vector (erasure.rs:2496-2545) through
    rsg_encode_blocks: the digests of all six shards."""
    v = ref_vectors["rs42_compat"]
    data = np.frombuffer(compat_data(v["len"]), dtype=np.uint8)
    S = -(-data.size // 4)
    b = Blk(4, 2, S, "packed", False, seed=1)
    flat = np.zeros(4 * S, dtype=np.uint8)
    flat[:data.size] = data
    for s in range(4):
        b.shards[s][:] = flat[s * S:(s + 1) * S]
    assert encode_blocks(rsgpu_lib, gpu, 4, 2, [b], HH) == 0
    assert [b.dig[32 * i: 32 * i + 32].tobytes().hex() for i in range(6)] == v["shard_hh256s"]


def _kinds(k, m, oracle):
    lens = (131072, KT + 1, 33, 1025, 87382, 17)
    kinds = [("packed", False), ("packed", True), ("separate", True)]
    blks = [Blk(k, m, S, *kinds[i % 3], seed=40 + i, pinned_digests=(i % 2 == 0) if kinds[i % 3][1] else False)
            for i, S in enumerate(lens)]
    for b in blks:
        b.reference(oracle)
    return blks


@pytest.mark.parametrize("zero_copy", ["0", "1"])
def test_memory_kinds(gpu, rsgpu_lib, oracle, zero_copy):
    """Pageable arrays, one page-locked buffer per block, separately
    page-locked shards: each kind alone and all three in one call, with and
    without digests, staged (RSG_ZERO_COPY=0) and in place."""
    from rustfs_amd import _lib
    k, m = 8, 4
    blks = _kinds(k, m, oracle)
    with _lib.tuned(RSG_ZERO_COPY=zero_copy):
        for algo in (NONE, HH):
            for group in (blks[0::3], blks[1::3], blks[2::3], blks):
                for b in group:
                    b.reset()
                assert encode_blocks(rsgpu_lib, gpu, k, m, group, algo) == 0
                for b in group:
                    b.check(oracle, algo, (zero_copy, algo))


def test_validation_errors_write_nothing(gpu, rsgpu_lib):
    from rustfs_amd import _lib
    k, m = 4, 2
    def fresh():
        return [Blk(k, m, S, "packed", False, seed=70 + i) for i, S in enumerate((100, 4097, 33))]

    def expect(blks, status, algo=HH, k_=k, m_=m):
        assert encode_blocks(rsgpu_lib, gpu, k_, m_, blks, algo) == status
        for b in blks:
            b.check_untouched()

    blks = fresh()
    for s in (0, k):  # a NULL data pointer, a NULL parity pointer, in the last block
        blks[2].ptrs[s] = None
        expect(blks, _lib.RSG_ERR_INVALID_ARG)
        blks[2].ptrs[s] = blks[2].shards[s].ctypes.data
    blks[1].S = 0
    expect(blks, _lib.RSG_ERR_EMPTY_SHARD)
    blks[1].S = 1 << 32
    expect(blks, _lib.RSG_ERR_INVALID_ARG)
    blks[1].S = 4097
    # parity of block 2 over one byte of block 0's data
    blks[2].ptrs[k] = blks[0].shards[0].ctypes.data + 99
    expect(blks, _lib.RSG_ERR_INVALID_ARG)
    expect(blks, _lib.RSG_ERR_INVALID_ARG, algo=NONE)
    blks[2].ptrs[k] = blks[2].shards[k].ctypes.data
    # digests of block 0 over parity of block 1: only with an algo
    keep = blks[0].dig
    blks[0].dig = blks[1].shards[k + 1][5:5 + 32 * (k + m)]
    expect(blks, _lib.RSG_ERR_INVALID_ARG)
    blks[0].dig = keep
    # geometry errors are rsg_encode's
    expect(blks, _lib.RSG_ERR_ZERO_PARITY_SHARDS, k_=4, m_=0)
    expect(blks, _lib.RSG_ERR_ZERO_DATA_SHARDS, k_=0, m_=2)
    expect(blks, _lib.RSG_ERR_INVALID_ARG, algo=9)
    assert rsgpu_lib.rsg_encode_blocks(gpu.handle, k, m, 0, None, HH) == 0
    assert rsgpu_lib.rsg_encode_blocks(gpu.handle, k, m, 2, None, HH) == _lib.RSG_ERR_INVALID_ARG


@pytest.mark.parametrize("S", [1, 33, KT + 1, 131072])
def test_encode_hashed(gpu, rsgpu_lib, oracle, S):
    """rsg_encode_hashed = rsg_encode, then the oracle's digests of all k+m
    shards."""
    k, m = 8, 4
    a, b = Blk(k, m, S, "packed", False, seed=S), Blk(k, m, S, "separate", False, seed=S)
    for s in range(k):
        b.shards[s][:] = a.shards[s]
    b.before = [x.copy() for x in b.arrays]
    assert rsgpu_lib.rsg_encode(gpu.handle, k, m, S, a.ptrs) == 0
    for algo in (HH, LEGACY):
        b.reset()
        assert rsgpu_lib.rsg_encode_hashed(gpu.handle, k, m, S, b.ptrs, b.dig.ctypes.data, algo) == 0
        b.check(oracle, algo)
        for r in range(m):
            assert (b.shards[k + r] == a.shards[k + r]).all()
        full = [a.shards[i] for i in range(k + m)]
        want = b"".join((oracle.hh256s if algo == HH else oracle.hh256s_legacy)(x) for x in full)
        assert b.dig.tobytes() == want
    from rustfs_amd import _lib
    assert rsgpu_lib.rsg_encode_hashed(gpu.handle, k, m, S, b.ptrs, None, HH) == _lib.RSG_ERR_INVALID_ARG


@pytest.mark.parametrize("k,m", [(5, 5), (17, 3)])
def test_other_geometries_fall_back(gpu, rsgpu_lib, oracle, k, m):
    blks = [Blk(k, m, S, lay, False, seed=90 + i, with_digests=(i != 1))
            for i, (S, lay) in enumerate(((1025, "packed"), (33, "separate"), (KT + 1, "packed")))]
    for algo in (HH, NONE):
        for b in blks:
            b.reset()
        assert encode_blocks(rsgpu_lib, gpu, k, m, blks, algo) == 0
        for b in blks:
            b.check(oracle, algo)


def test_block_larger_than_the_stage(gpu, rsgpu_lib, oracle):
    """RS(2,1) with 3 shards just over a third of the stage each: that block
    goes alone through the per-block path, its neighbours through the kernels."""
    from rustfs_amd import _lib
    k, m = 2, 1
    big = _lib.RSG_BLOCKS_STAGE_BYTES // 3 + 4096
    blks = [Blk(k, m, S, "packed", False, seed=95 + i) for i, S in enumerate((1025, big, 33))]
    assert encode_blocks(rsgpu_lib, gpu, k, m, blks, HH) == 0
    for b in blks:
        b.check(oracle, HH)


def test_python_surface(gpu, oracle):
    """Erasure.encode_blocks and ReedSolomonEncoder.encode_hashed."""
    from rustfs_amd import Erasure, ReedSolomonEncoder
    k, m = 4, 2
    blks = [Blk(k, m, S, "separate", False, seed=400 + i) for i, S in enumerate((33, KT + 1, 1025))]
    digs = [b.dig.reshape(k + m, 32) for b in blks]
    digs[1] = None
    blks[1].with_digests = False
    Erasure(k, m, 1 << 20).encode_blocks([b.shards for b in blks], digests=digs)
    for b in blks:
        b.check(oracle, HH)
        b.reset()
    Erasure(k, m, 1 << 20).encode_blocks([b.shards for b in blks])
    for b in blks:
        b.check(oracle, NONE)
        b.reset()
    d = ReedSolomonEncoder(k, m).encode_hashed(blks[0].shards)
    blks[0].check(oracle, NONE)
    assert d.tobytes() == blks[0].reference(oracle)[1][HH]
