"""Mixed-length batch deep scan on the GPU (rsg_bitrot_verify_mixed_dev /
_host, k_verify_mixed): whole-file verification of many shard files with
different part sizes, shard sizes, lengths and alignments in one call.  The
files are built from oracle digests (oracle.hh256s, oracle.hh256s_legacy) over
seeded bodies; the expected status of every file follows from how it was built
(what was flipped, cut or appended), never from the library's own output."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = 0xA5
HH, LEGACY, NONE = 1, 2, 0  # RSG_HASH_HIGHWAY256S, RSG_HASH_HIGHWAY256S_LEGACY, RSG_HASH_NONE
OK, INVALID, MISMATCH, DEVICE, UNSUPPORTED, SIZE, EOF, TRAILING = 0, 1, 11, 13, 15, 16, 17, 18
# the packet (32), the 8-packet batch (256) and the DEPTH = 2 and 3 pipeline fills (512, 768)
SHARD_SIZES = [1, 7, 8, 31, 32, 33, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1025, 87382]

_BODY, _FILE = {}, {}


def body(n):
    """The first n bytes of one seeded stream (shared, never modified)."""
    if "b" not in _BODY or _BODY["b"].size < n:
        b = np.random.default_rng(20261).integers(0, 256, max(n, 1 << 22), dtype=np.uint8)
        b.setflags(write=False)
        _BODY["b"] = b
    return _BODY["b"][:n]


def shard_file(O, part, shard, algo=HH):
    """The complete shard file of a part of `part` body bytes in records of
    `shard`: [oracle digest][bytes] per record, the last one short.  Built once
    per shape and shared, never modified."""
    key = (part, shard, algo)
    if key not in _FILE:
        h = O.hh256s if algo == HH else O.hh256s_legacy
        b = body(part)
        out = []
        for at in range(0, part, shard or 1):
            piece = b[at:at + shard]
            out += [np.frombuffer(h(piece), dtype=np.uint8), piece]
        f = np.concatenate(out) if out else np.zeros(0, dtype=np.uint8)
        f.setflags(write=False)
        _FILE[key] = f
    return _FILE[key]


class Batch:
    """Files packed into arenas of FILL: add() places a file's bytes at the
    next offset of its arena that is `res` mod 8 and records its descriptor
    and the status its construction implies."""

    def __init__(self, n_arenas):
        self.parts = [[] for _ in range(n_arenas)]
        self.at = [0] * n_arenas
        self.rows, self.want = [], []

    def add(self, data, want_size, part, shard, arena, expect, res=None):
        if res is not None:
            pad = (res - self.at[arena]) % 8
            self.parts[arena].append(np.full(pad, FILL, dtype=np.uint8))
            self.at[arena] += pad
        self.rows.append((self.at[arena], len(data), want_size, part, shard, arena))
        self.want.append(expect)
        self.parts[arena].append(np.asarray(data, dtype=np.uint8))
        self.at[arena] += len(data)
        return len(self.rows) - 1

    def arenas(self):
        return [np.concatenate(p + [np.full(3, FILL, dtype=np.uint8)]) for p in self.parts]

    def run_dev(self, algo=HH):
        import torch
        from rustfs_amd.bitrot import HashAlgorithm, bitrot_verify_many
        host = self.arenas()
        dev = [torch.from_numpy(a).cuda() for a in host]
        status = bitrot_verify_many(dev, self.rows, HashAlgorithm(algo))
        for a, d in zip(host, dev):
            assert np.array_equal(d.cpu().numpy(), a), "an arena was written"
        return status

    def check_dev(self, algo=HH):
        status = self.run_dev(algo)
        wrong = [(i, self.rows[i], s, w) for i, (s, w) in enumerate(zip(status, self.want)) if s != w]
        assert not wrong, wrong[:8]


def flipped(f, at):
    g = np.array(f)
    g[at] ^= 0x40
    return g


def test_smallest_launch(gpu, oracle):
    """One file of one 1-byte record: healthy, then with its only body byte
    flipped, then with a header byte flipped."""
    f = shard_file(oracle, 1, 1)
    assert f.size == 33
    for data, expect in ((f, OK), (flipped(f, 32), MISMATCH), (flipped(f, 0), MISMATCH)):
        b = Batch(1)
        b.add(data, 33, 1, 1, 0, expect)
        b.check_dev()


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_length_boundaries(gpu, oracle, depth):
    """Every boundary shard size with 0..3 full records and tails of 0, 1 and
    shard_size - 1, each shape at file offsets 0..7 mod 8, under every
    pipeline depth: all healthy in arena 0; in arena 1 the same files with the
    last byte of their last record flipped, which only that file's status
    shows (a part of 0 bytes has no record to flip)."""
    from rustfs_amd import _lib
    b = Batch(2)
    for S in SHARD_SIZES:
        shapes = sorted({full * S + tail for full in range(4) for tail in (0, 1, S - 1) if tail < S})
        for part in shapes:
            f = shard_file(oracle, part, S)
            for res in range(8):
                b.add(f, f.size, part, S, 0, OK, res)
                b.add(flipped(f, f.size - 1) if part else f, f.size, part, S, 1, MISMATCH if part else OK, res)
    with _lib.tuned(RSG_HASH_DEPTH=str(depth)):
        b.check_dev()
    assert _lib.get_tuning("RSG_HASH_DEPTH") == "2"


@pytest.mark.parametrize("units", [1, 15, 16, 17, 65])
def test_mixed_lengths_in_one_wave(gpu, oracle, units):
    """One-record files of very different lengths, interleaved over 3 arenas.
    From 15 units on, the sort by length puts a 1-byte and a >= 4 KiB record
    into the same wave (16 units); 1, 15, 17 and 65 units leave the last wave
    partly empty, 16 fill it (1 unit is the 1-byte record alone).  Every third
    file is rotten, so the statuses show that each verdict lands at its
    caller index."""
    small = [1, 33, 255, 7, 300]
    b = Batch(3)
    for i in range(units):
        n = small[(i // 13) % len(small)] if i % 13 == 0 else 4096 + 611 * i
        f = shard_file(oracle, n, n)
        bad = i % 3 == 1
        b.add(flipped(f, 32 + (n * 7 // 11)) if bad else f, f.size, n, n, i % 3, MISMATCH if bad else OK, res=(5 * i) % 8)
    lens = sorted((r[3] for r in b.rows), key=lambda n: -(n >> 8))  # the planner's order: stable, by 256-byte batches
    if units >= 15:  # the wave that holds the 1-byte record also holds a >= 4 KiB one
        w = lens.index(1) // 16
        assert lens[16 * w] >= 4096
    b.check_dev()


def test_rot(gpu, oracle):
    """One flipped byte in the header, the first body byte, the last byte of a
    whole packet (inside a batch, and of a single packet) or the remainder's
    last byte, in the first, a middle or the last record: only that file
    reports BITROT_MISMATCH, and two bad records give a single mismatch."""
    S, part = 300, 3 * 300 + 77  # 9 packets + 12 bytes per full record; the last record: 2 packets + 13 bytes
    rec = 32 + S
    f = shard_file(oracle, part, S)
    assert f.size == 3 * rec + 32 + 77
    b = Batch(3)
    i = 0
    b.add(f, f.size, part, S, 0, OK, res=3)
    for r, n in ((0, S), (1, S), (2, S), (3, 77)):
        spots = [5, 32, 32 + 31, 32 + n - 1]           # header, first body byte, a whole packet's end, the remainder's end
        spots += [32 + 255, 32 + 287] if n == S else [32 + 63]  # the batch's last byte, the single packet's last byte
        for at in spots:
            i += 1
            b.add(flipped(f, r * rec + at), f.size, part, S, i % 3, MISMATCH, res=i % 8)
            b.add(f, f.size, part, S, (i + 1) % 3, OK, res=(i + 3) % 8)
    two = flipped(flipped(f, 40), 3 * rec + 50)
    b.add(two, f.size, part, S, 0, MISMATCH)
    b.add(f, f.size, part, S, 0, OK)
    b.check_dev()


def test_decision_order(gpu, oracle):
    """bitrot_verify's order per file: size mismatch, then the first bad
    complete record, then early EOF, then trailing data."""
    S, part = 513, 2 * 513 + 100
    rec = 32 + S
    f = shard_file(oracle, part, S)
    want = f.size
    extra = np.concatenate([f, np.full(9, 7, dtype=np.uint8)])
    b = Batch(2)
    cut = 2 * rec + 32 + 50  # mid-body of the last record: records 0 and 1 are complete
    b.add(flipped(f, rec + 100)[:cut], want, part, S, 0, MISMATCH, res=1)  # rot before the cut
    b.add(f[:cut], want, part, S, 1, EOF, res=2)                           # the same file without rot
    b.add(flipped(f, 2 * rec + 40)[:cut], want, part, S, 0, EOF, res=3)    # rot only in the record the cut removes
    b.add(f[:rec], want, part, S, 1, EOF, res=4)                           # cut at a record boundary
    b.add(f[:rec + 7], want, part, S, 0, EOF, res=5)                       # ... mid-header
    b.add(f[:want - 1], want, part, S, 0, EOF, res=7)                      # the short last record incomplete
    b.add(flipped(f, want - 1)[:want - 1], want, part, S, 1, EOF)
    b.add(f[:0], want, part, S, 1, EOF)                                    # nothing there
    b.add(extra, want, part, S, 0, TRAILING, res=6)                        # longer
    b.add(flipped(extra, 2 * rec + 33), want, part, S, 1, MISMATCH, res=7)  # longer and rotten
    b.add(flipped(extra, want + 3), want, part, S, 1, TRAILING)            # the surplus bytes are not hashed
    b.add(f, want + 1, part, S, 0, SIZE)                                   # a wrong want_size ...
    b.add(flipped(f, 50), want - 32, part, S, 1, SIZE)                     # ... even when the bytes are rotten
    b.add(f, want, part - 1, S, 0, SIZE)
    assert -(-part // (S + 1)) == 3  # shard_size S + 1: the size still fits, the records are not where the digests are
    b.add(f, want, part, S + 1, 1, MISMATCH)
    b.add(f, want, part, 2 * S, 1, SIZE)
    b.add(f[:0], 0, 0, 0, 0, OK)                                           # an empty part
    b.add(f[:0], 0, 0, S, 1, OK)
    b.add(f[:5], 0, 0, 0, 0, TRAILING)                                     # part_size == 0 with a non-empty file
    b.add(f, want, part, S, 0, OK)
    b.check_dev()


def test_algorithms(gpu, oracle):
    """LEGACY accepts legacy digests and rejects plain ones (and the reverse);
    NONE checks sizes only; a whole-file algorithm is UNSUPPORTED."""
    from rustfs_amd import _lib
    S, part = 257, 600
    plain, legacy = shard_file(oracle, part, S, HH), shard_file(oracle, part, S, LEGACY)
    assert not np.array_equal(plain, legacy)
    for algo, good, other in ((LEGACY, legacy, plain), (HH, plain, legacy)):
        b = Batch(2)
        b.add(good, good.size, part, S, 0, OK, res=1)
        b.add(other, other.size, part, S, 1, MISMATCH, res=6)
        b.add(good[:100], good.size, part, S, 0, EOF)
        b.check_dev(algo)
    b = Batch(1)
    raw = np.array(body(part))
    b.add(raw, part, part, S, 0, OK, res=1)              # NONE: the file is the part
    b.add(flipped(plain, 40), plain.size, part, S, 0, SIZE)  # ... so a framed file is a size mismatch
    b.add(raw[:part - 1], part, part, S, 0, EOF)
    b.add(np.concatenate([raw, raw[:1]]), part, part, S, 0, TRAILING)
    b.add(raw[:0], 0, 0, 0, 0, OK)
    b.check_dev(NONE)
    arena = np.array(plain)
    desc = np.array([(0, plain.size, plain.size, part, S, 0)], dtype=np.dtype(list(_lib.FILE_DESC_FIELDS)))
    st = (ctypes.c_int * 1)(77)
    ap = (ctypes.c_void_p * 1)(arena.ctypes.data)
    lib = _lib.load()
    assert lib.rsg_bitrot_verify_mixed_host(gpu.handle, 3, 1, ap, 1, desc.ctypes.data, st) == UNSUPPORTED
    assert lib.rsg_bitrot_verify_mixed_dev(gpu.handle, 5, 1, ap, 1, desc.ctypes.data, st, None) == UNSUPPORTED
    assert st[0] == 77


def test_validation(gpu, oracle):
    """Each rejection is RSG_ERR_INVALID_ARG with the statuses left untouched,
    in both forms; n == 0 is RSG_OK."""
    import torch
    from rustfs_amd import _lib
    S, part = 100, 250
    f = shard_file(oracle, part, S)
    host = [np.concatenate([f, f]), np.array(f)]
    dev = [torch.from_numpy(a).cuda() for a in host]
    dt = np.dtype(list(_lib.FILE_DESC_FIELDS))
    good = [(0, f.size, f.size, part, S, 0), (0, f.size, f.size, part, S, 1), (f.size, f.size, f.size, part, S, 0),
            (0, 0, 0, 0, 0, 1)]
    lib = _lib.load()

    def call(form, rows, n_arenas=2, arenas="all", algo=HH, status=True, desc=True):
        d = np.array(rows, dtype=dt)
        ptrs = [a.ctypes.data for a in host] if form == "host" else [a.data_ptr() for a in dev]
        if arenas == "null1":
            ptrs[1] = None
        ap = (ctypes.c_void_p * len(ptrs))(*ptrs) if arenas != "none" else None
        st = (ctypes.c_int * len(rows))(*[77] * len(rows))
        args = [gpu.handle, algo, n_arenas, ap, len(rows), d.ctypes.data if desc else None, st if status else None]
        code = lib.rsg_bitrot_verify_mixed_host(*args) if form == "host" else lib.rsg_bitrot_verify_mixed_dev(*args, None)
        return code, list(st)

    def changed(j, field, value):
        rows = [list(r) for r in good]
        rows[j][field] = value
        return [tuple(r) for r in rows]

    for form in ("dev", "host"):
        assert call(form, good) == (OK, [OK] * 4)
        bad = [
            dict(rows=good, arenas="none"),                    # NULL pointers
            dict(rows=good, desc=False),
            dict(rows=good, status=False),
            dict(rows=good, algo=-1),                          # an unknown algo
            dict(rows=good, n_arenas=0),
            dict(rows=good, n_arenas=33),
            dict(rows=good, n_arenas=1),                       # arena >= n_arenas
            dict(rows=changed(3, 5, 2)),
            dict(rows=changed(3, 3, 1)),                       # shard_size == 0 with part_size > 0
            dict(rows=changed(0, 0, 2 ** 64 - 5)),             # a range that wraps
            dict(rows=changed(2, 0, f.size - 1)),              # ranges of one arena overlap
            dict(rows=[good[2], good[1], good[0], good[3]]),   # ... not ascending in list order
            dict(rows=good, arenas="null1"),                   # a non-empty file in a NULL arena
        ]
        for kw in bad:
            code, st = call(form, **kw)
            assert code == INVALID, kw
            assert st == [77] * 4, kw
        # a NULL arena may hold empty files; files of different arenas interleave freely
        assert call(form, [good[0], good[3], good[2]], arenas="null1") == (OK, [OK] * 3)
        assert call(form, [good[1], good[0], good[3], good[2]]) == (OK, [OK] * 4)
        st = (ctypes.c_int * 1)(77)
        ap = (ctypes.c_void_p * 2)(None, None)
        if form == "dev":
            assert lib.rsg_bitrot_verify_mixed_dev(gpu.handle, HH, 2, ap, 0, None, st, None) == OK
        else:
            assert lib.rsg_bitrot_verify_mixed_host(gpu.handle, HH, 2, ap, 0, None, st) == OK
        assert st[0] == 77
        # n == 0 wins over NULL pointers; the context, algo and n_arenas are still checked
        if form == "dev":
            assert lib.rsg_bitrot_verify_mixed_dev(gpu.handle, HH, 2, None, 0, None, None, None) == OK
            assert lib.rsg_bitrot_verify_mixed_dev(gpu.handle, HH, 0, None, 0, None, None, None) == INVALID
        else:
            assert lib.rsg_bitrot_verify_mixed_host(gpu.handle, HH, 2, None, 0, None, None) == OK
            assert lib.rsg_bitrot_verify_mixed_host(gpu.handle, -1, 2, None, 0, None, None) == INVALID


def test_offsets_past_4g(gpu, oracle):
    """Files at offsets past 4 GiB in a large uninitialised device buffer (only
    the files' ranges filled): 64-bit addressing end to end.  The rotten one
    shows that the bytes there are the ones hashed."""
    import torch
    from rustfs_amd.bitrot import bitrot_verify_many
    S, part = 1025, 3 * 1025 + 700
    f = shard_file(oracle, part, S)
    offs = [5, (1 << 32) + 9, (1 << 32) + 100003]
    datas = [f, f, flipped(f, 2 * (32 + S) + 600)]
    big = torch.empty((1 << 32) + (1 << 20), dtype=torch.uint8, device="cuda")
    for off, d in zip(offs, datas):
        big[off:off + d.size] = torch.from_numpy(np.array(d)).cuda()
    rows = [(off, f.size, f.size, part, S, 0) for off in offs]
    assert bitrot_verify_many([big], rows) == [OK, OK, MISMATCH]


def test_table_longer_than_one_launch(gpu, oracle):
    """A file of 2^20 + 5 one-byte records, more than one launch's table of
    the device form takes: healthy, then with the last record's body flipped
    (a unit of the second launch), a second file behind it in both."""
    n = (1 << 20) + 5
    b = body(n)
    dig = np.stack([np.frombuffer(oracle.hh256s(np.array([v], dtype=np.uint8)), dtype=np.uint8) for v in range(256)])
    f = np.concatenate([dig[b], b[:, None]], axis=1).reshape(-1)
    assert f.size == 33 * n
    g = shard_file(oracle, 1025, 513)
    for data, expect in ((f, OK), (flipped(f, f.size - 1), MISMATCH), (flipped(f, 33 * (1 << 19) + 7), MISMATCH)):
        bt = Batch(2)
        bt.add(data, f.size, n, 1, 0, expect, res=3)
        bt.add(g, g.size, 1025, 513, 1, OK, res=5)
        bt.check_dev()


@pytest.mark.parametrize("pinned", [True, False])
def test_host_form(gpu, oracle, pinned):
    """Pinned and pageable arenas.  A size-mismatch file, a file that ends 40
    bytes early, one cut inside its first record and one with surplus bytes
    are in the list before the sub-batches are counted with the planner's own
    cost rule (only what is read is staged: a file without a complete record
    and the bytes past want_size cost nothing), so the count is the library's:
    at least three, with a rotten file inside the middle one and inside the
    last one.  Then rsg_test_fail_subbatch(1) fails the call and is reset."""
    import torch
    from rustfs_amd import _lib
    from rustfs_amd._lib import RsgError
    from rustfs_amd.bitrot import bitrot_verify_many
    shapes = [(3 * 1048576 + 12345, 1048576), (87382, 87382), (700001, 174763), (0, 0), (2 * 349526 + 1, 349526)]
    b = Batch(3)
    for i in range(100):
        part, S = shapes[i % len(shapes)]
        f = shard_file(oracle, part, S)
        if i == 0:      # a wrong want_size: never read
            b.add(f, f.size + 32, part, S, i % 3, SIZE, res=0)
        elif i == 37:   # cut inside its first record: no complete record
            b.add(f[:20], f.size, part, S, i % 3, EOF, res=5)
        elif i == 40:   # surplus bytes, which are not read
            b.add(np.concatenate([f, np.full(70001, 9, dtype=np.uint8)]), f.size, part, S, i % 3, TRAILING, res=2)
        elif i == 80:   # the file ends 40 bytes early: its last record is incomplete
            b.add(f[:f.size - 40], f.size, part, S, i % 3, EOF, res=7)
        else:
            b.add(f, f.size, part, S, i % 3, OK, res=(3 * i) % 8)
    # the planner's split (rs_mixed_verify_plan.h): per touched arena the span
    # of what is read, the unit table, the flags
    rnd = lambda x: (x + 255) // 256 * 256

    def records(row):
        off, flen, want, part, S, arena = row
        if not part or want != part + 32 * -(-part // S):
            return 0
        full, rec, ln = part // S, 32 + S, min(flen, want)
        a = min(ln // rec, full)
        tail = part - full * S
        return a + 1 if a == full and tail and ln - full * rec >= 32 + tail else a

    def cost(a, z):
        lo, hi, units = {}, {}, 0
        for row in b.rows[a:z]:
            if not records(row):
                continue
            lo.setdefault(row[5], row[0])
            hi[row[5]] = row[0] + min(row[1], row[2])
            units += records(row)
        return sum(rnd(hi[x] - lo[x]) for x in lo) + rnd(16 * units) + rnd(units)
    subs, first = [], 0
    for j in range(len(b.rows) + 1):
        if j == len(b.rows) or (j > first and cost(first, j + 1) > _lib.RSG_MIXED_STAGE_BYTES):
            subs.append((first, j))
            first = j
    assert len(subs) >= 3, subs
    host = b.arenas()
    # a rotten file strictly inside the middle sub-batch and inside the last one
    for a, z in (subs[1], subs[-1]):
        j = next(j for j in range(a + 1, z - 1) if b.want[j] == OK and records(b.rows[j]) > 1)
        off, flen = b.rows[j][0], b.rows[j][1]
        host[b.rows[j][5]][off + flen // 2] ^= 1
        b.want[j] = MISMATCH
    assert [records(r) for r in (b.rows[0], b.rows[37], b.rows[40], b.rows[80])] == [0, 0, 4, 3]

    def mk(a):
        if not pinned:
            return a.copy()
        h = torch.empty(a.size, dtype=torch.uint8).pin_memory().numpy()
        h[:] = a
        return h
    arenas = [mk(a) for a in host]
    status = bitrot_verify_many(arenas, b.rows)
    for a, h in zip(arenas, host):
        assert np.array_equal(a, h), "an arena was written"
    assert status == b.want
    lib = _lib.load()
    assert lib.rsg_test_fail_subbatch(gpu.handle, 1) == OK
    try:
        with pytest.raises(RsgError) as err:
            bitrot_verify_many(arenas, b.rows)
        assert err.value.code == DEVICE
    finally:
        assert lib.rsg_test_fail_subbatch(gpu.handle, -1) == OK
    assert bitrot_verify_many(arenas, b.rows) == b.want


@pytest.mark.parametrize("k,m", [(4, 2), (12, 4)])
def test_loopback_verify_objects(gpu, oracle, tmp_path, k, m):
    """put_objects of 24 objects at 1 MiB blocks, then one shard file with a
    flipped byte, one truncated, one with a byte appended and one deleted:
    verify_objects gives the statuses this construction implies, and they equal
    the verify_object loop; a missing object raises, or is returned as an
    exception with return_exceptions."""
    from rustfs_amd.loopback import LocalErasureSet
    t, bs = k + m, 1 << 20
    dirs = [str(tmp_path / f"d{i}") for i in range(t)]
    for d in dirs:
        os.makedirs(d)
    s = LocalErasureSet(dirs, k, m, bs)
    sizes = [0, 1, k - 1, k, k + 1, 300 * 1024 + 7, 200 * 1024, 513 * 1024 + 1, bs - 1, bs, bs + 1, 2 * bs + 17]
    sizes = sizes + [x + 3 for x in sizes]
    assert len(sizes) == 24
    rng = np.random.default_rng(7 * k + m)
    names = [f"o{j}" for j in range(len(sizes))]
    s.put_objects([(n, rng.integers(0, 256, sz, dtype=np.uint8)) for n, sz in zip(names, sizes)])
    want = [[OK] * t for _ in names]

    def path(j, i):
        p = s.part_file(i, names[j])
        assert p is not None
        return p
    # a flipped byte in the middle of a multi-block object's shard file
    p = path(11, 1)
    raw = bytearray(open(p, "rb").read())
    raw[len(raw) // 2] ^= 0x10
    open(p, "wb").write(bytes(raw))
    want[11][1] = MISMATCH
    # ... and in the only body byte of a 1-byte object's first shard
    p = path(1, 0)
    raw = bytearray(open(p, "rb").read())
    assert len(raw) == 33
    raw[32] ^= 1
    open(p, "wb").write(bytes(raw))
    want[1][0] = MISMATCH
    # truncated by one byte, one byte appended, deleted
    p = path(5, t - 1)
    os.truncate(p, os.path.getsize(p) - 1)
    want[5][t - 1] = EOF
    p = path(9, 2)
    with open(p, "ab") as f:
        f.write(b"\0")
    want[9][2] = TRAILING
    p = path(0, 3)  # the empty object's empty file gets a byte too
    with open(p, "ab") as f:
        f.write(b"\0")
    want[0][3] = TRAILING
    os.unlink(path(7, 0))
    want[7][0] = EOF
    got = s.verify_objects(names)
    assert got == want
    assert got == [s.verify_object(n) for n in names]
    with pytest.raises(FileNotFoundError):
        s.verify_objects(names[:3] + ["nope"])
    r = s.verify_objects(["nope", names[11], "nope2"], return_exceptions=True)
    assert isinstance(r[0], FileNotFoundError) and isinstance(r[2], FileNotFoundError) and r[1] == want[11]
    assert s.verify_objects([]) == []
    s.close()
