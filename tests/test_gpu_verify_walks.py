"""The same-length verify-only record walks on the GPU, at every built shape:
k_verify_records_dma<NF> (NF = 1..15, the 3-slot and the 2-slot ring),
k_hh256_quad<0, DEPTH> (DEPTH 1..3) and its funnel form <0, 2, UNAL>, as the
in-place GET with every data file present (verify_data_begin, then
verify_parity_rest over a sub-range) and whole-file bitrot_verify launch them.

Every input is built on the host: seeded payloads, parity from the CPU oracle,
digests from oracle.hh256s (hh256s_legacy for one whole-file call), records
[digest][body].  Every shard file is a slice of one device tensor (an arena),
placed at a chosen residue mod 16 between random filler bytes, and the arena
is compared with its host copy after every call.  What a call must return
follows from how its input was built (which bytes were flipped, where a file
was cut) and, for whole files, from the host mirror bitrot.bitrot_verify over
the oracle hash — never from the library.

The parameter rows come from verify_shapes.py; test_verify_shapes.py proves on
the CPU that they reach every built shape."""
import io

import numpy as np
import pytest

import verify_shapes as V
from conftest import SLOT_FILL
from test_gpu_decode import engine_path  # noqa: F401  (both record engines)

pytestmark = pytest.mark.gpu

M = V.M
OK, TOO_FEW, MISMATCH, EOF, TRAILING = 0, 8, 11, 17, 18
_CASES = {}


def test_status_codes():
    from rustfs_amd import _lib
    assert (OK, TOO_FEW, MISMATCH, EOF, TRAILING) == (
        _lib.RSG_OK, _lib.RSG_ERR_TOO_FEW_SHARDS, _lib.RSG_ERR_BITROT_MISMATCH, _lib.RSG_ERR_UNEXPECTED_EOF,
        _lib.RSG_ERR_TRAILING_DATA)


def records(O, k, S, n):
    """(data (n, k, S), [k + M arrays (n, 32 + S)]: the shard files' records)
    of one seeded batch, built once and never modified."""
    key = (k, S, n)
    if key not in _CASES:
        rng = np.random.default_rng(1000003 * k + 1009 * S + n)
        shards = np.zeros((n, k + M, S), dtype=np.uint8)
        shards[:, :k] = rng.integers(0, 256, (n, k, S), dtype=np.uint8)
        files = [np.zeros((n, 32 + S), dtype=np.uint8) for _ in range(k + M)]
        for s in range(n):
            O.encode(k, M, shards[s])
            for i in range(k + M):
                files[i][s, :32] = np.frombuffer(O.hh256s(shards[s, i]), dtype=np.uint8)
                files[i][s, 32:] = shards[s, i]
        for a in [shards] + files:
            a.setflags(write=False)
        _CASES[key] = (shards[:, :k], files)
    return _CASES[key]


class GetCase:
    """One GET row's files in an arena: filler, the k + M record files at the
    row's residues, `rot` = [(file, stripe, offset in the record)] flipped."""

    def __init__(self, O, row, rot=()):
        self.row, self.rot = row, list(rot)
        self.data, files = records(O, row.k, row.S, row.n)
        self.offs, size = V.get_layout(row)
        self.rec = 32 + row.S
        host = np.random.default_rng(row.k * 7 + row.S).integers(0, 256, size, dtype=np.uint8)
        for o, f in zip(self.offs, files):
            host[o:o + f.size] = f.reshape(-1)
        for f, s, at in self.rot:
            host[self.offs[f] + s * self.rec + at] ^= 0x40
        self.host = host

    def flip_neighbours(self):
        """The filler byte before each file and the one after its last record."""
        for o in self.offs:
            self.host[o - 1] ^= 0xFF
            self.host[o + self.row.n * self.rec] ^= 0xFF
        return self

    def expect(self):
        """(status, src or None per stripe): a stripe with more than M rotten
        records has too few shards; elsewhere every rotten data record is
        rebuilt and every other one served from its record."""
        k, n = self.row.k, self.row.n
        bad = {}
        for f, s, _ in self.rot:
            bad.setdefault(s, set()).add(f)
        status = [TOO_FEW if len(bad.get(s, ())) > M else OK for s in range(n)]
        src = np.ones((k, n), dtype=bool)
        for s, fs in bad.items():
            for f in fs:
                if f < k:
                    src[f, s] = False
        return status, src

    def run(self, label=""):
        import torch
        from rustfs_amd import Erasure
        row, k, n, S = self.row, self.row.k, self.row.n, self.row.S
        arena = torch.from_numpy(self.host).cuda()
        assert arena.data_ptr() % 16 == 0
        files = [arena[o:o + n * self.rec] for o in self.offs]
        assert [f.data_ptr() % 16 for f in files] == V.residues(row.pattern, k) + list(V.PARITY_RESIDUES)
        slots = torch.full((n, k * S), SLOT_FILL, dtype=torch.uint8, device="cuda")
        _, src, status = Erasure(k, M, k * S).decode_records_into_batch(files, S, n, targets=slots)
        assert np.array_equal(arena.cpu().numpy(), self.host), "the arena was written"
        want_status, want_src = self.expect()
        where = (label, tuple(row))
        assert status == want_status, where
        got = slots.cpu().numpy().reshape(n, k, S)
        for s in range(n):
            if want_status[s] != OK:  # nothing to serve: what the slots hold is not specified
                continue
            assert np.array_equal(src[:, s], want_src[:, s]), (where, s, src[:, s].tolist())
            for f in range(k):
                if want_src[f, s]:
                    assert (got[s, f] == SLOT_FILL).all(), (where, "slot written though served", s, f)
                else:
                    assert np.array_equal(got[s, f], self.data[s, f]), (where, "rebuilt shard", s, f)
        return src, status


def too_few_rot(row):
    """M + 1 rotten records in the last stripe alone: data files first."""
    return [(f, row.n - 1, V.rot_spots(row.S)[f % len(V.rot_spots(row.S))]) for f in range(M + 1)]


GROUPS = ([("ring%d" % nf, V.ring_rows(nf)) for nf in range(1, V.MAX_RING + 1)]
          + [("quad-depth%d" % d, V.quad_rows(d)) for d in (1, 2, 3)] + [("funnel", V.unal_rows())])


def test_groups_are_the_sweep():
    assert [r for _, rows in GROUPS for r in rows] == V.get_rows()


@pytest.mark.parametrize("rows", [g[1] for g in GROUPS], ids=[g[0] for g in GROUPS])
def test_get_verdicts(gpu, oracle, engine_path, rows):
    """The in-place GET with every data file present, per row: a healthy batch
    (every record served, no slot byte written); the row's rotten records
    (exactly those rebuilt, into their slots; the parity check runs over the
    sub-range of the rotten stripes); M + 1 rotten records in the last stripe
    (that stripe alone has too few shards)."""
    from rustfs_amd import _lib
    for row in rows:
        with _lib.tuned(RSG_HASH_DEPTH=str(row.depth)):
            src, status = GetCase(oracle, row).run("healthy")
            assert src.all() and status == [OK] * row.n
            GetCase(oracle, row, V.get_rot(row)).run("rotten")
            _, status = GetCase(oracle, row, too_few_rot(row)).run("too few")
            assert status == [OK] * (row.n - 1) + [TOO_FEW]
        assert _lib.get_tuning("RSG_HASH_DEPTH") == "2"


@pytest.mark.parametrize("name", ["ring", "ring2", "quad", "unal"])
def test_neighbouring_bytes_do_not_count(gpu, oracle, name):
    """The byte before each file and the byte after its last record flipped:
    the same verdicts (the ragged last step's zero fill; the funnel's ninth
    word, which reaches past the record)."""
    row = V.NAMED[name]
    for rot in ([], V.get_rot(row)):
        a = GetCase(oracle, row, rot).run("as built")
        b = GetCase(oracle, row, rot).flip_neighbours().run("neighbours flipped")
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def all_rotten(row):
    return [(f, s, 3 + (f + s) % 29) for f in range(row.k + M) for s in range(row.n)]


def sub_range_rot(row, parity):
    """Data file 0 rotten in stripes 2 .. n - 3 (the parity check's range);
    with `parity`, both parity records of those stripes too."""
    stripes = range(2, row.n - 2)
    rot = [(0, s, 32 + s) for s in stripes]
    if parity:
        rot += [(row.k + j, s, 7 + j) for j in range(M) for s in stripes]
    return rot


@pytest.mark.parametrize("name", ["ring", "quad", "unal", "parity"])
def test_no_memory_between_calls(gpu, oracle, name):
    """One context, one stream, the same pooled scratch: every record rotten,
    then healthy, then rotten again; a healthy call of another record count
    after a rotten one, both ways.  Each call's result is its own: neither a
    flag the ring wrote nor one the quad kernel cleared in an earlier call
    shows in a later one.  "parity": the flags of the sub-range launch — both
    parity records of a range rotten (too few shards there), then the data
    record alone (rebuilt from parity whose flags the earlier call left 0)."""
    small, large = V.NAMED[name], V.LARGER[name]
    if name == "parity":
        rotten = lambda row: sub_range_rot(row, True)
        for row in (small, large):
            assert len(set(s for _, s, _ in rotten(row))) >= 2 and row.k + M - (M + 1) < row.k
    else:
        rotten = all_rotten
    seq = [(small, True), (small, False), (small, True), (large, False), (large, True), (small, False), (small, True)]
    for step, (row, bad) in enumerate(seq):
        src, status = GetCase(oracle, row, rotten(row) if bad else []).run("call %d" % step)
        if not bad:
            assert status == [OK] * row.n and src.all()
        elif name != "parity":
            assert status == [TOO_FEW] * row.n and not src.any()
        else:
            assert [s != OK for s in status] == [2 <= s < row.n - 2 for s in range(row.n)]
            GetCase(oracle, row, sub_range_rot(row, False)).run("call %d, then the data record alone" % step)


# -- whole files ---------------------------------------------------------------------------------

def whole_case(O, row, legacy):
    """[(outcome, bytes)] of a row's files, from one healthy file of seeded
    body bytes."""
    h = O.hh256s_legacy if legacy else O.hh256s
    part = np.random.default_rng(row.S * 31 + row.full).integers(0, 256, row.full * row.S + row.tail, dtype=np.uint8)
    pieces = []
    for at in range(0, part.size, row.S):
        pieces += [np.frombuffer(h(part[at:at + row.S]), dtype=np.uint8), part[at:at + row.S]]
    good = np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.uint8)
    assert good.size == V.whole_want(row)
    out = []
    for o, length, rot in V.whole_files(row):
        f = np.concatenate([good, np.full(max(0, length - good.size), 0x5C, dtype=np.uint8)])[:length].copy()
        if rot is not None:
            f[rot] ^= 0x40
        out.append((o, f))
    return out


@pytest.mark.parametrize("files,S,full,tail,pattern", [(5, 513, 3, 1, "six"), (16, 512, 3, 1, "zero"),
                                                       (16, 513, 3, 512, "mis8")], ids=["ring", "quad", "funnel"])
def test_whole_file_no_memory_between_calls(gpu, oracle, files, S, full, tail, pattern):
    """Whole-file verify on one context: every record of every file rotten,
    then the healthy files, then rotten again, then healthy files of one
    record fewer.  The per-record flags sit in the same pooled scratch each
    time; each call reports its own files."""
    import torch
    from rustfs_amd.bitrot import HashAlgorithm, bitrot_verify_batch
    for step, (nfull, bad) in enumerate([(full, True), (full, False), (full, True), (full - 1, False), (full, True),
                                         (full, False)]):
        row = V.WholeRow(files, S, nfull, tail, pattern, 2)
        picks = [p for _, p in V.whole_picks(row._replace(mix="full"))]
        want_kind = {"six": ("ring", False), "zero": ("quad", False), "mis8": ("quad", True)}[pattern]
        assert {(p.kind, p.unal) for p in picks} == {want_kind}  # every launch of the call is the named kernel
        good = whole_case(oracle, row._replace(files=1, mix="full"), False)[0][1]
        assert good.size == V.whole_want(row)
        f = good.copy()
        if bad:
            for r in range(nfull + 1):
                f[r * (32 + S) + 9] ^= 0x01  # a digest byte of every record
        offs, size = V.place([f.size] * files, V.residues(pattern, files))
        host = np.random.default_rng(step).integers(0, 256, size, dtype=np.uint8)
        for o in offs:
            host[o:o + f.size] = f
        arena = torch.from_numpy(host).cuda()
        status = bitrot_verify_batch([arena[o:o + f.size] for o in offs], f.size, nfull * S + tail,
                                     HashAlgorithm.HighwayHash256S, S)
        assert status == [MISMATCH if bad else OK] * files, (step, status)
        assert np.array_equal(arena.cpu().numpy(), host), "the arena was written"


IMPLIED = {"healthy": OK, "trailing": TRAILING, "empty": EOF, "short": EOF, "short_rot": MISMATCH, "cut_body": EOF,
           "cut_header": EOF, "cut_records": EOF, "rot_first": MISMATCH, "rot_middle": MISMATCH, "rot_last": MISMATCH,
           "rot_tail": MISMATCH}


@pytest.mark.parametrize("row", V.whole_rows(), ids=lambda r: "%dfiles-S%d-%s" % (r.files, r.S, r.mix))
def test_whole_file_verdicts(gpu, oracle, monkeypatch, row):
    """bitrot_verify_batch over 1..15, 16, 17, 32 and 33 files of one part in
    one call, outcomes mixed in list order: the status of every file is the
    host mirror's (bitrot.bitrot_verify over the oracle hash), and what its
    construction implies."""
    import torch
    from rustfs_amd import _lib
    from rustfs_amd.bitrot import HashAlgorithm, bitrot_verify, bitrot_verify_batch
    legacy = row.files == 7
    algo = HashAlgorithm.HighwayHash256SLegacy if legacy else HashAlgorithm.HighwayHash256S
    h = oracle.hh256s_legacy if legacy else oracle.hh256s
    files = whole_case(oracle, row, legacy)
    want, part = V.whole_want(row), row.full * row.S + row.tail
    # the host mirror's hash: the oracle, not the library
    monkeypatch.setattr(HashAlgorithm, "hash_encode", lambda self, data, device=None: h(np.frombuffer(bytes(data), np.uint8)))
    expect = []
    for o, f in files:
        try:
            bitrot_verify(io.BytesIO(f.tobytes()), want, part, algo, row.S)
            got = OK
        except EOFError:
            got = EOF
        except IOError as exc:
            got = {"bitrot hash mismatch": MISMATCH, "bitrot shard file has trailing data": TRAILING}[str(exc)]
        assert got == IMPLIED[o], (o, got)
        expect.append(got)
    offs, size = V.place([f.size for _, f in files], V.residues(row.pattern, row.files))
    host = np.random.default_rng(row.files).integers(0, 256, size, dtype=np.uint8)
    for o, (_, f) in zip(offs, files):
        host[o:o + f.size] = f
    arena = torch.from_numpy(host).cuda()
    assert arena.data_ptr() % 16 == 0
    with _lib.tuned(RSG_HASH_DEPTH=str(row.depth)):
        status = bitrot_verify_batch([arena[o:o + f.size] for o, (_, f) in zip(offs, files)], want, part, algo, row.S)
    assert np.array_equal(arena.cpu().numpy(), host), "the arena was written"
    wrong = [(i, files[i][0], s, w) for i, (s, w) in enumerate(zip(status, expect)) if s != w]
    assert not wrong, wrong
