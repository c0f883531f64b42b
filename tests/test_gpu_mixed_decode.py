"""Mixed-length batch GET on the GPU (rsg_decode_mixed_dev / _host,
k_decode_mixed): verify-before-use and rebuild of n record stripes with
different shard lengths, present sets and rot, always against oracle-built
records (oracle.encode, oracle.hh256s, oracle.hh256s_legacy) and the original
data, never against the library's own output."""
import os
import shutil

import numpy as np
import pytest

from mixed_shapes import SMALL_PERM, get_cases, sweep_params, plan_get, popcount, settle

pytestmark = pytest.mark.gpu

FILL = 0xA5
LENGTHS = [0, 1, 7, 8, 31, 32, 33, 511, 512, 513, 1023, 1024, 1025, 87382]
GEOMETRIES = [(2, 2), (3, 1), (4, 2), (5, 3), (8, 4), (12, 4), (16, 4)]
HH, LEGACY = 1, 2  # RSG_HASH_HIGHWAY256S, RSG_HASH_HIGHWAY256S_LEGACY
OK, TOO_FEW, INCONSISTENT, INVALID = 0, 8, 10, 1

_REF = {}


def spw_for(t):
    """Stripes per workgroup of the kernel for t rows (rs_mixed_decode_plan.h decode_spw_for over rs_fused.h fused_spw_for)."""
    return 2 if t >= 20 else 1 if t % 16 == 0 else 2 if t % 8 == 0 else 4 if (t % 4 == 0 or t <= 6) else 2


def ref_stripe(O, k, m, S):
    """Oracle stripe of shard length S: ((k+m, S) shards, {algo: [k+m digests]});
    computed once per (k, m, S) and shared, never modified."""
    key = (k, m, S)
    if key not in _REF:
        st = np.zeros((k + m, S), dtype=np.uint8)
        st[:k] = np.random.default_rng(104729 * k + 37 * m + S).integers(0, 256, (k, S), dtype=np.uint8)
        if m and S:
            O.encode(k, m, st)
        st.setflags(write=False)
        digs = {HH: [O.hh256s(st[i]) for i in range(k + m)], LEGACY: [O.hh256s_legacy(st[i]) for i in range(k + m)]}
        _REF[key] = (st, digs)
    return _REF[key]


def bits(idx):
    v = 0
    for i in idx:
        v |= 1 << i
    return v


class Recs:
    """n stripes of the given lengths as [digest][shard] records at odd
    rec_off with 1-3 byte gaps in k+m arenas, out windows at odd out_off with
    the same kind of gaps; the gaps, 64 bytes after each arena and the whole
    out arena hold FILL.  absent[j]: shards whose present bit is cleared."""

    def __init__(self, O, k, m, lens, algo=HH, absent=None, seed=0):
        self.O, self.k, self.m, self.t, self.n, self.lens, self.algo = O, k, m, k + m, len(lens), list(lens), algo
        rng = np.random.default_rng(seed)
        self.absent = [set(a) for a in (absent or [()] * self.n)]
        self.rec_off, self.out_off = [], []
        r, o = 1, 3
        for S in lens:
            self.rec_off.append(r)
            self.out_off.append(o)
            r += 32 + S + int(rng.integers(1, 4))
            o += k * S + int(rng.integers(1, 4))
        self.files = [np.full(r + 64, FILL, dtype=np.uint8) for _ in range(self.t)]
        self.out_len = o + 64
        for j, S in enumerate(lens):
            st, digs = ref_stripe(O, k, m, S)
            for i in range(self.t):
                a, r0 = self.files[i], self.rec_off[j]
                a[r0:r0 + 32] = np.frombuffer(digs[algo][i], dtype=np.uint8)
                a[r0 + 32:r0 + 32 + S] = st[i]
        self.null = set()  # arenas passed as NULL

    def desc(self):
        all_bits = (1 << self.t) - 1
        return [[self.rec_off[j], self.out_off[j], self.lens[j], all_bits & ~bits(self.absent[j])]
                for j in range(self.n)]

    def flip(self, j, shard, at):
        """Flip one byte of stripe j's record of `shard`: at < 0 in the header
        (32 + at), else in the body."""
        self.files[shard][self.rec_off[j] + 32 + at] ^= 0x40

    def rewrite(self, j, shard):
        """Alter the body of stripe j's record of `shard` and re-hash its header."""
        r0, S = self.rec_off[j], self.lens[j]
        body = self.files[shard][r0 + 32:r0 + 32 + S]
        body[S // 2] ^= 0x01
        h = self.O.hh256s(body) if self.algo == HH else self.O.hh256s_legacy(body)
        self.files[shard][r0:r0 + 32] = np.frombuffer(h, dtype=np.uint8)

    def run_dev(self, verify_surplus=True):
        import torch
        from rustfs_amd import Erasure
        e = Erasure(self.k, self.m, 1 << 20)
        files = [None if i in self.null else torch.from_numpy(self.files[i].copy()).cuda() for i in range(self.t)]
        out = torch.full((self.out_len,), FILL, dtype=torch.uint8, device="cuda")
        status, served = e.decode_mixed(files, self.desc(), out, verify_surplus, self.algo)
        torch.cuda.synchronize()
        for i, f in enumerate(files):
            assert f is None or np.array_equal(f.cpu().numpy(), self.files[i]), f"arena {i} changed"
        return status, served, out.cpu().numpy()

    def check(self, res, lost, failed=None):
        """lost[j]: the data shards of stripe j that must have been rebuilt
        (default: those absent); failed: {stripe: status}.  Rebuilt windows
        hold the original data, served bits are the rest, and every other
        byte of out holds FILL.  The windows of a failed stripe's absent data
        shards are unspecified, and so are those of the data shards lost[j]
        names for it: the ones the case made rotten, which count as absent
        from the round that finds them and are written before the verdict."""
        status, served, out = res
        failed = failed or {}
        k = self.k
        want = np.full(self.out_len, FILL, dtype=np.uint8)
        skip = np.zeros(self.out_len, dtype=bool)
        for j, S in enumerate(self.lens):
            assert status[j] == failed.get(j, OK), f"status of stripe {j} (len {S}): {status[j]}"
            o0 = self.out_off[j]
            if j in failed:
                for c in range(k):
                    if c in self.absent[j] or c in self.null or c in lost.get(j, ()):
                        skip[o0 + c * S:o0 + (c + 1) * S] = True
                continue
            gone = set(lost.get(j, [c for c in range(k) if c in self.absent[j] or c in self.null]))
            assert served[j] == bits(range(k)) & ~bits(gone), f"served bits of stripe {j}: {served[j]:#x}"
            st, _ = ref_stripe(self.O, k, self.m, S)
            for c in gone:
                want[o0 + c * S:o0 + (c + 1) * S] = st[c]
        bad = np.flatnonzero((out != want) & ~skip)
        assert bad.size == 0, f"out differs at {bad[:8]} (rebuilt windows = data, all else {FILL:#x})"


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


def absent_for(k, m, kind):
    if kind == "all":
        return ()
    if kind == "one":
        return (min(1, k - 1),)
    gone = (0, 2 if k > 2 else 1)[:min(m, 2)]  # min(m, 2) data shards, and a parity shard where m >= 3
    return gone + ((k + 1,) if m >= 3 else ())


# -- 1 -----------------------------------------------------------------------------

def test_smallest_launch(gpu, oracle):
    """n = 1, RS(4,2), S = 1025, data shard 1 absent."""
    b = Recs(oracle, 4, 2, [1025], absent=[(1,)])
    b.check(b.run_dev(), {})


# -- 2 -----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["all", "one", "more"])
@pytest.mark.parametrize("k,m", GEOMETRIES)
def test_lengths(gpu, oracle, k, m, kind):
    """Every length class in one batch, three orders, three masks per
    geometry; both hash keys on RS(4,2)."""
    gone = absent_for(k, m, kind)
    for how in ("ascending", "descending", "alternating"):
        lens = ordered(LENGTHS, how)
        for algo in ((HH, LEGACY) if (k, m) == (4, 2) else (HH,)):
            b = Recs(oracle, k, m, lens, algo, absent=[gone] * len(lens))
            b.check(b.run_dev(), {})


@pytest.mark.parametrize("C,R", sweep_params(0))
def test_every_shape(gpu, oracle, C, R):
    """Instantiation <C, R> of the kernel, every one of them, over the small
    length set (mixed_shapes.py): (C, 0, 0) with all present, and every
    (C, R, e) as geometry (C, R) with e data shards absent in every stripe and
    verify_surplus on, once the lowest e (sources are not the data prefix) and
    once the highest e (lost[] takes large values).  Rebuilt windows hold the
    data, served bits are right, every other byte of out holds FILL, the
    arenas are unchanged.  The union over the parameters is every
    reachable shape (test_mixed_shapes.py)."""
    for k, m, absent, shape in get_cases(C, R):
        plan = plan_get(k, m, (1 << (k + m)) - 1 & ~bits(absent), True)
        assert (k, len(plan[1]) + len(plan[2]), len(plan[1])) == shape, (k, m, absent)
        b = Recs(oracle, k, m, SMALL_PERM, absent=[absent] * len(SMALL_PERM), seed=m)
        try:
            b.check(b.run_dev(), {})
        except AssertionError as err:
            raise AssertionError(f"shape {shape}, RS({k},{m}), absent {absent}: {err}") from err


def test_null_arena_is_absent_whatever_present_says(gpu, oracle):
    b = Recs(oracle, 8, 4, [513, 0, 87382, 7])
    b.null = {2, 9}
    b.check(b.run_dev(), {})


# -- 3 -----------------------------------------------------------------------------

@pytest.mark.parametrize("gone", [(), (1,)])
@pytest.mark.parametrize("k,m", [(4, 2), (8, 4), (12, 4)])
def test_degenerate_batches(gpu, oracle, k, m, gone):
    spw = spw_for(k + m if gone else k)
    for lens in ([1025] + [0] * spw, [0] * (2 * spw + 1), [0]):
        b = Recs(oracle, k, m, lens, absent=[gone] * len(lens))
        b.check(b.run_dev(), {})


# -- 4 -----------------------------------------------------------------------------

def test_mixed_masks_land_at_caller_indices(gpu, oracle):
    """Three masks interleaved into groups of 1, SPW and SPW+1 stripes, in a
    caller order that differs from the kernel order (lengths not sorted)."""
    k, m = 8, 4
    spw = spw_for(k + m)
    A, B, C = (), (1,), (0, 2, 11)
    absent = []
    for i in range(spw + 1):
        absent.append(B)
        if i < spw:
            absent.append(C)
        if i == 1:
            absent.append(A)
    lens = [(33, 1025, 0, 513, 7, 87382, 512, 1, 1023, 8)[i % 10] for i in range(len(absent))]
    b = Recs(oracle, k, m, lens, absent=absent)
    b.check(b.run_dev(), {})


# -- 5 -----------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(8, 4), (5, 3)])
def test_rot_found_during_the_read(gpu, oracle, k, m):
    """Rot that only the read finds: each rotten stripe between clean
    neighbours, every stripe RSG_OK with the right bytes and served bits."""
    lens, absent, rots, lost = [], [], [], {}
    for S in (7, 513, 1025, 32):
        for what in ("body", "header", "source-parity", "surplus-parity"):
            j = len(lens)
            degraded = what.endswith("parity")
            lens += [S, S]  # the rotten stripe, then a clean neighbour
            absent += [(0,) if degraded else (), (0,) if degraded else ()]
            if what == "body":
                rots.append((j, 2, S - 1))
                lost[j] = [2]
            elif what == "header":
                rots.append((j, k - 1, -5))
                lost[j] = [k - 1]
            elif what == "source-parity":  # sources: data 1..k-1 and parity k
                rots.append((j, k, S // 2))
            else:
                rots.append((j, k + m - 1, 0))
    b = Recs(oracle, k, m, lens, absent=absent)
    for j, shard, at in rots:
        b.flip(j, shard, at)
    b.check(b.run_dev(), lost)


# -- 5b: redo cascades ---------------------------------------------------------------
#
# More than two rounds: state that lives on the device across rounds (the
# mismatch words, the flags by kernel row, the table region, out windows
# written from a source that later proves rotten).  The round count is not
# observable through the ABI; what is expected of each stripe comes from the
# planner rule restated in mixed_shapes.settle, whose round counts are asserted
# here against literal figures, so a case that stops reaching the depth it was
# written for fails.

class Cascade:
    """Stripes of lengths 7, 33, 513 and 1025 for every case (absent, rotten,
    rewritten), each followed by a clean neighbour of the same length: the
    shards of `rotten` get one byte flipped (header and body in turn),
    those of `rewritten` a valid digest over a wrong body.  From the model:
    the final masks, the rounds, lost[j] (the data shards outside the final
    mask) and failed (TOO_FEW: fewer than k left; INCONSISTENT: a rewritten
    record among the last plan's surplus)."""

    def __init__(self, O, k, m, cases, verify_surplus, lens=(7, 33, 513, 1025)):
        specs = []
        for S in lens:
            for case in cases:
                specs += [(S,) + tuple(case), (S, (), (), ())]
        self.b = Recs(O, k, m, [s[0] for s in specs], absent=[s[1] for s in specs], seed=k)
        self.vs, self.lost, self.failed, self.rounds, self.final, self.shapes = verify_surplus, {}, {}, [], [], []
        for j, (S, absent, rotten, rewritten) in enumerate(specs):
            for i, shard in enumerate(rotten):
                self.b.flip(j, shard, (S - 1, -5, S // 2, -32)[(j // 2 + i) % 4])
            for shard in rewritten:
                self.b.rewrite(j, shard)
            final, rounds, shapes = settle(k, m, (1 << (k + m)) - 1 & ~bits(absent), bits(rotten), verify_surplus)
            self.final.append(final)
            self.rounds.append(rounds)
            self.shapes.append(shapes)
            self.lost[j] = [c for c in range(k) if not final >> c & 1]
            if popcount(final) < k:
                self.failed[j] = TOO_FEW
            else:
                src, _, surplus = plan_get(k, m, final, verify_surplus)
                assert not set(rewritten) & set(src)  # a wrong body under a valid digest is only ever compared
                if set(rewritten) & set(surplus):
                    self.failed[j] = INCONSISTENT
        self.per_case = len(cases)

    def of_case(self, values):
        """values of the rotten stripes, per case (the same for every length)."""
        rows = [values[a:a + 2 * self.per_case:2] for a in range(0, len(values), 2 * self.per_case)]
        assert all(r == rows[0] for r in rows)
        return rows[0]

    def status_of_case(self):
        return self.of_case([self.failed.get(j, OK) for j in range(self.b.n)])

    def check_dev(self):
        res = self.b.run_dev(self.vs)
        self.b.check(res, self.lost, self.failed)
        return res


def ladder_cases(k):
    """Data shard 2 rotten (found in round 1, which reads the data shards
    only) and the parity shards k+i of each set rotten; then data shard 2
    absent from the start, which ends on the same masks one round sooner."""
    sets = [(), (0,), (0, 1), (0, 1, 2), (0, 1, 2, 3), (1, 2, 3), (1,)]
    cases = [((), (2,) + tuple(k + i for i in p), ()) for p in sets]
    return cases + [((2,), (), ()), ((2,), (k,), ()), ((2,), (k, k + 1, k + 2), ())]


# rounds of ladder_cases, m = 4, for any k >= 3 (those of RS(5,4) are CHECKed
# against the shipped planner in tests/host/mixed_decode_plan_main.cpp); the
# fifth case ends with k - 1 shards
LADDER_ROUNDS = {False: [2, 3, 4, 5, 5, 2, 2, 1, 2, 4], True: [2, 3, 3, 3, 2, 3, 3, 1, 2, 2]}
LADDER_STATUS = [OK, OK, OK, OK, TOO_FEW, OK, OK, OK, OK, OK]


def ladder(O, k, verify_surplus):
    c = Cascade(O, k, 4, ladder_cases(k), verify_surplus)
    assert c.of_case(c.rounds) == LADDER_ROUNDS[verify_surplus]
    assert c.status_of_case() == LADDER_STATUS
    assert c.rounds[1::2] == [1] * (c.b.n // 2)  # the clean neighbours
    final = c.of_case(c.final)
    assert final[1] == final[8] and c.of_case(c.rounds)[1] > c.of_case(c.rounds)[8]  # one mask, reached in different rounds
    if not verify_surplus:
        assert c.of_case(c.shapes)[3][1:] == [(k, 1, 1)] * 4
        assert final[5] == (1 << (k + 4)) - 1 & ~(1 << 2)  # parity k+1 onwards is never read
    else:
        assert c.of_case(c.shapes)[1][1:] == [(k, 4, 1), (k, 3, 1)]
        assert final[5] == bits(range(k + 1)) & ~(1 << 2)  # a rotten surplus leaves the mask too
    return c


@pytest.mark.parametrize("verify_surplus", [False, True])
@pytest.mark.parametrize("k", [5, 8])
def test_redo_ladder(gpu, oracle, k, verify_surplus):
    """Stripes that need one to five rounds in one batch, each beside a clean
    neighbour of its workgroup: every stripe RSG_OK with the data in the
    rebuilt window (written in an early round from a source that later proved
    rotten, and again) except the one left with k - 1 shards; all other out
    bytes FILL."""
    ladder(oracle, k, verify_surplus).check_dev()


@pytest.mark.parametrize("verify_surplus", [False, True])
def test_redo_ladder_host_form(gpu, oracle, verify_surplus):
    """The RS(5,4) ladder through rsg_decode_mixed_host (one sub-batch): the
    device form's statuses, served bits and bytes; the copy-back goes by the
    final masks, so h_out is untouched outside the rebuilt windows of good
    stripes, the failed stripe's windows included."""
    from rustfs_amd import Erasure
    c = ladder(oracle, 5, verify_surplus)
    b = c.b
    files = [f.copy() for f in b.files]
    out = np.full(b.out_len, FILL, dtype=np.uint8)
    status, served = Erasure(5, 4, 1 << 20).decode_mixed_host(files, b.desc(), out, verify_surplus)
    for i in range(b.t):
        assert np.array_equal(files[i], b.files[i]), f"arena {i} changed"
    b.check((status, served, out), c.lost, c.failed)
    dev = c.check_dev()
    assert dev[0] == status
    same = np.ones(b.out_len, dtype=bool)
    for j in c.failed:
        o0, S = b.out_off[j], b.lens[j]
        assert (out[o0:o0 + b.k * S] == FILL).all(), f"h_out of failed stripe {j} written"
        same[o0:o0 + b.k * S] = False  # the device form's windows of a failed stripe are unspecified
    assert [s for j, s in enumerate(served) if j not in c.failed] == [s for j, s in enumerate(dev[1]) if j not in c.failed]
    assert np.array_equal(out[same], dev[2][same])


def test_mismatch_word_across_rounds(gpu, oracle):
    """A stripe's mismatch word is set in one round and must not decide a
    later one.  RS(4,2): (a) data 0 absent, surplus parity 5 flipped: round 1
    compares good sources with a rotten surplus, round 2 is (4,1,1) with no
    compared row, RSG_OK; (b) the same plus source parity 4 flipped: TOO_FEW,
    not INCONSISTENT.  RS(5,3): (c) data 2 flipped and surplus 6 rewritten
    (valid digest, wrong body): INCONSISTENT, from round 2 (the rewritten
    record verifies, so the model gives two rounds); (c') data 2 and source
    parity 5 flipped, surplus 7 rewritten: round 2 compares against garbage,
    round 3 finds the real mismatch, INCONSISTENT after three rounds; (d) data
    0 absent and source parity 5 flipped: round 1 computed from garbage, set
    the word and wrote the window, round 2 leaves RSG_OK and the data."""
    a = Cascade(oracle, 4, 2, [((0,), (5,), ()), ((0,), (4, 5), ())], True)
    assert a.of_case(a.rounds) == [2, 1] and a.status_of_case() == [OK, TOO_FEW]
    assert a.of_case(a.shapes)[0] == [(4, 2, 1), (4, 1, 1)]
    a.check_dev()
    c = Cascade(oracle, 5, 3, [((), (2,), (6,)), ((), (2, 5), (7,)), ((0,), (5,), ())], True)
    assert c.of_case(c.rounds) == [2, 3, 2] and c.status_of_case() == [INCONSISTENT, INCONSISTENT, OK]
    assert c.of_case(c.shapes) == [[(5, 0, 0), (5, 3, 1)], [(5, 0, 0), (5, 3, 1), (5, 2, 1)], [(5, 3, 1), (5, 2, 1)]]
    c.check_dev()
    # without verify_surplus nothing is compared: the rewritten records are never read
    d = Cascade(oracle, 5, 3, [((), (2,), (6,)), ((), (2, 5), (7,)), ((0,), (5,), ())], False)
    assert d.of_case(d.rounds) == [2, 3, 2] and d.status_of_case() == [OK, OK, OK]
    d.check_dev()


# -- 6 -----------------------------------------------------------------------------

def test_statuses(gpu, oracle):
    k, m = 4, 2
    lens = [513, 1025, 700, 513, 7, 1025, 33]
    absent = [(), (0, 5), (1, 2, 4), (0, 3), (), (0,), ()]
    b = Recs(oracle, k, m, lens, absent=absent)
    b.flip(3, 4, 100)   # k valid by mask, one of them rotten: k - 1
    b.rewrite(5, 5)     # a surplus parity that verifies but does not fit the sources
    # stripe 1: exactly k valid; 2: k - 1 by mask; 3: k - 1 by rot; 5: inconsistent
    b.check(b.run_dev(True), {}, failed={2: TOO_FEW, 3: TOO_FEW, 5: INCONSISTENT})
    b.check(b.run_dev(False), {}, failed={2: TOO_FEW, 3: TOO_FEW})


# -- 7 -----------------------------------------------------------------------------

def test_m0_only_verifies(gpu, oracle):
    b = Recs(oracle, 5, 0, [0, 1, 513, 1025, 87382, 33])
    b.flip(3, 2, 7)
    b.absent[5] = {4}
    b.check(b.run_dev(), {}, failed={3: TOO_FEW, 5: TOO_FEW})


@pytest.mark.parametrize("k,m", [(10, 6), (17, 3)])
def test_fallback_geometries(gpu, oracle, k, m):
    """m > 4 and k > 16: the same results through the per-length engine."""
    lens = [1, 33, 513, 0, 1025, 700, 513]
    absent = [(), (1,), (0, 2, k + 1), (), (), tuple(range(m + 1)), ()]
    b = Recs(oracle, k, m, lens, absent=absent)
    b.flip(4, 3, 100)
    b.check(b.run_dev(), {4: [3]}, failed={5: TOO_FEW})


# -- 8 -----------------------------------------------------------------------------

def test_offsets_past_4g(gpu, oracle):
    """One stripe with rec_off and one with out_off past 4 GiB (large
    uninitialised device buffers, only the stripes' ranges filled and read
    back): 64-bit addressing end to end."""
    import torch
    from rustfs_amd import Erasure
    k, m, t = 4, 2, 6
    lens = [1025, 700, 513]
    recs = [5, (1 << 31) + 7, (1 << 32) + 9]
    outs = [(1 << 31) - 1, (1 << 32) + 3, (1 << 32) + 8191]
    gone = [(1,), (0, 3), (2,)]
    pitch = 8192  # arena i begins i*pitch into the one buffer: records of different shards never meet
    big = torch.empty((1 << 32) + (1 << 20), dtype=torch.uint8, device="cuda")
    out = torch.empty((1 << 32) + (1 << 16), dtype=torch.uint8, device="cuda")
    files = [big[i * pitch:] for i in range(t)]
    for j, S in enumerate(lens):
        st, digs = ref_stripe(oracle, k, m, S)
        for i in range(t):
            rec = np.concatenate([np.frombuffer(digs[HH][i], dtype=np.uint8), st[i]])
            files[i][recs[j]:recs[j] + 32 + S] = torch.from_numpy(rec).cuda()
        out[outs[j] - 8:outs[j] + k * S + 8] = FILL
    desc = [[recs[j], outs[j], lens[j], 0x3f & ~bits(gone[j])] for j in range(3)]
    status, served = Erasure(k, m, 1 << 20).decode_mixed(files, desc, out)
    assert status == [OK] * 3
    for j, S in enumerate(lens):
        st, _ = ref_stripe(oracle, k, m, S)
        assert served[j] == 0xf & ~bits(gone[j])
        got = out[outs[j] - 8:outs[j] + k * S + 8].cpu().numpy()
        want = np.full(k * S + 16, FILL, dtype=np.uint8)
        for c in gone[j]:
            want[8 + c * S:8 + (c + 1) * S] = st[c]
        assert np.array_equal(got, want), f"out window of stripe {j}"


# -- 9 -----------------------------------------------------------------------------

@pytest.mark.parametrize("pinned", [True, False])
def test_host_form(gpu, oracle, pinned):
    """Pinned and pageable arenas, a batch of three sub-batches with a rotten
    record in the middle one: the device form's results, h_out untouched
    outside the rebuilt windows."""
    import torch
    from rustfs_amd import Erasure, _lib
    k, m, t = 4, 2, 6
    lens = [350001, 87382, 0, 400000, 513] * 9
    absent = [(1,) if j % 3 == 0 else () for j in range(len(lens))]
    b = Recs(oracle, k, m, lens, absent=absent)
    # the planner's split: T record spans + the out span per sub-batch
    rnd = lambda x: (x + 255) // 256 * 256
    subs, first = [], 0
    for j in range(b.n + 1):
        def cost(a, z):
            outs = [i for i in range(a, z) if lens[i]]
            ospan = b.out_off[outs[-1]] + k * lens[outs[-1]] - b.out_off[outs[0]] if outs else 0
            return t * rnd(b.rec_off[z - 1] + 32 + lens[z - 1] - b.rec_off[a]) + rnd(ospan)
        if j == b.n or (j > first and cost(first, j + 1) > _lib.RSG_MIXED_STAGE_BYTES):
            subs.append((first, j))
            first = j
    assert len(subs) >= 3, subs
    mid = next(j for j in range(*subs[1]) if lens[j] > 1000)
    b.flip(mid, 0, lens[mid] // 2)
    lost = {mid: sorted(set(absent[mid]) | {0})}

    def mk(a):
        if not pinned:
            return a.copy()
        h = torch.empty(a.size, dtype=torch.uint8).pin_memory().numpy()
        h[:] = a
        return h
    files = [mk(f) for f in b.files]
    out = mk(np.full(b.out_len, FILL, dtype=np.uint8))
    status, served = Erasure(k, m, 1 << 20).decode_mixed_host(files, b.desc(), out)
    for i in range(t):
        assert np.array_equal(files[i], b.files[i]), f"arena {i} changed"
    b.check((status, served, out), lost)
    dev = b.run_dev()
    assert (dev[0], dev[1]) == (status, served) and np.array_equal(dev[2], out)


# -- 10 ----------------------------------------------------------------------------

def test_validation(gpu, oracle):
    """Each rejection is RSG_ERR_INVALID_ARG and out still holds its fill."""
    import torch
    from rustfs_amd import Erasure
    from rustfs_amd._lib import RsgError
    k, m = 4, 2
    b = Recs(oracle, k, m, [513, 33, 0, 1025])
    e = Erasure(k, m, 1 << 20)
    files = [torch.from_numpy(f.copy()).cuda() for f in b.files]
    out = torch.full((b.out_len,), FILL, dtype=torch.uint8, device="cuda")
    good = b.desc()

    def changed(j, field, value):
        d = [list(r) for r in good]
        d[j][field] = value
        return d
    bad = [
        changed(1, 3, 1 << 6),                           # a present bit at k+m
        changed(1, 0, good[0][0] + 31),                  # record ranges overlap
        changed(3, 0, good[0][0]),                       # ... not ascending
        changed(1, 1, good[0][1] + k * 513 - 1),         # out ranges overlap
        changed(3, 1, good[0][1]),                       # ... not ascending
    ]
    for d in bad:
        with pytest.raises(RsgError) as err:
            e.decode_mixed(files, d, out)
        assert err.value.code == INVALID
    # the out span meets the span of an arena that is read
    both = torch.full((b.files[0].size + b.out_len,), FILL, dtype=torch.uint8, device="cuda")
    both[:b.files[0].size] = files[3]
    with pytest.raises(RsgError) as err:
        e.decode_mixed(files[:3] + [both[:b.files[0].size]] + files[4:], good, both[100:100 + b.out_len])
    assert err.value.code == INVALID
    assert bool((both[b.files[0].size:] == FILL).all())
    # ... but not one that no stripe reads
    d = [[r[0], r[1], r[2], r[3] & ~(1 << 3)] for r in good]
    status, _ = e.decode_mixed(files[:3] + [both[:b.files[0].size]] + files[4:], d, both[100:100 + b.out_len])
    assert status == [OK] * 4
    # ranges that wrap reach the library only through the raw entry
    import ctypes
    from rustfs_amd import _lib
    dt = np.dtype(list(_lib.RECORD_DESC_FIELDS))
    fp = (ctypes.c_void_p * 6)(*[f.data_ptr() for f in files])
    st_arr, sv_arr = (ctypes.c_int * 4)(), (ctypes.c_uint32 * 4)()
    for field, value in (("rec_off", 2 ** 64 - 40), ("out_off", 2 ** 64 - 8)):
        raw = np.array([tuple(r) for r in good], dtype=dt)
        raw[field][3] = value
        assert _lib.load().rsg_decode_mixed_dev(gpu.handle, k, m, 4, raw.ctypes.data, fp, HH, 1, out.data_ptr(),
                                                sv_arr, st_arr, None) == INVALID
    assert _lib.load().rsg_decode_mixed_dev(gpu.handle, k, m, 0, None, None, HH, 1, None, None, None, None) == OK
    torch.cuda.synchronize()
    assert bool((out == FILL).all())


# -- 11 ----------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(8, 4), (12, 4), (5, 0)])
def test_inline_shards_many_round_trip(gpu, k, m):
    from rustfs_amd import Erasure
    from rustfs_amd._lib import RsgError
    rng = np.random.default_rng(k * 100 + m)
    sizes = [0, 1, k - 1, k, 4097, 100_000, 0, 300_001, 65536, 12345]
    datas = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]
    e = Erasure(k, m, 1 << 20)
    objs = e.encode_inline_shards_many(datas)
    assert e.decode_inline_shards_many(objs, sizes) == datas
    # None entries up to m, a record of the wrong length, one object below quorum
    objs = [list(o) for o in objs]
    for j, o in enumerate(objs):
        if not o:
            continue  # an empty object has no shards
        for c in range(max(0, m - 1) if j == 4 else min(m, j % (m + 1))):
            o[(j + 1 + 2 * c) % (k + m)] = None
    if m:
        objs[4][0] = objs[4][0][:-1]  # wrong length: absent
    quorum = 7
    for c in range(m + 1):
        objs[quorum][c] = None
    got = e.decode_inline_shards_many(objs, sizes)
    for j, d in enumerate(datas):
        if j == quorum:
            assert isinstance(got[j], RsgError) and got[j].code == TOO_FEW
        else:
            assert got[j] == d, f"object {j}"


def test_put_objects_then_get_objects(gpu, tmp_path):
    from rustfs_amd.loopback import LocalErasureSet
    from rustfs_amd._lib import RsgError
    k, m, bs = 4, 2, 1 << 16
    dirs = [str(tmp_path / f"d{i}") for i in range(k + m)]
    for d in dirs:
        os.makedirs(d)
    s = LocalErasureSet(dirs, k, m, block_size=bs)
    rng = np.random.default_rng(11)
    sizes = [1, 4097, bs, bs + 1, 3 * bs + 777, 0, 2 * bs]
    items = [(f"obj{j}", rng.integers(0, 256, n, dtype=np.uint8).tobytes()) for j, n in enumerate(sizes)]
    names = [n for n, _ in items]
    bodies = [b for _, b in items]
    s.put_objects(items)
    try:
        assert s.get_objects(names) == bodies                      # healthy
        assert [s.get_object(n) for n in names] == bodies
        shutil.rmtree(dirs[1])                                       # one disk away
        assert s.get_objects(names) == bodies
        path = s.part_file(0, "obj4")                                # one shard file of one object corrupted
        raw = bytearray(open(path, "rb").read())
        raw[len(raw) // 2] ^= 0x10
        open(path, "wb").write(bytes(raw))
        assert s.get_objects(names) == bodies
        assert s.get_object("obj4") == bodies[4]
        for i in (2, 3):                                             # obj3 below quorum: 3 of 6 shard files left
            os.remove(s.part_file(i, "obj3"))
        got = s.get_objects(names, return_exceptions=True)
        assert isinstance(got[3], RsgError) and got[3].code == TOO_FEW
        assert [g for j, g in enumerate(got) if j != 3] == [b for j, b in enumerate(bodies) if j != 3]
        with pytest.raises(RsgError) as err:
            s.get_objects(names)
        assert err.value.code == TOO_FEW
    finally:
        s.close()
