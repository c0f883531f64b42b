"""Mixed-length batch heal on the GPU (rsg_heal_mixed_dev / _host,
k_heal_mixed): verify-before-use of the source records and the rebuild of the
target shards' [HH256S][shard] records over n stripes with different shard
lengths, present sets and rot.  The expected target records are the records
the oracle builds for the original stripe (oracle.encode, oracle.hh256s,
oracle.hh256s_legacy): a healed record equals the one the encode wrote.  They
are never the library's own output, and statuses follow from how a case was
built."""
import ctypes
import os
import shutil

import numpy as np
import pytest

from mixed_shapes import SMALL_PERM, heal_cases, sweep_params, plan_heal, settle_heal

pytestmark = pytest.mark.gpu

FILL = 0xA5
LENGTHS = [0, 1, 7, 8, 31, 32, 33, 511, 512, 513, 1023, 1024, 1025, 87382]
GEOMETRIES = [(2, 2), (3, 1), (4, 2), (5, 3), (8, 4), (12, 4), (16, 4)]
HH, LEGACY = 1, 2  # RSG_HASH_HIGHWAY256S, RSG_HASH_HIGHWAY256S_LEGACY
OK, TOO_FEW, INCONSISTENT, INVALID, ZERO_PARITY, UNSUPPORTED = 0, 8, 10, 1, 3, 15

_REF = {}


def spw_for(t):
    """Stripes per workgroup of the kernel for t rows (decode_spw_for over fused_spw_for)."""
    return 2 if t >= 20 else 1 if t % 16 == 0 else 2 if t % 8 == 0 else 4 if (t % 4 == 0 or t <= 6) else 2


def ref_stripe(O, k, m, S):
    """Oracle stripe of shard length S: ((k+m, S) shards, {algo: [k+m digests]});
    computed once per (k, m, S) and shared, never modified."""
    key = (k, m, S)
    if key not in _REF:
        st = np.zeros((k + m, S), dtype=np.uint8)
        st[:k] = np.random.default_rng(15485863 * k + 41 * m + S).integers(0, 256, (k, S), dtype=np.uint8)
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


def target_sets(k, m):
    """{kind: shards}: one data shard, one parity shard, a data and a parity
    shard and m shards, as far as m allows."""
    sets = {"data": (min(1, k - 1),), "parity": (k + m - 1,)}
    if m >= 2:
        sets["data+parity"] = (0, k)
    many = []
    for i in (0, 2 if k > 2 else 1, k, k + m - 1):
        if i not in many:
            many.append(i)
    sets["m"] = tuple(sorted(many[:m]))
    return sets


class Heal:
    """n stripes of the given lengths as [digest][shard] records at odd
    rec_off with 1-3 byte gaps in k+m source arenas; the records of the
    `targets` shards are healed into target arenas at odd out_off with 1-3
    byte gaps (or packed densely from offset 0), whose every other byte, 64
    bytes after the last record included, holds FILL.  The source arena of a
    target shard holds 0x5A only: it is never read.  absent[j]: shards whose
    present bit is cleared in stripe j."""

    def __init__(self, O, k, m, lens, targets, algo=HH, absent=None, dense=False, seed=0):
        self.O, self.k, self.m, self.t, self.n, self.lens, self.algo = O, k, m, k + m, len(lens), list(lens), algo
        self.targets = sorted(targets)
        rng = np.random.default_rng(seed)
        self.absent = [set(a) for a in (absent or [()] * self.n)]
        self.rec_off, self.out_off = [], []
        r, o = 1, 0 if dense else 3
        for S in lens:
            self.rec_off.append(r)
            self.out_off.append(o)
            r += 32 + S + int(rng.integers(1, 4))
            o += 32 + S + (0 if dense else int(rng.integers(1, 4)))
        self.files = [np.full(r + 64, FILL, dtype=np.uint8) for _ in range(self.t)]
        self.out_len = o + 64
        for j, S in enumerate(lens):
            st, digs = ref_stripe(O, k, m, S)
            for i in range(self.t):
                a, r0 = self.files[i], self.rec_off[j]
                a[r0:r0 + 32] = np.frombuffer(digs[algo][i], dtype=np.uint8)
                a[r0 + 32:r0 + 32 + S] = st[i]
        for i in self.targets:
            self.files[i][:] = 0x5A
        self.null = set()  # source arenas passed as NULL

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

    def run_dev(self):
        import torch
        from rustfs_amd import Erasure
        e = Erasure(self.k, self.m, 1 << 20)
        files = [None if i in self.null else torch.from_numpy(self.files[i].copy()).cuda() for i in range(self.t)]
        tg = [torch.full((self.out_len,), FILL, dtype=torch.uint8, device="cuda") if i in self.targets else None
              for i in range(self.t)]
        status = e.heal_mixed(files, tg, self.desc(), self.algo)
        torch.cuda.synchronize()
        for i, f in enumerate(files):
            assert f is None or np.array_equal(f.cpu().numpy(), self.files[i]), f"source arena {i} changed"
        return status, {i: tg[i].cpu().numpy() for i in self.targets}

    def expected_status(self, failed=None):
        """From how the case was built: a stripe with fewer than k readable
        non-target shards is TOO_FEW; `failed` names what rot adds."""
        failed = failed or {}
        out = []
        for j in range(self.n):
            readable = self.t - len(set(self.targets) | self.absent[j] | self.null)
            out.append(failed.get(j, OK if readable >= self.k else TOO_FEW))
        return out

    def check(self, res, failed=None, span_only=False):
        """Every target arena holds the oracle's record of every good stripe,
        an all-zero header for a failed one (its body is unspecified), and
        FILL in every other byte (span_only, the host form: only outside the
        span from the first record's start to the last record's end)."""
        status, tgs = res
        want_status = self.expected_status(failed)
        assert status == want_status, f"statuses {status}, expected {want_status}"
        for i in self.targets:
            want = np.full(self.out_len, FILL, dtype=np.uint8)
            skip = np.zeros(self.out_len, dtype=bool)
            if span_only and self.n:
                skip[self.out_off[0]:self.out_off[-1] + 32 + self.lens[-1]] = True
            for j, S in enumerate(self.lens):
                o0 = self.out_off[j]
                skip[o0:o0 + 32 + S] = False
                if want_status[j] != OK:
                    want[o0:o0 + 32] = 0
                    skip[o0 + 32:o0 + 32 + S] = True
                    continue
                st, digs = ref_stripe(self.O, self.k, self.m, S)
                want[o0:o0 + 32] = np.frombuffer(digs[self.algo][i], dtype=np.uint8)
                want[o0 + 32:o0 + 32 + S] = st[i]
            bad = np.flatnonzero((tgs[i] != want) & ~skip)
            assert bad.size == 0, (f"target {i} differs at {bad[:8]} (stripe offsets {self.out_off[:6]}...; "
                                   f"records = the oracle's, all else {FILL:#x})")


def ordered(lens, how):
    up = sorted(lens)
    if how == "ascending":
        return up
    if how == "descending":
        return up[::-1]
    rng = np.random.default_rng(len(lens))
    return [up[i] for i in rng.permutation(len(up))]


LENGTH_CASES = [(k, m, kind) for k, m in GEOMETRIES for kind in target_sets(k, m)]


# -- 1 -----------------------------------------------------------------------------

def test_smallest_launch(gpu, oracle):
    """n = 1, RS(4,2), S = 1025, data shard 1 healed."""
    b = Heal(oracle, 4, 2, [1025], targets=(1,))
    b.check(b.run_dev())


# -- 2 -----------------------------------------------------------------------------

@pytest.mark.parametrize("k,m,kind", LENGTH_CASES)
def test_lengths(gpu, oracle, k, m, kind):
    """Every length class in one batch, ascending, descending and shuffled,
    for every target set of every geometry; both hash keys on RS(4,2).
    Target records at odd offsets between guard bytes."""
    targets = target_sets(k, m)[kind]
    for how in ("ascending", "descending", "shuffled"):
        lens = ordered(LENGTHS, how)
        for algo in ((HH, LEGACY) if (k, m) == (4, 2) else (HH,)):
            b = Heal(oracle, k, m, lens, targets, algo)
            b.check(b.run_dev())


@pytest.mark.parametrize("C,R", sweep_params(1))
def test_every_shape(gpu, oracle, C, R):
    """Instantiation <C, R> of the kernel, every one of them, over the small
    length set (mixed_shapes.py): every (C, R, e) as geometry (C, R) with e
    targets and every other shard present, once the lowest e shard indices
    (data first) with the target records packed back to back, so that a
    spilled store lands in the neighbour's header, and once the highest e
    (parity) at odd offsets between guard bytes.  Whole target arenas
    compared, source arenas unchanged.  The union over the parameters is all
    160 shapes (test_mixed_shapes.py)."""
    for k, m, targets, dense, shape in heal_cases(C, R):
        plan = plan_heal(k, m, (1 << (k + m)) - 1, bits(targets))
        assert (k, len(plan[1]) + len(plan[2]), len(plan[1])) == shape, (k, m, targets)
        b = Heal(oracle, k, m, SMALL_PERM, targets, dense=dense, seed=m)
        try:
            b.check(b.run_dev())
        except AssertionError as err:
            raise AssertionError(f"shape {shape}, RS({k},{m}), targets {targets}: {err}") from err


@pytest.mark.parametrize("k,m", [(2, 2), (4, 2), (5, 3), (8, 4), (16, 4)])
def test_densely_packed_targets(gpu, oracle, k, m):
    """Target records back to back: a store that spills over a record's end
    lands in the next record's header, which another workgroup writes."""
    for kind, targets in target_sets(k, m).items():
        b = Heal(oracle, k, m, ordered(LENGTHS, "shuffled") + [7, 1, 0, 513], targets, dense=True)
        b.check(b.run_dev())


# -- 3 -----------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(4, 2), (8, 4), (12, 4), (16, 4)])
def test_batch_sizes(gpu, oracle, k, m):
    """Batches of 1, SPW and SPW+1 stripes (one workgroup, exactly; one more),
    with empty stripes beside a long one."""
    for targets in ((1,), (0, k)):
        spw = spw_for(k + m)  # every readable shard past the sources is a row: R = m
        pool = [1025, 0, 513, 7, 87382, 32, 0, 1, 700]
        for n in (1, spw, spw + 1, 2 * spw + 1):
            b = Heal(oracle, k, m, pool[:n], targets)
            b.check(b.run_dev())
        b = Heal(oracle, k, m, [0] * (spw + 1), targets)  # only bare digests
        b.check(b.run_dev())


# -- 4 -----------------------------------------------------------------------------

def test_mixed_masks_land_at_caller_indices(gpu, oracle):
    """Three masks interleaved into groups of 1, SPW and SPW+1 stripes, in a
    caller order that differs from the kernel order (lengths not sorted); the
    third mask leaves fewer than k readable shards."""
    k, m = 8, 4
    spw = spw_for(k + m)
    A, B, C = (), (1, 11), (0, 3, 9, 10)  # with target 2: 11, 9 and 7 readable
    absent = []
    for i in range(spw + 1):
        absent.append(B)
        if i < spw:
            absent.append(C)
        if i == 1:
            absent.append(A)
    lens = [(33, 1025, 0, 513, 7, 87382, 512, 1, 1023, 8)[i % 10] for i in range(len(absent))]
    b = Heal(oracle, k, m, lens, targets=(2,), absent=absent)
    want = b.expected_status()
    assert want.count(TOO_FEW) == spw and want.count(OK) == spw + 2
    b.check(b.run_dev())


def test_null_arena_is_absent_whatever_present_says(gpu, oracle):
    b = Heal(oracle, 8, 4, [513, 0, 87382, 7], targets=(0, 9))
    b.null = {2, 10}
    b.check(b.run_dev())
    b.null = {2, 10, 11}  # 7 left
    assert b.expected_status() == [TOO_FEW] * 4
    b.check(b.run_dev())


def test_target_shard_is_never_read(gpu, oracle):
    """The target's own source arena may be anything, the target arena
    itself included; its present bit changes nothing."""
    import torch
    from rustfs_amd import Erasure
    k, m = 4, 2
    b = Heal(oracle, k, m, [513, 7, 0, 1025], targets=(1,))
    files = [torch.from_numpy(f.copy()).cuda() for f in b.files]
    tg = torch.full((max(b.out_len, b.files[1].size),), FILL, dtype=torch.uint8, device="cuda")
    files[1] = tg
    for present in (0x3f, 0x3d):
        tg[:] = FILL
        d = [[r[0], r[1], r[2], present] for r in b.desc()]
        status = Erasure(k, m, 1 << 20).heal_mixed(files, [None, tg, None, None, None, None], d)
        b.check((status, {1: tg[:b.out_len].cpu().numpy()}))


# -- 5 -----------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(8, 4), (5, 3)])
def test_rot_found_during_the_read(gpu, oracle, k, m):
    """Rot that only the read finds, each rotten stripe between clean
    neighbours of the same workgroup.  Target: data shard 0; sources data
    1..k-1 and parity k, surplus parity k+1..k+m-1."""
    lens, rots, rew, failed = [], [], [], {}
    for S in (7, 513, 1025, 32):
        for what in ("body", "header", "surplus", "too-few", "inconsistent"):
            j = len(lens)
            lens += [S, S]  # the rotten stripe, then a clean neighbour
            if what == "body":        # a source's body: the stripe heals from the others
                rots.append((j, 2, S - 1))
            elif what == "header":    # a source's header
                rots.append((j, k, -5))
            elif what == "surplus":   # a surplus record that fails its hash is dropped, not compared
                rots.append((j, k + m - 1, 0))
            elif what == "too-few":   # m rotten records: k - 1 verified
                for i in range(m):
                    rots.append((j, 1 + i, S // 2 if i % 2 else -1 - i))
                failed[j] = TOO_FEW
            else:                     # a surplus parity with a valid digest over wrong bytes
                rew.append((j, k + 1))
                failed[j] = INCONSISTENT
    b = Heal(oracle, k, m, lens, targets=(0,))
    for j, shard, at in rots:
        b.flip(j, shard, at)
    for j, shard in rew:
        b.rewrite(j, shard)
    # the planner rule (mixed_shapes.py): a heal reads every readable non-target
    # shard in its first round, so none of these stripes launches more than twice
    for j in range(b.n):
        rotten = bits(s for jj, s, _ in rots if jj == j)
        final, rounds, _ = settle_heal(k, m, bits(range(k + m)), bits((0,)), rotten)
        assert rounds <= 2 and (rounds == 2) == (bool(rotten) and failed.get(j) != TOO_FEW)
        assert (bin(final).count("1") < k) == (failed.get(j) == TOO_FEW)
    b.check(b.run_dev(), failed)
    # the same rot, two targets (a data and a parity shard), dense records
    b2 = Heal(oracle, k, m, lens, targets=(0, k + m - 1), dense=True)
    failed2 = {}
    for S_i, S in enumerate((7, 513, 1025, 32)):
        j = 10 * S_i
        b2.flip(j, 2, S - 1)                         # heals from the others
        for i in range(m - 1):                       # m - 1 rotten with two targets: k - 1 verified
            b2.flip(j + 2, 1 + i, S // 2)
        failed2[j + 2] = TOO_FEW
        b2.rewrite(j + 4, k + 1)                     # surplus k+1 (sources: data 1..k-1, parity k)
        failed2[j + 4] = INCONSISTENT
    b2.check(b2.run_dev(), failed2)


# -- 6 -----------------------------------------------------------------------------

@pytest.mark.parametrize("k,m", [(10, 6), (17, 3)])
def test_fallback_geometries(gpu, oracle, k, m):
    """m > 4 and k > 16: the same results through the per-length engine."""
    lens = [1, 33, 513, 0, 1025, 700, 513, 0]
    absent = [(), (1,), (0, 2), (), (), tuple(range(2, m + 2)), (), tuple(range(2, m + 2))]
    b = Heal(oracle, k, m, lens, targets=(1, k + 1), absent=absent)
    b.flip(4, 3, 100)
    b.check(b.run_dev())


def test_more_targets_than_m(gpu, oracle):
    b = Heal(oracle, 4, 2, [513, 0, 7], targets=(0, 1, 5))
    assert b.expected_status() == [TOO_FEW] * 3
    b.check(b.run_dev())


def test_offsets_past_4g(gpu, oracle):
    """Records and target records past 2 GiB and 4 GiB (large uninitialised
    device buffers, only the stripes' ranges filled and read back): 64-bit
    addressing end to end, the zeroed header of a failed stripe included."""
    import torch
    from rustfs_amd import Erasure
    k, m, t = 4, 2, 6
    lens = [1025, 700, 513, 33]
    recs = [5, (1 << 31) + 7, (1 << 32) + 9, (1 << 32) + 2001]
    outs = [(1 << 31) - 1, (1 << 32) + 3, (1 << 32) + 8191, (1 << 32) + 9001]
    gone = [(), (0,), (3,), (0, 3)]  # with target 1: 5, 4, 4 and 3 readable
    pitch = 8192  # arena i begins i*pitch into the one buffer: records of different shards never meet
    big = torch.empty((1 << 32) + (1 << 20), dtype=torch.uint8, device="cuda")
    tg = torch.empty((1 << 32) + (1 << 16), dtype=torch.uint8, device="cuda")
    files = [None if i == 1 else big[i * pitch:] for i in range(t)]
    for j, S in enumerate(lens):
        st, digs = ref_stripe(oracle, k, m, S)
        for i in range(t):
            if i != 1:
                rec = np.concatenate([np.frombuffer(digs[HH][i], dtype=np.uint8), st[i]])
                files[i][recs[j]:recs[j] + 32 + S] = torch.from_numpy(rec).cuda()
        tg[outs[j] - 8:outs[j] + 32 + S + 8] = FILL
    desc = [[recs[j], outs[j], lens[j], 0x3f & ~bits(gone[j])] for j in range(4)]
    status = Erasure(k, m, 1 << 20).heal_mixed(files, [None, tg, None, None, None, None], desc)
    assert status == [OK, OK, OK, TOO_FEW]
    for j, S in enumerate(lens):
        st, digs = ref_stripe(oracle, k, m, S)
        got = tg[outs[j] - 8:outs[j] + 32 + S + 8].cpu().numpy()
        want = np.full(32 + S + 16, FILL, dtype=np.uint8)
        if status[j] == OK:
            want[8:40] = np.frombuffer(digs[HH][1], dtype=np.uint8)
            want[40:40 + S] = st[1]
        else:
            want[8:40] = 0
            got[40:40 + S] = FILL  # the body of a failed stripe is unspecified
        assert np.array_equal(got, want), f"target record of stripe {j}"


# -- 7 -----------------------------------------------------------------------------

def _pinned_or_not(a, pinned):
    import torch
    if not pinned:
        return a.copy()
    h = torch.empty(a.size, dtype=torch.uint8).pin_memory().numpy()
    h[:] = a
    return h


@pytest.mark.parametrize("pinned", [True, False])
def test_host_form(gpu, oracle, pinned):
    """Pinned and pageable arenas, a batch of at least three sub-batches with
    a rotten record and a failed stripe in the middle one: the device form's
    statuses and records; the sources and the target bytes outside the span
    of records untouched."""
    from rustfs_amd import Erasure, _lib
    k, m, t = 4, 2, 6
    targets = (1, 4)
    lens = [350001, 87382, 0, 400000, 513] * 15
    b = Heal(oracle, k, m, lens, targets, dense=True)
    # the planner's split: the record span per arena read, the target span per target
    rnd = lambda x: (x + 255) // 256 * 256
    nf, nt = t - len(targets), len(targets)

    def cost(a, z):
        return (nf * rnd(b.rec_off[z - 1] + 32 + lens[z - 1] - b.rec_off[a]) +
                nt * rnd(b.out_off[z - 1] + 32 + lens[z - 1] - b.out_off[a]))
    subs, first = [], 0
    for j in range(b.n + 1):
        if j == b.n or (j > first and cost(first, j + 1) > _lib.RSG_MIXED_STAGE_BYTES):
            subs.append((first, j))
            first = j
    assert len(subs) >= 3, subs
    mid = [j for j in range(*subs[1]) if lens[j] > 1000]
    # two targets leave exactly k readable shards: any rot loses the quorum
    b.flip(mid[0], 0, lens[mid[0]] // 2)
    b.flip(mid[1], 2, 5)
    b.flip(mid[1], 3, -1)
    failed = {mid[0]: TOO_FEW, mid[1]: TOO_FEW}
    files = [_pinned_or_not(f, pinned) for f in b.files]
    tgs = {i: _pinned_or_not(np.full(b.out_len, FILL, dtype=np.uint8), pinned) for i in targets}
    status = Erasure(k, m, 1 << 20).heal_mixed_host(files, [tgs.get(i) for i in range(t)], b.desc())
    for i in range(t):
        assert np.array_equal(files[i], b.files[i]), f"source arena {i} changed"
    b.check((status, tgs), failed, span_only=True)
    dev = b.run_dev()
    assert dev[0] == status
    b.check(dev, failed)


def test_host_form_heals_through_rot_and_fault_injection(gpu, oracle):
    """One target, so a rotten source still leaves k: OK through the host
    form, sparse target records; rsg_test_fail_subbatch makes sub-batch 1 fail
    and the call return the error."""
    from rustfs_amd import Erasure, _lib
    from rustfs_amd._lib import RsgError
    k, m, t = 4, 2, 6
    lens = [400000, 0, 513, 87382, 7] * 20
    b = Heal(oracle, k, m, lens, targets=(5,))
    b.flip(40, 1, 77)
    b.rewrite(43, 4)  # sources 0..3, surplus 4
    e = Erasure(k, m, 1 << 20)
    tg = np.full(b.out_len, FILL, dtype=np.uint8)
    status = e.heal_mixed_host(b.files, [None] * 5 + [tg], b.desc())
    b.check((status, {5: tg}), {43: INCONSISTENT}, span_only=True)
    lib = _lib.load()
    assert lib.rsg_test_fail_subbatch(gpu.handle, 1) == OK
    try:
        with pytest.raises(RsgError) as err:
            e.heal_mixed_host(b.files, [None] * 5 + [tg.copy()], b.desc())
        assert err.value.code == _lib.RSG_ERR_DEVICE
    finally:
        assert lib.rsg_test_fail_subbatch(gpu.handle, -1) == OK
    tg2 = np.full(b.out_len, FILL, dtype=np.uint8)
    assert e.heal_mixed_host(b.files, [None] * 5 + [tg2], b.desc()) == status
    b.check((status, {5: tg2}), {43: INCONSISTENT}, span_only=True)


# -- 8 -----------------------------------------------------------------------------

def test_validation(gpu, oracle):
    """Each rejection leaves the targets with their fill."""
    import torch
    from rustfs_amd import Erasure, _lib
    from rustfs_amd._lib import RsgError
    k, m, t = 4, 2, 6
    b = Heal(oracle, k, m, [513, 33, 0, 1025], targets=(1, 5))
    e = Erasure(k, m, 1 << 20)
    files = [torch.from_numpy(f.copy()).cuda() for f in b.files]
    tg = [torch.full((b.out_len,), FILL, dtype=torch.uint8, device="cuda") if i in (1, 5) else None for i in range(t)]
    good = b.desc()

    def changed(j, field, value):
        d = [list(r) for r in good]
        d[j][field] = value
        return d
    bad = [
        changed(1, 3, 1 << 6),                    # a present bit at k+m
        changed(1, 0, good[0][0] + 31),           # record ranges overlap
        changed(3, 0, good[0][0]),                # ... not ascending
        changed(1, 1, good[0][1] + 32 + 513 - 1),  # target ranges overlap
        changed(3, 1, good[2][1] + 31),           # ... with the bare digest of a zero-length stripe
        changed(3, 1, good[0][1]),                # ... not ascending
    ]
    for d in bad:
        with pytest.raises(RsgError) as err:
            e.heal_mixed(files, tg, d)
        assert err.value.code == INVALID, d
    with pytest.raises(RsgError) as err:          # no target at all
        e.heal_mixed(files, [None] * t, good)
    assert err.value.code == INVALID
    with pytest.raises(RsgError) as err:          # an unknown algo
        e.heal_mixed(files, tg, good, algo=77)
    assert err.value.code == INVALID
    # a target span meets the span of an arena that is read / of another target
    both = torch.full((b.files[0].size + b.out_len,), FILL, dtype=torch.uint8, device="cuda")
    both[:b.files[0].size] = files[3]
    src3 = both[:b.files[0].size]
    with pytest.raises(RsgError) as err:
        e.heal_mixed(files[:3] + [src3] + files[4:], [None, both[100:100 + b.out_len], None, None, None, tg[5]], good)
    assert err.value.code == INVALID
    with pytest.raises(RsgError) as err:
        e.heal_mixed(files, [None, both[:b.out_len], None, None, None, both[40:40 + b.out_len]], good)
    assert err.value.code == INVALID
    assert bool((both[b.files[0].size:] == FILL).all()) and np.array_equal(src3.cpu().numpy(), b.files[3])
    # ... but not an arena that no stripe reads
    # (one target, so that k shards stay readable without shard 3)
    b1 = Heal(oracle, k, m, b.lens, targets=(1,))
    f1 = [torch.from_numpy(f.copy()).cuda() for f in b1.files]
    d = [[r[0], r[1], r[2], r[3] & ~(1 << 3)] for r in good]
    only1 = [None, both[100:100 + b.out_len], None, None, None, None]
    status = e.heal_mixed(f1[:3] + [src3] + f1[4:], only1, d)
    assert status == [OK] * 4
    got = both[100:100 + b.out_len].cpu().numpy()
    for j, S in enumerate(b.lens):
        st, digs = ref_stripe(oracle, k, m, S)
        want = np.concatenate([np.frombuffer(digs[HH][1], dtype=np.uint8), st[1]])
        assert np.array_equal(got[b.out_off[j]:b.out_off[j] + 32 + S], want), f"stripe {j}"
    # ranges that wrap, NULL pointers and geometry errors through the raw entry
    dt = np.dtype(list(_lib.RECORD_DESC_FIELDS))
    lib = _lib.load()
    fp = (ctypes.c_void_p * t)(*[f.data_ptr() for f in files])
    tp = (ctypes.c_void_p * t)(*[g.data_ptr() if g is not None else None for g in tg])
    st_arr = (ctypes.c_int * 4)()
    raw = np.array([tuple(r) for r in good], dtype=dt)
    for field, value in (("rec_off", 2 ** 64 - 40), ("out_off", 2 ** 64 - 40)):
        w = raw.copy()
        w[field][3] = value
        assert lib.rsg_heal_mixed_dev(gpu.handle, k, m, 4, w.ctypes.data, fp, tp, HH, st_arr, None) == INVALID
    assert lib.rsg_heal_mixed_dev(gpu.handle, k, m, 4, None, fp, tp, HH, st_arr, None) == INVALID
    assert lib.rsg_heal_mixed_dev(gpu.handle, k, m, 4, raw.ctypes.data, None, tp, HH, st_arr, None) == INVALID
    assert lib.rsg_heal_mixed_dev(gpu.handle, k, m, 4, raw.ctypes.data, fp, None, HH, st_arr, None) == INVALID
    assert lib.rsg_heal_mixed_dev(gpu.handle, k, m, 4, raw.ctypes.data, fp, tp, HH, None, None) == INVALID
    assert lib.rsg_heal_mixed_dev(gpu.handle, k, 0, 4, raw.ctypes.data, fp, tp, HH, st_arr, None) == ZERO_PARITY
    assert lib.rsg_heal_mixed_dev(gpu.handle, 30, 3, 4, raw.ctypes.data, fp, tp, HH, st_arr, None) == UNSUPPORTED
    assert lib.rsg_heal_mixed_dev(gpu.handle, k, m, 0, None, None, None, HH, None, None) == OK
    assert lib.rsg_heal_mixed_host(gpu.handle, k, m, 0, None, None, None, HH, None) == OK
    torch.cuda.synchronize()
    for i in (1, 5):
        assert bool((tg[i] == FILL).all()), f"target {i} written by a rejected call"
    # the host form rejects the same lists with its arenas untouched
    htg = [np.full(b.out_len, FILL, dtype=np.uint8) if i in (1, 5) else None for i in range(t)]
    for dsc in bad:
        with pytest.raises(RsgError) as err:
            e.heal_mixed_host(b.files, htg, dsc)
        assert err.value.code == INVALID
    assert all(bool((g == FILL).all()) for g in htg if g is not None)


# -- 9 -----------------------------------------------------------------------------

def test_put_objects_then_heal_objects(gpu, tmp_path):
    """put_objects of 40 objects of mixed sizes; two disks' part files saved
    and deleted; heal_objects brings back byte-equal files, and the data
    still reads with two other disks removed."""
    from rustfs_amd.loopback import LocalErasureSet
    from rustfs_amd._lib import RsgError
    k, m, bs = 4, 2, 1 << 16
    dirs = [str(tmp_path / f"d{i}") for i in range(k + m)]
    for d in dirs:
        os.makedirs(d)
    s = LocalErasureSet(dirs, k, m, block_size=bs)
    rng = np.random.default_rng(17)
    sizes = [0, 1, k - 1, k, 4097, bs - 1, bs, bs + 1, 3 * bs + 777, 2 * bs, 5 * bs + 1]
    sizes += [int(v) for v in rng.integers(1, 3 * bs, 40 - len(sizes))]
    items = [(f"obj{j}", rng.integers(0, 256, n, dtype=np.uint8).tobytes()) for j, n in enumerate(sizes)]
    names = [n for n, _ in items]
    bodies = [body for _, body in items]
    s.put_objects(items)
    try:
        healed_disks = [1, 4]
        saved = {}
        for i in healed_disks:
            for name in names:
                path = s.part_file(i, name)
                saved[i, name] = (path, open(path, "rb").read())
            shutil.rmtree(dirs[i])
            os.makedirs(dirs[i])
        assert s.heal_objects(names, healed_disks) == [None] * len(names)
        for (i, name), (path, raw) in saved.items():
            assert s.part_file(i, name) == path, f"disk {i} {name}: metadata"
            assert open(path, "rb").read() == raw, f"disk {i} {name}: healed part differs from what PUT wrote"
        for i in (0, 5):  # two other disks away: the healed ones serve
            shutil.rmtree(dirs[i])
        assert s.get_objects(names) == bodies
        assert s.heal_objects(names, [0, 5]) == [None] * len(names)  # and heal those from the healed ones
        assert [s.get_object(n) for n in names[:12]] == bodies[:12]
        # one object below quorum does not stop the others
        for i in (2, 3):
            os.remove(s.part_file(i, "obj8"))
        got = s.heal_objects(names[6:10], [5], return_exceptions=True)
        assert isinstance(got[2], RsgError) and got[2].code == TOO_FEW
        assert got[:2] == [None, None] and got[3] is None
        with pytest.raises(RsgError) as err:
            s.heal_objects(names[6:10], [5])
        assert err.value.code == TOO_FEW
    finally:
        s.close()
