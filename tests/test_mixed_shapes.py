"""The shape sweeps of the mixed-length kernels' GPU tests (test_gpu_mixed.py,
test_gpu_mixed_decode.py, test_gpu_mixed_heal.py) leave no instantiation out:
the union of what the parameters of each sweep launch is the full set
of shapes the planner can ask for, worked out here from the planner rule
(mixed_shapes.py) over every mask.  No GPU needed."""
import pytest

from mixed_shapes import (ENCODE_SHAPES, GET_SHAPES, HEAL_SHAPES, MAX_C, MAX_R, SMALL, SMALL_PERM, bits, chunks,
                          get_cases, heal_cases, plan_get, plan_heal, popcount, read_mask, settle,
                          settle_heal, shape_of, sweep_params)


def test_small_length_order():
    assert sorted(SMALL_PERM) == SMALL and SMALL_PERM != SMALL
    by_chunks = sorted(SMALL_PERM, key=chunks, reverse=True)
    assert SMALL_PERM != by_chunks  # not the kernel's order either
    for a in range(0, len(SMALL_PERM), 4):
        assert len({chunks(S) for S in SMALL_PERM[a:a + 4]}) >= 2
    assert {chunks(S) for S in SMALL} == {0, 1, 2, 3}


def reachable_get(k_max):
    """Every shape plan_mask gives over every mask of every geometry k <=
    k_max, m <= 4, with and without verify_surplus."""
    out = set()
    for k in range(1, k_max + 1):
        for m in range(0, MAX_R + 1):
            for mask in range(1 << (k + m)):
                for vs in (True, False):
                    p = plan_get(k, m, mask, vs)
                    if p is not None:
                        out.add(shape_of(k, p))
    return out


def reachable_heal(k_max):
    """Every shape plan_heal_mask gives over every mask and target set."""
    out = set()
    for k in range(1, k_max + 1):
        for m in range(1, MAX_R + 1):
            t = k + m
            for targets in range(1, 1 << t):
                if popcount(targets) > m:
                    continue
                for mask in range(1 << t):
                    if mask & targets:
                        continue  # the target's own bit changes nothing
                    p = plan_heal(k, m, mask, targets)
                    if p is not None:
                        out.add(shape_of(k, p))
    return out


def by_counts_get():
    """The same for every k <= 16: a plan's shape depends only on how many
    data and how many parity shards are readable, so one mask per pair of
    counts stands for all."""
    out = set()
    for k in range(1, MAX_C + 1):
        for m in range(0, MAX_R + 1):
            for nd in range(k + 1):
                for npar in range(m + 1):
                    mask = bits(range(nd)) | bits(range(k, k + npar))
                    for vs in (True, False):
                        p = plan_get(k, m, mask, vs)
                        if p is not None:
                            out.add(shape_of(k, p))
    return out


def by_counts_heal():
    out = set()
    for k in range(1, MAX_C + 1):
        for m in range(1, MAX_R + 1):
            for td in range(min(k, m) + 1):          # targets among the data shards ...
                for tp in range(m - td + 1):          # ... and among the parity shards
                    if td + tp == 0:
                        continue
                    targets = bits(range(td)) | bits(range(k, k + tp))
                    for gd in range(k - td + 1):      # further shards unreadable
                        for gp in range(m - tp + 1):
                            gone = bits(range(td, td + gd)) | bits(range(k + tp, k + tp + gp))
                            p = plan_heal(k, m, bits(range(k + m)) & ~gone, targets)
                            if p is not None:
                                out.add(shape_of(k, p))
    return out


def test_reachable_shapes_are_the_stated_sets():
    """Over every mask for k <= 5 and over every pair of counts for k <= 16
    the planner rule reaches exactly GET_SHAPES / HEAL_SHAPES: 166 and 160."""
    small = lambda shapes: {s for s in shapes if s[0] <= 5}
    assert reachable_get(5) == small(GET_SHAPES) == small(by_counts_get())
    assert reachable_heal(5) == small(HEAL_SHAPES) == small(by_counts_heal())
    assert by_counts_get() == GET_SHAPES and len(GET_SHAPES) == 166
    assert by_counts_heal() == HEAL_SHAPES and len(HEAL_SHAPES) == 160
    assert len(ENCODE_SHAPES) == 64
    # every reachable shape is one the kernels are built for
    assert all(1 <= C <= MAX_C and 0 <= R <= MAX_R and e <= R for C, R, e in GET_SHAPES | HEAL_SHAPES)
    # the triples no GET reaches: more written rows than data shards
    assert len(HEAL_SHAPES - GET_SHAPES) == 10 and all(e > C for C, R, e in HEAL_SHAPES - GET_SHAPES)


def test_sweeps_launch_every_shape():
    """The union over the parameters of each sweep (one per <C, R>
    instantiation) is the full set: no shape is left out, and each case's
    shape is what its geometry says."""
    get, heal = set(), set()
    for C, R in sweep_params(0):
        for k, m, absent, shape in get_cases(C, R):
            assert shape == (k, m, len(absent)) and (k, m) == (C, R) and all(c < k for c in absent)
            get.add(shape)
    for C, R in sweep_params(1):
        dense = {True: set(), False: set()}
        for k, m, targets, d, shape in heal_cases(C, R):
            assert shape == (k, m, len(targets)) and (k, m) == (C, R)
            heal.add(shape)
            dense[d].add(shape)
        assert dense[True] == dense[False]  # every heal shape once densely packed, once between guards
    assert set(sweep_params(1)) == ENCODE_SHAPES and len(sweep_params(0)) == 80
    assert get == GET_SHAPES
    assert heal == HEAL_SHAPES
    # both placements: lost[] / target rows take low and high shard indices
    assert any(absent and max(absent) == 15 for _, _, absent, _ in get_cases(16, 4))
    assert any(max(t) == 19 for _, _, t, _, _ in heal_cases(16, 4)) and any(min(t) == 0 for _, _, t, _, _ in heal_cases(16, 4))


# RS(5,4) with data shard 2 rotten and further rotten parity shards: (rotten
# parity, rounds and final verdict without verify_surplus, with it).  The same
# figures are CHECKed against the shipped planner in
# tests/host/mixed_decode_plan_main.cpp.
LADDER_5_4 = [
    ((), (2, True), (2, True)),
    ((5,), (3, True), (3, True)),
    ((5, 6), (4, True), (3, True)),
    ((5, 6, 7), (5, True), (3, True)),
    ((5, 6, 7, 8), (5, False), (2, False)),
    ((6, 7, 8), (2, True), (3, True)),
    ((6,), (2, True), (3, True)),
]


@pytest.mark.parametrize("parity,off,on", LADDER_5_4)
def test_settle_round_counts(parity, off, on):
    k, m = 5, 4
    rotten = bits((2,) + parity)
    for vs, (rounds, ok) in ((False, off), (True, on)):
        final, got, shapes = settle(k, m, 0x1ff, rotten, vs)
        assert got == rounds == len(shapes) and (popcount(final) >= k) == ok
        assert shapes[0] == (5, 0, 0)
        if ok:  # the last plan read nothing rotten
            assert read_mask(plan_get(k, m, final, vs)) & rotten == 0
    if parity == (5, 6, 7):
        assert settle(k, m, 0x1ff, rotten, False)[2][1:] == [(5, 1, 1)] * 4
    if parity == (5,):
        assert settle(k, m, 0x1ff, rotten, True)[2][1:] == [(5, 4, 1), (5, 3, 1)]
    if parity == (6, 7, 8):  # parity 6 onwards is never read without verify_surplus
        assert settle(k, m, 0x1ff, rotten, False)[0] == 0x1ff & ~bits((2,))


def test_heal_settles_in_two_rounds():
    """A heal reads every readable non-target shard in its first round, so
    whatever is rotten it launches at most twice: RS(3,2), every target set,
    mask and set of rotten records."""
    k, m, t = 3, 2, 5
    for targets in range(1, 1 << t):
        for mask in range(1 << t):
            for rotten in range(1 << t):
                final, rounds, _ = settle_heal(k, m, mask, targets, rotten)
                assert rounds <= 2
                assert final == (mask & ~targets if popcount(mask & ~targets) < k else mask & ~targets & ~rotten)
