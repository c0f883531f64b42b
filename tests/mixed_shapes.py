"""What the mixed-length kernels' GPU tests share that needs no GPU: the small
length set, a Python restatement of the host planner's rule for one mask
(rustfs_amd/csrc/rs_mixed_decode_plan.h plan_mask, rs_mixed_heal_plan.h
plan_heal_mask: the first k readable shards in ascending index are the
sources, then the written rows, then the surplus), the redo rounds of one
stripe under that rule (tests/host/record_rounds_check.h settle), and the
generators of the shape sweeps.  The kernels are templates over <C, R>: C
sources, R computed rows, of which the first e (a run-time value) are written
and the others compared; a shape is (C, R, e).

tests/test_mixed_shapes.py checks the generators against the full set of
reachable shapes; tests/host/mixed_decode_plan_main.cpp pins the round counts
used here to the shipped planner."""

# The smallest lengths at which each loader form and each hasher path is
# taken: the empty message; the byte gather (1..7); the shifted last 8 bytes
# with a tail below 8 (513) and from 8 on; one whole 512-byte chunk; 32-byte
# packet remainders 0, 1 and 31; one, two and three chunks.
SMALL = [0, 1, 7, 8, 9, 31, 32, 33, 511, 512, 513, 1025]
# One fixed caller order.  Nine of the twelve lengths are one chunk long, so
# neighbours cannot all differ in chunk count; the three that differ (0, 513,
# 1025) are spread so that every aligned run of four holds two counts, and the
# order is neither the kernel's (chunk count descending) nor sorted.
SMALL_PERM = [33, 1025, 7, 511, 512, 0, 9, 31, 1, 513, 8, 32]
MAX_C, MAX_R = 16, 4


def chunks(S):
    return -(-S // 512)


def bits(idx):
    v = 0
    for i in idx:
        v |= 1 << i
    return v


def popcount(v):
    return bin(v).count("1")


def plan_get(k, m, mask, verify_surplus):
    """plan_mask: (src, written, surplus), or None with fewer than k readable."""
    if popcount(mask) < k:
        return None
    written = [i for i in range(k) if not mask >> i & 1]
    src, surplus = [], []
    for i in range(k + m):
        if not mask >> i & 1:
            continue
        if len(src) < k:
            src.append(i)
        elif verify_surplus and written:
            surplus.append(i)
    return src, written, surplus


def plan_heal(k, m, mask, targets):
    """plan_heal_mask: targets (a bit mask) are written and never read."""
    mask &= ~targets
    if popcount(mask) < k:
        return None
    written = [i for i in range(k + m) if targets >> i & 1]
    readable = [i for i in range(k + m) if mask >> i & 1]
    return readable[:k], written, readable[k:]


def shape_of(k, plan):
    """(C, R, e) of the launch of a plan."""
    _, written, surplus = plan
    return (k, len(written) + len(surplus), len(written))


def read_mask(plan):
    return bits(plan[0]) | bits(plan[2])


def settle_with(plan, k, mask, rotten):
    """One stripe to its end: plan, drop what the plan reads that is rotten,
    again.  (final mask, launching rounds, the rounds' shapes)."""
    rounds, shapes = 0, []
    while True:
        p = plan(mask)
        if p is None:
            return mask, rounds, shapes
        rounds += 1
        shapes.append(shape_of(k, p))
        bad = read_mask(p) & rotten
        if not bad:
            return mask, rounds, shapes
        mask &= ~bad


def settle(k, m, mask, rotten, verify_surplus):
    """A GET's stripe: (final mask, rounds, shapes).  The stripe is
    TOO_FEW iff fewer than k bits remain; its served bits are the final
    mask's data bits."""
    return settle_with(lambda x: plan_get(k, m, x, verify_surplus), k, mask, rotten)


def settle_heal(k, m, mask, targets, rotten):
    return settle_with(lambda x: plan_heal(k, m, x, targets), k, mask & ~targets, rotten)


# -- the sweeps ----------------------------------------------------------------------

def sweep_params(r_min):
    """The parameters of a sweep: one test per <C, R> instantiation."""
    return [(C, R) for C in range(1, MAX_C + 1) for R in range(r_min, MAX_R + 1)]


def get_cases(C, R):
    """[(k, m, absent, shape)] of instantiation <C, R>, verify_surplus on:
    geometry (C, R) with all present for R = 0, else for every e in
    1..min(R, C) with the lowest and with the highest e data shards absent in
    every stripe.
    The ten triples with e > C, which no GET can reach (only data shards are
    written): (1,2,2) (1,3,2) (1,3,3) (1,4,2) (1,4,3) (1,4,4) (2,3,3) (2,4,3)
    (2,4,4) (3,4,4)."""
    if R == 0:
        return [(C, 0, (), shape_of(C, plan_get(C, 0, bits(range(C)), True)))]
    out = []
    for e in range(1, min(R, C) + 1):
        for absent in dict.fromkeys((tuple(range(e)), tuple(range(C - e, C)))):
            mask = bits(range(C + R)) & ~bits(absent)
            out.append((C, R, absent, shape_of(C, plan_get(C, R, mask, True))))
    return out


def heal_cases(C, R):
    """[(k, m, targets, dense, shape)] of instantiation <C, R>: for every e in
    1..R geometry (C, R) with the lowest e shard indices (data first) as
    targets, target records packed densely, and with the highest e (parity) at
    odd offsets between guard bytes; every other shard present."""
    out = []
    for e in range(1, R + 1):
        for targets, dense in ((tuple(range(e)), True), (tuple(range(C + R - e, C + R)), False)):
            plan = plan_heal(C, R, bits(range(C + R)), bits(targets))
            out.append((C, R, targets, dense, shape_of(C, plan)))
    return out


ENCODE_SHAPES = {(C, R) for C in range(1, MAX_C + 1) for R in range(1, MAX_R + 1)}
GET_SHAPES = ({(C, 0, 0) for C in range(1, MAX_C + 1)} |
              {(C, R, e) for C in range(1, MAX_C + 1) for R in range(1, MAX_R + 1) for e in range(1, min(R, C) + 1)})
HEAL_SHAPES = {(C, R, e) for C in range(1, MAX_C + 1) for R in range(1, MAX_R + 1) for e in range(1, R + 1)}
