"""What the same-length verify walks' GPU tests (test_gpu_verify_walks.py)
share that needs no GPU: a Python restatement of the kernel choice
(rustfs_amd/csrc/rs_verify_pick.h pick_hash_launch), of how the three callers
build their launches (rsgpu.cpp launch_verify_group, verify_data_begin /
verify_parity_rest, rsg_bitrot_verify_dev), the arena layout the tests place
their shard files in, and the parameter rows of the GPU sweeps.

tests/test_verify_shapes.py pins the restated pick to the shipped one line by
line (tests/host/verify_pick_main.cpp) and proves that the sweeps' rows, run
through the restatement, reach every class of REQUIRED; every row owns at
least one class, so a deleted row is reported by the class it leaves out."""
from collections import namedtuple

MAX_BASES, STEP, RING_RECORDS, MAX_RING = 32, 512, 4, 15

# The boundary lengths: the packet (32), the 8-packet batch (256), the ring's
# 512-byte step and its multiples, one byte either side.
LENGTHS = [1, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1024, 1025, 1536, 2049]
# Three 256-byte batches (768..1023) have no member in LENGTHS: 768 (no
# remainder) and 1023 (31 packets + 31 bytes).  The 2-slot ring (13-15 files)
# runs at even addresses only and every even member of LENGTHS is a multiple
# of 32: 258 (8 packets + 2 bytes) and 2050 (5 steps, a 2-byte last one) give
# it ragged last steps.
EXTRA_LENGTHS = [768, 1023, 258, 2050]
RECORDS = [1, 2, 3, 4, 5, 8, 9]
M = 2  # parity files of every GET here

Pick = namedtuple("Pick", "kind blocks nf rd steps copy depth unal len per_base stride bases role")


# -- the pick (rs_verify_pick.h) ------------------------------------------------------

def pick(nbases, per_base, length, stride, bases, n=None, digest_off=-32, flags=False, has_copy=None,
         has_flag=None, depth=2, unal=True, direct_copy=False, data=0, shard_pitch=0, role=""):
    """pick_hash_launch over one launch's shape."""
    n = nbases * per_base if n is None else n
    has_copy = [False] * nbases if has_copy is None else has_copy
    has_flag = [True] * nbases if has_flag is None else has_flag
    bases = list(bases)
    mk = lambda kind, **kw: Pick(**{**dict(kind=kind, blocks=0, nf=0, rd=0, steps=0, copy=0, depth=0, unal=False,
                                           len=length, per_base=per_base, stride=stride, bases=tuple(bases),
                                           role=role), **kw})
    if n == 0:
        return mk("none")
    blocks = (n * 4 + 255) // 256
    if blocks > 0x7fffffff:
        return mk("invalid")
    copy = any(has_copy[:nbases])
    if not copy:
        ring = _ring(nbases, per_base, length, stride, bases, digest_off, flags, has_copy, has_flag)
        if ring:
            return mk("ring", **ring)
    if nbases:
        even = stride % 2 == 0 and all(b % 2 == 0 for b in bases[:nbases])
    else:
        even = data % 2 == 0 and stride % 2 == 0 and shard_pitch % 2 == 0
    un = (not copy) and depth == 2 and (not even) and unal
    return mk("quad", blocks=blocks, copy=0 if not copy else 1 if direct_copy else 2, unal=un,
              depth=2 if un else depth if depth in (1, 2) else 3)


def _ring(nbases, per_base, length, stride, bases, digest_off, flags, has_copy, has_flag):
    if nbases < 1 or nbases > MAX_RING or digest_off != -32 or length == 0 or per_base == 0 or flags:
        return None
    aligned = stride % 16 == 0
    for b in range(nbases):
        if has_copy[b] or not has_flag[b]:
            return None
        aligned = aligned and bases[b] % 16 == 0
    if aligned:
        return None
    odd = stride % 2 != 0 or any(b % 2 for b in bases[:nbases])
    if nbases > 12 and odd:
        return None
    steps = (length + STEP - 1) // STEP
    blocks = (per_base + RING_RECORDS - 1) // RING_RECORDS
    if steps > 0xffffffff or blocks > 0x7fffffff or 3 * stride >= 1 << 32:
        return None
    return dict(blocks=blocks, nf=nbases, rd=3 if nbases <= 12 else 2, steps=steps)


def line(p):
    """One pick as verify_pick_main prints it."""
    if p.kind == "ring":
        return "ring nf=%d rd=%d blocks=%d steps=%d" % (p.nf, p.rd, p.blocks, p.steps)
    if p.kind == "quad":
        return "quad copy=%d depth=%d unal=%d blocks=%d" % (p.copy, p.depth, int(p.unal), p.blocks)
    return p.kind


# -- the fixed table both sides evaluate (verify_pick_main.cpp walks the same loops) --------------

T_NBASES = list(range(0, 18)) + [32]
T_PER_BASE = [0, 1, 5]
T_LEN = [0, 1, 511, 512, 513, 87382]
T_PAD = [0, 1, 6, 16]           # stride = 32 + len + pad
T_PLACE = 5                     # base placements, table_base()
T_VARIANT = 5                   # flag / copy variants, table_variant()
T_TUNING = [(2, True, False), (1, True, False), (3, True, False), (2, False, False), (2, True, True), (1, True, True),
            (3, False, True)]
T_ORIGIN = 0x7F0000000000


def table_base(place, b):
    res = (0, 6, 1, (3 * b) % 16, 2 if b == 0 else 0)[place]
    return T_ORIGIN + b * 0x100000 + res


def table_variant(v, nbases):
    """(flags, digest_off, has_copy, has_flag): the verify launch; a copy
    target on file 0; one flag array for the launch; the last file a digest
    target (no flag); digests 16 bytes before the body."""
    has_copy, has_flag = [False] * nbases, [True] * nbases
    flags, digest_off = False, -32
    if v == 1 and nbases:
        has_copy[0] = True
    elif v == 2:
        flags, has_flag = True, [False] * nbases
    elif v == 3 and nbases:
        has_flag[nbases - 1] = False
    elif v == 4:
        digest_off = -16
    return flags, digest_off, has_copy, has_flag


# (nbases, per_base, len, stride): the ring's and the grid's 32-bit limits
T_LIMITS = [
    (4, (1 << 33) + 4, 100, 134), (4, 1 << 36, 100, 134), (4, 1 << 33, 100, 134),
    (4, 3, 1000, 1431655765), (4, 3, 1000, 1431655766), (4, 3, 1 << 41, 38), (4, 3, ((1 << 32) - 1) * 512, 38),
    (1, 1 << 37, 7, 39), (1, (1 << 37) - 64, 7, 39), (16, 1 << 33, 7, 39), (13, 1 << 20, 7, 38),
]


def table():
    """Every input of the fixed table, as keyword arguments of pick()."""
    for nb in T_NBASES:
        for per in T_PER_BASE:
            for ln in T_LEN:
                for pad in T_PAD:
                    for place in range(T_PLACE):
                        for v in range(T_VARIANT):
                            flags, doff, hc, hf = table_variant(v, nb)
                            for depth, unal, direct in T_TUNING:
                                yield dict(nbases=nb, per_base=per, length=ln, stride=32 + ln + pad,
                                           bases=[table_base(place, b) for b in range(nb)],
                                           n=nb * per if nb else per, digest_off=doff, flags=flags, has_copy=hc,
                                           has_flag=hf, depth=depth, unal=unal, direct_copy=direct,
                                           data=table_base(place, 0), shard_pitch=ln + pad)
    for nb, per, ln, stride in T_LIMITS:
        yield dict(nbases=nb, per_base=per, length=ln, stride=stride, bases=[table_base(1, b) for b in range(nb)])


# -- the callers (rsgpu.cpp) ---------------------------------------------------------------------

def verify_group(addrs, S, lo, hi, copy=(), role="", **tuning):
    """launch_verify_group: the files at `addrs` (in list order), records
    [lo, hi), up to 32 files a launch; copy[i]: file i has a copy target."""
    rec = 32 + S
    out = []
    for g0 in range(0, len(addrs), MAX_BASES):
        g = addrs[g0:g0 + MAX_BASES]
        hc = [bool(copy) and copy[g0 + x] for x in range(len(g))]
        out.append(pick(len(g), hi - lo, S, rec, [a + lo * rec + 32 for a in g], has_copy=hc, role=role, **tuning))
    return out


def get_all_present(data_addrs, parity_addrs, S, n, rotten_stripes, **tuning):
    """The in-place GET with every data file present: verify_data_begin, then
    verify_parity_rest over the span of the stripes with a rotten data record."""
    out = verify_group(data_addrs, S, 0, n, role="data", **tuning)
    if rotten_stripes and parity_addrs:
        lo, hi = min(rotten_stripes), max(rotten_stripes) + 1
        out += verify_group(parity_addrs, S, lo, hi, role="parity lo=%d of %d" % (lo, n), **tuning)
    return out


def whole_file(addrs, file_lens, part_size, shard_size, **tuning):
    """rsg_bitrot_verify_dev with the right want_size: a short file's complete
    records in a launch of its own, then the full records of the other files
    (32 a launch), then their short last records.  [(files, pick)]."""
    hs = 32
    full, tail = part_size // shard_size, part_size % shard_size
    recs, rec = full + (1 if tail else 0), hs + shard_size
    want = recs * hs + part_size
    avail, bulk_full, bulk_tail = [], [], []
    for f, ln in enumerate(file_lens):
        ln = min(ln, want)
        a = min(ln // rec, full)
        if a == full and tail and ln - full * rec >= hs + tail:
            a = recs
        avail.append(a)
        if not a:
            continue
        if a >= full and full:
            bulk_full.append(f)
        if a > full:
            bulk_tail.append(f)
    out = []
    for f, a in enumerate(avail):
        if a and a < full:
            out.append(([f], pick(1, a, shard_size, rec, [addrs[f] + hs], n=a, role="short", **tuning)))
    for which, lst in (("full", bulk_full), ("tail", bulk_tail)):
        for g0 in range(0, len(lst), MAX_BASES):
            g = lst[g0:g0 + MAX_BASES]
            role = which + (" split%d" % (g0 // MAX_BASES) if len(lst) > MAX_BASES else "")
            if which == "full":
                p = pick(len(g), full, shard_size, rec, [addrs[f] + hs for f in g], role=role, **tuning)
            else:
                p = pick(len(g), 1, tail, rec, [addrs[f] + full * rec + hs for f in g], role=role, **tuning)
            out.append((g, p))
    return out


# -- the arena -----------------------------------------------------------------------------------

def place(sizes, residues):
    """Offsets of files of `sizes` bytes in one arena whose base is 16-byte
    aligned: file i at the next offset that is residues[i] mod 16 and leaves
    at least one filler byte after its predecessor; (offsets, arena bytes) with
    filler after the last file too."""
    offs, at = [], 0
    for size, res in zip(sizes, residues):
        at += 1
        at += (res - at) % 16
        offs.append(at)
        at += size
    return offs, at + 24


RESIDUES = {
    "six": lambda i: 6,                     # the pitch of RS(12,4) at 1 MiB blocks: 6 mod 16
    "alt60": lambda i: 6 if i % 2 == 0 else 0,
    "odd": lambda i: (2 * i + 1) % 16,
    "mis8": lambda i: (5 * i + 3) % 16,     # every residue mod 8 (and mod 16) within 16 files
    "zero": lambda i: 0,
    "even": lambda i: (6 * i) % 16,         # 0, 6, 12, 2, 8, 14, 4, 10
}
PARITY_RESIDUES = (5, 8)  # one of the two shifted parity bases is odd whatever lo * pitch is


def residues(pattern, count):
    return [RESIDUES[pattern](i) for i in range(count)]


# -- the sweeps ----------------------------------------------------------------------------------

GetRow = namedtuple("GetRow", "k S n pattern depth")


def ring_rows(nf):
    """The in-place GET rows of the ring kernel of nf files, depth 2: each row
    owns a class of ring_classes (first column of the comment)."""
    if nf <= 12:
        return [GetRow(nf, 512, 5, "six", 2),     # a whole last step; aligned pitch, bases at 6; 2 workgroups
                GetRow(nf, 1025, 2, "odd", 2),    # 3 steps; records = 2 mod 4; odd pitch and bases
                GetRow(nf, 256, 3, "alt60", 2),   # ragged, whole packets only; records = 3 mod 4
                GetRow(nf, 2049, 8, "odd", 2),    # >= 4 steps; records = 0 mod 4
                GetRow(nf, 513, 1, "alt60", 2),   # 2 steps; one record
                GetRow(nf, 255, 4, "six", 2)]     # ragged: 7 packets + 31 bytes
    # even addresses only: whole steps from LENGTHS, ragged ones from EXTRA_LENGTHS
    return [GetRow(nf, 512, 5, "six", 2),         # records = 1 mod 4
            GetRow(nf, 1536, 2, "alt60", 2),      # 3 steps; records = 2 mod 4
            GetRow(nf, 256, 3, "alt60", 2),       # ragged, whole packets only; records = 3 mod 4
            GetRow(nf, 2050, 8, "even", 2),       # >= 4 steps; a last step below 32 bytes
            GetRow(nf, 1024, 4, "six", 2),        # 2 steps
            GetRow(nf, 258, 4, "six", 2)]         # ragged: 8 packets + 2 bytes


def quad_rows(depth):
    """16 data files (past the ring) at even bases: the quad kernel at this
    depth for an even pitch, and at depths 1 and 3 (no funnel there) for an odd
    one; the launch of 4 aligned files is the one the ring leaves to it.  Each
    row owns a batch count.  (Depth 2 hashes remainders of 1 and 31 bytes in
    the whole-file sweep's tail launches.)"""
    if depth == 2:
        return [GetRow(16, 32, 5, "even", 2), GetRow(16, 256, 9, "even", 2), GetRow(16, 512, 3, "even", 2),
                GetRow(16, 768, 2, "even", 2), GetRow(4, 1024, 8, "zero", 2)]
    return [GetRow(16, 33, 8, "even", depth), GetRow(16, 256, 9, "even", depth), GetRow(16, 512, 3, "even", depth),
            GetRow(16, 1023, 2, "even", depth), GetRow(4, 1024, 8, "zero", depth)]


def unal_rows():
    """Odd pitches past the ring (16 files; 13 at odd addresses): the funnel."""
    return [GetRow(16, 31, 9, "mis8", 2), GetRow(16, 257, 8, "mis8", 2), GetRow(16, 513, 3, "odd", 2),
            GetRow(16, 1023, 2, "mis8", 2), GetRow(13, 1025, 5, "mis8", 2)]


def get_rows():
    return ([r for nf in range(1, MAX_RING + 1) for r in ring_rows(nf)] + [r for d in (1, 2, 3) for r in quad_rows(d)]
            + unal_rows())


WholeRow = namedtuple("WholeRow", "files S full tail pattern depth mix", defaults=("all",))

# (shard size, full records, tail bytes) of the calls of 1..15 files
_WHOLE_SHAPES = [(513, 3, 1), (1024, 1, 1023), (33, 9, 0), (512, 2, 511), (257, 0, 256), (2049, 2, 1), (256, 4, 255),
                 (1025, 5, 0), (32, 8, 31), (511, 1, 0), (1536, 3, 1535), (255, 9, 1), (31, 6, 30), (1, 7, 0),
                 (513, 4, 512)]


def whole_rows():
    """bitrot_verify_batch calls of 1..15, 16, 17, 32 and 33 files; 0..9 full
    records and tails of 0, 1 and S - 1 bytes.  The calls of 16 files and more
    are past the ring: at aligned files and an even shard size the depth-2 quad
    kernel hashes tails of 1 and S - 1 bytes (remainders 1 and 31).  Two calls
    of 33 files, every file complete so that both the full-record and the tail
    launches are split at 32 files: file 32, alone in the second launch, is
    rotten in a full record in one call and in its tail record in the other."""
    rows = [WholeRow(nf, S, full, tail, ("six", "odd", "alt60")[nf % 3], 2)
            for nf, (S, full, tail) in zip(range(1, 16), _WHOLE_SHAPES)]
    rows += [WholeRow(16, 512, 3, 1, "zero", 2), WholeRow(17, 512, 2, 511, "zero", 2),
             WholeRow(32, 513, 3, 512, "mis8", 2), WholeRow(33, 1025, 2, 1, "six", 2, "full"),
             WholeRow(33, 257, 3, 256, "odd", 2, "tail")]
    return rows


# How a file of a whole-file call differs from the healthy one, in list order.
# "short": cut inside the full records, at least one of them complete (a
# launch of its own); "short_rot": the same with its first record rotten.
OUTCOMES = ["healthy", "rot_first", "rot_tail", "cut_body", "short", "rot_middle", "cut_header", "cut_records",
            "trailing", "rot_last", "empty", "short_rot", "healthy"]
COMPLETE = ["healthy", "rot_first", "trailing", "rot_tail", "healthy", "rot_middle", "rot_last"]  # every record there


def whole_want(row):
    """bitrot_shard_file_size of a row's part."""
    return row.full * (32 + row.S) + ((32 + row.tail) if row.tail else 0)


def whole_files(row):
    """[(outcome, file length, offset of the rotten byte or None)] of a row's
    files.  An outcome the shape has no room for becomes a neighbouring one:
    no tail record to rot -> the last full record; fewer than 2 records ->
    a cut inside the body; fewer than 2 full records -> no short file."""
    S, full, tail = row.S, row.full, row.tail
    rec = 32 + S
    nrec = full + (1 if tail else 0)
    want = full * rec + ((32 + tail) if tail else 0)
    last = (nrec - 1) * rec  # where the last record begins
    last_len = tail or S
    out = []
    for i in range(row.files):
        o = OUTCOMES[(i + row.files) % len(OUTCOMES)]
        if row.mix != "all":
            o = COMPLETE[i % len(COMPLETE)] if i < MAX_BASES else "rot_last" if row.mix == "full" else "rot_tail"
        if nrec == 0:
            o = "healthy" if o != "trailing" else o
        if o in ("short", "short_rot") and full < 2:
            o = "cut_body"
        if o == "cut_records" and nrec < 2:
            o = "cut_body"
        if o == "rot_tail" and not tail:
            o = "rot_last"
        if o in ("rot_middle", "rot_last", "rot_first") and not full:
            o = "rot_tail"
        spots = lambda n: rot_spots(n)[(i + row.files) % len(rot_spots(n))]
        length, rot = want, None
        if o == "rot_first" or o == "short_rot":
            rot = spots(S)
        elif o == "rot_middle":
            rot = (full // 2) * rec + spots(S)
        elif o == "rot_last":
            rot = (full - 1) * rec + spots(S)
        elif o == "rot_tail":
            rot = full * rec + spots(tail)
        if o == "cut_body":
            length = last + 32 + last_len // 2
        elif o == "cut_header":
            length = last + 7
        elif o == "cut_records":
            length = last
        elif o in ("short", "short_rot"):
            length = (full - 1) * rec + 9
        elif o == "trailing":
            length = want + 1
        elif o == "empty":
            length = 0
        out.append((o, length, rot))
    return out


# Shapes of the tests that are not sweeps: (k, S, n, residues) picked so that
# the data launch is the named kernel; "parity": a ring GET whose parity check
# runs over a proper sub-range.
NAMED = {
    "ring": GetRow(5, 1025, 5, "odd", 2), "ring2": GetRow(14, 258, 5, "six", 2),
    "quad": GetRow(16, 512, 5, "even", 2), "unal": GetRow(16, 513, 9, "mis8", 2),
    "parity": GetRow(3, 513, 8, "six", 2),
}
LARGER = {"ring": GetRow(5, 1025, 9, "odd", 2), "quad": GetRow(16, 512, 9, "even", 2),
          "unal": GetRow(16, 513, 5, "mis8", 2), "parity": GetRow(3, 513, 9, "six", 2)}


def get_layout(row):
    """(offsets of the k + M files, arena bytes) of a GET row."""
    res = residues(row.pattern, row.k) + list(PARITY_RESIDUES)
    return place([row.n * (32 + row.S)] * (row.k + M), res)


def rot_spots(S):
    """Offsets in a record of the bytes a test rots, in cycle order: a digest
    byte, the first body byte, the last byte of a whole packet, either side of
    a 512-byte step boundary, the last body byte."""
    spots = [5, 32]
    if S >= 32:
        spots.append(32 + (S // 32) * 32 - 1)
    if S > 512:
        spots += [32 + 511, 32 + 512]
    return spots + [32 + S - 1]


def get_rot(row):
    """[(file, stripe, offset in the record)] of a row's rotten batch: at most
    M a stripe; the last stripe's record of file 0 always; from 3 stripes on a
    second record of file 0; from 2 stripes on no rot in stripe 0, so the
    parity check starts past it."""
    k, n = row.k, row.n
    recs = [(0, n - 1)]
    if k >= 2:
        recs.append((k - 1, n - 1))
    if n >= 3:
        recs.append((0, 1))
    if n >= 5 and k >= 3:
        recs.append((k // 2, n - 2))
    spots = rot_spots(row.S)
    return [(f, s, spots[(i + k + n) % len(spots)]) for i, (f, s) in enumerate(recs)]


def get_picks(row, rot=None):
    offs, _ = get_layout(row)
    stripes = sorted({s for f, s, _ in (get_rot(row) if rot is None else rot) if f < row.k})
    return get_all_present(offs[:row.k], offs[row.k:], row.S, row.n, stripes, depth=row.depth)


def whole_picks(row):
    lens = [ln for _, ln, _ in whole_files(row)]
    offs, _ = place(lens, residues(row.pattern, row.files))
    return whole_file(offs, lens, row.full * row.S + row.tail, row.S, depth=row.depth)


# -- classes -------------------------------------------------------------------------------------

def walk_classes(p):
    """The classes one data or whole-file launch reaches."""
    out = set()
    if p.kind == "ring":
        tail = p.len - (p.steps - 1) * STEP
        c = [("records%4", p.per_base % 4), ("steps", min(p.steps, 4)),
             ("tail", "whole" if tail == STEP else "<32" if tail < 32 else "packets" if tail % 32 == 0 else "rem")]
        if p.blocks >= 2:
            c.append(("workgroups", ">=2"))
        if tail != STEP and tail % 32:
            c.append(("tail%32", "nonzero"))
        out |= {("ring", p.nf) + x for x in c}
    elif p.kind == "quad" and p.copy == 0:
        fam = ("unal",) if p.unal else ("quad", p.depth)
        out.add(fam + ("batches", min(p.len // 256, 5)))
        if not p.unal:
            out.add(fam + ("rem", p.len % 32))
        else:
            for b in p.bases:
                out |= {fam + ("mis", (b + r * p.stride) % 8) for r in range(p.per_base)}
    return out


def row_classes(picks):
    out = set()
    for p in picks:
        role = p.role.split()[0] if p.role else ""
        if role == "parity":
            lo, n = int(p.role.split()[1][3:]), int(p.role.split()[3])
            if lo > 0 and p.per_base < n and any(b % 2 for b in p.bases):
                out.add(("parity", "sub-range lo > 0, odd base"))
            continue
        if role in ("short", "full", "tail"):  # the whole-file sweep: credited under its own name
            out |= {("whole-file", role) + c for c in walk_classes(p)}
            if role == "short":
                out.add(("whole-file", "short file", p.kind))
        else:
            out |= walk_classes(p)
    return out


def required():
    req = set()
    for nf in range(1, MAX_RING + 1):
        req |= {("ring", nf, "records%4", r) for r in range(4)} | {("ring", nf, "steps", s) for s in (1, 2, 3, 4)}
        req |= {("ring", nf, "tail", t) for t in ("whole", "<32", "packets", "rem")}
        req |= {("ring", nf, "workgroups", ">=2"), ("ring", nf, "tail%32", "nonzero")}
    for d in (1, 2, 3):
        req |= {("quad", d, "batches", b) for b in range(5)} | {("quad", d, "rem", 0)}
        # at depth 2 an odd remainder means an odd pitch and the funnel: the
        # plain kernel meets it in a whole-file call's tail launch
        req |= {(("quad", d, "rem", r) if d != 2 else ("whole-file", "tail", "quad", 2, "rem", r)) for r in (1, 31)}
    req |= {("unal", "mis", v) for v in range(8)} | {("unal", "batches", b) for b in range(5)}
    req |= {("whole-file", "split at 32", "full", "rot in the second launch"),
            ("whole-file", "split at 32", "tail", "rot in the second launch"),
            ("whole-file", "short file", "ring"), ("whole-file", "short file", "quad"),
            ("parity", "sub-range lo > 0, odd base")}
    req |= {("whole-file", "files", nf) for nf in list(range(1, 16)) + [16, 17, 32, 33]}
    return req


def sweep_classes(get=None, whole=None):
    """What the sweeps' rows reach: {class: [rows]}."""
    reach = {}
    for row in (get_rows() if get is None else get):
        for c in row_classes(get_picks(row)):
            reach.setdefault(c, []).append(row)
    for row in (whole_rows() if whole is None else whole):
        for c in whole_classes(row):
            reach.setdefault(c, []).append(row)
    return reach


def whole_classes(row):
    files, picks = whole_files(row), whole_picks(row)
    out = row_classes([p for _, p in picks]) | {("whole-file", "files", row.files)}
    rotten = {"full": ("rot_first", "rot_middle", "rot_last"), "tail": ("rot_tail",)}
    for g, p in picks:  # a split launch's second part: is the verdict of one of its files decided there?
        which = p.role.split()[0]
        if p.role.endswith("split1") and any(files[f][0] in rotten[which] for f in g):
            out.add(("whole-file", "split at 32", which, "rot in the second launch"))
    return out
