"""The same-length verify walks' shape sweeps (test_gpu_verify_walks.py) leave
no built kernel shape out.  The kernel choice is plain C++
(rustfs_amd/csrc/rs_verify_pick.h); tests/host/verify_pick_main.cpp evaluates
it over a fixed table under AddressSanitizer + UBSan and checks its structural
facts; verify_shapes.py restates it, and the callers that build the launches,
in Python.  Here: the restatement equals the shipped pick line by line, and the
sweeps' rows, run through it, reach every class of verify_shapes.required() —
a missing class is named, and every row owns one.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

import verify_shapes as V
from conftest import ROOT


@pytest.fixture(scope="module")
def pick_program(tmp_path_factory):
    """verify_pick_main built with the host compiler under ASan + UBSan (the
    _build_and_run recipe of test_blocks_plan.py, keeping the program)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("verify_pick") / "verify_pick_main")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-o", exe,
                            os.path.join(ROOT, "tests", "host", "verify_pick_main.cpp")],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    return exe


def test_restated_pick_equals_the_shipped_one(pick_program):
    """Every line of the fixed table (19 file counts x 3 record counts x 6
    lengths x 4 pitches x 5 placements x 5 flag / copy variants x 7 tunings,
    and the 32-bit limits); the program's own CHECKs are the structural facts:
    no ring with a copy target, none when everything is 16-byte aligned, none
    past 12 files at an odd address or past 15 at all, the funnel only at depth
    2 with hash_unal, the grid and DMA offset limits."""
    run = subprocess.run([pick_program], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    got = run.stdout.splitlines()
    assert got[-1] == "verify pick ok"
    n = 0
    for n, (kw, have) in enumerate(zip(V.table(), got[:-1]), 1):
        want = V.line(V.pick(**kw))
        assert have == want, (n, kw, have, want)
    assert n == len(got) - 1 == 19 * 3 * 6 * 4 * 5 * 5 * 7 + len(V.T_LIMITS)
    kinds = {l.split()[0] for l in got[:-1]}
    assert kinds == {"none", "invalid", "ring", "quad"}
    # every instantiation appears in the table: 15 rings, 3 x 3 quad forms, the funnel
    assert {l.split()[1] for l in got if l.startswith("ring")} == {"nf=%d" % nf for nf in range(1, 16)}
    assert len({l.rsplit(" ", 1)[0] for l in got if l.startswith("quad")}) == 10


def test_real_call_shapes(pick_program):
    """The picks of rustfs's default geometries at 1 MiB blocks, as worked out
    by hand from the conditions: pitch 32 + ceil(2^20 / k), files in aligned
    allocations, so only the pitch decides."""
    want = {
        (8, 4): ("quad copy=0 depth=2 unal=0", "quad copy=0 depth=2 unal=0"),     # 131104 = 0 mod 16: aligned
        (12, 4): ("ring nf=12 rd=3", "quad copy=0 depth=2 unal=0"),              # 87414 = 6 mod 16; 16 files: quad
        (6, 4): ("ring nf=6 rd=3", "ring nf=10 rd=3"),                           # 174795 odd, up to 12 files
        (10, 4): ("ring nf=10 rd=3", "ring nf=14 rd=2"),                         # 104890 = 10 mod 16, even
        (14, 2): ("quad copy=0 depth=2 unal=1", "quad copy=0 depth=2 unal=1"),   # 74931 odd, 14 and 16 files
    }
    for (k, m), (get, whole) in want.items():
        run = subprocess.run([pick_program, str(k), str(m), str(1 << 20)], capture_output=True, text=True, timeout=60)
        assert run.returncode == 0, run.stderr
        a, b = run.stdout.splitlines()
        assert "all-present GET of %d files: %s" % (k, get) in a, a
        assert "whole-file verify of %d files: %s" % (k + m, whole) in b, b


def test_layout_and_rows_are_what_they_claim():
    """Lengths and record counts come from the stated sets; files sit at their
    residues with filler on both sides; the rot of every GET row keeps to M a
    stripe, hits the last stripe and, from two stripes on, spares stripe 0."""
    for row in V.get_rows() + list(V.NAMED.values()) + list(V.LARGER.values()):
        assert row.S in V.LENGTHS + V.EXTRA_LENGTHS and row.n in V.RECORDS and 1 <= row.k <= 16
        offs, size = V.get_layout(row)
        res = V.residues(row.pattern, row.k) + list(V.PARITY_RESIDUES)
        span = row.n * (32 + row.S)
        assert [o % 16 for o in offs] == res and offs[0] >= 1 and size > offs[-1] + span
        assert all(b - a > span for a, b in zip(offs, offs[1:]))
        rot = V.get_rot(row)
        per_stripe = {}
        for f, s, at in rot:
            assert f < row.k and 0 <= at < 32 + row.S
            per_stripe[s] = per_stripe.get(s, 0) + 1
        assert len(set((f, s) for f, s, _ in rot)) == len(rot) and max(per_stripe.values()) <= V.M
        assert row.n - 1 in per_stripe and (row.n == 1 or 0 not in per_stripe)
    assert any(sum(1 for f, _, _ in V.get_rot(r) if f == 0) == 2 for r in V.get_rows())
    spots = set()
    for row in V.get_rows():
        spots |= {(at if at < 64 else "last" if at == 31 + row.S else at) for _, _, at in V.get_rot(row)}
    assert {5, 32, 63, 32 + 511, 32 + 512, "last"} <= spots
    assert sorted(r.files for r in V.whole_rows()) == list(range(1, 16)) + [16, 17, 32, 33, 33]
    outcomes = set()
    for row in V.whole_rows():
        assert row.S in V.LENGTHS and 0 <= row.full <= 9 and row.tail in (0, 1, row.S - 1)
        files = V.whole_files(row)
        outcomes |= {o for o, _, _ in files}
        for o, length, rot in files:
            assert rot is None or rot < length
        if row.mix != "all":  # every file of a split call is complete; the 33rd is the rotten one
            assert all(length >= V.whole_want(row) for _, length, _ in files) and files[32][2] is not None
    assert outcomes == set(V.OUTCOMES)
    assert {r.full for r in V.whole_rows()} == set(range(10)) and {(r.tail > 1) - (r.tail == 0) for r in V.whole_rows()} == {-1, 0, 1}


def test_named_shapes_take_their_kernel():
    """The shapes of the neighbouring-bytes and no-memory tests run the kernel
    they are named after, and "parity" re-verifies over a proper sub-range."""
    for table in (V.NAMED, V.LARGER):
        for name, row in table.items():
            data = V.get_picks(row, rot=[])
            assert len(data) == 1
            p = data[0]
            if name in ("ring", "parity"):
                assert p.kind == "ring" and p.rd == 3
            elif name == "ring2":
                assert p.kind == "ring" and p.rd == 2
            elif name == "quad":
                assert p.kind == "quad" and not p.unal and p.copy == 0
            else:
                assert p.kind == "quad" and p.unal
    assert ("parity", "sub-range lo > 0, odd base") in V.row_classes(V.get_picks(V.NAMED["parity"]))
    for name in V.LARGER:
        assert V.LARGER[name].n != V.NAMED[name].n and V.LARGER[name][:2] == V.NAMED[name][:2]


def test_sweeps_reach_every_class():
    reach = V.sweep_classes()
    missing = sorted(V.required() - set(reach), key=repr)
    assert not missing, "no row of the GPU sweeps reaches: %r" % (missing,)


def test_every_row_owns_a_class():
    """Without any one row of a sweep a required class is left out: the rows
    are no more than the classes need, and a deleted row is noticed."""
    reach = V.sweep_classes()
    req = V.required()
    owned = {}
    for c in req:
        rows = reach[c]
        if len(set(rows)) == 1:
            owned.setdefault(rows[0], []).append(c)
    rows = V.get_rows() + V.whole_rows()
    assert len(set(rows)) == len(rows)
    idle = [r for r in rows if r not in owned]
    assert not idle, "rows that no required class depends on: %r" % (idle,)


def test_a_deleted_row_is_named():
    """The check of test_sweeps_reach_every_class with one row taken out, for
    a row of each sweep: the message names the class."""
    get = [r for r in V.get_rows() if r != V.GetRow(14, 2050, 8, "even", 2)]
    missing = V.required() - set(V.sweep_classes(get=get))
    assert missing == {("ring", 14, "steps", 4), ("ring", 14, "tail", "<32")}
    whole = [r for r in V.whole_rows() if r.mix != "tail"]
    missing = V.required() - set(V.sweep_classes(whole=whole))
    assert missing == {("whole-file", "split at 32", "tail", "rot in the second launch")}
