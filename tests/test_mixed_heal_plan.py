"""Mixed-length batch heal, the parts that need no GPU: the host planner
(rustfs_amd/csrc/rs_mixed_heal_plan.h: validation of target ranges, the heal
plan of a mask, grouping, kernel ordering, sub-batch splitting, redo from
verify flags) checked by a stand-alone C++ program built with the host compiler
and AddressSanitizer + UBSan, and the argument checks of the two C-ABI entries
and of the Python surface."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def test_heal_planner_program_under_sanitizers(tmp_path):
    """tests/host/mixed_heal_plan_main.cpp (its own main): every rejection of
    the validation, zero-length stripes (their 32-byte target range counts),
    groups of 1, SPW and SPW+1 stripes out of three interleaved masks, masks
    with fewer than k readable non-target shards, R = e + surplus <= m for
    every mask of RS(4,2) and RS(8,4) with 1..m targets, the kernel order as a
    permutation with non-increasing chunk counts, sub-batches covering every
    stripe once, and redo regrouping ending within k+m rounds."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "mixed_heal_plan_main")
    src = os.path.join(ROOT, "tests", "host", "mixed_heal_plan_main.cpp")
    # the sanitizer runtimes linked statically (g++ links them dynamically by
    # default; clang++ statically, and does not know g++'s flag names)
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else []
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-o", exe, src],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mixed heal plan ok" in run.stdout


def test_heal_mixed_entries_reject_null_context(rsgpu_lib):
    """The two entries exist and check their context first (no device
    needed): RSG_ERR_INVALID_ARG."""
    from rustfs_amd import _lib
    assert rsgpu_lib.rsg_heal_mixed_dev(None, 4, 2, 0, None, None, None, _lib.RSG_HASH_HIGHWAY256S, None,
                                        None) == _lib.RSG_ERR_INVALID_ARG
    assert rsgpu_lib.rsg_heal_mixed_host(None, 4, 2, 0, None, None, None, _lib.RSG_HASH_HIGHWAY256S,
                                         None) == _lib.RSG_ERR_INVALID_ARG


def test_heal_entries_declared_and_exported():
    """Both entries are in the header and in _lib.EXPORTED, and the ABI
    version stayed 6."""
    import re
    from rustfs_amd import _lib
    src = open(os.path.join(ROOT, "include", "rsgpu.h")).read()
    for name in ("rsg_heal_mixed_dev", "rsg_heal_mixed_host"):
        assert re.search(r"\bint %s\(rsg_ctx \*ctx, int k, int m, size_t n, const rsg_record_desc \*h_desc," % name, src)
        assert name in _lib.EXPORTED
    assert re.search(r"#define RSG_ABI_VERSION 6\b", src)


def test_python_surface_refuses_stripe_outside_arena():
    """Erasure.heal_mixed_host checks every stripe against its source arenas
    and its target arenas before anything reaches the library (no device
    needed)."""
    from rustfs_amd import Erasure, _lib
    from rustfs_amd._lib import RsgError
    e = Erasure(4, 2, 1 << 20)
    files = [np.zeros(100, np.uint8) for _ in range(6)]
    files[1] = None
    targets = [None] * 6
    targets[1] = np.zeros(60, np.uint8)
    bad = (
        [[59, 0, 10, 0x3f]],           # record [59, 101) past its 100-byte arena
        [[0, 19, 10, 0x3f]],           # target record [19, 61) past the 60-byte target arena
        [[0, 29, 0, 0x3f]],            # ... a bare digest [29, 61) too
        [[2 ** 64 - 1, 0, 10, 0x3f]],  # would wrap
        [[0, 2 ** 64 - 1, 10, 0x3f]],
        [[0, 0, 2 ** 32, 0x3f]],       # shard_len does not fit the descriptor
    )
    for desc in bad:
        with pytest.raises(RsgError) as err:
            e.heal_mixed_host(files, targets, desc)
        assert err.value.code == _lib.RSG_ERR_INVALID_ARG, desc
    # a short source arena matters only to the stripes that may read it ...
    files[5] = np.zeros(10, np.uint8)
    with pytest.raises(RsgError) as err:
        e.heal_mixed_host(files, targets, [[0, 0, 10, 0x3f]])
    assert err.value.code == _lib.RSG_ERR_INVALID_ARG
    # ... and a second, shorter target arena to every stripe
    files[5] = None
    targets[5] = np.zeros(41, np.uint8)
    with pytest.raises(RsgError) as err:
        e.heal_mixed_host(files, targets, [[0, 0, 10, 0x3f]])
    assert err.value.code == _lib.RSG_ERR_INVALID_ARG
    with pytest.raises(RsgError) as err:
        e.heal_mixed_host(files[:5], targets, [[0, 0, 10, 0x1f]])
    assert err.value.code == _lib.RSG_ERR_INVALID_SHARD_COUNT
    with pytest.raises(RsgError) as err:
        e.heal_mixed_host(files, targets[:5], [[0, 0, 10, 0x1f]])
    assert err.value.code == _lib.RSG_ERR_INVALID_SHARD_COUNT
    with pytest.raises(TypeError):
        e.heal_mixed_host(files, [None if g is None else g.astype(np.uint16) for g in targets], [[0, 0, 10, 0x1f]])
    ro = np.zeros(60, np.uint8)
    ro.setflags(write=False)
    with pytest.raises((ValueError, TypeError, RsgError)):
        e.heal_mixed_host(files, [None, ro, None, None, None, None], [[0, 0, 10, 0x1f]])
