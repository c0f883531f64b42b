"""Mixed-length batch GET, the parts that need no GPU: the host planner
(rustfs_amd/csrc/rs_mixed_decode_plan.h: validation, grouping by mask, kernel
ordering, sub-batch splitting, redo from verify flags) checked by a stand-alone
C++ program built with the host compiler and AddressSanitizer + UBSan, and the
argument checks of the two C-ABI entries and of the Python surface."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def test_decode_planner_program_under_sanitizers(tmp_path):
    """tests/host/mixed_decode_plan_main.cpp (its own main): every rejection
    of the validation, zero-length stripes, groups of 1, SPW and SPW+1 stripes
    out of three interleaved masks, masks with fewer than k bits, the kernel
    order as a permutation with non-increasing chunk counts inside a group,
    `job` mapping back to the caller's index, sub-batches covering every
    stripe once, and redo regrouping from a flag array ending within k+m
    rounds."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "mixed_decode_plan_main")
    src = os.path.join(ROOT, "tests", "host", "mixed_decode_plan_main.cpp")
    # the sanitizer runtimes linked statically (g++ links them dynamically by
    # default; clang++ statically, and does not know g++'s flag names)
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else []
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-o", exe, src],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mixed decode plan ok" in run.stdout


def test_decode_mixed_entries_reject_null_context(rsgpu_lib):
    """The two entries exist and check their context first (no device
    needed): RSG_ERR_INVALID_ARG."""
    from rustfs_amd import _lib
    assert rsgpu_lib.rsg_decode_mixed_dev(None, 4, 2, 0, None, None, _lib.RSG_HASH_HIGHWAY256S, 1, None, None, None,
                                          None) == _lib.RSG_ERR_INVALID_ARG
    assert rsgpu_lib.rsg_decode_mixed_host(None, 4, 2, 0, None, None, _lib.RSG_HASH_HIGHWAY256S, 1, None, None,
                                           None) == _lib.RSG_ERR_INVALID_ARG


def test_record_desc_layout_matches_header():
    """_lib.RECORD_DESC_FIELDS is rsg_record_desc: 24 bytes, the header's
    field order."""
    import re
    from rustfs_amd import _lib
    dt = np.dtype(list(_lib.RECORD_DESC_FIELDS))
    assert dt.itemsize == 24 and [dt.fields[n][1] for n in dt.names] == [0, 8, 16, 20]
    src = open(os.path.join(ROOT, "include", "rsgpu.h")).read()
    body = re.search(r"typedef struct rsg_record_desc \{(.*?)\} rsg_record_desc;", src, re.S).group(1)
    assert re.findall(r"uint(?:64|32)_t\s+(\w+);", body) == list(dt.names)


def test_python_surface_refuses_stripe_outside_arena():
    """Erasure.decode_mixed_host checks every stripe against its arenas
    before anything reaches the library (no device needed)."""
    from rustfs_amd import Erasure, _lib
    from rustfs_amd._lib import RsgError
    e = Erasure(4, 2, 1 << 20)
    files = [np.zeros(100, np.uint8) for _ in range(6)]
    out = np.zeros(40, np.uint8)
    bad = (
        [[59, 0, 10, 0x3f]],          # record [59, 101) past its 100-byte arena
        [[0, 1, 10, 0x3f]],           # out window [1, 41) past the 40-byte out arena
        [[2 ** 64 - 1, 0, 10, 0x3f]],  # would wrap
        [[0, 2 ** 64 - 1, 10, 0x3f]],
        [[0, 0, 2 ** 32, 0x3f]],      # shard_len does not fit the descriptor
    )
    for desc in bad:
        with pytest.raises(RsgError) as err:
            e.decode_mixed_host(files, desc, out)
        assert err.value.code == _lib.RSG_ERR_INVALID_ARG
    # a short arena matters only to the stripes that may read it
    files[5] = np.zeros(10, np.uint8)
    with pytest.raises(RsgError) as err:
        e.decode_mixed_host(files, [[0, 0, 10, 0x3f]], out)
    assert err.value.code == _lib.RSG_ERR_INVALID_ARG
    with pytest.raises(RsgError) as err:
        e.decode_mixed_host(files[:5], [[0, 0, 10, 0x1f]], out)
    assert err.value.code == _lib.RSG_ERR_INVALID_SHARD_COUNT
    with pytest.raises(TypeError):
        e.decode_mixed_host([f.astype(np.uint16) for f in files], [[0, 0, 10, 0x1f]], out)
