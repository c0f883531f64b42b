"""Mixed-length batch encode, the parts that need no GPU: the host planner
(rustfs_amd/csrc/rs_mixed_plan.h: validation, kernel ordering, sub-batch
splitting) checked by a stand-alone C++ program built with the host compiler
and AddressSanitizer + UBSan, and the new C-ABI entries' argument checks."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_planner_program_under_sanitizers(tmp_path):
    """tests/host/mixed_plan_main.cpp (its own main) feeds the planner valid
    tables (zero-length stripes, the aliased a3 layout, n in {0, 1, SPW,
    SPW+1}), every rejection, and sub-batch splits with an oversized stripe;
    it checks that the kernel order is a permutation with non-increasing chunk
    counts and that the sub-batches cover every stripe once, in order."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "mixed_plan_main")
    src = os.path.join(ROOT, "tests", "host", "mixed_plan_main.cpp")
    # the sanitizer runtimes linked statically (g++ links them dynamically by
    # default; clang++ statically, and does not know g++'s flag names)
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else []
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-o", exe, src],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mixed plan ok" in run.stdout


def test_mixed_entries_reject_null_context(rsgpu_lib):
    """The three entries exist and check their context first (no device
    needed): RSG_ERR_INVALID_ARG."""
    import ctypes
    from rustfs_amd import _lib
    tk = ctypes.c_uint64(7)
    assert rsgpu_lib.rsg_encode_mixed_dev(None, 4, 2, 0, None, None, None, None, 0, None) == _lib.RSG_ERR_INVALID_ARG
    assert rsgpu_lib.rsg_encode_mixed_host(None, 4, 2, 0, None, None, None, None, 0) == _lib.RSG_ERR_INVALID_ARG
    assert rsgpu_lib.rsg_encode_mixed_host_submit(None, 4, 2, 0, None, None, None, None, 0,
                                                  ctypes.byref(tk)) == _lib.RSG_ERR_INVALID_ARG
    assert tk.value == 0
    assert rsgpu_lib.rsg_encode_mixed_host_submit(None, 4, 2, 0, None, None, None, None, 0,
                                                  None) == _lib.RSG_ERR_INVALID_ARG


def test_stage_constant_matches_header():
    import re
    from rustfs_amd import _lib
    src = open(os.path.join(ROOT, "include", "rsgpu.h")).read()
    m = re.search(r"#define\s+RSG_MIXED_STAGE_BYTES\s+\((\d+)u\s*<<\s*(\d+)\)", src)
    assert m and (int(m.group(1)) << int(m.group(2))) == _lib.RSG_MIXED_STAGE_BYTES


def test_python_surface_checks_arenas():
    """Erasure.encode_mixed_host refuses a stripe outside its arena before
    anything reaches the library."""
    import numpy as np
    from rustfs_amd import Erasure, _lib
    from rustfs_amd._lib import RsgError
    e = Erasure(4, 2, 1 << 20)
    data, parity = np.zeros(40, np.uint8), np.zeros(20, np.uint8)
    for desc in ([[1, 0, 10]], [[0, 1, 10]], [[2 ** 64 - 1, 0, 10]]):
        with pytest.raises(RsgError) as err:
            e.encode_mixed_host(data, parity, desc)
        assert err.value.code == _lib.RSG_ERR_INVALID_ARG
