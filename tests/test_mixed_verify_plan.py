"""Mixed-length batch deep scan, the parts that need no GPU: the host planner
(rustfs_amd/csrc/rs_mixed_verify_plan.h: validation, expansion of files into
units, kernel order, sub-batch splitting, reduction of unit flags to per-file
verdicts) checked by a stand-alone C++ program built with the host compiler and
AddressSanitizer + UBSan, and the argument checks of the two C-ABI entries and
of the Python surface."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def test_verify_planner_program_under_sanitizers(tmp_path):
    """tests/host/mixed_verify_plan_main.cpp (its own main): every rejection of
    the validation; the unit expansion of parts of 0..3 full records with
    tails 0, 1 and shard_size - 1, of files cut mid-header, mid-body and at a
    record boundary, of longer files and of a size-mismatch file among healthy
    ones, every unit's header and body inside its file; the kernel order as a
    stable permutation with non-increasing batch counts; sub-batches covering
    every file once, in order, within the limit or alone; the reduction giving
    mismatch before EOF before trailing data."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "mixed_verify_plan_main")
    src = os.path.join(ROOT, "tests", "host", "mixed_verify_plan_main.cpp")
    # the sanitizer runtimes linked statically (g++ links them dynamically by
    # default; clang++ statically, and does not know g++'s flag names)
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else []
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-o", exe, src],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mixed verify plan ok" in run.stdout


def test_verify_mixed_entries_reject_null_context(rsgpu_lib):
    """The two entries exist and check their context first (no device
    needed): RSG_ERR_INVALID_ARG."""
    from rustfs_amd import _lib
    assert rsgpu_lib.rsg_bitrot_verify_mixed_dev(None, _lib.RSG_HASH_HIGHWAY256S, 1, None, 0, None, None,
                                                 None) == _lib.RSG_ERR_INVALID_ARG
    assert rsgpu_lib.rsg_bitrot_verify_mixed_host(None, _lib.RSG_HASH_HIGHWAY256S, 1, None, 0, None,
                                                  None) == _lib.RSG_ERR_INVALID_ARG


def test_verify_entries_declared_and_exported():
    """Both entries and their descriptor are in the header, the entries in
    _lib.EXPORTED, FILE_DESC_FIELDS has the struct's layout, and the ABI
    version stayed 6."""
    import re
    from rustfs_amd import _lib
    src = open(os.path.join(ROOT, "include", "rsgpu.h")).read()
    for name in ("rsg_bitrot_verify_mixed_dev", "rsg_bitrot_verify_mixed_host"):
        assert re.search(r"\bint %s\(rsg_ctx \*ctx, int algo, int n_arenas, const uint8_t \*const \*\w+,\s*"
                         r"size_t n, const rsg_file_desc \*h_desc, int \*h_status" % name, src)
        assert name in _lib.EXPORTED
    struct = re.search(r"typedef struct rsg_file_desc \{(.*?)\} rsg_file_desc;", src, re.S).group(1)
    fields = re.findall(r"(uint64_t|uint32_t) (\w+);", struct)
    assert [(n, "<u8" if t == "uint64_t" else "<u4") for t, n in fields] == list(_lib.FILE_DESC_FIELDS)
    assert np.dtype(list(_lib.FILE_DESC_FIELDS)).itemsize == 40
    assert re.search(r"#define RSG_ABI_VERSION 6\b", src)


def test_python_surface_refuses_file_outside_arena():
    """bitrot_verify_many checks every descriptor against its arena before
    anything reaches the library (no device needed)."""
    from rustfs_amd import _lib
    from rustfs_amd._lib import RsgError
    from rustfs_amd.bitrot import bitrot_verify_many
    arenas = [np.zeros(100, np.uint8), None, np.zeros(50, np.uint8)]
    bad = (
        [[1, 100, 100, 68, 68, 0]],          # [1, 101) past its 100-byte arena
        [[0, 51, 100, 68, 68, 2]],           # past the 50-byte arena
        [[0, 1, 33, 1, 1, 1]],               # a file with bytes in an arena that has none
        [[0, 0, 0, 0, 0, 3]],                # arena index out of range
        [[2 ** 64 - 1, 2, 34, 2, 2, 0]],     # would wrap
        [[0, 2 ** 64, 34, 2, 2, 0]],         # file_len does not fit the descriptor
        [[0, 34, 34, 2, 2 ** 32, 0]],        # shard_size does not fit the descriptor
        [[0, 34, 34, 2, 2, -1]],
        [[0, 33, 33, 1, 1, 0], [90, 11, 33, 1, 1, 0]],  # the second file is outside
    )
    for desc in bad:
        with pytest.raises(RsgError) as err:
            bitrot_verify_many(arenas, desc)
        assert err.value.code == _lib.RSG_ERR_INVALID_ARG, desc
    for n in (0, 33):
        with pytest.raises(RsgError) as err:
            bitrot_verify_many([None] * n, [])
        assert err.value.code == _lib.RSG_ERR_INVALID_ARG
    with pytest.raises(TypeError):
        bitrot_verify_many([np.zeros(100, np.uint16)], [[0, 33, 33, 1, 1, 0]])
    with pytest.raises(TypeError):
        bitrot_verify_many([np.zeros((10, 20), np.uint8)[:, :10]], [[0, 33, 33, 1, 1, 0]])
