"""Gathered block encode, the parts that need no GPU: the host planner
(rustfs_amd/csrc/rs_blocks_plan.h) checked by a stand-alone C++ program built
with the host compiler under AddressSanitizer + UBSan, and the new C-ABI
entries' argument checks."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _build_and_run(tmp_path, name, sanitize, marker, run_timeout, extra=()):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / (name + "_" + sanitize.replace(",", "_")))
    src = os.path.join(ROOT, "tests", "host", name + ".cpp")
    # the sanitizer runtimes linked statically (g++ links them dynamically by
    # default; clang++ statically, and does not know g++'s flag names)
    static = []
    if "clang" not in os.path.basename(cxx):
        static = ["-static-lib" + {"address": "asan", "undefined": "ubsan", "thread": "tsan"}[s]
                  for s in sanitize.split(",")]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread",
                            "-fsanitize=" + sanitize, "-fno-sanitize-recover=all", *static, *extra, "-o", exe, src],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=run_timeout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert marker in run.stdout


def test_planner_program_under_sanitizers(tmp_path):
    """tests/host/blocks_plan_main.cpp: every rejection, overlap detection
    among parity, digest and data ranges in either list order, tile tables
    that cover every byte once (lengths 1, kTile-1, kTile, kTile+1, 3*kTile+5),
    a unit table that is a permutation in non-increasing length, sub-batch
    splits with an oversized block, and the copy and launch counts of an
    all-pinned, an all-pageable and a mixed batch, with and without digests."""
    _build_and_run(tmp_path, "blocks_plan_main", "address,undefined", "blocks plan ok", 120)


def test_block_entries_reject_null_context(rsgpu_lib):
    """The new entries check their context first (no device needed) and leave
    their outputs untouched."""
    from rustfs_amd import _lib
    k, m, S = 4, 2, 64
    buf = np.full((k + m) * S, 0xA5, dtype=np.uint8)
    dig = np.full((k + m) * 32, 0xA5, dtype=np.uint8)
    ptrs = (ctypes.c_void_p * (k + m))(*[buf.ctypes.data + i * S for i in range(k + m)])
    blk = _lib.rsg_block(ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p)), S, dig.ctypes.data)
    assert rsgpu_lib.rsg_encode_blocks(None, k, m, 1, ctypes.byref(blk), _lib.RSG_HASH_HIGHWAY256S) == _lib.RSG_ERR_INVALID_ARG
    assert rsgpu_lib.rsg_encode_hashed(None, k, m, S, ptrs, dig.ctypes.data, _lib.RSG_HASH_HIGHWAY256S) == _lib.RSG_ERR_INVALID_ARG
    assert (buf == 0xA5).all() and (dig == 0xA5).all()


def test_constants_match_header():
    from rustfs_amd import _lib
    src = open(os.path.join(ROOT, "include", "rsgpu.h")).read()
    m = re.search(r"#define\s+RSG_BLOCKS_STAGE_BYTES\s+\((\d+)u\s*<<\s*(\d+)\)", src)
    assert m and (int(m.group(1)) << int(m.group(2))) == _lib.RSG_BLOCKS_STAGE_BYTES
    assert ctypes.sizeof(_lib.rsg_block) == 24


def test_python_surface_checks_blocks():
    """Erasure.encode_blocks refuses a wrong shard count, shards of unequal
    length and a wrongly sized digest array before anything reaches the
    library."""
    from rustfs_amd import Erasure, _lib
    from rustfs_amd._lib import RsgError
    e = Erasure(2, 1, 1 << 20)
    s = [np.zeros(8, np.uint8) for _ in range(3)]
    with pytest.raises(RsgError) as err:
        e.encode_blocks([s[:2]])
    assert err.value.code == _lib.RSG_ERR_INVALID_SHARD_COUNT
    with pytest.raises(RsgError) as err:
        e.encode_blocks([[s[0], s[1], np.zeros(9, np.uint8)]])
    assert err.value.code == _lib.RSG_ERR_INCONSISTENT_LENGTH
    with pytest.raises(TypeError):
        e.encode_blocks([s], digests=[np.zeros(95, np.uint8)])
    with pytest.raises(TypeError):
        e.encode_blocks([s], digests=[])
