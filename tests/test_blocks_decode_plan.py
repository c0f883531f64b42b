"""Gathered block reconstruct, the parts that need no GPU: the host planner
(rustfs_amd/csrc/rs_blocks_decode_plan.h) checked by a stand-alone C++ program
built with the host compiler under AddressSanitizer + UBSan, and the new C-ABI
entry's and Erasure.decode_blocks' argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_blocks_plan import _build_and_run


def test_planner_program_under_sanitizers(tmp_path):
    """tests/host/blocks_decode_plan_main.cpp: every rejection, overlap
    detection in either list order, survivors / targets / group split of every
    RS(4,2) and RS(8,4) mask in three modes against a restatement by hand,
    pattern ids, entries and tile tables that cover every target byte once
    (lengths 1, kTile-1, kTile, kTile+1, 3*kTile+5), no entry without a target
    or with too few shards, effective masks from bad bytes, a hash-unit table
    that is a permutation in non-increasing length over present shards only,
    sub-batch splits with an oversized block, and the copy, launch and wait
    counts of all-pinned, all-pageable and mixed sub-batches, verified and
    not."""
    _build_and_run(tmp_path, "blocks_decode_plan_main", "address,undefined", "blocks decode plan ok", 120)


def test_entry_rejects_null_context(rsgpu_lib):
    """The new entry checks its context first (no device needed) and leaves
    every output untouched."""
    from rustfs_amd import _lib
    k, m, S = 4, 2, 64
    t = k + m
    buf = np.full(t * S, 0xA5, dtype=np.uint8)
    dig = np.full(t * 32, 0xA5, dtype=np.uint8)
    bad = np.full(t, 0xA5, dtype=np.uint8)
    present = np.array([0, 1, 1, 1, 1, 1], dtype=np.uint8)
    status = (ctypes.c_int * 1)(0x5A5A)
    ptrs = (ctypes.c_void_p * t)(*[buf.ctypes.data + i * S for i in range(t)])
    blk = _lib.rsg_rblock(ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p)), S, present.ctypes.data, dig.ctypes.data,
                          bad.ctypes.data)
    for mode in (_lib.RSG_RECONSTRUCT_DATA, _lib.RSG_RECONSTRUCT_MISSING, _lib.RSG_RECONSTRUCT_REENCODE_PARITY):
        assert rsgpu_lib.rsg_reconstruct_blocks(None, k, m, 1, ctypes.byref(blk), mode, _lib.RSG_HASH_HIGHWAY256S,
                                                status) == _lib.RSG_ERR_INVALID_ARG
    assert (buf == 0xA5).all() and (dig == 0xA5).all() and (bad == 0xA5).all() and status[0] == 0x5A5A


def test_struct_and_abi_version():
    from rustfs_amd import _lib
    assert ctypes.sizeof(_lib.rsg_rblock) == 40
    src = open(os.path.join(ROOT, "include", "rsgpu.h")).read()
    assert int(re.search(r"#define\s+RSG_ABI_VERSION\s+(\d+)", src).group(1)) == 6
    assert "rsg_reconstruct_blocks" in _lib.EXPORTED


def test_python_surface_checks_blocks():
    """Erasure.decode_blocks refuses a wrong shard count, shards of unequal
    length and a wrongly sized digest array before anything reaches the
    library."""
    from rustfs_amd import Erasure, _lib
    from rustfs_amd._lib import RsgError
    e = Erasure(2, 1, 1 << 20)
    s = [np.zeros(8, np.uint8) for _ in range(3)]
    with pytest.raises(RsgError) as err:
        e.decode_blocks([s[:2]])
    assert err.value.code == _lib.RSG_ERR_INVALID_SHARD_COUNT
    with pytest.raises(RsgError) as err:
        e.decode_blocks([[s[0], None, np.zeros(9, np.uint8)]])
    assert err.value.code == _lib.RSG_ERR_INCONSISTENT_LENGTH
    with pytest.raises(TypeError):
        e.decode_blocks([[s[0], None, s[2]]], digests=[np.zeros(95, np.uint8)])
    with pytest.raises(TypeError):
        e.decode_blocks([[s[0], None, s[2]]], digests=[])
