"""Host-side mirror of rustfs's erasure codec surface, running on librsgpu.so.

Mirrors, name for name and error for error:
  * ``Erasure``            crates/ecstore/src/erasure/coding/erasure.rs:617-1095
  * ``ReedSolomonEncoder`` erasure.rs:358-446
  * ``calc_shard_size``    erasure.rs:655
  * ``RustfsCodecDecodeEngine.reconstruct_into``  crates/ecstore/src/erasure/codec/bridge.rs:274-307

Every GF(2^8) byte is computed by the HIP kernels behind include/rsgpu.h; this
module only validates, marshals pointers and maps status codes to exceptions.
The device-batch entry points (``*_batch``) take torch uint8 tensors resident
on the GPU and run asynchronously on the current torch stream.
"""
from __future__ import annotations

import contextlib
import ctypes
import threading
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import InvalidDataError, RsgError, check

MODERN_MAX_TOTAL_SHARDS = 256  # galois_8::Field::ORDER, erasure.rs:72


# ---------------------------------------------------------------------------
# ErasureConstructionError (erasure.rs:87-121)

class ErasureConstructionError(ValueError):
    pass


class ZeroDataShards(ErasureConstructionError):
    def __init__(self):
        super().__init__("data_shards must be greater than zero")


class ZeroBlockSize(ErasureConstructionError):
    def __init__(self):
        super().__init__("block_size must be greater than zero")


class UnsupportedModernShardCount(ErasureConstructionError):
    def __init__(self, data_shards: int, parity_shards: int):
        super().__init__(f"modern codec does not support {data_shards} data shards and {parity_shards} parity shards")


def calc_shard_size(block_size: int, data_shards: int) -> int:
    """erasure.rs:655 — plain ceiling division (MinIO-compatible sizing)."""
    return -(-block_size // data_shards)


def _as_array(buf) -> np.ndarray:
    if isinstance(buf, np.ndarray):
        return buf
    return np.frombuffer(buf, dtype=np.uint8)


def _ptrs(arrs: Sequence[np.ndarray]):
    return (ctypes.c_void_p * len(arrs))(*[a.ctypes.data if a.size else 0 for a in arrs])


def _writable(buf) -> np.ndarray:
    a = _as_array(buf)
    if not a.flags.writeable:
        raise TypeError("shard buffer is read-only; pass bytearray / numpy arrays")
    return a


def _shard_view(buf) -> np.ndarray:
    """A shard as the flat uint8 byte run the C ABI reads and writes through
    one pointer: a strided view (buf[:, i]) or another dtype would make the
    library touch bytes outside the caller's shard, so those are rejected."""
    a = _as_array(buf)
    if a.dtype != np.uint8 or not a.flags.c_contiguous:
        raise TypeError("shard buffers must be C-contiguous uint8 (bytes, bytearray or numpy uint8 arrays)")
    return a


# ---------------------------------------------------------------------------

class ReedSolomonEncoder:
    """ReedSolomonEncoder (erasure.rs:358-446) over the GPU codec."""

    def __init__(self, data_shards: int, parity_shards: int, device: Optional[int] = None):
        st = _lib.load().rsg_check_geometry(data_shards, parity_shards)
        if st != _lib.RSG_OK:
            raise RsgError(st, "Failed to create Reed-Solomon encoder")
        self.data_shards = data_shards
        self.parity_shards = parity_shards
        self._device = device

    @property
    def total(self) -> int:
        return self.data_shards + self.parity_shards

    def _ctx(self):
        return _lib.context(self._device)

    def encode(self, shards: List) -> None:
        """In place: shards[k..k+m) overwritten with parity (erasure.rs:396-408)."""
        if len(shards) == 0 or self.parity_shards == 0:
            return
        if len(shards) != self.total:
            raise RsgError(_lib.RSG_ERR_INVALID_SHARD_COUNT, "Reed-Solomon encode failed")
        arrs = [_shard_view(s) for s in shards]
        n = arrs[0].size
        if any(a.size != n for a in arrs):
            raise RsgError(_lib.RSG_ERR_INCONSISTENT_LENGTH, "Reed-Solomon encode failed")
        for a in arrs[self.data_shards:]:
            _writable(a)
        check(_lib.load().rsg_encode(self._ctx().handle, self.data_shards, self.parity_shards, n, _ptrs(arrs)),
              "Reed-Solomon encode failed")

    def encode_hashed(self, shards: List, algo: int = _lib.RSG_HASH_HIGHWAY256S) -> np.ndarray:
        """encode plus the BitrotWriter digest of every shard (rsg_encode_hashed,
        bitrot.rs:496-502): parity in place, returns the (k+m, 32) digests."""
        if len(shards) != self.total:
            raise RsgError(_lib.RSG_ERR_INVALID_SHARD_COUNT, "Reed-Solomon encode failed")
        arrs = [_shard_view(s) for s in shards]
        n = arrs[0].size
        if any(a.size != n for a in arrs):
            raise RsgError(_lib.RSG_ERR_INCONSISTENT_LENGTH, "Reed-Solomon encode failed")
        for a in arrs[self.data_shards:]:
            _writable(a)
        digests = np.zeros((self.total, 32), dtype=np.uint8)
        check(_lib.load().rsg_encode_hashed(self._ctx().handle, self.data_shards, self.parity_shards, n, _ptrs(arrs),
                                            digests.ctypes.data, algo), "Reed-Solomon encode failed")
        return digests

    def _reconstruct(self, shards: List, mode: int) -> None:
        if len(shards) != self.total:
            raise RsgError(_lib.RSG_ERR_INVALID_SHARD_COUNT,
                           f"invalid shard count: got {len(shards)}, expected {self.total}")
        present = [s is not None for s in shards]
        lens = {len(s) for s in shards if s is not None}
        if len(lens) > 1:
            raise RsgError(_lib.RSG_ERR_INCONSISTENT_LENGTH, "Reed-Solomon reconstruct failed")
        n = lens.pop() if lens else 0
        if n == 0:
            # recover_empty_payload_data_shards (erasure.rs:563-594 / bridge.rs:54-84)
            st = _lib.load().rsg_reconstruct(self._ctx().handle, self.data_shards, self.parity_shards, 0,
                                             None, (ctypes.c_uint8 * self.total)(*present), mode)
            check(st, "Reed-Solomon reconstruct failed")
            fill = range(self.data_shards) if mode == _lib.RSG_RECONSTRUCT_DATA else range(self.total)
            for i in fill:
                if shards[i] is None and (i < self.data_shards or mode != _lib.RSG_RECONSTRUCT_DATA):
                    shards[i] = bytearray()
            return
        if self.parity_shards == 0:
            return
        arrs = []
        for i, s in enumerate(shards):
            is_parity = i >= self.data_shards
            if s is None:
                s = bytearray(n)  # Option::None -> freshly allocated Vec (filled by the codec)
                if not is_parity or mode != _lib.RSG_RECONSTRUCT_DATA:
                    shards[i] = s
            elif is_parity and mode == _lib.RSG_RECONSTRUCT_REENCODE_PARITY and not _as_array(s).flags.writeable:
                s = bytearray(s)  # re-encoded parity replaces the present buffer
                shards[i] = s
            arrs.append(_shard_view(s))
        st = _lib.load().rsg_reconstruct(self._ctx().handle, self.data_shards, self.parity_shards, n,
                                         _ptrs(arrs), (ctypes.c_uint8 * self.total)(*present), mode)
        check(st, "Reed-Solomon reconstruct failed")

    def reconstruct_data(self, shards: List) -> None:
        """erasure.rs:411-422: rebuild missing data shards (parity stays None)."""
        self._reconstruct(shards, _lib.RSG_RECONSTRUCT_DATA)

    def reconstruct(self, shards: List) -> None:
        """erasure.rs:425-428: reconstruct_data then re-encode every parity shard."""
        self._reconstruct(shards, _lib.RSG_RECONSTRUCT_REENCODE_PARITY)

    def reconstruct_opt(self, shards: List) -> None:
        """reconstruct_opt (bridge.rs:296): rebuild every missing shard."""
        self._reconstruct(shards, _lib.RSG_RECONSTRUCT_MISSING)

    def verify(self, shards: Sequence) -> bool:
        """erasure.rs:430-441."""
        if all(len(s) == 0 for s in shards):
            return True
        if self.parity_shards == 0:
            return True
        if len(shards) != self.total:
            raise RsgError(_lib.RSG_ERR_INVALID_SHARD_COUNT, "Reed-Solomon verify failed")
        arrs = [np.ascontiguousarray(_as_array(s)) for s in shards]
        n = arrs[0].size
        if any(a.size != n for a in arrs):
            raise RsgError(_lib.RSG_ERR_INCONSISTENT_LENGTH, "Reed-Solomon verify failed")
        ok = ctypes.c_int(0)
        check(_lib.load().rsg_verify(self._ctx().handle, self.data_shards, self.parity_shards, n, _ptrs(arrs),
                                     ctypes.byref(ok)), "Reed-Solomon verify failed")
        return bool(ok.value)


# ---------------------------------------------------------------------------

class Erasure:
    """Erasure (erasure.rs:617-1095), modern GF(2^8) backend only."""

    def __init__(self, data_shards: int, parity_shards: int, block_size: int, device: Optional[int] = None):
        if data_shards == 0:
            raise ZeroDataShards()
        if block_size == 0:
            raise ZeroBlockSize()
        if parity_shards > 0 and data_shards + parity_shards > MODERN_MAX_TOTAL_SHARDS:
            raise UnsupportedModernShardCount(data_shards, parity_shards)
        self.data_shards = data_shards
        self.parity_shards = parity_shards
        self.block_size = block_size
        self.encoder = ReedSolomonEncoder(data_shards, parity_shards, device) if parity_shards > 0 else None
        self._device = device
        self._mixed_arenas = None  # page-locked (data, parity, digests) of the mixed-length calls, reused
        self._mixed_lock = threading.Lock()

    try_new = classmethod(lambda cls, k, m, b, device=None: cls(k, m, b, device))

    # -- geometry (erasure.rs:1021-1095) --
    def total_shard_count(self) -> int:
        return self.data_shards + self.parity_shards

    def shard_size(self) -> int:
        return calc_shard_size(self.block_size, self.data_shards)

    def has_valid_dimensions(self) -> bool:
        return self.block_size > 0 and self.data_shards > 0

    def shard_file_size(self, total_length: int) -> int:
        if total_length == 0:
            return 0
        if total_length < 0:
            return total_length
        num_shards = total_length // self.block_size
        last = total_length % self.block_size
        return num_shards * self.shard_size() + calc_shard_size(last, self.data_shards)

    def shard_file_offset(self, start_offset: int, length: int, total_length: int) -> int:
        shard_size = self.shard_size()
        shard_file_size = self.shard_file_size(total_length)
        end_shard = (start_offset + length) // self.block_size
        till = end_shard * shard_size + shard_size
        return min(till, shard_file_size)

    # -- encode (erasure.rs:784-887) --
    def encode_buffer(self, data) -> np.ndarray:
        """Copy + zero-pad to (k+m)*S and encode; returns the (k+m, S) stripe."""
        data = _as_array(data)
        per_shard = calc_shard_size(data.size, self.data_shards)
        if per_shard == 0:
            return np.zeros((self.total_shard_count(), 0), dtype=np.uint8)
        buf = np.zeros((self.total_shard_count(), per_shard), dtype=np.uint8)
        buf.reshape(-1)[: data.size] = data
        if self.encoder is not None:
            self.encoder.encode([buf[i] for i in range(self.total_shard_count())])
        return buf

    def encode_data(self, data) -> List[bytes]:
        buf = self.encode_buffer(data)
        return [buf[i].tobytes() for i in range(buf.shape[0])]

    def encode_inline_shards(self, data) -> List[bytes]:
        """encode_inline_shards_with_size_hint (encode.rs:601-628): encode one
        small object and return each shard as its BitrotWriter payload
        ``[HighwayHash256S(shard)][shard]`` (empty list for an empty object).
        Parity and all k+m digests come from one rsg_encode_batch_host call
        (fused encode + hash on the device)."""
        data = _as_array(data)
        if data.size == 0:
            return []
        per_shard = calc_shard_size(data.size, self.data_shards)
        t = self.total_shard_count()
        buf = np.zeros((1, t, per_shard), dtype=np.uint8)
        buf.reshape(-1)[: data.size] = data
        dig = np.zeros((1, t, 32), dtype=np.uint8)
        if self.parity_shards:
            self.encode_batch_host(buf, dig)
        else:
            from .bitrot import HashAlgorithm
            for i in range(t):
                dig[0, i] = np.frombuffer(HashAlgorithm.HighwayHash256S.hash_encode(buf[0, i], self._device), np.uint8)
        return [dig[0, i].tobytes() + buf[0, i].tobytes() for i in range(t)]

    def encode_inline_shards_many(self, datas: Sequence) -> List[List[bytes]]:
        """encode_inline_shards for many objects at once: entry j equals
        ``encode_inline_shards(datas[j])`` (``[]`` for an empty object, which
        submits no stripe).  The objects' zero-padded k*S_j data regions are
        packed into one page-locked data arena, with a parity arena and a
        digest array beside it (reused across calls), and parity and all
        digests of every object come from one rsg_encode_mixed_host call."""
        k, m, t = self.data_shards, self.parity_shards, self.total_shard_count()
        arrs = [_as_array(d).reshape(-1).view(np.uint8) for d in datas]
        live = [j for j, a in enumerate(arrs) if a.size]
        out: List[List[bytes]] = [[] for _ in arrs]
        if not live:
            return out
        S = np.array([calc_shard_size(arrs[j].size, k) for j in live], dtype=np.uint64)
        desc = np.zeros((len(live), 3), dtype=np.uint64)
        desc[:, 2] = S
        desc[1:, 0] = np.cumsum(S[:-1] * np.uint64(k))
        desc[1:, 1] = np.cumsum(S[:-1] * np.uint64(m))
        nd, npar = int(S.sum()) * k, int(S.sum()) * m
        with self.mixed_stage(nd, npar, len(live)) as (data, parity, dig):
            for i, j in enumerate(live):
                a, off, s = arrs[j], int(desc[i, 0]), int(S[i])
                data[off:off + a.size] = a
                data[off + a.size:off + k * s] = 0  # the pad up to k*S (erasure.rs:858-866)
            self.encode_mixed_host(data, parity, desc, dig)
            for i, j in enumerate(live):
                do, po, s = int(desc[i, 0]), int(desc[i, 1]), int(S[i])
                d = dig[i].tobytes()
                out[j] = [d[32 * c:32 * c + 32] + data[do + c * s:do + (c + 1) * s].tobytes() for c in range(k)] + \
                         [d[32 * (k + r):32 * (k + r) + 32] + parity[po + r * s:po + (r + 1) * s].tobytes()
                          for r in range(m)]
        return out

    @contextlib.contextmanager
    def mixed_stage(self, data_bytes: int, parity_bytes: int, n: int):
        """Arenas for a mixed-length host call: (data, parity, digests (n, k+m,
        32)) uint8 arrays of at least the sizes asked for, page-locked and
        reused across calls (PutStage's role); a caller that finds them in use
        by another thread gets pageable arrays of its own.  Contents are
        unspecified on entry."""
        t = self.total_shard_count()
        if not self._mixed_lock.acquire(blocking=False):
            yield (np.empty(data_bytes, np.uint8), np.empty(parity_bytes, np.uint8),
                   np.empty((n, t, 32), np.uint8))
            return
        try:
            have = self._mixed_arenas
            if have is None or have[0].size < data_bytes or have[1].size < parity_bytes or have[2].size < n * t * 32:
                import torch

                def pinned(nbytes, old):  # grow by half again, so a slowly growing batch does not re-pin each call
                    want = max(nbytes, 1)
                    if old is not None and old.size >= want:
                        return old
                    return torch.empty(want + want // 2, dtype=torch.uint8).pin_memory().numpy()
                old = have or (None, None, None)
                have = self._mixed_arenas = (pinned(data_bytes, old[0]), pinned(parity_bytes, old[1]),
                                             pinned(n * t * 32, old[2]))
            yield have[0][:data_bytes], have[1][:parity_bytes], have[2][:n * t * 32].reshape(n, t, 32)
        finally:
            self._mixed_lock.release()

    # -- decode (erasure.rs:897-1019) --
    def decode_data(self, shards: List) -> None:
        if self.encoder is not None:
            self.encoder.reconstruct_data(shards)

    def decode_data_and_parity(self, shards: List) -> None:
        if self.encoder is not None:
            self.encoder.reconstruct(shards)

    def decode_data_with_reconstruction_verification(self, shards: List) -> None:
        k = self.data_shards
        missing_data = any(s is None for s in shards[:k])
        available = sum(s is not None for s in shards)
        source_parity = []
        if missing_data and available > k:
            source_parity = [(i, bytes(s)) for i, s in enumerate(shards) if i >= k and s is not None]
        if not source_parity:
            self.decode_data(shards)
            return
        self.decode_data_and_parity(shards)
        for i, src in source_parity:
            if shards[i] is None:
                raise InvalidDataError(_lib.RSG_ERR_INCONSISTENT_SOURCES,
                                       "missing rebuilt parity shard after read verification")
            if bytes(shards[i]) != src:
                raise InvalidDataError(_lib.RSG_ERR_INCONSISTENT_SOURCES)

    def verify_data_and_parity(self, shards: Sequence) -> bool:
        if len(shards) != self.total_shard_count():
            raise RsgError(_lib.RSG_ERR_INVALID_SHARD_COUNT,
                           f"invalid shard count: got {len(shards)}, expected {self.total_shard_count()}")
        if self.parity_shards == 0:
            return True
        for i, s in enumerate(shards):
            if s is None:
                raise RsgError(_lib.RSG_ERR_INVALID_ARG, f"missing shard {i} for data/parity verification")
        return self.encoder.verify(shards)

    # -- device batches (the GPU dispatch point of encode_batched, encode.rs:795-919) --
    def encode_batch(self, stripes, digests=None, algo: int = _lib.RSG_HASH_HIGHWAY256S, stream=None) -> None:
        """stripes: cuda uint8 tensor (n, k+m, S) in the a3 layout; parity written
        in place.  digests: optional (n, k+m, 32) tensor for the fused HH256S."""
        n, t, S = _check_batch(stripes, self.total_shard_count())
        d = digests.data_ptr() if digests is not None else None
        check(_lib.load().rsg_encode_batch_dev(
            _lib.context(_device_of(stripes)).handle, self.data_shards, self.parity_shards, S, n,
            stripes.data_ptr(), S, t * S, d, algo if d else _lib.RSG_HASH_NONE, _stream_of(stripes, stream)),
            "Reed-Solomon encode failed")

    def encode_batch_host(self, stripes: np.ndarray, digests: Optional[np.ndarray] = None,
                          algo: int = _lib.RSG_HASH_HIGHWAY256S) -> None:
        """Host-memory batch (n, k+m, S) uint8, parity written in place; pipelined
        H2D -> encode(+digests) -> D2H inside librsgpu (rsg_encode_batch_host)."""
        n, t, S, d = self._host_batch_args(stripes, digests)
        check(_lib.load().rsg_encode_batch_host(
            _lib.context(self._device).handle, self.data_shards, self.parity_shards, S, n, stripes.ctypes.data,
            S, t * S, d, algo if d else _lib.RSG_HASH_NONE), "Reed-Solomon encode failed")

    def encode_batch_host_submit(self, stripes: np.ndarray, digests: Optional[np.ndarray] = None,
                                 algo: int = _lib.RSG_HASH_HIGHWAY256S) -> "HostBatchTicket":
        """Asynchronous encode_batch_host (rsg_encode_batch_host_submit): returns
        at once with a ticket; the arrays must stay alive and untouched until
        the ticket is done (poll() / wait()).  Jobs run in submission order and
        overlap each other's copies and kernels (encode_batched's bounded
        in-flight queue, encode.rs:64-72, 795-919)."""
        n, t, S, d = self._host_batch_args(stripes, digests)
        tk = ctypes.c_uint64(0)
        ctx = _lib.context(self._device)
        check(_lib.load().rsg_encode_batch_host_submit(
            ctx.handle, self.data_shards, self.parity_shards, S, n, stripes.ctypes.data, S, t * S, d,
            algo if d else _lib.RSG_HASH_NONE, ctypes.byref(tk)), "Reed-Solomon encode failed")
        return HostBatchTicket(ctx, tk.value, (stripes, digests))

    # -- gathered blocks: n unrelated blocks of k+m shard buffers each (rsg_encode_blocks) --
    def encode_blocks(self, blocks: Sequence[Sequence], digests: Optional[Sequence] = None,
                      algo: int = _lib.RSG_HASH_HIGHWAY256S) -> None:
        """Encode n unrelated blocks in one call (rsg_encode_blocks): blocks[i]
        is a list of k+m uint8 buffers of one length (its own), k data then m
        parity, anywhere in host memory and at any alignment; the parity
        buffers are overwritten.  digests, if given, holds per block a
        writable (k+m, 32) uint8 array or None (parity only for that block).
        One launch pair per 32 MiB of staged shards for k <= 16, m <= 4."""
        t = self.total_shard_count()
        if digests is not None and len(digests) != len(blocks):
            raise TypeError("digests must hold one entry (an array or None) per block")
        n = len(blocks)
        descs = (_lib.rsg_block * max(n, 1))()
        keep = []
        for i, shards in enumerate(blocks):
            if len(shards) != t:
                raise RsgError(_lib.RSG_ERR_INVALID_SHARD_COUNT, "Reed-Solomon encode failed")
            arrs = [_shard_view(s) for s in shards]
            if any(a.size != arrs[0].size for a in arrs):
                raise RsgError(_lib.RSG_ERR_INCONSISTENT_LENGTH, "Reed-Solomon encode failed")
            for a in arrs[self.data_shards:]:
                _writable(a)
            ptrs = _ptrs(arrs)
            dg = digests[i] if digests is not None else None
            if dg is not None:
                dg = _writable(_shard_view(dg))
                if dg.size != t * 32:
                    raise TypeError("a block's digests must hold (k+m, 32) bytes")
            keep.append((arrs, ptrs, dg))
            descs[i].shards = ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p))
            descs[i].shard_len = arrs[0].size
            descs[i].digests = dg.ctypes.data if dg is not None else None
        check(_lib.load().rsg_encode_blocks(_lib.context(self._device).handle, self.data_shards, self.parity_shards, n,
                                            ctypes.byref(descs), algo if digests is not None else _lib.RSG_HASH_NONE),
              "Reed-Solomon encode failed")

    def decode_blocks(self, blocks: Sequence[List], digests: Optional[Sequence] = None,
                      mode: int = _lib.RSG_RECONSTRUCT_DATA, algo: int = _lib.RSG_HASH_HIGHWAY256S) -> list:
        """Rebuild n unrelated degraded blocks in one call
        (rsg_reconstruct_blocks): blocks[i] is a list of k+m uint8 buffers of
        one length (its own) or None for a shard that was not read, as
        ReedSolomonEncoder's reconstruct calls take them; the shards the mode
        fills are allocated in the list (parity stays None under
        RSG_RECONSTRUCT_DATA).  digests, if given, holds per block the
        expected (k+m, 32) uint8 digests or None: a present shard that does
        not hash to its entry is treated as not read and rebuilt in place if
        the mode rebuilds it.  Returns per block (status, bad): RSG_OK or
        RSG_ERR_TOO_FEW_SHARDS (nothing of that block written), and a (k+m,)
        uint8 array with 1 at every shard found rotten.  Raises only for
        errors of the whole call."""
        t, k = self.total_shard_count(), self.data_shards
        if digests is not None and len(digests) != len(blocks):
            raise TypeError("digests must hold one entry (an array or None) per block")
        n = len(blocks)
        descs = (_lib.rsg_rblock * max(n, 1))()
        status = (ctypes.c_int * max(n, 1))()
        bad = np.zeros((n, t), dtype=np.uint8)
        keep = []
        for i, shards in enumerate(blocks):
            if len(shards) != t:
                raise RsgError(_lib.RSG_ERR_INVALID_SHARD_COUNT, f"invalid shard count: got {len(shards)}, expected {t}")
            lens = {_shard_view(s).size for s in shards if s is not None}
            if len(lens) > 1:
                raise RsgError(_lib.RSG_ERR_INCONSISTENT_LENGTH, "Reed-Solomon reconstruct failed")
            size = lens.pop() if lens else 0
            dg = digests[i] if digests is not None else None
            if dg is not None:
                dg = np.ascontiguousarray(_shard_view(dg))
                if dg.size != t * 32:
                    raise TypeError("a block's digests must hold (k+m, 32) bytes")
            present = np.array([s is not None for s in shards], dtype=np.uint8)
            arrs = []
            for j, s in enumerate(shards):
                if s is None:
                    s = bytearray(size)  # Option::None -> freshly allocated Vec (filled by the codec)
                    if j < k or mode != _lib.RSG_RECONSTRUCT_DATA:
                        shards[j] = s
                elif not _as_array(s).flags.writeable and (
                        dg is not None or (j >= k and mode == _lib.RSG_RECONSTRUCT_REENCODE_PARITY)):
                    # a rebuilt rotten shard, or re-encoded parity, replaces the present buffer
                    s = bytearray(s)
                    shards[j] = s
                arrs.append(_shard_view(s))
            ptrs = _ptrs(arrs)
            keep.append((arrs, ptrs, dg, present))
            descs[i].shards = ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p))
            descs[i].shard_len = size
            descs[i].present = present.ctypes.data
            descs[i].digests = dg.ctypes.data if dg is not None else None
            descs[i].bad = bad[i].ctypes.data
        check(_lib.load().rsg_reconstruct_blocks(_lib.context(self._device).handle, k, self.parity_shards, n,
                                                 ctypes.byref(descs), mode, algo if digests is not None else _lib.RSG_HASH_NONE,
                                                 status), "Reed-Solomon reconstruct failed")
        return [(st, bad[i]) for i, st in enumerate(_lib.status_list(status, n))]

    # -- mixed-length batches: every stripe its own shard length (rsg_encode_mixed_*) --
    def _mixed_desc(self, desc, data_len: int, parity_len: int, digests_len: Optional[int]) -> np.ndarray:
        """The (n, 3) uint64 descriptor array [data_off, parity_off, shard_len]
        (rsg_stripe_desc), with every range checked against the arenas."""
        d = np.ascontiguousarray(np.asarray(desc, dtype=np.uint64).reshape(-1, _lib.STRIPE_DESC_FIELDS))
        k, m = self.data_shards, self.parity_shards
        o = d[d[:, 2] != 0].astype(object)  # exact integers: an offset near 2^64 must not wrap
        if o.shape[0] and ((o[:, 0] + k * o[:, 2]).max() > data_len or
                           (m and (o[:, 1] + m * o[:, 2]).max() > parity_len)):
            raise RsgError(_lib.RSG_ERR_INVALID_ARG, "mixed-length stripe outside its arena")
        if digests_len is not None and digests_len < d.shape[0] * (k + m) * 32:
            raise TypeError("digests must hold (n, k+m, 32) bytes")
        return d

    def encode_mixed(self, data, parity, desc, digests=None, algo: int = _lib.RSG_HASH_HIGHWAY256S,
                     stream=None) -> None:
        """Mixed-length batch on the device (rsg_encode_mixed_dev): `data` and
        `parity` are contiguous cuda uint8 arenas (the same tensor for an
        aliased layout such as a3), `desc` an (n, 3) array of [data_off,
        parity_off, shard_len]; stripe j's k data shards lie back to back at
        data_off, its m parity shards are written back to back at parity_off,
        its k+m digests to digests[j] (cuda (n, k+m, 32), optional).
        Asynchronous on the current torch stream; one launch for k <= 16,
        m = 1..4."""
        for a in (data, parity) + ((digests,) if digests is not None else ()):
            if a.dtype.__str__() != "torch.uint8" or not a.is_cuda or not a.is_contiguous():
                raise TypeError("arenas and digests must be contiguous cuda uint8 tensors")
        d = self._mixed_desc(desc, data.numel(), parity.numel(), digests.numel() if digests is not None else None)
        check(_lib.load().rsg_encode_mixed_dev(
            _lib.context(_device_of(data)).handle, self.data_shards, self.parity_shards, d.shape[0], d.ctypes.data,
            data.data_ptr(), parity.data_ptr(), digests.data_ptr() if digests is not None else None,
            algo if digests is not None else _lib.RSG_HASH_NONE, _stream_of(data, stream)),
            "Reed-Solomon encode failed")

    def _mixed_host_args(self, data, parity, desc, digests):
        for a in (data, parity) + ((digests,) if digests is not None else ()):
            if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or not a.flags.c_contiguous:
                raise TypeError("arenas and digests must be C-contiguous uint8 arrays")
        _writable(parity)
        d = self._mixed_desc(desc, data.size, parity.size, digests.size if digests is not None else None)
        return d, (digests.ctypes.data if digests is not None else None)

    def encode_mixed_host(self, data: np.ndarray, parity: np.ndarray, desc, digests: Optional[np.ndarray] = None,
                          algo: int = _lib.RSG_HASH_HIGHWAY256S) -> None:
        """encode_mixed on host arenas (rsg_encode_mixed_host): sub-batches of
        consecutive stripes pipelined H2D -> one launch -> D2H inside
        librsgpu.  The parity arena's bytes between the parity ranges of a
        sub-batch come back unspecified: pack the arenas densely."""
        d, dg = self._mixed_host_args(data, parity, desc, digests)
        check(_lib.load().rsg_encode_mixed_host(
            _lib.context(self._device).handle, self.data_shards, self.parity_shards, d.shape[0], d.ctypes.data,
            data.ctypes.data, parity.ctypes.data, dg, algo if dg else _lib.RSG_HASH_NONE),
            "Reed-Solomon encode failed")

    def encode_mixed_host_submit(self, data: np.ndarray, parity: np.ndarray, desc,
                                 digests: Optional[np.ndarray] = None,
                                 algo: int = _lib.RSG_HASH_HIGHWAY256S) -> "HostBatchTicket":
        """Asynchronous encode_mixed_host (rsg_encode_mixed_host_submit): the
        arrays must stay alive and untouched until the ticket is done."""
        d, dg = self._mixed_host_args(data, parity, desc, digests)
        tk = ctypes.c_uint64(0)
        ctx = _lib.context(self._device)
        check(_lib.load().rsg_encode_mixed_host_submit(
            ctx.handle, self.data_shards, self.parity_shards, d.shape[0], d.ctypes.data, data.ctypes.data,
            parity.ctypes.data, dg, algo if dg else _lib.RSG_HASH_NONE, ctypes.byref(tk)),
            "Reed-Solomon encode failed")
        return HostBatchTicket(ctx, tk.value, (data, parity, d, digests))

    # -- mixed-length GET: every stripe its own shard length and present set (rsg_decode_mixed_*) --
    def _record_desc(self, desc, file_lens: Sequence[Optional[int]], out_len: int) -> np.ndarray:
        """The rsg_record_desc array of `desc` (a structured array of
        _lib.RECORD_DESC_FIELDS, or (n, 4) integers [rec_off, out_off,
        shard_len, present]), with every stripe checked against its arenas
        before anything reaches the library."""
        dt = np.dtype(list(_lib.RECORD_DESC_FIELDS))
        if isinstance(desc, np.ndarray) and desc.dtype == dt:
            d = np.ascontiguousarray(desc.reshape(-1))
        else:
            rows = [tuple(int(v) for v in r) for r in np.asarray(desc, dtype=object).reshape(-1, 4)]
            if any(not (0 <= r[0] < 1 << 64 and 0 <= r[1] < 1 << 64 and 0 <= r[2] < 1 << 32 and 0 <= r[3] < 1 << 32)
                   for r in rows):
                raise RsgError(_lib.RSG_ERR_INVALID_ARG, "mixed-length record descriptor out of range")
            d = np.array(rows, dtype=dt) if rows else np.zeros(0, dtype=dt)
        k, t = self.data_shards, self.total_shard_count()
        if len(file_lens) != t:
            raise RsgError(_lib.RSG_ERR_INVALID_SHARD_COUNT, f"invalid shard count: got {len(file_lens)}")
        if d.size:
            rec_end = d["rec_off"].astype(object) + 32 + d["shard_len"].astype(object)  # exact integers: no wrap
            out_end = d["out_off"].astype(object) + k * d["shard_len"].astype(object)
            live = d["shard_len"] != 0
            if live.any() and out_end[live].max() > out_len:
                raise RsgError(_lib.RSG_ERR_INVALID_ARG, "mixed-length stripe outside its out arena")
            for i, n in enumerate(file_lens):
                if n is None:
                    continue
                use = (d["present"] >> np.uint32(i) & np.uint32(1)).astype(bool) if i < 32 else np.zeros(d.size, bool)
                if use.any() and rec_end[use].max() > n:
                    raise RsgError(_lib.RSG_ERR_INVALID_ARG, f"mixed-length record outside arena {i}")
        return d

    def decode_mixed(self, files: Sequence, desc, out, verify_surplus: bool = True,
                     algo: int = _lib.RSG_HASH_HIGHWAY256S, stream=None):
        """Mixed-length batch GET on the device (rsg_decode_mixed_dev):
        `files[i]` is shard i's record arena (a contiguous cuda uint8 tensor,
        or None: absent for every stripe), `desc` lists per stripe [rec_off,
        out_off, shard_len, present]; every record a stripe's decode uses is
        verified against its 32-byte header first, and only the data shards no
        verified record serves are rebuilt, at out + out_off + c*shard_len.
        Returns (status, served): per stripe an rsg_status and the bit mask of
        data shards served from their records.  Synchronous."""
        t = self.total_shard_count()
        for a in [f for f in files if f is not None] + [out]:
            if a.dtype.__str__() != "torch.uint8" or not a.is_cuda or not a.is_contiguous():
                raise TypeError("arenas and out must be contiguous cuda uint8 tensors")
        d = self._record_desc(desc, [f.numel() if f is not None else None for f in files], out.numel())
        n = d.size
        status, served = (ctypes.c_int * max(n, 1))(), (ctypes.c_uint32 * max(n, 1))()
        fp = (ctypes.c_void_p * t)(*[f.data_ptr() if f is not None else None for f in files])
        check(_lib.load().rsg_decode_mixed_dev(
            _lib.context(_device_of(out)).handle, self.data_shards, self.parity_shards, n, d.ctypes.data, fp, algo,
            1 if verify_surplus else 0, out.data_ptr(), served, status, _stream_of(out, stream)),
            "mixed-length decode failed")
        return _lib.status_list(status, n), list(served[:n])

    def decode_mixed_host(self, files: Sequence, desc, out: np.ndarray, verify_surplus: bool = True,
                          algo: int = _lib.RSG_HASH_HIGHWAY256S):
        """decode_mixed on host arenas (rsg_decode_mixed_host): numpy uint8
        arrays, page-locked or pageable; sub-batches of consecutive stripes go
        through the host-batch staging slots, and only the windows of rebuilt
        shards of good stripes come back into `out`."""
        t = self.total_shard_count()
        for a in [f for f in files if f is not None] + [out]:
            if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or not a.flags.c_contiguous:
                raise TypeError("arenas and out must be C-contiguous uint8 arrays")
        _writable(out)
        d = self._record_desc(desc, [f.size if f is not None else None for f in files], out.size)
        n = d.size
        status, served = (ctypes.c_int * max(n, 1))(), (ctypes.c_uint32 * max(n, 1))()
        fp = (ctypes.c_void_p * t)(*[f.ctypes.data if f is not None else None for f in files])
        check(_lib.load().rsg_decode_mixed_host(
            _lib.context(self._device).handle, self.data_shards, self.parity_shards, n, d.ctypes.data, fp, algo,
            1 if verify_surplus else 0, out.ctypes.data, served, status), "mixed-length decode failed")
        return _lib.status_list(status, n), list(served[:n])

    def _heal_desc(self, desc, file_lens: Sequence[Optional[int]], target_lens: Sequence[Optional[int]]) -> np.ndarray:
        """The rsg_record_desc array of a mixed-length heal: _record_desc's
        forms, with out_off the offset of the stripe's record in every target
        arena; every stripe is checked against the source arenas it may read
        (a target's source arena is never read) and against every target arena
        before anything reaches the library."""
        t = self.total_shard_count()
        if len(target_lens) != t:
            raise RsgError(_lib.RSG_ERR_INVALID_SHARD_COUNT, f"invalid shard count: got {len(target_lens)} targets")
        if len(file_lens) == t:
            file_lens = [None if target_lens[i] is not None else n for i, n in enumerate(file_lens)]
        d = self._record_desc(desc, file_lens, 1 << 128)  # the out check is the targets' own, below
        if d.size:
            out_end = (d["out_off"].astype(object) + 32 + d["shard_len"].astype(object)).max()
            for i, n in enumerate(target_lens):
                if n is not None and out_end > n:
                    raise RsgError(_lib.RSG_ERR_INVALID_ARG, f"mixed-length record outside target arena {i}")
        return d

    def heal_mixed(self, files: Sequence, targets: Sequence, desc, algo: int = _lib.RSG_HASH_HIGHWAY256S,
                   stream=None) -> List[int]:
        """Mixed-length batch heal on the device (rsg_heal_mixed_dev):
        `files[i]` is shard i's record arena (a contiguous cuda uint8 tensor,
        or None: absent for every stripe), `targets[i]` is not None where
        shard i is a heal target (never read, whatever files[i] and `present`
        say); `desc` lists per stripe [rec_off, out_off, shard_len, present].
        Every source record used is verified against its 32-byte header first;
        target i receives the stripe's record [HH256S][shard_len] at
        targets[i] + out_off.  Returns the per-stripe rsg_status list; a failed
        stripe's target records carry an all-zero header.  Synchronous."""
        t = self.total_shard_count()
        live = [a for a in list(files) + list(targets) if a is not None]
        for a in live:
            if a.dtype.__str__() != "torch.uint8" or not a.is_cuda or not a.is_contiguous():
                raise TypeError("arenas and targets must be contiguous cuda uint8 tensors")
        d = self._heal_desc(desc, [f.numel() if f is not None else None for f in files],
                            [g.numel() if g is not None else None for g in targets])
        if not live:
            raise RsgError(_lib.RSG_ERR_INVALID_ARG, "mixed-length heal without arenas")
        n = d.size
        status = (ctypes.c_int * max(n, 1))()
        fp = (ctypes.c_void_p * t)(*[f.data_ptr() if f is not None else None for f in files])
        tp = (ctypes.c_void_p * t)(*[g.data_ptr() if g is not None else None for g in targets])
        check(_lib.load().rsg_heal_mixed_dev(
            _lib.context(_device_of(live[0])).handle, self.data_shards, self.parity_shards, n, d.ctypes.data, fp, tp,
            algo, status, _stream_of(live[0], stream)), "mixed-length heal failed")
        return _lib.status_list(status, n)

    def heal_mixed_host(self, files: Sequence, targets: Sequence, desc,
                        algo: int = _lib.RSG_HASH_HIGHWAY256S) -> List[int]:
        """heal_mixed on host arenas (rsg_heal_mixed_host): numpy uint8
        arrays, page-locked or pageable; sub-batches of consecutive stripes go
        through the host-batch staging slots, and the span of target records
        of a sub-batch comes back whole into every target (bytes between the
        records are overwritten: pack the target arenas densely)."""
        t = self.total_shard_count()
        for a in [a for a in list(files) + list(targets) if a is not None]:
            if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or not a.flags.c_contiguous:
                raise TypeError("arenas and targets must be C-contiguous uint8 arrays")
        for g in targets:
            if g is not None:
                _writable(g)
        d = self._heal_desc(desc, [f.size if f is not None else None for f in files],
                            [g.size if g is not None else None for g in targets])
        n = d.size
        status = (ctypes.c_int * max(n, 1))()
        fp = (ctypes.c_void_p * t)(*[f.ctypes.data if f is not None else None for f in files])
        tp = (ctypes.c_void_p * t)(*[g.ctypes.data if g is not None else None for g in targets])
        check(_lib.load().rsg_heal_mixed_host(
            _lib.context(self._device).handle, self.data_shards, self.parity_shards, n, d.ctypes.data, fp, tp, algo,
            status), "mixed-length heal failed")
        return _lib.status_list(status, n)

    def decode_inline_shards_many(self, objects: Sequence, sizes: Sequence[int],
                                  algo: int = _lib.RSG_HASH_HIGHWAY256S) -> list:
        """The inverse of encode_inline_shards_many: objects[j] is a list of
        k+m ``[hash][shard]`` byte strings (None, or a string of the wrong
        length: the shard is not there) of an object of sizes[j] bytes.  Entry
        j of the result is the object's bytes, or the RsgError instance (not
        raised) that verify-before-use followed by a per-object
        decode_data_with_reconstruction_verification would have raised, so one
        bad object does not lose the rest.  A size of 0 gives b"" and submits
        no stripe.  Every object is one stripe of one rsg_decode_mixed_host
        call."""
        k, t = self.data_shards, self.total_shard_count()
        out: list = [b""] * len(objects)
        live = [j for j, sz in enumerate(sizes) if sz]
        if not live:
            return out
        S = [calc_shard_size(int(sizes[j]), k) for j in live]
        dt = np.dtype(list(_lib.RECORD_DESC_FIELDS))
        desc = np.zeros(len(live), dtype=dt)
        desc["shard_len"] = S
        recs = np.array([32 + s for s in S], dtype=np.uint64)
        desc["rec_off"][1:] = np.cumsum(recs[:-1])
        desc["out_off"][1:] = np.cumsum(np.array(S[:-1], dtype=np.uint64) * np.uint64(k))
        arenas = [np.zeros(int(recs.sum()), dtype=np.uint8) for _ in range(t)]
        for i, j in enumerate(live):
            shards = objects[j]
            if len(shards) != t:
                raise RsgError(_lib.RSG_ERR_INVALID_SHARD_COUNT, f"object {j}: invalid shard count: got {len(shards)}")
            off, want, present = int(desc["rec_off"][i]), 32 + S[i], 0
            for c, r in enumerate(shards):
                if r is not None and len(r) == want:
                    arenas[c][off:off + want] = np.frombuffer(r, dtype=np.uint8)
                    present |= 1 << c
            desc["present"][i] = present
        rebuilt = np.zeros(int(sum(S)) * k, dtype=np.uint8)
        status, served = self.decode_mixed_host(arenas, desc, rebuilt, True, algo)
        for i, j in enumerate(live):
            if status[i] == _lib.RSG_ERR_TOO_FEW_SHARDS:
                out[j] = RsgError(status[i], "read quorum lost")
            elif status[i] == _lib.RSG_ERR_INCONSISTENT_SOURCES:
                out[j] = InvalidDataError(status[i])
            elif status[i] != _lib.RSG_OK:
                out[j] = RsgError(status[i], "mixed-length decode failed")
            else:
                ro, oo, s = int(desc["rec_off"][i]) + 32, int(desc["out_off"][i]), S[i]
                out[j] = b"".join((arenas[c][ro:ro + s] if served[i] >> c & 1 else rebuilt[oo + c * s:oo + (c + 1) * s])
                                  .tobytes() for c in range(k))[:int(sizes[j])]
        return out

    def _host_batch_args(self, stripes, digests):
        if stripes.dtype != np.uint8 or stripes.ndim != 3 or not stripes.flags.c_contiguous:
            raise TypeError("stripes must be a C-contiguous uint8 array (n, k+m, S)")
        n, t, S = stripes.shape
        if t != self.total_shard_count():
            raise RsgError(_lib.RSG_ERR_INVALID_SHARD_COUNT, f"invalid shard count: got {t}")
        d = None
        if digests is not None:
            if digests.shape != (n, t, 32) or digests.dtype != np.uint8 or not digests.flags.c_contiguous:
                raise TypeError("digests must be a C-contiguous uint8 array (n, k+m, 32)")
            d = digests.ctypes.data
        return n, t, S, d

    def _record_files(self, files: Sequence, shard_len: int, n: int):
        """Validate the GET's record files; returns (device, ctypes pointer array)."""
        import torch
        t = self.total_shard_count()
        if len(files) != t:
            raise RsgError(_lib.RSG_ERR_INVALID_SHARD_COUNT, f"invalid shard count: got {len(files)}")
        rec = 32 + shard_len
        dev = None
        for f in files:
            if f is not None:
                if f.dtype != torch.uint8 or not f.is_cuda or not f.is_contiguous() or f.numel() < n * rec:
                    raise TypeError("each file must be a contiguous cuda uint8 tensor of n records")
                dev = f.device
        if dev is None:
            raise RsgError(_lib.RSG_ERR_TOO_FEW_SHARDS, "no shard available")
        return dev, (ctypes.c_void_p * t)(*[f.data_ptr() if f is not None else None for f in files])

    def _slots(self, targets, shard_len: int, n: int, dev, target_stride: Optional[int]):
        """The in-place GET's k data-shard slots: None -> a new (n, k*S) block
        tensor (slot i = columns [i*S, (i+1)*S)); a 2-D (n, k*S) tensor, the
        same layout; or k tensors with `target_stride` bytes between stripes
        (default S).  Returns (keep, ctypes pointer array, stride)."""
        import torch
        k = self.data_shards
        if targets is None:
            targets = torch.empty((n, k * shard_len), dtype=torch.uint8, device=dev)
        if isinstance(targets, torch.Tensor):
            if targets.dtype != torch.uint8 or not targets.is_cuda or not targets.is_contiguous() \
                    or targets.numel() < n * k * shard_len:
                raise TypeError("targets must be a contiguous cuda uint8 tensor (n, k*shard_len)")
            base = targets.data_ptr()
            return targets, (ctypes.c_void_p * k)(*[base + i * shard_len for i in range(k)]), k * shard_len
        if len(targets) != k:
            raise RsgError(_lib.RSG_ERR_INVALID_SHARD_COUNT, f"invalid slot count: got {len(targets)}, expected {k}")
        stride = shard_len if target_stride is None else target_stride
        for tg in targets:
            if tg is None or tg.dtype != torch.uint8 or not tg.is_cuda or not tg.is_contiguous() \
                    or (n and tg.numel() < (n - 1) * stride + shard_len):
                raise TypeError("each slot must be a contiguous cuda uint8 tensor of n strided shards")
        return targets, (ctypes.c_void_p * k)(*[tg.data_ptr() for tg in targets]), stride

    @staticmethod
    def _stream_handle(stream, dev):
        import torch
        if stream is None:
            return torch.cuda.current_stream(dev).cuda_stream
        return stream if isinstance(stream, int) else stream.cuda_stream

    def decode_records_batch(self, files: Sequence, shard_len: int, n: int, verify_surplus: bool = True,
                             algo: int = _lib.RSG_HASH_HIGHWAY256S, out=None, stream=None):
        """GET engine, gather form (rsg_decode_records_dev, deprecated since ABI
        6: decode_records_into_batch is the reference's form): `files[i]` is a
        cuda uint8 tensor holding shard i's n BitrotWriter records ([32-byte
        digest][shard_len]) or None.  Returns (data (n, k*shard_len) tensor,
        per-stripe status list)."""
        import torch
        dev, ptrs = self._record_files(files, shard_len, n)
        if out is None:
            out = torch.empty((n, self.data_shards * shard_len), dtype=torch.uint8, device=dev)
        status = (ctypes.c_int * max(n, 1))()
        check(_lib.load().rsg_decode_records_dev(
            _lib.context(dev.index or 0).handle, self.data_shards, self.parity_shards, shard_len, n, ptrs, algo,
            1 if verify_surplus else 0, out.data_ptr(), status, self._stream_handle(stream, dev)),
            "RustFS codec reconstruct failed")
        return out, _lib.status_list(status, n)

    def decode_records_into_batch(self, files: Sequence, shard_len: int, n: int, targets=None,
                                  target_stride: Optional[int] = None, verify_surplus: bool = True,
                                  algo: int = _lib.RSG_HASH_HIGHWAY256S, stream=None):
        """GET engine, in-place form (rsg_decode_records_into_dev): the
        reference's reconstruct_into contract (bridge.rs:274-307) — a data
        shard whose record verifies is served from that record and never
        copied; only the shards no verified record serves (file absent or
        record rotten) are rebuilt, into their slot (`targets`, see _slots).
        Returns (slots, src, status): src is a (k, n) bool array, True where
        data shard i of stripe s is the body of files[i]'s record s, False
        where it was written to slot i."""
        dev, ptrs = self._record_files(files, shard_len, n)
        slots, tptr, stride = self._slots(targets, shard_len, n, dev, target_stride)
        k = self.data_shards
        src = np.ones((k, max(n, 1)), dtype=np.uint8)
        status = (ctypes.c_int * max(n, 1))()
        check(_lib.load().rsg_decode_records_into_dev(
            _lib.context(dev.index or 0).handle, k, self.parity_shards, shard_len, n, ptrs, algo,
            1 if verify_surplus else 0, tptr, stride, src.ctypes.data, status, self._stream_handle(stream, dev)),
            "RustFS codec reconstruct failed")
        return slots, src[:, :n].astype(bool), _lib.status_list(status, n)

    def decode_records_submit(self, files: Sequence, shard_len: int, n: int, out=None, targets=None,
                              target_stride: Optional[int] = None, inplace: bool = False,
                              verify_surplus: bool = True, algo: int = _lib.RSG_HASH_HIGHWAY256S,
                              stream=None) -> "RecordTicket":
        """Asynchronous GET (rsg_decode_records_submit): returns at once; the
        ticket's wait() gives what the synchronous form returns — (data,
        status) for the gather form, (slots, src, status) with inplace=True."""
        import torch
        dev, ptrs = self._record_files(files, shard_len, n)
        k = self.data_shards
        status = (ctypes.c_int * max(n, 1))()
        src = np.ones((k, max(n, 1)), dtype=np.uint8) if inplace else None
        if inplace:
            slots, tptr, stride = self._slots(targets, shard_len, n, dev, target_stride)
            d_out, keep = None, slots
        else:
            if out is None:
                out = torch.empty((n, k * shard_len), dtype=torch.uint8, device=dev)
            d_out, tptr, stride, keep = out.data_ptr(), None, 0, out
        tk = ctypes.c_uint64(0)
        ctx = _lib.context(dev.index or 0)
        check(_lib.load().rsg_decode_records_submit(
            ctx.handle, k, self.parity_shards, shard_len, n, ptrs, algo, 1 if verify_surplus else 0, d_out, tptr,
            stride, src.ctypes.data if inplace else None, status, self._stream_handle(stream, dev),
            ctypes.byref(tk)), "RustFS codec reconstruct failed")

        def result():
            st = _lib.status_list(status, n)
            return (keep, src[:, :n].astype(bool), st) if inplace else (keep, st)
        return RecordTicket(ctx, tk.value, (files, keep, ptrs, tptr, status, src), result,
                            "RustFS codec reconstruct failed")

    def heal_records_submit(self, files: Sequence, targets: Sequence, shard_len: int, n: int,
                            algo: int = _lib.RSG_HASH_HIGHWAY256S, stream=None) -> "RecordTicket":
        """Asynchronous heal (rsg_heal_records_submit); wait() returns the
        per-stripe status list of heal_records_batch."""
        dev, src, dst = self._heal_args(files, targets, shard_len, n)
        status = (ctypes.c_int * max(n, 1))()
        tk = ctypes.c_uint64(0)
        ctx = _lib.context(dev.index or 0)
        check(_lib.load().rsg_heal_records_submit(
            ctx.handle, self.data_shards, self.parity_shards, shard_len, n, src, dst, algo, status,
            self._stream_handle(stream, dev), ctypes.byref(tk)), "erasure heal")
        return RecordTicket(ctx, tk.value, (files, targets, src, dst, status),
                            lambda: _lib.status_list(status, n), "erasure heal")

    def _heal_args(self, files, targets, shard_len, n):
        import torch
        t = self.total_shard_count()
        if len(files) != t or len(targets) != t:
            raise RsgError(_lib.RSG_ERR_INVALID_SHARD_COUNT,
                           f"invalid shard count: got {len(files)}/{len(targets)}, expected {t}")
        rec = 32 + shard_len
        dev = None
        for f in list(files) + list(targets):
            if f is not None:
                if f.dtype != torch.uint8 or not f.is_cuda or not f.is_contiguous() or f.numel() < n * rec:
                    raise TypeError("files/targets must be contiguous cuda uint8 tensors of n records")
                dev = f.device
        if dev is None:
            raise RsgError(_lib.RSG_ERR_INVALID_ARG, "invalid argument")
        src = (ctypes.c_void_p * t)(*[f.data_ptr() if f is not None else None for f in files])
        dst = (ctypes.c_void_p * t)(*[f.data_ptr() if f is not None else None for f in targets])
        return dev, src, dst

    def heal_records_batch(self, files: Sequence, targets: Sequence, shard_len: int, n: int,
                           algo: int = _lib.RSG_HASH_HIGHWAY256S, work=None, stream=None):
        """Batched heal (rsg_heal_records_dev; Erasure::heal, heal.rs:112-206).
        `work` is accepted for compatibility and unused (ABI 3).

        `files[i]`: cuda uint8 tensor with shard i's n BitrotWriter records, or
        None (no reader).  `targets[i]`: cuda uint8 tensor of n*(32+shard_len)
        bytes that receives the rebuilt records of shard i, or None (no
        writer).  Returns the per-stripe status list (RSG_OK,
        RSG_ERR_TOO_FEW_SHARDS = read quorum, RSG_ERR_INCONSISTENT_SOURCES)."""
        dev, src, dst = self._heal_args(files, targets, shard_len, n)
        status = (ctypes.c_int * max(n, 1))()
        check(_lib.load().rsg_heal_records_dev(
            _lib.context(dev.index or 0).handle, self.data_shards, self.parity_shards, shard_len, n, src, dst,
            algo, work.data_ptr() if work is not None else None, status, self._stream_handle(stream, dev)),
            "erasure heal")
        return _lib.status_list(status, n)

    def reconstruct_batch(self, stripes, present: Sequence[bool], mode: int = _lib.RSG_RECONSTRUCT_MISSING,
                          stream=None) -> None:
        n, t, S = _check_batch(stripes, self.total_shard_count())
        pres = (ctypes.c_uint8 * t)(*[1 if p else 0 for p in present])
        check(_lib.load().rsg_reconstruct_batch_dev(
            _lib.context(_device_of(stripes)).handle, self.data_shards, self.parity_shards, S, n,
            stripes.data_ptr(), S, t * S, pres, mode, _stream_of(stripes, stream)),
            "Reed-Solomon reconstruct failed")

    def verify_batch(self, stripes, stream=None):
        import torch
        n, t, S = _check_batch(stripes, self.total_shard_count())
        ok = torch.empty(n, dtype=torch.uint8, device=stripes.device)
        check(_lib.load().rsg_verify_batch_dev(
            _lib.context(_device_of(stripes)).handle, self.data_shards, self.parity_shards, S, n,
            stripes.data_ptr(), S, t * S, ok.data_ptr(), _stream_of(stripes, stream)),
            "Reed-Solomon verify failed")
        return ok


class HostBatchTicket:
    """A submitted host-batch encode (rsg_encode_batch_host_submit).  Holds
    references to the job's arrays until it completes."""

    def __init__(self, ctx, ticket: int, keep):
        self._ctx = ctx
        self.ticket = ticket
        self._keep = keep
        self._done = False

    def poll(self) -> bool:
        """True once the job has finished (raises its error, if any)."""
        if self._done:
            return True
        done = ctypes.c_int(0)
        st = _lib.load().rsg_poll(self._ctx.handle, self.ticket, ctypes.byref(done))
        if done.value:  # finished (successfully or not): nothing writes into the arrays any more
            self._done, self._keep = True, None
        check(st, "Reed-Solomon encode failed")
        return self._done

    def wait(self) -> None:
        if self._done:
            return
        st = _lib.load().rsg_wait(self._ctx.handle, self.ticket)
        self._done, self._keep = True, None
        check(st, "Reed-Solomon encode failed")

    def __del__(self):  # never leave a job writing into freed arrays
        try:
            if not self._done:
                self.wait()
        except Exception:
            pass


class RecordTicket:
    """A submitted GET or heal (rsg_decode_records_submit /
    rsg_heal_records_submit).  Holds the call's buffers and status arrays
    until it completes; wait() returns what the synchronous call returns."""

    def __init__(self, ctx, ticket: int, keep, result, what: str):
        self._ctx = ctx
        self.ticket = ticket
        self._keep = keep
        self._result = result
        self._what = what
        self._done = False
        self._value = None
        self._error = None

    def _complete(self, st: int) -> None:
        self._done = True
        try:
            check(st, self._what)
            self._value = self._result()
        except RsgError as err:
            self._error = err
        self._keep = None

    def poll(self) -> bool:
        if not self._done:
            done = ctypes.c_int(0)
            st = _lib.load().rsg_poll(self._ctx.handle, self.ticket, ctypes.byref(done))
            if not done.value:
                check(st, self._what)
                return False
            self._complete(st)
        return True

    def wait(self):
        if not self._done:
            self._complete(_lib.load().rsg_wait(self._ctx.handle, self.ticket))
        if self._error is not None:
            raise self._error
        return self._value

    def __del__(self):  # never leave a job reading or writing freed buffers
        try:
            if not self._done:
                self._complete(_lib.load().rsg_wait(self._ctx.handle, self.ticket))
        except Exception:
            pass


# ---------------------------------------------------------------------------
# The GET decode-engine seam (crates/ecstore/src/erasure/codec/bridge.rs:33-50):
# a GPU arm beside RustfsCodecDecodeEngine (bridge.rs:137-307), same outcome
# labels, same error messages.

GET_RECONSTRUCT_OUTCOME_SKIP_DATA_COMPLETE = "skip_data_complete"  # bridge.rs:25
GET_RECONSTRUCT_OUTCOME_SKIP_EMPTY_PAYLOAD = "skip_empty_payload"  # bridge.rs:26
GET_RECONSTRUCT_OUTCOME_GPU_CALLED = "rsgpu_called"


class GpuDecodeWorkspace:
    """RustfsCodecDecodeWorkspace's role: carries the shard length the engine
    was prepared for (the device buffers live in the library's context)."""

    def __init__(self, shard_len: int):
        self._shard_len = shard_len

    def shard_len(self) -> int:
        return self._shard_len


class GpuCodecDecodeEngine:
    """ErasureDecodeEngine (bridge.rs:33-50) on librsgpu, with
    RustfsCodecDecodeEngine::reconstruct_into's semantics (bridge.rs:274-307):
    data complete -> skip; all-empty payload -> empty data shards; a missing
    data shard with more than k shards available -> rebuild every missing
    shard and verify the whole set (InvalidData "inconsistent read source
    shards", bridge.rs:202-236); otherwise rebuild the missing data only."""

    def __init__(self, erasure: Erasure):
        self.erasure = erasure
        self._enc = ReedSolomonEncoder(erasure.data_shards, erasure.parity_shards, erasure._device) \
            if erasure.parity_shards else None

    def data_shards(self) -> int:
        return self.erasure.data_shards

    def parity_shards(self) -> int:
        return self.erasure.parity_shards

    def block_size(self) -> int:
        return self.erasure.block_size

    def engine_name(self) -> str:
        return "rsgpu"

    def supports_progressive_decode(self) -> bool:
        return False

    def supports_aligned_shards(self) -> bool:
        return False

    def prepare_workspace(self, shard_len: int) -> GpuDecodeWorkspace:
        return GpuDecodeWorkspace(shard_len)

    def reconstruct_into(self, shards: List, workspace: Optional[GpuDecodeWorkspace] = None) -> str:
        k, m = self.erasure.data_shards, self.erasure.parity_shards
        if len(shards) >= k and all(s is not None for s in shards[:k]):  # data_shards_complete, bridge.rs:52
            return GET_RECONSTRUCT_OUTCOME_SKIP_DATA_COMPLETE
        if len(shards) != k + m:  # recover_empty_payload_data_shards, bridge.rs:56-84
            raise RsgError(_lib.RSG_ERR_INVALID_SHARD_COUNT,
                           f"invalid shard count: got {len(shards)}, expected {k + m}")
        present = [s for s in shards if s is not None]
        if present and all(len(s) == 0 for s in present) and len(present) >= k:
            for i in range(k):
                if shards[i] is None:
                    shards[i] = bytearray()
            return GET_RECONSTRUCT_OUTCOME_SKIP_EMPTY_PAYLOAD
        if self._enc is not None:
            needs_verification = any(s is None for s in shards[:k]) and len(present) > k
            try:
                if needs_verification:
                    self._enc.reconstruct_opt(shards)
                else:
                    self._enc.reconstruct_data(shards)
            except RsgError as err:
                raise RsgError(err.code, "RustFS codec reconstruct failed") from err
            if needs_verification and not self._enc.verify(shards):
                raise InvalidDataError(_lib.RSG_ERR_INCONSISTENT_SOURCES)
        return GET_RECONSTRUCT_OUTCOME_GPU_CALLED


def _check_batch(stripes, total: int):
    if stripes.dtype.__str__() != "torch.uint8" or stripes.dim() != 3 or not stripes.is_contiguous():
        raise TypeError("stripes must be a contiguous uint8 tensor of shape (n, k+m, S)")
    if not stripes.is_cuda:
        raise TypeError("stripes must be device-resident (the batch path is GPU only)")
    n, t, S = stripes.shape
    if t != total:
        raise RsgError(_lib.RSG_ERR_INVALID_SHARD_COUNT, f"invalid shard count: got {t}, expected {total}")
    return int(n), int(t), int(S)


def _device_of(t) -> int:
    return t.device.index if t.device.index is not None else 0


def _stream_of(t, stream):
    if stream is not None:
        return stream if isinstance(stream, int) else stream.cuda_stream
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


def matrix(k: int, m: int) -> np.ndarray:
    """The (k+m) x k encoding matrix (host-side, rsg_matrix)."""
    out = np.zeros((k + m, k), dtype=np.uint8)
    check(_lib.load().rsg_matrix(k, m, out.ctypes.data), f"rsg_matrix({k},{m})")
    return out
