"""Single-node loopback erasure set: BASELINE config 1 plumbing.

A minimal mirror of the reference's set-level PUT/GET for one erasure set of
local directories (`SetDisks::put_object`, crates/ecstore/src/set_disk/ops/object.rs:1852;
`get_object_with_fileinfo`, crates/ecstore/src/set_disk/read.rs:683), kept to
what exercises the codec path:

* PUT: split the object into `block_size` blocks, encode every block
  (Erasure::encode_data), write each shard as interleaved `[HH256S][block]`
  records (BitrotWriter::write, bitrot.rs:464-510) to
  `<dir_i>/<object>/<version>/part.1`.
  Full blocks go through one batched call (rsg_encode_batch_host) that returns
  parity and all bitrot digests in the same pass (the encode_batched dispatch
  point, encode.rs:795-919); the short tail block through encode_data.
  put_objects takes many objects at once: all their blocks, short ones
  included, are one mixed-length batch (rsg_encode_mixed_host).
* GET: read every available shard file, verify each record before use
  (split_and_verify, bitrot.rs:227-247; a mismatching record marks that shard
  missing for the block), reconstruct missing data shards
  (decode_data_with_reconstruction_verification, erasure.rs:935-973), and
  return the first `size` bytes.  Full blocks go through the GPU GET engine
  (rsg_decode_records_into_dev, in place: only the rebuilt shards are written).
* HEAL: rebuild the shard files of replaced disks (Erasure::heal,
  heal.rs:112-206) — full blocks in one rsg_heal_records_dev call, the tail
  block through decode_data_and_parity — byte-identical to what PUT wrote.
  heal_objects heals many objects at once: all their blocks, short ones
  included, are one mixed-length batch (rsg_heal_mixed_host).
* VERIFY: deep-scan every shard file (bitrot_verify, bitrot.rs:616-655) with
  one rsg_bitrot_verify_dev call.  verify_objects scans many objects at once:
  every shard file of every object is one file of one mixed-length batch
  (rsg_bitrot_verify_mixed_host), the fourth side of put_objects, get_objects
  and heal_objects.

Commit: a PUT writes every shard file into a directory of its own version id
(the reference's per-version data_dir, which xl.meta points to), and only once
the write quorum holds replaces each disk's meta.json (naming that version and
its modification time) — one atomic rename switches a disk's part and
metadata together — then removes the version directory that meta.json named
before (a concurrent PUT's uncommitted directory is left to that PUT).  A
crash or an interleaved PUT can leave a disk on either version, never with one
version's part under another's metadata.  A disk whose writer was dropped
loses its previous version (heal rebuilds it), and a PUT that fails leaves the
previous version untouched (rename_data).  GET and heal pick the metadata
version held by at least k disks (read quorum; the most disks, then the newest
modification time) and read only the shard files of disks holding it (the
reference's quorum choice of FileInfo); no version with k disks is a read-quorum
error.

Shard placement is identity (shard i on disk i); the reference's key-hash
distribution, xl.meta, quorum and locking are out of scope.
"""
from __future__ import annotations

import json
import os
import shutil
import threading
import time
import uuid
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .bitrot import HashAlgorithm, bitrot_shard_file_size
from .erasure import Erasure, calc_shard_size
from .pipeline import DEFAULT_BATCH_BLOCKS, DEFAULT_INFLIGHT_BATCHES, GetStage, PutStage, get_stream, put_stream


class LocalErasureSet:
    def __init__(self, dirs: List[str], data_shards: int, parity_shards: int, block_size: int = 1 << 20,
                 algo: HashAlgorithm = HashAlgorithm.HighwayHash256S, device: Optional[int] = None):
        if len(dirs) != data_shards + parity_shards:
            raise ValueError("one directory per shard")
        self.dirs = dirs
        self.erasure = Erasure(data_shards, parity_shards, block_size, device=device)
        self.algo = algo
        self._put_stage = None  # page-locked PUT staging, reused across objects
        self._stage_lock = threading.Lock()  # put_object's use of _put_stage
        self._get_stage = GetStage()  # page-locked GET staging + device buffers, reused across objects
        self.last_put: dict = {}  # put_stream's counts and producer/consumer clocks

    def close(self) -> None:
        """Release the reusable GET stage's read pool (a later streamed GET
        starts a new one)."""
        self._get_stage.close()

    @property
    def k(self) -> int:
        return self.erasure.data_shards

    @property
    def m(self) -> int:
        return self.erasure.parity_shards

    def _path(self, i: int, name: str, version: str) -> str:
        """Disk i's part file of `version` (the version's own data dir)."""
        return os.path.join(self.dirs[i], name, version, "part.1")

    def part_file(self, i: int, name: str) -> Optional[str]:
        """Disk i's part file of the version its meta.json names (None: the
        disk holds no committed version of `name`)."""
        try:
            with open(os.path.join(self.dirs[i], name, "meta.json")) as f:
                return self._path(i, name, json.load(f)["version"])
        except (OSError, ValueError, KeyError):
            return None

    # ------------------------------------------------------------------ PUT
    def put_object(self, name: str, data) -> dict:
        data = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        e, k, t = self.erasure, self.k, self.k + self.m
        bs = e.block_size
        S = e.shard_size()
        nfull = data.size // bs
        tail = data.size - nfull * bs
        records: List[list] = [[] for _ in range(t)]  # buffers written with one writev per shard file
        staged = bool(nfull) and self._stage_lock.acquire(blocking=False)
        try:
            if nfull:
                if staged:
                    # page-locked (n, k+m, S) stripes + digests reused across
                    # objects (PutStage: the pad between a block's end and k*S
                    # is never written, so it stays zero, erasure.rs:858-866)
                    if self._put_stage is None or not self._put_stage.fits(1, nfull, t, S):
                        self._put_stage = PutStage(1, nfull, t, S)
                    st = self._put_stage.stripes[0][:nfull]
                    dig = self._put_stage.digests[0][:nfull]
                else:  # another thread's PUT holds the stage
                    st = np.zeros((nfull, t, S), dtype=np.uint8)
                    dig = np.zeros((nfull, t, 32), dtype=np.uint8)
                st.reshape(nfull, t * S)[:, :bs] = data[: nfull * bs].reshape(nfull, bs)
                e.encode_batch_host(st, dig, algo=self.algo.value)
                for b in range(nfull):
                    for i in range(t):
                        records[i] += [dig[b, i], st[b, i]]
            version = uuid.uuid4().hex
            try:
                self._write_records(name, records, data[nfull * bs:] if tail else None, version)
            except BaseException:
                self._discard(name, version)
                raise
        finally:
            if staged:
                self._stage_lock.release()
        return self._commit(name, int(data.size), version)

    def put_objects(self, items: Sequence[Tuple[str, object]]) -> List[dict]:
        """PUT of many objects with one encode call: every block of every
        object, full or short, is one stripe of one mixed-length batch
        (rsg_encode_mixed_host: parity and all bitrot digests in one pass),
        then each object is written and committed exactly as put_object does.
        The shard files are byte-identical to put_object's.  Returns the
        objects' metadata in order."""
        e, k, m, t = self.erasure, self.k, self.m, self.k + self.m
        bs = e.block_size
        bodies = [np.frombuffer(bytes(d), dtype=np.uint8) if not isinstance(d, np.ndarray) else d.reshape(-1)
                  for _, d in items]
        # one stripe per block, in object order: (object, offset in its body, bytes, shard length)
        blocks = [(j, b0, min(bs, body.size - b0), calc_shard_size(min(bs, body.size - b0), k))
                  for j, body in enumerate(bodies) for b0 in range(0, body.size, bs)]
        S = np.array([b[3] for b in blocks], dtype=np.uint64)
        desc = np.zeros((len(blocks), 3), dtype=np.uint64)
        desc[:, 2] = S
        if len(blocks) > 1:
            desc[1:, 0] = np.cumsum(S[:-1] * np.uint64(k))
            desc[1:, 1] = np.cumsum(S[:-1] * np.uint64(m))
        total = int(S.sum())
        metas: List[dict] = []
        with e.mixed_stage(total * k, total * m, len(blocks)) as (data, parity, dig):
            for i, (j, b0, nbytes, s) in enumerate(blocks):
                off = int(desc[i, 0])
                data[off:off + nbytes] = bodies[j][b0:b0 + nbytes]
                data[off + nbytes:off + k * s] = 0  # the pad up to k*S (erasure.rs:858-866)
            if blocks:
                e.encode_mixed_host(data, parity, desc, dig, algo=self.algo.value)
            records: List[List[list]] = [[[] for _ in range(t)] for _ in bodies]
            for i, (j, _, _, s) in enumerate(blocks):
                do, po = int(desc[i, 0]), int(desc[i, 1])
                for c in range(k):
                    records[j][c] += [dig[i, c], data[do + c * s:do + (c + 1) * s]]
                for r in range(m):
                    records[j][k + r] += [dig[i, k + r], parity[po + r * s:po + (r + 1) * s]]
            for j, (name, _) in enumerate(items):
                version = uuid.uuid4().hex
                try:
                    self._write_records(name, records[j], None, version)
                except BaseException:
                    self._discard(name, version)
                    raise
                metas.append(self._commit(name, int(bodies[j].size), version))
        return metas

    def _write_records(self, name: str, records: List[list], tail, version: str) -> None:
        e, t = self.erasure, self.k + self.m
        if tail is not None:
            shards = e.encode_data(tail)
            for i in range(t):
                records[i] += [self.algo.hash_encode(shards[i]), shards[i]]
        for i in range(t):
            os.makedirs(os.path.dirname(self._path(i, name, version)), exist_ok=True)
            fd = os.open(self._path(i, name, version), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            try:
                for c0 in range(0, len(records[i]), 512):  # IOV_MAX is 1024 on Linux
                    chunk = records[i][c0:c0 + 512]
                    done = os.writev(fd, chunk)
                    if done != sum(memoryview(r).nbytes for r in chunk):  # short write: finish plainly
                        rest = b"".join(bytes(r) for r in chunk)[done:]
                        while rest:
                            rest = rest[os.write(fd, rest):]
            finally:
                os.close(fd)

    def put_object_stream(self, name: str, reader, size: int, batch_blocks: int = DEFAULT_BATCH_BLOCKS,
                          inflight_batches: int = DEFAULT_INFLIGHT_BATCHES, read_threads: int = 4,
                          write_quorum: Optional[int] = None) -> dict:
        """PUT of a `size`-byte body read from `reader` (``readinto``) without
        holding it in memory: encode_batched's pipeline (encode.rs:795-919) —
        B-block batches through page-locked staging, GPU encode + HH256S of
        batch i overlapping the read of batch i+1 and the shard-file writes of
        batch i-1.  Produces the same files as put_object.  A shard file
        whose write fails is dropped and the PUT completes while the write
        quorum holds (MultiWriter::write_shards, encode.rs:374-430); the
        dropped shards are not committed and heal rebuilds them."""
        e, t = self.erasure, self.k + self.m
        fds: List[Optional[int]] = []
        version = uuid.uuid4().hex
        staged = self._stage_lock.acquire(blocking=False)  # else another PUT holds the stage
        try:
            for i in range(t):
                try:  # a disk that cannot take the part has no writer (DiskNotFound)
                    os.makedirs(os.path.dirname(self._path(i, name, version)), exist_ok=True)
                    fds.append(os.open(self._path(i, name, version), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644))
                except OSError:
                    fds.append(None)
            info = put_stream(e, reader, size, fds, self.algo, batch_blocks, inflight_batches,
                              self._put_stage if staged else None, read_threads, write_quorum)
            stage = info.pop("stage")
            if staged:
                self._put_stage = stage
            self.last_put = info
        except BaseException:
            self._discard(name, version)  # below quorum (or any failure): the previous version stays
            raise
        finally:
            if staged:
                self._stage_lock.release()
            for fd in fds:
                if fd is not None:
                    try:
                        os.close(fd)
                    except OSError:
                        pass
        # the dropped writers' disks are left out of the commit, as the
        # reference drops them before renaming the object into place
        return self._commit(name, size, version, skip=set(info["failed_shards"]))

    def _discard(self, name: str, version: str) -> None:
        for i in range(self.k + self.m):
            shutil.rmtree(os.path.join(self.dirs[i], name, version), ignore_errors=True)

    def _disk_version(self, i: int, name: str) -> Optional[str]:
        """The version disk i's meta.json names (None: none committed)."""
        try:
            with open(os.path.join(self.dirs[i], name, "meta.json")) as f:
                return json.load(f).get("version")
        except (OSError, ValueError):
            return None

    def _drop_version(self, i: int, name: str, version: Optional[str]) -> None:
        """Remove one version's directory on disk i — the one its meta.json
        named before a switch (nothing reads it any more).  Only that one: a
        concurrent PUT's uncommitted directory stays (that PUT commits or
        discards it)."""
        if version:
            shutil.rmtree(os.path.join(self.dirs[i], name, version), ignore_errors=True)

    def _commit(self, name: str, size: int, version: str, skip=()) -> dict:
        """Switch each disk to the new version: its meta.json is replaced in
        one rename (the part file already sits in the version's directory),
        then the disk's other versions are removed.  A skipped (dropped) disk
        keeps nothing of the previous version, so no GET or heal reads a stale
        part or size from it."""
        e = self.erasure
        meta = {"size": int(size), "data_blocks": self.k, "parity_blocks": self.m, "block_size": e.block_size,
                "shard_size": e.shard_size(), "algorithm": self.algo.name, "version": version,
                "mod_time": time.time_ns()}
        for i in range(self.k + self.m):
            old = self._disk_version(i, name)
            if i in skip:
                try:
                    os.unlink(os.path.join(self.dirs[i], name, "meta.json"))
                except OSError:
                    pass
                self._drop_version(i, name, old)
                self._drop_version(i, name, version)  # the dropped writer's partial part
                continue
            self._write_meta_file(i, name, meta)
            if old != version:
                self._drop_version(i, name, old)
        return meta

    def _write_meta_file(self, i: int, name: str, meta: dict) -> None:
        path = os.path.join(self.dirs[i], name, "meta.json")
        with open(path + ".tmp", "w") as f:
            json.dump(meta, f)
        os.replace(path + ".tmp", path)

    # ------------------------------------------------------------------ GET
    def _meta(self, name: str) -> dict:
        """The metadata version the set serves, with "disks": the disks that
        hold it.  Only a version on at least k disks can be read (read quorum,
        the reference's quorum choice of FileInfo); among those, the one held
        by the most disks, then the newest modification time.  No version
        with k disks: a read-quorum error."""
        votes: dict = {}
        for i in range(self.k + self.m):
            try:
                with open(os.path.join(self.dirs[i], name, "meta.json")) as f:
                    meta = json.load(f)
            except (OSError, ValueError):
                continue
            key = json.dumps(meta, sort_keys=True)
            votes.setdefault(key, (meta, []))[1].append(i)
        if not votes:
            raise FileNotFoundError(name)
        quorum = [v for v in votes.values() if len(v[1]) >= self.k]
        if not quorum:
            raise _lib.RsgError(_lib.RSG_ERR_TOO_FEW_SHARDS, f"{name}: no metadata version reaches read quorum")
        meta, disks = max(quorum, key=lambda v: (len(v[1]), v[0].get("mod_time", 0), -v[1][0]))
        return dict(meta, disks=disks)

    def _open_shards(self, name: str, size: int, version: str, disks=None) -> List[Optional[int]]:
        """Shard file descriptors; a missing or wrong-length file, or a disk
        not holding the chosen metadata version, is None (the reader for that
        disk is unavailable)."""
        e = self.erasure
        want = bitrot_shard_file_size(e.shard_file_size(size), e.shard_size(), self.algo)
        fds: List[Optional[int]] = []
        for i in range(self.k + self.m):
            if disks is not None and i not in disks:
                fds.append(None)
                continue
            try:
                fd = os.open(self._path(i, name, version), os.O_RDONLY)
            except OSError:
                fds.append(None)
                continue
            if os.fstat(fd).st_size != want:
                os.close(fd)
                fd = None
            fds.append(fd)
        return fds

    def get_object_stream(self, name: str, offset: int = 0, length: Optional[int] = None,
                          batch_blocks: int = DEFAULT_BATCH_BLOCKS, data_shards_only: bool = False) -> Iterator[bytes]:
        """Stream bytes [offset, offset + length) (default: to the end) of
        `name`: decode_inner's range read (decode.rs:1702-1968) with full
        blocks verified and rebuilt on the GPU B blocks at a time, the next
        batch read from the shard files while this one decodes.  The set's
        reusable GET stage stays locked while the stream is open: close() an
        abandoned stream (or consume it) so other GETs can reuse the stage;
        get_object_range does.  data_shards_only: the reference's optional
        data-shards-only read (RUSTFS_GET_LOCKSTEP_DATA_SHARDS_ONLY_ENABLE,
        pipeline.get_stream)."""
        meta = self._meta(name)
        size = meta["size"]
        fds = self._open_shards(name, size, meta["version"], meta["disks"])
        try:
            yield from get_stream(self.erasure, fds, size, offset, length, self.algo, batch_blocks, self._get_stage,
                                  data_shards_only=data_shards_only)
        finally:
            for fd in fds:
                if fd is not None:
                    os.close(fd)

    def get_object_range(self, name: str, offset: int = 0, length: Optional[int] = None) -> bytes:
        return b"".join(self.get_object_stream(name, offset, length))

    def get_object(self, name: str) -> bytes:
        return self.get_object_range(name)

    def get_objects(self, names: Sequence[str], return_exceptions: bool = False) -> list:
        """GET of many objects with one decode call, the read side of
        put_objects: every block of every object, full or short, is one stripe
        of one mixed-length batch (rsg_decode_mixed_host: verify-before-use of
        each record, then only the data shards no verified record serves are
        rebuilt).  Each shard file is read whole into its disk's host arena,
        all disks at equal offsets; a missing file, a file of the wrong length
        or a disk not holding the chosen metadata version is absent for that
        object's stripes, as _open_shards decides.  Each result equals
        get_object(name).  A failing object's exception stands in its place
        with return_exceptions; otherwise the first one is raised."""
        e, k, t = self.erasure, self.k, self.k + self.m
        bs, S = e.block_size, e.shard_size()
        results: list = [None] * len(names)
        raws: List[Optional[List[Optional[bytes]]]] = [None] * len(names)
        sizes = [0] * len(names)
        for j, name in enumerate(names):
            try:
                meta = self._meta(name)
                sizes[j] = int(meta["size"])
                if sizes[j] == 0:
                    results[j] = b""
                    continue
                fds = self._open_shards(name, sizes[j], meta["version"], meta["disks"])
                raw: List[Optional[bytes]] = []
                try:
                    for fd in fds:
                        raw.append(None if fd is None else os.pread(fd, os.fstat(fd).st_size, 0))
                finally:
                    for fd in fds:
                        if fd is not None:
                            os.close(fd)
                raws[j] = raw
            except Exception as ex:  # no metadata, no read quorum on it, an unreadable disk
                results[j] = ex
        # one stripe per block, in object order: (object, bytes, shard length, record offset, out offset)
        blocks = []
        file_off = {}
        rec_at = out_at = 0
        for j, raw in enumerate(raws):
            if raw is None:
                continue
            file_off[j] = rec_at
            for b0 in range(0, sizes[j], bs):
                nbytes = min(bs, sizes[j] - b0)
                s = calc_shard_size(nbytes, k)
                blocks.append((j, nbytes, s, rec_at, out_at))
                rec_at += 32 + s
                out_at += k * s
        if blocks:
            desc = np.zeros(len(blocks), dtype=np.dtype(list(_lib.RECORD_DESC_FIELDS)))
            desc["shard_len"] = [b[2] for b in blocks]
            desc["rec_off"] = [b[3] for b in blocks]
            desc["out_off"] = [b[4] for b in blocks]
            arenas = [np.empty(rec_at, dtype=np.uint8) for _ in range(t)]
            present = {}
            for j, off in file_off.items():
                mask = 0
                for i, r in enumerate(raws[j]):
                    if r is not None:
                        arenas[i][off:off + len(r)] = np.frombuffer(r, dtype=np.uint8)
                        mask |= 1 << i
                present[j] = mask
            desc["present"] = [present[b[0]] for b in blocks]
            rebuilt = np.empty(max(out_at, 1), dtype=np.uint8)
            status, served = e.decode_mixed_host(arenas, desc, rebuilt, True, self.algo.value)
            parts: dict = {j: [] for j in file_off}
            for i, (j, nbytes, s, ro, oo) in enumerate(blocks):
                if isinstance(parts[j], Exception):
                    continue
                if status[i] == _lib.RSG_ERR_TOO_FEW_SHARDS:
                    parts[j] = _lib.RsgError(status[i], "read quorum lost")
                elif status[i] != _lib.RSG_OK:
                    parts[j] = _lib.InvalidDataError(status[i]) if status[i] == _lib.RSG_ERR_INCONSISTENT_SOURCES \
                        else _lib.RsgError(status[i], f"get {names[j]}")
                else:
                    blk = b"".join((arenas[c][ro + 32:ro + 32 + s] if served[i] >> c & 1
                                    else rebuilt[oo + c * s:oo + (c + 1) * s]).tobytes() for c in range(k))
                    parts[j].append(blk[:nbytes])
            for j, p in parts.items():
                results[j] = p if isinstance(p, Exception) else b"".join(p)
        if not return_exceptions:
            for r in results:
                if isinstance(r, Exception):
                    raise r
        return results

    # ----------------------------------------------------------------- HEAL
    def heal_object(self, name: str, targets: List[int]) -> None:
        """Rewrite the part files of the disks in `targets` from the others."""
        import torch
        meta = self._meta(name)
        e, k, t = self.erasure, self.k, self.k + self.m
        size, bs = meta["size"], meta["block_size"]
        S = e.shard_size()
        want = bitrot_shard_file_size(e.shard_file_size(size), S, self.algo)
        raws: List[Optional[bytes]] = []
        for i in range(t):
            raw = None
            if i not in targets and i in meta["disks"]:
                try:
                    with open(self._path(i, name, meta["version"]), "rb") as f:
                        raw = f.read()
                except OSError:
                    raw = None
                if raw is not None and len(raw) != want:
                    raw = None
            raws.append(raw)
        nfull = size // bs
        rec = 32 + S
        out = {i: bytearray() for i in targets}
        if nfull:
            src = [torch.frombuffer(bytearray(r[: nfull * rec]), dtype=torch.uint8).to("cuda") if r else None
                   for r in raws]
            dst = [torch.empty(nfull * rec, dtype=torch.uint8, device="cuda") if i in targets else None
                   for i in range(t)]
            status = e.heal_records_batch(src, dst, S, nfull, algo=self.algo.value)
            bad = [x for x in status if x != _lib.RSG_OK]
            if bad:
                _lib.check(bad[0], f"heal {name}")
            for i in targets:
                out[i] += dst[i].cpu().numpy().tobytes()
        tail = size - nfull * bs
        if tail:  # the short last block: host path, verify-before-use per record
            s_blk = calc_shard_size(tail, k)
            hs = self.algo.size()
            shards: List[Optional[bytes]] = [None] * t
            for i, r in enumerate(raws):
                if r is None:
                    continue
                h, body = r[nfull * rec: nfull * rec + hs], r[nfull * rec + hs: nfull * rec + hs + s_blk]
                if len(body) == s_blk and self.algo.hash_encode(body) == h:
                    shards[i] = body
            if sum(x is not None for x in shards) < k:
                raise _lib.RsgError(_lib.RSG_ERR_TOO_FEW_SHARDS, f"heal {name}: read quorum")
            source_parity = {i: shards[i] for i in range(k, t) if shards[i] is not None}
            e.decode_data_and_parity(shards)
            for i, src_p in source_parity.items():
                if bytes(shards[i]) != bytes(src_p):
                    raise _lib.InvalidDataError(_lib.RSG_ERR_INCONSISTENT_SOURCES, f"heal {name}")
            for i in targets:
                out[i] += self.algo.hash_encode(bytes(shards[i])) + bytes(shards[i])
        self._write_healed(name, meta, out)

    def _write_healed(self, name: str, meta: dict, parts: dict) -> None:
        """The end of a heal: parts[i] is disk i's healed part file of the
        version `meta` (as _meta returns it) names."""
        meta = {key: v for key, v in meta.items() if key != "disks"}
        for i in parts:  # the healed part in the version's directory, then the disk's meta switches to it
            path = self._path(i, name, meta["version"])
            os.makedirs(os.path.dirname(path), exist_ok=True)
            tmp = path + ".heal-tmp"
            with open(tmp, "wb") as f:
                f.write(bytes(parts[i]))
            os.replace(tmp, path)
            old = self._disk_version(i, name)
            self._write_meta_file(i, name, meta)
            if old != meta["version"]:
                self._drop_version(i, name, old)

    def heal_objects(self, names: Sequence[str], targets: List[int], return_exceptions: bool = False) -> list:
        """Heal of many objects with one call, the third side of put_objects
        and get_objects: every block of every object, full or short, is one
        stripe of one mixed-length batch (rsg_heal_mixed_host: verify-before-use
        of each source record, the targets' shards rebuilt and their bitrot
        records written in the same pass).  Sources are read as get_objects
        reads them (the disks in `targets` are never read); the healed part
        files and per-disk metadata are written exactly as heal_object writes
        them, and are byte-identical to what PUT wrote.  Entry j of the result
        is None, or the exception heal_object(names[j], targets) would have
        raised, with return_exceptions; otherwise the first one is raised
        after the healthy objects have been written."""
        e, k, t = self.erasure, self.k, self.k + self.m
        targets = sorted(set(int(i) for i in targets))
        results: list = [None] * len(names)
        metas: List[Optional[dict]] = [None] * len(names)
        raws: List[Optional[List[Optional[bytes]]]] = [None] * len(names)
        for j, name in enumerate(names):
            try:
                meta = self._meta(name)
                size = int(meta["size"])
                fds = self._open_shards(name, size, meta["version"], [i for i in meta["disks"] if i not in targets])
                raw: List[Optional[bytes]] = []
                try:
                    for fd in fds:
                        raw.append(None if fd is None else os.pread(fd, os.fstat(fd).st_size, 0))
                finally:
                    for fd in fds:
                        if fd is not None:
                            os.close(fd)
                metas[j], raws[j] = meta, raw
            except Exception as ex:  # no metadata, no read quorum on it, an unreadable disk
                results[j] = ex
        # one stripe per block, in object order; an object's records lie at
        # the same offsets in the source arenas and in the target arenas
        blocks = []
        file_off, file_len = {}, {}
        rec_at = 0
        for j, raw in enumerate(raws):
            if raw is None:
                continue
            size, bs = int(metas[j]["size"]), int(metas[j]["block_size"])
            file_off[j] = rec_at
            for b0 in range(0, size, bs):
                s = calc_shard_size(min(bs, size - b0), k)
                blocks.append((j, s, rec_at))
                rec_at += 32 + s
            file_len[j] = rec_at - file_off[j]
        healed = {i: np.empty(max(rec_at, 1), dtype=np.uint8) for i in targets}
        if blocks:
            desc = np.zeros(len(blocks), dtype=np.dtype(list(_lib.RECORD_DESC_FIELDS)))
            desc["shard_len"] = [b[1] for b in blocks]
            desc["rec_off"] = [b[2] for b in blocks]
            desc["out_off"] = [b[2] for b in blocks]
            arenas = [None if i in targets else np.empty(rec_at, dtype=np.uint8) for i in range(t)]
            present = {}
            for j, off in file_off.items():
                mask = 0
                for i, r in enumerate(raws[j]):
                    if r is not None and arenas[i] is not None:
                        arenas[i][off:off + len(r)] = np.frombuffer(r, dtype=np.uint8)
                        mask |= 1 << i
                present[j] = mask
            desc["present"] = [present[b[0]] for b in blocks]
            status = e.heal_mixed_host(arenas, [healed.get(i) for i in range(t)], desc, self.algo.value)
            for i, (j, _, _) in enumerate(blocks):
                if results[j] is not None or status[i] == _lib.RSG_OK:
                    continue
                if status[i] == _lib.RSG_ERR_TOO_FEW_SHARDS:
                    results[j] = _lib.RsgError(status[i], f"heal {names[j]}: read quorum")
                elif status[i] == _lib.RSG_ERR_INCONSISTENT_SOURCES:
                    results[j] = _lib.InvalidDataError(status[i], f"heal {names[j]}")
                else:
                    results[j] = _lib.RsgError(status[i], f"heal {names[j]}")
        for j, name in enumerate(names):
            if results[j] is None:
                off = file_off[j]
                self._write_healed(name, metas[j], {i: healed[i][off:off + file_len[j]].tobytes() for i in targets})
        if not return_exceptions:
            for r in results:
                if isinstance(r, Exception):
                    raise r
        return results

    # --------------------------------------------------------------- VERIFY
    def verify_object(self, name: str) -> List[int]:
        """Deep scan: rsg_status of every shard file (RSG_OK = healthy)."""
        import torch
        from .bitrot import bitrot_verify_batch
        meta = self._meta(name)
        e, t = self.erasure, self.k + self.m
        S = e.shard_size()
        part = e.shard_file_size(meta["size"])
        want = bitrot_shard_file_size(part, S, self.algo)
        files = []
        for i in range(t):
            try:
                with open(self._path(i, name, meta["version"]), "rb") as f:
                    raw = f.read()
                files.append(torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda") if raw
                             else torch.empty(0, dtype=torch.uint8, device="cuda"))
            except OSError:
                files.append(None)
        present = [f for f in files if f is not None]
        status = bitrot_verify_batch(present, want, part, self.algo, S) if present else []
        it = iter(status)
        return [_lib.RSG_ERR_UNEXPECTED_EOF if f is None else next(it) for f in files]

    def verify_objects(self, names: Sequence[str], return_exceptions: bool = False) -> list:
        """Deep scan of many objects with one call, the fourth side of
        put_objects, get_objects and heal_objects: every shard file of every
        object is one file of one mixed-length batch
        (rsg_bitrot_verify_mixed_host), each disk's files packed into that
        disk's host arena.  Entry j equals verify_object(names[j]): the
        rsg_status of every shard file, a file that cannot be opened being
        RSG_ERR_UNEXPECTED_EOF (it gets no descriptor).  An object without
        readable metadata yields the exception verify_object would have raised,
        in its place with return_exceptions; otherwise the first one is raised.
        Memory: every shard file of every name is held at once, as read and
        again in its disk's arena (about twice the files' total bytes at the
        peak), so a caller scanning a large set passes the names in slices of
        the size it can afford; each slice is one call."""
        from .bitrot import bitrot_verify_many
        e, t = self.erasure, self.k + self.m
        S = e.shard_size()
        results: list = [None] * len(names)
        raws: List[list] = [[] for _ in range(t)]  # per disk: the files' bytes, in list order
        at = [0] * t
        rows = []   # (off, file_len, want_size, part_size, shard_size, arena)
        where = []  # (object, disk) of each row
        for j, name in enumerate(names):
            try:
                meta = self._meta(name)
            except Exception as ex:  # no metadata, no read quorum on it
                results[j] = ex
                continue
            part = e.shard_file_size(meta["size"])
            want = bitrot_shard_file_size(part, S, self.algo)
            results[j] = [_lib.RSG_ERR_UNEXPECTED_EOF] * t
            for i in range(t):
                try:
                    with open(self._path(i, name, meta["version"]), "rb") as f:
                        raw = f.read()
                except OSError:
                    continue
                rows.append((at[i], len(raw), want, part, S, i))
                where.append((j, i))
                if raw:
                    raws[i].append(raw)
                    at[i] += len(raw)
        if rows:
            arenas = [np.frombuffer(b"".join(r), dtype=np.uint8) if r else None for r in raws]
            desc = np.array(rows, dtype=np.dtype(list(_lib.FILE_DESC_FIELDS)))
            status = bitrot_verify_many(arenas, desc, self.algo)
            for (j, i), st in zip(where, status):
                results[j][i] = st
        if not return_exceptions:
            for r in results:
                if isinstance(r, Exception):
                    raise r
        return results
