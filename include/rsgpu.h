/*
 * rsgpu.h — C ABI of the MI355X-native Reed–Solomon GF(2^8) erasure engine.
 *
 * This is the drop-in boundary for the erasure hot path of rustfs
 * (crates/ecstore/src/erasure/).  Every entry point names the reference
 * interface it replaces; the Rust-side `extern "C"` binding a maintainer would
 * add is in INTEGRATION.md.  Plain pointers and sizes only; no torch types.
 *
 * Codec: GF(2^8) with polynomial 0x11D, generator 2, systematic matrix
 * V * inv(V[0..k]) with V[r][c] = r^c ("rs-vandermonde", the construction of
 * reed_solomon_erasure::galois_8::ReedSolomon used by rustfs and MinIO;
 * docs/architecture/erasure-coding.md:41-50).  Outputs are bit-exact with it.
 *
 * Threading: every function is thread-safe.  A context owns one device and
 * per-geometry coefficient caches.  Host-buffer calls (rsg_encode,
 * rsg_reconstruct, rsg_verify, rsg_hash) run on one of the context's 8 lanes
 * (own stream and device buffer), so up to 8 concurrent callers overlap and
 * further ones wait for a free lane (the reference calls encode from many
 * tokio workers concurrently, encode.rs:511-526).  Device-batch calls are
 * asynchronous on the caller's stream; every record-engine call (decode / heal /
 * bitrot_verify) takes its own scratch from the context's pool, so concurrent
 * calls overlap.  Tickets (host-batch PUT, asynchronous GET / heal) may be
 * polled or waited on from several threads.
 *
 * Errors: functions return an rsg_status; rsg_strerror() gives the message
 * fragment the reference uses for the same condition (erasure.rs:87-121,
 * 396-446, 505-594; bridge.rs:202-235; bitrot.rs:227-247).
 */
#ifndef RSGPU_H
#define RSGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSG_ABI_VERSION 6
#define RSG_MAX_TOTAL_SHARDS 256 /* galois_8::Field::ORDER, erasure.rs:72 */
#define RSG_DIGEST_BYTES 32      /* HighwayHash-256 */

typedef enum rsg_status {
    RSG_OK = 0,
    RSG_ERR_INVALID_ARG = 1,           /* null pointer / bad flag */
    RSG_ERR_ZERO_DATA_SHARDS = 2,      /* ErasureConstructionError::ZeroDataShards, erasure.rs:90 */
    RSG_ERR_ZERO_PARITY_SHARDS = 3,    /* reed_solomon_erasure::Error::TooFewParityShards */
    RSG_ERR_TOO_MANY_SHARDS = 4,       /* UnsupportedModernShardCount, erasure.rs:102 */
    RSG_ERR_INVALID_SHARD_COUNT = 5,   /* "invalid shard count", erasure.rs:512 */
    RSG_ERR_INCONSISTENT_LENGTH = 6,   /* "inconsistent shard length", erasure.rs:536 */
    RSG_ERR_EMPTY_SHARD = 7,           /* reed_solomon_erasure::Error::EmptyShard */
    RSG_ERR_TOO_FEW_SHARDS = 8,        /* Error::TooFewShardsPresent -> "Reed-Solomon reconstruct failed" */
    RSG_ERR_NO_VALID_SHARDS = 9,       /* "No valid shards found", erasure.rs:521 */
    RSG_ERR_INCONSISTENT_SOURCES = 10, /* InvalidData "inconsistent read source shards", bridge.rs:231 */
    RSG_ERR_BITROT_MISMATCH = 11,      /* InvalidData "bitrot hash mismatch", bitrot.rs:241 */
    RSG_ERR_NO_DEVICE = 12,            /* no HIP device / bad ordinal */
    RSG_ERR_DEVICE = 13,               /* HIP runtime failure */
    RSG_ERR_OUT_OF_MEMORY = 14,
    RSG_ERR_UNSUPPORTED = 15,
    RSG_ERR_FILE_SIZE_MISMATCH = 16,   /* "bitrot shard file size mismatch", bitrot.rs:627 */
    RSG_ERR_UNEXPECTED_EOF = 17,       /* io::ErrorKind::UnexpectedEof from read_exact, bitrot.rs:631,639 */
    RSG_ERR_TRAILING_DATA = 18         /* "bitrot shard file has trailing data", bitrot.rs:651 */
} rsg_status;

/* Bitrot hash selector (crates/utils/src/hash.rs:52-68). */
typedef enum rsg_hash_algo {
    RSG_HASH_NONE = 0,
    RSG_HASH_HIGHWAY256S = 1,        /* HashAlgorithm::HighwayHash256S (default), pi-derived key */
    RSG_HASH_HIGHWAY256S_LEGACY = 2  /* HashAlgorithm::HighwayHash256SLegacy, key [3,4,2,1] */
} rsg_hash_algo;

/* Reconstruct modes. */
typedef enum rsg_reconstruct_mode {
    /* ReedSolomonEncoder::reconstruct_data (erasure.rs:411-422): rebuild missing
     * data shards only; missing parity buffers are left untouched. */
    RSG_RECONSTRUCT_DATA = 0,
    /* reconstruct_opt (bridge.rs:296): rebuild every missing shard, data and parity. */
    RSG_RECONSTRUCT_MISSING = 1,
    /* ReedSolomonEncoder::reconstruct (erasure.rs:425-428): rebuild missing data,
     * then re-encode ALL parity shards from the data (present ones are overwritten). */
    RSG_RECONSTRUCT_REENCODE_PARITY = 2
} rsg_reconstruct_mode;

typedef struct rsg_ctx rsg_ctx;

/* ---- library / context ---- */
int rsg_abi_version(void);
const char *rsg_strerror(int status);
int rsg_device_count(int *count);
/* Create a context bound to HIP device `device`. */
int rsg_create(int device, rsg_ctx **out);
void rsg_destroy(rsg_ctx *ctx);

/* Measurement hook (no reference counterpart; bench.py): with timing on, the
 * record engines (rsg_decode_records_dev, rsg_heal_records_dev,
 * rsg_bitrot_verify_dev) record HIP events around their kernel launches on
 * the call's stream;
 * rsg_last_kernel_ms returns the summed kernel time of the last such call
 * (-1 if none was timed).  Off by default. */
int rsg_set_kernel_timing(rsg_ctx *ctx, int on);
int rsg_last_kernel_ms(rsg_ctx *ctx, float *ms);

/* Record-engine path of rsg_decode_records_dev / rsg_heal_records_dev (no
 * reference counterpart; tests and A/B runs).  AUTO (default): the one-pass
 * kernel from 1024 stripes where the geometry has one, else the two-pass
 * path; ONE_PASS / TWO_PASS force a path where the geometry allows it.  Both
 * paths produce identical bytes and statuses. */
typedef enum rsg_record_engine {
    RSG_RECORD_ENGINE_AUTO = 0,
    RSG_RECORD_ENGINE_ONE_PASS = 1,
    RSG_RECORD_ENGINE_TWO_PASS = 2
} rsg_record_engine;
int rsg_set_record_engine(rsg_ctx *ctx, int engine);

/* Kernel-choice knobs (no reference counterpart; ABI 6: tests and A/B runs).
 * The library runs its defaults; nothing in the process environment changes
 * them (the RSG_* variables are read only by measurement builds compiled with
 * RSG_MEASUREMENT_BUILD).  rsg_set_tuning(name, value) sets one knob for the
 * whole process (every context): value NULL = that knob's default, name NULL
 * = every knob's default; an unknown name or a value the knob does not take is
 * RSG_ERR_INVALID_ARG and changes nothing.  Launches already queued keep the
 * setting they were made with.  Every setting produces identical bytes and
 * statuses; only the kernel (and its speed) differs.  rsg_get_tuning writes
 * the knob's current value (NUL-terminated, at most cap bytes).  Knobs (value
 * syntax): RSG_FUSED, RSG_LOST_DISK_FAST, RSG_ZERO_COPY, RSG_ROLLED,
 * RSG_HASH_COPY, RSG_FUSED_SPW1, RSG_DECODE_NET, RSG_HASH_UNAL, RSG_GET_CACHED
 * (0|1); RSG_VEC_BLOCK (0|64|256); RSG_VEC_OCC (-1..8); RSG_HASH_DEPTH (1..3);
 * RSG_FUSED_KIND (auto|packed|ring|dma|wide2|wide4|split2|split4|net|table);
 * RSG_ENC_PRIO, RSG_DMA_PRIO, RSG_DMA_NT (0..3); RSG_DMA_EW (2|4);
 * RSG_DMA_SPW (4|8); RSG_NET12_RD (2; 4 only in measurement builds, whose
 * library carries that A/B kernel form).  INTEGRATION.md lists what each
 * selects. */
int rsg_set_tuning(const char *name, const char *value);
int rsg_get_tuning(const char *name, char *out, size_t cap);

/* Fault injection, tests only (no reference counterpart; ABI 5): sub-batch
 * `index` of every later rsg_encode_batch_host_submit on this context fails
 * to enqueue with RSG_ERR_DEVICE (-1, the default: never).  Lets the tests
 * check that a failing submit drains the sub-batches it had queued.  Nothing
 * else (no environment variable) can trigger it. */
int rsg_test_fail_subbatch(rsg_ctx *ctx, int index);

/* Encoding matrix ((k+m) x k, row-major) as reed_solomon_erasure::ReedSolomon::new
 * builds it (erasure.rs:448-470 cached_modern_reed_solomon).  Host only. */
int rsg_matrix(int k, int m, uint8_t *out);
/* Validate a geometry like Erasure::try_new_with_options (erasure.rs:708-773):
 * k > 0, k+m <= 256.  m == 0 is valid (no codec; encode is a no-op). */
int rsg_check_geometry(int k, int m);

/* ---- host-buffer API: drop-in for ReedSolomonEncoder (erasure.rs:358-446) ----
 * `shards` holds k+m host pointers of shard_len bytes each: k data then m parity. */

/* ReedSolomonEncoder::encode (erasure.rs:396-408): overwrite shards[k..k+m). */
int rsg_encode(rsg_ctx *ctx, int k, int m, size_t shard_len, uint8_t *const *shards);

/* ReedSolomonEncoder::reconstruct_data / reconstruct and reconstruct_opt
 * (erasure.rs:411-428, bridge.rs:295-301).  present[i] != 0 marks shard i valid;
 * every pointer must be a writable shard_len buffer; rebuilt shards are written
 * in place.  Fewer than k present -> RSG_ERR_TOO_FEW_SHARDS. */
int rsg_reconstruct(rsg_ctx *ctx, int k, int m, size_t shard_len, uint8_t *const *shards,
                    const uint8_t *present, int mode);

/* ReedSolomonEncoder::verify (erasure.rs:430-441): *ok = 1 when every parity
 * shard equals the parity re-encoded from the data shards. */
int rsg_verify(rsg_ctx *ctx, int k, int m, size_t shard_len, const uint8_t *const *shards, int *ok);

/* HashAlgorithm::hash_encode for the Highway variants (hash.rs:114-141). */
int rsg_hash(rsg_ctx *ctx, int algo, const uint8_t *data, size_t len, uint8_t out[32]);

/* ---- device-batch API: the batched GPU path (encode.rs:795-919 dispatch point) ----
 * d_stripes: device memory holding n stripes.  Stripe s, shard i starts at
 *   d_stripes + s*stripe_stride + i*shard_pitch   (a3 layout: shard_pitch = shard_len,
 *   stripe_stride = (k+m)*shard_len, erasure.rs:848-887).
 * stream: a hipStream_t; NULL = the HIP null (default) stream.  Calls are
 * asynchronous and ordered with other work on that stream. */

/* Encode parity for n stripes; if d_digests != NULL and algo != NONE also write
 * the (k+m) per-shard bitrot digests of every stripe, [n][k+m][32] — identical to
 * BitrotWriter::write's prefix (bitrot.rs:496-502) — in the same pass. */
int rsg_encode_batch_dev(rsg_ctx *ctx, int k, int m, size_t shard_len, size_t n,
                         uint8_t *d_stripes, size_t shard_pitch, size_t stripe_stride,
                         uint8_t *d_digests, int algo, void *stream);

/* Reconstruct n stripes that share one erasure pattern `present` (k+m host bytes). */
int rsg_reconstruct_batch_dev(rsg_ctx *ctx, int k, int m, size_t shard_len, size_t n,
                              uint8_t *d_stripes, size_t shard_pitch, size_t stripe_stride,
                              const uint8_t *present, int mode, void *stream);

/* Per-stripe parity check of n complete stripes: d_ok[s] = 1 if consistent. */
int rsg_verify_batch_dev(rsg_ctx *ctx, int k, int m, size_t shard_len, size_t n,
                         const uint8_t *d_stripes, size_t shard_pitch, size_t stripe_stride,
                         uint8_t *d_ok, void *stream);

/* Hash n messages of len bytes each (message j at d_data + j*stride) into
 * d_out[n][32] (HashAlgorithm::hash_encode, hash.rs:114). */
int rsg_hash_batch_dev(rsg_ctx *ctx, int algo, const uint8_t *d_data, size_t len, size_t stride,
                       size_t n, uint8_t *d_out, void *stream);

/* DEPRECATED since ABI 6 (kept so ABI-4 bindings stay valid; nothing in this
 * repository calls it): use rsg_decode_records_into_dev, the form the
 * reference's GET has — write_data_blocks writes from the per-shard buffers
 * (decode.rs:1390), so copying every present data shard into one block buffer
 * is work the reference does not do, and at RS(12,4) this form runs at a third
 * of the HBM roofline (records 2 mod 8 copied to 8-aligned rows).
 * GET-side engine, batched, gather form (RustfsCodecDecodeEngine::reconstruct_into,
 * bridge.rs:274-307, with BitrotReader's verify-before-use, bitrot.rs:227-247).
 * Shard i of n stripes is resident on the device in BitrotWriter layout:
 * record s at d_files[i] + s*(32+shard_len) = [32-byte digest][shard_len bytes]
 * (d_files[i] == NULL: shard unavailable).  Every available record is hashed
 * and compared with its digest; a mismatching record counts as missing for
 * that stripe only.  The k data shards of stripe s are written contiguously to
 * d_out + s*k*shard_len (present ones copied, missing ones rebuilt from the
 * first k valid shards).  With verify_surplus, stripes that rebuilt data while
 * holding more than k valid shards re-derive the surplus parity and compare
 * (decode_data_with_reconstruction_verification, erasure.rs:935-973).
 * h_status[s] (host array): RSG_OK, RSG_ERR_TOO_FEW_SHARDS or
 * RSG_ERR_INCONSISTENT_SOURCES.  Synchronous. */
int rsg_decode_records_dev(rsg_ctx *ctx, int k, int m, size_t shard_len, size_t n,
                           const uint8_t *const *d_files, int algo, int verify_surplus,
                           uint8_t *d_out, int *h_status, void *stream);

/* GET-side engine, in-place form (ABI 5): RustfsCodecDecodeEngine::reconstruct_into
 * (bridge.rs:274-307) fills only the None slots of its shards slice and skips a
 * stripe whose data shards are all present (data_shards_complete ->
 * skip_data_complete, bridge.rs:52-54); write_data_blocks then writes straight
 * from the per-shard buffers (decode.rs:1390).  Same sources, verification and
 * statuses as rsg_decode_records_dev, but a data shard whose record verifies is
 * served from that record (its body at d_files[i] + s*(32+shard_len) + 32) and
 * nothing is copied; only the shards no verified record serves — file absent or
 * record rotten — are rebuilt, into d_targets[i] + s*target_stride.
 * d_targets: k device slots, one per data shard, each at least
 * (n-1)*target_stride + shard_len bytes (target_stride >= shard_len;
 * target_stride = k*shard_len with d_targets[i] = base + i*shard_len gives the
 * contiguous block layout); a slot range overlapping a source record file, or
 * two slots with a stripe window in common (some s, s' with
 * [d_targets[i] + s*target_stride, +shard_len) and [d_targets[j] +
 * s'*target_stride, +shard_len) sharing a byte), is RSG_ERR_INVALID_ARG.  With every data file present the call only verifies
 * the k data records of each stripe (parity is read for a stripe only if one of
 * its data records is rotten).  h_src (host, optional, k*n bytes, [shard][stripe]):
 * 1 where data shard i of stripe s is served from its record, 0 where it was
 * written to its slot (unspecified for a failed stripe).  Synchronous. */
int rsg_decode_records_into_dev(rsg_ctx *ctx, int k, int m, size_t shard_len, size_t n,
                                const uint8_t *const *d_files, int algo, int verify_surplus,
                                uint8_t *const *d_targets, size_t target_stride, uint8_t *h_src,
                                int *h_status, void *stream);

/* Asynchronous GET (ABI 5): either form — d_out (gather, deprecated as
 * rsg_decode_records_dev) or d_targets + target_stride (in place), exactly one
 * non-NULL — queued on `stream` with a
 * ticket returned at once, so a caller decoding many batches (decode.rs's
 * pipeline, decode.rs:1702-1968) overlaps one batch's status handling with the
 * next batch's kernels.  rsg_poll / rsg_wait complete it (the same tickets as
 * the host-batch PUT); h_status and h_src are filled when the ticket completes,
 * and every buffer must stay alive and unmodified (sources) / unread (outputs)
 * until then.  Each call uses its own scratch: calls from several threads run
 * concurrently.  Completion normally needs no further device work; a batch with
 * a rotten record is redone for the affected stripes inside the wait/poll that
 * completes it. */
int rsg_decode_records_submit(rsg_ctx *ctx, int k, int m, size_t shard_len, size_t n,
                              const uint8_t *const *d_files, int algo, int verify_surplus,
                              uint8_t *d_out, uint8_t *const *d_targets, size_t target_stride,
                              uint8_t *h_src, int *h_status, void *stream, uint64_t *ticket);

/* Heal, batched (Erasure::heal, heal.rs:112-206, which calls
 * decode_data_and_parity, erasure.rs:917, per block).  Sources as in
 * rsg_decode_records_dev (d_files[i] == NULL: no reader; every record is
 * verified before use).  d_targets[i] != NULL marks shard i as a heal target
 * (a writer; a target range overlapping any source or another target is
 * RSG_ERR_INVALID_ARG): it receives n BitrotWriter records
 * [HH256S][shard_len bytes] (stride 32+shard_len) of the rebuilt shard i (data
 * shards as read/rebuilt, parity re-encoded), computed in one pass over the
 * survivors.  Every verified source parity is compared with the parity
 * re-encoded from the data (heal.rs:180-196).  d_work: unused since ABI 3
 * (may be NULL; kept so existing bindings stay valid).
 * h_status[s]: RSG_OK, RSG_ERR_TOO_FEW_SHARDS (ErasureReadQuorum) or
 * RSG_ERR_INCONSISTENT_SOURCES ("inconsistent heal source shards"); target
 * records of a failed stripe carry an all-zero digest header (they never
 * verify) and unspecified bodies.  Synchronous. */
int rsg_heal_records_dev(rsg_ctx *ctx, int k, int m, size_t shard_len, size_t n,
                         const uint8_t *const *d_files, uint8_t *const *d_targets, int algo,
                         uint8_t *d_work, int *h_status, void *stream);

/* Asynchronous heal (ABI 5): rsg_heal_records_dev queued with a ticket, as
 * rsg_decode_records_submit (heal.rs's per-block loop, heal.rs:112-206, batched
 * and overlapped). */
int rsg_heal_records_submit(rsg_ctx *ctx, int k, int m, size_t shard_len, size_t n,
                            const uint8_t *const *d_files, uint8_t *const *d_targets, int algo,
                            int *h_status, void *stream, uint64_t *ticket);

/* Whole-shard-file bitrot verification (bitrot_verify, bitrot.rs:616-655) of
 * n_files device-resident shard files of one part (file f: file_lens[f]
 * bytes at d_files[f]).  want_size must equal
 * bitrot_shard_file_size(part_size, shard_size, algo) (else every file gets
 * RSG_ERR_FILE_SIZE_MISMATCH); then records are checked in order like the
 * reference's read loop: h_status[f] = RSG_ERR_BITROT_MISMATCH at the first
 * bad digest, RSG_ERR_UNEXPECTED_EOF if the file ends early,
 * RSG_ERR_TRAILING_DATA if it is longer than want_size, else RSG_OK.
 * algo: HIGHWAY256S / LEGACY (streaming records) or NONE (sizes only);
 * whole-file algorithms are RSG_ERR_UNSUPPORTED, as in the reference.
 * Synchronous. */
int rsg_bitrot_verify_dev(rsg_ctx *ctx, int algo, size_t n_files, const uint8_t *const *d_files,
                          const size_t *file_lens, size_t want_size, size_t part_size, size_t shard_size,
                          int *h_status, void *stream);

/* Block until all work queued on `stream` (NULL = the null stream) is done. */
int rsg_sync(rsg_ctx *ctx, void *stream);

/* ---- host-batch API: the PUT path starts and ends in host memory ----
 * Encode n stripes held in HOST memory (same addressing as the device-batch
 * API): sub-batches are pipelined over the context's stream/staging slots
 * (H2D data -> encode + fused digests -> D2H parity + digests).  This is the
 * batched replacement for encode_batched's per-block encode_data_block calls
 * (encode.rs:795-919); pin the buffers (rsg_pin or a pinned allocation) for
 * full PCIe bandwidth and for the copies to run asynchronously.  With m == 0
 * only the digests are computed; an empty shard hashes as the empty message.
 *
 * Asynchronous form: rsg_encode_batch_host_submit queues the job and returns
 * a ticket at once; jobs run in submission order and the sub-batches of
 * consecutive jobs overlap, so a producer reads and submits batch i+1 (and
 * writes batch i-1's shards) while the GPU encodes batch i — the bounded
 * in-flight queue of encode_batched (RUSTFS_ERASURE_ENCODE_MAX_INFLIGHT_BYTES,
 * encode.rs:64-72) with the caller choosing the bound.  h_stripes / h_digests
 * must stay alive and untouched until the ticket completes.
 * rsg_poll sets *done = 1 (and releases the ticket) when the job has finished,
 * returning its status; rsg_wait blocks until then.  An unknown or already
 * released ticket is RSG_ERR_INVALID_ARG.  Several threads may poll or wait
 * on one ticket; all of them see it finish.  If submit returns an error, no
 * ticket is issued and none of the job's copies is still in flight: the
 * sub-batches it had already queued are drained before it returns, so the
 * caller may reuse or free h_stripes / h_digests at once (their contents are
 * then unspecified).  rsg_encode_batch_host = submit + wait. */
int rsg_encode_batch_host(rsg_ctx *ctx, int k, int m, size_t shard_len, size_t n, uint8_t *h_stripes,
                          size_t shard_pitch, size_t stripe_stride, uint8_t *h_digests, int algo);
int rsg_encode_batch_host_submit(rsg_ctx *ctx, int k, int m, size_t shard_len, size_t n, uint8_t *h_stripes,
                                 size_t shard_pitch, size_t stripe_stride, uint8_t *h_digests, int algo,
                                 uint64_t *ticket);
int rsg_poll(rsg_ctx *ctx, uint64_t ticket, int *done);
int rsg_wait(rsg_ctx *ctx, uint64_t ticket);

/* ---- mixed-length batch: n unrelated stripes, each with its own shard length ----
 * The batched form of the small-object path, encode_inline_shards_with_size_hint
 * (encode.rs:601-628), which encodes one body of whatever size the client sent,
 * and of the short last block of every object (encode_buffer's ceil(len / k)
 * shards, erasure.rs:848-887): parity and all k+m bitrot digests of n blocks
 * of different lengths in one launch.
 * Stripe j (h_desc[j], a host array the call does not keep): data shard c is
 * at data + data_off + c*shard_len (k shards back to back, as encode_buffer
 * lays them out), parity shard r is written at parity + parity_off +
 * r*shard_len, the k+m digests at digests + j*(k+m)*32 (caller order; NULL or
 * algo NONE: parity only).  Any shard length up to 0xffffffff and any
 * alignment; shard_len == 0 touches no memory and its digests are those of
 * the empty message.  The descriptors must list stripes in ascending,
 * disjoint order: data ranges [data_off, +k*shard_len) strictly ascending,
 * parity ranges [parity_off, +m*shard_len) likewise, and no parity range may
 * meet a data range or another parity range when the two arenas alias
 * (parity == data with parity_off = data_off + k*shard_len is the a3 layout
 * and is valid); anything else, a NULL pointer or an unknown algo is
 * RSG_ERR_INVALID_ARG with nothing written.  Geometry errors as
 * rsg_check_geometry; n == 0 is RSG_OK.
 * One launch for k <= 16 with m = 1..4 (the fused encode + hash kernels'
 * range); m == 0 (digests only), m > 4 and k > 16 give the same results
 * through the per-length kernels, a few launches per stripe.
 *
 * rsg_encode_mixed_dev: device arenas, asynchronous on `stream` like
 * rsg_encode_batch_dev.
 *
 * rsg_encode_mixed_host / _submit: host arenas, pipelined over the host-batch
 * stream/staging slots with the same tickets (rsg_poll / rsg_wait) and the
 * same contract as rsg_encode_batch_host_submit (a failed submit drains what
 * it queued).  Consecutive stripes are taken into sub-batches whose data span,
 * parity span (first start to last end, gaps included) and digests fit
 * RSG_MIXED_STAGE_BYTES of staging; a larger stripe gets a sub-batch of its
 * own.  Each sub-batch is one H2D copy of its data span, one small descriptor
 * copy, one launch, and one D2H copy each of its parity span and digests: the
 * bytes of the parity span between parity ranges are overwritten with
 * unspecified values, so pack the arenas densely.  The host data span and
 * parity span of a call must not intersect (RSG_ERR_INVALID_ARG). */
#define RSG_MIXED_STAGE_BYTES (32u << 20)
typedef struct rsg_stripe_desc {
    uint64_t data_off, parity_off, shard_len;
} rsg_stripe_desc;
int rsg_encode_mixed_dev(rsg_ctx *ctx, int k, int m, size_t n, const rsg_stripe_desc *h_desc,
                         const uint8_t *d_data, uint8_t *d_parity, uint8_t *d_digests, int algo,
                         void *stream);
int rsg_encode_mixed_host(rsg_ctx *ctx, int k, int m, size_t n, const rsg_stripe_desc *h_desc,
                          const uint8_t *h_data, uint8_t *h_parity, uint8_t *h_digests, int algo);
int rsg_encode_mixed_host_submit(rsg_ctx *ctx, int k, int m, size_t n, const rsg_stripe_desc *h_desc,
                                 const uint8_t *h_data, uint8_t *h_parity, uint8_t *h_digests, int algo,
                                 uint64_t *ticket);

/* ---- mixed-length batch GET: verify + rebuild n unrelated record stripes ----
 * The read side of the above: per stripe, verify-before-use of each
 * [hash][shard] record (bitrot.rs:139-247), then
 * decode_data_with_reconstruction_verification (erasure.rs:935-973) with only
 * the absent data shards filled (bridge.rs:274-307), over stripes whose shard
 * lengths, sets of present shards and rot all differ.  The contract is
 * rsg_decode_records_into_dev's, applied per stripe.
 * files: k+m record arenas, one per disk; a NULL arena means shard i is absent
 * for every stripe, whatever `present` says.  Stripe s (h_desc[s], a host array
 * the call does not keep): shard i's record [32-byte digest][shard_len bytes]
 * is at files[i] + rec_off when bit i of `present` is set; shard_len == 0: the
 * records are bare digests of the empty message.
 * Every record the decode of a stripe uses is hashed and compared with its
 * header first; a mismatching record counts as absent for that stripe only.
 * A data shard c whose record verifies is served from that record: bit c of
 * h_served[s] is set and nothing is written for it.  Only the data shards no
 * verified record serves are rebuilt, at out + out_off + c*shard_len, from
 * the first k verified shards in ascending index.  With verify_surplus, a
 * stripe that rebuilt data while holding more than k verified shards
 * re-derives every surplus parity shard and compares it byte for byte.  When
 * every data record of a stripe verifies, its parity records are not read.
 * h_status[s]: RSG_OK, RSG_ERR_TOO_FEW_SHARDS (fewer than k verified) or
 * RSG_ERR_INCONSISTENT_SOURCES; h_served[s] is unspecified for a failed stripe.
 * algo: HIGHWAY256S or HIGHWAY256S_LEGACY.  Synchronous.
 * The call leaves alone every byte of `out` outside the windows of rebuilt
 * shards (the gaps and the windows of served shards included) and every byte
 * of the sources.  The window of a data shard that `present` or a NULL arena
 * declares absent, or whose record fails its hash, is written before the
 * stripe's verdict is known, so it holds unspecified bytes when the stripe
 * fails (rsg_decode_mixed_dev; the host form copies nothing back for a failed
 * stripe).
 * RSG_ERR_INVALID_ARG with nothing written: a `present` bit at or above k+m;
 * record ranges [rec_off, +32+shard_len) or non-empty out ranges [out_off,
 * +k*shard_len) not strictly ascending and disjoint in list order; a range
 * that wraps the address space; the out span meeting the record span of an
 * arena that is read; a NULL pointer; an unknown algo; k+m > 32
 * (RSG_ERR_UNSUPPORTED).  Geometry errors as rsg_check_geometry; n == 0 is
 * RSG_OK.
 * k <= 16 with m <= 4 (m == 0 only verifies) run one launch per distinct set
 * of readable shards, and again for the stripes in which a record failed its
 * hash, under the reduced set (at most k+m rounds).  Other geometries give
 * the same results through rsg_decode_records_into_dev, stripe by stripe;
 * there a stripe with shard_len == 0 is judged by `present` alone.
 *
 * rsg_decode_mixed_dev: device arenas; runs on `stream` and waits for it.
 *
 * rsg_decode_mixed_host: host arenas, page-locked or pageable.  Consecutive
 * stripes are taken into sub-batches that fit RSG_MIXED_STAGE_BYTES of the
 * host-batch staging slots (a larger stripe gets a sub-batch of its own); a
 * sub-batch copies up the record span (first record's start to last record's
 * end) of every arena that some stripe of it may read, not only the files its
 * plans read, and copies back only the out windows of shards it rebuilt. */
typedef struct rsg_record_desc {
    uint64_t rec_off;   /* shard i's record of this stripe at files[i] + rec_off */
    uint64_t out_off;   /* a rebuilt data shard c is written to out + out_off + c*shard_len
                           (rsg_heal_mixed_*: target i's record at targets[i] + out_off) */
    uint32_t shard_len; /* 0: the records are bare digests of the empty message */
    uint32_t present;   /* bit i set: shard i's record of this stripe may be read (i < k+m) */
} rsg_record_desc;
int rsg_decode_mixed_dev(rsg_ctx *ctx, int k, int m, size_t n, const rsg_record_desc *h_desc,
                         const uint8_t *const *d_files, int algo, int verify_surplus, uint8_t *d_out,
                         uint32_t *h_served, int *h_status, void *stream);
int rsg_decode_mixed_host(rsg_ctx *ctx, int k, int m, size_t n, const rsg_record_desc *h_desc,
                          const uint8_t *const *h_files, int algo, int verify_surplus, uint8_t *h_out,
                          uint32_t *h_served, int *h_status);

/* ---- mixed-length batch heal: rebuild the target shards' records of n unrelated stripes ----
 * The third mixed-length path: Erasure::heal (heal.rs:112-206), which calls
 * decode_data_and_parity (erasure.rs:917) per block and writes the healed
 * shards through BitrotWriter (bitrot.rs:139-247), over stripes whose shard
 * lengths, sets of present shards and rot all differ: every block, full or
 * short, of every object on a replaced disk in one call.  The contract is
 * rsg_heal_records_dev's, applied per stripe.
 * files: k+m record arenas as in rsg_decode_mixed_dev (a NULL arena means
 * shard i is absent for every stripe, whatever `present` says); a source
 * record of stripe s (h_desc[s], rsg_record_desc, a host array the call does
 * not keep) is at files[i] + rec_off.  targets: k+m pointers; targets[i] !=
 * NULL marks shard i, data or parity, as a heal target for every stripe of the
 * call: its record [HH256S][shard_len bytes] of stripe s is written at
 * targets[i] + out_off.  A target shard is never read: files[i] and bit i of
 * `present` are ignored for it.  shard_len == 0 touches no body; the target
 * record is the bare digest of the empty message.
 * Every record used is hashed and compared with its header first; a
 * mismatching record counts as absent for that stripe only, and the stripe is
 * run again under the reduced set, at most k+m rounds, exactly as the GET does.
 * The targets are computed from the first k verified non-target shards in
 * ascending index; every verified source past those is re-derived and compared
 * byte for byte (heal.rs:180-196).
 * h_status[s]: RSG_OK, RSG_ERR_TOO_FEW_SHARDS (fewer than k verified sources;
 * more targets than m gives it for every stripe) or
 * RSG_ERR_INCONSISTENT_SOURCES.  Target records of a failed stripe carry an
 * all-zero 32-byte header (they never verify) and unspecified bodies.
 * algo: HIGHWAY256S or HIGHWAY256S_LEGACY.  Both forms are synchronous.
 * No source byte is written.
 * RSG_ERR_INVALID_ARG with nothing written: no target at all; a NULL pointer;
 * an unknown algo; a `present` bit at or above k+m; record ranges [rec_off,
 * +32+shard_len) or target ranges [out_off, +32+shard_len) not strictly
 * ascending and disjoint in list order (a zero-length stripe's range is its 32
 * header bytes); a range that wraps the address space; a target's span (first
 * range's start to last range's end) meeting the record span of an arena that
 * is read, or another target's span.  m == 0 is RSG_ERR_ZERO_PARITY_SHARDS,
 * k+m > 32 RSG_ERR_UNSUPPORTED, other geometry errors as rsg_check_geometry;
 * n == 0 is RSG_OK.
 * k <= 16 with m <= 4 run one launch per distinct set of readable shards, and
 * again for the stripes in which a record failed its hash; the headers of
 * failed stripes are zeroed in one small launch after the last round.  Other
 * geometries give the same results through rsg_heal_records_dev, stripe by
 * stripe; there a stripe with shard_len == 0 is judged by `present` alone.
 *
 * rsg_heal_mixed_dev: device arenas; runs on `stream` and waits for it.  No
 * byte of a target arena outside the stripes' target ranges is written.
 *
 * rsg_heal_mixed_host: host arenas, page-locked or pageable.  Consecutive
 * stripes are taken into sub-batches that fit RSG_MIXED_STAGE_BYTES of the
 * host-batch staging slots (a larger stripe gets a sub-batch of its own); a
 * sub-batch copies up the record span of every arena that some stripe of it
 * may read and copies back, once per target, its target span (first target
 * range's start to last one's end): the bytes of the span between target
 * ranges are overwritten with unspecified values, as in
 * rsg_encode_mixed_host, so pack the target arenas densely. */
int rsg_heal_mixed_dev(rsg_ctx *ctx, int k, int m, size_t n, const rsg_record_desc *h_desc,
                       const uint8_t *const *d_files, uint8_t *const *d_targets, int algo,
                       int *h_status, void *stream);
int rsg_heal_mixed_host(rsg_ctx *ctx, int k, int m, size_t n, const rsg_record_desc *h_desc,
                        const uint8_t *const *h_files, uint8_t *const *h_targets, int algo,
                        int *h_status);

/* ---- mixed-length batch deep scan: verify n unrelated shard files ----
 * The fourth mixed-length path: bitrot_verify (bitrot.rs:616-655), which
 * LocalDisk::verify_file (local.rs:8101-8146) calls once per part per disk for
 * the scanner's deep mode, verify_object_integrity and the heal's pre-check,
 * over files whose part sizes, shard sizes and lengths all differ: every shard
 * file of every object of a scan cycle in one call.  The contract is
 * rsg_bitrot_verify_dev's, applied per file.
 * arenas: n_arenas (1..32) byte arenas, one per disk in the intended use; a
 * NULL arena may hold only files with file_len == 0.  File f (h_desc[f], a
 * host array the call does not keep): file_len bytes at arenas[arena] + off,
 * records [32-byte digest][shard_size bytes], the last one short when
 * part_size is no multiple of shard_size.
 * h_status[f], decided in this order:
 *   1. RSG_ERR_FILE_SIZE_MISMATCH when want_size !=
 *      bitrot_shard_file_size(part_size, shard_size, algo); none of the file's
 *      bytes is read, its neighbours are unaffected;
 *   2. RSG_ERR_BITROT_MISMATCH at the first bad digest among the records that
 *      lie wholly inside min(file_len, want_size) (the short last record is
 *      one of them when it is complete);
 *   3. RSG_ERR_UNEXPECTED_EOF when file_len < want_size;
 *   4. RSG_ERR_TRAILING_DATA when file_len > want_size;
 *   5. RSG_OK otherwise.
 * algo, per call: HIGHWAY256S / HIGHWAY256S_LEGACY verify the records; NONE
 * checks sizes only and launches nothing; a whole-file algorithm is
 * RSG_ERR_UNSUPPORTED, as in the reference.
 * RSG_ERR_INVALID_ARG with nothing read and h_status untouched: a NULL pointer;
 * an unknown algo; n_arenas outside 1..32; arena >= n_arenas; shard_size == 0
 * with part_size > 0; a non-empty file in a NULL arena; a range [off,
 * +file_len) that wraps the address space; file ranges of one arena that are
 * not ascending and disjoint in list order (files of different arenas may
 * interleave freely, empty files occupy nothing).  More than 2^32-1 complete
 * records in one call (one sub-batch of the host form) is RSG_ERR_UNSUPPORTED.
 * n == 0 is RSG_OK whatever the pointers are (the context, algo and n_arenas
 * are still checked).  Both forms are synchronous.  No byte of any arena is
 * written.
 * The kernel reads whole aligned 8-byte words: up to 7 bytes on either side
 * of a record's body may be read with it, which are bytes of the record's own
 * header or of the 8-byte granule that holds the body's last byte.
 *
 * rsg_bitrot_verify_mixed_dev: device arenas; runs on `stream` and waits for
 * it.  One launch per call whatever n is (every complete record is one entry
 * of a table sorted by length); only a table of more than 2^20 records is cut
 * into several launches.
 *
 * rsg_bitrot_verify_mixed_host: host arenas, page-locked or pageable.
 * Consecutive files are taken into sub-batches whose per-arena spans (per
 * arena touched: its first file's start to its last file's end), record table
 * and flags fit RSG_MIXED_STAGE_BYTES of the host-batch staging slots; a
 * larger file gets a sub-batch of its own.  Only what is read counts and is
 * copied: a file's bytes past want_size, and a file without a complete record
 * (a size mismatch, an empty part, a file cut inside its first record), are
 * not part of a span.  A sub-batch is one H2D copy per
 * touched arena, one table copy, one launch and one flags D2H; sub-batches
 * overlap over the slots.
 *
 * Which call for a uniform part: the files of ONE part (one want_size,
 * part_size and shard_size) go through rsg_bitrot_verify_dev, whose record
 * walk needs no table and runs nearer to memory speed
 * (profiles/r10/mixed_verify/); this call is for batches of files that
 * differ. */
typedef struct rsg_file_desc {
    uint64_t off;        /* the file's bytes at arenas[arena] + off */
    uint64_t file_len;   /* bytes that are there */
    uint64_t want_size;  /* the size the caller expects (verify_file passes the file's own size) */
    uint64_t part_size;  /* Erasure::shard_file_size(part size): body bytes of the file */
    uint32_t shard_size; /* body bytes of a full record */
    uint32_t arena;      /* < n_arenas */
} rsg_file_desc;
int rsg_bitrot_verify_mixed_dev(rsg_ctx *ctx, int algo, int n_arenas, const uint8_t *const *d_arenas,
                                size_t n, const rsg_file_desc *h_desc, int *h_status, void *stream);
int rsg_bitrot_verify_mixed_host(rsg_ctx *ctx, int algo, int n_arenas, const uint8_t *const *h_arenas,
                                 size_t n, const rsg_file_desc *h_desc, int *h_status);

/* ---- gathered block encode: n unrelated blocks in one launch pair ----
 *
 * The reference calls ReedSolomonEncoder::encode once per 1 MiB block
 * (erasure.rs:396-408, from encode.rs:504-530) and BitrotWriter::write hashes
 * each of the k+m shards (bitrot.rs:496-502).  rsg_encode_blocks takes n such
 * blocks, each as the k+m host pointers rsg_encode takes, of any alignment
 * and with its own shard_len (1 .. 0xffffffff), writes every block's parity
 * and, with algo HIGHWAY256S or LEGACY, the (k+m)*32 digest bytes of every
 * block whose `digests` is not NULL (algo NONE ignores the pointers).
 * Synchronous.
 *
 * Validation is all or nothing, before anything is written: a NULL pointer,
 * a shard_len above 0xffffffff, or a parity or digest range that meets any
 * other shard or digest range of the call is RSG_ERR_INVALID_ARG; shard_len 0
 * is RSG_ERR_EMPTY_SHARD; geometry errors are rsg_encode's.  Data ranges may
 * overlap each other.  n == 0 is RSG_OK.
 *
 * For k <= 16, m <= 4 consecutive blocks are taken into sub-batches that fit
 * RSG_BLOCKS_STAGE_BYTES of staging, each one encode launch and, with
 * digests, one hash launch.  Shards in page-locked memory the device can
 * address are read, and their parity written, in place (RSG_ZERO_COPY=0:
 * staged like pageable ones); pageable shards are staged, contiguous runs
 * with one copy.  Exactly the bytes [shard, shard + shard_len) of a parity
 * shard and the (k+m)*32 digest bytes are written.  A block larger than the
 * stage, and every other geometry, goes block by block through rsg_encode's
 * path (and rsg_hash's digest launch): the same bytes.
 *
 * rsg_encode_hashed: rsg_encode plus the digest of every shard (the
 * BitrotWriter prefix), one block per call: the seam a caller uses to skip
 * the writer's own hash.  digests must not be NULL; algo NONE writes none. */
#define RSG_BLOCKS_STAGE_BYTES (32u << 20)
typedef struct rsg_block {
    uint8_t *const *shards; /* k+m host pointers, k data then m parity, as rsg_encode's */
    uint64_t shard_len;
    uint8_t *digests;       /* (k+m)*32 bytes in shard order, or NULL */
} rsg_block;
int rsg_encode_blocks(rsg_ctx *ctx, int k, int m, size_t n, const rsg_block *blocks, int algo);
int rsg_encode_hashed(rsg_ctx *ctx, int k, int m, size_t shard_len, uint8_t *const *shards,
                      uint8_t *digests, int algo);

/* ---- gathered block reconstruct: n degraded blocks, verified, one launch ----
 *
 * The read half of the seam above.  The reference reads a block's shards
 * through BitrotReader::read, which hashes each shard and fails on a mismatch
 * (bitrot.rs:139-244), and hands the Option<Vec<u8>> list to
 * ReedSolomonEncoder::reconstruct_data / reconstruct (erasure.rs:411-428,
 * 897-933; heal.rs:186), once per block.  rsg_reconstruct_blocks takes n such
 * blocks, each as rsg_reconstruct takes one (k+m writable shard_len buffers
 * of any alignment and its own `present` bytes), with its own shard_len
 * (1 .. 0xffffffff), and rebuilds them all in `mode` (one
 * rsg_reconstruct_mode for the call), whatever the mix of loss patterns.
 * Synchronous.
 *
 * Without verification (algo NONE, or a block's digests NULL) a block
 * behaves exactly as rsg_reconstruct does on it.  With algo HIGHWAY256S or
 * LEGACY and digests not NULL, every present shard of the block is hashed
 * first; one whose digest differs from its 32-byte entry is treated as absent
 * (as when BitrotReader::read fails), marked 1 in `bad` if that is given, and
 * rebuilt in place if the mode rebuilds it (a rotten parity shard under
 * RSG_RECONSTRUCT_DATA is only marked).  Entries of absent shards are
 * ignored; the expected digests never leave the host.  The survivors are the
 * first k usable shards in ascending order.
 *
 * status[i]: RSG_OK, or RSG_ERR_TOO_FEW_SHARDS when fewer than k shards of
 * block i are usable after verification: none of that block's shard buffers
 * is written, its `bad` is still filled, other blocks are unaffected.  The
 * call returns RSG_OK when it ran to the end.  `bad`, where given, and status
 * are always filled (zeros for a block that is not verified).
 *
 * Validation is all or nothing, before anything is written.
 * RSG_ERR_INVALID_ARG: a NULL block list, shard list, shard pointer or
 * `present`; shard_len above 0xffffffff; mode or algo out of range; status
 * NULL while any block is verified; a shard or `bad` range that meets any
 * other shard, `bad` or digest range of the call (digest ranges may meet each
 * other).  shard_len 0 is RSG_ERR_EMPTY_SHARD; a block with fewer than k
 * bytes set in `present` is RSG_ERR_TOO_FEW_SHARDS for the call; geometry
 * errors are rsg_reconstruct's.  n == 0 is RSG_OK; m == 0 is RSG_OK with
 * `bad` and status zeroed and nothing else written.
 *
 * For k <= 16, m <= 4 consecutive blocks are taken into sub-batches that fit
 * RSG_BLOCKS_STAGE_BYTES of staging.  Without verification a sub-batch is one
 * launch: shards in page-locked memory the device can address are read, and
 * rebuilt, in place (RSG_ZERO_COPY=0: staged like pageable ones); pageable
 * survivors are staged (only the k survivors, contiguous runs with one copy)
 * and pageable targets copied back.  With verification every present shard
 * is staged and crosses the link once; one hash launch, the digests back,
 * then the one reconstruct launch.  Exactly the bytes
 * [shard, shard + shard_len) of a rebuilt shard are written.  A block larger
 * than the stage, and every other geometry, goes block by block through
 * rsg_hash and rsg_reconstruct: the same bytes and outcomes. */
typedef struct rsg_rblock {
    uint8_t *const *shards; /* k+m host pointers, every one a writable shard_len buffer (as rsg_reconstruct) */
    uint64_t shard_len;     /* 1 .. 0xffffffff */
    const uint8_t *present; /* k+m bytes, != 0: the shard holds what was read */
    const uint8_t *digests; /* expected (k+m)*32 bytes in shard order, or NULL; absent shards' entries ignored */
    uint8_t *bad;           /* k+m bytes out or NULL: 1 where a present shard's digest did not match, else 0 */
} rsg_rblock;
int rsg_reconstruct_blocks(rsg_ctx *ctx, int k, int m, size_t n, const rsg_rblock *blocks,
                           int mode, int algo, int *status /* n, may be NULL when algo is NONE */);

/* Page-lock / release host memory for DMA (hipHostRegister). */
int rsg_pin(void *ptr, size_t bytes);
int rsg_unpin(void *ptr);

#ifdef __cplusplus
}
#endif
#endif /* RSGPU_H */
