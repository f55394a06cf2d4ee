/*
 * fec_hip.h — batch GF(2^8) erasure-coding API of libfec_hip.so (new; the reference has
 * no equivalent).  These are the entry points SURVEY.md §8(b) "New entry points" asks
 * for: explicit k and r, 64-bit layout, device-pointer variants on a caller stream,
 * device selection.  Plain C types only.
 *
 * Code: byte-wise GF(2^8), polynomial 0x11D, systematic generator
 * [I_k ; M] with M an r x k Cauchy matrix normalised so that row 0 and column 0 are all
 * ones.  Parity row 0 is therefore the reference XOR repair packet
 * (fec_xor_simd.cpp:411-427) byte for byte.  MDS for k + r <= 256.
 *
 * Layout (contiguous form):
 *   data   : G*k*P bytes, data shard (g,j) at (g*k + j)*P
 *   parity : G*r*P bytes, parity row (g,i) at (g*r + i)*P
 * Erasure mask of a group: bit s set (s < k+r) => shard s lost; s < k is data shard s,
 * s >= k is parity row s-k.  Every decode, recover and batcher call that takes one u64 mask per
 * group (or derives one from an address table) requires k + r <= 64; the wide calls
 * (fec_decode_wide_rs_dev, fec_recover_wide_rs_dev, and from an address table
 * fec_recover_scatter_wide_rs_dev) work with four u64 per group and serve k + r <= 256 with
 * min(k, r) <= 32.
 *
 * Decode rule: erased data shards are rebuilt in place in `data` from every surviving
 * data shard plus the lowest-indexed surviving parity rows (as many as there are erased
 * data shards).  A single lost data shard with parity row 0 alive is therefore the
 * reference XOR recovery (decoder.go:255-287).  Groups with more erased data shards than
 * surviving parity rows are left untouched and reported unrecoverable.
 */
#ifndef FEC_HIP_H
#define FEC_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "fec_xor_simd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Return codes.  -1 keeps the reference's meaning (NULL argument, fec_xor_simd.cpp:564). */
#define FEC_OK 0
#define FEC_ERR_NULL (-1)      /* a required pointer is NULL                      */
#define FEC_ERR_HIP (-2)       /* the HIP runtime reported an error               */
#define FEC_ERR_RANGE (-3)     /* k, r, packet size or group count unsupported     */
#define FEC_ERR_NODEV (-4)     /* no usable GPU                                   */
#define FEC_ERR_NOMEM (-5)     /* device or pinned allocation failed              */
#define FEC_ERR_AGAIN (-6)     /* fec_batcher_wait: not ready within the timeout   */
#define FEC_ERR_UNRECOVERABLE (-7) /* fec_batcher_wait_rebuilt: too many shards lost */

/* Number of visible HIP devices (0 when none or the runtime is unusable). */
int fec_hip_device_count(void);

/* Message of the calling thread's last failing call ("" if none; entry points taking a
 * context clear it on entry). */
const char* fec_hip_last_error(void);

/* Message of the last failing call on `ctx`, whichever thread made it (Go: a goroutine may
 * move to another OS thread between the failing call and the read, so the thread-local
 * text above may be empty or another call's).  Copies at most buflen-1 bytes plus a NUL
 * into buf (when buf != NULL and buflen > 0) and returns the message's full length; 0 for
 * a NULL context or no failure yet.  Replaces the cgo wrapper's code-only message
 * (fec_cgo.go:147-149). */
size_t fec_ctx_last_error(FECEncoderCtx* ctx, char* buf, size_t buflen);

/* fec_encoder_new on an explicit device ordinal (shards of a multi-GPU job). */
FECEncoderCtx* fec_encoder_new_device(double redundancy, uint32_t max_groups, int device);

/* Device ordinal a context is bound to, or -1 for NULL. */
int fec_encoder_device(const FECEncoderCtx* ctx);

/* Library build identifier, for logs: "libfec_hip <version> gfx950 src=<sha256 of the sources it was
 * built from>" (quic-test_amd/csrc/src_hash.py defines the hash; tests/test_abi.py checks it). */
const char* fec_hip_version(void);

/* The r x k parity matrix M, row-major (r*k bytes).  0, or FEC_ERR_RANGE. */
int fec_parity_matrix(uint32_t k, uint32_t r, uint8_t* out);

/* ---- synchronous API: host or device pointers (auto-detected) ----
 * offsets: NULL for the contiguous layout, else k*num_groups u64 byte offsets into
 * `data` (data shard (g,j) at data + offsets[g*k + j]); parity is always contiguous. */
int fec_encode_batch_rs(FECEncoderCtx* ctx, const uint8_t* data, const uint64_t* offsets,
                        uint64_t num_groups, uint32_t k, uint32_t r, uint32_t packet_size,
                        uint8_t* parity_out);

/* erasure_masks: one u64 per group.  Bit j < k set: data shard j is lost.  Bit k + i set (i < r):
 * parity row i is lost.  Bits at and above k + r are ignored: a caller need not clear them.  The
 * masks are only read.
 * status_out (nullable): one byte per group, 0 = recovered or nothing lost,
 * 1 = unrecoverable.  unrecoverable_out (nullable): count of status 1. */
int fec_decode_batch_rs(FECEncoderCtx* ctx, uint8_t* data, const uint8_t* parity,
                        const uint64_t* erasure_masks, uint64_t num_groups, uint32_t k,
                        uint32_t r, uint32_t packet_size, uint8_t* status_out,
                        uint64_t* unrecoverable_out);

/* ---- device-resident API: device pointers only, asynchronous on `stream`
 * (a hipStream_t; NULL = the context's own stream).  Contiguous layout only.
 * A call returns once its kernels are queued; they read the context's tables and workspaces
 * until they have run.  fec_encoder_free waits for the context's calls queued on caller
 * streams (it drains the device when any call took one) and on its own stream before it
 * frees them, so a context may be freed with work in flight; the caller's own buffers must
 * outlive that work as usual. ---- */
int fec_encode_batch_rs_dev(FECEncoderCtx* ctx, const uint8_t* d_data, uint64_t num_groups,
                            uint32_t k, uint32_t r, uint32_t packet_size, uint8_t* d_parity,
                            void* stream);

/* d_erasure_masks: the bits as fec_decode_batch_rs reads them, bits at and above k + r ignored.
 * d_status (nullable) as status_out above, written on the device. */
int fec_decode_batch_rs_dev(FECEncoderCtx* ctx, uint8_t* d_data, const uint8_t* d_parity,
                            const uint64_t* d_erasure_masks, uint64_t num_groups, uint32_t k,
                            uint32_t r, uint32_t packet_size, uint8_t* d_status, void* stream);

/* Recover: decode without touching d_data.  The rebuilt data shards of group g go to
 * d_rebuilt + (g*r + m)*P, m = 0..e-1 over the group's lost data shards in ascending shard
 * order -- the reference decoder hands recovered packets back as separate buffers
 * (decoder.go:16-22 Recovered{PacketID, Data}, the list built at :195-207), and a device-resident receiver
 * consumes them the same way.  d_rebuilt holds num_groups*r*P bytes; slots m >= e of a
 * group, and all slots of an unrecoverable group, are left unwritten.  Writing the rebuilt
 * packets back to back (the write pattern of encode's parity rows) instead of scattered
 * among the data shards measured 2.32 vs 2.47 ms at k=10 r=3, 2 erasures, 1M groups.
 * d_erasure_masks: the bits as fec_decode_batch_rs reads them. */
int fec_recover_batch_rs_dev(FECEncoderCtx* ctx, const uint8_t* d_data, const uint8_t* d_parity,
                             const uint64_t* d_erasure_masks, uint64_t num_groups, uint32_t k, uint32_t r,
                             uint32_t packet_size, uint8_t* d_rebuilt, uint8_t* d_status, void* stream);

/* ---- wide shapes: decode what encode accepts, k + r <= 256 ----
 * fec_decode_batch_rs_dev and fec_recover_batch_rs_dev for groups of more than 64 shards: the same
 * layouts, status bytes and stream behaviour, with an erasure mask of FEC_WIDE_MASK_WORDS u64 per
 * group.
 *   - Masks: group g's words are d_erasure_masks[4g .. 4g + 3]; shard s is bit s & 63 of word
 *     s >> 6.  The rule is the one-word rule: data shards are bits 0..k-1, parity rows are bits
 *     k..k+r-1; bits at and above k + r are ignored, in the partial word and in the whole words
 *     above it; a group is unrecoverable when fewer parity rows survive than data shards are lost;
 *     the survivors read are the surviving data shards and the lowest-indexed surviving parity
 *     rows, as many as data shards are lost.  The masks are only read.
 *   - fec_decode_wide_rs_dev rebuilds in place in d_data.  fec_recover_wide_rs_dev only reads
 *     d_data and writes the m-th lost data shard of group g (ascending) to d_rebuilt + (g*r + m)*P;
 *     slots m >= e of a group and every slot of an unrecoverable group are left unwritten.
 *     d_status (nullable): one byte per group, every one written, 0 or 1 as above.
 *   - Asynchronous on `stream` (NULL = the context's own); fec_encoder_free drains them like every
 *     _dev call.  The recovery records are built on the device per call, in the caller stream's
 *     workspace (at most 64 MiB of records at a time; larger calls are walked in chunks), whatever
 *     fec_decode_plan_mode says: there is no codebook and no host synchronise for a wide shape.
 *   - Served: k >= 1, r >= 1, k + r <= 256, min(k, r) <= 32, packet_size >= 16,
 *     0 < num_groups < 2^32.  Shapes with k + r <= 64 are served too, and give byte for byte what
 *     the one-word calls give, whatever words 1..3 hold.
 *   - Why min(k, r) <= 32: a group with e lost data shards needs the inverse of an e x e matrix,
 *     e <= min(k, r), which one wave computes in its slice of a compute unit's local memory.  At
 *     e = 32 the slice is about 9.5 KiB; at e = 128 it would be 48 KiB per wave, 192 KiB for a
 *     workgroup of four waves, and a compute unit has 160 KiB.
 * Refusals launch nothing and write nothing (fec_hip_last_error names the case): FEC_ERR_NULL for a
 * NULL context or required pointer; FEC_ERR_RANGE for k = 0, r = 0, k + r > 256, min(k, r) > 32,
 * packet_size < 16, num_groups == 0 or >= 2^32.  There are no host-pointer or batcher forms of
 * the wide calls; the packed form is fec_recover_packed_wide_rs_dev, the wide address-table calls
 * are fec_recover_scatter_wide_rs_dev and fec_encode_scatter_wide_rs_dev, below. */
#define FEC_WIDE_MASK_WORDS 4
int fec_decode_wide_rs_dev(FECEncoderCtx* ctx, uint8_t* d_data, const uint8_t* d_parity,
                           const uint64_t* d_erasure_masks, uint64_t num_groups, uint32_t k, uint32_t r,
                           uint32_t packet_size, uint8_t* d_status, void* stream);
int fec_recover_wide_rs_dev(FECEncoderCtx* ctx, const uint8_t* d_data, const uint8_t* d_parity,
                            const uint64_t* d_erasure_masks, uint64_t num_groups, uint32_t k, uint32_t r,
                            uint32_t packet_size, uint8_t* d_rebuilt, uint8_t* d_status, void* stream);

/* Build (and upload) the decode codebook for (k, r) ahead of the first decode.  The
 * codebook holds the recovery tables of every recoverable erasure pattern; its size is
 * returned in *bytes_out (nullable).  When it would exceed the 2 GiB cap (e.g. k=16 r=16)
 * decode instead builds records for the patterns present in each call ("sparse plan":
 * masks are read back to the host and the call completes synchronously); *bytes_out is
 * then 0.  FEC_ERR_RANGE if k + r > 64.  With the context in FEC_PLAN_DEVICE
 * (fec_decode_plan_mode) such a shape still reports 0 bytes; the call then uploads the parity
 * matrix the device builds records from, so that the first decode allocates nothing but its
 * workspace. */
int fec_decode_prepare(FECEncoderCtx* ctx, uint32_t k, uint32_t r, uint64_t* bytes_out);

/* The same recovery with the rebuilt packets of all groups back to back ("packed"), the
 * shape of decoder.go's Recovered list (:29-34): group g's m-th lost data shard (ascending
 * shard id) at d_rebuilt + (d_row_start[g] + m) * packet_size, where d_row_start[g] (u32, one
 * per group, written by the call) is the number of rows rebuilt for groups 0..g-1;
 * unrecoverable groups and groups without lost data rebuild none.  *d_total (nullable, device)
 * = all rows.  d_rebuilt holds at most num_groups * r rows.  No gaps between groups' rows:
 * the stores stream like encode's parity (C5-style sparse loss: 15% faster than the slot
 * layout in the probe, profiles/r02_probe_recover_write_layout.txt).  Mask-addressed shapes
 * only (k + r with an inline-classify form, r <= 3: k=10 with r = 1, 2, 3 and k=4 r=2), at
 * 256 < P <= 2047 (2048 has no inline-classify form); k=10 r=2, which has no tiled form for
 * short packets, also at 16 <= P <= 256.  Every other shape or size returns FEC_ERR_RANGE with
 * nothing written.  Asynchronous on `stream` like the call above.  d_masks: the bits as
 * fec_decode_batch_rs reads them. */
int fec_recover_batch_rs_dev_packed(FECEncoderCtx* ctx, const uint8_t* d_data, const uint8_t* d_parity,
                                    const uint64_t* d_masks, uint64_t num_groups, uint32_t k, uint32_t r,
                                    uint32_t packet_size, uint8_t* d_rebuilt, uint32_t* d_row_start,
                                    uint64_t* d_total, uint8_t* d_status, void* stream);

/* ---- packed recover for every shape, one-word masks ----
 * The packed layout of fec_recover_batch_rs_dev_packed for every shape fec_recover_batch_rs_dev
 * recovers on the device.  Use this call unless the caller depends on the old call's refusals.
 *   - Layouts: d_data and d_parity are in the contiguous layouts and are only read.  d_masks holds
 *     one u64 per group and is only read.
 *   - Decode rule: the mask rule, the choice of survivors, the status bytes and "bits at and above
 *     k + r are ignored" are those of fec_recover_batch_rs_dev: bit j < k means data shard j is
 *     lost, bit k + i parity row i; a group is unrecoverable when fewer parity rows survive than
 *     data shards are lost; the survivors read are the surviving data shards and the
 *     lowest-indexed surviving parity rows, as many as data shards are lost.
 *   - Rows per group: group g rebuilds rows_g rows: the number of its lost data shards when it is
 *     recoverable, 0 when nothing is lost or the group is unrecoverable.
 *   - d_row_start: d_row_start[g] is the sum of rows_h for h < g, a u32.  The call writes it for
 *     every group.
 *   - Row placement: the m-th lost data shard of group g, in ascending order, goes to
 *     d_rebuilt + (d_row_start[g] + m) * packet_size as a full packet_size-byte row.  No byte at
 *     or past total * packet_size is written.
 *   - d_total (nullable, device memory, u64): *d_total is the number of all rows.
 *   - d_status (nullable): one byte per group, every byte written; 0 = recovered or nothing lost,
 *     1 = unrecoverable.
 *   - No overlap: d_rebuilt must not overlap any input.
 *   - Stream behaviour: asynchronous on `stream` (NULL = the context's own stream); drained by
 *     fec_encoder_free like every _dev call.  There is no host synchronise and no readback.
 *   - Stream workspace: everything the call keeps in the caller stream's workspace -- the
 *     prefix's block sums, the record offsets, and the record arena where records are built on
 *     the device -- comes from ONE workspace request per call, because a second, larger request
 *     may synchronise and reallocate, which would leave the first pointer stale.
 *   - Served: k >= 1, r >= 1, k + r <= 64, packet_size >= 16, num_groups < 2^32.
 *     num_groups == 0 is served: nothing is launched, and *d_total = 0 when d_total is given.
 *   - Records: a shape with a dense codebook takes its records from the codebook, as
 *     fec_recover_gather_rs_dev does.  A shape past the 2 GiB cap (16+16, 32+8, 60+4) is served
 *     only on a context in FEC_PLAN_DEVICE (fec_decode_plan_mode): its records are built on the
 *     device per chunk of the arena, and the row starts stay global across chunks.  On a context
 *     in FEC_PLAN_CODEBOOK such a shape is refused with FEC_ERR_RANGE: this call never reads masks
 *     back.
 *   - A call fec_recover_batch_rs_dev_packed serves is handed to it: the output is byte for byte
 *     the old call's.  Every other call runs a row prefix, a classify and a record-addressed
 *     kernel that places a group's rows by d_row_start[g].
 *   - Zero pivot: the code's matrix is MDS, so a record build cannot meet one; if it did, the
 *     group would get status 1 and its reserved rows (counted in d_row_start and *d_total) would
 *     stay unwritten, as its slots do in fec_recover_batch_rs_dev.
 *   - Refusals launch nothing and write nothing, d_row_start and *d_total included;
 *     fec_hip_last_error names the case.  FEC_ERR_NULL for a NULL context or a NULL d_data,
 *     d_parity, d_masks, d_rebuilt or d_row_start (the message names the argument).
 *     FEC_ERR_RANGE for k = 0, r = 0, k + r > 64, packet_size < 16, num_groups >= 2^32,
 *     num_groups * min(k, r) >= 2^32 (row indices are 32-bit), and a shape past the codebook cap
 *     on a context in FEC_PLAN_CODEBOOK. */
int fec_recover_packed_rs_dev(FECEncoderCtx* ctx, const uint8_t* d_data, const uint8_t* d_parity,
                              const uint64_t* d_masks, uint64_t num_groups, uint32_t k, uint32_t r,
                              uint32_t packet_size, uint8_t* d_rebuilt, uint32_t* d_row_start,
                              uint64_t* d_total, uint8_t* d_status, void* stream);

/* ---- packed recover for every shape, four-word masks ----
 * The packed layout for what fec_recover_wide_rs_dev recovers: k + r <= 256.
 *   - Layouts: d_data and d_parity are in the contiguous layouts and are only read.
 *     d_erasure_masks holds FEC_WIDE_MASK_WORDS u64 per group, shard s at bit s & 63 of word
 *     s >> 6, and is only read.
 *   - Decode rule: the mask rule, the choice of survivors, the status bytes and "bits at and above
 *     k + r are ignored" (in the partial word and in the whole words above it) are those of
 *     fec_recover_wide_rs_dev: bit j < k means data shard j is lost, bit k + i parity row i; a
 *     group is unrecoverable when fewer parity rows survive than data shards are lost; the
 *     survivors read are the surviving data shards and the lowest-indexed surviving parity rows,
 *     as many as data shards are lost.
 *   - Rows per group: group g rebuilds rows_g rows: the number of its lost data shards when it is
 *     recoverable, 0 when nothing is lost or the group is unrecoverable.
 *   - d_row_start: d_row_start[g] is the sum of rows_h for h < g, a u32.  The call writes it for
 *     every group.
 *   - Row placement: the m-th lost data shard of group g, in ascending order, goes to
 *     d_rebuilt + (d_row_start[g] + m) * packet_size as a full packet_size-byte row.  No byte at
 *     or past total * packet_size is written.
 *   - d_total (nullable, device memory, u64): *d_total is the number of all rows.
 *   - d_status (nullable): one byte per group, every byte written; 0 = recovered or nothing lost,
 *     1 = unrecoverable.
 *   - No overlap: d_rebuilt must not overlap any input.
 *   - Stream behaviour: asynchronous on `stream` (NULL = the context's own stream); drained by
 *     fec_encoder_free like every _dev call.  There is no host synchronise and no readback.
 *   - Stream workspace: everything the call keeps in the caller stream's workspace -- the
 *     prefix's block sums, the record offsets, and the record arena -- comes from ONE workspace
 *     request per call, because a second, larger request may synchronise and reallocate, which
 *     would leave the first pointer stale.
 *   - Served: what fec_recover_wide_rs_dev serves on the same context: k >= 1, r >= 1,
 *     k + r <= 256, min(k, r) <= 32 by default and every min(k, r) after
 *     fec_wide_rows_mode(ctx, FEC_WIDE_ROWS_ALL); packet_size >= 16; 0 < num_groups < 2^32.
 *   - Records are always built on the device, whatever fec_decode_plan_mode says.
 *   - Shapes with k + r <= 64 are served and give byte for byte what fec_recover_packed_rs_dev
 *     gives for the same masks in word 0, whatever words 1..3 hold.
 *   - Zero pivot: the code's matrix is MDS, so a record build cannot meet one; if it did, the
 *     group would get status 1 and its reserved rows (counted in d_row_start and *d_total) would
 *     stay unwritten, as its slots do in fec_recover_wide_rs_dev.
 *   - Refusals launch nothing and write nothing, d_row_start and *d_total included;
 *     fec_hip_last_error names the case.  FEC_ERR_NULL for a NULL context or a NULL d_data,
 *     d_parity, d_erasure_masks, d_rebuilt or d_row_start (the message names the argument).
 *     FEC_ERR_RANGE for what fec_recover_wide_rs_dev refuses, with its texts (k = 0, r = 0,
 *     k + r > 256, min(k, r) > 32 in FEC_WIDE_ROWS_CAPPED, packet_size < 16, num_groups == 0 or
 *     >= 2^32), and for num_groups * min(k, r) >= 2^32, because row indices are 32-bit. */
int fec_recover_packed_wide_rs_dev(FECEncoderCtx* ctx, const uint8_t* d_data, const uint8_t* d_parity,
                                   const uint64_t* d_erasure_masks /* FEC_WIDE_MASK_WORDS per group */,
                                   uint64_t num_groups, uint32_t k, uint32_t r, uint32_t packet_size,
                                   uint8_t* d_rebuilt, uint32_t* d_row_start, uint64_t* d_total,
                                   uint8_t* d_status, void* stream);

/* ---- address tables: shards and packets wherever they are in device memory ----
 * A receiver that keeps its packets in device memory, in arrival order in a ring or an arena,
 * hands over a table of their addresses instead of copying them into the contiguous layout.
 *   - A shard may have any byte alignment; its packet_size bytes must be readable.
 *   - Shards may lie in any number of allocations on the context's device.
 *   - The output buffer must not overlap any shard.
 *   - The decode rule is unchanged: every surviving data shard plus the lowest-indexed surviving
 *     parity rows.  A lost shard's entry, and a parity row the rule does not use, is never read.
 *   - Both calls are asynchronous on `stream` like the other _dev calls, and fec_encoder_free
 *     drains them the same way.
 * Refused with nothing launched or written (fec_hip_last_error says which case applied):
 * FEC_ERR_NULL for a NULL context or required pointer; FEC_ERR_RANGE for k + r > 64, for
 * packet_size < 16 (QUIC packets are never that short), for num_groups == 0 or >= 2^32, and, for
 * the recover, for a shape whose decode codebook exceeds the 2 GiB cap (fec_decode_prepare: the
 * sparse plan reads masks back on the host, which this call does not do) unless the context is
 * in FEC_PLAN_DEVICE (fec_decode_plan_mode): the records are then built on the device and the
 * recover serves the shape like any other. */

/* Recover from shards wherever they are.  d_shard_addrs: num_groups*(k+r) absolute device
 * addresses (u64), group g's shard s at [g*(k+r) + s], data shards 0..k-1 then parity rows
 * 0..r-1; 0 = lost (the convention of fec_batcher_submit_shards).  Output and status exactly as
 * fec_recover_batch_rs_dev (slots (g*r + m)*P, slots m >= e and unrecoverable groups unwritten).
 * d_masks_out (nullable): the erasure mask derived for each group. */
int fec_recover_gather_rs_dev(FECEncoderCtx* ctx, const uint64_t* d_shard_addrs, uint64_t num_groups,
                              uint32_t k, uint32_t r, uint32_t packet_size, uint8_t* d_rebuilt,
                              uint8_t* d_status, uint64_t* d_masks_out, void* stream);

/* Encode k packets per group from absolute device addresses (num_groups*k of them, all valid);
 * parity contiguous as in fec_encode_batch_rs_dev. */
int fec_encode_gather_rs_dev(FECEncoderCtx* ctx, const uint64_t* d_packet_addrs, uint64_t num_groups,
                             uint32_t k, uint32_t r, uint32_t packet_size, uint8_t* d_parity, void* stream);

/* ---- address tables with a length per entry: variable-length packets, partial groups ----
 * The two calls above with a second table, u32 in device memory and indexed exactly like the
 * address table: entry (g, s) is the number of readable bytes at that shard's address.
 *   - packet_size (P) is the symbol size and the row pitch of the output.  A length above P is
 *     clamped to P.  Shard (g, s) is the bytes [0, min(len, P)) at its address followed by zeros
 *     up to P, as the reference's decoder pads a symbol and its encoder XORs only the bytes a
 *     packet has.
 *   - No byte at or past address + len is ever read: a packet may be the last thing in its
 *     allocation.  A present shard of length 0 is all zero and its address is never dereferenced.
 *   - Recover: address 0 is still the only loss marker; the length of a lost entry is ignored.
 *     The table carries the parity shards with their lengths too, because a repair packet on the
 *     wire holds only its group's symbol length.
 *   - Encode: address 0 means the packet is absent (a flush of a partial group) and counts as all
 *     zero; a group with every packet absent gets all-zero rows.  The parity rows are written as
 *     full P-byte rows.
 *   - Output layout as in the fixed-length calls (rebuilt rows at (g*r + m)*P, slots m >= e and
 *     every slot of an unrecoverable group unwritten; parity at (g*r + i)*P).  Every written row
 *     is a full P bytes, with zeros where every contributing shard had ended.
 *   - d_symbol_len_out (nullable, u32 per group): written for every group when given; the largest
 *     min(len, P) over the group's present entries, 0 when none is present -- the decoder's symbol
 *     length, and on the encode side the length of the repair payload.
 * Refused like the fixed-length calls, with nothing launched or written; a NULL length table is
 * FEC_ERR_NULL and the message names it.  Asynchronous on `stream`, drained by fec_encoder_free;
 * the recover's record offsets live in the caller stream's workspace, no new per-context state. */
int fec_recover_gather_var_rs_dev(FECEncoderCtx* ctx, const uint64_t* d_shard_addrs,
                                  const uint32_t* d_shard_lens, uint64_t num_groups, uint32_t k, uint32_t r,
                                  uint32_t packet_size, uint8_t* d_rebuilt, uint8_t* d_status,
                                  uint64_t* d_masks_out, uint32_t* d_symbol_len_out, void* stream);

int fec_encode_gather_var_rs_dev(FECEncoderCtx* ctx, const uint64_t* d_packet_addrs,
                                 const uint32_t* d_packet_lens, uint64_t num_groups, uint32_t k, uint32_t r,
                                 uint32_t packet_size, uint8_t* d_parity, uint32_t* d_symbol_len_out, void* stream);

/* ---- scatter recover: rebuilt packets written to a table of destinations ----
 * The gather recovers above write every rebuilt packet into a library-shaped buffer as a full
 * P-byte row.  This call writes each rebuilt packet where the caller says, and only the bytes the
 * packet has (the reference's decoder returns each recovered packet as a buffer of its symbol
 * length).
 *   - Inputs: d_shard_addrs and d_shard_lens exactly as fec_recover_gather_var_rs_dev (clamping
 *     at P, zero padding, no byte at or past address + len read, a present shard of length 0 never
 *     dereferenced).  d_shard_lens == NULL: every present shard has P bytes, the inputs of
 *     fec_recover_gather_rs_dev.
 *   - d_symbol_len_out (nullable, u32 per group), written for every group: L_g, the largest
 *     min(len, P) over the group's present entries (P without a length table), 0 when none is
 *     present.
 *   - d_dest_addrs: num_groups*k absolute device addresses (u64), entry [g*k + j] for data shard j
 *     of group g, any byte alignment.  If the call rebuilds that shard it writes exactly L_g bytes
 *     there (the rebuilt bytes past L_g are zero by construction): no byte before the address or
 *     at or past address + L_g is written, so a rebuilt packet may sit between two live ones.
 *     L_g == 0 writes nothing and dereferences nothing.
 *   - An entry is read only for a data shard that is lost in a recoverable group; the entries of
 *     present shards, of groups with nothing lost and of unrecoverable groups are ignored.  An
 *     entry of 0 for a shard the call would rebuild means "not wanted": that row is not stored,
 *     the group's other rows are, and the status stays 0.
 *   - Decode rule, d_status and d_masks_out as in the gather recovers; a lost shard's source entry
 *     and a parity row the rule does not use are never read.
 *   - A destination range must not overlap any shard the call reads, in any group, nor another
 *     destination range.  Destinations that are the holes the receiver reserved for the lost
 *     packets in its arena give in-place gathered decode; destinations back to back give packed
 *     output; destinations at d_rebuilt + (g*r + m)*P give the slot layout of the gather recovers.
 * Refused like the gather calls, with nothing launched or written; a NULL context, address table
 * or destination table is FEC_ERR_NULL and the message names it.  Asynchronous on `stream`,
 * drained by fec_encoder_free; record offsets (and L_g, when d_symbol_len_out is NULL) live in the
 * caller stream's workspace, no new per-context state. */
int fec_recover_scatter_rs_dev(FECEncoderCtx* ctx, const uint64_t* d_shard_addrs,
                               const uint32_t* d_shard_lens, const uint64_t* d_dest_addrs,
                               uint64_t num_groups, uint32_t k, uint32_t r, uint32_t packet_size,
                               uint8_t* d_status, uint64_t* d_masks_out, uint32_t* d_symbol_len_out,
                               void* stream);

/* ---- wide scatter recover: k + r <= 256 from scattered shards ----
 * fec_recover_scatter_rs_dev for groups of up to 256 shards: shards taken where they lie in device
 * memory through a table of addresses, each rebuilt packet written where a table of destinations
 * says, cut at the group's symbol length.  One call: destinations at d_rebuilt + (g*r + m)*P with a
 * NULL length table give the slot layout of fec_recover_wide_rs_dev, without its contiguous,
 * zero-padded copy of every shard and without a mask built by the caller.
 *   - Served: k >= 1, r >= 1, k + r <= 256, min(k, r) <= 32 (why: see the wide calls above),
 *     packet_size >= 16, 0 < num_groups < 2^32.  Shapes with k + r <= 64 are served too and give
 *     byte for byte what fec_recover_scatter_rs_dev gives for the same tables.  The cap on
 *     min(k, r) is this side's alone: fec_encode_scatter_wide_rs_dev, below, builds no record and
 *     has none, so it produces parity for shapes (33 + 33, 128 + 128) that no wide call recovers
 *     unless the context is in FEC_WIDE_ROWS_ALL (fec_wide_rows_mode, below).
 *   - d_shard_addrs: num_groups*(k+r) absolute device addresses (u64), entry [g*(k+r) + s] for shard
 *     s of group g (s < k: data shard s; else parity row s - k), any byte alignment.  Address 0 is
 *     the only loss marker.  The table is only read.
 *   - d_shard_lens (nullable): num_groups*(k+r) u32, indexed alike: the readable bytes of each
 *     present shard.  A lost entry's length is ignored.  A length above P is clamped to P.  Shard
 *     (g, s) stands for the P-byte symbol whose bytes [0, min(len, P)) are the bytes at its address
 *     and whose other bytes are zero.  No byte at or past address + len is read, and a present shard
 *     of length 0 is never dereferenced.  NULL: every present shard has P bytes.
 *   - Decode rule: the one-word rule over the mask the zero addresses imply.  A group is
 *     unrecoverable when fewer parity rows are present than data shards are lost.  The survivors
 *     read are the present data shards and the lowest-indexed present parity rows, as many as data
 *     shards are lost.  A lost shard's source entry is never dereferenced (it is 0), and neither is
 *     a present parity row the rule does not use.
 *   - d_symbol_len_out (nullable, u32 per group), written for every group when given: L_g, the
 *     largest min(len, P) over the group's present entries (P without a length table), 0 when none
 *     is present.
 *   - d_dest_addrs: num_groups*k absolute device addresses (u64), entry [g*k + j] for data shard j
 *     of group g, any byte alignment.  An entry is read only for a data shard the call rebuilds (a
 *     lost data shard of a recoverable group); every other entry is ignored.  An entry of 0 means
 *     "not wanted": that row is not stored, the group's other rows are, and the status stays 0.
 *     At any other entry the call writes exactly L_g bytes: nothing before the address and nothing
 *     at or past address + L_g.  L_g == 0 writes nothing and dereferences nothing.  Unrecoverable
 *     groups write nothing.
 *   - d_status (nullable): one byte per group, every one written when given: 0 = rebuilt or nothing
 *     lost, 1 = unrecoverable.
 *   - d_masks_out (nullable): FEC_WIDE_MASK_WORDS u64 per group, group g's words at
 *     d_masks_out[4g .. 4g + 3], the erasure mask derived from the addresses: shard s is bit s & 63
 *     of word s >> 6, and every bit at and above k + r is zero.
 *   - A destination range must not overlap any shard the call reads, in any group, nor another
 *     destination range.
 *   - Asynchronous on `stream` (NULL = the context's own), drained by fec_encoder_free; no host
 *     synchronise and no readback.  The recovery records are always built on the device per call,
 *     in the caller stream's workspace (record offsets, the masks when d_masks_out is NULL, L_g when
 *     there is a length table and d_symbol_len_out is NULL, and at most 64 MiB of records at a time;
 *     larger calls are walked in chunks), whatever fec_decode_plan_mode says.  No per-context state
 *     beyond the shape's parity matrix on the device, which the wide calls keep too.
 * Refusals launch nothing and write nothing (fec_hip_last_error names the case): FEC_ERR_NULL for a
 * NULL context, address table or destination table, the message naming the argument;
 * FEC_ERR_RANGE, with the texts of the wide calls, for k = 0, r = 0, k + r > 256, min(k, r) > 32,
 * packet_size < 16, num_groups == 0 or >= 2^32. */
int fec_recover_scatter_wide_rs_dev(FECEncoderCtx* ctx, const uint64_t* d_shard_addrs,
                                    const uint32_t* d_shard_lens, const uint64_t* d_dest_addrs,
                                    uint64_t num_groups, uint32_t k, uint32_t r, uint32_t packet_size,
                                    uint8_t* d_status, uint64_t* d_masks_out, uint32_t* d_symbol_len_out,
                                    void* stream);

/* ---- scatter encode: parity rows written to a table of destinations ----
 * The gather encodes above write every parity row into a library-shaped buffer as a full P-byte
 * row at (g*r + i)*P.  This call writes each parity row where the caller says, and only the bytes
 * the repair payload has (the reference's repair packet carries the group's symbol length of
 * it), so a sender that keeps its packets in a device arena needs no second pass to move the
 * payloads behind their wire headers.
 *   - Inputs: d_packet_addrs (num_groups*k u64 addresses) and d_packet_lens (u32, indexed alike)
 *     exactly as fec_encode_gather_var_rs_dev: a length above P is clamped to P; a packet is its
 *     bytes [0, min(len, P)) followed by zeros; no byte at or past address + len is read; a
 *     present packet of length 0 is never dereferenced; address 0 means absent (the flush of a
 *     partial group) and counts as all zero.  d_packet_lens == NULL: every present packet has P
 *     bytes, the inputs of fec_encode_gather_rs_dev; address 0 is still "absent".
 *   - d_symbol_len_out (nullable, u32 per group), written for every group: L_g, the largest
 *     min(len, P) over the group's present packets (P without a length table when any packet is
 *     present), 0 when none is present -- the length of the group's repair payloads.
 *   - d_dest_addrs: num_groups*r absolute device addresses (u64), entry [g*r + i] for parity row i
 *     of group g, any byte alignment.  The call writes exactly L_g bytes of the row there (the
 *     row's bytes past L_g are zero by construction): no byte before the address or at or past
 *     address + L_g is written, so a repair payload may sit between a header and the next live
 *     packet.  An entry of 0 means "not wanted": that row is not stored, the group's other rows
 *     are (a sender whose plan is r rows may send fewer for some groups).
 *   - L_g == 0 writes nothing and dereferences nothing.  This differs from the gather encodes,
 *     which write all-zero rows for a group with no packet present.
 *   - Destinations at d_parity + (g*r + i)*P with every length P give the gather encode's output;
 *     destinations back to back give packed repair payloads.
 *   - A destination range must not overlap any packet the call reads, in any group, nor another
 *     destination range.
 * Refused like the gather calls, with nothing launched or written: FEC_ERR_NULL for a NULL
 * context, address table or destination table (the message names it); FEC_ERR_RANGE for
 * k + r > 64, packet_size < 16, num_groups == 0 or >= 2^32.  There is no codebook cap (encode has
 * none).  Asynchronous on `stream`, drained by fec_encoder_free; no new per-context state and no
 * workspace: every lane derives L_g from the k lengths of its own group. */
int fec_encode_scatter_rs_dev(FECEncoderCtx* ctx, const uint64_t* d_packet_addrs,
                              const uint32_t* d_packet_lens, const uint64_t* d_dest_addrs,
                              uint64_t num_groups, uint32_t k, uint32_t r, uint32_t packet_size,
                              uint32_t* d_symbol_len_out, void* stream);

/* ---- wide scatter encode: k + r <= 256 from scattered packets ----
 * fec_encode_scatter_rs_dev for groups of up to 256 shards: packets taken where they lie in device
 * memory through a table of addresses, each parity row written where a table of destinations says,
 * cut at the group's symbol length.  One call: a NULL length table gives the fixed-length form,
 * destinations at d_parity + (g*r + i)*P give the contiguous rows of fec_encode_batch_rs_dev
 * without its contiguous, zero-padded copy of every packet, destinations back to back give packed
 * repair payloads.
 *   - Served: k >= 1, r >= 1, k + r <= 256, packet_size >= 16, 0 < num_groups < 2^32.  There is no
 *     min(k, r) cap: the cap min(k, r) <= 32 of the wide decode, the wide recover and
 *     fec_recover_scatter_wide_rs_dev is the record builder's (the inverse of an e x e matrix in
 *     local memory), and an encode builds no record.  33 + 33, 128 + 128 and 1 + 255 are served
 *     here and refused there.  Shapes with k + r <= 64 are served too and give byte for byte what
 *     fec_encode_scatter_rs_dev gives for the same tables.
 *   - d_packet_addrs: num_groups*k absolute device addresses (u64), entry [g*k + j] for packet j of
 *     group g, any byte alignment.  Address 0 means absent (the flush of a partial group): the
 *     packet counts as all zero and is never dereferenced.  The table is only read.
 *   - d_packet_lens (nullable): num_groups*k u32, indexed alike: the readable bytes of each present
 *     packet.  A length above P is clamped to P.  A packet is its bytes [0, min(len, P)) followed
 *     by zeros up to P.  No byte at or past address + len is read.  A present packet of length 0 is
 *     never dereferenced.  An absent packet's length entry is ignored.  NULL: every present packet
 *     has P bytes; address 0 is still "absent".
 *   - d_symbol_len_out (nullable, u32 per group), written for every group when given: L_g, the
 *     largest min(len, P) over the group's present packets; without a length table P when any
 *     packet is present; 0 when none is present -- the length of the group's repair payloads.
 *   - d_dest_addrs: num_groups*r absolute device addresses (u64), entry [g*r + i] for parity row i
 *     of group g, any byte alignment.  An entry of 0 means "not wanted": that row is not stored,
 *     the group's other rows are.  At any other entry the call writes exactly L_g bytes of the row
 *     (the row's bytes past L_g are zero by construction): nothing before the address and nothing
 *     at or past address + L_g.  L_g == 0 writes nothing and dereferences nothing.
 *   - A destination range must not overlap any packet the call reads, in any group, nor another
 *     destination range.
 *   - Asynchronous on `stream` (NULL = the context's own), drained by fec_encoder_free.  No host
 *     synchronise after the shape's first call, no readback and no workspace.  Per-context state:
 *     only the shape's r x k coefficient table on the device, uploaded at the shape's first call
 *     (none for r = 1).
 * Refusals launch nothing and write nothing (fec_hip_last_error names the case): FEC_ERR_NULL for a
 * NULL context, address table or destination table, the message naming the argument;
 * FEC_ERR_RANGE for k = 0, r = 0, k + r > 256, packet_size < 16, num_groups == 0 or >= 2^32. */
int fec_encode_scatter_wide_rs_dev(FECEncoderCtx* ctx, const uint64_t* d_packet_addrs,
                                   const uint32_t* d_packet_lens, const uint64_t* d_dest_addrs,
                                   uint64_t num_groups, uint32_t k, uint32_t r, uint32_t packet_size,
                                   uint32_t* d_symbol_len_out, void* stream);

/* Expected share (0..1) of groups that lost data shards in this context's device-resident
 * decode calls, e.g. 1 - (1 - p)^k for iid loss p (the receiver knows its network profile;
 * satellite p = 0.01, k = 10: ~0.10).  Below 0.25 the decode checks several groups per
 * wave instead of dispatching one wave per group, which saves the waves that would find
 * nothing to do; results are identical either way.  share < 0 or > 1: unknown (default,
 * treated as dense loss).  The host-pointer calls measure the share from the masks. */
int fec_decode_loss_hint(FECEncoderCtx* ctx, double share);

/* Where the device-resident calls of this context take their recovery records from, for a shape
 * whose codebook of every erasure pattern exceeds the 2 GiB cap (k=20 r=7, 24+6, 12+12, 16+16,
 * 32+8, 60+4, 32+32, ...; fec_decode_prepare reports 0 bytes for them).
 *   FEC_PLAN_CODEBOOK (default): fec_decode_batch_rs_dev and fec_recover_batch_rs_dev read the
 *     masks back to the host, build a record per distinct pattern there and complete
 *     synchronously; the three address-table recovers refuse the shape.
 *   FEC_PLAN_DEVICE: each group's record is built on the device, in the caller stream's
 *     workspace (at most 64 MiB of records per stream at a time; larger calls are walked in
 *     chunks), right before the kernel that reads it.  The two contiguous calls are then
 *     asynchronous on `stream` like every other shape, with no host synchronise and every status
 *     byte written on the device, and fec_recover_gather_rs_dev, fec_recover_gather_var_rs_dev
 *     and fec_recover_scatter_rs_dev serve the shape, outputs exactly as documented for the
 *     others.  The records are byte for byte the host's, so results are identical in both modes.
 * Shapes whose codebook fits keep it in either mode.  The host-pointer calls (fec_decode_batch_rs,
 * fec_group_*) and the batchers keep the host-built records (their masks are on the host
 * already), and fec_recover_batch_rs_dev_packed stays refused for these shapes.  Per context, like
 * fec_decode_loss_hint; applies to the calls made after it returns.  FEC_ERR_NULL for a NULL
 * context, FEC_ERR_RANGE for an unknown mode (the mode is then unchanged). */
#define FEC_PLAN_CODEBOOK 0
#define FEC_PLAN_DEVICE 1
int fec_decode_plan_mode(FECEncoderCtx* ctx, int mode);

/* Whether the three wide decoders -- fec_decode_wide_rs_dev, fec_recover_wide_rs_dev and
 * fec_recover_scatter_wide_rs_dev -- stop at min(k, r) <= 32 or recover every shape the encodes
 * produce.  Per context, like fec_decode_plan_mode.
 *   FEC_WIDE_ROWS_CAPPED (default): min(k, r) <= 32, as documented for each call above; 33 + 33,
 *     100 + 100 and 128 + 128 are refused with FEC_ERR_RANGE, byte for byte as before this mode
 *     existed.
 *   FEC_WIDE_ROWS_ALL: every k >= 1, r >= 1, k + r <= 256 with packet_size >= 16 and
 *     0 < num_groups < 2^32 is served: what fec_encode_batch_rs_dev and
 *     fec_encode_scatter_wide_rs_dev produce, these calls recover.  Every other contract point is
 *     the call's own as documented above: the mask rule, which survivors are read, the status
 *     bytes, the slots or destinations left unwritten, exactly L_g bytes at each destination,
 *     "not wanted" destinations, asynchronous on `stream` with no host synchronise and no
 *     readback, drained by fec_encoder_free.  A shape with min(k, r) <= 32 takes exactly the path
 *     of the capped mode: the same launches, the same bytes.  A shape past the cap takes the deep
 *     path for every group, whatever the group's own losses: each record is built by a whole
 *     workgroup (48.5 KiB of local memory, three workgroups per compute unit) instead of a wave.
 *   What a shape past the cap costs: the record slot is 512 + min(k, r) * k * 32 bytes, which is
 *     524,800 B at 128 + 128, so 127 groups fit in one 64 MiB plan chunk; each chunk takes one
 *     record build and ceil(min(k, r) / 8) consumer launches, up to 16, every one of which reads
 *     the group's survivors again.  DESIGN.md quotes what was measured.
 * The mode is read under the context's lock when a call starts and applies to the calls made
 * after this one returns.  FEC_ERR_NULL for a NULL context, FEC_ERR_RANGE for an unknown mode (the
 * mode is then unchanged). */
#define FEC_WIDE_ROWS_CAPPED 0
#define FEC_WIDE_ROWS_ALL 1
int fec_wide_rows_mode(FECEncoderCtx* ctx, int mode);

/* ---- utilities for benchmarks and tests ---- */
/* Fill d_dst with the counter-based splitmix64 stream (byte i of the stream at
 * byte_offset + i), asynchronously on stream. */
int fec_fill_random_dev(FECEncoderCtx* ctx, uint8_t* d_dst, uint64_t nbytes, uint64_t seed,
                        uint64_t byte_offset, void* stream);

/* d_dst <- d_src with the engine's own 16-B-per-lane access pattern, asynchronously on
 * stream: the HBM copy rate a box achieves, which the benchmark reports the FEC kernels
 * against.  nbytes and both addresses must be multiples of 16 (else FEC_ERR_RANGE). */
int fec_copy_dev(FECEncoderCtx* ctx, const uint8_t* d_src, uint8_t* d_dst, uint64_t nbytes, void* stream);

/* Wait for the context's own stream. */
int fec_synchronize(FECEncoderCtx* ctx);

/* ---- device groups: one host batch sharded over several GPUs ----
 * Groups are independent: shard i of n takes groups [G*i/n, G*(i+1)/n) on its own
 * context (device, streams, staging buffers) from its own host thread; no data moves
 * between devices.  Host buffers only (page-locked ones from
 * fec_alloc_slab stream at DMA rate); a device buffer gives FEC_ERR_RANGE.  Return codes
 * as the single-context calls; on failure fec_hip_last_error() names the shard. */
typedef struct FECDeviceGroup FECDeviceGroup;

/* devices: ordinals to use (repeats allowed), or NULL / ndevices <= 0 for every visible
 * device.  NULL when no GPU is usable or an ordinal is out of range. */
FECDeviceGroup* fec_group_new(const int* devices, int ndevices);
void fec_group_free(FECDeviceGroup* group);
int fec_group_size(const FECDeviceGroup* group);
/* Context of shard i (for device-resident work on that GPU), NULL if out of range. */
FECEncoderCtx* fec_group_context(FECDeviceGroup* group, int i);

int fec_group_encode_batch_rs(FECDeviceGroup* group, const uint8_t* data, uint64_t num_groups,
                              uint32_t k, uint32_t r, uint32_t packet_size, uint8_t* parity_out);

int fec_group_decode_batch_rs(FECDeviceGroup* group, uint8_t* data, const uint8_t* parity,
                              const uint64_t* erasure_masks, uint64_t num_groups, uint32_t k,
                              uint32_t r, uint32_t packet_size, uint8_t* status_out,
                              uint64_t* unrecoverable_out);

/* ---- batcher: one process-wide batch for the groups of many streams ----
 * The reference encodes one group per call (encoder_hybrid.go:115, one HybridFECEncoder per
 * QUIC stream, client.go:783).  A batcher collects finished groups from every stream of the
 * process and encodes them in one launch when max_groups are pending OR deadline_us have
 * passed since the oldest pending group arrived (deadline_us = 0: as soon as the flusher is
 * free; groups arriving meanwhile share the next launch).  A repair therefore waits at most
 * deadline_us plus one encode.  Groups are k slots of slot_bytes (shorter packets
 * zero-padded, a group of count < k packets has zero slots count..k-1, as encoder.go:133-143
 * XORs only the packets present); each group's r repair payloads are as long as its longest
 * packet (the reference's repair length, encoder_hybrid.go:91-98).  Memory: `slabs` (>= 2)
 * page-locked slabs of max_groups groups; submitters wait while every slab is in use.
 * Thread-safe; one flusher thread per batcher.  NULL on failure (fec_batcher_last_error). */
typedef struct FECBatcher FECBatcher;

typedef struct {
  uint64_t groups;            /* groups encoded                                    */
  uint64_t batches;           /* launches                                          */
  uint64_t full_flushes;      /* batches closed because max_groups were pending    */
  uint64_t deadline_flushes;  /* batches closed by the deadline (or fec_batcher_flush) */
  uint64_t max_batch;         /* largest batch                                     */
  uint64_t expired;           /* results dropped uncollected (see fec_batcher_wait) */
} FECBatcherStats;

FECBatcher* fec_batcher_new(int device, uint32_t k, uint32_t r, uint32_t slot_bytes, uint32_t max_groups,
                            uint32_t deadline_us, uint32_t slabs);
/* Encodes what is pending, then frees.  No call may be in flight on the batcher. */
void fec_batcher_free(FECBatcher* b);

/* One group: `count` (1..k) packets back to back in `packed`, packet j `lens[j]` bytes
 * (<= slot_bytes; not all empty).  Returns the group's ticket (>= 0) or a negative code. */
int64_t fec_batcher_submit(FECBatcher* b, const uint8_t* packed, const uint32_t* lens, uint32_t count);

/* The same with the packets where they are (packet j at packets[j]): one copy fewer for
 * C / C++ callers (cgo may not pass Go memory that holds Go pointers, so Go packs). */
int64_t fec_batcher_submit_packets(FECBatcher* b, const uint8_t* const* packets, const uint32_t* lens,
                                   uint32_t count);

/* Waits for a ticket's batch (timeout_us < 0: no limit; 0: poll) and copies its r repair
 * payloads to out (row i at out + i*out_stride; NULL: discard).  Returns the payload length,
 * FEC_ERR_AGAIN on timeout (the ticket stays valid), or another negative code.  Each ticket
 * can be collected once; the payloads are copied straight from the batcher's page-locked
 * parity ring.  A result not collected before 2 * slabs * max_groups newer groups are encoded
 * may be dropped (FEC_ERR_RANGE).  Polling (timeout 0) a ticket never issued returns
 * FEC_ERR_AGAIN; a blocking wait on it returns FEC_ERR_RANGE. */
int fec_batcher_wait(FECBatcher* b, int64_t ticket, uint8_t* out, uint32_t out_stride, int64_t timeout_us);

/* ---- decoder batcher: the receiving side's FECDecoder rebuilds one group per call
 * (decoder.go:216-287); a decoder batcher shares launches across every connection the same
 * way.  k + r <= 64.  A connection submits a group's k + r shards (data shards, then parity
 * rows 0..r-1; NULL = lost), each `len` <= slot_bytes bytes (the group's symbol length,
 * shorter packets zero-padded as decoder.go:62-69 does), and gets a ticket.  The batch runs
 * fec_recover_batch_rs_dev.  fec_batcher_flush / _stats / _free / _last_error apply. */
FECBatcher* fec_batcher_new_decoder(int device, uint32_t k, uint32_t r, uint32_t slot_bytes, uint32_t max_groups,
                                    uint32_t deadline_us, uint32_t slabs);
int64_t fec_batcher_submit_shards(FECBatcher* b, const uint8_t* const* shards, uint32_t len);

/* Waits as fec_batcher_wait and copies the group's rebuilt data shards, in ascending shard
 * order, to out (row i at out + i*out_stride, `len` bytes each); *lost_mask (nullable) = the
 * submitted erasure mask.  Returns the number of rows (0: nothing was lost),
 * FEC_ERR_UNRECOVERABLE when more shards were lost than parity rows survive, FEC_ERR_AGAIN,
 * or another negative code. */
int fec_batcher_wait_rebuilt(FECBatcher* b, int64_t ticket, uint8_t* out, uint32_t out_stride, uint64_t* lost_mask,
                             int64_t timeout_us);

/* Several GPUs behind one handle (SURVEY.md §8(e) for the host-resident path): one batcher
 * per listed device (ordinals, repeats allowed; NULL / ndevices <= 0: every visible device),
 * each with its own context, slabs, output ring and flusher thread.  A host-resident batch is
 * bound by its GPU's PCIe link, so N devices give N links.  Groups are dealt round robin,
 * passing over a device whose slabs are all busy while another has room; tickets stay unique
 * (device i of n hands out its ticket t as t * n + i) and every fec_batcher_* call above takes
 * the handle.  Stats sum over the devices (max_batch: the largest).  With one device this is
 * fec_batcher_new / fec_batcher_new_decoder.  NULL on failure (fec_batcher_last_error names
 * the device). */
FECBatcher* fec_batcher_new_multi(const int* devices, int ndevices, uint32_t k, uint32_t r, uint32_t slot_bytes,
                                  uint32_t max_groups, uint32_t deadline_us, uint32_t slabs);
FECBatcher* fec_batcher_new_decoder_multi(const int* devices, int ndevices, uint32_t k, uint32_t r,
                                          uint32_t slot_bytes, uint32_t max_groups, uint32_t deadline_us,
                                          uint32_t slabs);
/* Devices behind a batcher handle (1 for fec_batcher_new / _new_decoder). */
int fec_batcher_devices(const FECBatcher* b);

/* Closes the pending batch now (e.g. at the end of a stream) instead of at its deadline. */
int fec_batcher_flush(FECBatcher* b);

int fec_batcher_stats(FECBatcher* b, FECBatcherStats* out);

/* Message of the calling thread's last failing fec_batcher_* call. */
const char* fec_batcher_last_error(void);

/* ---- legacy-call coalescing (fec_coalesce.cpp) ----
 * Calls from page-locked slabs (fec_alloc_slab, as the Go wrapper packs them) of 1..8 groups
 * go to a resident encoder instead: one workgroup per device that stays launched while calls
 * keep coming and serves a ring of submission slots, so a call costs no kernel launch
 * (QUICFEC_RESIDENT=0 turns it off).  On a large-BAR device the ring is in device memory the
 * host writes directly (QUICFEC_RESIDENT_VRAM=0: page-locked host memory), and calls of at most
 * 4 groups with packet_size <= 1536 and a multiple of 4 have their packets copied into their
 * slot -- from any host memory, pageable slabs included.  The rest:
 * The reference's unchanged call site encodes one group per fec_encode_batch call, each stream
 * on its own context (encoder_hybrid.go:115 via fec_cgo.go:138, client.go:783).  Host-resident
 * legacy calls of at most QUICFEC_COALESCE_MAX_GROUPS groups (default 64) are joined, across
 * every context of the process, into shared launches on their device: a caller records its
 * packets' addresses (page-locked slabs are read in place, pageable ones copied to page-locked
 * staging), the first caller to find no launch slot busy closes the batch and launches it
 * (group commit: no flusher thread, so a lone caller pays no hand-off), and every caller gets
 * its own repair rows back with the legacy return codes (fec_xor_simd.cpp:556-594).
 * QUICFEC_COALESCE=0 turns it off (one launch and synchronize per call on the caller's context). */
typedef struct {
  uint64_t calls;      /* legacy calls that went through the coalescer */
  uint64_t groups;     /* their groups */
  uint64_t batches;    /* launches */
  uint64_t max_batch;  /* groups in the largest launch */
  uint64_t max_calls;  /* calls in the largest launch */
  uint64_t close_ns;   /* sums over launches: leader waiting for the batch's address writes, */
  uint64_t launch_ns;  /*   the launch calls, */
  uint64_t done_ns;    /*   and launch until the leader saw the batch complete */
  uint64_t resident_calls;     /* legacy calls served by the resident encoder instead */
  uint64_t resident_launches;  /* instances of the resident encoder launched */
  uint64_t resident_pre_ns;    /* sums over resident calls: entry until the slot was published, */
  uint64_t resident_wait_ns;   /*   published until its done word was seen, */
  uint64_t resident_post_ns;   /*   and from there to the return */
  uint64_t resident_inline;    /* resident calls whose packets the host copied into the slot */
  uint64_t resident_vram;      /* devices whose resident ring is in device memory (not reset) */
  uint64_t resident_bad_slots; /* polls that found a published slot with a word not yet landed, retried (not reset) */
  uint64_t resident_scrubs;    /* slots the resident encoder zeroed at a tag-epoch boundary (not reset) */
  uint64_t resident_servers;   /* serving workgroups per resident instance (QUICFEC_RESIDENT_SERVERS), the
                                  largest over devices; 0 before any resident encoder exists (not reset) */
} FECCoalesceStats;

/* Process-wide totals over every device and packet size; reset = 1 zeroes them after the read.
 * Writes min(out_bytes, sizeof(FECCoalesceStats)) bytes: pass sizeof(*out) of the struct the
 * caller was built with, so fields a later library appends are never written past it.
 * FEC_ERR_RANGE when out_bytes is below the first published layout (15 words). */
int fec_coalesce_stats_sized(FECCoalesceStats* out, size_t out_bytes, int reset);

/* The first published form: writes the first 15 fields only (calls .. resident_vram). */
int fec_coalesce_stats(FECCoalesceStats* out, int reset);

#ifdef __cplusplus
}
#endif

#endif /* FEC_HIP_H */
