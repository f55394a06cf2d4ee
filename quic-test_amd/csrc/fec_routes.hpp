// fec_routes.hpp — which way a host-memory call (fec_encode_batch_rs, fec_decode_batch_rs, the
// legacy fec_encode_batch) goes, and the host-side rules those ways share: the chunk size of the
// DMA pipeline, the window of a call's packet offsets (the rule of an erasure mask: fec_mask.hpp).
// Host-only (no HIP include, no device code, no environment), so a plain C++ program can ask for
// every combination (tests/csrc/routes_dump.cpp).  fec_shim.cpp classifies the pointers, reads the
// limits' overrides, asks here and switches on the answer.
#pragma once

#include <cstdint>

#include "fec_mask.hpp"  // the rule of an erasure mask: mask_losses, lost_data / lost_parity, for_each_lost

namespace qfec {

// Where a caller's pointer lives: pageable host memory, page-locked host memory (kernels can
// address it over PCIe), device memory.
enum class Mem { kHost, kPinned, kDevice };

// ---- the limits ----
// Host-resident calls up to a small-call limit (data + parity bytes) run zero-copy: the kernels
// address page-locked host memory directly over PCIe -- the caller's buffers when they are
// page-locked (fec_alloc_slab), else the context's page-locked staging, filled and drained by CPU
// memcpy.  No DMA copies: one kernel launch and one stream synchronize per call, where the DMA
// path pays a copy-engine round trip per buffer.  Measured (tools/latency.cpp, k=10 r=3 1200 B,
// profiles/r01_latency_sweep.txt): one group 33 -> 15 us (legacy fec_encode_batch).  With
// page-locked buffers zero-copy beats the DMA pipeline at every size (4096 groups: 942 vs 1013 us
// encode, 947 vs 1281 us decode; 1M groups, 12 GB: encode 52.0 vs 48.7 GiB/s, 2-erasure decode
// 52.4 vs 34.8, C5 sparse-loss decode 454 vs 243; profiles/r01_e2e_zero_copy.txt), so it has no
// limit; staged pageable buffers pay a CPU memcpy and break even near 3 MB.
constexpr uint64_t kZeroCopyPinnedBytes = ~0ull;
constexpr uint64_t kZeroCopyStagedBytes = 2ull << 20;
struct SmallCallLimits {
  uint64_t pinned, staged;  // every buffer of the call page-locked / some through the context's staging
  constexpr uint64_t of(bool all_pinned) const { return all_pinned ? pinned : staged; }
};
// override_bytes >= 0 (QUICFEC_SMALL_CALL_BYTES) replaces both limits, 0 = always DMA.
constexpr SmallCallLimits small_call_limits(long long override_bytes) {
  const uint64_t x = static_cast<uint64_t>(override_bytes);
  return override_bytes >= 0 ? SmallCallLimits{x, x} : SmallCallLimits{kZeroCopyPinnedBytes, kZeroCopyStagedBytes};
}
// Host-resident decode moves only the groups to rebuild when they are at most 1 in
// kCompactMaxShare of the batch; above that the whole batch streams through the pipeline.
constexpr uint64_t kCompactMaxShare = 2;
// The host<->device pipeline: chunk c of ~64 MB of data on slot c % kPipeSlots, so the copy engines
// (H2D and D2H run on separate DMA engines) and the kernels of neighbouring chunks overlap.
constexpr int kPipeSlots = 3;
constexpr uint64_t kPipeChunkBytes = 64ull << 20;  // data bytes per pipelined chunk
// Groups per chunk of a pipelined call of n groups of in_g data bytes: at least one, at most all.
constexpr uint64_t pipe_chunk_groups(uint64_t chunk_bytes, uint64_t in_g, uint64_t n) {
  return chunk_bytes / in_g == 0 ? 1 : (chunk_bytes / in_g > n ? n : chunk_bytes / in_g);
}

// ---- the routes ----
// kZeroCopy: the kernels address host memory (above); kPipelined: chunks through the DMA pipeline;
// kStaged: a buffer is on the device or the packets sit at offsets: whatever is on the host goes
// through the context's device buffers in one shot.
enum class EncodeRoute { kZeroCopy, kPipelined, kStaged };
constexpr EncodeRoute encode_route(Mem data, Mem out, bool offsets, uint64_t total_bytes, SmallCallLimits lim) {
  if (offsets || data == Mem::kDevice || out == Mem::kDevice) return EncodeRoute::kStaged;
  const bool small = total_bytes <= lim.of(data == Mem::kPinned && out == Mem::kPinned);
  return small ? EncodeRoute::kZeroCopy : EncodeRoute::kPipelined;
}

// The buffers of a decode; a NULL status_out counts as host memory.
struct DecodeMem {
  Mem data, parity, masks, status;
  // nothing on the device: the host reads the masks, so it knows the statuses and the groups to rebuild
  constexpr bool host_resident() const {
    return data != Mem::kDevice && parity != Mem::kDevice && masks != Mem::kDevice && status != Mem::kDevice;
  }
};
// kNothing: no group to rebuild, the statuses of the host's scan are the whole answer; kCompacted:
// only the `need` groups to rebuild go through the pipeline (a small call: zero-copy, whatever the
// share).  `need` is read for host-resident calls only.
enum class DecodeRoute { kNothing, kZeroCopy, kCompacted, kPipelined, kStaged };
constexpr DecodeRoute decode_route(DecodeMem mem, uint64_t total_bytes, uint64_t G, uint64_t need, SmallCallLimits lim) {
  if (!mem.host_resident()) return DecodeRoute::kStaged;
  const bool small = total_bytes <= lim.of(mem.data == Mem::kPinned && mem.parity == Mem::kPinned);
  if (!small && need * kCompactMaxShare > G) return DecodeRoute::kPipelined;
  return need == 0 ? DecodeRoute::kNothing : small ? DecodeRoute::kZeroCopy : DecodeRoute::kCompacted;
}

// The legacy call: packets at u32 offsets into a slab.  Zero-copy when slab and output are on the
// host, the call is small and the slab is page-locked or its window [lo, hi + P) small enough to
// stage; else staged.  `rebase`: the kernel reads a copy of the window, so offsets count from lo (a
// host slab that is not addressed in place).  `span` is read for host slabs only.
struct LegacyEncodeRoute {
  EncodeRoute route;  // kZeroCopy or kStaged
  bool rebase;
};
constexpr LegacyEncodeRoute legacy_encode_route(Mem slab, Mem out, uint64_t total_bytes, uint64_t span,
                                                SmallCallLimits lim) {
  if (slab == Mem::kDevice) return {EncodeRoute::kStaged, false};
  const uint64_t small = lim.of(slab == Mem::kPinned && out == Mem::kPinned);
  if (out != Mem::kDevice && total_bytes <= small && (slab == Mem::kPinned || span <= small))
    return {EncodeRoute::kZeroCopy, slab != Mem::kPinned};
  return {EncodeRoute::kStaged, true};
}

// ---- packet offsets ----
// The window of n >= 1 packets of P bytes at offsets off[i]: [lo, hi + P), span bytes long.
template <class T>
struct OffsetWindow {
  T lo, hi;
  uint64_t span;
};
template <class T>
inline OffsetWindow<T> offset_window(const T* off, uint64_t n, uint64_t P) {
  T lo = static_cast<T>(~T(0)), hi = 0;
  for (uint64_t i = 0; i < n; ++i) lo = off[i] < lo ? off[i] : lo, hi = off[i] > hi ? off[i] : hi;
  return {lo, hi, static_cast<uint64_t>(hi) + P - lo};
}
// The offsets counted from the window's start.
template <class T>
inline void rebase_offsets(const T* off, uint64_t n, T lo, T* out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = off[i] - lo;
}

}  // namespace qfec
