// fec_decode.hip — gfx950 (MI355X, CDNA4) kernels of libfec_hip: the record-addressed decodes and
// launch_decode, the one entry of every contiguous decode.
//
//  * classify: one lane per group, erasure mask -> codebook record and status byte
//    (classify_mask, fec_device.hpp).  What a mask means -- losses, rows per group, the pick of
//    survivors and rows, the ranks and the record -- is fec_mask.hpp's for the cold kernels
//    (classify here, the rows_* prefix kernels of fec_runs.hip), which call it.  The mask-addressed
//    hot kernels (decode_fused's DIRECT / INLINE forms in fec_decode_fused.hip, recover_runs in
//    fec_runs.hip) do NOT: each keeps its own hand-written statement of the same rule
//    (profiles/mask_rule/VERDICT.md).
//  * decode_wave<K,MAXE>: one wave per group, record-addressed; the piece rebuild
//    (decode_piece) and the record header (RecHead) are fec_device.hpp's, shared with the
//    address-table recover of fec_gather.hip.
//  * decode_v16<K,MAXE>: one wave per group, so the record (survivor list + tables) is
//    wave-uniform and lives in SGPRs; lanes walk the group's 16-byte columns.
//  * decode_tiled<K,MAXE>: a workgroup owns whole groups, one lane per 16-byte column (packets of
//    <= 256 B).
//  * decode_bytes: packets shorter than 16 B (one lane per byte), same tables.
//
// Packet sizes and alignment: as for the encodes (fec_encode.hip header).
//
// launch_decode walks the plan chunks of a call whose records are built on the device
// (fec_plan.hip), checks the call against the chosen form, launches the classify and dispatches
// every form but decode_fused's, which are fec_decode_fused.hip's (launch_decode_fused): that
// family is 90 instantiations and most of the library's compile time.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "fec_device.hpp"  // Tab, ld16 / st16, rec_byte, decode_block; Sel, prep, mac, xor_into, gmul_byte, col_off16;
                           // classify_mask, RecHead, decode_piece
#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_launch.hpp"  // launch limits, for_chunks, for_wave_passes, for_plan_chunks, launch_record, knob, decode_swizzle

namespace qfec {
namespace {

// ---------------------------------------------------------------------------------
// Decode
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void classify(const uint64_t* __restrict__ masks, uint64_t groups,
                                                uint32_t k, uint32_t r,
                                                const uint64_t* __restrict__ binom, LevelMeta meta,
                                                uint32_t* __restrict__ rec_off,
                                                uint8_t* __restrict__ status) {
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
  if (g >= groups) return;
  const Classified c = classify_mask(masks[g], k, r, binom, meta);
  rec_off[g] = c.rec;
  if (status) status[g] = c.status;
}

// One wave per group, so the record is wave-uniform (SGPRs).  A packet is covered by
// whole 1 KiB passes of 16 B per lane, then the remainder (< 1 KiB) by 256 B passes of
// 4 B per lane: at 1200 B that is 64 + 44 busy lanes instead of 64 + 11 lanes doing
// 16-B work, i.e. 5 instead of 8 dword slots of VALU per lane and survivor.  Tail pieces
// past the packet end are shifted back to [P - 4, P) (duplicates of a neighbour's bytes,
// same values), so any P >= 4 works and no lane branches on the packet end.
template <int K, int MAXE, int POL = 0>
__global__ __launch_bounds__(256) void decode_wave(uint8_t* __restrict__ data,
                                                   const uint8_t* __restrict__ parity,
                                                   const uint32_t* __restrict__ rec_off,
                                                   const uint8_t* __restrict__ codebook,
                                                   uint64_t groups, uint32_t P, uint32_t k_rt, uint32_t r,
                                                   uint32_t m0, uint8_t* __restrict__ out, uint32_t never,
                                                   uint32_t swz, uint32_t lds_slice) {
  // Dynamic LDS: an occupancy cap, or (kLdsTabs) 4 per-wave slices of `lds_slice` bytes
  // holding the wave's coefficient rows (see kLdsTabs and decode_fused).
  extern __shared__ __attribute__((aligned(16))) uint8_t occupancy_lds[];
  if (never) occupancy_lds[threadIdx.x] = 0;
  const uint64_t gw = static_cast<uint64_t>(decode_block(swz)) * 4u +
                      static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
  if (gw >= groups) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t rec = __builtin_amdgcn_readfirstlane(rec_off[gw]);
  if (rec >= kRecBad) return;
  const uint32_t k = K > 0 ? static_cast<uint32_t>(K) : k_rt;
  const RecHead h = rec_head(codebook, rec);
  const uint32_t* rw = h.rw;
  const uint32_t e = h.e();
  const bool xor_only = h.xor_only();
  if (m0 >= e) return;
  const Tab* tabs = h.tabs();
  if constexpr ((POL & kLdsTabs) != 0) {
    if (!xor_only) {
      // rows [m0, m0 + min(e - m0, MAXE)) of the record into this wave's slice, by
      // direct-to-LDS loads (LDS address = wave base + lane * 16); every pass over the
      // packet then reads them from LDS instead of re-reading them through the scalar cache
      const uint32_t pieces = (e - m0 < MAXE ? e - m0 : MAXE) * k * 2u;
      const uint8_t* src = reinterpret_cast<const uint8_t*>(tabs + m0 * k);
      uint8_t* slice = occupancy_lds + (threadIdx.x >> 6) * lds_slice;
      for (uint32_t i = 0; i * 64u < pieces; ++i) {
        uint32_t idx = lane + 64u * i;
        if (idx >= pieces) idx = pieces - 1u;  // slots past the rows: unused, inside the slice
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(src + idx * 16u),
                                         (__attribute__((address_space(3))) void*)(slice + i * 1024u), 16, 0, 0);
      }
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      // decode_piece (fec_device.hpp) indexes rows from m0
      tabs = reinterpret_cast<const Tab*>(slice) - static_cast<ptrdiff_t>(m0) * k;
    }
  }
  const uint8_t* dg = data + gw * k * static_cast<uint64_t>(P);
  const uint8_t* pg = parity + gw * r * static_cast<uint64_t>(P);
  uint8_t* og = out + gw * ((POL & kCompactOut) != 0 ? r : k) * static_cast<uint64_t>(P);
  // decode_walk's two loops, spelled out: routed through the helper, the compile-time-k
  // instantiations come out with another instruction order (same instructions)
  const uint32_t main_end = P & ~1023u;
  for (uint32_t base = 0; base < main_end; base += 1024u)
    decode_piece<K, MAXE, POL, 4>(rw, tabs, dg, pg, og, k, P, base + lane * 16u, e, m0, xor_only);
  for (uint32_t base = main_end; base < P; base += 256u) {
    const uint32_t off = base + lane * 4u;
    decode_piece<K, MAXE, POL, 1>(rw, tabs, dg, pg, og, k, P, off + 4u <= P ? off : P - 4u, e, m0, xor_only);
  }
}

// One wave per group.  K > 0: compile-time k (survivor loads all issued first).
// MAXE: rows rebuilt per pass (rows [m0, m0 + MAXE) of the record's e).
template <int K, int MAXE, int POL = 0>
__global__ __launch_bounds__(256) void decode_v16(uint8_t* __restrict__ data,
                                                  const uint8_t* __restrict__ parity,
                                                  const uint32_t* __restrict__ rec_off,
                                                  const uint8_t* __restrict__ codebook,
                                                  uint64_t groups, uint32_t cpp, uint32_t P,
                                                  uint32_t k_rt, uint32_t r, uint32_t m0) {
  const uint64_t gw = static_cast<uint64_t>(blockIdx.x) * 4u +
                      static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
  if (gw >= groups) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t rec = __builtin_amdgcn_readfirstlane(rec_off[gw]);
  if (rec >= kRecBad) return;
  const uint32_t k = K > 0 ? static_cast<uint32_t>(K) : k_rt;
  const RecHead h = rec_head(codebook, rec);
  const uint32_t* rw = h.rw;
  const uint32_t e = h.e();
  const bool xor_only = h.xor_only();
  if (m0 >= e) return;
  const Tab* tabs = h.tabs();
  uint8_t* dg = data + gw * k * static_cast<uint64_t>(P);
  const uint8_t* pg = parity + gw * r * static_cast<uint64_t>(P);

  for (uint32_t col = lane; col < cpp; col += 64u) {
    const size_t coff = col_off16(col, P);
    if (xor_only) {  // single data loss rebuilt from parity row 0: the reference XOR
      u32x4 acc = {0u, 0u, 0u, 0u};
      for (uint32_t s = 0; s < k; ++s) {
        const uint32_t sid = rec_byte(rw, s);
        const uint8_t* src = sid < k ? dg + sid * static_cast<uint64_t>(P) : pg + (sid - k) * static_cast<uint64_t>(P);
        acc ^= ld16<POL>(src + coff);
      }
      st16<POL>(dg + rec_byte(rw, 64) * static_cast<uint64_t>(P) + coff, acc);
      continue;
    }
    u32x4 acc[MAXE];
#pragma unroll
    for (int m = 0; m < MAXE; ++m) acc[m] = u32x4{0u, 0u, 0u, 0u};
    if constexpr (K > 0) {
      u32x4 x[K];
#pragma unroll
      for (int s = 0; s < K; ++s) {
        const uint32_t sid = rec_byte(rw, s);
        const uint8_t* src = sid < k ? dg + sid * static_cast<uint64_t>(P) : pg + (sid - k) * static_cast<uint64_t>(P);
        x[s] = ld16<POL>(src + coff);
      }
#pragma unroll
      for (int s = 0; s < K; ++s) {
        Sel sl;
        prep(x[s], sl);
#pragma unroll
        for (int m = 0; m < MAXE; ++m) {
          if (m0 + m < e) {
            const Tab& t = tabs[(m0 + m) * K + s];
            if (t.coef == 1u) xor_into(acc[m], x[s]);
            else if (t.coef != 0u) mac(acc[m], sl, t);
          }
        }
      }
    } else {
#pragma unroll 2
      for (uint32_t s = 0; s < k; ++s) {
        const uint32_t sid = rec_byte(rw, s);
        const uint8_t* src = sid < k ? dg + sid * static_cast<uint64_t>(P) : pg + (sid - k) * static_cast<uint64_t>(P);
        const u32x4 xv = ld16<POL>(src + coff);
        Sel sl;
        prep(xv, sl);
#pragma unroll
        for (int m = 0; m < MAXE; ++m) {
          if (m0 + m < e) {
            const Tab& t = tabs[(m0 + m) * k + s];
            if (t.coef == 1u) xor_into(acc[m], xv);
            else if (t.coef != 0u) mac(acc[m], sl, t);
          }
        }
      }
    }
#pragma unroll
    for (int m = 0; m < MAXE; ++m) {
      if (m0 + m < e) {
        const uint32_t eid = rec_byte(rw, 64 + m0 + m);
        st16<POL>(dg + eid * static_cast<uint64_t>(P) + coff, acc[m]);
      }
    }
  }
}

// Tiled decode: a workgroup owns `tile` whole groups and one lane owns one 16-byte column
// of one group (all lanes busy, like encode_v16's tiled form).  A wave may then hold two
// groups with different erasure patterns, so each lane reads its own record (header and
// tables through the vector cache; lanes of one group read the same lines) and runs the
// multiply for every coefficient, 0 and 1 included (their tables are the zero / identity
// maps): no lane-divergent branches except the row count e.  The library's form for
// packets of <= 256 B, where one group per wave would leave most lanes idle (k=10 r=3,
// 2 erasures: 64 B 3.4 vs 0.72 TB/s, 256 B 4.6 vs 3.7; profiles/r01_probe_decode_small.txt).
template <int K, int MAXE, int POL = 0>
__global__ __launch_bounds__(512) void decode_tiled(const uint8_t* __restrict__ data,
                                                    const uint8_t* __restrict__ parity,
                                                    const uint32_t* __restrict__ rec_off,
                                                    const uint8_t* __restrict__ codebook,
                                                    uint64_t groups, uint32_t cpp, uint32_t P,
                                                    uint32_t r, uint32_t tile, uint8_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x;
  uint32_t gl = lane / cpp;
  const uint32_t col = lane - gl * cpp;
  if (gl >= tile) return;
  gl += blockIdx.x * tile;
  if (gl >= groups) return;
  const uint64_t g = gl;
  const uint32_t rec = rec_off[g];
  if (rec >= kRecBad) return;
  const RecHead h = rec_head(codebook, rec);  // per lane: a wave may hold two groups
  const uint32_t* rw = h.rw;
  const uint32_t e = h.e();
  const Tab* tabs = h.tabs();
  const uint8_t* dg = data + g * K * static_cast<uint64_t>(P);
  const uint8_t* pg = parity + g * r * static_cast<uint64_t>(P);
  // in place: the erased shard's slot; kCompactOut: row m of the group's run (g*r + m)*P
  uint8_t* og = out + g * ((POL & kCompactOut) != 0 ? r : K) * static_cast<uint64_t>(P);
  const size_t coff = col_off16(col, P);
  uint32_t sw[(K + 3) / 4];
#pragma unroll
  for (int q = 0; q < (K + 3) / 4; ++q) sw[q] = rw[q];
  u32x4 x[K];
#pragma unroll
  for (int s = 0; s < K; ++s) {
    const uint32_t sid = (sw[s >> 2] >> (8 * (s & 3))) & 0xFFu;
    const uint8_t* src = sid < K ? dg + sid * static_cast<uint64_t>(P) : pg + (sid - K) * static_cast<uint64_t>(P);
    x[s] = ld16<POL>(src + coff);
  }
  u32x4 acc[MAXE];
#pragma unroll
  for (int m = 0; m < MAXE; ++m) acc[m] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
  for (int s = 0; s < K; ++s) {
    Sel sl;
    prep(x[s], sl);
#pragma unroll
    for (int m = 0; m < MAXE; ++m) {
      if (static_cast<uint32_t>(m) < e) mac(acc[m], sl, tabs[m * K + s]);
    }
  }
  const uint32_t ew = rw[16];  // erased ids E_0..E_3 (bytes 64..67)
#pragma unroll
  for (int m = 0; m < MAXE; ++m) {
    if (static_cast<uint32_t>(m) < e) {
      const uint32_t eid = (POL & kCompactOut) != 0 ? static_cast<uint32_t>(m)
                           : m < 4                     ? (ew >> (8 * m)) & 0xFFu
                                                       : rec_byte(rw, 64 + m);
      st16<POL>(og + eid * static_cast<uint64_t>(P) + coff, acc[m]);
    }
  }
}

// Decode, one lane per byte (packets shorter than 16 B).
__global__ __launch_bounds__(256) void decode_bytes(const uint8_t* __restrict__ data,
                                                    const uint8_t* __restrict__ parity,
                                                    const uint32_t* __restrict__ rec_off,
                                                    const uint8_t* __restrict__ codebook,
                                                    uint64_t g_first, uint32_t nthreads, uint32_t P,
                                                    uint32_t k, uint32_t r, uint8_t* __restrict__ out,
                                                    uint32_t compact) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= nthreads) return;
  const uint32_t gl = t / P;
  const uint32_t b = t - gl * P;
  const uint64_t g = g_first + gl;
  const uint32_t rec = rec_off[g];
  if (rec >= kRecBad) return;
  const uint8_t* recp = codebook + static_cast<uint64_t>(rec) * 32u;
  const uint32_t e = recp[96];
  const Tab* tabs = reinterpret_cast<const Tab*>(recp + 128);
  const uint8_t* dg = data + g * k * static_cast<uint64_t>(P);
  const uint8_t* pg = parity + g * r * static_cast<uint64_t>(P);
  for (uint32_t m = 0; m < e; ++m) {
    uint32_t acc = 0;
    for (uint32_t s = 0; s < k; ++s) {
      const uint32_t sid = recp[s];
      const uint32_t x = sid < k ? dg[sid * static_cast<uint64_t>(P) + b] : pg[(sid - k) * static_cast<uint64_t>(P) + b];
      acc ^= gmul_byte(x, tabs[m * k + s]);
    }
    // Erased shards are never survivors, so writing here cannot feed a later read.
    const uint64_t slot = compact ? g * r + m : g * k + recp[64 + m];
    out[slot * static_cast<uint64_t>(P) + b] = static_cast<uint8_t>(acc);
  }
}

}  // namespace

// ---------------------------------------------------------------------------------
// Launchers: which form a call takes is decided in fec_forms.hpp; these only launch it.
// ---------------------------------------------------------------------------------
namespace {

hipError_t run_classify(const DecodeLaunch& a, hipStream_t s) {
  return for_chunks(a.groups, max_launch_threads(), [&](uint64_t g0, uint64_t gn) {
    trace_launch(launch_record(LaunchForm::kClassify, blocks_for(gn), 256, g0, gn));
    hipLaunchKernelGGL(classify, dim3(blocks_for(gn)), dim3(256), 0, s, a.masks + g0, gn, a.k, a.r,
                       a.binom, a.meta, a.rec_off ? a.rec_off + g0 : nullptr, a.status ? a.status + g0 : nullptr);
  });
}

hipError_t run_decode_bytes(const DecodeLaunch& a, hipStream_t s) {
  return for_chunks(a.groups, groups_per_launch(a.P), [&](uint64_t g0, uint64_t gn) {
    const uint32_t n = static_cast<uint32_t>(gn * a.P);
    LaunchRecord t = launch_record(LaunchForm::kDecodeBytes, blocks_for(n), 256, g0, gn);
    t.k = 0, t.pol = a.compact_out ? kCompactOut : 0;
    trace_launch(t);
    hipLaunchKernelGGL(decode_bytes, dim3(blocks_for(n)), dim3(256), 0, s, a.data, a.parity,
                       a.rec_off, a.codebook, g0, n, a.P, a.k, a.r, a.out ? a.out : a.data,
                       a.compact_out ? 1u : 0u);
  });
}

// The wave-per-group decodes chunk their groups by whole workgroups, at most max_wave_blocks() of
// them per launch: decode_v16 and decode_wave (4 groups per workgroup) through for_wave_passes
// (fec_launch.hpp); decode_fused (fec_decode_fused.hip), whose scan forms take more groups per
// workgroup, in a loop of its own.
template <int K, int MAXE>
hipError_t run_decode_v16(const DecodeLaunch& a, hipStream_t s) {
  const uint32_t cpp = (a.P + 15u) / 16u;
  return for_wave_passes(a.groups, a.r, MAXE, [&](uint64_t g0, uint64_t gn, uint64_t bn, uint32_t m0) {
    LaunchRecord t = launch_record(LaunchForm::kDecodeV16, bn, 256, g0, gn);
    t.k = K, t.r = MAXE, t.aux = m0;
    trace_launch(t);
    hipLaunchKernelGGL((decode_v16<K, MAXE>), dim3(static_cast<uint32_t>(bn)), dim3(256), 0, s,
                       a.data + g0 * a.k * static_cast<uint64_t>(a.P),
                       a.parity + g0 * a.r * static_cast<uint64_t>(a.P), a.rec_off ? a.rec_off + g0 : nullptr, a.codebook,
                       gn, cpp, a.P, a.k, a.r, m0);
  });
}

template <int K, int MAXE, int POL>
hipError_t run_decode_wave(const DecodeLaunch& a, hipStream_t s) {
  const uint32_t cap = occupancy_cap_lds(a.waves_per_cu ? a.waves_per_cu : knob(TestKnob::kDecodeWaves, kDecodeWavesPerCU), 4);
  return for_wave_passes(a.groups, a.r, MAXE, [&](uint64_t g0, uint64_t gn, uint64_t bn, uint32_t m0) {
    // kLdsTabs: per-wave slice of whole 1 KiB wave-loads covering this pass's rows
    const uint32_t rows = a.r - m0 < MAXE ? a.r - m0 : MAXE;
    const uint32_t slice = (POL & kLdsTabs) != 0 ? (rows * a.k * 2u + 63u) / 64u * 1024u : 0u;
    const uint32_t smem = cap > 4 * slice ? cap : 4 * slice;
    LaunchRecord t = launch_record(LaunchForm::kDecodeWave, bn, 256, g0, gn);
    t.k = K, t.r = MAXE, t.pol = POL, t.aux = m0;
    trace_launch(t);
    hipLaunchKernelGGL((decode_wave<K, MAXE, POL>), dim3(static_cast<uint32_t>(bn)), dim3(256), smem, s,
                       a.data + g0 * a.k * static_cast<uint64_t>(a.P),
                       a.parity + g0 * a.r * static_cast<uint64_t>(a.P), a.rec_off ? a.rec_off + g0 : nullptr, a.codebook, gn, a.P,
                       a.k, a.r, m0, (a.out ? a.out : a.data) + g0 * ((POL & kCompactOut) != 0 ? a.r : a.k) * static_cast<uint64_t>(a.P), 0u,
                       decode_swizzle(a, kDecodeWaveXcdSwizzle), slice);
  });
}

template <int K, int MAXE, int POL>
hipError_t run_decode_tiled(const DecodeLaunch& a, uint32_t tile, hipStream_t s) {
  const uint32_t cpp = (a.P + 15u) / 16u;
  const uint32_t bs = (tile * cpp + 63) / 64 * 64;
  // whole workgroups per launch: blocks * bs stays a 32-bit grid
  return for_chunks(a.groups, groups_per_launch(bs) * tile, [&](uint64_t g0, uint64_t gn) {
    const uint64_t bn = (gn + tile - 1) / tile;
    LaunchRecord t = launch_record(LaunchForm::kDecodeTiled, bn, bs, g0, gn);
    t.k = K, t.r = MAXE, t.pol = POL, t.tile = tile;
    trace_launch(t);
    hipLaunchKernelGGL((decode_tiled<K, MAXE, POL>), dim3(static_cast<uint32_t>(bn)), dim3(bs), 0, s,
                       a.data + g0 * a.k * static_cast<uint64_t>(a.P),
                       a.parity + g0 * a.r * static_cast<uint64_t>(a.P), a.rec_off ? a.rec_off + g0 : nullptr, a.codebook, gn, cpp,
                       a.P, a.r, tile,
                       (a.out ? a.out : a.data) + g0 * ((POL & kCompactOut) != 0 ? a.r : a.k) * static_cast<uint64_t>(a.P));
  });
}

// One entry of this unit's form lists (fec_forms.hpp QFEC_DECODE_OTHER_FORMS, QFEC_PROBE_DECODE_FORMS)
// to its instantiation.
template <DecodeKernel KERNEL, int K, int MAXE, int NM, int NT, int POL, bool DIRECT, int SCAN>
hipError_t run_decode_form(const DecodeLaunch& a, uint32_t tile, hipStream_t s) {
  static_assert(KERNEL != DecodeKernel::kFused, "decode_fused's forms are fec_decode_fused.hip's");
  if constexpr (KERNEL == DecodeKernel::kTiled) return run_decode_tiled<K, MAXE, POL>(a, tile, s);
  else if constexpr (KERNEL == DecodeKernel::kWave) return run_decode_wave<K, MAXE, POL>(a, s);
  else if constexpr (KERNEL == DecodeKernel::kV16) return run_decode_v16<K, MAXE>(a, s);
  else return run_decode_bytes(a, s);
}

}  // namespace

hipError_t launch_decode(const DecodeLaunch& a, hipStream_t s) {
  const DecodeForm f = decode_form(a);
  if (f.kernel == DecodeKernel::kNone) return hipSuccess;
  if (a.plan.arena != nullptr) {
    // Records built on the device: the classify on an all-zero level table (0 where a record is
    // needed, else kRecNone / kRecBad, and every status byte), then per chunk of the arena the
    // records and this form's launches on them (plan_chunk: rec_ready, the arena as codebook).
    if (!a.rec_ready || !f.rec_off || a.rec_off == nullptr || a.masks == nullptr || a.packed_rows || a.plan.per_chunk == 0)
      return hipErrorInvalidValue;
    return for_plan_chunks(
        a.groups, a.plan.per_chunk,
        [&] {
          DecodeLaunch c = a;
          c.meta = LevelMeta{};
          return run_classify(c, s);
        },
        [&](uint64_t g0, uint64_t gn) {
          return launch_build_records(a.plan, a.masks + g0, a.rec_off + g0, a.status ? a.status + g0 : nullptr, g0, gn, a.k,
                                      a.r, s);
        },
        [&](uint64_t g0, uint64_t gn) { return launch_decode(plan_chunk(a, g0, gn), s); });
  }
  // the codebook's format must be the one the chosen form reads
  if (a.compact_tables != f.compact_tables) return hipErrorInvalidValue;
  if (f.rec_off && a.rec_off == nullptr) return hipErrorInvalidValue;
  if (f.classify) {
    const hipError_t e = run_classify(a, s);
    if (e != hipSuccess) return e;
  }
  // the lists that name what is compiled are the ones decode_form's predicates come from; the
  // probes' forms are not in the product library
  if (f.kernel == DecodeKernel::kFused) return launch_decode_fused(a, f, s);
#define QFEC_FORM(KERNEL, KK, MM, NMM, NTT, PP, DD, SS)                                                             \
  if (f.kernel == DecodeKernel::KERNEL && f.K == KK && f.MAXE == MM && f.NM == NMM && f.NT == NTT && f.POL == (PP) && \
      f.DIRECT == DD && f.SCAN == static_cast<int>(SS))                                                             \
    return run_decode_form<DecodeKernel::KERNEL, KK, MM, NMM, NTT, PP, DD, SS>(a, f.tile, s);
  QFEC_DECODE_OTHER_FORMS(QFEC_FORM)
#ifdef QUICFEC_PROBE_FORMS
  QFEC_PROBE_DECODE_FORMS(QFEC_FORM)
#endif
#undef QFEC_FORM
  return hipErrorNotSupported;
}

// `classify` alone, for another unit's call (fec_packed.hip): run_classify on the fields it reads.
// With an all-zero a.meta it is the device plans' classify (0 where a record is needed).
hipError_t launch_classify(const DecodeLaunch& a, hipStream_t s) {
  if (a.masks == nullptr || a.rec_off == nullptr || a.groups == 0) return hipErrorInvalidValue;
  return run_classify(a, s);
}

hipError_t load_decode_unit() {
  hipFuncAttributes at;
  return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(classify));
}

}  // namespace qfec
