// fec_decode_fused.hip — gfx950 (MI355X, CDNA4) kernels of libfec_hip: decode_fused, the
// wave-per-group decode with a packet's 16-B and 4-B passes fused, record-addressed (with its
// tables through LDS for r > 3) and mask-addressed (DIRECT / INLINE, and the scan form for sparse
// loss).  A unit of its own because its 90 instantiations are most of the library's compile time;
// entered only from fec_decode.hip's launch_decode, through launch_decode_fused.
//
// The mask-addressed forms do NOT call fec_mask.hpp: fused_group keeps its own hand-written
// statement of the rule, because every call into the header that was tried changed their
// instructions (profiles/mask_rule/VERDICT.md).  They share ChooseSmall, low_bits(K) and
// piece_load only, and only the GPU tests check their copy: test_every_mask (tests/test_gpu_forms.py), clean
// and with junk in the bits at and above k + r, and the decode cases, whose masks all carry such junk.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "coef_tables.hpp"
#include "fec_device.hpp"  // Tab, st16, gmul, piece_load, SelN / sel_split, rec_byte, decode_block, RecHead, RankMeta;
                           // fec_mask.hpp: low_bits, ChooseSmall
#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_launch.hpp"  // launch limits, for_chunks, launch_record, knob, decode_swizzle, rank_meta

namespace qfec {
namespace {

// Per-wave LDS slice of N coefficient entries (decode_fused with kLdsTabs; 4 waves per
// workgroup).  Only instantiated by the kernels that use it.
template <int N>
__device__ __forceinline__ Tab* wave_tabs_lds() {
  __shared__ __attribute__((aligned(16))) Tab t[4 * N];
  return t + (threadIdx.x >> 6) * N;
}

// f(std::integral_constant<int, n>) for a wave-uniform n in [1, N]: one straight-line body
// per row count.
template <int N, typename F>
__device__ __forceinline__ void for_row_count(uint32_t n, F& f) {
  if constexpr (N >= 1) {
    if (n == static_cast<uint32_t>(N)) {
      f(std::integral_constant<int, N>{});
      return;
    }
    for_row_count<N - 1>(n, f);
  }
}

// decode_wave with the main (16 B/lane) and tail (4 B/lane) passes fused: each lane holds
// NM 16-byte pieces and NT 4-byte pieces of every survivor, so every coefficient table is
// loaded (scalar) and branched on once per wave instead of once per pass.  Packet sizes
// with NM = P / 1024 and NT = ceil((P % 1024) / 256) matching the instantiation.  Tail
// pieces past the packet end are shifted back to [P - 4, P) (same bytes, same values as
// the lane that owns them), so every lane loads and stores and no packet size needs a
// mask; P >= 4.
//
// DIRECT: the survivor and erased shard ids come from the group's erasure mask (scalar bit
// scans) instead of the record header, so the survivor loads depend on one scalar load
// (the mask) rather than two in a chain (rec_off, then the record); the record is then
// read only for its coefficient tables, behind the data loads.  Same ids in the same order
// as the record (gf256.hpp build_record: surviving data ascending, then the e lowest
// surviving parity rows; erased data ascending).
//
// INLINE (mask-addressed only, e <= 3): the kernel classifies its group itself — status
// byte, colex ranks of the erased data set and of the parity rows used, record offset,
// exactly as `classify` does — so no classify launch (and no rec_off round trip through
// HBM) precedes it.  One launch per decode call instead of two.
//
// SCAN > 0 (mask-addressed inline forms): one wave per SCAN consecutive groups (see the
// kernel).
//
// One group of decode_fused (below): `m` is the group's erasure mask (DIRECT forms; wave-
// uniform), `lane` the lane in the wave.
template <int K, int MAXE, int POL, int NM, int NT, bool DIRECT, bool INLINE>
__device__ __forceinline__ void fused_group(uint64_t gw, uint64_t m, uint32_t lane, const uint8_t* __restrict__ data,
                                            const uint8_t* __restrict__ parity,
                                            const uint32_t* __restrict__ rec_off,
                                            const uint8_t* __restrict__ codebook, uint32_t P, uint32_t r,
                                            uint32_t m0, uint8_t* __restrict__ out, const RankMeta& rm,
                                            uint8_t* __restrict__ status) {
  constexpr int NW = 4 * NM + NT;  // dwords per lane and survivor
  // (the classify, the ranks and the pick below restate fec_mask.hpp's mask_losses, mask_record and
  // mask_pick by hand: calling them, colex_rank alone, or low_bits(r) for the rows' mask, moves all
  // 90 mask-addressed decode_fused instantiations.  Not checked on the CPU: `& kmask` and both `& rmask`
  // are held by the GPU cases' junk in the mask bits at and above k + r, tests/unread_shards.py high_bits.)
  constexpr uint64_t kmask = low_bits(K);
  uint64_t rec_byte_off;
  if constexpr (INLINE) {
    uint64_t dm = m & kmask;
    const uint64_t rmask = (1ull << r) - 1;
    const uint64_t pm = (m >> K) & rmask;
    const uint32_t ne = static_cast<uint32_t>(__popcll(dm));
    const bool bad = ne > r - static_cast<uint32_t>(__popcll(pm));
    if (status != nullptr && lane == 0) status[gw] = bad ? 1 : 0;
    if (ne == 0 || bad) return;
    uint64_t rank_e = 0, rank_r = 0;
    for (uint32_t t = 0; dm; ++t) {
      rank_e += ChooseSmall{}(static_cast<uint32_t>(__builtin_ctzll(dm)), t + 1u);
      dm &= dm - 1;
    }
    uint64_t sp = ~pm & rmask;
    for (uint32_t t = 0; t < ne; ++t) {
      rank_r += ChooseSmall{}(static_cast<uint32_t>(__builtin_ctzll(sp)), t + 1u);
      sp &= sp - 1;
    }
    rec_byte_off = rm.base[ne] + (rank_e * rm.count_r[ne] + rank_r) * rm.stride[ne];
  } else {
    const uint32_t rec = __builtin_amdgcn_readfirstlane(rec_off[gw]);
    if (rec >= kRecBad) return;
    rec_byte_off = static_cast<uint64_t>(rec) * 32u;
  }
  const uint8_t* recp = codebook + rec_byte_off;
  const RecHead h = rec_head(recp);
  const uint32_t* rw = h.rw;
  uint32_t e;
  bool xor_only;
  // DIRECT: survivor ids (ascending bits of `surv`) and erased ids (bits of `lost`).
  uint64_t surv = 0, lost = 0;
  if constexpr (DIRECT) {
    lost = m & kmask;
    e = static_cast<uint32_t>(__popcll(lost));
    uint64_t alive = ~(m >> K) & ((r >= 64 ? 0ull : (1ull << r)) - 1);  // low_bits(r)
    xor_only = e == 1 && (alive & 1u);
    uint64_t rsel = 0;
    for (uint32_t t = 0; t < e; ++t) {
      rsel |= alive & (~alive + 1);
      alive &= alive - 1;
    }
    surv = (~lost & kmask) | (rsel << K);
  } else {
    e = h.e();
    xor_only = h.xor_only();
  }
  if (m0 >= e) return;
  const Tab* tabs = h.tabs();
  const uint8_t* dg = data + gw * K * static_cast<uint64_t>(P);
  const uint8_t* pg = parity + gw * r * static_cast<uint64_t>(P);
  uint8_t* og = out + gw * K * static_cast<uint64_t>(P);
  uint32_t toff[NT > 0 ? NT : 1];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    toff[t] = NM * 1024u + t * 256u + lane * 4u;
    if (toff[t] + 4u > P) toff[t] = P - 4u;
  }
  // (the load is fec_device.hpp's piece_load, shared with runs_load; the same for the tail offsets
  // or the store moves decode_fused<20,5,2115,0,2>, and for recover_runs' row stores 14 or 15 of its 36
  // instantiations: those stay spelled out)
  auto load = [&](const uint8_t* base, uint32_t (&v)[NW]) { piece_load<NM, NT, POL>(base, lane, toff, v); };
  auto store = [&](uint8_t* base, const uint32_t (&v)[NW]) {
#pragma unroll
    for (int i = 0; i < NM; ++i) st16<POL>(base + i * 1024u + lane * 16u, u32x4{v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]});
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if constexpr ((POL & kNtStore) != 0) __builtin_nontemporal_store(v[4 * NM + t], reinterpret_cast<u32u*>(base + toff[t]));
      else *reinterpret_cast<u32u*>(base + toff[t]) = v[4 * NM + t];
    }
  };
  auto shard = [&](uint32_t sid) {
    return sid < K ? dg + sid * static_cast<uint64_t>(P) : pg + (sid - K) * static_cast<uint64_t>(P);
  };
  // Survivor slot s -> shard id, and erased slot m -> data shard id.
  uint32_t sid[K];
#pragma unroll
  for (int s = 0; s < K; ++s) {
    if constexpr (DIRECT) {
      sid[s] = static_cast<uint32_t>(__builtin_ctzll(surv));
      surv &= surv - 1;
    } else {
      sid[s] = rec_byte(rw, s);
    }
  }
  // destination of rebuilt row m (erased data shard `erased(m)`)
  auto dest = [&](uint32_t m, uint32_t eid) -> uint8_t* {
    if constexpr ((POL & kCompactOut) != 0) {
      // packed rows (fec_recover_batch_rs_dev_packed): the group's first row from its prefix
      // sum, passed in rec_off, which the inline-classify forms do not otherwise read
      uint64_t row = gw * r + m;
      if constexpr (INLINE) {
        if (rec_off != nullptr) row = static_cast<uint64_t>(__builtin_amdgcn_readfirstlane(rec_off[gw])) + m;
      }
      return out + row * static_cast<uint64_t>(P);
    } else {
      return og + eid * static_cast<uint64_t>(P);
    }
  };
  auto erased = [&](uint32_t m) -> uint32_t {
    if constexpr (DIRECT) {
      uint64_t x = lost;
      for (uint32_t t = 0; t < m; ++t) x &= x - 1;
      return static_cast<uint32_t>(__builtin_ctzll(x));
    } else {
      return rec_byte(rw, 64 + m);
    }
  };
  if (xor_only) {  // single data loss rebuilt from parity row 0: the reference XOR
    uint32_t acc[NW] = {};
#pragma unroll
    for (int s = 0; s < K; ++s) {
      uint32_t v[NW];
      load(shard(sid[s]), v);
#pragma unroll
      for (int q = 0; q < NW; ++q) acc[q] ^= v[q];
    }
    store(dest(0, erased(0)), acc);
    return;
  }
  // kLdsTabs: the wave's coefficient rows [m0, m0 + MAXE) come in with vector loads issued
  // next to the survivor loads and are read back from LDS, instead of one scalar load per
  // coefficient (records of large codebooks miss the scalar cache; see kLdsTabs).
  constexpr bool kLds = (POL & kLdsTabs) != 0;
  constexpr int kTabPieces = MAXE * K * 2;  // 16-B pieces of MAXE rows of K entries
  constexpr int kTabIter = kLds ? (kTabPieces + 63) / 64 : 1;
  const uint32_t tab_pieces = (e - m0 < MAXE ? e - m0 : MAXE) * K * 2u;
  // the slice holds kTabIter whole wave-loads (16 B per lane), so no load writes past it
  constexpr int kSliceTabs = kTabIter * 64 / 2;
  // kCoefBytes: coefficient (m, s) of this pass is byte m * K + s after the compact record's
  // header; lane i loads coefficient i (+ 64 j) now, ahead of the survivor loads, and builds
  // its tables into the LDS slice once the survivor loads are in flight (below).
  constexpr int kCoefIter = (MAXE * K + 63) / 64;
  uint32_t coef[kCoefIter];
  if constexpr (kLds && (POL & kCoefBytes) != 0) {
    const uint8_t* cb = recp + 128 + m0 * K;
    const uint32_t ncoef = tab_pieces / 2u;
#pragma unroll
    for (int j = 0; j < kCoefIter; ++j) {
      const uint32_t i = lane + 64u * j;
      coef[j] = i < ncoef ? cb[i] : 0u;
    }
  } else if constexpr (kLds) {
    // direct-to-LDS loads (global_load_lds_dwordx4: LDS address = wave base + lane * 16, no
    // VGPR destination); pieces past the rows re-read the last piece into unused slots
    const uint8_t* src = reinterpret_cast<const uint8_t*>(tabs + m0 * K);
    uint8_t* dst = reinterpret_cast<uint8_t*>(wave_tabs_lds<kSliceTabs>());
#pragma unroll
    for (int i = 0; i < kTabIter; ++i) {
      uint32_t idx = lane + 64u * i;
      if (idx >= tab_pieces) idx = tab_pieces - 1u;
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(src + idx * 16u),
                                       (__attribute__((address_space(3))) void*)(dst + i * 1024), 16, 0, 0);
    }
  }
  // kLds: survivors stream through a window of kWin loads in flight (survivor s + kWin is
  // loaded as survivor s is consumed), so K = 20 needs a third of the data VGPRs: 114 VGPRs,
  // 4 waves per SIMD at 1200 B (window 10: 153, 3 waves; 5-erasure decode 4.73 vs 4.28-4.50
  // TB/s, profiles/r01_probe_decode_window.txt).  The first window is in flight with the
  // table loads.
  constexpr bool kWinPath = kLds;
  constexpr int kWinW = 6;
  constexpr int kWin = kWinPath ? (K < kWinW ? K : kWinW) : K;
  uint32_t x[K][NW];
#pragma unroll
  for (int s = 0; s < kWin; ++s) load(shard(sid[s]), x[s]);
  if constexpr (kLds && (POL & kCoefBytes) != 0) {
    Tab* lt = wave_tabs_lds<kSliceTabs>();
    const uint32_t ncoef = tab_pieces / 2u;
#pragma unroll
    for (int j = 0; j < kCoefIter; ++j) {
      const uint32_t i = lane + 64u * j;
      if (i < ncoef) {
        const TabWords w = tab_words(coef[j]);
        lt[i] = Tab{w.t0lo, w.t0hi, w.t1lo, w.t1hi, w.t2, coef[j], 0u, 0u};
      }
    }
  }
  const Tab* rt = tabs + m0 * K;  // rows of this pass: entry (m, s) at rt[m * K + s]
  if constexpr (kWinPath) {
    const Tab* lt = rt;
    if constexpr (kLds) {
      // Wait for every load so far (vmcnt(0): the compiler may order the survivor loads
      // around the LDS loads, so no counted wait), then keep LDS reads below the wait.
      __builtin_amdgcn_s_waitcnt(0x0F70);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      lt = wave_tabs_lds<kSliceTabs>();
    }
    // Straight-line body per row count NR (no branch on the row index or the coefficient:
    // table values are VGPRs here, and the 0 / 1 entries are the zero / identity maps).
    auto rebuild = [&](auto nr_c) __attribute__((always_inline)) {
      constexpr int NR = decltype(nr_c)::value;
      uint32_t acc[NR][NW];
#pragma unroll
      for (int m = 0; m < NR; ++m)
#pragma unroll
        for (int q = 0; q < NW; ++q) acc[m][q] = 0;
#pragma unroll
      for (int s = 0; s < K; ++s) {
        // survivor s's selectors, table reads and the next window load stay in its
        // iteration (the compiler otherwise hoists them all: 472 VGPRs + AGPRs, one wave
        // per SIMD)
#pragma unroll
        for (int q = 0; q < NW; ++q) __asm__ volatile("" : "+v"(x[s][q]));
        __builtin_amdgcn_sched_barrier(0);
        if (s + kWin < K) load(shard(sid[s + kWin]), x[s + kWin]);  // folded when unrolled
        SelN<NW> sel;
        sel_split(x[s], sel);
#pragma unroll
        for (int m = 0; m < NR; ++m) {
          const Tab t = lt[m * K + s];
#pragma unroll
          for (int q = 0; q < NW; ++q) {
            acc[m][q] ^= gmul(sel.s0[q], sel.s1[q], sel.s2[q], t);
            // pin the accumulation order: reassociating the K-term XOR chains into trees
            // keeps every survivor's products live at once (spills)
            __asm__ volatile("" : "+v"(acc[m][q]));
          }
        }
      }
#pragma unroll
      for (int m = 0; m < NR; ++m) store(dest(m0 + m, erased(m0 + m)), acc[m]);
    };
    for_row_count<MAXE>(e - m0 < MAXE ? e - m0 : MAXE, rebuild);
    return;
  } else {
#pragma unroll
    for (int s = kWin; s < K; ++s) load(shard(sid[s]), x[s]);
  }
  uint32_t acc[MAXE][NW];
#pragma unroll
  for (int m = 0; m < MAXE; ++m)
#pragma unroll
    for (int q = 0; q < NW; ++q) acc[m][q] = 0;
#pragma unroll
  for (int s = 0; s < K; ++s) {
    // (sel_split here moves ten decode_fused instantiations: spelled out)
    uint32_t s0[NW], s1[NW], s2[NW];
#pragma unroll
    for (int q = 0; q < NW; ++q) {
      s0[q] = x[s][q] & 0x07070707u;
      s1[q] = (x[s][q] >> 3) & 0x07070707u;
      s2[q] = (x[s][q] >> 6) & 0x03030303u;
    }
#pragma unroll
    for (int m = 0; m < MAXE; ++m) {
      if (m0 + m < e) {
        const Tab& t = rt[m * K + s];
        if (t.coef == 1u) {
#pragma unroll
          for (int q = 0; q < NW; ++q) acc[m][q] ^= x[s][q];
        } else if (t.coef != 0u) {
#pragma unroll
          for (int q = 0; q < NW; ++q) acc[m][q] ^= gmul(s0[q], s1[q], s2[q], t);
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MAXE; ++m)
    if (m0 + m < e) store(dest(m0 + m, erased(m0 + m)), acc[m]);
}

template <int K, int MAXE, int POL, int NM, int NT, bool DIRECT = false, bool INLINE = DIRECT, int SCAN = 0>
__global__ __launch_bounds__(256) void decode_fused(const uint8_t* __restrict__ data,
                                                    const uint8_t* __restrict__ parity,
                                                    const uint32_t* __restrict__ rec_off,
                                                    const uint8_t* __restrict__ codebook,
                                                    uint64_t groups, uint32_t P, uint32_t r, uint32_t m0,
                                                    uint8_t* __restrict__ out, uint32_t never, uint32_t swz,
                                                    const uint64_t* __restrict__ masks, RankMeta rm,
                                                    uint8_t* __restrict__ status) {
  static_assert(!INLINE || (DIRECT && MAXE <= 3), "inline classify: mask-addressed forms with r <= 3");
  static_assert(SCAN == 0 || (DIRECT && INLINE && SCAN <= 64), "scan: mask-addressed inline forms, <= 64 groups per wave");
  extern __shared__ __attribute__((aligned(16))) uint8_t occupancy_lds[];  // see encode_v16
  if (never) occupancy_lds[threadIdx.x] = 0;
  const uint64_t wv = static_cast<uint64_t>(decode_block(swz)) * 4u +
                      static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
  const uint32_t lane = threadIdx.x & 63u;
  if constexpr (SCAN == 0) {
    if (wv >= groups) return;
    const uint64_t m = DIRECT ? masks[wv] : 0;
    fused_group<K, MAXE, POL, NM, NT, DIRECT, INLINE>(wv, m, lane, data, parity, rec_off, codebook, P, r, m0, out, rm,
                                                      status);
  } else {
    // SCAN groups per wave: lanes 0..SCAN-1 read the masks with one vector load and write
    // the status bytes; the groups with lost, recoverable data shards (a ballot) are then
    // rebuilt one after another by the whole wave.  Sparse loss (C5: ~10% of groups) costs
    // one wave per SCAN groups instead of one per group.
    const uint64_t g0 = wv * SCAN;
    if (g0 >= groups) return;
    uint64_t mv = 0;
    bool need = false;
    if (lane < static_cast<uint32_t>(SCAN) && g0 + lane < groups) {
      mv = masks[g0 + lane];
      // fec_mask.hpp's mask_losses / mask_rows, restated by hand as in fused_group
      constexpr uint64_t kmask = low_bits(K);
      const uint32_t ne = static_cast<uint32_t>(__popcll(mv & kmask));
      const bool bad = ne > r - static_cast<uint32_t>(__popcll((mv >> K) & ((1ull << r) - 1)));
      if (status != nullptr) status[g0 + lane] = bad ? 1 : 0;
      need = ne > 0 && !bad;
    }
    uint64_t work = __ballot(need);
    while (work) {
      const uint32_t b = static_cast<uint32_t>(__builtin_ctzll(work));
      work &= work - 1;
      const uint64_t m = (static_cast<uint64_t>(__builtin_amdgcn_readlane(static_cast<uint32_t>(mv >> 32), b)) << 32) |
                         __builtin_amdgcn_readlane(static_cast<uint32_t>(mv), b);
      fused_group<K, MAXE, POL, NM, NT, DIRECT, INLINE>(g0 + b, m, lane, data, parity, rec_off, codebook, P, r, m0,
                                                        out, rm, nullptr);
    }
  }
}

}  // namespace

// ---------------------------------------------------------------------------------
// Launchers: which form a call takes is decided in fec_forms.hpp; these only launch it.
// ---------------------------------------------------------------------------------
namespace {

template <int K, int MAXE, int POL, int NM, int NT, bool DIRECT = false, bool INLINE = DIRECT, int SCAN = 0>
hipError_t run_decode_fused(const DecodeLaunch& a, hipStream_t s) {
  constexpr uint64_t kGroupsPerBlock = 4u * (SCAN > 0 ? SCAN : 1);
  const uint32_t passes = (a.r + MAXE - 1) / MAXE;
  const uint32_t smem = occupancy_cap_lds(a.waves_per_cu ? a.waves_per_cu : knob(TestKnob::kDecodeWaves, kDecodeWavesPerCU), 4);
  const RankMeta rm = rank_meta(a.meta);
  // Output of the chunk starting at group g0: packed rows are placed by their global row
  // start (rec_off), so every chunk gets the base; the other layouts are offset per chunk.
  auto out_at = [&](uint64_t g0) -> uint8_t* {
    if (a.packed_rows) return a.out;
    return (a.out ? a.out : a.data) + g0 * ((POL & kCompactOut) != 0 ? a.r : a.k) * static_cast<uint64_t>(a.P);
  };
  for (uint32_t p = 0; p < passes; ++p) {
    const uint32_t m0 = p * MAXE;
    const hipError_t e = for_chunks(a.groups, max_wave_blocks() * kGroupsPerBlock, [&](uint64_t g0, uint64_t gn) {
      const uint64_t bn = (gn + kGroupsPerBlock - 1) / kGroupsPerBlock;
      LaunchRecord t = launch_record(LaunchForm::kDecodeFused, bn, 256, g0, gn);
      t.k = K, t.r = MAXE, t.nm = NM, t.nt = NT, t.pol = POL, t.direct = DIRECT, t.scan = SCAN, t.aux = m0;
      trace_launch(t);
      hipLaunchKernelGGL((decode_fused<K, MAXE, POL, NM, NT, DIRECT, INLINE, SCAN>), dim3(static_cast<uint32_t>(bn)), dim3(256), smem, s,
                         a.data + g0 * a.k * static_cast<uint64_t>(a.P),
                         a.parity + g0 * a.r * static_cast<uint64_t>(a.P), a.rec_off ? a.rec_off + g0 : nullptr, a.codebook, gn, a.P,
                         a.r, m0, out_at(g0), 0u, decode_swizzle(a, kDecodeFusedXcdSwizzle), DIRECT ? a.masks + g0 : nullptr, rm,
                         INLINE && a.status ? a.status + g0 : nullptr);
    });
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

// launch_decode's dispatch (fec_decode.hip) for f.kernel == DecodeKernel::kFused: one entry of
// fec_forms.hpp's QFEC_DECODE_FUSED_FORMS to its instantiation.
hipError_t launch_decode_fused(const DecodeLaunch& a, const DecodeForm& f, hipStream_t s) {
#define QFEC_FORM(KERNEL, KK, MM, NMM, NTT, PP, DD, SS)                                                             \
  if (f.kernel == DecodeKernel::KERNEL && f.K == KK && f.MAXE == MM && f.NM == NMM && f.NT == NTT && f.POL == (PP) && \
      f.DIRECT == DD && f.SCAN == static_cast<int>(SS))                                                             \
    return run_decode_fused<KK, MM, PP, NMM, NTT, DD, DD, SS>(a, s);
  QFEC_DECODE_FUSED_FORMS(QFEC_FORM)
#undef QFEC_FORM
  return hipErrorNotSupported;
}

hipError_t load_decode_fused_unit() {
  hipFuncAttributes at;
  return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(decode_fused<10, 3, kNtStore, 1, 1>));  // QFEC_RECORD_FORMS
}

}  // namespace qfec
