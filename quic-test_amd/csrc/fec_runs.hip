// fec_runs.hip — gfx950 (MI355X, CDNA4) kernels of libfec_hip: the packed recover's rows.
//
//  * recover_runs<K,R,NM,NT,...>: the packed recover in one launch (fec_recover_batch_rs_dev_packed):
//    a workgroup classifies a tile of groups, finds its run's first row by decoupled look-back and
//    rebuilds its rows through an LDS image of the run.  Mask-addressed, decode_fused's INLINE
//    arithmetic; like it, the kernel keeps its own hand-written statement of fec_mask.hpp's rule
//    (profiles/mask_rule/VERDICT.md) and shares ChooseSmall, low_bits and piece_load only.
//  * rows_block_sums, rows_scan_blocks, rows_write: row_start[g], the exclusive prefix sum of the
//    rows every group rebuilds, for the two-step packed recover (then decode_fused's compact
//    forms, fec_decode_fused.hip).  Cold kernels: they call fec_mask.hpp's mask_rows.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fec_device.hpp"  // Tab, st16, gmul, piece_load, SelN / sel_split, RankMeta; fec_mask.hpp: low_bits,
                           // ChooseSmall, mask_rows
#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_launch.hpp"  // launch limits, for_chunks, launch_record, knob, rank_meta
#include "fec_scan.hpp"    // block_inclusive_scan, block_sum

namespace qfec {
namespace {

// ---------------------------------------------------------------------------------
// Packed recover in one launch: recover_runs (fec_recover_batch_rs_dev_packed; DESIGN.md §5,
// round 4).  The reference decoder hands rebuilt packets back as separate buffers
// (decoder.go:16-22 `Recovered`, listed at :195-207); the packed list puts all of a batch's rebuilt packets back
// to back, group g's from row row_start[g] (exclusive prefix sum of the rows every group
// rebuilds: its lost data shards when recoverable, else 0).
//
// A workgroup owns a tile of consecutive groups (one erasure mask per thread), so all of
// their rebuilt rows form ONE contiguous run of the packed list:
//  1. every thread classifies its group (status byte; rows), the block scans the rows and
//     lists the groups to rebuild in LDS, in group order;
//  2. wave 0 finds the run's first row by decoupled look-back over the blocks before it
//     (blocks take their tile from an atomic ticket, so every block one waits on has
//     started and publishes its own row count before it waits on anything) and publishes
//     its inclusive prefix; row_start[g] is written for every group.  No prefix launches;
//  3. the 4 waves rebuild the listed groups (mask-addressed, exactly decode_fused's INLINE
//     arithmetic) into an LDS image of the run; rows past the image's capacity (dense loss)
//     are stored straight to HBM;
//  4. the block copies the image out with 16-B stores by consecutive threads, so the run
//     leaves as whole 128-B lines except at its two ends -- instead of every 1.2-KB row being
//     stored by its own wave with partial lines at both ends.
// Look-back words: epoch (bits 34..63) | flag (bits 32..33: kRunAgg, kRunIncl) | rows.  The
// epoch is the launch's, so words left by earlier launches never match (no reset launch).
// ---------------------------------------------------------------------------------
constexpr uint64_t kRunAgg = 1ull << 32;
constexpr uint64_t kRunIncl = 2ull << 32;
constexpr uint32_t kRunEpochShift = 34;

// One group's rebuild of recover_runs, in two stages: runs_load issues the survivor loads and
// finds the record, runs_compute forms the rows.  Same survivor choice, record and arithmetic as
// fused_group's DIRECT + INLINE path (the rule of fec_mask.hpp).
// (one function for both stages moves all 36 recover_runs instantiations, and so does colex_rank
// or for_each_chosen in place of the loops below: two stages, the rule restated by hand.  Not
// checked on the CPU: the GPU tests check this copy, tests/test_gpu_forms.py test_every_mask clean
// and with junk in the mask bits at and above k + r, and the packed cases, whose masks all carry
// such junk -- that is what holds `& kmask` and `& rmask` here and in the kernel's classify)
struct RunMeta {
  const Tab* tabs;
  uint32_t e;
  bool xor_only;
};

template <int K, int R, int NM, int NT, int POL>
__device__ __forceinline__ RunMeta runs_load(uint64_t g, uint64_t m, uint32_t lane, const uint8_t* __restrict__ data,
                                             const uint8_t* __restrict__ parity, const uint8_t* __restrict__ codebook,
                                             const RankMeta& rm, uint32_t P, const uint32_t (&toff)[NT > 0 ? NT : 1],
                                             uint32_t (&x)[K][4 * NM + NT]) {
  constexpr uint64_t kmask = low_bits(K);
  constexpr uint64_t rmask = low_bits(R);
  const uint64_t lost = m & kmask;
  const uint32_t e = static_cast<uint32_t>(__popcll(lost));
  const uint64_t pm = (m >> K) & rmask;
  uint64_t rank_e = 0, rank_r = 0, rsel = 0;
  {
    uint64_t dm = lost;
    for (uint32_t t = 0; dm; ++t) {
      rank_e += ChooseSmall{}(static_cast<uint32_t>(__builtin_ctzll(dm)), t + 1u);
      dm &= dm - 1;
    }
    uint64_t sp = ~pm & rmask;
    for (uint32_t t = 0; t < e; ++t) {
      const uint32_t bit = static_cast<uint32_t>(__builtin_ctzll(sp));
      rank_r += ChooseSmall{}(bit, t + 1u);
      rsel |= 1ull << bit;
      sp &= sp - 1;
    }
  }
  RunMeta mt;
  mt.e = e;
  mt.xor_only = e == 1 && (pm & 1u) == 0;
  mt.tabs = reinterpret_cast<const Tab*>(codebook + rm.base[e] + (rank_e * rm.count_r[e] + rank_r) * rm.stride[e] + 128);
  uint64_t surv = (~lost & kmask) | (rsel << K);
  const uint8_t* dg = data + g * K * static_cast<uint64_t>(P);
  const uint8_t* pg = parity + g * R * static_cast<uint64_t>(P);
#pragma unroll
  for (int s = 0; s < K; ++s) {
    const uint32_t sid = static_cast<uint32_t>(__builtin_ctzll(surv));
    surv &= surv - 1;
    const uint8_t* src = sid < K ? dg + sid * static_cast<uint64_t>(P) : pg + (sid - K) * static_cast<uint64_t>(P);
    piece_load<NM, NT, POL>(src, lane, toff, x[s]);
  }
  return mt;
}

template <int K, int R, int NM, int NT>
__device__ __forceinline__ void runs_compute(const RunMeta& mt, uint32_t (&x)[K][4 * NM + NT], uint32_t (&acc)[R][4 * NM + NT]) {
  constexpr int NW = 4 * NM + NT;
#pragma unroll
  for (int mm = 0; mm < R; ++mm)
#pragma unroll
    for (int q = 0; q < NW; ++q) acc[mm][q] = 0;
  if (mt.xor_only) {  // single data loss rebuilt from parity row 0: the reference XOR
#pragma unroll
    for (int s = 0; s < K; ++s)
#pragma unroll
      for (int q = 0; q < NW; ++q) acc[0][q] ^= x[s][q];
    return;
  }
#pragma unroll
  for (int s = 0; s < K; ++s) {
    // survivor s's selectors stay in its iteration (left alone, LLVM hoists every survivor's
    // selectors ahead of the arithmetic: 160 VGPRs, 3 waves per SIMD; see decode_fused kLdsTabs)
#pragma unroll
    for (int q = 0; q < NW; ++q) __asm__ volatile("" : "+v"(x[s][q]));
    SelN<NW> sel;
    sel_split(x[s], sel);
#pragma unroll
    for (int mm = 0; mm < R; ++mm) {
      if (static_cast<uint32_t>(mm) < mt.e) {
        const Tab& t = mt.tabs[mm * K + s];
        if (t.coef == 1u) {
#pragma unroll
          for (int q = 0; q < NW; ++q) acc[mm][q] ^= x[s][q];
        } else if (t.coef != 0u) {
#pragma unroll
          for (int q = 0; q < NW; ++q) acc[mm][q] ^= gmul(sel.s0[q], sel.s1[q], sel.s2[q], t);
        }
      }
    }
  }
}

// recover_runs (probe form): the run image leaves by plain stores while rows past the image keep
// the POL's store policy.
constexpr int kRunImgPlain = 32768;

// stage_bytes: dynamic LDS of the run image (0: every row straight to HBM).  The image is used
// only when P % 16 == 0 and `out` is 16-B aligned (the launcher passes 0 otherwise), so row
// starts in the image and in HBM are 16-B aligned alike.
// base_in (nullable): rows before this launch (chunked launches: the previous chunk's total).
// POL: kNtLoad for the survivor loads, kNtStore for the row stores.  WAVES: waves per workgroup;
// TG: groups per workgroup (<= 64 * WAVES: the first TG threads classify one group each).
// flags bit 0 (probes only): no row stores at all.
template <int K, int R, int NM, int NT, int POL, int WAVES, int TG = 64 * WAVES>
__global__ __launch_bounds__(64 * WAVES) void recover_runs(const uint8_t* __restrict__ data,
                                                    const uint8_t* __restrict__ parity,
                                                    const uint64_t* __restrict__ masks, uint64_t groups,
                                                    uint32_t P, const uint8_t* __restrict__ codebook, RankMeta rm,
                                                    uint8_t* __restrict__ out, uint32_t* __restrict__ row_start,
                                                    uint8_t* __restrict__ status, uint64_t* __restrict__ lb,
                                                    uint32_t* __restrict__ ticket, uint32_t epoch,
                                                    uint32_t stage_bytes, const uint64_t* __restrict__ base_in,
                                                    uint64_t* __restrict__ total_out, uint64_t* __restrict__ total_user,
                                                    uint32_t flags) {
  static_assert(R <= 3, "mask-addressed shapes: r <= 3");
  static_assert(TG <= 64 * WAVES && (TG % 64 == 0 || TG < 64), "one classifying thread per group");
  constexpr uint32_t kTile = TG;
  constexpr uint32_t kScanWaves = TG >= 64 ? TG / 64 : 1;
  constexpr int NW = 4 * NM + NT;
  constexpr uint64_t kmask = low_bits(K);
  constexpr uint64_t rmask = low_bits(R);
  extern __shared__ __attribute__((aligned(16))) uint8_t run_image[];
  __shared__ uint64_t s_mask[kTile];
  __shared__ uint32_t s_item[kTile];  // (local group << 16) | first row in the run
  __shared__ uint32_t s_wrows[kScanWaves], s_wwork[kScanWaves];
  __shared__ uint32_t s_tile, s_first;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(tid >> 6));
  if (tid == 0) {
    const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // every ticket of this launch is taken: the counter starts from 0 for the next launch
    // (which the stream orders after this one)
    if (t == gridDim.x - 1u) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_tile = t;
  }
  __syncthreads();
  const uint32_t tile = s_tile;
  const uint64_t g = static_cast<uint64_t>(tile) * kTile + tid;
  uint64_t m = 0;
  uint32_t rows = 0;
  if (tid < kTile && g < groups) {
    m = masks[g];
    // fec_mask.hpp's mask_losses / mask_rows, restated by hand (called, they move every recover_runs)
    const uint32_t ne = static_cast<uint32_t>(__popcll(m & kmask));
    const bool bad = ne > R - static_cast<uint32_t>(__popcll((m >> K) & rmask));
    if (status != nullptr) status[g] = bad ? 1 : 0;
    rows = ne > 0 && !bad ? ne : 0u;
  }
  uint32_t incl = rows;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t v = __shfl_up(incl, d, 64);
    if (lane >= d) incl += v;
  }
  const uint64_t need = __ballot(rows != 0u);
  if (wave < kScanWaves) {
    if (lane == 63u) s_wrows[wave] = incl;
    if (lane == 0u) s_wwork[wave] = static_cast<uint32_t>(__popcll(need));
  }
  __syncthreads();
  uint32_t wrow = 0, witem = 0, A = 0, nwork = 0;
#pragma unroll
  for (uint32_t w = 0; w < kScanWaves; ++w) {
    if (w < wave) {
      wrow += s_wrows[w];
      witem += s_wwork[w];
    }
    A += s_wrows[w];
    nwork += s_wwork[w];
  }
  const uint32_t lrow = wrow + incl - rows;  // the group's first row inside the run
  if (rows != 0u) {
    const uint32_t i = witem + static_cast<uint32_t>(__popcll(need & ((1ull << lane) - 1)));
    s_mask[i] = m;
    s_item[i] = (tid << 16) | lrow;
  }
  // The run's first row (wave 0): decoupled look-back over the tiles before this one.
  auto find_first = [&]() {
    const uint64_t tag = static_cast<uint64_t>(epoch) << kRunEpochShift;
    const uint32_t base = base_in != nullptr ? static_cast<uint32_t>(*base_in) : 0u;
    uint32_t excl = 0;
    if (tile == 0) {
      excl = base;  // published with its row count below
    } else {
      int64_t pos = static_cast<int64_t>(tile) - 1;
      for (;;) {
        const int64_t idx = pos - static_cast<int64_t>(lane);
        uint64_t s = tag | kRunIncl | base;  // "before tile 0": the rows before this launch
        if (idx >= 0) {
          for (;;) {
            s = __hip_atomic_load(&lb[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((s >> kRunEpochShift) == epoch && (s & (kRunAgg | kRunIncl)) != 0) break;
            __builtin_amdgcn_s_sleep(1);
          }
        }
        const uint64_t inc = __ballot((s & kRunIncl) != 0);
        const uint32_t stop = inc ? static_cast<uint32_t>(__builtin_ctzll(inc)) : 64u;
        uint32_t v = lane <= stop ? static_cast<uint32_t>(s) : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        excl += v;
        if (inc) break;
        pos -= 64;
      }
      if (lane == 0) __hip_atomic_store(&lb[tile], tag | kRunIncl | (excl + A), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (lane == 0) {
      s_first = excl;
      if (tile == gridDim.x - 1u) {
        if (total_out != nullptr) *total_out = static_cast<uint64_t>(excl) + A;
        if (total_user != nullptr) *total_user = static_cast<uint64_t>(excl) + A;
      }
    }
  };
  // Publish this tile's row count at once (successors look back through it), then find the run's
  // first row: before the rebuild when some rows go straight to HBM (they need their place), after
  // it when every row fits the LDS image -- the look-back's wait then hides behind the rebuild.
  const uint32_t cap_rows = stage_bytes / P;
  const bool defer = (flags & 1u) == 0 && A <= cap_rows;
  // (tile 0 knows its first row already: the rows before this launch)
  if (wave == 0 && lane == 0) {
    const uint64_t tag = static_cast<uint64_t>(epoch) << kRunEpochShift;
    const uint64_t w = tile == 0 ? tag | kRunIncl | ((base_in != nullptr ? static_cast<uint32_t>(*base_in) : 0u) + A)
                                 : tag | kRunAgg | A;
    __hip_atomic_store(&lb[tile], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!defer && wave == 0) find_first();
  __syncthreads();
  uint32_t toff[NT > 0 ? NT : 1];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    toff[t] = NM * 1024u + t * 256u + lane * 4u;
    if (toff[t] + 4u > P) toff[t] = P - 4u;
  }
  auto item_of = [&](uint32_t i, uint64_t& gi, uint64_t& mw, uint32_t& r0) {
    const uint64_t mi = s_mask[i];
    mw = (static_cast<uint64_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(mi >> 32))) << 32) |
         __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(mi));
    const uint32_t item = __builtin_amdgcn_readfirstlane(s_item[i]);
    gi = static_cast<uint64_t>(tile) * kTile + (item >> 16);
    r0 = item & 0xFFFFu;
  };
  for (uint32_t i = wave; i < nwork; i += WAVES) {
    uint64_t gi, mw;
    uint32_t r0;
    item_of(i, gi, mw, r0);
    uint32_t acc[R][NW], x[K][NW];
    const RunMeta mt = runs_load<K, R, NM, NT, POL>(gi, mw, lane, data, parity, codebook, rm, P, toff, x);
    runs_compute<K, R, NM, NT>(mt, x, acc);
    const uint32_t e = mt.xor_only ? 1u : mt.e;
    if (flags & 1u) continue;  // probe: reads and arithmetic only
#pragma unroll
    for (int mm = 0; mm < R; ++mm) {
      if (static_cast<uint32_t>(mm) < e) {
        const uint32_t row = r0 + mm;
        if (row < cap_rows) {  // into the run image (16-B aligned rows: see stage_bytes)
          uint8_t* dst = run_image + row * P;
#pragma unroll
          for (int q = 0; q < NM; ++q)
            *reinterpret_cast<u32x4*>(dst + q * 1024u + lane * 16u) =
                u32x4{acc[mm][4 * q], acc[mm][4 * q + 1], acc[mm][4 * q + 2], acc[mm][4 * q + 3]};
#pragma unroll
          for (int t = 0; t < NT; ++t) *reinterpret_cast<uint32_t*>(dst + toff[t]) = acc[mm][4 * NM + t];
        } else {  // past the image (never when defer): straight to the row's place
          uint8_t* dst = out + (static_cast<uint64_t>(s_first) + row) * P;
#pragma unroll
          for (int q = 0; q < NM; ++q)
            st16<POL>(dst + q * 1024u + lane * 16u,
                      u32x4{acc[mm][4 * q], acc[mm][4 * q + 1], acc[mm][4 * q + 2], acc[mm][4 * q + 3]});
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            if constexpr ((POL & kNtStore) != 0) __builtin_nontemporal_store(acc[mm][4 * NM + t], reinterpret_cast<u32u*>(dst + toff[t]));
            else *reinterpret_cast<u32u*>(dst + toff[t]) = acc[mm][4 * NM + t];
          }
        }
      }
    }
  }
  if (defer) {
    __syncthreads();  // (the image is complete, too)
    if (wave == 0) find_first();
  }
  __syncthreads();
  const uint32_t first = s_first;
  if (tid < kTile && g < groups) row_start[g] = first + lrow;
  const uint32_t staged = (flags & 1u) ? 0u : (A < cap_rows ? A : cap_rows);
  if (staged == 0u) return;
  // the image leaves in 16-B pieces by consecutive threads: whole lines but at the run's ends
  uint8_t* run = out + static_cast<uint64_t>(first) * P;
  const uint32_t n16 = staged * P / 16u;
  constexpr int kImgPol = (POL & kRunImgPlain) != 0 ? (POL & ~kNtStore) : POL;
  for (uint32_t c = tid; c < n16; c += 64u * WAVES)
    st16<kImgPol>(run + c * 16u, *reinterpret_cast<const u32x4*>(run_image + c * 16u));
}

// Packed recover rows: row_start[g] = exclusive prefix sum over groups of the number of rows a
// group rebuilds (its lost data shards when recoverable, else 0).  Block sums of kRowsPerBlock
// groups first; then every block of rows_write adds up the sums of the blocks before it itself
// (at most kRowsDirectBlocks of them: two launches in all), or, past that, a one-block scan of
// the sums runs in between.  rocprof at C5 (1M groups): the first form with 4096-group blocks
// took 23 us in three launches (rows_write 11.5, block sums 6.9, one-block scan 4.9).
constexpr uint32_t kRowsPerThread = 4;
// thread_rows loads the masks as one u64x4 and the scans add rows[0..3]
static_assert(kRowsPerThread == 4, "thread_rows and the rows_* kernels are written for 4 groups per thread");
constexpr uint32_t kRowsPerBlock = 256 * kRowsPerThread;
constexpr uint32_t kRowsDirectBlocks = 4096;
// (block_inclusive_scan and block_sum: fec_scan.hpp, shared with the prefix over four-word masks,
// fec_packed.hip, which takes the same block and the same limit from fec_forms.hpp)
static_assert(kRowsPerBlock == kPackedRowsPerBlock && kRowsDirectBlocks == kPackedRowsDirectBlocks,
              "fec_forms.hpp states the prefix's block and its two-launch limit for fec_packed.hip and host-only code");

// The rows of a thread's kRowsPerThread consecutive groups (one 32-B load of their masks when
// they are all in range).
__device__ __forceinline__ void thread_rows(const uint64_t* __restrict__ masks, uint64_t groups, uint64_t g0,
                                            uint32_t k, uint32_t r, uint32_t (&rows)[kRowsPerThread]) {
  if (g0 + kRowsPerThread <= groups) {
    typedef uint64_t u64x4 __attribute__((ext_vector_type(4), aligned(8)));  // masks may be 8-B aligned
    const u64x4 m = *reinterpret_cast<const u64x4*>(masks + g0);
    rows[0] = mask_rows(m.x, k, r);
    rows[1] = mask_rows(m.y, k, r);
    rows[2] = mask_rows(m.z, k, r);
    rows[3] = mask_rows(m.w, k, r);
  } else {
    for (uint32_t i = 0; i < kRowsPerThread; ++i) rows[i] = g0 + i < groups ? mask_rows(masks[g0 + i], k, r) : 0u;
  }
}

__global__ __launch_bounds__(256) void rows_block_sums(const uint64_t* __restrict__ masks, uint64_t groups, uint32_t k,
                                                       uint32_t r, uint32_t* __restrict__ block_sums) {
  __shared__ uint32_t lds[4];
  const uint64_t g0 = static_cast<uint64_t>(blockIdx.x) * kRowsPerBlock + threadIdx.x * kRowsPerThread;
  uint32_t rows[kRowsPerThread];
  thread_rows(masks, groups, g0, k, r, rows);
  const uint32_t total = block_sum(rows[0] + rows[1] + rows[2] + rows[3], lds);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// One block: block_sums[0, nb) -> exclusive prefix sums, in place; *total = the sum.
__global__ __launch_bounds__(256) void rows_scan_blocks(uint32_t* __restrict__ block_sums, uint32_t nb,
                                                        uint64_t* __restrict__ total) {
  __shared__ uint32_t lds[256];
  uint32_t carry = 0;
  for (uint32_t b0 = 0; b0 < nb; b0 += 256) {
    const uint32_t i = b0 + threadIdx.x;
    const uint32_t v = i < nb ? block_sums[i] : 0u;
    const uint32_t incl = block_inclusive_scan(v, lds);
    if (i < nb) block_sums[i] = carry + incl - v;
    carry += lds[255];
    __syncthreads();
  }
  if (threadIdx.x == 0 && total != nullptr) *total = carry;
}

// DIRECT: block_sums holds the blocks' own sums; each block adds up those before it (and the
// last block writes the total).  Else block_sums holds exclusive offsets (rows_scan_blocks).
template <bool DIRECT>
__global__ __launch_bounds__(256) void rows_write(const uint64_t* __restrict__ masks, uint64_t groups, uint32_t k,
                                                  uint32_t r, const uint32_t* __restrict__ block_sums,
                                                  uint32_t* __restrict__ row_start, uint64_t* __restrict__ total) {
  __shared__ uint32_t lds[256];
  uint32_t base;
  if constexpr (DIRECT) {
    uint32_t part = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += 256) part += block_sums[b];
    base = block_sum(part, lds);
  } else {
    base = block_sums[blockIdx.x];
  }
  const uint64_t g0 = static_cast<uint64_t>(blockIdx.x) * kRowsPerBlock + threadIdx.x * kRowsPerThread;
  uint32_t rows[kRowsPerThread];
  thread_rows(masks, groups, g0, k, r, rows);
  const uint32_t sum = rows[0] + rows[1] + rows[2] + rows[3];
  const uint32_t incl = block_inclusive_scan(sum, lds);
  uint32_t at = base + incl - sum;
  for (uint32_t i = 0; i < kRowsPerThread; ++i) {
    if (g0 + i < groups) row_start[g0 + i] = at;
    at += rows[i];
  }
  if constexpr (DIRECT) {
    if (total != nullptr && blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) *total = base + incl;
  }
}

}  // namespace

// ---------------------------------------------------------------------------------
// Launchers: which form a call takes is decided in fec_forms.hpp; these only launch it.
// ---------------------------------------------------------------------------------
uint64_t rows_prefix_workspace_bytes(uint64_t groups) {
  return ((groups + kRowsPerBlock - 1) / kRowsPerBlock) * sizeof(uint32_t);
}

hipError_t launch_rows_prefix(const uint64_t* masks, uint64_t groups, uint32_t k, uint32_t r, uint32_t* row_start,
                              uint32_t* block_sums, uint64_t* total, hipStream_t s) {
  if (groups == 0) return hipSuccess;
  const uint64_t nb = (groups + kRowsPerBlock - 1) / kRowsPerBlock;
  if (nb > 0xFFFFFFFFull) return hipErrorInvalidValue;
  // the two-launch form's block limit (the test library's TestKnob::kRowsDirectBlocks forces the other form)
  const uint64_t direct_max = static_cast<uint64_t>(knob(TestKnob::kRowsDirectBlocks, kRowsDirectBlocks));
  const dim3 grid(static_cast<uint32_t>(nb));
  const bool direct = nb <= direct_max;
  {
    trace_launch(launch_record(LaunchForm::kRowsBlockSums, nb, 256, 0, groups));
    if (!direct) trace_launch(launch_record(LaunchForm::kRowsScanBlocks, 1, 256, 0, groups));
    LaunchRecord t = launch_record(LaunchForm::kRowsWrite, nb, 256, 0, groups);
    t.direct = direct;
    trace_launch(t);
  }
  hipLaunchKernelGGL(rows_block_sums, grid, dim3(256), 0, s, masks, groups, k, r, block_sums);
  if (direct) {
    hipLaunchKernelGGL(rows_write<true>, grid, dim3(256), 0, s, masks, groups, k, r, block_sums, row_start, total);
  } else {
    hipLaunchKernelGGL(rows_scan_blocks, dim3(1), dim3(256), 0, s, block_sums, static_cast<uint32_t>(nb), total);
    hipLaunchKernelGGL(rows_write<false>, grid, dim3(256), 0, s, masks, groups, k, r, block_sums, row_start,
                       nullptr);
  }
  return hipGetLastError();
}

// rows_scan_blocks alone, for the prefix over four-word masks (fec_packed.hip): the one-block scan of
// block sums does not read a mask.
hipError_t launch_rows_scan_blocks(uint32_t* block_sums, uint64_t blocks, uint64_t groups, uint64_t* total, hipStream_t s) {
  if (block_sums == nullptr || blocks == 0 || blocks > 0xFFFFFFFFull) return hipErrorInvalidValue;
  trace_launch(launch_record(LaunchForm::kRowsScanBlocks, 1, 256, 0, groups));
  hipLaunchKernelGGL(rows_scan_blocks, dim3(1), dim3(256), 0, s, block_sums, static_cast<uint32_t>(blocks), total);
  return hipGetLastError();
}

namespace {

// The library's form: 8 waves per workgroup, 512 groups per tile, NT loads and stores (tools/
// probe_runs.hip over four boxes, C5: 0.229-0.251 ms vs 0.241-0.268 for the slot rows and
// 0.241-0.262 for the two-step packed rows; 4 waves x 256 groups 0.247-0.253; profiles/r04_probe_runs_*.txt).
constexpr int kRunWaves = 8;
constexpr uint32_t kRunGroups = 64u * kRunWaves;

uint64_t runs_blocks_per_launch(uint64_t groups) {
  const uint64_t nb = (groups + kRunGroups - 1) / kRunGroups;
  const uint64_t mb = max_wave_blocks();
  return nb < mb ? nb : mb;
}

// The tile recover's row stores are non-temporal.  Back-to-back recovers alone favour plain
// stores by 10-15% on round 5's boxes (profiles/r05c, r05e, r05i probe_runs_c5.txt), but there
// the 0.13 GB of rows stay in the Infinity Cache from one launch to the next (the form's time
// equals its no-store floor); in the bench's step, after the encode's 15.6 GB, the two policies
// recover in the same 0.254 ms and the plain rows' write-back lands in the next encode (+0.01 ms;
// profiles/r05j/ab_legs.jsonl).
template <int K, int R, int NM, int NT, int POL = kNtLoad | kNtStore>
hipError_t run_recover_runs(const RunsLaunch& a, uint32_t stage, hipStream_t s) {
  const RankMeta rm = rank_meta(a.meta);
  uint8_t* ws = static_cast<uint8_t*>(a.workspace);
  uint32_t* ticket = reinterpret_cast<uint32_t*>(ws);
  const uint64_t per = runs_blocks_per_launch(a.groups) * kRunGroups;
  const uint32_t launches = runs_launches(a.groups);
  uint64_t* totals = reinterpret_cast<uint64_t*>(ws + 64);
  uint64_t* lb = reinterpret_cast<uint64_t*>(ws + 64 + 8 * static_cast<uint64_t>(launches));
  return for_chunks(a.groups, per, [&](uint64_t g0, uint64_t gn) {
    const uint32_t c = static_cast<uint32_t>(g0 / per);  // this launch of `launches`
    const uint32_t nb = static_cast<uint32_t>((gn + kRunGroups - 1) / kRunGroups);
    LaunchRecord t = launch_record(LaunchForm::kRecoverRuns, nb, 64 * kRunWaves, g0, gn);
    t.k = K, t.r = R, t.nm = NM, t.nt = NT, t.pol = POL, t.tile = kRunGroups, t.aux = stage;
    trace_launch(t);
    hipLaunchKernelGGL((recover_runs<K, R, NM, NT, POL, kRunWaves>), dim3(nb), dim3(64 * kRunWaves), stage, s, a.data + g0 * K * static_cast<uint64_t>(a.P),
                       a.parity + g0 * R * static_cast<uint64_t>(a.P), a.masks + g0, gn, a.P, a.codebook, rm, a.out,
                       a.row_start + g0, a.status ? a.status + g0 : nullptr, lb, ticket, a.epoch + c, stage,
                       c > 0 ? totals + (c - 1) : nullptr, totals + c, c + 1 == launches ? a.total : nullptr, 0u);
  });
}

}  // namespace

uint32_t runs_launches(uint64_t groups) {
  if (groups == 0) return 0;
  const uint64_t per = runs_blocks_per_launch(groups) * kRunGroups;
  return static_cast<uint32_t>((groups + per - 1) / per);
}

uint64_t runs_workspace_bytes(uint64_t groups) {
  return 64 + 8 * static_cast<uint64_t>(runs_launches(groups)) + 8 * runs_blocks_per_launch(groups);
}

uint32_t runs_stage_bytes(const RunsLaunch& a) {
  // the run image needs 16-B aligned row starts in LDS and in HBM
  if (a.P % 16u != 0 || reinterpret_cast<uintptr_t>(a.out) % 16u != 0) return 0;
  const int v = a.stage_bytes >= 0 ? a.stage_bytes : knob(TestKnob::kRunsStage, kRunsStageBytes);
  if (v <= 0) return 0;
  const uint32_t cap = 64u * 1024u;  // dynamic LDS per workgroup (160 KiB per CU)
  return static_cast<uint32_t>(v) < cap ? static_cast<uint32_t>(v) : cap;
}

hipError_t launch_recover_runs(const RunsLaunch& a, hipStream_t s) {
  if (a.groups == 0) return hipSuccess;
  if (a.workspace == nullptr || a.row_start == nullptr || a.out == nullptr || a.masks == nullptr) return hipErrorInvalidValue;
  if (!runs_supported(a.k, a.r, a.P)) return hipErrorNotSupported;
  const Layout lay = layout_of(a.P);
#define QFEC_RUNS(KK, RR, NMM, NTT) \
  if (a.k == KK && a.r == RR && lay.nm == NMM && lay.nt == NTT) return run_recover_runs<KK, RR, NMM, NTT>(a, runs_stage_bytes(a), s);
  QFEC_RUNS_FORMS(QFEC_RUNS)
#undef QFEC_RUNS
  return hipErrorNotSupported;
}

hipError_t load_runs_unit() {
  hipFuncAttributes at;
  return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(rows_block_sums));
}

}  // namespace qfec
