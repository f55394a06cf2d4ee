// fec_gather.hip — gfx950 kernels of fec_recover_gather_rs_dev: recover from shards wherever they
// are in device memory.  The caller hands over a table of absolute shard addresses, k + r per
// group (data shards, then parity rows; 0 = lost), instead of contiguous data / parity buffers
// and erasure masks.
//
//  * classify_gather: forms each group's erasure mask from its table entries (bit s set where
//    entry s is 0) and from it the status byte and the codebook record, exactly as `classify`
//    (fec_kernels.hip) does from a given mask.
//  * recover_gather<K, MAXE, POL>: one wave per group, record-addressed like decode_wave.  The
//    base address of the record's survivor s is the group's table entry of that shard id, fetched
//    once per group (compile-time k: scalar loads into SGPRs; runtime k: a per-wave LDS slice);
//    the packet is then walked as decode_wave walks it -- whole 1 KiB passes of 16 B per lane,
//    the remainder in 256-B passes of 4 B per lane, tail pieces shifted back to end at P -- and the
//    rebuilt rows go to the compact slot layout, out + (g * r + m) * P.
//
// Shards may have any byte alignment (unaligned 16-B / 4-B global access, as in fec_kernels.hip)
// and P >= 16.  A lost shard's entry and a parity row the decode rule does not use are never
// dereferenced: the record lists only the k survivors it rebuilds from.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fec_device.hpp"
#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_launch.hpp"

namespace qfec {
namespace {

// Workgroup of 256 lanes = 256 consecutive groups.  The groups' table entries are one
// contiguous run, read by consecutive lanes; a zero entry sets its bit in the group's mask in
// LDS.  Lane t then classifies group t like `classify`.
__global__ __launch_bounds__(256) void classify_gather(const uint64_t* __restrict__ addrs, uint64_t groups,
                                                       uint32_t k, uint32_t r,
                                                       const uint64_t* __restrict__ binom, LevelMeta meta,
                                                       uint32_t* __restrict__ rec_off,
                                                       uint8_t* __restrict__ status,
                                                       uint64_t* __restrict__ masks_out) {
  __shared__ unsigned long long lost[256];
  const uint64_t g0 = static_cast<uint64_t>(blockIdx.x) * 256u;
  const uint32_t gn = groups - g0 < 256u ? static_cast<uint32_t>(groups - g0) : 256u;
  const uint32_t n = k + r;
  lost[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t* __restrict__ tab = addrs + g0 * n;
  const uint32_t entries = gn * n;  // at most 256 * 64
  for (uint32_t i = threadIdx.x; i < entries; i += 256u) {
    if (tab[i] == 0) atomicOr(&lost[i / n], 1ull << (i % n));
  }
  __syncthreads();
  if (threadIdx.x >= gn) return;
  const uint64_t g = g0 + threadIdx.x;
  const uint64_t m = lost[threadIdx.x];
  const uint64_t kmask = (1ull << k) - 1;  // k + r <= 64 and r >= 1: k < 64
  const uint64_t rmask = (1ull << r) - 1;
  uint64_t dm = m & kmask;
  const uint64_t pm = (m >> k) & rmask;
  const uint32_t e = __popcll(dm);
  uint32_t rec = kRecNone;
  uint8_t st = 0;
  if (e > 0) {
    const uint32_t alive = r - __popcll(pm);
    if (e > alive) {
      rec = kRecBad;
      st = 1;
    } else {
      // colex ranks of the erased data set and of the e lowest surviving parity rows
      uint64_t rank_e = 0, rank_r = 0;
      for (uint32_t t = 0; dm; ++t) {
        const uint32_t j = __ffsll(static_cast<unsigned long long>(dm)) - 1;
        rank_e += binom[j * 65 + t + 1];
        dm &= dm - 1;
      }
      uint64_t sp = ~pm & rmask;
      for (uint32_t t = 0; t < e; ++t) {
        const uint32_t i = __ffsll(static_cast<unsigned long long>(sp)) - 1;
        rank_r += binom[i * 65 + t + 1];
        sp &= sp - 1;
      }
      const uint64_t idx = rank_e * meta.count_r[e] + rank_r;
      rec = static_cast<uint32_t>((meta.base[e] + idx * meta.stride[e]) >> 5);
    }
  }
  rec_off[g] = rec;
  if (status) status[g] = st;
  if (masks_out) masks_out[g] = m;
}

// A table entry as a packet pointer.  The entry is cast to a global-memory pointer first, so the
// loads through it are global loads; a pointer made straight from the integer would be generic
// (flat loads, which also count against the LDS / scalar counter).
__device__ __forceinline__ const uint8_t* shard_ptr(uint64_t addr) {
  typedef const __attribute__((address_space(1))) uint8_t* global_u8p;
  return (const uint8_t*)reinterpret_cast<global_u8p>(addr);
}

// Rebuild rows [m0, m0 + MAXE) of one group at byte offset `off` of every shard, NW dwords per
// lane (decode_piece of fec_kernels.hip with the survivors' bases from src(s)).  The tables
// are wave-uniform: SGPRs.  Rows go to the compact layout: row m at og + m * P.
template <int K, int MAXE, int POL, int NW, typename SRC>
__device__ __forceinline__ void gather_piece(const Tab* __restrict__ tabs, const SRC& src, uint8_t* __restrict__ og,
                                             uint32_t k, uint32_t P, uint32_t off, uint32_t e, uint32_t m0,
                                             bool xor_only) {
  // Runtime k: survivors in batches of kBatch loads in flight (slots past k re-load
  // survivor 0, a valid address, and are not used).
  constexpr uint32_t kBatch = 8;
  if (xor_only) {  // single data loss rebuilt from parity row 0: the reference XOR
    uint32_t acc[NW] = {};
    if constexpr (K > 0) {
      uint32_t x[K][NW];
#pragma unroll
      for (int s = 0; s < K; ++s) ldw<NW, POL>(src(s) + off, x[s]);
#pragma unroll
      for (int s = 0; s < K; ++s)
#pragma unroll
        for (int q = 0; q < NW; ++q) acc[q] ^= x[s][q];
    } else {
      for (uint32_t s0 = 0; s0 < k; s0 += kBatch) {
        uint32_t v[kBatch][NW];
#pragma unroll
        for (uint32_t b = 0; b < kBatch; ++b) ldw<NW, POL>(src(s0 + b < k ? s0 + b : 0) + off, v[b]);
#pragma unroll
        for (uint32_t b = 0; b < kBatch; ++b)
          if (s0 + b < k)
#pragma unroll
            for (int q = 0; q < NW; ++q) acc[q] ^= v[b][q];
      }
    }
    stw<NW, POL>(og + off, acc);
    return;
  }
  uint32_t acc[MAXE][NW];
#pragma unroll
  for (int m = 0; m < MAXE; ++m)
#pragma unroll
    for (int q = 0; q < NW; ++q) acc[m][q] = 0;
  auto consume = [&](const uint32_t (&v)[NW], uint32_t s, uint32_t kk) {
    uint32_t s0[NW], s1[NW], s2[NW];
#pragma unroll
    for (int q = 0; q < NW; ++q) {
      s0[q] = v[q] & 0x07070707u;
      s1[q] = (v[q] >> 3) & 0x07070707u;
      s2[q] = (v[q] >> 6) & 0x03030303u;
    }
#pragma unroll
    for (int m = 0; m < MAXE; ++m) {
      if (m0 + m < e) {
        const Tab& t = tabs[(m0 + m) * kk + s];
        if constexpr ((POL & kNoCoefBranch) != 0) {
          // coefficient 0 / 1 tables are the zero / identity maps: no branch on the value
#pragma unroll
          for (int q = 0; q < NW; ++q) acc[m][q] ^= gmul(s0[q], s1[q], s2[q], t);
        } else if (t.coef == 1u) {
#pragma unroll
          for (int q = 0; q < NW; ++q) acc[m][q] ^= v[q];
        } else if (t.coef != 0u) {
#pragma unroll
          for (int q = 0; q < NW; ++q) acc[m][q] ^= gmul(s0[q], s1[q], s2[q], t);
        }
      }
    }
  };
  if constexpr (K > 0) {
    uint32_t x[K][NW];
#pragma unroll
    for (int s = 0; s < K; ++s) ldw<NW, POL>(src(s) + off, x[s]);
#pragma unroll
    for (int s = 0; s < K; ++s) consume(x[s], s, K);
  } else {
    for (uint32_t s0 = 0; s0 < k; s0 += kBatch) {
      uint32_t v[kBatch][NW];
#pragma unroll
      for (uint32_t b = 0; b < kBatch; ++b) ldw<NW, POL>(src(s0 + b < k ? s0 + b : 0) + off, v[b]);
#pragma unroll
      for (uint32_t b = 0; b < kBatch; ++b)
        if (s0 + b < k) consume(v[b], s0 + b, k);
    }
  }
#pragma unroll
  for (int m = 0; m < MAXE; ++m) {
    if (m0 + m < e) stw<NW, POL>(og + (m0 + m) * static_cast<uint64_t>(P) + off, acc[m]);
  }
}

// The piece walk of decode_wave over one group.
template <int K, int MAXE, int POL, typename SRC>
__device__ __forceinline__ void gather_walk(const Tab* __restrict__ tabs, const SRC& src, uint8_t* __restrict__ og,
                                            uint32_t k, uint32_t P, uint32_t lane, uint32_t e, uint32_t m0,
                                            bool xor_only) {
  const uint32_t main_end = P & ~1023u;
  for (uint32_t base = 0; base < main_end; base += 1024u)
    gather_piece<K, MAXE, POL, 4>(tabs, src, og, k, P, base + lane * 16u, e, m0, xor_only);
  for (uint32_t base = main_end; base < P; base += 256u) {
    const uint32_t off = base + lane * 4u;
    gather_piece<K, MAXE, POL, 1>(tabs, src, og, k, P, off + 4u <= P ? off : P - 4u, e, m0, xor_only);
  }
}

// One wave per group (4 per workgroup).  K > 0: compile-time k, one pass of MAXE = r rows, the k
// survivor addresses in SGPRs.  K = 0: runtime k, rows [m0, m0 + MAXE) per launch, the addresses
// in the wave's LDS slice (64 entries: k + r <= 64).
template <int K, int MAXE, int POL>
__global__ __launch_bounds__(256) void recover_gather(const uint64_t* __restrict__ addrs,
                                                      const uint32_t* __restrict__ rec_off,
                                                      const uint8_t* __restrict__ codebook, uint64_t groups,
                                                      uint32_t P, uint32_t k_rt, uint32_t r, uint32_t m0,
                                                      uint8_t* __restrict__ out, uint32_t swz) {
  const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
  const uint64_t gw = static_cast<uint64_t>(decode_block(swz)) * 4u + wave;
  if (gw >= groups) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t rec = __builtin_amdgcn_readfirstlane(rec_off[gw]);
  if (rec >= kRecBad) return;
  const uint32_t k = K > 0 ? static_cast<uint32_t>(K) : k_rt;
  const uint8_t* recp = codebook + static_cast<uint64_t>(rec) * 32u;
  const uint32_t* rw = reinterpret_cast<const uint32_t*>(recp);
  const uint32_t e = rw[24] & 0xFFu;
  const bool xor_only = ((rw[24] >> 8) & 0xFFu) != 0;
  if (m0 >= e) return;
  const Tab* tabs = reinterpret_cast<const Tab*>(recp + 128);
  const uint64_t* __restrict__ ga = addrs + gw * (k + r);
  uint8_t* og = out + gw * r * static_cast<uint64_t>(P);
  if constexpr (K > 0) {
    const uint8_t* base[K];
#pragma unroll
    for (int s = 0; s < K; ++s) base[s] = shard_ptr(ga[rec_byte(rw, s)]);
    const auto src = [&base](int s) { return base[s]; };
    gather_walk<K, MAXE, POL>(tabs, src, og, k, P, lane, e, m0, xor_only);
  } else {
    __shared__ uint64_t slices[4 * 64];
    uint64_t* slice = slices + wave * 64u;
    if (lane < k) slice[lane] = ga[recp[lane]];  // survivor `lane` of the record
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const auto src = [slice](uint32_t s) { return shard_ptr(slice[s]); };
    gather_walk<K, MAXE, POL>(tabs, src, og, k, P, lane, e, m0, xor_only);
  }
}

hipError_t run_classify_gather(const GatherLaunch& a, hipStream_t s) {
  const uint64_t n = a.k + a.r;
  return for_chunks(a.groups, max_launch_threads(), [&](uint64_t g0, uint64_t gn) {
    trace_launch(launch_record(static_cast<int64_t>(GatherLaunchForm::kClassifyGather), blocks_for(gn), 256, g0, gn));
    hipLaunchKernelGGL(classify_gather, dim3(blocks_for(gn)), dim3(256), 0, s, a.addrs + g0 * n, gn, a.k, a.r,
                       a.binom, a.meta, a.rec_off + g0, a.status ? a.status + g0 : nullptr,
                       a.masks_out ? a.masks_out + g0 : nullptr);
  });
}

// Wave-per-group launches chunk their groups by whole workgroups, like the decodes.
template <int K, int MAXE, int POL>
hipError_t run_recover_gather(const GatherLaunch& a, hipStream_t s) {
  const uint32_t passes = (a.r + MAXE - 1) / MAXE;  // e <= r
  const uint64_t n = a.k + a.r;
  for (uint32_t p = 0; p < passes; ++p) {
    const uint32_t m0 = p * MAXE;
    const hipError_t e = for_chunks(a.groups, max_wave_blocks() * 4, [&](uint64_t g0, uint64_t gn) {
      const uint64_t bn = (gn + 3) / 4;
      LaunchRecord t = launch_record(static_cast<int64_t>(GatherLaunchForm::kRecoverGather), bn, 256, g0, gn);
      t.k = K, t.r = MAXE, t.pol = POL, t.aux = m0;
      trace_launch(t);
      hipLaunchKernelGGL((recover_gather<K, MAXE, POL>), dim3(static_cast<uint32_t>(bn)), dim3(256), 0, s,
                         a.addrs + g0 * n, a.rec_off + g0, a.codebook, gn, a.P, a.k, a.r, m0,
                         a.out + g0 * a.r * static_cast<uint64_t>(a.P), static_cast<uint32_t>(kDecodeWaveXcdSwizzle));
    });
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

// Which form runs is decided in fec_forms.hpp (gather_form); this only launches it.
hipError_t launch_recover_gather(const GatherLaunch& a, hipStream_t s) {
  if (a.groups == 0) return hipSuccess;
  const GatherForm f = gather_form(a.k, a.r, a.P);
  if (!f.supported) return hipErrorInvalidValue;
  hipError_t (*run)(const GatherLaunch&, hipStream_t) = nullptr;
#define QFEC_GATHER(KK, MM, PP) \
  if (f.K == KK && f.MAXE == MM && f.POL == (PP)) run = run_recover_gather<KK, MM, PP>;
  QFEC_GATHER_FORMS(QFEC_GATHER)
#undef QFEC_GATHER
  if (run == nullptr) return hipErrorNotSupported;
  const hipError_t e = run_classify_gather(a, s);
  return e != hipSuccess ? e : run(a, s);
}

}  // namespace qfec
