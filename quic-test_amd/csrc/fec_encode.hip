// fec_encode.hip — gfx950 (MI355X, CDNA4) kernels of libfec_hip: the contiguous encodes.
//
// Hot path (SURVEY.md §8(a) a1/a4 and the new GF rows): batched systematic erasure
// encode of QUIC packet groups.  Byte-field arithmetic, HBM-bound: no MFMA.
//
//  * encode_v16<K,R,...>: one lane per 16-byte column of one group (flat over all groups,
//    so a wave covers 64 consecutive columns and its loads are 1 KiB coalesced rows).
//    A lane loads its column of all K data packets (K dwordx4 loads in flight), XORs them
//    into parity row 0 (the reference XOR, fec_xor_simd.cpp:411-427) and multiplies them
//    into rows 1..R-1 with v_perm_b32 table lookups (3 per dword per coefficient, tables
//    in SGPRs via scalar loads), then stores R dwordx4.
//  * encode_bits<K,R,W,...>: the bit-sliced form (bitslice.hpp), the code's coefficients compiled
//    in, a lane owning one column of two groups.
//  * encode_bytes: packets shorter than 16 B (one lane per byte), same tables.
//
// Any packet size P >= 16 and any packet alignment run on the vector kernels: the last
// 16-byte column of a packet is shifted back to [P - 16, P) (it overlaps the column before
// it; both lanes compute the same bytes and store the same values), and loads / stores of
// 16 B at any byte address are legal on gfx950 (unaligned global access, which the
// compiler also assumes for amdhsa).  GF arithmetic is byte-wise with one coefficient per
// packet, so a column's position inside its packet never changes its arithmetic.  The same holds
// for the column decodes of fec_decode.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "bitslice.hpp"
#include "fec_device.hpp"  // Tab, ld16 / st16, gmul, xor3, xcd_tile; Sel, prep, mac, xor_into, gmul_byte, col_off16
#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_launch.hpp"  // launch limits, for_chunks, for_row_passes, launch_record, knob

namespace qfec {
namespace {

// acc ^= a*ta ^ b*tb (two coefficients, see kPairMac)
__device__ __forceinline__ uint32_t mac2_dword(uint32_t acc, uint32_t sa0, uint32_t sa1, uint32_t sa2, const Tab& ta,
                                               uint32_t sb0, uint32_t sb1, uint32_t sb2, const Tab& tb) {
  const uint32_t a0 = __builtin_amdgcn_perm(ta.t0hi, ta.t0lo, sa0);
  const uint32_t a1 = __builtin_amdgcn_perm(ta.t1hi, ta.t1lo, sa1);
  const uint32_t a2 = __builtin_amdgcn_perm(ta.t2, ta.t2, sa2);
  const uint32_t b0 = __builtin_amdgcn_perm(tb.t0hi, tb.t0lo, sb0);
  const uint32_t b1 = __builtin_amdgcn_perm(tb.t1hi, tb.t1lo, sb1);
  const uint32_t b2 = __builtin_amdgcn_perm(tb.t2, tb.t2, sb2);
  return xor3(xor3(xor3(acc, a0, a1), a2, b0), b1, b2);
}

__device__ __forceinline__ void mac2(u32x4& acc, const Sel& a, const Tab& ta, const Sel& b, const Tab& tb) {
  acc.x = mac2_dword(acc.x, a.s0[0], a.s1[0], a.s2[0], ta, b.s0[0], b.s1[0], b.s2[0], tb);
  acc.y = mac2_dword(acc.y, a.s0[1], a.s1[1], a.s2[1], ta, b.s0[1], b.s1[1], b.s2[1], tb);
  acc.z = mac2_dword(acc.z, a.s0[2], a.s1[2], a.s2[2], ta, b.s0[2], b.s1[2], b.s2[2], tb);
  acc.w = mac2_dword(acc.w, a.s0[3], a.s1[3], a.s2[3], ta, b.s0[3], b.s1[3], b.s2[3], tb);
}

__device__ __forceinline__ void xor2_into(u32x4& acc, const u32x4& x, const u32x4& y) {
  acc.x = xor3(acc.x, x.x, y.x);
  acc.y = xor3(acc.y, x.y, y.y);
  acc.z = xor3(acc.z, x.z, y.z);
  acc.w = xor3(acc.w, x.w, y.w);
}

template <int OFF>
__device__ __forceinline__ const uint8_t* packet_ptr(const uint8_t* data, const void* offsets,
                                                     uint64_t g, uint32_t k, uint32_t j, uint32_t P) {
  if constexpr (OFF == 0) {
    return data + (g * k + j) * static_cast<uint64_t>(P);
  } else if constexpr (OFF == 1) {
    return data + static_cast<const uint32_t*>(offsets)[g * k + j];
  } else if constexpr (OFF == 2) {
    return data + static_cast<const uint64_t*>(offsets)[g * k + j];
  } else {  // absolute packet addresses (OffsetKind::kAddr)
    return reinterpret_cast<const uint8_t*>(static_cast<const uint64_t*>(offsets)[g * k + j]);
  }
}

// kStageRows: after the workgroup's barrier, its staged window (bytes, a multiple of 16) leaves
// LDS as consecutive 16-B pieces from consecutive lanes.
template <int POL>
__device__ __forceinline__ void stage_rows_out(const uint8_t* lds, uint8_t* dst, uint32_t bytes) {
  __syncthreads();
  for (uint32_t o = threadIdx.x * 16u; o < bytes; o += blockDim.x * 16u)
    st16<POL>(dst + o, *reinterpret_cast<const u32x4*>(lds + o));
}

// ---------------------------------------------------------------------------------
// Encode, 16-byte columns.  K > 0: compile-time group size, all K loads issued before
// the arithmetic.  K == 0: runtime k, loop.  Rows [row0, row0 + R) of the parity; when
// FIRST (row0 == 0) row 0 is the plain XOR.  Column 0 of every row is 1 by construction.
// ---------------------------------------------------------------------------------
//
// Columns per packet cpp = ceil(P / 16); column c covers bytes [min(16c, P - 16), +16).
// Thread -> (group, column) mapping, two forms:
//  * tiled (tile > 0): a workgroup owns `tile` whole groups (lanes [0, tile*cpp), the rest
//    idle).  The workgroup's data window then starts and ends on group boundaries, so no
//    cache line is split between workgroups (which sit on different XCDs, each with its
//    own L2) and every line is fetched from HBM once.  Measured +2..4% over flat at
//    k=10/1200 B (tools/probe_encode.hip).
//  * flat (tile == 0): one lane per column over all groups (packet sizes > 512 columns).
template <int K, int R, int OFF, bool FIRST, int POL = 0>
__global__ __launch_bounds__(512) void encode_v16(const uint8_t* __restrict__ data,
                                                  const void* __restrict__ offsets,
                                                  uint8_t* __restrict__ parity, uint64_t g_first,
                                                  uint32_t nthreads, uint32_t cpp, uint32_t P,
                                                  uint32_t k_rt, uint32_t r_total, uint32_t row0,
                                                  const Tab* __restrict__ tabs, uint32_t tile,
                                                  uint64_t groups, uint32_t never) {
  // Dynamic LDS is only an occupancy cap (occupancy_cap_lds).  It is declared and
  // referenced so that every HIP runtime honours the launch's dynamic LDS size; `never`
  // is always 0.
  extern __shared__ __attribute__((aligned(16))) uint8_t occupancy_lds[];
  if (never) occupancy_lds[threadIdx.x] = 0;
  // kStageRows: the rows through LDS (the launcher sizes the dynamic LDS for the window)
  const bool stage = (POL & kStageRows) != 0 && tile > 0 && (P & 15u) == 0 && row0 == 0 && r_total == static_cast<uint32_t>(R);
  uint32_t gl, col, gtile = 0, glocal = 0;
  bool active = true;
  if (tile > 0) {
    const uint32_t lane = threadIdx.x;
    gl = lane / cpp;
    col = lane - gl * cpp;
    glocal = gl;
    active = gl < tile;
    gtile = xcd_tile(blockIdx.x, gridDim.x) * tile;
    gl += gtile;
    active = active && gl < groups;
  } else {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    active = t < nthreads;
    gl = t / cpp;
    col = t - gl * cpp;
  }
  // (staged: an idle lane stays for the workgroup's barrier)
  if (!active && !stage) return;
  const uint64_t g = g_first + gl;
  const uint32_t k = K > 0 ? static_cast<uint32_t>(K) : k_rt;
  const size_t coff = col_off16(col, P);

  u32x4 acc[R];
  if (active) {
  if constexpr (K > 0) {
    u32x4 d[K];
#pragma unroll
    for (int j = 0; j < K; ++j) d[j] = ld16<POL>(packet_ptr<OFF>(data, offsets, g, K, j, P) + coff);
#pragma unroll
    for (int i = 0; i < R; ++i) acc[i] = d[0];
    // kPairMac: coefficients j = 1..K-1 two at a time; an odd one left over takes the
    // single-coefficient loop below (jstart)
    constexpr bool kPair = (POL & kPairMac) != 0 && !(FIRST && R == 1);
    constexpr int kPairs = kPair ? (K - 1) / 2 : 0;
#pragma unroll
    for (int pj = 0; pj < kPairs; ++pj) {
      const int j = 1 + 2 * pj;
      Sel sa, sb;
      prep(d[j], sa);
      prep(d[j + 1], sb);
#pragma unroll
      for (int i = 0; i < R; ++i) {
        if (FIRST && i == 0) {
          xor2_into(acc[0], d[j], d[j + 1]);
        } else {
          const uint32_t row = row0 + static_cast<uint32_t>(i);
          mac2(acc[i], sa, tabs[(row - 1) * K + j], sb, tabs[(row - 1) * K + j + 1]);
        }
      }
    }
    constexpr int jstart = 1 + 2 * kPairs;
#pragma unroll
    for (int j = jstart; j < K; ++j) {
      if constexpr (FIRST && R == 1) {
        xor_into(acc[0], d[j]);
      } else {
        Sel s;
        prep(d[j], s);
#pragma unroll
        for (int i = 0; i < R; ++i) {
          if (FIRST && i == 0) {
            xor_into(acc[0], d[j]);
          } else {
            const uint32_t row = row0 + static_cast<uint32_t>(i);
            mac(acc[i], s, tabs[(row - 1) * K + j]);
          }
        }
      }
    }
  } else {
    const u32x4 d0 = ld16<POL>(packet_ptr<OFF>(data, offsets, g, k, 0, P) + coff);
#pragma unroll
    for (int i = 0; i < R; ++i) acc[i] = d0;
#pragma unroll 4
    for (uint32_t j = 1; j < k; ++j) {
      const u32x4 x = ld16<POL>(packet_ptr<OFF>(data, offsets, g, k, j, P) + coff);
      Sel s;
      prep(x, s);
#pragma unroll
      for (int i = 0; i < R; ++i) {
        if (FIRST && i == 0) {
          xor_into(acc[0], x);
        } else {
          const uint32_t row = row0 + static_cast<uint32_t>(i);
          mac(acc[i], s, tabs[(row - 1) * k + j]);
        }
      }
    }
  }
  }
  if (!stage) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      st16<POL>(parity + (g * r_total + row0 + static_cast<uint32_t>(i)) * static_cast<uint64_t>(P) + coff, acc[i]);
    }
    return;
  }
  // staged: the tile's rows (tile groups x R rows, back to back as in HBM) into LDS, then out
  if (active) {
#pragma unroll
    for (int i = 0; i < R; ++i)
      *reinterpret_cast<u32x4*>(occupancy_lds + (glocal * R + static_cast<uint32_t>(i)) * P + coff) = acc[i];
  }
  stage_rows_out<POL>(occupancy_lds, parity + (g_first + gtile) * R * static_cast<uint64_t>(P),
                      static_cast<uint32_t>((groups - gtile < tile ? groups - gtile : tile) * R * P));
}

// ---------------------------------------------------------------------------------
// Encode, bit-sliced (bitslice.hpp): the code's coefficients compiled in, no tables.
// A lane owns one 16-byte column of two groups: group gl and group gl + tile of its
// workgroup's 2 * tile groups.  The 32 bytes a lane transposes need not be neighbours —
// every byte of packet j is multiplied by the same coefficient in every group — so each load
// instruction of a wave reads 64 consecutive columns exactly as encode_v16 does.  A second
// group past the end repeats the first and is not stored.  All R rows, device-contiguous
// packets.  Measured alternatives (profiles/r03_ab_bits_*.jsonl): a 32-byte chunk of one packet
// per lane (two column runs per instruction) 10% slower at k=10 r=3; adjacent groups, or wave
// pairs over one run of columns, the same as this form; non-temporal loads no better.
// ---------------------------------------------------------------------------------
template <int K, int R, int W, int POL>
__global__ __launch_bounds__(512) void encode_bits(const uint8_t* __restrict__ data,
                                                   uint8_t* __restrict__ parity, uint64_t g_first,
                                                   uint32_t cpp, uint32_t P, uint32_t tile,
                                                   uint64_t groups, uint32_t never) {
  extern __shared__ __attribute__((aligned(16))) uint8_t occupancy_lds[];
  if (never) occupancy_lds[threadIdx.x] = 0;
  // kStageRows: the workgroup's 2 * tile groups' rows through LDS (the launcher sizes it)
  const bool stage = (POL & kStageRows) != 0 && (P & 15u) == 0;
  const uint32_t lane = threadIdx.x;
  const uint32_t glocal = lane / cpp;
  const uint32_t c = lane - glocal * cpp;
  const uint32_t gtile = xcd_tile(blockIdx.x, gridDim.x) * (2 * tile);
  const uint32_t gl = gtile + glocal;
  const bool active = glocal < tile && gl < groups;
  // (staged: an idle lane stays for the workgroup's barrier)
  if (!active && !stage) return;
  const bool second = gl + tile < groups;
  const uint64_t g = g_first + gl, g2 = second ? g + tile : g;
  const uint32_t o = col_off16(c, P);
  uint32_t out[R][8];
  if (active) {
    const uint8_t* base = data + g * K * static_cast<uint64_t>(P) + o;
    const uint8_t* base2 = data + g2 * K * static_cast<uint64_t>(P) + o;
    auto load = [&](int j, uint32_t(&x)[8]) {
      const u32x4 a = ld16<POL>(base + static_cast<uint64_t>(j) * P), b = ld16<POL>(base2 + static_cast<uint64_t>(j) * P);
      x[0] = a.x, x[1] = a.y, x[2] = a.z, x[3] = a.w;
      x[4] = b.x, x[5] = b.y, x[6] = b.z, x[7] = b.w;
    };
    bs::encode_stream<K, R, W>(load, out);
  }
  if (!stage) {
#pragma unroll
    for (int i = 0; i < R; ++i)
      st16<POL>(parity + (g * R + i) * static_cast<uint64_t>(P) + o, u32x4{out[i][0], out[i][1], out[i][2], out[i][3]});
    if (second) {
#pragma unroll
      for (int i = 0; i < R; ++i)
        st16<POL>(parity + (g2 * R + i) * static_cast<uint64_t>(P) + o, u32x4{out[i][4], out[i][5], out[i][6], out[i][7]});
    }
    return;
  }
  if (active) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      *reinterpret_cast<u32x4*>(occupancy_lds + (glocal * R + static_cast<uint32_t>(i)) * P + o) =
          u32x4{out[i][0], out[i][1], out[i][2], out[i][3]};
      if (second)
        *reinterpret_cast<u32x4*>(occupancy_lds + ((glocal + tile) * R + static_cast<uint32_t>(i)) * P + o) =
            u32x4{out[i][4], out[i][5], out[i][6], out[i][7]};
    }
  }
  stage_rows_out<POL>(occupancy_lds, parity + (g_first + gtile) * R * static_cast<uint64_t>(P),
                      static_cast<uint32_t>((groups - gtile < 2 * tile ? groups - gtile : 2 * tile) * R * P));
}

// Encode, one lane per byte (any size / alignment).  All r rows.
template <int OFF>
__global__ __launch_bounds__(256) void encode_bytes(const uint8_t* __restrict__ data,
                                                    const void* __restrict__ offsets,
                                                    uint8_t* __restrict__ parity, uint64_t g_first,
                                                    uint32_t nthreads, uint32_t P, uint32_t k,
                                                    uint32_t r, const Tab* __restrict__ tabs) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= nthreads) return;
  const uint32_t gl = t / P;
  const uint32_t b = t - gl * P;
  const uint64_t g = g_first + gl;
  for (uint32_t i = 0; i < r; ++i) {
    uint32_t acc = 0;
    for (uint32_t j = 0; j < k; ++j) {
      const uint32_t x = packet_ptr<OFF>(data, offsets, g, k, j, P)[b];
      acc ^= (i == 0 || j == 0) ? x : gmul_byte(x, tabs[(i - 1) * k + j]);
    }
    parity[(g * r + i) * static_cast<uint64_t>(P) + b] = static_cast<uint8_t>(acc);
  }
}

}  // namespace

// ---------------------------------------------------------------------------------
// Launchers: which form a call takes is decided in fec_forms.hpp; these only launch it.
// ---------------------------------------------------------------------------------
namespace {

// POL: parity is written once and not re-read by this kernel (non-temporal stores).
template <int K, int R, int OFF, bool FIRST, int POL = kNtStore>
hipError_t run_encode_v16(const EncodeLaunch& a, uint32_t row0, hipStream_t s) {
  const uint32_t cpp = (a.P + 15u) / 16u;
  const uint32_t tile = encode_tile(a);
  return for_chunks(a.groups, groups_per_launch(cpp), [&](uint64_t g0, uint64_t gn) {
    const uint32_t n = static_cast<uint32_t>(gn * cpp);
    {
      const uint32_t bs = tile > 0 ? (tile * cpp + 63) / 64 * 64 : 256u;
      LaunchRecord t = launch_record(LaunchForm::kEncodeV16, tile > 0 ? (gn + tile - 1) / tile : blocks_for(n), bs, g0, gn);
      t.k = K, t.r = R, t.off = OFF, t.first = FIRST, t.pol = POL, t.tile = tile, t.aux = row0;
      trace_launch(t);
    }
    if (tile > 0) {
      const uint32_t bs = (tile * cpp + 63) / 64 * 64;
      const uint32_t blocks = static_cast<uint32_t>((gn + tile - 1) / tile);
      // Workgroups per CU: the compile-time-k kernels with few table rows stream best at 2;
      // with r >= 4 rows of table arithmetic per load the kernel is VALU-bound and wants more
      // waves: k=20 r=5 at 4 workgroups 5.22-5.40 ms, 3: 5.35-5.50, uncapped 5.22-5.59
      // (profiles/r02_ab_encode_blocks_c4.txt, two boxes).  The runtime-k loop runs uncapped.
      // The XOR-only kernel (r = 1, the reference's computation) streams best at ~15 waves per
      // CU: k=10 at 1200 B (5-wave workgroups) 2.30 ms at 3 workgroups vs 2.39 at 2 and 2.36 at
      // 4; at 1400 B (7-wave workgroups) 2 (14 waves) beats 3 (21) by 1.7%
      // (profiles/r02_ab_encode_blocks_r1.txt, r02_ab_encode_blocks_r2.txt).
      constexpr int kDefBlocks = K == 0 ? 0 : (R >= 4 ? kEncodeBlocksPerCU + 2 : kEncodeBlocksPerCU);
      const int blocks_env = knob(TestKnob::kEncodeBlocks, -1);
      const int blocks_per_cu = blocks_env >= 0 ? blocks_env : kDefBlocks;
      const bool xor_waves = K > 0 && FIRST && R == 1 && blocks_env < 0;
      const int waves = a.waves_per_cu ? a.waves_per_cu
                                       : knob(TestKnob::kEncodeWaves, xor_waves ? kEncodeXorWavesPerCU
                                                                                : blocks_per_cu * static_cast<int>(bs / 64));
      uint32_t smem = occupancy_cap_lds(waves, bs / 64);
      if constexpr ((POL & kStageRows) != 0) smem = std::max<uint32_t>(smem, tile * R * a.P);
      hipLaunchKernelGGL((encode_v16<K, R, OFF, FIRST, POL>), dim3(blocks), dim3(bs), smem, s, a.data,
                         a.offsets, a.parity, g0, n, cpp, a.P, a.k, a.r, row0,
                         static_cast<const Tab*>(a.tables), tile, gn, 0u);
    } else {
      hipLaunchKernelGGL((encode_v16<K, R, OFF, FIRST, POL>), dim3(blocks_for(n)), dim3(256), 0, s, a.data,
                         a.offsets, a.parity, g0, n, cpp, a.P, a.k, a.r, row0,
                         static_cast<const Tab*>(a.tables), 0u, gn, 0u);
    }
  });
}

template <int K, int R, int W, int POL = kNtStore>
hipError_t run_encode_bits(const EncodeLaunch& a, hipStream_t s) {
  const uint32_t cpp = (a.P + 15u) / 16u;
  const uint32_t tile = encode_tile(a);
  if (tile == 0) return hipErrorInvalidValue;  // callers route P > 8,192 elsewhere
  const uint32_t bs = (tile * cpp + 63) / 64 * 64;
  return for_chunks(a.groups, max_wave_blocks() * 2 * tile, [&](uint64_t g0, uint64_t gn) {
    const uint32_t blocks = static_cast<uint32_t>((gn + 2 * tile - 1) / (2 * tile));
    // Unstaged: uncapped (k=20 r=5 at 12 / 18 / 24 waves per CU within 0.2%, 3 waves per SIMD by
    // VGPRs).  Staged rows (kStageRows): 2 workgroups per CU, 5.163 vs 5.246 ms uncapped on two
    // boxes (scripts/sweep_encode_tiles.py, profiles/r05h, r05i).
    constexpr int kDefWaves = (POL & kStageRows) != 0 ? 10 : 0;
    const int waves = a.waves_per_cu ? a.waves_per_cu : knob(TestKnob::kEncodeWaves, kDefWaves);
    uint32_t smem = occupancy_cap_lds(waves, bs / 64);
    if constexpr ((POL & kStageRows) != 0) smem = std::max<uint32_t>(smem, 2 * tile * R * a.P);
    LaunchRecord t = launch_record(LaunchForm::kEncodeBits, blocks, bs, g0, gn);
    t.k = K, t.r = R, t.off = 0, t.pol = POL, t.tile = tile, t.aux = W;
    trace_launch(t);
    hipLaunchKernelGGL((encode_bits<K, R, W, POL>), dim3(blocks), dim3(bs), smem, s, a.data, a.parity, g0, cpp, a.P,
                       tile, gn, 0u);
  });
}

// Runtime k, or packets shorter than 16 B.
template <int OFF>
hipError_t run_encode_generic(const EncodeLaunch& a, hipStream_t s) {
  if (a.P < kVecMinP) {
    return for_chunks(a.groups, groups_per_launch(a.P), [&](uint64_t g0, uint64_t gn) {
      const uint32_t n = static_cast<uint32_t>(gn * a.P);
      LaunchRecord t = launch_record(LaunchForm::kEncodeBytes, blocks_for(n), 256, g0, gn);
      t.k = 0, t.off = OFF;
      trace_launch(t);
      hipLaunchKernelGGL(encode_bytes<OFF>, dim3(blocks_for(n)), dim3(256), 0, s, a.data, a.offsets,
                         a.parity, g0, n, a.P, a.k, a.r, static_cast<const Tab*>(a.tables));
    });
  }
  // Runtime k: passes of up to 8 parity rows (for_row_passes); the first pass owns the XOR row.
  return for_row_passes(a.r, [&](uint32_t row0, uint32_t rows, bool first) {
#define QFEC_PASS(_, RR) \
  if (rows == RR) return first ? run_encode_v16<0, RR, OFF, true>(a, row0, s) : run_encode_v16<0, RR, OFF, false>(a, row0, s);
    QFEC_ENCODE_PASS_ROWS(QFEC_PASS, ~)
#undef QFEC_PASS
    return hipErrorInvalidValue;
  });
}

}  // namespace

hipError_t launch_encode(const EncodeLaunch& a, hipStream_t s) {
  if (a.groups == 0) return hipSuccess;
  const EncodeForm f = encode_form(a);
  if (f.K == 0)  // runtime k or the byte kernel, per kind of offsets
    return f.OFF == 0 ? run_encode_generic<0>(a, s) : f.OFF == 1 ? run_encode_generic<1>(a, s)
         : f.OFF == 2 ? run_encode_generic<2>(a, s) : run_encode_generic<3>(a, s);
#define QFEC_V16(KK, RR, OO, PP)                                                              \
  if (f.kernel == EncodeKernel::kV16 && f.K == KK && f.R == RR && f.OFF == OO && f.POL == (PP)) \
    return run_encode_v16<KK, RR, OO, true, PP>(a, 0, s);
#define QFEC_BITS(KK, RR, OO, PP)                                                              \
  if (f.kernel == EncodeKernel::kBits && f.K == KK && f.R == RR && f.OFF == OO && f.POL == (PP)) \
    return run_encode_bits<KK, RR, 4, PP>(a, s);
  QFEC_ENCODE_V16_FORMS(QFEC_V16)
  QFEC_ENCODE_BITS_FORMS(QFEC_BITS)
#undef QFEC_BITS
#undef QFEC_V16
  return hipErrorNotSupported;
}

hipError_t load_encode_unit() {
  hipFuncAttributes at;
  return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(encode_bytes<0>));
}

}  // namespace qfec
