// fec_device.hpp — the device code shared by the kernel translation units (fec_encode.hip,
// fec_decode.hip, fec_decode_fused.hip, fec_runs.hip, fec_gather.hip, fec_gather_var.hip,
// fec_scatter.hip; what only the address-table units share is fec_table.hpp's).  First the small
// pieces: the coefficient table entry,
// byte-aligned packet loads and stores under a memory policy, the GF(2^8) product of a dword, the
// selector split of a dword (SelN / sel_split), record bytes and the workgroup order; piece_load, a
// lane's load of its 4 * NM + NT dwords in the fused walk (decode_fused, recover_runs); the
// 16-byte-column pieces of the encodes and the column decodes (Sel, prep, mac, xor_into, gmul_byte,
// col_off16); RankMeta, the codebook levels the mask-addressed kernels rank in.  Then the
// record-addressed decode, stated once:
//  * classify_mask: erasure mask -> codebook record and status (the rule is fec_mask.hpp's; the
//    mask-addressed kernels of fec_decode_fused.hip and fec_runs.hip spell their own);
//  * RecHead / rec_head: a record's header (row count, XOR flag, coefficient tables);
//  * decode_piece: the rebuild of one lane's piece of every lost row.  The survivors' bases come
//    from the record and the group's contiguous data / parity (RecordBases, the default), or
//    from a caller's functor (the address-table recovers); the rebuilt rows go to the record's
//    places in the group's output (RecordRows, the default) or through a caller's functor (the
//    scatter recover);
//  * decode_walk: the walk of a wave over a packet, piece by piece.
// Everything is internal to its translation unit (unnamed namespace).  The helpers keep the
// statement order of the kernels they were taken from: the kernels' instruction order follows it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "fec_forms.hpp"    // the POL bits (kNtLoad .. kStageRows), LevelMeta
#include "fec_kernels.hpp"  // kRecNone, kRecBad
#include "fec_mask.hpp"     // the rule of an erasure mask: losses, the pick, ranks and the record

namespace qfec {
namespace {

struct Tab {
  uint32_t t0lo, t0hi, t1lo, t1hi, t2, coef, p0, p1;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// Byte-aligned views for packet memory (any P, any packet address): same dwordx4 / dword
// instructions as the aligned types.
typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t u32u __attribute__((aligned(1)));

// The memory policy / form bits of the kernels' POL parameter (kNtLoad .. kStageRows): fec_forms.hpp.

template <int POL>
__device__ __forceinline__ u32x4 ld16(const uint8_t* p) {
  if constexpr ((POL & kNtLoad) != 0) return __builtin_nontemporal_load(reinterpret_cast<const u32x4u*>(p));
  else return *reinterpret_cast<const u32x4u*>(p);
}

template <int POL>
__device__ __forceinline__ void st16(uint8_t* p, u32x4 v) {
  if constexpr ((POL & kNtStore) != 0) __builtin_nontemporal_store(v, reinterpret_cast<u32x4u*>(p));
  else *reinterpret_cast<u32x4u*>(p) = v;
}

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// GF(2^8) product of four bytes with the table's constant.
__device__ __forceinline__ uint32_t gmul(uint32_t s0, uint32_t s1, uint32_t s2, const Tab& t) {
  return xor3(__builtin_amdgcn_perm(t.t0hi, t.t0lo, s0), __builtin_amdgcn_perm(t.t1hi, t.t1lo, s1),
              __builtin_amdgcn_perm(t.t2, t.t2, s2));
}

// XCD-aware order of the workgroups' tiles.  Workgroups are dealt round-robin to the 8
// XCDs (b and b + 8 share one; MI355X_MICROARCH.md "Workgroup dispatch"), so mapping
// b -> (b % 8) * (n / 8) + b / 8 hands every XCD one contiguous eighth of the batch
// instead of every eighth tile.  Placement only changes speed, never results (any
// bijection of tiles is correct).  Measured +4..8% on encode (tools/probe_encode.hip).
__device__ __forceinline__ uint32_t xcd_tile(uint32_t b, uint32_t n) {
  const uint32_t per = n >> 3;
  return b < (per << 3) ? (b & 7u) * per + (b >> 3) : b;
}

// Tile of a decode workgroup by the launch's `swz`: bit 0 the XCD-aware order (xcd_tile),
// bit 1 the groups from last to first.
__device__ __forceinline__ uint32_t decode_block(uint32_t swz) {
  const uint32_t b = (swz & 2u) ? gridDim.x - 1u - blockIdx.x : blockIdx.x;
  return (swz & 1u) ? xcd_tile(b, gridDim.x) : b;
}

__device__ __forceinline__ uint32_t rec_byte(const uint32_t* __restrict__ w, uint32_t i) {
  return (w[i >> 2] >> (8u * (i & 3u))) & 0xFFu;
}

// NW-dword (NW = 4: 16 B, NW = 1: 4 B) load/store of one lane's piece.
template <int NW, int POL>
__device__ __forceinline__ void ldw(const uint8_t* p, uint32_t (&v)[NW]) {
  if constexpr (NW == 4) {
    const u32x4 t = ld16<POL>(p);
    v[0] = t.x;
    v[1] = t.y;
    v[2] = t.z;
    v[3] = t.w;
  } else {
    v[0] = *reinterpret_cast<const u32u*>(p);
  }
}

template <int NW, int POL>
__device__ __forceinline__ void stw(uint8_t* p, const uint32_t (&v)[NW]) {
  if constexpr (NW == 4) {
    st16<POL>(p, u32x4{v[0], v[1], v[2], v[3]});
  } else {
    if constexpr ((POL & kNtStore) != 0) __builtin_nontemporal_store(v[0], reinterpret_cast<u32u*>(p));
    else *reinterpret_cast<u32u*>(p) = v[0];
  }
}

// One lane's piece of a packet in the fused walk (decode_fused, recover_runs): NM 16-byte pieces at
// i * 1024 + lane * 16, then NT 4-byte tail pieces at toff[t] (the kernel's: NM * 1024 + t * 256 +
// lane * 4, shifted back to end at P), 4 * NM + NT dwords in all.
template <int NM, int NT, int POL>
__device__ __forceinline__ void piece_load(const uint8_t* base, uint32_t lane, const uint32_t (&toff)[NT > 0 ? NT : 1],
                                           uint32_t (&v)[4 * NM + NT]) {
#pragma unroll
  for (int i = 0; i < NM; ++i) {
    const u32x4 t = ld16<POL>(base + i * 1024u + lane * 16u);
    v[4 * i] = t.x;
    v[4 * i + 1] = t.y;
    v[4 * i + 2] = t.z;
    v[4 * i + 3] = t.w;
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if constexpr ((POL & kNtLoad) != 0) v[4 * NM + t] = __builtin_nontemporal_load(reinterpret_cast<const u32u*>(base + toff[t]));
    else v[4 * NM + t] = *reinterpret_cast<const u32u*>(base + toff[t]);
  }
}

// Selector bytes for the three pieces of every byte of NW dwords.
template <int NW>
struct SelN {
  uint32_t s0[NW], s1[NW], s2[NW];
};

template <int NW>
__device__ __forceinline__ void sel_split(const uint32_t (&v)[NW], SelN<NW>& s) {
#pragma unroll
  for (int q = 0; q < NW; ++q) {
    s.s0[q] = v[q] & 0x07070707u;
    s.s1[q] = (v[q] >> 3) & 0x07070707u;
    s.s2[q] = (v[q] >> 6) & 0x03030303u;
  }
}

// Selector bytes of a 16-byte column: the encodes (fec_encode.hip) and the column decodes
// (fec_decode.hip decode_v16, decode_tiled).
using Sel = SelN<4>;

__device__ __forceinline__ void prep(const u32x4& x, Sel& s) {
  const uint32_t w[4] = {x.x, x.y, x.z, x.w};
  sel_split(w, s);
}

__device__ __forceinline__ void mac(u32x4& acc, const Sel& s, const Tab& t) {
  acc.x ^= gmul(s.s0[0], s.s1[0], s.s2[0], t);
  acc.y ^= gmul(s.s0[1], s.s1[1], s.s2[1], t);
  acc.z ^= gmul(s.s0[2], s.s1[2], s.s2[2], t);
  acc.w ^= gmul(s.s0[3], s.s1[3], s.s2[3], t);
}

__device__ __forceinline__ void xor_into(u32x4& acc, const u32x4& x) { acc ^= x; }

__device__ __forceinline__ uint8_t gmul_byte(uint32_t x, const Tab& t) {
  return static_cast<uint8_t>(gmul(x & 7u, (x >> 3) & 7u, (x >> 6) & 3u, t));
}

// Byte offset of 16-byte column `col` inside a packet of P >= 16 bytes: the last column
// is shifted back to end at P (fec_encode.hip header).
__device__ __forceinline__ uint32_t col_off16(uint32_t col, uint32_t P) {
  const uint32_t o = col * 16u;
  return o + 16u <= P ? o : P - 16u;
}

// Codebook levels e = 1..3 for the inline classify of the mask-addressed kernels (decode_fused,
// recover_runs take it by value; fec_launch.hpp rank_meta fills it).
struct RankMeta {
  uint64_t base[4], stride[4], count_r[4];
};

// The classify rule (fec_mask.hpp) as the record-addressed kernels read it: erasure mask ->
// codebook record (in 32-B units) and status.  Nothing lost: kRecNone.  Unrecoverable: kRecBad,
// status 1.  Else the pick's record (`binom`: the C(n, t) table, rows of 65).
struct Classified {
  uint32_t rec;
  uint8_t status;
};

__device__ __forceinline__ Classified classify_mask(uint64_t m, uint32_t k, uint32_t r,
                                                    const uint64_t* __restrict__ binom, const LevelMeta& meta) {
  const MaskLosses l = mask_losses(m, k, r);
  if (l.lost == 0) return {kRecNone, 0};
  if (l.unrecoverable) return {kRecBad, 1};
  return {static_cast<uint32_t>(mask_record(m, k, r, l.lost, meta, ChooseTable{binom}) >> 5), 0};
}

// A record's header (gf256.hpp build_record): survivor ids from byte 0, erased ids from byte 64,
// e and the XOR flag in word 24, the coefficient tables (row m, survivor s at tabs[m * k + s])
// from byte 128.
struct RecHead {
  const uint32_t* rw;  // the record as words
  // rows to rebuild
  __device__ uint32_t e() const { return rw[24] & 0xFFu; }
  // one data shard lost and parity row 0 alive: the plain XOR
  __device__ bool xor_only() const { return ((rw[24] >> 8) & 0xFFu) != 0; }
  __device__ const Tab* tabs() const { return reinterpret_cast<const Tab*>(reinterpret_cast<const uint8_t*>(rw) + 128); }
};

__device__ __forceinline__ RecHead rec_head(const uint8_t* recp) { return {reinterpret_cast<const uint32_t*>(recp)}; }

// `rec` as classify_mask gives it (< kRecBad).
__device__ __forceinline__ RecHead rec_head(const uint8_t* codebook, uint32_t rec) {
  return rec_head(codebook + static_cast<uint64_t>(rec) * 32u);
}

// decode_piece's default address mode: survivor s is shard rec_byte(rw, s) of the group's
// contiguous data (dg) or parity (pg).  Any other SRC is a functor s -> base of survivor s.
struct RecordBases {};

// A functor SRC with a member type `loads_piece` loads a lane's piece itself,
// src.load<NW, POL>(s, off, v), instead of decode_piece loading NW dwords at src(s) + off (the
// variable-length address-table recover, fec_gather_var.hip: the load is masked by the shard's
// length).
template <typename SRC, typename = void>
struct loads_piece : std::false_type {};
template <typename SRC>
struct loads_piece<SRC, std::void_t<typename SRC::loads_piece>> : std::true_type {};

// decode_piece's default destination: row m0 + m at the erased shard's place in `og` (in place)
// or at row m0 + m of the group's compact run (kCompactOut).  Any other DST is a functor that
// stores the lane's piece of row m0 + m itself, dst.store<NW, POL>(m, off, v) (the scatter
// recover, fec_scatter.hip: the row goes to a destination of the caller's).
struct RecordRows {};

// Rebuild rows [m0, m0 + MAXE) of one group's record at byte offset `off` of every
// packet, NW dwords per lane.  The record (survivors, tables) is wave-uniform: SGPRs.
template <int K, int MAXE, int POL, int NW, typename SRC = RecordBases, typename DST = RecordRows>
__device__ __forceinline__ void decode_piece(const uint32_t* __restrict__ rw, const Tab* __restrict__ tabs,
                                             const uint8_t* __restrict__ dg, const uint8_t* __restrict__ pg,
                                             uint8_t* __restrict__ og, uint32_t k, uint32_t P, uint32_t off,
                                             uint32_t e, uint32_t m0, bool xor_only, SRC src = SRC{},
                                             DST dst = DST{}) {
  auto src_of = [&](uint32_t s) -> const uint8_t* {
    if constexpr (std::is_same_v<SRC, RecordBases>) {
      const uint32_t sid = rec_byte(rw, s);
      return sid < k ? dg + sid * static_cast<uint64_t>(P) : pg + (sid - k) * static_cast<uint64_t>(P);
    } else if constexpr (loads_piece<SRC>::value) {
      return nullptr;  // not used: src loads the piece itself
    } else {
      return src(s);
    }
  };
  // Runtime k: survivors in batches of kBatch loads in flight (slots past k re-load
  // survivor 0, a valid address, and are not used).
  constexpr uint32_t kBatch = 8;
  if (xor_only) {  // single data loss rebuilt from parity row 0: the reference XOR
    uint32_t acc[NW] = {};
    if constexpr (K > 0 && !std::is_same_v<SRC, RecordBases>) {
      // functor bases, compile-time k: exactly K loads, all in flight
      uint32_t x[K][NW];
#pragma unroll
      for (int s = 0; s < K; ++s) {
        if constexpr (loads_piece<SRC>::value) src.template load<NW, POL>(s, off, x[s]);
        else ldw<NW, POL>(src(s) + off, x[s]);
      }
#pragma unroll
      for (int s = 0; s < K; ++s)
#pragma unroll
        for (int q = 0; q < NW; ++q) acc[q] ^= x[s][q];
    } else {
      for (uint32_t s0 = 0; s0 < k; s0 += kBatch) {
        uint32_t v[kBatch][NW];
#pragma unroll
        for (uint32_t b = 0; b < kBatch; ++b) {
          if constexpr (loads_piece<SRC>::value) src.template load<NW, POL>(s0 + b < k ? s0 + b : 0, off, v[b]);
          else ldw<NW, POL>(src_of(s0 + b < k ? s0 + b : 0) + off, v[b]);
        }
#pragma unroll
        for (uint32_t b = 0; b < kBatch; ++b)
          if (s0 + b < k)
#pragma unroll
            for (int q = 0; q < NW; ++q) acc[q] ^= v[b][q];
      }
    }
    if constexpr (std::is_same_v<DST, RecordRows>)
      stw<NW, POL>(og + ((POL & kCompactOut) != 0 ? 0u : rec_byte(rw, 64)) * static_cast<uint64_t>(P) + off, acc);
    else dst.template store<NW, POL>(0u, off, acc);  // e = 1: row 0, m0 = 0
    return;
  }
  uint32_t acc[MAXE][NW];
#pragma unroll
  for (int m = 0; m < MAXE; ++m)
#pragma unroll
    for (int q = 0; q < NW; ++q) acc[m][q] = 0;
  auto consume = [&](const uint32_t (&v)[NW], uint32_t s, uint32_t kk) {
    SelN<NW> sel;
    sel_split(v, sel);
#pragma unroll
    for (int m = 0; m < MAXE; ++m) {
      if (m0 + m < e) {
        const Tab& t = tabs[(m0 + m) * kk + s];
        if constexpr ((POL & kNoCoefBranch) != 0) {
#pragma unroll
          for (int q = 0; q < NW; ++q) acc[m][q] ^= gmul(sel.s0[q], sel.s1[q], sel.s2[q], t);
        } else if (t.coef == 1u) {
#pragma unroll
          for (int q = 0; q < NW; ++q) acc[m][q] ^= v[q];
        } else if (t.coef != 0u) {
#pragma unroll
          for (int q = 0; q < NW; ++q) acc[m][q] ^= gmul(sel.s0[q], sel.s1[q], sel.s2[q], t);
        }
      }
    }
  };
  if constexpr (K > 0) {
    uint32_t x[K][NW];
#pragma unroll
    for (int s = 0; s < K; ++s) {
      if constexpr (std::is_same_v<SRC, RecordBases>) {
        const uint32_t sid = rec_byte(rw, s);
        const uint8_t* sp = sid < K ? dg + sid * static_cast<uint64_t>(P) : pg + (sid - K) * static_cast<uint64_t>(P);
        ldw<NW, POL>(sp + off, x[s]);
      } else if constexpr (loads_piece<SRC>::value) {
        src.template load<NW, POL>(s, off, x[s]);
      } else {
        ldw<NW, POL>(src(s) + off, x[s]);
      }
    }
#pragma unroll
    for (int s = 0; s < K; ++s) consume(x[s], s, K);
  } else {
    for (uint32_t s0 = 0; s0 < k; s0 += kBatch) {
      uint32_t v[kBatch][NW];
#pragma unroll
      for (uint32_t b = 0; b < kBatch; ++b) {
        if constexpr (loads_piece<SRC>::value) src.template load<NW, POL>(s0 + b < k ? s0 + b : 0, off, v[b]);
        else ldw<NW, POL>(src_of(s0 + b < k ? s0 + b : 0) + off, v[b]);
      }
#pragma unroll
      for (uint32_t b = 0; b < kBatch; ++b)
        if (s0 + b < k) consume(v[b], s0 + b, k);
    }
  }
#pragma unroll
  for (int m = 0; m < MAXE; ++m) {
    if (m0 + m < e) {
      // in place: at the erased shard; compact (kCompactOut): row m0 + m of the group's run
      if constexpr (std::is_same_v<DST, RecordRows>) {
        const uint32_t eid = (POL & kCompactOut) != 0 ? m0 + m : rec_byte(rw, 64 + m0 + m);
        stw<NW, POL>(og + eid * static_cast<uint64_t>(P) + off, acc[m]);
      } else {
        dst.template store<NW, POL>(static_cast<uint32_t>(m), off, acc[m]);
      }
    }
  }
}

// One wave's walk over a group's packets: whole 1 KiB passes of 16 B per lane, then the
// remainder (< 1 KiB) in 256-B passes of 4 B per lane, tail pieces past the packet end shifted
// back to [P - 4, P) (a neighbour's bytes, same values), so any P >= 4 works and no lane
// branches on the packet end.
template <int K, int MAXE, int POL, typename SRC = RecordBases>
__device__ __forceinline__ void decode_walk(const uint32_t* rw, const Tab* tabs, const uint8_t* dg, const uint8_t* pg,
                                            uint8_t* og, uint32_t k, uint32_t P, uint32_t lane, uint32_t e,
                                            uint32_t m0, bool xor_only, SRC src = SRC{}) {
  const uint32_t main_end = P & ~1023u;
  for (uint32_t base = 0; base < main_end; base += 1024u)
    decode_piece<K, MAXE, POL, 4>(rw, tabs, dg, pg, og, k, P, base + lane * 16u, e, m0, xor_only, src);
  for (uint32_t base = main_end; base < P; base += 256u) {
    const uint32_t off = base + lane * 4u;
    decode_piece<K, MAXE, POL, 1>(rw, tabs, dg, pg, og, k, P, off + 4u <= P ? off : P - 4u, e, m0, xor_only, src);
  }
}

}  // namespace
}  // namespace qfec
