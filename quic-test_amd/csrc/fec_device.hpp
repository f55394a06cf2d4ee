// fec_device.hpp — device helpers shared by the kernel translation units (fec_kernels.hip,
// fec_gather.hip): the coefficient table entry, byte-aligned packet loads and stores under a
// memory policy, the GF(2^8) product of a dword, record bytes and the workgroup order.
// Everything is internal to its translation unit (unnamed namespace), as it was when
// fec_kernels.hip was the only one.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fec_forms.hpp"  // the POL bits (kNtLoad .. kStageRows)

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

}  // namespace
}  // namespace qfec
