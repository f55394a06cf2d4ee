// fec_gather_var.hip — gfx950 kernels of fec_recover_gather_var_rs_dev and
// fec_encode_gather_var_rs_dev: the address-table calls with a length per table entry.  Shard
// (g, s) is the bytes [0, min(len, P)) at its address followed by zeros up to P; no byte at or
// past addr + len is read, and an entry of length 0 is never dereferenced.
//
//  * classify_table<Lens::kGiven> (fec_table.hpp; the launch trace's classify_gather_var): the
//    classify scan plus the symbol length -- the lanes that scan a workgroup's table entries read
//    the lengths too and keep each group's largest min(len, P) over its present entries in LDS
//    beside the mask.
//  * recover_gather_var<K, MAXE, POL>: one wave per group, record-addressed like recover_gather.
//    The survivors' lengths are fetched once per group beside their addresses (compile-time k:
//    scalar loads into SGPRs; runtime k: a second per-wave LDS slice).  A pass of the walk that
//    lies below every survivor's length (a wave-uniform test) is decode_piece with plain loads,
//    as in recover_gather; any other pass loads through the length-masked piece load
//    (fec_varlen.hpp var_load, the only place that decides where a lane reads).
//  * encode_gather_var<0, R, FIRST>: one lane per 16-B column of a group, runtime k, rows
//    [row0, row0 + R) per launch; every packet load is masked by its length, address 0 (absent)
//    contributes zeros; the lane of column 0 of the first pass writes the group's symbol length.
// The rule, the record header, the piece rebuild and the GF(2^8) product are fec_device.hpp's;
// the classify scan, the table-entry pointer, the masked piece load (load_masked) and the
// survivor functors (VarSurvivors, VarSurvivorsLds) are fec_table.hpp's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fec_device.hpp"
#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_launch.hpp"
#include "fec_table.hpp"
#include "fec_varlen.hpp"

namespace qfec {
namespace {

// decode_walk's walk with the choice per pass: a pass whose bytes [base, end) lie below
// `minlen`, the shortest survivor (wave-uniform), takes `plain` (s -> base, unmasked loads: every
// byte it reads is below every survivor's length); any other pass takes `masked`.
template <int K, int MAXE, int POL, typename PLAIN, typename MASKED>
__device__ __forceinline__ void var_walk(const uint32_t* rw, const Tab* tabs, uint8_t* og, uint32_t k, uint32_t P,
                                         uint32_t lane, uint32_t e, uint32_t m0, bool xor_only, uint32_t minlen,
                                         PLAIN plain, MASKED masked) {
  const uint32_t main_end = P & ~1023u;
  for (uint32_t base = 0; base < main_end; base += 1024u) {
    const uint32_t off = base + lane * 16u;
    if (base + 1024u <= minlen) decode_piece<K, MAXE, POL, 4>(rw, tabs, nullptr, nullptr, og, k, P, off, e, m0, xor_only, plain);
    else decode_piece<K, MAXE, POL, 4>(rw, tabs, nullptr, nullptr, og, k, P, off, e, m0, xor_only, masked);
  }
  for (uint32_t base = main_end; base < P; base += 256u) {
    const uint32_t o = base + lane * 4u;
    const uint32_t off = o + 4u <= P ? o : P - 4u;  // tail pieces shifted back to [P - 4, P)
    if (min_u32(base + 256u, P) <= minlen) decode_piece<K, MAXE, POL, 1>(rw, tabs, nullptr, nullptr, og, k, P, off, e, m0, xor_only, plain);
    else decode_piece<K, MAXE, POL, 1>(rw, tabs, nullptr, nullptr, og, k, P, off, e, m0, xor_only, masked);
  }
}

// One wave per group (4 per workgroup), the shapes of recover_gather.
template <int K, int MAXE, int POL>
__global__ __launch_bounds__(256) void recover_gather_var(const uint64_t* __restrict__ addrs,
                                                          const uint32_t* __restrict__ lens,
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
  const RecHead h = rec_head(codebook, rec);
  const uint32_t e = h.e();
  const bool xor_only = h.xor_only();
  if (m0 >= e) return;
  const Tab* tabs = h.tabs();
  const uint64_t* __restrict__ ga = addrs + gw * (k + r);
  const uint32_t* __restrict__ gl = lens + gw * (k + r);
  uint8_t* og = out + gw * r * static_cast<uint64_t>(P);
  static_assert((POL & kCompactOut) != 0, "recover_gather_var writes compact rows");
  if constexpr (K > 0) {
    VarSurvivors<K> sv;
    uint32_t minlen = P;
#pragma unroll
    for (int s = 0; s < K; ++s) {
      const uint32_t sid = rec_byte(h.rw, s);
      sv.base[s] = shard_ptr(ga[sid]);
      sv.len[s] = min_u32(gl[sid], P);
      minlen = min_u32(minlen, sv.len[s]);
    }
    const auto plain = [&sv](uint32_t s) { return sv.base[s]; };
    var_walk<K, MAXE, POL>(h.rw, tabs, og, k, P, lane, e, m0, xor_only, minlen, plain, sv);
  } else {
    __shared__ uint64_t slices[4 * 64];
    __shared__ uint32_t len_slices[4 * 64];
    __shared__ uint32_t shortest[4];
    uint64_t* slice = slices + wave * 64u;
    uint32_t* len_slice = len_slices + wave * 64u;
    if (lane == 0) shortest[wave] = P;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < k) {  // survivor `lane` of the record
      const uint32_t sid = reinterpret_cast<const uint8_t*>(h.rw)[lane];
      const uint32_t l = min_u32(gl[sid], P);
      slice[lane] = ga[sid];
      len_slice[lane] = l;
      atomicMin(&shortest[wave], l);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint32_t minlen = __builtin_amdgcn_readfirstlane(shortest[wave]);
    const auto plain = [slice](uint32_t s) { return shard_ptr(slice[s]); };
    var_walk<K, MAXE, POL>(h.rw, tabs, og, k, P, lane, e, m0, xor_only, minlen, plain, VarSurvivorsLds{slice, len_slice});
  }
}

// One lane per 16-B column of a group over all groups of the launch (column c covers bytes
// [min(16c, P - 16), +16), as encode_v16's), runtime k.  Rows [row0, row0 + R) of the parity; when
// FIRST (row0 == 0) row 0 is the plain XOR.  Every row is written whole: zeros where every
// packet had ended.
template <int K, int R, bool FIRST>
__global__ __launch_bounds__(256) void encode_gather_var(const uint64_t* __restrict__ addrs,
                                                         const uint32_t* __restrict__ lens,
                                                         uint8_t* __restrict__ parity,
                                                         uint32_t* __restrict__ symlen_out, uint32_t nthreads,
                                                         uint32_t cpp, uint32_t P, uint32_t k, uint32_t r_total,
                                                         uint32_t row0, const Tab* __restrict__ tabs) {
  static_assert(K == 0, "encode_gather_var takes k at run time");
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nthreads) return;
  const uint32_t g = t / cpp;
  const uint32_t col = t - g * cpp;
  const uint32_t coff = col * 16u + 16u <= P ? col * 16u : P - 16u;
  const uint64_t* __restrict__ ga = addrs + static_cast<uint64_t>(g) * k;
  const uint32_t* __restrict__ gl = lens + static_cast<uint64_t>(g) * k;
  uint32_t acc[R][4];
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[i][q] = 0;
  uint32_t symlen = 0;
#pragma unroll 4
  for (uint32_t j = 0; j < k; ++j) {
    const uint64_t a = ga[j];
    const uint32_t len = a != 0 ? min_u32(gl[j], P) : 0u;  // absent: all zero, never dereferenced
    symlen = symlen > len ? symlen : len;
    uint32_t x[4];
    load_masked<4, kTableEncodePol>(shard_ptr(a), coff, len, x);
    SelN<4> sel;
    sel_split(x, sel);
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (FIRST && i == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[0][q] ^= x[q];
      } else {
        const Tab& tb = tabs[(row0 + static_cast<uint32_t>(i) - 1u) * k + j];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[i][q] ^= gmul(sel.s0[q], sel.s1[q], sel.s2[q], tb);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < R; ++i)
    stw<4, kTableEncodePol>(parity + (static_cast<uint64_t>(g) * r_total + row0 + static_cast<uint32_t>(i)) * P + coff, acc[i]);
  if (FIRST && col == 0 && symlen_out) symlen_out[g] = symlen;
}

template <int K, int MAXE, int POL>
hipError_t run_recover_gather_var(const TableRecoverLaunch& a, hipStream_t s) {
  const uint64_t n = a.k + a.r;
  return for_wave_passes(a.groups, a.r, MAXE, [&](uint64_t g0, uint64_t gn, uint64_t bn, uint32_t m0) {
    LaunchRecord t = launch_record(static_cast<int64_t>(GatherVarLaunchForm::kRecoverGatherVar), bn, 256, g0, gn);
    t.k = K, t.r = MAXE, t.pol = POL, t.aux = m0;
    trace_launch(t);
    hipLaunchKernelGGL((recover_gather_var<K, MAXE, POL>), dim3(static_cast<uint32_t>(bn)), dim3(256), 0, s,
                       a.addrs + g0 * n, a.lens + g0 * n, a.rec_off + g0, a.codebook, gn, a.P, a.k, a.r, m0,
                       a.out + g0 * a.r * static_cast<uint64_t>(a.P), static_cast<uint32_t>(kDecodeWaveXcdSwizzle));
  });
}

template <int R, bool FIRST>
hipError_t run_encode_gather_var(const TableEncodeLaunch& a, uint32_t row0, hipStream_t s) {
  const uint32_t cpp = (a.P + 15u) / 16u;
  return for_chunks(a.groups, groups_per_launch(cpp), [&](uint64_t g0, uint64_t gn) {
    const uint32_t n = static_cast<uint32_t>(gn * cpp);
    LaunchRecord t = launch_record(static_cast<int64_t>(GatherVarLaunchForm::kEncodeGatherVar), blocks_for(n), 256, g0, gn);
    t.k = 0, t.r = R, t.first = FIRST, t.pol = kTableEncodePol, t.tile = 0, t.aux = row0;
    trace_launch(t);
    hipLaunchKernelGGL((encode_gather_var<0, R, FIRST>), dim3(blocks_for(n)), dim3(256), 0, s, a.addrs + g0 * a.k,
                       a.lens + g0 * a.k, a.parity + g0 * a.r * static_cast<uint64_t>(a.P),
                       a.symlen_out ? a.symlen_out + g0 : nullptr, n, cpp, a.P, a.k, a.r, row0,
                       static_cast<const Tab*>(a.tables));
  });
}

}  // namespace

// Which form runs is decided in fec_forms.hpp (table_recover_form); this only launches it.
hipError_t launch_recover_gather_var(const TableRecoverLaunch& a, hipStream_t s) {
  if (a.groups == 0) return hipSuccess;
  const TableRecoverForm f = table_recover_form(a.k, a.r, a.P, true);
  if (!f.supported) return hipErrorInvalidValue;
  hipError_t (*run)(const TableRecoverLaunch&, hipStream_t) = nullptr;
#define QFEC_GATHER_VAR(_, KK, MM, PP) \
  if (f.K == KK && f.MAXE == MM && f.POL == (PP)) run = run_recover_gather_var<KK, MM, PP>;
  QFEC_TABLE_RECOVER_FORMS(QFEC_GATHER_VAR, ~)
#undef QFEC_GATHER_VAR
  if (run == nullptr) return hipErrorNotSupported;
  const auto classify = [s](const TableRecoverLaunch& c) {
    return run_classify_table<Lens::kGiven>(c, static_cast<int64_t>(GatherVarLaunchForm::kClassifyGatherVar), s);
  };
  return run_table_recover(a, classify, run, s);
}

// The passes of table_encode_form (fec_forms.hpp); the first owns the XOR row.
hipError_t launch_encode_gather_var(const TableEncodeLaunch& a, hipStream_t s) {
  if (a.groups == 0) return hipSuccess;
  if (!table_encode_form(a.k, a.r, a.P, true).supported) return hipErrorInvalidValue;
  return for_row_passes(a.r, [&](uint32_t row0, uint32_t rows, bool first) {
#define QFEC_PASS(_, RR) \
  if (rows == RR) return first ? run_encode_gather_var<RR, true>(a, row0, s) : run_encode_gather_var<RR, false>(a, row0, s);
    QFEC_ENCODE_PASS_ROWS(QFEC_PASS, ~)
#undef QFEC_PASS
    return hipErrorInvalidValue;
  });
}

}  // namespace qfec
