// fec_util.hip — gfx950 (MI355X, CDNA4) kernels of libfec_hip: the utilities around the hot path.
//
//  * fill_words, fill_bytes: synthetic data, counter-based splitmix64 (16 B or 1 B per lane).
//  * copy_words: a plain 16-B-per-lane copy, the box calibration bench.py reports the kernels
//    against.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_launch.hpp"  // launch limits, for_chunks, launch_record

namespace qfec {
namespace {

// ---------------------------------------------------------------------------------
// Synthetic data: counter-based splitmix64 (oracle_fill_splitmix restates it on the CPU).
// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void fill_words(uint8_t* __restrict__ dst, uint32_t n16,
                                                  uint64_t seed, uint64_t word0) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n16) return;
  const uint64_t w = word0 + 2ull * t;
  const uint64_t a = mix64(seed + (w + 1) * 0x9E3779B97F4A7C15ull);
  const uint64_t b = mix64(seed + (w + 2) * 0x9E3779B97F4A7C15ull);
  reinterpret_cast<uint4*>(dst)[t] =
      make_uint4(static_cast<uint32_t>(a), static_cast<uint32_t>(a >> 32), static_cast<uint32_t>(b),
                 static_cast<uint32_t>(b >> 32));
}

__global__ __launch_bounds__(256) void fill_bytes(uint8_t* __restrict__ dst, uint32_t n, uint64_t seed,
                                                  uint64_t pos0) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n) return;
  const uint64_t pos = pos0 + t;
  const uint64_t w = mix64(seed + (pos / 8 + 1) * 0x9E3779B97F4A7C15ull);
  dst[t] = static_cast<uint8_t>(w >> (8 * (pos % 8)));
}

// Box calibration: a plain 16-B-per-lane copy, the same access pattern as the encode's loads
// and stores without the arithmetic; bench.py reports the kernels against its rate.
__global__ __launch_bounds__(256) void copy_words(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                  uint32_t n16) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t < n16) dst[t] = src[t];
}

}  // namespace

// Launchers: chunked so that every grid stays inside the per-launch limits (fec_launch.hpp).
hipError_t launch_fill_splitmix(uint8_t* dst, uint64_t nbytes, uint64_t seed, uint64_t byte_offset,
                                hipStream_t s) {
  if (nbytes == 0) return hipSuccess;
  const bool fast = (byte_offset % 8 == 0) && (reinterpret_cast<uintptr_t>(dst) % 16 == 0);
  const uint64_t n16 = fast ? nbytes / 16 : 0;
  const hipError_t e = for_chunks(n16, max_launch_threads(), [&](uint64_t c0, uint64_t cn) {
    LaunchRecord t = launch_record(LaunchForm::kFill, blocks_for(cn), 256, c0, cn);
    t.aux = 16;
    trace_launch(t);
    hipLaunchKernelGGL(fill_words, dim3(blocks_for(cn)), dim3(256), 0, s, dst + c0 * 16,
                       static_cast<uint32_t>(cn), seed, (byte_offset / 8) + 2 * c0);
  });
  if (e != hipSuccess) return e;
  const uint64_t done = n16 * 16;
  return for_chunks(nbytes - done, max_launch_threads(), [&](uint64_t b0, uint64_t cn) {
    const uint64_t c0 = done + b0;
    LaunchRecord t = launch_record(LaunchForm::kFill, blocks_for(cn), 256, c0, cn);
    t.aux = 1;
    trace_launch(t);
    hipLaunchKernelGGL(fill_bytes, dim3(blocks_for(cn)), dim3(256), 0, s, dst + c0,
                       static_cast<uint32_t>(cn), seed, byte_offset + c0);
  });
}

hipError_t launch_copy_words(const uint8_t* src, uint8_t* dst, uint64_t nbytes, hipStream_t s) {
  return for_chunks(nbytes / 16, max_launch_threads(), [&](uint64_t c0, uint64_t cn) {
    LaunchRecord t = launch_record(LaunchForm::kCopy, blocks_for(cn), 256, c0, cn);
    t.aux = 16;
    trace_launch(t);
    hipLaunchKernelGGL(copy_words, dim3(blocks_for(cn)), dim3(256), 0, s,
                       reinterpret_cast<const uint4*>(src + c0 * 16), reinterpret_cast<uint4*>(dst + c0 * 16),
                       static_cast<uint32_t>(cn));
  });
}

hipError_t load_util_unit() {
  hipFuncAttributes at;
  return hipFuncGetAttributes(&at, reinterpret_cast<const void*>(fill_words));
}

}  // namespace qfec
