// mean1d.h -- what the decode + mean kernels (decode_mean.hip) and the fused decode + mean + encode kernel
// (mean_enc1d.hip) share: the mean's scaling and the compiler-visible stream-word loads.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gcow {

// acc / nstreams for the N sums of a lane: an IEEE division, or -- nstreams a power of two (the usual world size) --
// the product by the exact reciprocal, which is the same correctly rounded value of the same quotient (a uniform
// branch: the division's expansion runs only for other world sizes).
template <int N>
__device__ __forceinline__ void mean_scale(float* a, uint32_t nstreams)
{
#pragma clang fp contract(off)
  if ((nstreams & (nstreams - 1u)) == 0u) {
    const float inv = 1.0f / (float)nstreams;
#pragma unroll
    for (int i = 0; i < N; i++) a[i] = a[i] * inv;
  } else {
    const float nf = (float)nstreams;
#pragma unroll
    for (int i = 0; i < N; i++) a[i] = a[i] / nf;
  }
}

// One stream word (a whole 64- or 32-bit block) as a compiler-visible buffer load: the one-shot mean kernels carry the
// words across their stream loop, and a value loaded by inline asm must not be carried (the loop's register copies
// would read the destination before the load has written it).
template <uint32_t WB> struct MeanWord;
template <> struct MeanWord<64> {
  typedef uint64_t T;
  static __device__ __forceinline__ T load(__amdgpu_buffer_rsrc_t rs, uint32_t b)
  {
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(b * 8u), 0, 0);
    return (uint64_t)v[0] | ((uint64_t)v[1] << 32);
  }
};
template <> struct MeanWord<32> {
  typedef uint32_t T;
  static __device__ __forceinline__ T load(__amdgpu_buffer_rsrc_t rs, uint32_t b)
  {
    return __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(b * 4u), 0, 0);
  }
};

}  // namespace gcow
