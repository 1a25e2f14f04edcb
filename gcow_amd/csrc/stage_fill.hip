// stage_fill.hip -- kernels that exist for the tests and the benchmark: the per-stage kernels for parity bisection
// (hw/stages/*.cpp counterparts) and the deterministic synthetic gradients.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "codec_device.h"
#include "kernels.h"

namespace gcow {

// ------------------------------------------------------------------------------------------------ stages
template <int D>
__global__ void k_stage_emax(const float* __restrict__ blocks, uint32_t n, int32_t* __restrict__ emax)
{
  constexpr int B = Dim<D>::B;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float f[B];
#pragma unroll
  for (int j = 0; j < B; j++) f[j] = blocks[(uint64_t)i * B + j];
  emax[i] = block_emax<B>(f);
}

template <int D>
__global__ void k_stage_cast(const float* __restrict__ blocks, const int32_t* __restrict__ emax, uint32_t n,
                             int32_t* __restrict__ q)
{
  constexpr int B = Dim<D>::B;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float s = cast_scale(emax[i]);
  for (int j = 0; j < B; j++) q[(uint64_t)i * B + j] = cast1(blocks[(uint64_t)i * B + j], s);
}

template <int D>
__global__ void k_stage_xform(int32_t* __restrict__ q, uint32_t n, int inverse)
{
  constexpr int B = Dim<D>::B;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int32_t a[B];
#pragma unroll
  for (int j = 0; j < B; j++) a[j] = q[(uint64_t)i * B + j];
  if (inverse) inv_xform<D>(a);
  else fwd_xform<D>(a);
#pragma unroll
  for (int j = 0; j < B; j++) q[(uint64_t)i * B + j] = a[j];
}

template <int D>
__global__ void k_stage_reorder(const int32_t* __restrict__ q, uint32_t n, uint32_t* __restrict__ u)
{
  constexpr int B = Dim<D>::B;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int32_t a[B];
  uint32_t o[B];
#pragma unroll
  for (int j = 0; j < B; j++) a[j] = q[(uint64_t)i * B + j];
  fwd_reorder<D>(o, a);
#pragma unroll
  for (int j = 0; j < B; j++) u[(uint64_t)i * B + j] = o[j];
}

// Coder on one ublock per lane into its own zeroed slot (32-bit LDS-free variant: a private global window).
struct GlobalSlotWriter {
  uint32_t* w;
  uint32_t pos, limit;
  __device__ __forceinline__ void put(uint64_t v, uint32_t n)
  {
    if (pos >= limit || n == 0) { pos += n; return; }
    uint32_t room = limit - pos;
    if (n > room) v &= lowmask64(room);
    uint32_t i = pos >> 5, sh = pos & 31;
    w[i] |= (uint32_t)(v << sh);
    w[i + 1] |= (uint32_t)((v << sh) >> 32);
    if (sh) w[i + 2] |= (uint32_t)(v >> (64 - sh));
    pos += n;
  }
  __device__ __forceinline__ void skip(uint32_t n) { pos += n; }
};

template <int D>
__global__ void k_stage_encode_ints(const uint32_t* __restrict__ ublocks, uint32_t n, uint32_t budget,
                                    uint32_t maxprec, uint64_t* __restrict__ slots, uint32_t slot_words,
                                    uint32_t* __restrict__ bits)
{
  constexpr int B = Dim<D>::B;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t u[B];
#pragma unroll
  for (int j = 0; j < B; j++) u[j] = ublocks[(uint64_t)i * B + j];
  uint32_t lim = slot_words * 64 - 64;  // keep the spill word inside the slot
  GlobalSlotWriter w{(uint32_t*)(slots + (uint64_t)i * slot_words), 0, budget < lim ? budget : lim};
  bits[i] = encode_ints<B>(w, u, budget, maxprec);
}

// ------------------------------------------------------------------------------------------------ synthetic data
__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ void k_fill_normal(float* __restrict__ out, uint64_t count, double sigma, uint64_t seed, int inject)
{
  // one lane per 4-value block: two Box-Muller pairs from counter-based splitmix64
  const uint64_t blk = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (blk * 4 >= count) return;
  float v[4];
#pragma unroll
  for (int pr = 0; pr < 2; pr++) {
    const uint64_t c = blk * 4 + 2 * pr;
    const double u1 = ((double)(mix64(seed ^ (c * 0xD1B54A32D192ED03ull)) >> 11) + 1.0) * 0x1.0p-53;
    const double u2 = (double)(mix64(seed ^ ((c + 1) * 0xD1B54A32D192ED03ull)) >> 11) * 0x1.0p-53;
    const double r = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincospi(2.0 * u2, &sn, &cs);
    v[2 * pr] = (float)(sigma * r * cs);
    v[2 * pr + 1] = (float)(sigma * r * sn);
  }
  if (inject) {
    const uint64_t h = mix64(blk ^ seed);
    double scale = 1.0;
    if (h % 64 == 0) scale = 0.0;
    else if (h % 4096 == 1) scale = 1e-35 / sigma;
    else if (h % 4096 == 2) scale = 1e-40 / sigma;
    if (scale != 1.0)
#pragma unroll
      for (int i = 0; i < 4; i++) v[i] = (float)((double)v[i] * scale);
  }
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (blk * 4 + i < count) out[blk * 4 + i] = v[i];
}

// ------------------------------------------------------------------------------------------------ launchers
static inline hipStream_t S(void* s) { return (hipStream_t)s; }

#define GCOW_STAGE(D)                                                                                          \
  switch (which) {                                                                                             \
    case 0: k_stage_emax<D><<<grid, 64, 0, st>>>((const float*)a, n, (int32_t*)out); break;                    \
    case 1: k_stage_cast<D><<<grid, 64, 0, st>>>((const float*)a, (const int32_t*)b, n, (int32_t*)out); break; \
    case 2: k_stage_xform<D><<<grid, 64, 0, st>>>((int32_t*)out, n, (int)x0); break;                           \
    case 3: k_stage_reorder<D><<<grid, 64, 0, st>>>((const int32_t*)a, n, (uint32_t*)out); break;              \
    case 4:                                                                                                    \
      k_stage_encode_ints<D><<<grid, 64, 0, st>>>((const uint32_t*)a, n, x0, x1, (uint64_t*)out, slot_words,   \
                                                  (uint32_t*)out2);                                            \
      break;                                                                                                   \
    default: return hipErrorInvalidValue;                                                                      \
  }
hipError_t launch_stage(int which, int dims, const void* a, const void* b, uint32_t n, void* out, uint32_t x0,
                        uint32_t x1, void* out2, uint32_t slot_words, void* stream)
{
  const uint32_t grid = (n + 63) / 64;
  if (!grid) return hipSuccess;
  hipStream_t st = S(stream);
  if (dims == 1) { GCOW_STAGE(1) }
  else if (dims == 2) { GCOW_STAGE(2) }
  else { GCOW_STAGE(3) }
  return hipGetLastError();
}
#undef GCOW_STAGE

hipError_t launch_fill_normal(float* out, uint64_t count, double sigma, uint64_t seed, int inject, void* stream)
{
  const uint64_t blocks = (count + 3) / 4;
  const uint64_t grid = (blocks + 255) / 256;
  if (!grid) return hipSuccess;
  k_fill_normal<<<grid, 256, 0, S(stream)>>>(out, count, sigma, seed, inject);
  return hipGetLastError();
}

}  // namespace gcow
