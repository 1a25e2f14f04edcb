// rate_table1d.h -- the per-block pieces of the rate table, shared by the pass over a contiguous field
// (rate_table1d.hip), the pass over a tensor list's plan (rate_table_list1d.hip) and the pass that keeps a table per
// tensor (rate_table_rel1d.hip): a lane's raw rows, one block's updates of two 288-bin histograms (in LDS, or straight
// in a table's workspace: the sinks), the LDS histograms' zeroing and flush, and the rows of a plan's direct chunk.
// The header of rate_table1d.hip has the derivation.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec_device.h"
#include "field_io.h"
#include "kernels.h"
#include "lean1d.h"
#include "pipe.h"
#include "var1d_prep.h"

namespace gcow {

constexpr uint32_t RTT = 256;                    // lanes per workgroup
constexpr uint32_t RTU = 4;                      // consecutive blocks per lane
constexpr uint32_t RT_TILE = RTT * RTU;          // blocks per workgroup and iteration
constexpr uint32_t RT_BINS = kRateTableEntries;  // 288
constexpr uint32_t RT_COPIES = 16;               // interleaved LDS copies of each array
constexpr uint32_t RT_HIST_WORDS = 2 * RT_BINS * RT_COPIES;  // steps, then impulses: 36 864 B
static_assert(RT_TILE * 4 == kRateTableTileValues, "kernels.h states the tile for the tests");

// the lane's RTU consecutive blocks of a tile as raw words (fp32: one 16-byte load per block; bf16: one per two)
template <int DT>
struct RtRaw {
  static constexpr int N = DT == DT_BF16 ? RTU / 2 : RTU;
  uint4 w[N];
  // a tile of whole blocks in a contiguous, 16-byte aligned field
  __device__ __forceinline__ void load_wide(const FieldDesc& F, uint32_t t)
  {
    const uint64_t bl = (uint64_t)t * RT_TILE + (uint64_t)threadIdx.x * RTU;
    const uint4* src = (const uint4*)F.data + (DT == DT_BF16 ? bl / 2 : bl);
#pragma unroll
    for (int h = 0; h < N; h++) w[h] = src[h];
  }
  // any tile: blocks past the field read nothing, the partial last block is padded as the encoder pads it
  __device__ __forceinline__ void gather(const FieldDesc& F, uint32_t t)
  {
    const uint64_t bl = (uint64_t)t * RT_TILE + (uint64_t)threadIdx.x * RTU;
    uint32_t* d = (uint32_t*)w;
#pragma unroll
    for (uint32_t k = 0; k < RTU; k++) {
      float f[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (bl + k < F.nblocks) gather_block<1, DT>(F, (uint32_t)(bl + k), f);
      if constexpr (DT == DT_BF16) {
        d[2 * k] = (__float_as_uint(f[0]) >> 16) | (__float_as_uint(f[1]) & 0xffff0000u);
        d[2 * k + 1] = (__float_as_uint(f[2]) >> 16) | (__float_as_uint(f[3]) & 0xffff0000u);
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++) d[4 * k + i] = __float_as_uint(f[i]);
      }
    }
  }
  __device__ __forceinline__ void block(uint32_t k, float* f) const
  {
    const uint32_t* d = (const uint32_t*)w;
    if constexpr (DT == DT_BF16) {
      f[0] = __uint_as_float(d[2 * k] << 16);
      f[1] = __uint_as_float(d[2 * k] & 0xffff0000u);
      f[2] = __uint_as_float(d[2 * k + 1] << 16);
      f[3] = __uint_as_float(d[2 * k + 1] & 0xffff0000u);
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++) f[i] = __uint_as_float(d[4 * k + i]);
    }
  }
};

// bin t of the lane's copy; t outside the table (only -1 occurs) is dropped
__device__ __forceinline__ void rt_add(uint32_t* h, uint32_t copy, int t, uint32_t v)
{
  if ((uint32_t)t < RT_BINS) atomicAdd(h + (uint32_t)t * RT_COPIES + copy, v);
}

// Where a block's updates go. RtLdsSink: the lane's copy of the workgroup's two LDS arrays (every pass over whole
// tiles). RtGlobalSink: straight to a table's 2 x 288 workspace words by 64-bit atomics, steps sign-extended as
// rt_hist_flush extends them -- for blocks whose neighbours in the workgroup belong to other tables (the gather blocks
// of rate_table_rel1d.hip).
struct RtLdsSink {
  uint32_t* step;
  uint32_t* imp;
  uint32_t copy;
  __device__ __forceinline__ void add_step(int t, uint32_t v) const { rt_add(step, copy, t, v); }
  __device__ __forceinline__ void add_imp(int t, uint32_t v) const { rt_add(imp, copy, t, v); }
};

struct RtGlobalSink {
  unsigned long long* ws;  // the table's workspace: steps, then impulses
  __device__ __forceinline__ void add(unsigned long long* h, int t, uint32_t v) const
  {
    if ((uint32_t)t < RT_BINS) atomicAdd(h + (uint32_t)t, (unsigned long long)(long long)(int32_t)v);
  }
  __device__ __forceinline__ void add_step(int t, uint32_t v) const { add(ws, t, v); }
  __device__ __forceinline__ void add_imp(int t, uint32_t v) const { add(ws + RT_BINS, t, v); }
};

// one block's updates; a1 = a - 1 = emax + 157, the entry at which the block has precision 1
template <class Sink>
__device__ __forceinline__ void rt_block(const Sink& sink, int a1, const uint32_t* u, uint32_t pmax)
{
  const uint32_t S2 = u[2] | u[3], S1 = u[1] | S2, S0 = u[0] | S1;
  const uint32_t z[3] = {min(ffbh_hw(S0), 32u), min(ffbh_hw(S1), 32u), min(ffbh_hw(S2), 32u)};
  uint32_t l1 = 12u, start = 1u, level = 0u;  // l1 = L(1) - 1
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const uint32_t b = shl_hw(u[j], z[j]) >> 31;  // bit 31 - z_j of u_j; z_j = 32: u_j = 0
    l1 += z[j] == 0 ? b : 0u;
    l1 -= min(z[j], 1u);
    start += z[j] <= 1u ? 1u : 0u;
    const bool in = z[j] >= 1u && z[j] < pmax;
    if (in && b) sink.add_imp(a1 - (int)z[j], 1u);
    if (in && z[j] >= 2u) {
      sink.add_step(a1 - (int)z[j], 1u);
      level++;
    }
  }
  sink.add_imp(a1, l1);
  sink.add_step(a1 - 1, start);
  sink.add_step(a1 - (int)pmax, 0u - (start + level));
}

// one block from its four values (padded by the caller): the coefficients, then rt_block. real: the block exists.
// A zero block adds nothing whether it exists or not.
template <class Sink>
__device__ __forceinline__ void rt_values(const float* f, bool real, uint32_t pmax, const Sink& sink)
{
  uint32_t u[4];
  bool inf;
  const uint32_t m = v1_coeffs(f, u, inf);
  int a1 = (int)(m >> 23) + 31;  // emax = E - 126
  bool live = m != 0u;
  if (inf) {  // Inf / NaN: the generic rule for the exponent and the cast (emax from the finite values, Inf: 0)
    const Params full{1u, 16658u, 64u, -1074};  // precision > 0 for every emax: be = emax + 127, 0 for a zero block
    const BlockHead h = prepare_block<1>(f, full, u);
    a1 = (int)h.be + 30;
    live = h.be != 0u;
  }
  if (live && real) rt_block(sink, a1, u, pmax);
}

__device__ __forceinline__ void rt_values(const float* f, bool real, uint32_t pmax, uint32_t* step, uint32_t* imp,
                                          uint32_t copy)
{
  rt_values(f, real, pmax, RtLdsSink{step, imp, copy});
}

template <int DT>
__device__ __forceinline__ void rt_tile(const FieldDesc& F, const RtRaw<DT>& raw, uint32_t t, uint32_t pmax,
                                        uint32_t* step, uint32_t* imp, uint32_t copy)
{
  const uint64_t bl = (uint64_t)t * RT_TILE + (uint64_t)threadIdx.x * RTU;
#pragma unroll
  for (uint32_t k = 0; k < RTU; k++) {
    float f[4];
    raw.block(k, f);
    rt_values(f, bl + k < F.nblocks, pmax, step, imp, copy);
  }
}

// the workgroup's histograms zeroed (with the barrier), and at the end summed over the copies and added to the global
// workspace with 64-bit atomics (steps sign-extended): the caller has a barrier between its last update and the flush
__device__ __forceinline__ void rt_hist_zero(uint32_t* hist)
{
  for (uint32_t i = threadIdx.x; i < RT_HIST_WORDS; i += RTT) hist[i] = 0u;
  __syncthreads();
}

__device__ __forceinline__ void rt_hist_flush(const uint32_t* hist, unsigned long long* __restrict__ ws)
{
  for (uint32_t i = threadIdx.x; i < 2 * RT_BINS; i += RTT) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t c = 0; c < RT_COPIES; c++) s += hist[i * RT_COPIES + c];
    if (s) atomicAdd(ws + i, (unsigned long long)(long long)(int32_t)s);
  }
}

// rt_hist_flush that leaves the arrays zeroed for the next table (a workgroup that goes on to another tensor): the
// caller has a barrier before it, as for rt_hist_flush, and one after it before the next update
__device__ __forceinline__ void rt_hist_flush_zero(uint32_t* hist, unsigned long long* __restrict__ ws)
{
  for (uint32_t i = threadIdx.x; i < 2 * RT_BINS; i += RTT) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t c = 0; c < RT_COPIES; c++) {
      s += hist[i * RT_COPIES + c];
      hist[i * RT_COPIES + c] = 0u;
    }
    if (s) atomicAdd(ws + i, (unsigned long long)(long long)(int32_t)s);
  }
}

// ---------------------------------------------------------------------------------------------- direct chunks of a plan
// A direct chunk of a list plan (RtListDirect, RtRelDirect: in, out, nb and one more word) is up to 2048 whole blocks of
// one tensor whose first row is 4-byte aligned. It is read through a buffer resource over its nb rows by raw buffer
// loads, as two halves of RT_TILE blocks, each lane RTU consecutive rows (rate_table_list1d.hip has the reasons).
constexpr uint32_t RTL_HALF = RT_TILE;  // blocks per half chunk: 256 lanes x RTU
static_assert(kRtListChunkBlocks == 2 * RTL_HALF, "a direct chunk is two halves");

template <int DT> constexpr uint32_t rtl_row_bytes() { return DT == DT_BF16 ? 8u : 16u; }

__device__ __forceinline__ uint32_t rtl_sgpr(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// The input rows of direct chunk d as a buffer resource: num_records = the chunk's nb rows in bytes. d is uniform
// (derived from blockIdx and kernel arguments); readfirstlane makes every word provably so.
template <int DT, class Direct>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rtl_in_rows(const Direct* __restrict__ d)
{
  const uint64_t in = d->in;
  const uint32_t lo = rtl_sgpr((uint32_t)in), hi = rtl_sgpr((uint32_t)(in >> 32));
  const uint32_t nb = min(rtl_sgpr(d->nb), kRtListChunkBlocks);
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0, (int)(nb * rtl_row_bytes<DT>()),
                                           0x00020000);
}

// the lane's RTU consecutive rows of half h of a chunk, as raw words
template <int DT>
struct RtlRows {
  static constexpr int W = DT == DT_BF16 ? 2 : 4;  // dwords per row
  uint32_t d[RTU * W];
  __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rin, uint32_t h)
  {
    const uint32_t row = h * RTL_HALF + threadIdx.x * RTU;  // < 2048: offsets stay below 2^15
#pragma unroll
    for (uint32_t k = 0; k < RTU; k++) {
      const int off = (int)((row + k) * rtl_row_bytes<DT>());
      if constexpr (DT == DT_BF16) {
        const pipe_v2u v = __builtin_amdgcn_raw_buffer_load_b64(rin, off, 0, 0);
        d[2 * k] = v.x, d[2 * k + 1] = v.y;
      } else {
        const pipe_v4u v = __builtin_amdgcn_raw_buffer_load_b128(rin, off, 0, 0);
        d[4 * k] = v.x, d[4 * k + 1] = v.y, d[4 * k + 2] = v.z, d[4 * k + 3] = v.w;
      }
    }
  }
  __device__ __forceinline__ void block(uint32_t k, float* f) const
  {
    if constexpr (DT == DT_BF16) {
      f[0] = __uint_as_float(d[2 * k] << 16);
      f[1] = __uint_as_float(d[2 * k] & 0xffff0000u);
      f[2] = __uint_as_float(d[2 * k + 1] << 16);
      f[3] = __uint_as_float(d[2 * k + 1] & 0xffff0000u);
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++) f[i] = __uint_as_float(d[4 * k + i]);
    }
  }
};

template <int DT>
__device__ __forceinline__ void rtl_half(const RtlRows<DT>& rows, uint32_t pmax, uint32_t* step, uint32_t* imp,
                                         uint32_t copy)
{
#pragma unroll
  for (uint32_t k = 0; k < RTU; k++) {
    float f[4];
    rows.block(k, f);
    rt_values(f, true, pmax, step, imp, copy);  // a row past the chunk is a zero block
  }
}

}  // namespace gcow
