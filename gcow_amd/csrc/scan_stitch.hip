// scan_stitch.hip -- stream utilities: the range scans (k_scan_ranges, k_scan_ranges_mw), the header prepend, the
// shard bit-stitch (multi-GPU variable rate), the packed16 index and small helpers, with their launchers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>

#include "kernels.h"

namespace gcow {

// ------------------------------------------------------------------------------------------------ scans
__device__ __forceinline__ uint64_t wave_incl_scan64(uint64_t x)
{
  const uint32_t lane = __lane_id();
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const uint32_t lo = __shfl_up((uint32_t)x, o), hi = __shfl_up((uint32_t)(x >> 32), o);
    if (lane >= o) x += (uint64_t)lo | ((uint64_t)hi << 32);
  }
  return x;
}

// Exclusive scan of the range totals (one workgroup). base[] gets nranges + 1 entries (last = total bits); the
// 32-bit words two ranges share are zeroed so both sides can atomicOr into them; the stream's flush word too.
// d_base (optional): the stream already holds *d_base bits (chunked / appended encode); every offset starts there and
// the first range ORs its first word into the bits before it. Where *d_base lies inside a 32-bit word, that word holds
// the end of the earlier stream (zero above it) and is never zeroed here, not even for a later range that starts in it
// (4-D: a range is one block, and a block can be a single bit).
// One workgroup: the range totals are read in coalesced chunks of 8192 through LDS (each thread then scans 8
// consecutive totals; wave prefix by shuffles, 16 wave totals through LDS), so every global access is coalesced --
// a per-thread walk over its own contiguous slice touched 64 cache lines per wave load (82 us at 32 Ki ranges).
__global__ __launch_bounds__(1024) void k_scan_ranges(const uint64_t* __restrict__ sums, uint32_t nranges,
                                                      uint64_t* __restrict__ base, uint64_t* __restrict__ total,
                                                      uint32_t* __restrict__ out32, const uint64_t* __restrict__ d_base)
{
  constexpr uint32_t T = 1024, K = 8, C = T * K;
  __shared__ uint64_t v[C];
  __shared__ uint64_t wsum[T / 64];
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const uint64_t base0 = d_base ? *d_base : 0ull;
  const uint64_t keep = (base0 & 31) ? base0 >> 5 : ~0ull;  // the word of the earlier stream's end, if it is partial
  uint64_t carry = base0;
  for (uint32_t c0 = 0; c0 < nranges; c0 += C) {
    const uint32_t n = min(C, nranges - c0);
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
      const uint32_t j = t + T * k;
      v[j] = j < n ? sums[c0 + j] : 0ull;
    }
    __syncthreads();
    uint64_t loc[K], s = 0;
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
      loc[k] = v[t * K + k];
      s += loc[k];
    }
    const uint64_t incl = wave_incl_scan64(s);
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    uint64_t before = 0, chunk = 0;
#pragma unroll
    for (uint32_t w = 0; w < T / 64; w++) {
      const uint64_t x = wsum[w];
      before += w < wv ? x : 0ull;
      chunk += x;
    }
    uint64_t run = carry + before + incl - s;
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
      v[t * K + k] = run;
      run += loc[k];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
      const uint32_t j = t + T * k;
      if (j < n) {
        const uint64_t b = v[j];
        base[c0 + j] = b;
        // a word two ranges share: zeroed for their atomicOr
        if (c0 + j > 0 && (b & 31) && (b >> 5) != keep) out32[b >> 5] = 0u;
      }
    }
    carry += chunk;
    __syncthreads();
  }
  if (t == 0) {
    base[nranges] = carry;
    if (total) *total = carry;
  }
}

// Many-workgroup form of k_scan_ranges for up to kScanMwMax ranges: workgroup g scans ranges [1024 g, 1024 g + 1024)
// and finds its starting offset by summing every earlier range total itself (O(n^2 / 2048) loads in all, from L2:
// 0.5 M loads at 32 Ki ranges), so no second launch, no partials buffer and no inter-workgroup protocol.
constexpr uint32_t kScanMwMax = 1u << 16;

// gsums (optional): totals of consecutive groups of 8 ranges (the 1-D tile count writes them), so the earlier totals
// each workgroup sums are 1/8 as many.
__global__ __launch_bounds__(256) void k_scan_ranges_mw(const uint64_t* __restrict__ sums, uint32_t nranges,
                                                        uint64_t* __restrict__ base, uint64_t* __restrict__ total,
                                                        uint32_t* __restrict__ out32,
                                                        const uint64_t* __restrict__ d_base,
                                                        const uint64_t* __restrict__ gsums)
{
  constexpr uint32_t T = 256, K = 4, C = T * K;
  __shared__ uint64_t v[C];
  __shared__ uint64_t wsum[T / 64];
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const uint32_t c0 = blockIdx.x * C;
  const uint32_t n = min(C, nranges - c0);
#pragma unroll
  for (uint32_t k = 0; k < K; k++) {
    const uint32_t j = t + T * k;
    v[j] = j < n ? sums[c0 + j] : 0ull;
  }
  uint64_t pre = 0;  // every earlier range total (or group total), 8 loads in flight per thread
  const uint64_t* ps = gsums ? gsums : sums;
  const uint32_t pn = gsums ? c0 / 8u : c0;
  uint32_t i = t;
  for (; i + 7 * T < pn; i += 8 * T) {
    uint64_t a[8];
#pragma unroll
    for (int k = 0; k < 8; k++) a[k] = ps[i + k * T];
#pragma unroll
    for (int k = 0; k < 8; k++) pre += a[k];
  }
  for (; i < pn; i += T) pre += ps[i];
  __syncthreads();
  uint64_t loc[K], s = 0;
#pragma unroll
  for (uint32_t k = 0; k < K; k++) {
    loc[k] = v[t * K + k];
    s += loc[k];
  }
  const uint64_t incl = wave_incl_scan64(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)pre, o), hi = __shfl_xor((uint32_t)(pre >> 32), o);
    pre += (uint64_t)lo | ((uint64_t)hi << 32);
  }
  __shared__ uint64_t wpre[T / 64];
  if (lane == 63) wsum[wv] = incl;
  if (lane == 0) wpre[wv] = pre;
  __syncthreads();
  const uint64_t base0 = d_base ? *d_base : 0ull;
  const uint64_t keep = (base0 & 31) ? base0 >> 5 : ~0ull;  // as in k_scan_ranges
  uint64_t before = 0, chunk = 0, carry = base0;
#pragma unroll
  for (uint32_t w = 0; w < T / 64; w++) {
    before += w < wv ? wsum[w] : 0ull;
    chunk += wsum[w];
    carry += wpre[w];
  }
  uint64_t run = carry + before + incl - s;
#pragma unroll
  for (uint32_t k = 0; k < K; k++) {
    v[t * K + k] = run;
    run += loc[k];
  }
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < K; k++) {
    const uint32_t j = t + T * k;
    if (j < n) {
      const uint64_t b = v[j];
      base[c0 + j] = b;
      if (c0 + j > 0 && (b & 31) && (b >> 5) != keep) out32[b >> 5] = 0u;
    }
  }
  if (blockIdx.x == gridDim.x - 1 && t == 0) {
    base[nranges] = carry + chunk;
    if (total) *total = carry + chunk;
  }
}

static void scan_ranges(const uint64_t* sums, uint32_t nranges, uint64_t* base, uint64_t* total, uint32_t* out32,
                        const uint64_t* d_base, hipStream_t st, const uint64_t* gsums = nullptr)
{
  if (nranges > 4096 && (nranges <= kScanMwMax || gsums))
    k_scan_ranges_mw<<<(nranges + 1023) / 1024, 256, 0, st>>>(sums, nranges, base, total, out32, d_base, gsums);
  else
    k_scan_ranges<<<1, 1024, 0, st>>>(sums, nranges, base, total, out32, d_base);
}

__global__ void k_widen_u32(const uint32_t* __restrict__ a, uint32_t n, uint64_t* __restrict__ o)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) o[i] = a[i];
}

__global__ void k_set_u64(uint64_t* p, uint64_t v) { *p = v; }

// zfp_decompress's cache check: flag = 1 where the caller's device stream differs from the cached copy (plain
// vector stores of the same value; the flag was zeroed by a preceding launch on the stream)
__global__ void k_words_differ(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, uint64_t n,
                               uint64_t* __restrict__ flag)
{
  bool d = false;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    d = d || a[i] != b[i];
  if (d) *flag = 1ull;
}

// ------------------------------------------------------------------------------------------------ header stream
// dst = header bits [0, off) followed by src bits [0, *d_bits), flushed to whole words (zfp_write_header then
// zfp_compress at the following bit). Plain stores, one lane per destination word; lanes past the end exit. Lane 0
// also publishes the total bit count.
__global__ void k_prepend_header(uint64_t* __restrict__ dst, uint32_t off, const uint64_t* __restrict__ src,
                                 const uint64_t* __restrict__ d_bits, uint64_t h0, uint64_t h1, uint64_t h2,
                                 uint64_t* __restrict__ d_total)
{
  const uint64_t bits = *d_bits, end = off + bits;
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w == 0 && d_total) *d_total = end;
  if ((w << 6) >= end) return;
  const uint64_t nsw = (bits + 63) >> 6;
  uint64_t v = 0;
  if (w < 3 && (w << 6) < off) {  // header part of this word
    const uint64_t h = w == 0 ? h0 : (w == 1 ? h1 : h2);
    const uint64_t hb = off - (w << 6);
    v = hb >= 64 ? h : (h & ((1ull << hb) - 1ull));
  }
  const int64_t s = (int64_t)(w << 6) - (int64_t)off;  // source bit landing on bit 0 of dst[w]
  if (s + 64 > 0 && nsw) {
    if (s < 0) {
      v |= src[0] << (uint32_t)(-s);
    } else {
      const uint64_t i = (uint64_t)s >> 6;
      const uint32_t sh = (uint32_t)(s & 63);
      uint64_t x = i < nsw ? src[i] >> sh : 0ull;
      if (sh && i + 1 < nsw) x |= src[i + 1] << (64 - sh);
      v |= x;
    }
  }
  const uint64_t lo = w << 6;
  if (end < lo + 64) v &= (1ull << (end - lo)) - 1ull;  // end > lo here
  dst[w] = v;
}

// ------------------------------------------------------------------------------------------------ stitch
__global__ void k_stitch(uint64_t* __restrict__ dst, uint64_t off, const uint64_t* __restrict__ src, uint64_t bits)
{
  // dst bit range [off, off + bits) |= src bits [0, bits); one lane per destination word.
  const uint64_t w0 = off >> 6, w1 = (off + bits + 63) >> 6;
  const uint64_t w = w0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= w1) return;
  const uint64_t nsw = (bits + 63) >> 6;
  const int64_t s = (int64_t)(w << 6) - (int64_t)off;  // source bit that lands on bit 0 of dst[w]
  uint64_t v;
  if (s < 0) {
    v = src[0] << (uint32_t)(-s);
  } else {
    const uint64_t i = (uint64_t)s >> 6;
    const uint32_t sh = (uint32_t)(s & 63);
    v = src[i] >> sh;
    if (sh && i + 1 < nsw) v |= src[i + 1] << (64 - sh);
  }
  const uint64_t lo = w << 6;
  if (off + bits < lo + 64) v &= (1ull << (off + bits - lo)) - 1ull;  // off + bits > lo here
  dst[w] |= v;
}

// All shard streams in one launch (the receive side of a variable-rate all-gather): shard r
// holds lens[r] bits at src + r * shard_words and lands at bit O_r = lens[0] + ... + lens[r - 1] (a per-lane running
// sum over the shards: nshards is the world size). One lane per destination word, which it writes whole -- the OR of
// every shard's bits that fall on it, zero past the stream's end -- so dst needs no zeroing and no atomics.
__global__ __launch_bounds__(256) void k_stitch_shards(uint64_t* __restrict__ dst, uint64_t dst_words,
                                                       const uint64_t* __restrict__ src, uint64_t shard_words,
                                                       const uint64_t* __restrict__ lens, uint32_t nshards)
{
  const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (w >= dst_words) return;
  const uint64_t lo = w << 6;
  uint64_t v = 0, off = 0;
  for (uint32_t r = 0; r < nshards; r++) {
    const uint64_t bits = lens[r];
    const uint64_t end = off + bits;
    if (bits && off < lo + 64 && end > lo) {
      const uint64_t* sr = src + (uint64_t)r * shard_words;
      const uint64_t nsw = (bits + 63) >> 6;
      const int64_t sb = (int64_t)lo - (int64_t)off;  // shard bit landing on bit 0 of dst[w]
      uint64_t x;
      if (sb < 0) {
        x = sr[0] << (uint32_t)(-sb);  // -sb < 64: the shard starts inside this word
      } else {
        const uint64_t i = (uint64_t)sb >> 6;  // < nsw: sb < bits
        const uint32_t sh = (uint32_t)(sb & 63);
        x = sr[i] >> sh;
        if (sh && i + 1 < nsw) x |= sr[i + 1] << (64 - sh);
      }
      if (end < lo + 64) x &= (1ull << (end - lo)) - 1ull;  // drop the shard's own flush padding
      v |= x;
    }
    off = end;
  }
  dst[w] = v;
}

// GCOW_INDEX_PACKED16 from an index every 8 blocks: entry c = idx8[2c] | (idx8[2c + 1] - idx8[2c]) << 48 (offset 0
// where block 16 c + 8 does not exist).
__global__ __launch_bounds__(256) void k_index_pack16(const uint64_t* __restrict__ idx8, uint64_t n8,
                                                      uint64_t* __restrict__ out, uint64_t n16)
{
  const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (c >= n16) return;
  const uint64_t a = idx8[2 * c];
  const uint64_t d = 2 * c + 1 < n8 ? idx8[2 * c + 1] - a : 0ull;
  out[c] = a | (d << 48);
}

// ------------------------------------------------------------------------------------------------ launchers
static inline hipStream_t S(void* s) { return (hipStream_t)s; }

// exclusive scan of per-block lengths: one "range" per block through k_scan_ranges (which also zeroes the words
// two blocks share); d_base as there (the 4-D appended encode)
hipError_t launch_scan_blocks(const uint32_t* lens, uint32_t nblocks, uint64_t* sums, uint64_t* base, uint64_t* total,
                              uint32_t* out32, const uint64_t* d_base, void* stream)
{
  k_widen_u32<<<(nblocks + 255) / 256, 256, 0, S(stream)>>>(lens, nblocks, sums);
  scan_ranges(sums, nblocks, base, total, out32, d_base, S(stream));
  return hipGetLastError();
}

hipError_t launch_scan_ranges(const uint64_t* sums, uint32_t nranges, uint64_t* base, uint64_t* total, uint32_t* out32,
                              const uint64_t* d_base, void* stream, const uint64_t* gsums)
{
  scan_ranges(sums, nranges, base, total, out32, d_base, S(stream), gsums);
  return hipGetLastError();
}

hipError_t launch_set_u64(uint64_t* p, uint64_t v, void* stream)
{
  k_set_u64<<<1, 1, 0, S(stream)>>>(p, v);
  return hipGetLastError();
}

hipError_t launch_words_differ(const uint64_t* a, const uint64_t* b, uint64_t n, uint64_t* flag, void* stream)
{
  k_set_u64<<<1, 1, 0, S(stream)>>>(flag, 0ull);
  if (n) {
    const uint64_t g = std::min<uint64_t>((n + 255) / 256, 4096);
    k_words_differ<<<(uint32_t)g, 256, 0, S(stream)>>>(a, b, n, flag);
  }
  return hipGetLastError();
}

hipError_t launch_prepend_header(uint64_t* dst, uint32_t off, const uint64_t* src, const uint64_t* d_bits,
                                 const uint64_t* header, uint64_t max_words, uint64_t* d_total, void* stream)
{
  const uint64_t grid = (max_words + 255) / 256;
  k_prepend_header<<<(uint32_t)(grid ? grid : 1), 256, 0, S(stream)>>>(dst, off, src, d_bits, header[0], header[1],
                                                                      header[2], d_total);
  return hipGetLastError();
}

hipError_t launch_stitch(uint64_t* dst, uint64_t off, const uint64_t* src, uint64_t bits, void* stream)
{
  if (!bits) return hipSuccess;
  const uint64_t words = ((off + bits + 63) >> 6) - (off >> 6);
  const uint64_t grid = (words + 255) / 256;
  k_stitch<<<grid, 256, 0, S(stream)>>>(dst, off, src, bits);
  return hipGetLastError();
}

hipError_t launch_stitch_shards(uint64_t* dst, uint64_t dst_words, const uint64_t* src, uint64_t shard_words,
                                const uint64_t* lens, uint32_t nshards, void* stream)
{
  const uint64_t grid = (dst_words + 255) / 256;
  if (!grid) return hipSuccess;
  k_stitch_shards<<<(uint32_t)grid, 256, 0, S(stream)>>>(dst, dst_words, src, shard_words, lens, nshards);
  return hipGetLastError();
}

hipError_t launch_index_pack16(const uint64_t* idx8, uint64_t n8, uint64_t* out, void* stream)
{
  const uint64_t n16 = (n8 + 1) / 2;
  if (!n16) return hipSuccess;
  k_index_pack16<<<(uint32_t)((n16 + 255) / 256), 256, 0, S(stream)>>>(idx8, n8, out, n16);
  return hipGetLastError();
}

}  // namespace gcow
