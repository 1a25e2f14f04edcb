// regbits.h -- bit readers and writers over registers, for kernels that decode a block they have just coded without
// the stream in between: the fused encode + residual kernel (enc_resid1d.hip) and the fused round trip
// (roundtrip1d.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec_device.h"

namespace gcow {

// The word a block was just coded to, read back by the generic decoder (the decoders' special lanes): the stream
// store is non-temporal and not visible yet, so the word comes from the register. Bits past the word read as zero;
// the block's budget (maxbits) keeps the decoder inside it.
struct RegReader64 {
  uint64_t w;
  uint32_t pos;
  __device__ __forceinline__ uint64_t peek64() const { return pos < 64u ? w >> pos : 0ull; }
  __device__ __forceinline__ uint64_t get(uint32_t n)
  {
    if (!n) return 0;
    const uint64_t v = peek64() & lowmask64(n);
    pos += n;
    return v;
  }
  __device__ __forceinline__ uint32_t bit()
  {
    const uint32_t b = (uint32_t)peek64() & 1u;
    pos++;
    return b;
  }
  __device__ __forceinline__ void skip(uint64_t k) { pos += (uint32_t)k; }
};

// The first 192 bits of a block's code in three registers (the longest 1-D block code is 9 + 3 + 4 * 32 = 140 bits;
// what a coder appends past that is zero padding up to minbits, which only moves pos). The word a value lands in is
// chosen by selects, never by an index, so the three words stay in registers.
struct RegWriter192 {
  uint64_t w0, w1, w2;
  uint32_t pos;
  __device__ __forceinline__ void put(uint64_t v, uint32_t n)
  {
    const uint32_t i = pos >> 6, sh = pos & 63u;
    const uint64_t lo = v << sh, hi = sh ? v >> (64u - sh) : 0ull;
    w0 |= i == 0 ? lo : 0ull;
    w1 |= i == 1 ? lo : (i == 0 ? hi : 0ull);
    w2 |= i == 2 ? lo : (i == 1 ? hi : 0ull);
    pos += n;
  }
  __device__ __forceinline__ void skip(uint32_t n) { pos += n; }
};

// Reader over the same three registers, kept as one 192-bit value that is shifted down as bits are consumed (w0's low
// bit is the next stream bit); every bit past bit 192 reads as zero.
struct RegReader192 {
  uint64_t w0, w1, w2;
  __device__ __forceinline__ uint64_t peek64() const { return w0; }
  __device__ __forceinline__ void skip(uint64_t k)
  {
    uint32_t n = (uint32_t)(k < 192u ? k : 192u);
    if (n >= 128u) {
      w0 = w2;
      w1 = w2 = 0ull;
      n -= 128u;
    } else if (n >= 64u) {
      w0 = w1;
      w1 = w2;
      w2 = 0ull;
      n -= 64u;
    }
    if (n == 64u) {
      w0 = w1;
      w1 = w2;
      w2 = 0ull;
    } else if (n) {
      w0 = (w0 >> n) | (w1 << (64u - n));
      w1 = (w1 >> n) | (w2 << (64u - n));
      w2 >>= n;
    }
  }
  __device__ __forceinline__ uint64_t get(uint32_t n)
  {
    if (!n) return 0;
    const uint64_t v = w0 & lowmask64(n);
    skip(n);
    return v;
  }
  __device__ __forceinline__ uint32_t bit()
  {
    const uint32_t b = (uint32_t)w0 & 1u;
    skip(1);
    return b;
  }
};

}  // namespace gcow
