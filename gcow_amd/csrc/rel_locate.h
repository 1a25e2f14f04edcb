// rel_locate.h -- a gather block of the relative form's plan (gcow_roundtrip_rel_plan; kernels.h RtRel*) found from its
// virtual number, shared by the round trip (roundtrip_rel1d.hip) and the table pass (rate_table_rel1d.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace gcow {

__device__ __forceinline__ uint32_t rel_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// Virtual block vb0 + i of a gather chunk: the last piece that starts at or before it (at most log2(pieces of the
// chunk) steps), then the block's place in that piece's tensor.
struct RelBlock {
  const char* in;
  char* out;
  uint64_t x0;  // the block's first value in its tensor
  uint32_t nv;  // real values, 1 .. 4
  uint32_t seg;
};

__device__ __forceinline__ uint32_t rel_locate_piece(const RtRelGather& c, const RtRelPiece* __restrict__ pieces,
                                                     uint32_t i)
{
  const uint32_t v = c.vb0 + i;
  uint32_t lo = c.p_lo, hi = c.p_hi;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (pieces[mid].vb <= v) lo = mid;
    else hi = mid - 1u;
  }
  return lo;
}

__device__ __forceinline__ RelBlock rel_locate(const RtRelGather& c, const RtRelPiece* __restrict__ pieces, uint32_t i)
{
  const uint32_t v = c.vb0 + i;
  const RtRelPiece e = pieces[rel_locate_piece(c, pieces, i)];
  RelBlock b;
  b.in = (const char*)e.in;
  b.out = (char*)e.out;
  b.x0 = 4ull * ((uint64_t)e.b0 + (v - e.vb));
  b.nv = (uint32_t)min<uint64_t>(4, e.n - b.x0);
  b.seg = e.seg;
  return b;
}

}  // namespace gcow
