// rtlist_gather.h -- one block of a gather chunk of a tensor-list plan (kernels.h RtList*), located and loaded: the
// address arithmetic of k_roundtrip_list_gather (roundtrip_list1d.hip, which keeps its own text of it) for the kernels
// added since: its device-parameter twin and the rate table over the plan (rate_table_list1d.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field_io.h"
#include "kernels.h"

namespace gcow {

// Block i of chunk c (act: i is below the chunk's block count; else nothing is read and f stays zero). The segment of
// the block's first value is found by bisection between the segments of the chunk's first and last value, then the
// walk goes forward: segments are non-empty, so four values cross at most three seams. f: the four values, padded by
// pad_index's rule (field_io.h; encode.c:41-60), a bf16 input widened exactly. OE: bytes per output element, and
// o[x] = the address value x is written to (real values only); OE = 0: inputs only, o untouched. Returns the number
// of real values.
template <int DT_IN, uint32_t OE>
__device__ __forceinline__ uint32_t rtl_gather_block(const RtListGather& c, const RtListSeg* __restrict__ segs,
                                                     uint64_t nvals, uint32_t i, bool act, float* f, char** o)
{
  const uint64_t x0 = 4ull * ((uint64_t)c.b0 + i);
  const uint32_t nv = act ? (uint32_t)min<uint64_t>(4, nvals - x0) : 0u;
  if (act) {
    uint32_t lo = c.seg_lo, hi = c.seg_hi;
    while (lo < hi) {  // the last segment that starts at or before x0
      const uint32_t mid = (lo + hi + 1u) >> 1;
      if (segs[mid].start <= x0) lo = mid;
      else hi = mid - 1u;
    }
    uint32_t s = lo;
    uint64_t s0 = segs[s].start, s1 = segs[s + 1].start;  // the sentinel ends the table: start = nvals
    const char* ip = (const char*)segs[s].in;
    char* op = OE ? (char*)segs[s].out : nullptr;
#pragma unroll
    for (uint32_t x = 0; x < 4u; x++) {
      if (x < nv) {
        const uint64_t xi = x0 + x;
        while (xi >= s1) {
          s++;
          s0 = s1;
          s1 = segs[s + 1].start;
          ip = (const char*)segs[s].in;
          if constexpr (OE != 0) op = (char*)segs[s].out;
        }
        f[x] = load_elem<DT_IN>(ip, (int64_t)(xi - s0));
        if constexpr (OE != 0) o[x] = op + (xi - s0) * OE;
      }
    }
    // pad_index written out: 1 -> v0 v0 v0 v0, 2 -> v0 v1 v1 v0, 3 -> v0 v1 v2 v0
    if (nv < 2u) f[1] = f[0];
    if (nv < 3u) f[2] = nv == 2u ? f[1] : f[0];
    if (nv < 4u) f[3] = f[0];
  }
  return nv;
}

}  // namespace gcow
