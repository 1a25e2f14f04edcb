// rel_minexp.h -- the one definition of the relative tolerance's word: a tensor's minexp from its largest finite
// magnitude (include/gcow.h gcow_roundtrip_rel_device). Shared by the round trip over a tensor list
// (roundtrip_rel1d.hip: rel_params builds its Params from it) and the words pass of a segmented field
// (seg_resid1d.hip: k_seg_rel_words writes it where the segmented kernels read it). The text is roundtrip_rel1d.hip's,
// moved here unchanged (its kernels compile to the instructions they had: profiles/r20_segrel_rel1d_isa_diff.log).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace gcow {

// |x| as bits, 0 for Inf / NaN
__device__ __forceinline__ uint32_t rel_mag(uint32_t bits)
{
  const uint32_t a = bits & 0x7fffffffu;
  return a < 0x7f800000u ? a : 0u;
}

// The tensor's minexp from its largest finite magnitude (as bits): emax = (a >> 23) - 126, a subnormal or zero
// maximum gives -126. The floor keeps every block whose values all cast to INT_MIN (emax <= -98) at precision 0.
// The headroom cap keeps the decode finite: a value decodes to within 2^minexp of itself, so a tensor whose maximum
// lies in the top binade (emax = 128) needs a + 2^minexp < 2^128, or a finite value near the maximum comes back as
// Inf. With g = 2^128 - a = (2^24 - mantissa) 2^104 and hexp = floor(log2 g), minexp <= hexp - 2 leaves
// |decode| <= 2^128 - 3 g / 4, which is below the fp32 rounding boundary 2^128 - 2^103 since g >= 2^104. For
// emax <= 127, a + 2^minexp < 2^128 holds by itself and the cap is absent.
__device__ __forceinline__ int rel_minexp(uint32_t a, uint32_t rel_bits)
{
  const uint32_t E = a >> 23;
  int minexp = max((int)E - 126 - (int)rel_bits, kRtRelMinExpFloor);
  if (E == 254u) {
    const uint32_t gap = 0x1000000u - ((a & 0x7fffffu) | 0x800000u);  // 1 .. 2^23, in units of 2^104
    minexp = min(minexp, 104 + (31 - (int)__builtin_clz(gap)) - kRtRelHeadroom);
  }
  return minexp;
}

}  // namespace gcow
