// var1d_prep.h -- one 1-D block's coefficients, precision and bit length in closed form, for parameter sets whose
// budget never truncates a block (minbits <= 1, maxbits >= 160), and the block's decode from those coefficients without
// a stream: shared by the variable-rate encoder and its residual form (var1d.hip), the fused round trip
// (roundtrip1d.hip) and the fixed-rate residual encoder (enc_resid1d.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec_device.h"
#include "lean1d.h"
#include "regbits.h"

namespace gcow {

// v_lshlrev_b32 as an opaque instruction: the shift count's low 5 bits (a count of 32 shifts by 0, not UB)
__device__ __forceinline__ uint32_t shl_hw(uint32_t x, uint32_t n)
{
  uint32_t r;
  asm("v_lshlrev_b32 %0, %1, %2" : "=v"(r) : "v"(n), "v"(x));
  return r;
}

// One block's header, coefficients and bit length (encode_fblock's return value, sw/src/encode.c:457-495, for
// minbits <= 1 and maxbits >= 160). cexp = -122 - minexp (precision = emax - minexp + 4, emax = E - 126 for the
// biased exponent E of max |f|: subnormal maxima, E = 0, clamp to -126). hdr = the 9-bit header 2 (emax + 127) + 1,
// or 0 for a one-bit block (zero block or no precision); K = 31 - kmin. inf: Inf / NaN present (the generic coder takes the block).
__device__ __forceinline__ uint32_t v1_prep(const float* f, int cexp, int maxprec, uint32_t* u, uint32_t& hdr,
                                            uint32_t& K, bool& inf)
{
  uint32_t m;  // max |f| as bits (v_max3 with |.| modifiers; NaN is caught below, it never wins encode.c:146-150)
  asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(m) : "v"(f[0]), "v"(f[1]), "v"(f[2]));
  asm("v_max_f32_e64 %0, %0, |%1|" : "+v"(m) : "v"(f[3]));
  inf = m > 0x7f7fffffu || __builtin_isunordered(f[0], f[1]) || __builtin_isunordered(f[2], f[3]);
  const uint32_t E = m >> 23;
  // get_precision, d = 1 (common.c:226-229); subnormal maxima clamp emax to -126 (encode.c:142-152)
  // K = min(prec, 32) - 1 clamped to 0 = clamp(E + cexp - 1, 0, min(maxprec, 32) - 1); the block is a single bit
  // when prec = 0, i.e. E + cexp <= 0 or maxprec = 0
  const int ep = (int)E + cexp, kmax = min(maxprec, 32) - 1;  // kmax < 0: maxprec = 0, every block one bit
  K = (uint32_t)max(min(ep - 1, kmax), 0);
  const float s = __uint_as_float(0x8d800000u - (m & 0x7f800000u));  // 2^(30 - emax)
  // every value of a block with E < 29 casts to INT_MIN (the scale overflows; x86 cvttss2si, encode.c:162-187):
  // an integer mask selects it per value (v_bfi), no compare-to-mask selects
  const uint32_t tm = (uint32_t)((int32_t)(E - 29u) >> 31);
  auto cast = [&](float v) { return ((uint32_t)cvt_i32_hw(v * s) & ~tm) | (tm & 0x80000000u); };
  uint32_t x = cast(f[0]), y = cast(f[1]), z = cast(f[2]), w = cast(f[3]);
  auto asr = [](uint32_t v) { return (uint32_t)((int32_t)v >> 1); };
  constexpr uint32_t NB = 0xaaaaaaaau;
  x = asr(x + w); w -= x;  // fwd_lift (encode.c:212-225), int32 wraparound
  z = asr(z + y); y -= z;
  x = asr(x + z); z -= x;
  w = asr(w + y); y -= w;
  w += asr(y); y -= asr(w);
  u[0] = (x + NB) ^ NB;  // twoscomplement_to_negabinary (encode.c:263-275)
  u[1] = (y + NB) ^ NB;
  u[2] = (z + NB) ^ NB;
  u[3] = (w + NB) ^ NB;
  const bool one = m == 0 || ep <= 0 || kmax < 0;  // a single 0 bit (encode.c:471-475; prec = 0)
  hdr = one ? 0u : 2u * E + 3u;
  // encode_ints' length from the leading planes (codec_device.h encode_ints_length, B = 4), integer-only:
  //   4 + 4 K - sum_{j<3} c_j + sum_{j<3} e_j,  c_j = min(z_j, K + 1), z_j = ffbh(S_j) of the suffix OR S_j,
  //   e_j = [c_j <= K and bit 31 - z_j of u_j is set] (L_j = R_j: u_j holds the leading plane of S_j)
  // (the c = 4 case of the general form folded in; tests/test_length_formula.py checks it against the oracle)
  const uint32_t S2 = u[2] | u[3], S1 = u[1] | S2, S0 = u[0] | S1;
  const uint32_t K1 = K + 1u;
  const uint32_t c2 = min(ffbh_hw(S2), K1), c1 = min(ffbh_hw(S1), K1), c0 = min(ffbh_hw(S0), K1);
  const uint32_t e2 = (shl_hw(u[2], c2) >> 31) & min(K1 - c2, 1u);  // c_j = 32 (K = 31, S_j = 0): e_j = 0
  const uint32_t e1 = (shl_hw(u[1], c1) >> 31) & min(K1 - c1, 1u);
  const uint32_t e0 = (shl_hw(u[0], c0) >> 31) & min(K1 - c0, 1u);
  const uint32_t len = 4u + 4u * K - (c0 + c1 + c2) + (e0 + e1 + e2);
  return one ? 1u : 9u + len;
}

// The front of v1_prep alone, for callers that need the coefficients but no parameter set (rate_table1d.hip): u as
// v1_prep forms them, which do not depend on minexp (the cast scales by the block's own exponent). Returns max |f| as
// bits: the biased exponent is E = m >> 23 (emax = E - 126), m == 0 an all-zero block. inf: Inf / NaN present (the
// caller takes prepare_block<1>).
__device__ __forceinline__ uint32_t v1_coeffs(const float* f, uint32_t* u, bool& inf)
{
  uint32_t m;
  asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(m) : "v"(f[0]), "v"(f[1]), "v"(f[2]));
  asm("v_max_f32_e64 %0, %0, |%1|" : "+v"(m) : "v"(f[3]));
  inf = m > 0x7f7fffffu || __builtin_isunordered(f[0], f[1]) || __builtin_isunordered(f[2], f[3]);
  const uint32_t E = m >> 23;
  const float s = __uint_as_float(0x8d800000u - (m & 0x7f800000u));  // 2^(30 - emax)
  const uint32_t tm = (uint32_t)((int32_t)(E - 29u) >> 31);          // E < 29: every value casts to INT_MIN
  auto cast = [&](float v) { return ((uint32_t)cvt_i32_hw(v * s) & ~tm) | (tm & 0x80000000u); };
  uint32_t x = cast(f[0]), y = cast(f[1]), z = cast(f[2]), w = cast(f[3]);
  auto asr = [](uint32_t v) { return (uint32_t)((int32_t)v >> 1); };
  constexpr uint32_t NB = 0xaaaaaaaau;
  x = asr(x + w); w -= x;  // fwd_lift
  z = asr(z + y); y -= z;
  x = asr(x + z); z -= x;
  w = asr(w + y); y -= w;
  w += asr(y); y -= asr(w);
  u[0] = (x + NB) ^ NB;
  u[1] = (y + NB) ^ NB;
  u[2] = (z + NB) ^ NB;
  u[3] = (w + NB) ^ NB;
  return m;
}

// The decode of a block no budget truncated, from v1_prep's u, hdr and K (K = 31 - kmin): an untruncated code holds
// planes 31 .. kmin of every coefficient whole, so the decoder's coefficients are u_j with the planes below kmin
// cleared; a block whose header is the single '0' bit (hdr = 0: a zero block, or no precision) decodes to +0. Then the
// inverse negabinary map, inv_lift and dequant_scale(emax) * (float)q as decode_block has it (scale first, one
// multiply: a subnormal maximum decodes to +-0). Not for blocks with Inf / NaN (v1_prep's inf): rt_block_generic.
__device__ __forceinline__ void v1_decode_closed(const uint32_t* u, uint32_t hdr, uint32_t K, float* d)
{
  const uint32_t keep = hdr ? ~((1u << (31u - K)) - 1u) : 0u;
  int32_t q[4];
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = (int32_t)(((u[i] & keep) ^ 0xaaaaaaaau) - 0xaaaaaaaau);
  inv_lift(q[0], q[1], q[2], q[3]);
  const float sc = dequant_scale((int)(hdr >> 1) - 127);  // hdr = 2 (emax + 127) + 1; hdr = 0: q = 0, any finite scale
#pragma unroll
  for (int i = 0; i < 4; i++) d[i] = sc * (float)q[i];
}

// Any parameter set: the block's code in three registers, decoded from them. Returns the block's bit length
// (encode_block's return value: minbits padding and the maxbits cut included).
__device__ __forceinline__ uint32_t rt_block_generic(const float* f, const Params& p, float* d)
{
  RegWriter192 wr{0ull, 0ull, 0ull, 0u};
  const uint32_t len = encode_block<1>(wr, f, p);
  RegReader192 rd{wr.w0, wr.w1, wr.w2};
  decode_block<1>(rd, p, d);
  return len;
}

// y - d as one IEEE subtract (no contraction, denormals kept); a non-finite result (NaN / Inf gradient, x + e overflow)
// carries nothing forward
__device__ __forceinline__ uint32_t resid_bits(float y, float d)
{
  const uint32_t r = __float_as_uint(__fsub_rn(y, d));
  return (r & 0x7f800000u) == 0x7f800000u ? 0u : r;
}

// The parameter set of the device-parameter ("fitted") kernels (gcow_encode_fitted_device, gcow_roundtrip_fitted_device,
// include/gcow.h): accuracy mode at the minexp a word of device memory holds, clamped to the rate table's range
// [-154, 133] -- outside it the stream no longer changes (gcow.h "the range is complete"), and inside it emax - minexp
// cannot leave int whatever the word holds. Called once at the top of a kernel: the address is a kernel argument, so
// the load is uniform (a scalar load, which counts in lgkmcnt and not in vmcnt).
// WAITED, for kernels that issue loads from inline asm and count vmcnt by hand: the empty asm takes the clamped value
// in an SGPR, so the compiler has waited for the word -- on whichever counter its load counts -- before that point, and
// no asm statement moves across it. Called before the kernel's first asm load, the hand-counted waits therefore see
// exactly the loads they count: none is outstanding when the first of them is issued.
constexpr int32_t kFitMinExpLo = -154, kFitMinExpHi = 133;
template <bool WAITED>
__device__ __forceinline__ Params fitted_params_dev(uint32_t maxprec, const int32_t* __restrict__ d_minexp)
{
  int m = __builtin_amdgcn_readfirstlane(min(max(*d_minexp, kFitMinExpLo), kFitMinExpHi));
  if constexpr (WAITED) asm volatile("" : "+s"(m) : : "memory");
  return Params{1u, 16658u, maxprec, m};
}

// Where a kernel's parameter set comes from: a template parameter of the kernels that exist for both cases, passed by
// value as a kernel argument. The kernel calls get once at its top -- with WAITED = true, ahead of its first asm load,
// where it counts vmcnt by hand (the rule above).
struct ParamsHost {  // the launch's own Params
  Params p;
  template <bool WAITED>
  __device__ __forceinline__ Params get() const
  {
    return p;
  }
};
struct ParamsDev {  // accuracy mode at the minexp word in device memory
  uint32_t maxprec;
  const int32_t* d_minexp;
  template <bool WAITED>
  __device__ __forceinline__ Params get() const
  {
    return fitted_params_dev<WAITED>(maxprec, d_minexp);
  }
};

}  // namespace gcow
