// enc_fixed1d.h -- the per-block coders of the fixed-rate 1-D encoders, shared by the encoder (enc_fixed1d.hip) and the
// fused encode + residual kernel (enc_resid1d.hip): the padded block load, the generic whole-word coder
// encode_block1d_fixed and the lean-6 closed-form coder encode_block1d_lean6 (tables and helpers: lean1d.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec_device.h"
#include "field_io.h"
#include "lean1d.h"

namespace gcow {

// ------------------------------------------------------------------------------------------------ 1-D fast path
template <int DT>
__device__ __forceinline__ void load_block1d(const void* in, uint64_t nvals, uint32_t b, float* f)
{
  const uint64_t i0 = 4ull * b;
  if (i0 + 4 <= nvals) {
    load_row4<DT>(in, (int64_t)i0, f);
  } else {
    const uint32_t nv = (uint32_t)(nvals - i0);
#pragma unroll
    for (int x = 0; x < 4; x++) f[x] = load_elem<DT>(in, (int64_t)(i0 + pad_index(x, nv)));
  }
}

// Spread the low 16 bits of x to the even bit positions of a 32-bit word.
__device__ __forceinline__ uint32_t spread2_16(uint32_t x)
{
  x = (x | (x << 8)) & 0x00FF00FFu;
  x = (x | (x << 4)) & 0x0F0F0F0Fu;
  x = (x | (x << 2)) & 0x33333333u;
  x = (x | (x << 1)) & 0x55555555u;
  return x;
}

// 4-way bit interleave of four 16-bit values: bit 4j + i of the result = bit j of value i.
__device__ __forceinline__ uint64_t interleave4_16(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
  const uint32_t P = spread2_16(a) | (spread2_16(c) << 1);  // a_j at 2j, c_j at 2j+1
  const uint32_t Q = spread2_16(b) | (spread2_16(d) << 1);  // b_j at 2j, d_j at 2j+1
  const uint32_t lo = spread2_16(P & 0xffffu) | (spread2_16(Q & 0xffffu) << 1);
  const uint32_t hi = spread2_16(P >> 16) | (spread2_16(Q >> 16) << 1);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

// One 4-value block -> WB bits (WB = 32 or 64), header included (sw/src/encode.c:457-495 for d = 1).
// The embedded coder (encode.c:279-339) is evaluated in three closed-form phases from the coefficients' leading
// one-bit planes L_i (M0 = max L_i): planes above M0 are empty and cost one '0' bit each (n = 0); planes M0..L3
// run the group tests through the LDS plane table while n < 4; from plane L3 - 1 down every coefficient is
// significant (n = 4) and each plane is its 4 bits verbatim, i.e. a contiguous run of the 4-way interleave of the
// bit-reversed coefficients, built with shift/mask spreads instead of a per-plane loop.
template <uint32_t WB>
__device__ __forceinline__ uint64_t encode_block1d_fixed(const float* f, const Params& p, const uint16_t* tab)
{
  float fa[4] = {f[0], f[1], f[2], f[3]};
  const int emax = block_emax<4>(fa);
  const uint32_t prec = precision(emax, p.maxprec, p.minexp, 1);
  if (!prec || emax == -127) return 0ull;  // zero block: one 0 bit padded with zeros
  const float s = cast_scale(emax);
  int32_t q[4];
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = cast1(fa[i], s);
  fwd_lift(q[0], q[1], q[2], q[3]);
  uint32_t u[4];
#pragma unroll
  for (int i = 0; i < 4; i++) u[i] = ((uint32_t)q[i] + 0xaaaaaaaau) ^ 0xaaaaaaaau;
  const int kmin = prec < 32 ? 32 - (int)prec : 0;
  uint64_t acc = 2ull * (uint32_t)(emax + 127) + 1ull;
  uint32_t pos = 9;
  {
    // leading one-bit plane of each coefficient (-1 for zero)
    const int L0 = 31 - (int)__builtin_clz(u[0] | 1u) - (u[0] ? 0 : 1);
    const int L1 = 31 - (int)__builtin_clz(u[1] | 1u) - (u[1] ? 0 : 1);
    const int L2 = 31 - (int)__builtin_clz(u[2] | 1u) - (u[2] ? 0 : 1);
    const int L3 = 31 - (int)__builtin_clz(u[3] | 1u) - (u[3] ? 0 : 1);
    const int M0 = max(max(L0, L1), max(L2, L3));
    // phase 1: empty planes 31 .. max(M0, kmin - 1) + 1, one '0' bit each
    const int top = max(M0, kmin - 1);
    pos += (uint32_t)(31 - top);
    // phase 2: group tests while n < 4 (planes top .. max(L3, kmin))
    uint32_t n = 0;
    const int glo = max(L3, kmin);
    for (int k = top; k >= glo && pos < WB; --k) {
      const uint32_t x = ((u[0] >> k) & 1u) | (((u[1] >> k) & 1u) << 1) | (((u[2] >> k) & 1u) << 2) |
                         (((u[3] >> k) & 1u) << 3);
      const uint32_t e = tab[(n << 4) | x];
      acc |= (uint64_t)(e & 127u) << pos;
      pos += (e >> 7) & 7u;
      n = e >> 10;
    }
    // phase 3: all significant: planes L3-1 .. kmin verbatim (at most 16 planes are ever needed here)
    const int kt = L3 - 1;
    if (pos < WB && kt >= kmin) {
      const uint32_t sh = (uint32_t)(31 - kt);
      const uint32_t g0 = __builtin_bitreverse32(u[0]) >> sh, g1 = __builtin_bitreverse32(u[1]) >> sh;
      const uint32_t g2 = __builtin_bitreverse32(u[2]) >> sh, g3 = __builtin_bitreverse32(u[3]) >> sh;
      uint64_t J = interleave4_16(g0 & 0xffffu, g1 & 0xffffu, g2 & 0xffffu, g3 & 0xffffu);
      const uint32_t cnt = (uint32_t)(kt - kmin + 1);  // planes available
      if (cnt < 16) J &= (1ull << (4 * cnt)) - 1ull;
      acc |= J << pos;
    }
  }
  return WB == 64 ? acc : (acc & ((1ull << WB) - 1ull));
}

// Lean-6 block: the lean-5 stream (encode.c:457-495 for d = 1, fixed rate, kmin = 0) with
//  * the block maximum as a float max3 of |f| (NaN caught by two unordered compares: it never wins the maximum,
//    encode.c:146-150, but it casts to INT_MIN, so such blocks take the generic coder);
//  * the lift and the negabinary map fused, the map's add folded into the last lifting add where there is one;
//  * the window from window_lds;
//  * the group-phase end jg = clz(u2 | u3) - sh, with 31 for o23 = 0 (jg = M0);
//  * zero blocks coded by the main path (u = 0 codes to all-zero bits after a zero header), so only tiny-normal and
//    subnormal maxima (0 < E < 29) take the constant payload.
template <uint32_t WB, bool W2LOW = false>
__device__ __forceinline__ uint64_t encode_block1d_lean6(const float* f, const uint32_t* tab, const uint32_t* rs,
                                                         bool& special)
{
  uint32_t m;  // max |f| as bits: v_max3_f32 / v_max_f32 with |.| modifiers (no canonicalising fmaxf)
  asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(m) : "v"(f[0]), "v"(f[1]), "v"(f[2]));
  asm("v_max_f32_e64 %0, %0, |%1|" : "+v"(m) : "v"(f[3]));
  special = m >= 0x7f800000u || __builtin_isunordered(f[0], f[1]) || __builtin_isunordered(f[2], f[3]);
  const uint32_t E = m >> 23;
  const float s = __uint_as_float((283u - E) << 23);  // 2^(30 - e); meaningless for tiny / special lanes
  uint32_t x = (uint32_t)cvt_i32_hw(f[0] * s), y = (uint32_t)cvt_i32_hw(f[1] * s);
  uint32_t z = (uint32_t)cvt_i32_hw(f[2] * s), w = (uint32_t)cvt_i32_hw(f[3] * s);
  // fwd_lift (encode.c:212-225), int32 wraparound; arithmetic shifts on the signed view
  auto asr = [](uint32_t v) { return (uint32_t)((int32_t)v >> 1); };
  constexpr uint32_t NB = 0xaaaaaaaau;
  x = asr(x + w); w -= x;
  z = asr(z + y); y -= z;
  x = asr(x + z); z -= x;
  w = asr(w + y); y -= w;
  const uint32_t u3 = (w + asr(y) + NB) ^ NB;  // w += y >> 1, then the negabinary map
  const uint32_t u1 = (y - asr(w + asr(y)) + NB) ^ NB;
  const uint32_t u0 = (x + NB) ^ NB, u2 = (z + NB) ^ NB;
  const uint32_t o23 = u2 | u3;
  const uint32_t sh = __builtin_clz(u0 | u1 | o23 | 1u);  // 31 - M0
  const int M0 = 31 - (int)sh;
  const int jg = (int)min(ffbh_hw(o23), 31u) - (int)sh;  // group phase: window nibbles 0 .. jg (o23 = 0: M0)
  const uint32_t w0 = u0 << sh, w1 = u1 << sh, w2 = u2 << sh, w3 = u3 << sh;
  const uint64_t Y = window_lds(rs, w0, w1, w2, w3);
  uint32_t pos = 9 + sh;
  uint32_t e = tab[(uint32_t)Y & 255u];
  uint32_t G = e >> 17, gl = (e >> 13) & 15u;
  // pair 1 for every lane, no wave vote (~92 % of waves take it anyway; profiles/r05_c2_pair1_vote_ab.log): past a
  // lane's group phase the table's rows n >= 3 code planes 2 and 3 as their verbatim nibbles, the bits the verbatim
  // run would give them
  int j = 4;
  e = tab5_next(tab, e, ((uint32_t)Y >> 8) & 255u);
  G |= (e >> 17) << gl;
  gl += (e >> 13) & 15u;
  const uint32_t hdr = m ? 2u * E + 3u : 0u;  // zero block: a single 0 bit, every later bit 0 as well
  uint64_t acc = (uint64_t)hdr | ((uint64_t)G << pos);
  pos += gl;
#pragma unroll
  for (int jj = 4; jj < 16; jj += 2) {
    if (j < jj || !__any(jj <= jg)) break;
    e = tab5_next(tab, e, (uint32_t)(Y >> (4 * jj)) & 255u);
    const uint32_t code = pos < WB ? (e >> 17) : 0u;  // 64-bit shifts wrap: nothing past the budget
    acc |= (uint64_t)code << pos;
    pos += (e >> 13) & 15u;
    j = jj + 2;
  }
  const bool tiny = m - 1u < (29u << 23) - 1u;  // 0 < E < 29: tiny-normal and subnormal maxima (coded below)
  special = special || (!tiny && jg >= 16 && pos < WB);  // group phase runs past the 16-plane window
  if (j < 16 && pos < WB) acc |= (Y >> (4 * j)) << pos;  // rest of the window, verbatim
  const uint32_t p2 = pos + 4u * (uint32_t)(16 - j);      // where plane M0 - 16 lands
  if (__any(p2 < WB && M0 >= 16)) {
    uint64_t Y2;  // planes M0-16 .. M0-31
    if constexpr (W2LOW) {
      Y2 = window_lds_low(rs, w0, w1, w2, w3);
    } else {
      const uint32_t s2 = sh + 16u;  // <= 31 where used (M0 >= 16)
      Y2 = window_lds(rs, u0 << s2, u1 << s2, u2 << s2, u3 << s2);
    }
    if (p2 < WB && M0 >= 16) acc |= Y2 << p2;
  }
  constexpr uint64_t TINY = tiny_payload_cx((int)WB - 9) << 9;
  acc = tiny ? (TINY | hdr) : acc;  // every value casts to INT_MIN
  return WB == 64 ? acc : (acc & ((1ull << WB) - 1ull));
}

}  // namespace gcow
