// dec1d.h -- the 1-D decode tables and per-block decoders shared by the 1-D decoders (dec1d.hip) and decode_mean
// (decode_mean.hip): the plane / pair / gather / lean-pair tables (__device__ const, so each unit that uses one
// carries its own copy), decode_block1d_fast / _pair (fixed rate, whole-word blocks), decode_block1d_var and
// dec_block1d_lean (variable rate) with their stream windows, and the 8 x 8 lane transpose of the whole-line stores.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec_device.h"

namespace gcow {

// Delta swap: exchanges the bits of x selected by m with the bits d positions above them (one index-bit swap of a
// bit-matrix transpose: one 64-bit shift pair and two 3-input bit ops).
__device__ __forceinline__ uint64_t dswap64(uint64_t x, uint64_t m, uint32_t d)
{
  const uint64_t t = ((x >> d) ^ x) & m;
  return x ^ t ^ (t << d);
}

// ------------------------------------------------------------------------------------------------ fast 1-D decode
// Fixed-rate 1-D decoder for whole-word blocks (maxbits 64 / 32, kmin = 0), the inverse of the lean-4 encoder:
//  * header: bit 0 = 0 -> zero block; else biased emax in bits 1..8;
//  * the empty planes above M0 are single '0' bits, so M0 = 31 - ctz(word >> 9);
//  * group phase: one stream-window lookup per plane in a (n, next 7 bits) -> (nibble, length, n') table that
//    restates libzfp decode_ints' unary run-length decode (decode.c:156-189 with the block-size fix); rows n >= 3
//    are verbatim nibbles, so a wave-uniform loop runs until every lane has n >= 3 and the rest is a contiguous
//    nibble run taken straight from the word;
//  * the nibble window is turned back into four coefficients by the inverse 4 x 16 bit transpose.
// A lane whose group phase runs past the 16-plane window falls back to the generic decoder.
// Entry (n, r, b): decode one plane from state n with the next 7 stream bits b of which only r + 1 are inside the
// block's bit budget (r = 7: at least 8). The budget matters exactly like libzfp's: when it runs out inside the
// unary scan, decode_ints still deposits the coefficient at the current n (x += 1 << n++ after the inner loop).
struct alignas(16) DecTab1 {
  uint16_t v[5 * 8 * 128];
};

__host__ __device__ constexpr uint32_t dec_plane_cx(uint32_t t)
{
  const uint32_t n0 = t >> 10, r = (t >> 7) & 7u, b = t & 127u;
  uint32_t n = n0, bits = r + 1, pos = 0, x = 0;
  if (n >= 4) {  // verbatim nibble (zero past the budget)
    const uint32_t m = bits < 4 ? bits : 4;
    return (b & ((1u << m) - 1u)) | (m << 4) | (4u << 8);
  }
  const uint32_t m = n < bits ? n : bits;  // first n bits verbatim
  x = b & ((1u << m) - 1u);
  pos = m;
  bits -= m;
  while (n < 4 && bits) {
    bits--;
    if (!((b >> pos++) & 1u)) break;  // group test
    while (n < 3 && bits) {
      bits--;
      if ((b >> pos++) & 1u) break;
      n++;
    }
    x += 1u << n;
    n++;
  }
  return x | (pos << 4) | (n << 8);
}

__host__ __device__ constexpr DecTab1 make_dec_tab1()
{
  DecTab1 T{};
  for (uint32_t t = 0; t < 5 * 8 * 128; t++) T.v[t] = (uint16_t)dec_plane_cx(t);
  return T;
}

__device__ const DecTab1 g_dec_tab1 = make_dec_tab1();

// The no-budget rows (r = 7) of the plane table, indexed (n, 7 bits): what the variable-rate decoders use (640 entries,
// 1280 bytes: one 16-byte load for 80 lanes).
struct alignas(16) DecTab7 {
  uint16_t v[5 * 128];
};

__host__ __device__ constexpr DecTab7 make_dec_tab7()
{
  DecTab7 T{};
  for (uint32_t t = 0; t < 5 * 128; t++) T.v[t] = (uint16_t)dec_plane_cx(((((t >> 7) << 3) | 7u) << 7) | (t & 127u));
  return T;
}

__device__ const DecTab7 g_dec_tab7 = make_dec_tab7();

__device__ __forceinline__ uint64_t inv_transpose4x16(uint64_t x)
{
  x = dswap64(x, 0x00000000FF00FF00ull, 24);
  x = dswap64(x, 0x0000F0F00000F0F0ull, 12);
  x = dswap64(x, 0x00000000CCCCCCCCull, 30);
  x = dswap64(x, 0x0000AAAA0000AAAAull, 15);
  return x;
}

// coefficient i's bits for 16 planes starting at plane `top` going down, from a nibble window
__device__ __forceinline__ void window_to_coeffs(uint64_t Y, int top, uint32_t* u)
{
  const uint64_t x = inv_transpose4x16(Y);
  const uint32_t sh = (uint32_t)(31 - top);
#pragma unroll
  for (int i = 0; i < 4; i++) u[i] |= __builtin_bitreverse32((uint32_t)(x >> (16 * i)) & 0xffffu) >> sh;
}

template <uint32_t WB>
__device__ __forceinline__ void decode_block1d_fast(uint64_t w, const uint16_t* dtab, float* f, bool& special)
{
  const bool nonzero = w & 1u;
  const int emax = (int)((w >> 1) & 255u) - 127;
  const uint64_t r = w >> 9;
  const int z = r ? (int)__builtin_ctzll(r) : 64;
  const int M0 = 31 - z;  // < 0: every coded plane empty
  uint32_t pos = 9u + (uint32_t)z;
  uint64_t Y = 0;
  uint32_t n = 0;
  int j = 0;
#pragma unroll
  for (; j < 16; j++) {
    if (!__any(n < 3 && pos < WB && j <= M0)) break;
    const uint32_t b7 = pos < WB ? (uint32_t)(w >> pos) & 127u : 0u;
    const uint32_t rb = min(WB - pos, 8u) - 1u;  // budget bits left in this plane (pos >= WB: b7 = 0, any row)
    const uint32_t e = dtab[(((n << 3) | rb) << 7) | b7];
    Y |= (uint64_t)(e & 15u) << (4 * j);
    pos += (e >> 4) & 15u;
    n = e >> 8;
  }
  special = n < 3 && pos < WB && j <= M0;  // still in the group phase after 16 planes
  if (j < 16 && pos < WB) Y |= (w >> pos) << (4 * j);  // verbatim nibbles (bits past the word are zero)
  uint32_t u[4] = {0, 0, 0, 0};
  if (M0 >= 0) {
    window_to_coeffs(Y, M0, u);
    const uint32_t p2 = pos + 4u * (uint32_t)(16 - j);  // stream position of plane M0 - 16
    if (__any(p2 < WB && M0 >= 16)) {
      const uint64_t Y2 = p2 < WB && M0 >= 16 ? w >> p2 : 0ull;
      if (M0 >= 16) window_to_coeffs(Y2, M0 - 16, u);
    }
  }
  int32_t q[4];
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = (int32_t)((u[i] ^ 0xaaaaaaaau) - 0xaaaaaaaau);
  inv_lift(q[0], q[1], q[2], q[3]);
  const float sc = dequant_scale(emax);
#pragma unroll
  for (int i = 0; i < 4; i++) f[i] = nonzero ? sc * (float)q[i] : 0.0f;  // header bit 0: +0 whatever follows
}

// ---- two planes per lookup (64-bit blocks). The group phase lasts 1.5 planes on average on gradient-like data but
// the wave-uniform loop above runs the wave's maximum (4.6 planes: profiles/r04_dec_pair_table.log), so each step
// here decodes as many of the next two planes as the next 10 stream bits determine, and lanes step on their own.
// Entry (n < 3, 10 bits): nibbles of plane 1 [0, 4) and plane 2 [4, 8), plane 1's length [8, 12), both planes'
// length [12, 16), min(n, 3) after plane 1 [16, 18) and after plane 2 [18, 20), plane 2 decoded [20] (only when its
// code ends inside the 10 bits: decoded with the bits past them zero, a code that stops before them read none).
struct alignas(16) DecTabP {
  uint32_t v[3 * 1024];
};

__host__ __device__ constexpr uint32_t dec_pair_cx(uint32_t t)
{
  const uint32_t n = t >> 10, b = t & 1023u;
  const uint32_t e1 = dec_plane_cx((((n << 3) | 7u) << 7) | (b & 127u));
  const uint32_t x1 = e1 & 15u, l1 = (e1 >> 4) & 15u, n1 = e1 >> 8;
  const uint32_t e2 = dec_plane_cx((((n1 << 3) | 7u) << 7) | ((b >> l1) & 127u));
  const uint32_t x2 = e2 & 15u, l2 = (e2 >> 4) & 15u, n2 = e2 >> 8;
  const uint32_t r1 = n1 < 3 ? n1 : 3u, r2 = n2 < 3 ? n2 : 3u;
  if (l1 + l2 <= 10u) return x1 | (x2 << 4) | (l1 << 8) | ((l1 + l2) << 12) | (r1 << 16) | (r2 << 18) | (1u << 20);
  return x1 | (l1 << 8) | (l1 << 12) | (r1 << 16) | (r1 << 18);
}

__host__ __device__ constexpr DecTabP make_dec_pair()
{
  DecTabP T{};
  for (uint32_t t = 0; t < 3 * 1024; t++) T.v[t] = dec_pair_cx(t);
  return T;
}

__device__ const DecTabP g_dec_pair = make_dec_pair();

// The inverse of the encoder's spread tables (lean1d.h SpreadTab): the nibble window back to coefficient bytes by
// lookups. Window byte k (nibbles 2k, 2k + 1: planes top - 2k, top - 2k - 1) through table s = k mod 4 puts
// coefficient i's two bits at bits 7 - 2s and 6 - 2s of byte i; OR-ing bytes 0..3 gives A (byte i = coefficient i's
// planes top .. top - 7, MSB first), bytes 4..7 give B (planes top - 8 .. top - 15), and one v_perm_b32 per
// coefficient lays A_i, B_i into bits 31..16 ahead of the shift to `top`. 8 LDS reads and ~20 VALU per window where
// window_to_coeffs' four 64-bit delta swaps, bit reversals and shifts take ~52.
struct alignas(16) GatherTab {
  uint32_t v[4 * 256];
};

__host__ __device__ constexpr GatherTab make_gather_tab()
{
  GatherTab T{};
  for (uint32_t s = 0; s < 4; s++)
    for (uint32_t b = 0; b < 256; b++) {
      uint32_t r = 0;
      for (uint32_t i = 0; i < 4; i++) {
        r |= ((b >> i) & 1u) << (8 * i + 7 - 2 * s);
        r |= ((b >> (4 + i)) & 1u) << (8 * i + 6 - 2 * s);
      }
      T.v[256 * s + b] = r;
    }
  return T;
}

// the pair table and the gather tables as one LDS image (the fixed-rate pair decoders stage both in one pass)
struct alignas(16) DecTabPG {
  uint32_t v[3 * 1024 + 4 * 256];
};

__host__ __device__ constexpr DecTabPG make_dec_pair_gather()
{
  DecTabPG T{};
  const DecTabP P = make_dec_pair();
  const GatherTab G = make_gather_tab();
  for (uint32_t t = 0; t < 3 * 1024; t++) T.v[t] = P.v[t];
  for (uint32_t t = 0; t < 4 * 256; t++) T.v[3 * 1024 + t] = G.v[t];
  return T;
}

__device__ const DecTabPG g_dec_pair_gather = make_dec_pair_gather();

// The variable-rate lean decoder's LDS image: the pair table as 16-bit entries (n < 3, next 10 bits) -> nibbles
// [0, 8), bits taken [8, 12), min(n, 3) after [12, 14), two planes taken [14] (dec_pair_cx's fields), then the plane
// table's 640 entries (DecTab7) for a step that may take one plane only (the block's last coded plane, or the last
// of the 8-plane group window) and for the general decoder. 7424 bytes.
struct alignas(16) DecTabLP {
  uint16_t v[3 * 1024 + 5 * 128];
};

__host__ __device__ constexpr DecTabLP make_dec_lean_pair()
{
  DecTabLP T{};
  for (uint32_t t = 0; t < 3 * 1024; t++) {
    const uint32_t e = dec_pair_cx(t);
    T.v[t] = (uint16_t)((e & 255u) | (((e >> 12) & 15u) << 8) | (((e >> 18) & 3u) << 12) | (((e >> 20) & 1u) << 14));
  }
  const DecTab7 S = make_dec_tab7();
  for (uint32_t t = 0; t < 5 * 128; t++) T.v[3 * 1024 + t] = S.v[t];
  return T;
}

__device__ const DecTabLP g_dec_lean_pair = make_dec_lean_pair();


__device__ __forceinline__ void window_to_coeffs_lds(const uint32_t* gt, uint64_t Y, int top, uint32_t* u)
{
  const uint32_t lo = (uint32_t)Y, hi = (uint32_t)(Y >> 32);
  const uint32_t A = gt[lo & 255u] | gt[256 + ((lo >> 8) & 255u)] | gt[512 + ((lo >> 16) & 255u)] | gt[768 + (lo >> 24)];
  const uint32_t B = gt[hi & 255u] | gt[256 + ((hi >> 8) & 255u)] | gt[512 + ((hi >> 16) & 255u)] | gt[768 + (hi >> 24)];
  const uint32_t sh = (uint32_t)(31 - top);
#pragma unroll
  for (uint32_t i = 0; i < 4; i++) u[i] |= __builtin_amdgcn_perm(A, B, ((4u + i) << 24) | (i << 16) | 0x0c0cu) >> sh;
}

// decode_block1d_fast<64> with the pair table: a lane leaves the loop when its group phase ends (n >= 3), its planes
// run out (j > M0) or the 16-plane window is full; a plane that would cross the 64-bit budget goes to the generic
// decoder (special), as does a group phase longer than the window.
template <bool GATHER>
__device__ __forceinline__ void decode_block1d_pair(uint64_t w, const uint32_t* dtp, float* f, bool& special)
{
  const bool nonzero = w & 1u;
  const int emax = (int)((w >> 1) & 255u) - 127;
  // header bit 0: +0 whatever follows -- taken as a block whose planes are all empty (u = 0, so every value is
  // sc * 0 = +0 with sc >= 0), not selected per value at the end
  const uint64_t r = nonzero ? w >> 9 : 0ull;
  const int z = r ? (int)__builtin_ctzll(r) : 64;
  const int M0 = 31 - z;  // < 0: every coded plane empty
  uint32_t pos = 9u + (uint32_t)z;
  uint64_t Y = 0;
  uint32_t n = 0;
  int j = 0;
  // Select-free steps (measured against budget- and window-guarded steps in profiles/r05_dec_pair2_ab.log). Every
  // step takes the entry's two-plane fields (which fall back to the first plane's when the second is not decoded within the 10 bits), with no per-step budget or window selects; what they would have guarded only makes
  // the block special: a plane code crossing the 64-bit budget leaves pos > 64, and a step from nibble 15 (j ends at
  // 17) consumed plane M0 - 16, which belongs to the second window. A second plane below plane 0 (a step from j = M0)
  // lands past the coefficients' low bit and is shifted out by window_to_coeffs; its length only matters for pos > 64.
  const int jm = min(M0, 15);
#pragma unroll
  for (int it = 0; it < 16; it++) {
    // the first step is every lane with a coded plane (n = 0, j = 0, pos <= 40): no wave vote
    const bool act = it == 0 ? M0 >= 0 : n < 3 && pos < 64u && j <= jm;
    if (it > 0 && !__any(act)) break;
    if (act) {
      const uint32_t e = dtp[(n << 10) | ((uint32_t)(w >> pos) & 1023u)];
      Y |= (uint64_t)(e & 255u) << (4 * j);
      pos += (e >> 12) & 15u;
      n = (e >> 18) & 3u;
      j += 1 + (int)((e >> 20) & 1u);
    }
  }
  // special: a plane code crossed the budget, or the steps reached nibble 16 (a group phase as long as the window, or
  // a step from nibble 15 that consumed plane M0 - 16; a group phase that ended exactly at nibble 16 is decoded
  // generically too, which only costs time). Otherwise every coded plane is in Y: the loop stopped with n >= 3, with
  // the budget used up (pos = 64), or past plane 0.
  special = M0 >= 0 && (pos > 64u || j >= 16);
  // verbatim nibbles (bits past the word are zero): pos >= 9, so the two-step shift gives 0 at pos = 64; lanes with
  // pos > 64 or j >= 16 are special and their Y is not used
  Y |= ((w >> (pos - 1u)) >> 1) << (4 * j);
  uint32_t u[4] = {0, 0, 0, 0};
  if (M0 >= 0) {
    if constexpr (GATHER) window_to_coeffs_lds(dtp + 3 * 1024, Y, M0, u);
    else window_to_coeffs(Y, M0, u);
    const uint32_t p2 = pos + 4u * (uint32_t)(16 - min(j, 16));  // stream position of plane M0 - 16
    if (__any(p2 < 64u && M0 >= 16)) {
      const uint64_t Y2 = p2 < 64u && M0 >= 16 ? w >> p2 : 0ull;
      if (M0 >= 16) {
        if constexpr (GATHER) window_to_coeffs_lds(dtp + 3 * 1024, Y2, M0 - 16, u);
        else window_to_coeffs(Y2, M0 - 16, u);
      }
    }
  }
  int32_t q[4];
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = (int32_t)((u[i] ^ 0xaaaaaaaau) - 0xaaaaaaaau);
  inv_lift(q[0], q[1], q[2], q[3]);
  // (float)q * 2^(emax - 30) as one v_ldexp_f32 per value: the product by the exact power of two that dequant_scale
  // gives, rounded once alike (denormal results included); below 2^-149 dequant_scale's 0 gives a signed zero, which
  // the ldexp gives at any exponent under -181 (|q| < 2^31)
  const int e = emax - 30 < -149 ? -256 : emax - 30;
#pragma unroll
  for (int i = 0; i < 4; i++) f[i] = __builtin_amdgcn_ldexpf((float)q[i], e);  // header bit 0: q = 0 above
}

// ------------------------------------------------------------------------------------------------ 1-D variable-rate
// decode. Variable-rate 1-D streams whose budget never truncates a block (minbits <= 1, maxbits >= 160: accuracy,
// precision, expert) decode block by block with the fixed-rate decoder's plane table instead of bit by bit: header,
// then the empty planes (one '0' each: a count-trailing-zeros), the group phase (one (n, 7 stream bits) lookup per
// plane while n < 3, down to kmin), then the remaining planes as a verbatim nibble run (a plane with n >= 3 is its
// nibble) and the inverse bit transpose; libzfp decode_ints semantics (decode.c:141-183 with the block-size fix).
// One lane per block-index chunk, blocks in sequence (each block's start is the previous block's end).
__device__ __forceinline__ uint64_t stream_window(const uint64_t* in, uint64_t pos)
{
  const uint64_t i = pos >> 6;
  const uint32_t sh = (uint32_t)(pos & 63);
  const uint64_t lo = in[i] >> sh;
  return sh ? lo | (in[i + 1] << (64 - sh)) : lo;
}

// 64 stream bits at a bit position, from global memory or from words staged in LDS (positions relative to them)
struct GlobalWindow {
  const uint64_t* in;
  __device__ __forceinline__ uint64_t operator()(uint64_t pos) const { return stream_window(in, pos); }
};
struct LdsWindow {
  const uint64_t* w;
  __device__ __forceinline__ uint64_t operator()(uint64_t pos) const
  {
    const uint32_t i = (uint32_t)(pos >> 6), sh = (uint32_t)(pos & 63);
    const uint64_t lo = w[i] >> sh;
    return sh ? lo | (w[i + 1] << (64 - sh)) : lo;
  }
};

// dtab: the full (n, r, 7 bits) plane table, or (COMPACT) its r = 7 rows only, indexed (n, 7 bits)
template <class Win, bool COMPACT = true>
__device__ __forceinline__ void decode_block1d_var(const Win& win, uint64_t& pos, const uint16_t* dtab, int minexp,
                                                   uint32_t maxprec, float* f)
{
  uint64_t w = win(pos);
  if (!(w & 1u)) {  // zero block (or prec = 0): one 0 bit
    f[0] = f[1] = f[2] = f[3] = 0.0f;
    pos += 1;
    return;
  }
  const int emax = (int)((w >> 1) & 255u) - 127;
  const int prec = min((int)maxprec, max(0, emax - minexp + 4));
  const int kmin = prec < 32 ? 32 - prec : 0;
  const int np = 32 - kmin;  // coded planes 31 .. kmin
  pos += 9;
  w = win(pos);
  const int z = w ? (int)__builtin_ctzll(w) : 64;
  uint32_t u[4] = {0u, 0u, 0u, 0u};
  if (z >= np) {
    pos += (uint32_t)np;  // every coded plane empty
  } else {
    pos += (uint32_t)z;
    const int M0 = 31 - z;
    const int nbelow = M0 - kmin + 1;  // planes M0 .. kmin
    uint64_t Ylo = 0, Yhi = 0;         // plane nibbles M0 - j, j = 0..31
    uint32_t n = 0, used = 0;
    int j = 0;
    w = win(pos);
    while (n < 3 && j < nbelow) {
      if (used > 56) {
        pos += used;
        used = 0;
        w = win(pos);
      }
      const uint32_t e = dtab[(COMPACT ? (n << 7) : ((((n << 3) | 7u)) << 7)) | ((uint32_t)(w >> used) & 127u)];
      const uint64_t nib = e & 15u;
      if (j < 16) Ylo |= nib << (4 * j);
      else Yhi |= nib << (4 * (j - 16));
      used += (e >> 4) & 15u;
      n = e >> 8;
      j++;
    }
    pos += used;
    const int t = nbelow - j;  // planes left: 4 bits each, verbatim
    if (t > 0) {
      const uint32_t nb = 4u * (uint32_t)t;  // <= 128
      uint64_t v0 = win(pos), v1 = nb > 64 ? win(pos + 64) : 0ull;
      if (nb < 64) v0 &= (1ull << nb) - 1ull;
      else if (nb < 128) v1 &= (1ull << (nb - 64)) - 1ull;
      const uint32_t sft = 4u * (uint32_t)j;  // nibble position of the run; sft + nb <= 128
      if (sft == 0) {
        Ylo |= v0;
        Yhi |= v1;
      } else if (sft < 64) {
        Ylo |= v0 << sft;
        Yhi |= (v0 >> (64 - sft)) | (v1 << sft);
      } else {
        Yhi |= v0 << (sft - 64);
      }
      pos += nb;
    }
    window_to_coeffs(Ylo, M0, u);
    if (M0 >= 16) window_to_coeffs(Yhi, M0 - 16, u);
  }
  int32_t q[4];
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = (int32_t)((u[i] ^ 0xaaaaaaaau) - 0xaaaaaaaau);
  inv_lift(q[0], q[1], q[2], q[3]);
  const float sc = dequant_scale(emax);
#pragma unroll
  for (int i = 0; i < 4; i++) f[i] = sc * (float)q[i];
}

// ------------------------------------------------------------------------------------------------ lean 1-D var decode
// The variable-rate block decoder of the staged kernels, cut to what a block needs (libzfp decode_ints semantics,
// decode.c:141-183 with the block-size fix; minbits <= 1, maxbits >= 160, so no budget truncates):
//  * one 64-bit window at the block start gives the header, the precision and the run of empty planes (ctz over the
//    55 bits after the header covers any np <= 32) and, in the common case, the group phase's bits too (the window
//    is re-read only when a group plane's 7 lookup bits would run past it);
//  * the group phase (planes while fewer than 3 coefficients are significant) is at most 8 planes here, its nibbles
//    packed into one 32-bit word; a block whose group phase is longer takes the general decoder (rare: three
//    coefficients spread over more than 8 planes);
//  * the verbatim nibble run (4 bits per remaining plane) is one window, two past 64 bits;
//  * the inverse 4 x 16 bit transposes run for the planes present: the second half only when more than 16 planes
//    are coded (accuracy 1e-6 on gradient-scale data codes ~14).
// Positions are 32-bit, relative to the staged words (LDS), and windows are built from three 32-bit words with two
// v_alignbit_b32. (An XOR-swizzled stage with qword reads cut the LDS bank conflicts from 9.6 to 2.6 per instruction
// and was worth at most 1.8 %: profiles/r06_lds_swizzle_ab.log. The spans are staged linearly.)
__device__ __forceinline__ uint64_t lds_win64(const uint32_t* w, uint32_t pos)
{
  const uint32_t i = pos >> 5;
  const uint32_t a = w[i], b = w[i + 1], c = w[i + 2];
  return ((uint64_t)__builtin_amdgcn_alignbit(c, b, pos) << 32) | __builtin_amdgcn_alignbit(b, a, pos);
}

// returns false when the block needs the general decoder (pos unchanged then). PAIR: tab is the DecTabLP image and
// the group phase decodes up to two planes per lookup; else tab is DecTab7.
template <bool PAIR = false>
__device__ __forceinline__ bool dec_block1d_lean(const uint32_t* sw, uint32_t& pos, const uint16_t* tab, int cexp,
                                                 int maxprec, float* f)
{
  const uint64_t w = lds_win64(sw, pos);
  const int emax = (int)((w >> 1) & 255u) - 127;
  const int np = min(32, min(maxprec, max(0, emax + cexp)));  // coded planes 31 .. 32 - np
  // empty planes: ctz of the 55 bits after the header, a sentinel one at bit 55 for none (any np <= 32 < 55)
  const int z = (int)__builtin_ctzll((w >> 9) | (1ull << 55));
  f[0] = f[1] = f[2] = f[3] = 0.0f;
  if (!(w & 1u)) {  // zero block (or no precision): one 0 bit
    pos += 1;
    return true;
  }
  if (z >= np) {  // every coded plane empty: the values are +0
    pos += 9u + (uint32_t)np;
    return true;
  }
  const int M0 = 31 - z, nbelow = np - z;  // planes M0 .. M0 - nbelow + 1
  // group phase: one (n, 7 bits) lookup per plane while n < 3
  uint64_t gw = w;
  uint32_t off = 9u + (uint32_t)z, wbase = pos;
  uint32_t n = 0, G = 0;
  int j = 0;
  if constexpr (PAIR) {
    // (n, 10 bits) -> one or two planes; a second plane past the block's coded planes or past the 8-plane window is
    // not taken: that step re-reads the plane table for the first plane alone
    const uint16_t* dt7 = tab + 3 * 1024;
    const int lim = min(nbelow, 8);
    while (n < 3 && j < lim) {
      if (off > 54u) {
        wbase += off;
        gw = lds_win64(sw, wbase);
        off = 0;
      }
      const uint32_t b = (uint32_t)(gw >> off) & 1023u;
      const uint32_t e = tab[(n << 10) | b];
      uint32_t nib = e & 255u, len = (e >> 8) & 15u, nn = (e >> 12) & 3u, two = e >> 14;
      if (two && j + 1 >= lim) {
        const uint32_t e7 = dt7[(n << 7) | (b & 127u)];
        nib = e7 & 15u;
        len = (e7 >> 4) & 15u;
        nn = e7 >> 8;
        two = 0;
      }
      G |= nib << (4 * j);
      off += len;
      n = nn;
      j += 1 + (int)two;
    }
  } else {
    const uint16_t* dt7 = tab;
    while (n < 3 && j < nbelow && j < 8) {
      if (off > 57u) {
        wbase += off;
        gw = lds_win64(sw, wbase);
        off = 0;
      }
      const uint32_t e = dt7[(n << 7) | ((uint32_t)(gw >> off) & 127u)];
      G |= (e & 15u) << (4 * j);
      off += (e >> 4) & 15u;
      n = e >> 8;
      j++;
    }
  }
  if (n < 3 && j < nbelow) return false;  // group phase longer than 8 planes
  const uint32_t vpos = wbase + off;
  const uint32_t t = (uint32_t)(nbelow - j);  // verbatim planes, 4 bits each
  const uint32_t nb = 4u * t;                 // <= 128
  // the run's window is not masked at nb: the next block's bits beyond it land on planes below kmin = 32 - np, which
  // one mask of the coefficients clears
  uint64_t v0 = lds_win64(sw, vpos), v1 = 0;
  if (nb > 64) v1 = lds_win64(sw, vpos + 64);
  const uint32_t sft = 4u * (uint32_t)j;  // <= 32
  const uint64_t Ylo = (uint64_t)G | (v0 << sft);
  uint32_t u[4] = {0u, 0u, 0u, 0u};
  window_to_coeffs(Ylo, M0, u);
  if (nbelow > 16) {
    const uint64_t Yhi = ((v0 >> 1) >> (63u - sft)) | (v1 << sft);
    window_to_coeffs(Yhi, M0 - 16, u);
  }
  const uint32_t keep = ~0u << (uint32_t)(32 - np);  // planes 31 .. kmin (np >= 1 here)
#pragma unroll
  for (int i = 0; i < 4; i++) u[i] &= keep;
  pos = vpos + nb;
  int32_t q[4];
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = (int32_t)((u[i] ^ 0xaaaaaaaau) - 0xaaaaaaaau);
  inv_lift(q[0], q[1], q[2], q[3]);
  const int e = emax - 30 < -149 ? -256 : emax - 30;  // as decode_block1d_pair: ldexp = dequant_scale(emax) * q
#pragma unroll
  for (int i = 0; i < 4; i++) f[i] = __builtin_amdgcn_ldexpf((float)q[i], e);
  return true;
}

// One stage of the 8 x 8 transpose of float4 elements across the 8-lane groups of a wave (butterfly over lane bit D:
// lanes exchange with lane ^ D the elements whose index differs from theirs in bit D). DPP moves, no LDS.
template <int D>
__device__ __forceinline__ void xpose8_stage(float (&g)[8][4], uint32_t lane)
{
  const bool hi = (lane & D) != 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    if (!(k & D)) continue;
    const int a = k ^ D, b = k;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int send = __float_as_int(hi ? g[a][c] : g[b][c]);
      int recv;
      if constexpr (D == 1) {
        recv = __builtin_amdgcn_mov_dpp(send, 0xB1, 0xf, 0xf, false);  // quad_perm [1, 0, 3, 2]
      } else if constexpr (D == 2) {
        recv = __builtin_amdgcn_mov_dpp(send, 0x4E, 0xf, 0xf, false);  // quad_perm [2, 3, 0, 1]
      } else {
        const int up = __builtin_amdgcn_mov_dpp(send, 0x104, 0xf, 0xf, false);  // row_shl:4 (lane + 4)
        const int dn = __builtin_amdgcn_mov_dpp(send, 0x114, 0xf, 0xf, false);  // row_shr:4 (lane - 4)
        recv = hi ? dn : up;
      }
      if (hi) g[a][c] = __int_as_float(recv);
      else g[b][c] = __int_as_float(recv);
    }
  }
}

}  // namespace gcow
