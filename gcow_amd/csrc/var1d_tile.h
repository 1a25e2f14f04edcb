// var1d_tile.h -- the parts of the 1-D variable-rate tile form that do not depend on where a block's values and
// parameter set come from: the tunables and window sizes, the pair table, a block's code (v1_code), the window store
// (v1_tile_store), the coders' LDS (v1_lds) and the workspace layout (V1Workspace). Shared by the encoder over one
// field (var1d.hip) and the segmented encoder (seg1d.hip); the text is var1d.hip's, moved here unchanged.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec_device.h"
#include "kernels.h"
#include "lean1d.h"

// ---- tunables (A/B builds: tools/build_variant.sh, tools/ubench/var1d_ablate.sh)
#ifndef GCOW_V1T
#define GCOW_V1T 256  // lanes per workgroup (512 measured neutral: profiles/r06_c5_t512_negative.log)
#endif
// V1_ABLATE (measurement builds only, tools/ubench/var1d_ablate.sh; 0 in the product): 1 = no look-back (tile t at
// t * 64 Ki bits), 2 = no coding (zero codes / prepared words, lengths kept), 4 = no window store, 8 = no pair loop,
// 16 = no prepare in the tile coder (raw words as coefficients), 32 = no length computation in the tile count,
// 64 = no input / length loads in the tile coder (synthetic words, 58-bit blocks), 128 = no LDS window writes in the
// tile coder (the accumulator words folded into one register), 256 = no spread-table window lookups in the coder
#ifndef V1_ABLATE
#define V1_ABLATE 0
#endif

namespace gcow {

constexpr uint32_t V1T = GCOW_V1T;                           // lanes per workgroup
constexpr uint32_t V1U = 4;                                  // consecutive blocks per lane
constexpr uint32_t V1TILE = V1T * V1U;                       // blocks per tile
constexpr uint32_t V1MAXB = 140;                             // 9 + 3 + 4 * 32: the longest 1-D block
constexpr uint32_t V1Q = (V1TILE * V1MAXB + 63) / 64 + 2;    // LDS window, 64-bit words
constexpr uint32_t V1CT = 8;                                     // tiles per count workgroup
constexpr uint32_t V1QS = 1500 * (V1T / 256);                     // small window, qwords (95 bits per block)
constexpr uint32_t V1TAB = 1024;                                  // pair-table rows 0..3 in LDS

// The lean-5 pair table with its rows n = 3 and 4 emptied (no bits, the row kept): from n = 3 on every plane is its
// nibble verbatim (encode.c:301-333 with one coefficient left), which the variable-rate coder takes from the window
// instead, so a lane whose group phase is over adds nothing more -- no per-lane selects in the pair loop.
// Row n' = 4 is folded into row 3 (both are empty), so the tile kernels keep only rows 0..3 (4 KB) in LDS.
__host__ __device__ constexpr PlaneTab2 make_plane_tab_var()
{
  PlaneTab2 T = make_plane_tab5();
  for (uint32_t t = 0; t < 3 * 256; t++)
    if ((T.v[t] & 0x1c00u) == (4u << 10)) T.v[t] = (T.v[t] & ~0x1c00u) | (3u << 10);
  for (uint32_t t = 3 * 256; t < 1280; t++) T.v[t] = 3u << 10;
  return T;
}
__device__ const PlaneTab2 g_plane_tab_var = make_plane_tab_var();

// A block's code (sw/src/encode.c:457-495 + :279-339) OR-ed into the lane's bit accumulator at bit `fill`, its full
// 64-bit words stored to the window: c = the first 128 bits of the code of every plane -- the code of planes 31 ..
// kmin is a prefix of it, so the coder ignores kmin and the length cuts it. Same evaluation as the fixed-rate lean-6
// coder (enc_fixed1d.hip): header | one '0' per empty plane above M0 | group phase through the pair table, two
// planes per wave-uniform step, until no lane of the wave has a coded group plane left | the rest of the 32-plane
// window verbatim from the lane's nibble jl. special: the block needs the generic coder (a group phase past the
// 16-plane window, a group code of 64 bits or more, a code past 128 bits); its bits are left zero here.
__device__ __forceinline__ void v1_code(const uint32_t* u, uint32_t hdr, uint32_t len, uint32_t K, const uint32_t* tab,
                                        const uint32_t* rs, uint64_t& c0, uint64_t& c1, bool& special)
{
  const uint32_t S2 = u[2] | u[3];
  const uint32_t sh = ffbh_hw(u[0] | u[1] | S2 | 1u);  // 31 - M0
  const int M0 = 31 - (int)sh;
  // group phase: window nibbles 0 .. jg, of which planes >= kmin are coded (nibbles <= K - sh)
  const int jg = (int)min(ffbh_hw(S2), K) - (int)sh;
  const uint32_t w0 = u[0] << sh, w1 = u[1] << sh, w2 = u[2] << sh, w3 = u[3] << sh;
  const uint64_t Y = (V1_ABLATE & 256) ? (((uint64_t)(w0 ^ w1) << 32) | (w2 ^ w3))
                                        : window_lds(rs, w0, w1, w2, w3);  // planes M0 .. M0 - 15 as nibbles
  const uint32_t pos0 = 9u + sh;                      // header + one '0' per empty plane
  uint32_t e = tab[(uint32_t)Y & 255u];
  uint64_t G = e >> 17;
  uint32_t gl = (e >> 13) & 15u;
#pragma unroll
  for (int jj = 2; jj < ((V1_ABLATE & 8) ? 2 : 16); jj += 2) {
    if (!__any(jj <= jg)) break;
    e = tab5_next(tab, e, (uint32_t)(Y >> (4 * jj)) & 255u);  // rows n >= 3 add nothing
    G |= (uint64_t)(e >> 17) << (gl & 63u);
    gl += (e >> 13) & 15u;
  }
  const uint32_t jl = (uint32_t)min(max((jg & ~1) + 2, 2), 16);  // first nibble after the lane's last group pair
  special = special || gl > 63u || len > 128u || (jg >= 16 && pos0 + gl < len);
  // V = the 32-plane window from nibble jl on (planes M0 - 16 .. M0 - 31 only where a lane's code reaches them);
  // R = group code | V after it; c = header | R after the empty planes
  const uint32_t vs = 4u * jl - 8u;  // 0 .. 56: V = W >> (vs + 8)
  uint64_t V0 = (Y >> 8) >> vs, V1 = 0;
  if (__any(M0 >= 16 && pos0 + gl + 56u - vs < len)) {  // plane M0 - 16 lands at pos0 + gl + 4 (16 - jl)
    const uint64_t Y2 = (V1_ABLATE & 256) ? (((uint64_t)(w0 + w1) << 32) | (w2 + w3))
                                          : window_lds_low(rs, w0, w1, w2, w3);
    V0 |= Y2 << (56u - vs);
    V1 = (Y2 >> 8) >> vs;
  }
  const uint32_t g = gl & 63u;  // >= 2
  const uint64_t R0 = G | (V0 << g), R1 = (V0 >> (64u - g)) | (V1 << g);
  c0 = (uint64_t)hdr | (R0 << pos0);  // pos0: 9 .. 40
  c1 = (R0 >> (64u - pos0)) | (R1 << pos0);
}

// The window's 16-byte chunks c (stream words 4c .. 4c + 3 from word g0 = (B >> 7) * 4): the tile owns words kf .. kl;
// the first / last chunk holds words of the neighbouring tiles and the two words it shares with them (atomicOr), so
// those two chunks go word by word.
__device__ __forceinline__ void v1_edge_chunk(uint32_t c, const uint32_t* win32, uint32_t* __restrict__ out32,
                                              uint64_t g0, uint32_t kf, uint32_t kl, bool head_shared,
                                              bool tail_shared)
{
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) {
    const uint32_t k = 4u * c + j;
    if (k < kf || k > kl) continue;
    const uint32_t val = win32[k];
    if ((k == kf && head_shared) || (k == kl && tail_shared)) atomicOr(out32 + g0 + k, val);
    else out32[g0 + k] = val;
  }
}

// Store the coded window of tile t (total bits from B): every interior chunk is one ds_read_b128 + one 16-byte store.
__device__ __forceinline__ void v1_tile_store(uint32_t t, uint64_t B, uint32_t total, const uint64_t* win,
                                              uint32_t* __restrict__ out32, uint32_t ntiles)
{
  const uint32_t* win32 = (const uint32_t*)win;
  const uint32_t tid = threadIdx.x;
  const uint32_t lb = (uint32_t)(B & 127u);
  // ---- store the window: 16-byte chunks of stream words from word g0 = (B >> 7) * 4, coalesced. The tile owns
  // words kf .. kl; the first / last chunk holds words of the neighbouring tiles and the two words it shares with
  // them (atomicOr), so those two chunks go word by word, every other chunk is one ds_read_b128 + one 16-byte store.
  const uint64_t g0 = (B >> 7) << 2;
  const uint32_t kf = lb >> 5, kl = (lb + total - 1u) >> 5;
  const bool head_shared = (lb & 31u) != 0;
  const bool last_tile = t == ntiles - 1;
  const bool tail_shared = ((lb + total) & 31u) != 0 && !last_tile;
  const uint32_t nch = (V1_ABLATE & 4) ? 0u : (kl >> 2) + 1u;
  const bool wide = (((uintptr_t)out32) & 15u) == 0;
  for (uint32_t c = tid; c < nch; c += V1T) {
    if (wide && c != 0 && c != nch - 1) *(uint4*)(out32 + g0 + 4u * c) = *(const uint4*)(win32 + 4u * c);
    else v1_edge_chunk(c, win32, out32, g0, kf, kl, head_shared, tail_shared);
  }
  if (last_tile && tid == 0) {
    const uint64_t endw = (B + total + 31) >> 5;
    if (endw & 1) out32[endw] = 0u;  // stream_flush: zero-pad to a 64-bit boundary (stream.c:132-138)
  }
}

// qwords of window a tile needs: its bits from bit B & 127 of the window (the 16-byte stream boundary below B), plus
// the two qwords the accumulator may touch past its last bit (a special block's zero third word)
__device__ __forceinline__ uint32_t v1_tile_qwords(uint64_t B, uint32_t total)
{
  return ((uint32_t)(B & 127u) + total + 63u) / 64u + 2u;
}

// The coders' LDS with a window of Q qwords, the pair table (rows 0..3, lean-5 entries, row 3 empty) and the window
// spread tables staged.
struct V1Lds {
  uint32_t *tab, *rs;
  uint64_t* win;  // the tile's code from bit base & 127 of its window
  uint32_t *scan_sh, *s_special;
};
template <uint32_t Q>
__device__ __forceinline__ V1Lds v1_lds()
{
  __shared__ __attribute__((aligned(16))) uint32_t tab[V1TAB];
  __shared__ uint32_t rs[1024];
  __shared__ __attribute__((aligned(16))) uint64_t win[Q];
  __shared__ uint32_t scan_sh[V1T / 64];
  __shared__ uint32_t s_special;
  stage_table<V1T, V1TAB>(tab, g_plane_tab_var.v);
#pragma unroll
  for (uint32_t i = 0; i < 1024 / V1T; i++) rs[threadIdx.x + V1T * i] = rspread_entry(threadIdx.x + V1T * i);
  return V1Lds{tab, rs, win, scan_sh, &s_special};
}

// The workspace: sums[ntiles], base[ntiles + 1] (uint64), the oversized-tile list (count + ntiles uint32, rounded to 8
// bytes), the byte lengths of whole tiles, then the totals of groups of V1CT tiles.
struct V1Workspace {
  uint32_t ntiles;
  size_t o_base, o_over, o_lens8, o_gsums, words;  // in uint64 words
  explicit V1Workspace(uint64_t nblocks) : ntiles((uint32_t)((nblocks + V1TILE - 1) / V1TILE))
  {
    static_assert(V1T % 2 == 0, "a tile's byte lengths are whole uint64 words");
    o_base = ntiles;
    o_over = o_base + ntiles + 2;
    o_lens8 = o_over + (ntiles + 2) / 2;
    o_gsums = o_lens8 + (size_t)ntiles * (V1T / 2);
    words = o_gsums + (ntiles + V1CT - 1) / V1CT;
  }
};

}  // namespace gcow
