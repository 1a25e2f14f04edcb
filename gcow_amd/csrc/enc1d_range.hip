// enc1d_range.hip -- the range form of the variable-rate 1-D encoder (form 1 of Var1dVariant; forms 0 and 2 are in
// var1d.hip) and launch_encode_tiles, which dispatches the 1-D forms and the generic tile kernels (tiles.h):
//   k_count1d_var   pass 1: per-range sums of block bit lengths (closed form)
//   k_scan_ranges   (scan_stitch.hip, through launch_scan_ranges) range offsets, zeroes the words two ranges share
//   k_encode1d_var  pass 2: the closed-form coder over tiles of 256 U blocks, codes assembled in an LDS window
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "codec_device.h"
#include "kernels.h"
#include "lean1d.h"
#include "tiles.h"

namespace gcow {

// ------------------------------------------------------------------------------------------------ 1-D variable rate
// Closed-form coder for variable-rate 1-D blocks (accuracy / precision / expert modes whose budget never truncates a
// block: minbits <= 1, maxbits >= 160). Same structure as lean-6 (enc_fixed1d.hip), with the plane range ending at kmin = 32 - prec:
//   header (9) | empty planes 31 .. max(M0, kmin - 1) + 1 ('0' each) | group phase M0 .. max(T2, kmin), two planes
//   per wave-uniform step through the pair table (lanes past their own group phase emit verbatim nibbles, lanes
//   past kmin emit nothing) | verbatim nibbles down to kmin from the 32-plane window.
// Returns the block's bit length; with CODE the bits in c[0..2] (a block is at most 140 bits). special: Inf/NaN, or a
// group phase longer than 16 planes or 64 bits -> generic coder.
template <bool CODE>
__device__ __forceinline__ uint32_t encode_block1d_var(const float* f, const uint16_t* tab, const uint32_t* tab2,
                                                      const uint32_t* rs, int minexp, uint32_t maxprec, uint64_t* c,
                                                      bool& special)
{
  const uint32_t a0 = __float_as_uint(f[0]) & 0x7fffffffu, a1 = __float_as_uint(f[1]) & 0x7fffffffu;
  const uint32_t a2 = __float_as_uint(f[2]) & 0x7fffffffu, a3 = __float_as_uint(f[3]) & 0x7fffffffu;
  const uint32_t m = max(max(a0, a1), max(a2, a3));
  special = m >= 0x7f800000u;
  const uint32_t E = special ? 150u : (m >> 23);
  const int emax = E ? (int)E - 126 : -126;  // frexp exponent of max|x|; subnormal maxima clamp to -126
  const int prec = min((int)maxprec, max(0, emax - minexp + 4));
  if (CODE) c[0] = c[1] = c[2] = 0ull;
  if (m == 0 || prec == 0) return 1u;  // one 0 bit
  const int kmin = prec < 32 ? 32 - prec : 0;
  const bool tiny = E < 29u;
  const float s = __uint_as_float((283u - (tiny ? 150u : E)) << 23);
  int32_t q[4];
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = tiny ? (int32_t)0x80000000 : (int32_t)(f[i] * s);
  fwd_lift(q[0], q[1], q[2], q[3]);
  uint32_t u[4];
#pragma unroll
  for (int i = 0; i < 4; i++) u[i] = ((uint32_t)q[i] + 0xaaaaaaaau) ^ 0xaaaaaaaau;
  const uint32_t o23 = u[2] | u[3];
  const int M0 = 31 - (int)__builtin_clz(u[0] | u[1] | o23 | 1u);
  const int T2 = o23 ? 31 - (int)__builtin_clz(o23) : 0;
  const uint32_t pos0 = 9u + (uint32_t)(31 - max(M0, kmin - 1));  // header + empty planes
  const int nplanes = max(M0 - kmin + 1, 0);                        // planes M0 .. kmin
  const int jg = M0 - max(T2, kmin);                                 // last group-phase plane (window index)
  const uint32_t sh = (uint32_t)(31 - M0);  // M0 >= 0: the |1 in the clz
  const uint64_t Y = window_lds(rs, u[0] << sh, u[1] << sh, u[2] << sh, u[3] << sh);
  uint64_t g = 0;  // group-phase bits, relative to pos0
  uint32_t glen = 0, n = 0;
  int j = 0;
  // two planes per step through the lean-5 pair table (tab2: n' << 10 | len << 13 | code << 17); a pair whose second
  // plane is below kmin takes its first plane's code from the single-plane table (tab)
#pragma unroll
  for (; j < 16; j += 2) {
    if (!__any(j <= jg)) break;
    const uint32_t byte = (uint32_t)(Y >> (4 * j)) & 255u;
    const uint32_t e = tab2[(n << 8) | byte];
    const bool act2 = j + 1 < nplanes, act1 = j < nplanes;
    uint32_t code = act2 ? e >> 17 : 0u, len = act2 ? (e >> 13) & 15u : 0u;
    if (__any(act1 && !act2)) {
      const uint32_t e1 = tab[(n << 4) | (byte & 15u)];
      if (act1 && !act2) {
        code = e1 & 127u;
        len = (e1 >> 7) & 7u;
      }
    }
    if (CODE) g |= (uint64_t)(glen < 64 ? code : 0u) << glen;
    glen += len;
    n = act2 ? (e >> 10) & 7u : n;
  }
  j = min(j, 16);
  special = special || jg >= 16 || glen > 64;
  const int tplanes = max(nplanes - j, 0);  // verbatim planes after the group phase
  const uint32_t len = pos0 + glen + 4u * (uint32_t)tplanes;
  if (CODE) {
    const uint64_t hdr = 2ull * E + 3ull;
    c[0] = hdr | (pos0 < 64 ? g << pos0 : 0ull);
    c[1] = pos0 ? g >> (64 - pos0) : 0ull;  // pos0 >= 9
    if (tplanes > 0) {
      // tail nibbles j .. nplanes-1 of the 32-plane window (Y, then planes M0-16 .. M0-31)
      const uint32_t s2 = sh + 16u;  // <= 31 where used (nplanes > 16 needs M0 >= 16)
      const uint64_t Y2 = nplanes > 16 ? window_lds(rs, u[0] << s2, u[1] << s2, u[2] << s2, u[3] << s2) : 0ull;
      // j is the wave-uniform group-loop count, 1..16 (16 when another lane's group phase filled the window)
      uint64_t t0 = j == 16 ? Y2 : (Y >> (4 * j)) | (Y2 << (64 - 4 * j));
      uint64_t t1 = j == 16 ? 0ull : Y2 >> (4 * j);
      const uint32_t tb = 4u * (uint32_t)tplanes;  // <= 128
      if (tb < 64) { t0 &= (1ull << tb) - 1ull; t1 = 0; }
      else if (tb < 128) t1 &= (1ull << (tb - 64)) - 1ull;
      const uint32_t pt = pos0 + glen;  // in [9, 137]
      if (pt < 64) {
        c[0] |= t0 << pt;
        c[1] |= (t0 >> (64 - pt)) | (t1 << pt);
        c[2] |= t1 >> (64 - pt);
      } else if (pt < 128) {
        const uint32_t q2 = pt - 64;
        c[1] |= t0 << q2;
        c[2] |= (q2 ? t0 >> (64 - q2) : 0ull) | (t1 << q2);
      } else {
        c[2] |= t0 << (pt - 128);
      }
    }
  }
  return len;
}

// Bit length of a variable-rate 1-D block (same domain as encode_block1d_var; Inf/NaN -> special) from the leading
// one-bit planes L_i of its four negabinary coefficients alone. With n_k = 1 + max{i : L_i >= k} the prefix after
// plane k (encode.c:279-339 carries n across planes), plane k costs n_{k+1} verbatim bits plus, when n_{k+1} < 4,
// either one '0' (nothing new) or m + (q == 3 ? 3 : q + 2) - n_{k+1} bits (m new one-bits, the last at q: one group
// flag each, the run up to q, a closing '0' unless q is the implied last position). With R_j = max_{i >= j} L_i summed
// over planes kmin .. 31:
//   sum_j max(0, R_j - kmin) + (32 - max(kmin, L_3)) + #{j : L_j = R_j >= kmin}
//   + sum_j [R_j >= kmin, last index at its level] (j < 3 ? j + 1 : 2) - sum_j [R_j >= kmin, first at its level] j,
// where the last two sums cancel except where R crosses kmin (see encode_ints_length).
__device__ __forceinline__ uint32_t count_block1d_var(const float* f, int minexp, uint32_t maxprec, bool& special)
{
  const uint32_t a0 = __float_as_uint(f[0]) & 0x7fffffffu, a1 = __float_as_uint(f[1]) & 0x7fffffffu;
  const uint32_t a2 = __float_as_uint(f[2]) & 0x7fffffffu, a3 = __float_as_uint(f[3]) & 0x7fffffffu;
  const uint32_t m = max(max(a0, a1), max(a2, a3));
  special = m >= 0x7f800000u;
  const uint32_t E = special ? 150u : (m >> 23);
  const int emax = E ? (int)E - 126 : -126;
  const int prec = min((int)maxprec, max(0, emax - minexp + 4));
  if (m == 0 || prec == 0) return 1u;
  const bool tiny = E < 29u;
  const float s = __uint_as_float((283u - (tiny ? 150u : E)) << 23);
  int32_t q[4];
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = tiny ? (int32_t)0x80000000 : (int32_t)(f[i] * s);
  fwd_lift(q[0], q[1], q[2], q[3]);
  uint32_t u[4];
#pragma unroll
  for (int i = 0; i < 4; i++) u[i] = ((uint32_t)q[i] + 0xaaaaaaaau) ^ 0xaaaaaaaau;
  return 9u + encode_ints_length<4>(u, (uint32_t)prec);  // closed form (codec_device.h), prec >= 1 here
}

// Variable-rate 1-D pass 1: per-range sums of block bit lengths (closed form from the leading planes; generic for
// Inf/NaN blocks).
// Tiles of 256 U blocks; contiguous bf16 input takes coalesced 16-B loads with the next tile prefetched.
template <int DT, int U>
__global__ __launch_bounds__(256) void k_count1d_var(FieldDesc F, Params p, uint32_t range, uint64_t* __restrict__ sums)
{
  constexpr uint32_t TILE = 256u * U;
  constexpr int BPL = DT == DT_BF16 ? 2 : 1;  // blocks per 16-B load
  constexpr int NL = U / BPL;                 // 16-B loads per lane per tile
  static_assert(U % BPL == 0, "U must hold whole 16-B loads");
  __shared__ uint64_t red[4];
  const uint32_t tid = threadIdx.x;
  const uint64_t b0 = (uint64_t)blockIdx.x * range;
  const uint64_t b1 = min<uint64_t>(b0 + range, F.nblocks);
  uint64_t acc = 0;
  uint64_t t0 = b0;
  // Contiguous, 16-B aligned bf16 input: whole tiles of full blocks read with coalesced 16-B loads (load j of lane t
  // covers blocks t0 + (256 j + t) BPL ..; the sum is order-free), the next tile's loads issued before this tile is
  // counted (C5 acc 1e-6 0.878 -> 0.843 ms). The same form measured slower for fp32 (0.876 -> 1.043 ms): fp32 keeps the
  // per-lane gather below.
  if (DT == DT_BF16 && F.vec && F.s[0] == 1 && (((uintptr_t)F.data) & 15u) == 0) {
    const uint64_t lim = min<uint64_t>(b1, F.n[0] / 4);
    const uint64_t tend = lim > b0 ? b0 + (lim - b0) / TILE * TILE : b0;
    const uint4* src = (const uint4*)F.data;  // 16-B units: one f32 block or two bf16 blocks
    uint4 cur[NL], nxt[NL];
    if (t0 < tend) {
#pragma unroll
      for (int j = 0; j < NL; j++) cur[j] = src[t0 / BPL + 256u * j + tid];
    }
    for (; t0 < tend; t0 += TILE) {
      if (t0 + TILE < tend) {
#pragma unroll
        for (int j = 0; j < NL; j++) nxt[j] = src[(t0 + TILE) / BPL + 256u * j + tid];
      }
#pragma unroll
      for (int j = 0; j < NL; j++) {
        float f[BPL][4];
        if constexpr (DT == DT_BF16) {
          const uint32_t w[4] = {cur[j].x, cur[j].y, cur[j].z, cur[j].w};
#pragma unroll
          for (int h = 0; h < 2; h++) {
            f[h][0] = __uint_as_float(w[2 * h] << 16);
            f[h][1] = __uint_as_float(w[2 * h] & 0xffff0000u);
            f[h][2] = __uint_as_float(w[2 * h + 1] << 16);
            f[h][3] = __uint_as_float(w[2 * h + 1] & 0xffff0000u);
          }
        } else {
          f[0][0] = __uint_as_float(cur[j].x); f[0][1] = __uint_as_float(cur[j].y);
          f[0][2] = __uint_as_float(cur[j].z); f[0][3] = __uint_as_float(cur[j].w);
        }
#pragma unroll
        for (int h = 0; h < BPL; h++) {
          bool special;
          uint32_t len = count_block1d_var(f[h], p.minexp, p.maxprec, special);
          if (special) len = count_block<1>(f[h], p);
          acc += len;
        }
      }
#pragma unroll
      for (int j = 0; j < NL; j++) cur[j] = nxt[j];
    }
  }
  for (; t0 < b1; t0 += TILE) {  // the rest (partial tiles, the padded last block, strided input)
    float f[U][4];
#pragma unroll
    for (int k = 0; k < U; k++) {
      const uint64_t b = t0 + (uint64_t)tid * U + k;
      f[k][0] = f[k][1] = f[k][2] = f[k][3] = 0.0f;
      if (b < b1) gather_block<1, DT>(F, (uint32_t)b, f[k]);
    }
#pragma unroll
    for (int k = 0; k < U; k++) {
      const uint64_t b = t0 + (uint64_t)tid * U + k;
      bool special;
      uint32_t len = count_block1d_var(f[k], p.minexp, p.maxprec, special);
      if (special && b < b1) len = count_block<1>(f[k], p);
      acc += b < b1 ? len : 0u;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) sums[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// Variable-rate 1-D pass 2: k_encode_tiles with the closed-form coder over tiles of 256 U blocks (U consecutive
// blocks per lane: U times the work per barrier round); each lane ORs its <= 140-bit codes into the tile's LDS window
// with 64-bit LDS atomics.
template <int DT, int U>
__global__ __launch_bounds__(256) void k_encode1d_var(FieldDesc F, Params p, uint32_t range,
                                                      const uint64_t* __restrict__ rbase, uint32_t* __restrict__ out32,
                                                      uint64_t* __restrict__ index, uint32_t index_shift)
{
  constexpr uint32_t T = 256;
  __shared__ uint64_t lds64[(31 + T * U * 160 + 63) / 64 + 4];
  __shared__ uint32_t scan_sh[T / 64];
  __shared__ uint16_t tab[80];
  __shared__ __attribute__((aligned(16))) uint32_t tab2[1280];
  __shared__ uint32_t rs[1024];  // window spread tables (window_lds)
  uint32_t* lds = (uint32_t*)lds64;
  const uint32_t tid = threadIdx.x;
  if (tid < 80) tab[tid] = plane_entry4(tid);
  stage_table<T, 1280>(tab2, g_plane_tab5.v);
#pragma unroll
  for (uint32_t t = 0; t < 1024 / T; t++) rs[tid + T * t] = rspread_entry(tid + T * t);
  const uint64_t b0 = (uint64_t)blockIdx.x * range;
  const uint64_t b1 = min<uint64_t>(b0 + range, F.nblocks);
  const bool final_range = b1 == F.nblocks;
  uint64_t base = rbase[blockIdx.x];
  const uint64_t first_word = base >> 5;
  const bool first_shared = (base & 31) != 0;
  uint32_t carry = 0;
  // Contiguous, 16-B aligned bf16: a lane's U consecutive blocks are U/2 16-B loads, issued one tile ahead (before
  // this tile's scan / LDS / store rounds) for every tile made of full blocks only. (The same for fp32, U 16-B loads
  // per lane, measured slower: 0.875 -> 0.968 ms at accuracy 1e-6.)
  constexpr bool WIDE = DT == DT_BF16 && U % 2 == 0;
  constexpr int NW = WIDE ? U / 2 : 1;
  const bool wide = WIDE && F.vec && F.s[0] == 1 && (((uintptr_t)F.data) & 15u) == 0;
  const uint64_t full_end = min<uint64_t>(b1, F.n[0] / 4);  // blocks below this are full
  const uint4* src = (const uint4*)F.data;
  uint4 nxt[NW];
  auto wide_tile = [&](uint64_t t) { return wide && t + T * U <= full_end; };
  if (wide_tile(b0)) {
#pragma unroll
    for (int h = 0; h < NW; h++) nxt[h] = src[(b0 + (uint64_t)tid * U) / 2 + h];
  }
  __syncthreads();
  for (uint64_t t0 = b0; t0 < b1; t0 += T * U) {
    float f[U][4];
    if (wide_tile(t0)) {
      uint4 cur[NW];
#pragma unroll
      for (int h = 0; h < NW; h++) cur[h] = nxt[h];
      if (wide_tile(t0 + T * U)) {
#pragma unroll
        for (int h = 0; h < NW; h++) nxt[h] = src[(t0 + T * U + (uint64_t)tid * U) / 2 + h];
      }
#pragma unroll
      for (int h = 0; h < NW; h++) {
        const uint32_t w[4] = {cur[h].x, cur[h].y, cur[h].z, cur[h].w};
#pragma unroll
        for (int g = 0; g < 2 && 2 * h + g < U; g++) {
          f[2 * h + g][0] = __uint_as_float(w[2 * g] << 16);
          f[2 * h + g][1] = __uint_as_float(w[2 * g] & 0xffff0000u);
          f[2 * h + g][2] = __uint_as_float(w[2 * g + 1] << 16);
          f[2 * h + g][3] = __uint_as_float(w[2 * g + 1] & 0xffff0000u);
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < U; k++) {
        const uint64_t b = t0 + (uint64_t)tid * U + k;
        f[k][0] = f[k][1] = f[k][2] = f[k][3] = 0.0f;
        if (b < b1) gather_block<1, DT>(F, (uint32_t)b, f[k]);
      }
    }
    uint64_t c[U][3];
    uint32_t len[U];
    bool sp[U];
    uint32_t lsum = 0;
#pragma unroll
    for (int k = 0; k < U; k++) {
      const bool valid = t0 + (uint64_t)tid * U + k < b1;
      len[k] = encode_block1d_var<true>(f[k], tab, tab2, rs, p.minexp, p.maxprec, c[k], sp[k]);
      sp[k] = sp[k] && valid;
      if (sp[k]) {
        len[k] = count_block<1>(f[k], p);
      }
      len[k] = valid ? len[k] : 0u;
      lsum += len[k];
    }
    uint32_t tile_total;
    const uint32_t excl = block_exclusive_scan<T>(lsum, &tile_total, scan_sh);
    const uint32_t lbase = (uint32_t)(base & 31);
    const uint32_t end_local = lbase + tile_total;
    const uint32_t W = (end_local + 31) >> 5;
    for (uint32_t j = tid; j < (W + 3) / 2; j += T) lds64[j] = 0ull;
    __syncthreads();
    if (tid == 0) lds[0] |= carry;
    __syncthreads();
    uint32_t o = lbase + excl;
#pragma unroll
    for (int k = 0; k < U; k++) {
      if (len[k]) {
        if (sp[k]) {
          LdsWriter w{lds, o, o + len[k]};
          encode_block<1>(w, f[k], p);
        } else {
          const uint32_t qw = o >> 6, sh = o & 63u;
          const uint32_t nq = (sh + len[k] + 63) >> 6;  // 1..4 qwords touched
          atomicOr((unsigned long long*)&lds64[qw], (unsigned long long)(c[k][0] << sh));
          if (nq > 1) atomicOr((unsigned long long*)&lds64[qw + 1],
                               (unsigned long long)((sh ? c[k][0] >> (64 - sh) : 0ull) | (c[k][1] << sh)));
          if (nq > 2) atomicOr((unsigned long long*)&lds64[qw + 2],
                               (unsigned long long)((sh ? c[k][1] >> (64 - sh) : 0ull) | (c[k][2] << sh)));
          if (nq > 3) atomicOr((unsigned long long*)&lds64[qw + 3], (unsigned long long)(c[k][2] >> (64 - sh)));
        }
        const uint64_t b = t0 + (uint64_t)tid * U + k;
        if (index && ((b & ((1ull << index_shift) - 1)) == 0)) index[b >> index_shift] = base + (o - lbase);
      }
      o += len[k];
    }
    __syncthreads();
    const bool last_tile = t0 + T * U >= b1;
    const bool partial = (end_local & 31) != 0;
    const uint32_t Wstore = (last_tile || !partial) ? W : (end_local >> 5);
    const uint64_t gw0 = base >> 5;
    for (uint32_t j = tid; j < Wstore; j += T) {
      const uint64_t gw = gw0 + j;
      const uint32_t v = lds[j];
      const bool shared = (gw == first_word && first_shared) || (last_tile && partial && !final_range && j == W - 1);
      if (shared) atomicOr(out32 + gw, v);
      else out32[gw] = v;
    }
    if (last_tile && final_range && tid == 0) {
      const uint64_t endw = (base + tile_total + 31) >> 5;
      if (endw & 1) out32[endw] = 0u;
    }
    carry = (!last_tile && partial) ? lds[end_local >> 5] : 0u;
    base += tile_total;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ launchers
static inline hipStream_t S(void* s) { return (hipStream_t)s; }

template <int D, int DT, uint32_t T>
static hipError_t launch_tiles_t(const FieldDesc& F, const Params& p, const TilePlan& plan, uint32_t* out32,
                                 uint64_t* ws_sums, uint64_t* ws_base, uint64_t* d_total, uint64_t* index,
                                 uint32_t index_shift, const uint64_t* d_base, hipStream_t st)
{
  const size_t lds = (size_t)plan.lds_words * 4;
  if (plan.fixed) {
    auto kern = k_encode_tiles<D, DT, T, true>;
    if (lds > 65536) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    kern<<<plan.nranges, T, lds, st>>>(F, p, plan.range, nullptr, out32, index, index_shift);
    return hipGetLastError();
  }
  const bool var1d = D == 1 && T == 256 && p.minbits <= 1 && p.maxbits >= 160;
  // variant 2 (A/B, tests): the single-pass look-back encoder (var1d.hip). Not the default: on C5 it ran 0.907 ms
  // against 0.757 ms for count + scan + encode (profiles/r03_c5_single_pass_ab.log)
  const int form = g_var1d_variant.form;
  if (var1d && form == 2) return launch_encode1d_var_sp(F, p, out32, ws_sums, d_total, index, index_shift, d_base, st);
  // variant 1 (A/B, tests): the count + scan + k_encode1d_var form over ranges of plan.range blocks.
  // Default: the tile form (var1d.hip: count per tile with byte lengths, scan, the tile coder placed by the scan)
  if (var1d && form != 1)
    return launch_encode1d_var_tile(F, p, out32, ws_sums, d_total, index, index_shift, d_base, st);
  if (var1d) k_count1d_var<DT, 4><<<plan.nranges, T, 0, st>>>(F, p, plan.range, ws_sums);
  else k_count<D, DT, T><<<plan.nranges, T, 0, st>>>(F, p, plan.range, ws_sums);
  hipError_t e = launch_scan_ranges(ws_sums, plan.nranges, ws_base, d_total, out32, d_base, st);
  if (e != hipSuccess) return e;
  if (var1d) {
    // U = 4 blocks per lane (U = 8 measured 0.835 -> 1.083 ms on C5 acc 1e-6: register pressure)
    k_encode1d_var<DT, 4><<<plan.nranges, T, 0, st>>>(F, p, plan.range, ws_base, out32, index, index_shift);
    return hipGetLastError();
  }
  auto kern = k_encode_tiles<D, DT, T, false>;
  if (lds > 65536) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  kern<<<plan.nranges, T, lds, st>>>(F, p, plan.range, ws_base, out32, index, index_shift);
  return hipGetLastError();
}

#define GCOW_TILES(D, T)                                                                                       \
  return bf ? launch_tiles_t<D, DT_BF16, T>(F, p, plan, out32, ws_sums, ws_base, d_total, index, index_shift, d_base, st) \
            : launch_tiles_t<D, DT_F32, T>(F, p, plan, out32, ws_sums, ws_base, d_total, index, index_shift, d_base, st)
hipError_t launch_encode_tiles(const FieldDesc& F, const Params& p, const TilePlan& plan, uint32_t* out32,
                               uint64_t* ws_sums, uint64_t* ws_base, uint64_t* d_total, uint64_t* index,
                               uint32_t index_shift, const uint64_t* d_base, void* stream)
{
  hipStream_t st = S(stream);
  const bool bf = F.dtype == DT_BF16;
  if (F.dims != 1) return launch_encode_tiles23(F, p, plan, out32, ws_sums, ws_base, d_total, index, index_shift, d_base, st);
  if (plan.threads == 256) { GCOW_TILES(1, 256); } else { GCOW_TILES(1, 64); }
}
#undef GCOW_TILES

}  // namespace gcow
