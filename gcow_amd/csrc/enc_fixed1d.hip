// enc_fixed1d.hip -- the fused fixed-rate 1-D encoder (the headline kernel): one 4-value block per lane, block b at
// bits [b * maxbits, ...) (sw/src/zfp.c:31-56 loop + sw/src/encode.c:41-495; hw/src/zfp.cpp:31-75 dataflow stages).
//   k_encode_fixed1d_np       one-shot grid, the lean-6 closed-form coder (whole-word blocks, kmin = 0)
//   k_encode_fixed1d_generic  parameters outside the lean coder's domain
//   k_encode_fixed1d_tail     the partial last block
//   k_copy_pattern1d          the memory floor of the same access pattern (bench.py roofline.copy_ceiling)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>

#include "codec_device.h"
#include "field_io.h"
#include "kernels.h"
#include "lean1d.h"
#include "pipe.h"

// ---- tunables (A/B builds: tools/build_variant.sh NAME "-DGCOW_C2_U=4" enc_fixed1d.hip)
#ifndef GCOW_C2_U
#define GCOW_C2_U 8  // blocks per lane of the one-shot grid
#endif

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

// One-shot (non-persistent) fixed-rate 1-D encoder: each lane codes U blocks 256 apart inside its workgroup's chunk
// of 256 U blocks. All U loads are issued first (before the LDS table fill), then each block waits for its own load
// only: with U loads followed by k stores outstanding, load k has landed once at most U - 1 operations remain
// (vmcnt counts loads and stores together, in issue order). Out-of-range lanes read zeros and their stores are
// dropped by the buffer range check, so control flow stays wave-uniform. Measured against a persistent grid-stride
// pipeline (tools/ubench/legacy_variants.hip), the one-shot shape streams HBM like a plain copy kernel (DESIGN.md
// section 6). The raw loads, stores and counted waits are in pipe.h.
template <int DT, uint32_t WB, int U, uint32_t T = 256, int V = 0>
__global__ __launch_bounds__(T) void k_encode_fixed1d_np(const void* __restrict__ in, uint32_t nfull, Params p,
                                                         void* __restrict__ out)
{
  __shared__ __attribute__((aligned(16))) uint32_t tab[1280 + 1024];  // pair table, then the four window spread tables
  constexpr uint32_t IB = DT == DT_BF16 ? 8u : 16u;  // input bytes per block
  const pipe_v4i rin = buf_rsrc(in, nfull * IB), rout = buf_rsrc(out, nfull * (WB / 8));
  const uint32_t b0 = blockIdx.x * (T * U) + threadIdx.x;
  typename PipeRow<DT>::T r[U];
  if constexpr ((V & 1) != 0) {
    // pair-table loads issued first (hand-counted like the data loads), so waiting for them is vmcnt(U) and block 0
    // can start as soon as its own load lands (a compiler-issued table load after the data loads waits vmcnt(0))
    static_assert(T == 256, "table fill assumes 256 threads");
    constexpr int NT = 1280 / 256;
    const pipe_v4i rt = buf_rsrc(&g_plane_tab5, sizeof(PlaneTab2));
    uint32_t tv[NT];
#pragma unroll
    for (int i = 0; i < NT; i++) tv[i] = buf_load_u32((threadIdx.x + 256u * i) * 4u, rt);
#pragma unroll
    for (int k = 0; k < U; k++) r[k] = PipeRow<DT>::load((b0 + T * k) * IB, rin);
#pragma unroll
    for (uint32_t t = threadIdx.x; t < 1024; t += T) tab[1280 + t] = rspread_entry(t);
    asm volatile("s_waitcnt vmcnt(%5)" : "+v"(tv[0]), "+v"(tv[1]), "+v"(tv[2]), "+v"(tv[3]), "+v"(tv[4]) : "n"(U)
                 : "memory");
#pragma unroll
    for (int i = 0; i < NT; i++) tab[threadIdx.x + 256u * i] = tv[i];
  } else {
#pragma unroll
    for (int k = 0; k < U; k++) r[k] = PipeRow<DT>::load((b0 + T * k) * IB, rin);
#pragma unroll
    for (uint32_t t = threadIdx.x; t < 1280; t += T) tab[t] = g_plane_tab5.v[t];
    // the spread tables are computed, not loaded: entry 256 i + b = byte b reversed onto nibble bit i
#pragma unroll
    for (uint32_t t = threadIdx.x; t < 1024; t += T) tab[1280 + t] = rspread_entry(t);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < U; k++) {
    pipe_wait<U - 1>(r[k]);
    float f[4];
    PipeRow<DT>::unpack(r[k], f);
    bool special;
    uint64_t w = encode_block1d_lean6<WB, (V & 2) != 0>(f, tab, tab + 1280, special);
    if (special) {
      RegWriter64 rw{0ull, 0u};
      encode_block<1>(rw, f, p);
      w = WB == 64 ? rw.acc : (rw.acc & ((1ull << WB) - 1ull));
    }
    pipe_store<WB>((b0 + T * k) * (WB / 8), rout, w);
  }
}

// The memory floor of the fixed-rate 1-D encoder's access pattern (bench.py `roofline.copy_ceiling`): the same
// one-shot grid, U = 8 blocks per lane, the same raw buffer loads (16 B fp32 / 8 B bf16 per block) and WB-bit
// non-temporal stores with the same hand-counted waits, and no coding (each block's store is an xor-fold of its load).
template <int DT, uint32_t WB, int U>
__global__ __launch_bounds__(256) void k_copy_pattern1d(const void* __restrict__ in, uint32_t nfull,
                                                        void* __restrict__ out)
{
  constexpr uint32_t T = 256;
  constexpr uint32_t IB = DT == DT_BF16 ? 8u : 16u;
  const pipe_v4i rin = buf_rsrc(in, nfull * IB), rout = buf_rsrc(out, nfull * (WB / 8));
  const uint32_t b0 = blockIdx.x * (T * U) + threadIdx.x;
  typename PipeRow<DT>::T r[U];
#pragma unroll
  for (int k = 0; k < U; k++) r[k] = PipeRow<DT>::load((b0 + T * k) * IB, rin);
#pragma unroll
  for (int k = 0; k < U; k++) {
    pipe_wait<U - 1>(r[k]);
    float f[4];
    PipeRow<DT>::unpack(r[k], f);
    const uint64_t w = ((uint64_t)(__float_as_uint(f[0]) ^ __float_as_uint(f[1])) << 32) |
                       (__float_as_uint(f[2]) ^ __float_as_uint(f[3]));
    pipe_store<WB>((b0 + T * k) * (WB / 8), rout, w);
  }
}

// Generic fixed-rate 1-D encoder over the full 4-value blocks [0, nfull) for parameters outside the lean coder's
// domain (maxprec < 32 or minexp > -154: kmin > 0 possible); two blocks per lane, loads issued first.
template <int DT, uint32_t WB>
__global__ __launch_bounds__(256) void k_encode_fixed1d_generic(const void* __restrict__ in, uint32_t nfull, Params p,
                                                                void* __restrict__ out)
{
  __shared__ uint16_t tab[80];
  if (threadIdx.x < 80) tab[threadIdx.x] = plane_entry4(threadIdx.x);
  __syncthreads();
  constexpr int U = 2;
  const uint32_t b0 = blockIdx.x * (256u * U) + threadIdx.x;
  float f[U][4];
#pragma unroll
  for (int j = 0; j < U; j++) {
    const uint32_t b = b0 + 256u * j;
    if (b < nfull) load_row4<DT>(in, 4ll * b, f[j]);
  }
#pragma unroll
  for (int j = 0; j < U; j++) {
    const uint32_t b = b0 + 256u * j;
    if (b < nfull) {
      const uint64_t w = encode_block1d_fixed<WB>(f[j], p, tab);
      if constexpr (WB == 64) ((uint64_t*)out)[b] = w;
      else ((uint32_t*)out)[b] = (uint32_t)w;
    }
  }
}

// The partial last block of a 1-D bucket (nvals % 4 != 0): padded gather (encode.c:41-60), one lane.
template <int DT, uint32_t WB>
__global__ void k_encode_fixed1d_tail(const void* __restrict__ in, uint64_t nvals, uint32_t b, Params p,
                                      void* __restrict__ out)
{
  __shared__ uint16_t tab[80];
  if (threadIdx.x < 80) tab[threadIdx.x] = plane_entry4(threadIdx.x);
  __syncthreads();
  if (threadIdx.x) return;
  float f[4];
  load_block1d<DT>(in, nvals, b, f);
  const uint64_t w = encode_block1d_fixed<WB>(f, p, tab);
  if constexpr (WB == 64) ((uint64_t*)out)[b] = w;
  else ((uint32_t*)out)[b] = (uint32_t)w;
}

// ------------------------------------------------------------------------------------------------ launchers
static inline hipStream_t S(void* s) { return (hipStream_t)s; }

template <int DT, uint32_t WB>
static void launch_fixed1d_t(const void* in, uint64_t nvals, const Params& p, void* out, hipStream_t st)
{
  const uint32_t nfull = (uint32_t)(nvals / 4);
  if (nfull) {
    // the lean coder needs prec >= 32 for every nonzero block: e >= -126 => e - minexp + 4 >= 32
    const bool kmin0 = p.maxprec >= 32 && p.minexp <= -154;
    if (!kmin0) {
      k_encode_fixed1d_generic<DT, WB><<<(nfull + 511) / 512, 256, 0, st>>>(in, nfull, p, out);
    } else {
      // one-shot grid, U = 8 blocks per lane; chunks keep every buffer offset below 2^32
      constexpr uint32_t CH = 1u << 27;
      constexpr uint32_t IB = DT == DT_BF16 ? 8u : 16u;
      for (uint32_t c0 = 0; c0 < nfull; c0 += CH) {
        const uint32_t nc = min(CH, nfull - c0);
        const void* ic = (const char*)in + (size_t)c0 * IB;
        void* oc = (char*)out + (size_t)c0 * (WB / 8);
        constexpr int U = GCOW_C2_U;
        k_encode_fixed1d_np<DT, WB, U, 256, 3><<<(nc + 256 * U - 1) / (256 * U), 256, 0, st>>>(ic, nc, p, oc);
      }
    }
  }
  if (nvals % 4) k_encode_fixed1d_tail<DT, WB><<<1, 128, 0, st>>>(in, nvals, nfull, p, out);
}

hipError_t launch_copy_pattern1d(const void* in, int dtype, uint64_t nvals, uint32_t wb, void* out, void* stream)
{
  const uint32_t nfull = (uint32_t)(nvals / 4);
  constexpr uint32_t CH = 1u << 27;
  const uint32_t IB = dtype == DT_BF16 ? 8u : 16u;
  for (uint32_t c0 = 0; c0 < nfull; c0 += CH) {
    const uint32_t nc = std::min(CH, nfull - c0);
    const void* ic = (const char*)in + (size_t)c0 * IB;
    void* oc = (char*)out + (size_t)c0 * (wb / 8);
    const uint32_t g = (nc + 2047) / 2048;
    if (dtype == DT_BF16) {
      if (wb == 64) k_copy_pattern1d<DT_BF16, 64, 8><<<g, 256, 0, S(stream)>>>(ic, nc, oc);
      else k_copy_pattern1d<DT_BF16, 32, 8><<<g, 256, 0, S(stream)>>>(ic, nc, oc);
    } else {
      if (wb == 64) k_copy_pattern1d<DT_F32, 64, 8><<<g, 256, 0, S(stream)>>>(ic, nc, oc);
      else k_copy_pattern1d<DT_F32, 32, 8><<<g, 256, 0, S(stream)>>>(ic, nc, oc);
    }
  }
  return hipGetLastError();
}

hipError_t launch_encode_fixed1d(const void* in, int dtype, uint64_t nvals, uint32_t nblocks, const Params& p,
                                 void* out, void* stream)
{
  (void)nblocks;
  hipStream_t st = S(stream);
  if (dtype == DT_F32) {
    if (p.maxbits == 64) launch_fixed1d_t<DT_F32, 64>(in, nvals, p, out, st);
    else launch_fixed1d_t<DT_F32, 32>(in, nvals, p, out, st);
  } else {
    if (p.maxbits == 64) launch_fixed1d_t<DT_BF16, 64>(in, nvals, p, out, st);
    else launch_fixed1d_t<DT_BF16, 32>(in, nvals, p, out, st);
  }
  return hipGetLastError();
}

}  // namespace gcow
