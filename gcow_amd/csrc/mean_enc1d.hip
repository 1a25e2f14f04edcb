// mean_enc1d.hip -- the sharded hook's second stage: W received stream pieces straight into the stream of their mean
// (gcow_decode_mean_encode_device, include/gcow.h), optionally with the error-feedback residual of that stream.
//   k_decode_mean_encode_fixed1d_np    the lean fixed-rate domain (whole-word blocks, kmin = 0), one-shot grid: per
//                                      block the W words decoded and summed in rank order (k_decode_mean_fixed1d_np),
//                                      the mean, y = m + e, the word (encode_block1d_lean6) and, with a residual, the
//                                      word decoded from its register and e' = finite(y - decode)
//                                      (k_encode_resid1d_np): 8 W + 8 (rate 16) bytes per block where decode_mean into
//                                      an fp32 field followed by the encoder moves 8 W + 16 + 16 + 8
//   k_decode_mean_encode_fixed1d_tail  the partial last block, one lane
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>
#include <type_traits>

#include "codec_device.h"
#include "dec1d.h"
#include "enc_fixed1d.h"
#include "field_io.h"
#include "kernels.h"
#include "lean1d.h"
#include "mean1d.h"
#include "pipe.h"
#include "regbits.h"
#include "var1d_prep.h"  // resid_bits

// ---- tunables (A/B builds: tools/build_variant.sh)
#ifndef GCOW_MEANENC_U
#define GCOW_MEANENC_U 2  // blocks per lane (k_decode_mean_fixed1d_np's GCOW_DMEAN_U)
#endif

namespace gcow {

enum { kMeanEncPlain = 0, kMeanEncResidE = 1, kMeanEncResid0 = 2 };  // RES: no residual / with e_in / e_in = zeros

// The decoder table image: 64-bit blocks take the pair table with the gather tables behind it (DecTabPG), which
// serves both the W stream decodes and the decode of the word just coded; 32-bit blocks the plane table.
template <uint32_t WB> struct MeanEncDecTab {
  using T = typename std::conditional<WB == 64, DecTabPG, DecTab1>::type;
  static __device__ __forceinline__ const void* ptr()
  {
    if constexpr (WB == 64) return &g_dec_pair_gather;
    else return &g_dec_tab1;
  }
};

// One whole-word block from a register; special lanes (a group phase longer than the window, a plane code crossing
// the budget) through the generic decoder over the same register.
template <uint32_t WB>
__device__ __forceinline__ void meanenc_decode(uint64_t w, const uint32_t* dtab32, const Params& p, float* f)
{
  bool special;
  if constexpr (WB == 64) decode_block1d_pair<true>(w, dtab32, f, special);
  else decode_block1d_fast<WB>(w, (const uint16_t*)dtab32, f, special);
  if (special) {
    RegReader64 rd{w, 0u};
    decode_block<1>(rd, p, f);
  }
}

// k_decode_mean_fixed1d_np's shape: a one-shot grid, each lane U blocks 256 apart inside its workgroup's chunk of
// 256 U blocks; both tables are requested first (raw loads, one hand-counted wait), then stream 0's U words; stream
// r + 1's words are requested before stream r's blocks are decoded. The e rows are requested after the table barrier
// and used after the stream loop. Every load and store behind the table prologue is a compiler builtin. e_in and
// e_out may be the same buffer: a lane reads the e rows of its own blocks only, all of them before its first store.
// Out-of-range lanes read zeros (a zero word decodes to a zero block, which codes to a zero word) and their stores are
// dropped by the buffer range checks, so control flow stays wave-uniform. Full blocks only.
template <uint32_t WB, int U, int RES>
__global__ __launch_bounds__(256) void k_decode_mean_encode_fixed1d_np(Params p, const uint64_t* __restrict__ in,
                                                                       uint64_t stream_words, uint32_t nstreams,
                                                                       uint32_t nfull, const float* e_in, float* e_out,
                                                                       void* __restrict__ out)
{
#pragma clang fp contract(off)
  using DTab = typename MeanEncDecTab<WB>::T;
  // k_encode_resid1d_np's layout: the encoder's pair table and spread tables, then the decoder's image
  __shared__ __attribute__((aligned(16))) uint32_t tab[1280 + 1024];
  __shared__ __attribute__((aligned(16))) uint32_t dtab32[sizeof(DTab) / 4];
  constexpr uint32_t WBYTES = WB / 8;
  const uint32_t b0 = blockIdx.x * (256u * U) + threadIdx.x;
  constexpr int NT = 1280 / 256;
  constexpr uint32_t TCH = sizeof(DTab) / 16, TR = (TCH + 255) / 256;
  const pipe_v4i rt = buf_rsrc(&g_plane_tab5, sizeof(PlaneTab2));
  const pipe_v4i rdt = buf_rsrc(MeanEncDecTab<WB>::ptr(), sizeof(DTab));
  uint32_t tv[NT];
#pragma unroll
  for (int i = 0; i < NT; i++) tv[i] = buf_load_u32((threadIdx.x + 256u * i) * 4u, rt);
  pipe_v4u dv[TR];
#pragma unroll
  for (uint32_t i = 0; i < TR; i++) dv[i] = buf_load_b128((threadIdx.x + 256u * i) * 16u, rdt);
  auto rsrc = [&](uint32_t r) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(in + (uint64_t)r * stream_words), 0, (int)(nfull * WBYTES),
                                             0x00020000);
  };
  typename MeanWord<WB>::T cur[U];
  {
    const auto rs = rsrc(0);
#pragma unroll
    for (int k = 0; k < U; k++) cur[k] = MeanWord<WB>::load(rs, b0 + 256u * k);
  }
#pragma unroll
  for (uint32_t t = threadIdx.x; t < 1024; t += 256) tab[1280 + t] = rspread_entry(t);
  // the table loads are the oldest: once at most U loads are outstanding they have landed
  asm volatile("s_waitcnt vmcnt(%5)" : "+v"(tv[0]), "+v"(tv[1]), "+v"(tv[2]), "+v"(tv[3]), "+v"(tv[4]) : "n"(U)
               : "memory");
  table_wait<U>(dv);
#pragma unroll
  for (int i = 0; i < NT; i++) tab[threadIdx.x + 256u * i] = tv[i];
#pragma unroll
  for (uint32_t i = 0; i < TR; i++)
    if (threadIdx.x + 256u * i < TCH) ((pipe_v4u*)dtab32)[threadIdx.x + 256u * i] = dv[i];
  __syncthreads();
  pipe_v4f re[RES == kMeanEncResidE ? U : 1];
  if constexpr (RES == kMeanEncResidE) {
    const __amdgpu_buffer_rsrc_t rein = __builtin_amdgcn_make_buffer_rsrc((void*)e_in, 0, (int)(nfull * 16u), 0x00020000);
#pragma unroll
    for (int k = 0; k < U; k++) {
      const pipe_v4u v = __builtin_amdgcn_raw_buffer_load_b128(rein, (int)((b0 + 256u * k) * 16u), 0, 0);
      re[k] = __builtin_bit_cast(pipe_v4f, v);
    }
  }
  float acc[U][4];
#pragma unroll
  for (int k = 0; k < U; k++) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0f;
  for (uint32_t r = 0; r < nstreams; r++) {
    typename MeanWord<WB>::T nxt[U];  // stream r + 1's words
    if (r + 1 < nstreams) {
      const auto rs = rsrc(r + 1);
#pragma unroll
      for (int k = 0; k < U; k++) nxt[k] = MeanWord<WB>::load(rs, b0 + 256u * k);
    }
#pragma unroll
    for (int k = 0; k < U; k++) {
      float f[4];
      meanenc_decode<WB>((uint64_t)cur[k], dtab32, p, f);
#pragma unroll
      for (int i = 0; i < 4; i++) acc[k][i] = acc[k][i] + f[i];
    }
#pragma unroll
    for (int k = 0; k < U; k++) cur[k] = nxt[k];
  }
  mean_scale<U * 4>(&acc[0][0], nstreams);
  const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)(nfull * WBYTES), 0x00020000);
  const __amdgpu_buffer_rsrc_t rerr =
      __builtin_amdgcn_make_buffer_rsrc((void*)e_out, 0, RES == kMeanEncPlain ? 0 : (int)(nfull * 16u), 0x00020000);
#pragma unroll
  for (int k = 0; k < U; k++) {
    const uint32_t b = b0 + 256u * k;
    float y[4];
    if constexpr (RES == kMeanEncResidE) {
      y[0] = __fadd_rn(acc[k][0], re[k].x);
      y[1] = __fadd_rn(acc[k][1], re[k].y);
      y[2] = __fadd_rn(acc[k][2], re[k].z);
      y[3] = __fadd_rn(acc[k][3], re[k].w);
    } else if constexpr (RES == kMeanEncResid0) {
#pragma unroll
      for (int i = 0; i < 4; i++) y[i] = __fadd_rn(acc[k][i], 0.0f);  // e = +0: -0 becomes +0 as in resid_block
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++) y[i] = acc[k][i];
    }
    bool special;
    uint64_t w = encode_block1d_lean6<WB, true>(y, tab, tab + 1280, special);
    if (special) {
      RegWriter64 rw{0ull, 0u};
      encode_block<1>(rw, y, p);
      w = WB == 64 ? rw.acc : (rw.acc & ((1ull << WB) - 1ull));
    }
    // aux 2 = non-temporal
    if constexpr (WB == 64) {
      pipe_v2u wv;
      wv.x = (uint32_t)w;
      wv.y = (uint32_t)(w >> 32);
      __builtin_amdgcn_raw_buffer_store_b64(wv, rout, (int)(b * 8u), 0, 2);
    } else {
      __builtin_amdgcn_raw_buffer_store_b32((uint32_t)w, rout, (int)(b * 4u), 0, 2);
    }
    if constexpr (RES != kMeanEncPlain) {
      float d[4];
      meanenc_decode<WB>(w, dtab32, p, d);
      pipe_v4u v;
      v.x = resid_bits(y[0], d[0]);
      v.y = resid_bits(y[1], d[1]);
      v.z = resid_bits(y[2], d[2]);
      v.w = resid_bits(y[3], d[3]);
      __builtin_amdgcn_raw_buffer_store_b128(v, rerr, (int)(b * 16u), 0, 2);
    }
  }
}

// The partial last block (nvals % 4 != 0), one lane: the generic decode of the W partial blocks (each from its own
// word), the mean, the padded gather of m and e (encode.c:41-60; the padding values are copies of real y values), the
// generic whole-word coder and, with a residual (e_out set; e_in null: zeros), the real values' residuals only.
template <uint32_t WB>
__global__ void k_decode_mean_encode_fixed1d_tail(Params p, const uint64_t* __restrict__ in, uint64_t stream_words,
                                                  uint32_t nstreams, uint64_t nvals, uint32_t b, const float* e_in,
                                                  float* e_out, void* __restrict__ out)
{
#pragma clang fp contract(off)
  __shared__ uint16_t tab[80];
  if (threadIdx.x < 80) tab[threadIdx.x] = plane_entry4(threadIdx.x);
  __syncthreads();
  if (threadIdx.x) return;
  const uint64_t i0 = 4ull * b;
  const uint32_t nv = (uint32_t)(nvals - i0);
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (uint32_t r = 0; r < nstreams; r++) {
    const uint64_t* sr = in + (uint64_t)r * stream_words;
    RegReader64 rd{WB == 64 ? sr[b] : (uint64_t)((const uint32_t*)sr)[b], 0u};
    float f[4];
    decode_block<1>(rd, p, f);
#pragma unroll
    for (int i = 0; i < 4; i++) acc[i] = acc[i] + f[i];
  }
  mean_scale<4>(acc, nstreams);
  float y[4];
#pragma unroll
  for (uint32_t x = 0; x < 4u; x++) {
    const uint32_t j = pad_index(x, nv);
    const float m = j == 0u ? acc[0] : (j == 1u ? acc[1] : (j == 2u ? acc[2] : acc[3]));
    y[x] = e_out ? __fadd_rn(m, e_in ? e_in[i0 + j] : 0.0f) : m;
  }
  const uint64_t w = encode_block1d_fixed<WB>(y, p, tab);
  if constexpr (WB == 64) ((uint64_t*)out)[b] = w;
  else ((uint32_t*)out)[b] = (uint32_t)w;
  if (!e_out) return;
  RegReader64 rd{w, 0u};
  float d[4];
  decode_block<1>(rd, p, d);
#pragma unroll
  for (uint32_t x = 0; x < 4u; x++)
    if (x < nv) e_out[i0 + x] = __uint_as_float(resid_bits(y[x], d[x]));
}

// ------------------------------------------------------------------------------------------------ launcher
template <uint32_t WB>
static void launch_meanenc_t(uint64_t nvals, const Params& p, const uint64_t* in, uint64_t stream_words,
                             uint32_t nstreams, const float* e_in, float* e_out, void* out, hipStream_t st)
{
  const uint32_t nfull = (uint32_t)(nvals / 4);
  // chunks keep every offset into the buffers below 2^32 (16 bytes per block at most); a chunk starts on a whole
  // stream word (2^27 blocks of 32 bits)
  constexpr uint32_t CH = 1u << 27;
  constexpr int U = GCOW_MEANENC_U;
  for (uint32_t c0 = 0; c0 < nfull; c0 += CH) {
    const uint32_t nc = std::min(CH, nfull - c0);
    const uint64_t* ic = (const uint64_t*)((const char*)in + (size_t)c0 * (WB / 8));
    void* oc = (char*)out + (size_t)c0 * (WB / 8);
    const float* ei = e_in ? e_in + (size_t)c0 * 4 : nullptr;
    float* eo = e_out ? e_out + (size_t)c0 * 4 : nullptr;
    const uint32_t g = (nc + 256 * U - 1) / (256 * U);
    if (!e_out)
      k_decode_mean_encode_fixed1d_np<WB, U, kMeanEncPlain><<<g, 256, 0, st>>>(p, ic, stream_words, nstreams, nc,
                                                                                 nullptr, nullptr, oc);
    else if (e_in)
      k_decode_mean_encode_fixed1d_np<WB, U, kMeanEncResidE><<<g, 256, 0, st>>>(p, ic, stream_words, nstreams, nc, ei,
                                                                                  eo, oc);
    else
      k_decode_mean_encode_fixed1d_np<WB, U, kMeanEncResid0><<<g, 256, 0, st>>>(p, ic, stream_words, nstreams, nc,
                                                                                  nullptr, eo, oc);
  }
  if (nvals % 4)
    k_decode_mean_encode_fixed1d_tail<WB><<<1, 128, 0, st>>>(p, in, stream_words, nstreams, nvals, nfull, e_in, e_out,
                                                             out);
}

hipError_t launch_decode_mean_encode_fixed1d(uint64_t nvals, const Params& p, const uint64_t* in,
                                             uint64_t stream_words, uint32_t nstreams, const float* e_in, float* e_out,
                                             void* out, void* stream)
{
  if (!nvals) return hipSuccess;
  if (p.maxbits == 64) launch_meanenc_t<64>(nvals, p, in, stream_words, nstreams, e_in, e_out, out, (hipStream_t)stream);
  else launch_meanenc_t<32>(nvals, p, in, stream_words, nstreams, e_in, e_out, out, (hipStream_t)stream);
  return hipGetLastError();
}

}  // namespace gcow
