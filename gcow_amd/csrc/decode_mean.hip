// decode_mean.hip -- decode + mean of nstreams 1-D streams in one launch (block decoders and tables: dec1d.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <stdint.h>

#include "codec_device.h"
#include "dec1d.h"
#include "field_io.h"
#include "kernels.h"
#include "mean1d.h"
#include "pipe.h"

// ---- tunables (A/B builds: tools/build_variant.sh)
#ifndef GCOW_DMEAN_U
#define GCOW_DMEAN_U 2  // k_decode_mean_fixed1d_np: blocks per lane (U = 1 / 4 / 8: 2.47 / 2.37 / 3.0 against 2.33 ms, W = 8 rate 16: profiles/r04_decode_mean_blocks_per_lane.log)
#endif
#ifndef GCOW_DMEAN_D
#define GCOW_DMEAN_D 1  // k_decode_mean_fixed1d_np: streams whose words are requested ahead (1 or 2)
#endif
#ifndef GCOW_DMV_WAVES
#define GCOW_DMV_WAVES 3  // 16-block chunks: 64 sums per lane, no spills at 3 waves (4 waves: 33 spilled VGPRs)
#endif
#ifndef GCOW_DMV8_WAVES
#define GCOW_DMV8_WAVES 5  // 8-block chunks: 32 sums per lane, 96 VGPRs (2 spilled) at 5 waves: 3.43 -> 3.05 ms (W = 8)
#endif

namespace gcow {

// ------------------------------------------------------------------------------------------------ decode + mean
// The receive side of the compressed all-gather hook: nstreams 1-D streams of the same shape
// (one per rank, stream_words apart) are decoded and averaged in one launch instead of one decode and one add per
// rank. Each lane accumulates in fp32 in rank order, acc = ((0 + x_0) + x_1) + ..., then stores acc / nstreams: the
// values a sequence of decode -> add kernels would give (no contraction of the dequantising multiply into the add).

// Fixed rate. WB = 64 / 32: the one-shot table decoder (whole-word blocks, kmin = 0); WB = 0: the generic decoder
// (any fixed rate). One block per lane.
template <uint32_t WB>
__global__ __launch_bounds__(256) void k_decode_mean_fixed1d(FieldDesc F, Params p, const uint64_t* __restrict__ in,
                                                             uint64_t stream_words, uint32_t nstreams, uint64_t bfirst)
{
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) uint16_t dtab[WB ? 5 * 8 * 128 : 8];
  if (WB) {
    stage_lds16<256, sizeof(DecTab1) / 16>(dtab, &g_dec_tab1, sizeof(DecTab1));
    __syncthreads();
  }
  const uint64_t b = bfirst + (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (b >= F.nblocks) return;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (uint32_t r = 0; r < nstreams; r++) {
    const uint64_t* sr = in + (uint64_t)r * stream_words;
    float f[4];
    bool special = true;
    if constexpr (WB == 64) decode_block1d_fast<64>(sr[b], dtab, f, special);
    else if constexpr (WB == 32) decode_block1d_fast<32>(((const uint32_t*)sr)[b], dtab, f, special);
    if (special) {
      BitReader rd{sr, b * p.maxbits};
      decode_block<1>(rd, p, f);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) acc[i] = acc[i] + f[i];
  }
  mean_scale<4>(acc, nstreams);
  store_block1d(F, b, acc);
}

// The fixed-rate mean in the shape of k_decode_fixed1d_np (whole-word blocks, kmin = 0): one-shot, U blocks per lane
// 256 apart, the plane table requested first (raw loads, hand-counted wait); stream s + 1's U words are requested
// before stream s's blocks are decoded. The stream words are compiler-visible buffer loads: they are carried across
// the stream loop, and a value loaded by inline asm must not be carried (the loop's register copies would read the
// destination before the load has written it). Full blocks only (the launcher sends a partial last block to
// k_decode_mean_fixed1d).
template <uint32_t WB, int U, int D>
__global__ __launch_bounds__(256) void k_decode_mean_fixed1d_np(FieldDesc F, Params p, const uint64_t* __restrict__ in,
                                                                uint64_t stream_words, uint32_t nstreams,
                                                                uint32_t nfull)
{
#pragma clang fp contract(off)
  // 64-bit blocks: the two-plane table (profiles/r04_dec_pair_table.log) with the inverse window transpose through the
  // LDS gather tables (W = 8: 2.08 -> 1.87 ms, profiles/r05_dec_gather_ab.log), staged as one image
  constexpr bool PAIR = WB == 64;
  using PTab = DecTabPG;
  using Tab = typename std::conditional<PAIR, PTab, DecTab1>::type;
  __shared__ __attribute__((aligned(16))) uint32_t dtab32[sizeof(Tab) / 4];
  const uint16_t* dtab = (const uint16_t*)dtab32;
  constexpr uint32_t WBYTES = WB / 8;
  const uint32_t b0 = blockIdx.x * (256u * U) + threadIdx.x;
  constexpr uint32_t TCH = sizeof(Tab) / 16, TR = (TCH + 255) / 256;
  const pipe_v4i rt = PAIR ? buf_rsrc(&g_dec_pair_gather, sizeof(PTab)) : buf_rsrc(&g_dec_tab1, sizeof(DecTab1));
  pipe_v4u tv[TR];
#pragma unroll
  for (uint32_t i = 0; i < TR; i++) tv[i] = buf_load_b128((threadIdx.x + 256u * i) * 16u, rt);
  auto rsrc = [&](uint32_t r) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(in + (uint64_t)r * stream_words), 0, (int)(nfull * WBYTES),
                                             0x00020000);
  };
  typename MeanWord<WB>::T cur[U], nx1[U];
  {
    const auto rs = rsrc(0);
#pragma unroll
    for (int k = 0; k < U; k++) cur[k] = MeanWord<WB>::load(rs, b0 + 256u * k);
    if (D == 2 && nstreams > 1) {
      const auto rs1 = rsrc(1);
#pragma unroll
      for (int k = 0; k < U; k++) nx1[k] = MeanWord<WB>::load(rs1, b0 + 256u * k);
    }
  }
  // the table loads are the oldest: once at most D U loads are outstanding they have landed
  table_wait<D * U>(tv);
#pragma unroll
  for (uint32_t i = 0; i < TR; i++)
    if (threadIdx.x + 256u * i < TCH) ((pipe_v4u*)dtab32)[threadIdx.x + 256u * i] = tv[i];
  __syncthreads();
  float acc[U][4];
#pragma unroll
  for (int k = 0; k < U; k++) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0f;
  for (uint32_t r = 0; r < nstreams; r++) {
    typename MeanWord<WB>::T nxt[U];  // stream r + D's words
    if (r + D < nstreams) {
      const auto rs = rsrc(r + D);
#pragma unroll
      for (int k = 0; k < U; k++) nxt[k] = MeanWord<WB>::load(rs, b0 + 256u * k);
    }
    const uint64_t* sr = in + (uint64_t)r * stream_words;
#pragma unroll
    for (int k = 0; k < U; k++) {
      const uint32_t b = b0 + 256u * k;
      float f[4];
      bool special;
      if constexpr (PAIR) decode_block1d_pair<true>((uint64_t)cur[k], dtab32, f, special);
      else decode_block1d_fast<WB>((uint64_t)cur[k], dtab, f, special);
      if (special && b < nfull) {
        BitReader rd{sr, (uint64_t)b * WB};
        decode_block<1>(rd, p, f);
      }
#pragma unroll
      for (int i = 0; i < 4; i++) acc[k][i] = acc[k][i] + f[i];
    }
#pragma unroll
    for (int k = 0; k < U; k++) {
      if (D == 2) {
        cur[k] = nx1[k];
        nx1[k] = nxt[k];
      } else {
        cur[k] = nxt[k];
      }
    }
  }
  mean_scale<U * 4>(&acc[0][0], nstreams);
  float* out = (float*)F.data;
#pragma unroll
  for (int k = 0; k < U; k++) {
    const uint32_t b = b0 + 256u * k;
    if (b < nfull) {
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; i++) v[i] = acc[k][i];
      if (F.vec && F.dtype != DT_BF16) *(float4*)(out + 4 * (uint64_t)b) = make_float4(v[0], v[1], v[2], v[3]);
      else store_block1d(F, b, v);
    }
  }
}

// Block-index readers of the variable-rate decode_mean kernels: plain (one uint64 bit position per index chunk), or
// packed16 (GCOW_INDEX_PACKED16: one uint64 per 16 blocks -- low 48 bits the position of block 16 c, high 16 bits the
// offset of block 16 c + 8 from it -- read as the positions of 8-block chunks).
template <bool PK> struct IndexRd {
  const uint64_t* ix;
  __device__ __forceinline__ uint64_t operator[](uint64_t c) const { return ix[c]; }
};
template <> struct IndexRd<true> {
  const uint64_t* ix;
  __device__ __forceinline__ uint64_t operator[](uint64_t c) const
  {
    const uint64_t v = ix[c >> 1];
    return (v & 0xffffffffffffull) + ((c & 1) ? (v >> 48) : 0ull);
  }
};

// Variable rate (1-D closed-form domain), the lean decoder's shape (k_decode1d_var_lean): LANES 16-block chunks per
// workgroup; for each stream in rank order its span is staged in LDS (in 1, 2 or 4 parts, as there) and each lane
// decodes its chunk into 64 registers of sums; the means leave through the 8 x 8 lane transposes as whole-line
// stores. Complete workgroups only (whole chunks, full blocks, contiguous output); the launcher sends the rest to
// k_decode_mean1d_var.
template <uint32_t LANES, uint32_t CAPB, uint32_t CH, bool PK = false>
__global__ __launch_bounds__(LANES) __attribute__((amdgpu_waves_per_eu(CH == 8 ? GCOW_DMV8_WAVES : GCOW_DMV_WAVES, 8))) void k_decode_mean1d_var_lean(FieldDesc F, Params p,
                                                                  const uint64_t* __restrict__ in,
                                                                  uint64_t stream_words,
                                                                  const uint64_t* __restrict__ index,
                                                                  uint64_t index_words, uint64_t nchunks,
                                                                  uint32_t nstreams)
{
#pragma clang fp contract(off)
  constexpr uint32_t CAP = LANES * CH * CAPB / 64;
  static_assert(LANES % 32 == 0 && CAP >= 32 * CH * 140 / 64 + 4 && CH % 8 == 0, "a quarter workgroup's longest span must fit");
  // the DecTabLP image: the group phase through the 16-bit pair table (8-block chunks 3.04 -> 2.93 ms,
  // profiles/r05_dmean_lean_pair_ab.log; 16-block chunks at 3 waves 3.67 -> 3.58 ms, profiles/r05_dmean16_lp_w3_ab.log)
  __shared__ __attribute__((aligned(16))) uint16_t dtab[3 * 1024 + 5 * 128];
  const uint16_t* dt7 = dtab + 3 * 1024;
  __shared__ __attribute__((aligned(16))) uint64_t sw[CAP + 4];
  const uint32_t tid = threadIdx.x;
  const uint64_t c0 = (uint64_t)blockIdx.x * LANES;
  const uint64_t c = c0 + tid;
  const uint32_t* sw32 = (const uint32_t*)sw;
  const int cexp = 4 - p.minexp, maxprec = (int)min(p.maxprec, 64u);
  stage_lds16<LANES, sizeof(DecTabLP) / 16>(dtab, &g_dec_lean_pair, sizeof(DecTabLP));
  float acc[CH][4];
#pragma unroll
  for (int k = 0; k < (int)CH; k++) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0f;
  for (uint32_t r = 0; r < nstreams; r++) {
    const uint64_t* sr = in + (uint64_t)r * stream_words;
    const IndexRd<PK> ix{index + (uint64_t)r * index_words};
    const uint64_t sbase = (uint64_t)r * stream_words;
    // a span starts on a 16-byte boundary of the whole buffer (streams are stream_words apart, which may be odd):
    // w0 may be one word before this stream's first word (the previous stream's last word, never decoded)
    auto w_first = [&](uint64_t a) { return (int64_t)((sbase + (ix[a] >> 6)) & ~1ull) - (int64_t)sbase; };
    auto w_end = [&](uint64_t b) { return (int64_t)min<uint64_t>(b < nchunks ? (ix[b] + 63) >> 6 : stream_words, stream_words); };
    const uint64_t mine = ix[c];
    uint32_t P = 4;
    if (w_end(c0 + LANES) - w_first(c0) <= (int64_t)CAP) P = 1;
    else if (w_end(c0 + LANES / 2) - w_first(c0) <= (int64_t)CAP && w_end(c0 + LANES) - w_first(c0 + LANES / 2) <= (int64_t)CAP)
      P = 2;
    const uint32_t per = LANES / P;
    for (uint32_t part = 0; part < P; part++) {
      const uint64_t a = c0 + part * per;
      const int64_t w0 = w_first(a);
      const uint64_t span = (uint64_t)(w_end(a + per) - w0);
      __syncthreads();  // the previous span is no longer read
      stage_lds16<LANES, (CAP + 4) / 2>(sw, sr + w0, (uint32_t)(8 * span));
      __syncthreads();
      if (tid / per != part) continue;
      uint32_t pos = (uint32_t)((int64_t)mine - 64 * w0);
#pragma unroll
      for (int k = 0; k < (int)CH; k++) {
        const uint32_t start = pos;
        float f[4];
        if (!dec_block1d_lean<true>(sw32, pos, dtab, cexp, maxprec, f)) {
          uint64_t p64 = start;
          decode_block1d_var(LdsWindow{sw}, p64, dt7, p.minexp, p.maxprec, f);
          pos = (uint32_t)p64;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) acc[k][i] = acc[k][i] + f[i];
      }
    }
  }
  // CH = 8: the mean through mean_scale (a power-of-two world: the exact reciprocal; 2.94 -> 2.89 ms,
  // profiles/r05_dmean8_scale_ab.log). CH = 16: a plain division (the two-path mean_scale costs that kernel
  // registers, +4 %)
  if constexpr (CH == 8) mean_scale<CH * 4>(&acc[0][0], nstreams);
  const float nf = CH == 8 ? 1.0f : (float)nstreams;
  const uint32_t lane = tid & 63u, m = lane & 7u;
  float4* o4 = (float4*)F.data + (c - m) * CH + m;
  uint2* o2 = (uint2*)F.data + (c - m) * CH + m;  // bf16 output: 8 bytes per block, a chunk is one 128-byte line
  const bool bf = F.dtype == DT_BF16;
#pragma unroll
  for (int rnd = 0; rnd < (int)CH / 8; rnd++) {
    float g[8][4];
#pragma unroll
    for (int k = 0; k < 8; k++)
#pragma unroll
      for (int i = 0; i < 4; i++) g[k][i] = acc[8 * rnd + k][i] / nf;
    xpose8_stage<1>(g, lane);
    xpose8_stage<2>(g, lane);
    xpose8_stage<4>(g, lane);
    if (bf) {
#pragma unroll
      for (int i = 0; i < 8; i++)
        o2[CH * i + 8 * rnd] = make_uint2(bf16x2_rne(g[i][0], g[i][1]), bf16x2_rne(g[i][2], g[i][3]));
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++) o4[CH * i + 8 * rnd] = make_float4(g[i][0], g[i][1], g[i][2], g[i][3]);
    }
  }
}

// Variable rate (1-D closed-form domain) with each stream's block index every 16 blocks (index_words entries apart):
// the shape of k_decode1d_var_lean -- LANES chunks of 16 blocks per workgroup, the workgroup's span of each stream
// staged in LDS in turn -- with the 16 blocks' 64 values accumulated in registers across the streams and stored once.
template <uint32_t LANES, uint32_t CH, bool PK = false>
__global__ __launch_bounds__(LANES) void k_decode_mean1d_var(FieldDesc F, Params p, const uint64_t* __restrict__ in,
                                                             uint64_t stream_words, const uint64_t* __restrict__ index,
                                                             uint64_t index_words, uint64_t nchunks, uint32_t nstreams,
                                                             uint64_t cfirst)
{
#pragma clang fp contract(off)
  constexpr uint32_t CAP = LANES * CH * 80 / 64;
  __shared__ __attribute__((aligned(16))) uint16_t dt7[5 * 128];
  __shared__ __attribute__((aligned(16))) uint64_t sw[CAP + 4];
  const uint32_t tid = threadIdx.x;
  stage_lds16<LANES, sizeof(DecTab7) / 16>(dt7, &g_dec_tab7, sizeof(DecTab7));
  const uint64_t c0 = cfirst + (uint64_t)blockIdx.x * LANES;
  const uint64_t c = c0 + tid;
  const uint64_t b0 = c * CH, b1 = min<uint64_t>(b0 + CH, F.nblocks);
  float acc[CH][4];
#pragma unroll
  for (int k = 0; k < (int)CH; k++) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0f;
  for (uint32_t r = 0; r < nstreams; r++) {
    const uint64_t* sr = in + (uint64_t)r * stream_words;
    const IndexRd<PK> ix{index + (uint64_t)r * index_words};
    // the staged span starts on a 16-byte boundary of the whole buffer (streams are stream_words apart, which may be
    // odd): w0 may be one word before this stream's first word (the previous stream's last word, never decoded)
    const uint64_t sbase = (uint64_t)r * stream_words;
    const int64_t w0 = (int64_t)((sbase + (ix[c0] >> 6)) & ~1ull) - (int64_t)sbase;
    const uint64_t wend = c0 + LANES < nchunks ? ((ix[c0 + LANES] + 63) >> 6) : stream_words;
    const uint64_t span = (uint64_t)((int64_t)min<uint64_t>(wend, stream_words) - w0);
    const bool staged = span <= CAP;
    __syncthreads();  // the previous stream's span is no longer read
    if (staged) stage_lds16<LANES, (CAP + 4) / 2>(sw, sr + w0, (uint32_t)(8 * span));
    __syncthreads();
    if (c >= nchunks) continue;
    uint64_t pos = ix[c];
    auto run = [&](const auto& win) {
#pragma unroll
      for (int k = 0; k < (int)CH; k++) {
        if (b0 + k < b1) {
          float f[4];
          decode_block1d_var(win, pos, dt7, p.minexp, p.maxprec, f);
#pragma unroll
          for (int i = 0; i < 4; i++) acc[k][i] = acc[k][i] + f[i];
        }
      }
    };
    if (staged) {
      pos = (uint64_t)((int64_t)pos - 64 * w0);
      run(LdsWindow{sw});
    } else {
      run(GlobalWindow{sr});
    }
  }
  if (c >= nchunks) return;
  mean_scale<CH * 4>(&acc[0][0], nstreams);
  float* out = (float*)F.data;
#pragma unroll
  for (int k = 0; k < (int)CH; k++) {
    const uint64_t b = b0 + k;
    if (b < b1) {
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; i++) v[i] = acc[k][i];
      if (F.vec && F.dtype != DT_BF16 && 4 * b + 4 <= F.n[0]) *(float4*)(out + 4 * b) = make_float4(v[0], v[1], v[2], v[3]);
      else store_block1d(F, b, v);
    }
  }
}

// Variable rate outside the closed-form domain (expert parameters with minbits > 1 or maxbits < 160: a budget can
// truncate blocks): one lane per 16-block index chunk, the generic libzfp decoder (decode_block) on each stream in
// rank order, the same fp32 accumulation as above.
template <bool PK = false>
__global__ __launch_bounds__(256) void k_decode_mean1d_generic(FieldDesc F, Params p, const uint64_t* __restrict__ in,
                                                               uint64_t stream_words, const uint64_t* __restrict__ index,
                                                               uint64_t index_words, uint64_t nchunks,
                                                               uint32_t nstreams, uint32_t chunk)
{
#pragma clang fp contract(off)
  const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (c >= nchunks) return;
  const uint64_t b0 = c * chunk, b1 = min<uint64_t>(b0 + chunk, F.nblocks);  // chunk <= 16
  float acc[16][4];
#pragma unroll
  for (int k = 0; k < 16; k++) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0f;
  for (uint32_t r = 0; r < nstreams; r++) {
    BitReader rd{in + (uint64_t)r * stream_words, IndexRd<PK>{index + (uint64_t)r * index_words}[c]};
#pragma unroll
    for (int k = 0; k < 16; k++) {
      if (b0 + k < b1) {
        float f[4];
        decode_block<1>(rd, p, f);
#pragma unroll
        for (int i = 0; i < 4; i++) acc[k][i] = acc[k][i] + f[i];
      }
    }
  }
  mean_scale<64>(&acc[0][0], nstreams);
#pragma unroll
  for (int k = 0; k < 16; k++) {
    if (b0 + k < b1) {
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; i++) v[i] = acc[k][i];
      store_block1d(F, b0 + k, v);
    }
  }
}

// ------------------------------------------------------------------------------------------------ launchers
static inline hipStream_t S(void* s) { return (hipStream_t)s; }

hipError_t launch_decode_mean1d(const FieldDesc& F, const Params& p, const uint64_t* in, uint64_t stream_words,
                                uint32_t nstreams, const uint64_t* index, uint64_t index_words, void* stream,
                                uint32_t chunk)
{
  if (!F.nblocks) return hipSuccess;
  hipStream_t st = S(stream);
  if (p.minbits == p.maxbits) {
    const bool lean = p.maxprec >= 32 && p.minexp <= -154 && (p.maxbits == 64 || p.maxbits == 32);
    const uint32_t nfull = (uint32_t)(F.n[0] / 4);
    uint64_t done = 0;
    // whole-word blocks: the one-shot grid, GCOW_DMEAN_U blocks per lane (one block per lane through
    // k_decode_mean_fixed1d: 2.69 ms against 2.33 ms, W = 8 rate 16; profiles/r04_vdec_dmean_baseline.log,
    // profiles/r04_decode_mean_blocks_per_lane.log)
    if (lean && nfull && F.nblocks < (1u << 27)) {
      constexpr int U = GCOW_DMEAN_U, D = GCOW_DMEAN_D;
      const uint32_t g = (nfull + 256 * U - 1) / (256 * U);
      if (p.maxbits == 64) k_decode_mean_fixed1d_np<64, U, D><<<g, 256, 0, st>>>(F, p, in, stream_words, nstreams, nfull);
      else k_decode_mean_fixed1d_np<32, U, D><<<g, 256, 0, st>>>(F, p, in, stream_words, nstreams, nfull);
      done = nfull;
    }
    const uint64_t rest = F.nblocks - done;
    if (rest) {
      const uint32_t g = (uint32_t)((rest + 255) / 256);
      if (p.maxprec >= 32 && p.minexp <= -154 && p.maxbits == 64)
        k_decode_mean_fixed1d<64><<<g, 256, 0, st>>>(F, p, in, stream_words, nstreams, done);
      else if (p.maxprec >= 32 && p.minexp <= -154 && p.maxbits == 32)
        k_decode_mean_fixed1d<32><<<g, 256, 0, st>>>(F, p, in, stream_words, nstreams, done);
      else k_decode_mean_fixed1d<0><<<g, 256, 0, st>>>(F, p, in, stream_words, nstreams, done);
    }
    return hipGetLastError();
  }
  // variable rate: one lane per index chunk of `chunk` blocks (the streams' index stride, 8 or 16; the packed16
  // index is read as 8-block chunks)
  const bool pk = chunk == kIndexPacked16;
  if (pk) chunk = 8;
  if (chunk != 8 && chunk != 16) return hipErrorInvalidValue;
  const uint64_t nchunks = (F.nblocks + chunk - 1) / chunk;
  if (!(p.minbits <= 1 && p.maxbits >= 160)) {  // a budget can truncate blocks: generic decoder
    const uint32_t g = (uint32_t)((nchunks + 255) / 256);
    if (pk) k_decode_mean1d_generic<true><<<g, 256, 0, st>>>(F, p, in, stream_words, index, index_words, nchunks,
                                                             nstreams, chunk);
    else k_decode_mean1d_generic<false><<<g, 256, 0, st>>>(F, p, in, stream_words, index, index_words, nchunks,
                                                           nstreams, chunk);
    return hipGetLastError();
  }
  // complete workgroups (128 whole chunks of full blocks, contiguous output) by the lean kernel, the rest by the
  // general one
  uint64_t nlean = 0;
  if (F.vec) {
    const uint64_t fullchunks = (F.n[0] / 4) / chunk;
    nlean = std::min<uint64_t>(fullchunks, nchunks) / 128;
    if (nlean) {
      if (pk)
        k_decode_mean1d_var_lean<128, 64, 8, true><<<(uint32_t)nlean, 128, 0, st>>>(F, p, in, stream_words, index,
                                                                                    index_words, nchunks, nstreams);
      else if (chunk == 8)
        k_decode_mean1d_var_lean<128, 64, 8><<<(uint32_t)nlean, 128, 0, st>>>(F, p, in, stream_words, index,
                                                                              index_words, nchunks, nstreams);
      else
        k_decode_mean1d_var_lean<128, 64, 16><<<(uint32_t)nlean, 128, 0, st>>>(F, p, in, stream_words, index,
                                                                               index_words, nchunks, nstreams);
    }
  }
  const uint64_t cfirst = nlean * 128;
  if (cfirst < nchunks) {
    const uint32_t g = (uint32_t)((nchunks - cfirst + 127) / 128);
    if (pk)
      k_decode_mean1d_var<128, 8, true><<<g, 128, 0, st>>>(F, p, in, stream_words, index, index_words, nchunks,
                                                           nstreams, cfirst);
    else if (chunk == 8)
      k_decode_mean1d_var<128, 8><<<g, 128, 0, st>>>(F, p, in, stream_words, index, index_words, nchunks, nstreams,
                                                     cfirst);
    else
      k_decode_mean1d_var<128, 16><<<g, 128, 0, st>>>(F, p, in, stream_words, index, index_words, nchunks, nstreams,
                                                      cfirst);
  }
  return hipGetLastError();
}

}  // namespace gcow
