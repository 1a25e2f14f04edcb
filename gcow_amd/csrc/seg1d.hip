// seg1d.hip -- the segmented 1-D variable-rate codec (include/gcow.h "Segmented fields"): one
// contiguous buffer cut into S tensors, every tensor a field of its own (its blocks counted from its first value, its
// last block padded, no block across a seam) under expert(1, 16658, maxprec, clamp(minexp_s, -154, 133)), the words
// read on the device. The stream is the tensors' streams concatenated bit by bit, i.e. what a chain of S
// gcow_encode_device_append calls leaves, in a number of launches that does not depend on S.
//
// Blocks are numbered through the list (virtual blocks; empty tensors have none). The plan (gcow_seg_plan,
// gcow_api.cpp; kernels.h Seg*) holds, for the non-empty tensors in list order, their first virtual block, first value
// and number in the caller's list, and per tile of V1TILE virtual blocks the tensor of its first block and whether the
// whole tile is whole blocks of that one tensor: a lane bisects over the tensors of its own tile only, then walks.
//
// The encoder is the tile form of var1d.hip over virtual blocks (count -> launch_scan_ranges -> coder -> oversized
// tiles, the V1Workspace layout), with v1_prep / v1_code / count_block / encode_block / v1_tile_store as they are. What
// differs is the load and the parameter set, both per block, so the bodies of v1_count_tile and v1_tile_code are
// repeated here with those two made per block instead of shared (sharing would change the existing kernels' code).
// Every load is a plain, compiler-visible load: a lane's number of loads depends on the data in mixed tiles, so no
// wait is counted by hand in this unit.
//
// The decode-mean is k_decode_mean1d_var's shape (decode_mean.hip): one lane per index chunk of 8 or 16 virtual
// blocks, each stream's span staged in LDS in turn (a span above the stage is read from global memory), fp32 sums in
// registers in rank order, mean_scale, then each block's row to its tensor's place.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "codec_device.h"
#include "dec1d.h"
#include "field_io.h"
#include "kernels.h"
#include "mean1d.h"
#include "seg1d.h"
#include "tiles.h"
#include "var1d_prep.h"
#include "var1d_tile.h"

namespace gcow {

template <int DT>
__global__ __launch_bounds__(V1T) void k_seg_count(SegPlanDev P, const void* __restrict__ in, uint32_t maxprec,
                                                   const int32_t* __restrict__ mx, uint32_t stride,
                                                   uint64_t* __restrict__ sums, uint32_t* __restrict__ lens8,
                                                   uint32_t* __restrict__ nover, uint64_t* __restrict__ gsums)
{
  __shared__ uint32_t red[V1CT][V1T / 64];
  const uint32_t tid = threadIdx.x, t0 = blockIdx.x * V1CT;
  if (blockIdx.x == 0 && tid == 0) *nover = 0u;  // the oversized-tile list of k_seg_encode starts empty
  for (uint32_t i = 0; i < V1CT; i++) {
    uint32_t lsum = 0;
    if (t0 + i < P.ntiles) {
      SegLane<DT> L;
      L.load(P, in, mx, stride, t0 + i);
      lens8[(size_t)(t0 + i) * V1T + tid] = seg_count_tile<DT>(L, maxprec, lsum);
    }
    lsum = wave_sum_dpp(lsum);
    if ((tid & 63u) == 0) red[i][tid >> 6] = lsum;
  }
  __syncthreads();
  if (tid < 64) {  // wave 0: the tile totals, and their sum for the scan's group totals
    uint64_t tot = 0;
    if (tid < V1CT && t0 + tid < P.ntiles) {
#pragma unroll
      for (uint32_t w = 0; w < V1T / 64; w++) tot += red[tid][w];
      sums[t0 + tid] = tot;
    }
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) {
      const uint32_t lo = __shfl_xor((uint32_t)tot, o, 64), hi = __shfl_xor((uint32_t)(tot >> 32), o, 64);
      tot += (uint64_t)lo | ((uint64_t)hi << 32);
    }
    if (tid == 0) gsums[blockIdx.x] = tot;
  }
}

// The coder. BIG false: one tile per workgroup, the small window; a tile that needs more is listed (over[0] = count)
// and nothing of it is stored. BIG true: a grid-stride loop over that list with the worst-case window.
template <int DT, bool BIG>
__global__ __launch_bounds__(V1T) void k_seg_encode(SegPlanDev P, const void* __restrict__ in, uint32_t maxprec,
                                                    const int32_t* __restrict__ mx, uint32_t stride,
                                                    const uint64_t* __restrict__ rbase,
                                                    const uint32_t* __restrict__ lens8, uint32_t* __restrict__ out32,
                                                    uint64_t* __restrict__ index, uint32_t index_shift,
                                                    uint32_t* __restrict__ over)
{
  if constexpr (!BIG) {
    const uint32_t t = blockIdx.x;
    SegLane<DT> L;
    L.load(P, in, mx, stride, t);
    const uint32_t lw = lens8[(size_t)t * V1T + threadIdx.x];
    const V1Lds S = v1_lds<V1QS>();
    const uint64_t B = rbase[t];
    const uint32_t total = (uint32_t)(rbase[t + 1] - B);
    if (v1_tile_qwords(B, total) > V1QS) {
      if (threadIdx.x == 0) over[1 + atomicAdd(over, 1u)] = t;
      return;
    }
    seg_tile_code<DT>(L, maxprec, t, B, lw, index, index_shift, S.tab, S.rs, S.win, S.scan_sh, S.s_special);
    v1_tile_store(t, B, total, S.win, out32, P.ntiles);
  } else {
    const uint32_t n = over[0];
    if (blockIdx.x >= n) return;
    const V1Lds S = v1_lds<V1Q + 2>();
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
      const uint32_t t = over[1 + i];
      const uint64_t B = rbase[t];
      const uint32_t total = (uint32_t)(rbase[t + 1] - B);
      SegLane<DT> L;
      L.load(P, in, mx, stride, t);
      const uint32_t lw = lens8[(size_t)t * V1T + threadIdx.x];
      seg_tile_code<DT>(L, maxprec, t, B, lw, index, index_shift, S.tab, S.rs, S.win, S.scan_sh, S.s_special);
      v1_tile_store(t, B, total, S.win, out32, P.ntiles);
      __syncthreads();  // the window and scan slots are reused by the next tile
    }
  }
}

size_t seg1d_workspace_bytes(uint64_t nvb) { return V1Workspace(nvb).words * 8; }

template <int DT>
static hipError_t seg_launch_encode(const SegPlanDev& P, const void* in, uint32_t maxprec, const int32_t* mx,
                                    uint32_t stride, uint32_t* out32, uint64_t* ws, uint64_t* d_total, uint64_t* index,
                                    uint32_t index_shift, hipStream_t st)
{
  const V1Workspace W(P.nvb);
  const uint32_t ntiles = W.ntiles, ncw = (ntiles + V1CT - 1) / V1CT;
  uint64_t *sums = ws, *base = ws + W.o_base, *gsums = ws + W.o_gsums;
  uint32_t *over = (uint32_t*)(ws + W.o_over), *lens8 = (uint32_t*)(ws + W.o_lens8);
  k_seg_count<DT><<<ncw, V1T, 0, st>>>(P, in, maxprec, mx, stride, sums, lens8, over, gsums);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_scan_ranges(sums, ntiles, base, d_total, out32, nullptr, st, gsums);
  if (e != hipSuccess) return e;
  const uint32_t nbig = std::min(ntiles, 1280u);  // grid-stride workgroups of the oversized-tile pass (5 per CU)
  k_seg_encode<DT, false><<<ntiles, V1T, 0, st>>>(P, in, maxprec, mx, stride, base, lens8, out32, index, index_shift,
                                                  over);
  k_seg_encode<DT, true><<<nbig, V1T, 0, st>>>(P, in, maxprec, mx, stride, base, lens8, out32, index, index_shift,
                                               over);
  return hipGetLastError();
}

hipError_t launch_encode_seg1d(const SegHeader& H, const void* d_plan, const void* in, uint32_t maxprec,
                               const int32_t* d_minexp, uint32_t stride_words, uint32_t* out32, uint64_t* ws,
                               uint64_t* d_total, uint64_t* index, uint32_t index_shift, void* stream)
{
  hipStream_t st = (hipStream_t)stream;
  if (!H.nvb) return d_total ? launch_set_u64(d_total, 0, stream) : hipSuccess;
  const SegPlanDev P = seg_plan_dev(H, d_plan);
  if (H.dtype == DT_BF16)
    return seg_launch_encode<DT_BF16>(P, in, maxprec, d_minexp, stride_words, out32, ws, d_total, index, index_shift, st);
  return seg_launch_encode<DT_F32>(P, in, maxprec, d_minexp, stride_words, out32, ws, d_total, index, index_shift, st);
}

// ------------------------------------------------------------------------------------------------ decode + mean
// One lane per index chunk of CH virtual blocks (CH divides V1TILE, so a chunk lies in one tile of the plan). For each
// stream in rank order the workgroup's span is staged in LDS (w0 on a 16-byte boundary of the whole buffer, as in
// k_decode_mean1d_var; a span above the stage -- streams near 140 bits per block -- is read from global memory) and
// the lane decodes its blocks in sequence, each under its tensor's word of that stream's set. The means go to
// out + off_s + 4 (v - vb0_s): a whole row at a 16-byte (bf16: 8-byte) aligned address as one store, else the tensor's
// real values one by one.
template <uint32_t LANES, uint32_t CH, int DT>
__global__ __launch_bounds__(LANES) void k_seg_decode_mean(SegPlanDev P, uint32_t maxprec,
                                                           const int32_t* __restrict__ mx, uint32_t stride,
                                                           uint64_t stream_stride, const uint64_t* __restrict__ in,
                                                           uint64_t stream_words, const uint64_t* __restrict__ index,
                                                           uint64_t index_words, uint64_t nchunks, uint32_t nstreams,
                                                           void* __restrict__ out)
{
#pragma clang fp contract(off)
  static_assert(V1TILE % CH == 0, "a chunk lies in one tile");
  constexpr uint32_t CAP = LANES * CH * 80 / 64;
  __shared__ __attribute__((aligned(16))) uint16_t dt7[5 * 128];
  __shared__ __attribute__((aligned(16))) uint64_t sw[CAP + 4];
  const uint32_t tid = threadIdx.x;
  stage_lds16<LANES, sizeof(DecTab7) / 16>(dt7, &g_dec_tab7, sizeof(DecTab7));
  const uint64_t c0 = (uint64_t)blockIdx.x * LANES;
  const uint64_t c = c0 + tid;
  const uint64_t b0 = c * CH, b1 = min<uint64_t>(b0 + CH, P.nvb);
  const bool live = c < nchunks;
  SegWalk W0;
  W0.li = 0;
  W0.e = W0.nx = SegEnt{0, 0, 0};
  if (live) W0.start(P, seg_locate(P, (uint32_t)(b0 / V1TILE), b0));
  float acc[CH][4];
#pragma unroll
  for (int k = 0; k < (int)CH; k++) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0f;
  for (uint32_t r = 0; r < nstreams; r++) {
    const uint64_t* sr = in + (uint64_t)r * stream_words;
    const uint64_t* ix = index + (uint64_t)r * index_words;
    const int32_t* mr = mx + (uint64_t)r * stream_stride;
    const uint64_t sbase = (uint64_t)r * stream_words;
    const int64_t w0 = (int64_t)((sbase + (ix[c0] >> 6)) & ~1ull) - (int64_t)sbase;
    const uint64_t wend = c0 + LANES < nchunks ? ((ix[c0 + LANES] + 63) >> 6) : stream_words;
    const uint64_t span = (uint64_t)((int64_t)min<uint64_t>(wend, stream_words) - w0);
    const bool staged = span <= CAP;
    __syncthreads();  // the previous stream's span is no longer read
    if (staged) stage_lds16<LANES, (CAP + 4) / 2>(sw, sr + w0, (uint32_t)(8 * span));
    __syncthreads();
    if (!live) continue;
    uint64_t pos = ix[c];
    auto run = [&](const auto& win) {
      SegWalk W = W0;
      int m = seg_clamp(mr[(uint64_t)W.e.seg * stride]);
#pragma unroll
      for (int k = 0; k < (int)CH; k++) {
        if (b0 + k < b1) {
          if (W.advance(P, b0 + k)) m = seg_clamp(mr[(uint64_t)W.e.seg * stride]);
          float f[4];
          decode_block1d_var(win, pos, dt7, m, maxprec, f);
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
  if (!live) return;
  mean_scale<CH * 4>(&acc[0][0], nstreams);
  SegWalk W = W0;
#pragma unroll
  for (int k = 0; k < (int)CH; k++) {
    const uint64_t v = b0 + k;
    if (v < b1) {
      W.advance(P, v);
      const uint64_t x0 = W.first(v);
      const uint32_t nv = W.nreal(v);
      if constexpr (DT == DT_BF16) {
        uint16_t* o = (uint16_t*)out + x0;
        if (nv == 4 && ((uintptr_t)o & 7u) == 0) {
          *(uint2*)o = make_uint2(bf16x2_rne(acc[k][0], acc[k][1]), bf16x2_rne(acc[k][2], acc[k][3]));
        } else {
#pragma unroll
          for (uint32_t i = 0; i < 4; i++)
            if (i < nv) o[i] = (uint16_t)bf16_rne(acc[k][i]);
        }
      } else {
        float* o = (float*)out + x0;
        if (nv == 4 && ((uintptr_t)o & 15u) == 0) {
          *(float4*)o = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
        } else {
#pragma unroll
          for (uint32_t i = 0; i < 4; i++)
            if (i < nv) o[i] = acc[k][i];
        }
      }
    }
  }
}

hipError_t launch_decode_mean_seg1d(const SegHeader& H, const void* d_plan, uint32_t maxprec, const int32_t* d_minexp,
                                    uint32_t stride_words, uint64_t stream_stride_words, const uint64_t* in,
                                    uint64_t stream_words, uint32_t nstreams, const uint64_t* index,
                                    uint64_t index_words, uint32_t chunk, void* out, int out_dtype, void* stream)
{
  if (!H.nvb) return hipSuccess;
  if (chunk != 8 && chunk != 16) return hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const SegPlanDev P = seg_plan_dev(H, d_plan);
  const uint64_t nchunks = (H.nvb + chunk - 1) / chunk;
  const uint32_t g = (uint32_t)((nchunks + 127) / 128);
  const bool bf = out_dtype == DT_BF16;
#define GCOW_SEG_DM(CHV, DTV)                                                                                       \
  k_seg_decode_mean<128, CHV, DTV><<<g, 128, 0, st>>>(P, maxprec, d_minexp, stride_words, stream_stride_words, in,  \
                                                      stream_words, index, index_words, nchunks, nstreams, out)
  if (chunk == 8) {
    if (bf) GCOW_SEG_DM(8, DT_BF16);
    else GCOW_SEG_DM(8, DT_F32);
  } else {
    if (bf) GCOW_SEG_DM(16, DT_BF16);
    else GCOW_SEG_DM(16, DT_F32);
  }
#undef GCOW_SEG_DM
  return hipGetLastError();
}

}  // namespace gcow
