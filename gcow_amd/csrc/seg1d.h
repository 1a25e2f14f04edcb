// seg1d.h -- the plan walk, the lane load and the tile bodies of the segmented 1-D codec, shared by
// the encoder and decode-mean over a buffer's own values (seg1d.hip) and the residual form over y = x + e and its rate
// tables (seg_resid1d.hip). The text is seg1d.hip's, moved here unchanged (every kernel of seg1d.hip
// compiles to the instructions it had: profiles/r19_segr_seg1d_isa_diff.log).
// Two bodies here have a hand-kept copy in seg_resid1d.hip: seg_tile_code (segr_tile_code there, with a per-block hook)
// and seg1d.hip's k_seg_count (k_segr_count there). A change to either goes into its copy as well; DESIGN.md 5.16 has
// why they are copies.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "codec_device.h"
#include "field_io.h"
#include "kernels.h"
#include "tiles.h"
#include "var1d_prep.h"
#include "var1d_tile.h"

namespace gcow {


static_assert(kSegTileBlocks == V1TILE, "the plan's tiles are the coder's");

struct SegPlanDev {
  const SegEnt* __restrict__ ents;     // nlive + 1 (the last one a sentinel)
  const uint32_t* __restrict__ tiles;  // ntiles
  uint32_t nlive, ntiles;
  uint64_t nvb;
};

static SegPlanDev seg_plan_dev(const SegHeader& H, const void* d_plan)
{
  const char* base = (const char*)d_plan;
  return SegPlanDev{(const SegEnt*)(base + H.off_ents), (const uint32_t*)(base + H.off_tiles), H.nlive, H.ntiles, H.nvb};
}

__device__ __forceinline__ int seg_clamp(int m) { return min(max(m, kFitMinExpLo), kFitMinExpHi); }

// The plan entry of virtual block v of tile t: the tile's first tensor when the tile is uniform, else the last tensor
// of the tile that starts at or before v.
__device__ __forceinline__ uint32_t seg_locate(const SegPlanDev& P, uint32_t t, uint64_t v)
{
  const uint32_t tw = P.tiles[t];
  uint32_t lo = tw & 0x7fffffffu;
  if (tw >> 31) return lo;
  uint32_t hi = t + 1 < P.ntiles ? (P.tiles[t + 1] & 0x7fffffffu) : P.nlive - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (P.ents[mid].vb0 <= v) lo = mid;
    else hi = mid - 1u;
  }
  return lo;
}

// A walk through the plan entries in step with rising virtual blocks
struct SegWalk {
  uint32_t li;
  SegEnt e, nx;
  __device__ __forceinline__ void start(const SegPlanDev& P, uint32_t i)
  {
    li = i;
    e = P.ents[i];
    nx = P.ents[i + 1];
  }
  // true when the entry changed; v < nvb, so the sentinel (vb0 = nvb) ends the loop
  __device__ __forceinline__ bool advance(const SegPlanDev& P, uint64_t v)
  {
    bool moved = false;
    while ((uint64_t)nx.vb0 <= v) {
      li++;
      e = nx;
      nx = P.ents[li + 1];
      moved = true;
    }
    return moved;
  }
  // block v's first value in the buffer, and its real values (1 .. 4)
  __device__ __forceinline__ uint64_t first(uint64_t v) const { return e.off + 4ull * (v - e.vb0); }
  __device__ __forceinline__ uint32_t nreal(uint64_t v) const
  {
    return (uint32_t)min<uint64_t>(4, nx.off - first(v));
  }
};

// The lane's V1U consecutive virtual blocks of tile t: values (bf16 widened exactly; a partial block padded as
// gather_block pads), the clamped minexp of each block's tensor, and which of them exist.
template <int DT>
struct SegLane {
  float f[V1U][4];
  int minexp[V1U];
  uint32_t valid;
  __device__ __forceinline__ void load(const SegPlanDev& P, const void* __restrict__ in,
                                       const int32_t* __restrict__ mx, uint32_t stride, uint32_t t)
  {
    const uint64_t v0 = (uint64_t)t * V1TILE + (uint64_t)threadIdx.x * V1U;
    valid = 0;
#pragma unroll
    for (uint32_t k = 0; k < V1U; k++) {
      f[k][0] = f[k][1] = f[k][2] = f[k][3] = 0.0f;
      minexp[k] = 0;
    }
    if (v0 >= P.nvb) return;
    SegWalk W;
    W.start(P, seg_locate(P, t, v0));
    int m = seg_clamp(mx[(uint64_t)W.e.seg * stride]);
#pragma unroll
    for (uint32_t k = 0; k < V1U; k++) {
      const uint64_t v = v0 + k;
      if (v >= P.nvb) continue;
      if (W.advance(P, v)) m = seg_clamp(mx[(uint64_t)W.e.seg * stride]);
      const uint64_t x0 = W.first(v);
      const uint32_t nv = W.nreal(v);
      const char* row = (const char*)in + x0 * (DT == DT_BF16 ? 2u : 4u);
      if (nv == 4 && ((uintptr_t)row & (DT == DT_BF16 ? 7u : 15u)) == 0) {
        load_row4<DT>(row, 0, f[k]);
      } else {
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) f[k][i] = load_elem<DT>(row, (int64_t)pad_index(i, nv));
      }
      minexp[k] = m;
      valid |= 1u << k;
    }
  }
};

// v1_count_tile with the parameter set per block
template <int DT>
__device__ __forceinline__ uint32_t seg_count_tile(const SegLane<DT>& L, uint32_t maxprec, uint32_t& lsum)
{
  const int mp = (int)min(maxprec, 64u);
  uint32_t pk = 0;
  lsum = 0;
#pragma unroll
  for (uint32_t k = 0; k < V1U; k++) {
    uint32_t u[4], hdr, K;
    bool inf;
    uint32_t len = v1_prep(L.f[k], -122 - L.minexp[k], mp, u, hdr, K, inf);
    const bool valid = (L.valid >> k) & 1u;
    if (inf && valid) len = count_block<1>(L.f[k], Params{1u, 16658u, maxprec, L.minexp[k]});
    len = valid ? len : 0u;  // <= 140
    pk |= len << (8 * k);
    lsum += len;
  }
  return pk;
}

// v1_tile_code with the parameter set per block: tile t (the lane's blocks L, their byte lengths lw) coded into the
// window `win` from bit B & 127; tab / rs already in LDS. Ends with the window complete and the index written.
template <int DT>
__device__ __forceinline__ void seg_tile_code(const SegLane<DT>& L, uint32_t maxprec, uint32_t t, uint64_t B,
                                              uint32_t lw, uint64_t* __restrict__ index, uint32_t index_shift,
                                              const uint32_t* tab, const uint32_t* rs, uint64_t* win,
                                              uint32_t* scan_sh, uint32_t* s_special)
{
  uint32_t* win32 = (uint32_t*)win;
  const uint32_t tid = threadIdx.x;
  const uint32_t lb = (uint32_t)(B & 127u);
  uint32_t len[V1U], lsum = 0;
#pragma unroll
  for (uint32_t k = 0; k < V1U; k++) {
    len[k] = (lw >> (8 * k)) & 255u;
    lsum += len[k];
  }
  uint32_t tot_unused;
  const uint32_t excl = lb + block_exclusive_scan<V1T, false>(lsum, &tot_unused, scan_sh);  // barrier below
  if (lsum) {  // the two words this lane shares with its neighbours start at zero
    win[excl >> 6] = 0ull;
    win[(excl + lsum - 1) >> 6] = 0ull;
  }
  if (tid == 0) *s_special = 0;
  __syncthreads();

  const int mp = (int)min(maxprec, 64u);
  uint64_t acc = 0;
  uint32_t q = excl >> 6, fill = excl & 63u;
  const uint32_t qhead = q;
  uint32_t spmask = 0;
#pragma unroll
  for (uint32_t k = 0; k < V1U; k++) {
    uint32_t u[4], hdr, K;
    bool inf;
    (void)v1_prep(L.f[k], -122 - L.minexp[k], mp, u, hdr, K, inf);  // the length comes from the count pass
    bool sp = inf && ((L.valid >> k) & 1u);
    uint64_t c0, c1;
    v1_code(u, hdr, len[k], K, tab, rs, c0, c1, sp);
    sp = sp && len[k];
    if (sp) c0 = c1 = 0ull;  // coded below by the generic coder, OR-ed into these zero bits
    spmask |= (uint32_t)sp << k;
    acc |= c0 << fill;
    const uint64_t mid = ((c0 >> 1) >> (63u - fill)) | (c1 << fill);
    const uint64_t hi = (c1 >> 1) >> (63u - fill);
    const uint32_t nf = fill + len[k];
    if (nf >= 64u) {
      if (q == qhead) atomicOr((unsigned long long*)&win[q], (unsigned long long)acc);
      else win[q] = acc;
      q++;
      acc = mid;
      if (nf >= 128u) {
        win[q] = acc;
        q++;
        acc = hi;
        if (nf >= 192u) {  // a special block of up to 140 bits (its code is zero here) completes a third word
          win[q] = acc;
          q++;
          acc = 0ull;
        }
      }
    }
    fill = nf & 63u;
    acc &= (1ull << fill) - 1ull;
  }
  if (fill) atomicOr((unsigned long long*)&win[q], (unsigned long long)acc);
  if (spmask) *s_special = 1u;
  __syncthreads();
  if (*s_special) {  // Inf / NaN blocks, long group phases, codes past 128 bits: the generic coder, the block's own set
    uint32_t o = excl;
#pragma unroll
    for (uint32_t k = 0; k < V1U; k++) {
      if ((spmask >> k) & 1u) {
        LdsWriter wr{win32, o, o + len[k]};
        encode_block<1>(wr, L.f[k], Params{1u, 16658u, maxprec, L.minexp[k]});
      }
      o += len[k];
    }
    __syncthreads();
  }
  if (index) {
    const uint64_t bl = (uint64_t)t * V1TILE + (uint64_t)tid * V1U;
    uint32_t o = excl;
#pragma unroll
    for (uint32_t k = 0; k < V1U; k++) {
      const uint64_t b = bl + k;
      if (len[k] && (b & ((1ull << index_shift) - 1ull)) == 0) index[b >> index_shift] = (B & ~127ull) + o;
      o += len[k];
    }
  }
}

}  // namespace gcow
