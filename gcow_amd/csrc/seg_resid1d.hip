// seg_resid1d.hip -- error feedback under per-tensor budgets (include/gcow.h "Segmented fields with a residual";
// DESIGN.md 5.16): the segmented encoder of seg1d.hip over y = x + e with e' = finite(y - decode) written to each
// tensor's place (gcow_encode_seg_residual_device), and the rate table of y per tensor from one pass over the plan's
// tiles (gcow_rate_table_seg_device). x is the bucket (fp32 or bf16), e an fp32 array parallel to it (or absent: zeros);
// y = fadd(widen(x), e) is formed in registers per value and never stored, and a partial block is padded from y.
//
// The plan, the walk and the per-block parameter sets are seg1d.h's; the launches are seg1d.hip's (count ->
// launch_scan_ranges -> coder -> oversized tiles, the V1Workspace layout), so stream, bit count and index are those of
// gcow_encode_seg_device for the fp32 array y.
//   lane load   the walk of SegLane::load; the x row and the e row of a block each move as one vector when the block is
//               whole and that array's own row address is aligned, else value by value with the encoder's padding
//               indices (the same for both, so a padding value of y is a copy of a real one). The place and the real
//               values of each row are kept for the store.
//   count       seg_count_tile on y; nothing is written to e_out.
//   coders      segr_tile_code: seg_tile_code's body with the per-block hook v1_tile_code has (var1d.hip) -- given that
//               hook, even one that compiles to nothing, the compiler emits other code for k_seg_encode
//               (profiles/r19_segr_hooked_isa_diff.log), so seg_tile_code stays as it is and its body is repeated here. The hook turns the u, hdr, K of the one
//               v1_prep per block into the residual row (v1_decode_closed, resid_bits), kept in the lane until the
//               window is stored; Inf / NaN blocks are redone by rt_block_generic under the block's own set. A row
//               goes to e_out + first(v) as one 16-byte store when the block is whole and that address aligned, else
//               its real values one by one: a partial last block never reaches the next tensor's values.
// e_in may be e_out: a lane reads the e rows of its own blocks, all of them, before its first store, and no other lane
// reads them. The first coder pass leaves a tile it lists as oversized before any store, window or rows; the second
// pass reads that tile's old e and writes its e'. Every load is a plain compiler-visible load (no wait is counted by
// hand, for seg1d.hip's reason), and the wide store is a plain vector store.
// The 4 x 4 quad transpose of V1ResidOut::store_quad is not built: rows leave one 16-byte store per block.
//
// The table pass, k_rate_table_seg: at most kRateTableRelMaxGrid workgroups, each a contiguous run of the plan's tiles
// (RT_TILE = V1TILE). A uniform tile updates the workgroup's two LDS histograms (RtLdsSink), which are flushed to the
// tensor's workspace slice and zeroed only when the run moves to another tensor; the blocks of a mixed tile go straight
// to their tensors' slices (RtGlobalSink), and the lane that holds a tensor's first block inside the tile adds the
// number of that tensor's blocks inside the tile to its count word, as rate_table_rel1d.hip counts gather pieces. The
// workspace is rate_table_rel1d.hip's (kRateTableRelWords per tensor, the caller's numbering), zeroed by a kernel in
// stream order; launch_rate_table_finish_batch turns it into the rows. Integer adds only.
//
// The maximum pass, k_seg_absmax (gcow_seg_rel_minexp_device): the table pass's runs and loads, with
// the largest finite |y| per tensor as the only result. |y| is taken as integer bits with Inf / NaN masked to 0
// (rel_mag), so an unsigned maximum is the maximum magnitude and a padding value, a copy of a real one, cannot change
// it. A uniform tile updates one register per lane, reduced over the workgroup into one atomicMax when the run moves
// to another tensor and at its end; the blocks of a mixed tile go to their tensors' slots, one atomic per wave where
// the lanes that have something share a tensor (k_rel_absmax's shortcut), else one per lane. A zero maximum issues no
// atomic: the slots are zeroed by k_seg_absmax_zero in stream order. k_seg_rel_words turns slot s into the word
// rel_minexp(a_s, rel_bits) (rel_minexp.h) at d_minexp[s * stride]. Integer maxima only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "codec_device.h"
#include "field_io.h"
#include "kernels.h"
#include "rate_table1d.h"
#include "rel_minexp.h"
#include "seg1d.h"
#include "tiles.h"
#include "var1d_prep.h"
#include "var1d_tile.h"

namespace gcow {

namespace {

static_assert(RT_TILE == V1TILE && RTT == V1T && RTU == V1U, "the plan's tiles serve the coder and the table pass");

// The lane's V1U consecutive virtual blocks of tile t of y = x + e. y: values, clamped words and existence as SegLane
// has them (mx null: no words are read, the table pass). x0 / nvs: each row's first value in the buffer and its real
// values (3 bits each), for the store. TAB: the block's tensor in the caller's numbering and, in the lane that holds
// the tensor's first block inside the tile, the number of the tensor's blocks inside the tile (else 0).
template <int DT, bool TAB>
struct SegYLane {
  SegLane<DT_F32> y;
  uint64_t x0[V1U];
  uint32_t nvs;
  uint32_t seg[V1U], cnt[V1U];
  __device__ __forceinline__ uint32_t nreal(uint32_t k) const { return (nvs >> (3 * k)) & 7u; }
  __device__ __forceinline__ void load(const SegPlanDev& P, const void* __restrict__ in, const float* e_in,
                                       const int32_t* __restrict__ mx, uint32_t stride, uint32_t t)
  {
    const uint64_t vt = (uint64_t)t * V1TILE, v0 = vt + (uint64_t)threadIdx.x * V1U;
    y.valid = 0;
    nvs = 0;
#pragma unroll
    for (uint32_t k = 0; k < V1U; k++) {
      y.f[k][0] = y.f[k][1] = y.f[k][2] = y.f[k][3] = 0.0f;
      y.minexp[k] = 0;
      x0[k] = 0;
      seg[k] = cnt[k] = 0;
    }
    if (v0 >= P.nvb) return;
    SegWalk W;
    W.start(P, seg_locate(P, t, v0));
    int m = mx ? seg_clamp(mx[(uint64_t)W.e.seg * stride]) : 0;
#pragma unroll
    for (uint32_t k = 0; k < V1U; k++) {
      const uint64_t v = v0 + k;
      if (v >= P.nvb) continue;
      if (W.advance(P, v) && mx) m = seg_clamp(mx[(uint64_t)W.e.seg * stride]);
      const uint64_t first = W.first(v);
      const uint32_t nv = W.nreal(v);
      float fx[4], fe[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      const char* row = (const char*)in + first * (DT == DT_BF16 ? 2u : 4u);
      if (nv == 4 && ((uintptr_t)row & (DT == DT_BF16 ? 7u : 15u)) == 0) {
        load_row4<DT>(row, 0, fx);
      } else {
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) fx[i] = load_elem<DT>(row, (int64_t)pad_index(i, nv));
      }
      if (e_in) {
        const float* er = e_in + first;
        if (nv == 4 && ((uintptr_t)er & 15u) == 0) {
          load_row4<DT_F32>(er, 0, fe);
        } else {
#pragma unroll
          for (uint32_t i = 0; i < 4; i++) fe[i] = er[pad_index(i, nv)];
        }
      }
#pragma unroll
      for (uint32_t i = 0; i < 4; i++) y.f[k][i] = __fadd_rn(fx[i], fe[i]);  // e absent: + 0, so -0 becomes +0
      y.minexp[k] = m;
      y.valid |= 1u << k;
      x0[k] = first;
      nvs |= nv << (3 * k);
      if constexpr (TAB) {
        seg[k] = W.e.seg;
        const uint64_t lo = max((uint64_t)W.e.vb0, vt), hi = min((uint64_t)W.nx.vb0, min(vt + V1TILE, P.nvb));
        cnt[k] = v == lo ? (uint32_t)(hi - lo) : 0u;
      }
    }
  }
};

// ------------------------------------------------------------------------------------------------------ the encoder
template <int DT>
__global__ __launch_bounds__(V1T) void k_segr_count(SegPlanDev P, const void* __restrict__ in, const float* e_in,
                                                    uint32_t maxprec, const int32_t* __restrict__ mx, uint32_t stride,
                                                    uint64_t* __restrict__ sums, uint32_t* __restrict__ lens8,
                                                    uint32_t* __restrict__ nover, uint64_t* __restrict__ gsums)
{
  __shared__ uint32_t red[V1CT][V1T / 64];
  const uint32_t tid = threadIdx.x, t0 = blockIdx.x * V1CT;
  if (blockIdx.x == 0 && tid == 0) *nover = 0u;  // the oversized-tile list of k_segr_encode starts empty
  for (uint32_t i = 0; i < V1CT; i++) {
    uint32_t lsum = 0;
    if (t0 + i < P.ntiles) {
      SegYLane<DT, false> L;
      L.load(P, in, e_in, mx, stride, t0 + i);
      lens8[(size_t)(t0 + i) * V1T + tid] = seg_count_tile<DT_F32>(L.y, maxprec, lsum);
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

// seg_tile_code with a per-block hook (the header has why the body is repeated): hook(k, f, u, hdr, K, inf) sees every
// block k of the lane once, with what the one v1_prep returned for it.
template <class Hook>
__device__ __forceinline__ void segr_tile_code(const SegLane<DT_F32>& L, uint32_t maxprec, uint32_t t, uint64_t B,
                                               uint32_t lw, uint64_t* __restrict__ index, uint32_t index_shift,
                                               const uint32_t* tab, const uint32_t* rs, uint64_t* win,
                                               uint32_t* scan_sh, uint32_t* s_special, const Hook& hook)
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
    hook(k, L.f[k], u, hdr, K, inf);
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

// resid_bits (var1d_prep.h) with the subtract under contract(off). The decode ends in scale * (float)q, and __fsub_rn
// is a plain `y - d` to the compiler: under the default -ffp-contract the multiply and the subtract may become one fma,
// which subtracts the unrounded product. Where the decode overflows to Inf (a finite value in the top binade under a
// coarse word) the residual would then be a finite -2^104 instead of the non-finite result that carries nothing
// forward. A subtract without the contract flag is not fused. resid_bits itself is shared with existing kernels and
// stays as it is here.
__device__ __forceinline__ uint32_t segr_resid_bits(float y, float d)
{
#pragma clang fp contract(off)
  const uint32_t r = __float_as_uint(y - d);
  return (r & 0x7f800000u) == 0x7f800000u ? 0u : r;
}

__device__ __forceinline__ uint4 segr_resid_row(const float* y, const float* d)
{
  return make_uint4(segr_resid_bits(y[0], d[0]), segr_resid_bits(y[1], d[1]), segr_resid_bits(y[2], d[2]),
                    segr_resid_bits(y[3], d[3]));
}

// The hook: the block's residual row from the coefficients the coder was given, kept in the lane until the tile is
// coded. Blocks with Inf / NaN (infmask) are redone by segr_tile.
struct SegResidHook {
  uint32_t& infmask;
  uint4 (&rows)[V1U];
  __device__ __forceinline__ void operator()(uint32_t k, const float* y, const uint32_t* u, uint32_t hdr, uint32_t K,
                                             bool inf) const
  {
    infmask |= (uint32_t)inf << k;
    float d[4];
    v1_decode_closed(u, hdr, K, d);
    rows[k] = segr_resid_row(y, d);
  }
};

// Code and store one tile of y, then its residual rows: row k to e_out + x0[k], whole and 16-byte aligned as one store,
// else its real values one by one.
template <int DT>
__device__ __forceinline__ void segr_tile(const SegYLane<DT, false>& L, float* e_out, uint32_t maxprec, uint32_t t,
                                          uint64_t B, uint32_t total, uint32_t lw, uint32_t* __restrict__ out32,
                                          uint64_t* __restrict__ index, uint32_t index_shift, uint32_t ntiles,
                                          const V1Lds& S)
{
  uint32_t infmask = 0;
  uint4 rows[V1U];
  segr_tile_code(L.y, maxprec, t, B, lw, index, index_shift, S.tab, S.rs, S.win, S.scan_sh, S.s_special,
                 SegResidHook{infmask, rows});
  v1_tile_store(t, B, total, S.win, out32, ntiles);
  infmask &= L.y.valid;
  if (infmask) {  // Inf / NaN present: the generic coder and decoder in the lane, the block's own set
#pragma unroll
    for (uint32_t k = 0; k < V1U; k++) {
      if ((infmask >> k) & 1u) {
        float d[4];
        (void)rt_block_generic(L.y.f[k], Params{1u, 16658u, maxprec, L.y.minexp[k]}, d);
        rows[k] = segr_resid_row(L.y.f[k], d);
      }
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < V1U; k++) {
    if (!((L.y.valid >> k) & 1u)) continue;
    uint32_t* o = (uint32_t*)e_out + L.x0[k];
    const uint32_t nv = L.nreal(k);
    if (nv == 4 && ((uintptr_t)o & 15u) == 0) {
      *(uint4*)o = rows[k];
    } else {
      o[0] = rows[k].x;
      if (nv > 1) o[1] = rows[k].y;
      if (nv > 2) o[2] = rows[k].z;
      if (nv > 3) o[3] = rows[k].w;
    }
  }
}

// The coder, k_seg_encode's shape. BIG false: one tile per workgroup, the small window; a tile that needs more is
// listed and nothing of it is stored, neither window nor rows. BIG true: a grid-stride loop over that list with the
// worst-case window; it reads the tile's e, which the first pass left as it was.
template <int DT, bool BIG>
__global__ __launch_bounds__(V1T) void k_segr_encode(SegPlanDev P, const void* __restrict__ in, const float* e_in,
                                                     float* e_out, uint32_t maxprec, const int32_t* __restrict__ mx,
                                                     uint32_t stride, const uint64_t* __restrict__ rbase,
                                                     const uint32_t* __restrict__ lens8, uint32_t* __restrict__ out32,
                                                     uint64_t* __restrict__ index, uint32_t index_shift,
                                                     uint32_t* __restrict__ over)
{
  if constexpr (!BIG) {
    const uint32_t t = blockIdx.x;
    SegYLane<DT, false> L;
    L.load(P, in, e_in, mx, stride, t);
    const uint32_t lw = lens8[(size_t)t * V1T + threadIdx.x];
    const V1Lds S = v1_lds<V1QS>();
    const uint64_t B = rbase[t];
    const uint32_t total = (uint32_t)(rbase[t + 1] - B);
    if (v1_tile_qwords(B, total) > V1QS) {
      if (threadIdx.x == 0) over[1 + atomicAdd(over, 1u)] = t;
      return;
    }
    segr_tile<DT>(L, e_out, maxprec, t, B, total, lw, out32, index, index_shift, P.ntiles, S);
  } else {
    const uint32_t n = over[0];
    if (blockIdx.x >= n) return;
    const V1Lds S = v1_lds<V1Q + 2>();
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
      const uint32_t t = over[1 + i];
      const uint64_t B = rbase[t];
      const uint32_t total = (uint32_t)(rbase[t + 1] - B);
      SegYLane<DT, false> L;
      L.load(P, in, e_in, mx, stride, t);
      const uint32_t lw = lens8[(size_t)t * V1T + threadIdx.x];
      segr_tile<DT>(L, e_out, maxprec, t, B, total, lw, out32, index, index_shift, P.ntiles, S);
      __syncthreads();  // the window and scan slots are reused by the next tile
    }
  }
}

template <int DT>
hipError_t segr_launch_encode(const SegPlanDev& P, const void* in, const float* e_in, float* e_out, uint32_t maxprec,
                              const int32_t* mx, uint32_t stride, uint32_t* out32, uint64_t* ws, uint64_t* d_total,
                              uint64_t* index, uint32_t index_shift, hipStream_t st)
{
  const V1Workspace W(P.nvb);
  const uint32_t ntiles = W.ntiles, ncw = (ntiles + V1CT - 1) / V1CT;
  uint64_t *sums = ws, *base = ws + W.o_base, *gsums = ws + W.o_gsums;
  uint32_t *over = (uint32_t*)(ws + W.o_over), *lens8 = (uint32_t*)(ws + W.o_lens8);
  k_segr_count<DT><<<ncw, V1T, 0, st>>>(P, in, e_in, maxprec, mx, stride, sums, lens8, over, gsums);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_scan_ranges(sums, ntiles, base, d_total, out32, nullptr, st, gsums);
  if (e != hipSuccess) return e;
  const uint32_t nbig = std::min(ntiles, 1280u);  // grid-stride workgroups of the oversized-tile pass (5 per CU)
  k_segr_encode<DT, false><<<ntiles, V1T, 0, st>>>(P, in, e_in, e_out, maxprec, mx, stride, base, lens8, out32, index,
                                                   index_shift, over);
  k_segr_encode<DT, true><<<nbig, V1T, 0, st>>>(P, in, e_in, e_out, maxprec, mx, stride, base, lens8, out32, index,
                                                index_shift, over);
  return hipGetLastError();
}

// -------------------------------------------------------------------------------------------------- the rate tables
constexpr uint32_t RTS_WORDS = kRateTableRelWords;
constexpr uint32_t RTS_COUNT = 2 * RT_BINS;  // the block count's word
static_assert(RTS_WORDS == RTS_COUNT + 1, "two arrays and the block count");
// A 32-bit LDS bin cannot wrap: a block adds at most 12 to one bin (rate_table1d.hip), a plan has fewer than 2^32
// virtual blocks, i.e. at most 2^22 tiles, and a run is at most ntiles / grid + 1 tiles of RT_TILE blocks.
static_assert(((1ull << 32) / RT_TILE / kRateTableRelMaxGrid + 1) * RT_TILE * 12 < (1ull << 31), "LDS bins are 32-bit");

__global__ __launch_bounds__(256) void k_rate_table_seg_zero(unsigned long long* __restrict__ ws, uint64_t nwords)
{
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nwords; i += (uint64_t)gridDim.x * 256u) ws[i] = 0ull;
}

template <int DT>
__global__ __launch_bounds__(RTT) void k_rate_table_seg(SegPlanDev P, const void* __restrict__ in,
                                                        const float* __restrict__ e_in, uint32_t pmax, uint32_t nruns,
                                                        unsigned long long* __restrict__ ws)
{
  __shared__ uint32_t hist[RT_HIST_WORDS];
  // run r of nruns <= ntiles: tiles t0 .. t1 - 1, at least one
  const uint32_t r = blockIdx.x;
  const uint32_t t0 = (uint32_t)((uint64_t)r * P.ntiles / nruns), t1 = (uint32_t)((uint64_t)(r + 1) * P.ntiles / nruns);
  rt_hist_zero(hist);
  uint32_t* step = hist;
  uint32_t* imp = hist + RT_BINS * RT_COPIES;
  const uint32_t copy = threadIdx.x & (RT_COPIES - 1u);
  uint32_t seg = ~0u;  // the tensor whose updates the LDS arrays hold (none yet)
  uint64_t nb = 0;     // its blocks seen since the last flush
  for (uint32_t t = t0; t < t1; t++) {
    const uint32_t tw = P.tiles[t];  // uniform over the workgroup
    SegYLane<DT, true> L;
    L.load(P, in, e_in, nullptr, 0u, t);
    if (tw >> 31) {  // whole blocks of one tensor
      const uint32_t s = P.ents[tw & 0x7fffffffu].seg;
      if (s != seg) {
        if (seg != ~0u) {  // the run moves on to another tensor
          __syncthreads();
          unsigned long long* w = ws + (uint64_t)seg * RTS_WORDS;
          rt_hist_flush_zero(hist, w);
          if (threadIdx.x == 0) atomicAdd(w + RTS_COUNT, (unsigned long long)nb);
          __syncthreads();
        }
        seg = s;
        nb = 0;
      }
      nb += min<uint64_t>(RT_TILE, P.nvb - (uint64_t)t * RT_TILE);
      if (pmax) {  // pmax 0: every block is one bit, only the count matters
#pragma unroll
        for (uint32_t k = 0; k < RTU; k++)
          rt_values(L.y.f[k], (L.y.valid >> k) & 1u, pmax, RtLdsSink{step, imp, copy});
      }
    } else {  // blocks of several tensors, or a partial last block: each to its tensor's slice
#pragma unroll
      for (uint32_t k = 0; k < RTU; k++) {
        const bool real = (L.y.valid >> k) & 1u;
        unsigned long long* w = ws + (uint64_t)L.seg[k] * RTS_WORDS;
        if (real && L.cnt[k]) atomicAdd(w + RTS_COUNT, (unsigned long long)L.cnt[k]);
        rt_values(L.y.f[k], real && pmax != 0u, pmax, RtGlobalSink{w});
      }
    }
  }
  if (seg != ~0u) {  // uniform
    __syncthreads();
    unsigned long long* w = ws + (uint64_t)seg * RTS_WORDS;
    rt_hist_flush(hist, w);
    if (threadIdx.x == 0) atomicAdd(w + RTS_COUNT, (unsigned long long)nb);
  }
}

// ---------------------------------------------------------------------------------------- the maximum and the words
__global__ __launch_bounds__(256) void k_seg_absmax_zero(uint32_t* __restrict__ absmax, uint32_t nsegs)
{
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nsegs; i += gridDim.x * 256u) absmax[i] = 0u;
}

// the largest of a block's four magnitudes (a missing block holds zeros)
__device__ __forceinline__ uint32_t seg_block_mag(const float* f)
{
  return max(max(rel_mag(__float_as_uint(f[0])), rel_mag(__float_as_uint(f[1]))),
             max(rel_mag(__float_as_uint(f[2])), rel_mag(__float_as_uint(f[3]))));
}

__device__ __forceinline__ uint32_t seg_wave_max(uint32_t m)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
  return m;
}

// The workgroup's maximum into the tensor's slot: one atomic, none for zero. Every lane of the workgroup calls it.
__device__ __forceinline__ void seg_absmax_flush(uint32_t m, uint32_t seg, uint32_t* sh, uint32_t* absmax)
{
  m = seg_wave_max(m);
  if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t mm = sh[0];
#pragma unroll
    for (uint32_t w = 1; w < RTT / 64; w++) mm = max(mm, sh[w]);
    if (mm) atomicMax(absmax + seg, mm);
  }
  __syncthreads();  // sh is written again by the next flush
}

template <int DT>
__global__ __launch_bounds__(RTT) void k_seg_absmax(SegPlanDev P, const void* __restrict__ in,
                                                    const float* __restrict__ e_in, uint32_t nruns, uint32_t* absmax)
{
  __shared__ uint32_t sh[RTT / 64];
  // run r of nruns <= ntiles: tiles t0 .. t1 - 1, at least one (k_rate_table_seg's cut)
  const uint32_t r = blockIdx.x;
  const uint32_t t0 = (uint32_t)((uint64_t)r * P.ntiles / nruns), t1 = (uint32_t)((uint64_t)(r + 1) * P.ntiles / nruns);
  uint32_t seg = ~0u;  // the tensor whose maximum m holds (none yet)
  uint32_t m = 0;
  for (uint32_t t = t0; t < t1; t++) {
    const uint32_t tw = P.tiles[t];  // uniform over the workgroup
    SegYLane<DT, true> L;
    L.load(P, in, e_in, nullptr, 0u, t);
    if (tw >> 31) {  // whole blocks of one tensor
      const uint32_t s = P.ents[tw & 0x7fffffffu].seg;
      if (s != seg) {
        if (seg != ~0u) seg_absmax_flush(m, seg, sh, absmax);  // the run moves on to another tensor
        seg = s;
        m = 0;
      }
#pragma unroll
      for (uint32_t k = 0; k < RTU; k++) m = max(m, seg_block_mag(L.y.f[k]));
    } else {  // blocks of several tensors, or a partial last block: each to its tensor's slot
#pragma unroll
      for (uint32_t k = 0; k < RTU; k++) {
        const uint32_t mk = seg_block_mag(L.y.f[k]), sk = L.seg[k];
        // lanes with mk = 0 have nothing to add; where the others of the wave share a tensor, one atomic serves them
        const uint64_t need = __ballot(mk != 0u);
        if (need == 0ull) continue;
        const uint32_t sref = (uint32_t)__shfl((int)sk, __ffsll((unsigned long long)need) - 1, 64);
        if (__all(mk == 0u || sk == sref)) {
          const uint32_t w = seg_wave_max(mk);
          if ((threadIdx.x & 63u) == 0) atomicMax(absmax + sref, w);
        } else if (mk != 0u) {
          atomicMax(absmax + sk, mk);
        }
      }
    }
  }
  if (seg != ~0u) seg_absmax_flush(m, seg, sh, absmax);  // uniform
}

// slot s -> the word of tensor s; an empty tensor's slot is 0, whose word is the floor
__global__ __launch_bounds__(256) void k_seg_rel_words(const uint32_t* __restrict__ absmax, uint32_t nsegs,
                                                       uint32_t rel_bits, int32_t* __restrict__ minexp, uint32_t stride)
{
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nsegs; i += gridDim.x * 256u)
    minexp[(uint64_t)i * stride] = rel_minexp(absmax[i], rel_bits);
}

}  // namespace

// zero -> pass -> words
hipError_t launch_seg_rel_minexp1d(const SegHeader& H, const void* d_plan, const void* in, const float* e_in,
                                   uint32_t rel_bits, uint32_t* absmax, int32_t* d_minexp, uint32_t stride_words,
                                   void* stream)
{
  hipStream_t st = (hipStream_t)stream;
  if (!H.nsegs) return hipSuccess;
  const uint32_t ng = std::min((H.nsegs + 255u) / 256u, 64u);
  k_seg_absmax_zero<<<ng, 256, 0, st>>>(absmax, H.nsegs);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (H.ntiles) {
    const SegPlanDev P = seg_plan_dev(H, d_plan);
    const uint32_t nruns = std::min(H.ntiles, kRateTableRelMaxGrid);
    if (H.dtype == DT_BF16) k_seg_absmax<DT_BF16><<<nruns, RTT, 0, st>>>(P, in, e_in, nruns, absmax);
    else k_seg_absmax<DT_F32><<<nruns, RTT, 0, st>>>(P, in, e_in, nruns, absmax);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  k_seg_rel_words<<<ng, 256, 0, st>>>(absmax, H.nsegs, rel_bits, d_minexp, stride_words);
  return hipGetLastError();
}

hipError_t launch_encode_seg_resid1d(const SegHeader& H, const void* d_plan, const void* in, const float* e_in,
                                     float* e_out, uint32_t maxprec, const int32_t* d_minexp, uint32_t stride_words,
                                     uint32_t* out32, uint64_t* ws, uint64_t* d_total, uint64_t* index,
                                     uint32_t index_shift, void* stream)
{
  hipStream_t st = (hipStream_t)stream;
  if (!H.nvb) return d_total ? launch_set_u64(d_total, 0, stream) : hipSuccess;
  const SegPlanDev P = seg_plan_dev(H, d_plan);
  if (H.dtype == DT_BF16)
    return segr_launch_encode<DT_BF16>(P, in, e_in, e_out, maxprec, d_minexp, stride_words, out32, ws, d_total, index,
                                       index_shift, st);
  return segr_launch_encode<DT_F32>(P, in, e_in, e_out, maxprec, d_minexp, stride_words, out32, ws, d_total, index,
                                    index_shift, st);
}

// zero -> pass -> finish
hipError_t launch_rate_table_seg1d(const SegHeader& H, const void* d_plan, const void* in, const float* e_in,
                                   uint32_t maxprec, uint64_t* tables, uint64_t* ws, void* stream)
{
  hipStream_t st = (hipStream_t)stream;
  if (!H.nsegs) return hipSuccess;
  const uint64_t nwords = (uint64_t)H.nsegs * RTS_WORDS;
  k_rate_table_seg_zero<<<(uint32_t)std::min<uint64_t>((nwords + 255) / 256, 1024), 256, 0, st>>>(
      (unsigned long long*)ws, nwords);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (H.ntiles) {
    const SegPlanDev P = seg_plan_dev(H, d_plan);
    const uint32_t pmax = std::min(maxprec, 32u);
    const uint32_t nruns = std::min(H.ntiles, kRateTableRelMaxGrid);
    unsigned long long* w = (unsigned long long*)ws;
    if (H.dtype == DT_BF16) k_rate_table_seg<DT_BF16><<<nruns, RTT, 0, st>>>(P, in, e_in, pmax, nruns, w);
    else k_rate_table_seg<DT_F32><<<nruns, RTT, 0, st>>>(P, in, e_in, pmax, nruns, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return launch_rate_table_finish_batch(ws, H.nsegs, RTS_WORDS, RTS_COUNT, tables, stream);
}

}  // namespace gcow
