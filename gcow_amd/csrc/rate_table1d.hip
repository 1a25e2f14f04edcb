// rate_table1d.hip -- the rate table of a 1-D field (gcow_rate_table_device): table[t], t = 0 .. 287,
// is the stream length of the field under expert(1, 16658, maxprec, -154 + t), for all t from one pass over the input.
//
// A block's coefficients do not depend on minexp (the cast scales by the block's own exponent), and in the no-budget
// domain its code length is a closed form of the leading planes of the suffix ORs of its four coefficients (v1_prep,
// var1d_prep.h). With a = emax + 158 the block's precision at entry t is P = min(pmax, max(0, a - t)),
// pmax = min(maxprec, 32), and its length is L(0) = 1,
//   L(P) = 13 + 4 (P - 1) - sum_{j<3} min(z_j, P) + sum_{j<3} [z_j <= P - 1] b_j        (P >= 1)
// with z_j = clz(S_j) (32 for 0) of S_2 = u_2 | u_3, S_1 = u_1 | S_2, S_0 = u_0 | S_1 and b_j = bit 31 - z_j of u_j.
// Its first difference over t, F[t] = L(a - t) - L(a - t - 1), is L(1) - 1 at t = a - 1 and
//   F[a - 1 - P] = 1 + #{j : z_j <= P} + sum_j [z_j = P] b_j                               (P = 1 .. pmax - 1):
// a step function of P (1 + #{z_j <= P}) plus impulses (b_j at P = z_j). So a block is at most 9 updates of two 288-bin
// arrays -- steps: + (1 + #{z_j <= 1}) at a - 2, + 1 at a - 1 - z_j for 2 <= z_j <= pmax - 1, minus their sum at
// a - 1 - pmax; impulses: L(1) - 1 at a - 1, b_j at a - 1 - z_j for 1 <= z_j <= pmax - 1 -- and
//   table[t] = nblocks + sum_{s >= t} (impulse[s] + sum_{r >= s} step[r]).
// A zero block (or pmax = 0) is one bit at every t and adds nothing. Indices run from -1 (the step end of an
// emax = -126 block at pmax = 32, dropped: the table starts at 0) to 285.
//
//   k_rate_table1d        RT_TILE blocks per workgroup and iteration, a grid-stride loop with the next tile's loads
//                         issued before a tile is processed. The two arrays live in LDS as 32-bit integers, RT_COPIES
//                         interleaved copies each (lane & 15 picks the copy): a gradient bucket puts most blocks of a
//                         wave on the same few bins, and same-address LDS atomics serialise, so the copies cut a
//                         64-deep conflict to 4. At the end the workgroup sums the copies and adds its non-zero bins
//                         to the global workspace with 64-bit atomics (steps sign-extended).
//   k_rate_table1d_xe     the same pass over two rows, x and a carried error e: the table of y = x + e formed in
//                         registers (gcow_rate_table_residual_device).
//   k_rate_table_finish   288 x 2 workspace words -> the table: both suffix sums in one backward sweep. One workgroup
//                         per table: a batch of tables (rate_table_rel1d.hip, a table per tensor) is one launch.
//   k_rate_table_fit      a table and a budget -> the gcow_fit record; one workgroup per table as well.
//   k_rate_table_zero     the workspace zeroed in stream order ahead of the first kernel. A kernel and not a memset:
//                         in a captured graph that also holds the fit and the encoder (FittedEncoder), the memset
//                         node's fill wrote a stale 16-byte pattern from the second replay on (the workspace then held
//                         that pattern plus the pass's own counts, and the table was garbage).
// The table is written whole. Integer adds only: the result does not depend on the order of the atomics.
// The per-block pieces (RtRaw, rt_add, rt_block, rt_values, rt_tile, the LDS arrays' zeroing and flush) are in
// rate_table1d.h, which the pass over a tensor list's plan shares (rate_table_list1d.hip; it runs between this unit's
// zero and finish kernels through launch_rate_table_zero / launch_rate_table_finish).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "codec_device.h"
#include "field_io.h"
#include "kernels.h"
#include "lean1d.h"
#include "rate_table1d.h"
#include "var1d_prep.h"

namespace gcow {

namespace {

constexpr uint32_t RT_MAXGRID = 1024;  // 4 workgroups of 36 KB LDS per CU on 256 CUs
// A 32-bit LDS bin cannot wrap: a block adds at most 12 to one bin (L(1) - 1 <= 12; a step start or end is at most 4
// in magnitude), a call has fewer than 2^32 blocks in at most 2^22 tiles, so a workgroup of a full grid sees at most
// 2^22 / RT_MAXGRID + 1 tiles = 2^22 + 2^10 blocks, and (2^22 + 2^10) * 12 < 2^26.
static_assert(((1ull << 32) / RT_TILE / RT_MAXGRID + 1) * RT_TILE * 12 < (1ull << 31), "LDS bins are 32-bit");

template <int DT>
__global__ __launch_bounds__(RTT) void k_rate_table1d(FieldDesc F, uint32_t pmax, uint32_t ntiles,
                                                      unsigned long long* __restrict__ ws)
{
  __shared__ uint32_t hist[RT_HIST_WORDS];
  const uint32_t tid = threadIdx.x;
  rt_hist_zero(hist);
  uint32_t* step = hist;
  uint32_t* imp = hist + RT_BINS * RT_COPIES;
  const uint32_t copy = tid & (RT_COPIES - 1u);
  const bool wide_ok = F.vec && (((uintptr_t)F.data) & 15u) == 0;
  const uint32_t nfull = wide_ok ? (uint32_t)(F.n[0] / 4 / RT_TILE) : 0u;  // tiles of whole blocks, loaded wide
  RtRaw<DT> cur{}, nxt{};
  uint32_t t = blockIdx.x;
  if (t < nfull) cur.load_wide(F, t);
  for (; t < ntiles; t += gridDim.x) {
    if (t >= nfull) cur.gather(F, t);
    const uint32_t tn = t + gridDim.x;  // < 2^22 + 2^10
    if (tn < nfull) nxt.load_wide(F, tn);
    rt_tile<DT>(F, cur, t, pmax, step, imp, copy);
    cur = nxt;
  }
  __syncthreads();
  rt_hist_flush(hist, ws);
}

// The lane's RTU blocks of y = x + e from its x words and e words: the single fadd of the residual encoder
// (v1_form_y, var1d.hip), a bf16 x widened exactly. y lives in registers only.
template <int DT>
__device__ __forceinline__ void rt_form_y(const RtRaw<DT>& rx, const RtRaw<DT_F32>& re, RtRaw<DT_F32>& y)
{
#pragma unroll
  for (uint32_t k = 0; k < RTU; k++) {
    float f[4], e[4];
    rx.block(k, f);
    re.block(k, e);
    y.w[k] = make_uint4(__float_as_uint(__fadd_rn(f[0], e[0])), __float_as_uint(__fadd_rn(f[1], e[1])),
                        __float_as_uint(__fadd_rn(f[2], e[2])), __float_as_uint(__fadd_rn(f[3], e[3])));
  }
}

// k_rate_table1d over two input rows (gcow_rate_table_residual_device): the table of y = x + e. The same tiles,
// grid-stride loop and next-tile prefetch, which now holds the lane's x rows (fp32: 4, bf16: 2) and its 4 e rows; the
// blocks go through rt_tile as fp32 y, so Inf / NaN blocks of y (x + e may overflow) take the generic rule there.
// The wide path needs both rows 16-byte aligned; else every tile is gathered, x and e with the same padding indices,
// so a padding value of y is a copy of a real one -- the encoder's padding of y.
template <int DT>
__global__ __launch_bounds__(RTT) void k_rate_table1d_xe(FieldDesc F, const float* __restrict__ e_in, uint32_t pmax,
                                                         uint32_t ntiles, unsigned long long* __restrict__ ws)
{
  __shared__ uint32_t hist[RT_HIST_WORDS];
  const uint32_t tid = threadIdx.x;
  rt_hist_zero(hist);
  uint32_t* step = hist;
  uint32_t* imp = hist + RT_BINS * RT_COPIES;
  const uint32_t copy = tid & (RT_COPIES - 1u);
  FieldDesc Fe = F;
  Fe.data = e_in;
  Fe.dtype = DT_F32;
  Fe.vec = (((uintptr_t)e_in) & 15u) == 0 ? 1u : 0u;
  const bool wide_ok = F.vec && (((uintptr_t)F.data) & 15u) == 0 && Fe.vec;
  const uint32_t nfull = wide_ok ? (uint32_t)(F.n[0] / 4 / RT_TILE) : 0u;  // tiles of whole blocks, loaded wide
  RtRaw<DT> curx{}, nxtx{};
  RtRaw<DT_F32> cure{}, nxte{};
  uint32_t t = blockIdx.x;
  if (t < nfull) {
    curx.load_wide(F, t);
    cure.load_wide(Fe, t);
  }
  for (; t < ntiles; t += gridDim.x) {
    if (t >= nfull) {
      curx.gather(F, t);
      cure.gather(Fe, t);
    }
    const uint32_t tn = t + gridDim.x;  // < 2^22 + 2^10
    if (tn < nfull) {
      nxtx.load_wide(F, tn);
      nxte.load_wide(Fe, tn);
    }
    RtRaw<DT_F32> y;
    rt_form_y<DT>(curx, cure, y);
    rt_tile<DT_F32>(F, y, t, pmax, step, imp, copy);
    curx = nxtx;
    cure = nxte;
  }
  __syncthreads();
  rt_hist_flush(hist, ws);
}

__global__ __launch_bounds__(RT_BINS) void k_rate_table_zero(unsigned long long* __restrict__ ws)
{
  ws[threadIdx.x] = 0ull;
  ws[RT_BINS + threadIdx.x] = 0ull;
}

// Table blockIdx.x of a batch: its workspace is stride words after the one before, its row RT_BINS words. count_word
// != 0: the table's block count is that word of its workspace (the per-tensor pass counts it there), else nblocks.
__global__ __launch_bounds__(RT_BINS) void k_rate_table_finish(const unsigned long long* __restrict__ ws,
                                                               uint64_t stride, uint32_t count_word, uint64_t nblocks,
                                                               uint64_t* __restrict__ table)
{
  __shared__ uint64_t s[2 * RT_BINS];
  const uint32_t tid = threadIdx.x;
  ws += (uint64_t)blockIdx.x * stride;
  table += (uint64_t)blockIdx.x * RT_BINS;
  s[tid] = ws[tid];
  s[RT_BINS + tid] = ws[RT_BINS + tid];
  __syncthreads();
  if (tid == 0) {
    uint64_t level = 0, acc = count_word ? (uint64_t)ws[count_word] : nblocks;
    for (int t = (int)RT_BINS - 1; t >= 0; t--) {
      level += s[t];
      acc += level + s[RT_BINS + t];
      s[t] = acc;
    }
  }
  __syncthreads();
  table[tid] = s[tid];
}

// The fit (gcow_rate_table_fit_device, gcow_rate_table_fit_batch_device): the table is non-increasing, so the entries
// within the budget are a suffix and the answer is the smallest index among them -- a min over the lanes whose entry
// fits, one LDS atomic each. No entry fits: the coarsest set, flagged. One workgroup per table: table blockIdx.x
// against budgets[blockIdx.x] (budgets null: budget) into fit[blockIdx.x]; lanes below lo -- a floor on minexp -- take
// no part.
__global__ __launch_bounds__(RT_BINS) void k_rate_table_fit(const uint64_t* __restrict__ table,
                                                            const uint64_t* __restrict__ budgets, uint64_t budget,
                                                            uint32_t lo, RateFit* __restrict__ fit)
{
  __shared__ uint32_t best;
  const uint32_t tid = threadIdx.x;
  table += (uint64_t)blockIdx.x * RT_BINS;
  fit += blockIdx.x;
  if (budgets) budget = budgets[blockIdx.x];
  if (tid == 0) best = RT_BINS;
  __syncthreads();
  const uint64_t v = table[tid];
  if (v <= budget && tid >= lo) atomicMin(&best, tid);
  __syncthreads();
  if (tid == min(best, RT_BINS - 1u)) {  // the lane that holds the chosen entry
    fit->minexp = kRateTableMinExpLo + (int32_t)tid;
    fit->status = best == RT_BINS ? 1u : 0u;
    fit->bits = v;
  }
}

}  // namespace

hipError_t launch_rate_table_fit(const uint64_t* table, uint64_t budget_bits, RateFit* fit, void* stream)
{
  k_rate_table_fit<<<1, RT_BINS, 0, (hipStream_t)stream>>>(table, nullptr, budget_bits, 0u, fit);
  return hipGetLastError();
}

hipError_t launch_rate_table_fit_batch(const uint64_t* tables, uint32_t ntables, const uint64_t* budgets,
                                       int32_t minexp_floor, RateFit* fits, void* stream)
{
  if (!ntables) return hipSuccess;
  const int64_t lo = (int64_t)minexp_floor - kRateTableMinExpLo;  // above 287: no lane takes part, status 1
  k_rate_table_fit<<<ntables, RT_BINS, 0, (hipStream_t)stream>>>(
      tables, budgets, 0ull, (uint32_t)std::min<int64_t>(std::max<int64_t>(lo, 0), RT_BINS), fits);
  return hipGetLastError();
}

size_t rate_table_workspace_bytes() { return 2 * RT_BINS * sizeof(uint64_t); }

hipError_t launch_rate_table_zero(uint64_t* ws, void* stream)
{
  k_rate_table_zero<<<1, RT_BINS, 0, (hipStream_t)stream>>>((unsigned long long*)ws);
  return hipGetLastError();
}

hipError_t launch_rate_table_finish(const uint64_t* ws, uint64_t nblocks, uint64_t* table, void* stream)
{
  k_rate_table_finish<<<1, RT_BINS, 0, (hipStream_t)stream>>>((const unsigned long long*)ws, 0ull, 0u, nblocks, table);
  return hipGetLastError();
}

hipError_t launch_rate_table_finish_batch(const uint64_t* ws, uint32_t ntables, uint64_t stride_words,
                                          uint32_t count_word, uint64_t* tables, void* stream)
{
  if (!ntables) return hipSuccess;
  k_rate_table_finish<<<ntables, RT_BINS, 0, (hipStream_t)stream>>>((const unsigned long long*)ws, stride_words,
                                                                    count_word, 0ull, tables);
  return hipGetLastError();
}

// zero -> pass -> finish; e_in null: the table of x (y = x + 0 codes as x), else of y = x + e
hipError_t launch_rate_table1d_resid(const FieldDesc& F, const float* e_in, uint32_t maxprec, uint64_t* table,
                                     uint64_t* ws, void* stream)
{
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* w = (unsigned long long*)ws;
  hipError_t e = launch_rate_table_zero(ws, stream);
  if (e != hipSuccess) return e;
  const uint32_t pmax = std::min(maxprec, 32u);
  if (F.nblocks && pmax) {
    const uint32_t ntiles = (uint32_t)(((uint64_t)F.nblocks + RT_TILE - 1) / RT_TILE);
    const uint32_t grid = std::min(ntiles, RT_MAXGRID);
    const bool bf16 = F.dtype == DT_BF16;
    if (!e_in && bf16) k_rate_table1d<DT_BF16><<<grid, RTT, 0, st>>>(F, pmax, ntiles, w);
    else if (!e_in) k_rate_table1d<DT_F32><<<grid, RTT, 0, st>>>(F, pmax, ntiles, w);
    else if (bf16) k_rate_table1d_xe<DT_BF16><<<grid, RTT, 0, st>>>(F, e_in, pmax, ntiles, w);
    else k_rate_table1d_xe<DT_F32><<<grid, RTT, 0, st>>>(F, e_in, pmax, ntiles, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return launch_rate_table_finish(ws, F.nblocks, table, stream);
}

hipError_t launch_rate_table1d(const FieldDesc& F, uint32_t maxprec, uint64_t* table, uint64_t* ws, void* stream)
{
  return launch_rate_table1d_resid(F, nullptr, maxprec, table, ws, stream);
}

}  // namespace gcow
