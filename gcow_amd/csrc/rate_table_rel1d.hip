// rate_table_rel1d.hip -- a rate table per tensor of a list (gcow_rate_table_rel_device, include/gcow.h; DESIGN.md
// 5.14): tables[s][t] is what k_rate_table1d gives for tensor s as a field of its own, from the plan of the relative
// round trip (gcow_roundtrip_rel_plan, kernels.h RtRel*) as it is. In that plan blocks are each tensor's own and no
// block crosses a tensor, so every block belongs to one table; the per-block pieces are rate_table1d.h's.
//
// The workspace is kRateTableRelWords = 2 * 288 + 1 words per tensor, the caller's numbering: the two 288-bin arrays
// of rate_table1d.hip, then the tensor's block count ceil(n_s / 4), which the finish needs and the plan has no table
// of: the pass counts it (a direct run adds its chunks' nb; the lane that holds a piece's first gather block adds the
// piece's ceil(n / 4) - b0), so the plan's layout stays as it is.
//
//   k_rate_table_rel_zero  the workspace zeroed in stream order (a kernel, not a memset node: rate_table1d.hip).
//   k_rate_table_rel       one launch, gather chunks first as k_rel_absmax orders them (their lanes chase dependent
//                          loads and, started last, would run on alone):
//     gather chunks        one workgroup per RtRelGather, one block per lane. The workgroup's 256 blocks may lie in
//                          dozens of tensors, so the LDS arrays are of no use: the lane locates its block
//                          (rel_locate_piece), loads its values one by one, pads a partial block as
//                          k_roundtrip_rel_gather does, and adds the block's <= 9 updates straight to its tensor's
//                          workspace by 64-bit atomics (RtGlobalSink: steps sign-extended).
//     direct chunks        zeroing and flushing the 36 KB of LDS arrays costs about as many LDS operations as a chunk's
//                          own updates, so a workgroup does not take one chunk: the ndirect chunks are cut into
//                          min(ndirect, kRateTableRelMaxGrid) contiguous runs, one per workgroup. The plan's chunks of
//                          a tensor are consecutive, so a run changes tensor rarely; only then (and at its end) the
//                          arrays are flushed to the tensor's workspace and zeroed again (rt_hist_flush_zero). A chunk
//                          is read as k_rate_table_list reads it (RtlRows: raw buffer loads on a per-chunk resource,
//                          rows past nb read zeros, a zero block adds nothing), two halves with the other half's -- or
//                          the next chunk's first half's -- loads in flight while a half is processed; a flush between
//                          two chunks leaves those loads in flight too.
//   k_rate_table_finish    (rate_table1d.hip) one workgroup per tensor, the block count from the workspace. An empty
//                          tensor has an all-zero workspace slice and gets an all-zero row.
// Integer adds only: the same bits run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "field_io.h"
#include "kernels.h"
#include "pipe.h"
#include "rate_table1d.h"
#include "rel_locate.h"

namespace gcow {

namespace {

constexpr uint32_t RTR_WORDS = kRateTableRelWords;
constexpr uint32_t RTR_COUNT = 2 * RT_BINS;  // the block count's word
static_assert(RTR_WORDS == RTR_COUNT + 1, "two arrays and the block count");
static_assert(kRtRelGatherBlocks == RTT, "a gather chunk is one block per lane");
// A 32-bit LDS bin cannot wrap: a block adds at most 12 to one bin (rate_table1d.hip). The plan has fewer than 2^32
// blocks and every direct chunk but a tensor's last is 2048 of them; a run is at most ndirect / grid + 1 chunks.
// Were every chunk of a full grid's run a full one: (2^32 / 2048 / kRateTableRelMaxGrid + 1) * 2048 * 12 < 2^27.
static_assert(((1ull << 32) / kRtListChunkBlocks / kRateTableRelMaxGrid + 1) * kRtListChunkBlocks * 12 < (1ull << 31),
              "LDS bins are 32-bit");

__global__ __launch_bounds__(256) void k_rate_table_rel_zero(unsigned long long* __restrict__ ws, uint64_t nwords)
{
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nwords; i += (uint64_t)gridDim.x * 256u) ws[i] = 0ull;
}

template <int DT>
__global__ __launch_bounds__(RTT) void k_rate_table_rel(const RtRelDirect* __restrict__ direct, uint32_t ndirect,
                                                        uint32_t nruns, const RtRelGather* __restrict__ chunks,
                                                        uint32_t ngather, const RtRelPiece* __restrict__ pieces,
                                                        uint32_t pmax, unsigned long long* __restrict__ ws)
{
  __shared__ uint32_t hist[RT_HIST_WORDS];
  if (blockIdx.x < ngather) {  // uniform over the workgroup
    const RtRelGather c = chunks[blockIdx.x];
    const bool act = threadIdx.x < c.nb;
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t seg = 0;
    if (act) {
      const RtRelPiece e = pieces[rel_locate_piece(c, pieces, threadIdx.x)];
      const uint32_t v = c.vb0 + threadIdx.x;
      const uint64_t x0 = 4ull * ((uint64_t)e.b0 + (v - e.vb));
      const uint32_t nv = (uint32_t)min<uint64_t>(4, e.n - x0);
      seg = e.seg;
#pragma unroll
      for (uint32_t x = 0; x < 4u; x++)
        if (x < nv) f[x] = load_elem<DT>((const char*)e.in, (int64_t)(x0 + x));
      // pad_index (field_io.h) written out: 1 -> v0 v0 v0 v0, 2 -> v0 v1 v1 v0, 3 -> v0 v1 v2 v0
      if (nv < 2u) f[1] = f[0];
      if (nv < 3u) f[2] = nv == 2u ? f[1] : f[0];
      if (nv < 4u) f[3] = f[0];
      if (v == e.vb)  // the piece's first block: all its gather blocks counted at once
        atomicAdd(ws + (uint64_t)seg * RTR_WORDS + RTR_COUNT, (unsigned long long)((e.n + 3) / 4 - e.b0));
    }
    rt_values(f, act && pmax != 0u, pmax, RtGlobalSink{ws + (uint64_t)seg * RTR_WORDS});  // pmax 0: one bit a block
    return;
  }

  // run r of nruns <= ndirect: chunks c0 .. c1 - 1, at least one
  const uint32_t r = blockIdx.x - ngather;
  const uint32_t c0 = (uint32_t)((uint64_t)r * ndirect / nruns), c1 = (uint32_t)((uint64_t)(r + 1) * ndirect / nruns);
  rt_hist_zero(hist);
  uint32_t* step = hist;
  uint32_t* imp = hist + RT_BINS * RT_COPIES;
  const uint32_t copy = threadIdx.x & (RT_COPIES - 1u);
  RtlRows<DT> a{}, b{};
  a.load(rtl_in_rows<DT>(direct + c0), 0u);
  uint32_t seg = rtl_sgpr(direct[c0].seg);
  uint64_t nb = 0;  // the blocks of seg seen since the last flush
  for (uint32_t d = c0; d < c1; d++) {
    const uint32_t s = rtl_sgpr(direct[d].seg);
    if (s != seg) {  // uniform: the run moves on to another tensor
      __syncthreads();
      unsigned long long* w = ws + (uint64_t)seg * RTR_WORDS;
      rt_hist_flush_zero(hist, w);
      if (threadIdx.x == 0) atomicAdd(w + RTR_COUNT, (unsigned long long)nb);
      __syncthreads();
      seg = s;
      nb = 0;
    }
    nb += min(rtl_sgpr(direct[d].nb), kRtListChunkBlocks);
    b.load(rtl_in_rows<DT>(direct + d), 1u);
    if (pmax) rtl_half<DT>(a, pmax, step, imp, copy);  // pmax 0: every block is one bit, only the count matters
    if (d + 1u < c1) a.load(rtl_in_rows<DT>(direct + d + 1u), 0u);
    if (pmax) rtl_half<DT>(b, pmax, step, imp, copy);
  }
  __syncthreads();
  unsigned long long* w = ws + (uint64_t)seg * RTR_WORDS;
  rt_hist_flush(hist, w);
  if (threadIdx.x == 0) atomicAdd(w + RTR_COUNT, (unsigned long long)nb);
}

}  // namespace

size_t rate_table_rel_workspace_bytes(uint32_t nsegs)
{
  return (size_t)std::max(nsegs, 1u) * RTR_WORDS * sizeof(uint64_t);
}

// zero -> pass -> finish
hipError_t launch_rate_table_rel1d(const RtRelHeader& h, const void* d_plan, uint32_t maxprec, uint64_t* tables,
                                   uint64_t* ws, void* stream)
{
  hipStream_t st = (hipStream_t)stream;
  if (!h.nsegs) return hipSuccess;
  const uint64_t nwords = (uint64_t)h.nsegs * RTR_WORDS;
  k_rate_table_rel_zero<<<(uint32_t)std::min<uint64_t>((nwords + 255) / 256, 1024), 256, 0, st>>>(
      (unsigned long long*)ws, nwords);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const uint32_t pmax = std::min(maxprec, 32u);
  if (h.ndirect + h.ngather) {
    const char* dp = (const char*)d_plan;
    const RtRelDirect* dd = (const RtRelDirect*)(dp + h.off_direct);
    const RtRelGather* gg = (const RtRelGather*)(dp + h.off_gather);
    const RtRelPiece* pp = (const RtRelPiece*)(dp + h.off_pieces);
    const uint32_t nruns = std::min(h.ndirect, kRateTableRelMaxGrid);
    unsigned long long* w = (unsigned long long*)ws;
    if (h.in_dtype == DT_BF16)
      k_rate_table_rel<DT_BF16><<<h.ngather + nruns, RTT, 0, st>>>(dd, h.ndirect, nruns, gg, h.ngather, pp, pmax, w);
    else
      k_rate_table_rel<DT_F32><<<h.ngather + nruns, RTT, 0, st>>>(dd, h.ndirect, nruns, gg, h.ngather, pp, pmax, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return launch_rate_table_finish_batch(ws, h.nsegs, RTR_WORDS, RTR_COUNT, tables, stream);
}

}  // namespace gcow
