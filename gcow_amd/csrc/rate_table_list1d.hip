// rate_table_list1d.hip -- the rate table (rate_table1d.hip) of the concatenation X of a list of
// tensors, each read where it lies (gcow_rate_table_list_device, include/gcow.h): table[t] is what
// k_rate_table1d gives for the contiguous X, from the plan of the list round trip (gcow_roundtrip_list_plan, kernels.h
// RtList*) as it is. Blocks are X's blocks and a block's updates do not depend on where its values came from, so only
// the loads know about the list; the per-block pieces are rate_table1d.h's, one definition for both passes.
//
//   k_rate_table_list   one launch over the plan's chunks of 2048 blocks. The work items are numbered gather units
//                       first -- a gather chunk is 8 units of 256 blocks -- then direct chunks; workgroup w of a grid
//                       of G takes items w, w + G, ...:
//     gather units      one block per lane: a gather lane's time is a chain of dependent loads (the bisection, then
//                       its values) that only more workgroups shorten, so a chunk is spread over 8 of them and comes
//                       first (started last, its lanes would run on alone). Every value is located in the segment
//                       table as k_roundtrip_list_gather locates it (rtl_gather_block), the partial last block padded
//                       by pad_index's rule, bf16 widened exactly, then rt_values.
//     direct chunks     up to 2048 whole blocks of one tensor whose first row is 4-byte aligned -- not necessarily 16,
//                       and for bf16 not necessarily 8 -- so no wide pointer dereference: a buffer resource over the
//                       chunk's nb rows (as rtl_resources builds it) and raw buffer loads, which need dword alignment
//                       only (a 16-byte row by one load, an 8-byte bf16 row by one load: rows, not pairs of rows, so
//                       that the range check never splits an access). A chunk runs as two halves of 1024 blocks, each
//                       lane 4 consecutive blocks as in k_rate_table1d; the other half's -- or the next chunk's first
//                       half's -- loads are issued before a half is processed, the first chunk's ahead of the
//                       workgroup's gather units. Rows past nb read zeros, and a zero block adds nothing to either
//                       histogram: no lane mask. The loads are the compiler-visible builtins: there is no store in
//                       the loop for vmcnt to mix them with, and the compiler's own counted waits keep the other half
//                       in flight.
//   Both kinds add to the same two 288-bin LDS arrays (16 interleaved copies, 36 864 B) and the workgroup flushes them
//   once, by 64-bit atomics. k_rate_table_zero runs ahead and k_rate_table_finish behind (launch_rate_table_zero /
//   _finish), with nblocks = ceil(N / 4) from the plan's header. Integer adds only: the same bits run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"
#include "pipe.h"
#include "rate_table1d.h"
#include "rtlist_gather.h"

namespace gcow {

namespace {

constexpr uint32_t RTL_GU = kRtListChunkBlocks / RTT;            // gather units (one block per lane) per chunk
// A 32-bit LDS bin cannot wrap: a block adds at most 12 to one bin (rate_table1d.hip). X has fewer than 2^32 blocks,
// so the plan has at most 2^32 / 2048 = 2^21 chunks (every chunk but the last is 2048 blocks of X). A workgroup of a
// full grid takes at most 2^21 / kRateTableListMaxGrid + 1 = 2049 direct chunks and, were every chunk a gather chunk,
// 8 * 2^21 / kRateTableListMaxGrid + 1 gather units of 256 blocks: (2049 * 2048 + (2^14 + 1) * 256) * 12 < 2^27.
// A smaller grid is one item per workgroup.
static_assert((((1ull << 32) / kRtListChunkBlocks / kRateTableListMaxGrid + 1) * kRtListChunkBlocks +
               ((1ull << 32) / RTT / kRateTableListMaxGrid + 1) * RTT) * 12 < (1ull << 31), "LDS bins are 32-bit");

// RtlRows, rtl_in_rows and rtl_half -- a direct chunk's rows -- are rate_table1d.h's, shared with rate_table_rel1d.hip.
template <int DT>
__global__ __launch_bounds__(RTT) void k_rate_table_list(const RtListDirect* __restrict__ direct, uint32_t ndirect,
                                                         const RtListGather* __restrict__ gather, uint32_t ngather,
                                                         const RtListSeg* __restrict__ segs, uint64_t nvals,
                                                         uint32_t pmax, unsigned long long* __restrict__ ws)
{
  __shared__ uint32_t hist[RT_HIST_WORDS];
  rt_hist_zero(hist);
  uint32_t* step = hist;
  uint32_t* imp = hist + RT_BINS * RT_COPIES;
  const uint32_t copy = threadIdx.x & (RT_COPIES - 1u);
  const uint32_t grid = gridDim.x;

  // item ngu + d, direct chunk d, belongs to workgroup (ngu + d) mod grid; its first half is requested ahead of the
  // gather units, whose dependent loads it then overlaps
  const uint32_t ngu = ngather * RTL_GU;  // < 2^24
  uint32_t d = (blockIdx.x + grid - ngu % grid) % grid;
  RtlRows<DT> a{}, b{};
  if (d < ndirect) a.load(rtl_in_rows<DT>(direct + d), 0u);

  const uint64_t nblocks = (nvals + 3) / 4;
  for (uint32_t u = blockIdx.x; u < ngu; u += grid) {
    const RtListGather c = gather[u / RTL_GU];
    const uint32_t nb = (uint32_t)min<uint64_t>(kRtListChunkBlocks, nblocks - c.b0);
    const uint32_t i = threadIdx.x + RTT * (u % RTL_GU);
    const bool act = i < nb;
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    rtl_gather_block<DT, 0u>(c, segs, nvals, i, act, f, nullptr);
    rt_values(f, act, pmax, step, imp, copy);
  }

  for (; d < ndirect; d += grid) {
    b.load(rtl_in_rows<DT>(direct + d), 1u);
    rtl_half<DT>(a, pmax, step, imp, copy);
    const uint32_t dn = d + grid;  // < 2^21 + 2^10
    if (dn < ndirect) a.load(rtl_in_rows<DT>(direct + dn), 0u);
    rtl_half<DT>(b, pmax, step, imp, copy);
  }
  __syncthreads();
  rt_hist_flush(hist, ws);
}

}  // namespace

// zero -> pass -> finish
hipError_t launch_rate_table_list1d(const RtListHeader& h, const void* d_plan, uint32_t maxprec, uint64_t* table,
                                    uint64_t* ws, void* stream)
{
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = launch_rate_table_zero(ws, stream);
  if (e != hipSuccess) return e;
  const uint32_t pmax = std::min(maxprec, 32u);
  const uint64_t nitems = (uint64_t)h.ndirect + (uint64_t)h.ngather * RTL_GU;
  if (h.nvals && pmax && nitems) {
    const char* dp = (const char*)d_plan;
    const RtListDirect* dd = (const RtListDirect*)(dp + h.off_direct);
    const RtListGather* gg = (const RtListGather*)(dp + h.off_gather);
    const RtListSeg* ss = (const RtListSeg*)(dp + h.off_segs);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(nitems, kRateTableListMaxGrid);
    unsigned long long* w = (unsigned long long*)ws;
    if (h.in_dtype == DT_BF16)
      k_rate_table_list<DT_BF16><<<grid, RTT, 0, st>>>(dd, h.ndirect, gg, h.ngather, ss, h.nvals, pmax, w);
    else
      k_rate_table_list<DT_F32><<<grid, RTT, 0, st>>>(dd, h.ndirect, gg, h.ngather, ss, h.nvals, pmax, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return launch_rate_table_finish(ws, (h.nvals + 3) / 4, table, stream);
}

}  // namespace gcow
