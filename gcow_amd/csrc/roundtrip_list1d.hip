// roundtrip_list1d.hip -- the fused round trip (roundtrip1d.hip) of the concatenation X of a list of tensors, each
// tensor read and written where it lies (gcow_roundtrip_list_device, include/gcow.h): what the reference's training
// loop computes between collect_gradients and assign_gradients (hw/models/train_imagenet.py:448-475) without the
// torch.cat before it and the copy per parameter after it. Blocks are X's blocks; every block's round trip is
// independent, so only the address arithmetic knows about the list. The host plan (gcow_roundtrip_list_plan,
// kernels.h RtList*) cuts X into chunks of 256 U blocks, the contiguous kernels' workgroup chunk:
//   k_roundtrip_list_fixed   direct chunks of the lean fixed-rate domain: one workgroup per RtListDirect, the
//   k_roundtrip_list_var     resources built from its two row pointers, then rt_fixed_chunk / rt_var_chunk
//                            (roundtrip1d.h) unchanged -- the block sequence of k_roundtrip1d_fixed_np / _var
//   k_roundtrip_list_gather  every other chunk (a seam between tensors, rows off 4-byte alignment, the partial last
//                            block; every chunk of the generic domain): one workgroup per RtListGather, each lane U
//                            blocks, every value located in the segment table and loaded on its own, the block coded
//                            by the domain's block function (rt_fixed_code, rt_var_code, rt_block_generic)
//   k_roundtrip_list_var_fitted, k_roundtrip_list_gather_fitted   the no-budget kernels with minexp from a word of
//                            device memory (gcow_roundtrip_list_fitted_device)
// The results are bit for bit those of gcow_roundtrip_device on the contiguous X.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>
#include <utility>

#include "field_io.h"
#include "roundtrip1d.h"
#include "rtlist_gather.h"

namespace gcow {

static_assert(kRtListChunkBlocks == 256u * GCOW_RT_U, "the plan's chunk is the workgroup's chunk");

// ------------------------------------------------------------------------------------------------ direct chunks
// The workgroup's descriptor, as two buffer resources over the chunk's nb rows. The descriptor's address is uniform
// (a kernel argument indexed by blockIdx), so these are scalar loads; readfirstlane makes every word provably
// wave-uniform for the "s" operands of the row loads and folds away where the compiler already knows it.
__device__ __forceinline__ uint32_t rtl_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

template <int DT_IN, int DT_OUT>
__device__ __forceinline__ void rtl_resources(const RtListDirect* __restrict__ desc, pipe_v4i& rin,
                                              __amdgpu_buffer_rsrc_t& rout, uint32_t& nb)
{
  const RtListDirect* d = desc + blockIdx.x;
  const uint64_t in = d->in, out = d->out;
  const uint32_t ilo = rtl_uniform((uint32_t)in), ihi = rtl_uniform((uint32_t)(in >> 32));
  const uint32_t olo = rtl_uniform((uint32_t)out), ohi = rtl_uniform((uint32_t)(out >> 32));
  nb = min(rtl_uniform(d->nb), kRtListChunkBlocks);
  rin.x = (int)ilo;
  rin.y = (int)(ihi & 0xffffu);                        // stride 0
  rin.z = (int)(nb * rt_row_bytes<DT_IN>());            // num_records: the chunk's rows, in bytes
  rin.w = 0x00020000;
  rout = __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)ohi << 32) | olo), 0, (int)(nb * rt_row_bytes<DT_OUT>()),
                                           0x00020000);
}

// Lanes past the chunk's nb blocks read zeros and have their stores dropped by the range check.
template <int DT_IN, int DT_OUT, uint32_t WB, int U>
__global__ __launch_bounds__(256) void k_roundtrip_list_fixed(const RtListDirect* __restrict__ desc, Params p)
{
  using DTab = typename RtDecTab<WB>::T;
  __shared__ __attribute__((aligned(16))) uint32_t tab[1280 + 1024];
  __shared__ __attribute__((aligned(16))) uint32_t dtab32[sizeof(DTab) / 4];
  pipe_v4i rin;
  __amdgpu_buffer_rsrc_t rout;
  uint32_t nb;
  rtl_resources<DT_IN, DT_OUT>(desc, rin, rout, nb);
  rt_fixed_chunk<DT_IN, DT_OUT, WB, U>(rin, rout, threadIdx.x, p, tab, dtab32);
}

template <int DT_IN, int DT_OUT, bool COUNT, int U>
__global__ __launch_bounds__(256) void k_roundtrip_list_var(const RtListDirect* __restrict__ desc, Params p,
                                                            uint64_t* total)
{
  __shared__ uint32_t cnt_sh[4];
  pipe_v4i rin;
  __amdgpu_buffer_rsrc_t rout;
  uint32_t nb;
  rtl_resources<DT_IN, DT_OUT>(desc, rin, rout, nb);
  const uint32_t lsum = rt_var_chunk<DT_IN, DT_OUT, COUNT, U>(rin, rout, threadIdx.x, nb, p);
  if constexpr (COUNT) rt_count(lsum, cnt_sh, total);
}

// ------------------------------------------------------------------------------------------------ gather chunks
enum { kRtlLean64 = 0, kRtlLean32 = 1, kRtlVar = 2, kRtlGeneric = 3 };

// One workgroup per chunk, each lane the blocks i = threadIdx.x + 256 k of it. A lane finds the segment of its block's
// first value by bisection between the segments of the chunk's first and last value (RtListGather: at most
// log2(chunk values) steps however many one-value tensors there are), then walks forward: segments are non-empty, so
// four values cross at most three seams. All four (padded: encode.c:41-60) values are read before any is written and
// only real values are written, so a tensor may be its own output. Lanes past the chunk code a zero block and neither
// load nor store: the block functions run with every lane active.
template <int DT_IN, int DT_OUT, int DOM, int U>
__global__ __launch_bounds__(256) void k_roundtrip_list_gather(const RtListGather* __restrict__ chunks,
                                                               const RtListSeg* __restrict__ segs, uint64_t nvals,
                                                               Params p, uint64_t* total)
{
  __shared__ uint32_t cnt_sh[4];
  constexpr bool LEAN = DOM == kRtlLean64 || DOM == kRtlLean32;
  constexpr uint32_t WB = DOM == kRtlLean32 ? 32u : 64u;
  using DTab = typename RtDecTab<WB>::T;
  __shared__ __attribute__((aligned(16))) uint32_t tab[LEAN ? 1280 + 1024 : 4];
  __shared__ __attribute__((aligned(16))) uint32_t dtab32[LEAN ? sizeof(DTab) / 4 : 4];
  if constexpr (LEAN) {  // the tables of rt_fixed_chunk, by plain loads
    for (uint32_t t = threadIdx.x; t < 1280u; t += 256u) tab[t] = g_plane_tab5.v[t];
    for (uint32_t t = threadIdx.x; t < 1024u; t += 256u) tab[1280u + t] = rspread_entry(t);
    const uint32_t* dsrc = (const uint32_t*)RtDecTab<WB>::ptr();
    for (uint32_t t = threadIdx.x; t < sizeof(DTab) / 4; t += 256u) dtab32[t] = dsrc[t];
    __syncthreads();
  }
  constexpr uint32_t OE = DT_OUT == DT_BF16 ? 2u : 4u;
  const RtListGather c = chunks[blockIdx.x];
  const uint64_t nblocks = (nvals + 3) / 4;
  const uint32_t nb = (uint32_t)min<uint64_t>(kRtListChunkBlocks, nblocks - c.b0);
  uint32_t lsum = 0;
#pragma unroll 1
  for (int k = 0; k < U; k++) {
    const uint32_t i = threadIdx.x + 256u * k;
    const bool act = i < nb;
    const uint64_t x0 = 4ull * ((uint64_t)c.b0 + i);
    const uint32_t nv = act ? (uint32_t)min<uint64_t>(4, nvals - x0) : 0u;
    float f[4] = {0.f, 0.f, 0.f, 0.f}, d[4];
    char* o[4] = {nullptr, nullptr, nullptr, nullptr};
    if (act) {
      uint32_t lo = c.seg_lo, hi = c.seg_hi;
      while (lo < hi) {  // the last segment that starts at or before x0
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (segs[mid].start <= x0) lo = mid;
        else hi = mid - 1u;
      }
      uint32_t s = lo;
      uint64_t s0 = segs[s].start, s1 = segs[s + 1].start;  // the sentinel ends the table: start = nvals
      const char* ip = (const char*)segs[s].in;
      char* op = (char*)segs[s].out;
#pragma unroll
      for (uint32_t x = 0; x < 4u; x++) {
        if (x < nv) {
          const uint64_t xi = x0 + x;
          while (xi >= s1) {
            s++;
            s0 = s1;
            s1 = segs[s + 1].start;
            ip = (const char*)segs[s].in;
            op = (char*)segs[s].out;
          }
          f[x] = load_elem<DT_IN>(ip, (int64_t)(xi - s0));
          o[x] = op + (xi - s0) * OE;
        }
      }
      // pad_index (field_io.h) written out: 1 -> v0 v0 v0 v0, 2 -> v0 v1 v1 v0, 3 -> v0 v1 v2 v0
      if (nv < 2u) f[1] = f[0];
      if (nv < 3u) f[2] = nv == 2u ? f[1] : f[0];
      if (nv < 4u) f[3] = f[0];
    }
    uint32_t len;
    if constexpr (LEAN) {
      rt_fixed_code<WB>(f, tab, dtab32, p, d);
      len = WB;
    } else if constexpr (DOM == kRtlVar) {
      len = rt_var_code(f, p, d);
    } else {
      len = rt_block_generic(f, p, d);
    }
    lsum += act ? len : 0u;
#pragma unroll
    for (uint32_t x = 0; x < 4u; x++)
      if (x < nv) {
        if constexpr (DT_OUT == DT_BF16) *(uint16_t*)o[x] = (uint16_t)bf16_rne(d[x]);
        else *(float*)o[x] = d[x];
      }
  }
  if (total) rt_count(lsum, cnt_sh, total);  // total: a kernel argument, uniform over the workgroup
}

// ---------------------------------------------------------------------------------------------- minexp from the device
// gcow_roundtrip_list_fitted_device (include/gcow.h): the two no-budget kernels under
// Params{1, 16658, maxprec, clamp(*d_minexp)}, the word read when the kernel runs (fitted_params_dev, var1d_prep.h).
// Twins with their own argument lists, as in roundtrip1d.hip, so that the host-parameter kernels above keep their
// code. The bit count is always taken. In the direct kernel the word is read and waited for ahead of rt_var_chunk's
// first asm row load (fitted_params_dev<true>), and the descriptor's words are scalar loads the compiler waits for
// itself: the rule of rt_var_block (N = U - 1 for every block) holds as it stands. The gather kernel has no
// hand-counted wait; its blocks are located by rtl_gather_block (rtlist_gather.h), the text of the loop above.
template <int DT_IN, int DT_OUT, int U>
__global__ __launch_bounds__(256) void k_roundtrip_list_var_fitted(const RtListDirect* __restrict__ desc,
                                                                   uint32_t maxprec,
                                                                   const int32_t* __restrict__ d_minexp,
                                                                   uint64_t* total)
{
  __shared__ uint32_t cnt_sh[4];
  const Params p = fitted_params_dev<true>(maxprec, d_minexp);
  pipe_v4i rin;
  __amdgpu_buffer_rsrc_t rout;
  uint32_t nb;
  rtl_resources<DT_IN, DT_OUT>(desc, rin, rout, nb);
  const uint32_t lsum = rt_var_chunk<DT_IN, DT_OUT, true, U>(rin, rout, threadIdx.x, nb, p);
  rt_count(lsum, cnt_sh, total);
}

template <int DT_IN, int DT_OUT, int U>
__global__ __launch_bounds__(256) void k_roundtrip_list_gather_fitted(const RtListGather* __restrict__ chunks,
                                                                      const RtListSeg* __restrict__ segs,
                                                                      uint64_t nvals, uint32_t maxprec,
                                                                      const int32_t* __restrict__ d_minexp,
                                                                      uint64_t* total)
{
  __shared__ uint32_t cnt_sh[4];
  const Params p = fitted_params_dev<false>(maxprec, d_minexp);
  constexpr uint32_t OE = DT_OUT == DT_BF16 ? 2u : 4u;
  const RtListGather c = chunks[blockIdx.x];
  const uint64_t nblocks = (nvals + 3) / 4;
  const uint32_t nb = (uint32_t)min<uint64_t>(kRtListChunkBlocks, nblocks - c.b0);
  uint32_t lsum = 0;
#pragma unroll 1
  for (int k = 0; k < U; k++) {
    const uint32_t i = threadIdx.x + 256u * k;
    const bool act = i < nb;
    float f[4] = {0.f, 0.f, 0.f, 0.f}, d[4];
    char* o[4] = {nullptr, nullptr, nullptr, nullptr};
    const uint32_t nv = rtl_gather_block<DT_IN, OE>(c, segs, nvals, i, act, f, o);  // all read before any is written
    const uint32_t len = rt_var_code(f, p, d);  // lanes past the chunk code a zero block
    lsum += act ? len : 0u;
#pragma unroll
    for (uint32_t x = 0; x < 4u; x++)
      if (x < nv) {
        if constexpr (DT_OUT == DT_BF16) *(uint16_t*)o[x] = (uint16_t)bf16_rne(d[x]);
        else *(float*)o[x] = d[x];
      }
  }
  rt_count(lsum, cnt_sh, total);
}

// ------------------------------------------------------------------------------------------------ launchers
template <int DT_IN, int DT_OUT>
static void launch_rtl_fitted_t(const RtListHeader& h, const char* d_plan, uint32_t maxprec, const int32_t* d_minexp,
                                uint64_t* total, hipStream_t st)
{
  constexpr int U = GCOW_RT_U;
  const RtListDirect* dd = (const RtListDirect*)(d_plan + h.off_direct);
  const RtListGather* gg = (const RtListGather*)(d_plan + h.off_gather);
  const RtListSeg* ss = (const RtListSeg*)(d_plan + h.off_segs);
  if (h.ndirect) k_roundtrip_list_var_fitted<DT_IN, DT_OUT, U><<<h.ndirect, 256, 0, st>>>(dd, maxprec, d_minexp, total);
  if (h.ngather)
    k_roundtrip_list_gather_fitted<DT_IN, DT_OUT, U><<<h.ngather, 256, 0, st>>>(gg, ss, h.nvals, maxprec, d_minexp,
                                                                               total);
}

template <int DT_IN, int DT_OUT>
static void launch_rtl_t(const RtListHeader& h, const char* d_plan, const Params& p, uint64_t* total, hipStream_t st)
{
  constexpr int U = GCOW_RT_U;
  const RtListDirect* dd = (const RtListDirect*)(d_plan + h.off_direct);
  const RtListGather* gg = (const RtListGather*)(d_plan + h.off_gather);
  const RtListSeg* ss = (const RtListSeg*)(d_plan + h.off_segs);
  const bool w64 = p.maxbits == 64;
  if (h.ndirect) {
    if (h.domain == kRoundtripLean) {
      if (w64) k_roundtrip_list_fixed<DT_IN, DT_OUT, 64, U><<<h.ndirect, 256, 0, st>>>(dd, p);
      else k_roundtrip_list_fixed<DT_IN, DT_OUT, 32, U><<<h.ndirect, 256, 0, st>>>(dd, p);
    } else if (total) {
      k_roundtrip_list_var<DT_IN, DT_OUT, true, U><<<h.ndirect, 256, 0, st>>>(dd, p, total);
    } else {
      k_roundtrip_list_var<DT_IN, DT_OUT, false, U><<<h.ndirect, 256, 0, st>>>(dd, p, nullptr);
    }
  }
  if (h.ngather) {
    if (h.domain == kRoundtripLean) {
      if (w64) k_roundtrip_list_gather<DT_IN, DT_OUT, kRtlLean64, U><<<h.ngather, 256, 0, st>>>(gg, ss, h.nvals, p, total);
      else k_roundtrip_list_gather<DT_IN, DT_OUT, kRtlLean32, U><<<h.ngather, 256, 0, st>>>(gg, ss, h.nvals, p, total);
    } else if (h.domain == kRoundtripVar) {
      k_roundtrip_list_gather<DT_IN, DT_OUT, kRtlVar, U><<<h.ngather, 256, 0, st>>>(gg, ss, h.nvals, p, total);
    } else {
      k_roundtrip_list_gather<DT_IN, DT_OUT, kRtlGeneric, U><<<h.ngather, 256, 0, st>>>(gg, ss, h.nvals, p, total);
    }
  }
}

hipError_t launch_roundtrip_list1d(const RtListHeader& h, const void* d_plan, const Params& p, uint64_t* total,
                                   void* stream)
{
  hipStream_t st = (hipStream_t)stream;
  const char* dp = (const char*)d_plan;
  if (h.in_dtype == DT_F32) {
    if (h.out_dtype == DT_F32) launch_rtl_t<DT_F32, DT_F32>(h, dp, p, total, st);
    else launch_rtl_t<DT_F32, DT_BF16>(h, dp, p, total, st);
  } else {
    if (h.out_dtype == DT_F32) launch_rtl_t<DT_BF16, DT_F32>(h, dp, p, total, st);
    else launch_rtl_t<DT_BF16, DT_BF16>(h, dp, p, total, st);
  }
  return hipGetLastError();
}

// h.domain == kRoundtripVar (the caller has checked it): the plan's direct chunks are the no-budget kernel's
hipError_t launch_roundtrip_list1d_fitted(const RtListHeader& h, const void* d_plan, uint32_t maxprec,
                                          const int32_t* d_minexp, uint64_t* total, void* stream)
{
  hipStream_t st = (hipStream_t)stream;
  const char* dp = (const char*)d_plan;
  if (h.in_dtype == DT_F32) {
    if (h.out_dtype == DT_F32) launch_rtl_fitted_t<DT_F32, DT_F32>(h, dp, maxprec, d_minexp, total, st);
    else launch_rtl_fitted_t<DT_F32, DT_BF16>(h, dp, maxprec, d_minexp, total, st);
  } else {
    if (h.out_dtype == DT_F32) launch_rtl_fitted_t<DT_BF16, DT_F32>(h, dp, maxprec, d_minexp, total, st);
    else launch_rtl_fitted_t<DT_BF16, DT_BF16>(h, dp, maxprec, d_minexp, total, st);
  }
  return hipGetLastError();
}

}  // namespace gcow
