// roundtrip_rel1d.hip -- the fused no-budget round trip (roundtrip1d.hip k_roundtrip1d_var) of every tensor of a list
// as a field of its own, with a tolerance relative to that tensor (gcow_roundtrip_rel_device, include/gcow.h):
// tensor s is coded under expert(1, 16658, maxprec, minexp_s), minexp_s = max(emax_s - rel_bits, -94), where emax_s is
// the block-exponent (biased exponent - 126) of the tensor's largest finite magnitude a_s (and, for emax_s = 128 only,
// minexp_s capped so that the decode stays finite: rel_params). Nothing is synchronised
// with the host: a first pass leaves a_s in absmax[s] and the round trip kernels read it from there.
//   k_rel_init       absmax[0 .. nsegs) = 0 and *total = 0, in stream order
//   k_rel_absmax     one pass over all values, one workgroup per plan chunk. |x| is taken as integer bits with Inf / NaN
//                    masked to 0, so the unsigned maximum is the maximum magnitude. A direct chunk (one tensor) loads
//                    its rows as the round trip does (16-byte fp32 rows, 8-byte bf16 rows, zeros past the chunk),
//                    reduces over the workgroup and issues one atomicMax; a gather chunk reduces per wave where the
//                    wave's blocks lie in one tensor, else per lane
//   k_roundtrip_rel_direct   one workgroup per RtRelDirect: rt_var_chunk (roundtrip1d.h) unchanged, its Params built
//                    once per workgroup from the tensor's slot of absmax (a uniform load, then scalar arithmetic)
//   k_roundtrip_rel_gather   one workgroup per RtRelGather (kRtRelGatherBlocks = 256 blocks: one per lane, so that the
//                    dependent loads of the bisection run in as many workgroups as there are): the lane finds its block's
//                    tensor by bisection, loads its up to four values one by one, pads a partial block
//                    (encode.c:41-60), reads all before it writes any and writes only real values. A block never
//                    crosses a tensor. The block function is rt_var_code with the lane's own Params
// The results are bit for bit those of gcow_roundtrip_device on each tensor under its parameter set.
// The two round trip kernels are templates over the source of that set (RelFromAbsmax / RelFromWord below): the second
// instance is gcow_roundtrip_rel_fitted_device, tensor s under clamp(d_minexp[s * stride], -154, 133) from device memory
// (a budget per tensor: rate_table_rel1d.hip writes the tables, k_rate_table_fit the words). It has no
// first pass: *total is zeroed by k_rel_init and the coders run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>
#include <utility>

#include "field_io.h"
#include "rel_locate.h"
#include "rel_minexp.h"
#include "roundtrip1d.h"
#include "var1d_prep.h"

namespace gcow {

static_assert(kRtListChunkBlocks == 256u * GCOW_RT_U, "the plan's chunk is the workgroup's chunk");
static_assert(kRtRelGatherBlocks <= kRtListChunkBlocks, "a gather chunk fits the workgroup's U rounds");

typedef unsigned int rel_v2u __attribute__((ext_vector_type(2)));
typedef unsigned int rel_v4u __attribute__((ext_vector_type(4)));

// The tensor's parameter set from its largest finite magnitude (as bits): minexp by rel_minexp (rel_minexp.h, the one
// definition of the rule: the floor at -94 and the headroom cap of a maximum in the top binade are explained there).
__device__ __forceinline__ Params rel_params(uint32_t a, uint32_t rel_bits, uint32_t maxprec)
{
  return Params{1u, 16658u, maxprec, rel_minexp(a, rel_bits)};
}

// Where a tensor's parameter set comes from. Both kernels below are templates over it, called once per workgroup
// (uniform: the direct kernel) or once per block (raw, then params: the gather kernel, whose lanes past the chunk code a
// zero block under params(0)).
//   RelFromAbsmax   the relative form: rel_params of the tensor's slot of absmax. The slot's address is uniform, so the
//                   load is scalar and none that rt_var_chunk's hand-counted vmcnt waits count.
//   RelFromWord     the fitted form (gcow_roundtrip_rel_fitted_device): minexp = clamp(d_minexp[seg * stride], -154, 133),
//                   the word read when the kernel runs. Direct: seg has gone through readfirstlane, so the address is
//                   uniform, and fitted_params_dev<true> has the word waited for ahead of rt_var_chunk's first asm row
//                   load (the rule is stated there, var1d_prep.h). Gather: one word per lane, the same clamp.
struct RelFromAbsmax {
  const uint32_t* __restrict__ absmax;
  uint32_t rel_bits, maxprec;
  __device__ __forceinline__ Params uniform(uint32_t seg) const
  {
    return rel_params(rel_uniform(absmax[seg]), rel_bits, maxprec);
  }
  __device__ __forceinline__ uint32_t raw(uint32_t seg) const { return absmax[seg]; }
  __device__ __forceinline__ Params params(uint32_t raw) const { return rel_params(raw, rel_bits, maxprec); }
};

struct RelFromWord {
  const int32_t* __restrict__ d_minexp;
  uint32_t stride, maxprec;  // stride in 4-byte words: 4 for an array of gcow_fit, 1 for packed words
  __device__ __forceinline__ Params uniform(uint32_t seg) const
  {
    return fitted_params_dev<true>(maxprec, d_minexp + (uint64_t)seg * stride);
  }
  __device__ __forceinline__ uint32_t raw(uint32_t seg) const { return (uint32_t)d_minexp[(uint64_t)seg * stride]; }
  __device__ __forceinline__ Params params(uint32_t raw) const
  {
    return Params{1u, 16658u, maxprec, min(max((int)raw, kFitMinExpLo), kFitMinExpHi)};
  }
};
static_assert(sizeof(RelFromAbsmax) == 16 && sizeof(RelFromWord) == 16, "one pointer and two words of kernel arguments");

__global__ __launch_bounds__(256) void k_rel_init(uint32_t* __restrict__ absmax, uint32_t nsegs, uint64_t* total)
{
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nsegs; i += gridDim.x * 256u) absmax[i] = 0u;
  if (total && blockIdx.x == 0 && threadIdx.x == 0) *total = 0ull;
}

// ------------------------------------------------------------------------------------------------ the maximum
// The gather chunks come first in the grid: their lanes chase dependent loads (the bisection), and started last they
// would run on alone after the direct chunks have drained.
template <int DT_IN, int U>
__global__ __launch_bounds__(256) void k_rel_absmax(const RtRelDirect* __restrict__ desc,
                                                    const RtRelGather* __restrict__ chunks, uint32_t ngather,
                                                    const RtRelPiece* __restrict__ pieces, uint32_t* absmax)
{
  __shared__ uint32_t sh[4];
  if (blockIdx.x >= ngather) {  // uniform over the workgroup
    constexpr uint32_t IB = rt_row_bytes<DT_IN>();
    const RtRelDirect* d = desc + (blockIdx.x - ngather);
    const uint64_t in = d->in;
    const uint32_t nb = min(rel_uniform(d->nb), kRtListChunkBlocks), seg = rel_uniform(d->seg);
    const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(((uint64_t)rel_uniform((uint32_t)(in >> 32)) << 32) | rel_uniform((uint32_t)in)), 0, (int)(nb * IB),
        0x00020000);
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < U; k++) {  // rows past the chunk read zeros
      const int off = (int)((threadIdx.x + 256u * k) * IB);
      if constexpr (DT_IN == DT_BF16) {
        const rel_v2u v = __builtin_amdgcn_raw_buffer_load_b64(rin, off, 0, 0);
        m = max(max(m, rel_mag(v.x << 16)), max(rel_mag(v.x & 0xffff0000u), rel_mag(v.y << 16)));
        m = max(m, rel_mag(v.y & 0xffff0000u));
      } else {
        const rel_v4u v = __builtin_amdgcn_raw_buffer_load_b128(rin, off, 0, 0);
        m = max(max(m, rel_mag(v.x)), max(rel_mag(v.y), max(rel_mag(v.z), rel_mag(v.w))));
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t mm = max(max(sh[0], sh[1]), max(sh[2], sh[3]));
      if (mm) atomicMax(absmax + seg, mm);  // the slot was zeroed: a zero maximum has nothing to add
    }
    return;
  }
  const RtRelGather c = chunks[blockIdx.x];
#pragma unroll 1
  for (int k = 0; k < U && 256u * k < c.nb; k++) {  // c.nb: uniform over the workgroup
    const uint32_t i = threadIdx.x + 256u * k;
    uint32_t m = 0, seg = 0;
    if (i < c.nb) {
      const RelBlock b = rel_locate(c, pieces, i);
      seg = b.seg;
      for (uint32_t x = 0; x < b.nv; x++)
        m = max(m, rel_mag(__float_as_uint(load_elem<DT_IN>(b.in, (int64_t)(b.x0 + x)))));
    }
    // lanes with m = 0 have nothing to add; where the others of the wave share a tensor, one atomic serves them
    const uint64_t need = __ballot(m != 0u);
    if (need == 0ull) continue;
    const uint32_t sref = (uint32_t)__shfl((int)seg, __ffsll((unsigned long long)need) - 1, 64);
    if (__all(m == 0u || seg == sref)) {
      uint32_t w = m;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) w = max(w, (uint32_t)__shfl_xor((int)w, o, 64));
      if ((threadIdx.x & 63u) == 0) atomicMax(absmax + sref, w);
    } else if (m != 0u) {
      atomicMax(absmax + seg, m);
    }
  }
}

// ------------------------------------------------------------------------------------------------ direct chunks
// Lanes past the chunk's nb blocks read zeros and have their stores dropped by the range check (rt_var_chunk).
template <int DT_IN, int DT_OUT, bool COUNT, int U, class PS>
__global__ __launch_bounds__(256) void k_roundtrip_rel_direct(const RtRelDirect* __restrict__ desc, PS ps,
                                                              uint64_t* total)
{
  __shared__ uint32_t cnt_sh[4];
  const RtRelDirect* d = desc + blockIdx.x;
  const uint64_t in = d->in, out = d->out;
  const uint32_t ilo = rel_uniform((uint32_t)in), ihi = rel_uniform((uint32_t)(in >> 32));
  const uint32_t olo = rel_uniform((uint32_t)out), ohi = rel_uniform((uint32_t)(out >> 32));
  const uint32_t nb = min(rel_uniform(d->nb), kRtListChunkBlocks);
  pipe_v4i rin;
  rin.x = (int)ilo;
  rin.y = (int)(ihi & 0xffffu);               // stride 0
  rin.z = (int)(nb * rt_row_bytes<DT_IN>());   // num_records: the chunk's rows, in bytes
  rin.w = 0x00020000;
  const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(((uint64_t)ohi << 32) | olo), 0, (int)(nb * rt_row_bytes<DT_OUT>()), 0x00020000);
  // the tensor's slot or word: the descriptor's address is uniform, so is this load's
  const Params p = ps.uniform(rel_uniform(d->seg));
  const uint32_t lsum = rt_var_chunk<DT_IN, DT_OUT, COUNT, U>(rin, rout, threadIdx.x, nb, p);
  if constexpr (COUNT) rt_count(lsum, cnt_sh, total);
}

// ------------------------------------------------------------------------------------------------ gather chunks
// Lanes past the chunk code a zero block and neither load nor store: the block function runs with every lane active.
template <int DT_IN, int DT_OUT, int U, class PS>
__global__ __launch_bounds__(256) void k_roundtrip_rel_gather(const RtRelGather* __restrict__ chunks,
                                                              const RtRelPiece* __restrict__ pieces, PS ps,
                                                              uint64_t* total)
{
  __shared__ uint32_t cnt_sh[4];
  constexpr uint32_t OE = DT_OUT == DT_BF16 ? 2u : 4u;
  const RtRelGather c = chunks[blockIdx.x];
  uint32_t lsum = 0;
#pragma unroll 1
  for (int k = 0; k < U && 256u * k < c.nb; k++) {  // c.nb: uniform over the workgroup
    const uint32_t i = threadIdx.x + 256u * k;
    const bool act = i < c.nb;
    float f[4] = {0.f, 0.f, 0.f, 0.f}, d[4];
    char* o = nullptr;
    uint32_t nv = 0, a = 0;
    if (act) {
      const RelBlock b = rel_locate(c, pieces, i);
      nv = b.nv;
      a = ps.raw(b.seg);
      o = b.out + b.x0 * OE;
#pragma unroll
      for (uint32_t x = 0; x < 4u; x++)
        if (x < nv) f[x] = load_elem<DT_IN>(b.in, (int64_t)(b.x0 + x));
      // pad_index (field_io.h) written out: 1 -> v0 v0 v0 v0, 2 -> v0 v1 v1 v0, 3 -> v0 v1 v2 v0
      if (nv < 2u) f[1] = f[0];
      if (nv < 3u) f[2] = nv == 2u ? f[1] : f[0];
      if (nv < 4u) f[3] = f[0];
    }
    const Params p = ps.params(a);
    const uint32_t len = rt_var_code(f, p, d);
    lsum += act ? len : 0u;
#pragma unroll
    for (uint32_t x = 0; x < 4u; x++)
      if (x < nv) {
        if constexpr (DT_OUT == DT_BF16) ((uint16_t*)o)[x] = (uint16_t)bf16_rne(d[x]);
        else ((float*)o)[x] = d[x];
      }
  }
  if (total) rt_count(lsum, cnt_sh, total);  // total: a kernel argument, uniform over the workgroup
}

// ------------------------------------------------------------------------------------------------ launchers
template <int DT_IN, int DT_OUT, class PS>
static void launch_rel_coders(const RtRelHeader& h, const char* d_plan, PS ps, uint64_t* total, hipStream_t st)
{
  constexpr int U = GCOW_RT_U;
  const RtRelDirect* dd = (const RtRelDirect*)(d_plan + h.off_direct);
  const RtRelGather* gg = (const RtRelGather*)(d_plan + h.off_gather);
  const RtRelPiece* pp = (const RtRelPiece*)(d_plan + h.off_pieces);
  if (h.ndirect) {
    if (total) k_roundtrip_rel_direct<DT_IN, DT_OUT, true, U, PS><<<h.ndirect, 256, 0, st>>>(dd, ps, total);
    else k_roundtrip_rel_direct<DT_IN, DT_OUT, false, U, PS><<<h.ndirect, 256, 0, st>>>(dd, ps, nullptr);
  }
  if (h.ngather) k_roundtrip_rel_gather<DT_IN, DT_OUT, U, PS><<<h.ngather, 256, 0, st>>>(gg, pp, ps, total);
}

template <int DT_IN, int DT_OUT>
static void launch_rel_t(const RtRelHeader& h, const char* d_plan, uint32_t rel_bits, uint32_t maxprec,
                         uint32_t* absmax, uint64_t* total, hipStream_t st)
{
  const RtRelDirect* dd = (const RtRelDirect*)(d_plan + h.off_direct);
  const RtRelGather* gg = (const RtRelGather*)(d_plan + h.off_gather);
  const RtRelPiece* pp = (const RtRelPiece*)(d_plan + h.off_pieces);
  k_rel_absmax<DT_IN, GCOW_RT_U><<<h.ngather + h.ndirect, 256, 0, st>>>(dd, gg, h.ngather, pp, absmax);
  launch_rel_coders<DT_IN, DT_OUT>(h, d_plan, RelFromAbsmax{absmax, rel_bits, maxprec}, total, st);
}

hipError_t launch_roundtrip_rel1d(const RtRelHeader& h, const void* d_plan, uint32_t rel_bits, uint32_t maxprec,
                                  uint32_t* absmax, uint64_t* total, void* stream)
{
  hipStream_t st = (hipStream_t)stream;
  if (h.nsegs || total)
    k_rel_init<<<std::max(1u, std::min((h.nsegs + 255u) / 256u, 64u)), 256, 0, st>>>(absmax, h.nsegs, total);
  if (h.ndirect + h.ngather) {
    const char* dp = (const char*)d_plan;
    if (h.in_dtype == DT_F32) {
      if (h.out_dtype == DT_F32) launch_rel_t<DT_F32, DT_F32>(h, dp, rel_bits, maxprec, absmax, total, st);
      else launch_rel_t<DT_F32, DT_BF16>(h, dp, rel_bits, maxprec, absmax, total, st);
    } else {
      if (h.out_dtype == DT_F32) launch_rel_t<DT_BF16, DT_F32>(h, dp, rel_bits, maxprec, absmax, total, st);
      else launch_rel_t<DT_BF16, DT_BF16>(h, dp, rel_bits, maxprec, absmax, total, st);
    }
  }
  return hipGetLastError();
}

// The fitted form: *total = 0 in stream order (k_rel_init over no slots), then the two coders under RelFromWord.
hipError_t launch_roundtrip_rel1d_fitted(const RtRelHeader& h, const void* d_plan, uint32_t maxprec,
                                         const int32_t* d_minexp, uint32_t stride_words, uint64_t* total, void* stream)
{
  hipStream_t st = (hipStream_t)stream;
  if (total) k_rel_init<<<1, 256, 0, st>>>(nullptr, 0u, total);
  if (h.ndirect + h.ngather) {
    const char* dp = (const char*)d_plan;
    const RelFromWord ps{d_minexp, stride_words, maxprec};
    if (h.in_dtype == DT_F32) {
      if (h.out_dtype == DT_F32) launch_rel_coders<DT_F32, DT_F32>(h, dp, ps, total, st);
      else launch_rel_coders<DT_F32, DT_BF16>(h, dp, ps, total, st);
    } else {
      if (h.out_dtype == DT_F32) launch_rel_coders<DT_BF16, DT_F32>(h, dp, ps, total, st);
      else launch_rel_coders<DT_BF16, DT_BF16>(h, dp, ps, total, st);
    }
  }
  return hipGetLastError();
}

}  // namespace gcow
