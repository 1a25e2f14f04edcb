// roundtrip1d.hip -- out = decode(encode(in)) of a contiguous 1-D field in one pass, no stream written
// (gcow_roundtrip_device, include/gcow.h): what the reference's training loop does with zfpy.compress_numpy followed
// at once by zfpy.decompress_numpy (hw/models/train_imagenet.py:448-475). Every block's round trip is independent of
// every other block's, so there is no length scan, no block index and no workspace.
//   k_roundtrip1d_fixed_np   the lean fixed-rate domain (whole-word blocks, kmin = 0), the one-shot grid of
//                            k_encode_resid1d_np: the word (encode_block1d_lean6) decoded from its register
//                            (decode_block1d_pair / _fast); one row read and one row written per block
//   k_roundtrip1d_var        blocks that no budget truncates (minbits <= 1, maxbits >= 160): the decoded coefficients
//                            are the coded ones with the planes below kmin cleared (v1_prep gives both), so there is
//                            no embedded coder at all; Inf / NaN blocks take the generic function in their lane
//   k_roundtrip1d_generic    every other parameter set, buffers off 16-byte alignment and the partial last block of
//                            every path: encode_block<1> into three registers, decode_block<1> from them
// The bit length of the stream that was not written (COUNT) is summed per workgroup and added to *total.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>
#include <type_traits>
#include <utility>

#include "field_io.h"
#include "roundtrip1d.h"

namespace gcow {

// ------------------------------------------------------------------------------------------------ (a) lean fixed rate
// The one-shot grid of k_encode_resid1d_np (each lane U blocks 256 apart inside its workgroup's chunk of 256 U blocks)
// without the error rows and without the stream store. Table loads are requested first (the encoder's pair table as 5
// dwords per lane, the decoder's table as 3 16-byte chunks per lane), then the U row loads; the tables are waited for
// with vmcnt(U), which leaves the rows in flight. in and out may be the same buffer when the dtypes are equal: a lane
// reads the rows of its own blocks only, all of them before its first store. Out-of-range lanes read zeros, code a
// zero block and their stores are dropped by the buffer range check, so control flow stays wave-uniform.
// (The text of rt_fixed_chunk, roundtrip1d.h, kept in the kernel: called through that function, five of the eight
// instantiations here allocate one more VGPR.)
template <int DT_IN, int DT_OUT, uint32_t WB, int U>
__global__ __launch_bounds__(256) void k_roundtrip1d_fixed_np(const void* in, uint32_t nfull, Params p, void* out)
{
  using DTab = typename RtDecTab<WB>::T;
  __shared__ __attribute__((aligned(16))) uint32_t tab[1280 + 1024];
  __shared__ __attribute__((aligned(16))) uint32_t dtab32[sizeof(DTab) / 4];
  constexpr uint32_t IB = rt_row_bytes<DT_IN>(), OB = rt_row_bytes<DT_OUT>();
  const pipe_v4i rin = buf_rsrc(in, nfull * IB);
  const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)(nfull * OB), 0x00020000);
  const uint32_t b0 = blockIdx.x * (256u * U) + threadIdx.x;
  constexpr int NT = 1280 / 256;
  constexpr uint32_t TCH = sizeof(DTab) / 16, TR = (TCH + 255) / 256;
  static_assert(TR == 3, "three decode-table chunks per lane");
  const pipe_v4i rt = buf_rsrc(&g_plane_tab5, sizeof(PlaneTab2));
  const pipe_v4i rdt = buf_rsrc(RtDecTab<WB>::ptr(), sizeof(DTab));
  uint32_t tv[NT];
#pragma unroll
  for (int i = 0; i < NT; i++) tv[i] = buf_load_u32((threadIdx.x + 256u * i) * 4u, rt);
  pipe_v4u dv[TR];
#pragma unroll
  for (uint32_t i = 0; i < TR; i++) dv[i] = buf_load_b128((threadIdx.x + 256u * i) * 16u, rdt);
  typename PipeRow<DT_IN>::T rx[U];
#pragma unroll
  for (int k = 0; k < U; k++) rx[k] = PipeRow<DT_IN>::load((b0 + 256u * k) * IB, rin);
#pragma unroll
  for (uint32_t t = threadIdx.x; t < 1024; t += 256) tab[1280 + t] = rspread_entry(t);
  // the U row loads are behind the table loads
  asm volatile("s_waitcnt vmcnt(%5)" : "+v"(tv[0]), "+v"(tv[1]), "+v"(tv[2]), "+v"(tv[3]), "+v"(tv[4]) : "n"(U)
               : "memory");
  table_wait<U>(dv);
#pragma unroll
  for (int i = 0; i < NT; i++) tab[threadIdx.x + 256u * i] = tv[i];
#pragma unroll
  for (uint32_t i = 0; i < TR; i++)
    if (threadIdx.x + 256u * i < TCH) ((pipe_v4u*)dtab32)[threadIdx.x + 256u * i] = dv[i];
  __syncthreads();
  rt_fixed_blocks<DT_IN, DT_OUT, WB, U>(std::make_integer_sequence<int, U>{}, rx, tab, dtab32, p, b0, rout);
}

// ------------------------------------------------------------------------------------------------ (b) no budget
// The same one-shot grid (rt_var_chunk); in and out may be the same buffer when the dtypes are equal, as above.
template <int DT_IN, int DT_OUT, bool COUNT, int U = GCOW_RT_U>
__global__ __launch_bounds__(256) void k_roundtrip1d_var(const void* in, uint32_t nfull, Params p, void* out,
                                                         uint64_t* total)
{
  __shared__ uint32_t cnt_sh[4];
  constexpr uint32_t IB = rt_row_bytes<DT_IN>(), OB = rt_row_bytes<DT_OUT>();
  const pipe_v4i rin = buf_rsrc(in, nfull * IB);
  const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)(nfull * OB), 0x00020000);
  const uint32_t b0 = blockIdx.x * (256u * U) + threadIdx.x;
  const uint32_t lsum = rt_var_chunk<DT_IN, DT_OUT, COUNT, U>(rin, rout, b0, nfull, p);
  if constexpr (COUNT) rt_count(lsum, cnt_sh, total);
}

// ------------------------------------------------------------------------------------------------ (c) generic
// One lane per block, blocks b0 .. b0 + nb - 1 of a field of nvals values (any alignment; the last block may be
// partial: the padded gather of encode.c:41-60, and only its real values are written). A lane reads its block's values
// before it writes them, so in and out may be the same buffer when the dtypes are equal.
template <int DT_IN, int DT_OUT>
__global__ __launch_bounds__(256) void k_roundtrip1d_generic(const void* in, uint64_t nvals, uint64_t b0, uint64_t nb,
                                                             Params p, void* out, uint64_t* total)
{
  __shared__ uint32_t cnt_sh[4];
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  uint32_t len = 0;
  if (i < nb) {
    const uint64_t x0 = 4ull * (b0 + i);
    const uint32_t nv = (uint32_t)min<uint64_t>(4, nvals - x0);
    float f[4], d[4];
#pragma unroll
    for (uint32_t x = 0; x < 4u; x++) f[x] = load_elem<DT_IN>(in, (int64_t)(x0 + pad_index(x, nv)));
    len = rt_block_generic(f, p, d);
#pragma unroll
    for (uint32_t x = 0; x < 4u; x++)
      if (x < nv) {
        if constexpr (DT_OUT == DT_BF16) ((uint16_t*)out)[x0 + x] = (uint16_t)bf16_rne(d[x]);
        else ((float*)out)[x0 + x] = d[x];
      }
  }
  if (total) rt_count(len, cnt_sh, total);  // total: a kernel argument, uniform over the workgroup
}

// ------------------------------------------------------------------------------------------------ minexp from the device
// gcow_roundtrip_fitted_device (include/gcow.h): kernels (b) and (c) under
// Params{1, 16658, maxprec, clamp(*d_minexp)}, the word read when the kernel runs (fitted_params_dev, var1d_prep.h).
// rt_var_chunk issues its U row loads from inline asm and waits vmcnt(U - 1) per block by hand. The word is loaded and
// waited for before the first of them is issued (fitted_params_dev<true>), and as a uniform load from a kernel argument
// it is a scalar load, which vmcnt does not count: the rule of rt_var_block (N = U - 1 for every block) holds as it
// stands. The generic kernel has no hand-counted wait.
template <int DT_IN, int DT_OUT, bool COUNT, int U = GCOW_RT_U>
__global__ __launch_bounds__(256) void k_roundtrip1d_var_fitted(const void* in, uint32_t nfull, uint32_t maxprec,
                                                                const int32_t* __restrict__ d_minexp, void* out,
                                                                uint64_t* total)
{
  __shared__ uint32_t cnt_sh[4];
  const Params p = fitted_params_dev<true>(maxprec, d_minexp);
  constexpr uint32_t IB = rt_row_bytes<DT_IN>(), OB = rt_row_bytes<DT_OUT>();
  const pipe_v4i rin = buf_rsrc(in, nfull * IB);
  const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)(nfull * OB), 0x00020000);
  const uint32_t b0 = blockIdx.x * (256u * U) + threadIdx.x;
  const uint32_t lsum = rt_var_chunk<DT_IN, DT_OUT, COUNT, U>(rin, rout, b0, nfull, p);
  if constexpr (COUNT) rt_count(lsum, cnt_sh, total);
}

template <int DT_IN, int DT_OUT>
__global__ __launch_bounds__(256) void k_roundtrip1d_generic_fitted(const void* in, uint64_t nvals, uint64_t b0,
                                                                    uint64_t nb, uint32_t maxprec,
                                                                    const int32_t* __restrict__ d_minexp, void* out,
                                                                    uint64_t* total)
{
  __shared__ uint32_t cnt_sh[4];
  const Params p = fitted_params_dev<false>(maxprec, d_minexp);
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  uint32_t len = 0;
  if (i < nb) {
    const uint64_t x0 = 4ull * (b0 + i);
    const uint32_t nv = (uint32_t)min<uint64_t>(4, nvals - x0);
    float f[4], d[4];
#pragma unroll
    for (uint32_t x = 0; x < 4u; x++) f[x] = load_elem<DT_IN>(in, (int64_t)(x0 + pad_index(x, nv)));
    len = rt_block_generic(f, p, d);
#pragma unroll
    for (uint32_t x = 0; x < 4u; x++)
      if (x < nv) {
        if constexpr (DT_OUT == DT_BF16) ((uint16_t*)out)[x0 + x] = (uint16_t)bf16_rne(d[x]);
        else ((float*)out)[x0 + x] = d[x];
      }
  }
  if (total) rt_count(len, cnt_sh, total);  // total: a kernel argument, uniform over the workgroup
}

// ------------------------------------------------------------------------------------------------ launchers
// One set for both parameter sources (ParamsHost / ParamsDev, var1d_prep.h): the source picks a kernel or its _fitted
// twin, which keep their own argument lists (as templates over the source their device code changed).
template <int DT_IN, int DT_OUT, class PS>
static void launch_rt_generic(const void* in, uint64_t nvals, uint64_t b0, uint64_t nb, const PS& ps, void* out,
                              uint64_t* total, hipStream_t st)
{
  constexpr uint64_t CH = 1ull << 30;  // blocks per launch: the grid stays below 2^31 workgroups
  for (uint64_t c0 = 0; c0 < nb; c0 += CH) {
    const uint64_t nc = std::min(CH, nb - c0);
    const uint32_t g = (uint32_t)((nc + 255) / 256);
    if constexpr (std::is_same<PS, ParamsHost>::value)
      k_roundtrip1d_generic<DT_IN, DT_OUT><<<g, 256, 0, st>>>(in, nvals, b0 + c0, nc, ps.p, out, total);
    else
      k_roundtrip1d_generic_fitted<DT_IN, DT_OUT><<<g, 256, 0, st>>>(in, nvals, b0 + c0, nc, ps.maxprec, ps.d_minexp,
                                                                     out, total);
  }
}

template <int DT_IN, int DT_OUT, bool COUNT, class PS>
static void launch_rt_var(const void* in, uint32_t nfull, const PS& ps, void* out, uint64_t* total, uint32_t g,
                          hipStream_t st)
{
  if constexpr (std::is_same<PS, ParamsHost>::value)
    k_roundtrip1d_var<DT_IN, DT_OUT, COUNT><<<g, 256, 0, st>>>(in, nfull, ps.p, out, total);
  else
    k_roundtrip1d_var_fitted<DT_IN, DT_OUT, COUNT><<<g, 256, 0, st>>>(in, nfull, ps.maxprec, ps.d_minexp, out, total);
}

// domain: ParamsHost any; ParamsDev kRoundtripVar or kRoundtripGeneric (the lean kernel is host-parameter only)
template <int DT_IN, int DT_OUT, class PS>
static void launch_rt_t(const void* in, uint64_t nvals, const PS& ps, int domain, void* out, uint64_t* total,
                        hipStream_t st)
{
  const uint64_t nblocks = (nvals + 3) / 4;
  if (domain == kRoundtripGeneric) {
    launch_rt_generic<DT_IN, DT_OUT>(in, nvals, 0, nblocks, ps, out, total, st);
    return;
  }
  const uint32_t nfull = (uint32_t)(nvals / 4);
  // chunks keep every offset into the two buffers below 2^32 (16 bytes per block at most)
  constexpr uint32_t CH = 1u << 27;
  constexpr uint32_t IB = rt_row_bytes<DT_IN>(), OB = rt_row_bytes<DT_OUT>();
  constexpr int U = GCOW_RT_U;
  for (uint32_t c0 = 0; c0 < nfull; c0 += CH) {
    const uint32_t nc = std::min(CH, nfull - c0);
    const void* ic = (const char*)in + (size_t)c0 * IB;
    void* oc = (char*)out + (size_t)c0 * OB;
    const uint32_t g = (nc + 256 * U - 1) / (256 * U);
    if (domain == kRoundtripLean) {
      if constexpr (std::is_same<PS, ParamsHost>::value) {
        if (ps.p.maxbits == 64) k_roundtrip1d_fixed_np<DT_IN, DT_OUT, 64, U><<<g, 256, 0, st>>>(ic, nc, ps.p, oc);
        else k_roundtrip1d_fixed_np<DT_IN, DT_OUT, 32, U><<<g, 256, 0, st>>>(ic, nc, ps.p, oc);
      }
    } else if (total) {
      launch_rt_var<DT_IN, DT_OUT, true>(ic, nc, ps, oc, total, g, st);
    } else {
      launch_rt_var<DT_IN, DT_OUT, false>(ic, nc, ps, oc, nullptr, g, st);
    }
  }
  if (nvals % 4) launch_rt_generic<DT_IN, DT_OUT>(in, nvals, nfull, 1, ps, out, total, st);
}

template <class PS>
static hipError_t launch_rt(const void* in, int in_dtype, uint64_t nvals, const PS& ps, int domain, void* out,
                            int out_dtype, uint64_t* total, void* stream)
{
  hipStream_t st = (hipStream_t)stream;
  if (in_dtype == DT_F32) {
    if (out_dtype == DT_F32) launch_rt_t<DT_F32, DT_F32>(in, nvals, ps, domain, out, total, st);
    else launch_rt_t<DT_F32, DT_BF16>(in, nvals, ps, domain, out, total, st);
  } else {
    if (out_dtype == DT_F32) launch_rt_t<DT_BF16, DT_F32>(in, nvals, ps, domain, out, total, st);
    else launch_rt_t<DT_BF16, DT_BF16>(in, nvals, ps, domain, out, total, st);
  }
  return hipGetLastError();
}

hipError_t launch_roundtrip1d(const void* in, int in_dtype, uint64_t nvals, const Params& p, int domain, void* out,
                              int out_dtype, uint64_t* total, void* stream)
{
  return launch_rt(in, in_dtype, nvals, ParamsHost{p}, domain, out, out_dtype, total, stream);
}

hipError_t launch_roundtrip1d_fitted(const void* in, int in_dtype, uint64_t nvals, uint32_t maxprec,
                                     const int32_t* d_minexp, bool rows16, void* out, int out_dtype, uint64_t* total,
                                     void* stream)
{
  return launch_rt(in, in_dtype, nvals, ParamsDev{maxprec, d_minexp}, rows16 ? kRoundtripVar : kRoundtripGeneric, out,
                   out_dtype, total, stream);
}

}  // namespace gcow
