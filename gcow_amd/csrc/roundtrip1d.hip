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
#include <utility>

#include "codec_device.h"
#include "dec1d.h"
#include "enc_fixed1d.h"
#include "field_io.h"
#include "kernels.h"
#include "lean1d.h"
#include "pipe.h"
#include "regbits.h"
#include "var1d_prep.h"

#ifndef GCOW_RT_U
#define GCOW_RT_U 8  // blocks per lane: U rows in flight (32 VGPRs at U = 8, fp32)
#endif

namespace gcow {

// ------------------------------------------------------------------------------------------------ shared pieces
// One decoded block as an output row: 16 bytes (fp32) or 8 bytes (bf16, each value rounded to nearest even as
// store_block1d does). The store goes through the compiler builtin: an inline-asm wide store after VALU writes stored
// stale lanes (enc_resid1d.hip resid_block, dec1d.hip k_decode_fixed1d_np). It counts in vmcnt once; aux 2 =
// non-temporal.
template <int DT_OUT>
__device__ __forceinline__ void rt_store_row(__amdgpu_buffer_rsrc_t rout, uint32_t b, const float* d)
{
  if constexpr (DT_OUT == DT_BF16) {
    pipe_v2u v;
    v.x = bf16x2_rne(d[0], d[1]);
    v.y = bf16x2_rne(d[2], d[3]);
    __builtin_amdgcn_raw_buffer_store_b64(v, rout, (int)(b * 8u), 0, 2);
  } else {
    pipe_v4u v;
    v.x = __float_as_uint(d[0]);
    v.y = __float_as_uint(d[1]);
    v.z = __float_as_uint(d[2]);
    v.w = __float_as_uint(d[3]);
    __builtin_amdgcn_raw_buffer_store_b128(v, rout, (int)(b * 16u), 0, 2);
  }
}

// Sum v over the workgroup's 256 lanes and add it to *total: one 64-bit atomic per workgroup.
__device__ __forceinline__ void rt_count(uint32_t v, uint32_t* sh, uint64_t* total)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd((unsigned long long*)total, (unsigned long long)sh[0] + sh[1] + sh[2] + sh[3]);
}

template <int DT> constexpr uint32_t rt_row_bytes() { return DT == DT_BF16 ? 8u : 16u; }

// ------------------------------------------------------------------------------------------------ (a) lean fixed rate
// LDS image: the encoder's pair table and spread tables (2304 words), then the decoder's table (64-bit blocks: the pair
// table, 12 KiB; 32-bit blocks: the plane table, 10 KiB).
template <uint32_t WB> struct RtDecTab {
  using T = typename std::conditional<WB == 64, DecTabP, DecTab1>::type;
  static __device__ __forceinline__ const void* ptr()
  {
    if constexpr (WB == 64) return &g_dec_pair;
    else return &g_dec_tab1;
  }
};

// One block of the one-shot kernel (K is a compile-time block number: the row registers are indexed by it).
// Waits: the lane issued its row loads in the order x_0 x_1 ... x_{U-1}, and every block before K issued one store
// (its output row). vmcnt counts loads and stores together in issue order, so once at most N operations are
// outstanding, everything but the last N issued has landed. Before block K, the operations issued after x_K are the
// later blocks' row loads, U - 1 - K of them, and the K stores: N = U - 1, the same for every block.
template <int DT_IN, int DT_OUT, uint32_t WB, int U, int K>
__device__ __forceinline__ void rt_fixed_block(typename PipeRow<DT_IN>::T (&rx)[U], const uint32_t* tab,
                                               const uint32_t* dtab32, const Params& p, uint32_t b0,
                                               __amdgpu_buffer_rsrc_t rout)
{
  pipe_wait<U - 1>(rx[K]);
  const uint32_t b = b0 + 256u * K;
  float f[4];
  PipeRow<DT_IN>::unpack(rx[K], f);  // coded as it is: -0 stays -0
  bool special;
  uint64_t w = encode_block1d_lean6<WB, true>(f, tab, tab + 1280, special);
  if (special) {
    RegWriter64 rw{0ull, 0u};
    encode_block<1>(rw, f, p);
    w = WB == 64 ? rw.acc : (rw.acc & ((1ull << WB) - 1ull));
  }
  float d[4];
  bool dspecial;
  if constexpr (WB == 64) decode_block1d_pair<false>(w, dtab32, d, dspecial);
  else decode_block1d_fast<WB>(w, (const uint16_t*)dtab32, d, dspecial);
  if (dspecial) {  // group phase longer than the window, or a plane code crossing the budget
    RegReader64 rd{w, 0u};
    decode_block<1>(rd, p, d);
  }
  rt_store_row<DT_OUT>(rout, b, d);
}

template <int DT_IN, int DT_OUT, uint32_t WB, int U, int... K>
__device__ __forceinline__ void rt_fixed_blocks(std::integer_sequence<int, K...>, typename PipeRow<DT_IN>::T (&rx)[U],
                                                const uint32_t* tab, const uint32_t* dtab32, const Params& p,
                                                uint32_t b0, __amdgpu_buffer_rsrc_t rout)
{
  (rt_fixed_block<DT_IN, DT_OUT, WB, U, K>(rx, tab, dtab32, p, b0, rout), ...);
}

// The one-shot grid of k_encode_resid1d_np (each lane U blocks 256 apart inside its workgroup's chunk of 256 U blocks)
// without the error rows and without the stream store. Table loads are requested first (the encoder's pair table as 5
// dwords per lane, the decoder's table as 3 16-byte chunks per lane), then the U row loads; the tables are waited for
// with vmcnt(U), which leaves the rows in flight. in and out may be the same buffer when the dtypes are equal: a lane
// reads the rows of its own blocks only, all of them before its first store. Out-of-range lanes read zeros, code a
// zero block and their stores are dropped by the buffer range check, so control flow stays wave-uniform.
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
// The decode is v1_decode_closed (var1d_prep.h) of what v1_prep returns; Inf / NaN blocks take rt_block_generic. Same
// wait rule as rt_fixed_block: N = U - 1 for every block.
template <int DT_IN, int DT_OUT, bool COUNT, int U, int K>
__device__ __forceinline__ void rt_var_block(typename PipeRow<DT_IN>::T (&rx)[U], const Params& p, uint32_t b0,
                                             uint32_t nfull, __amdgpu_buffer_rsrc_t rout, uint32_t& lsum)
{
  pipe_wait<U - 1>(rx[K]);
  const uint32_t b = b0 + 256u * K;
  float f[4], d[4];
  PipeRow<DT_IN>::unpack(rx[K], f);
  uint32_t u[4], hdr, Kp;
  bool inf;
  uint32_t len = v1_prep(f, -122 - p.minexp, (int)min(p.maxprec, 64u), u, hdr, Kp, inf);
  v1_decode_closed(u, hdr, Kp, d);
  if (inf) len = rt_block_generic(f, p, d);  // Inf / NaN present: cast and header follow the reference's integer path
  rt_store_row<DT_OUT>(rout, b, d);
  if constexpr (COUNT) lsum += b < nfull ? len : 0u;
}

template <int DT_IN, int DT_OUT, bool COUNT, int U, int... K>
__device__ __forceinline__ void rt_var_blocks(std::integer_sequence<int, K...>, typename PipeRow<DT_IN>::T (&rx)[U],
                                              const Params& p, uint32_t b0, uint32_t nfull,
                                              __amdgpu_buffer_rsrc_t rout, uint32_t& lsum)
{
  (rt_var_block<DT_IN, DT_OUT, COUNT, U, K>(rx, p, b0, nfull, rout, lsum), ...);
}

// The same one-shot grid; in and out may be the same buffer when the dtypes are equal, as above.
template <int DT_IN, int DT_OUT, bool COUNT, int U = GCOW_RT_U>
__global__ __launch_bounds__(256) void k_roundtrip1d_var(const void* in, uint32_t nfull, Params p, void* out,
                                                         uint64_t* total)
{
  __shared__ uint32_t cnt_sh[4];
  constexpr uint32_t IB = rt_row_bytes<DT_IN>(), OB = rt_row_bytes<DT_OUT>();
  const pipe_v4i rin = buf_rsrc(in, nfull * IB);
  const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)(nfull * OB), 0x00020000);
  const uint32_t b0 = blockIdx.x * (256u * U) + threadIdx.x;
  typename PipeRow<DT_IN>::T rx[U];
#pragma unroll
  for (int k = 0; k < U; k++) rx[k] = PipeRow<DT_IN>::load((b0 + 256u * k) * IB, rin);
  uint32_t lsum = 0;
  rt_var_blocks<DT_IN, DT_OUT, COUNT, U>(std::make_integer_sequence<int, U>{}, rx, p, b0, nfull, rout, lsum);
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

// ------------------------------------------------------------------------------------------------ launchers
template <int DT_IN, int DT_OUT>
static void launch_rt_generic(const void* in, uint64_t nvals, uint64_t b0, uint64_t nb, const Params& p, void* out,
                              uint64_t* total, hipStream_t st)
{
  constexpr uint64_t CH = 1ull << 30;  // blocks per launch: the grid stays below 2^31 workgroups
  for (uint64_t c0 = 0; c0 < nb; c0 += CH) {
    const uint64_t nc = std::min(CH, nb - c0);
    k_roundtrip1d_generic<DT_IN, DT_OUT><<<(uint32_t)((nc + 255) / 256), 256, 0, st>>>(in, nvals, b0 + c0, nc, p, out,
                                                                                      total);
  }
}

template <int DT_IN, int DT_OUT>
static void launch_rt_t(const void* in, uint64_t nvals, const Params& p, int domain, void* out, uint64_t* total,
                        hipStream_t st)
{
  const uint64_t nblocks = (nvals + 3) / 4;
  if (domain == kRoundtripGeneric) {
    launch_rt_generic<DT_IN, DT_OUT>(in, nvals, 0, nblocks, p, out, total, st);
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
      if (p.maxbits == 64) k_roundtrip1d_fixed_np<DT_IN, DT_OUT, 64, U><<<g, 256, 0, st>>>(ic, nc, p, oc);
      else k_roundtrip1d_fixed_np<DT_IN, DT_OUT, 32, U><<<g, 256, 0, st>>>(ic, nc, p, oc);
    } else if (total) {
      k_roundtrip1d_var<DT_IN, DT_OUT, true><<<g, 256, 0, st>>>(ic, nc, p, oc, total);
    } else {
      k_roundtrip1d_var<DT_IN, DT_OUT, false><<<g, 256, 0, st>>>(ic, nc, p, oc, nullptr);
    }
  }
  if (nvals % 4) launch_rt_generic<DT_IN, DT_OUT>(in, nvals, nfull, 1, p, out, total, st);
}

hipError_t launch_roundtrip1d(const void* in, int in_dtype, uint64_t nvals, const Params& p, int domain, void* out,
                              int out_dtype, uint64_t* total, void* stream)
{
  hipStream_t st = (hipStream_t)stream;
  if (in_dtype == DT_F32) {
    if (out_dtype == DT_F32) launch_rt_t<DT_F32, DT_F32>(in, nvals, p, domain, out, total, st);
    else launch_rt_t<DT_F32, DT_BF16>(in, nvals, p, domain, out, total, st);
  } else {
    if (out_dtype == DT_F32) launch_rt_t<DT_BF16, DT_F32>(in, nvals, p, domain, out, total, st);
    else launch_rt_t<DT_BF16, DT_BF16>(in, nvals, p, domain, out, total, st);
  }
  return hipGetLastError();
}

}  // namespace gcow
