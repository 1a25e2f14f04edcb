// roundtrip1d.h -- the block sequences of the fused 1-D round trip, shared by the contiguous-field kernels
// (roundtrip1d.hip) and the tensor-list kernels (roundtrip_list1d.hip): a workgroup of 256 lanes takes a chunk of
// 256 U blocks, each lane U blocks 256 apart, through two buffer resources whose range check covers the chunk's rows.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <type_traits>
#include <utility>

#include "codec_device.h"
#include "dec1d.h"
#include "enc_fixed1d.h"
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

// One block's word decoded from its register (f: the block's values as they are: -0 stays -0).
template <uint32_t WB>
__device__ __forceinline__ void rt_fixed_code(const float* f, const uint32_t* tab, const uint32_t* dtab32,
                                              const Params& p, float* d)
{
  bool special;
  uint64_t w = encode_block1d_lean6<WB, true>(f, tab, tab + 1280, special);
  if (special) {
    RegWriter64 rw{0ull, 0u};
    encode_block<1>(rw, f, p);
    w = WB == 64 ? rw.acc : (rw.acc & ((1ull << WB) - 1ull));
  }
  bool dspecial;
  if constexpr (WB == 64) decode_block1d_pair<false>(w, dtab32, d, dspecial);
  else decode_block1d_fast<WB>(w, (const uint16_t*)dtab32, d, dspecial);
  if (dspecial) {  // group phase longer than the window, or a plane code crossing the budget
    RegReader64 rd{w, 0u};
    decode_block<1>(rd, p, d);
  }
}

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
  float d[4];
  rt_fixed_code<WB>(f, tab, dtab32, p, d);
  rt_store_row<DT_OUT>(rout, b, d);
}

template <int DT_IN, int DT_OUT, uint32_t WB, int U, int... K>
__device__ __forceinline__ void rt_fixed_blocks(std::integer_sequence<int, K...>, typename PipeRow<DT_IN>::T (&rx)[U],
                                                const uint32_t* tab, const uint32_t* dtab32, const Params& p,
                                                uint32_t b0, __amdgpu_buffer_rsrc_t rout)
{
  (rt_fixed_block<DT_IN, DT_OUT, WB, U, K>(rx, tab, dtab32, p, b0, rout), ...);
}

// A workgroup's whole chunk: table loads are requested first (the encoder's pair table as 5 dwords per lane, the
// decoder's table as 3 16-byte chunks per lane), then the U row loads of blocks b0, b0 + 256, ... of rin; the tables
// are waited for with vmcnt(U), which leaves the rows in flight. A lane reads the rows of its own blocks only, all of
// them before its first store, so rin and rout may cover the same memory when the dtypes are equal. Lanes past the
// resources' range read zeros, code a zero block and their stores are dropped by the buffer range check, so control
// flow stays wave-uniform. tab: 1280 + 1024 words of LDS, dtab32: sizeof(RtDecTab<WB>::T) bytes of LDS, both 16-byte
// aligned.
template <int DT_IN, int DT_OUT, uint32_t WB, int U>
__device__ __forceinline__ void rt_fixed_chunk(pipe_v4i rin, __amdgpu_buffer_rsrc_t rout, uint32_t b0, const Params& p,
                                               uint32_t* tab, uint32_t* dtab32)
{
  using DTab = typename RtDecTab<WB>::T;
  constexpr uint32_t IB = rt_row_bytes<DT_IN>();
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
// The decode is v1_decode_closed (var1d_prep.h) of what v1_prep returns; Inf / NaN blocks take rt_block_generic.
// Returns the block's bit length.
__device__ __forceinline__ uint32_t rt_var_code(const float* f, const Params& p, float* d)
{
  uint32_t u[4], hdr, Kp;
  bool inf;
  uint32_t len = v1_prep(f, -122 - p.minexp, (int)min(p.maxprec, 64u), u, hdr, Kp, inf);
  v1_decode_closed(u, hdr, Kp, d);
  if (inf) len = rt_block_generic(f, p, d);  // Inf / NaN present: cast and header follow the reference's integer path
  return len;
}

// Same wait rule as rt_fixed_block: N = U - 1 for every block.
template <int DT_IN, int DT_OUT, bool COUNT, int U, int K>
__device__ __forceinline__ void rt_var_block(typename PipeRow<DT_IN>::T (&rx)[U], const Params& p, uint32_t b0,
                                             uint32_t nfull, __amdgpu_buffer_rsrc_t rout, uint32_t& lsum)
{
  pipe_wait<U - 1>(rx[K]);
  const uint32_t b = b0 + 256u * K;
  float f[4], d[4];
  PipeRow<DT_IN>::unpack(rx[K], f);
  const uint32_t len = rt_var_code(f, p, d);
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

// A workgroup's whole chunk of nfull blocks behind rin / rout; returns the lane's sum of block lengths (COUNT).
template <int DT_IN, int DT_OUT, bool COUNT, int U>
__device__ __forceinline__ uint32_t rt_var_chunk(pipe_v4i rin, __amdgpu_buffer_rsrc_t rout, uint32_t b0, uint32_t nfull,
                                                 const Params& p)
{
  constexpr uint32_t IB = rt_row_bytes<DT_IN>();
  typename PipeRow<DT_IN>::T rx[U];
#pragma unroll
  for (int k = 0; k < U; k++) rx[k] = PipeRow<DT_IN>::load((b0 + 256u * k) * IB, rin);
  uint32_t lsum = 0;
  rt_var_blocks<DT_IN, DT_OUT, COUNT, U>(std::make_integer_sequence<int, U>{}, rx, p, b0, nfull, rout, lsum);
  return lsum;
}

}  // namespace gcow
