// enc_resid1d.hip -- error feedback: the fixed-rate 1-D encode that also writes the residual of its own stream
// (gcow_encode_residual_device, include/gcow.h), and the two elementwise passes of the composed path.
//   k_encode_resid1d_np     the lean encoder's domain (whole-word blocks, kmin = 0), one-shot grid: per block
//                           y = x + e, the word (encode_block1d_lean6), the word decoded in registers
//                           (decode_block1d_pair / _fast), e' = finite(y - decode): 16 (8) + 16 bytes read, 8 (4) + 16
//                           written per block, where encode + decode + two torch passes move 144 (fp32, rate 16)
//   k_encode_resid1d_tail   the partial last block
//   k_resid_form            y = x + e               (composed path: what neither this kernel nor the variable-rate
//                                                   form in var1d.hip takes)
//   k_resid_finish          e' = finite(y - decode)
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
#include "var1d_prep.h"  // resid_bits

#ifndef GCOW_EF_U
#define GCOW_EF_U 8  // blocks per lane: 2 U rows in flight (64 VGPRs at U = 8, fp32)
#endif

namespace gcow {

// LDS image: the encoder's pair table and spread tables (2304 words), then the decoder's table (64-bit blocks: the pair
// table, 12 KiB; 32-bit blocks: the plane table, 10 KiB).
template <uint32_t WB> struct ResidDecTab {
  using T = typename std::conditional<WB == 64, DecTabP, DecTab1>::type;
  static __device__ __forceinline__ const void* ptr()
  {
    if constexpr (WB == 64) return &g_dec_pair;
    else return &g_dec_tab1;
  }
};

// One block of the one-shot kernel (K is a compile-time block number: the row registers are indexed by it and the
// wait below is counted from it).
// Waits: the lane issued its row loads in the order x_0 e_0 x_1 e_1 ... (HASE; else x_0 x_1 ...), and every block
// before K issued two stores (the word, then the residual row). vmcnt counts loads and stores together in issue order,
// so once at most N operations are outstanding, everything but the last N issued has landed. Before block K, the
// operations issued after e_K (without HASE: after x_K) are the later blocks' row loads, 2 (U - 1 - K) of them (without
// HASE: U - 1 - K), and the 2 K stores: N = 2 U - 2 with HASE -- the same for every block -- and U - 1 + K without.
template <int DT, uint32_t WB, int U, bool HASE, int K>
__device__ __forceinline__ void resid_block(typename PipeRow<DT>::T (&rx)[U], pipe_v4f (&re)[HASE ? U : 1],
                                            const uint32_t* tab, const uint32_t* dtab32, const Params& p, uint32_t b0,
                                            pipe_v4i rout, __amdgpu_buffer_rsrc_t rerr)
{
  constexpr int N = HASE ? 2 * U - 2 : U - 1 + K;
  if constexpr (HASE) {
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(rx[K]), "+v"(re[K]) : "n"(N) : "memory");
  } else {
    pipe_wait<N>(rx[K]);
  }
  const uint32_t b = b0 + 256u * K;
  float f[4], y[4];
  PipeRow<DT>::unpack(rx[K], f);
  if constexpr (HASE) {
    y[0] = __fadd_rn(f[0], re[K].x);
    y[1] = __fadd_rn(f[1], re[K].y);
    y[2] = __fadd_rn(f[2], re[K].z);
    y[3] = __fadd_rn(f[3], re[K].w);
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) y[i] = __fadd_rn(f[i], 0.0f);  // e = +0: -0 becomes +0 as in the model
  }
  bool special;
  uint64_t w = encode_block1d_lean6<WB, true>(y, tab, tab + 1280, special);
  if (special) {
    RegWriter64 rw{0ull, 0u};
    encode_block<1>(rw, y, p);
    w = WB == 64 ? rw.acc : (rw.acc & ((1ull << WB) - 1ull));
  }
  pipe_store<WB>(b * (WB / 8), rout, w);
  float d[4];
  bool dspecial;
  if constexpr (WB == 64) decode_block1d_pair<false>(w, dtab32, d, dspecial);
  else decode_block1d_fast<WB>(w, (const uint16_t*)dtab32, d, dspecial);
  if (dspecial) {  // group phase longer than the window, or a plane code crossing the budget
    RegReader64 rd{w, 0u};
    decode_block<1>(rd, p, d);
  }
  // the row store goes through the compiler (dec1d.hip k_decode_fixed1d_np: an inline-asm wide store after VALU writes
  // stored stale lanes); it counts in vmcnt once, as the waits assume; aux 2 = non-temporal
  pipe_v4u v;
  v.x = resid_bits(y[0], d[0]);
  v.y = resid_bits(y[1], d[1]);
  v.z = resid_bits(y[2], d[2]);
  v.w = resid_bits(y[3], d[3]);
  __builtin_amdgcn_raw_buffer_store_b128(v, rerr, (int)(b * 16u), 0, 2);
}

template <int DT, uint32_t WB, int U, bool HASE, int... K>
__device__ __forceinline__ void resid_blocks(std::integer_sequence<int, K...>, typename PipeRow<DT>::T (&rx)[U],
                                             pipe_v4f (&re)[HASE ? U : 1], const uint32_t* tab, const uint32_t* dtab32,
                                             const Params& p, uint32_t b0, pipe_v4i rout, __amdgpu_buffer_rsrc_t rerr)
{
  (resid_block<DT, WB, U, HASE, K>(rx, re, tab, dtab32, p, b0, rout, rerr), ...);
}

// The one-shot grid of k_encode_fixed1d_np (each lane U blocks 256 apart inside its workgroup's chunk of 256 U blocks)
// with a second input row and a second output row per block. Table loads are requested first (the encoder's pair table
// as 5 dwords per lane, the decoder's table as 3 16-byte chunks per lane), then the 2 U row loads; the tables are waited
// for with vmcnt(number of row loads), which leaves the rows in flight. e_in and e_out may be the same buffer: a lane
// reads the e rows of its own blocks only, all of them before its first store. Out-of-range lanes read zeros, code a
// zero block and their stores are dropped by the buffer range checks, so control flow stays wave-uniform.
template <int DT, uint32_t WB, int U, bool HASE>
__global__ __launch_bounds__(256) void k_encode_resid1d_np(const void* __restrict__ in, const float* e_in, float* e_out,
                                                           uint32_t nfull, Params p, void* __restrict__ out)
{
  using DTab = typename ResidDecTab<WB>::T;
  __shared__ __attribute__((aligned(16))) uint32_t tab[1280 + 1024];
  __shared__ __attribute__((aligned(16))) uint32_t dtab32[sizeof(DTab) / 4];
  constexpr uint32_t IB = DT == DT_BF16 ? 8u : 16u;
  const pipe_v4i rin = buf_rsrc(in, nfull * IB), rout = buf_rsrc(out, nfull * (WB / 8));
  const pipe_v4i rein = buf_rsrc(e_in, HASE ? nfull * 16u : 0u);
  const __amdgpu_buffer_rsrc_t rerr = __builtin_amdgcn_make_buffer_rsrc(e_out, 0, (int)(nfull * 16u), 0x00020000);
  const uint32_t b0 = blockIdx.x * (256u * U) + threadIdx.x;
  constexpr int NT = 1280 / 256;
  constexpr uint32_t TCH = sizeof(DTab) / 16, TR = (TCH + 255) / 256;
  static_assert(TR == 3, "three decode-table chunks per lane");
  const pipe_v4i rt = buf_rsrc(&g_plane_tab5, sizeof(PlaneTab2));
  const pipe_v4i rdt = buf_rsrc(ResidDecTab<WB>::ptr(), sizeof(DTab));
  uint32_t tv[NT];
#pragma unroll
  for (int i = 0; i < NT; i++) tv[i] = buf_load_u32((threadIdx.x + 256u * i) * 4u, rt);
  pipe_v4u dv[TR];
#pragma unroll
  for (uint32_t i = 0; i < TR; i++) dv[i] = buf_load_b128((threadIdx.x + 256u * i) * 16u, rdt);
  typename PipeRow<DT>::T rx[U];
  pipe_v4f re[HASE ? U : 1];
#pragma unroll
  for (int k = 0; k < U; k++) {
    rx[k] = PipeRow<DT>::load((b0 + 256u * k) * IB, rin);
    if constexpr (HASE) re[k] = PipeRow<DT_F32>::load((b0 + 256u * k) * 16u, rein);
  }
#pragma unroll
  for (uint32_t t = threadIdx.x; t < 1024; t += 256) tab[1280 + t] = rspread_entry(t);
  constexpr int NROW = HASE ? 2 * U : U;  // row loads behind the table loads
  asm volatile("s_waitcnt vmcnt(%5)" : "+v"(tv[0]), "+v"(tv[1]), "+v"(tv[2]), "+v"(tv[3]), "+v"(tv[4]) : "n"(NROW)
               : "memory");
  table_wait<NROW>(dv);
#pragma unroll
  for (int i = 0; i < NT; i++) tab[threadIdx.x + 256u * i] = tv[i];
#pragma unroll
  for (uint32_t i = 0; i < TR; i++)
    if (threadIdx.x + 256u * i < TCH) ((pipe_v4u*)dtab32)[threadIdx.x + 256u * i] = dv[i];
  __syncthreads();
  resid_blocks<DT, WB, U, HASE>(std::make_integer_sequence<int, U>{}, rx, re, tab, dtab32, p, b0, rout, rerr);
}

// The partial last block (nvals % 4 != 0), one lane: the padded gather of x and e (encode.c:41-60; the padding values
// are copies of real y values), the generic whole-word coder and decoder, and the real values' residuals only.
template <int DT, uint32_t WB>
__global__ void k_encode_resid1d_tail(const void* __restrict__ in, const float* e_in, float* e_out, uint64_t nvals,
                                      uint32_t b, Params p, void* __restrict__ out)
{
  __shared__ uint16_t tab[80];
  if (threadIdx.x < 80) tab[threadIdx.x] = plane_entry4(threadIdx.x);
  __syncthreads();
  if (threadIdx.x) return;
  const uint64_t i0 = 4ull * b;
  const uint32_t nv = (uint32_t)(nvals - i0);
  float y[4];
#pragma unroll
  for (int x = 0; x < 4; x++) {
    const uint64_t i = i0 + pad_index(x, nv);
    y[x] = __fadd_rn(load_elem<DT>(in, (int64_t)i), e_in ? e_in[i] : 0.0f);
  }
  const uint64_t w = encode_block1d_fixed<WB>(y, p, tab);
  if constexpr (WB == 64) ((uint64_t*)out)[b] = w;
  else ((uint32_t*)out)[b] = (uint32_t)w;
  RegReader64 rd{w, 0u};
  float d[4];
  decode_block<1>(rd, p, d);
#pragma unroll
  for (uint32_t x = 0; x < 4u; x++)
    if (x < nv) e_out[i0 + x] = __uint_as_float(resid_bits(y[x], d[x]));
}

// ------------------------------------------------------------------------------------------------ composed path
template <int DT>
__global__ __launch_bounds__(256) void k_resid_form(const void* __restrict__ in, const float* e_in, float* y,
                                                    uint64_t n)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) y[i] = __fadd_rn(load_elem<DT>(in, (int64_t)i), e_in ? e_in[i] : 0.0f);
}

// e holds the decode on entry
__global__ __launch_bounds__(256) void k_resid_finish(const float* __restrict__ y, float* e, uint64_t n)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) e[i] = __uint_as_float(resid_bits(y[i], e[i]));
}

// ------------------------------------------------------------------------------------------------ launchers
static inline hipStream_t S(void* s) { return (hipStream_t)s; }

template <int DT, uint32_t WB>
static void launch_resid1d_t(const void* in, const float* e_in, float* e_out, uint64_t nvals, const Params& p,
                             void* out, hipStream_t st)
{
  const uint32_t nfull = (uint32_t)(nvals / 4);
  // chunks keep every offset into the three buffers below 2^32 (16 bytes per block at most)
  constexpr uint32_t CH = 1u << 27;
  constexpr uint32_t IB = DT == DT_BF16 ? 8u : 16u;
  constexpr int U = GCOW_EF_U;
  for (uint32_t c0 = 0; c0 < nfull; c0 += CH) {
    const uint32_t nc = std::min(CH, nfull - c0);
    const void* ic = (const char*)in + (size_t)c0 * IB;
    void* oc = (char*)out + (size_t)c0 * (WB / 8);
    float* eo = e_out + (size_t)c0 * 4;
    const uint32_t g = (nc + 256 * U - 1) / (256 * U);
    if (e_in) k_encode_resid1d_np<DT, WB, U, true><<<g, 256, 0, st>>>(ic, e_in + (size_t)c0 * 4, eo, nc, p, oc);
    else k_encode_resid1d_np<DT, WB, U, false><<<g, 256, 0, st>>>(ic, nullptr, eo, nc, p, oc);
  }
  if (nvals % 4) k_encode_resid1d_tail<DT, WB><<<1, 128, 0, st>>>(in, e_in, e_out, nvals, nfull, p, out);
}

hipError_t launch_encode_resid1d(const void* in, int dtype, uint64_t nvals, const Params& p, const float* e_in,
                                 float* e_out, void* out, void* stream)
{
  hipStream_t st = S(stream);
  if (dtype == DT_F32) {
    if (p.maxbits == 64) launch_resid1d_t<DT_F32, 64>(in, e_in, e_out, nvals, p, out, st);
    else launch_resid1d_t<DT_F32, 32>(in, e_in, e_out, nvals, p, out, st);
  } else {
    if (p.maxbits == 64) launch_resid1d_t<DT_BF16, 64>(in, e_in, e_out, nvals, p, out, st);
    else launch_resid1d_t<DT_BF16, 32>(in, e_in, e_out, nvals, p, out, st);
  }
  return hipGetLastError();
}

hipError_t launch_resid_form(const void* in, int dtype, uint64_t nvals, const float* e_in, float* y, void* stream)
{
  if (!nvals) return hipSuccess;
  const uint32_t g = (uint32_t)((nvals + 255) / 256);
  if (dtype == DT_BF16) k_resid_form<DT_BF16><<<g, 256, 0, S(stream)>>>(in, e_in, y, nvals);
  else k_resid_form<DT_F32><<<g, 256, 0, S(stream)>>>(in, e_in, y, nvals);
  return hipGetLastError();
}

hipError_t launch_resid_finish(const float* y, float* e, uint64_t nvals, void* stream)
{
  if (!nvals) return hipSuccess;
  k_resid_finish<<<(uint32_t)((nvals + 255) / 256), 256, 0, S(stream)>>>(y, e, nvals);
  return hipGetLastError();
}

}  // namespace gcow
