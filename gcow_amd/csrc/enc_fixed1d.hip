// enc_fixed1d.hip -- the fused fixed-rate 1-D encoder (the headline kernel): one 4-value block per lane, block b at
// bits [b * maxbits, ...) (sw/src/zfp.c:31-56 loop + sw/src/encode.c:41-495; hw/src/zfp.cpp:31-75 dataflow stages).
//   k_encode_fixed1d_np       one-shot grid, the lean-6 closed-form coder (whole-word blocks, kmin = 0)
//   k_encode_fixed1d_generic  parameters outside the lean coder's domain
//   k_encode_fixed1d_tail     the partial last block
//   k_copy_pattern1d          the memory floor of the same access pattern (bench.py roofline.copy_ceiling)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>

#include "codec_device.h"
#include "enc_fixed1d.h"
#include "field_io.h"
#include "kernels.h"
#include "lean1d.h"
#include "pipe.h"

// ---- tunables (A/B builds: tools/build_variant.sh NAME "-DGCOW_C2_U=4" enc_fixed1d.hip)
#ifndef GCOW_C2_U
#define GCOW_C2_U 8  // blocks per lane of the one-shot grid
#endif

namespace gcow {

// One-shot (non-persistent) fixed-rate 1-D encoder: each lane codes U blocks 256 apart inside its workgroup's chunk
// of 256 U blocks. All U loads are issued first (before the LDS table fill), then each block waits for its own load
// only: with U loads followed by k stores outstanding, load k has landed once at most U - 1 operations remain
// (vmcnt counts loads and stores together, in issue order). Out-of-range lanes read zeros and their stores are
// dropped by the buffer range check, so control flow stays wave-uniform. Measured against a persistent grid-stride
// pipeline (tools/ubench/legacy_variants.hip), the one-shot shape streams HBM like a plain copy kernel (DESIGN.md
// section 6). The raw loads, stores and counted waits are in pipe.h.
template <int DT, uint32_t WB, int U, uint32_t T = 256, int V = 0>
__global__ __launch_bounds__(T) void k_encode_fixed1d_np(const void* __restrict__ in, uint32_t nfull, Params p,
                                                         void* __restrict__ out)
{
  __shared__ __attribute__((aligned(16))) uint32_t tab[1280 + 1024];  // pair table, then the four window spread tables
  constexpr uint32_t IB = DT == DT_BF16 ? 8u : 16u;  // input bytes per block
  const pipe_v4i rin = buf_rsrc(in, nfull * IB), rout = buf_rsrc(out, nfull * (WB / 8));
  const uint32_t b0 = blockIdx.x * (T * U) + threadIdx.x;
  typename PipeRow<DT>::T r[U];
  if constexpr ((V & 1) != 0) {
    // pair-table loads issued first (hand-counted like the data loads), so waiting for them is vmcnt(U) and block 0
    // can start as soon as its own load lands (a compiler-issued table load after the data loads waits vmcnt(0))
    static_assert(T == 256, "table fill assumes 256 threads");
    constexpr int NT = 1280 / 256;
    const pipe_v4i rt = buf_rsrc(&g_plane_tab5, sizeof(PlaneTab2));
    uint32_t tv[NT];
#pragma unroll
    for (int i = 0; i < NT; i++) tv[i] = buf_load_u32((threadIdx.x + 256u * i) * 4u, rt);
#pragma unroll
    for (int k = 0; k < U; k++) r[k] = PipeRow<DT>::load((b0 + T * k) * IB, rin);
#pragma unroll
    for (uint32_t t = threadIdx.x; t < 1024; t += T) tab[1280 + t] = rspread_entry(t);
    asm volatile("s_waitcnt vmcnt(%5)" : "+v"(tv[0]), "+v"(tv[1]), "+v"(tv[2]), "+v"(tv[3]), "+v"(tv[4]) : "n"(U)
                 : "memory");
#pragma unroll
    for (int i = 0; i < NT; i++) tab[threadIdx.x + 256u * i] = tv[i];
  } else {
#pragma unroll
    for (int k = 0; k < U; k++) r[k] = PipeRow<DT>::load((b0 + T * k) * IB, rin);
#pragma unroll
    for (uint32_t t = threadIdx.x; t < 1280; t += T) tab[t] = g_plane_tab5.v[t];
    // the spread tables are computed, not loaded: entry 256 i + b = byte b reversed onto nibble bit i
#pragma unroll
    for (uint32_t t = threadIdx.x; t < 1024; t += T) tab[1280 + t] = rspread_entry(t);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < U; k++) {
    pipe_wait<U - 1>(r[k]);
    float f[4];
    PipeRow<DT>::unpack(r[k], f);
    bool special;
    uint64_t w = encode_block1d_lean6<WB, (V & 2) != 0>(f, tab, tab + 1280, special);
    if (special) {
      RegWriter64 rw{0ull, 0u};
      encode_block<1>(rw, f, p);
      w = WB == 64 ? rw.acc : (rw.acc & ((1ull << WB) - 1ull));
    }
    pipe_store<WB>((b0 + T * k) * (WB / 8), rout, w);
  }
}

// The memory floor of the fixed-rate 1-D encoder's access pattern (bench.py `roofline.copy_ceiling`): the same
// one-shot grid, U = 8 blocks per lane, the same raw buffer loads (16 B fp32 / 8 B bf16 per block) and WB-bit
// non-temporal stores with the same hand-counted waits, and no coding (each block's store is an xor-fold of its load).
template <int DT, uint32_t WB, int U>
__global__ __launch_bounds__(256) void k_copy_pattern1d(const void* __restrict__ in, uint32_t nfull,
                                                        void* __restrict__ out)
{
  constexpr uint32_t T = 256;
  constexpr uint32_t IB = DT == DT_BF16 ? 8u : 16u;
  const pipe_v4i rin = buf_rsrc(in, nfull * IB), rout = buf_rsrc(out, nfull * (WB / 8));
  const uint32_t b0 = blockIdx.x * (T * U) + threadIdx.x;
  typename PipeRow<DT>::T r[U];
#pragma unroll
  for (int k = 0; k < U; k++) r[k] = PipeRow<DT>::load((b0 + T * k) * IB, rin);
#pragma unroll
  for (int k = 0; k < U; k++) {
    pipe_wait<U - 1>(r[k]);
    float f[4];
    PipeRow<DT>::unpack(r[k], f);
    const uint64_t w = ((uint64_t)(__float_as_uint(f[0]) ^ __float_as_uint(f[1])) << 32) |
                       (__float_as_uint(f[2]) ^ __float_as_uint(f[3]));
    pipe_store<WB>((b0 + T * k) * (WB / 8), rout, w);
  }
}

// Generic fixed-rate 1-D encoder over the full 4-value blocks [0, nfull) for parameters outside the lean coder's
// domain (maxprec < 32 or minexp > -154: kmin > 0 possible); two blocks per lane, loads issued first.
template <int DT, uint32_t WB>
__global__ __launch_bounds__(256) void k_encode_fixed1d_generic(const void* __restrict__ in, uint32_t nfull, Params p,
                                                                void* __restrict__ out)
{
  __shared__ uint16_t tab[80];
  if (threadIdx.x < 80) tab[threadIdx.x] = plane_entry4(threadIdx.x);
  __syncthreads();
  constexpr int U = 2;
  const uint32_t b0 = blockIdx.x * (256u * U) + threadIdx.x;
  float f[U][4];
#pragma unroll
  for (int j = 0; j < U; j++) {
    const uint32_t b = b0 + 256u * j;
    if (b < nfull) load_row4<DT>(in, 4ll * b, f[j]);
  }
#pragma unroll
  for (int j = 0; j < U; j++) {
    const uint32_t b = b0 + 256u * j;
    if (b < nfull) {
      const uint64_t w = encode_block1d_fixed<WB>(f[j], p, tab);
      if constexpr (WB == 64) ((uint64_t*)out)[b] = w;
      else ((uint32_t*)out)[b] = (uint32_t)w;
    }
  }
}

// The partial last block of a 1-D bucket (nvals % 4 != 0): padded gather (encode.c:41-60), one lane.
template <int DT, uint32_t WB>
__global__ void k_encode_fixed1d_tail(const void* __restrict__ in, uint64_t nvals, uint32_t b, Params p,
                                      void* __restrict__ out)
{
  __shared__ uint16_t tab[80];
  if (threadIdx.x < 80) tab[threadIdx.x] = plane_entry4(threadIdx.x);
  __syncthreads();
  if (threadIdx.x) return;
  float f[4];
  load_block1d<DT>(in, nvals, b, f);
  const uint64_t w = encode_block1d_fixed<WB>(f, p, tab);
  if constexpr (WB == 64) ((uint64_t*)out)[b] = w;
  else ((uint32_t*)out)[b] = (uint32_t)w;
}

// ------------------------------------------------------------------------------------------------ launchers
static inline hipStream_t S(void* s) { return (hipStream_t)s; }

template <int DT, uint32_t WB>
static void launch_fixed1d_t(const void* in, uint64_t nvals, const Params& p, void* out, hipStream_t st)
{
  const uint32_t nfull = (uint32_t)(nvals / 4);
  if (nfull) {
    // the lean coder needs prec >= 32 for every nonzero block: e >= -126 => e - minexp + 4 >= 32
    const bool kmin0 = p.maxprec >= 32 && p.minexp <= -154;
    if (!kmin0) {
      k_encode_fixed1d_generic<DT, WB><<<(nfull + 511) / 512, 256, 0, st>>>(in, nfull, p, out);
    } else {
      // one-shot grid, U = 8 blocks per lane; chunks keep every buffer offset below 2^32
      constexpr uint32_t CH = 1u << 27;
      constexpr uint32_t IB = DT == DT_BF16 ? 8u : 16u;
      for (uint32_t c0 = 0; c0 < nfull; c0 += CH) {
        const uint32_t nc = min(CH, nfull - c0);
        const void* ic = (const char*)in + (size_t)c0 * IB;
        void* oc = (char*)out + (size_t)c0 * (WB / 8);
        constexpr int U = GCOW_C2_U;
        k_encode_fixed1d_np<DT, WB, U, 256, 3><<<(nc + 256 * U - 1) / (256 * U), 256, 0, st>>>(ic, nc, p, oc);
      }
    }
  }
  if (nvals % 4) k_encode_fixed1d_tail<DT, WB><<<1, 128, 0, st>>>(in, nvals, nfull, p, out);
}

hipError_t launch_copy_pattern1d(const void* in, int dtype, uint64_t nvals, uint32_t wb, void* out, void* stream)
{
  const uint32_t nfull = (uint32_t)(nvals / 4);
  constexpr uint32_t CH = 1u << 27;
  const uint32_t IB = dtype == DT_BF16 ? 8u : 16u;
  for (uint32_t c0 = 0; c0 < nfull; c0 += CH) {
    const uint32_t nc = std::min(CH, nfull - c0);
    const void* ic = (const char*)in + (size_t)c0 * IB;
    void* oc = (char*)out + (size_t)c0 * (wb / 8);
    const uint32_t g = (nc + 2047) / 2048;
    if (dtype == DT_BF16) {
      if (wb == 64) k_copy_pattern1d<DT_BF16, 64, 8><<<g, 256, 0, S(stream)>>>(ic, nc, oc);
      else k_copy_pattern1d<DT_BF16, 32, 8><<<g, 256, 0, S(stream)>>>(ic, nc, oc);
    } else {
      if (wb == 64) k_copy_pattern1d<DT_F32, 64, 8><<<g, 256, 0, S(stream)>>>(ic, nc, oc);
      else k_copy_pattern1d<DT_F32, 32, 8><<<g, 256, 0, S(stream)>>>(ic, nc, oc);
    }
  }
  return hipGetLastError();
}

hipError_t launch_encode_fixed1d(const void* in, int dtype, uint64_t nvals, uint32_t nblocks, const Params& p,
                                 void* out, void* stream)
{
  (void)nblocks;
  hipStream_t st = S(stream);
  if (dtype == DT_F32) {
    if (p.maxbits == 64) launch_fixed1d_t<DT_F32, 64>(in, nvals, p, out, st);
    else launch_fixed1d_t<DT_F32, 32>(in, nvals, p, out, st);
  } else {
    if (p.maxbits == 64) launch_fixed1d_t<DT_BF16, 64>(in, nvals, p, out, st);
    else launch_fixed1d_t<DT_BF16, 32>(in, nvals, p, out, st);
  }
  return hipGetLastError();
}

}  // namespace gcow
