// dec1d.hip -- the 1-D decoders (block decoders and tables: dec1d.h).
//   k_decode_fixed1d_np            fixed rate, whole-word blocks: one-shot grid, hand-counted waits
//   k_decode_tail1d                the partial last block of a fixed-rate field
//   k_decode1d_var                 variable rate, one lane per index chunk, global-memory windows
//   k_decode1d_var_lean (_big)     variable rate, index every 16 blocks: the workgroup's span staged in LDS, by
//                                  stage capacity tier; groups whose span does not fit go to the second pass
//   launch_decode1d_var, launch_decode_fixed1d
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <type_traits>
#include <stdint.h>

#include "codec_device.h"
#include "dec1d.h"
#include "field_io.h"
#include "kernels.h"
#include "pipe.h"

// ---- tunables (A/B builds: tools/build_variant.sh)
#ifndef GCOW_C2DEC_U
#define GCOW_C2DEC_U 8  // k_decode_fixed1d_np, 64-bit blocks: words per lane (at 16 the pair loop keeps the block loop rolled)
#endif
#ifndef GCOW_VDEC_CAPB
#define GCOW_VDEC_CAPB 64  // k_decode1d_var_lean: stage capacity in bits per block when no tier is chosen
#endif
#ifndef GCOW_VDEC_BIGB
#define GCOW_VDEC_BIGB 144  // the second pass's stage: any span (a 1-D block codes at most 140 bits)
#endif

namespace gcow {

// One-shot fixed-rate 1-D decoder (the shape of k_encode_fixed1d_np): each lane decodes U blocks 256 apart inside
// its workgroup's chunk; the U word loads are issued before the table fill, and block k waits for its own word only
// (U loads then k stores outstanding: vmcnt(U - 1)).
template <uint32_t WB, int U, bool BF = false>
__global__ __launch_bounds__(256) void k_decode_fixed1d_np(const void* __restrict__ in, uint32_t nfull, Params p,
                                                           void* __restrict__ out, uint64_t base_bits)
{
  // 64-bit blocks: the two-plane table, at U = 8 (at U = 16 the unrolled pair loop keeps the block loop rolled, which
  // its counted waits cannot take; profiles/r04_dec_pair_table.log); 32-bit blocks: the one-plane table
  constexpr bool PAIR = WB == 64;
  // the delta-swap inverse transpose: gather tables measured +4.5 % steady here (-6 % cold; profiles/r05_dec_gather_ab.log)
  using PTab = DecTabP;
  using Tab = typename std::conditional<PAIR, PTab, DecTab1>::type;
  __shared__ __attribute__((aligned(16))) uint32_t dtab32[sizeof(Tab) / 4];
  const uint16_t* dtab = (const uint16_t*)dtab32;
  constexpr uint32_t WBYTES = WB / 8;
  const pipe_v4i rin = buf_rsrc((const char*)in + base_bits / 8, nfull * WBYTES);
  // output: 16 B per block (fp32), or 8 B (BF: bf16, rounded to nearest even)
  const __amdgpu_buffer_rsrc_t rout_b = __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)(nfull * (BF ? 8u : 16u)), 0x00020000);
  const uint32_t b0 = blockIdx.x * (256u * U) + threadIdx.x;
  // the plane table (10 KiB, 640 16-byte chunks; 64-bit blocks: the 12 KiB pair table and the 4 KiB gather tables,
  // 1024 chunks; 3-4 per lane, the range check zeroes the rest) is requested first and
  // waited for with vmcnt(U): the U word loads behind it stay in flight, and no wait counts a memory round trip per
  // table chunk (as a compiler-issued copy loop does)
  constexpr uint32_t TCH = sizeof(Tab) / 16, TR = (TCH + 255) / 256;
  const pipe_v4i rt = PAIR ? buf_rsrc(&g_dec_pair, sizeof(PTab)) : buf_rsrc(&g_dec_tab1, sizeof(DecTab1));
  pipe_v4u tv[TR];
#pragma unroll
  for (uint32_t i = 0; i < TR; i++) tv[i] = buf_load_b128((threadIdx.x + 256u * i) * 16u, rt);
  typename PipeWord<WB>::T r[U];
#pragma unroll
  for (int k = 0; k < U; k++) r[k] = PipeWord<WB>::load((b0 + 256u * k) * WBYTES, rin);
  table_wait<U>(tv);
#pragma unroll
  for (uint32_t i = 0; i < TR; i++)
    if (threadIdx.x + 256u * i < TCH) ((pipe_v4u*)dtab32)[threadIdx.x + 256u * i] = tv[i];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < U; k++) {
    pipe_wait<U - 1>(r[k]);
    const uint32_t b = b0 + 256u * k;
    float f[4];
    bool special;
    if constexpr (PAIR) decode_block1d_pair<false>(PipeWord<WB>::get(r[k]), dtab32, f, special);
    else decode_block1d_fast<WB>(PipeWord<WB>::get(r[k]), dtab, f, special);
    if (special && b < nfull) {
      BitReader rd{(const uint64_t*)in, base_bits + (uint64_t)b * WB};
      decode_block<1>(rd, p, f);
    }
    // 16-B (8-B) store through the compiler (it inserts the VALU-write -> wide-store wait states that an inline-asm
    // store would need by hand; with an asm store lanes 12-15 of each row stored stale data). It still counts in vmcnt
    // exactly once per block, as the hand-counted waits assume; aux 2 = non-temporal.
    if constexpr (BF) {
      pipe_v2u v;
      v.x = bf16x2_rne(f[0], f[1]);
      v.y = bf16x2_rne(f[2], f[3]);
      __builtin_amdgcn_raw_buffer_store_b64(v, rout_b, (int)(b * 8u), 0, 2);
    } else {
      pipe_v4u v;
      v.x = __float_as_uint(f[0]); v.y = __float_as_uint(f[1]); v.z = __float_as_uint(f[2]); v.w = __float_as_uint(f[3]);
      __builtin_amdgcn_raw_buffer_store_b128(v, rout_b, (int)(b * 16u), 0, 2);
    }
  }
}

__global__ __launch_bounds__(256) void k_decode1d_var(FieldDesc F, Params p, const uint64_t* __restrict__ in,
                                                      const uint64_t* __restrict__ index, uint32_t chunk,
                                                      uint64_t nchunks, uint64_t base_bits,
                                                      uint64_t* __restrict__ end_out)
{
  __shared__ __attribute__((aligned(16))) uint16_t dtab[5 * 128];  // r = 7 rows of the plane table
  stage_lds16<256, sizeof(DecTab7) / 16>(dtab, &g_dec_tab7, sizeof(DecTab7));
  __syncthreads();
  const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (c >= nchunks) return;
  uint64_t pos = base_bits + (index ? index[c] : 0ull);
  const uint64_t b0 = c * chunk, b1 = min<uint64_t>(b0 + chunk, F.nblocks);
  float* out = (float*)F.data;
  if (chunk == 16 && 4 * b1 <= F.n[0] && b1 - b0 == 16) {
    // the chunk's 256 output bytes are decoded into registers and stored in one burst: stored as they are decoded,
    // every 128-B line stays half-written in L2 for most of the chunk's decode time
    float g[16][4];
#pragma unroll
    for (int k = 0; k < 16; k++) decode_block1d_var(GlobalWindow{in}, pos, dtab, p.minexp, p.maxprec, g[k]);
    if (F.dtype == DT_BF16) {
#pragma unroll
      for (int k = 0; k < 16; k++) store_block1d(F, b0 + k, g[k]);
    } else {
#pragma unroll
      for (int k = 0; k < 16; k++) *(float4*)(out + 4 * (b0 + k)) = make_float4(g[k][0], g[k][1], g[k][2], g[k][3]);
    }
    if (end_out && c == nchunks - 1) *end_out = pos;
    return;
  }
  for (uint64_t b = b0; b < b1; b++) {
    float f[4];
    decode_block1d_var(GlobalWindow{in}, pos, dtab, p.minexp, p.maxprec, f);
    if (F.dtype != DT_BF16 && 4 * b + 4 <= F.n[0]) *(float4*)(out + 4 * b) = make_float4(f[0], f[1], f[2], f[3]);
    else store_block1d(F, b, f);
  }
  if (end_out && c == nchunks - 1) *end_out = pos;
}

// One lane per 16-block index chunk, LANES chunks per workgroup, the workgroup's stream span staged in LDS (one round
// trip, stage_lds16). A lane decodes its chunk in two rounds of eight blocks; an 8 x 8 transpose across each group of
// 8 lanes (DPP) then gives lane 8q + m block m of the group's chunk 8q + i for i = 0..7, so every store instruction
// writes whole 128-byte lines (8 lanes x 16 bytes of one chunk). Stored as decoded -- each lane's 16 bytes 256 bytes
// apart, 64 lines per instruction -- the stores alone cost as much as the decode: 1 GiB in 0.37 ms against 0.19 ms
// for full-line instructions (tools/ubench/store_pattern.hip, modes 1 / 4).
// The stage is sized for 64 bits per block on average (accuracy 1e-6 on gradient-scale data codes ~63), which sets the
// occupancy (LDS-bound: 4.5 waves per SIMD at 64 bits, 3.5 at 80 -- C5 bucket 0.469 against 0.535 ms,
// profiles/r04_var_decode_occupancy_ab.log). A workgroup whose span does not fit (a higher rate), partial chunks and
// strided outputs take the general path (global-memory windows; staging such a workgroup in 2 or 4 parts instead
// measured slower on the common path, profiles/r04_var_decode_parts_negative.log).

// Stage capacity in stream words: the main kernel's (GCOW_VDEC_CAPB bits per block on average) and the second pass's
// (any span: a 1-D block codes at most 140 bits, plus the 16-byte alignment of the span's start)
template <uint32_t LANES, uint32_t CAPB = GCOW_VDEC_CAPB> constexpr uint32_t vdec_cap() { return LANES * 16 * CAPB / 64; }
template <uint32_t LANES> constexpr uint32_t vdec_cap_big() { return LANES * 16 * GCOW_VDEC_BIGB / 64; }

// A group of LANES index chunks (one workgroup's work) whose span does not fit the main kernel's stage, and which is
// whole (no partial chunk or block) with a contiguous output: left by the main kernel to k_decode1d_var_lean_big.
// Not the last group: its span ends at the stream's end, which the index does not give (the buffer's end bounds it),
// so it takes the main kernel's general path.
template <uint32_t LANES>
__device__ __forceinline__ bool vdec_left_to_big_w(const FieldDesc& F, const uint64_t* index, uint64_t in_words,
                                                   uint64_t nchunks, uint64_t base_bits, uint64_t c0, uint64_t capw)
{
  const bool whole = c0 + LANES < nchunks && 16 * (c0 + LANES) <= (uint64_t)F.n[0] / 4;
  if (!whole || !F.vec) return false;
  const uint64_t w0 = ((base_bits + index[c0]) >> 6) & ~1ull;
  const uint64_t wend = (base_bits + index[c0 + LANES] + 63) >> 6;
  return min<uint64_t>(wend, in_words) - w0 > capw;
}

template <uint32_t LANES, uint32_t CAPB>
__device__ __forceinline__ bool vdec_left_to_big(const FieldDesc& F, const uint64_t* index, uint64_t in_words,
                                                 uint64_t nchunks, uint64_t base_bits, uint64_t c0)
{
  return vdec_left_to_big_w<LANES>(F, index, in_words, nchunks, base_bits, c0, vdec_cap<LANES, CAPB>());
}

// The stage tier of a stream from its block index (1: the 32-bit-per-block stage, 3: the 64-bit one): 1 when the
// 32-bit stage holds 1.25 x the stream's average bits per block over chunks 0 .. nchunks - 2 -- the rule the launcher
// applies to an exact-length buffer, taken here on the device for a buffer whose size says nothing (a capacity-sized
// Encoder.words). The two tiers are launched gated; the workgroups of the one that does not match return after two
// index loads (~13 us for the whole empty launch; a 48-bit tier measured as a second empty launch and was dropped).
__device__ __forceinline__ uint32_t vdec_tier(const uint64_t* index, uint64_t nchunks)
{
  if (nchunks < 2) return 1;
  const uint64_t span = index[nchunks - 1] - index[0], nbk = (nchunks - 1) * 16;
  return span * 5 <= nbk * 32 * 4 ? 1u : 3u;
}

// One group: its span staged in sw (CAP words), each lane's 16 blocks decoded by the lean block decoder, stored
// through the 8 x 8 lane transposes. BIG: the second pass (stage the caller's sw only after a barrier: the previous
// group's readers are done); else the main kernel, which stages dt7 with the span in one round trip. The group phase
// goes through the one-plane table: the pair table (7.4 KB more LDS) measured slower at every stage size here
// (occupancy; profiles/r05_vdec_adaptive_stage_ab.log, profiles/r04_var_decode_pair8_negative.log).
template <uint32_t LANES, uint32_t CAP, bool BIG>
__device__ __forceinline__ void vdec_group(const FieldDesc& F, const Params& p, const uint64_t* __restrict__ in,
                                           uint64_t in_words, const uint64_t* __restrict__ index, uint64_t nchunks,
                                           uint64_t base_bits, uint64_t* __restrict__ end_out, uint64_t c0,
                                           uint16_t* dt7, uint64_t* sw)
{
  const uint32_t tid = threadIdx.x;
  const uint64_t w0 = ((base_bits + index[c0]) >> 6) & ~1ull;  // 16-byte aligned start
  const uint64_t wend = c0 + LANES < nchunks ? ((base_bits + index[c0 + LANES] + 63) >> 6) : in_words;
  const uint64_t span = min<uint64_t>(wend, in_words) - w0;
  const bool staged = span <= CAP;
  const uint64_t c = c0 + tid;
  const uint64_t mine = c < nchunks ? index[c] : 0ull;
  if constexpr (BIG) __syncthreads();
  else stage_lds16<LANES, sizeof(DecTab7) / 16>(dt7, &g_dec_tab7, sizeof(DecTab7));
  if (staged) stage_lds16<LANES, (CAP + 4) / 2>(sw, in + w0, (uint32_t)(8 * span));
  __syncthreads();
  float* out = (float*)F.data;
  const bool whole = c0 + LANES <= nchunks && 16 * (c0 + LANES) <= (uint64_t)F.n[0] / 4;  // no partial chunk or block
  if (!staged || !whole || !F.vec) {  // the general path (wave-uniform: the whole workgroup)
    if (c >= nchunks) return;
    const uint64_t b0 = c * 16, b1 = min<uint64_t>(b0 + 16, F.nblocks);
    uint64_t pos = base_bits + mine;
    if (staged) {
      pos -= 64 * w0;
      for (uint64_t b = b0; b < b1; b++) {
        float f[4];
        decode_block1d_var(LdsWindow{sw}, pos, dt7, p.minexp, p.maxprec, f);
        store_block1d(F, b, f);
      }
      pos += 64 * w0;
    } else {
      for (uint64_t b = b0; b < b1; b++) {
        float f[4];
        decode_block1d_var(GlobalWindow{in}, pos, dt7, p.minexp, p.maxprec, f);
        store_block1d(F, b, f);
      }
    }
    if (end_out && c == nchunks - 1) *end_out = pos;
    return;
  }
  const uint32_t* sw32 = (const uint32_t*)sw;
  const int cexp = 4 - p.minexp, maxprec = (int)min(p.maxprec, 64u);
  uint32_t pos = (uint32_t)(base_bits + mine - 64 * w0);
  const uint32_t lane = tid & 63u, m = lane & 7u;
  float4* o4 = (float4*)out + (c - m) * 16 + m;  // block m of the group's first chunk
  uint2* o2 = (uint2*)F.data + (c - m) * 16 + m;  // bf16 output: 8 bytes per block
  const bool bf = F.dtype == DT_BF16;
#pragma unroll 1  // two copies of the 8-block body are past the unroller's size limit (nothing here needs them)
  for (int rnd = 0; rnd < 2; rnd++) {
    float g[8][4];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const uint32_t start = pos;
      if (!dec_block1d_lean(sw32, pos, dt7, cexp, maxprec, g[k])) {
        uint64_t p64 = start;
        decode_block1d_var(LdsWindow{sw}, p64, dt7, p.minexp, p.maxprec, g[k]);
        pos = (uint32_t)p64;
      }
    }
    xpose8_stage<1>(g, lane);
    xpose8_stage<2>(g, lane);
    xpose8_stage<4>(g, lane);
    if (bf) {
#pragma unroll
      for (int i = 0; i < 8; i++)
        o2[16 * i + 8 * rnd] = make_uint2(bf16x2_rne(g[i][0], g[i][1]), bf16x2_rne(g[i][2], g[i][3]));
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++) o4[16 * i + 8 * rnd] = make_float4(g[i][0], g[i][1], g[i][2], g[i][3]);
    }
  }
  if (end_out && c == nchunks - 1) *end_out = pos + 64 * w0;
}

template <uint32_t LANES, uint32_t CAPB>
__global__ __launch_bounds__(LANES) void k_decode1d_var_lean(FieldDesc F, Params p, const uint64_t* __restrict__ in,
                                                             uint64_t in_words, const uint64_t* __restrict__ index,
                                                             uint64_t nchunks, uint64_t base_bits,
                                                             uint64_t* __restrict__ end_out, uint64_t* __restrict__ left,
                                                             uint64_t seq, uint32_t tier)
{
  __shared__ __attribute__((aligned(16))) uint16_t dtab[5 * 128];  // r = 7 rows of the plane table
  __shared__ __attribute__((aligned(16))) uint64_t sw[vdec_cap<LANES, CAPB>() + 4];
  if (tier && vdec_tier(index, nchunks) != tier) return;  // gated: another tier's launch decodes this stream
  const uint64_t c0 = (uint64_t)blockIdx.x * LANES;
  if (vdec_left_to_big<LANES, CAPB>(F, index, in_words, nchunks, base_bits, c0)) {  // workgroup-uniform
    if (left && threadIdx.x == 0) atomicMax((unsigned long long*)left, (unsigned long long)seq);  // second pass has work
    return;
  }
  vdec_group<LANES, vdec_cap<LANES, CAPB>(), false>(F, p, in, in_words, index, nchunks, base_bits, end_out, c0, dtab, sw);
}

template <uint32_t LANES>
__device__ __forceinline__ void vdec_group_big(const FieldDesc& F, const Params& p, const uint64_t* __restrict__ in,
                                            uint64_t in_words, const uint64_t* __restrict__ index, uint64_t nchunks,
                                            uint64_t base_bits, uint64_t* __restrict__ end_out, uint64_t c0,
                                            uint16_t* dt7, uint64_t* sw)
{
  vdec_group<LANES, vdec_cap_big<LANES>(), true>(F, p, in, in_words, index, nchunks, base_bits, end_out, c0, dt7, sw);
}

template <uint32_t LANES, uint32_t CAPB>
__global__ __launch_bounds__(LANES) void k_decode1d_var_lean_big(FieldDesc F, Params p, const uint64_t* __restrict__ in,
                                                                 uint64_t in_words, const uint64_t* __restrict__ index,
                                                                 uint64_t nchunks, uint64_t base_bits,
                                                                 uint64_t* __restrict__ end_out,
                                                                 const uint64_t* __restrict__ left, uint64_t seq,
                                                                 bool tiered)
{
  __shared__ __attribute__((aligned(16))) uint16_t dt7[5 * 128];
  __shared__ __attribute__((aligned(16))) uint64_t sw[vdec_cap_big<LANES>() + 4];
  __shared__ uint32_t todo[LANES];
  __shared__ uint32_t ntodo;
  if (left && *left < seq) return;  // the main kernel left nothing (no flag word: check every group)
  // the stage of the main launch that decoded this stream: CAPB, or (tiered) the tier vdec_tier picks
  uint64_t capw = vdec_cap<LANES, CAPB>();
  if (tiered) {
    const uint32_t t = vdec_tier(index, nchunks);
    capw = t == 1 ? vdec_cap<LANES, 32>() : vdec_cap<LANES, 64>();
  }
  const uint64_t ng = (nchunks + LANES - 1) / LANES;
  bool staged_tab = false;
  // sweep k: workgroup w checks groups k G LANES + t G + w (t < LANES, G = gridDim.x): the groups spread over every
  // workgroup of the grid
  const uint64_t G = gridDim.x;
  for (uint64_t gb = 0; gb < ng; gb += G * LANES) {
    if (threadIdx.x == 0) ntodo = 0;
    __syncthreads();
    const uint64_t g = gb + (uint64_t)threadIdx.x * G + blockIdx.x;
    if (g < ng && vdec_left_to_big_w<LANES>(F, index, in_words, nchunks, base_bits, g * LANES, capw))
      todo[atomicAdd(&ntodo, 1u)] = threadIdx.x;
    __syncthreads();
    const uint32_t nt = ntodo;
    if (nt && !staged_tab) {  // the decode table only once there is work
      stage_lds16<LANES, sizeof(DecTab7) / 16>(dt7, &g_dec_tab7, sizeof(DecTab7));
      staged_tab = true;
    }
    for (uint32_t i = 0; i < nt; i++)
      vdec_group_big<LANES>(F, p, in, in_words, index, nchunks, base_bits, end_out,
                            (gb + (uint64_t)todo[i] * G + blockIdx.x) * LANES, dt7, sw);
    __syncthreads();  // todo / ntodo are rewritten next sweep
  }
}

// the partial last block of a 1-D field (generic decoder, one lane)
__global__ void k_decode_tail1d(FieldDesc F, Params p, const uint64_t* __restrict__ in, uint64_t base_bits,
                                uint32_t b)
{
  BitReader r{in, base_bits + (uint64_t)b * p.maxbits};
  float f[4];
  decode_block<1>(r, p, f);
  store_block1d(F, b, f);
}

// ------------------------------------------------------------------------------------------------ launchers
static inline hipStream_t S(void* s) { return (hipStream_t)s; }

// The second-pass flag words of launch_decode1d_var: kVdecFlagRing zeroed uint64 words per device, allocated on first
// use and kept for the life of the process (nullptr if the allocation fails: the second pass then checks every group).
// The first use allocates and zeroes on the caller's stream and waits for it; a first use inside stream capture
// (where neither is allowed) returns nullptr instead -- that decode checks every group, and the ring is allocated by
// the next uncaptured call.
constexpr uint32_t kVdecFlagRing = 256;
static uint64_t* vdec_flag_ring(hipStream_t st)
{
  static std::mutex mu;
  static uint64_t* ring[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
    (void)hipGetLastError();
    return nullptr;
  }
  std::lock_guard<std::mutex> lk(mu);
  if (!ring[dev]) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
      (void)hipGetLastError();
      return nullptr;
    }
    uint64_t* r = nullptr;
    if (hipMalloc((void**)&r, kVdecFlagRing * sizeof(uint64_t)) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    if (hipMemsetAsync(r, 0, kVdecFlagRing * sizeof(uint64_t), st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(r);
      return nullptr;
    }
    ring[dev] = r;
  }
  return ring[dev];
}

hipError_t launch_decode1d_var(const FieldDesc& F, const Params& p, const uint64_t* in, uint64_t in_words,
                               const uint64_t* index, uint32_t chunk, uint64_t nchunks, uint64_t base_bits,
                               uint64_t* end_out, void* stream)
{
  if (index && chunk == 16 && in_words) {  // the workgroup's stream span staged in LDS, 128 lanes
    constexpr uint32_t L = 128;
    const uint64_t ng = (nchunks + L - 1) / L;
    // a stream-ordered flag word: a main-kernel workgroup that leaves its group to the second pass raises the word to
    // this call's sequence number (atomicMax), and the second pass returns at once unless the word is >= its number,
    // so an empty second pass costs one load per workgroup instead of every group's span check (~40 us). The words
    // are a persistent per-device ring (no allocation per call, nothing captured into a graph but the pointer):
    // numbers only grow, so a word raised by a later call or by a concurrent decode on another stream can only make a
    // second pass check every group (slower, still exact), never skip one that has work.
    static std::atomic<uint64_t> g_seq{1};
    const uint64_t seq = g_seq.fetch_add(1);
    hipStream_t st = S(stream);
    uint64_t* left = vdec_flag_ring(st);
    if (left) left += seq % kVdecFlagRing;
    // the main kernel's stage, sized per call (LDS sets its occupancy: 8 / 6 / 4.5 waves per SIMD at 32 / 48 / 64 bits
    // per block; accuracy 1e-3 bf16, 24 bits per block: 0.43 -> 0.35 ms, profiles/r05_vdec_adaptive_stage_ab.log):
    //  * a buffer sized like its stream (what a receiver holds): the smallest of 32 / 48 / 64 bits per block that
    //    holds 1.25 x the buffer's average -- the 48-bit tier exists on this path only;
    //  * a capacity-sized buffer (Encoder.words): the 32- and 64-bit tiers only, both launched, gated on the device.
    const uint64_t nb = F.nblocks ? F.nblocks : 1, avail = in_words * 64 - std::min<uint64_t>(base_bits, in_words * 64);
    const uint32_t gbig = (uint32_t)std::min<uint64_t>(ng, 1024);
    if (avail >= nb * 128) {
      // a buffer of (near) the encoder's capacity (140 bits per block) says nothing about the stream: the 32- and
      // 64-bit stage tiers (no 48-bit one: it measured as a second empty launch) launched gated on the stream's own
      // average from its index (vdec_tier), the one that does not match returning after two index loads per workgroup
      // (accuracy 1e-3 in a capacity buffer: 0.42 -> 0.37 ms; 1e-6: +13 us for the empty tier,
      // profiles/r06_vdec_capacity_tiers.log)
      k_decode1d_var_lean<L, 32><<<(uint32_t)ng, L, 0, st>>>(F, p, in, in_words, index, nchunks, base_bits, end_out,
                                                             left, seq, 1u);
      k_decode1d_var_lean<L, 64><<<(uint32_t)ng, L, 0, st>>>(F, p, in, in_words, index, nchunks, base_bits, end_out,
                                                             left, seq, 3u);
      k_decode1d_var_lean_big<L, 64><<<gbig, L, 0, st>>>(F, p, in, in_words, index, nchunks, base_bits, end_out, left,
                                                         seq, true);
    } else if (avail * 5 <= nb * 32 * 4) {
      k_decode1d_var_lean<L, 32><<<(uint32_t)ng, L, 0, st>>>(F, p, in, in_words, index, nchunks, base_bits, end_out,
                                                             left, seq, 0u);
      k_decode1d_var_lean_big<L, 32><<<gbig, L, 0, st>>>(F, p, in, in_words, index, nchunks, base_bits, end_out, left,
                                                         seq, false);
    } else if (avail * 5 <= nb * 48 * 4) {
      k_decode1d_var_lean<L, 48><<<(uint32_t)ng, L, 0, st>>>(F, p, in, in_words, index, nchunks, base_bits, end_out,
                                                             left, seq, 0u);
      k_decode1d_var_lean_big<L, 48><<<gbig, L, 0, st>>>(F, p, in, in_words, index, nchunks, base_bits, end_out, left,
                                                         seq, false);
    } else {
      k_decode1d_var_lean<L, GCOW_VDEC_CAPB><<<(uint32_t)ng, L, 0, st>>>(F, p, in, in_words, index, nchunks, base_bits,
                                                                         end_out, left, seq, 0u);
      k_decode1d_var_lean_big<L, GCOW_VDEC_CAPB><<<gbig, L, 0, st>>>(F, p, in, in_words, index, nchunks, base_bits,
                                                                     end_out, left, seq, false);
    }
    return hipGetLastError();
  }
  k_decode1d_var<<<(uint32_t)((nchunks + 255) / 256), 256, 0, S(stream)>>>(F, p, in, index, chunk, nchunks, base_bits,
                                                                           end_out);
  return hipGetLastError();
}

hipError_t launch_decode_fixed1d(const FieldDesc& F, const Params& p, const uint64_t* in, uint64_t base_bits,
                                 void* stream)
{
  const uint32_t nfull = (uint32_t)(F.n[0] / 4);
  constexpr uint32_t CH = 1u << 27;
  for (uint32_t c0 = 0; c0 < nfull; c0 += CH) {  // one-shot grid, U = 8 (64-bit blocks) / 16 (32-bit) words per lane
    const uint32_t nc = min(CH, nfull - c0);
    const bool bf = F.dtype == DT_BF16;
    void* out = (char*)F.data + (size_t)c0 * 4 * (bf ? 2 : 4);
    const uint64_t bb = base_bits + (uint64_t)c0 * p.maxbits;
    constexpr uint32_t U64 = GCOW_C2DEC_U;
    const uint32_t g64 = (nc + 256 * U64 - 1) / (256 * U64), g32 = (nc + 4095) / 4096;
    if (p.maxbits == 64 && bf) k_decode_fixed1d_np<64, U64, true><<<g64, 256, 0, S(stream)>>>(in, nc, p, out, bb);
    else if (p.maxbits == 64) k_decode_fixed1d_np<64, U64><<<g64, 256, 0, S(stream)>>>(in, nc, p, out, bb);
    else if (bf) k_decode_fixed1d_np<32, 16, true><<<g32, 256, 0, S(stream)>>>(in, nc, p, out, bb);
    else k_decode_fixed1d_np<32, 16><<<g32, 256, 0, S(stream)>>>(in, nc, p, out, bb);
  }
  if (F.n[0] % 4) k_decode_tail1d<<<1, 1, 0, S(stream)>>>(F, p, in, base_bits, nfull);
  return hipGetLastError();
}

}  // namespace gcow
