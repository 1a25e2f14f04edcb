// var1d.hip -- single-pass 1-D variable-rate encoder (accuracy / precision / expert with minbits <= 1,
// maxbits >= 160: no budget ever truncates a block), the C5 path of BASELINE configs[4].
//
// Reference: sw/src/zfp.c:31-56 (block loop), sw/src/encode.c:457-495 (encode_fblock) and :279-339 (the embedded
// coder), sw/src/stream.c:61-138 (LSB-first packing). The reference codes blocks one after another into one stream;
// the position of block b is the sum of the lengths of blocks 0 .. b-1, which is what this kernel computes in one
// pass over the input:
//
//  * one workgroup per tile of 1024 consecutive blocks (256 lanes x 4): every lane derives its blocks' coefficients
//    once, their lengths by the closed form and its offset in the tile by a workgroup scan;
//  * the tile's length total is published at once (a decoupled look-back status word, MI355X_MICROARCH.md
//    "Valid forms" R2 granule: value and flag in ONE 8-byte agent-scope store, no fence), the blocks are coded into
//    the tile's LDS window at tile-relative positions, and only then does one wave look back over the predecessors'
//    status words for the tile's stream offset -- by then they have published. A predecessor that has not published
//    after a bounded wait has its total computed here from its input instead, so no workgroup ever depends on
//    another one being scheduled (no dispatch-order assumption, no deadlock);
//  * each lane packs its consecutive blocks in a 64-bit register accumulator: whole words are plain LDS stores,
//    only the two words it shares with its neighbours are ds_or;
//  * the window is stored shifted to the tile's bit offset as coalesced 32-bit words; the one word a tile shares with
//    each neighbour is combined through a per-boundary 64-bit atomicOr (the second contributor writes it).
// The status and boundary words are zeroed by a memset node before every launch (gcow_amd/csrc/var1d.hip launcher).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdlib.h>

#include <algorithm>

#include "codec_device.h"
#include "field_io.h"
#include "kernels.h"
#include "lean1d.h"
#include "tiles.h"
#include "var1d_prep.h"
#include "var1d_tile.h"  // GCOW_V1T, V1_ABLATE, the window sizes, v1_code, v1_tile_store, v1_lds, V1Workspace

// ---- tunables of this unit alone (A/B builds: tools/build_variant.sh, tools/ubench/var1d_ablate.sh)
#ifndef V1_COUNT_PF
#define V1_COUNT_PF 1  // tiles of loads in flight ahead of the counted one (k_count1d_var_tile), 1 .. 3
#endif

namespace gcow {

constexpr uint64_t V1VAL = (1ull << 62) - 1;                 // status word: flag << 62 | value
constexpr uint32_t V1SPIN = 96;  // polls (~1.5 us each) of a missing predecessor before computing its total here

// The lane's V1U consecutive blocks of tile t as raw words: 16-B loads of a whole tile of full, contiguous, 16-B
// aligned blocks (fp32: one per block; bf16: one per two blocks), else the padded / strided gather (encode.c:41-126)
// repacked into the same words (bf16 values narrowed back exactly).
template <int DT>
struct V1Raw {
  static constexpr int N = DT == DT_BF16 ? V1U / 2 : V1U;
  uint4 w[N];
  __device__ __forceinline__ void load(const FieldDesc& F, uint32_t t, bool wide_ok)
  {
    const uint64_t bl = (uint64_t)t * V1TILE + (uint64_t)threadIdx.x * V1U;
    if (wide_ok && (uint64_t)(t + 1) * V1TILE <= F.n[0] / 4) {
      const uint4* src = (const uint4*)F.data + (DT == DT_BF16 ? bl / 2 : bl);
#pragma unroll
      for (int h = 0; h < N; h++) w[h] = src[h];
    } else {
#pragma unroll
      for (uint32_t k = 0; k < V1U; k++) {
        float f[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (bl + k < F.nblocks) gather_block<1, DT>(F, (uint32_t)(bl + k), f);
        uint32_t* d = (uint32_t*)w;
        if constexpr (DT == DT_BF16) {
          d[2 * k] = (__float_as_uint(f[0]) >> 16) | (__float_as_uint(f[1]) & 0xffff0000u);
          d[2 * k + 1] = (__float_as_uint(f[2]) >> 16) | (__float_as_uint(f[3]) & 0xffff0000u);
        } else {
#pragma unroll
          for (int i = 0; i < 4; i++) d[4 * k + i] = __float_as_uint(f[i]);
        }
      }
    }
  }
  __device__ __forceinline__ void block(uint32_t k, float* f) const
  {
    const uint32_t* d = (const uint32_t*)w;
    if constexpr (DT == DT_BF16) {
      f[0] = __uint_as_float(d[2 * k] << 16);
      f[1] = __uint_as_float(d[2 * k] & 0xffff0000u);
      f[2] = __uint_as_float(d[2 * k + 1] << 16);
      f[3] = __uint_as_float(d[2 * k + 1] & 0xffff0000u);
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++) f[i] = __uint_as_float(d[4 * k + i]);
    }
  }
};

// Per-lane state of one tile between its preparation and its store: the blocks' coefficients, headers, K and
// lengths, the lane's offset in the tile and the tile's total.
struct V1Tile {
  uint32_t u[V1U][4], hdr[V1U], K[V1U], len[V1U];
  bool inf[V1U];
  uint32_t excl, total;
};

// Prepare tile t (coefficients, closed-form lengths, the lane's offset by a workgroup scan) and publish its total as
// its status word -- one 8-byte agent-scope store, value and flag in one granule (MI355X_MICROARCH.md "Valid forms").
template <int DT>
__device__ __forceinline__ void v1_prepare(const FieldDesc& F, const Params& p, const V1Raw<DT>& raw, uint32_t t,
                                           V1Tile& T, uint32_t* scan_sh, uint64_t* status, uint64_t incl_base)
{
  const uint64_t bl = (uint64_t)t * V1TILE + (uint64_t)threadIdx.x * V1U;
  uint32_t lsum = 0;
#pragma unroll
  for (uint32_t k = 0; k < V1U; k++) {
    float f[4];
    raw.block(k, f);
    const bool valid = bl + k < F.nblocks;
    T.len[k] = v1_prep(f, -122 - p.minexp, (int)min(p.maxprec, 64u), T.u[k], T.hdr[k], T.K[k], T.inf[k]);
    T.inf[k] = T.inf[k] && valid;
    if (T.inf[k]) T.len[k] = count_block<1>(f, p);
    T.len[k] = valid ? T.len[k] : 0u;
    lsum += T.len[k];
  }
  T.excl = block_exclusive_scan<V1T>(lsum, &T.total, scan_sh);
  if (threadIdx.x == 0)  // incl_base given (tile 0): the inclusive prefix at once
    __hip_atomic_store(status + t, incl_base != ~0ull ? ((2ull << 62) | (incl_base + T.total)) : ((1ull << 62) | T.total),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One of the two contributors of a 32-bit word shared by tiles x and x + 1 (role 0: tile x's last word, role 1: tile
// x + 1's first word): OR its bits and its arrival flag into the boundary's word; the second to arrive stores it.
__device__ __forceinline__ void v1_boundary(uint64_t* bnd, uint32_t x, uint32_t role, uint32_t* out, uint32_t val)
{
  const uint64_t old = atomicOr((unsigned long long*)(bnd + x), (unsigned long long)((1ull << (32 + role)) | val));
  if ((old >> (33 - role)) & 1ull) *out = val | (uint32_t)old;
}

// Total bit length of tile `tile` by one wave, from the input: the look-back's fallback for a predecessor without a
// status after a bounded wait (the same lengths the tile's own workgroup sums).
template <int DT>
__device__ uint64_t v1_wave_total(const FieldDesc& F, const Params& p, uint32_t tile, uint32_t lane)
{
  uint64_t s = 0;
  const uint64_t b0 = (uint64_t)tile * V1TILE;
  const uint64_t b1 = min<uint64_t>(b0 + V1TILE, F.nblocks);
  for (uint64_t b = b0 + lane; b < b1; b += 64) {
    float f[4];
    gather_block<1, DT>(F, (uint32_t)b, f);
    uint32_t u[4], hdr, K;
    bool inf;
    uint32_t len = v1_prep(f, -122 - p.minexp, (int)min(p.maxprec, 64u), u, hdr, K, inf);
    if (inf) len = count_block<1>(f, p);
    s += len;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// Decoupled look-back (one wave): the stream offset of tile t = base0 + the totals of tiles 0 .. t-1, from the
// predecessors' status words, 4 per lane = 256 per round trip (flag 2 = inclusive prefix: stop at the nearest one;
// flag 1 = the tile's own total). A predecessor without a status after `spin` polls has its total computed here
// (v1_wave_total), so no tile depends on another being scheduled.
template <int DT>
__device__ uint64_t v1_lookback(uint64_t* status, uint32_t t, uint64_t base0, const FieldDesc& F, const Params& p,
                                uint32_t lane, uint32_t spin, uint64_t* stats)
{
  constexpr int L = 4;
  uint64_t excl = 0;
  int64_t j = (int64_t)t - 1;  // nearest predecessor of the window
  uint32_t polls = 0, fallbacks = 0, windows = 0;
  uint64_t fb[L] = {0, 0, 0, 0};  // totals computed here (this window, this lane), flag in bit 62
  while (true) {
    uint64_t v[L];
    int first = L;  // this lane's nearest inclusive entry
#pragma unroll
    for (int i = 0; i < L; i++) {
      const int64_t idx = j - (int64_t)(L * lane) - i;
      v[i] = idx >= 0 ? __hip_atomic_load(status + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                      : ((2ull << 62) | (idx == -1 ? base0 : 0ull));  // "tile -1": the stream's start
      if ((v[i] >> 62) == 0 && fb[i]) v[i] = fb[i];
    }
#pragma unroll
    for (int i = L - 1; i >= 0; i--) first = (v[i] >> 62) == 2 ? i : first;
    const uint64_t incl = __ballot(first < L);
    const uint32_t L0 = incl ? (uint32_t)__builtin_ctzll(incl) : 64u;  // lane holding the nearest inclusive
    const int nneed = lane < L0 ? L : (lane == L0 ? first + 1 : 0);     // entries this lane contributes
    int miss = L;
#pragma unroll
    for (int i = L - 1; i >= 0; i--) miss = (i < nneed && (v[i] >> 62) == 0) ? i : miss;
    const uint64_t missing = __ballot(miss < L);
    if (missing) {
      if (++polls <= spin) {
        __builtin_amdgcn_s_sleep(8);
        continue;
      }
      const uint32_t k = (uint32_t)__builtin_ctzll(missing);
      const int mi = __shfl(miss, (int)k, 64);
      const uint64_t tot = v1_wave_total<DT>(F, p, (uint32_t)(j - (int64_t)(L * k) - mi), lane);
#pragma unroll
      for (int i = 0; i < L; i++)
        if (lane == k && i == mi) fb[i] = (1ull << 62) | tot;
      fallbacks++;
      continue;
    }
    windows++;
    uint64_t x = 0;
#pragma unroll
    for (int i = 0; i < L; i++) x += i < nneed ? (v[i] & V1VAL) : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    excl += x;
    if (incl) {
      if (stats && lane == 0) {  // variant stats: look-back behaviour, summed over the launch
        atomicAdd((unsigned long long*)stats, (unsigned long long)polls);
        atomicAdd((unsigned long long*)stats + 1, (unsigned long long)fallbacks);
        atomicAdd((unsigned long long*)stats + 2, (unsigned long long)windows);
        if (polls) {  // tiles that polled at all, the most polls of one tile, polls of the first 2048 tiles
          atomicAdd((unsigned long long*)stats + 3, 1ull);
          atomicMax((unsigned long long*)stats + 4, (unsigned long long)polls);
          if (t < 2048) atomicAdd((unsigned long long*)stats + 5, (unsigned long long)polls);
        }
      }
      return excl;
    }
    j -= 64 * L;
#pragma unroll
    for (int i = 0; i < L; i++) fb[i] = 0;
  }
}

// The encoder: one workgroup per tile of V1TILE blocks. Tile t: prepare (coefficients, closed-form lengths, the
// lanes' offsets by a workgroup scan) and publish its total at once; code into the LDS window at tile-relative
// positions; look back (one wave) for the stream offset; store the window shifted to the offset, the two words shared
// with the neighbouring tiles through v1_boundary.
template <int DT>
__global__ __launch_bounds__(V1T) void k_encode1d_var_sp(FieldDesc F, Params p, uint64_t* __restrict__ status,
                                                         uint64_t* __restrict__ bnd, uint32_t* __restrict__ out32,
                                                         uint64_t* __restrict__ index, uint32_t index_shift,
                                                         const uint64_t* __restrict__ d_base,
                                                         uint64_t* __restrict__ d_total, uint32_t ntiles,
                                                         uint32_t spin, uint64_t* __restrict__ stats)
{
  __shared__ __attribute__((aligned(16))) uint32_t tab[1280];  // pair table (lean-5 entries, rows n >= 3 empty)
  __shared__ uint32_t rs[1024];   // window spread tables
  __shared__ uint64_t win[V1Q];   // the tile's code, tile-relative bit positions
  __shared__ uint32_t scan_sh[V1T / 64];
  __shared__ uint64_t s_base;
  __shared__ uint32_t s_special;
  uint32_t* win32 = (uint32_t*)win;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t t = blockIdx.x;
  stage_table<V1T, 1280>(tab, g_plane_tab_var.v);
#pragma unroll
  for (uint32_t i = 0; i < 1024 / V1T; i++) rs[tid + V1T * i] = rspread_entry(tid + V1T * i);
  if (tid == 0) s_special = 0;
  const bool wide_ok = F.vec && (((uintptr_t)F.data) & 15u) == 0;
  const uint64_t base0 = d_base ? *d_base : 0ull;
  V1Raw<DT> raw;
  raw.load(F, t, wide_ok);
  V1Tile T;
  v1_prepare<DT>(F, p, raw, t, T, scan_sh, status, t == 0 ? base0 : ~0ull);
  const uint32_t excl = T.excl, total = T.total;
  uint32_t lsum = 0;
#pragma unroll
  for (uint32_t k = 0; k < V1U; k++) lsum += T.len[k];
  if (lsum) {  // the two words this lane shares with its neighbours start at zero
    win[excl >> 6] = 0ull;
    win[(excl + lsum - 1) >> 6] = 0ull;
  }
  __syncthreads();

  // ---- code the lane's blocks: a 64-bit accumulator; whole words are plain LDS stores, the two shared ones ds_or
  uint64_t acc = 0;
  uint32_t q = excl >> 6, fill = excl & 63u;
  const uint32_t qhead = q;
  bool sp[V1U];
  bool any_sp = false;
#pragma unroll
  for (uint32_t k = 0; k < V1U; k++) {
    uint64_t c0, c1;
    sp[k] = T.inf[k];
    if constexpr (V1_ABLATE & 2) {
      c0 = T.u[k][0] ^ T.u[k][1];
      c1 = T.u[k][2] ^ T.u[k][3];
    } else {
      v1_code(T.u[k], T.hdr[k], T.len[k], T.K[k], tab, rs, c0, c1, sp[k]);
    }
    sp[k] = sp[k] && T.len[k];
    if (sp[k]) c0 = c1 = 0ull;  // coded below by the generic coder, OR-ed into these zero bits
    any_sp = any_sp || sp[k];
    // bits past the block's length are cleared from the accumulator after the full words leave it (a full word
    // holds only bits below the length)
    acc |= c0 << fill;
    const uint64_t mid = ((c0 >> 1) >> (63u - fill)) | (c1 << fill);
    const uint64_t hi = (c1 >> 1) >> (63u - fill);
    const uint32_t nf = fill + T.len[k];
    if (nf >= 64u) {
      if (q == qhead) atomicOr((unsigned long long*)&win[q], (unsigned long long)acc);
      else win[q] = acc;
      q++;
      acc = mid;
      if (nf >= 128u) {
        win[q] = acc;
        q++;
        acc = hi;
        if (nf >= 192u) {  // a special block of up to 140 bits (its code is zero here) completes a third word
          win[q] = acc;
          q++;
          acc = 0ull;
        }
      }
    }
    fill = nf & 63u;
    acc &= (1ull << fill) - 1ull;
  }
  if (fill) atomicOr((unsigned long long*)&win[q], (unsigned long long)acc);
  if (any_sp) s_special = 1u;
  __syncthreads();
  if (s_special) {  // Inf / NaN blocks, long group phases, codes past 128 bits: the generic coder
    uint32_t o = excl;
#pragma unroll
    for (uint32_t k = 0; k < V1U; k++) {
      if (sp[k]) {
        float f[4];
        raw.block(k, f);
        LdsWriter wr{win32, o, o + T.len[k]};
        encode_block<1>(wr, f, p);
      }
      o += T.len[k];
    }
    __syncthreads();
  }

  // ---- the tile's stream offset (wave 0)
  if (tid < 64) {
    const uint64_t B = t == 0 ? base0
                              : ((V1_ABLATE & 1) ? (uint64_t)t << 16
                                                 : v1_lookback<DT>(status, t, base0, F, p, lane, spin, stats));
    if (lane == 0) {
      if (t) __hip_atomic_store(status + t, (2ull << 62) | (B + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_base = B;
    }
  }
  __syncthreads();
  const uint64_t B = s_base;
  const uint64_t bl = (uint64_t)t * V1TILE + (uint64_t)tid * V1U;
  if (index) {
    uint32_t o = excl;
#pragma unroll
    for (uint32_t k = 0; k < V1U; k++) {
      const uint64_t b = bl + k;
      if (T.len[k] && (b & ((1ull << index_shift) - 1ull)) == 0) index[b >> index_shift] = B + o;
      o += T.len[k];
    }
  }

  // ---- store the window shifted to the tile's offset: 32-bit words, coalesced
  const uint32_t rb = (uint32_t)(B & 31u);
  const uint64_t g0 = B >> 5;
  const uint32_t nw = (rb + total + 31u) >> 5;  // global words the tile touches
  const uint32_t lw = (total + 31u) >> 5;       // window words holding the tile's bits
  const bool last_tile = t == ntiles - 1;
  for (uint32_t k = tid; k < ((V1_ABLATE & 4) ? 0u : nw); k += V1T) {
    const uint32_t hi = k < lw ? win32[k] : 0u;
    const uint32_t lo = (k > 0 && k - 1 < lw) ? win32[k - 1] : 0u;
    const uint32_t val = rb ? (hi << rb) | (lo >> (32u - rb)) : hi;
    uint32_t* dst = out32 + g0 + k;
    const bool first = k == 0 && rb != 0;
    const bool tail = k == nw - 1 && ((rb + total) & 31u) != 0 && !last_tile;
    if (first) {
      if (t == 0) atomicOr(dst, val);  // bits already in the stream before d_base (append)
      else v1_boundary(bnd, t - 1, 1u, dst, val);
    } else if (tail) {
      v1_boundary(bnd, t, 0u, dst, val);
    } else {
      *dst = val;
    }
  }
  if (last_tile && tid == 0) {
    const uint64_t end = B + total;
    const uint64_t endw = (end + 31) >> 5;
    if (endw & 1) out32[endw] = 0u;  // stream_flush: zero-pad to a 64-bit boundary (stream.c:132-138)
    if (d_total) *d_total = end;
  }
}

// The workspace: status[ntiles] then bnd[ntiles] (uint64 each) and 4 words of statistics, zeroed before the launch.
Var1dVariant g_var1d_variant = {0, -1, 0};

size_t var1d_sp_workspace_bytes(uint64_t nblocks)
{
  const uint64_t ntiles = (nblocks + V1TILE - 1) / V1TILE;
  return (size_t)(16 * ntiles + 64);
}

hipError_t launch_encode1d_var_sp(const FieldDesc& F, const Params& p, uint32_t* out32, uint64_t* ws,
                                  uint64_t* d_total, uint64_t* index, uint32_t index_shift, const uint64_t* d_base,
                                  void* stream)
{
  hipStream_t st = (hipStream_t)stream;
  const uint32_t ntiles = (uint32_t)((F.nblocks + V1TILE - 1) / V1TILE);
  hipError_t e = hipMemsetAsync(ws, 0, (size_t)16 * ntiles + 64, st);
  if (e != hipSuccess) return e;
  uint64_t* status = ws;
  uint64_t* bnd = ws + ntiles;
  // spin (tests): polls before a missing predecessor's total is computed locally; 0 exercises that path
  const uint32_t spin = g_var1d_variant.spin >= 0 ? (uint32_t)g_var1d_variant.spin : V1SPIN;
  // stats (measurement): polls, fallbacks, look-back windows, polling tiles, most polls, polls of the first 2048
  // tiles into ws[2 ntiles .. + 6)
  uint64_t* stats = g_var1d_variant.stats ? ws + 2 * (size_t)ntiles : nullptr;
  if (F.dtype == DT_BF16)
    k_encode1d_var_sp<DT_BF16><<<ntiles, V1T, 0, st>>>(F, p, status, bnd, out32, index, index_shift, d_base, d_total,
                                                       ntiles, spin, stats);
  else
    k_encode1d_var_sp<DT_F32><<<ntiles, V1T, 0, st>>>(F, p, status, bnd, out32, index, index_shift, d_base, d_total,
                                                      ntiles, spin, stats);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ tile form (default)
// count + scan + placed tile coder. The look-back above waits on predecessors spread over the eight XCDs (C5: 0.91 ms
// against 0.71 ms for this form, profiles/r03_c5_forms_ab.log); here the offsets come from a scan instead:
//   k_count1d_var_tile   V1CT tiles of V1TILE blocks per workgroup, the next tile's loads issued before a tile is counted:
//                        each block's length (closed form, v1_prep) as a byte (lens8: one 32-bit word per lane and
//                        tile, its V1U blocks) and each tile's total (sums[t]);
//   k_scan_ranges(_mw)   the tiles' stream offsets (base), zeroing the words two tiles share;
//   k_encode1d_var_tile  one tile per workgroup: the lane's offset in the tile by a workgroup scan of the stored
//                        lengths (before any block is prepared, so prepare and code run per block and the
//                        coefficients live only for one block), the blocks coded at their bit position relative to the
//                        16-byte stream boundary below the tile (base & 127 + the lane offset) into an LDS window
//                        through the lane accumulator, and the window stored as 16-byte chunks of stream words (no
//                        shifting; the two words shared with the neighbours by atomicOr). The window holds V1QS qwords (95 bits per block on
//                        average) so that 8 workgroups fit a CU (the kernel waits on memory and LDS latency: occupancy,
//                        not VALU issue, bounds it); a tile that needs more is skipped and coded by
//   k_encode1d_var_tile_big  the same body with the worst-case window (140 bits per block), a grid-stride loop over
//                        the list of oversized tiles k_encode1d_var_tile appended to (the count kernel empties it).
// The kernels exist for the field's own values and, named _resid, for y = x + e with the residual e' written by the
// coders; each is a template over its parameter source (ParamsHost / ParamsDev, var1d_prep.h). The device functions
// come first; the kernels, the one launcher and the workspace layout are at the end of this file.

// Raw buffer loads issued from inline asm, invisible to the compiler's waitcnt pass, with hand-counted waits (the
// scheme of k_encode_fixed1d_np): vmcnt counts loads and stores together, in issue order.
typedef int v1_v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v1_v4i v1_rsrc(const void* p, uint32_t bytes)
{
  const uint64_t a = (uint64_t)p;
  v1_v4i r;
  r.x = (int)(uint32_t)a;
  r.y = (int)((uint32_t)(a >> 32) & 0xffffu);  // stride 0
  r.z = (int)bytes;                             // num_records: range check in bytes
  r.w = 0x00020000;                             // raw buffer, no swizzle
  return r;
}

typedef unsigned v1_u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v1_u4 v1_ld16(uint32_t off, v1_v4i rs)
{
  v1_u4 v;
  asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(v) : "v"(off), "s"(rs) : "memory");
  return v;
}

// wait until at most N vector memory operations are outstanding; ties the tile's raw words to after the wait
template <int N, int NL>
__device__ __forceinline__ void v1_wait_n(v1_u4 (&w)[NL])
{
  if constexpr (NL == 2)
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(w[0]), "+v"(w[1]) : "n"(N) : "memory");
  else
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]) : "n"(N) : "memory");
}

// the same for k tiles of NL loads each still in flight (k folds to a constant in the unrolled tile loop)
template <int NL>
__device__ __forceinline__ void v1_wait_tiles(v1_u4 (&w)[NL], uint32_t k)
{
  switch (k) {
    case 0: v1_wait_n<0>(w); break;
    case 1: v1_wait_n<NL>(w); break;
    case 2: v1_wait_n<2 * NL>(w); break;
    default: v1_wait_n<3 * NL>(w); break;
  }
}

// One tile's block lengths (bytes packed per lane) and the lane's sum. FULL: every block of the tile is inside the
// field (no per-block range check).
template <int DT, bool FULL = false>
__device__ __forceinline__ uint32_t v1_count_tile(const FieldDesc& F, const Params& p, const V1Raw<DT>& raw,
                                                  uint32_t t, uint32_t& lsum)
{
  const uint64_t bl = (uint64_t)t * V1TILE + (uint64_t)threadIdx.x * V1U;
  const int cexp = -122 - p.minexp, maxprec = (int)min(p.maxprec, 64u);
  uint32_t pk = 0;
  lsum = 0;
#pragma unroll
  for (uint32_t k = 0; k < V1U; k++) {
    float f[4];
    raw.block(k, f);
    uint32_t u[4], hdr, K;
    bool inf;
    uint32_t len;
    if constexpr ((V1_ABLATE & 32) != 0) {  // measurement builds: no length computation in the count
      len = 9u + ((__float_as_uint(f[0]) ^ __float_as_uint(f[3])) & 63u);
      inf = false;
    } else {
      len = v1_prep(f, cexp, maxprec, u, hdr, K, inf);
    }
    const bool valid = FULL || bl + k < F.nblocks;
    if (inf && valid) len = count_block<1>(f, p);
    len = valid ? len : 0u;  // <= 140
    pk |= len << (8 * k);
    lsum += len;
  }
  return pk;
}

// One tile (raw words and the lane's byte lengths lw given) coded into the window `win`, from bit B & 127 (the
// 16-byte stream boundary below the tile's first bit); tab / rs already in LDS. Ends with the window complete
// (barrier) and the block index written. hook(k, f, u, hdr, K, inf) sees every block k of the lane once, with what
// v1_prep returned for it (the residual form below takes its decode from there); the default does nothing.
struct V1NoHook {
  __device__ __forceinline__ void operator()(uint32_t, const float*, const uint32_t*, uint32_t, uint32_t, bool) const {}
};

template <int DT, class Hook = V1NoHook>
__device__ __forceinline__ void v1_tile_code(const FieldDesc& F, const Params& p, uint32_t t, uint64_t B,
                                             const V1Raw<DT>& raw, uint32_t lw, uint64_t* __restrict__ index,
                                             uint32_t index_shift, const uint32_t* tab, const uint32_t* rs,
                                             uint64_t* win, uint32_t* scan_sh, uint32_t* s_special,
                                             const Hook& hook = Hook())
{
  uint32_t* win32 = (uint32_t*)win;
  const uint32_t tid = threadIdx.x;
  const uint32_t lb = (uint32_t)(B & 127u);
  uint32_t len[V1U], lsum = 0;
#pragma unroll
  for (uint32_t k = 0; k < V1U; k++) {
    len[k] = (lw >> (8 * k)) & 255u;
    lsum += len[k];
  }
  uint32_t tot_unused;
  const uint32_t excl = lb + block_exclusive_scan<V1T, false>(lsum, &tot_unused, scan_sh);  // barrier below
  if (lsum) {  // the two words this lane shares with its neighbours start at zero
    win[excl >> 6] = 0ull;
    win[(excl + lsum - 1) >> 6] = 0ull;
  }
  if (tid == 0) *s_special = 0;
  __syncthreads();

  // ---- prepare and code the lane's blocks one at a time: a 64-bit accumulator; whole words are plain LDS stores,
  // the two shared ones ds_or
  const uint64_t bl = (uint64_t)t * V1TILE + (uint64_t)tid * V1U;
  const int cexp = -122 - p.minexp, maxprec = (int)min(p.maxprec, 64u);
  uint64_t acc = 0;
  uint32_t q = excl >> 6, fill = excl & 63u;
  const uint32_t qhead = q;
  uint32_t spmask = 0;
  [[maybe_unused]] uint64_t sink = 0;
#pragma unroll
  for (uint32_t k = 0; k < V1U; k++) {
    float f[4];
    raw.block(k, f);
    uint32_t u[4], hdr, K;
    bool inf;
    if constexpr ((V1_ABLATE & 16) != 0) {
      for (int i = 0; i < 4; i++) u[i] = __float_as_uint(f[i]);
      hdr = 3u + (u[0] >> 23);
      K = 16;
      inf = false;
    } else {
      (void)v1_prep(f, cexp, maxprec, u, hdr, K, inf);  // the length comes from the count pass
    }
    hook(k, f, u, hdr, K, inf);
    bool sp = inf && bl + k < F.nblocks;
    uint64_t c0, c1;
    if constexpr ((V1_ABLATE & 2) != 0) {  // measurement builds: no coder (the prepared words stand in for the code)
      c0 = ((uint64_t)u[1] << 32 | u[0]) ^ hdr;
      c1 = (uint64_t)u[3] << 32 | u[2];
      sp = false;
    } else {
      v1_code(u, hdr, len[k], K, tab, rs, c0, c1, sp);
    }
    sp = sp && len[k];
    if (sp) c0 = c1 = 0ull;  // coded below by the generic coder, OR-ed into these zero bits
    spmask |= (uint32_t)sp << k;
    acc |= c0 << fill;
    const uint64_t mid = ((c0 >> 1) >> (63u - fill)) | (c1 << fill);
    const uint64_t hi = (c1 >> 1) >> (63u - fill);
    const uint32_t nf = fill + len[k];
    if (nf >= 64u) {
      if constexpr ((V1_ABLATE & 128) != 0) sink ^= acc;
      else if (q == qhead) atomicOr((unsigned long long*)&win[q], (unsigned long long)acc);
      else win[q] = acc;
      q++;
      acc = mid;
      if (nf >= 128u) {
        if constexpr ((V1_ABLATE & 128) != 0) sink ^= acc;
        else win[q] = acc;
        q++;
        acc = hi;
        if (nf >= 192u) {  // a special block of up to 140 bits (its code is zero here) completes a third word
          if constexpr ((V1_ABLATE & 128) != 0) sink ^= acc;
          else win[q] = acc;
          q++;
          acc = 0ull;
        }
      }
    }
    fill = nf & 63u;
    acc &= (1ull << fill) - 1ull;
  }
  if constexpr ((V1_ABLATE & 128) != 0) win[qhead] = sink ^ acc;  // keeps the code alive
  else if (fill) atomicOr((unsigned long long*)&win[q], (unsigned long long)acc);
  if (spmask) *s_special = 1u;
  __syncthreads();
  if (*s_special) {  // Inf / NaN blocks, long group phases, codes past 128 bits: the generic coder
    uint32_t o = excl;
#pragma unroll
    for (uint32_t k = 0; k < V1U; k++) {
      if ((spmask >> k) & 1u) {
        float f[4];
        raw.block(k, f);
        LdsWriter wr{win32, o, o + len[k]};
        encode_block<1>(wr, f, p);
      }
      o += len[k];
    }
    __syncthreads();
  }
  if (index) {
    uint32_t o = excl;
#pragma unroll
    for (uint32_t k = 0; k < V1U; k++) {
      const uint64_t b = bl + k;
      if (len[k] && (b & ((1ull << index_shift) - 1ull)) == 0) index[b >> index_shift] = (B & ~127ull) + o;
      o += len[k];
    }
  }

}

// Load, code and store one tile.
template <int DT>
__device__ __forceinline__ void v1_tile(const FieldDesc& F, const Params& p, uint32_t t, uint64_t B, uint32_t total,
                                        const uint32_t* __restrict__ lens8, uint32_t* __restrict__ out32,
                                        uint64_t* __restrict__ index, uint32_t index_shift, uint32_t ntiles,
                                        const uint32_t* tab, const uint32_t* rs, uint64_t* win, uint32_t* scan_sh,
                                        uint32_t* s_special)
{
  const bool wide_ok = F.vec && (((uintptr_t)F.data) & 15u) == 0;
  V1Raw<DT> raw;
  uint32_t lw;
  if constexpr ((V1_ABLATE & 64) != 0) {  // measurement builds: no input or length loads (words from the tile index)
    const uint32_t h = (t * 2654435761u) ^ (threadIdx.x * 40503u);
#pragma unroll
    for (int i = 0; i < V1Raw<DT>::N; i++)  // normal values near 5e-4 (bf16 / fp32 halves: sign, exponent 0x74)
      raw.w[i] = make_uint4((h & 0x807f807fu) | 0x3a003a00u, ((h * 3u) & 0x807f807fu) | 0x3a003a00u,
                            ((h * 5u) & 0x807f807fu) | 0x3a003a00u, ((h * 7u) & 0x807f807fu) | 0x3a003a00u);
    lw = 0x3a3a3a3au;
  } else {
    raw.load(F, t, wide_ok);
    lw = lens8[(size_t)t * V1T + threadIdx.x];
  }
  v1_tile_code<DT>(F, p, t, B, raw, lw, index, index_shift, tab, rs, win, scan_sh, s_special);
  v1_tile_store(t, B, total, win, out32, ntiles);
}

// ------------------------------------------------------------------------------------- tile form with the residual
// Error feedback at variable rate (gcow_encode_residual_device, include/gcow.h): the tile form
// on the field y = x + e (fp32; x fp32 or bf16, e fp32 or absent), whose code pass also writes e' = finite(y - yhat).
// yhat needs no decoder: in this domain it is v1_decode_closed of the coefficients v1_prep hands the coder anyway
// (the hook of v1_tile_code), so the residual costs one more row read in each pass and one row written.
//   count   on y: the x rows and the e rows of tile i + PF are requested before tile i is counted; writes lens8 /
//           sums / gsums, nothing to e_out
//   coders  on y, plus the tile's e' rows
// e_in may be e_out: a lane reads the e rows of its own blocks only, and the e' rows it stores are those of its quad
// of lanes (V1ResidOut::store_quad), computed from values all four have loaded -- so every row a wave writes it has
// read before, and no other wave reads it. Every tile is coded (its e read and its e' written) exactly once, by the
// main kernel or by the _big one: an oversized tile leaves the main kernel before any store. y = fadd(x, e) with e = +0 when e_in is null, so that -0 becomes +0
// as in the model (tests/residual_model.py).
#ifndef V1_RESID_PF
#define V1_RESID_PF 1  // tiles of loads in flight ahead of the counted one (k_count1d_var_tile_resid), 1 .. 3
#endif

__device__ __forceinline__ bool v1_aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

// The lane's V1U blocks of y from its x words and e words
template <int DT_X>
__device__ __forceinline__ void v1_form_y(const V1Raw<DT_X>& rx, const V1Raw<DT_F32>& re, V1Raw<DT_F32>& y)
{
#pragma unroll
  for (uint32_t k = 0; k < V1U; k++) {
    float f[4], e[4];
    rx.block(k, f);
    re.block(k, e);
    y.w[k] = make_uint4(__float_as_uint(__fadd_rn(f[0], e[0])), __float_as_uint(__fadd_rn(f[1], e[1])),
                        __float_as_uint(__fadd_rn(f[2], e[2])), __float_as_uint(__fadd_rn(f[3], e[3])));
  }
}

// Tile t of y through compiler-managed loads: whole 16-byte rows of a full tile, else the padded gather of x and of e
// (the same padding indices for both, so a padding value of y is a copy of a real one).
template <int DT_X>
__device__ __forceinline__ void v1_load_y(const FieldDesc& F, const float* e_in, uint32_t t, V1Raw<DT_F32>& y)
{
  V1Raw<DT_X> rx;
  V1Raw<DT_F32> re;
  rx.load(F, t, F.vec && v1_aligned16(F.data));
  if (e_in) {
    FieldDesc Fe = F;
    Fe.data = e_in;
    Fe.dtype = DT_F32;
    Fe.vec = v1_aligned16(e_in) ? 1u : 0u;
    re.load(Fe, t, Fe.vec != 0);
  } else {
#pragma unroll
    for (uint32_t k = 0; k < V1U; k++) re.w[k] = make_uint4(0u, 0u, 0u, 0u);
  }
  v1_form_y<DT_X>(rx, re, y);
}

// wait until at most N vector memory operations are outstanding; ties the tile's x and e words to after the wait
template <int N, int NX>
__device__ __forceinline__ void v1_wait_xe(v1_u4 (&x)[NX], v1_u4 (&e)[V1U])
{
  if constexpr (NX == 2)
    asm volatile("s_waitcnt vmcnt(%6)"
                 : "+v"(x[0]), "+v"(x[1]), "+v"(e[0]), "+v"(e[1]), "+v"(e[2]), "+v"(e[3])
                 : "n"(N)
                 : "memory");
  else
    asm volatile("s_waitcnt vmcnt(%8)"
                 : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(e[0]), "+v"(e[1]), "+v"(e[2]), "+v"(e[3])
                 : "n"(N)
                 : "memory");
}

// the same for k tiles still in flight, NX x loads and (HASE) V1U e loads each
template <int NX, bool HASE>
__device__ __forceinline__ void v1_wait_tiles_xe(v1_u4 (&x)[NX], v1_u4 (&e)[V1U], uint32_t k)
{
  if constexpr (HASE) {
    constexpr int NT = NX + (int)V1U;
    switch (k) {
      case 0: v1_wait_xe<0, NX>(x, e); break;
      case 1: v1_wait_xe<NT, NX>(x, e); break;
      case 2: v1_wait_xe<2 * NT, NX>(x, e); break;
      default: v1_wait_xe<3 * NT, NX>(x, e); break;
    }
  } else {
    v1_wait_tiles<NX>(x, k);
  }
}


// The e' rows of one tile: whole rows go through a buffer whose range is the tile's whole blocks inside the field (a
// row past it is dropped: padding blocks give no residual, nothing lands past e_out[n - 1]); the real values of the
// partial last block are stored one by one. The wide store is the compiler's builtin, not inline asm (DESIGN.md 5.1:
// an inline-asm wide store after VALU writes stored stale lanes); aux 2 = non-temporal.
struct V1ResidOut {
  __amdgpu_buffer_rsrc_t rows;
  float* e_out;
  uint64_t nvals, b0;  // b0: the tile's first block
  __device__ __forceinline__ V1ResidOut(float* e, uint64_t n, uint32_t t) : e_out(e), nvals(n), b0((uint64_t)t * V1TILE)
  {
    const uint64_t nfull = n / 4;
    const uint32_t nrows = (uint32_t)min<uint64_t>(V1TILE, nfull > b0 ? nfull - b0 : 0ull);
    rows = __builtin_amdgcn_make_buffer_rsrc(e + 4 * b0, 0, (int)(nrows * 16u), 0x00020000);
  }
  // row r of the tile
  __device__ __forceinline__ void store_row(uint32_t r, v1_u4 v) const
  {
    __builtin_amdgcn_raw_buffer_store_b128(v, rows, (int)(r * 16u), 0, 2);
    const uint32_t nv = (uint32_t)(nvals & 3u);
    if (nv && b0 + r == nvals / 4) {
      float* dst = e_out + 4 * (b0 + r);
      dst[0] = __uint_as_float(v.x);
      if (nv > 1) dst[1] = __uint_as_float(v.y);
      if (nv > 2) dst[2] = __uint_as_float(v.z);
    }
  }
  static __device__ __forceinline__ v1_u4 resid(const float* y, const float* d)
  {
    v1_u4 v;
    v.x = resid_bits(y[0], d[0]);
    v.y = resid_bits(y[1], d[1]);
    v.z = resid_bits(y[2], d[2]);
    v.w = resid_bits(y[3], d[3]);
    return v;
  }
  // The lane's V1U rows after a 4 x 4 transpose inside its quad of lanes (two DPP quad_perm exchanges per register):
  // store j of lane l then holds lane j's row l, so the quad's 16 rows leave as four contiguous 64-byte runs. Stored
  // straight from the lane -- each store 16-byte pieces 64 bytes apart -- the whole call took 1.67 against 1.19 ms
  // (fp32, accuracy 1e-3, 256 Mi values; profiles/r08_ef_var_time.log). Every lane of the quad must be active.
  __device__ __forceinline__ void store_quad(v1_u4 (&r)[V1U]) const
  {
    static_assert(V1U == 4, "a 4 x 4 transpose");
    const uint32_t l = threadIdx.x & 3u;
#pragma unroll
    for (int stage = 0; stage < 2; stage++) {
      const bool hi = stage == 0 ? (l & 1u) != 0 : (l & 2u) != 0;
#pragma unroll
      for (int pr = 0; pr < 2; pr++) {
        const int k0 = stage == 0 ? 2 * pr : pr, k1 = stage == 0 ? 2 * pr + 1 : pr + 2;
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const uint32_t a = r[k0][c], b = r[k1][c];
          const int send = (int)(hi ? a : b);
          const uint32_t recv =
              (uint32_t)(stage == 0 ? __builtin_amdgcn_mov_dpp(send, 0xB1, 0xf, 0xf, false)    // quad_perm [1, 0, 3, 2]
                                    : __builtin_amdgcn_mov_dpp(send, 0x4E, 0xf, 0xf, false));  // quad_perm [2, 3, 0, 1]
          r[k0][c] = hi ? recv : a;
          r[k1][c] = hi ? b : recv;
        }
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < V1U; j++) store_row((threadIdx.x & ~3u) * V1U + 4u * j + l, r[j]);
  }
};

// v1_tile_code's hook: the block's residual row from the coefficients the coder was given, kept in the lane until the
// tile is coded. Blocks with Inf / NaN (infmask) are redone by v1_tile_resid.
struct V1ResidHook {
  uint32_t& infmask;
  v1_u4 (&rows)[V1U];
  __device__ __forceinline__ void operator()(uint32_t k, const float* y, const uint32_t* u, uint32_t hdr, uint32_t K,
                                             bool inf) const
  {
    infmask |= (uint32_t)inf << k;
    float d[4];
    v1_decode_closed(u, hdr, K, d);
    rows[k] = V1ResidOut::resid(y, d);
  }
};

// Code and store one tile of y and its residual.
__device__ __forceinline__ void v1_tile_resid(const FieldDesc& F, const Params& p, float* e_out, uint32_t t, uint64_t B,
                                              uint32_t total, const V1Raw<DT_F32>& y, uint32_t lw,
                                              uint32_t* __restrict__ out32, uint64_t* __restrict__ index,
                                              uint32_t index_shift, uint32_t ntiles, const uint32_t* tab,
                                              const uint32_t* rs, uint64_t* win, uint32_t* scan_sh,
                                              uint32_t* s_special)
{
  const V1ResidOut eo(e_out, F.n[0], t);
  uint32_t infmask = 0;
  v1_u4 rows[V1U];
  v1_tile_code<DT_F32>(F, p, t, B, y, lw, index, index_shift, tab, rs, win, scan_sh, s_special,
                       V1ResidHook{infmask, rows});
  v1_tile_store(t, B, total, win, out32, ntiles);
  if (infmask) {  // Inf / NaN present: the generic coder and decoder in the lane (padding blocks' rows are dropped)
#pragma unroll
    for (uint32_t k = 0; k < V1U; k++) {
      if ((infmask >> k) & 1u) {
        float f[4], d[4];
        y.block(k, f);
        (void)rt_block_generic(f, p, d);
        rows[k] = V1ResidOut::resid(f, d);
      }
    }
  }
  eo.store_quad(rows);
}

// ----------------------------------------------------------------------------------------- tile form: the kernels
// Every kernel is a template over its parameter source PS (ParamsHost / ParamsDev, var1d_prep.h), called once at the
// top. The count kernels count vmcnt by hand, so they take the parameters WAITED: a device word is loaded and waited
// for before the ring's first raw buffer load is issued, and as a scalar load it is none vmcnt counts (the rule is
// stated at fitted_params_dev). The coders' loads are all compiler-managed; there the word's load goes out with the
// tile's others and is first used after them.
// The field's own values (k_count1d_var_tile, k_encode1d_var_tile, _big) and y = x + e (the same names with _resid)
// keep a body each where their text differs -- how a tile's loads are requested, waited for and formed into values,
// and what is called around v1_tile_code: folded into one body, the compiler schedules the field's kernels
// differently (the same instructions in another order, other registers), and so it does even when the count
// kernels' stores and totals or the oversized-tile test move into a function of their own: those stay in the kernels'
// text. Written once are the coders' LDS and tables (v1_lds), the launcher and the workspace layout.
static_assert(V1CT == 8, "the scan's group totals (gsums) cover 8 tiles");

template <int DT, class PS>
__global__ __launch_bounds__(V1T) void k_count1d_var_tile(FieldDesc F, PS ps, uint32_t ntiles,
                                                          uint64_t* __restrict__ sums, uint32_t* __restrict__ lens8,
                                                          uint32_t* __restrict__ nover, uint64_t* __restrict__ gsums)
{
  // V1CT consecutive tiles per workgroup. Full contiguous tiles are software-pipelined: tile i + 1's raw buffer loads
  // are issued before tile i is counted (hand-counted waits), and nothing is stored until the loop is done -- the
  // workgroups of a one-shot grid otherwise run in lock step, all loading and then all computing.
  const Params p = ps.template get<true>();  // a device word is loaded and waited for: nothing outstanding here
  __shared__ uint32_t red[V1CT][V1T / 64];
  const uint32_t tid = threadIdx.x, t0 = blockIdx.x * V1CT;
  if (blockIdx.x == 0 && tid == 0) *nover = 0u;  // the oversized-tile list of k_encode1d_var_tile starts empty
  const bool wide_ok = F.vec && (((uintptr_t)F.data) & 15u) == 0;
  constexpr int NL = V1Raw<DT>::N;                                 // 16-byte loads per lane per tile
  constexpr uint32_t TB = V1TILE * (DT == DT_BF16 ? 8u : 16u);     // bytes per tile
  uint32_t packed[V1CT];
  if (wide_ok && (uint64_t)(t0 + V1CT) * V1TILE <= F.n[0] / 4) {
    const v1_v4i rs = v1_rsrc((const char*)F.data + (size_t)t0 * TB, V1CT * TB);
    // a ring of PF + 1 tiles: tile i + PF is requested before tile i is counted, so PF tiles of loads stay in flight
    constexpr uint32_t PF = V1_COUNT_PF, RING = PF + 1;
    v1_u4 buf[RING][NL];
#pragma unroll
    for (uint32_t i = 0; i < PF && i < V1CT; i++)
#pragma unroll
      for (int h = 0; h < NL; h++) buf[i][h] = v1_ld16(i * TB + (tid * NL + h) * 16u, rs);
#pragma unroll
    for (uint32_t i = 0; i < V1CT; i++) {
      if (i + PF < V1CT) {
#pragma unroll
        for (int h = 0; h < NL; h++) buf[(i + PF) % RING][h] = v1_ld16((i + PF) * TB + (tid * NL + h) * 16u, rs);
      }
      // loads issued after tile i's: those of tiles i + 1 .. min(i + PF, V1CT - 1)
      v1_wait_tiles<NL>(buf[i % RING], (i + PF < V1CT ? PF : V1CT - 1 - i));
      V1Raw<DT> cur;
#pragma unroll
      for (int h = 0; h < NL; h++) {
        const v1_u4 v = buf[i % RING][h];
        cur.w[h] = make_uint4(v.x, v.y, v.z, v.w);
      }
      uint32_t lsum;
      packed[i] = v1_count_tile<DT, true>(F, p, cur, t0 + i, lsum);
      lsum = wave_sum_dpp(lsum);
      if ((tid & 63u) == 0) red[i][tid >> 6] = lsum;
    }
  } else {  // partial tiles, the padded last block, strided or unaligned input
#pragma unroll
    for (uint32_t i = 0; i < V1CT; i++) {
      uint32_t lsum = 0;
      packed[i] = 0;
      if (t0 + i < ntiles) {
        V1Raw<DT> raw;
        raw.load(F, t0 + i, wide_ok);
        packed[i] = v1_count_tile<DT>(F, p, raw, t0 + i, lsum);
      }
      lsum = wave_sum_dpp(lsum);
      if ((tid & 63u) == 0) red[i][tid >> 6] = lsum;
    }
  }
#pragma unroll
  for (uint32_t i = 0; i < V1CT; i++)
    if (t0 + i < ntiles) lens8[(size_t)(t0 + i) * V1T + tid] = packed[i];
  __syncthreads();
  if (tid < 64) {  // wave 0: the tile totals, and their sum for the scan's group totals
    uint64_t tot = 0;
    if (tid < V1CT && t0 + tid < ntiles) {
#pragma unroll
      for (uint32_t w = 0; w < V1T / 64; w++) tot += red[tid][w];
      sums[t0 + tid] = tot;
    }
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) {
      const uint32_t lo = __shfl_xor((uint32_t)tot, o, 64), hi = __shfl_xor((uint32_t)(tot >> 32), o, 64);
      tot += (uint64_t)lo | ((uint64_t)hi << 32);
    }
    if (tid == 0) gsums[blockIdx.x] = tot;
  }
}

template <int DT_X, bool HASE, class PS>
__global__ __launch_bounds__(V1T) void k_count1d_var_tile_resid(FieldDesc F, PS ps, const float* e_in, uint32_t ntiles,
                                                                uint64_t* __restrict__ sums,
                                                                uint32_t* __restrict__ lens8,
                                                                uint32_t* __restrict__ nover,
                                                                uint64_t* __restrict__ gsums)
{
  // k_count1d_var_tile's shape. Loads per lane and tile, in issue order: NX x rows (fp32: 4, bf16: 2), then with HASE
  // the V1U = 4 e rows -- NT = 8 (fp32), 6 (bf16), or 4 / 2 without e. Nothing is stored inside the loop, so vmcnt
  // counts loads only: once tile i's loads are issued, the operations issued after them are the loads of tiles
  // i + 1 .. min(i + PF, V1CT - 1), k tiles of NT each, and tile i has landed at vmcnt(k NT) (at most 3 x 8 = 24 of
  // the counter's 63).
  const Params p = ps.template get<true>();  // a device word is loaded and waited for: nothing outstanding here
  __shared__ uint32_t red[V1CT][V1T / 64];
  const uint32_t tid = threadIdx.x, t0 = blockIdx.x * V1CT;
  if (blockIdx.x == 0 && tid == 0) *nover = 0u;  // the oversized-tile list of k_encode1d_var_tile_resid starts empty
  const bool wide_ok = F.vec && v1_aligned16(F.data) && (!HASE || v1_aligned16(e_in));
  constexpr int NX = V1Raw<DT_X>::N;                                  // 16-byte x loads per lane per tile
  constexpr uint32_t TBX = V1TILE * (DT_X == DT_BF16 ? 8u : 16u);     // x bytes per tile
  constexpr uint32_t TBE = V1TILE * 16u;                              // e bytes per tile
  uint32_t packed[V1CT];
  if (wide_ok && (uint64_t)(t0 + V1CT) * V1TILE <= F.n[0] / 4) {
    const v1_v4i rsx = v1_rsrc((const char*)F.data + (size_t)t0 * TBX, V1CT * TBX);
    const v1_v4i rse = v1_rsrc((const char*)e_in + (size_t)t0 * TBE, HASE ? V1CT * TBE : 0u);
    constexpr uint32_t PF = V1_RESID_PF, RING = PF + 1;
    v1_u4 bx[RING][NX], be[HASE ? RING : 1][V1U];
    auto request = [&](uint32_t i) {
#pragma unroll
      for (int h = 0; h < NX; h++) bx[i % RING][h] = v1_ld16(i * TBX + (tid * NX + h) * 16u, rsx);
      if constexpr (HASE) {
#pragma unroll
        for (uint32_t h = 0; h < V1U; h++) be[i % RING][h] = v1_ld16(i * TBE + (tid * V1U + h) * 16u, rse);
      }
    };
#pragma unroll
    for (uint32_t i = 0; i < PF && i < V1CT; i++) request(i);
#pragma unroll
    for (uint32_t i = 0; i < V1CT; i++) {
      if (i + PF < V1CT) request(i + PF);
      v1_wait_tiles_xe<NX, HASE>(bx[i % RING], be[HASE ? i % RING : 0], (i + PF < V1CT ? PF : V1CT - 1 - i));
      V1Raw<DT_X> rx;
      V1Raw<DT_F32> re, y;
#pragma unroll
      for (int h = 0; h < NX; h++) {
        const v1_u4 v = bx[i % RING][h];
        rx.w[h] = make_uint4(v.x, v.y, v.z, v.w);
      }
#pragma unroll
      for (uint32_t h = 0; h < V1U; h++) {
        if constexpr (HASE) {
          const v1_u4 v = be[i % RING][h];
          re.w[h] = make_uint4(v.x, v.y, v.z, v.w);
        } else {
          re.w[h] = make_uint4(0u, 0u, 0u, 0u);
        }
      }
      v1_form_y<DT_X>(rx, re, y);
      uint32_t lsum;
      packed[i] = v1_count_tile<DT_F32, true>(F, p, y, t0 + i, lsum);
      lsum = wave_sum_dpp(lsum);
      if ((tid & 63u) == 0) red[i][tid >> 6] = lsum;
    }
  } else {  // partial tiles, the padded last block, n % 4 != 0
#pragma unroll
    for (uint32_t i = 0; i < V1CT; i++) {
      uint32_t lsum = 0;
      packed[i] = 0;
      if (t0 + i < ntiles) {
        V1Raw<DT_F32> y;
        v1_load_y<DT_X>(F, HASE ? e_in : nullptr, t0 + i, y);
        packed[i] = v1_count_tile<DT_F32>(F, p, y, t0 + i, lsum);
      }
      lsum = wave_sum_dpp(lsum);
      if ((tid & 63u) == 0) red[i][tid >> 6] = lsum;
    }
  }
#pragma unroll
  for (uint32_t i = 0; i < V1CT; i++)
    if (t0 + i < ntiles) lens8[(size_t)(t0 + i) * V1T + tid] = packed[i];
  __syncthreads();
  if (tid < 64) {  // wave 0: the tile totals, and their sum for the scan's group totals
    uint64_t tot = 0;
    if (tid < V1CT && t0 + tid < ntiles) {
#pragma unroll
      for (uint32_t w = 0; w < V1T / 64; w++) tot += red[tid][w];
      sums[t0 + tid] = tot;
    }
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) {
      const uint32_t lo = __shfl_xor((uint32_t)tot, o, 64), hi = __shfl_xor((uint32_t)(tot >> 32), o, 64);
      tot += (uint64_t)lo | ((uint64_t)hi << 32);
    }
    if (tid == 0) gsums[blockIdx.x] = tot;
  }
}

template <int DT, class PS>
__global__ __launch_bounds__(V1T) void k_encode1d_var_tile(FieldDesc F, PS ps, const uint64_t* __restrict__ rbase,
                                                           const uint32_t* __restrict__ lens8,
                                                           uint32_t* __restrict__ out32, uint64_t* __restrict__ index,
                                                           uint32_t index_shift, uint32_t ntiles,
                                                           uint32_t* __restrict__ over)
{
  const uint32_t t = blockIdx.x;
  const Params p = ps.template get<false>();
  // every load the tile needs is issued before anything waits (one memory round trip per workgroup): the input rows,
  // the lane's byte lengths, the pair table, the tile's stream offsets
  V1Raw<DT> raw;
  raw.load(F, t, F.vec && (((uintptr_t)F.data) & 15u) == 0);
  const uint32_t lw = lens8[(size_t)t * V1T + threadIdx.x];
  const V1Lds L = v1_lds<V1QS>();
  const uint64_t B = rbase[t];
  const uint32_t total = (uint32_t)(rbase[t + 1] - B);
  if (v1_tile_qwords(B, total) > V1QS) {  // oversized: listed for the _big kernel (over[0] = count), nothing stored
    if (threadIdx.x == 0) over[1 + atomicAdd(over, 1u)] = t;
    return;
  }
  v1_tile_code<DT>(F, p, t, B, raw, lw, index, index_shift, L.tab, L.rs, L.win, L.scan_sh, L.s_special);
  v1_tile_store(t, B, total, L.win, out32, ntiles);
}

template <int DT, class PS>
__global__ __launch_bounds__(V1T) void k_encode1d_var_tile_big(FieldDesc F, PS ps, const uint64_t* __restrict__ rbase,
                                                               const uint32_t* __restrict__ lens8,
                                                               uint32_t* __restrict__ out32,
                                                               uint64_t* __restrict__ index, uint32_t index_shift,
                                                               uint32_t ntiles, const uint32_t* __restrict__ over)
{
  const uint32_t n = over[0];
  if (blockIdx.x >= n) return;
  const Params p = ps.template get<false>();
  const V1Lds L = v1_lds<V1Q + 2>();
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t t = over[1 + i];
    const uint64_t B = rbase[t];
    const uint32_t total = (uint32_t)(rbase[t + 1] - B);
    v1_tile<DT>(F, p, t, B, total, lens8, out32, index, index_shift, ntiles, L.tab, L.rs, L.win, L.scan_sh,
                L.s_special);
    __syncthreads();  // the window and scan slots are reused by the next tile
  }
}

template <int DT_X, class PS>
__global__ __launch_bounds__(V1T) void k_encode1d_var_tile_resid(FieldDesc F, PS ps, const float* e_in, float* e_out,
                                                                 const uint64_t* __restrict__ rbase,
                                                                 const uint32_t* __restrict__ lens8,
                                                                 uint32_t* __restrict__ out32,
                                                                 uint64_t* __restrict__ index, uint32_t index_shift,
                                                                 uint32_t ntiles, uint32_t* __restrict__ over)
{
  const uint32_t t = blockIdx.x;
  const Params p = ps.template get<false>();
  // as in k_encode1d_var_tile, every load the tile needs is issued before anything waits: the x and e rows (all of
  // the lane's e rows, before any e' store), the byte lengths, the pair table, the stream offsets
  V1Raw<DT_F32> y;
  v1_load_y<DT_X>(F, e_in, t, y);
  const uint32_t lw = lens8[(size_t)t * V1T + threadIdx.x];
  const V1Lds L = v1_lds<V1QS>();
  const uint64_t B = rbase[t];
  const uint32_t total = (uint32_t)(rbase[t + 1] - B);
  if (v1_tile_qwords(B, total) > V1QS) {  // oversized: listed for the _big kernel (over[0] = count), nothing stored
    if (threadIdx.x == 0) over[1 + atomicAdd(over, 1u)] = t;
    return;
  }
  v1_tile_resid(F, p, e_out, t, B, total, y, lw, out32, index, index_shift, ntiles, L.tab, L.rs, L.win, L.scan_sh,
                L.s_special);
}

template <int DT_X, class PS>
__global__ __launch_bounds__(V1T) void k_encode1d_var_tile_big_resid(FieldDesc F, PS ps, const float* e_in,
                                                                     float* e_out, const uint64_t* __restrict__ rbase,
                                                                     const uint32_t* __restrict__ lens8,
                                                                     uint32_t* __restrict__ out32,
                                                                     uint64_t* __restrict__ index,
                                                                     uint32_t index_shift, uint32_t ntiles,
                                                                     const uint32_t* __restrict__ over)
{
  const uint32_t n = over[0];
  if (blockIdx.x >= n) return;
  const Params p = ps.template get<false>();
  const V1Lds L = v1_lds<V1Q + 2>();
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t t = over[1 + i];
    const uint64_t B = rbase[t];
    const uint32_t total = (uint32_t)(rbase[t + 1] - B);
    V1Raw<DT_F32> y;
    v1_load_y<DT_X>(F, e_in, t, y);
    const uint32_t lw = lens8[(size_t)t * V1T + threadIdx.x];
    v1_tile_resid(F, p, e_out, t, B, total, y, lw, out32, index, index_shift, ntiles, L.tab, L.rs, L.win, L.scan_sh,
                  L.s_special);
    __syncthreads();  // the window and scan slots are reused by the next tile
  }
}

// ------------------------------------------------------------------------- tile form: the workspace and the launchers

size_t var1d_tile_workspace_bytes(uint64_t nblocks) { return V1Workspace(nblocks).words * 8; }

// count -> scan -> coder -> oversized tiles, of the field's values (resid false: e_in, e_out unused) or of y = x + e
// (e_in may be null) with the residual written to e_out.
template <int DT, class PS>
static hipError_t v1_launch_tile(const FieldDesc& F, const PS& ps, bool resid, const float* e_in, float* e_out,
                                 uint32_t* out32, uint64_t* ws, uint64_t* d_total, uint64_t* index,
                                 uint32_t index_shift, const uint64_t* d_base, hipStream_t st)
{
  const V1Workspace W(F.nblocks);
  const uint32_t ntiles = W.ntiles, ncw = (ntiles + V1CT - 1) / V1CT;
  uint64_t *sums = ws, *base = ws + W.o_base, *gsums = ws + W.o_gsums;
  uint32_t *over = (uint32_t*)(ws + W.o_over), *lens8 = (uint32_t*)(ws + W.o_lens8);
  if (!resid)
    k_count1d_var_tile<DT, PS><<<ncw, V1T, 0, st>>>(F, ps, ntiles, sums, lens8, over, gsums);
  else if (e_in)
    k_count1d_var_tile_resid<DT, true, PS><<<ncw, V1T, 0, st>>>(F, ps, e_in, ntiles, sums, lens8, over, gsums);
  else
    k_count1d_var_tile_resid<DT, false, PS><<<ncw, V1T, 0, st>>>(F, ps, nullptr, ntiles, sums, lens8, over, gsums);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_scan_ranges(sums, ntiles, base, d_total, out32, d_base, st, gsums);
  if (e != hipSuccess) return e;
  const uint32_t nbig = std::min(ntiles, 1280u);  // grid-stride workgroups of the oversized-tile pass (5 per CU)
  if (!resid) {
    k_encode1d_var_tile<DT, PS><<<ntiles, V1T, 0, st>>>(F, ps, base, lens8, out32, index, index_shift, ntiles, over);
    k_encode1d_var_tile_big<DT, PS><<<nbig, V1T, 0, st>>>(F, ps, base, lens8, out32, index, index_shift, ntiles, over);
  } else {
    k_encode1d_var_tile_resid<DT, PS><<<ntiles, V1T, 0, st>>>(F, ps, e_in, e_out, base, lens8, out32, index,
                                                              index_shift, ntiles, over);
    k_encode1d_var_tile_big_resid<DT, PS><<<nbig, V1T, 0, st>>>(F, ps, e_in, e_out, base, lens8, out32, index,
                                                                index_shift, ntiles, over);
  }
  return hipGetLastError();
}

template <class PS>
static hipError_t v1_launch(const FieldDesc& F, const PS& ps, bool resid, const float* e_in, float* e_out,
                            uint32_t* out32, uint64_t* ws, uint64_t* d_total, uint64_t* index, uint32_t index_shift,
                            const uint64_t* d_base, void* stream)
{
  hipStream_t st = (hipStream_t)stream;
  if (F.dtype == DT_BF16)
    return v1_launch_tile<DT_BF16>(F, ps, resid, e_in, e_out, out32, ws, d_total, index, index_shift, d_base, st);
  return v1_launch_tile<DT_F32>(F, ps, resid, e_in, e_out, out32, ws, d_total, index, index_shift, d_base, st);
}

// x as a contiguous 1-D field: what the residual entry points are given in place of a FieldDesc
static FieldDesc v1_field1d(const void* x, int x_dtype, uint64_t nvals)
{
  FieldDesc F = {};
  F.data = x;
  F.n[0] = nvals;
  F.n[1] = F.n[2] = F.n[3] = 1;
  F.s[0] = 1;
  F.nblocks = F.bx = (uint32_t)((nvals + 3) / 4);
  F.by = F.bz = F.bw = 1;
  F.dims = 1;
  F.dtype = (uint32_t)x_dtype;
  F.vec = ((uintptr_t)x % (x_dtype == DT_BF16 ? 8u : 16u)) == 0 ? 1u : 0u;
  return F;
}

hipError_t launch_encode1d_var_tile(const FieldDesc& F, const Params& p, uint32_t* out32, uint64_t* ws,
                                    uint64_t* d_total, uint64_t* index, uint32_t index_shift, const uint64_t* d_base,
                                    void* stream)
{
  return v1_launch(F, ParamsHost{p}, false, nullptr, nullptr, out32, ws, d_total, index, index_shift, d_base, stream);
}

// gcow_encode_fitted_device (include/gcow.h): the tile form under
// Params{1, 16658, maxprec, clamp(*d_minexp)}, the word read when the kernels run -- a fit that a kernel earlier in the
// stream wrote (k_rate_table_fit) needs no host read in between, and a captured graph follows the data it is replayed
// on. Nothing on the host depends on minexp: the workspace layout, the scan and the oversized-tile list are the same.
hipError_t launch_encode1d_var_tile_fitted(const FieldDesc& F, uint32_t maxprec, const int32_t* d_minexp,
                                           uint32_t* out32, uint64_t* ws, uint64_t* d_total, uint64_t* index,
                                           uint32_t index_shift, void* stream)
{
  return v1_launch(F, ParamsDev{maxprec, d_minexp}, false, nullptr, nullptr, out32, ws, d_total, index, index_shift,
                   nullptr, stream);
}

hipError_t launch_encode_resid1d_var(const void* x, int x_dtype, uint64_t nvals, const Params& p, const float* e_in,
                                     float* e_out, uint32_t* out32, uint64_t* ws, uint64_t* d_total, uint64_t* index,
                                     uint32_t index_shift, void* stream)
{
  return v1_launch(v1_field1d(x, x_dtype, nvals), ParamsHost{p}, true, e_in, e_out, out32, ws, d_total, index,
                   index_shift, nullptr, stream);
}

// gcow_encode_residual_fitted_device (include/gcow.h): the residual form under the device word.
hipError_t launch_encode_resid1d_var_fitted(const void* x, int x_dtype, uint64_t nvals, uint32_t maxprec,
                                            const int32_t* d_minexp, const float* e_in, float* e_out, uint32_t* out32,
                                            uint64_t* ws, uint64_t* d_total, uint64_t* index, uint32_t index_shift,
                                            void* stream)
{
  return v1_launch(v1_field1d(x, x_dtype, nvals), ParamsDev{maxprec, d_minexp}, true, e_in, e_out, out32, ws, d_total,
                   index, index_shift, nullptr, stream);
}

}  // namespace gcow
