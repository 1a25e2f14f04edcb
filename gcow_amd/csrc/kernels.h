// kernels.h -- host-visible kernel launch interface (internal to libgcow.so).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec_device.h"

namespace gcow {

// Field geometry as the kernels see it: extents/strides fastest-first, unused dims have extent 1.
struct FieldDesc {
  const void* data;  // input (encode) or output (decode) device pointer
  uint64_t n[4];
  int64_t s[4];
  uint32_t bx, by, bz, bw;
  uint32_t nblocks;
  uint32_t dims;
  uint32_t dtype;
  uint32_t vec;  // rows of 4 values are contiguous and vector-aligned
};

// Workgroup range decomposition for the tile kernels.
struct TilePlan {
  uint32_t threads;    // blocks per tile (= workgroup size)
  uint32_t range;      // blocks per workgroup range (multiple of threads)
  uint32_t nranges;    // grid size
  uint32_t lds_words;  // LDS window (32-bit words)
  bool fixed;          // minbits == maxbits: offsets are b * maxbits
};

hipError_t launch_encode_fixed1d(const void* in, int dtype, uint64_t nvals, uint32_t nblocks, const Params& p,
                                 void* out, void* stream);
hipError_t launch_encode_tiles(const FieldDesc& F, const Params& p, const TilePlan& plan, uint32_t* out32,
                               uint64_t* ws_sums, uint64_t* ws_base, uint64_t* d_total, uint64_t* index,
                               uint32_t index_shift, const uint64_t* d_base, void* stream);
// in_words: stream buffer size in uint64 (0 = unknown: no LDS staging)
hipError_t launch_decode(const FieldDesc& F, const Params& p, const uint64_t* in, const uint64_t* index,
                         uint32_t chunk, uint64_t nchunks, bool fixed, uint64_t base_bits, uint64_t* end_out,
                         void* stream, uint64_t in_words = 0);
// fixed-rate 1-D whole-word blocks (maxbits 64 / 32, maxprec >= 32, minexp <= -154), contiguous fp32 output,
// base_bits % 32 == 0
hipError_t launch_decode_fixed1d(const FieldDesc& F, const Params& p, const uint64_t* in, uint64_t base_bits,
                                 void* stream);
// fixed-rate 3-D blocks of a whole number of 32-bit words (fixed3d_ok); decode needs base_bits % 32 == 0
bool fixed3d_ok(uint32_t maxbits);
hipError_t launch_encode3d_fixed(const FieldDesc& F, const Params& p, uint32_t* out32, void* stream);
hipError_t launch_decode3d_fixed(const FieldDesc& F, const Params& p, const uint32_t* in32, void* stream);
// variable-rate 1-D, contiguous fp32 output, blocks never truncated (minbits <= 1, maxbits >= 160)
// in_words: stream buffer size (0 = unknown: no LDS staging)
hipError_t launch_decode1d_var(const FieldDesc& F, const Params& p, const uint64_t* in, uint64_t in_words,
                               const uint64_t* index, uint32_t chunk, uint64_t nchunks, uint64_t base_bits,
                               uint64_t* end_out, void* stream);
// 4-D blocks (one wave per block): lens (count pass), or write at rbase (variable) / b * maxbits (fixed, rbase null)
hipError_t launch_encode4d(const FieldDesc& F, const Params& p, uint32_t* lens, const uint64_t* rbase, uint32_t* out32,
                           uint64_t* index, uint32_t index_shift, void* stream);
hipError_t launch_decode4d(const FieldDesc& F, const Params& p, const uint64_t* in, const uint64_t* index,
                           uint64_t base_bits, void* stream);
hipError_t launch_decode4d_seq(const FieldDesc& F, const Params& p, const uint64_t* in, uint64_t base_bits,
                               uint64_t* end, void* stream);
hipError_t launch_scan_blocks(const uint32_t* lens, uint32_t nblocks, uint64_t* sums, uint64_t* base, uint64_t* total,
                              uint32_t* out32, const uint64_t* d_base, void* stream);
// 2-D / 3-D tiles (gcow_blocks.hip); launch_encode_tiles forwards d >= 2 here
hipError_t launch_encode_tiles23(const FieldDesc& F, const Params& p, const TilePlan& plan, uint32_t* out32,
                                 uint64_t* ws_sums, uint64_t* ws_base, uint64_t* d_total, uint64_t* index,
                                 uint32_t index_shift, const uint64_t* d_base, void* stream);
// gsums (optional): totals of consecutive groups of 8 ranges, which the many-workgroup scan sums instead of the ranges
hipError_t launch_scan_ranges(const uint64_t* sums, uint32_t nranges, uint64_t* base, uint64_t* total, uint32_t* out32,
                              const uint64_t* d_base, void* stream, const uint64_t* gsums = nullptr);
hipError_t launch_set_u64(uint64_t* p, uint64_t v, void* stream);
// Single-pass 1-D variable-rate encoder (var1d.hip): minbits <= 1, maxbits >= 160; ws = var1d_sp_workspace_bytes().
size_t var1d_sp_workspace_bytes(uint64_t nblocks);
// A/B variants of the 1-D variable-rate encoder, for tests and measurement tools only (set through the C ABI's
// gcow_debug_set_var1d_variant; the product default is the tile form): form 0 = tile, 1 = range (count + scan +
// k_encode1d_var), 2 = the look-back single pass; spin = polls before a missing predecessor's total is computed
// locally (< 0: V1SPIN); stats != 0: the look-back records its statistics in the workspace.
struct Var1dVariant {
  int form, spin, stats;
};
extern Var1dVariant g_var1d_variant;

hipError_t launch_encode1d_var_sp(const FieldDesc& F, const Params& p, uint32_t* out32, uint64_t* ws,
                                  uint64_t* d_total, uint64_t* index, uint32_t index_shift, const uint64_t* d_base,
                                  void* stream);
// The default 1-D variable-rate form (var1d.hip): count per tile + scan + the tile coder placed by the scan;
// ws = var1d_tile_workspace_bytes().
size_t var1d_tile_workspace_bytes(uint64_t nblocks);
hipError_t launch_encode1d_var_tile(const FieldDesc& F, const Params& p, uint32_t* out32, uint64_t* ws,
                                    uint64_t* d_total, uint64_t* index, uint32_t index_shift, const uint64_t* d_base,
                                    void* stream);
// Error feedback (enc_resid1d.hip). Fused: the lean fixed-rate domain (maxbits 64 / 32, maxprec >= 32, minexp <= -154),
// contiguous 16-byte aligned rows; y = x + e_in (e_in null: zeros) is coded to out and e_out = finite(y - decode);
// e_in == e_out allowed. Composed path: y = x + e_in, then e = finite(y - e) on a buffer that holds the decode.
hipError_t launch_encode_resid1d(const void* in, int dtype, uint64_t nvals, const Params& p, const float* e_in,
                                 float* e_out, void* out, void* stream);
// Fused at variable rate (var1d.hip): minbits <= 1 and maxbits >= 160, x (fp32 / bf16), e_in (or null) and e_out
// 16-byte aligned; the tile form of the encoder on y = x + e_in, whose code pass writes e_out = finite(y - decode)
// from the coder's own coefficients. ws = var1d_tile_workspace_bytes(), the tile form's layout; index as
// launch_encode1d_var_tile writes it. Always the tile form: g_var1d_variant does not apply.
hipError_t launch_encode_resid1d_var(const void* x, int x_dtype, uint64_t nvals, const Params& p, const float* e_in,
                                     float* e_out, uint32_t* out32, uint64_t* ws, uint64_t* d_total, uint64_t* index,
                                     uint32_t index_shift, void* stream);
hipError_t launch_resid_form(const void* in, int dtype, uint64_t nvals, const float* e_in, float* y, void* stream);
hipError_t launch_resid_finish(const float* y, float* e, uint64_t nvals, void* stream);
// Fused round trip (roundtrip1d.hip): out = decode(encode(in)) of nvals contiguous values, no stream. domain selects
// the kernel: Lean = the lean fixed-rate domain above, Var = minbits <= 1 and maxbits >= 160 (both need 16-byte aligned
// in and out; the partial last block goes through the generic kernel), Generic = anything. total (optional, zeroed by
// the caller) has every block's bit length added to it; pass null for fixed-rate sets.
enum { kRoundtripLean = 0, kRoundtripVar = 1, kRoundtripGeneric = 2 };
hipError_t launch_roundtrip1d(const void* in, int in_dtype, uint64_t nvals, const Params& p, int domain, void* out,
                              int out_dtype, uint64_t* total, void* stream);
// Round trip over a tensor list (roundtrip_list1d.hip): the field X is the concatenation of the plan's segments. The
// plan (gcow_roundtrip_list_plan, gcow_api.cpp) is one buffer: RtListHeader, then ndirect RtListDirect, ngather
// RtListGather and nsegs + 1 RtListSeg (the last one a sentinel: start = nvals). A chunk is 256 * GCOW_RT_U blocks of
// X (kRtListChunkBlocks; roundtrip_list1d.hip asserts the two agree).
constexpr uint32_t kRtListChunkBlocks = 2048;
constexpr uint32_t kRtListMagic = 0x4c545267u;  // "gRTL"
struct RtListDirect {  // a chunk whose nb whole blocks lie in one segment, rows at 4-byte aligned addresses
  uint64_t in, out;    // the chunk's first row
  uint32_t nb, pad;
};
struct RtListGather {  // any other chunk: blocks b0 .. min(b0 + kRtListChunkBlocks, nblocks) - 1 of X
  uint32_t b0;
  uint32_t seg_lo, seg_hi;  // the segments holding the chunk's first and last value
  uint32_t pad;
};
struct RtListSeg {  // a non-empty segment: values start .. next start - 1 of X
  uint64_t start, in, out;
};
struct RtListHeader {
  uint32_t magic, domain;  // kRoundtrip*
  uint32_t in_dtype, out_dtype;
  uint32_t nsegs, ndirect, ngather, pad;
  uint64_t nvals;
  uint32_t params[4];
  uint64_t off_direct, off_gather, off_segs, bytes;  // byte offsets into the plan; bytes = the plan's used size
};
static_assert(sizeof(RtListDirect) == 24 && sizeof(RtListGather) == 16 && sizeof(RtListSeg) == 24 &&
              sizeof(RtListHeader) == 88, "plan layout");
// h: the plan's header (HOST copy); d_plan: the whole plan on the DEVICE. total as launch_roundtrip1d's.
hipError_t launch_roundtrip_list1d(const RtListHeader& h, const void* d_plan, const Params& p, uint64_t* total,
                                   void* stream);
// Round trip over a tensor list with a tolerance relative to each tensor (roundtrip_rel1d.hip): every tensor is a
// field of its own, coded with minexp_s = max(emax_s - rel_bits, kRtRelMinExpFloor), emax_s the exponent of the
// tensor's largest finite magnitude, which a first pass leaves in absmax[seg]. The plan (gcow_roundtrip_rel_plan,
// gcow_api.cpp) is one buffer: RtRelHeader, then ndirect RtRelDirect, ngather RtRelGather and npieces RtRelPiece.
// Blocks are each tensor's own. A tensor's whole blocks run direct, in chunks of up to kRtListChunkBlocks, when it has
// at least kRtRelMinDirectBlocks of them and its rows lie at 4-byte aligned addresses; every other block (the partial
// last block of any tensor, short tensors, rows off 4 bytes) is a gather block. Gather blocks are numbered through
// the pieces in list order (virtual blocks) and cut into chunks of kRtRelGatherBlocks: one block per lane, since a gather
// lane's time is a chain of dependent loads (the bisection, then its values) that only more workgroups shorten.
constexpr uint32_t kRtRelMagic = 0x4c525267u;  // "gRRL"
constexpr uint32_t kRtRelMinDirectBlocks = 256;
constexpr uint32_t kRtRelGatherBlocks = 256;
constexpr int32_t kRtRelMinExpFloor = -94;  // blocks with emax <= -98 then have precision 0 and decode to +0
constexpr uint32_t kRtRelMaxBits = 24;
constexpr int32_t kRtRelHeadroom = 2;  // a maximum in the top binade: minexp <= floor(log2(2^128 - a)) - this (rel_params)
struct RtRelDirect {  // nb whole blocks of tensor seg (the caller's numbering), rows at 4-byte aligned addresses
  uint64_t in, out;   // the chunk's first row
  uint32_t nb, seg;
};
struct RtRelGather {  // virtual blocks vb0 .. vb0 + nb - 1, which lie in pieces p_lo .. p_hi
  uint32_t vb0, nb;
  uint32_t p_lo, p_hi;
};
struct RtRelPiece {  // the gather blocks of one tensor: its blocks b0 .. ceil(n / 4) - 1 are virtual blocks vb ..
  uint64_t in, out;  // the tensor's first value
  uint64_t n;        // the tensor's values
  uint32_t vb, b0;
  uint32_t seg, pad;
};
struct RtRelHeader {
  uint32_t magic, in_dtype, out_dtype, nsegs;  // nsegs: the caller's list, empty tensors included
  uint32_t nlive, ndirect, ngather, npieces;
  uint64_t nvals, nblocks;
  uint64_t off_direct, off_gather, off_pieces, bytes;  // byte offsets into the plan; bytes = the plan's used size
};
static_assert(sizeof(RtRelDirect) == 24 && sizeof(RtRelGather) == 16 && sizeof(RtRelPiece) == 40 &&
              sizeof(RtRelHeader) == 80, "plan layout");
// h: the plan's header (HOST copy); d_plan: the whole plan on the DEVICE. absmax: DEVICE, h.nsegs words, written whole.
// total (optional): set to the sum of every block's bit length.
hipError_t launch_roundtrip_rel1d(const RtRelHeader& h, const void* d_plan, uint32_t rel_bits, uint32_t maxprec,
                                  uint32_t* absmax, uint64_t* total, void* stream);
// Rate table (rate_table1d.hip): table[t], t < kRateTableEntries, = the stream length of the contiguous 1-D field F
// (fp32 / bf16, any element-aligned address) under expert(1, 16658, maxprec, kRateTableMinExpLo + t), i.e. what
// launch_encode1d_var_tile leaves in *d_total. ws: rate_table_workspace_bytes(), 8-byte aligned; neither ws nor table
// needs zeroing. A workgroup covers kRateTableTileValues values per iteration of its grid-stride loop.
constexpr int32_t kRateTableMinExpLo = -154;
constexpr uint32_t kRateTableEntries = 288;
constexpr uint32_t kRateTableTileValues = 4096;
size_t rate_table_workspace_bytes();
hipError_t launch_rate_table1d(const FieldDesc& F, uint32_t maxprec, uint64_t* table, uint64_t* ws, void* stream);
// The table of y = fadd(x, e_in) (x = F, fp32 / bf16 widened exactly; e_in fp32 at any 4-byte aligned address, null:
// launch_rate_table1d), i.e. what launch_encode_resid1d_var leaves in *d_total. y is formed in registers and never
// stored; both rows 16-byte aligned take the wide loads, else every tile is gathered. ws and table as above.
hipError_t launch_rate_table1d_resid(const FieldDesc& F, const float* e_in, uint32_t maxprec, uint64_t* table,
                                     uint64_t* ws, void* stream);
// The two ends of every table pass (rate_table1d.hip): the workspace zeroed by a kernel, in stream order; the
// workspace's two 288-bin arrays summed into the table of a field of nblocks blocks.
hipError_t launch_rate_table_zero(uint64_t* ws, void* stream);
hipError_t launch_rate_table_finish(const uint64_t* ws, uint64_t nblocks, uint64_t* table, void* stream);
// The table of the concatenation X of a tensor list (rate_table_list1d.hip): what launch_rate_table1d writes for the
// contiguous X of the plan's input dtype, read where the tensors lie through the plan of launch_roundtrip_list1d (any
// domain's plan has the segment table; a plan of kRoundtripVar has direct chunks too). h: the plan's header (HOST
// copy); d_plan: the whole plan on the DEVICE; only the input pointers are read. ws and table as above. One launch: a
// workgroup takes items blockIdx.x, + grid, ... of the gather units (8 per gather chunk, 256 blocks each) followed by
// the direct chunks, and the grid is min(items, kRateTableListMaxGrid).
constexpr uint32_t kRateTableListMaxGrid = 1024;
hipError_t launch_rate_table_list1d(const RtListHeader& h, const void* d_plan, uint32_t maxprec, uint64_t* table,
                                    uint64_t* ws, void* stream);
// The fit on the device (rate_table1d.hip k_rate_table_fit; include/gcow.h gcow_fit has this layout): the smallest t
// with table[t] <= budget -> {kRateTableMinExpLo + t, 0, table[t]}; none -> {the last entry's minexp, 1, table[287]}.
// One workgroup of kRateTableEntries lanes; the record is written with plain stores and nothing past it.
struct RateFit {
  int32_t minexp;
  uint32_t status;
  uint64_t bits;
};
static_assert(sizeof(RateFit) == 16 && alignof(RateFit) == 8, "gcow_fit");
hipError_t launch_rate_table_fit(const uint64_t* table, uint64_t budget_bits, RateFit* fit, void* stream);
// The same kernel, one workgroup per table: fits[s] from tables[s] (288 words each) against budgets[s] (DEVICE), over
// the entries at minexp >= minexp_floor only (none fits: {133, 1, tables[s][287]}). minexp_floor = -154, ntables = 1:
// launch_rate_table_fit with the budget in device memory.
hipError_t launch_rate_table_fit_batch(const uint64_t* tables, uint32_t ntables, const uint64_t* budgets,
                                       int32_t minexp_floor, RateFit* fits, void* stream);
// A table per tensor of a list (rate_table_rel1d.hip): tables[s] (288 words, the caller's numbering, empty tensors
// included: an all-zero row) is what launch_rate_table1d writes for tensor s as a field of its own, read through the
// plan of launch_roundtrip_rel1d as it is (only the input pointers are read). ws: rate_table_rel_workspace_bytes(nsegs)
// = kRateTableRelWords words per tensor (the two arrays and the tensor's block count, which the pass takes), zeroed by a
// kernel in stream order. One launch over the plan: the gather chunks (one workgroup each), then the direct chunks cut
// into min(ndirect, kRateTableRelMaxGrid) contiguous runs; then launch_rate_table_finish_batch, one workgroup per table
// (table s from the words at ws + s * stride_words, its block count from word count_word of them).
constexpr uint32_t kRateTableRelWords = 2 * kRateTableEntries + 1;
constexpr uint32_t kRateTableRelMaxGrid = 1024;
size_t rate_table_rel_workspace_bytes(uint32_t nsegs);
hipError_t launch_rate_table_finish_batch(const uint64_t* ws, uint32_t ntables, uint64_t stride_words,
                                          uint32_t count_word, uint64_t* tables, void* stream);
hipError_t launch_rate_table_rel1d(const RtRelHeader& h, const void* d_plan, uint32_t maxprec, uint64_t* tables,
                                   uint64_t* ws, void* stream);
// Device-parameter ("fitted") forms: Params{1, 16658, maxprec, clamp(*d_minexp, -154, 133)} with the word read on the
// device when the kernels run (fitted_params_dev, var1d_prep.h). Nothing on the host depends on minexp.
// The tile-form kernels of var1d.hip are templates over their parameter source (ParamsHost / ParamsDev, var1d_prep.h):
// the two launchers below run the kernels of launch_encode1d_var_tile / launch_encode_resid1d_var with ParamsDev. The
// round trip (roundtrip1d.hip) keeps kernels of its own for the device word.
// The tile form of the 1-D variable-rate encoder (var1d.hip), ws = var1d_tile_workspace_bytes(): every output as
// launch_encode1d_var_tile writes it under that set (no d_base). Always the tile form: g_var1d_variant does not apply.
hipError_t launch_encode1d_var_tile_fitted(const FieldDesc& F, uint32_t maxprec, const int32_t* d_minexp,
                                           uint32_t* out32, uint64_t* ws, uint64_t* d_total, uint64_t* index,
                                           uint32_t index_shift, void* stream);
// launch_encode_resid1d_var under that set: the same arguments, workspace layout and outputs (stream, *d_total, index,
// e_out; e_in null: zeros, e_in == e_out allowed); x, e_in and e_out 16-byte aligned.
hipError_t launch_encode_resid1d_var_fitted(const void* x, int x_dtype, uint64_t nvals, uint32_t maxprec,
                                            const int32_t* d_minexp, const float* e_in, float* e_out, uint32_t* out32,
                                            uint64_t* ws, uint64_t* d_total, uint64_t* index, uint32_t index_shift,
                                            void* stream);
// launch_roundtrip1d under that set: rows16 (in and out 16-byte aligned) selects kRoundtripVar with the generic kernel
// for the partial last block, else kRoundtripGeneric throughout. total as launch_roundtrip1d's.
hipError_t launch_roundtrip1d_fitted(const void* in, int in_dtype, uint64_t nvals, uint32_t maxprec,
                                     const int32_t* d_minexp, bool rows16, void* out, int out_dtype, uint64_t* total,
                                     void* stream);
// launch_roundtrip_list1d under that set, for a plan of kRoundtripVar (roundtrip_list1d.hip keeps _fitted twins of its
// two no-budget kernels). total: required, zeroed by the caller.
hipError_t launch_roundtrip_list1d_fitted(const RtListHeader& h, const void* d_plan, uint32_t maxprec,
                                          const int32_t* d_minexp, uint64_t* total, void* stream);
// launch_roundtrip_rel1d with tensor s under Params{1, 16658, maxprec, clamp(d_minexp[s * stride_words], -154, 133)},
// the words read on the device (roundtrip_rel1d.hip: the same two kernels over another parameter source; no first
// pass). total (optional): set to the sum of every block's bit length.
hipError_t launch_roundtrip_rel1d_fitted(const RtRelHeader& h, const void* d_plan, uint32_t maxprec,
                                         const int32_t* d_minexp, uint32_t stride_words, uint64_t* total, void* stream);
// The segmented 1-D codec (seg1d.hip; include/gcow.h "Segmented fields"). The plan (gcow_seg_plan, gcow_api.cpp) is one
// buffer without pointers: SegHeader, then nlive + 1 SegEnt -- the non-empty tensors in list order and a sentinel
// {nvals, nvb, nsegs} -- and ntiles words, one per tile of kSegTileBlocks virtual blocks: the entry of the tensor that
// holds the tile's first block, and bit 31 set when every block of the tile is a whole block of that tensor.
constexpr uint32_t kSegMagic = 0x4c475367u;  // "gSGL"
constexpr uint32_t kSegTileBlocks = 1024;
struct SegEnt {
  uint64_t off;  // the tensor's first value in the buffer
  uint32_t vb0;  // its first virtual block
  uint32_t seg;  // its number in the caller's list
};
struct SegHeader {
  uint32_t magic, dtype, nsegs, nlive;
  uint64_t nvals, nvb;  // values, virtual blocks
  uint32_t ntiles, nuniform;
  uint64_t off_ents, off_tiles, bytes;  // byte offsets into the plan; bytes = the plan's used size
};
static_assert(sizeof(SegEnt) == 16 && sizeof(SegHeader) == 64, "plan layout");
// ws = seg1d_workspace_bytes(nvb), the V1Workspace layout; stream, *d_total, index as launch_encode1d_var_tile writes
// them for one field of nvb blocks (no d_base); tensor s under clamp(d_minexp[s * stride_words], -154, 133).
size_t seg1d_workspace_bytes(uint64_t nvb);
hipError_t launch_encode_seg1d(const SegHeader& H, const void* d_plan, const void* in, uint32_t maxprec,
                               const int32_t* d_minexp, uint32_t stride_words, uint32_t* out32, uint64_t* ws,
                               uint64_t* d_total, uint64_t* index, uint32_t index_shift, void* stream);
// mean of nstreams segmented streams (index every chunk = 8 or 16 virtual blocks, index_words entries apart); stream r
// reads its words at d_minexp[r * stream_stride_words + s * stride_words]; out: the buffer's first value.
hipError_t launch_decode_mean_seg1d(const SegHeader& H, const void* d_plan, uint32_t maxprec, const int32_t* d_minexp,
                                    uint32_t stride_words, uint64_t stream_stride_words, const uint64_t* in,
                                    uint64_t stream_words, uint32_t nstreams, const uint64_t* index,
                                    uint64_t index_words, uint32_t chunk, void* out, int out_dtype, void* stream);
// The residual form of the segmented encoder and the per-tensor tables of y = x + e (seg_resid1d.hip; include/gcow.h
// "Segmented fields with a residual"). e_in: fp32 parallel to the buffer, null = zeros; e_out: fp32, may be e_in.
// Stream, *d_total, index and ws as launch_encode_seg1d's for the fp32 array y; e_out receives finite(y - decode).
hipError_t launch_encode_seg_resid1d(const SegHeader& H, const void* d_plan, const void* in, const float* e_in,
                                     float* e_out, uint32_t maxprec, const int32_t* d_minexp, uint32_t stride_words,
                                     uint32_t* out32, uint64_t* ws, uint64_t* d_total, uint64_t* index,
                                     uint32_t index_shift, void* stream);
// tables[s] (288 words, the caller's numbering, an all-zero row for an empty tensor): launch_rate_table1d_resid's table
// of tensor s with its slice of e_in. ws: rate_table_rel_workspace_bytes(nsegs), zeroed by a kernel in stream order.
hipError_t launch_rate_table_seg1d(const SegHeader& H, const void* d_plan, const void* in, const float* e_in,
                                   uint32_t maxprec, uint64_t* tables, uint64_t* ws, void* stream);
// The words of a relative tolerance over a segmented field (seg_resid1d.hip; include/gcow.h "Relative tolerance over a
// segmented field"): absmax[s] (nsegs words, zeroed by a kernel in stream order) = the largest finite |fadd(x, e_in)| of
// tensor s as bits, and d_minexp[s * stride_words] = rel_minexp(absmax[s], rel_bits) (rel_minexp.h), an empty tensor's
// the floor. At most three launches: zero, the pass over min(ntiles, kRateTableRelMaxGrid) runs of tiles, the words.
hipError_t launch_seg_rel_minexp1d(const SegHeader& H, const void* d_plan, const void* in, const float* e_in,
                                   uint32_t rel_bits, uint32_t* absmax, int32_t* d_minexp, uint32_t stride_words,
                                   void* stream);
hipError_t launch_copy_pattern1d(const void* in, int dtype, uint64_t nvals, uint32_t wb, void* out, void* stream);
// *flag = 0, then 1 if a[i] != b[i] for any i < n
hipError_t launch_words_differ(const uint64_t* a, const uint64_t* b, uint64_t n, uint64_t* flag, void* stream);
hipError_t launch_prepend_header(uint64_t* dst, uint32_t off, const uint64_t* src, const uint64_t* d_bits,
                                 const uint64_t* header, uint64_t max_words, uint64_t* d_total, void* stream);
hipError_t launch_stitch(uint64_t* dst, uint64_t off, const uint64_t* src, uint64_t bits, void* stream);
// all shards of a sharded variable-rate stream in one launch (dst written whole: no zeroing needed)
hipError_t launch_stitch_shards(uint64_t* dst, uint64_t dst_words, const uint64_t* src, uint64_t shard_words,
                                const uint64_t* lens, uint32_t nshards, void* stream);
// GCOW_INDEX_PACKED16 (include/gcow.h): one uint64 per 16 blocks, the 8-block midpoint as a 16-bit offset on top
constexpr uint32_t kIndexPacked16 = 0x1010u;
// packed16 index (ceil(n8 / 2) entries) from an index every 8 blocks (n8 entries)
hipError_t launch_index_pack16(const uint64_t* idx8, uint64_t n8, uint64_t* out, void* stream);
// mean of nstreams 1-D streams (fixed rate: any params; variable: any params, index every 8 or 16 blocks or packed16)
hipError_t launch_decode_mean1d(const FieldDesc& F, const Params& p, const uint64_t* in, uint64_t stream_words,
                                uint32_t nstreams, const uint64_t* index, uint64_t index_words, void* stream,
                                uint32_t chunk = 16);  // chunk: variable rate's index stride, 8 or 16, or kIndexPacked16
// W stream pieces straight into the stream of their mean (mean_enc1d.hip): the lean fixed-rate domain, no index; the
// values gcow_decode_mean_device gives are coded as launch_encode_fixed1d codes them (e_out null) or, with e_out, as
// launch_encode_resid1d codes them with e_in (null: zeros; e_in == e_out allowed; 16-byte aligned rows)
hipError_t launch_decode_mean_encode_fixed1d(uint64_t nvals, const Params& p, const uint64_t* in,
                                             uint64_t stream_words, uint32_t nstreams, const float* e_in, float* e_out,
                                             void* out, void* stream);
hipError_t launch_stage(int which, int dims, const void* a, const void* b, uint32_t n, void* out, uint32_t x0,
                        uint32_t x1, void* out2, uint32_t slot_words, void* stream);
hipError_t launch_fill_normal(float* out, uint64_t count, double sigma, uint64_t seed, int inject, void* stream);

}  // namespace gcow
