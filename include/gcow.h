/*
 * gcow.h -- MI355X-native ZFP-style gradient codec: the C ABI (libgcow.so).
 *
 * Part 1 is the drop-in boundary: the reference's sw/ encoder/decoder call surface with the same type layouts,
 * names, argument meaning and return values (fpgasystems/gcow sw/include/{types,zfp,stream,common}.h), each
 * declaration citing the reference interface it replaces. The codec behind it runs as hand-written CDNA4 (gfx950)
 * HIP kernels; there is no CPU codec in libgcow.so.
 *
 * Part 2 is the device API the drop-in layer is built on: device pointers, an explicit hipStream_t (passed as
 * void*), explicit status codes. No torch/HIP types appear in any signature.
 *
 * Deviations from sw/ (all documented in INTEGRATION.md):
 *   - 1-D (dim = 1) and 3-D inputs are supported (sw/ only encodes 2-D: sw/src/zfp.c:12-24, common.c:122-125).
 *   - data may be a device pointer; it is then encoded in place on the GPU. free_zfp_input() frees host data
 *     exactly as sw/ does (sw/src/common.c:54-62) but never frees device memory it does not own.
 *   - zfp_decompress() decodes with libzfp 0.5.5 semantics (block size 4^d); sw/'s decoder passes dim where the
 *     block size is needed (sw/src/decode.c:193-202) and is not reproduced.
 *   - dtype_bf16 (extension): bf16 values are widened exactly to fp32 and coded by the fp32 codec.
 *   - the library never prints (sw/src/common.c:109,190,193 do).
 */
#ifndef GCOW_H
#define GCOW_H

#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ================================================================================================
 * Part 1 -- drop-in sw/ surface
 * ============================================================================================== */

/* sw/include/types.h:8-21 */
typedef unsigned char uchar;
typedef unsigned short ushort;
typedef unsigned int uint;
typedef unsigned long ulong;
typedef int8_t int8;
typedef uint8_t uint8;
typedef int16_t int16;
typedef uint16_t uint16;
typedef int32_t int32;
typedef uint32_t uint32;
typedef int64_t int64;
typedef uint64_t uint64;

/* sw/include/types.h:24 -- 64-bit stream words, bits appended LSB-first, words little-endian */
typedef uint64 stream_word;

/* sw/include/types.h:29-36 */
typedef enum {
  zfp_null = 0,
  zfp_expert = 1,
  zfp_fixed_rate = 2,
  zfp_fixed_precision = 3,
  zfp_fixed_accuracy = 4,
  zfp_reversible = 5
} zfp_mode;

/* sw/include/types.h:39-45 (+ dtype_bf16 extension) */
typedef enum {
  dtype_none = 0,
  dtype_int32 = 1,
  dtype_int64 = 2,
  dtype_float = 3,
  dtype_double = 4,
  dtype_bf16 = 5
} data_type;

/* sw/include/types.h:51-56 -- zero extents for unused dimensions, zero stride = contiguous a[nw][nz][ny][nx] */
typedef struct {
  data_type dtype;
  void* data;
  size_t nx, ny, nz, nw;
  ptrdiff_t sx, sy, sz, sw;
} zfp_input;

/* sw/include/stream.h:6-16 */
typedef struct stream stream;
struct stream {
  size_t buffered_bits;
  stream_word buffer;
  stream_word* begin;
  ptrdiff_t idx;
  ptrdiff_t end;
};

/* sw/include/types.h:58-65 */
typedef struct {
  uint minbits;
  uint maxbits;
  uint maxprec;
  int minexp;
  stream* data;
} zfp_output;

/* sw/include/common.h:10-13 */
#define ZFP_MIN_BITS 1
#define ZFP_MAX_BITS 16658
#define ZFP_MAX_PREC 64
#define ZFP_MIN_EXP -1074
#define ZFP_HEADER_MAX_BITS 148

/* ---- parameters / descriptors (sw/include/types.h:107-121, sw/src/common.c) ---- */
double set_zfp_output_accuracy(zfp_output* output, double tolerance);      /* common.c:6-21 */
zfp_input* alloc_zfp_input(void);                                           /* common.c:26-36 */
zfp_output* alloc_zfp_output(void);                                         /* common.c:41-52 */
void free_zfp_input(zfp_input* input);                                      /* common.c:54-62 */
void free_zfp_output(zfp_output* output);                                   /* common.c:64-75 */
void cleanup(zfp_input* input, zfp_output* output);                         /* common.c:77-81 */
zfp_input* init_zfp_input(void* data, data_type dtype, uint dim, ...);     /* common.c:83-103 (dim 1 added) */
zfp_output* init_zfp_output(const zfp_input* input);                        /* common.c:105-115 */
uint is_reversible(const zfp_output* output);                               /* common.c:117-120 */
uint get_input_dimension(const zfp_input* input);                           /* common.c:122-125 (1-D added) */
size_t get_input_num_blocks(const zfp_input* input);                        /* common.c:127-143 */
size_t get_input_size(const zfp_input* input, size_t* shape);               /* common.c:145-164 */
size_t get_dtype_size(data_type dtype);                                     /* common.c:166-180 */
uint get_input_precision(const zfp_input* input);                           /* common.c:182-185 */
size_t get_max_output_bytes(const zfp_output* output, const zfp_input* input); /* common.c:187-224 */
uint get_precision(int maxexp, uint maxprec, int minexp, int dim);          /* common.c:226-229 */
int exceeded_maxbits(uint maxbits, uint maxprec, uint size);                /* common.c:232-236 */

/* Extensions: the other libzfp 0.5.5 parameter setters (the Python caller uses rate / precision / accuracy,
 * hw/models/train_imagenet.py:459-464). */
double set_zfp_output_rate(zfp_output* output, double rate, uint dim);
uint set_zfp_output_precision(zfp_output* output, uint precision);
int set_zfp_output_expert(zfp_output* output, uint minbits, uint maxbits, uint maxprec, int minexp);

/* ---- array codec (sw/include/zfp.h:4-7, sw/src/zfp.c) ---- */
size_t zfp_compress(zfp_output* output, const zfp_input* input);            /* zfp.c:10-28 */
size_t zfp_decompress(zfp_output* output, const zfp_input* input);          /* zfp.c:58-76 */

/* ---- bit stream (sw/include/stream.h:18-33, sw/src/stream.c) ---- */
stream* stream_init(void* buffer, size_t bytes);                            /* stream.c:160-169 */
void stream_rewind(stream* s);                                              /* stream.c:153-158 */
size_t stream_size_bytes(const stream* s);                                  /* stream.c:176-179 */
size_t stream_flush(stream* s);                                             /* stream.c:132-138 */
uint64 stream_woffset(stream* s);                                           /* stream.c:141-144 */
uint64 stream_roffset(stream* s);                                           /* stream.c:147-150 */
void stream_pad(stream* s, uint64 n);                                       /* stream.c:121-129 */
stream_word stream_read_word(stream* s);                                    /* stream.c:6-15 */
void stream_write_word(stream* s, stream_word value);                       /* stream.c:18-26 */
uint64 stream_read_bits(stream* s, size_t n);                               /* stream.c:29-58 */
uint64 stream_write_bits(stream* s, uint64 value, size_t n);                /* stream.c:61-92 */
uint stream_read_bit(stream* s);                                            /* stream.c:95-106 */
uint stream_write_bit(stream* s, uint bit);                                 /* stream.c:109-118 */
void stream_rseek(stream* s, uint64 offset);                                /* stream.c:182-197 */
void stream_skip(stream* s, uint64 n);                                      /* stream.c:200-203 */
size_t stream_algin_next_word(stream* s);                                   /* stream.c:206-211 */

/* ---- block API (sw/include/encode.h:17-81, decode.h:8-12), batched onto the GPU stage kernels ---- */
void gather_2d_block(float* block, const float* raw, ptrdiff_t sx, ptrdiff_t sy);            /* encode.c:62-70 */
void gather_partial_2d_block(float* block, const float* raw, size_t nx, size_t ny, ptrdiff_t sx,
                             ptrdiff_t sy);                                                   /* encode.c:72-88 */
void gather_4d_block(float* block, const float* raw, ptrdiff_t sx, ptrdiff_t sy, ptrdiff_t sz,
                     ptrdiff_t sw);                                                           /* encode.c:90-99 */
void gather_partial_4d_block(float* block, const float* raw, size_t nx, size_t ny, size_t nz, size_t nw,
                             ptrdiff_t sx, ptrdiff_t sy, ptrdiff_t sz, ptrdiff_t sw);        /* encode.c:101-126 */
int get_scaler_exponent(float x);                                           /* encode.c:128-140 */
int get_block_exponent(const float* block, uint n);                         /* encode.c:142-152 */
void fwd_cast_block(int32* iblock, const float* fblock, uint n, int emax); /* encode.c:178-187 */
void fwd_decorrelate_2d_block(int32* iblock);                               /* encode.c:251-260 */
void fwd_reorder_int2uint(uint32* ublock, const int32* iblock, const uchar* perm, uint n); /* encode.c:269-275 */
uint encode_all_bitplanes(stream* const s, const uint32* const ublock, uint maxprec, uint block_size);
                                                                            /* encode.c:343-408 */
uint encode_partial_bitplanes(stream* const s, const uint32* const ublock, uint maxbits, uint maxprec,
                              uint block_size);                             /* encode.c:279-339 */
uint encode_iblock(stream* const out_data, uint minbits, uint maxbits, uint maxprec, int32* iblock,
                   size_t dim);                                             /* encode.c:412-455 */
uint encode_fblock(zfp_output* output, const float* fblock, size_t dim);   /* encode.c:457-495 */
uint decode_fblock(zfp_output* output, float* fblock, size_t dim);         /* decode.c:220-253 */
void scatter_2d_block(const float* block, float* raw, ptrdiff_t sx, ptrdiff_t sy);           /* decode.c:27-34 */
void scatter_partial_2d_block(const float* block, float* raw, size_t nx, size_t ny, ptrdiff_t sx,
                              ptrdiff_t sy);                                                  /* decode.c:36-42 */

/* PERM_2D (sw/include/types.h:71-97) is exported as data for fwd_reorder_int2uint callers. */
extern const uchar PERM_2D[16];

/* ================================================================================================
 * Part 2 -- device API (what the drop-in layer and the Python/torch host binding call)
 * ============================================================================================== */

typedef enum {
  GCOW_OK = 0,
  GCOW_ERR_INVALID = 1,     /* bad arguments / parameters */
  GCOW_ERR_CAPACITY = 2,    /* output buffer smaller than the bound gcow_max_output_bytes() */
  GCOW_ERR_HIP = 3,         /* a HIP runtime call failed (gcow_last_error() has the text) */
  GCOW_ERR_NODEVICE = 4,    /* no gfx950 device / kernels not loadable */
  GCOW_ERR_UNSUPPORTED = 5  /* valid but not supported (e.g. int32/int64/double dtypes) */
} gcow_status;

/* The four ZFP expert parameters (sw/include/types.h:58-62). */
typedef struct {
  uint minbits, maxbits, maxprec;
  int minexp;
} gcow_params;

const char* gcow_status_string(gcow_status s);
const char* gcow_last_error(void);
const char* gcow_version(void);

/* Upper bound on the flushed stream for `field` under `p` (the sw/ bound without the 148-bit header term). */
size_t gcow_max_output_bytes(const zfp_input* field, const gcow_params* p);
/* Device scratch needed by gcow_encode_device (variable-rate passes); 0 for fixed rate. */
size_t gcow_encode_workspace_bytes(const zfp_input* field, const gcow_params* p);
/* Number of uint64 entries of the block-offset index written with `index_stride` (0 = no index). */
size_t gcow_index_entries(const zfp_input* field, uint32_t index_stride);

/*
 * Encode field->data (DEVICE pointer, fp32 or bf16, 1-4 dims, any element strides) into d_out (device).
 * The stream is byte-identical to sw/'s zfp_compress on the same values (headerless, LSB-first 64-bit words,
 * flushed with zero bits to a 64-bit boundary). *d_total_bits (device uint64, may be NULL) receives the unflushed
 * bit count. d_index (device, may be NULL) receives the bit offset of every index_stride-th block (1..256, power of
 * two), which gcow_decode_device uses to decode variable-rate streams in parallel.
 * Asynchronous with respect to the host on hip_stream (NULL = default stream); no host synchronisation.
 */
gcow_status gcow_encode_device(const zfp_input* field, const gcow_params* p, void* d_out, size_t out_capacity,
                               uint64_t* d_total_bits, void* d_workspace, size_t workspace_bytes,
                               uint64_t* d_index, uint32_t index_stride, void* hip_stream);

/*
 * Chunked encode of one variable-rate stream: append field's blocks to a stream whose first *d_base_bits bits (a
 * DEVICE uint64) are already in d_out, as sw/'s stream_write_bits appends at the stream's current position
 * (sw/src/stream.c:61-92), without the stream_flush padding a separate zfp_compress call would insert
 * (sw/src/zfp.c:10-28). Encoding an array in chunks this way is byte-identical to one gcow_encode_device call on
 * the whole array; *d_total_bits = *d_base_bits + the chunk's bits, so it is the next chunk's base. d_out must hold
 * the previous bits plus gcow_max_output_bytes(field, p) (only the latter is checked against out_capacity). Block
 * index entries (d_index) are absolute stream offsets. Fixed-rate streams are chunked by offsetting d_out on the
 * host instead (GCOW_ERR_UNSUPPORTED here).
 * Every variable-rate field appends, 1-D to 4-D: the 4-D encoder's block scan starts at *d_base_bits like the range
 * scans of the others, and the chunk's first block ORs its first word into the bits before it. As with
 * gcow_encode_device, d_out past the previous bits, the workspace and the index need no zeroing: the chunk's flushed
 * words are written whole, apart from the bits of the word that *d_base_bits falls in, which are kept (the call
 * before left the rest of that word zero). A chunk without values is the field without extents (nx = ny = nz = nw =
 * 0; zfp_input cannot say "no rows of an N-D field"): it writes nothing but *d_total_bits = *d_base_bits.
 */
gcow_status gcow_encode_device_append(const zfp_input* field, const gcow_params* p, void* d_out, size_t out_capacity,
                                      const uint64_t* d_base_bits, uint64_t* d_total_bits, void* d_workspace,
                                      size_t workspace_bytes, uint64_t* d_index, uint32_t index_stride,
                                      void* hip_stream);

/*
 * Error feedback: gcow_encode_device of a 1-D bucket plus the carried compression error, which also writes the new
 * error. field->data: DEVICE, 1-D, contiguous, n values, fp32 or bf16. d_err_in: DEVICE fp32, n values, or NULL (all
 * zeros). d_err_out: DEVICE fp32, n values; d_err_in == d_err_out (in place) is allowed and gives the same result.
 *   1. y[i] = (float)x[i] + e_in[i]: one IEEE fp32 add, round to nearest, denormals kept.
 *   2. d_out receives the stream of the fp32 array y under p, byte-identical to gcow_encode_device of y (a bf16
 *      bucket is coded as the fp32 y, not as bf16). d_total_bits, d_index / index_stride as in gcow_encode_device.
 *   3. yhat = the libzfp 0.5.5 decode of that stream (what gcow_decode_device returns).
 *   4. r[i] = y[i] - yhat[i]: one IEEE fp32 subtract; e_out[i] = r[i] when r[i] is finite, else +0.0f, so that a NaN or
 *      Inf gradient (an AMP overflow step) or an overflowing x + e does not stay in the carried error.
 * The padding values of a partial last block give no residual: nothing is written past e_out[n - 1], nor past the
 * stream's flushed words. Over steps the sent values then average to the meant ones: sum_t yhat_t = sum_t x_t + e_0 - e_T.
 * Three paths give that result (gcow_encode_residual_path tells which one a call takes):
 *   GCOW_RESID_FUSED_FIXED  fixed rate with whole-word blocks (minbits == maxbits in {32, 64}, maxprec >= 32,
 *      minexp <= -154; rate 8 and 16), 16-byte aligned rows and no d_index: one kernel (each block coded, its word
 *      decoded in registers, both outputs stored: 14 bytes of HBM traffic per fp32 value at rate 16). No workspace.
 *   GCOW_RESID_FUSED_VAR    parameter sets whose budget truncates no block (minbits <= 1, maxbits >= 160: accuracy,
 *      precision, expert sets of that shape), field->data, d_err_in and d_err_out 16-byte aligned, with or without
 *      d_index at any legal stride: the variable-rate encoder's count, scan and code passes run on y formed in
 *      registers, and the code pass writes e_out from the coefficients it codes -- in this domain the decode of a
 *      block is those coefficients with the planes below kmin cleared, so no decoder runs, the stream is not read
 *      back and no index is needed. The workspace is gcow_encode_workspace_bytes of the fp32 field of n values.
 *   GCOW_RESID_COMPOSED     every other 1-D call (a budgeted variable-rate set, any other fixed rate, a lean call with
 *      d_index, buffers off 16-byte alignment): y into the workspace, the encoders on y, the decoder into d_err_out,
 *      r in place; a variable-rate stream is decoded through the caller's block index, or (d_index NULL) through one
 *      every 16 blocks kept in the workspace. The workspace covers y, the encoder's workspace and that index.
 * gcow_encode_residual_workspace_bytes is decided from p and, when field->data is set, its alignment (the error
 * buffers are taken as aligned; a call whose buffers turn out otherwise needs the composed path's size, which the
 * function returns for a field whose data pointer is set and off alignment). Capacity and workspace checks as
 * gcow_encode_device. Asynchronous on hip_stream; no host synchronisation, no allocation.
 * GCOW_ERR_UNSUPPORTED: dims != 1, a non-unit stride, a dtype other than float / bf16. GCOW_ERR_INVALID: NULL d_err_out.
 *
 * gcow_encode_residual_path: the path gcow_encode_residual_device takes for these arguments, or -1 for a call it
 * refuses. The pointers are inspected for alignment only and never dereferenced; NULL field->data or d_err_out means
 * "assume aligned" (d_err_in NULL is aligned: there is no input error). All three functions decide through the same
 * rule.
 */
enum { GCOW_RESID_COMPOSED = 0, GCOW_RESID_FUSED_FIXED = 1, GCOW_RESID_FUSED_VAR = 2 };
int gcow_encode_residual_path(const zfp_input* field, const gcow_params* p, const float* d_err_in,
                              const float* d_err_out, const uint64_t* d_index);
size_t gcow_encode_residual_workspace_bytes(const zfp_input* field, const gcow_params* p);
gcow_status gcow_encode_residual_device(const zfp_input* field, const gcow_params* p, const float* d_err_in,
                                        float* d_err_out, void* d_out, size_t out_capacity, uint64_t* d_total_bits,
                                        void* d_workspace, size_t workspace_bytes, uint64_t* d_index,
                                        uint32_t index_stride, void* hip_stream);

/*
 * Round trip without a stream: d_out[i] = decode(encode(field))[i], bit for bit what gcow_encode_device followed by
 * gcow_decode_device leaves in a field of out_dtype, in one pass that writes no stream, needs no workspace and no
 * block index -- the reference's training loop, which compresses the flattened gradients and decompresses them at
 * once to simulate the loss (hw/models/train_imagenet.py:448-475). *d_total_bits (optional, DEVICE uint64) = what
 * gcow_encode_device would report: the stream's bit length before stream_flush.
 * field->data: DEVICE, 1-D, contiguous (sx 0 or 1), n values, dtype_float or dtype_bf16. d_out: DEVICE, n values of
 * out_dtype, dtype_float or dtype_bf16 in any combination with the field's; a bf16 output is the fp32 decode rounded to
 * nearest even, as gcow_decode_device writes a bf16 field. Nothing is written past d_out[n - 1].
 * Aliasing: d_out == field->data is allowed when out_dtype == field->dtype (in place) and gives the same result. Any
 * other overlap of the two buffers is undefined.
 * Every 1-D parameter set gcow_encode_device accepts is supported, by one of three kernels:
 *   - fixed rate with whole-word blocks (minbits == maxbits in {32, 64}, maxprec >= 32, minexp <= -154; rate 8 and
 *     16), both buffers 16-byte aligned: each block coded and its word decoded in registers, one 16-byte (fp32) or
 *     8-byte (bf16) row read and one written per block;
 *   - no budget (minbits <= 1, maxbits >= 160: accuracy, precision and expert sets of that shape), both buffers
 *     16-byte aligned: the decoded coefficients are the coded ones with the planes below the block's precision
 *     cleared, so no embedded coder runs at all;
 *   - everything else, buffers off 16-byte alignment, and the partial last block of the two above: one lane per block
 *     through the generic block coder and decoder over registers.
 * Asynchronous on hip_stream: no allocation, no host synchronisation, *d_total_bits is never read on the host. n = 0
 * writes *d_total_bits = 0 and returns GCOW_OK.
 * GCOW_ERR_UNSUPPORTED: dims != 1, a non-unit stride, a field dtype or out_dtype other than float / bf16.
 * GCOW_ERR_INVALID: NULL field, p or d_out; field->data, d_out or d_total_bits misaligned for its element type;
 * check_params as in gcow_encode_device.
 */
gcow_status gcow_roundtrip_device(const zfp_input* field, const gcow_params* p, void* d_out, data_type out_dtype,
                                  uint64_t* d_total_bits, void* hip_stream);

/*
 * Round trip over a tensor list: the gradients where they lie, without the torch.cat before gcow_roundtrip_device and
 * the copy per parameter after it (the reference's collect_gradients / assign_gradients, hw/models/
 * train_imagenet.py:448-475). Let X = cat(t_0 ... t_{S-1}) be the 1-D field of N values. After the call out_s holds
 * roundtrip(X)[start_s : start_s + n_s], bit for bit what gcow_roundtrip_device writes for the contiguous X under the
 * same parameters and dtypes: blocks are X's blocks (a block may take its four values from up to four tensors), the
 * last block is padded as there, only real values are written and nothing outside [out_s, out_s + n_s) is.
 * All inputs share in_dtype and all outputs out_dtype (dtype_float or dtype_bf16, in any combination). out_s == in_s
 * is allowed when the dtypes are equal (in place: the normal use); any other overlap between any two buffers of the
 * call is undefined.
 *
 * The device call allocates nothing and never synchronises, so the address arithmetic is prepared on the host, once
 * per list, as a PLAN whose layout is private to the library:
 *   gcow_roundtrip_list_plan_bytes(nsegs, total_values): the size of a plan of nsegs tensors holding total_values
 *     values together (an upper bound: the plan drops empty tensors and gcow_roundtrip_list_plan reports what it used).
 *   gcow_roundtrip_list_plan: fills the caller's HOST buffer h_plan (8-byte aligned, plan_bytes long). in_ptrs /
 *     out_ptrs / counts: HOST arrays of nsegs DEVICE pointers and value counts; out_ptrs == NULL means in place (equal
 *     dtypes). *used_bytes (optional) = the bytes the caller copies to the device. The plan cuts X into chunks of 2048
 *     blocks (8192 values, the fused kernels' workgroup chunk) and records each as one of two kinds:
 *       direct: all its blocks are whole and lie inside one tensor, and its first row's input and output addresses are
 *               multiples of 4 bytes (GCOW_RTLIST_ROWS_DWORD: multi-dword buffer accesses are dword-aligned, so fp32
 *               rows always qualify and bf16 rows do at an even element offset; a tensor that starts at a flat offset
 *               that is no multiple of 4 still runs direct). One workgroup runs gcow_roundtrip_device's block
 *               sequence on it unchanged.
 *       gather: everything else -- a seam between tensors, rows off that alignment, the chunk holding the partial last
 *               block. Each value is located in the plan's tensor table and loaded on its own; blocks go through the
 *               same block functions, so the result is the same bits.
 *     The domain is picked once from the parameters as gcow_roundtrip_device picks it (whole-word fixed rate; no
 *     budget: minbits <= 1 and maxbits >= 160; else generic). In the generic domain every chunk is a gather chunk.
 *   gcow_roundtrip_list_plan_stats: what a plan holds (tests and the timing tool see which path runs).
 *   gcow_roundtrip_list_plan_chunk: TEST / MEASUREMENT ONLY: descriptor i of the direct (gather = 0: *a, *b = the
 *     first row's input and output address, *c = blocks) or gather (*a = first block, *b, *c = the indices, among the
 *     non-empty tensors, of those holding the chunk's first and last value) chunks.
 *   gcow_roundtrip_list_device: the launches. h_plan: the HOST plan (its header holds the launch geometry, which is
 *     why the call needs no synchronisation); d_plan: the caller's DEVICE copy of its first used_bytes bytes, 8-byte
 *     aligned, copied on hip_stream or complete before the call. p must be the plan's parameter set. *d_total_bits
 *     (optional, DEVICE uint64) = what gcow_encode_device(X) would report: nblocks * maxbits at fixed rate, else the
 *     sum of the block lengths. Asynchronous on hip_stream. N = 0 writes *d_total_bits = 0 and returns GCOW_OK. The
 *     plan is valid as long as the tensors stay where they are.
 * GCOW_ERR_UNSUPPORTED: a dtype other than float / bf16; 2^32 blocks or more in X. GCOW_ERR_INVALID: NULL p or
 * h_plan; a NULL or misaligned (for its element type) pointer with a non-zero count; out_ptrs NULL with unequal
 * dtypes; plan_bytes too small (plan: for the list; stats, device: for the plan); a device call whose p differs from
 * the plan's; misaligned d_plan or d_total_bits; check_params as in gcow_encode_device.
 */
enum { GCOW_RTLIST_ROWS_DWORD = 0, GCOW_RTLIST_ROWS_NATURAL = 1 };
typedef struct {
  uint64_t total_values;  /* N */
  uint64_t segments;      /* non-empty tensors */
  uint64_t direct_chunks;
  uint64_t gather_chunks;
  uint64_t used_bytes;    /* the plan's size */
  uint32_t domain;        /* 0 whole-word fixed rate, 1 no budget, 2 generic */
  uint32_t row_rule;      /* GCOW_RTLIST_ROWS_*: the alignment rule direct chunks were held to */
} gcow_roundtrip_list_stats;
size_t gcow_roundtrip_list_plan_bytes(size_t nsegs, uint64_t total_values);
gcow_status gcow_roundtrip_list_plan(const void* const* in_ptrs, void* const* out_ptrs, const uint64_t* counts,
                                     size_t nsegs, data_type in_dtype, data_type out_dtype, const gcow_params* p,
                                     void* h_plan, size_t plan_bytes, size_t* used_bytes);
gcow_status gcow_roundtrip_list_plan_stats(const void* h_plan, size_t plan_bytes, gcow_roundtrip_list_stats* stats);
gcow_status gcow_roundtrip_list_plan_chunk(const void* h_plan, size_t plan_bytes, int gather, uint64_t i, uint64_t* a,
                                           uint64_t* b, uint64_t* c);
gcow_status gcow_roundtrip_list_device(const void* h_plan, const void* d_plan, size_t plan_bytes,
                                       const gcow_params* p, uint64_t* d_total_bits, void* hip_stream);

/*
 * Round trip over a tensor list with a tolerance relative to each tensor. Every tensor t_s (n_s values) is a 1-D field
 * of its own, coded in accuracy mode under a tolerance that follows its largest magnitude, found on the device:
 *   a_s      = the largest |t_s[i]| over the finite values; +0 if there is none (empty, all zero, all NaN / Inf)
 *   emax_s   = (bits(a_s) >> 23) - 126, the codec's block-exponent convention (a subnormal or zero maximum: -126)
 *   minexp_s = max(emax_s - rel_bits, -94); for emax_s = 128 only, min(that, floor(log2(2^128 - a_s)) - 2)
 *   p_s      = expert(minbits 1, maxbits 16658, maxprec, minexp_s)
 *   out_s    = exactly what gcow_roundtrip_device(field(t_s), p_s, out_s, out_dtype, ...) writes: blocks are the
 *              tensor's own, counted from its first value, its last block padded as a partial block; only real values
 *              are written and nothing outside [out_s, out_s + n_s)
 *   d_absmax[s] = a_s as fp32 for every s of the caller's numbering (empty tensors: 0)
 *   *d_total_bits = the sum over s of the bit length gcow_encode_device(t_s, p_s) would report
 * Bound: |out - t| <= 2^minexp_s, below 2^(1 - rel_bits) max|t_s| where the floor is inactive, and every finite block
 * decodes to finite values. 0 <= rel_bits <= 24 (the bound fails once the 32-plane cap binds). Neither clamp is
 * cosmetic. The floor of -94: blocks with emax <= -98 cast every value to INT_MIN (the reference's x86 cast), and without
 * it a tensor of scale 1e-40 would decode to garbage of twice its magnitude; with it every such block has precision 0 and
 * decodes to +0. The cap for a maximum in the top binade: a value decodes to within 2^minexp_s of itself, so without
 * it a tensor of scale 3e38 at rel_bits 0 (4 planes, minexp_s = 128) decodes finite values of 2.4e38 and more to Inf.
 * With g = 2^128 - a_s >= 2^104, minexp_s <= floor(log2 g) - 2 keeps |out| <= 2^128 - 3 g / 4, below the point where
 * fp32 rounds to Inf. It costs a few more planes for such tensors only (at most rel_bits 26 in effect).
 * All inputs share in_dtype and all outputs out_dtype (dtype_float or dtype_bf16, in any combination; bf16 input is
 * widened exactly). out_s == in_s is allowed when the dtypes are equal; any other overlap is undefined.
 *
 * As for the list form the address arithmetic is a host PLAN of private layout; it depends on neither rel_bits nor
 * maxprec, which are arguments of the device call only:
 *   gcow_roundtrip_rel_plan_bytes(nsegs, total_values): an upper bound of the plan's size.
 *   gcow_roundtrip_rel_plan: fills the caller's HOST buffer h_plan (8-byte aligned). Arguments as
 *     gcow_roundtrip_list_plan's. A tensor's whole blocks run DIRECT, in chunks of up to 2048 blocks (one workgroup,
 *     gcow_roundtrip_device's block sequence), when it has at least 256 of them and its input and output lie at
 *     4-byte aligned addresses. Every other block is a GATHER block: the partial last block of any tensor, tensors
 *     of fewer than 256 whole blocks, bf16 tensors at an odd element offset. Gather blocks are numbered through the
 *     tensors in list order and cut into chunks of 256, one block per lane; a lane finds its block's tensor by
 *     bisection and loads its values one by one. No block crosses a tensor.
 *   gcow_roundtrip_rel_plan_stats: what a plan holds.
 *   gcow_roundtrip_rel_plan_chunk: TEST / MEASUREMENT ONLY: gather = 0: direct chunk i covers blocks *block0 ..
 *     *block0 + *nblocks - 1 of tensor *tensor (the caller's numbering); gather != 0: gather piece i (one per tensor
 *     that has gather blocks, i < the number of such tensors; GCOW_ERR_INVALID past it) likewise.
 *   gcow_roundtrip_rel_device: the launches -- d_absmax zeroed in stream order, one pass that takes every tensor's
 *     maximum (|x| as integer bits, non-finite values masked to 0, one atomic per workgroup and tensor), then the
 *     round trip kernels, which read minexp_s's source from d_absmax. d_absmax: DEVICE float[nsegs], required when
 *     nsegs > 0, 4-byte aligned; it doubles as the workspace. d_total_bits: optional DEVICE uint64. h_plan / d_plan /
 *     plan_bytes as gcow_roundtrip_list_device's. Asynchronous on hip_stream: no allocation, no host synchronisation.
 *     An empty list returns GCOW_OK and writes *d_total_bits = 0.
 * GCOW_ERR_UNSUPPORTED: a dtype other than float / bf16; 2^32 blocks or more. GCOW_ERR_INVALID: NULL h_plan; a NULL or
 * misaligned (for its element type) pointer with a non-zero count; out_ptrs NULL with unequal dtypes; plan_bytes too
 * small; rel_bits > 24; maxprec as check_params has it; NULL d_absmax with nsegs > 0; misaligned d_absmax, d_plan or
 * d_total_bits.
 */
typedef struct {
  uint64_t total_values;
  uint64_t total_blocks;  /* the sum of ceil(n_s / 4) */
  uint64_t segments;      /* non-empty tensors */
  uint64_t direct_chunks;
  uint64_t gather_chunks;
  uint64_t used_bytes;    /* the plan's size */
} gcow_roundtrip_rel_stats;
size_t gcow_roundtrip_rel_plan_bytes(size_t nsegs, uint64_t total_values);
gcow_status gcow_roundtrip_rel_plan(const void* const* in_ptrs, void* const* out_ptrs, const uint64_t* counts,
                                    size_t nsegs, data_type in_dtype, data_type out_dtype, void* h_plan,
                                    size_t plan_bytes, size_t* used_bytes);
gcow_status gcow_roundtrip_rel_plan_stats(const void* h_plan, size_t plan_bytes, gcow_roundtrip_rel_stats* stats);
gcow_status gcow_roundtrip_rel_plan_chunk(const void* h_plan, size_t plan_bytes, int gather, uint64_t i,
                                          uint64_t* tensor, uint64_t* block0, uint64_t* nblocks);
gcow_status gcow_roundtrip_rel_device(const void* h_plan, const void* d_plan, size_t plan_bytes, uint32_t rel_bits,
                                      uint32_t maxprec, float* d_absmax, uint64_t* d_total_bits, void* hip_stream);

/*
 * Rate table: accuracy mode under a bit budget. For a contiguous 1-D field (DEVICE, dtype_float or dtype_bf16, any
 * element-aligned address) one pass over the input writes d_table[t], t = 0 .. GCOW_RATE_TABLE_ENTRIES - 1 (DEVICE
 * uint64), for minexp = GCOW_RATE_TABLE_MINEXP_LO + t:
 *   d_table[t] = the unflushed bit count of the stream gcow_encode_device writes for the field under
 *                {minbits 1, maxbits 16658, maxprec, minexp} -- exactly the value that call stores in *d_total_bits.
 * The range is complete: below minexp -154 every block already has its full precision, so every smaller minexp gives
 * d_table[0]; from 132 on every block is a single bit, so d_table[286] = d_table[287] = the number of blocks and every
 * larger minexp gives the same. The table is non-increasing in t (a plane more of precision never shortens a block).
 * It is exact, not an estimate: integer sums only, the same bits run to run.
 *
 * d_workspace: gcow_rate_table_workspace_bytes(field) bytes, 8-byte aligned. Neither the table nor the workspace needs
 * zeroing by the caller; the table is written whole and nothing past it. No host synchronisation, no allocation; legal
 * inside a stream capture. nx = 0 gives an all-zero table.
 * GCOW_ERR_INVALID: a field that is not 1-D or has a non-unit stride, a NULL or misaligned pointer, a workspace below
 * the query. GCOW_ERR_UNSUPPORTED: a dtype other than float / bf16; 2^32 blocks or more.
 *
 * gcow_rate_table_fit (HOST; h_table: a host copy of the 288 entries): the smallest minexp in [-154, 133] whose entry
 * is <= budget_bits -- the finest tolerance whose stream fits -- and that entry. GCOW_ERR_INVALID when budget_bits <
 * h_table[287]: no accuracy-mode stream is shorter than one bit per block (*minexp and *bits are left alone).
 *
 * gcow_rate_table_residual_device: the table of y, y[i] = (float)x[i] + e_in[i] -- the array error feedback encodes.
 * The add is the single __fadd_rn of gcow_encode_residual_device step 1 (a bf16 x widened exactly); the pass forms y in
 * registers and never writes it to memory. d_table[t] is exactly the *d_total_bits gcow_encode_residual_device reports
 * for the same field and d_err_in under {1, 16658, maxprec, -154 + t}. d_err_in (DEVICE, n floats): any 4-byte aligned
 * address; NULL means zeros, and the table is gcow_rate_table_device's. Wide loads run when field->data and d_err_in
 * are both 16-byte aligned, else the element path; the partial last block is padded from y, as the encoder pads it.
 * Workspace, table, stream behaviour and errors as gcow_rate_table_device (the workspace query is unchanged), plus
 * GCOW_ERR_INVALID for a d_err_in off 4 bytes.
 */
#define GCOW_RATE_TABLE_MINEXP_LO (-154)
#define GCOW_RATE_TABLE_ENTRIES 288
size_t gcow_rate_table_workspace_bytes(const zfp_input* field);
gcow_status gcow_rate_table_device(const zfp_input* field, uint32_t maxprec, uint64_t* d_table, void* d_workspace,
                                   size_t workspace_bytes, void* hip_stream);
gcow_status gcow_rate_table_residual_device(const zfp_input* field, const float* d_err_in, uint32_t maxprec,
                                            uint64_t* d_table, void* d_workspace, size_t workspace_bytes,
                                            void* hip_stream);
gcow_status gcow_rate_table_fit(const uint64_t* h_table, uint64_t budget_bits, int* minexp, uint64_t* bits);

/*
 * The fit on the device, and encode / round trip under a minexp that lives in device memory: table, fit and encode (or
 * round trip) are launched back to back on one stream with no host read in between, and can be captured into one graph
 * that follows the data it is replayed on.
 *
 * gcow_rate_table_fit_device: d_table holds 288 DEVICE entries as gcow_rate_table_device writes them, or a sum of
 * several fields' tables (the ranks of an exchange: the length of all their streams under each minexp). One workgroup
 * writes *d_fit (DEVICE, 8-byte aligned) = what gcow_rate_table_fit returns on a host copy of the table: the smallest
 * minexp in [-154, 133] whose entry is <= budget_bits, that entry in bits, status = 0. Where the host call fails
 * (budget_bits below entry 287) the device call cannot: it writes minexp = 133, bits = d_table[287], status = 1 -- the
 * coarsest set, for the caller to accept or refuse when it next reads the record. The 16 bytes of the record are
 * written with ordinary stores and nothing past them. No allocation, no synchronisation; legal inside a stream
 * capture. GCOW_ERR_INVALID: a NULL or misaligned (8 bytes) d_table or d_fit.
 *
 * gcow_encode_fitted_device: field is 1-D, contiguous, dtype_float or dtype_bf16, at any element-aligned address.
 * With m = clamp(*d_minexp, -154, 133), the word read ON THE DEVICE when the kernels run, every output is byte for
 * byte what gcow_encode_device(field, {1, 16658, maxprec, m}, ...) writes with the same arguments: the stream,
 * *d_total_bits, the index at index_stride, the zeroed flush word, and nothing else. The clamp loses nothing: the rate
 * table's range is complete (above), below -154 and from 132 on the stream no longer changes; it keeps emax - minexp
 * inside int for any input word. d_minexp: any 4-byte aligned DEVICE word, unchanged by the call; the first word of a
 * gcow_fit is the intended source. out_capacity and the workspace are gcow_max_output_bytes / gcow_encode_workspace_bytes
 * of {1, 16658, maxprec, any minexp}: NEITHER DEPENDS ON minexp, so both can be sized before the fit exists. Always the
 * tile form of the 1-D variable-rate encoder: gcow_debug_set_var1d_variant does not apply. nx = 0 writes
 * *d_total_bits = 0. GCOW_ERR_UNSUPPORTED: dims != 1, a non-unit stride, a dtype other than float / bf16.
 * GCOW_ERR_INVALID: NULL field or d_out, a NULL or misaligned d_minexp, field->data misaligned for its element type,
 * d_out / d_total_bits / d_index / d_workspace off 8 bytes, a bad index_stride, a workspace below the query.
 * GCOW_ERR_CAPACITY: out_capacity below the bound.
 *
 * gcow_roundtrip_fitted_device: the same relation to gcow_roundtrip_device under {1, 16658, maxprec, m}: d_out and
 * *d_total_bits bit for bit. dtype_float / dtype_bf16 in and out in any combination; d_out == field->data is allowed
 * when the dtypes are equal. Buffers off 16-byte alignment and the partial last block go through the generic kernel
 * under the same device word. Errors as gcow_roundtrip_device's, and GCOW_ERR_INVALID for a NULL or misaligned d_minexp.
 *
 * gcow_encode_residual_fitted_device: error feedback under the device word. With m as above, every output is byte for
 * byte what gcow_encode_residual_device(field, {1, 16658, maxprec, m}, d_err_in, d_err_out, ...) writes on its
 * GCOW_RESID_FUSED_VAR path: the stream, *d_total_bits, the index, the zeroed flush word and e_out; nothing is written
 * past e_out[n - 1]. d_err_in == d_err_out is allowed, d_err_in == NULL means zeros. Always the tile form with the
 * residual; there is no composed fallback, because its decoder takes host parameters: field->data, d_err_in or
 * d_err_out off 16-byte alignment returns GCOW_ERR_UNSUPPORTED and writes nothing. The workspace is
 * gcow_encode_workspace_bytes and out_capacity gcow_max_output_bytes of the fp32 field of n values under
 * {1, 16658, maxprec, any minexp}: NEITHER DEPENDS ON minexp, so both can be sized before the fit exists. With
 * gcow_rate_table_residual_device and gcow_rate_table_fit_device ahead of it on the stream, table of y, fit and encode
 * run with no host read and the stream is within the budget for y, the array that is sent. nx = 0 writes
 * *d_total_bits = 0. Other errors as gcow_encode_fitted_device's, and GCOW_ERR_INVALID for a NULL d_err_out.
 *
 * Decoders are untouched: a stream is decoded under host parameters. A caller that needs minexp on the host reads the
 * 16-byte record when it next has to wait anyway.
 */
typedef struct {
  int32_t minexp;   /* the fitted minexp, GCOW_RATE_TABLE_MINEXP_LO .. + GCOW_RATE_TABLE_ENTRIES - 1 */
  uint32_t status;  /* 0: bits <= budget_bits; 1: no entry fits, the coarsest set was taken */
  uint64_t bits;    /* the table entry at minexp */
} gcow_fit;         /* 16 bytes, 8-byte aligned */
gcow_status gcow_rate_table_fit_device(const uint64_t* d_table, uint64_t budget_bits, gcow_fit* d_fit, void* hip_stream);
gcow_status gcow_encode_fitted_device(const zfp_input* field, uint32_t maxprec, const int32_t* d_minexp, void* d_out,
                                      size_t out_capacity, uint64_t* d_total_bits, void* d_workspace,
                                      size_t workspace_bytes, uint64_t* d_index, uint32_t index_stride,
                                      void* hip_stream);
gcow_status gcow_encode_residual_fitted_device(const zfp_input* field, uint32_t maxprec, const int32_t* d_minexp,
                                               const float* d_err_in, float* d_err_out, void* d_out,
                                               size_t out_capacity, uint64_t* d_total_bits, void* d_workspace,
                                               size_t workspace_bytes, uint64_t* d_index, uint32_t index_stride,
                                               void* hip_stream);
gcow_status gcow_roundtrip_fitted_device(const zfp_input* field, uint32_t maxprec, const int32_t* d_minexp, void* d_out,
                                         data_type out_dtype, uint64_t* d_total_bits, void* hip_stream);

/*
 * Accuracy mode under a bit budget over a tensor list: the rate table and the fitted round trip of the concatenation
 * X = cat(t_0 ... t_{S-1}) (N values, as in gcow_roundtrip_list_device's contract), every tensor read and written
 * where it lies. Table, gcow_rate_table_fit_device and round trip go on one stream with no host read, and can be
 * captured into one graph. The budget is one for the whole list (one table for the concatenation); a budget per tensor
 * is the block after this one (gcow_rate_table_rel_device).
 *
 * The plan. Both calls take a plan of gcow_roundtrip_list_plan as it is (h_plan, d_plan, plan_bytes as
 * gcow_roundtrip_list_device's), made for any set WITHOUT A BLOCK BUDGET: minbits <= 1 and maxbits >= 160
 * (gcow_roundtrip_list_stats.domain == 1), e.g. {1, 16658, maxprec, 0}. The plan's own maxprec and minexp are not
 * read: maxprec is an argument here and minexp is the table's index or the device word. A plan of another domain
 * returns GCOW_ERR_INVALID. (gcow_roundtrip_list_device still wants exactly the plan's parameter set.)
 *
 * gcow_rate_table_list_workspace_bytes: the workspace of the table call for that plan (0 for a NULL, short or foreign
 *   plan; else positive, and the same for every list).
 * gcow_rate_table_list_device: d_table[t], t = 0 .. 287 (DEVICE uint64), is exactly what gcow_rate_table_device writes
 *   for the contiguous X of the plan's input dtype, i.e. the *d_total_bits of gcow_roundtrip_list_device under
 *   {1, 16658, maxprec, -154 + t}. Only the plan's input pointers are read. The table is written whole and nothing
 *   past it; neither the table nor the workspace (8-byte aligned) needs zeroing by the caller, and the workspace is
 *   zeroed by a kernel in stream order, not by a memset node. No allocation and no synchronisation; legal inside a
 *   stream capture. N = 0 gives an all-zero table. Integer sums only: the same bits run to run.
 * gcow_roundtrip_list_fitted_device: with m = clamp(*d_minexp, -154, 133), the word read ON THE DEVICE when the kernels
 *   run, every out_s and *d_total_bits (DEVICE uint64, required) are bit for bit what gcow_roundtrip_list_device writes
 *   under {1, 16658, maxprec, m} -- hence what gcow_roundtrip_fitted_device writes for the contiguous X. Dtypes and
 *   outputs are the plan's; in place (out_s == in_s) is allowed for equal dtypes, as in the list call. N = 0 writes
 *   *d_total_bits = 0. d_minexp: any 4-byte aligned DEVICE word, unchanged by the call; the first word of a gcow_fit
 *   is the intended source. Asynchronous on hip_stream, no allocation, no synchronisation.
 * GCOW_ERR_INVALID, all decided on the host before any launch: a NULL, short (plan_bytes) or foreign h_plan; a plan of
 * another domain; a NULL or misaligned (8 bytes) d_plan, d_table, d_workspace or d_total_bits; a NULL or misaligned
 * (4 bytes) d_minexp; a workspace below the query; maxprec as check_params has it for {1, 16658, maxprec, 0}.
 */
size_t gcow_rate_table_list_workspace_bytes(const void* h_plan, size_t plan_bytes);
gcow_status gcow_rate_table_list_device(const void* h_plan, const void* d_plan, size_t plan_bytes, uint32_t maxprec,
                                        uint64_t* d_table, void* d_workspace, size_t workspace_bytes, void* hip_stream);
gcow_status gcow_roundtrip_list_fitted_device(const void* h_plan, const void* d_plan, size_t plan_bytes,
                                              uint32_t maxprec, const int32_t* d_minexp, uint64_t* d_total_bits,
                                              void* hip_stream);

/*
 * Accuracy mode under a bit budget PER TENSOR of a list: every tensor is a field of its own, as in
 * gcow_roundtrip_rel_device, with its own rate table, its own budget and its own fitted minexp, so that the loud
 * tensors of a gradient list neither decide the quiet ones' tolerance nor take their bits. Tables, fits and round trip
 * go on one stream with no host read in between, allocate nothing and can be captured into one graph that follows the
 * data it is replayed on. 1-D, dtype_float / dtype_bf16.
 *
 * The plan. All three plan calls take a plan of gcow_roundtrip_rel_plan as it is (h_plan, d_plan, plan_bytes as
 * gcow_roundtrip_rel_device's; S = nsegs tensors in the caller's numbering, empty ones included).
 *
 * gcow_rate_table_rel_workspace_bytes: the workspace of the table call: 0 for a NULL, short or foreign plan, else
 *   positive and a function of S only.
 * gcow_rate_table_rel_device: d_tables is DEVICE uint64[S][288]. Row s is exactly what gcow_rate_table_device writes for
 *   tensor s as a field of its own -- its blocks counted from its first value, its partial last block padded as the
 *   encoder pads it -- i.e. row s, entry t is the *d_total_bits of gcow_roundtrip_device(t_s, {1, 16658, maxprec,
 *   -154 + t}). An empty tensor gives an all-zero row. Only the plan's input pointers are read. The tables are written
 *   whole and nothing past them; neither they nor the workspace (8-byte aligned) need zeroing by the caller, and the
 *   workspace is zeroed by a kernel in stream order, not by a memset node. Integer sums only: the same bits run to run.
 * gcow_rate_table_fit_batch_device: one workgroup per table. d_tables: DEVICE uint64[ntables][288]; d_budgets: DEVICE
 *   uint64[ntables]; d_fits: DEVICE gcow_fit[ntables]. Record s = the smallest minexp in [max(minexp_floor, -154), 133]
 *   whose entry of table s is <= d_budgets[s], that entry, status 0; where no such entry fits, {133, 1, table_s[287]}.
 *   With minexp_floor = -154 and ntables = 1 it is gcow_rate_table_fit_device with the budget in device memory. The
 *   floor exists for the reason gcow_roundtrip_rel_device has one (above: "neither clamp is cosmetic"): at
 *   minexp >= -94 every block whose values all cast to INT_MIN (emax <= -98) has precision 0 and decodes to +0, not to
 *   garbage of twice its magnitude; a generous budget would otherwise fit a tensor of scale 1e-40 below that. The
 *   relative form's cap for a maximum in the top binade is NOT reproduced: a fit knows bits, not the maximum. A tensor
 *   of scale 3e38 behaves as gcow_roundtrip_fitted_device behaves on it: under a coarse fitted minexp finite values
 *   near the maximum may decode to Inf. ntables = 0 does nothing.
 * gcow_roundtrip_rel_fitted_device: tensor s is coded under m_s = clamp(d_minexp[s * minexp_stride_words], -154, 133),
 *   the words (DEVICE int32, 4-byte aligned, unchanged by the call) read ON THE DEVICE when the kernels run: a stride
 *   of 4 words walks an array of gcow_fit, a stride of 1 packed words. out_s is bit for bit what
 *   gcow_roundtrip_fitted_device(t_s, maxprec, &word_s, ...) writes, and *d_total_bits (optional DEVICE uint64) the sum
 *   over s of its bit counts. Dtypes, in place, and "only real values are written, nothing outside
 *   [out_s, out_s + n_s)" as gcow_roundtrip_rel_device. An empty list returns GCOW_OK and writes *d_total_bits = 0.
 * GCOW_ERR_INVALID, all decided on the host before any launch: a NULL, short (plan_bytes) or foreign h_plan; with
 * S > 0 (ntables > 0) a NULL or misaligned (8 bytes) d_plan, d_tables, d_workspace, d_budgets or d_fits, or a NULL or
 * misaligned (4 bytes) d_minexp; a misaligned d_total_bits; a workspace below the query; a stride of 0; maxprec as
 * check_params has it for {1, 16658, maxprec, 0}.
 */
size_t gcow_rate_table_rel_workspace_bytes(const void* h_plan, size_t plan_bytes);
gcow_status gcow_rate_table_rel_device(const void* h_plan, const void* d_plan, size_t plan_bytes, uint32_t maxprec,
                                       uint64_t* d_tables, void* d_workspace, size_t workspace_bytes, void* hip_stream);
gcow_status gcow_rate_table_fit_batch_device(const uint64_t* d_tables, size_t ntables, const uint64_t* d_budgets,
                                             int32_t minexp_floor, gcow_fit* d_fits, void* hip_stream);
gcow_status gcow_roundtrip_rel_fitted_device(const void* h_plan, const void* d_plan, size_t plan_bytes,
                                             uint32_t maxprec, const int32_t* d_minexp, uint32_t minexp_stride_words,
                                             uint64_t* d_total_bits, void* hip_stream);

/*
 * Segmented fields: a minexp per tensor ON THE WIRE. The calls above choose a tolerance per tensor but leave no
 * stream; these code one contiguous buffer that holds S tensors back to back into ONE stream, every tensor under its
 * own minexp, and decode-and-average W such streams, each in a number of launches that does not depend on S.
 *
 * A segmented field is
 *   - a contiguous 1-D DEVICE array of n values, dtype_float or dtype_bf16, at any element-aligned address;
 *   - a host list counts[S] with sum n (zeros allowed);
 *   - a DEVICE int32 array of minexp words, one per tensor in the caller's numbering, read at
 *     d_minexp[s * minexp_stride] ON THE DEVICE when the kernels run: a stride of 1 for packed words, 4 for an array
 *     of gcow_fit records (minexp is word 0 of a record).
 * Tensor s is the slice [off_s, off_s + n_s), off_s = sum_{r<s} n_r, and is a field of its own: its blocks are counted
 * from its first value, its last block is padded as a partial block, no block crosses a tensor. It is coded under
 * p_s = expert(1, 16658, maxprec, clamp(minexp_s, -154, 133)), the clamp of the fitted calls. Virtual block v counts
 * the blocks of all tensors in list order: vb0_s = sum_{r<s} ceil(n_r / 4). Empty tensors contribute none and their
 * word is never read.
 *
 * The stream is exactly what results from: start at bit 0; gcow_encode_device_append(field(t_s), p_s) for s = 0 ..
 * S - 1 in order; flush once to a 64-bit boundary at the end. The tensors' streams are concatenated at bit
 * granularity, no padding between them. *d_total_bits (optional) is the sum of the tensors' bit counts. With
 * index_stride (a power of two in [1, 256]; d_index NULL: no index) d_index[j] is the bit position of virtual block
 * j * index_stride, gcow_encode_seg_index_entries of them. Output, workspace and index need no zeroing by the caller;
 * nothing is written past the flushed words; an empty list writes *d_total_bits = 0 and nothing else.
 *
 * The plan (host; gcow_seg_plan_bytes bounds its size, used_bytes is what to copy to the device): a private layout that
 * holds no pointers and depends on neither maxprec nor the words, so one plan serves every buffer of that shape, the
 * encode and the decode. It carries vb0_s and off_s of the non-empty tensors and, per tile of 1024 virtual blocks, the
 * tensor of the tile's first block and whether every block of the tile is a whole block of that one tensor (a
 * "uniform" tile): a lane bisects over the tensors of its own tile only. gcow_seg_plan_stats reports the counts;
 * gcow_seg_plan_segment gives vb0_s / off_s / n_s of tensor s (an empty tensor: those of the next non-empty one, n 0),
 * gcow_seg_plan_tile the tensor (caller's numbering) of tile t's first block and the uniform flag.
 * gcow_encode_seg_max_output_bytes / _workspace_bytes / _index_entries: the sizes for a plan (0 for a NULL or foreign
 * one, index_stride 0: 0 entries).
 *
 * gcow_decode_mean_seg_device: for W = nstreams streams of one segmented shape (stream r at d_streams + r *
 * stream_words, its index -- relative to its own first word -- at d_index + r * index_words, index_stride 8 or 16),
 * tensor s of d_out receives exactly what gcow_decode_mean_device writes for a 1-D field of n_s values under p_{r,s},
 * from the W sub-streams at their bit positions: ((0 + x_0) + x_1 + ...) / W in fp32 in rank order; out_dtype
 * dtype_bf16 rounds to nearest even in the store. Stream r reads its words at d_minexp[r * minexp_stream_stride +
 * s * minexp_stride]; minexp_stream_stride = 0: one set for all streams. W = 1 is the plain decode. The decoders'
 * contract holds (below): every slot may hold anything from its stream's last bit on, the two words after the last
 * slot likewise (streams_bytes covers them), stream_words may be odd. Only real values are written, nothing outside
 * [d_out, d_out + n). An empty list does nothing.
 *
 * Refusals, all on the host before any launch. GCOW_ERR_UNSUPPORTED: 2^32 virtual blocks or more, 2^31 tensors or
 * more, a dtype other than dtype_float / dtype_bf16. GCOW_ERR_INVALID: a NULL h_plan or counts with nsegs > 0, a
 * plan buffer below gcow_seg_plan_bytes or misaligned (8 bytes); a NULL, short or foreign plan; with a non-empty list a
 * NULL or misaligned d_plan (8), d_in / d_out (element), d_minexp (4), d_out stream (8), workspace (8) below its query,
 * a misaligned d_total_bits / d_index, a minexp_stride of 0, an index_stride that is no power of two in [1, 256]
 * (decode: not 8 or 16, or a NULL index, or index_words below the entries), no streams, streams_bytes below
 * nstreams * stream_words + 2 words; maxprec as check_params has it. GCOW_ERR_CAPACITY: out_capacity below the query.
 */
typedef struct {
  uint64_t total_values;
  uint64_t virtual_blocks;
  uint64_t segments;       /* non-empty tensors */
  uint64_t tiles;          /* of 1024 virtual blocks */
  uint64_t uniform_tiles;
  uint64_t used_bytes;
} gcow_seg_stats;
size_t gcow_seg_plan_bytes(size_t nsegs, uint64_t total_values);
gcow_status gcow_seg_plan(const uint64_t* counts, size_t nsegs, data_type dtype, void* h_plan, size_t plan_bytes,
                          size_t* used_bytes);
gcow_status gcow_seg_plan_stats(const void* h_plan, size_t plan_bytes, gcow_seg_stats* stats);
gcow_status gcow_seg_plan_segment(const void* h_plan, size_t plan_bytes, uint64_t s, uint64_t* vb0, uint64_t* off,
                                  uint64_t* n);
gcow_status gcow_seg_plan_tile(const void* h_plan, size_t plan_bytes, uint64_t t, uint64_t* tensor, int* uniform);
size_t gcow_encode_seg_max_output_bytes(const void* h_plan, size_t plan_bytes);
size_t gcow_encode_seg_workspace_bytes(const void* h_plan, size_t plan_bytes);
size_t gcow_encode_seg_index_entries(const void* h_plan, size_t plan_bytes, uint32_t index_stride);
gcow_status gcow_encode_seg_device(const void* h_plan, const void* d_plan, size_t plan_bytes, const void* d_in,
                                   uint32_t maxprec, const int32_t* d_minexp, uint32_t minexp_stride, void* d_out,
                                   size_t out_capacity, uint64_t* d_total_bits, void* d_workspace,
                                   size_t workspace_bytes, uint64_t* d_index, uint32_t index_stride, void* hip_stream);
gcow_status gcow_decode_mean_seg_device(const void* h_plan, const void* d_plan, size_t plan_bytes, uint32_t maxprec,
                                        const int32_t* d_minexp, uint32_t minexp_stride, uint64_t minexp_stream_stride,
                                        const uint64_t* d_streams, size_t streams_bytes, uint64_t stream_words,
                                        uint32_t nstreams, const uint64_t* d_index, uint64_t index_words,
                                        uint32_t index_stride, void* d_out, data_type out_dtype, void* hip_stream);

/*
 * Segmented fields with a residual: error feedback under a minexp per tensor. Both calls take a segmented field as
 * defined above (plan, buffer, counts, words) and an error array parallel to the buffer:
 *   - d_err_in: DEVICE fp32, n values, or NULL for zeros; 4-byte aligned, no more;
 *   - d_err_out: DEVICE fp32, n values, 4-byte aligned; d_err_in == d_err_out is allowed (in place).
 * e_s is the slice [off_s, off_s + n_s) of the error array, and y = (float)x + e one __fadd_rn per value (a bf16 x
 * widened exactly), formed in registers and never stored. The plan is gcow_seg_plan's as it is: it holds no pointers, so
 * one plan serves the tables, the encode and the decode.
 *
 * gcow_rate_table_seg_workspace_bytes: the workspace of the table call: 0 for a NULL, short or foreign plan, else
 *   positive and a function of S only.
 * gcow_rate_table_seg_device: d_tables is DEVICE uint64[S][288], rows in the caller's numbering. Row s is exactly what
 *   gcow_rate_table_residual_device writes for tensor s as a field of its own with e_s: the table of y_s, its partial
 *   last block padded from y as the encoder pads it, Inf / NaN blocks of y (an overflowing x + e included) under the
 *   generic rule. An empty tensor gives an all-zero row. With d_err_in == NULL row s equals row s of
 *   gcow_rate_table_rel_device for the same tensors. The tables are written whole and nothing past them; neither they
 *   nor the workspace (8-byte aligned) need zeroing by the caller, and the workspace is zeroed by a kernel in stream
 *   order. Integer sums only: the same bits run to run. No host read, no allocation; legal inside a stream capture.
 * gcow_encode_seg_residual_device: stream, *d_total_bits and index are byte for byte what gcow_encode_seg_device writes
 *   for the fp32 array y under the same words and a plan of the same counts. d_err_out over tensor s is what
 *   gcow_encode_residual_device(t_s, {1, 16658, maxprec, clamp(word_s, -154, 133)}, e_s, ...) writes: e' = y - decode(y)
 *   by one __fsub_rn, a non-finite result replaced by +0.0f. Only real values are written: a tensor's partial last
 *   block does not reach the next tensor's first values, and nothing is written outside [d_err_out, d_err_out + n).
 *   d_in is never written. Rows may start at any element-aligned address: whether a row moves as one vector is decided
 *   at run time, per array, from its own address, so d_in, d_err_in and d_err_out may have three different alignments.
 *   Capacity, workspace and index entries are the plan's queries (gcow_encode_seg_max_output_bytes, _workspace_bytes,
 *   _index_entries); they depend on the counts only, not on the plan's dtype and not on the words. An empty list
 *   writes *d_total_bits = 0 and nothing else. The launch count does not depend on S. No host read, no allocation;
 *   legal inside a stream capture.
 * Refusals, on the host before any launch: those of gcow_encode_seg_device, and GCOW_ERR_INVALID for a NULL d_err_out
 * (non-empty list), an error pointer off 4 bytes, a NULL or misaligned (8 bytes) d_tables (S > 0), a workspace below its
 * query.
 */
size_t gcow_rate_table_seg_workspace_bytes(const void* h_plan, size_t plan_bytes);
gcow_status gcow_rate_table_seg_device(const void* h_plan, const void* d_plan, size_t plan_bytes, const void* d_in,
                                       const float* d_err_in, uint32_t maxprec, uint64_t* d_tables, void* d_workspace,
                                       size_t workspace_bytes, void* hip_stream);
gcow_status gcow_encode_seg_residual_device(const void* h_plan, const void* d_plan, size_t plan_bytes, const void* d_in,
                                            const float* d_err_in, float* d_err_out, uint32_t maxprec,
                                            const int32_t* d_minexp, uint32_t minexp_stride, void* d_out,
                                            size_t out_capacity, uint64_t* d_total_bits, void* d_workspace,
                                            size_t workspace_bytes, uint64_t* d_index, uint32_t index_stride,
                                            void* hip_stream);

/*
 * Relative tolerance over a segmented field: the per-tensor minexp words of gcow_roundtrip_rel_device's rule from one
 * pass over the buffer, written where the segmented calls above read them. The field is a segmented field as defined
 * above (gcow_seg_plan's plan, unchanged; d_in fp32 or bf16 at any element-aligned address) and d_err_in the error array
 * of the residual calls: DEVICE fp32 parallel to the buffer, 4-byte aligned, or NULL for zeros.
 *
 * gcow_seg_rel_minexp_device: for every tensor s of the caller's numbering,
 *   - y = (float)x + e, one __fadd_rn per value, formed in registers as gcow_encode_seg_residual_device forms it and never
 *     stored (a bf16 x widened exactly; without e this is x + 0);
 *   - d_absmax[s] = a_s, the largest finite |y| over the tensor's real values, as a float: Inf / NaN are left out, an
 *     overflowing x + e too; +0 when no value is finite, and for an empty tensor;
 *   - d_minexp[s * minexp_stride] = max(emax_s - rel_bits, -94), emax_s the block-exponent of a_s (-126 for zero and
 *     subnormals), and for emax_s = 128 additionally at most floor(log2(2^128 - a_s)) - 2: exactly the word tensor s is
 *     coded under by gcow_roundtrip_rel_device (one definition serves both calls). An empty tensor gets the word of
 *     a = 0, which is -94, so the words are deterministic.
 *   Only those words are written: with minexp_stride 4 (an array of gcow_fit) the other three words of each record stay
 *   as they were; with 1 the words are packed. d_absmax (S floats) doubles as the workspace and is zeroed by a kernel in
 *   stream order; it is required when S > 0. At most three launches whatever S is (zero, pass, words); integer maxima
 *   only: the same bits run to run. No host read, no allocation; legal inside a stream capture.
 * Refusals, on the host before any launch: GCOW_ERR_INVALID for a NULL, short or foreign plan; for rel_bits > 24; with
 * S > 0 for a NULL or misaligned (4 bytes) d_absmax or d_minexp or a minexp_stride of 0; with values present for a NULL
 * or misaligned (8 bytes) d_plan, a NULL d_in or one misaligned for its element type, a d_err_in off 4 bytes. An empty
 * list returns GCOW_OK and writes nothing.
 */
gcow_status gcow_seg_rel_minexp_device(const void* h_plan, const void* d_plan, size_t plan_bytes, const void* d_in,
                                       const float* d_err_in, uint32_t rel_bits, float* d_absmax, int32_t* d_minexp,
                                       uint32_t minexp_stride, void* hip_stream);

/*
 * Decode d_in into field->data (DEVICE fp32 pointer; for a 1-D field also dtype_bf16: the fp32 decode rounded to
 * nearest even, torch's conversion) with libzfp 0.5.5 semantics. Fixed-rate streams
 * (minbits == maxbits) decode one block per thread; variable-rate streams need the index written by
 * gcow_encode_device (d_index/index_stride), or, with d_index == NULL, are decoded by a single sequential GPU lane.
 * in_bytes may be the buffer's capacity; given the stream's own length (ceil(bits / 64) words), the 1-D
 * variable-rate decoder sizes its LDS stage from the stream's average bits per block (more waves for compressible
 * streams; the result is the same either way).
 *
 * The decoders' contract (gcow_decode_device, gcow_decode_device_at; tests/test_gpu_decode_contract.py pins it):
 *   - After the stream: ANYTHING. The bits of the stream's last word above its last bit and every word after it
 *     inside in_bytes are unspecified (the encoders say the same of the words up to their capacity, and a reused
 *     buffer keeps a longer stream's words there). The decoders look past a block's last bit -- 64-bit windows, the
 *     three 32-bit words of the LDS readers, staged spans that run to in_bytes -- and no value depends on what they
 *     see there.
 *   - Readable memory: d_in must be readable for ONE 64-bit word past the word that holds the stream's last bit,
 *     ceil((bit_offset + bits) / 64) + 1 words in all, whatever in_bytes says: the global-memory readers (BitReader,
 *     GlobalWindow) take the 64 bits at a bit position inside a block from its word and, off a word boundary, the
 *     next one. The staged kernels copy a workgroup's span into LDS, never past in_bytes / 8 words, and zero-fill the
 *     LDS behind it; what their readers take further out (up to three 32-bit words past a block's last bit) comes
 *     from there. The whole-word fixed-rate kernels load the blocks' own words only. in_bytes must not exceed the
 *     readable size; in_bytes == 0 means unknown (nothing is staged).
 *   - d_in and d_index are arrays of uint64: 8-byte aligned, no more. Staged spans start on a 16-byte boundary
 *     relative to d_in, and the 16-byte loads that copy them are buffer loads, which need 4-byte alignment.
 *   - field->data: any element strides, negative ones included (data then points at the element with index 0), at
 *     any element-aligned address. Rows that are contiguous and 16-byte aligned (fp32; 8 bytes for bf16) are written
 *     with vector stores, everything else value by value; nothing outside the field's elements is written.
 *   - index_stride: every power of two from 1 to 256 (one entry per index_stride blocks, gcow_index_entries of them;
 *     a stride above the block count is one entry). A 4-D field uses its index at stride 1 only: at any other stride
 *     d_index is ignored (never read) and the stream is walked in order, as with d_index == NULL.
 */
gcow_status gcow_decode_device(const zfp_input* field, const gcow_params* p, const void* d_in, size_t in_bytes,
                               const uint64_t* d_index, uint32_t index_stride, void* hip_stream);

/*
 * Bit-stitch for sharded variable-rate streams: OR `src_bits` bits of d_src into d_dst starting at bit
 * `dst_bit_offset` (d_dst words covering the target range must be zero beyond what earlier shards wrote).
 * Used after an all-gather of per-rank shard streams to rebuild the single-stream sw/ layout.
 */
gcow_status gcow_stitch_device(uint64_t* d_dst, uint64_t dst_bit_offset, const uint64_t* d_src, uint64_t src_bits,
                               void* hip_stream);

/*
 * The whole receive side of a sharded variable-rate all-gather in one launch: nshards shard
 * streams of d_lens[r] bits (DEVICE uint64 array; the per-rank unflushed bit counts), stored shard_words apart from
 * d_src (the padded all-gather buffer), are concatenated bit-exactly -- shard r at bit d_lens[0] + ... + d_lens[r-1],
 * its flush padding dropped -- into d_dst, all of whose dst_words words are written (zero past the stream's end: the
 * single stream's flush). Equal to one gcow_encode_device of the unsharded bucket. d_dst needs no zeroing.
 */
gcow_status gcow_stitch_shards_device(uint64_t* d_dst, uint64_t dst_words, const uint64_t* d_src, uint64_t shard_words,
                                      const uint64_t* d_lens, uint32_t nshards, void* hip_stream);

/*
 * Decode-and-average of nstreams 1-D streams of one bucket shape (the compressed all-gather DDP hook's receive side;
 * hw/models/train_imagenet.py:446-475 is the caller contract): field->data (DEVICE, 1-D, fp32 or bf16) receives,
 * elementwise in fp32, ((0 + x_0) + x_1 + ... + x_{n-1}) / nstreams with x_r the libzfp decode of stream r (a bf16
 * field -- a bf16 gradient bucket -- receives that fp32 mean rounded to nearest even, torch's conversion). Streams start
 * stream_words words apart at d_streams; streams_bytes is the buffer's size, which must cover nstreams * stream_words
 * + 2 words (the decoders read 64-bit windows past a stream's last bit; GCOW_ERR_INVALID otherwise). Fixed rate: any
 * parameters, d_index NULL and index_words = index_stride = 0. Variable rate: any parameters (minbits <= 1,
 * maxbits >= 160 take the closed-form decoder, others the generic one) and every stream's block index (index_stride
 * 8 or 16, entries index_words apart at d_index, as gcow_encode_device writes them; or GCOW_INDEX_PACKED16, entries
 * as gcow_index_pack16_device writes them -- the size of the 16-block index, decoded in 8-block chunks).
 * Every slot may hold anything from its stream's last bit to stream_words, and so may the 2 words after the last
 * slot (the decoders' contract above: gcow_decode_device). stream_words may be odd: streams then start 8 bytes off a
 * 16-byte boundary, which the kernels allow for. Index entries are relative to each stream's first word. The output
 * follows the same rules as gcow_decode_device's (any stride, any element-aligned base).
 */
gcow_status gcow_decode_mean_device(const zfp_input* field, const gcow_params* p, const uint64_t* d_streams,
                                    size_t streams_bytes, uint64_t stream_words, uint32_t nstreams,
                                    const uint64_t* d_index, uint64_t index_words, uint32_t index_stride,
                                    void* hip_stream);

/*
 * W received streams straight into the stream of their mean (the sharded DDP hook's second stage: the mean shard
 * travels compressed). field gives the shape only: 1-D, n values; field->data and field->dtype are ignored. The call
 * is defined by two others:
 *   1. m = what gcow_decode_mean_device writes into an fp32 field of n values from the same d_streams, streams_bytes,
 *      stream_words, nstreams, d_index_in, index_words and index_stride_in under p_in:
 *      ((0 + x_0) + x_1 + ...) / nstreams in fp32, no contraction.
 *   2. d_err_out == NULL (d_err_in must be NULL too): d_out, *d_total_bits and d_index_out receive exactly what
 *      gcow_encode_device of m under p_out writes. Otherwise they, and d_err_out, receive exactly what
 *      gcow_encode_residual_device(m, d_err_in, d_err_out, ...) under p_out writes: y = m + e_in,
 *      e_out = finite(y - decode(stream)); d_err_in == d_err_out (in place) is allowed, d_err_in NULL means zeros.
 * Nothing is written past the stream's flushed words nor past e_out[n - 1]. Asynchronous on hip_stream: no
 * allocation, no host synchronisation. n = 0 writes *d_total_bits = 0 and returns GCOW_OK.
 * Two paths give that result (gcow_decode_mean_encode_path tells which one a call takes):
 *   GCOW_MEANENC_FUSED_FIXED  p_in and p_out the same set, fixed rate with whole-word blocks (minbits == maxbits in
 *      {32, 64}, maxprec >= 32, minexp <= -154; rate 8 and 16), no index in or out, error buffers 16-byte aligned: one
 *      kernel (per block the W words decoded and summed in registers, the mean coded, the word stored and -- with
 *      error buffers -- decoded from its register for e_out), plus a one-lane kernel for a partial last block. The
 *      mean is never stored. No workspace.
 *   GCOW_MEANENC_COMPOSED     every other legal call (any other fixed rate, p_in != p_out, variable rate with the
 *      input index at stride 8, 16 or GCOW_INDEX_PACKED16, an output index, error buffers off 16-byte alignment):
 *      gcow_decode_mean_device into n fp32 values at the head of the workspace, then gcow_encode_device or
 *      gcow_encode_residual_device on that field with its own workspace behind.
 * gcow_decode_mean_encode_workspace_bytes: 0 for the fused path (decided from the parameter sets alone: error buffers
 * taken as aligned, no index), else 4 n rounded up to 256 plus the larger of the two inner calls' workspaces. A call
 * that takes the composed path for its pointers' sake needs the composed size. d_workspace 16-byte aligned.
 * Status codes follow the two calls: GCOW_ERR_INVALID when streams_bytes lacks the nstreams * stream_words + 2 words,
 * for a wrong or missing input index, a short workspace, d_err_in without d_err_out; GCOW_ERR_CAPACITY when
 * out_capacity < gcow_max_output_bytes of the fp32 field of n values under p_out; GCOW_ERR_UNSUPPORTED for dims != 1.
 * gcow_decode_mean_encode_path: the path for these arguments, or -1 for a call that is refused. Pointers are inspected
 * for presence (the indexes) and alignment (the error buffers) only, never dereferenced. All three functions decide
 * through the same rule.
 */
enum { GCOW_MEANENC_COMPOSED = 0, GCOW_MEANENC_FUSED_FIXED = 1 };
int gcow_decode_mean_encode_path(const zfp_input* field, const gcow_params* p_in, const gcow_params* p_out,
                                 const float* d_err_in, const float* d_err_out, const uint64_t* d_index_in,
                                 const uint64_t* d_index_out);
size_t gcow_decode_mean_encode_workspace_bytes(const zfp_input* field, const gcow_params* p_in,
                                               const gcow_params* p_out);
gcow_status gcow_decode_mean_encode_device(const zfp_input* field, const gcow_params* p_in, const uint64_t* d_streams,
                                           size_t streams_bytes, uint64_t stream_words, uint32_t nstreams,
                                           const uint64_t* d_index_in, uint64_t index_words, uint32_t index_stride_in,
                                           const gcow_params* p_out, const float* d_err_in, float* d_err_out,
                                           void* d_out, size_t out_capacity, uint64_t* d_total_bits, void* d_workspace,
                                           size_t workspace_bytes, uint64_t* d_index_out, uint32_t index_stride_out,
                                           void* hip_stream);

/*
 * Packed 16-block index (index_stride GCOW_INDEX_PACKED16 in gcow_decode_mean_device): one uint64 per 16 blocks, the
 * low 48 bits the stream bit position of block 16 c (as the index every 16 blocks holds it), the high 16 bits the
 * offset of block 16 c + 8 from it (0 where that block does not exist). It carries the 8-block chunk starts at the
 * 16-block index's size, so a receiver of every rank's index (the compressed all-gather hook) decodes in 8-block
 * chunks without the doubled index on the wire. gcow_index_pack16_device builds it on the device from the index every
 * 8 blocks of one stream of `field`'s shape (gcow_index_entries(field, 8) entries at d_index8) into
 * gcow_index_entries(field, 16) entries at d_out. GCOW_ERR_UNSUPPORTED when p lets 8 blocks exceed 65535 bits
 * (minbits > 8191) or the stream 2^48 bits; 1-D fields only.
 */
#define GCOW_INDEX_PACKED16 0x1010u
gcow_status gcow_index_pack16_device(const zfp_input* field, const gcow_params* p, const uint64_t* d_index8,
                                     uint64_t* d_out, void* hip_stream);

/*
 * zfp 0.5.5 stream header: the byte format zfpy.compress_numpy writes (hw/models/train_imagenet.py:459-465 calls
 * it), i.e. libzfp zfp_write_header(ZFP_HEADER_FULL): magic 'z','f','p' + codec version 5 (32 bits), field metadata
 * (52 bits: sizes, dims - 1, type - 1) and the compression mode (12-bit short form for rate / precision /
 * accuracy, else 64 bits). sw/ declares ZFP_HEADER_* (sw/include/common.h:16-21) but never writes a header.
 * Header metadata records zfp_type_float for fp32 and bf16 inputs (bf16 is coded by exact widening).
 */
uint gcow_header_bits(const gcow_params* p); /* 96 or 148 */
/* Host: write the header of (field shape, p) into words[0..3) (zeroed by the call); returns its bit count. */
uint gcow_write_header(const zfp_input* field, const gcow_params* p, uint64_t* words);
/* Host: parse a header (at least 3 words). Fills field->nx..nz and dtype (data/strides untouched) and p; returns
 * the header bit count, 0 when the magic or version does not match or the type is not float. */
uint gcow_read_header(const uint64_t* words, size_t nwords, zfp_input* field, gcow_params* p);
/* Workspace for gcow_encode_device_zfp: the headerless stream plus gcow_encode_workspace_bytes(). */
size_t gcow_encode_zfp_workspace_bytes(const zfp_input* field, const gcow_params* p);
/* Device encode to a header-prefixed stream (byte-identical to zfpy.compress_numpy). Capacity:
 * gcow_max_output_bytes() + 24. *d_total_bits (device, optional) = header bits + stream bits. */
gcow_status gcow_encode_device_zfp(const zfp_input* field, const gcow_params* p, void* d_out, size_t out_capacity,
                                   uint64_t* d_total_bits, void* d_workspace, size_t workspace_bytes,
                                   void* hip_stream);
/*
 * Decode a stream whose first block starts at bit_offset (e.g. gcow_read_header()'s return value); any bit_offset,
 * with anything below it. The contract of gcow_decode_device holds (in_bytes counts from d_in, not from the offset).
 *   - Index entries are RELATIVE TO bit_offset: block c * index_stride starts at bit bit_offset + d_index[c]. An
 *     index written by gcow_encode_device for the headerless stream serves the same stream behind a header unchanged.
 *   - Random access to a part of a field: a part cut along the slowest axis at a multiple of 4 rows consists of
 *     whole blocks that are consecutive in the stream (1-D: any multiple of 4 values). Describe the part alone in
 *     `field` and enter the whole stream at its first block b: fixed rate at bit_offset = b * maxbits; variable rate
 *     with d_index advanced to the part's first entry, d_index + b / index_stride (b a multiple of index_stride), and
 *     the bit_offset the entries are relative to -- 0 for the absolute entries gcow_encode_device and
 *     gcow_encode_device_append write. d_in and in_bytes stay those of the whole stream.
 *   - Whole-word fixed-rate streams (1-D rate 8 and 16, 3-D blocks of 2^k words) take their word kernels when
 *     bit_offset is a multiple of 32 and the generic block decoder otherwise; the values are the same.
 */
gcow_status gcow_decode_device_at(const zfp_input* field, const gcow_params* p, const void* d_in, size_t in_bytes,
                                  uint64_t bit_offset, const uint64_t* d_index, uint32_t index_stride,
                                  void* hip_stream);

/* Per-stage batched device kernels (the hw/stages split, for parity bisection; sw/tests/test_stages.cpp). */
gcow_status gcow_stage_emax_device(const float* d_blocks, uint32_t nblocks, uint32_t dims, int32_t* d_emax,
                                   void* hip_stream);
gcow_status gcow_stage_cast_device(const float* d_blocks, const int32_t* d_emax, uint32_t nblocks, uint32_t dims,
                                   int32_t* d_iblocks, void* hip_stream);
gcow_status gcow_stage_xform_device(int32_t* d_iblocks, uint32_t nblocks, uint32_t dims, int inverse,
                                    void* hip_stream);
gcow_status gcow_stage_reorder_device(const int32_t* d_iblocks, uint32_t nblocks, uint32_t dims,
                                      uint32_t* d_ublocks, void* hip_stream);
/* Embedded coder on one ublock per lane, each into its own zeroed slot of slot_words words after `header_bits`
 * bits of header (value header); bits written per block to d_bits. */
gcow_status gcow_stage_encode_ints_device(const uint32_t* d_ublocks, uint32_t nblocks, uint32_t dims,
                                          uint32_t budget, uint32_t maxprec, uint64_t* d_slots, uint32_t slot_words,
                                          uint32_t* d_bits, void* hip_stream);

/* Measurement kernel (bench.py roofline.copy_ceiling): the fixed-rate 1-D encoder's memory access pattern without the
 * coding -- the same grid, loads of every full 4-value block (16 B fp32 / 8 B bf16) and one out_bits_per_block (32 or
 * 64) store per block -- i.e. the HBM floor that kernel can reach. Output bytes are not a stream. */
gcow_status gcow_copy_pattern_device(const void* d_in, int dtype, size_t nvals, uint32_t out_bits_per_block,
                                     void* d_out, void* hip_stream);

/* Deterministic synthetic gradient bucket on the device (bench / smoke inputs; SURVEY 8(d) distribution):
 * N(0, sigma) via counter-based splitmix64 + Box-Muller, with zero / tiny / subnormal 4-value blocks injected at
 * 1/64, 1/4096, 1/4096. */
gcow_status gcow_fill_normal_device(float* d_out, size_t count, double sigma, uint64_t seed, int inject,
                                    void* hip_stream);

/* TEST / MEASUREMENT ONLY -- not part of the drop-in surface. Selects a measured-and-not-kept form of the 1-D
 * variable-rate encoder for the whole process (bit-identical output; tests cover each form): form 0 = the tile form
 * (the default), 1 = count + scan + range coder, 2 = the decoupled look-back single pass; spin (form 2) = polls before
 * a missing predecessor's total is computed locally (< 0: default); stats != 0 (form 2) records look-back statistics.
 * No reference counterpart. */
gcow_status gcow_debug_set_var1d_variant(int form, int spin, int stats);

#ifdef __cplusplus
}
#endif
#endif /* GCOW_H */
