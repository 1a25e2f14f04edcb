// pipe.h -- raw buffer loads and stores issued from inline asm with hand-counted s_waitcnt, shared by the one-shot
// fixed-rate 1-D encoder (enc_fixed1d.hip), the fixed-rate 1-D decoder (dec1d.hip) and decode_mean (decode_mean.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec_device.h"

namespace gcow {

// ---- hand-counted memory pipeline of the fixed-rate 1-D kernels
// Loads and stores are raw buffer instructions issued from inline asm, so the compiler's waitcnt pass does not see
// them; the waits are counted here instead. (With compiler-tracked loads the conditional / loop-carried prefetch
// collapsed to s_waitcnt vmcnt(0) at the loop head, i.e. every block waited for the previous block's store ack:
// vmcnt counts stores and loads together, in issue order.) Out-of-range lanes read zeros and their stores are dropped
// by the buffer range check (num_records), which keeps the loop exit wave-uniform and every step's op count fixed.
typedef int pipe_v4i __attribute__((ext_vector_type(4)));
typedef float pipe_v4f __attribute__((ext_vector_type(4)));
typedef unsigned int pipe_v2u __attribute__((ext_vector_type(2)));
typedef unsigned int pipe_v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ pipe_v4i buf_rsrc(const void* p, uint32_t bytes)
{
  const uint64_t a = (uint64_t)p;
  pipe_v4i r;
  r.x = (int)(uint32_t)a;
  r.y = (int)((uint32_t)(a >> 32) & 0xffffu);  // stride 0
  r.z = (int)bytes;                             // num_records: range check in bytes
  r.w = 0x00020000;                             // gfx9 dword-3 config (raw buffer, no swizzle)
  return r;
}

template <int DT> struct PipeRow;
template <> struct PipeRow<DT_F32> {
  typedef pipe_v4f T;
  static __device__ __forceinline__ T load(uint32_t off, pipe_v4i rs)
  {
    T v;
    asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen nt" : "=v"(v) : "v"(off), "s"(rs) : "memory");
    return v;
  }
  static __device__ __forceinline__ void unpack(const T& v, float* f) { f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w; }
};
template <> struct PipeRow<DT_BF16> {
  typedef pipe_v2u T;
  static __device__ __forceinline__ T load(uint32_t off, pipe_v4i rs)
  {
    T v;
    asm volatile("buffer_load_dwordx2 %0, %1, %2, 0 offen nt" : "=v"(v) : "v"(off), "s"(rs) : "memory");
    return v;
  }
  static __device__ __forceinline__ void unpack(const T& v, float* f)
  {
    f[0] = __uint_as_float(v.x << 16);
    f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = __uint_as_float(v.y << 16);
    f[3] = __uint_as_float(v.y & 0xffff0000u);
  }
};

template <int N, typename T>
__device__ __forceinline__ void pipe_wait(T& v)
{
  asm volatile("s_waitcnt vmcnt(%1)" : "+v"(v) : "n"(N) : "memory");  // ties v's uses to after the wait
}

template <uint32_t WB>
__device__ __forceinline__ void pipe_store(uint32_t off, pipe_v4i rs, uint64_t w)
{
  if constexpr (WB == 64)
    asm volatile("buffer_store_dwordx2 %0, %1, %2, 0 offen nt" : : "v"(w), "v"(off), "s"(rs) : "memory");
  else
    asm volatile("buffer_store_dword %0, %1, %2, 0 offen nt" : : "v"((uint32_t)w), "v"(off), "s"(rs) : "memory");
}

__device__ __forceinline__ uint32_t buf_load_u32(uint32_t off, pipe_v4i rs)
{
  uint32_t v;
  asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=v"(v) : "v"(off), "s"(rs) : "memory");
  return v;
}

__device__ __forceinline__ pipe_v4u buf_load_b128(uint32_t off, pipe_v4i rs)
{
  pipe_v4u v;
  asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(v) : "v"(off), "s"(rs) : "memory");
  return v;
}

// One stream word (a whole 64- or 32-bit block) per load, non-temporal
template <uint32_t WB> struct PipeWord;
template <> struct PipeWord<64> {
  typedef pipe_v2u T;
  static __device__ __forceinline__ T load(uint32_t off, pipe_v4i rs)
  {
    T v;
    asm volatile("buffer_load_dwordx2 %0, %1, %2, 0 offen nt" : "=v"(v) : "v"(off), "s"(rs) : "memory");
    return v;
  }
  static __device__ __forceinline__ uint64_t get(const T& v) { return (uint64_t)v.x | ((uint64_t)v.y << 32); }
};
template <> struct PipeWord<32> {
  typedef uint32_t T;
  static __device__ __forceinline__ T load(uint32_t off, pipe_v4i rs)
  {
    T v;
    asm volatile("buffer_load_dword %0, %1, %2, 0 offen nt" : "=v"(v) : "v"(off), "s"(rs) : "memory");
    return v;
  }
  static __device__ __forceinline__ uint64_t get(const T& v) { return (uint64_t)v; }
};

// Wait until at most N vector memory operations are outstanding, tying the TR table registers to after the wait.
template <int N, uint32_t TR>
__device__ __forceinline__ void table_wait(pipe_v4u (&tv)[TR])
{
  if constexpr (TR == 3) {
    asm volatile("s_waitcnt vmcnt(%3)" : "+v"(tv[0]), "+v"(tv[1]), "+v"(tv[2]) : "n"(N) : "memory");
  } else {
    static_assert(TR == 4, "three or four table registers per lane");
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(tv[0]), "+v"(tv[1]), "+v"(tv[2]), "+v"(tv[3]) : "n"(N) : "memory");
  }
}

}  // namespace gcow
