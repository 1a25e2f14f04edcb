// Host-side argument checks of gcow_rate_table_residual_device and gcow_encode_residual_fitted_device as a stand-alone
// program for a sanitizer build on the CPU: every call below returns before its first launch, so no device is needed
// and the "device" pointers are fake addresses that are never dereferenced. Build gcow_api.cpp and this file with the
// host sanitizers and link the kernel objects of a normal build (run from the repository root after `make`):
//
//   O=gcow_amd/csrc/build; S="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
//   for f in tools/host_checks/resid_fit_args.cpp gcow_amd/csrc/gcow_api.cpp; do
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC $S -Iinclude -Igcow_amd/csrc -c $f \
//       -o $O/san_$(basename $f).obj; done
//   hipcc --offload-arch=gfx950 $S $O/san_*.obj $(ls $O/*.o | grep -v gcow_api) -o $O/resid_fit_args
//   $O/resid_fit_args
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "gcow.h"

static int failures = 0;

#define EXPECT(call, want)                                                                          \
  do {                                                                                              \
    const int got_ = (int)(call);                                                                   \
    if (got_ != (int)(want)) {                                                                      \
      std::printf("line %d: %s = %d, expected %d (%s)\n", __LINE__, #call, got_, (int)(want), gcow_last_error()); \
      failures++;                                                                                   \
    }                                                                                               \
  } while (0)

static zfp_input field(data_type dt, uintptr_t data, size_t nx, size_t ny = 0, ptrdiff_t sx = 0)
{
  zfp_input f;
  std::memset(&f, 0, sizeof(f));
  f.dtype = dt;
  f.data = (void*)data;
  f.nx = nx;
  f.ny = ny;
  f.sx = sx;
  return f;
}

int main()
{
  const uintptr_t X = 0x10000, EI = 0x20000, EO = 0x30000, M = 0x40000, OUT = 0x50000, BITS = 0x60000, WS = 0x70000,
                  T = 0x80000, IDX = 0x90000;
  const size_t n = 64;
  zfp_input f = field(dtype_float, X, n), yf = field(dtype_float, 0, n);

  // ---- gcow_rate_table_residual_device
  const size_t tws = gcow_rate_table_workspace_bytes(&f);
  EXPECT(gcow_rate_table_residual_device(nullptr, (const float*)EI, 64, (uint64_t*)T, (void*)WS, tws, nullptr),
         GCOW_ERR_INVALID);
  zfp_input f2d = field(dtype_float, X, 8, 8), fstr = field(dtype_float, X, 32, 0, 2), fint = field(dtype_int32, X, n),
            fnull = field(dtype_float, 0, n), foff = field(dtype_float, X + 2, n);
  EXPECT(gcow_rate_table_residual_device(&f2d, (const float*)EI, 64, (uint64_t*)T, (void*)WS, tws, nullptr),
         GCOW_ERR_INVALID);
  EXPECT(gcow_rate_table_residual_device(&fstr, (const float*)EI, 64, (uint64_t*)T, (void*)WS, tws, nullptr),
         GCOW_ERR_INVALID);
  EXPECT(gcow_rate_table_residual_device(&fint, (const float*)EI, 64, (uint64_t*)T, (void*)WS, tws, nullptr),
         GCOW_ERR_UNSUPPORTED);
  EXPECT(gcow_rate_table_residual_device(&f, (const float*)EI, 64, nullptr, (void*)WS, tws, nullptr), GCOW_ERR_INVALID);
  EXPECT(gcow_rate_table_residual_device(&f, (const float*)EI, 64, (uint64_t*)(T + 4), (void*)WS, tws, nullptr),
         GCOW_ERR_INVALID);
  EXPECT(gcow_rate_table_residual_device(&f, (const float*)EI, 64, (uint64_t*)T, nullptr, tws, nullptr),
         GCOW_ERR_INVALID);
  EXPECT(gcow_rate_table_residual_device(&f, (const float*)EI, 64, (uint64_t*)T, (void*)WS, tws - 8, nullptr),
         GCOW_ERR_INVALID);
  EXPECT(gcow_rate_table_residual_device(&fnull, (const float*)EI, 64, (uint64_t*)T, (void*)WS, tws, nullptr),
         GCOW_ERR_INVALID);
  EXPECT(gcow_rate_table_residual_device(&foff, (const float*)EI, 64, (uint64_t*)T, (void*)WS, tws, nullptr),
         GCOW_ERR_INVALID);
  EXPECT(gcow_rate_table_residual_device(&f, (const float*)(EI + 2), 64, (uint64_t*)T, (void*)WS, tws, nullptr),
         GCOW_ERR_INVALID);

  // ---- gcow_encode_residual_fitted_device
  const gcow_params hp = {1u, 16658u, 64u, 0};
  const size_t cap = gcow_max_output_bytes(&yf, &hp), wsb = gcow_encode_workspace_bytes(&yf, &hp);
  for (int me : {-154, 133}) {  // neither query depends on minexp
    const gcow_params q = {1u, 16658u, 64u, me};
    EXPECT(gcow_max_output_bytes(&yf, &q) == cap, 1);
    EXPECT(gcow_encode_workspace_bytes(&yf, &q) == wsb, 1);
  }
  auto call = [&](const zfp_input* fp, uintptr_t m, uintptr_t ei, uintptr_t eo, uintptr_t out, size_t c, uintptr_t ws,
                  size_t wb, uintptr_t idx, uint32_t stride) {
    return gcow_encode_residual_fitted_device(fp, 64, (const int32_t*)m, (const float*)ei, (float*)eo, (void*)out, c,
                                              (uint64_t*)BITS, (void*)ws, wb, (uint64_t*)idx, stride, nullptr);
  };
  zfp_input fx4 = field(dtype_float, X + 4, n), fb8 = field(dtype_bf16, X + 8, n);
  EXPECT(call(nullptr, M, EI, EO, OUT, cap, WS, wsb, 0, 0), GCOW_ERR_INVALID);
  EXPECT(call(&f2d, M, EI, EO, OUT, cap, WS, wsb, 0, 0), GCOW_ERR_UNSUPPORTED);
  EXPECT(call(&fstr, M, EI, EO, OUT, cap, WS, wsb, 0, 0), GCOW_ERR_UNSUPPORTED);
  EXPECT(call(&fint, M, EI, EO, OUT, cap, WS, wsb, 0, 0), GCOW_ERR_UNSUPPORTED);
  EXPECT(call(&f, 0, EI, EO, OUT, cap, WS, wsb, 0, 0), GCOW_ERR_INVALID);
  EXPECT(call(&f, M + 2, EI, EO, OUT, cap, WS, wsb, 0, 0), GCOW_ERR_INVALID);
  EXPECT(call(&f, M, EI, 0, OUT, cap, WS, wsb, 0, 0), GCOW_ERR_INVALID);
  EXPECT(call(&f, M, EI, EO, 0, cap, WS, wsb, 0, 0), GCOW_ERR_INVALID);
  EXPECT(call(&f, M, EI, EO, OUT + 4, cap, WS, wsb, 0, 0), GCOW_ERR_INVALID);
  EXPECT(call(&f, M, EI, EO, OUT, cap, WS, wsb, IDX, 3), GCOW_ERR_INVALID);
  EXPECT(call(&f, M, EI, EO, OUT, cap, WS, wsb, IDX, 512), GCOW_ERR_INVALID);
  EXPECT(call(&fnull, M, EI, EO, OUT, cap, WS, wsb, 0, 0), GCOW_ERR_INVALID);
  EXPECT(call(&fx4, M, EI, EO, OUT, cap, WS, wsb, 0, 0), GCOW_ERR_UNSUPPORTED);
  EXPECT(call(&fb8, M, EI, EO, OUT, cap, WS, wsb, 0, 0), GCOW_ERR_UNSUPPORTED);
  EXPECT(call(&f, M, EI + 4, EO, OUT, cap, WS, wsb, 0, 0), GCOW_ERR_UNSUPPORTED);
  EXPECT(call(&f, M, EI, EO + 8, OUT, cap, WS, wsb, 0, 0), GCOW_ERR_UNSUPPORTED);
  EXPECT(call(&f, M, 0, EO + 8, OUT, cap, WS, wsb, 0, 0), GCOW_ERR_UNSUPPORTED);
  EXPECT(call(&f, M, EI, EO, OUT, cap - 8, WS, wsb, 0, 0), GCOW_ERR_CAPACITY);
  EXPECT(call(&f, M, EI, EO, OUT, cap, WS, wsb - 8, 0, 0), GCOW_ERR_INVALID);
  EXPECT(call(&f, M, EI, EO, OUT, cap, 0, wsb, 0, 0), GCOW_ERR_INVALID);
  std::printf(failures ? "%d FAILED\n" : "resid_fit_args ok\n", failures);
  return failures != 0;
}
