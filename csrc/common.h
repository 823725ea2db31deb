// Common helpers for sonata_amd CDNA4 (gfx950) kernels.
//
// Target: MI355X only — wave64, MFMA bf16 16x16x32, 160 KiB LDS/CU,
// 8 XCDs.  No CUDA-compat shims, no multi-arch dispatch.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <cstdint>

#define WAVE 64

using bf16 = __hip_bfloat16;

// MFMA fragment vector types (gfx950 mfma_f32_16x16x32_bf16):
// A/B: 8 bf16 per lane (4 VGPRs), C/D: 4 f32 per lane.
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ float bf2f(bf16 v) { return __bfloat162float(v); }
__device__ __forceinline__ bf16 f2bf(float v) { return __float2bfloat16(v); }

template <typename T> __device__ __forceinline__ float ld_f(const T* p);
template <> __device__ __forceinline__ float ld_f<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ld_f<bf16>(const bf16* p) { return bf2f(*p); }

template <typename T> __device__ __forceinline__ void st_f(T* p, float v);
template <> __device__ __forceinline__ void st_f<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void st_f<bf16>(bf16* p, float v) { *p = f2bf(v); }

__device__ __forceinline__ float sigmoidf_(float x) {
  return 1.0f / (1.0f + __expf(-x));
}

__device__ __forceinline__ float lrelu_(float x, float slope) {
  return x > 0.0f ? x : x * slope;
}

// Zero n bf16 elements from p with all nthreads threads of the block.  No
// alignment is assumed beyond the element's own: the span is split by
// ADDRESS into a scalar head up to the next 16-byte boundary, a body of
// 16-byte stores and a scalar tail (the split pcm16_rows makes).
__device__ __forceinline__ void zero_span_bf16(bf16* p, long n, int tid,
                                               int nthreads) {
  unsigned short* q = reinterpret_cast<unsigned short*>(p);
  const long mis = (long)((reinterpret_cast<uintptr_t>(q) >> 1) & 7);
  const long head = min(n, (8 - mis) & 7);
  const long nvec = (n - head) >> 3;
  const long tail0 = head + (nvec << 3);
  if (tid < head) q[tid] = 0;
  ulonglong2* body = reinterpret_cast<ulonglong2*>(q + head);
  for (long v = tid; v < nvec; v += nthreads) body[v] = make_ulonglong2(0, 0);
  if (tail0 + tid < n) q[tail0 + tid] = 0;
}

// Dead-tile fill of the channel-last kernels: zero rows [0, nrows) x
// columns [c0, c0+ncols) of a [.][pitch] bf16 image whose row 0 starts at
// base.  A tile that spans whole rows is one contiguous span; a column
// tile (Cout wider than the block's BN) is one span per row, a wave each.
__device__ __forceinline__ void zero_tile_bf16(bf16* base, long nrows,
                                               int pitch, int c0, int ncols,
                                               int tid, int nthreads) {
  if (ncols == pitch) {
    zero_span_bf16(base, nrows * pitch, tid, nthreads);
    return;
  }
  for (long r = tid / WAVE; r < nrows; r += nthreads / WAVE)
    zero_span_bf16(base + r * pitch + c0, ncols, tid % WAVE, WAVE);
}

#define HIP_CHECK(expr)                                                     \
  do {                                                                      \
    hipError_t _e = (expr);                                                 \
    if (_e != hipSuccess) {                                                 \
      TORCH_CHECK(false, "HIP error: ", hipGetErrorString(_e), " at ",      \
                  __FILE__, ":", __LINE__);                                 \
    }                                                                       \
  } while (0)

static inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

// dtype dispatch over float / bf16 torch tensors
#define DISPATCH_FT_CONV(TENSOR, ...)                                      \
  do {                                                                     \
    if ((TENSOR).scalar_type() == at::kFloat) {                            \
      using scalar_t = float;                                              \
      __VA_ARGS__;                                                         \
    } else if ((TENSOR).scalar_type() == at::kBFloat16) {                  \
      using scalar_t = bf16;                                               \
      __VA_ARGS__;                                                         \
    } else {                                                               \
      TORCH_CHECK(false, "unsupported dtype");                             \
    }                                                                      \
  } while (0)
