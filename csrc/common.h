// Common helpers for sonata_amd CDNA4 (gfx950) kernels.
//
// Target: MI355X only — wave64, MFMA bf16 16x16x32, 160 KiB LDS/CU,
// 8 XCDs.  No CUDA-compat shims, no multi-arch dispatch.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <cstdint>
#include <type_traits>

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

// ------------------------------------------------------------------------
// LDS staging of the channel-last MFMA conv kernels (conv1d_cl.hip,
// resblock_cl.hip).  512 threads; a wave stages 16 rows of 32 channels per
// pass of 128 rows, 16 bytes per lane: row sr_base0 + p*128 + sr_l, chunk
// sr_c (the conflict-free lane map described in resblock_cl.hip).
//
// Both helpers issue every global load of their group first and only then
// write LDS, with nothing conditional in between, so a group costs one
// memory round trip instead of one per load.  Every condition therefore
// sits outside the group or behind all of its loads: a test between one
// load and its write makes the compiler wait for each load on its own.
// ------------------------------------------------------------------------

// Calls f(std::integral_constant<int, n>) for a runtime n in [1, N]: the
// tap count of a staging window becomes a compile-time count chosen by one
// uniform branch.
template <int N, class F>
__device__ __forceinline__ void with_count(int n, F&& f) {
  if constexpr (N <= 1) {
    f(std::integral_constant<int, 1>{});
  } else {
    if (n == N) f(std::integral_constant<int, N>{});
    else with_count<N - 1>(n, f);
  }
}

// One weight window: Ws[tc][row][sr_c..+8] = w[wbase + tc*tap_stride +
// row*row_pitch + sr_c..+8] for NC taps and all BN rows.  NC is the exact
// tap count of the window, so no tap beyond the kernel's last is read.
// "Does this wave stage rows at all" (BN < 128) is tested once, around the
// whole group.
template <int NC, int BN, int PITCH>
__device__ __forceinline__ void stage_w_window(
    bf16 (*Ws)[BN][PITCH], const bf16* __restrict__ w, long wbase,
    long tap_stride, long row_pitch, int sr_base0, int sr_l, int sr_c) {
  static_assert(BN % 16 == 0 && (BN <= 128 || BN % 128 == 0),
                "a wave's 16 rows of a pass are all inside BN or all outside");
  constexpr int WPASS = (BN + 127) / 128;
  if (sr_base0 < BN) {
    // uniform base per (tap, pass) + one 32-bit lane offset for all of them
    const int off = (sr_base0 + sr_l) * (int)row_pitch + sr_c;
    ulonglong2 wv[NC][WPASS];
#pragma unroll
    for (int tc = 0; tc < NC; ++tc)
#pragma unroll
      for (int p = 0; p < WPASS; ++p) {
        const bf16* wt = w + wbase + tc * tap_stride + p * 128 * row_pitch;
        wv[tc][p] = *(const ulonglong2*)&wt[off];
      }
#pragma unroll
    for (int tc = 0; tc < NC; ++tc)
#pragma unroll
      for (int p = 0; p < WPASS; ++p)
        *(ulonglong2*)&Ws[tc][sr_base0 + p * 128 + sr_l][sr_c] = wv[tc][p];
  }
}

// Interior x staging of one K slice: Xs[r][sr_c..+8] = pre(x0[r*C + sr_c..+8])
// for r in [0, nrows), nrows <= XPASS*128, all rows and channels inside the
// tensor.  A lane whose row is >= nrows loads row nrows-1 instead (a row the
// group reads anyway) and writes nothing; pre is LeakyReLU(slope) where
// do_pre (uniform), tested once around the group's arithmetic.  x0 is
// uniform and nrows * C < 2^31 (nrows <= 384), so lane offsets are 32-bit.
template <int XPASS, int PITCH>
__device__ __forceinline__ void stage_x_interior(
    bf16 (*Xs)[PITCH], const bf16* __restrict__ x0, long C, int nrows,
    bool do_pre, float slope, int sr_base0, int sr_l, int sr_c) {
  __attribute__((aligned(16))) bf16 v8[XPASS][8];
#pragma unroll
  for (int p = 0; p < XPASS; ++p) {
    const int r = min(sr_base0 + p * 128 + sr_l, nrows - 1);
    *(ulonglong2*)v8[p] = *(const ulonglong2*)&x0[r * (int)C + sr_c];
  }
  if (do_pre) {
#pragma unroll
    for (int p = 0; p < XPASS; ++p)
#pragma unroll
      for (int q = 0; q < 8; ++q)
        v8[p][q] = f2bf(lrelu_(bf2f(v8[p][q]), slope));
  }
#pragma unroll
  for (int p = 0; p < XPASS; ++p) {
    const int r = sr_base0 + p * 128 + sr_l;
    if (r < nrows) *(ulonglong2*)&Xs[r][sr_c] = *(ulonglong2*)v8[p];
  }
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
