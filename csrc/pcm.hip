// Batched on-device PCM: [B, N] f32 / bf16 rows -> peak-normalised int16.
//
// Device counterpart of sonata_amd/audio/samples.py to_i16 (the CPU path and
// the semantic reference), bit for bit:
//
//   peak  = max_{i < len} |x[i]|                       (absmax_rows)
//   scale = peak > 1e-8 ? (float)(32767.0 / (double)peak) : 0   (in double,
//           rounded once to f32: NumPy applies the Python-float scale as an
//           f32 scalar); 32767.f without peak normalisation
//   y[i]  = (int16) trunc(clamp(x[i] * scale, -32768, 32767))    (pcm16_rows)
//
// Columns at or past len[b] are written as 0, so appended silence is free:
// the host slices len + silence samples out of a row.
//
// g711_rows writes 8-bit G.711 instead: the mu-law or A-law code of that
// int16 (sonata_amd/audio/g711.py encode, bit for bit), companded in the
// same pass, with the row's code of sample 0 in place of the zeros.
//
// Rows start at x + b*stride and y + b*N_out: nothing is assumed about
// their alignment.  Each tile is split by ADDRESS into a scalar head up to
// the next 16-byte boundary, a 16-byte vector body and a scalar tail.
#include "common.h"

#include <climits>
#include <cstdint>

#define PCM_THREADS 256
// elements per workgroup tile, both kernels: 256 threads x 16 elements
#define PCM_TILE 4096

typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;
typedef __attribute__((ext_vector_type(8))) short i16x8;

template <typename T> struct PcmVec;
// f32: one 16-byte load is 4 elements
template <> struct PcmVec<float> {
  static constexpr int V = 4;
  __device__ static __forceinline__ void load(const float* p, float* o) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = v[j];
  }
};
// bf16: one 16-byte load is 8 elements; widening to f32 is exact
template <> struct PcmVec<bf16> {
  static constexpr int V = 8;
  __device__ static __forceinline__ void load(const bf16* p, float* o) {
    const u16x8 v = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = __uint_as_float((unsigned)v[j] << 16);
  }
};

// elements from p to the next 16-byte boundary (p is element-aligned)
template <typename T>
__device__ __forceinline__ int head_elems_(const T* p) {
  constexpr int V = 16 / sizeof(T);
  const int mis = (int)((reinterpret_cast<uintptr_t>(p) / sizeof(T)) % V);
  return (V - mis) % V;
}

// --------------------------------------------------------------------------
// absmax_rows: grid (tiles, B).  Thread maximum over its elements, wave-64
// shuffle, the 4 waves through LDS, then ONE atomicMax per workgroup on the
// unsigned bit pattern of the non-negative float (that order is the float
// order, and a maximum does not depend on arrival order: deterministic).
// peaks[] is zeroed on the stream before every launch.  Nothing at or past
// len[b] is read.
// --------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(PCM_THREADS) void absmax_rows_kernel(
    const T* __restrict__ x, long stride, const int* __restrict__ len,
    unsigned* __restrict__ peaks, long N) {
  constexpr int V = PcmVec<T>::V;
  __shared__ float red[PCM_THREADS / WAVE];
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const long n = min(max((long)len[b], 0L), N);
  const long t0 = (long)blockIdx.x * PCM_TILE;
  if (t0 >= n) return;  // uniform over the workgroup
  const int cnt = (int)(min(n, t0 + PCM_TILE) - t0);
  const T* p = x + (long)b * stride + t0;

  const int head = min(cnt, head_elems_(p));
  const int nvec = (cnt - head) / V;
  const int tail0 = head + nvec * V;
  float m = 0.f;
  if (tid < head) m = fabsf(ld_f<T>(p + tid));
  for (int v = tid; v < nvec; v += PCM_THREADS) {
    float e[V];
    PcmVec<T>::load(p + head + v * V, e);
#pragma unroll
    for (int j = 0; j < V; ++j) m = fmaxf(m, fabsf(e[j]));
  }
  if (tail0 + tid < cnt) m = fmaxf(m, fabsf(ld_f<T>(p + tail0 + tid)));

#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, WAVE));
  if ((tid & (WAVE - 1)) == 0) red[tid / WAVE] = m;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < PCM_THREADS / WAVE; ++w) m = fmaxf(m, red[w]);
    if (m > 0.f) atomicMax(peaks + b, __float_as_uint(m));
  }
}

// --------------------------------------------------------------------------
// pcm16_rows: grid (output tiles, B).  The split is made on the OUTPUT
// address (8 int16 per 16-byte store); a vector group loads its 8 inputs
// with 16-byte loads when the input address is aligned too and the group
// lies inside the row, else element by element.  peaks == nullptr selects
// the fixed scale 32767 (no peak normalisation).
// --------------------------------------------------------------------------
__device__ __forceinline__ short to_pcm_(float x, float scale) {
  const float v = x * scale;  // one f32 multiply
  return (short)(int)fminf(fmaxf(v, -32768.f), 32767.f);  // cvt truncates
}

template <typename T>
__global__ __launch_bounds__(PCM_THREADS) void pcm16_rows_kernel(
    const T* __restrict__ x, long stride, const int* __restrict__ len,
    const unsigned* __restrict__ peaks, short* __restrict__ y, long N,
    long N_out) {
  constexpr int V = PcmVec<T>::V;
  __shared__ float scale_s;
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const long n = min(min(max((long)len[b], 0L), N), N_out);
  const long o0 = (long)blockIdx.x * PCM_TILE;
  if (o0 >= N_out) return;  // uniform over the workgroup
  const int cnt = (int)(min(N_out, o0 + PCM_TILE) - o0);
  const T* xr = x + (long)b * stride;  // read at indices < n only
  short* yr = y + (long)b * N_out;

  if (tid == 0) {
    float s = 32767.f;
    if (peaks != nullptr) {
      const double pk = (double)__uint_as_float(peaks[b]);
      s = pk > 1e-8 ? (float)(32767.0 / pk) : 0.f;
    }
    scale_s = s;
  }
  __syncthreads();
  const float scale = scale_s;

  const int head = min(cnt, head_elems_(yr + o0));
  const int nvec = (cnt - head) / 8;
  const int tail0 = head + nvec * 8;
  if (tid < head) {
    const long i = o0 + tid;
    yr[i] = i < n ? to_pcm_(ld_f<T>(xr + i), scale) : (short)0;
  }
  const long body = o0 + head;
  const bool x_aligned =
      (reinterpret_cast<uintptr_t>(xr + body) & 15) == 0;  // row-uniform
  for (int v = tid; v < nvec; v += PCM_THREADS) {
    const long i = body + (long)v * 8;
    i16x8 out = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i + 8 <= n && x_aligned) {
      float e[8];
#pragma unroll
      for (int q = 0; q < 8 / V; ++q) PcmVec<T>::load(xr + i + q * V, e + q * V);
#pragma unroll
      for (int j = 0; j < 8; ++j) out[j] = to_pcm_(e[j], scale);
    } else if (i < n) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (i + j < n) out[j] = to_pcm_(ld_f<T>(xr + i + j), scale);
    }
    *reinterpret_cast<i16x8*>(yr + i) = out;
  }
  if (tail0 + tid < cnt) {
    const long i = o0 + tail0 + tid;
    yr[i] = i < n ? to_pcm_(ld_f<T>(xr + i), scale) : (short)0;
  }
}

// --------------------------------------------------------------------------
// g711_rows: grid (output tiles, B).  to_pcm_ of the row, then G.711
// companding in integer VALU: the device counterpart of
// sonata_amd/audio/g711.py encode (the Sun/CCITT g711.c forms), bit for bit.
// The law is per row (0 = mu-law, anything else = A-law; the caller checks
// the values on the host), so the branch is uniform over the workgroup.
// The split is made on the OUTPUT address: 16 codes per 16-byte store, at
// most one vector group per lane of a tile.  Columns at or past len[b] are
// written as the row's code of sample 0 (0xFF / 0xD5), not 0.
// --------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

// bit length of v > 0
__device__ __forceinline__ int bitlen_(int v) { return 32 - __clz(v); }

__device__ __forceinline__ unsigned ulaw_(int x) {
  const int s = x >> 2;                           // 14-bit magnitude domain
  const int m = min(abs(s) + 33, 0x1FFF);         // bias, clip: 33 .. 8191
  const int seg = bitlen_(m) - 6;                 // 0 .. 7
  return (unsigned)((seg << 4) | ((m >> (seg + 1)) & 0xF)) ^
         (s < 0 ? 0x7Fu : 0xFFu);
}

__device__ __forceinline__ unsigned alaw_(int x) {
  const int ix = (x < 0 ? ~x : x) >> 4;           // 0 .. 2047
  const int e = bitlen_(ix | 16) - 4;             // 1 .. 7 for ix >= 16
  int c = ix < 16 ? ix : ((ix >> (e - 1)) - 16) + (e << 4);
  if (x >= 0) c |= 0x80;
  return (unsigned)c ^ 0x55u;
}

__device__ __forceinline__ unsigned g711_(int x, bool alaw) {
  return alaw ? alaw_(x) : ulaw_(x);
}

template <typename T>
__global__ __launch_bounds__(PCM_THREADS) void g711_rows_kernel(
    const T* __restrict__ x, long stride, const int* __restrict__ len,
    const int* __restrict__ law, const unsigned* __restrict__ peaks,
    unsigned char* __restrict__ y, long N, long N_out) {
  constexpr int V = PcmVec<T>::V;
  __shared__ float scale_s;
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const long n = min(min(max((long)len[b], 0L), N), N_out);
  const long o0 = (long)blockIdx.x * PCM_TILE;
  if (o0 >= N_out) return;  // uniform over the workgroup
  const int cnt = (int)(min(N_out, o0 + PCM_TILE) - o0);
  const T* xr = x + (long)b * stride;  // read at indices < n only
  unsigned char* yr = y + (long)b * N_out;
  const bool alaw = law[b] != 0;                  // row-uniform
  const unsigned zero = alaw ? 0xD5u : 0xFFu;     // code of sample 0

  if (tid == 0) {
    float s = 32767.f;
    if (peaks != nullptr) {
      const double pk = (double)__uint_as_float(peaks[b]);
      s = pk > 1e-8 ? (float)(32767.0 / pk) : 0.f;
    }
    scale_s = s;
  }
  __syncthreads();
  const float scale = scale_s;

  const int head = min(cnt, head_elems_(yr + o0));
  const int nvec = (cnt - head) / 16;  // <= PCM_THREADS: one group per lane
  const int tail0 = head + nvec * 16;
  if (tid < head) {
    const long i = o0 + tid;
    yr[i] = (unsigned char)(
        i < n ? g711_(to_pcm_(ld_f<T>(xr + i), scale), alaw) : zero);
  }
  const long body = o0 + head;
  const bool x_aligned =
      (reinterpret_cast<uintptr_t>(xr + body) & 15) == 0;  // row-uniform
  if (tid < nvec) {
    const long i = body + (long)tid * 16;
    unsigned c[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) c[j] = zero;
    if (i + 16 <= n && x_aligned) {
      float e[16];
#pragma unroll
      for (int q = 0; q < 16 / V; ++q)
        PcmVec<T>::load(xr + i + q * V, e + q * V);
#pragma unroll
      for (int j = 0; j < 16; ++j) c[j] = g711_(to_pcm_(e[j], scale), alaw);
    } else if (i < n) {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (i + j < n) c[j] = g711_(to_pcm_(ld_f<T>(xr + i + j), scale), alaw);
    }
    u32x4 out;
#pragma unroll
    for (int w = 0; w < 4; ++w)  // byte j of the store is code j
      out[w] = c[4 * w] | (c[4 * w + 1] << 8) | (c[4 * w + 2] << 16) |
               (c[4 * w + 3] << 24);
    *reinterpret_cast<u32x4*>(yr + i) = out;
  }
  if (tail0 + tid < cnt) {
    const long i = o0 + tail0 + tid;
    yr[i] = (unsigned char)(
        i < n ? g711_(to_pcm_(ld_f<T>(xr + i), scale), alaw) : zero);
  }
}

// ------------------------------ host wrapper --------------------------------
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

long pcm_tile() { return PCM_TILE; }

// x [B, N] f32 or bf16 with unit stride along N (any row stride: a
// [B, 1, T][:, 0, :] view is taken as it is), len int32 [B].  Returns
// (y int16 [B, N_out], peaks f32 [B]); peaks stay 0 without peak_normalize.
std::vector<torch::Tensor> pcm16_rows(torch::Tensor x, torch::Tensor len,
                                      long N_out, bool peak_normalize) {
  TORCH_CHECK(x.dim() == 2 && x.is_cuda() &&
                  (x.scalar_type() == at::kFloat ||
                   x.scalar_type() == at::kBFloat16),
              "pcm16_rows: x must be a cuda f32 or bf16 [B, N] tensor");
  const long B = x.size(0), N = x.size(1);
  TORCH_CHECK(N <= 1 || x.stride(1) == 1,
              "pcm16_rows: rows must be contiguous");
  TORCH_CHECK(x.stride(0) >= 0, "pcm16_rows: negative row stride");
  TORCH_CHECK(len.is_cuda() && len.is_contiguous() &&
                  len.scalar_type() == at::kInt && len.dim() == 1 &&
                  len.size(0) == B,
              "pcm16_rows: len must be a cuda int32 [B] tensor");
  TORCH_CHECK(N < INT_MAX && N_out >= 0 && N_out < INT_MAX && B < 65536,
              "pcm16_rows: shape out of range");
  auto y = torch::empty({B, N_out}, x.options().dtype(at::kShort));
  auto peaks = torch::empty({B}, x.options().dtype(at::kFloat));
  if (B == 0) return {y, peaks};
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  unsigned* pk = reinterpret_cast<unsigned*>(peaks.data_ptr<float>());
  HIP_CHECK(hipMemsetAsync(pk, 0, B * sizeof(unsigned), stream));
  const long stride = x.stride(0);
  DISPATCH_FT_CONV(x, {
    const scalar_t* xp = reinterpret_cast<const scalar_t*>(x.data_ptr());
    if (peak_normalize && N > 0)
      hipLaunchKernelGGL(absmax_rows_kernel<scalar_t>,
                         dim3(ceil_div(N, PCM_TILE), B), dim3(PCM_THREADS), 0,
                         stream, xp, stride, len.data_ptr<int>(), pk, N);
    if (N_out > 0)
      hipLaunchKernelGGL(pcm16_rows_kernel<scalar_t>,
                         dim3(ceil_div(N_out, PCM_TILE), B),
                         dim3(PCM_THREADS), 0, stream, xp, stride,
                         len.data_ptr<int>(),
                         peak_normalize ? (const unsigned*)pk : nullptr,
                         y.data_ptr<short>(), N, N_out);
  });
  return {y, peaks};
}

// g711_rows: x and len as pcm16_rows takes them, law int32 [B] (0 = mu-law,
// 1 = A-law; values are checked on the host before upload, the kernel reads
// any other value as A-law).  Returns (y uint8 [B, N_out], peaks f32 [B]).
std::vector<torch::Tensor> g711_rows(torch::Tensor x, torch::Tensor len,
                                     torch::Tensor law, long N_out,
                                     bool peak_normalize) {
  TORCH_CHECK(x.dim() == 2 && x.is_cuda() &&
                  (x.scalar_type() == at::kFloat ||
                   x.scalar_type() == at::kBFloat16),
              "g711_rows: x must be a cuda f32 or bf16 [B, N] tensor");
  const long B = x.size(0), N = x.size(1);
  TORCH_CHECK(N <= 1 || x.stride(1) == 1,
              "g711_rows: rows must be contiguous");
  TORCH_CHECK(x.stride(0) >= 0, "g711_rows: negative row stride");
  TORCH_CHECK(len.is_cuda() && len.is_contiguous() &&
                  len.scalar_type() == at::kInt && len.dim() == 1 &&
                  len.size(0) == B && len.device() == x.device(),
              "g711_rows: len must be a cuda int32 [B] tensor");
  TORCH_CHECK(law.is_cuda() && law.is_contiguous() &&
                  law.scalar_type() == at::kInt && law.dim() == 1 &&
                  law.size(0) == B && law.device() == x.device(),
              "g711_rows: law must be a cuda int32 [B] tensor");
  TORCH_CHECK(N < INT_MAX && N_out >= 0 && N_out < INT_MAX && B < 65536,
              "g711_rows: shape out of range");
  auto y = torch::empty({B, N_out}, x.options().dtype(at::kByte));
  auto peaks = torch::empty({B}, x.options().dtype(at::kFloat));
  if (B == 0) return {y, peaks};
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  unsigned* pk = reinterpret_cast<unsigned*>(peaks.data_ptr<float>());
  HIP_CHECK(hipMemsetAsync(pk, 0, B * sizeof(unsigned), stream));
  const long stride = x.stride(0);
  DISPATCH_FT_CONV(x, {
    const scalar_t* xp = reinterpret_cast<const scalar_t*>(x.data_ptr());
    if (peak_normalize && N > 0)
      hipLaunchKernelGGL(absmax_rows_kernel<scalar_t>,
                         dim3(ceil_div(N, PCM_TILE), B), dim3(PCM_THREADS), 0,
                         stream, xp, stride, len.data_ptr<int>(), pk, N);
    if (N_out > 0)
      hipLaunchKernelGGL(g711_rows_kernel<scalar_t>,
                         dim3(ceil_div(N_out, PCM_TILE), B),
                         dim3(PCM_THREADS), 0, stream, xp, stride,
                         len.data_ptr<int>(), law.data_ptr<int>(),
                         peak_normalize ? (const unsigned*)pk : nullptr,
                         y.data_ptr<uint8_t>(), N, N_out);
  });
  return {y, peaks};
}
