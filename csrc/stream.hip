// Batched realtime streams: the two data-movement kernels around one shared
// chunk decode (VitsVoice.stream_round).
//
//   gather_windows    packs R ragged latent windows, taken from separately
//                     allocated encoder outputs, into the [R, C, l_max]
//                     batch the decoder takes; columns past a row's length
//                     are written as 0.
//   stream_seam_rows  device form of the single-stream trim_and_emit, for R
//                     decoded rows at once: trim the padding, crossfade the
//                     first 42 samples with the tail the stream kept from its
//                     previous chunk, keep the next tail.
//
// Both are bit-exact: copies, the exact bf16 -> f32 widening, and for a seam
// sample two rounded f32 products and one rounded add (no FMA contraction),
// which is what audio.samples.crossfade computes in NumPy.
//
// Every index is validated on the host before a launch (the bindings below
// take the per-row parameters as host integers), and the kernels read only
// what those checks cover: a source row at [0, length), a decoded row at
// [lo, hi + ext).  Nothing is assumed about alignment: spans are split by
// ADDRESS into a scalar head, a 16-byte body and a scalar tail, as in
// pcm.hip, and a body group is loaded as a vector only when its source
// address is aligned as well and the whole group lies inside the row.
#include "common.h"

#include <climits>
#include <cstdint>

#define STREAM_THREADS 256
// output samples per workgroup of the seam kernel: 256 threads x 16
#define SEAM_TILE 4096
// samples of one kept tail (CROSSFADE_SAMPLES in models/voice.py)
#define SEAM_XF 42

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(4))) unsigned short u16x4;

// --------------------------------------------------------------------------
// gather_windows: grid (ceil(C / 4), R), one wave per (row, channel) line of
// l_max elements.  E is the raw element (4 bytes for f32, 2 for bf16); VE
// elements make one 16-byte store.  tab[r] = {address of
// zs[src][row, 0, start], channel stride in elements, length}.
// --------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(STREAM_THREADS) void gather_windows_kernel(
    const long* __restrict__ tab, E* __restrict__ out, int C, long l_max) {
  constexpr int VE = 16 / sizeof(E);
  const int r = blockIdx.y;
  const int c = blockIdx.x * (STREAM_THREADS / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (c >= C) return;  // uniform over the wave
  const E* s = reinterpret_cast<const E*>(tab[r * 3 + 0]) +
               (long)c * tab[r * 3 + 1];
  const long n = min(max(tab[r * 3 + 2], 0L), l_max);  // read s[i], i < n only
  E* o = out + ((long)r * C + c) * l_max;

  const long mis = (long)((reinterpret_cast<uintptr_t>(o) / sizeof(E)) % VE);
  const long head = min(l_max, (VE - mis) % VE);
  const long nvec = (l_max - head) / VE;
  const long tail0 = head + nvec * VE;
  if (lane < head) o[lane] = lane < n ? s[lane] : (E)0;
  const bool s_aligned =
      (reinterpret_cast<uintptr_t>(s + head) & 15) == 0;  // line-uniform
  for (long v = lane; v < nvec; v += WAVE) {
    const long i = head + v * VE;
    u32x4 w = {0u, 0u, 0u, 0u};
    if (i + VE <= n && s_aligned) {
      w = *reinterpret_cast<const u32x4*>(s + i);
    } else if (i < n) {
      E e[VE];
#pragma unroll
      for (int j = 0; j < VE; ++j) e[j] = i + j < n ? s[i + j] : (E)0;
      if constexpr (sizeof(E) == 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = e[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          w[j] = (unsigned)e[2 * j] | ((unsigned)e[2 * j + 1] << 16);
      }
    }
    *reinterpret_cast<u32x4*>(o + i) = w;
  }
  if (tail0 + lane < l_max) {
    const long i = tail0 + lane;
    o[i] = i < n ? s[i] : (E)0;
  }
}

// --------------------------------------------------------------------------
// stream_seam_rows: grid (ceil(n_out / SEAM_TILE), R).  par[r] = {lo, hi,
// ext, prev_ext, slot}.  out[r, i] for i < hi - lo is wav[r, lo + i] widened,
// mixed with the old tail for i < prev_ext; 0 from there to n_out.  The old
// tail of a row is read only by the row's first workgroup (SEAM_XF <
// SEAM_TILE), which writes the new one after a barrier: tails_in and
// tails_out may be the same buffer.  Rows name distinct slots.
// --------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ float seam_elem_(const T* w, long i, int prev_ext,
                                            const float* tail,
                                            const float* __restrict__ ramp) {
  const float cur = ld_f<T>(w + i);
  if (i >= prev_ext) return cur;
  // tail[i] * ramp[n-1-i] + cur * ramp[i], each operation rounded to f32
  return __fadd_rn(__fmul_rn(tail[i], ramp[prev_ext - 1 - i]),
                   __fmul_rn(cur, ramp[i]));
}

template <typename T>
__global__ __launch_bounds__(STREAM_THREADS) void stream_seam_rows_kernel(
    const T* __restrict__ wav, long stride, const int* __restrict__ par,
    const float* tails_in, float* tails_out, const float* __restrict__ ramp,
    float* __restrict__ out, long n_out) {
  const int r = blockIdx.y;
  const int tid = threadIdx.x;
  const int lo = par[r * 5 + 0], hi = par[r * 5 + 1], ext = par[r * 5 + 2];
  const int prev_ext = par[r * 5 + 3], slot = par[r * 5 + 4];
  const long n = min((long)(hi - lo), n_out);  // samples this row emits
  const long o0 = (long)blockIdx.x * SEAM_TILE;
  const int cnt = (int)(min(n_out, o0 + SEAM_TILE) - o0);
  const T* w = wav + (long)r * stride + lo;  // read at [0, n + ext) only
  const float* tail = tails_in + (long)slot * SEAM_XF;
  float* o = out + (long)r * n_out;

  const int mis = (int)((reinterpret_cast<uintptr_t>(o + o0) / 4) % 4);
  const int head = min(cnt, (4 - mis) % 4);
  const int nvec = (cnt - head) / 4;
  const int tail0 = head + nvec * 4;
  if (tid < head) {
    const long i = o0 + tid;
    o[i] = i < n ? seam_elem_<T>(w, i, prev_ext, tail, ramp) : 0.f;
  }
  const long body = o0 + head;
  const bool w_aligned = (reinterpret_cast<uintptr_t>(w + body) &
                          (4 * sizeof(T) - 1)) == 0;  // row-uniform
  for (int v = tid; v < nvec; v += STREAM_THREADS) {
    const long i = body + (long)v * 4;
    f32x4 y = {0.f, 0.f, 0.f, 0.f};
    if (i >= prev_ext && i + 4 <= n && w_aligned) {
      if constexpr (sizeof(T) == 4) {
        y = *reinterpret_cast<const f32x4*>(w + i);
      } else {
        const u16x4 b = *reinterpret_cast<const u16x4*>(w + i);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          y[j] = __uint_as_float((unsigned)b[j] << 16);
      }
    } else if (i < n) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i + j < n) y[j] = seam_elem_<T>(w, i + j, prev_ext, tail, ramp);
    }
    *reinterpret_cast<f32x4*>(o + i) = y;
  }
  if (tail0 + tid < cnt) {
    const long i = o0 + tail0 + tid;
    o[i] = i < n ? seam_elem_<T>(w, i, prev_ext, tail, ramp) : 0.f;
  }

  if (blockIdx.x != 0) return;  // uniform over the workgroup
  __syncthreads();              // every read of the old tail is done
  if (tid < ext)
    tails_out[(long)slot * SEAM_XF + tid] = ld_f<T>(w + (hi - lo) + tid);
}

// ------------------------------ host wrappers -------------------------------
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

long seam_crossfade_samples() { return SEAM_XF; }

// zs: cuda tensors [b_i, C, F_i], one dtype (f32 or bf16) and one C, unit
// stride along F.  Row r of the result is zs[src[r]][row[r], :, start[r] :
// start[r] + length[r]] and then zeros up to l_max.  One launch.
torch::Tensor gather_windows(std::vector<torch::Tensor> zs,
                             std::vector<int64_t> src,
                             std::vector<int64_t> row,
                             std::vector<int64_t> start,
                             std::vector<int64_t> length, long l_max) {
  TORCH_CHECK(!zs.empty(), "gather_windows: no source tensors");
  const long R = (long)src.size();
  TORCH_CHECK((long)row.size() == R && (long)start.size() == R &&
                  (long)length.size() == R,
              "gather_windows: one (src, row, start, length) per output row");
  const auto& z0 = zs[0];
  TORCH_CHECK(z0.dim() == 3 && z0.is_cuda() &&
                  (z0.scalar_type() == at::kFloat ||
                   z0.scalar_type() == at::kBFloat16),
              "gather_windows: sources must be cuda f32 or bf16 [b, C, F]");
  const long C = z0.size(1);
  const long esz = (long)z0.element_size();
  for (const auto& z : zs) {
    TORCH_CHECK(z.dim() == 3 && z.is_cuda() && z.device() == z0.device() &&
                    z.scalar_type() == z0.scalar_type() && z.size(1) == C,
                "gather_windows: sources differ in device, dtype or C");
    TORCH_CHECK(z.size(2) <= 1 || z.stride(2) == 1,
                "gather_windows: frames must have unit stride");
    TORCH_CHECK(z.stride(0) >= 0 && z.stride(1) >= 0,
                "gather_windows: negative stride");
  }
  TORCH_CHECK(l_max >= 0 && l_max < INT_MAX && R < 65536 && C < INT_MAX,
              "gather_windows: shape out of range");
  auto out = torch::empty({R, C, l_max}, z0.options());
  if (R == 0 || C == 0 || l_max == 0) return out;

  auto tab = torch::empty({R, 3}, torch::TensorOptions().dtype(at::kLong));
  long* t = tab.data_ptr<long>();
  for (long r = 0; r < R; ++r) {
    TORCH_CHECK(src[r] >= 0 && src[r] < (long)zs.size(),
                "gather_windows: src out of range");
    const auto& z = zs[src[r]];
    TORCH_CHECK(row[r] >= 0 && row[r] < z.size(0),
                "gather_windows: row out of range");
    TORCH_CHECK(start[r] >= 0 && length[r] >= 0 && length[r] <= l_max &&
                    start[r] + length[r] <= z.size(2),
                "gather_windows: window outside its source row");
    const char* base = reinterpret_cast<const char*>(z.data_ptr());
    t[r * 3 + 0] = (long)reinterpret_cast<uintptr_t>(
        base + (row[r] * z.stride(0) + start[r]) * esz);
    t[r * 3 + 1] = z.stride(1);
    t[r * 3 + 2] = length[r];
  }
  auto tab_d = tab.to(z0.device());
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const dim3 grid(ceil_div(C, STREAM_THREADS / WAVE), R);
  if (esz == 4)
    hipLaunchKernelGGL(gather_windows_kernel<unsigned int>, grid,
                       dim3(STREAM_THREADS), 0, stream,
                       tab_d.data_ptr<long>(),
                       reinterpret_cast<unsigned int*>(out.data_ptr()), (int)C,
                       l_max);
  else
    hipLaunchKernelGGL(gather_windows_kernel<unsigned short>, grid,
                       dim3(STREAM_THREADS), 0, stream,
                       tab_d.data_ptr<long>(),
                       reinterpret_cast<unsigned short*>(out.data_ptr()),
                       (int)C, l_max);
  return out;
}

// wav [R, 1, N] or [R, N] f32 / bf16 with unit stride along N; tails_in and
// tails_out f32 [S, SEAM_XF] (the same tensor is allowed), ramp f32
// [SEAM_XF].  Writes tails_out in place at the named slots and returns
// out f32 [R, n_out].
torch::Tensor stream_seam_rows(torch::Tensor wav, std::vector<int64_t> lo,
                               std::vector<int64_t> hi,
                               std::vector<int64_t> ext,
                               std::vector<int64_t> prev_ext,
                               std::vector<int64_t> slot,
                               torch::Tensor tails_in,
                               torch::Tensor tails_out, torch::Tensor ramp,
                               long n_out) {
  if (wav.dim() == 3) {
    TORCH_CHECK(wav.size(1) == 1, "stream_seam_rows: wav must be [R, 1, N]");
    wav = wav.select(1, 0);
  }
  TORCH_CHECK(wav.dim() == 2 && wav.is_cuda() &&
                  (wav.scalar_type() == at::kFloat ||
                   wav.scalar_type() == at::kBFloat16),
              "stream_seam_rows: wav must be a cuda f32 or bf16 tensor");
  const long R = wav.size(0), N = wav.size(1);
  TORCH_CHECK(N <= 1 || wav.stride(1) == 1,
              "stream_seam_rows: rows must be contiguous");
  TORCH_CHECK(wav.stride(0) >= 0, "stream_seam_rows: negative row stride");
  TORCH_CHECK((long)lo.size() == R && (long)hi.size() == R &&
                  (long)ext.size() == R && (long)prev_ext.size() == R &&
                  (long)slot.size() == R,
              "stream_seam_rows: one parameter of each kind per row");
  auto f32_on = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.device() == wav.device() && t.is_contiguous() &&
           t.scalar_type() == at::kFloat;
  };
  TORCH_CHECK(f32_on(tails_in) && tails_in.dim() == 2 &&
                  tails_in.size(1) == SEAM_XF && f32_on(tails_out) &&
                  tails_out.sizes() == tails_in.sizes(),
              "stream_seam_rows: tails must be cuda f32 [S, 42]");
  TORCH_CHECK(f32_on(ramp) && ramp.dim() == 1 && ramp.size(0) == SEAM_XF,
              "stream_seam_rows: ramp must be cuda f32 [42]");
  const long S = tails_in.size(0);
  TORCH_CHECK(N < INT_MAX && n_out >= 0 && n_out < INT_MAX && n_out % 4 == 0 &&
                  R < 65536,
              "stream_seam_rows: shape out of range");
  auto out = torch::empty({R, n_out}, wav.options().dtype(at::kFloat));
  if (R == 0) return out;

  auto par = torch::empty({R, 5}, torch::TensorOptions().dtype(at::kInt));
  int* p = par.data_ptr<int>();
  std::vector<char> named(S, 0);
  for (long r = 0; r < R; ++r) {
    TORCH_CHECK(prev_ext[r] == 0 || prev_ext[r] == SEAM_XF,
                "stream_seam_rows: prev_ext must be 0 or 42");
    TORCH_CHECK(ext[r] == 0 || ext[r] == SEAM_XF,
                "stream_seam_rows: ext must be 0 or 42");
    TORCH_CHECK(lo[r] >= 0 && hi[r] >= lo[r] && hi[r] + ext[r] <= N,
                "stream_seam_rows: [lo, hi + ext) outside the row");
    TORCH_CHECK(hi[r] - lo[r] >= prev_ext[r],
                "stream_seam_rows: chunk shorter than its seam");
    TORCH_CHECK(hi[r] - lo[r] <= n_out,
                "stream_seam_rows: n_out shorter than a row");
    TORCH_CHECK(slot[r] >= 0 && slot[r] < S && !named[slot[r]],
                "stream_seam_rows: slot out of range or named twice");
    named[slot[r]] = 1;
    p[r * 5 + 0] = (int)lo[r];
    p[r * 5 + 1] = (int)hi[r];
    p[r * 5 + 2] = (int)ext[r];
    p[r * 5 + 3] = (int)prev_ext[r];
    p[r * 5 + 4] = (int)slot[r];
  }
  auto par_d = par.to(wav.device());
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const dim3 grid(std::max(ceil_div(n_out, SEAM_TILE), 1), R);
  const long stride = wav.stride(0);
  DISPATCH_FT_CONV(wav, {
    hipLaunchKernelGGL(stream_seam_rows_kernel<scalar_t>, grid,
                       dim3(STREAM_THREADS), 0, stream,
                       reinterpret_cast<const scalar_t*>(wav.data_ptr()),
                       stride, par_d.data_ptr<int>(),
                       tails_in.data_ptr<float>(), tails_out.data_ptr<float>(),
                       ramp.data_ptr<float>(), out.data_ptr<float>(), n_out);
  });
  return out;
}
