// Batched on-device prosody: rate / pitch / volume on [B, N] f32 rows.
//
// Device counterparts of sonata_amd/audio/prosody.py (the CPU path and the
// semantic reference).  Every length (frame, half, search, n_frames, n_out,
// resample output length) is computed on the host by audio.prosody.wsola_plan
// / resample_out_len and passed in; the kernels never re-derive one.
//
//   - resample_linear_rows: linear interpolation, positions in double.
//   - wsola_rows:           WSOLA time stretch, one workgroup per row.
//   - scale_rows:           volume-only rows (no WSOLA launch).
#include "common.h"

#include <climits>

#define PROSODY_THREADS 256

// --------------------------------------------------------------------------
// resample_linear_rows: y[b, i] = x[b, i0]*(1-frac) + x[b, i1]*frac with
// pos = i*(len-1)/max(n_out-1, 1) evaluated in double (multiply, then
// divide: the order numpy uses), frac = (float)(pos - i0).  A row whose
// out_len equals its in_len is a copy (pos == i exactly).  Columns past
// out_len[b] are written as 0.
// --------------------------------------------------------------------------
__global__ void resample_linear_rows_kernel(const float* __restrict__ x,
                                            const int* __restrict__ in_len,
                                            const int* __restrict__ out_len,
                                            float* __restrict__ y, long N,
                                            long N_out) {
  const int b = blockIdx.y;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N_out) return;
  const int len = min(in_len[b], (int)N);
  const int n_out = out_len[b];
  float v = 0.f;
  if (i < n_out && len > 0) {
    const float* xr = x + (long)b * N;
    if (n_out == len) {
      v = xr[i];
    } else {
      const double pos =
          (double)i * (double)(len - 1) / (double)max(n_out - 1, 1);
      long i0 = (long)floor(pos);
      i0 = min(max(i0, 0L), (long)len - 1);
      const long i1 = min(i0 + 1, (long)len - 1);
      const float frac = (float)(pos - (double)i0);
      // f32 frac as the op defines it; the blend itself rounds once
      v = (float)((double)xr[i0] * (1.0 - (double)frac) +
                  (double)xr[i1] * (double)frac);
    }
  }
  y[(long)b * N_out + i] = v;
}

// --------------------------------------------------------------------------
// scale_rows: y[b, i] = x[b, i] * gain[b] for i < len[b], 0 past it.
// --------------------------------------------------------------------------
__global__ void scale_rows_kernel(const float* __restrict__ x,
                                  const int* __restrict__ len,
                                  const float* __restrict__ gain,
                                  float* __restrict__ y, long N) {
  const int b = blockIdx.y;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const long o = (long)b * N + i;
  y[o] = i < len[b] ? x[o] * gain[b] : 0.f;
}

// --------------------------------------------------------------------------
// wsola_rows: one 256-thread workgroup per row; frames are sequential (the
// search of frame k correlates against the tail chosen by frame k-1), the
// parallelism is across rows and across the candidates of one frame.
//
// Per frame k (analysis position t = (int)(k*ana_hop), in double):
//   k > 0:  lo = max(t-search, 0), hi = min(t+search, len-frame); when
//           hi > lo, x[lo : hi+frame] is staged in LDS once and serves the
//           search, the overlap-add and the next tail.  Candidate c scores
//           sum_j x[lo+c+j]*tail[j], j ascending, f32: one fixed order for
//           every candidate.  Block argmax: per-thread over its strided
//           candidates, wave-64 shuffle, then LDS across the 4 waves; on
//           equal score the LOWEST index wins (np.argmax), so silence
//           selects lo.
//   else:   target = t.
//   target is clamped to [0, len-frame].
// Hops are half a frame, so output sample k*half+j gets at most two
// contributions and is finalised as it is produced:
//   (prev*w[half+j] + cur*w[j]) / (w[half+j] + w[j])   (norm > 1e-6 only)
// times gain[b] (ola_ below).  No atomics, no zero-fill pass, no second kernel.
//
// A row with n_frames[b] == 0 is a pass-through row: copied and scaled.
// targets[b, k] records every frame's choice; unused slots are -1.
// LDS (dynamic only): seg[seg_cap] | tail[half] | red_s[4] | red_i[4].
// --------------------------------------------------------------------------
__device__ __forceinline__ bool better_(float s, int i, float so, int io) {
  return so > s || (so == s && io < i);
}

// One finished output sample: (a*wa + b*wb) / (wa + wb) * g.  The host
// accumulates in f32 and divides where its f32 norm exceeds 1e-6; the same
// test is made here on the same f32 sum, the arithmetic itself runs in
// double and rounds once (a handful of f64 ops per OUTPUT sample, nothing
// next to the search), so the result sits within one f32 rounding of the
// exact value whatever the gain.
__device__ __forceinline__ float ola_(float a, float wa, float b, float wb,
                                      float g) {
  double v = (double)a * (double)wa + (double)b * (double)wb;
  if (wa + wb > 1e-6f) v /= (double)wa + (double)wb;
  return (float)(v * (double)g);
}

__global__ __launch_bounds__(PROSODY_THREADS) void wsola_rows_kernel(
    const float* __restrict__ x, const int* __restrict__ in_len,
    const double* __restrict__ ana_hop, const int* __restrict__ n_frames,
    const int* __restrict__ out_len, const float* __restrict__ window,
    const float* __restrict__ gain, float* __restrict__ y,
    int* __restrict__ targets, long N, long N_out, int K_max, int half,
    int search, int seg_cap) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* seg = reinterpret_cast<float*>(smem_raw);
  float* tail = seg + seg_cap;            // seg_cap is a multiple of 4
  float* red_s = tail + ((half + 3) & ~3);
  int* red_i = reinterpret_cast<int*>(red_s + 4);

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int frame = 2 * half;
  const int len = max(min(in_len[b], (int)N), 0);
  const int K = min(n_frames[b], K_max);
  const int n_out = max(min(out_len[b], (int)N_out), 0);
  const float g = gain[b];
  const double hop = ana_hop[b];
  const float* xr = x + (long)b * N;
  float* yr = y + (long)b * N_out;
  int* tr = targets + (long)b * K_max;

  for (int k = K + tid; k < K_max; k += PROSODY_THREADS) tr[k] = -1;
  for (long i = n_out + tid; i < N_out; i += PROSODY_THREADS) yr[i] = 0.f;

  if (K <= 0 || len < frame) {  // pass-through row: copy and scale
    const int n = min(n_out, len);
    for (int i = tid; i < n; i += PROSODY_THREADS) yr[i] = xr[i] * g;
    for (int i = n + tid; i < n_out; i += PROSODY_THREADS) yr[i] = 0.f;
    return;
  }

  for (int k = 0; k < K; ++k) {
    int t = (int)((double)k * hop);
    int base, n_cand = 0;
    if (k > 0) {
      const int lo = max(t - search, 0);
      const int hi = min(t + search, len - frame);
      if (hi > lo) n_cand = hi - lo;
      base = lo;
    }
    if (n_cand == 0) {
      t = min(max(t, 0), len - frame);
      base = t;
    }
    // stage x[base : base + n_cand + frame] (n_cand + frame <= seg_cap,
    // base + n_cand + frame <= len by the clamps above)
    const int n_seg = min(n_cand + frame, seg_cap);
    for (int i = tid; i < n_seg; i += PROSODY_THREADS) seg[i] = xr[base + i];
    __syncthreads();

    int off = 0;
    if (n_cand > 0) {
      float best = -INFINITY;
      int best_i = INT_MAX;
      // Two candidates per thread per sweep (2*search = 440 at 22.05 kHz
      // is one sweep): they share the tail reads and give two independent
      // FMA chains; the unroll keeps a batch of LDS reads in flight (one
      // wave per SIMD has nothing else to hide their latency behind).
      // Each candidate still sums j = 0..half-1 in order.
      for (int c0 = tid; c0 < n_cand; c0 += 2 * PROSODY_THREADS) {
        const int c1 = c0 + PROSODY_THREADS;
        const bool has1 = c1 < n_cand;
        const float* s0 = seg + c0;
        const float* s1 = seg + (has1 ? c1 : c0);
        float a0 = 0.f, a1 = 0.f;
#pragma unroll 8
        for (int j = 0; j < half; ++j) {
          const float tj = tail[j];
          a0 += s0[j] * tj;
          a1 += s1[j] * tj;
        }
        if (a0 > best) {  // candidates ascend: first maximum kept
          best = a0;
          best_i = c0;
        }
        if (has1 && a1 > best) {
          best = a1;
          best_i = c1;
        }
      }
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) {
        const float so = __shfl_xor(best, d, 64);
        const int io = __shfl_xor(best_i, d, 64);
        if (better_(best, best_i, so, io)) {
          best = so;
          best_i = io;
        }
      }
      if (lane == 0) {
        red_s[wid] = best;
        red_i[wid] = best_i;
      }
      __syncthreads();
      best = red_s[0];
      best_i = red_i[0];
#pragma unroll
      for (int w = 1; w < PROSODY_THREADS / 64; ++w) {
        if (better_(best, best_i, red_s[w], red_i[w])) {
          best = red_s[w];
          best_i = red_i[w];
        }
      }
      // no finite score (NaN input): fall back to the first candidate
      off = (best_i >= 0 && best_i < n_cand) ? best_i : 0;
    }
    if (tid == 0) tr[k] = base + off;

    // overlap-add segment k: out[k*half + j], then the new tail
    const float* cur = seg + off;
    const long o0 = (long)k * half;
    for (int j = tid; j < half; j += PROSODY_THREADS) {
      const float w1 = window[j];
      const float w2 = k > 0 ? window[half + j] : 0.f;
      const float prev = k > 0 ? tail[j] : 0.f;
      if (o0 + j < n_out) yr[o0 + j] = ola_(prev, w2, cur[j], w1, g);
      tail[j] = cur[half + j];
    }
    __syncthreads();  // tail complete, seg free for the next frame
  }
  // last half frame: only frame K-1 contributes
  const long o0 = (long)K * half;
  for (int j = tid; j < half; j += PROSODY_THREADS) {
    if (o0 + j < n_out)
      yr[o0 + j] = ola_(tail[j], window[half + j], 0.f, 0.f, g);
  }
  // n_out never exceeds (K+1)*half on a planned row; zero anything past it
  for (long i = o0 + half + tid; i < n_out; i += PROSODY_THREADS) yr[i] = 0.f;
}

// ------------------------------ host wrappers -------------------------------
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

static inline hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

static void check_rows(const torch::Tensor& x, const char* name) {
  TORCH_CHECK(x.dim() == 2 && x.is_cuda() && x.is_contiguous() &&
                  x.scalar_type() == at::kFloat,
              name, ": x must be a contiguous cuda f32 [B, N] tensor");
  TORCH_CHECK(x.size(1) < INT_MAX, name, ": row too long");
}

static void check_vec(const torch::Tensor& v, at::ScalarType ty, long B,
                      const char* name) {
  TORCH_CHECK(v.is_cuda() && v.is_contiguous() && v.scalar_type() == ty &&
                  v.dim() == 1 && v.size(0) == B,
              name, ": bad per-row vector");
}

torch::Tensor resample_linear_rows(torch::Tensor x, torch::Tensor in_len,
                                   torch::Tensor out_len, long N_out_max) {
  check_rows(x, "resample_linear_rows");
  const long B = x.size(0), N = x.size(1);
  check_vec(in_len, at::kInt, B, "resample_linear_rows");
  check_vec(out_len, at::kInt, B, "resample_linear_rows");
  TORCH_CHECK(N_out_max >= 0 && N_out_max < INT_MAX && B < 65536);
  auto y = torch::empty({B, N_out_max}, x.options());
  if (B == 0 || N_out_max == 0) return y;
  hipLaunchKernelGGL(resample_linear_rows_kernel,
                     dim3(ceil_div(N_out_max, PROSODY_THREADS), B),
                     dim3(PROSODY_THREADS), 0, cur_stream(),
                     x.data_ptr<float>(), in_len.data_ptr<int>(),
                     out_len.data_ptr<int>(), y.data_ptr<float>(), N,
                     N_out_max);
  return y;
}

torch::Tensor scale_rows(torch::Tensor x, torch::Tensor len,
                         torch::Tensor gain) {
  check_rows(x, "scale_rows");
  const long B = x.size(0), N = x.size(1);
  check_vec(len, at::kInt, B, "scale_rows");
  check_vec(gain, at::kFloat, B, "scale_rows");
  TORCH_CHECK(B < 65536);
  auto y = torch::empty_like(x);
  if (B == 0 || N == 0) return y;
  hipLaunchKernelGGL(scale_rows_kernel,
                     dim3(ceil_div(N, PROSODY_THREADS), B),
                     dim3(PROSODY_THREADS), 0, cur_stream(),
                     x.data_ptr<float>(), len.data_ptr<int>(),
                     gain.data_ptr<float>(), y.data_ptr<float>(), N);
  return y;
}

std::vector<torch::Tensor> wsola_rows(torch::Tensor x, torch::Tensor in_len,
                                      torch::Tensor ana_hop,
                                      torch::Tensor n_frames,
                                      torch::Tensor out_len,
                                      torch::Tensor window, long half,
                                      long search, torch::Tensor gain,
                                      long N_out_max, long K_max) {
  check_rows(x, "wsola_rows");
  const long B = x.size(0), N = x.size(1);
  check_vec(in_len, at::kInt, B, "wsola_rows");
  check_vec(ana_hop, at::kDouble, B, "wsola_rows");
  check_vec(n_frames, at::kInt, B, "wsola_rows");
  check_vec(out_len, at::kInt, B, "wsola_rows");
  check_vec(gain, at::kFloat, B, "wsola_rows");
  TORCH_CHECK(half >= 1 && search >= 1 && half < (1 << 24) &&
                  search < (1 << 24),
              "wsola_rows: bad frame geometry");
  check_vec(window, at::kFloat, 2 * half, "wsola_rows");
  TORCH_CHECK(N_out_max >= 0 && N_out_max < INT_MAX && K_max >= 1 &&
              K_max < INT_MAX);
  const long seg_cap = (2 * search + 2 * half + 3) & ~3L;
  const long lds =
      (seg_cap + ((half + 3) & ~3L)) * sizeof(float) + 4 * 8;
  TORCH_CHECK(lds <= 64 * 1024, "wsola_rows: frame ", 2 * half, " + search ",
              search, " needs ", lds,
              " bytes of LDS, over the 64 KiB a workgroup may use");
  auto y = torch::empty({B, N_out_max}, x.options());
  auto targets = torch::empty({B, K_max}, x.options().dtype(at::kInt));
  if (B == 0) return {y, targets};
  hipLaunchKernelGGL(wsola_rows_kernel, dim3(B), dim3(PROSODY_THREADS),
                     (size_t)lds, cur_stream(), x.data_ptr<float>(),
                     in_len.data_ptr<int>(), ana_hop.data_ptr<double>(),
                     n_frames.data_ptr<int>(), out_len.data_ptr<int>(),
                     window.data_ptr<float>(), gain.data_ptr<float>(),
                     y.data_ptr<float>(), targets.data_ptr<int>(), N,
                     N_out_max, (int)K_max, (int)half, (int)search,
                     (int)seg_cap);
  return {y, targets};
}
