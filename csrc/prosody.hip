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

// ==========================================================================
// Streaming prosody: the same stages fed chunk by chunk, state on the device
// (audio.prosody.WsolaStreamPlan / ResampleStreamPlan hold the rules and the
// arithmetic; every number below comes from them).
//
// A row's logical input this round is carry[slot] ++ chunk row, addressed by
// GLOBAL position p of the stage's input: p < a0 lies in the carry (which
// starts at in_pos), p >= a0 in the chunk.  The old carry and tail are copied
// to LDS before anything is written, so the state buffers are updated in
// place; rows name distinct slots and one workgroup owns a row.
//
// Per-row parameters travel as one row of longs (one host-to-device copy per
// launch); doubles ride as their bit patterns.  The host wrapper validates
// every read and write the parameters imply before it launches.
// ==========================================================================
#include <cmath>
#include <cstring>

#define WS_SLOT 0
#define WS_M 1        // valid samples of the chunk row
#define WS_A0 2       // input received before this round
#define WS_IN_POS 3   // global position of carry[0] (== a0 when carry_len == 0)
#define WS_CARRY 4    // carry_len
#define WS_K0 5       // first frame
#define WS_NK 6       // frames this round
#define WS_N 7        // total input length of the stage
#define WS_E0 8       // output emitted before this round
#define WS_E1 9       // output emitted after it
#define WS_FLAGS 10   // 1: pass-through row, 2: closing half frame + zeros
#define WS_KEEP_POS 11
#define WS_KEEP 12    // keep_len
#define WS_HOP 13     // ana_hop, double bits
#define WS_GAIN 14    // gain, double bits
#define WS_PAR 16

#define RS_SLOT 0
#define RS_M 1
#define RS_A0 2
#define RS_IN_POS 3
#define RS_CARRY 4
#define RS_N 5        // total input length
#define RS_NOUT 6     // total output length
#define RS_E0 7
#define RS_E1 8
#define RS_FLAGS 9    // 1: copy row
#define RS_KEEP_POS 10
#define RS_KEEP 11
#define RS_PAR 12
#define RS_CARRY_CAP 1  // audio.prosody.RESAMPLE_CARRY

// --------------------------------------------------------------------------
// wsola_stream_rows: frames [k0, k0 + nk) of wsola_rows_kernel on the logical
// input: the same lo / hi / clamp with the GLOBAL n, the same staging,
// scoring order, argmax and ola_.  Output sample o of the stream lands in
// y[b, o - e0] for e0 <= o < e1; columns past e1 - e0 are 0.  targets[b, i]
// is the global start of frame k0 + i, -1 in unused slots.
// LDS: seg[seg_cap] | car[seg_cap] | tail[half] | red_s[4] | red_i[4].
// --------------------------------------------------------------------------
__global__ __launch_bounds__(PROSODY_THREADS) void wsola_stream_rows_kernel(
    const float* __restrict__ x, const long* __restrict__ par,
    float* carry, float* tails, const float* __restrict__ window,
    float* __restrict__ y, int* __restrict__ targets, long N, long N_out,
    int K_max, int half, int search, int seg_cap) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* seg = reinterpret_cast<float*>(smem_raw);
  float* car = seg + seg_cap;             // seg_cap is a multiple of 4
  float* tail = car + seg_cap;
  float* red_s = tail + ((half + 3) & ~3);
  int* red_i = reinterpret_cast<int*>(red_s + 4);

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int frame = 2 * half;
  const long* p = par + (long)b * WS_PAR;
  const int slot = (int)p[WS_SLOT];
  const int m = (int)p[WS_M];
  const int a0 = (int)p[WS_A0];
  const int in_pos = (int)p[WS_IN_POS];
  const int carry_len = (int)p[WS_CARRY];
  const int k0 = (int)p[WS_K0];
  const int flags = (int)p[WS_FLAGS];
  const int nk = (flags & 1) ? 0 : (int)p[WS_NK];
  const int len = (int)p[WS_N];
  const long e0 = p[WS_E0], e1 = p[WS_E1];
  const int keep_pos = (int)p[WS_KEEP_POS];
  const int keep_len = (int)p[WS_KEEP];
  const double hop = __longlong_as_double(p[WS_HOP]);
  const float g = (float)__longlong_as_double(p[WS_GAIN]);
  const float* xr = x + (long)b * N;
  float* yr = y + (long)b * N_out;
  int* tr = targets + (long)b * K_max;
  float* cr = carry + (long)slot * seg_cap;
  float* tl = tails + (long)slot * half;
  const long n_emit = min(e1 - e0, N_out);

  for (int k = nk + tid; k < K_max; k += PROSODY_THREADS) tr[k] = -1;
  for (long i = n_emit + tid; i < N_out; i += PROSODY_THREADS) yr[i] = 0.f;

  if (flags & 1) {  // pass-through row: copy and scale, no state
    for (long i = tid; i < n_emit; i += PROSODY_THREADS)
      yr[i] = i < m ? xr[i] * g : 0.f;
    return;
  }

  for (int i = tid; i < carry_len; i += PROSODY_THREADS) car[i] = cr[i];
  if (k0 > 0)
    for (int j = tid; j < half; j += PROSODY_THREADS) tail[j] = tl[j];
  __syncthreads();
  // logical input at global position q (in_pos <= q < a0 + m)
  auto in = [&](int q) -> float {
    return q < a0 ? car[q - in_pos] : xr[q - a0];
  };

  for (int k = k0; k < k0 + nk; ++k) {
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
    const int n_seg = min(n_cand + frame, seg_cap);
    for (int i = tid; i < n_seg; i += PROSODY_THREADS) seg[i] = in(base + i);
    __syncthreads();

    int off = 0;
    if (n_cand > 0) {
      float best = -INFINITY;
      int best_i = INT_MAX;
      // as wsola_rows_kernel: two candidates per thread per sweep, each
      // summing j = 0..half-1 in order
      for (int c0 = tid; c0 < n_cand; c0 += 2 * PROSODY_THREADS) {
        const int c1 = c0 + PROSODY_THREADS;
        const bool has1 = c1 < n_cand;
        const float* s0 = seg + c0;
        const float* s1 = seg + (has1 ? c1 : c0);
        float acc0 = 0.f, acc1 = 0.f;
#pragma unroll 8
        for (int j = 0; j < half; ++j) {
          const float tj = tail[j];
          acc0 += s0[j] * tj;
          acc1 += s1[j] * tj;
        }
        if (acc0 > best) {  // candidates ascend: first maximum kept
          best = acc0;
          best_i = c0;
        }
        if (has1 && acc1 > best) {
          best = acc1;
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
      off = (best_i >= 0 && best_i < n_cand) ? best_i : 0;
    }
    if (tid == 0) tr[k - k0] = base + off;

    const float* cur = seg + off;
    const long o0 = (long)k * half;
    for (int j = tid; j < half; j += PROSODY_THREADS) {
      const float w1 = window[j];
      const float w2 = k > 0 ? window[half + j] : 0.f;
      const float prev = k > 0 ? tail[j] : 0.f;
      const long o = o0 + j;
      if (o >= e0 && o - e0 < n_emit)
        yr[o - e0] = ola_(prev, w2, cur[j], w1, g);
      tail[j] = cur[half + j];
    }
    __syncthreads();  // tail complete, seg free for the next frame
  }

  if (flags & 2) {  // closing half frame, then zeros up to e1
    const long o0 = (long)(k0 + nk) * half;
    for (int j = tid; j < half; j += PROSODY_THREADS) {
      const long o = o0 + j;
      if (o >= e0 && o - e0 < n_emit)
        yr[o - e0] = ola_(tail[j], window[half + j], 0.f, 0.f, g);
    }
    for (long o = max(o0 + half, e0) + tid; o - e0 < n_emit;
         o += PROSODY_THREADS)
      yr[o - e0] = 0.f;
  }

  // new state: the old carry lives in LDS, the chunk row is read-only
  if (nk > 0)
    for (int j = tid; j < half; j += PROSODY_THREADS) tl[j] = tail[j];
  for (int i = tid; i < keep_len; i += PROSODY_THREADS)
    cr[i] = in(keep_pos + i);
}

// --------------------------------------------------------------------------
// resample_stream_rows: outputs [e0, e1) of resample_linear_rows_kernel on
// the logical input, positions from the GLOBAL n and n_out; one workgroup
// per row.  The carry is at most one sample: every thread holds it in a
// register before the barrier, the new one is written after it.
// --------------------------------------------------------------------------
__global__ __launch_bounds__(PROSODY_THREADS) void resample_stream_rows_kernel(
    const float* __restrict__ x, const long* __restrict__ par, float* carry,
    float* __restrict__ y, long N, long N_out) {
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const long* p = par + (long)b * RS_PAR;
  const int slot = (int)p[RS_SLOT];
  const int m = (int)p[RS_M];
  const long a0 = p[RS_A0];
  const int carry_len = (int)p[RS_CARRY];
  const long len = p[RS_N], n_out = p[RS_NOUT];
  const long e0 = p[RS_E0], e1 = p[RS_E1];
  const int flags = (int)p[RS_FLAGS];
  const long keep_pos = p[RS_KEEP_POS];
  const int keep_len = (int)p[RS_KEEP];
  const float* xr = x + (long)b * N;
  float* yr = y + (long)b * N_out;
  float* cr = carry + (long)slot * RS_CARRY_CAP;
  const long n_emit = min(e1 - e0, N_out);

  for (long i = n_emit + tid; i < N_out; i += PROSODY_THREADS) yr[i] = 0.f;
  if (flags & 1) {  // copy row, no state
    for (long i = tid; i < n_emit; i += PROSODY_THREADS)
      yr[i] = i < m ? xr[i] : 0.f;
    return;
  }
  const float c0 = carry_len > 0 ? cr[0] : 0.f;
  __syncthreads();  // every read of the old carry is done
  // logical input at global position q (in_pos <= q < a0 + m); the carry
  // holds position a0 - 1 only
  auto in = [&](long q) -> float { return q < a0 ? c0 : xr[q - a0]; };

  for (long i = e0 + tid; i - e0 < n_emit; i += PROSODY_THREADS) {
    float v;
    if (n_out == len) {
      v = in(i);
    } else {
      const double pos =
          (double)i * (double)(len - 1) / (double)max(n_out - 1, 1L);
      long i0 = (long)floor(pos);
      i0 = min(max(i0, 0L), len - 1);
      const long i1 = min(i0 + 1, len - 1);
      const float frac = (float)(pos - (double)i0);
      v = (float)((double)in(i0) * (1.0 - (double)frac) +
                  (double)in(i1) * (double)frac);
    }
    yr[i - e0] = v;
  }
  if (tid < keep_len) cr[tid] = in(keep_pos + tid);
}

// ------------------------------ host wrappers -------------------------------
static torch::Tensor par_to_device(const std::vector<long>& host, long R,
                                   long width, const torch::Tensor& like) {
  auto t = torch::empty({R, width}, torch::TensorOptions().dtype(at::kLong));
  std::memcpy(t.data_ptr<long>(), host.data(), host.size() * sizeof(long));
  return t.to(like.device());
}

static long dbits(double v) {
  long b;
  std::memcpy(&b, &v, sizeof(b));
  return b;
}

// x [R, N] f32 chunk rows; par: R rows of WS_PAR-2 integers in the order of
// the WS_* indices up to WS_KEEP; hop, gain per row.  carry f32 [S, seg_cap],
// tails f32 [S, half]: updated in place at the named slots.  Returns
// {y [R, N_out], targets [R, K_max]}.
std::vector<torch::Tensor> wsola_stream_rows(
    torch::Tensor x, std::vector<int64_t> par, std::vector<double> hop,
    std::vector<double> gain, torch::Tensor carry, torch::Tensor tails,
    torch::Tensor window, long half, long search, long N_out, long K_max) {
  check_rows(x, "wsola_stream_rows");
  const long R = x.size(0), N = x.size(1);
  constexpr long NP = WS_KEEP + 1;
  TORCH_CHECK((long)par.size() == R * NP && (long)hop.size() == R &&
                  (long)gain.size() == R,
              "wsola_stream_rows: one parameter row per chunk row");
  TORCH_CHECK(half >= 1 && search >= 1 && half < (1 << 24) &&
                  search < (1 << 24),
              "wsola_stream_rows: bad frame geometry");
  check_vec(window, at::kFloat, 2 * half, "wsola_stream_rows");
  const long frame = 2 * half;
  const long seg_cap = (2 * search + frame + 3) & ~3L;
  auto f32_on = [&](const torch::Tensor& t) {
    return t.is_cuda() && t.device() == x.device() && t.is_contiguous() &&
           t.scalar_type() == at::kFloat && t.dim() == 2;
  };
  TORCH_CHECK(f32_on(carry) && carry.size(1) == seg_cap && f32_on(tails) &&
                  tails.size(1) == half && tails.size(0) == carry.size(0),
              "wsola_stream_rows: state must be cuda f32 [S, ", seg_cap,
              "] and [S, ", half, "]");
  const long S = carry.size(0);
  TORCH_CHECK(N_out >= 0 && N_out < INT_MAX && K_max >= 1 && K_max < INT_MAX &&
                  R < 65536,
              "wsola_stream_rows: shape out of range");
  const long lds =
      (2 * seg_cap + ((half + 3) & ~3L)) * sizeof(float) + 4 * 8;
  TORCH_CHECK(lds <= 64 * 1024, "wsola_stream_rows: frame ", frame,
              " + search ", search, " needs ", lds,
              " bytes of LDS, over the 64 KiB a workgroup may use");
  auto y = torch::empty({R, N_out}, x.options());
  auto targets = torch::empty({R, K_max}, x.options().dtype(at::kInt));
  if (R == 0) return {y, targets};

  std::vector<long> host(R * WS_PAR, 0);
  std::vector<char> named(S, 0);
  for (long r = 0; r < R; ++r) {
    const int64_t* q = par.data() + r * NP;
    const long slot = q[WS_SLOT], m = q[WS_M], a0 = q[WS_A0];
    const long in_pos = q[WS_IN_POS], clen = q[WS_CARRY], k0 = q[WS_K0];
    const long nk = q[WS_NK], n = q[WS_N], e0 = q[WS_E0], e1 = q[WS_E1];
    const long flags = q[WS_FLAGS], keep_pos = q[WS_KEEP_POS];
    const long keep = q[WS_KEEP];
    TORCH_CHECK(slot >= 0 && slot < S && !named[slot],
                "wsola_stream_rows: slot out of range or named twice");
    named[slot] = 1;
    TORCH_CHECK(m >= 0 && m <= N && a0 >= 0 && n < INT_MAX && a0 + m <= n,
                "wsola_stream_rows: chunk outside the stream");
    TORCH_CHECK(e0 >= 0 && e1 >= e0 && e1 - e0 <= N_out && e1 < INT_MAX,
                "wsola_stream_rows: output range");
    TORCH_CHECK((flags & ~3L) == 0, "wsola_stream_rows: flags");
    if (flags & 1) {
      TORCH_CHECK(e1 - e0 == m, "wsola_stream_rows: pass-through length");
    } else {
      TORCH_CHECK(n >= frame, "wsola_stream_rows: row shorter than a frame");
      TORCH_CHECK(clen >= 0 && clen <= seg_cap &&
                      in_pos == (clen > 0 ? a0 - clen : a0),
                  "wsola_stream_rows: carry outside its buffer");
      TORCH_CHECK(k0 >= 0 && nk >= 0 && nk <= K_max && k0 + nk < (1 << 30),
                  "wsola_stream_rows: frame range");
      // every frame reads [base, base + n_cand + frame) of the logical input
      for (long k = k0; k < k0 + nk; ++k) {
        long t = (long)(int)((double)k * hop[r]);
        long base = t, n_cand = 0;
        if (k > 0) {
          const long lo = std::max(t - search, 0L);
          const long hi = std::min(t + search, n - frame);
          if (hi > lo) n_cand = hi - lo;
          base = lo;
        }
        if (n_cand == 0) base = std::min(std::max(t, 0L), n - frame);
        TORCH_CHECK(base >= in_pos && base + n_cand + frame <= a0 + m &&
                        n_cand + frame <= seg_cap,
                    "wsola_stream_rows: frame ", k,
                    " reads outside carry ++ chunk");
      }
      // frames write [k0*half, (k0+nk)*half), the closing flag the rest
      TORCH_CHECK(e0 >= std::min(k0 * half, e1) &&
                      ((flags & 2) || e1 == e0 || e1 <= (k0 + nk) * half),
                  "wsola_stream_rows: emitted range not covered");
      TORCH_CHECK(!(flags & 2) || k0 + nk > 0,
                  "wsola_stream_rows: closing before any frame");
      TORCH_CHECK(keep >= 0 && keep <= seg_cap &&
                      (keep == 0 ||
                       (keep_pos >= in_pos && keep_pos + keep == a0 + m)),
                  "wsola_stream_rows: new carry outside carry ++ chunk");
    }
    long* h = host.data() + r * WS_PAR;
    for (long i = 0; i < NP; ++i) h[i] = q[i];
    h[WS_HOP] = dbits(hop[r]);
    h[WS_GAIN] = dbits(gain[r]);
  }
  auto par_d = par_to_device(host, R, WS_PAR, x);
  hipLaunchKernelGGL(wsola_stream_rows_kernel, dim3(R), dim3(PROSODY_THREADS),
                     (size_t)lds, cur_stream(), x.data_ptr<float>(),
                     par_d.data_ptr<long>(), carry.data_ptr<float>(),
                     tails.data_ptr<float>(), window.data_ptr<float>(),
                     y.data_ptr<float>(), targets.data_ptr<int>(), N, N_out,
                     (int)K_max, (int)half, (int)search, (int)seg_cap);
  return {y, targets};
}

// x [R, N] f32 chunk rows; par: R rows of RS_PAR integers in the order of the
// RS_* indices; carry f32 [S, RS_CARRY_CAP], updated in place.  Returns
// y [R, N_out].
torch::Tensor resample_stream_rows(torch::Tensor x, std::vector<int64_t> par,
                                   torch::Tensor carry, long N_out) {
  check_rows(x, "resample_stream_rows");
  const long R = x.size(0), N = x.size(1);
  TORCH_CHECK((long)par.size() == R * RS_PAR,
              "resample_stream_rows: one parameter row per chunk row");
  TORCH_CHECK(carry.is_cuda() && carry.device() == x.device() &&
                  carry.is_contiguous() &&
                  carry.scalar_type() == at::kFloat && carry.dim() == 2 &&
                  carry.size(1) == RS_CARRY_CAP,
              "resample_stream_rows: carry must be cuda f32 [S, ",
              RS_CARRY_CAP, "]");
  const long S = carry.size(0);
  TORCH_CHECK(N_out >= 0 && N_out < INT_MAX && R < 65536,
              "resample_stream_rows: shape out of range");
  auto y = torch::empty({R, N_out}, x.options());
  if (R == 0) return y;

  std::vector<long> host(par.begin(), par.end());
  std::vector<char> named(S, 0);
  for (long r = 0; r < R; ++r) {
    const long* q = host.data() + r * RS_PAR;
    const long slot = q[RS_SLOT], m = q[RS_M], a0 = q[RS_A0];
    const long in_pos = q[RS_IN_POS], clen = q[RS_CARRY], n = q[RS_N];
    const long n_out = q[RS_NOUT], e0 = q[RS_E0], e1 = q[RS_E1];
    const long flags = q[RS_FLAGS], keep_pos = q[RS_KEEP_POS];
    const long keep = q[RS_KEEP];
    TORCH_CHECK(slot >= 0 && slot < S && !named[slot],
                "resample_stream_rows: slot out of range or named twice");
    named[slot] = 1;
    TORCH_CHECK(m >= 0 && m <= N && a0 >= 0 && n < INT_MAX && a0 + m <= n,
                "resample_stream_rows: chunk outside the stream");
    TORCH_CHECK(e0 >= 0 && e1 >= e0 && e1 - e0 <= N_out && e1 <= n_out &&
                    n_out < INT_MAX,
                "resample_stream_rows: output range");
    TORCH_CHECK((flags & ~1L) == 0, "resample_stream_rows: flags");
    if (flags & 1) {
      TORCH_CHECK(e1 - e0 == m, "resample_stream_rows: copy length");
      continue;
    }
    TORCH_CHECK(clen >= 0 && clen <= RS_CARRY_CAP &&
                    in_pos == (clen > 0 ? a0 - clen : a0),
                "resample_stream_rows: carry outside its buffer");
    if (e1 > e0) {
      // positions ascend: the first output reads the lowest sample, the
      // last one the highest
      TORCH_CHECK(n >= 1, "resample_stream_rows: output of an empty row");
      auto i0_of = [&](long i) {
        if (n_out == n) return i;
        const double pos =
            (double)i * (double)(n - 1) / (double)std::max(n_out - 1, 1L);
        return std::min(std::max((long)std::floor(pos), 0L), n - 1);
      };
      const long first = i0_of(e0);
      const long i0 = i0_of(e1 - 1);
      const long last = n_out == n ? i0 : std::min(i0 + 1, n - 1);
      TORCH_CHECK(first >= in_pos && last < a0 + m,
                  "resample_stream_rows: reads outside carry ++ chunk");
    }
    TORCH_CHECK(keep >= 0 && keep <= RS_CARRY_CAP &&
                    (keep == 0 ||
                     (keep_pos >= in_pos && keep_pos + keep == a0 + m)),
                "resample_stream_rows: new carry outside carry ++ chunk");
  }
  auto par_d = par_to_device(host, R, RS_PAR, x);
  hipLaunchKernelGGL(resample_stream_rows_kernel, dim3(R),
                     dim3(PROSODY_THREADS), 0, cur_stream(),
                     x.data_ptr<float>(), par_d.data_ptr<long>(),
                     carry.data_ptr<float>(), y.data_ptr<float>(), N, N_out);
  return y;
}
