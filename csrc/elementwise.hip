// Fused elementwise / normalization kernels for the VITS graph.
//
// Ops (SURVEY.md §2.2 kernel inventory):
//   - layer_norm_ct: LayerNorm across channels of [B, C, T]
//   - fused_gate:    WaveNet tanh(a+ga)·sigmoid(b+gb) gate
//   - prior_sample:  z = (m + eps·exp(logs)·noise_scale)·mask
//   - expand_states: duration length-regulator gather
//
// All are HBM-bandwidth-bound: one coalesced read per input element, one
// write per output, activations fused so no intermediate tensors hit HBM.
#include "common.h"

// --------------------------------------------------------------------------
// layer_norm_ct: x [B, C, T] -> per-(b,t) normalize across C.
// Thread t-major: lane i handles time position t0+i so every c-iteration
// reads a contiguous [blockDim.x] segment (fully coalesced along T).
// --------------------------------------------------------------------------
template <typename T, bool HAS_RES>
__global__ void layer_norm_ct_kernel(const T* __restrict__ x,
                                     const T* __restrict__ res,
                                     const float* __restrict__ gamma,
                                     const float* __restrict__ beta,
                                     T* __restrict__ out, int C, long T_len,
                                     float eps, long n_bt) {
  const long bt = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (bt >= n_bt) return;
  const long b = bt / T_len;
  const long t = bt % T_len;
  const long base = (b * C) * T_len + t;
  const T* xp = x + base;
  const T* rp = HAS_RES ? res + base : nullptr;
  // two passes (mean, then centred sum of squares): ss/C - mean^2 in one
  // f32 pass cancels catastrophically when |mean| >> std
  float s = 0.f;
  for (int c = 0; c < C; ++c) {
    float v = ld_f(xp + (long)c * T_len);
    if (HAS_RES) v += ld_f(rp + (long)c * T_len);
    s += v;
  }
  const float mean = s / C;
  float ss = 0.f;
  for (int c = 0; c < C; ++c) {
    float v = ld_f(xp + (long)c * T_len);
    if (HAS_RES) v += ld_f(rp + (long)c * T_len);
    v -= mean;
    ss += v * v;
  }
  const float rstd = rsqrtf(ss / C + eps);
  T* op = out + base;
  for (int c = 0; c < C; ++c) {
    float v = ld_f(xp + (long)c * T_len);
    if (HAS_RES) v += ld_f(rp + (long)c * T_len);
    st_f(op + (long)c * T_len, (v - mean) * rstd * gamma[c] + beta[c]);
  }
}

// Lane-split variant for small B*T (encoder: ~8k tokens underfills the
// 256-CU chip with one thread per token).  SPLIT lanes cooperate on one
// token: lane = part*(64/SPLIT) + token, so each 64-lane wave holds
// 64/SPLIT tokens; stats reduced with SPLIT-1 shfl_xor rounds.  Each
// part owns a contiguous channel chunk (coalesced along T within a
// part-group).
template <typename T, bool HAS_RES, int SPLIT>
__global__ void layer_norm_ct_split_kernel(const T* __restrict__ x,
                                           const T* __restrict__ res,
                                           const float* __restrict__ gamma,
                                           const float* __restrict__ beta,
                                           T* __restrict__ out, int C,
                                           long T_len, float eps,
                                           long n_bt) {
  constexpr int TOK = 64 / SPLIT;  // tokens per wave
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int part = lane / TOK;
  const int tok = lane % TOK;
  const long bt = ((long)blockIdx.x * (blockDim.x >> 6) + wid) * TOK + tok;
  const bool live = bt < n_bt;
  const long b = live ? bt / T_len : 0;
  const long t = live ? bt % T_len : 0;
  const long base = (b * C) * T_len + t;
  const T* xp = x + base;
  const T* rp = HAS_RES ? res + base : nullptr;
  const int cq = (C + SPLIT - 1) / SPLIT;
  const int c_lo = part * cq;
  const int c_hi = min(c_lo + cq, C);
  float s = 0.f;
  if (live) {
    for (int c = c_lo; c < c_hi; ++c) {
      float v = ld_f(xp + (long)c * T_len);
      if (HAS_RES) v += ld_f(rp + (long)c * T_len);
      s += v;
    }
  }
  // combine the SPLIT part-lanes of each token (they sit TOK apart)
#pragma unroll
  for (int d = TOK; d < 64; d <<= 1) s += __shfl_xor(s, d, 64);
  const float mean = s / C;
  // second pass + second butterfly: centred sum of squares (stable under
  // a channel offset, unlike ss/C - mean^2)
  float ss = 0.f;
  if (live) {
    for (int c = c_lo; c < c_hi; ++c) {
      float v = ld_f(xp + (long)c * T_len);
      if (HAS_RES) v += ld_f(rp + (long)c * T_len);
      v -= mean;
      ss += v * v;
    }
  }
#pragma unroll
  for (int d = TOK; d < 64; d <<= 1) ss += __shfl_xor(ss, d, 64);
  if (!live) return;
  const float rstd = rsqrtf(ss / C + eps);
  T* op = out + base;
  for (int c = c_lo; c < c_hi; ++c) {
    float v = ld_f(xp + (long)c * T_len);
    if (HAS_RES) v += ld_f(rp + (long)c * T_len);
    st_f(op + (long)c * T_len, (v - mean) * rstd * gamma[c] + beta[c]);
  }
}

// --------------------------------------------------------------------------
// fused_gate: x [B, 2C, T] (+ optional g) -> tanh·sigmoid gate [B, C, T]
// --------------------------------------------------------------------------
template <typename T, bool HAS_G>
__global__ void fused_gate_kernel(const T* __restrict__ x,
                                  const T* __restrict__ g,
                                  T* __restrict__ out, long C_T, long CT2,
                                  long T_len, long g_T,  // g time size: T or 1
                                  long n) {
  // n = B*C*T ; C_T = C*T (half-channel offset); CT2 = 2*C*T (batch stride)
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  long b = i / C_T;
  long r = i % C_T;
  long ia = b * CT2 + r;
  long ib = ia + C_T;
  float va = ld_f(x + ia), vb = ld_f(x + ib);
  if (HAS_G) {
    // g may be time-broadcast [B, 2C, 1] (speaker conditioning)
    long c = r / T_len;
    long t = g_T == 1 ? 0 : r % T_len;
    long C = C_T / T_len;
    long ga = (b * 2 * C + c) * g_T + t;
    va += ld_f(g + ga);
    vb += ld_f(g + (ga + C * g_T));
  }
  st_f(out + i, tanhf(va) * sigmoidf_(vb));
}

// --------------------------------------------------------------------------
// prior_sample
// --------------------------------------------------------------------------
template <typename T>
__global__ void prior_sample_kernel(const T* __restrict__ m,
                                    const T* __restrict__ logs,
                                    const T* __restrict__ mask,  // [B,1,T]
                                    const T* __restrict__ noise,
                                    T* __restrict__ out, long C_T, long T_len,
                                    long ms, float ns, long n) {
  // ms: batch stride of m and logs (C_T when contiguous; 2*C_T when both
  // are channel halves of one [B,2C,T] stats tensor)
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  long b = i / C_T;
  long t = i % T_len;
  long j = b * ms + (i - b * C_T);
  float msk = ld_f(mask + b * T_len + t);
  float v = ld_f(m + j) + ld_f(noise + i) * __expf(ld_f(logs + j)) * ns;
  st_f(out + i, v * msk);
}

// --------------------------------------------------------------------------
// expand_states: stats [B, C, T] + durations [B, T] -> out [B, C, F]
// Per block: batch row b.  Thread 0 builds the cumulative-duration ->
// phoneme-index table in LDS (T is a few hundred), then all threads gather
// coalesced along F.
// --------------------------------------------------------------------------
template <typename T>
__global__ void expand_states_kernel(const T* __restrict__ stats,
                                     const int* __restrict__ durs,
                                     T* __restrict__ out, int C, int T_ph,
                                     int F_max) {
  extern __shared__ int idx_lds[];  // [F_max] phoneme index per frame
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  // serial cumsum + fill (T_ph and F_max are small; ~µs)
  if (tid == 0) {
    int f = 0;
    for (int p = 0; p < T_ph && f < F_max; ++p) {
      int d = durs[b * T_ph + p];
      for (int k = 0; k < d && f < F_max; ++k) idx_lds[f++] = p;
    }
    // pad remaining frames with last phoneme (masked out later anyway)
    int last = T_ph - 1;
    while (f < F_max) idx_lds[f++] = last;
  }
  __syncthreads();
  const T* sp = stats + (long)b * C * T_ph;
  T* op = out + (long)b * C * F_max;
  for (long cf = tid; cf < (long)C * F_max; cf += blockDim.x) {
    int c = cf / F_max;
    int f = cf % F_max;
    op[cf] = sp[(long)c * T_ph + idx_lds[f]];
  }
}

// ========================================================================
// host wrappers
// ========================================================================
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

static inline hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

#define DISPATCH_FT(TENSOR, NAME, ...)                                     \
  do {                                                                     \
    if ((TENSOR).scalar_type() == at::kFloat) {                            \
      using scalar_t = float;                                              \
      __VA_ARGS__;                                                         \
    } else if ((TENSOR).scalar_type() == at::kBFloat16) {                  \
      using scalar_t = bf16;                                               \
      __VA_ARGS__;                                                         \
    } else {                                                               \
      TORCH_CHECK(false, NAME ": unsupported dtype");                      \
    }                                                                      \
  } while (0)

torch::Tensor layer_norm_ct(torch::Tensor x, c10::optional<torch::Tensor> res,
                            torch::Tensor gamma, torch::Tensor beta,
                            double eps) {
  TORCH_CHECK(x.dim() == 3 && x.is_cuda() && x.is_contiguous());
  const long B = x.size(0), C = x.size(1), T = x.size(2);
  auto out = torch::empty_like(x);
  auto gamma_f = gamma.to(at::kFloat).contiguous();
  auto beta_f = beta.to(at::kFloat).contiguous();
  // Fill the chip: one thread per token underfills at encoder sizes
  // (B*T ~ 8k vs 256 CUs), so split each token's channel reduction over
  // SPLIT lanes when the token count is small.
  const long n_bt = B * T;
  const int threads = 256;
#define LN_LAUNCH(KER, GRID)                                                \
  DISPATCH_FT(x, "layer_norm_ct", {                                        \
    if (res.has_value()) {                                                 \
      TORCH_CHECK(res->sizes() == x.sizes() && res->is_contiguous());      \
      hipLaunchKernelGGL((KER<scalar_t, true>), GRID, dim3(threads), 0,    \
                         cur_stream(), (const scalar_t*)x.data_ptr(),      \
                         (const scalar_t*)res->data_ptr(),                 \
                         gamma_f.data_ptr<float>(),                        \
                         beta_f.data_ptr<float>(),                         \
                         (scalar_t*)out.data_ptr(), (int)C, T, (float)eps, \
                         n_bt);                                            \
    } else {                                                               \
      hipLaunchKernelGGL((KER<scalar_t, false>), GRID, dim3(threads), 0,   \
                         cur_stream(), (const scalar_t*)x.data_ptr(),      \
                         (const scalar_t*)nullptr,                         \
                         gamma_f.data_ptr<float>(),                        \
                         beta_f.data_ptr<float>(),                         \
                         (scalar_t*)out.data_ptr(), (int)C, T, (float)eps, \
                         n_bt);                                            \
    }                                                                      \
  })
  if (n_bt <= 16384) {
    dim3 grid(ceil_div(n_bt, (long)threads / 8));
    DISPATCH_FT(x, "layer_norm_ct", {
      if (res.has_value()) {
        TORCH_CHECK(res->sizes() == x.sizes() && res->is_contiguous());
        hipLaunchKernelGGL((layer_norm_ct_split_kernel<scalar_t, true, 8>),
                           grid, dim3(threads), 0, cur_stream(),
                           (const scalar_t*)x.data_ptr(),
                           (const scalar_t*)res->data_ptr(),
                           gamma_f.data_ptr<float>(),
                           beta_f.data_ptr<float>(),
                           (scalar_t*)out.data_ptr(), (int)C, T, (float)eps,
                           n_bt);
      } else {
        hipLaunchKernelGGL((layer_norm_ct_split_kernel<scalar_t, false, 8>),
                           grid, dim3(threads), 0, cur_stream(),
                           (const scalar_t*)x.data_ptr(),
                           (const scalar_t*)nullptr,
                           gamma_f.data_ptr<float>(),
                           beta_f.data_ptr<float>(),
                           (scalar_t*)out.data_ptr(), (int)C, T, (float)eps,
                           n_bt);
      }
    });
  } else {
    dim3 grid(ceil_div(n_bt, (long)threads));
    LN_LAUNCH(layer_norm_ct_kernel, grid);
  }
#undef LN_LAUNCH
  return out;
}

torch::Tensor fused_gate(torch::Tensor x, c10::optional<torch::Tensor> g,
                         long n_channels) {
  TORCH_CHECK(x.dim() == 3 && x.is_cuda() && x.is_contiguous());
  const long B = x.size(0), C2 = x.size(1), T = x.size(2);
  TORCH_CHECK(C2 == 2 * n_channels, "fused_gate: channel mismatch");
  auto out = torch::empty({B, n_channels, T}, x.options());
  const long n = B * n_channels * T;
  const int threads = 256;
  const long blocks = (n + threads - 1) / threads;
  DISPATCH_FT(x, "fused_gate", {
    if (g.has_value()) {
      TORCH_CHECK(g->dim() == 3 && g->size(0) == B && g->size(1) == C2 &&
                      (g->size(2) == T || g->size(2) == 1),
                  "fused_gate: g must be [B,2C,T] or [B,2C,1]");
      hipLaunchKernelGGL((fused_gate_kernel<scalar_t, true>), dim3(blocks),
                         dim3(threads), 0, cur_stream(),
                         (const scalar_t*)x.data_ptr(),
                         (const scalar_t*)g->data_ptr(),
                         (scalar_t*)out.data_ptr(), n_channels * T,
                         2 * n_channels * T, T, g->size(2), n);
    } else {
      hipLaunchKernelGGL((fused_gate_kernel<scalar_t, false>), dim3(blocks),
                         dim3(threads), 0, cur_stream(),
                         (const scalar_t*)x.data_ptr(), (const scalar_t*)nullptr,
                         (scalar_t*)out.data_ptr(), n_channels * T,
                         2 * n_channels * T, T, 1, n);
    }
  });
  return out;
}

torch::Tensor prior_sample(torch::Tensor m, torch::Tensor logs,
                           torch::Tensor mask, torch::Tensor noise,
                           double noise_scale) {
  TORCH_CHECK(m.is_cuda() && m.dim() == 3);
  const long B = m.size(0), C = m.size(1), T = m.size(2);
  // m and logs: dense [C,T] planes; the batch stride is free, so the two
  // channel halves of one expanded [B,2C,T] tensor pass without a copy
  auto dense_planes = [&](const torch::Tensor& t) {
    return (T == 1 || t.stride(2) == 1) && (C == 1 || t.stride(1) == T);
  };
  TORCH_CHECK(m.sizes() == logs.sizes() && dense_planes(m) &&
                  dense_planes(logs) &&
                  (B == 1 || m.stride(0) == logs.stride(0)),
              "prior_sample: m/logs planes must be dense, one batch stride");
  TORCH_CHECK(noise.is_contiguous() && mask.is_contiguous());
  const long ms = B > 1 ? m.stride(0) : C * T;
  auto out = torch::empty({B, C, T}, m.options());
  const long n = B * C * T;
  const int threads = 256;
  DISPATCH_FT(m, "prior_sample", {
    hipLaunchKernelGGL(prior_sample_kernel<scalar_t>,
                       dim3((n + threads - 1) / threads), dim3(threads), 0,
                       cur_stream(), (const scalar_t*)m.data_ptr(),
                       (const scalar_t*)logs.data_ptr(),
                       (const scalar_t*)mask.data_ptr(),
                       (const scalar_t*)noise.data_ptr(),
                       (scalar_t*)out.data_ptr(), C * T, T, ms,
                       (float)noise_scale, n);
  });
  return out;
}

torch::Tensor expand_states(torch::Tensor stats, torch::Tensor durs,
                            long F_max) {
  TORCH_CHECK(stats.dim() == 3 && stats.is_cuda() && stats.is_contiguous());
  TORCH_CHECK(durs.scalar_type() == at::kInt && durs.is_contiguous());
  const long B = stats.size(0), C = stats.size(1), T = stats.size(2);
  auto out = torch::empty({B, C, F_max}, stats.options());
  size_t lds = F_max * sizeof(int);
  TORCH_CHECK(lds <= 160 * 1024, "expand_states: F too large for LDS");
  DISPATCH_FT(stats, "expand_states", {
    hipLaunchKernelGGL(expand_states_kernel<scalar_t>, dim3(B), dim3(256),
                       lds, cur_stream(), (const scalar_t*)stats.data_ptr(),
                       durs.data_ptr<int>(), (scalar_t*)out.data_ptr(),
                       (int)C, (int)T, (int)F_max);
  });
  return out;
}

// --------------------------------------------------------------------------
// mask_tail_: in-place zero of x[b, :, lens[b]:] for padded batches.
// Makes ragged-batch decoding bit-equal to single-utterance decoding when
// applied after each conv stage (padding region never feeds valid taps).
// One block per (b, c) row; threads sweep the tail only.
// --------------------------------------------------------------------------
template <typename T>
__global__ void mask_tail_kernel(T* __restrict__ x,
                                 const int* __restrict__ lens, int C,
                                 long T_len) {
  const int b = blockIdx.y;
  const int c = blockIdx.x;
  const long lo = lens[b];
  for (long t = lo + threadIdx.x; t < T_len; t += blockDim.x)
    x[((long)b * C + c) * T_len + t] = T(0);
}

torch::Tensor mask_tail_(torch::Tensor x, torch::Tensor lens) {
  TORCH_CHECK(x.dim() == 3 && x.is_cuda() && x.is_contiguous());
  TORCH_CHECK(lens.scalar_type() == at::kInt && lens.is_cuda() &&
              lens.is_contiguous() && lens.size(0) == x.size(0));
  const long B = x.size(0), C = x.size(1), T_len = x.size(2);
  DISPATCH_FT(x, "mask_tail_", {
    hipLaunchKernelGGL(mask_tail_kernel<scalar_t>, dim3(C, B), dim3(256), 0,
                       cur_stream(), (scalar_t*)x.data_ptr(),
                       lens.data_ptr<int>(), (int)C, T_len);
  });
  return x;
}

// --------------------------------------------------------------------------
// fused_gate_cl: channel-last WaveNet gate.
// x [B, F, 2C] (+ optional g [B, 2C] speaker bias or [B, F, 2C]) ->
// out [B, F, C] = tanh(xa + ga) * sigmoid(xb + gb).
// Channel-last rows are contiguous: coalesced along C.
// --------------------------------------------------------------------------
template <typename T, int GMODE>  // 0: none, 1: [B,2C] broadcast, 2: full
__global__ void fused_gate_cl_kernel(const T* __restrict__ x,
                                     const T* __restrict__ g,
                                     T* __restrict__ out, long C, long F_len,
                                     long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;  // n = B*F*C
  const long c = i % C;
  const long bf = i / C;
  const long b = bf / F_len;
  const long ia = bf * 2 * C + c;
  float va = ld_f(x + ia), vb = ld_f(x + ia + C);
  if (GMODE == 1) {
    va += ld_f(g + b * 2 * C + c);
    vb += ld_f(g + b * 2 * C + C + c);
  } else if (GMODE == 2) {
    va += ld_f(g + ia);
    vb += ld_f(g + ia + C);
  }
  st_f(out + i, tanhf(va) * sigmoidf_(vb));
}

torch::Tensor fused_gate_cl(torch::Tensor x, c10::optional<torch::Tensor> g,
                            long n_channels) {
  TORCH_CHECK(x.dim() == 3 && x.is_cuda() && x.is_contiguous());
  const long B = x.size(0), F_len = x.size(1), C2 = x.size(2);
  TORCH_CHECK(C2 == 2 * n_channels, "fused_gate_cl: channel mismatch");
  auto out = torch::empty({B, F_len, n_channels}, x.options());
  const long n = B * F_len * n_channels;
  const int threads = 256;
  const long blocks = (n + threads - 1) / threads;
  DISPATCH_FT(x, "fused_gate_cl", {
    if (!g.has_value()) {
      hipLaunchKernelGGL((fused_gate_cl_kernel<scalar_t, 0>), dim3(blocks),
                         dim3(threads), 0, cur_stream(),
                         (const scalar_t*)x.data_ptr(),
                         (const scalar_t*)nullptr,
                         (scalar_t*)out.data_ptr(), n_channels, F_len, n);
    } else if (g->dim() == 2 ||
               (g->dim() == 3 && g->size(1) == 1)) {
      TORCH_CHECK(g->numel() == B * C2, "fused_gate_cl: bad g");
      hipLaunchKernelGGL((fused_gate_cl_kernel<scalar_t, 1>), dim3(blocks),
                         dim3(threads), 0, cur_stream(),
                         (const scalar_t*)x.data_ptr(),
                         (const scalar_t*)g->contiguous().data_ptr(),
                         (scalar_t*)out.data_ptr(), n_channels, F_len, n);
    } else {
      TORCH_CHECK(g->sizes() == x.sizes(), "fused_gate_cl: bad g");
      hipLaunchKernelGGL((fused_gate_cl_kernel<scalar_t, 2>), dim3(blocks),
                         dim3(threads), 0, cur_stream(),
                         (const scalar_t*)x.data_ptr(),
                         (const scalar_t*)g->contiguous().data_ptr(),
                         (scalar_t*)out.data_ptr(), n_channels, F_len, n);
    }
  });
  return out;
}

// --------------------------------------------------------------------------
// depthwise_cl: channel-last depthwise Conv1d (DDSConv separable stage).
// out[b,t,c] = bias[c] + sum_j x[b, t + j*dil - pad, c] * w[c, j]
// Channel-last rows are contiguous: thread handles 8 channels of one row
// (b128 loads/stores); taps walk rows.  Memory-bound by design.
// --------------------------------------------------------------------------
template <typename T>
__global__ void depthwise_cl_kernel(const T* __restrict__ x,
                                    const T* __restrict__ w,  // [C][k]
                                    const float* __restrict__ bias,
                                    T* __restrict__ out, long Tlen, int C,
                                    int k, int dil, int pad, long n8) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;  // n8 = B*T*C/8
  const long c8 = (i % (C / 8)) * 8;
  const long bt = i / (C / 8);
  const long b = bt / Tlen;
  const long t = bt % Tlen;
  const T* xb = x + (b * Tlen) * C;
  float acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] = bias ? bias[c8 + q] : 0.f;
  for (int j = 0; j < k; ++j) {
    const long tt = t + (long)j * dil - pad;
    if (tt < 0 || tt >= Tlen) continue;
    const T* xr = xb + tt * C + c8;
#pragma unroll
    for (int q = 0; q < 8; ++q)
      acc[q] += ld_f(xr + q) * ld_f(w + (c8 + q) * k + j);
  }
  T* or_ = out + (b * Tlen + t) * C + c8;
#pragma unroll
  for (int q = 0; q < 8; ++q) st_f(or_ + q, acc[q]);
}

torch::Tensor depthwise_cl(torch::Tensor x, torch::Tensor w,
                           c10::optional<torch::Tensor> bias, long dil,
                           long pad) {
  // x: [B, T, C] channel-last; w: [C, 1, k] (nn.Conv1d groups=C weight)
  TORCH_CHECK(x.dim() == 3 && x.is_cuda() && x.is_contiguous());
  const long B = x.size(0), Tlen = x.size(1), C = x.size(2);
  TORCH_CHECK(C % 8 == 0, "depthwise_cl: C % 8 != 0");
  auto w2 = w.reshape({C, w.size(-1)}).contiguous();
  const long k = w2.size(1);
  auto out = torch::empty_like(x);
  torch::Tensor bias_f;
  const float* bias_p = nullptr;
  if (bias.has_value()) {
    bias_f = bias->scalar_type() == at::kFloat
                 ? *bias : bias->to(at::kFloat).contiguous();
    bias_p = bias_f.data_ptr<float>();
  }
  const long n8 = B * Tlen * (C / 8);
  const int threads = 256;
  DISPATCH_FT(x, "depthwise_cl", {
    hipLaunchKernelGGL(depthwise_cl_kernel<scalar_t>,
                       dim3((n8 + threads - 1) / threads), dim3(threads), 0,
                       cur_stream(), (const scalar_t*)x.data_ptr(),
                       (const scalar_t*)w2.data_ptr(), bias_p,
                       (scalar_t*)out.data_ptr(), Tlen, (int)C, (int)k,
                       (int)dil, (int)pad, n8);
  });
  return out;
}

// ------------------------------------------------------------------------- //
// seeded_noise: per-utterance deterministic standard-normal noise in ONE
// launch.  Replaces the per-row torch::randn loops (B x 2 generator
// launches per batch + per-row .item() syncs) that showed up as 1.4k
// distribution kernels per bench step.  Value at (b, c, t) depends ONLY
// on (seeds[b], c, t): noise is independent of batch composition, rank
// AND padding by construction (SURVEY.md section 7 hard part 7).
// RNG: splitmix64 counter hash -> Box-Muller.
// ------------------------------------------------------------------------- //
__device__ __forceinline__ unsigned long long sm64_(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

template <typename T>
__global__ void seeded_noise_kernel(T* __restrict__ out,
                                    const long* __restrict__ seeds,
                                    const int* __restrict__ lens,
                                    long B, long C, long Tm) {
  const long total = B * C * Tm;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    const long b = i / (C * Tm);
    const long rem = i - b * C * Tm;
    const long c = rem / Tm, t = rem - (rem / Tm) * Tm;
    float v = 0.f;
    if (t < (long)lens[b]) {
      const unsigned long long ctr =
          ((unsigned long long)(c + 1) << 40) ^ (unsigned long long)t;
      const unsigned long long r1 =
          sm64_((unsigned long long)seeds[b] ^ sm64_(ctr));
      const unsigned long long r2 = sm64_(r1);
      const float u1 = (float)((r1 >> 11) + 1) * 1.1102230246251565e-16f;
      const float u2 = (float)(r2 >> 11) * 1.1102230246251565e-16f;
      v = sqrtf(-2.0f * __logf(u1)) * __cosf(6.28318530717958f * u2);
    }
    st_f(out + i, v);
  }
}

torch::Tensor seeded_noise(long B, long C, long T_max, torch::Tensor lens,
                           torch::Tensor seeds, torch::ScalarType dtype) {
  TORCH_CHECK(lens.is_cuda() && lens.scalar_type() == at::kInt);
  TORCH_CHECK(seeds.is_cuda() && seeds.scalar_type() == at::kLong);
  TORCH_CHECK(lens.numel() == B && seeds.numel() == B);
  auto out = torch::empty(
      {B, C, T_max},
      torch::TensorOptions().device(lens.device()).dtype(dtype));
  if (out.numel() == 0) return out;
  const long total = B * C * T_max;
  const int blocks = (int)std::min<long>((total + 255) / 256, 4096);
  if (dtype == at::kBFloat16) {
    hipLaunchKernelGGL(seeded_noise_kernel<bf16>, dim3(blocks), dim3(256), 0,
                       cur_stream(), (bf16*)out.data_ptr(),
                       seeds.data_ptr<long>(), lens.data_ptr<int>(), B, C,
                       T_max);
  } else {
    TORCH_CHECK(dtype == at::kFloat, "seeded_noise: f32/bf16 only");
    hipLaunchKernelGGL(seeded_noise_kernel<float>, dim3(blocks), dim3(256),
                       0, cur_stream(), (float*)out.data_ptr(),
                       seeds.data_ptr<long>(), lens.data_ptr<int>(), B, C,
                       T_max);
  }
  return out;
}

// ------------------------------------------------------------------------- //
// row_ln_cl: LayerNorm over the last (channel) dim of channel-last rows
// with FUSED residual add: y = LN(x + r) * gamma + beta.  The encoder
// calls torch::layer_norm(x + y) ~400x per step (two launches + an
// intermediate tensor each); this is one launch, one pass.
// One wave per row (C <= 8*64 via per-lane accumulation + butterfly).
// ------------------------------------------------------------------------- //
template <typename T>
__global__ void row_ln_cl_kernel(const T* __restrict__ x,
                                 const T* __restrict__ r,
                                 const float* __restrict__ gamma,
                                 const float* __restrict__ beta,
                                 T* __restrict__ out, long rows, int C,
                                 float eps) {
  const long row = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const T* xr = x + row * C;
  const T* rr = r ? r + row * C : nullptr;
  float v[8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + i * 64;
    float t = 0.f;
    if (c < C) {
      t = ld_f(xr + c);
      if (rr) t += ld_f(rr + c);
    }
    v[i] = t;
    sum += t;
  }
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) sum += __shfl_xor(sum, sh, 64);
  const float mean = sum / C;
  float var = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + i * 64;
    if (c < C) {
      v[i] -= mean;
      var += v[i] * v[i];
    }
  }
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) var += __shfl_xor(var, sh, 64);
  const float inv = rsqrtf(var / C + eps);
  T* orow = out + row * C;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + i * 64;
    if (c < C) st_f(orow + c, v[i] * inv * gamma[c] + beta[c]);
  }
}

torch::Tensor row_ln_cl(torch::Tensor x, c10::optional<torch::Tensor> resid,
                        torch::Tensor gamma, torch::Tensor beta,
                        double eps) {
  TORCH_CHECK(x.dim() == 3 && x.is_cuda() && x.is_contiguous());
  const long B = x.size(0), T = x.size(1), C = x.size(2);
  TORCH_CHECK(C <= 512, "row_ln_cl: C too large");
  auto g32 = gamma.scalar_type() == at::kFloat ? gamma.contiguous()
                                               : gamma.to(at::kFloat).contiguous();
  auto b32 = beta.scalar_type() == at::kFloat ? beta.contiguous()
                                              : beta.to(at::kFloat).contiguous();
  auto out = torch::empty_like(x);
  const long rows = B * T;
  if (!rows) return out;
  const void* rp = nullptr;
  if (resid.has_value()) {
    TORCH_CHECK(resid->is_contiguous() && resid->sizes() == x.sizes());
    rp = resid->data_ptr();
  }
  const int waves_per_block = 4;  // 256 threads
  const int blocks = (int)((rows + waves_per_block - 1) / waves_per_block);
  DISPATCH_FT_CONV(x, hipLaunchKernelGGL(
      row_ln_cl_kernel<scalar_t>, dim3(blocks), dim3(64 * waves_per_block),
      0, cur_stream(), (const scalar_t*)x.data_ptr(),
      (const scalar_t*)rp, g32.data_ptr<float>(), b32.data_ptr<float>(),
      (scalar_t*)out.data_ptr(), rows, (int)C, (float)eps));
  return out;
}

// ------------------------------------------------------------------------- //
// Fused glue of the channel-last residual-coupling flow (bf16 only).
//
// The engine's flow used to run every mask multiply, residual add, cat and
// flip between its GEMMs as separate ATen passes over [B,F,H] tensors.  These
// kernels do the same arithmetic in one pass each and are BIT-IDENTICAL to
// the chains they replace: every operation is the same f32 operation in the
// same order, rounded to bf16 wherever the eager chain materialised a bf16
// tensor.  The mask is multiplied, never selected, so signed zeros come out
// as ATen's multiply leaves them.  8 bf16 (16 bytes) per thread.
// ------------------------------------------------------------------------- //
__device__ __forceinline__ void unpack_bf16x8(const uint4 u, float* f) {
  f[0] = __uint_as_float(u.x << 16);
  f[1] = __uint_as_float(u.x & 0xffff0000u);
  f[2] = __uint_as_float(u.y << 16);
  f[3] = __uint_as_float(u.y & 0xffff0000u);
  f[4] = __uint_as_float(u.z << 16);
  f[5] = __uint_as_float(u.z & 0xffff0000u);
  f[6] = __uint_as_float(u.w << 16);
  f[7] = __uint_as_float(u.w & 0xffff0000u);
}

__device__ __forceinline__ unsigned bf16_bits(float v) {
  return (unsigned)__bfloat16_as_ushort(f2bf(v));
}

__device__ __forceinline__ uint4 pack_bf16x8(const float* f) {
  uint4 u;
  u.x = bf16_bits(f[0]) | (bf16_bits(f[1]) << 16);
  u.y = bf16_bits(f[2]) | (bf16_bits(f[3]) << 16);
  u.z = bf16_bits(f[4]) | (bf16_bits(f[5]) << 16);
  u.w = bf16_bits(f[6]) | (bf16_bits(f[7]) << 16);
  return u;
}

// f32 value of bf16(v): the rounding an eager bf16 tensor puts between ops
__device__ __forceinline__ float rbf(float v) { return bf2f(f2bf(v)); }

// wn_step: one WaveNet layer's residual/skip update, in place.
//   LAYER 0 (first):  h <- bf16(bf16(h + rs[:H])*m); output <- bf16(0 + rs[H:])
//   LAYER 1 (middle): h <- bf16(bf16(h + rs[:H])*m); output <- bf16(output + rs[H:])
//   LAYER 2 (last):   rs is [rows,H]; output <- bf16(bf16(output + rs)*m)
// (0 + rs, not rs: the eager zeros_like + add turns -0 into +0.)
template <int LAYER>
__global__ void wn_step_kernel(bf16* __restrict__ h, bf16* __restrict__ output,
                               const bf16* __restrict__ rs,
                               const bf16* __restrict__ mc, int H, long n8) {
  // No FMA contraction here: the compiler narrows a product of two widened
  // bf16 values to a bf16 multiply (exact) and may then fuse it into the
  // next add across the widening, which drops the bf16 rounding of the
  // product that the eager chain performs.
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;  // n8 = rows*H/8
  const int hv = H / 8;
  const long row = i / hv;
  const int c8 = (int)(i % hv) * 8;
  const float m = bf2f(mc[row]);
  float a[8], b[8], o[8];
  if (LAYER == 2) {
    unpack_bf16x8(*reinterpret_cast<const uint4*>(output + row * H + c8), o);
    unpack_bf16x8(*reinterpret_cast<const uint4*>(rs + row * H + c8), a);
#pragma unroll
    for (int q = 0; q < 8; ++q) o[q] = rbf(o[q] + a[q]) * m;
    *reinterpret_cast<uint4*>(output + row * H + c8) = pack_bf16x8(o);
    return;
  }
  const bf16* rr = rs + row * 2 * H + c8;
  unpack_bf16x8(*reinterpret_cast<const uint4*>(rr), a);
  unpack_bf16x8(*reinterpret_cast<const uint4*>(rr + H), b);
  float x[8];
  unpack_bf16x8(*reinterpret_cast<const uint4*>(h + row * H + c8), x);
  if (LAYER == 1)
    unpack_bf16x8(*reinterpret_cast<const uint4*>(output + row * H + c8), o);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    x[q] = rbf(x[q] + a[q]) * m;
    o[q] = (LAYER == 0 ? 0.f : o[q]) + b[q];
  }
  *reinterpret_cast<uint4*>(h + row * H + c8) = pack_bf16x8(x);
  *reinterpret_cast<uint4*>(output + row * H + c8) = pack_bf16x8(o);
}

torch::Tensor wn_step(torch::Tensor h, c10::optional<torch::Tensor> output,
                      torch::Tensor rs, torch::Tensor mc, long layer) {
  // h, output [B,F,H] (updated in place); rs [B,F,2H] (layer 0/1) or
  // [B,F,H] (layer 2); mc [B,F,1].  layer 0 allocates and returns output;
  // layer 2 ignores h and returns output, which then holds the new h.
  TORCH_CHECK(rs.dim() == 3 && rs.is_cuda() && rs.is_contiguous() &&
              rs.scalar_type() == at::kBFloat16, "wn_step: rs");
  TORCH_CHECK(layer >= 0 && layer <= 2, "wn_step: layer");
  const long B = rs.size(0), F = rs.size(1);
  const long H = layer == 2 ? rs.size(2) : rs.size(2) / 2;
  TORCH_CHECK(H % 8 == 0 && (layer == 2 || rs.size(2) == 2 * H),
              "wn_step: H % 8 != 0");
  TORCH_CHECK(mc.is_contiguous() && mc.numel() == B * F &&
              mc.scalar_type() == at::kBFloat16, "wn_step: mc");
  auto check = [&](const torch::Tensor& t) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                t.scalar_type() == at::kBFloat16 && t.dim() == 3 &&
                t.size(0) == B && t.size(1) == F && t.size(2) == H,
                "wn_step: h/output must be contiguous bf16 [B,F,H]");
  };
  torch::Tensor out;
  if (layer == 0) {
    out = torch::empty({B, F, H}, rs.options());
  } else {
    TORCH_CHECK(output.has_value(), "wn_step: output required");
    out = *output;
    check(out);
  }
  if (layer != 2) check(h);
  const long n8 = B * F * (H / 8);
  if (!n8) return out;
  const int threads = 256;
  const dim3 grid((unsigned)((n8 + threads - 1) / threads));
  bf16* hp = layer == 2 ? nullptr : (bf16*)h.data_ptr();
#define WN_STEP_LAUNCH(L)                                                  \
  hipLaunchKernelGGL((wn_step_kernel<L>), grid, dim3(threads), 0,          \
                     cur_stream(), hp, (bf16*)out.data_ptr(),              \
                     (const bf16*)rs.data_ptr(), (const bf16*)mc.data_ptr(), \
                     (int)H, n8)
  if (layer == 0) WN_STEP_LAUNCH(0);
  else if (layer == 1) WN_STEP_LAUNCH(1);
  else WN_STEP_LAUNCH(2);
#undef WN_STEP_LAUNCH
  return out;
}

// coupling_tail: the end of one reverse coupling flow and the flip that
// opens the next, as index permutations of one pass.
//   ARITH: m = bf16(post*mc); x1 <- bf16(bf16(x1 - m)*mc)   (else x1 as is)
//   REV:   x0_out[j] = x1[half-1-j], x1_out[j] = x0[half-1-j]
//          (= the two halves of flip(cat(x0, x1)))
//   !REV:  x0_out = x0, x1_out = x1   (= cat(x0, x1) when the outputs are
//          the two halves of one [rows,2*half] buffer)
// x0/x1 rows are in_stride apart, outputs out_stride apart, so the same
// kernel splits a [rows,C] input (ARITH off) and fills a [rows,C] output.
template <bool REV, bool ARITH>
__global__ void coupling_tail_kernel(const bf16* __restrict__ x0,
                                     const bf16* __restrict__ x1,
                                     const bf16* __restrict__ post,
                                     const bf16* __restrict__ mc,
                                     bf16* __restrict__ x0_out,
                                     bf16* __restrict__ x1_out, int half,
                                     int in_stride, int out_stride, long n8) {
  // No FMA contraction here: the compiler narrows a product of two widened
  // bf16 values to a bf16 multiply (exact) and may then fuse it into the
  // next add across the widening, which drops the bf16 rounding of the
  // product that the eager chain performs.
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;  // n8 = rows*half/8
  const int hv = half / 8;
  const long row = i / hv;
  const int c8 = (int)(i % hv) * 8;
  float a[8], b[8];
  unpack_bf16x8(*reinterpret_cast<const uint4*>(x0 + row * in_stride + c8), a);
  unpack_bf16x8(*reinterpret_cast<const uint4*>(x1 + row * in_stride + c8), b);
  if (ARITH) {
    const float m = bf2f(mc[row]);
    float p[8];
    unpack_bf16x8(*reinterpret_cast<const uint4*>(post + row * half + c8), p);
#pragma unroll
    for (int q = 0; q < 8; ++q) b[q] = rbf(b[q] - rbf(p[q] * m)) * m;
  }
  if (REV) {
    float ra[8], rb[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      ra[q] = a[7 - q];
      rb[q] = b[7 - q];
    }
    const int d8 = half - 8 - c8;
    *reinterpret_cast<uint4*>(x0_out + row * out_stride + d8) =
        pack_bf16x8(rb);
    *reinterpret_cast<uint4*>(x1_out + row * out_stride + d8) =
        pack_bf16x8(ra);
  } else {
    *reinterpret_cast<uint4*>(x0_out + row * out_stride + c8) =
        pack_bf16x8(a);
    *reinterpret_cast<uint4*>(x1_out + row * out_stride + c8) =
        pack_bf16x8(b);
  }
}

static void coupling_launch(bool rev, bool arith, const bf16* x0,
                            const bf16* x1, const bf16* post, const bf16* mc,
                            bf16* o0, bf16* o1, long rows, long half,
                            long in_stride, long out_stride) {
  const long n8 = rows * (half / 8);
  if (!n8) return;
  const int threads = 256;
  const dim3 grid((unsigned)((n8 + threads - 1) / threads));
#define CT_LAUNCH(R, A)                                                    \
  hipLaunchKernelGGL((coupling_tail_kernel<R, A>), grid, dim3(threads), 0, \
                     cur_stream(), x0, x1, post, mc, o0, o1, (int)half,    \
                     (int)in_stride, (int)out_stride, n8)
  if (rev && arith) CT_LAUNCH(true, true);
  else if (rev) CT_LAUNCH(true, false);
  else if (arith) CT_LAUNCH(false, true);
  else TORCH_CHECK(false, "coupling_tail: nothing to do");
#undef CT_LAUNCH
}

static void check_bf16_rows(const torch::Tensor& t, long B, long F, long C,
                            const char* what) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
              t.scalar_type() == at::kBFloat16 && t.dim() == 3 &&
              t.size(0) == B && t.size(1) == F && t.size(2) == C,
              what, " must be contiguous bf16 [B,F,", C, "]");
}

// flow_split_rev: xc [B,F,C] -> the (x0, x1) halves of flip(xc, -1), each
// contiguous [B,F,C/2]
std::vector<torch::Tensor> flow_split_rev(torch::Tensor xc) {
  TORCH_CHECK(xc.dim() == 3 && xc.size(2) % 16 == 0,
              "flow_split_rev: C % 16 != 0");
  const long B = xc.size(0), F = xc.size(1), C = xc.size(2), half = C / 2;
  check_bf16_rows(xc, B, F, C, "flow_split_rev: xc");
  auto x0 = torch::empty({B, F, half}, xc.options());
  auto x1 = torch::empty({B, F, half}, xc.options());
  const bf16* p = (const bf16*)xc.data_ptr();
  coupling_launch(true, false, p, p + half, nullptr, nullptr,
                  (bf16*)x0.data_ptr(), (bf16*)x1.data_ptr(), B * F, half, C,
                  half);
  return {x0, x1};
}

// coupling_tail: (x0, x1, post, mc) -> last == false: the next flow's
// (x0, x1), flipped; last == true: {cat(x0, x1_new)} as one [B,F,C]
std::vector<torch::Tensor> coupling_tail(torch::Tensor x0, torch::Tensor x1,
                                         torch::Tensor post, torch::Tensor mc,
                                         bool last) {
  TORCH_CHECK(x0.dim() == 3 && x0.size(2) % 8 == 0,
              "coupling_tail: half % 8 != 0");
  const long B = x0.size(0), F = x0.size(1), half = x0.size(2);
  check_bf16_rows(x0, B, F, half, "coupling_tail: x0");
  check_bf16_rows(x1, B, F, half, "coupling_tail: x1");
  check_bf16_rows(post, B, F, half, "coupling_tail: post");
  TORCH_CHECK(mc.is_cuda() && mc.is_contiguous() && mc.numel() == B * F &&
              mc.scalar_type() == at::kBFloat16, "coupling_tail: mc");
  if (last) {
    auto xc = torch::empty({B, F, 2 * half}, x0.options());
    bf16* o = (bf16*)xc.data_ptr();
    coupling_launch(false, true, (const bf16*)x0.data_ptr(),
                    (const bf16*)x1.data_ptr(), (const bf16*)post.data_ptr(),
                    (const bf16*)mc.data_ptr(), o, o + half, B * F, half,
                    half, 2 * half);
    return {xc};
  }
  auto n0 = torch::empty_like(x0);
  auto n1 = torch::empty_like(x1);
  coupling_launch(true, true, (const bf16*)x0.data_ptr(),
                  (const bf16*)x1.data_ptr(), (const bf16*)post.data_ptr(),
                  (const bf16*)mc.data_ptr(), (bf16*)n0.data_ptr(),
                  (bf16*)n1.data_ptr(), B * F, half, half, half);
  return {n0, n1};
}

// ------------------------------------------------------------------------- //
// DDS layer of the duration predictor in two kernels (bf16, channel-last,
// one wave per row, C <= 512).  Each restates the eager chain
//   x*m -> depthwise_cl -> row_ln_cl -> gelu   and   row_ln_cl -> gelu -> add
// with the SAME expressions as depthwise_cl_kernel / row_ln_cl_kernel (lane
// mapping c = lane + 64*i, the two butterflies, the tap order) and ATen's
// erf GELU, rounding to bf16 wherever the chain stored a bf16 tensor.
// ------------------------------------------------------------------------- //

// row_ln_cl_kernel's arithmetic on a row already in registers: v[i] holds
// channel lane + 64*i (0 past C); on return v[i] = bf16(LN) as f32
__device__ __forceinline__ void row_ln_regs(float* v, int C, int lane,
                                            const float* __restrict__ gamma,
                                            const float* __restrict__ beta,
                                            float eps) {
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) sum += v[i];
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) sum += __shfl_xor(sum, sh, 64);
  const float mean = sum / C;
  float var = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + i * 64;
    if (c < C) {
      v[i] -= mean;
      var += v[i] * v[i];
    }
  }
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) var += __shfl_xor(var, sh, 64);
  const float inv = rsqrtf(var / C + eps);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + i * 64;
    if (c < C) v[i] = rbf(v[i] * inv * gamma[c] + beta[c]);
  }
}

// ATen's GeluCUDAKernelImpl, approximate == none, on a bf16 value
__device__ __forceinline__ float gelu_erf_bf(float x) {
  constexpr float kAlpha = M_SQRT1_2;
  return rbf(x * 0.5f * (1.0f + erff(x * kAlpha)));
}

// dds_sep_ln_gelu: y = gelu(LN(depthwise_k3(bf16(t*m)))), t = x (+ g).
// With g the kernel also writes t = bf16(x + g), the layer's residual.
template <bool HAS_G>
__global__ void dds_sep_ln_gelu_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ g,
    const bf16* __restrict__ mc, const bf16* __restrict__ w,  // [C][3]
    const float* __restrict__ bias, const float* __restrict__ gamma,
    const float* __restrict__ beta, bf16* __restrict__ y,
    bf16* __restrict__ t_out, long rows, long Tlen, int C, int dil,
    float eps) {
  const long row = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const long b = row / Tlen;
  const long t = row % Tlen;
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + i * 64;
    float acc = 0.f;
    if (c < C) {
      acc = bias ? bias[c] : 0.f;
      for (int j = 0; j < 3; ++j) {
        const long tt = t + (long)(j - 1) * dil;
        if (tt < 0 || tt >= Tlen) continue;
        const long r = b * Tlen + tt;
        float xv = bf2f(x[r * C + c]);
        if (HAS_G) {
          xv = rbf(xv + bf2f(g[r * C + c]));
          if (j == 1) t_out[r * C + c] = f2bf(xv);
        }
        xv = rbf(xv * bf2f(mc[r]));
        acc += xv * bf2f(w[c * 3 + j]);
      }
      acc = rbf(acc);
    }
    v[i] = acc;
  }
  row_ln_regs(v, C, lane, gamma, beta, eps);
  bf16* yr = y + row * C;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + i * 64;
    if (c < C) yr[c] = f2bf(gelu_erf_bf(v[i]));
  }
}

// ln_gelu_add: out = bf16(t + gelu(LN(y))), times m when LAST
template <bool LAST>
__global__ void ln_gelu_add_kernel(const bf16* __restrict__ y,
                                   const bf16* __restrict__ t,
                                   const bf16* __restrict__ mc,
                                   const float* __restrict__ gamma,
                                   const float* __restrict__ beta,
                                   bf16* __restrict__ out, long rows, int C,
                                   float eps) {
  const long row = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const bf16* yr = y + row * C;
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + i * 64;
    v[i] = c < C ? bf2f(yr[c]) : 0.f;
  }
  row_ln_regs(v, C, lane, gamma, beta, eps);
  const float m = LAST ? bf2f(mc[row]) : 1.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + i * 64;
    if (c < C) {
      float o = bf2f(t[row * C + c]) + gelu_erf_bf(v[i]);
      if (LAST) o = rbf(o) * m;
      out[row * C + c] = f2bf(o);
    }
  }
}

// ------------------------------------------------------------------------- //
// spline_tail: the per-element tail of the duration predictor's inverse
// rational-quadratic spline, after the softmax / cumsum / softplus that stay
// in ATen (their reduction order cannot be restated).  One thread per (b,t),
// BINS bins.  Every intermediate the dense ATen form stores as a bf16 tensor
// is rounded to bf16 here, in the same order:
//   knots = (2*tb)*pad(cum) - tb, ends pinned to -tb / +tb; bin widths and
//   heights as knot differences; bin = clamp(#(x >= knot_h) - 1, 0, BINS-1);
//   the gathers; the quadratic root; where(inside, out, inputs).
// ------------------------------------------------------------------------- //
template <int BINS>
__global__ void spline_tail_kernel(const bf16* __restrict__ in, long in_bs,
                                   long Tlen, const bf16* __restrict__ cw,
                                   const bf16* __restrict__ ch,
                                   const bf16* __restrict__ dv,
                                   bf16* __restrict__ out, float tb, long n) {
  // No FMA contraction here: the compiler narrows a product of two widened
  // bf16 values to a bf16 multiply (exact) and may then fuse it into the
  // next add across the widening, which drops the bf16 rounding of the
  // product that the eager chain performs.
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bf16 raw = in[(i / Tlen) * in_bs + (i % Tlen)];
  const float xin = bf2f(raw);
  const bool inside = (xin >= -tb) && (xin <= tb);
  // clamp as ATen does it: a NaN stays a NaN
  const float x = xin < -tb ? -tb : (xin > tb ? tb : xin);
  const float two_tb = 2.f * tb;
  auto knot = [&](const bf16* cum, int k) -> float {
#pragma clang fp contract(off)
    if (k == 0) return -tb;
    if (k == BINS) return tb;
    return rbf(rbf(two_tb * bf2f(cum[k - 1])) - tb);
  };
  const bf16* cwr = cw + i * BINS;
  const bf16* chr = ch + i * BINS;
  const bf16* dvr = dv + i * (BINS + 1);
  int bin = -1;
#pragma unroll
  for (int k = 0; k <= BINS; ++k) bin += (x >= knot(chr, k)) ? 1 : 0;
  bin = bin < 0 ? 0 : (bin > BINS - 1 ? BINS - 1 : bin);
  const float in_cw = knot(cwr, bin);
  const float in_w = rbf(knot(cwr, bin + 1) - in_cw);
  const float in_ch = knot(chr, bin);
  const float in_h = rbf(knot(chr, bin + 1) - in_ch);
  const float delta = rbf(in_h / in_w);
  const float d0 = bf2f(dvr[bin]);
  const float d1 = bf2f(dvr[bin + 1]);
  // s = in_deriv + in_deriv_p1 - 2*delta
  const float s = rbf(rbf(d0 + d1) - rbf(2.f * delta));
  const float xm = rbf(x - in_ch);
  const float xs = rbf(xm * s);
  const float a = rbf(xs + rbf(in_h * rbf(delta - d0)));
  const float bq = rbf(rbf(in_h * d0) - xs);
  const float c = rbf(-delta * xm);
  float disc = rbf(rbf(bq * bq) - rbf(rbf(4.f * a) * c));
  disc = disc < 0.f ? 0.f : disc;  // clamp_min: a NaN stays a NaN
  const float root = rbf(rbf(2.f * c) / rbf(-bq - rbf(sqrtf(disc))));
  const float o = rbf(root * in_w) + in_cw;
  out[i] = inside ? f2bf(o) : raw;
}

torch::Tensor spline_tail(torch::Tensor inputs, torch::Tensor cumwidths,
                          torch::Tensor cumheights, torch::Tensor derivatives,
                          double tail_bound) {
  // inputs [B,1,T] (any batch stride); cumwidths, cumheights [B,1,T,10] =
  // cumsum of the affine-mapped softmax; derivatives [B,1,T,11] =
  // min_derivative + softplus(padded ud).  Returns contiguous [B,1,T].
  constexpr int BINS = 10;
  TORCH_CHECK(inputs.is_cuda() && inputs.scalar_type() == at::kBFloat16 &&
              inputs.dim() == 3 && inputs.size(1) == 1 &&
              (inputs.size(2) == 1 || inputs.stride(2) == 1),
              "spline_tail: inputs must be bf16 [B,1,T], unit time stride");
  const long B = inputs.size(0), T = inputs.size(2), n = B * T;
  auto chk = [&](const torch::Tensor& t, long last, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
                t.is_contiguous() && t.dim() == 4 && t.size(0) == B &&
                t.size(1) == 1 && t.size(2) == T && t.size(3) == last,
                "spline_tail: ", what, " must be contiguous bf16 [B,1,T,",
                last, "]");
  };
  chk(cumwidths, BINS, "cumwidths");
  chk(cumheights, BINS, "cumheights");
  chk(derivatives, BINS + 1, "derivatives");
  const float tb = (float)tail_bound;
  TORCH_CHECK(tb > 0.f && (double)(float)c10::BFloat16(tb) == tail_bound,
              "spline_tail: tail_bound must be exact in bf16");
  auto out = torch::empty({B, 1, T}, inputs.options());
  if (!n) return out;
  const int threads = 64;  // n is a few thousand: spread over the CUs
  hipLaunchKernelGGL((spline_tail_kernel<BINS>),
                     dim3((unsigned)((n + threads - 1) / threads)),
                     dim3(threads), 0, cur_stream(),
                     (const bf16*)inputs.data_ptr(),
                     B > 1 ? inputs.stride(0) : T, T,
                     (const bf16*)cumwidths.data_ptr(),
                     (const bf16*)cumheights.data_ptr(),
                     (const bf16*)derivatives.data_ptr(),
                     (bf16*)out.data_ptr(), tb, n);
  return out;
}

static const float* f32_vec(const torch::Tensor& t, long C, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
              t.is_contiguous() && t.numel() == C, what,
              " must be a contiguous f32 [C] device tensor");
  return t.data_ptr<float>();
}

std::vector<torch::Tensor> dds_sep_ln_gelu(
    torch::Tensor x, c10::optional<torch::Tensor> g, torch::Tensor mc,
    torch::Tensor w, torch::Tensor bias, torch::Tensor gamma,
    torch::Tensor beta, long dil, double eps) {
  // x [B,T,C] (+ g [B,T,C]); mc [B,T,1]; w [C,1,3] bf16; bias, gamma, beta
  // f32 [C].  Returns {y} or, with g, {y, t = x + g}.
  TORCH_CHECK(x.dim() == 3, "dds_sep_ln_gelu: x must be [B,T,C]");
  const long B = x.size(0), T = x.size(1), C = x.size(2);
  TORCH_CHECK(C <= 512, "dds_sep_ln_gelu: C too large");
  TORCH_CHECK(dil >= 1, "dds_sep_ln_gelu: dilation");
  check_bf16_rows(x, B, T, C, "dds_sep_ln_gelu: x");
  TORCH_CHECK(mc.is_cuda() && mc.is_contiguous() && mc.numel() == B * T &&
              mc.scalar_type() == at::kBFloat16, "dds_sep_ln_gelu: mc");
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kBFloat16 &&
              w.numel() == C * 3, "dds_sep_ln_gelu: w must be bf16 [C,1,3]");
  auto w2 = w.reshape({C, 3}).contiguous();
  const float* bp = f32_vec(bias, C, "dds_sep_ln_gelu: bias");
  const float* gp = f32_vec(gamma, C, "dds_sep_ln_gelu: gamma");
  const float* btp = f32_vec(beta, C, "dds_sep_ln_gelu: beta");
  auto y = torch::empty_like(x);
  const long rows = B * T;
  const int wpb = 4;
  const dim3 grid((unsigned)((rows + wpb - 1) / wpb));
  if (g.has_value()) {
    check_bf16_rows(*g, B, T, C, "dds_sep_ln_gelu: g");
    auto t_out = torch::empty_like(x);
    if (rows)
      hipLaunchKernelGGL((dds_sep_ln_gelu_kernel<true>), grid, dim3(64 * wpb),
                         0, cur_stream(), (const bf16*)x.data_ptr(),
                         (const bf16*)g->data_ptr(),
                         (const bf16*)mc.data_ptr(),
                         (const bf16*)w2.data_ptr(), bp, gp, btp,
                         (bf16*)y.data_ptr(), (bf16*)t_out.data_ptr(), rows,
                         T, (int)C, (int)dil, (float)eps);
    return {y, t_out};
  }
  if (rows)
    hipLaunchKernelGGL((dds_sep_ln_gelu_kernel<false>), grid, dim3(64 * wpb),
                       0, cur_stream(), (const bf16*)x.data_ptr(),
                       (const bf16*)nullptr, (const bf16*)mc.data_ptr(),
                       (const bf16*)w2.data_ptr(), bp, gp, btp,
                       (bf16*)y.data_ptr(), (bf16*)nullptr, rows, T, (int)C,
                       (int)dil, (float)eps);
  return {y};
}

torch::Tensor ln_gelu_add(torch::Tensor y, torch::Tensor t, torch::Tensor mc,
                          torch::Tensor gamma, torch::Tensor beta,
                          bool last, double eps) {
  TORCH_CHECK(y.dim() == 3, "ln_gelu_add: y must be [B,T,C]");
  const long B = y.size(0), T = y.size(1), C = y.size(2);
  TORCH_CHECK(C <= 512, "ln_gelu_add: C too large");
  check_bf16_rows(y, B, T, C, "ln_gelu_add: y");
  check_bf16_rows(t, B, T, C, "ln_gelu_add: t");
  TORCH_CHECK(mc.is_cuda() && mc.is_contiguous() && mc.numel() == B * T &&
              mc.scalar_type() == at::kBFloat16, "ln_gelu_add: mc");
  const float* gp = f32_vec(gamma, C, "ln_gelu_add: gamma");
  const float* btp = f32_vec(beta, C, "ln_gelu_add: beta");
  auto out = torch::empty_like(y);
  const long rows = B * T;
  if (!rows) return out;
  const int wpb = 4;
  const dim3 grid((unsigned)((rows + wpb - 1) / wpb));
#define LGA_LAUNCH(L)                                                      \
  hipLaunchKernelGGL((ln_gelu_add_kernel<L>), grid, dim3(64 * wpb), 0,     \
                     cur_stream(), (const bf16*)y.data_ptr(),              \
                     (const bf16*)t.data_ptr(), (const bf16*)mc.data_ptr(), \
                     gp, btp, (bf16*)out.data_ptr(), rows, (int)C,         \
                     (float)eps)
  if (last) LGA_LAUNCH(true);
  else LGA_LAUNCH(false);
#undef LGA_LAUNCH
  return out;
}

// ------------------------------------------------------------------------- //
// Per-row synthesis scales: one batch, a noise_scale / length_scale /
// noise_w per request.  The scales stay f32 [B] on the device end to end: a
// bf16 tensor of scales would round 0.8 to 0.80078 before the multiply, and
// the scalar path multiplies by (float)0.8 in f32 and rounds the product
// once.  Each kernel is bit-identical to its scalar counterpart run on that
// row alone with the scalar scales[b].
// ------------------------------------------------------------------------- //

// the rounding an eager tensor of dtype T puts between two ops
template <typename T> __device__ __forceinline__ float rnd_t(float v);
template <> __device__ __forceinline__ float rnd_t<float>(float v) { return v; }
template <> __device__ __forceinline__ float rnd_t<bf16>(float v) {
  return rbf(v);
}

// prior_sample_kernel's body, ns read per batch row
template <typename T>
__global__ void prior_sample_rows_kernel(const T* __restrict__ m,
                                         const T* __restrict__ logs,
                                         const T* __restrict__ mask,  // [B,1,T]
                                         const T* __restrict__ noise,
                                         const float* __restrict__ ns_rows,
                                         T* __restrict__ out, long C_T,
                                         long T_len, long ms, long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  long b = i / C_T;
  long t = i % T_len;
  long j = b * ms + (i - b * C_T);
  const float ns = ns_rows[b];
  float msk = ld_f(mask + b * T_len + t);
  float v = ld_f(m + j) + ld_f(noise + i) * __expf(ld_f(logs + j)) * ns;
  st_f(out + i, v * msk);
}

torch::Tensor prior_sample_rows(torch::Tensor m, torch::Tensor logs,
                                torch::Tensor mask, torch::Tensor noise,
                                torch::Tensor noise_scale) {
  TORCH_CHECK(m.is_cuda() && m.dim() == 3);
  const long B = m.size(0), C = m.size(1), T = m.size(2);
  auto dense_planes = [&](const torch::Tensor& t) {
    return (T == 1 || t.stride(2) == 1) && (C == 1 || t.stride(1) == T);
  };
  TORCH_CHECK(m.sizes() == logs.sizes() && dense_planes(m) &&
                  dense_planes(logs) &&
                  (B == 1 || m.stride(0) == logs.stride(0)),
              "prior_sample_rows: m/logs planes must be dense, one batch "
              "stride");
  TORCH_CHECK(logs.scalar_type() == m.scalar_type() &&
                  mask.scalar_type() == m.scalar_type() &&
                  noise.scalar_type() == m.scalar_type() && mask.is_cuda() &&
                  noise.is_cuda(),
              "prior_sample_rows: one dtype, one device");
  TORCH_CHECK(noise.is_contiguous() && noise.numel() == B * C * T &&
                  mask.is_contiguous() && mask.numel() == B * T,
              "prior_sample_rows: noise [B,C,T], mask [B,1,T], contiguous");
  const float* nsp = f32_vec(noise_scale, B, "prior_sample_rows: noise_scale");
  const long ms = B > 1 ? m.stride(0) : C * T;
  auto out = torch::empty({B, C, T}, m.options());
  const long n = B * C * T;
  if (!n) return out;
  const int threads = 256;
  DISPATCH_FT(m, "prior_sample_rows", {
    hipLaunchKernelGGL(prior_sample_rows_kernel<scalar_t>,
                       dim3((n + threads - 1) / threads), dim3(threads), 0,
                       cur_stream(), (const scalar_t*)m.data_ptr(),
                       (const scalar_t*)logs.data_ptr(),
                       (const scalar_t*)mask.data_ptr(),
                       (const scalar_t*)noise.data_ptr(), nsp,
                       (scalar_t*)out.data_ptr(), C * T, T, ms, n);
  });
  return out;
}

// scale_mask_rows: z = noise * noise_w[b] * mask, the head of the duration
// predictor's reverse pass.  Two eager multiplies: the product with the f32
// scale is rounded to T once, the mask multiply (0/1, exact) once more; the
// mask is multiplied, never selected, so signed zeros come out as ATen's.
template <typename T>
__global__ void scale_mask_rows_kernel(const T* __restrict__ noise,
                                       const T* __restrict__ mask,  // [B,1,T]
                                       const float* __restrict__ scales,
                                       T* __restrict__ out, long C_T,
                                       long T_len, long n) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long b = i / C_T;
  const long t = i % T_len;
  const float v = rnd_t<T>(ld_f(noise + i) * scales[b]);
  st_f(out + i, v * ld_f(mask + b * T_len + t));
}

torch::Tensor scale_mask_rows(torch::Tensor noise, torch::Tensor mask,
                              torch::Tensor scales) {
  TORCH_CHECK(noise.is_cuda() && noise.dim() == 3 && noise.is_contiguous(),
              "scale_mask_rows: noise must be contiguous [B,C,T]");
  const long B = noise.size(0), C = noise.size(1), T = noise.size(2);
  TORCH_CHECK(mask.is_cuda() && mask.is_contiguous() &&
                  mask.numel() == B * T &&
                  mask.scalar_type() == noise.scalar_type(),
              "scale_mask_rows: mask must be contiguous [B,1,T], noise's dtype");
  const float* sp = f32_vec(scales, B, "scale_mask_rows: scales");
  auto out = torch::empty_like(noise);
  const long n = B * C * T;
  if (!n) return out;
  const int threads = 256;
  DISPATCH_FT(noise, "scale_mask_rows", {
    hipLaunchKernelGGL(scale_mask_rows_kernel<scalar_t>,
                       dim3((n + threads - 1) / threads), dim3(threads), 0,
                       cur_stream(), (const scalar_t*)noise.data_ptr(),
                       (const scalar_t*)mask.data_ptr(), sp,
                       (scalar_t*)out.data_ptr(), C * T, T, n);
  });
  return out;
}

// duration_rows: the eager chain
//   w = exp(logw) * x_mask * length_scale;  w_ceil = ceil(w)
//   y_lengths = clamp_min(sum(w_ceil, [1,2]), 1).long();  durs = int32(w_ceil)
// in one launch, one wave per row.  Every tensor the chain materialises in
// the activation dtype T is rounded to T here too: exp, both products, and
// the row sum (ATen accumulates it in f32 and stores it as T).  w_ceil holds
// integers, so the f32 accumulation is exact in any order below 2^24 frames.
template <typename T>
__global__ void duration_rows_kernel(const T* __restrict__ logw, long logw_bs,
                                     const T* __restrict__ mask,  // [B,1,T]
                                     const float* __restrict__ ls_rows,
                                     int* __restrict__ durs,
                                     long* __restrict__ y_lengths,
                                     long T_len) {
#pragma clang fp contract(off)
  const long b = blockIdx.x;
  const int lane = threadIdx.x;  // one wave per block
  const float ls = ls_rows[b];
  const T* lw = logw + b * logw_bs;
  const T* mk = mask + b * T_len;
  int* dr = durs + b * T_len;
  float acc = 0.f;
  for (long t = lane; t < T_len; t += WAVE) {
    float w = rnd_t<T>(expf(ld_f(lw + t)));
    w = rnd_t<T>(w * ld_f(mk + t));
    w = rnd_t<T>(w * ls);
    w = ceilf(w);
    dr[t] = (int)w;
    acc += w;
  }
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) acc += __shfl_xor(acc, sh, WAVE);
  if (lane == 0) {
    float tot = rnd_t<T>(acc);
    tot = tot < 1.f ? 1.f : tot;  // clamp_min: a NaN stays a NaN
    y_lengths[b] = (long)tot;
  }
}

std::vector<torch::Tensor> duration_rows(torch::Tensor logw,
                                         torch::Tensor x_mask,
                                         torch::Tensor length_scale) {
  // logw [B,1,T] (unit time stride, any batch stride: the narrow of the
  // duration flow's 2-channel state passes as is); x_mask [B,1,T] contiguous
  TORCH_CHECK(logw.is_cuda() && logw.dim() == 3 && logw.size(1) == 1 &&
                  (logw.size(2) == 1 || logw.stride(2) == 1),
              "duration_rows: logw must be [B,1,T], unit time stride");
  const long B = logw.size(0), T = logw.size(2);
  TORCH_CHECK(x_mask.is_cuda() && x_mask.is_contiguous() &&
                  x_mask.numel() == B * T &&
                  x_mask.scalar_type() == logw.scalar_type(),
              "duration_rows: x_mask must be contiguous [B,1,T], logw's dtype");
  const float* lsp = f32_vec(length_scale, B, "duration_rows: length_scale");
  auto durs = torch::empty({B, T}, logw.options().dtype(at::kInt));
  auto y_lengths = torch::empty({B}, logw.options().dtype(at::kLong));
  if (!B) return {durs, y_lengths};
  const long bs = B > 1 ? logw.stride(0) : T;
  DISPATCH_FT(logw, "duration_rows", {
    hipLaunchKernelGGL(duration_rows_kernel<scalar_t>, dim3((unsigned)B),
                       dim3(WAVE), 0, cur_stream(),
                       (const scalar_t*)logw.data_ptr(), bs,
                       (const scalar_t*)x_mask.data_ptr(), lsp,
                       durs.data_ptr<int>(), y_lengths.data_ptr<long>(), T);
  });
  return {durs, y_lengths};
}
