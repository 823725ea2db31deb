// Batched output sample-rate conversion: [B, N] f32 / bf16 rows -> f32 rows
// at rate_out, by the polyphase FIR of sonata_amd/audio/resample.py (the
// definition, the CPU path and the semantic reference):
//
//   t = m*M + H,  p = t mod L,  j = t div L
//   y[b][m] = sum_{k < K} bank[k*L + p] * x[b][j-k]     m < out_len[b]
//
// with x zero outside [0, in_len[b]) and y zero at and past out_len[b].
// Each thread adds its K products in f32, in ascending k.
//
// One workgroup computes RESAMPLE_TILE consecutive outputs of one row.  The
// input span they touch, x[j(m0)-(K-1) .. j(m_last)], is staged once in LDS
// (dynamic, sized on the host for the worst tile of the ratio) with zeros
// outside the row, so the tap loop has no bounds test and nothing at or past
// in_len[b] is ever read from memory.
//
// The bank is NOT staged: it is read through the vector cache in the [K][L]
// layout, which is the zero-padded prototype h itself (bank[k*L+p] =
// h[p+k*L]).  A tile of 256 outputs uses 256*K coefficients once each, or
// nearly so (the phases of consecutive outputs step by M mod L, so a tile
// revisits a phase only when L < 256): copying them to LDS first would move
// every coefficient twice for no reuse, and the largest bank (55 KB) would
// cost occupancy.  In [K][L] one tap's coefficients for a wave lie within
// L*4 bytes (640 B for 22050 -> 8000), a handful of cache lines per load, and
// the whole bank stays resident in L2 across the grid.
#include "common.h"

#include <climits>
#include <cstdint>

#define RESAMPLE_TILE 256
#define RESAMPLE_MAX_L 1024
// dynamic LDS a launch may ask for without raising the kernel's limit
#define RESAMPLE_MAX_LDS 65536

template <typename T>
__global__ __launch_bounds__(RESAMPLE_TILE) void resample_poly_rows_kernel(
    const T* __restrict__ x, const int* __restrict__ in_len,
    const int* __restrict__ out_len, const float* __restrict__ bank,
    float* __restrict__ y, long N, long n_out, int L, int M, int H, int K,
    int span_cap) {
  extern __shared__ float xs[];  // x[base .. base + span)
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const long m0 = (long)blockIdx.x * RESAMPLE_TILE;
  const long m = m0 + tid;
  float* yr = y + (long)b * n_out;
  const long n_o = min(max((long)out_len[b], 0L), n_out);
  if (m0 >= n_o) {  // dead tile (uniform over the workgroup): padding is zero
    if (m < n_out) yr[m] = 0.f;
    return;
  }
  const long n_i = min(max((long)in_len[b], 0L), N);
  const long m_last = min(m0 + RESAMPLE_TILE, n_o) - 1;
  const long j_lo = (m0 * M + H) / L;
  const long j_hi = (m_last * M + H) / L;
  const long base = j_lo - (K - 1);
  // span <= span_cap by the host's bound; the clamp only guards the LDS
  const int span = (int)min(j_hi - base + 1, (long)span_cap);
  const T* xr = x + (long)b * N;
  for (int i = tid; i < span; i += RESAMPLE_TILE) {
    const long jj = base + i;
    xs[i] = (jj >= 0 && jj < n_i) ? ld_f<T>(xr + jj) : 0.f;
  }
  __syncthreads();
  if (m >= n_out) return;
  float acc = 0.f;
  if (m < n_o) {
    const long t = m * M + H;
    const int p = (int)(t % L);
    const int i0 = (int)(t / L - base);  // in [K-1, span)
    const float* bp = bank + p;
    const float* xp = xs + i0;
#pragma unroll 4
    for (int k = 0; k < K; ++k) acc = fmaf(bp[(long)k * L], xp[-k], acc);
  }
  yr[m] = acc;
}

// ------------------------------ host wrapper --------------------------------
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

long resample_tile() { return RESAMPLE_TILE; }

// x [B, N] contiguous f32 or bf16, in_len / out_len int32 [B] on the device,
// bank f32 [L*K] on the device in the [K][L] layout, K = ceil((2H+1)/L).
// Returns y f32 [B, n_out].  Every refusal comes before any launch.
torch::Tensor resample_poly_rows(torch::Tensor x, torch::Tensor in_len,
                                 torch::Tensor out_len, torch::Tensor bank,
                                 long L, long M, long H, long n_out) {
  TORCH_CHECK(x.dim() == 2 && x.is_cuda() &&
                  (x.scalar_type() == at::kFloat ||
                   x.scalar_type() == at::kBFloat16),
              "resample_poly_rows: x must be a cuda f32 or bf16 [B, N] tensor");
  TORCH_CHECK(x.is_contiguous(), "resample_poly_rows: x must be contiguous");
  const long B = x.size(0), N = x.size(1);
  TORCH_CHECK(L >= 1 && L <= RESAMPLE_MAX_L && M >= 1 && M < INT_MAX && H >= 0,
              "resample_poly_rows: need 1 <= L <= ", RESAMPLE_MAX_L,
              ", M >= 1, H >= 0");
  // all indices are 64-bit; the largest, m*M + H, must fit one
  TORCH_CHECK(N < INT_MAX && n_out >= 0 && n_out < INT_MAX && B < 65536 &&
                  H < INT_MAX && n_out <= (LONG_MAX - H) / M,
              "resample_poly_rows: shape out of range");
  const long K = (2 * H + 1 + L - 1) / L;
  TORCH_CHECK(bank.is_cuda() && bank.is_contiguous() &&
                  bank.scalar_type() == at::kFloat && bank.dim() == 1 &&
                  bank.numel() == L * K && bank.device() == x.device(),
              "resample_poly_rows: bank must be a cuda f32 [L*K] tensor, K = "
              "ceil((2H+1)/L) = ", K);
  for (const torch::Tensor* t : {&in_len, &out_len})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                    t->scalar_type() == at::kInt && t->dim() == 1 &&
                    t->size(0) == B && t->device() == x.device(),
                "resample_poly_rows: in_len and out_len must be cuda int32 "
                "[B] tensors");
  // the worst tile's input span: j(m0 + TILE - 1) - j(m0) + K samples
  const long span_cap = ((RESAMPLE_TILE - 1) * M + L - 1) / L + K;
  TORCH_CHECK(span_cap * (long)sizeof(float) <= RESAMPLE_MAX_LDS,
              "resample_poly_rows: ratio M/L = ", M, "/", L,
              " needs a ", span_cap * sizeof(float),
              "-byte input tile, above ", RESAMPLE_MAX_LDS);
  if (B > 0) {
    // the lengths decide what is read as data: check them on the host
    const auto li = in_len.cpu(), lo = out_len.cpu();
    const int* pi = li.data_ptr<int>();
    const int* po = lo.data_ptr<int>();
    for (long b = 0; b < B; ++b) {
      TORCH_CHECK(pi[b] >= 0 && pi[b] <= N, "resample_poly_rows: in_len[", b,
                  "] = ", pi[b], " outside [0, N = ", N, "]");
      const long want = ((long)pi[b] * L + M - 1) / M;
      TORCH_CHECK(po[b] == want, "resample_poly_rows: out_len[", b, "] = ",
                  po[b], ", expected ceil(in_len*L/M) = ", want);
      TORCH_CHECK(po[b] <= n_out, "resample_poly_rows: out_len[", b, "] = ",
                  po[b], " above n_out = ", n_out);
    }
  }
  auto y = torch::empty({B, n_out}, x.options().dtype(at::kFloat));
  if (B == 0 || n_out == 0) return y;
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  DISPATCH_FT_CONV(x, {
    hipLaunchKernelGGL(resample_poly_rows_kernel<scalar_t>,
                       dim3(ceil_div(n_out, RESAMPLE_TILE), B),
                       dim3(RESAMPLE_TILE), span_cap * sizeof(float), stream,
                       reinterpret_cast<const scalar_t*>(x.data_ptr()),
                       in_len.data_ptr<int>(), out_len.data_ptr<int>(),
                       bank.data_ptr<float>(), y.data_ptr<float>(), N, n_out,
                       (int)L, (int)M, (int)H, (int)K, (int)span_cap);
  });
  HIP_CHECK(hipGetLastError());
  return y;
}
