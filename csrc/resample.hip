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

// One output's K products, added in f32 in ascending k: bp = bank + p, xp =
// the staged sample at j.  The one-shot and the streaming kernel share it, so
// a stream's chunks carry the one-shot kernel's bits.
__device__ __forceinline__ float poly_taps(const float* __restrict__ bp,
                                           const float* xp, int K, int L) {
  float acc = 0.f;
#pragma unroll 4
  for (int k = 0; k < K; ++k) acc = fmaf(bp[(long)k * L], xp[-k], acc);
  return acc;
}

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
    acc = poly_taps(bank + p, xs + i0, K, L);
  }
  yr[m] = acc;
}

// --------------------------------------------------------------------------
// resample_poly_stream_rows: one round of the same filter for R realtime
// streams.  A row's logical input is carry[slot] ++ chunk, addressed by its
// global position in the stream; the lengths of a push come from
// audio.resample.PolyStreamPlan.  Grid (tiles of RESAMPLE_TILE outputs, R):
// a tile computes outputs e0 + [c0, c0 + TILE) of its row and stages their
// input span exactly as the one-shot kernel does, taking positions below the
// chunk's start a0 from the carry.
//
// The state is ping-pong, [S][2][Kc]: a push reads buffer `parity` and tile
// 0 of the row writes the new carry, input [keep_pos, a0 + m), to buffer
// 1 - parity.  Several tiles of a row may read the old carry (at 8000 ->
// 192000 four do) and workgroups run in no fixed order, so the buffer that
// is read is never written in the same launch.  Every staged read is
// guarded by the chunk's and the carry's own lengths as well, so no
// parameter row can make the kernel read outside x or the state.
// --------------------------------------------------------------------------
enum {
  PS_SLOT, PS_M, PS_A0, PS_CARRY_POS, PS_CARRY, PS_N, PS_E0, PS_E1,
  PS_FLAGS,  // 1: copy row (no filter, no state)
  PS_KEEP_POS, PS_KEEP, PS_PARITY, PS_PAR
};

__global__ __launch_bounds__(RESAMPLE_TILE) void
resample_poly_stream_rows_kernel(const float* __restrict__ x,
                                 const long* __restrict__ par, float* state,
                                 const float* __restrict__ bank,
                                 float* __restrict__ y, long N, long n_out,
                                 int L, int M, int H, int K, int Kc,
                                 int span_cap) {
  extern __shared__ float xs[];  // logical input [base .. base + span)
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const long* p = par + (long)b * PS_PAR;
  const long c0 = (long)blockIdx.x * RESAMPLE_TILE;
  const long c = c0 + tid;  // column of y
  const float* xr = x + (long)b * N;
  float* yr = y + (long)b * n_out;
  const long m_in = min(max(p[PS_M], 0L), N);
  if (p[PS_FLAGS] & 1) {  // copy row
    if (c < n_out) yr[c] = c < m_in ? xr[c] : 0.f;
    return;
  }
  const long a0 = p[PS_A0], n = p[PS_N];
  const long carry_pos = p[PS_CARRY_POS];
  const long carry_len = min(max(p[PS_CARRY], 0L), (long)Kc);
  const int parity = (int)(p[PS_PARITY] & 1);
  const float* cr = state + ((long)p[PS_SLOT] * 2 + parity) * Kc;
  // logical input at global position q
  auto in = [&](long q) -> float {
    if (q < 0 || q >= n) return 0.f;
    if (q >= a0) return q - a0 < m_in ? xr[q - a0] : 0.f;
    const long i = q - carry_pos;
    return (i >= 0 && i < carry_len) ? cr[i] : 0.f;
  };
  if (blockIdx.x == 0) {  // the new carry, also when nothing is emitted
    float* cw = state + ((long)p[PS_SLOT] * 2 + (1 - parity)) * Kc;
    const long keep_pos = p[PS_KEEP_POS];
    const int keep_len = (int)min(max(p[PS_KEEP], 0L), (long)Kc);
    for (int i = tid; i < keep_len; i += RESAMPLE_TILE)
      cw[i] = in(keep_pos + i);
  }
  const long e0 = p[PS_E0];
  const long n_emit = min(max(p[PS_E1] - e0, 0L), n_out);
  if (c0 >= n_emit) {  // dead tile (uniform over the workgroup)
    if (c < n_out) yr[c] = 0.f;
    return;
  }
  const long m0 = e0 + c0;
  const long m_last = e0 + min(c0 + RESAMPLE_TILE, n_emit) - 1;
  const long j_lo = (m0 * M + H) / L;
  const long j_hi = (m_last * M + H) / L;
  const long base = j_lo - (K - 1);
  // span <= span_cap by the host's bound; the clamp only guards the LDS
  const int span = (int)min(j_hi - base + 1, (long)span_cap);
  for (int i = tid; i < span; i += RESAMPLE_TILE) xs[i] = in(base + i);
  __syncthreads();
  if (c >= n_out) return;
  float acc = 0.f;
  if (c < n_emit) {
    const long t = (e0 + c) * M + H;
    const int ph = (int)(t % L);
    const int i0 = (int)(t / L - base);  // in [K-1, span)
    acc = poly_taps(bank + ph, xs + i0, K, L);
  }
  yr[c] = acc;
}

// ------------------------------ host wrapper --------------------------------
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>
#include <cstring>
#include <vector>

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

// x [R, N] contiguous f32 chunk rows; par: R rows of PS_PAR integers in the
// order of the PS_* indices (audio.resample.PolyPush); state f32 [S, 2, Kc],
// Kc = round_up(K-1, 4): buffer par[PS_PARITY] of the named slot is read,
// the other one written; bank as for resample_poly_rows.  Returns y f32
// [R, n_out], zero past each row's e1 - e0.  The wrapper replays what the
// launch will read; every refusal comes before any launch.
torch::Tensor resample_poly_stream_rows(torch::Tensor x,
                                        std::vector<int64_t> par,
                                        torch::Tensor state,
                                        torch::Tensor bank, long L, long M,
                                        long H, long n_out) {
  TORCH_CHECK(x.dim() == 2 && x.is_cuda() && x.scalar_type() == at::kFloat,
              "resample_poly_stream_rows: x must be a cuda f32 [R, N] tensor");
  TORCH_CHECK(x.is_contiguous(),
              "resample_poly_stream_rows: x must be contiguous");
  const long R = x.size(0), N = x.size(1);
  TORCH_CHECK((long)par.size() == R * PS_PAR,
              "resample_poly_stream_rows: one parameter row per chunk row");
  TORCH_CHECK(L >= 1 && L <= RESAMPLE_MAX_L && M >= 1 && M < INT_MAX &&
                  H >= 0 && H < INT_MAX,
              "resample_poly_stream_rows: need 1 <= L <= ", RESAMPLE_MAX_L,
              ", M >= 1, H >= 0");
  TORCH_CHECK(N < INT_MAX && n_out >= 8 && n_out % 8 == 0 &&
                  n_out < INT_MAX && R < 65536,
              "resample_poly_stream_rows: shape out of range (n_out must be "
              "a multiple of 8, at least 8)");
  const long K = (2 * H + 1 + L - 1) / L;
  const long Kc = (K - 1 + 3) & ~3L;
  TORCH_CHECK(bank.is_cuda() && bank.is_contiguous() &&
                  bank.scalar_type() == at::kFloat && bank.dim() == 1 &&
                  bank.numel() == L * K && bank.device() == x.device(),
              "resample_poly_stream_rows: bank must be a cuda f32 [L*K] "
              "tensor, K = ceil((2H+1)/L) = ", K);
  TORCH_CHECK(state.is_cuda() && state.device() == x.device() &&
                  state.is_contiguous() &&
                  state.scalar_type() == at::kFloat && state.dim() == 3 &&
                  state.size(1) == 2 && state.size(2) == Kc,
              "resample_poly_stream_rows: state must be a cuda f32 [S, 2, ",
              Kc, "] tensor");
  const long S = state.size(0);
  // the worst tile's input span: j(m0 + TILE - 1) - j(m0) + K samples
  const long span_cap = ((RESAMPLE_TILE - 1) * M + L - 1) / L + K;
  TORCH_CHECK(span_cap * (long)sizeof(float) <= RESAMPLE_MAX_LDS,
              "resample_poly_stream_rows: ratio M/L = ", M, "/", L,
              " needs a ", span_cap * sizeof(float),
              "-byte input tile, above ", RESAMPLE_MAX_LDS);
  auto j_of = [&](long m) { return (m * M + H) / L; };
  std::vector<char> named(S, 0);
  for (long r = 0; r < R; ++r) {
    const int64_t* q = par.data() + r * PS_PAR;
    const long slot = q[PS_SLOT], m = q[PS_M], a0 = q[PS_A0];
    const long cpos = q[PS_CARRY_POS], clen = q[PS_CARRY], n = q[PS_N];
    const long e0 = q[PS_E0], e1 = q[PS_E1], flags = q[PS_FLAGS];
    const long keep_pos = q[PS_KEEP_POS], keep = q[PS_KEEP];
    const long parity = q[PS_PARITY];
    TORCH_CHECK(slot >= 0 && slot < S && !named[slot],
                "resample_poly_stream_rows: slot out of range or named twice");
    named[slot] = 1;
    TORCH_CHECK(m >= 0 && m <= N, "resample_poly_stream_rows: row ", r,
                " has m = ", m, " outside [0, N = ", N, "]");
    TORCH_CHECK((flags & ~1L) == 0, "resample_poly_stream_rows: flags");
    TORCH_CHECK(e0 >= 0 && e1 >= e0 && e1 - e0 <= n_out,
                "resample_poly_stream_rows: row ", r, " emits ", e1 - e0,
                " outputs, outside [0, n_out = ", n_out, "]");
    if (flags & 1) {
      TORCH_CHECK(e1 - e0 == m, "resample_poly_stream_rows: copy length");
      continue;
    }
    TORCH_CHECK(a0 >= 0 && n >= 0 && n < INT_MAX && a0 + m <= n,
                "resample_poly_stream_rows: chunk outside the stream");
    // all indices are 64-bit; the largest, e1*M + H, must fit one
    TORCH_CHECK(e1 <= (n * L + M - 1) / M && e1 <= (LONG_MAX - H) / M,
                "resample_poly_stream_rows: output range");
    TORCH_CHECK(parity == 0 || parity == 1,
                "resample_poly_stream_rows: parity");
    TORCH_CHECK(clen >= 0 && clen <= Kc && clen <= K - 1,
                "resample_poly_stream_rows: carry_len ", clen, " above ",
                K - 1);
    TORCH_CHECK(keep >= 0 && keep <= Kc && keep <= K - 1,
                "resample_poly_stream_rows: keep_len ", keep, " above ",
                K - 1);
    TORCH_CHECK(clen == 0 || cpos + clen == a0,
                "resample_poly_stream_rows: carry does not end at the chunk");
    const long in_pos = clen > 0 ? cpos : a0;
    if (e1 > e0) {
      // positions ascend with m: the first output reads the lowest sample,
      // the last one the highest; outside [0, n) the input is zero
      const long lo = std::max(j_of(e0) - (K - 1), 0L);
      const long hi = std::min(j_of(e1 - 1), n - 1);
      TORCH_CHECK(hi < lo || (lo >= in_pos && hi < a0 + m),
                  "resample_poly_stream_rows: row ", r,
                  " reads outside carry ++ chunk");
    }
    TORCH_CHECK(keep == 0 || (keep_pos >= in_pos && keep_pos + keep == a0 + m),
                "resample_poly_stream_rows: new carry outside carry ++ chunk");
  }
  auto y = torch::empty({R, n_out}, x.options());
  if (R == 0) return y;
  auto par_h = torch::empty({R, (long)PS_PAR},
                            torch::TensorOptions().dtype(at::kLong));
  std::memcpy(par_h.data_ptr<long>(), par.data(), par.size() * sizeof(long));
  auto par_d = par_h.to(x.device());
  hipStream_t stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  hipLaunchKernelGGL(resample_poly_stream_rows_kernel,
                     dim3(ceil_div(n_out, RESAMPLE_TILE), R),
                     dim3(RESAMPLE_TILE), span_cap * sizeof(float), stream,
                     x.data_ptr<float>(), par_d.data_ptr<long>(),
                     state.data_ptr<float>(), bank.data_ptr<float>(),
                     y.data_ptr<float>(), N, n_out, (int)L, (int)M, (int)H,
                     (int)K, (int)Kc, (int)span_cap);
  HIP_CHECK(hipGetLastError());
  return y;
}
