"""Dense float64 oracle and shared cases for output sample-rate conversion
(audio.resample, ops.resample_rows).  Used by test_resample_cpu.py (the host
functions and the op's fallback) and test_gpu_resample.py (csrc/resample.hip).

The oracle knows nothing of phases: zero-stuff the input by L, convolve with
the filter, take every M-th sample from offset H.  The filter is the one the
bank holds, h rounded to float32 (that rounding is part of the definition),
taken in float64.  `np.convolve` on the stuffed signal needs len(x)*L*(2H+1)
products, a minute for a 355-sample row at 22050 -> 48000, so `dense_oracle`
forms the same convolution by adding x[i]*h at offset i*L, the terms
np.convolve would multiply by a stuffed zero left out;
`dense_oracle_convolve` is the literal form, and the CPU suite holds the two
together on rows small enough for it.

The bound is derived, not tuned: a float32 sum of K products errs by at most
K * 2^-23 * S * max|x| with S = max_p sum_k |bank[p][k]| (1.87-1.97 here;
2e-5 for 22050 -> 8000), computed from the bank."""

import numpy as np
import torch

from sonata_amd import ops
from sonata_amd.audio import resample as R

PAIRS = [(22050, 8000), (22050, 48000), (22050, 16000), (16000, 8000),
         (16000, 48000), (22050, 44100)]
# rate_in, rate_out -> L, M, K
TABLE = {(22050, 8000): (160, 441, 89), (22050, 48000): (320, 147, 33),
         (22050, 16000): (320, 441, 45), (16000, 8000): (1, 2, 65),
         (16000, 48000): (3, 1, 33), (22050, 44100): (2, 1, 33)}


def filter_f64(d) -> np.ndarray:
    """The 2H+1 taps the bank holds, as float64."""
    flat = np.ascontiguousarray(d.bank.T).reshape(-1)  # [K][L] is h, padded
    return flat[: 2 * d.H + 1].astype(np.float64)


def dense_oracle(x, rate_in: int, rate_out: int) -> np.ndarray:
    d = R.design(rate_in, rate_out)
    x = np.asarray(x, dtype=np.float64)
    n_out = -(-len(x) * d.L // d.M)
    h = filter_f64(d)
    full = np.zeros(len(x) * d.L + len(h) + d.M, dtype=np.float64)
    for i in np.flatnonzero(x):
        full[i * d.L : i * d.L + len(h)] += x[i] * h
    return full[d.H :: d.M][:n_out]


def dense_oracle_convolve(x, rate_in: int, rate_out: int) -> np.ndarray:
    d = R.design(rate_in, rate_out)
    x = np.asarray(x, dtype=np.float64)
    n_out = -(-len(x) * d.L // d.M)
    up = np.zeros(len(x) * d.L + d.M, dtype=np.float64)
    up[: len(x) * d.L : d.L] = x
    return np.convolve(up, filter_f64(d))[d.H :: d.M][:n_out]


def bound(d, peak: float) -> float:
    S = float(np.abs(d.bank.astype(np.float64)).sum(axis=1).max())
    return d.K * 2.0 ** -23 * S * peak


def in_len_for(target: int, rate_in: int, rate_out: int) -> int:
    """The shortest input whose output has `target` samples; where the
    ratio steps over `target` (up-sampling), the next length it reaches."""
    n = 0
    while R.out_len(n, rate_in, rate_out) < target:
        n += 1
    return n


def ragged_batches(tile: int, rate_in: int, rate_out: int):
    """Input lengths of two B = 4 batches.  Output lengths: 0, a row
    shorter than one phase (n = 37), exactly one tile, one tile + 1; then
    three tiles + 5 beside three shorter rows.  A length the ratio steps
    over is replaced by its neighbour (255 for 256 at 22050 -> 48000)."""
    f = lambda t: in_len_for(t, rate_in, rate_out)  # noqa: E731
    # one tile, or the longest row within it where no length gives `tile`
    full = f(tile + 1) - 1
    return [[0, 37, full, f(tile + 1)],
            [f(3 * tile + 5), 37, f(tile + 1), 1]]


def run_rows_case(device, rate_in: int, rate_out: int, dtype, lens,
                  seed: int = 0):
    """ops.resample_rows on rows of `lens` samples inside a wider tensor
    whose every other element is NaN: finite, within the bound of the
    oracle, zero past out_len."""
    d = R.design(rate_in, rate_out)
    rng = np.random.default_rng(seed)
    B, N = len(lens), max(lens) + 19
    x = torch.full((B, N), float("nan"), dtype=torch.float32)
    for b, n in enumerate(lens):
        x[b, :n] = torch.from_numpy(
            rng.uniform(-1.0, 1.0, n).astype(np.float32))
    x = x.to(dtype)  # bf16: the oracle takes the rounded values
    y, out_lengths = ops.resample_rows(x.to(device), lens, rate_in, rate_out)
    want_len = [R.out_len(n, rate_in, rate_out) for n in lens]
    assert out_lengths.tolist() == want_len
    assert y.dtype == torch.float32 and tuple(y.shape) == (B, max(want_len))
    y = y.cpu().numpy()
    assert np.isfinite(y).all()
    xf = x.float().numpy()
    worst = 0.0
    for b, n in enumerate(lens):
        ref = dense_oracle(xf[b, :n], rate_in, rate_out)
        peak = float(np.abs(xf[b, :n]).max()) if n else 0.0
        err = float(np.abs(y[b, : want_len[b]] - ref).max()) if n else 0.0
        tol = bound(d, peak)
        print(f"{rate_in}->{rate_out} {dtype} row {b} n={n} "
              f"out={want_len[b]} err={err:.3e} bound={tol:.3e}")
        assert err <= tol, (b, err, tol)
        assert not y[b, want_len[b]:].any(), "padding is zero"
        worst = max(worst, err)
    return worst


def impulse_expected(d, n: int, j: int) -> np.ndarray:
    """Outputs for a row of n zeros with 1.0 at j: output m is tap
    m*M + H - j*L of the float32 filter, one exact product."""
    flat = np.ascontiguousarray(d.bank.T).reshape(-1)
    n_out = -(-n * d.L // d.M)
    idx = np.arange(n_out, dtype=np.int64) * d.M + d.H - j * d.L
    ok = (idx >= 0) & (idx <= 2 * d.H)
    out = np.zeros(n_out, dtype=np.float32)
    out[ok] = flat[idx[ok]]
    return out
