"""Output sample-rate conversion: one polyphase Kaiser-windowed-sinc FIR,
defined here for the host and for the device kernel (csrc/resample.hip).

Ratio: g = gcd(rate_in, rate_out), L = rate_out/g, M = rate_in/g,
W = max(L, M).  Prototype, designed in float64 with half length H = ZEROS*W
and 2H+1 taps:

    h[n] = (L*ROLLOFF/W) * sinc(ROLLOFF*(n-H)/W) * kaiser(2H+1, BETA)[n]

Polyphase form: K = ceil((2H+1)/L) taps per phase, bank[p][k] = h[p + k*L]
(zero past the end), stored as float32.  Output sample m of ceil(n*L/M):

    t = m*M + H,  p = t mod L,  j = t div L,
    y[m] = sum_k bank[p][k] * x[j-k]        (x is zero outside [0, n))

which is zero phase: there is no delay to trim.  `resample_poly` (float64
accumulation of the float32 bank, rounded to float32 once) is the semantic
reference and the CPU path; `StreamResampler` is its chunked form and its
chunks concatenate to the one-shot result.  `PolyStreamPlan` / `PolyStream`
are the chunked form for a stream whose total length is known up front: the
plan fixes every length of every push on the host, which is what the device
kernel for batched realtime streams runs on (see the end of this file).
"""

from __future__ import annotations

import functools
import math
from typing import NamedTuple, Optional

import numpy as np

ZEROS = 16
BETA = 8.6
ROLLOFF = 0.9

MIN_RATE = 4000
MAX_RATE = 192000
MAX_L = 1024


class PolyphaseFilter(NamedTuple):
    rate_in: int
    rate_out: int
    L: int
    M: int
    H: int
    K: int
    h: np.ndarray  # float64 [2H+1], the prototype
    bank: np.ndarray  # float32 [L, K], bank[p][k] = h[p + k*L]

    @property
    def lookahead(self) -> int:
        """Input samples past j = m*M div L that output m may still need."""
        return self.H // self.L


def check_rate(rate_in: int, rate_out: int) -> None:
    """Raise ValueError for a pair the filter does not serve."""
    if int(rate_in) != rate_in or int(rate_out) != rate_out or rate_in <= 0:
        raise ValueError(f"sample rates must be positive integers, got "
                         f"{rate_in!r} -> {rate_out!r}")
    if not (MIN_RATE <= rate_out <= MAX_RATE):
        raise ValueError(f"output sample rate {rate_out} outside "
                         f"[{MIN_RATE}, {MAX_RATE}]")
    L = int(rate_out) // math.gcd(int(rate_in), int(rate_out))
    if L > MAX_L:
        raise ValueError(
            f"{rate_in} -> {rate_out} needs {L} filter phases, above the "
            f"limit of {MAX_L}: choose a rate with a larger common divisor")


def is_identity(rate_in: int, rate_out: Optional[int]) -> bool:
    return rate_out is None or int(rate_out) == int(rate_in)


@functools.lru_cache(maxsize=64)
def _design(rate_in: int, rate_out: int) -> PolyphaseFilter:
    check_rate(rate_in, rate_out)
    g = math.gcd(rate_in, rate_out)
    L, M = rate_out // g, rate_in // g
    W = max(L, M)
    H = ZEROS * W
    n = np.arange(2 * H + 1, dtype=np.float64)
    h = ((L * ROLLOFF / W) * np.sinc(ROLLOFF * (n - H) / W)
         * np.kaiser(2 * H + 1, BETA))
    K = -(-(2 * H + 1) // L)
    pad = np.zeros(L * K, dtype=np.float64)
    pad[: 2 * H + 1] = h
    bank = np.ascontiguousarray(pad.reshape(K, L).T.astype(np.float32))
    h.setflags(write=False)
    bank.setflags(write=False)
    return PolyphaseFilter(rate_in, rate_out, L, M, H, K, h, bank)


def design(rate_in: int, rate_out: int) -> PolyphaseFilter:
    """The filter for one rate pair (cached; the arrays are read-only)."""
    return _design(int(rate_in), int(rate_out))


def out_len(n: int, rate_in: int, rate_out: Optional[int]) -> int:
    """Output length for n input samples: ceil(n*L/M)."""
    if is_identity(rate_in, rate_out):
        return int(n)
    d = design(rate_in, rate_out)
    return -(-int(n) * d.L // d.M)


def _outputs(d: PolyphaseFilter, buf: np.ndarray, buf0: int, m0: int,
             m1: int) -> np.ndarray:
    """Outputs [m0, m1) as float64, from `buf` holding x[buf0 : buf0 +
    len(buf)] (x is zero elsewhere).  Taps are added in ascending k."""
    if m1 <= m0:
        return np.zeros(0, dtype=np.float64)
    t = np.arange(m0, m1, dtype=np.int64) * d.M + d.H
    p, j = t % d.L, t // d.L
    lo, hi = int(j[0]) - (d.K - 1), int(j[-1])
    local = np.zeros(hi - lo + 1, dtype=np.float64)
    a, b = max(lo, buf0), min(hi + 1, buf0 + len(buf))
    if b > a:
        local[a - lo : b - lo] = buf[a - buf0 : b - buf0]
    bank = d.bank.astype(np.float64)
    jl = j - lo
    acc = np.zeros(m1 - m0, dtype=np.float64)
    for k in range(d.K):
        acc += bank[p, k] * local[jl - k]
    return acc


def resample_poly(x, rate_in: int, rate_out: Optional[int]) -> np.ndarray:
    """x (1-D) at rate_in -> float32 at rate_out, ceil(n*L/M) samples."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    if is_identity(rate_in, rate_out):
        return x
    d = design(rate_in, rate_out)
    n_out = -(-len(x) * d.L // d.M)
    y = _outputs(d, x.astype(np.float64), 0, 0, n_out)
    return y.astype(np.float32)


class StreamResampler:
    """Chunked resample_poly.  push(chunk) returns the outputs whose
    look-ahead (H div L input samples) has arrived, possibly none; flush()
    returns the rest, with zeros for the input that never came.  The chunks
    concatenate to resample_poly of the concatenated input."""

    def __init__(self, rate_in: int, rate_out: Optional[int]):
        self.rate_in = int(rate_in)
        self.rate_out = self.rate_in if rate_out is None else int(rate_out)
        self._d = (None if is_identity(rate_in, rate_out)
                   else design(self.rate_in, self.rate_out))
        self._buf = np.zeros(0, dtype=np.float64)  # x[_buf0 : _seen]
        self._buf0 = 0
        self._seen = 0  # input samples pushed
        self._done = 0  # output samples returned

    def _emit(self, m1: int) -> np.ndarray:
        d = self._d
        y = _outputs(d, self._buf, self._buf0, self._done, m1)
        self._done = max(self._done, m1)
        # the next output starts K-1 samples before its own j
        keep = max((self._done * d.M + d.H) // d.L - (d.K - 1), self._buf0)
        if keep > self._buf0:
            self._buf = self._buf[keep - self._buf0 :]
            self._buf0 = min(keep, self._seen)
        return y.astype(np.float32)

    def push(self, chunk) -> np.ndarray:
        chunk = np.asarray(chunk, dtype=np.float32).reshape(-1)
        d = self._d
        if d is None:
            return chunk
        self._buf = np.concatenate([self._buf, chunk.astype(np.float64)])
        self._seen += len(chunk)
        # output m is complete once x[j(m)] has arrived: j(m) < seen
        ready = max(-(-(self._seen * d.L - d.H) // d.M), 0)
        return self._emit(max(ready, self._done))

    def flush(self) -> np.ndarray:
        d = self._d
        if d is None:
            return np.zeros(0, dtype=np.float32)
        return self._emit(max(-(-self._seen * d.L // d.M), self._done))


# --------------------------------------------------------------------------- #
# Plan-driven streaming, for a stream whose total input length n is known up
# front (a realtime stream's frames * hop): every length of every push is
# host arithmetic, so the device kernel (csrc/resample.hip,
# resample_poly_stream_rows) needs no sync and no flush round.
#
# After A input samples, output m is ready once x[j(m)] has arrived (j(m) <
# A), so a push emits [done, e1) with
#     e1 = max(min(max(ceil((A*L - H)/M), 0), n_out), done),
# and the last push emits up to n_out = ceil(n*L/M): input past n is zero.
# The next output reads from j(e1) - (K-1) on, so the logical input [keep, A)
# with keep = clamp(j(e1) - (K-1), previous keep, A) is carried over.  j(e1)
# >= A whenever e1 < n_out, and j(n_out) >= n, so the carry never exceeds
# K - 1 samples (and reaches it).
# --------------------------------------------------------------------------- #
class PolyPush(NamedTuple):
    """One push of a PolyStreamPlan, in global positions: the chunk is input
    [a0, a0 + m), the carry read is input [carry_pos, carry_pos + carry_len)
    (carry_pos + carry_len == a0), outputs [e0, e1) are emitted and input
    [keep_pos, keep_pos + keep_len) (ending at a0 + m) is the new carry.
    `parity` names the state buffer that holds the carry read; the new one
    goes to buffer 1 - parity."""

    n: int
    n_out: int
    a0: int
    m: int
    carry_pos: int
    carry_len: int
    e0: int
    e1: int
    keep_pos: int
    keep_len: int
    parity: int


class PolyStreamPlan:
    """The lengths of chunked resample_poly for a stream of `n` input
    samples in all.  push(m, last) advances by one chunk of m samples."""

    def __init__(self, n: int, rate_in: int, rate_out: int):
        assert not is_identity(rate_in, rate_out), "identity needs no plan"
        self.d = design(rate_in, rate_out)
        self.n = int(n)
        assert self.n >= 0
        self.n_out = -(-self.n * self.d.L // self.d.M)
        self.seen = 0  # input samples pushed (A)
        self.done = 0  # output samples emitted
        self.keep = 0  # the carry is input [keep, seen)
        self.parity = 0  # flips on every push
        self.closed = False

    @property
    def carry_cap(self) -> int:
        return self.d.K - 1

    def _j(self, m: int) -> int:
        return (m * self.d.M + self.d.H) // self.d.L

    def push(self, m: int, last: bool = False) -> PolyPush:
        d = self.d
        m = int(m)
        assert m >= 0 and not self.closed, "push after the last chunk"
        a0 = self.seen
        A = a0 + m
        assert A <= self.n, "more input than the plan was opened for"
        e0 = self.done
        if last:
            assert A == self.n, "the chunk lengths must sum to n at last"
            e1 = self.n_out
            self.closed = True
        else:
            ready = max(-(-(A * d.L - d.H) // d.M), 0)
            e1 = max(min(ready, self.n_out), e0)
        carry_pos, carry_len = self.keep, a0 - self.keep
        keep = min(max(self._j(e1) - (d.K - 1), self.keep), A)
        keep_len = A - keep
        assert 0 <= carry_len <= d.K - 1 and 0 <= keep_len <= d.K - 1, \
            "carry above K - 1"
        if e1 > e0:
            # every index the emitted outputs read lies in carry ++ chunk,
            # or outside [0, n)
            lo = max(self._j(e0) - (d.K - 1), 0)
            hi = min(self._j(e1 - 1), self.n - 1)
            assert hi < lo or (lo >= carry_pos and hi < A), \
                "an emitted output reads outside carry ++ chunk"
        parity = self.parity
        self.seen, self.done, self.keep = A, e1, keep
        self.parity ^= 1
        return PolyPush(self.n, self.n_out, a0, m, carry_pos, carry_len, e0,
                        e1, keep, keep_len, parity)


class PolyStream:
    """A PolyStreamPlan plus, for the CPU path, the carry as a NumPy array:
    push(chunk, last) returns float32 outputs (possibly none) that
    concatenate to resample_poly of the whole input, bit for bit.  The
    device path (ops.resample_poly_stream_rows) pushes the plan alone and
    keeps the carry in an ops.PolyStreamState."""

    def __init__(self, n: int, rate_in: int, rate_out: int):
        self.plan = PolyStreamPlan(n, rate_in, rate_out)
        self.rate_in = self.plan.d.rate_in
        self.rate_out = self.plan.d.rate_out
        self._carry = np.zeros(0, dtype=np.float64)

    @property
    def n_out(self) -> int:
        return self.plan.n_out

    def push(self, chunk, last: bool = False) -> np.ndarray:
        chunk = np.asarray(chunk, dtype=np.float32).reshape(-1)
        p = self.plan.push(len(chunk), last)
        assert len(self._carry) == p.carry_len
        buf = np.concatenate([self._carry, chunk.astype(np.float64)])
        y = _outputs(self.plan.d, buf, p.carry_pos, p.e0, p.e1)
        self._carry = buf[p.keep_pos - p.carry_pos :]
        assert len(self._carry) == p.keep_len
        return y.astype(np.float32)
