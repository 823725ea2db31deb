"""Prosody post-processing: rate / volume / pitch on raw waveforms.

Parity: the reference delegates this to the `sonic` C library
(crates/sonata/synth/src/lib.rs:55-105: sonicCreateStream -> SetSpeed/
SetVolume/SetPitch -> WriteFloat -> Flush -> Read).  Here it is a fresh
CPU implementation: WSOLA time-stretch + linear-interpolation resampling,
which compose to give speed and pitch control with the same parameter
semantics (speed in (0.5, 5.5), volume in (0, 1], pitch in (0.5, 1.5) —
synth/src/lib.rs:13-15).
"""

from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from .window import hann_window


def resample_linear(x: np.ndarray, ratio: float) -> np.ndarray:
    """Resample by `ratio` (output length = len(x)/ratio) with linear interp."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    if x.size == 0 or abs(ratio - 1.0) < 1e-6:
        return x.copy()
    n_out = max(int(round(len(x) / ratio)), 1)
    pos = np.arange(n_out, dtype=np.float64) * (len(x) - 1) / max(n_out - 1, 1)
    i0 = np.floor(pos).astype(np.int64)
    i1 = np.minimum(i0 + 1, len(x) - 1)
    frac = (pos - i0).astype(np.float32)
    return (x[i0] * (1.0 - frac) + x[i1] * frac).astype(np.float32)


def time_stretch_wsola(
    x: np.ndarray,
    speed: float,
    sample_rate: int,
    frame_ms: float = 30.0,
    search_ms: float = 10.0,
) -> np.ndarray:
    """WSOLA time stretch: output duration = input/speed, pitch preserved."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    if x.size == 0 or abs(speed - 1.0) < 1e-3:
        return x.copy()
    frame = max(int(sample_rate * frame_ms / 1000.0), 64)
    half = frame // 2
    frame = half * 2
    search = max(int(sample_rate * search_ms / 1000.0), 16)
    syn_hop = half
    ana_hop = syn_hop * speed

    n_out_frames = max(int((len(x) - frame - search) / ana_hop), 1)
    out = np.zeros(n_out_frames * syn_hop + frame, dtype=np.float32)
    norm = np.zeros_like(out)
    win = hann_window(frame)

    prev_tail = None
    for k in range(n_out_frames):
        target = int(k * ana_hop)
        if prev_tail is not None and search > 1:
            lo = max(target - search, 0)
            hi = min(target + search, len(x) - frame)
            if hi > lo:
                # pick the candidate start maximizing correlation with the
                # previous synthesis frame's tail (natural continuation)
                seg = x[lo : hi + half]
                # vectorized cross-correlation over candidate offsets
                n_cand = hi - lo
                idx = np.arange(half)
                cand = seg[np.arange(n_cand)[:, None] + idx[None, :]]
                scores = cand @ prev_tail
                target = lo + int(np.argmax(scores))
        target = min(max(target, 0), len(x) - frame)
        fr = x[target : target + frame] * win
        pos = k * syn_hop
        out[pos : pos + frame] += fr
        norm[pos : pos + frame] += win
        prev_tail = x[target + syn_hop : target + syn_hop + half]

    nz = norm > 1e-6
    out[nz] /= norm[nz]
    n_expect = int(len(x) / speed)
    return out[:n_expect] if len(out) >= n_expect else out


def apply_prosody(
    samples: np.ndarray,
    sample_rate: int,
    speed: float = 1.0,
    volume: float = 1.0,
    pitch: float = 1.0,
) -> np.ndarray:
    """speed: 1.0 = unchanged, 2.0 = twice as fast (duration halved).
    pitch:  1.0 = unchanged, 2.0 = one octave up (duration preserved).
    volume: linear gain."""
    y = np.asarray(samples, dtype=np.float32).reshape(-1)
    if abs(pitch - 1.0) >= 1e-3:
        # shift pitch: resample by pitch (changes duration), then stretch back
        y = resample_linear(y, pitch)
        y = time_stretch_wsola(y, 1.0 / pitch, sample_rate)
    if abs(speed - 1.0) >= 1e-3:
        y = time_stretch_wsola(y, speed, sample_rate)
    if abs(volume - 1.0) >= 1e-6:
        y = y * np.float32(volume)
    return y


# --------------------------------------------------------------------------- #
# shared length / position arithmetic (used by the batched ops on both
# backends: the HIP kernels take every length from here and never re-derive
# one).  Same expressions, same Python float (double) arithmetic as
# time_stretch_wsola / resample_linear above.
# --------------------------------------------------------------------------- #
def wsola_plan(
    n: int,
    speed: float,
    sample_rate: int,
    frame_ms: float = 30.0,
    search_ms: float = 10.0,
):
    """(frame, half, search, ana_hop, n_frames, n_out) of time_stretch_wsola
    for an n-sample row."""
    frame = max(int(sample_rate * frame_ms / 1000.0), 64)
    half = frame // 2
    frame = half * 2
    search = max(int(sample_rate * search_ms / 1000.0), 16)
    ana_hop = half * speed
    n_frames = max(int((n - frame - search) / ana_hop), 1)
    n_out = min(n_frames * half + frame, int(n / speed))
    return frame, half, search, ana_hop, n_frames, n_out


def resample_out_len(n: int, ratio: float) -> int:
    """Output length of resample_linear for an n-sample row."""
    return max(int(round(n / ratio)), 1)


def wsola_is_passthrough(n: int, speed: float, frame: int) -> bool:
    """Rows the batched entry points copy unchanged: speed ~ 1 (as
    time_stretch_wsola does), empty rows, and rows shorter than one frame
    (where the single-row function has no defined behaviour)."""
    return n == 0 or abs(speed - 1.0) < 1e-3 or n < frame


# --------------------------------------------------------------------------- #
# streaming prosody: the same rate / pitch / volume, fed chunk by chunk.
#
# A stream's plain audio has a length known when the stream opens, so every
# quantity of wsola_plan / resample_out_len is fixed up front and each push
# is pure host arithmetic on those: which frames may run, what is emitted,
# what input is kept for the next push.  The concatenation of everything a
# stream emits equals the one-shot functions above on the concatenated
# input, whatever the chunk sizes (bit for bit in NumPy).  The plan objects
# below hold the arithmetic (the HIP kernels take every length from them and
# re-derive none); StreamProsody runs them in NumPy and is the CPU path and
# the semantic reference.
#
# WSOLA stage, total input n, plan (frame, half, search, ana_hop, K, n_out):
#   frame k (t = int(k*ana_hop)) may run once A >= min(t + search + frame, n)
#   samples arrived (k = 0: min(t + frame, n)): its search window ends at
#   hi = min(t + search, n - frame) and the last candidate reads up to
#   hi - 1 + frame.  Running frame k finalises output [k*half, (k+1)*half);
#   after frame K-1, once all n samples are in, the closing half frame and
#   the zeros up to n_out follow.  Kept between pushes: k_next, the raw
#   second half of the last chosen frame, and the input from
#   keep = max(int(k_next*ana_hop) - search, 0) on.  Frame k_next could not
#   run, so A < t + search + frame and the kept input is shorter than
#   2*search + frame: the existing kernel's seg_cap.  At high speed keep can
#   lie beyond A; nothing is carried then and arriving input is skipped.
#
# Resample stage, n -> n_out: output i reads i0 = floor(pos), i1 =
#   min(i0 + 1, n - 1), pos = i*(n-1)/max(n_out-1, 1) in double, and is
#   emitted once i1 < A.  Kept: the input from floor(pos) of the next output
#   on.  That output was not ready, so floor(pos) + 1 >= A: at most ONE
#   sample is carried.
# --------------------------------------------------------------------------- #
class WsolaPush(NamedTuple):
    """One push of a WSOLA stage.  Positions are global sample indices of
    the stage's input (a0, in_pos, keep_pos) or output (e0, e1)."""

    passthrough: bool  # the stage copies its input
    n: int             # total input length of the stage
    ana_hop: float
    a0: int            # input received before this push
    m: int             # input samples of this push
    in_pos: int        # position of the first sample of carry ++ chunk
    carry_len: int     # carried samples in front of the chunk
    k0: int            # first frame run by this push
    nk: int            # number of frames run
    closing: bool      # emits the closing half frame and the zeros after it
    e0: int            # output emitted before this push
    e1: int            # output emitted after it (out_len = e1 - e0)
    keep_pos: int      # position the next push's logical input starts at
    keep_len: int      # samples carried into the next push


class ResamplePush(NamedTuple):
    """One push of a resample stage (positions as in WsolaPush)."""

    copy: bool
    n: int
    n_out: int
    a0: int
    m: int
    in_pos: int
    carry_len: int
    e0: int
    e1: int
    keep_pos: int
    keep_len: int


RESAMPLE_CARRY = 1  # derived above; the device buffer has this many columns


def wsola_seg_cap(frame: int, search: int) -> int:
    """Bound of a WSOLA stage's carry: one frame's search segment."""
    return 2 * search + frame


class WsolaStreamPlan:
    def __init__(self, n: int, speed: float, sample_rate: int):
        (self.frame, self.half, self.search, self.ana_hop, self.n_frames,
         n_out) = wsola_plan(n, speed, sample_rate)
        self.n = int(n)
        self.passthrough = wsola_is_passthrough(n, speed, self.frame)
        self.n_out = self.n if self.passthrough else n_out
        self.received = 0
        self.k_next = 0
        self.emitted = 0
        self.keep_pos = 0
        self.closed = False

    def push(self, m: int) -> WsolaPush:
        m = int(m)
        a0, a1 = self.received, self.received + m
        assert m >= 0 and a1 <= self.n, "more input than the stage's total"
        carry_len = max(a0 - self.keep_pos, 0)
        in_pos = self.keep_pos if carry_len else a0
        self.received = a1
        e0 = self.emitted
        if self.passthrough:
            self.emitted = self.keep_pos = a1
            return WsolaPush(True, self.n, self.ana_hop, a0, m, a0, 0, 0, 0,
                             False, e0, a1, a1, 0)
        K, n = self.n_frames, self.n
        k0 = k = self.k_next
        while k < K:
            t = int(k * self.ana_hop)
            if a1 < min(t + (self.search if k > 0 else 0) + self.frame, n):
                break
            k += 1
        closing = k == K and a1 == n and not self.closed
        if closing:
            e1 = self.n_out
        elif self.closed:
            e1 = e0
        else:
            e1 = min(k * self.half, self.n_out)
        if k < K:
            keep_pos = max(int(k * self.ana_hop) - self.search, 0)
            keep_len = max(a1 - keep_pos, 0)
            assert keep_len <= wsola_seg_cap(self.frame, self.search)
            assert keep_pos >= in_pos
        else:
            keep_pos, keep_len = n, 0
        self.k_next, self.emitted, self.keep_pos = k, e1, keep_pos
        self.closed = self.closed or closing
        return WsolaPush(False, n, self.ana_hop, a0, m, in_pos, carry_len,
                         k0, k - k0, closing, e0, e1, keep_pos, keep_len)


class ResampleStreamPlan:
    def __init__(self, n: int, ratio: float):
        self.n = int(n)
        self.copy = self.n == 0 or abs(ratio - 1.0) < 1e-6
        self.n_out = self.n if self.copy else resample_out_len(n, ratio)
        self.received = 0
        self.emitted = 0
        self.keep_pos = 0

    def _pos(self, i: int) -> float:
        return i * (self.n - 1) / max(self.n_out - 1, 1)

    def _ready(self, a: int) -> int:
        """Number of outputs whose i1 lies below a."""
        if a >= self.n:
            return self.n_out
        if a <= 1:
            return 0
        # a < n: i1 < a  <=>  floor(pos) <= a - 2  <=>  pos < a - 1
        i = int((a - 1) * max(self.n_out - 1, 1) / (self.n - 1))
        i = min(max(i, 0), self.n_out)
        while i < self.n_out and self._pos(i) < a - 1:
            i += 1
        while i > 0 and not self._pos(i - 1) < a - 1:
            i -= 1
        return i

    def push(self, m: int) -> ResamplePush:
        m = int(m)
        a0, a1 = self.received, self.received + m
        assert m >= 0 and a1 <= self.n, "more input than the stage's total"
        carry_len = max(a0 - self.keep_pos, 0)
        in_pos = self.keep_pos if carry_len else a0
        self.received = a1
        e0 = self.emitted
        if self.copy:
            self.emitted = self.keep_pos = a1
            return ResamplePush(True, self.n, self.n_out, a0, m, a0, 0, e0,
                                a1, a1, 0)
        e1 = self._ready(a1)
        keep_pos = int(self._pos(e1)) if e1 < self.n_out else self.n
        keep_len = max(a1 - keep_pos, 0)
        assert keep_len <= RESAMPLE_CARRY and keep_pos >= in_pos
        self.emitted, self.keep_pos = e1, keep_pos
        return ResamplePush(False, self.n, self.n_out, a0, m, in_pos,
                            carry_len, e0, e1, keep_pos, keep_len)


class StreamPush(NamedTuple):
    """One push through the whole chain; a stage the triple does not use is
    None."""

    resample: Optional[ResamplePush]
    wsola_pitch: Optional[WsolaPush]
    wsola_speed: Optional[WsolaPush]
    out_len: int


class StreamProsodyPlan:
    """Host arithmetic of one stream's prosody chain, composed as in
    apply_prosody: resample by pitch, WSOLA by 1/pitch, WSOLA by speed,
    gain in the last stage that runs.  Each stage's total input is the
    previous stage's total output, so all lengths are fixed here."""

    def __init__(self, n_total: int, sample_rate: int, speed: float = 1.0,
                 volume: float = 1.0, pitch: float = 1.0):
        self.n_total = int(n_total)
        self.sample_rate = int(sample_rate)
        self.do_pitch = abs(pitch - 1.0) >= 1e-3
        self.do_speed = abs(speed - 1.0) >= 1e-3
        self.do_gain = abs(volume - 1.0) >= 1e-6
        self.gain = float(volume) if self.do_gain else 1.0
        self.frame, self.half, self.search = wsola_plan(
            0, 1.0, sample_rate)[:3]
        n = self.n_total
        self.resample = self.wsola_pitch = self.wsola_speed = None
        if self.do_pitch:
            self.resample = ResampleStreamPlan(n, pitch)
            self.wsola_pitch = WsolaStreamPlan(self.resample.n_out,
                                               1.0 / pitch, sample_rate)
            n = self.wsola_pitch.n_out
        if self.do_speed:
            self.wsola_speed = WsolaStreamPlan(n, speed, sample_rate)
            n = self.wsola_speed.n_out
        self.n_out = n
        self.received = 0

    @property
    def is_noop(self) -> bool:
        return not (self.do_pitch or self.do_speed or self.do_gain)

    def push(self, m: int, last: bool = False) -> StreamPush:
        m = int(m)
        self.received += m
        assert self.received <= self.n_total, "more input than announced"
        assert not last or self.received == self.n_total, \
            "last chunk before the announced length"
        rs = wp = ws = None
        if self.do_pitch:
            rs = self.resample.push(m)
            wp = self.wsola_pitch.push(rs.e1 - rs.e0)
            m = wp.e1 - wp.e0
        if self.do_speed:
            ws = self.wsola_speed.push(m)
            m = ws.e1 - ws.e0
        return StreamPush(rs, wp, ws, m)


def _resample_push_np(p: ResamplePush, carry: np.ndarray, chunk: np.ndarray):
    """(output, new carry) of one resample push."""
    if p.copy:
        return chunk.copy(), carry[:0]
    buf = np.concatenate([carry, chunk]) if p.carry_len else chunk
    i = np.arange(p.e0, p.e1, dtype=np.float64)
    pos = i * (p.n - 1) / max(p.n_out - 1, 1)
    i0 = np.floor(pos).astype(np.int64)
    i1 = np.minimum(i0 + 1, p.n - 1)
    frac = (pos - i0).astype(np.float32)
    y = (buf[i0 - p.in_pos] * (1.0 - frac)
         + buf[i1 - p.in_pos] * frac).astype(np.float32)
    keep = buf[p.keep_pos - p.in_pos:] if p.keep_len else buf[:0]
    assert len(keep) == p.keep_len
    return y, keep.copy()


def _wsola_push_np(p: WsolaPush, geom, carry, tail, chunk):
    """(output, new carry, new tail) of one WSOLA push: the frames of
    time_stretch_wsola, operation for operation, on carry ++ chunk."""
    if p.passthrough:
        return chunk.copy(), carry[:0], tail
    frame, half, search = geom
    buf = np.concatenate([carry, chunk]) if p.carry_len else chunk
    org = p.in_pos
    win = hann_window(frame)
    parts = []
    idx = np.arange(half)
    for k in range(p.k0, p.k0 + p.nk):
        target = int(k * p.ana_hop)
        if tail is not None and search > 1:
            lo = max(target - search, 0)
            hi = min(target + search, p.n - frame)
            if hi > lo:
                seg = buf[lo - org: hi + half - org]
                n_cand = hi - lo
                cand = seg[np.arange(n_cand)[:, None] + idx[None, :]]
                scores = cand @ tail
                target = lo + int(np.argmax(scores))
        target = min(max(target, 0), p.n - frame)
        fr = buf[target - org: target + frame - org] * win
        o = np.zeros(half, dtype=np.float32)
        nrm = np.zeros(half, dtype=np.float32)
        if tail is not None:
            o += tail * win[half:]
            nrm += win[half:]
        o += fr[:half]
        nrm += win[:half]
        nz = nrm > 1e-6
        o[nz] /= nrm[nz]
        parts.append(o)
        tail = buf[target + half - org: target + frame - org].copy()
    if p.closing:
        o = np.zeros(half, dtype=np.float32)
        o += tail * win[half:]
        nrm = np.zeros(half, dtype=np.float32)
        nrm += win[half:]
        nz = nrm > 1e-6
        o[nz] /= nrm[nz]
        parts.append(o)
        parts.append(np.zeros(half, dtype=np.float32))
    y = (np.concatenate(parts) if parts
         else np.zeros(0, dtype=np.float32))
    # parts start at output k0*half; [e0, e1) is what this push finalises
    start = p.k0 * half
    y = y[max(p.e0 - start, 0): max(p.e1 - start, 0)]
    assert len(y) == p.e1 - p.e0
    keep = buf[p.keep_pos - org:] if p.keep_len else buf[:0]
    assert len(keep) == p.keep_len
    return y, keep.copy(), tail


class StreamProsody:
    """apply_prosody for a stream of chunks whose total length `n_total` is
    known up front: the concatenation of what push() returns equals
    apply_prosody of the concatenated input (pass-through rules of
    ops.apply_prosody_rows included), whatever the chunk sizes.  A push may
    return an empty array."""

    def __init__(self, n_total: int, sample_rate: int, speed: float = 1.0,
                 volume: float = 1.0, pitch: float = 1.0):
        self.plan = StreamProsodyPlan(n_total, sample_rate, speed, volume,
                                      pitch)
        empty = np.zeros(0, dtype=np.float32)
        self._rs_carry = empty
        self._carry = [empty, empty]
        self._tail = [None, None]

    @property
    def n_out(self) -> int:
        return self.plan.n_out

    def push(self, chunk: np.ndarray, last: bool = False) -> np.ndarray:
        y = np.asarray(chunk, dtype=np.float32).reshape(-1)
        pl = self.plan
        step = pl.push(len(y), last)
        geom = (pl.frame, pl.half, pl.search)
        if step.resample is not None:
            y, self._rs_carry = _resample_push_np(step.resample,
                                                  self._rs_carry, y)
        for i, p in enumerate((step.wsola_pitch, step.wsola_speed)):
            if p is not None:
                y, self._carry[i], self._tail[i] = _wsola_push_np(
                    p, geom, self._carry[i], self._tail[i], y)
        if pl.do_gain:
            y = y * np.float32(pl.gain)
        elif step.resample is None and step.wsola_speed is None:
            y = y.copy()
        assert len(y) == step.out_len
        return y
