"""fp64 references and derived bounds for the batched prosody ops
(csrc/prosody.hip; sonata_amd.ops.resample_linear_rows / wsola_rows /
apply_prosody_rows).  No GPU, NumPy only.  Same derivation style as
tests/kernel_oracle.py: u32 = 2^-24, one headroom factor where stated,
no constant taken from what the kernels were measured to produce.

resample_ref
------------
The op is DEFINED with frac = (float)(pos - i0), pos in double (NumPy and
the kernel agree on this), so the reference evaluates

    y = x0·(1 - frac) + x1·frac

in fp64 with that f32 frac.  An f32 evaluation rounds (1 - frac), two
products and one add: four roundings, each relative to a term of
|x0|(1-f) + |x1|f, hence

    bound = 4·u32·(|x0|(1-f) + |x1|f) + tiny         tiny = smallest
                                                      normal f32

wsola_replay
------------
WSOLA picks, per frame, the candidate whose correlation with the previous
tail is largest.  Near-ties are real (margins below 1 occur on white
noise), so an f32 implementation with another summation order may
legitimately pick another candidate than NumPy's BLAS-ordered matmul, and
every later frame then differs.  The replay therefore FOLLOWS the choices
of the code under test: at frame k the tail comes from targets[k-1], and
the choice c* of frame k is accepted iff it is within rounding of the best:

    s[c]      fp64 score of candidate c
    bound[c]  2·half·u32·Σ_j |x_j·tail_j|      f32 accumulation of `half`
                                                rounded products in any
                                                order; headroom 2
    accept    s[c*] + bound[c*] >= s[best] - bound[best]

Two more rules come from the contract, not from rounding:

  * a frame that is not searched (k = 0, or hi <= lo) must choose
    clamp(t, 0, len-frame), t = int(k·ana_hop) in double;
  * one fixed summation order for every candidate means candidates whose
    windows hold identical data score identically, and np.argmax semantics
    then demand the LOWEST index: c* is rejected when an earlier candidate
    has a bitwise-identical window (all-zero / constant input: only lo).

The output is rebuilt in fp64 from the same targets,

    y = (a·w2 + b·w1)/(w2 + w1)·gain      (divide only where the f32 norm
                                           exceeds 1e-6, as the host does)

with per-element bound 4·u32·(|a|w2 + |b|w1)/norm·|gain| + tiny: two
products, one add, one divide, one gain, FMA contraction allowed.

margin[k] = (s[best] - s[second]) / (bound[best] + bound[second]) says how
decisive frame k is: at margin >= 2 every conforming implementation picks
the same candidate (exact-equality tests assert that precondition).
"""

from __future__ import annotations

from typing import List, NamedTuple

import numpy as np

U32 = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)


# --------------------------------------------------------------------------- #
# resample
# --------------------------------------------------------------------------- #
def resample_ref(x: np.ndarray, n_out: int):
    """(ref fp64 [n_out], bound fp64 [n_out]) of linear resampling an
    f32 row to n_out samples."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n = len(x)
    if n == 0 or n_out == 0:
        return np.zeros(0), np.zeros(0)
    pos = np.arange(n_out, dtype=np.float64) * (n - 1) / max(n_out - 1, 1)
    i0 = np.floor(pos).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    frac = (pos - i0).astype(np.float32).astype(np.float64)
    x64 = x.astype(np.float64)
    ref = x64[i0] * (1.0 - frac) + x64[i1] * frac
    bound = 4 * U32 * (np.abs(x64[i0]) * (1.0 - frac)
                       + np.abs(x64[i1]) * frac) + TINY
    return ref, bound


# --------------------------------------------------------------------------- #
# WSOLA replay
# --------------------------------------------------------------------------- #
class Replay(NamedTuple):
    ref: np.ndarray        # fp64 [n_out] output rebuilt from the targets
    bound: np.ndarray      # fp64 [n_out] allowed |got - ref|
    problems: List[str]    # rejected frames (empty: every choice accepted)
    margin: np.ndarray     # [K] decisiveness of searched frames, inf else
    searched: np.ndarray   # bool [K]
    lo: np.ndarray         # [K] window start of searched frames, -1 else
    hi: np.ndarray         # [K]


def frame_window(k: int, plan, n: int):
    """(t, lo, hi, searched) of frame k — the host's arithmetic."""
    frame, half, search, ana_hop = plan[:4]
    t = int(k * ana_hop)
    if k > 0:
        lo = max(t - search, 0)
        hi = min(t + search, n - frame)
        if hi > lo:
            return t, lo, hi, True
    return t, -1, -1, False


def wsola_replay(x, plan, window, targets, gain: float = 1.0) -> Replay:
    """Judge `targets` (the start of every analysis frame chosen by the
    code under test) and rebuild the output they imply.  plan = (frame,
    half, search, ana_hop, n_frames, n_out) as audio.prosody.wsola_plan
    returns it (tests may lengthen n_frames / n_out by hand)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    x64 = x.astype(np.float64)
    n = len(x)
    frame, half, search, ana_hop, K, n_out = plan
    w = np.asarray(window, dtype=np.float32)
    assert w.shape == (frame,) and n >= frame
    targets = np.asarray(targets).reshape(-1)
    problems: List[str] = []
    margin = np.full(K, np.inf)
    searched = np.zeros(K, dtype=bool)
    los = np.full(K, -1, dtype=np.int64)
    his = np.full(K, -1, dtype=np.int64)
    if len(targets) < K:
        problems.append(f"{len(targets)} targets for {K} frames")
        K = len(targets)

    valid = True  # targets so far index real frames
    for k in range(K):
        tgt = int(targets[k])
        if not 0 <= tgt <= n - frame:
            problems.append(f"frame {k}: target {tgt} outside "
                            f"[0, {n - frame}]")
            valid = False
            break
        t, lo, hi, srch = frame_window(k, plan, n)
        if not srch:
            want = min(max(t, 0), n - frame)
            if tgt != want:
                problems.append(f"frame {k}: unsearched frame chose {tgt}, "
                                f"must be clamp(t)={want}")
            continue
        searched[k], los[k], his[k] = True, lo, hi
        tp = int(targets[k - 1])
        tail = x64[tp + half: tp + frame]
        n_cand = hi - lo
        W = np.lib.stride_tricks.sliding_window_view(
            x64[lo: hi + half], half)[:n_cand]
        s = W @ tail
        b = 2 * half * U32 * (np.abs(W) @ np.abs(tail))
        best = int(np.argmax(s))
        if n_cand > 1:
            rest = np.delete(np.arange(n_cand), best)
            second = int(rest[np.argmax(s[rest])])
            den = b[best] + b[second]
            num = s[best] - s[second]
            margin[k] = num / den if den > 0 else (np.inf if num > 0 else 0.0)
        c = tgt - lo
        if not 0 <= c < n_cand:
            problems.append(f"frame {k}: target {tgt} outside the search "
                            f"window [{lo}, {hi})")
            continue
        if not s[c] + b[c] >= s[best] - b[best]:
            problems.append(
                f"frame {k}: chose {tgt} (score {s[c]:.9g} ± {b[c]:.3g}), "
                f"best {lo + best} scores {s[best]:.9g} ± {b[best]:.3g}")
        elif c > 0 and (W[:c] == W[c]).all(axis=1).any():
            first = int(np.nonzero((W[:c] == W[c]).all(axis=1))[0][0])
            problems.append(
                f"frame {k}: chose {tgt}, but candidate {lo + first} holds "
                f"identical data and the lowest index must win")

    # rebuild the output from the same targets
    w64 = w.astype(np.float64)
    total = K * half + frame
    acc = np.zeros(total)
    mag = np.zeros(total)
    norm32 = np.zeros(total, dtype=np.float32)
    norm = np.zeros(total)
    if valid:
        for k in range(K):
            tgt = int(targets[k])
            p = k * half
            acc[p: p + frame] += x64[tgt: tgt + frame] * w64
            mag[p: p + frame] += np.abs(x64[tgt: tgt + frame]) * w64
            norm32[p: p + frame] += w
            norm[p: p + frame] += w64
    nz = norm32 > np.float32(1e-6)
    div = np.where(nz, norm, 1.0)
    g = float(np.float32(gain))
    ref = acc / div * g
    bound = 4 * U32 * mag / div * abs(g) + TINY
    if n_out > total:  # nothing reaches past the last frame
        ref = np.concatenate([ref, np.zeros(n_out - total)])
        bound = np.concatenate([bound, np.full(n_out - total, TINY)])
    return Replay(ref[:n_out], bound[:n_out], problems, margin[:K],
                  searched[:K], los[:K], his[:K])


def wsola_check(x, plan, window, targets, y, gain: float = 1.0,
                what: str = "") -> Replay:
    """Assert that (y, targets) is an acceptable WSOLA of x under `plan`:
    every frame's choice accepted, y of the planned length and every
    element within bound of the replayed output.  Returns the Replay."""
    rp = wsola_replay(x, plan, window, targets, gain)
    assert not rp.problems, f"{what}: " + "; ".join(rp.problems[:4]) + \
        f" ({len(rp.problems)} problems)"
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    assert y.shape == rp.ref.shape, \
        f"{what}: output length {len(y)} != planned {len(rp.ref)}"
    assert_within(y, rp.ref, rp.bound, what)
    return rp


def assert_within(got, ref, bound, what: str = "") -> None:
    """Every element within its bound (NaN / inf count as failures); names
    the worst element."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    diff = np.abs(got - ref)
    bad = ~(diff <= bound)
    if bad.any():
        excess = np.where(bad, np.nan_to_num(diff - bound, nan=np.inf), 0.0)
        i = int(np.argmax(excess))
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.size} elements out of bound; "
            f"worst at {i}: got {got.flat[i]!r}, ref {ref.flat[i]!r}, "
            f"|diff| {diff.flat[i]:.3e} > bound {bound.flat[i]:.3e}")


# --------------------------------------------------------------------------- #
# instrumented f32 re-statement of audio.prosody.time_stretch_wsola
# --------------------------------------------------------------------------- #
def wsola_f32(x, plan, window, gain: float = 1.0, *, move_target=None,
              tie_last=False, skip_norm=False, window_shift=0,
              drop_lo_clamp=False, cut_at_frames=False, f32_positions=False):
    """time_stretch_wsola restated for an explicit plan, returning
    (y f32, targets).  With no keyword it is the NumPy algorithm operation
    for operation (same matmul, same accumulation); each keyword plants
    one defect the oracle must catch:

      move_target=(k, d)  frame k's choice moved by d samples
      tie_last            last instead of first index on equal scores
      skip_norm           the division by the window sum left out
      window_shift=s      window rolled by s samples
      drop_lo_clamp       the chosen index is added to t - search, the
                          unclamped window start
      cut_at_frames       output cut at K·half+frame instead of n_out
      f32_positions       t = int(f32(k)·f32(ana_hop)) instead of double
    """
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n = len(x)
    frame, half, search, ana_hop, K, n_out = plan
    win = np.asarray(window, dtype=np.float32)
    if window_shift:
        win = np.roll(win, window_shift)
    out = np.zeros(K * half + frame, dtype=np.float32)
    norm = np.zeros_like(out)
    targets = np.full(K, -1, dtype=np.int64)
    prev_tail = None
    for k in range(K):
        if f32_positions:
            target = int(np.float32(k) * np.float32(ana_hop))
        else:
            target = int(k * ana_hop)
        index_from_unclamped_lo = drop_lo_clamp
        if prev_tail is not None and search > 1:
            lo = max(target - search, 0)
            hi = min(target + search, n - frame)
            if hi > lo:
                n_cand = hi - lo
                seg = x[lo: hi + half]
                cand = seg[np.arange(n_cand)[:, None]
                           + np.arange(half)[None, :]]
                scores = cand @ prev_tail
                if tie_last:
                    pick = n_cand - 1 - int(np.argmax(scores[::-1]))
                else:
                    pick = int(np.argmax(scores))
                target = (target - search if index_from_unclamped_lo
                          else lo) + pick
        if move_target is not None and move_target[0] == k:
            target += move_target[1]
        target = min(max(target, 0), n - frame)
        targets[k] = target
        pos = k * half
        out[pos: pos + frame] += x[target: target + frame] * win
        norm[pos: pos + frame] += win
        prev_tail = x[target + half: target + frame]
    if not skip_norm:
        nz = norm > 1e-6
        out[nz] /= norm[nz]
    if not cut_at_frames:
        out = out[:n_out]
    if np.float32(gain) != np.float32(1.0):
        out = out * np.float32(gain)
    return out, targets


# --------------------------------------------------------------------------- #
# shared test inputs (CPU and GPU files use the same ones)
# --------------------------------------------------------------------------- #
def noise(seed: int, n: int) -> np.ndarray:
    return (np.random.default_rng(seed).standard_normal(n) * 0.3) \
        .astype(np.float32)


def voiced(seed: int, n: int, sample_rate: int) -> np.ndarray:
    """Voiced-speech-like: harmonics of a slowly gliding 110-140 Hz pitch
    plus a little noise — periodic, so neighbouring candidates score close
    (the near-tie regime)."""
    t = np.arange(n, dtype=np.float64) / sample_rate
    f0 = 110.0 + 30.0 * np.sin(2 * np.pi * 0.7 * t + seed)
    ph = 2 * np.pi * np.cumsum(f0) / sample_rate
    s = sum(np.sin(h * ph) / h for h in range(1, 9))
    s = 0.2 * s + 0.01 * np.random.default_rng(seed).standard_normal(n)
    return s.astype(np.float32)


# (seed, sample_rate, n, speed): white-noise inputs found by a CPU search
# to have margin >= 2 at every searched frame, so every conforming
# implementation must reproduce NumPy's targets exactly.  The tests assert
# the precondition before they use it.
EXACT_CASES = [
    (0, 16000, 4000, 0.5),
    (0, 16000, 3000, 0.75),
    (0, 16000, 4000, 1.37),
    (0, 16000, 4000, 2.0),
    (1, 16000, 3000, 0.5),
    (0, 22050, 4000, 0.5),
    (0, 22050, 4000, 0.75),
    (0, 22050, 3000, 1.37),
    (1, 22050, 4000, 2.0),
    (2, 22050, 4000, 0.75),
]

SPEEDS = (0.5, 0.75, 1.0, 1.37, 2.0, 5.5)


def matrix_lengths(frame: int, search: int):
    return (frame - 1, frame, frame + search, frame + search + 1, 3 * frame,
            4000, 9001)
