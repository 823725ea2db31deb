"""Shared cases for streaming output sample-rate conversion
(audio.resample.PolyStreamPlan / PolyStream, ops.resample_poly_stream_rows):
the rate pairs, the chunkings, and chunk lengths that make a push emit a
given number of outputs.  Used by test_stream_resample_cpu.py and
test_gpu_stream_resample.py."""

import numpy as np

from resample_oracle import PAIRS

from sonata_amd.audio import resample as R

# the six pairs of the one-shot tests, the longest carry (K - 1 = 176) and the
# ratio at which four tiles of a round read one carry
ALL_PAIRS = PAIRS + [(22050, 4000), (8000, 192000)]


def lengths(d):
    return [0, 1, 37, d.K - 1, d.K, 4000]


def chunkings(n: int, K: int, seed: int = 0):
    """Chunk lengths summing to n: a single chunk, all ones, a pattern with
    zero-length chunks and three chunks in a row shorter than K - 1, and a
    random one with lengths 0, 1 and 3 in it."""
    out = [[n], [1] * n if n else [0, 0]]
    short, left = [], n
    for c in (max(K - 2, 1), 0, 3, 1, max(K - 2, 1), K + 5, 0, 700):
        c = min(c, left)
        short.append(c)
        left -= c
    if left:
        short.append(left)
    out.append(short)
    rng = np.random.default_rng(seed + n)
    rand, left = [], n
    while left:
        c = int(rng.choice([0, 1, 3, int(rng.integers(1, 2 * K + 2)),
                            int(rng.integers(1, 1500))]))
        c = min(c, left)
        rand.append(c)
        left -= c
    out.append(rand + [0])
    for sizes in out:
        assert sum(sizes) == n
    return out


def stream_chunks(stream, x, sizes):
    """Push x through `stream` in chunks of `sizes`; the emitted parts."""
    parts, at = [], 0
    for i, c in enumerate(sizes):
        parts.append(stream.push(x[at : at + c], i == len(sizes) - 1))
        at += c
    return parts


def ready(d, A: int) -> int:
    """Outputs complete after A input samples (before the last push)."""
    return max(-(-(A * d.L - d.H) // d.M), 0)


def chunk_emitting(d, seen: int, done: int, target: int, over: bool) -> int:
    """The chunk length after `seen` samples whose push emits `target`
    outputs; where the ratio steps over `target` (up-sampling: one input
    sample completes several outputs), the nearest count below it, or above
    it with `over`."""
    A = seen
    while ready(d, A) - done < target:
        A += 1
    if ready(d, A) - done > target and not over:
        A -= 1
    return A - seen
