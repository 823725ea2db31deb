"""G.711 companding (8-bit mu-law / A-law) of int16 PCM, in NumPy.

The CPU path and the semantic reference of the device kernel
(csrc/pcm.hip g711_rows, bit for bit).  The encoders are the Sun/CCITT
g711.c forms (what audioop.lin2ulaw / lin2alaw give at width 2), written in
closed form; with x the int16 sample widened to int32, >> an arithmetic
shift and bitlen(v) = 32 - clz(v):

  mu-law  s = x >> 2;  m = min(|s| + 33, 0x1FFF);  seg = bitlen(m) - 6
          code = ((seg << 4) | ((m >> (seg + 1)) & 0xF)) ^ (s < 0 ? 0x7F : 0xFF)
  A-law   ix = (x < 0 ? ~x : x) >> 4
          c = ix                                     for ix < 16, else
          e = bitlen(ix) - 4;  c = ((ix >> (e - 1)) - 16) + (e << 4)
          c |= 0x80 for x >= 0;  code = c ^ 0x55

The G.711 result of a float row is encode(to_i16(row, peak_normalize), law)
followed by appended silence as ZERO[law] bytes.
"""

from __future__ import annotations

import numpy as np

LAWS = ("ulaw", "alaw")
# code of sample 0: silence and padding
ZERO = {"ulaw": 0xFF, "alaw": 0xD5}
# WAVE format tags
WAVE_TAG = {"ulaw": 7, "alaw": 6}


def check_law(law) -> str:
    """`law` if it names a G.711 law, else ValueError."""
    if law not in LAWS:
        raise ValueError(f"G.711 law must be one of {LAWS}, got {law!r}")
    return law


# wire encodings of a result: 16-bit linear PCM or one of the laws
ENCODINGS = ("pcm16",) + LAWS


def check_encoding(encoding) -> str:
    """The wire encoding `encoding` names (None is "pcm16"), else
    ValueError."""
    if encoding is None:
        return "pcm16"
    if encoding not in ENCODINGS:
        raise ValueError(
            f"encoding must be one of {ENCODINGS}, got {encoding!r}")
    return encoding


def _bitlen(v: np.ndarray) -> np.ndarray:
    """Bit length of int32 v in [1, 2^14): exact through frexp."""
    return np.frexp(v.astype(np.float32))[1].astype(np.int32)


def encode(pcm, law: str) -> np.ndarray:
    """int16 samples -> uint8 G.711 codes."""
    check_law(law)
    x = np.asarray(pcm, dtype=np.int16).reshape(-1).astype(np.int32)
    if law == "ulaw":
        s = x >> 2
        m = np.minimum(np.abs(s) + 33, 0x1FFF)
        seg = _bitlen(m) - 6
        code = ((seg << 4) | ((m >> (seg + 1)) & 0xF)) ^ np.where(
            s < 0, 0x7F, 0xFF)
    else:
        ix = np.where(x < 0, ~x, x) >> 4
        e = _bitlen(ix | 16) - 4  # 1 below 16: the shift stays legal
        c = np.where(ix < 16, ix, ((ix >> (e - 1)) - 16) + (e << 4))
        c = np.where(x >= 0, c | 0x80, c)
        code = c ^ 0x55
    return code.astype(np.uint8)


def decode(codes, law: str) -> np.ndarray:
    """uint8 G.711 codes -> int16 samples (g711.c ulaw2linear /
    alaw2linear)."""
    check_law(law)
    c = np.asarray(codes, dtype=np.uint8).reshape(-1).astype(np.int32)
    if law == "ulaw":
        u = ~c & 0xFF
        t = (((u & 0xF) << 3) + 0x84) << ((u & 0x70) >> 4)
        out = np.where(u & 0x80, 0x84 - t, t - 0x84)
    else:
        a = c ^ 0x55
        seg = (a & 0x70) >> 4
        t = (a & 0xF) << 4
        t = np.where(seg == 0, t + 8,
                     (t + 0x108) << np.maximum(seg - 1, 0))
        out = np.where(a & 0x80, t, -t)
    return out.astype(np.int16)
