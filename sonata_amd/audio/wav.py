"""Minimal RIFF/WAVE writer (16-bit PCM mono/stereo).

Parity: reference crates/audio/ops/src/wave_writer.rs:18-93 (riff-wave).
"""

from __future__ import annotations

import io
import struct

import numpy as np

from .samples import to_i16


def wav_header(data_bytes: int, sample_rate: int, num_channels: int = 1,
               sample_width: int = 2) -> bytes:
    """44-byte RIFF/WAVE header for a PCM payload of `data_bytes`."""
    import struct

    byte_rate = sample_rate * num_channels * sample_width
    block_align = num_channels * sample_width
    return (b"RIFF" + struct.pack("<I", 36 + data_bytes) + b"WAVE"
            + b"fmt " + struct.pack("<IHHIIHH", 16, 1, num_channels,
                                    sample_rate, byte_rate, block_align,
                                    sample_width * 8)
            + b"data" + struct.pack("<I", data_bytes))


def wav_bytes(samples, sample_rate: int, num_channels: int = 1,
              peak_normalize: bool = True) -> bytes:
    return wav_bytes_pcm(to_i16(samples, peak_normalize=peak_normalize),
                         sample_rate, num_channels)


def wav_bytes_pcm(pcm, sample_rate: int, num_channels: int = 1) -> bytes:
    """WAV file bytes for int16 samples that are already PCM (what
    wav_bytes writes for the float samples they came from)."""
    pcm = np.asarray(pcm, dtype=np.int16).reshape(-1).astype("<i2").tobytes()
    byte_rate = sample_rate * num_channels * 2
    block_align = num_channels * 2
    buf = io.BytesIO()
    buf.write(b"RIFF")
    buf.write(struct.pack("<I", 36 + len(pcm)))
    buf.write(b"WAVE")
    buf.write(b"fmt ")
    buf.write(struct.pack("<IHHIIHH", 16, 1, num_channels, sample_rate,
                          byte_rate, block_align, 16))
    buf.write(b"data")
    buf.write(struct.pack("<I", len(pcm)))
    buf.write(pcm)
    return buf.getvalue()


def write_wav_file(path: str, samples, sample_rate: int,
                   num_channels: int = 1) -> None:
    with open(path, "wb") as f:
        f.write(wav_bytes(samples, sample_rate, num_channels))


def write_wav_file_pcm(path: str, pcm, sample_rate: int,
                       num_channels: int = 1) -> None:
    with open(path, "wb") as f:
        f.write(wav_bytes_pcm(pcm, sample_rate, num_channels))


def wav_header_g711(data_bytes: int, sample_rate: int, law: str,
                    num_channels: int = 1) -> bytes:
    """58-byte RIFF/WAVE header for a G.711 payload of `data_bytes`: the
    non-PCM layout, an 18-byte fmt chunk (tag 7 mu-law / 6 A-law, 8 bits,
    cbSize 0) and a fact chunk with the sample count per channel.  The RIFF
    size counts the pad byte an odd payload gets."""
    from .g711 import WAVE_TAG, check_law

    tag = WAVE_TAG[check_law(law)]
    return (b"RIFF" + struct.pack("<I", 50 + data_bytes + (data_bytes & 1))
            + b"WAVE"
            + b"fmt " + struct.pack("<IHHIIHHH", 18, tag, num_channels,
                                    sample_rate, sample_rate * num_channels,
                                    num_channels, 8, 0)
            + b"fact" + struct.pack("<II", 4, data_bytes // num_channels)
            + b"data" + struct.pack("<I", data_bytes))


def wav_bytes_g711(codes, sample_rate: int, law: str,
                   num_channels: int = 1) -> bytes:
    """WAV file bytes for uint8 G.711 codes (audio.g711.encode)."""
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1).tobytes()
    return (wav_header_g711(len(codes), sample_rate, law, num_channels)
            + codes + b"\x00" * (len(codes) & 1))


def write_wav_file_g711(path: str, codes, sample_rate: int, law: str,
                        num_channels: int = 1) -> None:
    with open(path, "wb") as f:
        f.write(wav_bytes_g711(codes, sample_rate, law, num_channels))


def read_wav_file(path: str):
    """Read a 16-bit PCM or 8-bit G.711 (tags 7 and 6, decoded) WAV back to
    float32 in [-1,1]. Test helper."""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:4] == b"RIFF" and data[8:12] == b"WAVE"
    # walk chunks
    pos = 12
    fmt = None
    pcm = None
    while pos + 8 <= len(data):
        cid = data[pos : pos + 4]
        size = struct.unpack("<I", data[pos + 4 : pos + 8])[0]
        body = data[pos + 8 : pos + 8 + size]
        if cid == b"fmt ":
            fmt = struct.unpack("<HHIIHH", body[:16])
        elif cid == b"data":
            pcm = body
        pos += 8 + size + (size & 1)
    assert fmt is not None and pcm is not None
    tag, channels, rate, _, _, bits = fmt
    if tag in (6, 7):
        from .g711 import decode

        assert bits == 8
        x = decode(np.frombuffer(pcm, dtype=np.uint8),
                   "ulaw" if tag == 7 else "alaw")
        return x.astype(np.float32) / 32767.0, rate, channels
    assert bits == 16
    x = np.frombuffer(pcm, dtype="<i2").astype(np.float32) / 32767.0
    return x, rate, channels
