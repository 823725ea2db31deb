"""Host oracle and shared cases for the batched-stream ops (ops.gather_windows,
ops.stream_seam_rows): slicing plus audio.samples.crossfade, nothing else.
Used by test_stream_batch_cpu.py (op fallbacks) and test_gpu_stream_batch.py
(csrc/stream.hip); both compare with assert_array_equal."""

import numpy as np
import torch

from sonata_amd.audio.samples import crossfade

XF = 42

SENTENCES = [
    "ðɪs ɪz ə lˈɔŋ tɛst ʌv ðə stɹˈimɪŋ pˈæθ, wɪθ mˈɛni wˈɝdz.",
    "wˈʌn tˈuː θɹˈiː fˈoːɹ fˈaɪv sˈɪks sˈɛvən ˈeɪt nˈaɪn tˈɛn ɪlˈɛvən twˈɛlv.",
    "hˈɛloʊ.",
    "ðə kwˈɪk bɹˈaʊn fˈɑːks dʒˈʌmps ˈoʊvɚ ðə lˈeɪzi dˈɑːɡ ænd ɹˈʌnz ɐwˈeɪ "
    "fɹʌm ðə fˈɑːɹmɚ.",
]


def bits(t: torch.Tensor) -> np.ndarray:
    """The raw bits of a f32 / bf16 tensor, as a host integer array."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32
                  else torch.int16).numpy()


def _noise(rng, n):
    """Noise with per-sample amplitudes log-uniform over 1e-6 .. 10 (as
    test_gpu_pcm._noise)."""
    amps = (10.0 ** rng.uniform(-6.0, 1.0, n)).astype(np.float32)
    return (amps * rng.standard_normal(n)).astype(np.float32)


# ------------------------------ gather_windows ------------------------------ #
# (src, row, start, length): five windows on the F = 207 source (batch 2),
# one with start + length == F, and the whole F = 28 source
GATHER_ROWS = [(1, 0, 0, 48), (1, 1, 45, 96), (1, 1, 141, 66), (1, 0, 7, 1),
               (1, 1, 13, 35), (0, 0, 0, 28)]
GATHER_LMAX = [96, 101]


def gather_sources(C: int, dtype, seed: int = 0):
    """Two separately allocated sources, [1, C, 28] and [2, C, 207]."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((1, C, 28), generator=g).to(dtype),
            torch.randn((2, C, 207), generator=g).to(dtype)]


def gather_sources_in_canaries(C: int, dtype, seed: int = 0):
    """The same two sources as views into larger buffers filled with 1e3:
    an overread in any direction shows up in the output."""
    out = []
    for z in gather_sources(C, dtype, seed):
        b, _, F = z.shape
        buf = torch.full((b + 2, C + 2, F + 9), 1e3, dtype=dtype)
        buf[1 : 1 + b, 1 : 1 + C, 5 : 5 + F] = z
        out.append(buf)
    return out


def gather_oracle(zs, rows, l_max: int) -> torch.Tensor:
    C = zs[0].shape[1]
    out = torch.zeros((len(rows), C, l_max), dtype=zs[0].dtype)
    for r, (s, b, t0, n) in enumerate(rows):
        out[r, :, :n] = zs[s].cpu()[b, :, t0 : t0 + n]
    return out


# ----------------------------- stream_seam_rows ----------------------------- #
SEAM_N = 101 * 256
SEAM_SLOTS = 8
# lo, hi, ext, prev_ext per row: a first chunk, an interior chunk, a last
# chunk, a one-shot chunk, and a row with lo = 5 and an odd hi
SEAM_ROWS = [
    (0, SEAM_N - 3 * 256, XF, 0),
    (3 * 256, SEAM_N - 3 * 256, XF, XF),
    (3 * 256, SEAM_N, 0, XF),
    (0, SEAM_N, 0, 0),
    (5, 20001, XF, XF),
]
SEAM_SLOT_1 = [3, 0, 6, 1, 4]
SEAM_SLOT_2 = [0, 3, 1, 4, 6]  # second call: reads what the first one left


def seam_inputs(dtype, seed: int):
    """(wav [R, 1, N] in dtype, tails f32 [SEAM_SLOTS, 42])."""
    rng = np.random.default_rng(seed)
    R = len(SEAM_ROWS)
    wav = torch.from_numpy(_noise(rng, R * SEAM_N).reshape(R, 1, SEAM_N))
    tails = torch.from_numpy(
        _noise(rng, SEAM_SLOTS * XF).reshape(SEAM_SLOTS, XF))
    return wav.to(dtype), tails


def seam_oracle(wav, rows, slot, tails):
    """trim_and_emit of VitsVoice._stream_decode, row by row.  wav [R, 1, N]
    or [R, N] (any float dtype, widened as .float() does), tails f32 host
    array [S, 42].  Returns (list of f32 chunks, new tails array)."""
    w = wav.detach().float().cpu().numpy().reshape(wav.shape[0], -1)
    new_tails = np.array(tails, dtype=np.float32, copy=True)
    chunks = []
    for r, (lo, hi, ext, prev_ext) in enumerate(rows):
        cur = w[r, lo : hi + ext]
        if prev_ext:
            cur = crossfade(tails[slot[r]], cur, prev_ext)
        cut = len(cur) - ext
        if ext:
            new_tails[slot[r]] = cur[cut:]
        chunks.append(cur[:cut].astype(np.float32))
    return chunks, new_tails


def check_seam(got, rows, want_chunks, want_tails):
    """got = ops.stream_seam_rows(...) against the oracle, bit for bit."""
    out, out_len, tails_out = got
    assert out.dtype == torch.float32 and out.shape[1] % 8 == 0
    assert out_len.tolist() == [len(c) for c in want_chunks]
    assert out.shape[1] >= max(out_len.tolist())
    o = out.detach().cpu().numpy()
    for r, c in enumerate(want_chunks):
        np.testing.assert_array_equal(o[r, : len(c)].view(np.int32),
                                      c.view(np.int32), err_msg=f"row {r}")
        assert not o[r, len(c):].view(np.int32).any(), f"row {r} padding"
    np.testing.assert_array_equal(
        tails_out.detach().cpu().numpy().view(np.int32),
        want_tails.view(np.int32))


def run_gather_cases(device, C, dtype):
    """Every gather case on `device`; shared by the CPU and the GPU test."""
    from sonata_amd import ops

    src, row, start, length = (list(v) for v in zip(*GATHER_ROWS))
    for l_max in GATHER_LMAX:
        zs = gather_sources(C, dtype)
        want = gather_oracle(zs, GATHER_ROWS, l_max)
        got = ops.gather_windows([z.to(device) for z in zs], src, row, start,
                                 length, l_max)
        assert got.shape == want.shape and got.dtype == dtype
        assert got.device.type == torch.device(device).type
        np.testing.assert_array_equal(bits(got), bits(want))
        for r, n in enumerate(length):  # pad columns: exactly +0
            assert not bits(got)[r, :, n:].any()
        # views into canary-filled buffers: same result, no 1e3 anywhere
        bufs = [b.to(device)
                for b in gather_sources_in_canaries(C, dtype)]
        views = [b[1:-1, 1 : 1 + C, 5:-4] for b in bufs]
        assert [tuple(v.shape) for v in views] == [tuple(z.shape) for z in zs]
        assert not views[1].is_contiguous()
        got = ops.gather_windows(views, src, row, start, length, l_max)
        np.testing.assert_array_equal(bits(got), bits(want))


def run_seam_cases(device, dtype):
    """Two chained seam calls on `device` against the oracle."""
    from sonata_amd import ops
    from sonata_amd.audio.samples import _quarter_sine_ramp

    ramp = torch.from_numpy(_quarter_sine_ramp(XF).copy()).to(device)
    lo, hi, ext, prev_ext = (list(v) for v in zip(*SEAM_ROWS))
    wav1, tails0 = seam_inputs(dtype, 11)
    wav2, _ = seam_inputs(dtype, 12)
    t_host = tails0.numpy()
    t_dev = tails0.to(device)
    for wav, slot in ((wav1, SEAM_SLOT_1), (wav2, SEAM_SLOT_2)):
        assert slot != sorted(slot) and len(slot) < SEAM_SLOTS
        chunks, t_want = seam_oracle(wav, SEAM_ROWS, slot, t_host)
        before = t_dev.clone()
        got = ops.stream_seam_rows(wav.to(device), lo, hi, ext, prev_ext,
                                   slot, t_dev, ramp)
        check_seam(got, SEAM_ROWS, chunks, t_want)
        # the input tails are left alone; unnamed slots carry over
        np.testing.assert_array_equal(bits(t_dev), bits(before))
        unnamed = [s for s in range(SEAM_SLOTS) if s not in slot]
        kept = [s for s, (_, _, e, _) in zip(slot, SEAM_ROWS) if not e]
        assert unnamed and kept
        for s in unnamed + kept:
            np.testing.assert_array_equal(bits(got[2])[s], bits(before)[s])
        changed = [s for s, (_, _, e, _) in zip(slot, SEAM_ROWS) if e]
        assert all((t_want[s] != t_host[s]).any() for s in changed)
        t_host, t_dev = t_want, got[2]
    # in place: tails_out = tails_in gives the same rows and tails
    chunks, t_want = seam_oracle(wav1, SEAM_ROWS, SEAM_SLOT_1, tails0.numpy())
    t_dev = tails0.to(device)
    got = ops.stream_seam_rows(wav1.to(device), lo, hi, ext, prev_ext,
                               SEAM_SLOT_1, t_dev, ramp, tails_out=t_dev)
    assert got[2] is t_dev
    check_seam(got, SEAM_ROWS, chunks, t_want)
