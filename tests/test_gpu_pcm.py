"""csrc/pcm.hip on the GPU against audio.samples.to_i16, bit for bit: the
kernels alone, VitsVoice.speak_batch_pcm on both engines, and the routing
of the synthesizer.  No tolerance anywhere."""

import numpy as np
import pytest
import torch

from sonata_amd import ops
from sonata_amd.audio.samples import generate_silence, merge, to_i16
from sonata_amd.ops.functional import PCM_TILE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTENCES = ["wˈʌn.", "wˈʌn tˈuː θɹˈiː fˈoːɹ.", "hˈɛloʊ ðˈɛr ˈɛvɹiwˌʌn."]


def _amps(rng, n):
    """Per-sample amplitudes log-uniform over 1e-6 .. 10."""
    return (10.0 ** rng.uniform(-6.0, 1.0, n)).astype(np.float32)


def _noise(rng, n):
    return (_amps(rng, n) * rng.standard_normal(n)).astype(np.float32)


def _pcm(x, lens, sil=None, **kw):
    """ops.pcm16_rows on the device for a host [B, N] array."""
    pcm, out = ops.pcm16_rows(torch.from_numpy(np.ascontiguousarray(x))
                              .to(DEV), lens, sil, **kw)
    assert pcm.dtype == torch.int16 and pcm.is_cuda
    return pcm.cpu().numpy(), out.tolist()


def _check_row(got_row, x_row, n, peak_normalize=True, msg=""):
    np.testing.assert_array_equal(
        got_row[:n], to_i16(x_row[:n], peak_normalize), err_msg=msg)
    assert not got_row[n:].any(), msg


def test_tile_constant_matches_the_kernel():
    assert ops.hip_ext(required=True).PCM_TILE == PCM_TILE


@pytest.mark.parametrize("n", [0, 1, 2, 7, 8, 9, 255, 256, 257])
@pytest.mark.parametrize("peak_normalize", [True, False])
def test_single_row_small(n, peak_normalize):
    rng = np.random.default_rng(n)
    x = _noise(rng, n).reshape(1, n)
    got, out = _pcm(x, [n], peak_normalize=peak_normalize)
    assert out == [n] and got.shape[1] >= n
    _check_row(got[0], x[0], n, peak_normalize)
    if n >= 255:  # both signs, clamping (without normalisation) seen
        want = to_i16(x[0], peak_normalize)
        assert (want > 0).any() and (want < 0).any()
        assert peak_normalize or (abs(want.astype(int)) >= 32767).any()


@pytest.mark.parametrize("where", ["first", "middle", "last", "very_last"])
def test_peak_in_each_tile(where):
    n = 3 * PCM_TILE + 5
    rng = np.random.default_rng(7)
    x = np.clip(_noise(rng, n), -8.0, 8.0)
    at = {"first": 11, "middle": PCM_TILE + 123, "last": 3 * PCM_TILE + 1,
          "very_last": n - 1}[where]
    x[at] = -32.0  # 32767/32 is exact in f32: the peak maps to -32767
    got, _ = _pcm(x.reshape(1, n), [n])
    _check_row(got[0], x, n, msg=where)
    assert got[0, at] == -32767 and abs(got[0].astype(int)).max() == 32767


def test_ragged_batch_odd_stride():
    lens = [4097, 1, 1000, 0, 3]
    sil = [0, 5, 0, 7, 1]
    N = 4097
    rng = np.random.default_rng(3)
    x = np.full((len(lens), N), 1e3, dtype=np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = _noise(rng, n)
    for pn in (True, False):
        got, out = _pcm(x, lens, sil, peak_normalize=pn)
        assert out == [n + s for n, s in zip(lens, sil)]
        assert got.shape[1] >= max(out)
        for b, n in enumerate(lens):
            _check_row(got[b], x[b], n, pn, msg=f"row {b}")
    # the binding with an odd output stride as well: every second output
    # row starts off a 16-byte boundary; peaks see nothing of the padding
    ext = ops.hip_ext(required=True)
    xd = torch.from_numpy(x).to(DEV)
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for n_out in (4097, 4105):
        y, peaks = ext.pcm16_rows(xd, ld, n_out, True)
        y, peaks = y.cpu().numpy(), peaks.cpu().numpy()
        assert y.shape == (len(lens), n_out)
        for b, n in enumerate(lens):
            _check_row(y[b], x[b], n, msg=f"n_out {n_out} row {b}")
            want = np.abs(x[b, :n]).max() if n else np.float32(0)
            assert peaks[b] == want, b


def test_peak_threshold_rows():
    tiny = np.float32(1e-8)
    above = np.nextafter(tiny, np.float32(1))
    assert float(tiny) <= 1e-8 < float(above)
    n = 300
    x = np.zeros((4, n), dtype=np.float32)
    x[1, ::3], x[1, 1::3] = tiny, -tiny            # peak exactly f32(1e-8)
    x[2, ::3], x[2, 1::3] = above, -above          # next float: normalised
    x[3] = np.linspace(-0.5, 0.25, n, dtype=np.float32)  # peak is negative
    got, _ = _pcm(x, [n] * 4)
    for b in range(4):
        _check_row(got[b], x[b], n, msg=f"row {b}")
    assert not got[0].any() and not got[1].any()
    # normalised to full scale.  The product x * f32(32767/peak) carries one
    # f32 rounding of the scale and one of the product (1 ulp = 2^-9 at
    # 32767), so to_i16 itself truncates this row's peak to 32766, not
    # 32767; equality with to_i16 above is the check, this is the intent.
    assert got[2].max() == -got[2].min() and got[2].max() in (32766, 32767)
    assert got[3].min() == -32767 and got[3, 0] == -32767
    assert got[3].max() < 32767


def test_fixed_scale_clamps_and_truncates():
    x = np.array([[3, -4, 0.5, 1, -1]], dtype=np.float32)
    got, _ = _pcm(x, [5], peak_normalize=False)
    assert got[0, :5].tolist() == [32767, -32768, 16383, 32767, -32767]
    np.testing.assert_array_equal(got[0, :5], to_i16(x[0], False))


def test_bf16_input_and_channel_view():
    rng = np.random.default_rng(5)
    B, T = 3, 2 * PCM_TILE + 77   # odd row stride in 2-byte elements
    lens = [T, 900, PCM_TILE + 1]
    x = torch.from_numpy(
        np.clip(_noise(rng, B * T), -8, 8).reshape(B, 1, T)).to(DEV)
    xb = x.to(torch.bfloat16)
    view = xb[:, 0, :]
    assert view.data_ptr() == xb.data_ptr()
    pcm, _ = ops.pcm16_rows(view, lens, [0, 3, 0])
    ref = xb.float().cpu().numpy()[:, 0, :]
    got = pcm.cpu().numpy()
    for b, n in enumerate(lens):
        _check_row(got[b], ref[b], n, msg=f"bf16 row {b}")
    # the same through an f32 view of a [B, 1, T] tensor
    pcm32, _ = ops.pcm16_rows(x[:, 0, :], lens)
    ref32 = x.cpu().numpy()[:, 0, :]
    for b, n in enumerate(lens):
        _check_row(pcm32.cpu().numpy()[b], ref32[b], n, msg=f"f32 row {b}")


def test_no_stale_peak_between_calls():
    rng = np.random.default_rng(9)
    n = PCM_TILE + 9
    loud = (5.0 * rng.standard_normal((2, n))).astype(np.float32)
    quiet = (1e-3 * rng.standard_normal((2, n))).astype(np.float32)
    _pcm(loud, [n, n])
    got, _ = _pcm(quiet, [n, n])
    for b in range(2):
        _check_row(got[b], quiet[b], n)
        assert abs(got[b].astype(int)).max() >= 32766  # its own full scale


# ------------------------------ whole voice -------------------------------- #
@pytest.fixture(scope="module", params=["auto", "python"])
def gpu_voice(request, xlow_voice_path):
    from sonata_amd.models import load_voice

    v = load_voice(xlow_voice_path, device=DEV, engine=request.param)
    assert (v._engine is not None) == (request.param == "auto")
    return v


@pytest.mark.parametrize("prosody", [None, (1.3, 0.7, 1.1)])
def test_speak_batch_pcm_equals_host_conversion(gpu_voice, prosody,
                                                monkeypatch):
    monkeypatch.setenv("SONATA_DEVICE_PCM", "1")
    v = gpu_voice
    rows = [prosody] * len(SENTENCES) if prosody else None
    ref = (v.speak_batch(SENTENCES, prosody=rows) if rows
           else v.speak_batch(SENTENCES))
    assert len({len(r.samples) for r in ref}) > 1  # a ragged batch
    sr = v.config.sample_rate
    calls = []
    real = ops.pcm16_rows
    monkeypatch.setattr(ops, "pcm16_rows",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    for silence_ms in (0, 30):
        got = v.speak_batch_pcm(SENTENCES, prosody=rows,
                                silence_ms=silence_ms)
        for g, r in zip(got, ref):
            want = to_i16(merge(r.samples, generate_silence(silence_ms, sr)))
            np.testing.assert_array_equal(g.pcm, want)
            assert g.info == r.info and g.inference_ms > 0
    assert len(calls) == 2  # the kernels produced these


# -------------------------------- routing ---------------------------------- #
def test_synthesizer_routes_pcm_to_the_device(xlow_voice_path, monkeypatch):
    from sonata_amd.core import PcmAudio
    from sonata_amd.models import load_voice
    from sonata_amd.synth.synthesizer import (AudioOutputConfig,
                                              SonataSpeechSynthesizer)

    synth = SonataSpeechSynthesizer(load_voice(xlow_voice_path, device=DEV))
    calls = []
    real = ops.pcm16_rows
    monkeypatch.setattr(ops, "pcm16_rows",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    cfg = AudioOutputConfig(rate=30, volume=60, pitch=60,
                            appended_silence_ms=25)
    text = "wˈʌn tˈuː. θɹˈiː fˈoːɹ fˈaɪv."

    def run():
        out = []
        for mode in (synth.synthesize_parallel, synth.synthesize_lazy):
            for c in (None, cfg):
                got = list(mode(text, c, pcm=True))
                assert all(isinstance(g, PcmAudio) for g in got)
                out.append([g.as_wave_bytes() for g in got])
        return out

    monkeypatch.setenv("SONATA_DEVICE_PCM", "1")
    on = run()
    assert len(calls) == 2 + 4  # parallel: one batch each; lazy: 2 sentences
    del calls[:]
    monkeypatch.setenv("SONATA_DEVICE_PCM", "0")
    off = run()
    assert not calls
    assert on == off
    floats = [[a.as_wave_bytes() for a in mode(text, c)]
              for mode in (synth.synthesize_parallel, synth.synthesize_lazy)
              for c in (None, cfg)]
    assert off == floats
