"""csrc/resample.hip on the GPU: ops.resample_rows against the dense float64
oracle within the derived bound (resample_oracle.py), unit impulses bit for
bit against the bank, the binding's refusals, and the option through
speak_batch / speak_batch_pcm, where the same kernel on the same input must
give the same bits."""

import numpy as np
import pytest
import torch

from sonata_amd import ops
from sonata_amd.audio import resample as R
from resample_oracle import impulse_expected, ragged_batches, run_rows_case
from stream_oracle import SENTENCES

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _tile():
    return ops.hip_ext(required=True).RESAMPLE_TILE


def test_tile_constant_matches_the_kernel():
    from sonata_amd.ops.functional import RESAMPLE_TILE

    assert _tile() == RESAMPLE_TILE


# M > L with the largest bank, L > M, L = 1, M = 1
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("pair", [(22050, 8000), (22050, 48000),
                                  (16000, 8000), (22050, 44100)])
def test_resample_rows_within_the_bound(pair, dtype):
    tile = _tile()
    first, second = ragged_batches(tile, *pair)
    out = [R.out_len(n, *pair) for n in first + second]
    # 22050 -> 48000 steps from 255 to 257, 22050 -> 44100 gives even lengths
    assert out[0] == 0 and 0 < out[1] < tile and out[2] in (tile - 1, tile)
    assert out[3] in (tile + 1, tile + 2)
    assert out[4] in (3 * tile + 5, 3 * tile + 6)
    run_rows_case(DEV, *pair, dtype, first, seed=1)
    run_rows_case(DEV, *pair, dtype, second, seed=2)


@pytest.mark.parametrize("pair", [(22050, 8000), (22050, 48000)])
def test_unit_impulse_is_the_bank_bit_for_bit(pair):
    d = R.design(*pair)
    n = 700
    rows = [0, n // 2, n - 1]
    x = torch.zeros((len(rows), n))
    for b, j in enumerate(rows):
        x[b, j] = 1.0
    y, out_lengths = ops.resample_rows(x.to(DEV), [n] * len(rows), *pair)
    y = y.cpu().numpy()
    for b, j in enumerate(rows):
        want = impulse_expected(d, n, j)
        assert int(out_lengths[b]) == len(want)
        assert np.count_nonzero(want) >= d.H // d.M // 2  # it reaches H/M
        np.testing.assert_array_equal(y[b, : len(want)], want)


def test_binding_refusals_launch_nothing():
    ext = ops.hip_ext(required=True)
    d = R.design(22050, 8000)
    bank = torch.from_numpy(
        np.ascontiguousarray(d.bank.T).reshape(-1).copy()).to(DEV)
    x = torch.zeros((2, 441), device=DEV)
    i32 = lambda v, dev=DEV: torch.tensor(v, dtype=torch.int32,  # noqa: E731
                                          device=dev)
    good = dict(x=x, in_len=i32([441, 37]), out_len=i32([160, 14]), bank=bank,
                L=d.L, M=d.M, H=d.H, n_out=160)
    y = ext.resample_poly_rows(**good)
    assert tuple(y.shape) == (2, 160)
    torch.cuda.synchronize()
    bad = [
        (dict(x=x.cpu()), "cuda"),
        (dict(in_len=good["in_len"].cpu()), "cuda int32"),
        (dict(bank=bank.cpu()), "bank"),
        (dict(x=torch.zeros((2, 882), device=DEV)[:, ::2]), "contiguous"),
        (dict(in_len=i32([442, 37]), out_len=i32([161, 14]), n_out=161),
         "in_len"),
        (dict(out_len=i32([160, 15])), "out_len"),
        (dict(out_len=i32([159, 14])), "out_len"),
        (dict(bank=bank[:-1].clone()), "bank"),
        (dict(bank=bank.double()), "bank"),
        (dict(L=d.L + 1), "bank"),
        (dict(n_out=2 ** 31), "out of range"),
        (dict(L=2048), "1024"),
    ]
    for change, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            ext.resample_poly_rows(**{**good, **change})
    # nothing was launched and nothing is pending: the device is as it was
    torch.cuda.synchronize()
    assert torch.equal(ext.resample_poly_rows(**good), y)


# ------------------------------- whole voice -------------------------------- #
@pytest.fixture(scope="module")
def voice_path(tmp_path_factory):
    from sonata_amd.models import create_random_voice

    return create_random_voice(str(tmp_path_factory.mktemp("rate_voice")),
                               "xlow_rate", quality="x_low")


@pytest.fixture(scope="module", params=["cpp", "python"])
def gpu_voice(request, voice_path):
    from sonata_amd.models import load_voice

    v = load_voice(voice_path, device=DEV, engine=request.param)
    assert (v._engine is not None) == (request.param == "cpp")
    return v


@pytest.fixture(scope="module")
def plain(gpu_voice):
    return gpu_voice.speak_batch(SENTENCES)


def _rows_on_device(audios):
    lens = [len(a.samples) for a in audios]
    x = np.zeros((len(audios), max(lens)), dtype=np.float32)
    for b, a in enumerate(audios):
        x[b, : lens[b]] = a.samples
    return torch.from_numpy(x).to(DEV), lens


def test_speak_batch_at_8k_is_the_kernel_on_its_own_output(gpu_voice, plain):
    assert gpu_voice.supports_output_rate
    got = gpu_voice.speak_batch(SENTENCES, sample_rate=8000)
    x, lens = _rows_on_device(plain)
    y, out_lengths = ops.resample_rows(x, lens, 16000, 8000)
    y = y.cpu().numpy()
    for b, g in enumerate(got):
        assert g.info.sample_rate == 8000
        assert len(g.samples) == int(out_lengths[b]) == -(-lens[b] // 2)
        np.testing.assert_array_equal(g.samples, y[b, : len(g.samples)])
    assert gpu_voice.audio_output_info().sample_rate == 16000


def test_speak_batch_pcm_at_8k_is_resample_then_pcm(gpu_voice, plain):
    got = gpu_voice.speak_batch_pcm(SENTENCES, sample_rate=8000,
                                    silence_ms=50)
    x, lens = _rows_on_device(plain)
    y, out_lengths = ops.resample_rows(x, lens, 16000, 8000)
    pcm, pcm_lengths = ops.pcm16_rows(y, out_lengths, 400)  # 50 ms at 8 kHz
    pcm = pcm.cpu().numpy()
    for b, g in enumerate(got):
        assert g.info.sample_rate == 8000
        assert len(g.pcm) == int(pcm_lengths[b]) == -(-lens[b] // 2) + 400
        np.testing.assert_array_equal(g.pcm, pcm[b, : len(g.pcm)])


def test_mixed_rates_give_each_row_its_uniform_result(gpu_voice, plain):
    sents = SENTENCES[:3]
    rates = [None, 8000, 48000]
    mixed = gpu_voice.speak_batch(sents, sample_rate=rates)
    mixed_pcm = gpu_voice.speak_batch_pcm(sents, sample_rate=rates,
                                          silence_ms=20)
    for b, rate in enumerate(rates):
        uni = gpu_voice.speak_batch(sents, sample_rate=rate)[b]
        uni_pcm = gpu_voice.speak_batch_pcm(sents, sample_rate=rate,
                                            silence_ms=20)[b]
        assert mixed[b].info.sample_rate == uni.info.sample_rate \
            == mixed_pcm[b].info.sample_rate == (rate or 16000)
        np.testing.assert_array_equal(mixed[b].samples, uni.samples)
        np.testing.assert_array_equal(mixed_pcm[b].pcm, uni_pcm.pcm)


def test_synthesizer_passes_the_rate_to_the_device(gpu_voice, monkeypatch):
    from sonata_amd.synth.synthesizer import (AudioOutputConfig,
                                              SonataSpeechSynthesizer)

    calls = []
    real = ops.resample_rows

    def counted(x, *a, **k):
        calls.append(x.device.type)
        return real(x, *a, **k)

    monkeypatch.setattr(ops, "resample_rows", counted)
    text = "hˈɛloʊ ðˈɛr. wˈʌn tˈuː θɹˈiː."
    sents = list(gpu_voice.phonemize_text(text))
    synth = SonataSpeechSynthesizer(gpu_voice)
    cfg = AudioOutputConfig(volume=50, sample_rate=8000,
                            appended_silence_ms=100)
    triple = [cfg.prosody_triple()] * len(sents)
    want = gpu_voice.speak_batch(sents, prosody=triple, sample_rate=8000)
    want_pcm = gpu_voice.speak_batch_pcm(sents, prosody=triple,
                                         sample_rate=8000, silence_ms=100)
    del calls[:]
    got = list(synth.synthesize_parallel(text, cfg))
    got_pcm = list(synth.synthesize_parallel(text, cfg, pcm=True))
    lazy = list(synth.synthesize_lazy(text, cfg))
    assert calls == ["cuda"] * (2 + len(sents))
    for g, q, z, w, wq in zip(got, got_pcm, lazy, want, want_pcm):
        assert g.info.sample_rate == q.info.sample_rate == 8000
        n = len(w.samples)
        np.testing.assert_array_equal(g.samples[:n], w.samples)
        assert len(g.samples) == len(z.samples) == n + 800
        assert not g.samples[n:].any()
        np.testing.assert_array_equal(q.pcm, wq.pcm)
