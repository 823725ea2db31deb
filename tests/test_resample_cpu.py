"""Output sample-rate conversion on the host: the filter design, the one-shot
and streaming forms of audio.resample against the dense oracle
(resample_oracle.py), and the option through the synthesizer, the dynamic
batcher and gRPC on the CPU voice."""

import struct

import grpc
import numpy as np
import pytest
import torch

from sonata_amd import ops
from sonata_amd.audio import resample as R
from sonata_amd.audio.samples import to_i16
from sonata_amd.core import Audio, PcmAudio
from sonata_amd.synth.batcher import DynamicBatcher
from sonata_amd.synth.synthesizer import (AudioOutputConfig,
                                          SonataSpeechSynthesizer)
from resample_oracle import (PAIRS, TABLE, bound, dense_oracle,
                             dense_oracle_convolve, run_rows_case)

TEXT = "hˈɛloʊ ðˈɛr. wˈʌn tˈuː θɹˈiː."
ONE = "hˈɛloʊ ðˈɛr ˈɛvɹiwˌʌn."


# --------------------------------- design ----------------------------------- #
@pytest.mark.parametrize("pair", PAIRS)
def test_design_table(pair):
    d = R.design(*pair)
    assert (d.L, d.M, d.K) == TABLE[pair]
    W = max(d.L, d.M)
    assert d.H == R.ZEROS * W and len(d.h) == 2 * d.H + 1
    assert d.h.dtype == np.float64
    assert d.bank.dtype == np.float32 and d.bank.shape == (d.L, d.K)
    pad = np.zeros(d.L * d.K)
    pad[: 2 * d.H + 1] = d.h
    np.testing.assert_array_equal(d.bank,
                                  pad.reshape(d.K, d.L).T.astype(np.float32))
    assert R.design(*pair) is d  # cached per rate pair


def test_largest_bank_is_55_kb():
    assert R.design(22050, 8000).bank.nbytes == 160 * 89 * 4 == 56960


def test_out_len():
    for n, want in [(0, 0), (1, 1), (441, 160), (22050, 8000)]:
        assert R.out_len(n, 22050, 8000) == want
    assert [R.out_len(n, 16000, 48000) for n in (0, 1, 441)] == [0, 3, 1323]
    assert R.out_len(37, 16000, 16000) == R.out_len(37, 16000, None) == 37


def test_rejects():
    # 8003 is coprime to 22050: L = 8003
    with pytest.raises(ValueError, match="1024"):
        R.design(22050, 8003)
    for bad in (3999, 192001, 0):
        with pytest.raises(ValueError, match="4000"):
            R.design(22050, bad)
    R.design(22050, 4000), R.design(16000, 192000)  # the ends are inside


def test_identity_returns_the_same_samples():
    x = np.arange(5, dtype=np.float32)
    for rate in (16000, None):
        y = R.resample_poly(x, 16000, rate)
        assert np.shares_memory(y, x) and y.shape == x.shape
    t = torch.arange(10.0).reshape(2, 5)
    y, lens = ops.resample_rows(t, [5, 3], 16000, None)
    assert y is t and lens.tolist() == [5, 3]


# -------------------------------- accuracy ---------------------------------- #
@pytest.mark.parametrize("pair", [(16000, 8000), (16000, 48000),
                                  (22050, 44100)])
def test_dense_oracle_is_np_convolve(pair):
    x = np.random.default_rng(1).uniform(-1, 1, 61)
    np.testing.assert_allclose(dense_oracle(x, *pair),
                               dense_oracle_convolve(x, *pair),
                               rtol=0, atol=1e-14)


@pytest.mark.parametrize("pair", PAIRS)
def test_resample_poly_within_the_bound(pair):
    d = R.design(*pair)
    rng = np.random.default_rng(2)
    for n in (1, 37, 700):
        x = rng.uniform(-1, 1, n).astype(np.float32)
        y = R.resample_poly(x, *pair)
        assert y.dtype == np.float32 and len(y) == R.out_len(n, *pair)
        err = float(np.abs(y - dense_oracle(x, *pair)).max())
        assert err <= bound(d, float(np.abs(x).max())), err


@pytest.mark.parametrize("pair", [(22050, 8000), (22050, 48000)])
def test_op_fallback_runs_the_shared_cases(pair):
    run_rows_case("cpu", *pair, torch.float32, [0, 37, 300, 301])
    run_rows_case("cpu", *pair, torch.bfloat16, [5, 0, 37, 1])


# --------------------------- frequency response ----------------------------- #
def _level_db(rate_in, rate_out, f):
    n = 4000
    x = np.sin(2 * np.pi * f * np.arange(n) / rate_in).astype(np.float32)
    y = R.resample_poly(x, rate_in, rate_out).astype(np.float64)
    mid = y[len(y) // 4 : len(y) - len(y) // 4]
    rms = np.sqrt(np.mean(mid ** 2))
    return 20 * np.log10(max(rms, 1e-30) / np.sqrt(0.5))


@pytest.mark.parametrize("pair", [(22050, 8000), (22050, 16000),
                                  (16000, 8000)])
def test_frequency_response(pair):
    ny = min(pair) / 2
    for frac in (0.25, 0.75):
        db = _level_db(*pair, frac * ny)
        print(pair, frac, db)
        assert abs(db) <= 0.1
    db = _level_db(*pair, 1.05 * ny)
    print(pair, 1.05, db)
    assert db <= -50.0
    db = _level_db(*pair, 1.3 * ny)
    print(pair, 1.3, db)
    assert db <= -80.0


# ------------------------------ StreamResampler ----------------------------- #
@pytest.mark.parametrize("pair", PAIRS)
def test_stream_resampler_concatenates_to_one_shot(pair):
    sizes = [1, 7, 256, 11520, 3]
    x = np.random.default_rng(3).uniform(-1, 1, sum(sizes)).astype(np.float32)
    rs = R.StreamResampler(*pair)
    chunks, at = [], 0
    for s in sizes:
        chunks.append(rs.push(x[at : at + s]))
        at += s
    # the first sample's look-ahead (H div L >= 16 samples) has not arrived
    assert len(chunks[0]) == 0 and chunks[0].dtype == np.float32
    chunks.append(rs.flush())
    assert len(rs.flush()) == 0
    got = np.concatenate(chunks)
    want = R.resample_poly(x, *pair)
    assert len(got) == len(want) == R.out_len(len(x), *pair)
    assert float(np.abs(got - want).max()) <= 1e-6


def test_stream_resampler_identity_passes_chunks_through():
    rs = R.StreamResampler(16000, None)
    x = np.arange(4, dtype=np.float32)
    np.testing.assert_array_equal(rs.push(x), x)
    assert len(rs.flush()) == 0


# ------------------------------- synthesizer -------------------------------- #
@pytest.fixture(scope="module")
def synth(xlow_voice):
    return SonataSpeechSynthesizer(xlow_voice)


@pytest.fixture(scope="module")
def plain(synth):
    return list(synth.synthesize_parallel(TEXT))


def _close(a, b):
    assert len(a) == len(b)
    assert float(np.abs(np.asarray(a) - np.asarray(b)).max()) <= 1e-6


def test_config_keeps_is_noop(xlow_voice):
    cfg = AudioOutputConfig(sample_rate=8000)
    assert cfg.is_noop and AudioOutputConfig().sample_rate is None
    assert xlow_voice.supports_output_rate
    assert xlow_voice.audio_output_info().sample_rate == 16000


@pytest.mark.parametrize("mode", ["parallel", "lazy"])
def test_synthesizer_8k(synth, plain, mode):
    run = getattr(synth, "synthesize_" + mode)
    got = list(run(TEXT, AudioOutputConfig(sample_rate=8000)))
    assert len(got) == len(plain) == 2
    for g, p in zip(got, plain):
        assert isinstance(g, Audio) and g.info.sample_rate == 8000
        assert len(g.samples) == -(-len(p.samples) // 2)
        _close(g.samples, R.resample_poly(p.samples, 16000, 8000))
    sil = list(run(TEXT, AudioOutputConfig(sample_rate=8000,
                                           appended_silence_ms=100)))
    for s, g in zip(sil, got):
        assert len(s.samples) == len(g.samples) + 800
        assert not s.samples[len(g.samples):].any()
    pcm = list(run(TEXT, AudioOutputConfig(sample_rate=8000,
                                           appended_silence_ms=100), pcm=True))
    for q, s in zip(pcm, sil):
        assert isinstance(q, PcmAudio) and q.info.sample_rate == 8000
        np.testing.assert_array_equal(q.pcm, to_i16(s.samples))


def test_synthesizer_host_prosody_then_rate(synth):
    cfg = AudioOutputConfig(volume=50, sample_rate=8000)
    want = list(synth.synthesize_parallel(TEXT, AudioOutputConfig(volume=50)))
    got = list(synth.synthesize_parallel(TEXT, cfg))
    for g, w in zip(got, want):
        assert g.info.sample_rate == 8000
        _close(g.samples, R.resample_poly(w.samples, 16000, 8000))


def test_synthesize_to_file_header(synth, plain, tmp_path):
    path = str(tmp_path / "out8k.wav")
    audio = synth.synthesize_to_file(path, TEXT,
                                     AudioOutputConfig(sample_rate=8000))
    assert audio.info.sample_rate == 8000
    assert len(audio.samples) == sum(-(-len(p.samples) // 2) for p in plain)
    with open(path, "rb") as f:
        head = f.read(44)
    assert head[:4] == b"RIFF" and struct.unpack("<I", head[24:28])[0] == 8000


@pytest.mark.parametrize("mode", ["chunk", "continuous"])
def test_realtime_chunks_concatenate(xlow_voice, mode):
    s = SonataSpeechSynthesizer(xlow_voice)
    s.stream_prosody = mode
    base = np.concatenate(list(s.synthesize_streamed(ONE)))
    chunks = list(s.synthesize_streamed(ONE,
                                        AudioOutputConfig(sample_rate=8000)))
    assert all(len(c) for c in chunks)  # empty chunks are dropped
    _close(np.concatenate(chunks), R.resample_poly(base, 16000, 8000))
    with_sil = list(s.synthesize_streamed(
        ONE, AudioOutputConfig(sample_rate=8000, appended_silence_ms=100)))
    assert len(with_sil[-1]) == 800 and not with_sil[-1].any()


@pytest.mark.parametrize("rate", [16000, None])
def test_native_rate_changes_nothing(synth, plain, rate):
    cfg = AudioOutputConfig(sample_rate=rate)
    for run in (synth.synthesize_parallel, synth.synthesize_lazy):
        for g, p in zip(run(TEXT, cfg), run(TEXT)):
            assert g.info.sample_rate == 16000
            np.testing.assert_array_equal(g.samples, p.samples)
    for g, p in zip(synth.synthesize_parallel(TEXT, cfg, pcm=True), plain):
        np.testing.assert_array_equal(g.pcm, to_i16(p.samples))
    a = np.concatenate(list(synth.synthesize_streamed(ONE)))
    b = np.concatenate(list(synth.synthesize_streamed(ONE, cfg)))
    np.testing.assert_array_equal(a, b)


def test_unsupported_rate_raises(synth):
    with pytest.raises(ValueError, match="1024"):
        list(synth.synthesize_parallel(TEXT,
                                       AudioOutputConfig(sample_rate=8003)))
    with pytest.raises(ValueError):
        list(synth.synthesize_lazy(TEXT, AudioOutputConfig(sample_rate=100)))


# ------------------------------ voice, batcher ------------------------------ #
def test_speak_batch_mixed_rates(xlow_voice):
    sents = list(xlow_voice.phonemize_text(TEXT)) + [ONE]
    base = xlow_voice.speak_batch(sents)
    got = xlow_voice.speak_batch(sents, sample_rate=[None, 8000, 48000])
    pcm = xlow_voice.speak_batch_pcm(sents, sample_rate=[None, 8000, 48000],
                                     silence_ms=[10, 10, None])
    for g, q, b, rate, sil in zip(got, pcm, base, [16000, 8000, 48000],
                                  [160, 80, 0]):
        assert g.info.sample_rate == q.info.sample_rate == rate
        _close(g.samples, R.resample_poly(b.samples, 16000, rate))
        assert len(q.pcm) == len(g.samples) + sil
        np.testing.assert_array_equal(q.pcm[: len(g.samples)],
                                      to_i16(g.samples))
    assert xlow_voice.audio_output_info().sample_rate == 16000


class _Counting:
    """The voice, with its batch calls counted."""

    def __init__(self, voice):
        self._v = voice
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._v, name)

    def speak_batch(self, *a, **k):
        self.calls.append("speak_batch")
        return self._v.speak_batch(*a, **k)

    def speak_batch_pcm(self, *a, **k):
        self.calls.append("speak_batch_pcm")
        return self._v.speak_batch_pcm(*a, **k)


@pytest.mark.parametrize("pcm", [False, True])
def test_batcher_mixed_rates_share_one_call(xlow_voice, pcm):
    m = _Counting(xlow_voice)
    base = xlow_voice.speak_batch([ONE])[0]
    b = DynamicBatcher(m, max_batch=3, max_wait_ms=2000)
    futures = [b.submit(ONE, pcm=pcm, sample_rate=r)
               for r in (None, 8000, 48000)]
    got = [f.result(timeout=120) for f in futures]
    b.close()
    assert m.calls == ["speak_batch_pcm" if pcm else "speak_batch"]
    for g, rate in zip(got, (16000, 8000, 48000)):
        assert g.info.sample_rate == rate
        n = len(g.pcm) if pcm else len(g.samples)
        assert n == R.out_len(len(base.samples), 16000, rate)
    b2 = DynamicBatcher(m, max_batch=1, max_wait_ms=1)
    with pytest.raises(ValueError, match="1024"):
        b2.submit(ONE, sample_rate=8003)
    b2.close()


# ----------------------------------- gRPC ----------------------------------- #
@pytest.fixture(scope="module")
def running(xlow_voice_path):
    from sonata_amd.frontends.grpc import create_server
    from sonata_amd.frontends.grpc.client import SonataGrpcClient

    server, port, _ = create_server(port=0, device="cpu")
    server.start()
    client = SonataGrpcClient(f"127.0.0.1:{port}")
    yield client, xlow_voice_path
    client.close()
    server.stop(grace=None)


def test_grpc_sample_rate(running):
    from sonata_amd.frontends.grpc.proto import MESSAGES

    client, pack = running
    vid = client.LoadVoice(MESSAGES["VoicePath"](config_path=pack)).voice_id
    args = MESSAGES["SpeechArgs"]
    assert args().SerializeToString() == b""  # unset: serialises as before
    assert args(sample_rate=8000).SerializeToString() == b"\x28\xc0\x3e"

    def utt(**kw):
        return MESSAGES["Utterance"](voice_id=vid, text=TEXT, **kw)

    base = list(client.SynthesizeUtterance(utt()))
    for mode in (0, 1):
        half = list(client.SynthesizeUtterance(
            utt(speech_args=args(sample_rate=8000), synthesis_mode=mode)))
        assert len(half) == len(base) == 2
        for h, b in zip(half, base):
            n = len(b.wav_samples) // 2
            assert len(h.wav_samples) == 2 * -(-n // 2)
    rt = b"".join(c.wav_samples for c in client.SynthesizeUtteranceRealtime(
        utt()))
    rt8 = b"".join(c.wav_samples for c in client.SynthesizeUtteranceRealtime(
        utt(speech_args=args(sample_rate=8000))))
    # one resampler per sentence: each rounds its own length up
    assert len(rt) // 4 <= len(rt8) // 2 <= len(rt) // 4 + 2
    for call in (client.SynthesizeUtterance,
                 client.SynthesizeUtteranceRealtime):
        with pytest.raises(grpc.RpcError) as e:
            list(call(utt(speech_args=args(sample_rate=8003))))
        assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT


# ------------------------------ CLI, pysonata ------------------------------- #
def _wav_rate_and_bytes(data):
    assert data[:4] == b"RIFF"
    return struct.unpack("<I", data[24:28])[0], len(data) - 44


@pytest.mark.parametrize("mode", ["parallel", "lazy", "realtime"])
def test_cli_flag_and_json_key(xlow_voice_path, mode):
    import io
    import json

    from sonata_amd.frontends import cli

    def run(argv, req):
        buf = io.BytesIO()
        rc = cli.main([xlow_voice_path, "--device", "cpu", "-m", mode] + argv,
                      stdin=io.StringIO(json.dumps(req) + "\n"), stdout=buf)
        assert rc == 0
        return _wav_rate_and_bytes(buf.getvalue())

    rate, n = run([], {"text": ONE})
    assert rate == 16000
    by_flag = run(["--sample-rate", "8000"], {"text": ONE})
    by_key = run([], {"text": ONE, "sample_rate": 8000})
    assert by_flag == by_key == (8000, 2 * -(-(n // 2) // 2))


def test_pysonata_config_carries_the_rate(xlow_voice_path):
    from sonata_amd.frontends import pysonata

    cfg = pysonata.AudioOutputConfig(sample_rate=8000)
    assert cfg._to_internal().sample_rate == 8000
    assert pysonata.AudioOutputConfig()._to_internal().sample_rate is None
