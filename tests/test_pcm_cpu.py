"""int16 PCM path without a GPU: ops.pcm16_rows on CPU tensors, PcmAudio,
VitsVoice.speak_batch_pcm, the batcher's PCM buckets and the gRPC wire
bytes.  Every comparison is exact equality with audio.samples.to_i16."""

import numpy as np
import pytest
import torch

from sonata_amd import ops
from sonata_amd.audio.samples import generate_silence, merge, to_i16
from sonata_amd.core import Audio, AudioInfo, PcmAudio
from sonata_amd.synth import DynamicBatcher
from sonata_amd.synth.synthesizer import (AudioOutputConfig,
                                          SonataSpeechSynthesizer)

SENTENCES = ["wˈʌn.", "wˈʌn tˈuː θɹˈiː fˈoːɹ.", "hˈɛloʊ ðˈɛr ˈɛvɹiwˌʌn."]
TRIPLE = AudioOutputConfig(rate=30, volume=60, pitch=60).prosody_triple()


def _rows(seed=0):
    """Ragged rows across five decades of amplitude, one of them empty."""
    rng = np.random.default_rng(seed)
    lens = [700, 1, 0, 33, 256]
    amps = [3.0, 1e-5, 1.0, 0.3, 1e-2]
    x = np.full((len(lens), max(lens)), 1e3, dtype=np.float32)
    for b, (n, a) in enumerate(zip(lens, amps)):
        x[b, :n] = (a * rng.standard_normal(n)).astype(np.float32)
    return x, lens


@pytest.mark.parametrize("peak_normalize", [True, False])
def test_pcm16_rows_cpu_is_to_i16(peak_normalize):
    x, lens = _rows()
    sil = [0, 5, 7, 0, 2]
    pcm, out = ops.pcm16_rows(torch.from_numpy(x), lens, sil,
                              peak_normalize=peak_normalize)
    assert pcm.dtype == torch.int16 and pcm.shape[0] == len(lens)
    assert out.tolist() == [n + s for n, s in zip(lens, sil)]
    assert pcm.shape[1] >= max(out.tolist())
    pcm = pcm.numpy()
    for b, n in enumerate(lens):
        np.testing.assert_array_equal(
            pcm[b, :n], to_i16(x[b, :n], peak_normalize), err_msg=str(b))
        assert not pcm[b, n:].any(), b  # silence and padding
    # no silence, one silence for all rows
    p0, o0 = ops.pcm16_rows(torch.from_numpy(x), lens)
    assert o0.tolist() == lens
    p3, o3 = ops.pcm16_rows(torch.from_numpy(x), torch.tensor(lens), 3)
    assert o3.tolist() == [n + 3 for n in lens]
    np.testing.assert_array_equal(p3.numpy()[:, :max(lens)],
                                  p0.numpy()[:, :max(lens)])
    assert isinstance(ops.functional.PCM_TILE, int)


def test_pcm_audio(tmp_path):
    rng = np.random.default_rng(1)
    info = AudioInfo(sample_rate=16000)
    audio = Audio(0.4 * rng.standard_normal(4001).astype(np.float32), info,
                  inference_ms=12.5)
    p = PcmAudio.from_audio(audio)
    assert p.pcm.dtype == np.int16 and p.pcm.ndim == 1
    np.testing.assert_array_equal(p.pcm, to_i16(audio.samples))
    assert p.as_wave_bytes() == audio.as_wave_bytes()
    assert p.duration_ms == audio.duration_ms
    assert p.real_time_factor == audio.real_time_factor
    assert p.info is info and p.inference_ms == 12.5
    audio.save_to_file(str(tmp_path / "f.wav"))
    p.save_to_file(str(tmp_path / "p.wav"))
    assert (tmp_path / "f.wav").read_bytes() == (tmp_path / "p.wav").read_bytes()
    # appended silence equals silence merged before the conversion
    q = PcmAudio.from_audio(audio, 37)
    merged = Audio(merge(audio.samples, np.zeros(37, np.float32)), info, 12.5)
    assert q.as_wave_bytes() == merged.as_wave_bytes()
    assert q.duration_ms == merged.duration_ms
    # lists and 2-D input are flattened to int16, empty audio has no rtf
    assert PcmAudio([[1, -2, 3]], info).pcm.tolist() == [1, -2, 3]
    assert PcmAudio(np.zeros(0), info, 3.0).real_time_factor == 0.0


@pytest.mark.parametrize("prosody", [None, TRIPLE])
def test_speak_batch_pcm_equals_host_conversion(xlow_voice, prosody):
    v = xlow_voice
    assert v.supports_device_pcm
    rows = [prosody] * len(SENTENCES) if prosody else None
    ref = (v.speak_batch(SENTENCES, prosody=rows) if rows
           else v.speak_batch(SENTENCES))
    sr = v.config.sample_rate
    for silence_ms in (None, 30, [0, 12.5, 30]):
        got = v.speak_batch_pcm(SENTENCES, prosody=rows,
                                silence_ms=silence_ms)
        assert len(got) == len(SENTENCES)
        per_row = (silence_ms if isinstance(silence_ms, list)
                   else [silence_ms or 0] * len(SENTENCES))
        for g, r, ms in zip(got, ref, per_row):
            assert isinstance(g, PcmAudio)
            want = to_i16(merge(r.samples, generate_silence(ms, sr)))
            np.testing.assert_array_equal(g.pcm, want)
            assert g.info == r.info and g.inference_ms > 0


class _Stub:
    """Model stub that records which batch method ran, with what."""

    info = AudioInfo(sample_rate=16000)
    supports_device_pcm = True

    def __init__(self):
        self.calls = []

    @staticmethod
    def _samples(p):
        rng = np.random.default_rng(len(p))
        return (0.5 * rng.standard_normal(100 + len(p))).astype(np.float32)

    def speak_batch(self, phonemes, prosody=None):
        self.calls.append(("speak_batch", list(phonemes), prosody))
        return [Audio(self._samples(p), self.info, 1.0) for p in phonemes]

    def speak_batch_pcm(self, phonemes, prosody=None, silence_ms=None):
        self.calls.append(("speak_batch_pcm", list(phonemes), prosody,
                           list(silence_ms)))
        return [PcmAudio.from_audio(Audio(self._samples(p), self.info, 1.0),
                                    int(round((ms or 0) * 16)))
                for p, ms in zip(phonemes, silence_ms)]


def _drain(batcher, submits):
    """Queue everything before the worker wakes, so it is one bucket."""
    futures = [batcher.submit(*a, **k) for a, k in submits]
    out = [f.result(timeout=60) for f in futures]
    batcher.close()
    return out


def _want(p, ms=0):
    return to_i16(merge(_Stub._samples(p), generate_silence(ms, 16000)))


def test_batcher_all_pcm_bucket_runs_speak_batch_pcm():
    m = _Stub()
    b = DynamicBatcher(m, max_batch=3, max_wait_ms=2000)
    got = _drain(b, [(("aaaaaaaaa",), dict(pcm=True)),
                     (("aaaaaaaab", (1.5, 1.0, 1.0)),
                      dict(pcm=True, silence_ms=10)),
                     (("aaaaaaaac",), dict(pcm=True, silence_ms=20))])
    assert [c[0] for c in m.calls] == ["speak_batch_pcm"]
    _, phon, prosody, sil = m.calls[0]
    assert prosody == [None, (1.5, 1.0, 1.0), None] and sil == [None, 10, 20]
    for g, p, ms in zip(got, ["aaaaaaaaa", "aaaaaaaab", "aaaaaaaac"],
                        [0, 10, 20]):
        assert isinstance(g, PcmAudio)
        np.testing.assert_array_equal(g.pcm, _want(p, ms))


def test_batcher_mixed_bucket_converts_on_the_host():
    m = _Stub()
    b = DynamicBatcher(m, max_batch=3, max_wait_ms=2000)
    got = _drain(b, [(("aaaaaaaaa",), dict(pcm=True, silence_ms=10)),
                     (("aaaaaaaab",), dict()),
                     (("aaaaaaaac",), dict(pcm=True))])
    assert [c[0] for c in m.calls] == ["speak_batch"]
    assert m.calls[0][2] is None  # no prosody asked for, none passed
    assert isinstance(got[0], PcmAudio) and isinstance(got[2], PcmAudio)
    np.testing.assert_array_equal(got[0].pcm, _want("aaaaaaaaa", 10))
    np.testing.assert_array_equal(got[2].pcm, _want("aaaaaaaac"))
    assert isinstance(got[1], Audio)
    np.testing.assert_array_equal(got[1].samples, _Stub._samples("aaaaaaaab"))
    # a model without speak_batch_pcm still serves PCM requests
    class Old:
        def speak_batch(self, phonemes):
            return [Audio(_Stub._samples(p), _Stub.info) for p in phonemes]

    b = DynamicBatcher(Old(), max_wait_ms=1)
    g = b.submit("aaaaaaaaa", pcm=True, silence_ms=5).result(timeout=60)
    b.close()
    np.testing.assert_array_equal(g.pcm, _want("aaaaaaaaa", 5))


@pytest.mark.parametrize("cfg", [
    None,
    AudioOutputConfig(appended_silence_ms=25),
    AudioOutputConfig(rate=30, volume=60, pitch=60, appended_silence_ms=40),
])
def test_synthesizer_pcm_bytes_equal_float_bytes(xlow_voice, cfg):
    synth = SonataSpeechSynthesizer(xlow_voice)
    text = "wˈʌn tˈuː. θɹˈiː fˈoːɹ fˈaɪv."
    for mode in (synth.synthesize_parallel, synth.synthesize_lazy):
        ref = [a.as_wave_bytes() for a in mode(text, cfg)]
        got = list(mode(text, cfg, pcm=True))
        assert all(isinstance(g, PcmAudio) for g in got)
        assert [g.as_wave_bytes() for g in got] == ref and len(ref) == 2


@pytest.fixture(scope="module")
def grpc_loopback(xlow_voice_path):
    from sonata_amd.frontends.grpc import create_server
    from sonata_amd.frontends.grpc.client import SonataGrpcClient
    from sonata_amd.frontends.grpc.proto import MESSAGES

    server, port, service = create_server(port=0, device="cpu")
    server.start()
    client = SonataGrpcClient(f"127.0.0.1:{port}")
    vid = client.LoadVoice(
        MESSAGES["VoicePath"](config_path=xlow_voice_path)).voice_id
    yield client, vid, service
    client.close()
    server.stop(grace=None)


@pytest.mark.parametrize("mode", ["parallel", "lazy"])
@pytest.mark.parametrize("args", [
    dict(),
    dict(appended_silence_ms=35),
    dict(rate=30, volume=60, pitch=60, appended_silence_ms=35),
])
def test_grpc_wire_bytes_equal_float_path(grpc_loopback, mode, args):
    from sonata_amd.frontends.grpc.proto import (MESSAGES, MODE_LAZY,
                                                 MODE_PARALLEL)

    client, vid, service = grpc_loopback
    text = "wˈʌn tˈuː. θɹˈiː fˈoːɹ fˈaɪv."
    req = MESSAGES["Utterance"](
        voice_id=vid, text=text,
        synthesis_mode=MODE_LAZY if mode == "lazy" else MODE_PARALLEL)
    if args:
        req.speech_args.CopyFrom(MESSAGES["SpeechArgs"](**args))
    got = [r.wav_samples for r in client.SynthesizeUtterance(req)]
    synth = service._voices[vid].synth
    cfg = AudioOutputConfig(**args) if args else None
    float_mode = (synth.synthesize_lazy if mode == "lazy"
                  else synth.synthesize_parallel)
    want = [a.as_wave_bytes() for a in float_mode(text, cfg)]
    assert len(want) == 2 and got == want
