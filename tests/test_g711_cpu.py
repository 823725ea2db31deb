"""G.711 output without a GPU: the NumPy reference against pinned tables,
the WAV layout, PcmAudio, ops.g711_rows on CPU tensors, the voice, both
batchers, the synthesizer, the CLI and the gRPC wire.  Every comparison is
exact equality with g711.encode(to_i16(...))."""

import hashlib
import io
import json
import struct

import numpy as np
import pytest
import torch

from sonata_amd import ops
from sonata_amd.audio import g711
from sonata_amd.audio.samples import generate_silence, merge, to_i16
from sonata_amd.audio.wav import (read_wav_file, wav_bytes_g711,
                                  wav_bytes_pcm, write_wav_file_g711)
from sonata_amd.core import Audio, AudioInfo, PcmAudio
from sonata_amd.synth import DynamicBatcher, StreamBatcher
from sonata_amd.synth.synthesizer import (AudioOutputConfig,
                                          SonataSpeechSynthesizer)

SENTENCES = ["wˈʌn.", "wˈʌn tˈuː θɹˈiː fˈoːɹ.", "hˈɛloʊ ðˈɛr ˈɛvɹiwˌʌn."]
TEXT = "wˈʌn tˈuː. θɹˈiː fˈoːɹ fˈaɪv."
ALL16 = np.arange(-32768, 32768).astype(np.int16)
SHA = {
    ("ulaw", "encode"):
        "81d633c9e6972a18c74a58720b96cb8ca0bdd096d4060b646dd708c3b846019a",
    ("alaw", "encode"):
        "38488f6fd710f4686360edc4d38639f96c491595ef93f8eb8d62d5e07ca6ce7b",
    ("ulaw", "decode"):
        "3dab54339e520bb2c924826e3b72a917a2b612e9fd12fc867500f1d983a75827",
    ("alaw", "decode"):
        "e04788d110e58ff8c70c93b8480190d973e3b67876b6119abbaec766cc75c174",
}


# ------------------------------ the reference ------------------------------ #
def test_constants():
    assert g711.LAWS == ("ulaw", "alaw")
    assert g711.ZERO == {"ulaw": 0xFF, "alaw": 0xD5}
    assert g711.check_law("ulaw") == "ulaw"
    for bad in ("pcm16", None, "mulaw", 1):
        with pytest.raises(ValueError):
            g711.check_law(bad)
    with pytest.raises(ValueError):
        g711.encode(ALL16[:4], "pcm16")
    with pytest.raises(ValueError):
        g711.decode([0], "law")


@pytest.mark.parametrize("law", g711.LAWS)
def test_tables_match_the_pinned_hashes(law):
    enc = g711.encode(ALL16, law)
    assert enc.dtype == np.uint8 and enc.shape == (65536,)
    assert hashlib.sha256(enc.tobytes()).hexdigest() == SHA[law, "encode"]
    dec = g711.decode(np.arange(256), law)
    assert dec.dtype == np.int16 and dec.shape == (256,)
    assert hashlib.sha256(dec.astype("<i2").tobytes()).hexdigest() \
        == SHA[law, "decode"]


def test_spot_values():
    u = lambda v: int(g711.encode([v], "ulaw")[0])  # noqa: E731
    a = lambda v: int(g711.encode([v], "alaw")[0])  # noqa: E731
    assert [u(v) for v in (0, -1, 3, 4, 32767, -32768)] \
        == [0xFF, 0x7E, 0xFF, 0xFE, 0x80, 0x00]
    assert [a(v) for v in (0, -1, 32767, -32768)] == [0xD5, 0x55, 0xAA, 0x2A]
    for law in g711.LAWS:
        assert u(0) == g711.ZERO["ulaw"] and a(0) == g711.ZERO["alaw"]
        # any shape and plain lists are taken, flattened
        assert g711.encode([[0, 0]], law).tolist() == [g711.ZERO[law]] * 2


def test_code_sets_round_trip_and_monotonicity():
    eu, ea = g711.encode(ALL16, "ulaw"), g711.encode(ALL16, "alaw")
    assert 0x7F not in eu and len(np.unique(eu)) == 255  # no negative zero
    assert len(np.unique(ea)) == 256
    codes = np.arange(256)
    du, da = g711.decode(codes, "ulaw"), g711.decode(codes, "alaw")
    assert du.min() == -32124 and du.max() == 32124
    assert du[0xFF] == 0 and du[0x7F] == 0
    assert da.min() == -32256 and da.max() == 32256 and 0 not in da
    want_u = codes.copy()
    want_u[0x7F] = 0xFF
    np.testing.assert_array_equal(g711.encode(du, "ulaw"), want_u)
    np.testing.assert_array_equal(g711.encode(da, "alaw"), codes)
    for law, e in (("ulaw", eu), ("alaw", ea)):
        back = g711.decode(e, law).astype(np.int32)
        assert (np.diff(back) >= 0).all(), law


@pytest.mark.parametrize("law", g711.LAWS)
def test_against_audioop(law):
    audioop = pytest.importorskip("audioop")
    lin2, to_lin = ((audioop.lin2ulaw, audioop.ulaw2lin) if law == "ulaw"
                    else (audioop.lin2alaw, audioop.alaw2lin))
    want = np.frombuffer(lin2(ALL16.astype("<i2").tobytes(), 2), np.uint8)
    np.testing.assert_array_equal(g711.encode(ALL16, law), want)
    want = np.frombuffer(to_lin(bytes(range(256)), 2), "<i2")
    np.testing.assert_array_equal(g711.decode(np.arange(256), law), want)


# --------------------------------- the WAV ---------------------------------- #
@pytest.mark.parametrize("law,tag", [("ulaw", 7), ("alaw", 6)])
@pytest.mark.parametrize("n", [10, 11, 0])
def test_wav_layout(law, tag, n, tmp_path):
    rng = np.random.default_rng(n)
    codes = g711.encode(rng.integers(-32768, 32768, n).astype(np.int16), law)
    data = wav_bytes_g711(codes, 8000, law)
    pad = n & 1
    assert len(data) == 58 + n + pad
    assert data[:4] == b"RIFF" and data[8:12] == b"WAVE"
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8 == 50 + n + pad
    assert data[12:16] == b"fmt "
    size, ftag, ch, rate, byte_rate, align, bits, cb = struct.unpack(
        "<IHHIIHHH", data[16:38])
    assert (size, ftag, ch, rate, byte_rate, align, bits, cb) \
        == (18, tag, 1, 8000, 8000, 1, 8, 0)
    assert data[38:42] == b"fact"
    assert struct.unpack("<II", data[42:50]) == (4, n)
    assert data[50:54] == b"data"
    assert struct.unpack("<I", data[54:58])[0] == n
    assert data[58:58 + n] == codes.tobytes()
    assert data[58 + n:] == b"\x00" * pad
    path = str(tmp_path / "g.wav")
    write_wav_file_g711(path, codes, 8000, law)
    assert open(path, "rb").read() == data
    x, rate, ch = read_wav_file(path)
    assert (rate, ch) == (8000, 1) and x.dtype == np.float32
    np.testing.assert_array_equal(
        x, g711.decode(codes, law).astype(np.float32) / 32767.0)


def test_wav_two_channels_and_pcm_reader_unchanged(tmp_path):
    hdr = wav_bytes_g711(np.zeros(8, np.uint8), 16000, "alaw", 2)
    assert struct.unpack("<IHHIIHHH", hdr[16:38]) \
        == (18, 6, 2, 16000, 32000, 2, 8, 0)
    assert struct.unpack("<II", hdr[42:50]) == (4, 4)  # samples per channel
    pcm = np.array([0, 1, -1, 32767, -32768], np.int16)
    p = tmp_path / "p.wav"
    p.write_bytes(wav_bytes_pcm(pcm, 22050))
    x, rate, ch = read_wav_file(str(p))
    assert (rate, ch) == (22050, 1)
    np.testing.assert_array_equal(x, pcm.astype(np.float32) / 32767.0)


# -------------------------------- PcmAudio ---------------------------------- #
@pytest.mark.parametrize("law", g711.LAWS)
def test_pcm_audio_with_an_encoding(law, tmp_path):
    rng = np.random.default_rng(1)
    info = AudioInfo(sample_rate=8000)
    audio = Audio(0.4 * rng.standard_normal(4001).astype(np.float32), info,
                  inference_ms=12.5)
    lin = PcmAudio.from_audio(audio, 37)
    assert lin.encoding == "pcm16" and lin.info is info
    assert lin.to_int16() is lin.pcm
    p = PcmAudio.from_audio(audio, 37, encoding=law)
    assert p.encoding == law and p.pcm.dtype == np.uint8 and p.pcm.ndim == 1
    np.testing.assert_array_equal(p.pcm, g711.encode(lin.pcm, law))
    assert (p.pcm[-37:] == g711.ZERO[law]).all()
    assert p.info == AudioInfo(sample_rate=8000, sample_width=1)
    assert p.as_wave_bytes() == p.pcm.tobytes()
    assert len(p.as_wave_bytes()) == 4038
    assert p.duration_ms == lin.duration_ms  # samples, not bytes
    assert p.real_time_factor == lin.real_time_factor
    np.testing.assert_array_equal(p.to_int16(), g711.decode(p.pcm, law))
    p.save_to_file(str(tmp_path / "g.wav"))
    assert (tmp_path / "g.wav").read_bytes() \
        == wav_bytes_g711(p.pcm, 8000, law)
    assert PcmAudio([[1, 2, 255]], info, encoding=law).pcm.tolist() \
        == [1, 2, 255]
    with pytest.raises(ValueError):
        PcmAudio([1], info, encoding="g722")


# ---------------------------------- the op ---------------------------------- #
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
@pytest.mark.parametrize("law", ["ulaw", "alaw",
                                 ["ulaw", "alaw", "alaw", "ulaw", "alaw"]])
def test_g711_rows_cpu_is_the_definition(law, peak_normalize):
    x, lens = _rows()
    sil = [0, 5, 7, 0, 2]
    codes, out = ops.g711_rows(torch.from_numpy(x), lens, sil, law,
                               peak_normalize=peak_normalize)
    assert codes.dtype == torch.uint8 and codes.shape[0] == len(lens)
    assert out.tolist() == [n + s for n, s in zip(lens, sil)]
    assert codes.shape[1] == 704  # max(out) = 700 up to a multiple of 16
    codes = codes.numpy()
    laws = [law] * len(lens) if isinstance(law, str) else law
    for b, n in enumerate(lens):
        np.testing.assert_array_equal(
            codes[b, :n],
            g711.encode(to_i16(x[b, :n], peak_normalize), laws[b]),
            err_msg=str(b))
        assert (codes[b, n:] == g711.ZERO[laws[b]]).all(), b
    # it is the encoding of pcm16_rows, padding included
    pcm, _ = ops.pcm16_rows(torch.from_numpy(x), lens, sil,
                            peak_normalize=peak_normalize)
    for b in range(len(lens)):
        np.testing.assert_array_equal(
            codes[b, :700], g711.encode(pcm.numpy()[b, :700], laws[b]))


def test_g711_rows_arguments():
    x, lens = _rows()
    t = torch.from_numpy(x)
    c0, o0 = ops.g711_rows(t, lens)  # mu-law, no silence
    assert o0.tolist() == lens
    np.testing.assert_array_equal(
        c0.numpy(), ops.g711_rows(t, torch.tensor(lens), 0, "ulaw")[0].numpy())
    for bad in ("pcm16", "g722", ["ulaw"] * 4 + ["pcm16"], ["ulaw", 1, 0, 0, 0]):
        with pytest.raises(ValueError):
            ops.g711_rows(t, lens, law=bad)
    with pytest.raises(AssertionError):
        ops.g711_rows(t, lens, law=["ulaw"] * 4)
    with pytest.raises(AssertionError):
        ops.g711_rows(t, [701, 1, 0, 33, 256])
    e, oe = ops.g711_rows(torch.zeros((0, 5)), [])
    assert e.shape == (0, 0) and oe.tolist() == []


# --------------------------------- the voice -------------------------------- #
@pytest.fixture(scope="module")
def int16_rows(xlow_voice):
    """speak_batch_pcm without an encoding, at the voice's rate and at
    8 kHz, with 30 ms of silence: the reference the voice tests share."""
    return {rate: xlow_voice.speak_batch_pcm(SENTENCES, silence_ms=30,
                                             sample_rate=rate)
            for rate in (None, 8000)}


@pytest.mark.parametrize("rate", [None, 8000])
@pytest.mark.parametrize("law", g711.LAWS)
def test_speak_batch_pcm_encoding(xlow_voice, int16_rows, law, rate):
    got = xlow_voice.speak_batch_pcm(SENTENCES, silence_ms=30,
                                     sample_rate=rate, encoding=law)
    for g, r in zip(got, int16_rows[rate]):
        assert g.encoding == law and g.pcm.dtype == np.uint8
        np.testing.assert_array_equal(g.pcm, g711.encode(r.pcm, law))
        assert g.info.sample_rate == r.info.sample_rate
        assert g.info.sample_width == 1 and g.inference_ms > 0
        assert (g.pcm[-(30 * g.info.sample_rate // 1000):]
                == g711.ZERO[law]).all()


def test_speak_batch_pcm_mixed_rows(xlow_voice, int16_rows):
    v = xlow_voice
    encs = ["alaw", None, "ulaw"]
    rates = [8000, 8000, None]
    got = v.speak_batch_pcm(SENTENCES, silence_ms=30, sample_rate=rates,
                            encoding=encs)
    for g, e, rate, b in zip(got, encs, rates, range(3)):
        ref = int16_rows[rate][b]
        if e is None:
            assert g.encoding == "pcm16" and g.pcm.dtype == np.int16
            np.testing.assert_array_equal(g.pcm, ref.pcm)
            assert g.info == ref.info
        else:
            assert g.encoding == e
            np.testing.assert_array_equal(g.pcm, g711.encode(ref.pcm, e))
    # "pcm16" is the unset path
    lin = v.speak_batch_pcm(SENTENCES, silence_ms=30, encoding="pcm16")
    for g, r in zip(lin, int16_rows[None]):
        assert g.encoding == "pcm16" and g.info == r.info
        np.testing.assert_array_equal(g.pcm, r.pcm)
    with pytest.raises(ValueError):
        v.speak_batch_pcm(SENTENCES, encoding="g722")
    with pytest.raises(AssertionError):
        v.speak_batch_pcm(SENTENCES, encoding=["ulaw"])


def test_stream_chunks_are_the_codes_of_the_int16_chunks(xlow_voice):
    v = xlow_voice
    two = SENTENCES[1:]
    want = [[] for _ in two]
    for i, chunk in v.stream_synthesis_batch(two, 20, 2, pcm=True):
        want[i].append(chunk)
    assert sum(len(w) for w in want) > 2  # streams of several chunks
    for encs in ("ulaw", ["alaw", "ulaw"]):
        laws = [encs] * 2 if isinstance(encs, str) else encs
        got = [[] for _ in two]
        for i, chunk in v.stream_synthesis_batch(two, 20, 2, encoding=encs):
            assert chunk.dtype == np.uint8
            got[i].append(chunk)
        for g, w, law in zip(got, want, laws):
            assert len(g) == len(w)
            for a, b in zip(g, w):
                np.testing.assert_array_equal(a, g711.encode(b, law))
    # a round has one output dtype
    with pytest.raises(ValueError):
        next(v.stream_synthesis_batch(two, 20, 2, encoding=["ulaw", None]))
    with pytest.raises(ValueError):
        next(v.stream_synthesis_batch(two, 20, 2, encoding="g722"))
    assert len(v._tail_free) == v._tails.shape[0]
    assert not v._infer_lock.locked()


# -------------------------------- the batchers ------------------------------ #
class _Stub:
    """Model stub that records which batch method ran, with what."""

    info = AudioInfo(sample_rate=16000)
    supports_device_pcm = True

    def __init__(self):
        self.calls = []

    def audio_output_info(self):
        return self.info

    @staticmethod
    def _samples(p):
        rng = np.random.default_rng(len(p))
        return (0.5 * rng.standard_normal(100 + len(p))).astype(np.float32)

    def speak_batch(self, phonemes, prosody=None):
        self.calls.append(("speak_batch", list(phonemes)))
        return [Audio(self._samples(p), self.info, 1.0) for p in phonemes]

    def speak_batch_pcm(self, phonemes, prosody=None, silence_ms=None,
                        encoding=None):
        self.calls.append(("speak_batch_pcm", list(phonemes), encoding))
        encoding = encoding or ["pcm16"] * len(phonemes)
        return [PcmAudio.from_audio(Audio(self._samples(p), self.info, 1.0),
                                    int(round((ms or 0) * 16)), e)
                for p, ms, e in zip(phonemes, silence_ms, encoding)]


def _want(p, ms=0):
    return to_i16(merge(_Stub._samples(p), generate_silence(ms, 16000)))


def test_dynamic_batcher_mixed_encodings_share_one_call():
    m = _Stub()
    b = DynamicBatcher(m, max_batch=3, max_wait_ms=2000)
    futures = [b.submit("aaaaaaaaa", pcm=True, encoding="ulaw"),
               b.submit("aaaaaaaab", pcm=True, silence_ms=10),
               b.submit("aaaaaaaac", pcm=True, silence_ms=20,
                        encoding="alaw")]
    got = [f.result(timeout=60) for f in futures]
    assert m.calls == [("speak_batch_pcm",
                        ["aaaaaaaaa", "aaaaaaaab", "aaaaaaaac"],
                        ["ulaw", "pcm16", "alaw"])]
    np.testing.assert_array_equal(
        got[0].pcm, g711.encode(_want("aaaaaaaaa"), "ulaw"))
    np.testing.assert_array_equal(got[1].pcm, _want("aaaaaaaab", 10))
    np.testing.assert_array_equal(
        got[2].pcm, g711.encode(_want("aaaaaaaac", 20), "alaw"))
    assert [g.encoding for g in got] == ["ulaw", "pcm16", "alaw"]
    with pytest.raises(ValueError):
        b.submit("a", pcm=True, encoding="g722")
    with pytest.raises(AssertionError):
        b.submit("a", encoding="ulaw")
    b.close()
    # an all-int16 bucket passes no encoding on: models that do not know
    # the keyword are served as before
    m = _Stub()
    b = DynamicBatcher(m, max_batch=1, max_wait_ms=1)
    b.submit("aaaaaaaaa", pcm=True, encoding="pcm16").result(timeout=60)
    b.close()
    assert m.calls == [("speak_batch_pcm", ["aaaaaaaaa"], None)]


def test_dynamic_batcher_host_route_encodes_too():
    m = _Stub()
    b = DynamicBatcher(m, max_batch=2, max_wait_ms=2000)
    futures = [b.submit("aaaaaaaaa", pcm=True, silence_ms=10,
                        encoding="alaw"),
               b.submit("aaaaaaaab")]  # a float row: the bucket is mixed
    got = [f.result(timeout=60) for f in futures]
    b.close()
    assert [c[0] for c in m.calls] == ["speak_batch"]
    assert got[0].encoding == "alaw" and isinstance(got[1], Audio)
    np.testing.assert_array_equal(
        got[0].pcm, g711.encode(_want("aaaaaaaaa", 10), "alaw"))


def test_stream_buckets_separate_by_output_dtype():
    from sonata_amd.models.chunker import ChunkSpec
    from sonata_amd.synth.batcher import _StreamHandle

    class _S:
        def __init__(self, n):
            self.next_spec = ChunkSpec(0, n, 0, 0, False)

    hs = []
    for n, pcm, enc in ((48, False, "pcm16"), (50, True, "pcm16"),
                        (52, True, "ulaw"), (54, False, "alaw"),
                        (56, False, "pcm16")):
        h = _StreamHandle("x", 20, 2, pcm, encoding=enc)
        h.state = _S(n)
        hs.append(h)
    got = [[(h.window(), h.kind) for h in b]
           for b in StreamBatcher._buckets(hs)]
    assert got == [[(48, 0), (56, 0)], [(50, 1)], [(52, 2), (54, 2)]]


def test_stream_batcher_mixed_encodings(xlow_voice):
    v = xlow_voice
    two = SENTENCES[1:]
    want = [[] for _ in two]
    for i, chunk in v.stream_synthesis_batch(two, 20, 2, pcm=True):
        want[i].append(chunk)
    calls = []
    real = v.stream_round

    def spy(states, pcm=False, **kw):
        calls.append((len(states), pcm, kw.get("encoding")))
        return real(states, pcm=pcm, **kw)

    v.stream_round = spy
    sb = StreamBatcher(v, max_streams=8, max_wait_ms=500.0)
    try:
        its = [sb.open(two[0], 20, 2, encoding="ulaw"),
               sb.open(two[1], 20, 2, pcm=True, encoding="alaw"),
               sb.open(two[1], 20, 2, pcm=True),
               sb.open(two[1], 20, 2, pcm=True, encoding="pcm16")]
        got = [list(it) for it in its]
        with pytest.raises(ValueError):
            sb.open(two[0], encoding="g722")
    finally:
        sb.close()
        del v.stream_round
    for g, w, law in ((got[0], want[0], "ulaw"), (got[1], want[1], "alaw")):
        assert len(g) == len(w)
        for a, b in zip(g, w):
            assert a.dtype == np.uint8
            np.testing.assert_array_equal(a, g711.encode(b, law))
    for g in got[2:]:
        assert len(g) == len(want[1])
        for a, b in zip(g, want[1]):
            assert a.dtype == np.int16
            np.testing.assert_array_equal(a, b)
    # both laws shared rounds; int16 streams ran apart, without the keyword
    assert (2, False, ["ulaw", "alaw"]) in calls \
        or (2, True, ["ulaw", "alaw"]) in calls
    assert all(enc is None for _, pcm, enc in calls
               if enc is None or "pcm16" in enc)
    assert all(set(enc) <= {"ulaw", "alaw"} for _, _, enc in calls if enc)
    assert len(v._tail_free) == v._tails.shape[0]


# ------------------------------ the synthesizer ----------------------------- #
def test_output_config_field():
    cfg = AudioOutputConfig(encoding="ulaw")
    assert cfg.is_noop and AudioOutputConfig().encoding is None
    enc = SonataSpeechSynthesizer.output_encoding
    assert enc(None) == "pcm16" and enc(AudioOutputConfig()) == "pcm16"
    assert enc(AudioOutputConfig(encoding="pcm16")) == "pcm16"
    assert enc(cfg) == "ulaw"
    with pytest.raises(ValueError):
        enc(AudioOutputConfig(encoding="g722"))


@pytest.mark.parametrize("kw", [
    dict(),
    dict(appended_silence_ms=25, sample_rate=8000),
    dict(rate=30, volume=60, pitch=60, appended_silence_ms=40),
])
@pytest.mark.parametrize("law", g711.LAWS)
def test_synthesizer_modes(xlow_voice, kw, law):
    synth = SonataSpeechSynthesizer(xlow_voice)
    plain = AudioOutputConfig(**kw) if kw else None
    cfg = AudioOutputConfig(encoding=law, **kw)
    for mode in (synth.synthesize_parallel, synth.synthesize_lazy):
        ref = list(mode(TEXT, plain, pcm=True))
        got = list(mode(TEXT, cfg, pcm=True))
        assert len(got) == len(ref) == 2
        for g, r in zip(got, ref):
            assert isinstance(g, PcmAudio) and g.encoding == law
            np.testing.assert_array_equal(g.pcm, g711.encode(r.pcm, law))
            assert g.info.sample_rate == r.info.sample_rate
        # float results never change
        fl, fr = list(mode(TEXT, cfg)), list(mode(TEXT, plain))
        for a, b in zip(fl, fr):
            assert isinstance(a, Audio)
            np.testing.assert_array_equal(a.samples, b.samples)
    a = next(iter(synth.synthesize_parallel(TEXT, plain)))
    got = synth.to_pcm(a, cfg, prosody_done=True)
    assert got.encoding == law
    np.testing.assert_array_equal(
        got.pcm,
        g711.encode(synth.to_pcm(a, plain, prosody_done=True).pcm, law))


def test_synthesizer_refuses_an_unknown_encoding(xlow_voice, tmp_path):
    synth = SonataSpeechSynthesizer(xlow_voice)
    cfg = AudioOutputConfig(encoding="g722")
    with pytest.raises(ValueError):
        next(synth.synthesize_lazy(TEXT, cfg, pcm=True))
    with pytest.raises(ValueError):
        synth.synthesize_parallel(TEXT, cfg, pcm=True)
    with pytest.raises(ValueError):
        synth.synthesize_to_file(str(tmp_path / "x.wav"), TEXT, cfg)


@pytest.mark.parametrize("law", g711.LAWS)
def test_synthesize_to_file(xlow_voice, law, tmp_path):
    synth = SonataSpeechSynthesizer(xlow_voice)
    kw = dict(appended_silence_ms=20, sample_rate=8000)
    p16, p8 = tmp_path / "lin.wav", tmp_path / "g.wav"
    a16 = synth.synthesize_to_file(str(p16), TEXT, AudioOutputConfig(**kw))
    a8 = synth.synthesize_to_file(str(p8), TEXT,
                                  AudioOutputConfig(encoding=law, **kw))
    np.testing.assert_array_equal(a8.samples, a16.samples)
    lin = np.frombuffer(p16.read_bytes()[44:], "<i2")
    assert p8.read_bytes() == wav_bytes_g711(g711.encode(lin, law), 8000, law)
    x, rate, _ = read_wav_file(str(p8))
    assert rate == 8000 and len(x) == len(lin)


def test_pysonata_inherits_the_encoding(xlow_voice_path):
    from sonata_amd.frontends import pysonata

    synth = pysonata.Sonata.with_piper(
        pysonata.PiperModel(xlow_voice_path, device="cpu"))
    cfg = pysonata.AudioOutputConfig(encoding="alaw")
    for mode in (synth.synthesize_parallel, synth.synthesize_lazy):
        ref = [w.get_wave_bytes() for w in mode(TEXT)]
        got = [w.get_wave_bytes() for w in mode(TEXT, cfg)]
        assert len(ref) == 2
        assert got == [g711.encode(np.frombuffer(r, "<i2"), "alaw").tobytes()
                       for r in ref]
    ref = list(synth.synthesize_streamed(TEXT))
    got = list(synth.synthesize_streamed(TEXT, cfg))
    assert got == [g711.encode(np.frombuffer(r, "<i2"), "alaw").tobytes()
                   for r in ref]


# ---------------------------------- the CLI --------------------------------- #
@pytest.mark.parametrize("law", g711.LAWS)
def test_cli_file_and_stdout(xlow_voice_path, law, tmp_path):
    from sonata_amd.frontends import cli

    inp = tmp_path / "in.txt"
    inp.write_text("həˈloʊ wˈɜːld.")
    base = [xlow_voice_path, "--device", "cpu", "--sample-rate", "8000"]
    lin, g = tmp_path / "lin.wav", tmp_path / "g.wav"
    assert cli.main(base + ["-f", str(inp), "-o", str(lin)]) == 0
    assert cli.main(base + ["-f", str(inp), "-o", str(g),
                            "--encoding", law]) == 0
    pcm = np.frombuffer(lin.read_bytes()[44:], "<i2")
    want = wav_bytes_g711(g711.encode(pcm, law), 8000, law)
    assert g.read_bytes() == want
    # stdout, with the encoding in the request line
    for mode in ("parallel", "lazy"):
        buf = io.BytesIO()
        line = io.StringIO(json.dumps(
            {"text": "həˈloʊ wˈɜːld.", "encoding": law}) + "\n")
        assert cli.main(base + ["-m", mode], stdin=line, stdout=buf) == 0
        assert buf.getvalue() == want
    # --encoding pcm16 is the unset output
    p16 = tmp_path / "p16.wav"
    assert cli.main(base + ["-f", str(inp), "-o", str(p16),
                            "--encoding", "pcm16"]) == 0
    assert p16.read_bytes() == lin.read_bytes()


def test_cli_realtime_stdout(xlow_voice_path):
    from sonata_amd.frontends import cli

    base = [xlow_voice_path, "--device", "cpu", "-m", "realtime",
            "--chunk-size", "20", "--chunk-padding", "2"]
    req = json.dumps({"text": "hˈaɪ ðˈɛr."}) + "\n"
    lin = io.BytesIO()
    assert cli.main(base, stdin=io.StringIO(req), stdout=lin) == 0
    pcm = np.frombuffer(lin.getvalue()[44:], "<i2")
    buf = io.BytesIO()
    assert cli.main(base + ["--encoding", "ulaw"], stdin=io.StringIO(req),
                    stdout=buf) == 0
    assert len(pcm) > 1000
    assert buf.getvalue() == wav_bytes_g711(g711.encode(pcm, "ulaw"), 16000,
                                            "ulaw")


# ---------------------------------- gRPC ------------------------------------ #
def test_speech_args_serialisation():
    from sonata_amd.frontends.grpc.proto import MESSAGES

    args = MESSAGES["SpeechArgs"]
    assert args().SerializeToString() == b""
    assert args(encoding=1).SerializeToString() == b"\x30\x01"
    assert args.FromString(b"\x30\x02").encoding == 2
    assert not args().HasField("encoding")
    assert args(encoding=0).HasField("encoding")


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


def _utterance(vid, mode, **args):
    from sonata_amd.frontends.grpc.proto import (MESSAGES, MODE_LAZY,
                                                 MODE_PARALLEL)

    req = MESSAGES["Utterance"](
        voice_id=vid, text=TEXT,
        synthesis_mode=MODE_LAZY if mode == "lazy" else MODE_PARALLEL)
    if args:
        req.speech_args.CopyFrom(MESSAGES["SpeechArgs"](**args))
    return req


@pytest.mark.parametrize("mode", ["parallel", "lazy", "realtime"])
@pytest.mark.parametrize("number,law", [(1, "ulaw"), (2, "alaw")])
def test_grpc_wav_samples_hold_the_codes(grpc_loopback, mode, number, law):
    client, vid, _ = grpc_loopback
    rpc = (client.SynthesizeUtteranceRealtime if mode == "realtime"
           else client.SynthesizeUtterance)
    args = dict(appended_silence_ms=35, sample_rate=8000)
    ref = [r.wav_samples for r in rpc(_utterance(vid, mode, **args))]
    assert ref == [r.wav_samples for r in rpc(
        _utterance(vid, mode, encoding=0, **args))]
    got = [r.wav_samples for r in rpc(
        _utterance(vid, mode, encoding=number, **args))]
    assert len(got) == len(ref) >= 2
    assert got == [g711.encode(np.frombuffer(r, "<i2"), law).tobytes()
                   for r in ref]


@pytest.mark.parametrize("mode", ["parallel", "lazy", "realtime"])
def test_grpc_refuses_an_unknown_encoding(grpc_loopback, mode):
    import grpc

    client, vid, _ = grpc_loopback
    rpc = (client.SynthesizeUtteranceRealtime if mode == "realtime"
           else client.SynthesizeUtterance)
    with pytest.raises(grpc.RpcError) as e:
        list(rpc(_utterance(vid, mode, encoding=3)))
    assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
