"""Per-request speaker and synthesis scales inside one batch, on the CPU:
VitsVoice (speak_batch, stream_synthesis_batch), DynamicBatcher, the gRPC
Utterance.synthesis_options field and the CLI's per-line keys, each against
the same sentence rendered alone with the config set voice-wide.

All on an x_low voice with three speakers."""

import io
import json
import struct
import threading

import grpc
import numpy as np
import pytest
import torch

from sonata_amd.models import SynthesisConfig, create_random_voice, load_voice

SENTS = ["hˈɛloʊ wˈɝld.", "ɡˈʊd mˈɔɹnɪŋ tu ju.",
         "ðɪs ɪz ə lˈɔŋɡɚ sˈɛntəns."]
# long enough for several chunks at chunk_size 45
STREAM_SENTS = [
    "ðɪs ɪz ə lˈɔŋ tɛst ʌv ðə stɹˈimɪŋ pˈæθ, wɪθ mˈɛni wˈɝdz.",
    "hˈɛloʊ wˈɝld.",
    "ɡˈʊd mˈɔɹnɪŋ tu ju, ænd ə vˈɛɹi ɡˈʊd dˈeɪ tu ˈɔl ʌv ju.",
]
CFG_A = SynthesisConfig(1, 0.667, 1.0, 0.8)
CFG_C = SynthesisConfig(2, 0.5, 1.3, 0.6)
STREAM_TOL = 1e-6  # tests/test_stream_batch_cpu.py TOL


@pytest.fixture(scope="module")
def pack(tmp_path_factory):
    d = tmp_path_factory.mktemp("rows_voice")
    return create_random_voice(str(d), "rows_voice", quality="x_low",
                               num_speakers=3)


@pytest.fixture(scope="module")
def voice(pack):
    return load_voice(pack)


def _alone(voice, sentence, cfg):
    """speak_one_sentence with cfg set voice-wide (None: as the voice is)."""
    base = voice.get_synthesis_config()
    if cfg is not None:
        voice.set_synthesis_config(cfg)
    try:
        return voice.speak_one_sentence(sentence).samples
    finally:
        voice.set_synthesis_config(base)


def _batch_matches_single(single, batched):
    """tests/test_model_cpu.py::test_batch_matches_single, per row"""
    assert len(single) == len(batched)
    n = len(single)
    head = max(n - 4096, 0)
    assert np.allclose(single[:head], batched[:head], atol=1e-3)
    assert np.corrcoef(single, batched)[0, 1] > 0.99


# ------------------------------- the voice -------------------------------- #
def test_announces_row_synthesis(voice):
    assert voice.supports_row_synthesis is True


def test_mixed_batch_equals_single_calls(voice):
    rows = [CFG_A, None, CFG_C]
    before = voice.get_synthesis_config()
    batch = voice.speak_batch(SENTS, synthesis=rows)
    assert voice.get_synthesis_config() == before
    singles = [_alone(voice, s, r) for s, r in zip(SENTS, rows)]
    for one, b in zip(singles, batch):
        _batch_matches_single(one, b.samples)
    # the rows really are different speakers: row 0 is not the default's
    default0 = _alone(voice, SENTS[0], None)
    assert (len(default0) != len(batch[0].samples)
            or np.abs(default0 - batch[0].samples).max() > 1e-3)


def test_uniform_rows_are_the_scalar_path_bit_for_bit(voice):
    cfg = SynthesisConfig(2, 0.5, 1.2, 0.7)
    base = voice.get_synthesis_config()
    voice.set_synthesis_config(cfg)
    try:
        want = voice.speak_batch(SENTS)
    finally:
        voice.set_synthesis_config(base)
    got = voice.speak_batch(SENTS, synthesis=[cfg.copy() for _ in SENTS])
    for w, g in zip(want, got):
        assert np.array_equal(w.samples, g.samples)


def test_per_row_length_scale(voice):
    s = "ðɪs ɪz ə lˈɔŋɡɚ sˈɛntəns."
    fast = SynthesisConfig(0, 0.667, 0.5, 0.8)
    slow = SynthesisConfig(0, 0.667, 2.0, 0.8)
    a_fast, a_slow = voice.speak_batch([s, s], synthesis=[fast, slow])
    # tests/test_model_cpu.py::test_length_scale_controls_duration
    assert len(a_slow.samples) > 2 * len(a_fast.samples)


@pytest.mark.parametrize("bad, word", [
    (SynthesisConfig(3, 0.667, 1.0, 0.8), "3"),
    (SynthesisConfig(1, 0.667, 0.0, 0.8), "length_scale"),
    (SynthesisConfig(1, 0.667, 1.0, float("nan")), "noise_w"),
])
def test_validation_runs_before_any_inference(voice, monkeypatch, bad, word):
    def boom(*a, **k):
        raise AssertionError("inference ran")

    monkeypatch.setattr(voice.net, "infer", boom)
    monkeypatch.setattr(voice.net, "infer_encoder", boom)
    with pytest.raises(ValueError, match=word):
        voice.speak_batch(SENTS, synthesis=[CFG_A, bad, None])
    with pytest.raises(ValueError, match=word):
        voice.speak_batch_pcm(SENTS, synthesis=[CFG_A, bad, None])
    with pytest.raises(ValueError, match=word):
        voice.stream_open(SENTS, synthesis=[CFG_A, bad, None])
    with pytest.raises(ValueError, match=word):
        next(voice.stream_synthesis(SENTS[0], synthesis=bad))


def test_single_speaker_voice_ignores_the_id(xlow_voice):
    cfg = xlow_voice.get_synthesis_config()
    cfg.speaker_id = 7
    xlow_voice.check_synthesis_config(cfg)
    out = xlow_voice.speak_batch(SENTS[:2], synthesis=[cfg, None])
    assert all(len(a.samples) > 1000 for a in out)


def test_stream_synthesis_batch_rows(voice):
    rows = [CFG_A, None, CFG_C]
    batch = voice.speak_batch(STREAM_SENTS, synthesis=rows)
    # chunked: per stream the chunks of stream_synthesis with that config,
    # under the stream-batch test's bound, and the rows' exact timeline
    got = [[] for _ in STREAM_SENTS]
    for i, chunk in voice.stream_synthesis_batch(STREAM_SENTS, 45, 3,
                                                 synthesis=rows):
        got[i].append(chunk)
    assert max(len(g) for g in got) >= 2  # really chunked
    for s, r, g, b in zip(STREAM_SENTS, rows, got, batch):
        want = list(voice.stream_synthesis(s, 45, 3, synthesis=r))
        assert [len(c) for c in g] == [len(c) for c in want]
        assert float(np.abs(np.concatenate(g)
                            - np.concatenate(want)).max()) <= STREAM_TOL
        assert sum(len(c) for c in g) == len(b.samples)
    # one window per stream: the decode sees what speak_batch's sees, so
    # the chunks concatenate to its rows under the same bound
    got = [[] for _ in STREAM_SENTS]
    for i, chunk in voice.stream_synthesis_batch(STREAM_SENTS, 4096, 3,
                                                 synthesis=rows):
        got[i].append(chunk)
    for g, b in zip(got, batch):
        x = np.concatenate(g)
        assert len(x) == len(b.samples)
        assert float(np.abs(x - b.samples).max()) <= STREAM_TOL
    assert len(voice._tail_free) == voice._tails.shape[0]


def test_engine_rows_on_the_cpu(pack):
    """The C++ engine's host path: infer_encoder_rows against the scalar
    infer_encoder, row by row (fp32, the same ATen ops up to the broadcast)."""
    from sonata_amd import ops

    ext = ops.hip_ext()
    if ext is None:
        pytest.skip("extension not built")
    eng = ext.VitsEngine(pack, "cpu", "f32")
    ids_l = [eng.phonemes_to_ids(s) for s in SENTS]
    T = max(len(i) for i in ids_l)
    ids = torch.zeros((3, T), dtype=torch.long)
    for b, il in enumerate(ids_l):
        ids[b, :len(il)] = torch.tensor(il)
    lengths = torch.tensor([len(i) for i in ids_l])
    sid = torch.tensor([0, 2, 1])
    ns, ls, nw = [0.667, 0.3, 1.0], [1.0, 1.4, 0.6], [0.8, 0.0, 0.5]
    seeds = [11, 22, 33]
    z, y_mask, g = eng.infer_encoder_rows(ids, lengths, sid, ns, ls, nw,
                                          seeds)
    for b in range(3):
        zb, mb, gb = eng.infer_encoder(
            ids[b:b + 1, :len(ids_l[b])], lengths[b:b + 1], sid[b:b + 1],
            ns[b], ls[b], nw[b], seeds[b:b + 1])
        F = int(mb.sum())
        assert int(y_mask[b].sum()) == F
        assert torch.equal(g[b:b + 1], gb)
        assert float((z[b:b + 1, :, :F] - zb[:, :, :F]).abs().max()) < 1e-4
    with pytest.raises(RuntimeError, match="per-row"):
        eng.infer_encoder_rows(ids, lengths, sid, ns[:2], ls, nw, seeds)


# ------------------------------ the batcher ------------------------------- #
def test_dynamic_batcher_shares_one_batch(voice, monkeypatch):
    from sonata_amd.synth.batcher import DynamicBatcher

    s = "ɡˈʊd mˈɔɹnɪŋ tu ju."
    cfgs = [SynthesisConfig(k, 0.667, 1.0, 0.8) for k in range(3)]
    want = [_alone(voice, s, c) for c in cfgs]
    calls = []
    real = voice.speak_batch

    entered, release = threading.Event(), threading.Event()

    def counted(*a, **k):
        calls.append(len(a[0]))
        if len(calls) == 1:  # the plug: hold the worker while three queue up
            entered.set()
            assert release.wait(60)
        return real(*a, **k)

    monkeypatch.setattr(voice, "speak_batch", counted)
    b = DynamicBatcher(voice, max_batch=8, max_wait_ms=1.0)
    try:
        plug = b.submit("hˈaɪ.")
        assert entered.wait(60)
        futs = [None] * 3

        def go(k):
            futs[k] = b.submit(s, synthesis=cfgs[k])

        ts = [threading.Thread(target=go, args=(k,)) for k in range(3)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        release.set()
        plug.result(timeout=120)
        got = [f.result(timeout=120).samples for f in futs]
        with pytest.raises(ValueError, match="speaker_id 3"):
            b.submit(s, synthesis=SynthesisConfig(3, 0.667, 1.0, 0.8))
    finally:
        b.close()
    assert calls == [1, 3]  # the plug, then ONE speak_batch, three speakers
    for w, g in zip(want, got):
        _batch_matches_single(w, g)
    assert not np.array_equal(got[0], got[1])
    assert not np.array_equal(got[1], got[2])


class _NoRows:
    """A model of before: no synthesis= anywhere, one config per voice."""

    def __init__(self, voice):
        self._v = voice
        self.configs_seen = []
        self.entered, self.release = threading.Event(), threading.Event()

    def __getattr__(self, name):
        if name in ("supports_row_synthesis", "check_synthesis_config"):
            raise AttributeError(name)
        return getattr(self._v, name)

    def speak_batch(self, phonemes, **kw):
        assert "synthesis" not in kw
        if not self.configs_seen:  # the plug: hold the worker meanwhile
            self.entered.set()
            assert self.release.wait(60)
        self.configs_seen.append(
            (self._v.get_synthesis_config().speaker_id, len(phonemes)))
        return self._v.speak_batch(phonemes, **kw)


def test_batcher_groups_for_a_model_without_rows(voice):
    from sonata_amd.synth.batcher import DynamicBatcher

    s = "ɡˈʊd mˈɔɹnɪŋ tu ju."
    model = _NoRows(voice)
    before = voice.get_synthesis_config()
    cfg1, cfg2 = (SynthesisConfig(k, 0.667, 1.0, 0.8) for k in (1, 2))
    b = DynamicBatcher(model, max_batch=8, max_wait_ms=1.0)
    try:
        plug = b.submit("hˈaɪ.")
        assert model.entered.wait(60)
        futs = [b.submit(s, synthesis=c) for c in (cfg1, cfg2, cfg1, None)]
        model.release.set()
        plug.result(timeout=120)
        got = [f.result(timeout=120).samples for f in futs]
    finally:
        b.close()
    assert model.configs_seen[0] == (before.speaker_id, 1)  # the plug
    assert sorted(model.configs_seen[1:]) == sorted(
        [(1, 2), (2, 1), (before.speaker_id, 1)])
    assert voice.get_synthesis_config() == before
    assert np.array_equal(got[0], got[2])
    _batch_matches_single(_alone(voice, s, cfg2), got[1])


# --------------------------------- gRPC ----------------------------------- #
@pytest.fixture(scope="module")
def running(pack):
    from sonata_amd.frontends.grpc import create_server
    from sonata_amd.frontends.grpc.client import SonataGrpcClient

    server, port, service = create_server(port=0, device="cpu")
    server.start()
    client = SonataGrpcClient(f"127.0.0.1:{port}")
    yield client, pack
    client.close()
    server.stop(grace=None)


def _opts(vid, client):
    from sonata_amd.frontends.grpc.proto import MESSAGES

    return client.GetSynthesisOptions(
        MESSAGES["VoiceIdentifier"](voice_id=vid)).SerializeToString()


@pytest.mark.parametrize("mode", [1, 2, 3])  # lazy, parallel, batched
def test_grpc_speaker_per_request(running, mode):
    from sonata_amd.frontends.grpc.proto import MESSAGES

    client, pack = running
    vid = client.LoadVoice(MESSAGES["VoicePath"](config_path=pack)).voice_id
    text = "ɡˈʊd mˈɔɹnɪŋ tu ju."
    before = _opts(vid, client)

    def say(**kw):
        res = list(client.SynthesizeUtterance(MESSAGES["Utterance"](
            voice_id=vid, text=text, synthesis_mode=mode, **kw)))
        assert len(res) == 1
        return res[0].wav_samples

    per_request = {
        name: say(synthesis_options=MESSAGES["SynthesisOptions"](
            speaker=name))
        for name in ("spk1", "spk2")}
    assert _opts(vid, client) == before
    assert per_request["spk1"] != per_request["spk2"]
    try:
        for name in ("spk1", "spk2"):
            client.SetSynthesisOptions(MESSAGES["VoiceSynthesisOptions"](
                voice_id=vid,
                synthesis_options=MESSAGES["SynthesisOptions"](speaker=name)))
            assert say() == per_request[name]
    finally:
        client.SetSynthesisOptions(MESSAGES["VoiceSynthesisOptions"](
            voice_id=vid,
            synthesis_options=MESSAGES["SynthesisOptions"](speaker="spk0")))
    assert _opts(vid, client) == before


def test_grpc_realtime_and_rejections(running):
    from sonata_amd.frontends.grpc.proto import MESSAGES

    client, pack = running
    vid = client.LoadVoice(MESSAGES["VoicePath"](config_path=pack)).voice_id
    text = "ɡˈʊd mˈɔɹnɪŋ tu ju."
    before = _opts(vid, client)

    def stream(**kw):
        return b"".join(c.wav_samples for c in
                        client.SynthesizeUtteranceRealtime(
                            MESSAGES["Utterance"](voice_id=vid, text=text,
                                                  **kw)))

    a = stream(synthesis_options=MESSAGES["SynthesisOptions"](speaker="spk1"))
    b = stream(synthesis_options=MESSAGES["SynthesisOptions"](speaker="spk2"))
    assert a != b and a != stream()
    try:
        client.SetSynthesisOptions(MESSAGES["VoiceSynthesisOptions"](
            voice_id=vid,
            synthesis_options=MESSAGES["SynthesisOptions"](speaker="spk1")))
        assert stream() == a
    finally:
        client.SetSynthesisOptions(MESSAGES["VoiceSynthesisOptions"](
            voice_id=vid,
            synthesis_options=MESSAGES["SynthesisOptions"](speaker="spk0")))
    assert _opts(vid, client) == before
    # the status SetSynthesisOptions gives an unknown speaker
    with pytest.raises(grpc.RpcError) as want:
        client.SetSynthesisOptions(MESSAGES["VoiceSynthesisOptions"](
            voice_id=vid,
            synthesis_options=MESSAGES["SynthesisOptions"](speaker="nobody")))
    for rpc in (client.SynthesizeUtterance,
                client.SynthesizeUtteranceRealtime):
        with pytest.raises(grpc.RpcError) as e:
            list(rpc(MESSAGES["Utterance"](
                voice_id=vid, text=text,
                synthesis_options=MESSAGES["SynthesisOptions"](
                    speaker="nobody"))))
        assert e.value.code() == want.value.code()
        with pytest.raises(grpc.RpcError) as e:
            list(rpc(MESSAGES["Utterance"](
                voice_id=vid, text=text,
                synthesis_options=MESSAGES["SynthesisOptions"](
                    length_scale=0.0))))
        assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
    assert _opts(vid, client) == before


def test_utterance_wire_bytes():
    from sonata_amd.frontends.grpc.proto import MESSAGES

    # an Utterance without the field: the bytes of before (fields 1, 2, 4)
    plain = MESSAGES["Utterance"](voice_id="v", text="hi", synthesis_mode=2)
    assert plain.SerializeToString() == b"\x0a\x01v\x12\x02hi\x20\x02"
    assert not plain.HasField("synthesis_options")
    # with it: field 5, length-delimited, holding the SynthesisOptions bytes
    opts = MESSAGES["SynthesisOptions"](speaker="spk1", length_scale=1.5)
    ob = opts.SerializeToString()
    assert ob == b"\x0a\x04spk1\x15" + struct.pack("<f", 1.5)
    full = MESSAGES["Utterance"](voice_id="v", text="hi", synthesis_mode=2,
                                 synthesis_options=opts)
    assert full.SerializeToString() == (
        plain.SerializeToString() + b"\x2a" + bytes([len(ob)]) + ob)
    back = MESSAGES["Utterance"].FromString(full.SerializeToString())
    assert back.synthesis_options.speaker == "spk1"
    assert not back.synthesis_options.HasField("noise_w")


# ---------------------------------- CLI ----------------------------------- #
def test_cli_lines_carry_their_own_speaker(pack, monkeypatch):
    from sonata_amd.audio.wav import wav_bytes
    from sonata_amd.frontends import cli
    from sonata_amd.models import voice as voice_mod

    loaded = []
    real_load = voice_mod.load_voice

    def load(*a, **k):
        loaded.append(real_load(*a, **k))
        return loaded[-1]

    monkeypatch.setattr(voice_mod, "load_voice", load)
    text = "ɡˈʊd mˈɔɹnɪŋ tu ju."
    buf = io.BytesIO()
    lines = io.StringIO(
        json.dumps({"text": text, "speaker_id": 1}) + "\n"
        + json.dumps({"text": text, "speaker_id": 2, "length_scale": 1.3})
        + "\n" + json.dumps({"text": text}) + "\n")
    rc = cli.main([pack, "--device", "cpu", "-s", "0", "--noise-w", "0.7"],
                  stdin=lines, stdout=buf)
    assert rc == 0
    v = loaded[0]
    default = SynthesisConfig(0, 0.667, 1.0, 0.7)
    assert v.get_synthesis_config() == default
    want = b""
    for cfg in (SynthesisConfig(1, 0.667, 1.0, 0.7),
                SynthesisConfig(2, 0.667, 1.3, 0.7), default):
        ph = list(v.phonemize_text(text))
        base = v.get_synthesis_config()
        v.set_synthesis_config(cfg)
        try:
            samples = np.concatenate(
                [a.samples for a in v.speak_batch(ph)])
        finally:
            v.set_synthesis_config(base)
        want += wav_bytes(samples, v.config.sample_rate)
    assert buf.getvalue() == want
