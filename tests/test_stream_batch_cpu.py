"""Batched realtime streams on the CPU: the op fallbacks against the host
oracle (bit for bit), VitsVoice.stream_open / stream_round /
stream_synthesis_batch against stream_synthesis per stream, StreamBatcher,
and the opt-in route of synthesize_streamed.

The 1e-6 bound on samples: batched net.decode(..., lengths) of a round's
windows differs from the single-window decode by fp32 reassociation between
batch sizes only, measured at most 4.1e-8 on a signal peak of 0.054 for these
sentences (207, 262, 28 and 348 frames: 3, 3, 1 and 4 chunks).  1e-6 leaves
about 25x over that and is 2e-5 of the peak.  Past length*hop the batched
decoder output is not zero on the CPU (about 0.05), so the same comparison
shows that the seam never reads past hi + ext."""

import threading

import numpy as np
import pytest
import torch

from stream_oracle import SENTENCES, run_gather_cases, run_seam_cases

TOL = 1e-6


# ------------------------------- op fallbacks ------------------------------- #
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [96, 192])
def test_gather_windows_fallback(C, dtype):
    run_gather_cases("cpu", C, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_stream_seam_rows_fallback(dtype):
    run_seam_cases("cpu", dtype)


def test_seam_wrapper_asserts_what_the_chunker_guarantees():
    from sonata_amd import ops

    wav = torch.zeros((1, 1, 512))
    tails = torch.zeros((2, 42))
    ramp = torch.zeros(42)
    ok = dict(lo=0, hi=400, ext=42, prev_ext=42, slot=0)
    ops.stream_seam_rows(wav, **ok, tails_in=tails, ramp=ramp)
    for bad in (dict(prev_ext=7), dict(ext=41), dict(hi=500),
                dict(lo=380), dict(slot=2)):
        with pytest.raises(AssertionError):
            ops.stream_seam_rows(wav, **{**ok, **bad}, tails_in=tails,
                                 ramp=ramp)
    with pytest.raises(AssertionError):  # a window past its source row
        ops.gather_windows([torch.zeros((1, 4, 10))], [0], [0], [3], [8], 8)


# ------------------------------ the voice API ------------------------------- #
@pytest.fixture(scope="module")
def single(xlow_voice):
    """stream_synthesis per sentence: the reference every test shares."""
    return [list(xlow_voice.stream_synthesis(s, 45, 3)) for s in SENTENCES]


def _lens(chunks):
    return [len(c) for c in chunks]


def _same(got_chunks, want_chunks):
    assert _lens(got_chunks) == _lens(want_chunks)
    got, want = np.concatenate(got_chunks), np.concatenate(want_chunks)
    assert got.dtype == np.float32
    assert float(np.abs(got - want).max()) <= TOL


def test_stream_synthesis_batch_equals_stream_synthesis(xlow_voice, single):
    v = xlow_voice
    assert [len(c) for c in single] == [3, 3, 1, 4]
    got = [[] for _ in SENTENCES]
    for i, chunk in v.stream_synthesis_batch(SENTENCES, 45, 3):
        got[i].append(chunk)
    for g, w in zip(got, single):
        _same(g, w)
    assert not v._infer_lock.locked()
    assert len(v._tail_free) == v._tails.shape[0]  # every slot came back


def test_rounds_join_and_leave(xlow_voice, single):
    v = xlow_voice
    states = v.stream_open(SENTENCES, 45, 3)
    assert [s.frames for s in states] == [207, 262, 28, 348]
    assert len({s.slot for s in states}) == 4
    got = [[] for _ in SENTENCES]
    live_per_round = []
    while any(not s.done for s in states):
        out = v.stream_round(states)
        live_per_round.append([s.index for s, _ in out])
        for s, chunk in out:
            got[s.index].append(chunk)
    assert len(live_per_round[0]) >= 3          # a real shared round
    assert live_per_round[1] == [0, 1, 3]       # the one-shot stream left
    assert live_per_round[-1] == [3]            # one stream runs a round on
    assert len(live_per_round) == 4
    assert v.stream_round(states) == []
    for g, w in zip(got, single):
        _same(g, w)
    assert all(s.slot is None for s in states)


def test_per_row_chunk_size(xlow_voice, single):
    v = xlow_voice
    want = list(single)
    want[1] = list(v.stream_synthesis(SENTENCES[1], 90, 3))
    assert _lens(want[1]) != _lens(single[1])
    got = [[] for _ in SENTENCES]
    for i, chunk in v.stream_synthesis_batch(SENTENCES, [45, 90, 45, 45], 3):
        got[i].append(chunk)
    assert [_lens(g) for g in got] == [_lens(w) for w in want]


def test_pcm_chunks_and_abandoned_iterator(xlow_voice, single):
    from sonata_amd.audio.samples import to_i16

    v = xlow_voice
    floats = [[] for _ in SENTENCES]
    for i, chunk in v.stream_synthesis_batch(SENTENCES, 45, 3):
        floats[i].append(chunk)
    got = [[] for _ in SENTENCES]
    for i, chunk in v.stream_synthesis_batch(SENTENCES, 45, 3, pcm=True):
        assert chunk.dtype == np.int16
        got[i].append(chunk)
    for g, f in zip(got, floats):
        assert _lens(g) == _lens(f)
        for a, b in zip(g, f):
            np.testing.assert_array_equal(a, to_i16(b))
    # an iterator closed midway gives its slots back and leaves the lock free
    it = v.stream_synthesis_batch(SENTENCES, 45, 3)
    next(it)
    assert len(v._tail_free) < v._tails.shape[0]
    it.close()
    assert len(v._tail_free) == v._tails.shape[0]
    assert not v._infer_lock.locked()


def test_two_speakers_share_a_round(tmp_path):
    from sonata_amd.models import create_random_voice, load_voice

    v = load_voice(create_random_voice(str(tmp_path), "spk3", quality="x_low",
                                       num_speakers=3))
    cfg = v.get_synthesis_config()
    want, states = [], []
    for sid, sent in ((0, SENTENCES[0]), (2, SENTENCES[1])):
        cfg.speaker_id = sid
        v.set_synthesis_config(cfg)
        want.append(list(v.stream_synthesis(sent, 45, 3)))
        states += v.stream_open([sent], 45, 3)
    assert states[0].z is not states[1].z and states[0].g is not None
    assert not torch.equal(states[0].g, states[1].g)
    got = [[], []]
    while any(not s.done for s in states):
        out = v.stream_round(states)
        assert len(out) == 2  # both advance in every round (3 chunks each)
        for k, (s, chunk) in enumerate(out):
            assert s is states[k]
            got[k].append(chunk)
    for g, w in zip(got, want):
        _same(g, w)
    # and the speakers do differ: the rows were conditioned apart
    a = np.concatenate(want[0])
    cfg.speaker_id = 2
    v.set_synthesis_config(cfg)
    b = np.concatenate(list(v.stream_synthesis(SENTENCES[0], 45, 3)))
    assert len(a) != len(b) or float(np.abs(a - b).max()) > 100 * TOL


# ------------------------------ StreamBatcher ------------------------------- #
def _no_batcher_threads():
    return not [t for t in threading.enumerate()
                if t.name == "sonata_stream_batcher"]


def test_stream_batcher_staggered_waves(xlow_voice, single):
    from sonata_amd.synth.batcher import StreamBatcher

    v = xlow_voice
    rounds = []
    real_round = v.stream_round

    second_queued = threading.Event()

    def counting_round(states, pcm=False):
        rounds.append(len([s for s in states if not s.done]))
        return real_round(states, pcm=pcm)

    v.stream_round = counting_round
    sb = StreamBatcher(v, max_streams=8, max_wait_ms=1.0)
    real_admit = sb._admit

    def gated_admit(n_live):
        if n_live:
            # the second stream is queued before the first one's second tick:
            # its 48-frame window and the first one's 96 share a bucket
            assert second_queued.wait(60)
        return real_admit(n_live)

    sb._admit = gated_admit
    try:
        # thread k opens when thread k-1 has its first chunk: the second wave
        # arrives while the first is mid-stream.  Longest sentence first.
        order = [3, 0, 1, 2]
        started = [threading.Event() for _ in order]
        results, errors = {}, []

        def consumer(k):
            try:
                if k:
                    assert started[k - 1].wait(60)
                chunks = []
                it = sb.open(SENTENCES[order[k]], 45, 3)
                if k == 1:
                    second_queued.set()
                for c in it:
                    chunks.append(c)
                    started[k].set()
                results[k] = chunks
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
                started[k].set()
                second_queued.set()

        threads = [threading.Thread(target=consumer, args=(k,))
                   for k in range(len(order))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(120)
        assert not errors, errors
        for k, i in enumerate(order):
            _same(results[k], single[i])
        assert rounds[:2] == [1, 2]  # the newcomer joined a live stream

        # one consumer leaves after its first chunk, the others finish, and a
        # speak_batch from another thread completes while streams are live
        its = [sb.open(SENTENCES[i], 45, 3) for i in (3, 0, 1)]
        first = next(its[0])
        assert len(first) == len(single[3][0])
        its[0].close()
        spoken = []
        t = threading.Thread(
            target=lambda: spoken.append(v.speak_batch([SENTENCES[2]])))
        t.start()
        _same(list(its[1]), single[0])
        _same(list(its[2]), single[1])
        t.join(60)
        assert spoken and len(spoken[0][0].samples) == len(single[2][0])
    finally:
        del v.stream_round
        sb.close()
    assert not sb._worker.is_alive()
    assert _no_batcher_threads()
    assert len(v._tail_free) == v._tails.shape[0]
    with pytest.raises(RuntimeError):
        sb.open(SENTENCES[2])


def test_stream_batcher_error_reaches_the_round_and_service_goes_on(
        xlow_voice, single):
    from sonata_amd.synth.batcher import StreamBatcher

    v = xlow_voice
    real_round = v.stream_round
    fail = [True]

    def flaky_round(states, pcm=False):
        if fail[0]:
            fail[0] = False
            raise ValueError("round failed")
        return real_round(states, pcm=pcm)

    v.stream_round = flaky_round
    sb = StreamBatcher(v, max_wait_ms=50.0)
    try:
        its = [sb.open(SENTENCES[i], 45, 3) for i in (0, 2)]
        for it in its:
            with pytest.raises(ValueError, match="round failed"):
                list(it)
        _same(list(sb.open(SENTENCES[1], 45, 3)), single[1])
    finally:
        del v.stream_round
        sb.close()
    assert _no_batcher_threads()
    assert len(v._tail_free) == v._tails.shape[0]


def test_bucket_rule_runs_short_windows_first():
    from sonata_amd.synth.batcher import StreamBatcher, _StreamHandle

    class _S:
        def __init__(self, n):
            from sonata_amd.models.chunker import ChunkSpec

            self.next_spec = ChunkSpec(0, n, 0, 0, False)

    hs = []
    for n, pcm in ((225, False), (48, False), (93, False), (96, False),
                   (231, False), (51, True)):
        h = _StreamHandle("x", 45, 3, pcm)
        h.state = _S(n)
        hs.append(h)
    got = [[(h.window(), h.pcm) for h in b] for b in StreamBatcher._buckets(hs)]
    assert got == [[(48, False), (93, False), (96, False)], [(51, True)],
                   [(225, False), (231, False)]]


# ------------------------------ opt-in wiring ------------------------------- #
def test_grpc_voice_attaches_a_stream_batcher_only_when_asked(
        xlow_voice, monkeypatch):
    from sonata_amd.frontends.grpc.server import _Voice
    from sonata_amd.synth import SonataSpeechSynthesizer, StreamBatcher

    monkeypatch.delenv("SONATA_STREAM_BATCH", raising=False)
    off = _Voice("1", SonataSpeechSynthesizer(xlow_voice))
    assert off.synth.stream_batcher is None
    off.close()
    monkeypatch.setenv("SONATA_STREAM_BATCH", "1")
    on = _Voice("2", SonataSpeechSynthesizer(xlow_voice))
    try:
        assert isinstance(on.synth.stream_batcher, StreamBatcher)
        assert on.synth.stream_batcher.model is xlow_voice
    finally:
        on.close()
    assert _no_batcher_threads()


# --------------------------- synthesize_streamed ---------------------------- #
def test_synthesize_streamed_through_the_stream_batcher(xlow_voice):
    from sonata_amd.synth import (AudioOutputConfig, SonataSpeechSynthesizer,
                                  StreamBatcher)

    text = ("This is a long test of the streaming path, with many words in "
            "it. One two three four five six seven eight nine ten.")
    cfg = AudioOutputConfig(volume=50, appended_silence_ms=20)
    synth = SonataSpeechSynthesizer(xlow_voice)
    assert synth.stream_batcher is None
    want = [list(synth.synthesize_streamed(text, c)) for c in (None, cfg)]
    assert len(want[0]) > 2
    synth.stream_batcher = StreamBatcher(xlow_voice)
    try:
        opened = []
        real_open = synth.stream_batcher.open
        synth.stream_batcher.open = \
            lambda *a, **k: opened.append(a) or real_open(*a, **k)
        got = [list(synth.synthesize_streamed(text, c)) for c in (None, cfg)]
    finally:
        synth.stream_batcher.close()
    assert len(opened) == 2 * len(xlow_voice.phonemize_text(text))
    for g, w in zip(got, want):
        _same(g, w)
    assert _no_batcher_threads()
