"""Continuous prosody for realtime streams on the CPU: StreamProsody (the
NumPy streaming stretcher, audio.prosody) against ops.apply_prosody_rows on
the whole row, bit for bit and for every chunking; then the voice API, the
StreamBatcher and synthesize_streamed against the one-shot result of the
concatenated plain stream.

The streaming rules reproduce the one-shot functions operation for
operation, so the comparisons are on the int32 views of the float samples;
the one exception (streams decoded in different company) is explained at
TOL."""

import threading

import numpy as np
import pytest
import torch

from stream_oracle import SENTENCES

import prosody_oracle as po

# Streams that share a round are decoded in another batch than alone: the
# plain audio then differs by fp32 reassociation (at most 4.1e-8 measured,
# bound 1e-6: tests/test_stream_batch_cpu.py).  Resampling and overlap-add
# are convex combinations and every gain is <= 1, so with the same frames
# chosen the bound carries over unchanged; lengths are exact.
TOL = 1e-6

TRIPLES = [(1.3, .8, 1.05), (.75, .5, .9), (1, 1, 1.2), (5.5, 1, 1),
           (.5, .3, .5), (1, .5, 1), (2, 1, 1.5), (1, 1, 1)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(got, want, what=""):
    assert got.dtype == np.float32, what
    assert got.shape == want.shape, f"{what}: {got.shape} != {want.shape}"
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


def _one_shot(x, sr, triple):
    from sonata_amd import ops

    y, n = ops.apply_prosody_rows(
        torch.from_numpy(np.ascontiguousarray(x)).reshape(1, -1), [len(x)],
        sr, [triple[0]], [triple[1]], [triple[2]])
    return y[0, : int(n[0])].numpy()


def _chunkings(n, half):
    out = [[n]]
    sizes, left = [], n
    for c in (1, half - 1, half + 1, 700, 1100, 2048):
        c = min(c, left)
        if c:
            sizes.append(c)
            left -= c
    if left:
        sizes.append(left)
    out.append(sizes)
    out.append([768] * (n // 768) + ([n % 768] if n % 768 else []))
    if n <= 1500:
        out.append([1] * n)
    return out


def _lengths(sr):
    from sonata_amd.audio.prosody import wsola_plan

    frame, half, search = wsola_plan(0, 1.0, sr)[:3]
    return (0, 1, frame - 1, frame, frame + search + 1, 1500, 6007), half


def _signal(seed, n, sr):
    # half noise, half voiced: near-ties and decisive frames both occur
    return (po.noise(seed, n) if seed % 2 else po.voiced(seed, n, sr))


_WANT = {}


def _want(sr, n, triple):
    key = (sr, n, triple)
    if key not in _WANT:
        x = _signal(n, n, sr)
        _WANT[key] = (x, _one_shot(x, sr, triple))
    return _WANT[key]


@pytest.mark.parametrize("triple", TRIPLES, ids=str)
@pytest.mark.parametrize("sr", [16000, 22050])
def test_stream_prosody_equals_one_shot(sr, triple):
    from sonata_amd.audio.prosody import StreamProsody

    lengths, half = _lengths(sr)
    for n in lengths:
        x, want = _want(sr, n, triple)
        for sizes in _chunkings(n, half):
            assert sum(sizes) == n
            sp = StreamProsody(n, sr, *triple)
            parts, at = [], 0
            for i, c in enumerate(sizes):
                parts.append(sp.push(x[at: at + c], i == len(sizes) - 1))
                at += c
            if not sizes:
                parts.append(sp.push(x[:0], True))
            got = np.concatenate(parts)
            what = f"sr {sr} n {n} triple {triple} chunks {sizes[:8]}"
            assert sp.n_out == len(want), what
            _same_bits(got, want, what)


@pytest.mark.parametrize("sr", [16000, 22050])
def test_carry_stays_within_one_search_segment(sr):
    """While frames remain a WSOLA stage keeps less than 2*search + frame
    samples (the one-shot kernel's seg_cap sizes the device carry), the
    resample stage at most one; at high speed nothing is kept and input is
    skipped."""
    from sonata_amd.audio.prosody import (ResampleStreamPlan,
                                          WsolaStreamPlan, wsola_plan)

    frame, half, search = wsola_plan(0, 1.0, sr)[:3]
    cap = 2 * search + frame
    skipped = 0
    for speed in (0.5, 0.75, 1.37, 2.0, 5.5):
        for n in (frame, frame + search + 1, 6007, 40000):
            for c in (1, 7, half, 768, 2048, n):
                pl = WsolaStreamPlan(n, speed, sr)
                left, worst = n, 0
                while left:
                    p = pl.push(min(c, left))
                    left -= p.m
                    assert 0 <= p.carry_len <= cap and p.keep_len <= cap
                    assert p.keep_pos >= p.in_pos
                    if pl.k_next < pl.n_frames:
                        assert p.keep_len < cap
                    if p.keep_pos > p.a0 + p.m:
                        skipped += 1
                    worst = max(worst, p.keep_len)
                assert pl.closed and pl.emitted == pl.n_out
                assert p.keep_len == 0
    assert skipped > 0
    for ratio in (0.5, 0.8, 1.3, 1.5):
        for n in (2, 3, 1500, 6007):
            for c in (1, 2, 3, 768, n):
                pl = ResampleStreamPlan(n, ratio)
                left = n
                while left:
                    p = pl.push(min(c, left))
                    left -= p.m
                    assert p.carry_len <= 1 and p.keep_len <= 1
                assert pl.emitted == pl.n_out


# ------------------------------ the voice API ------------------------------- #
E2E_TRIPLES = [(1.3, .8, 1.05), None, (1, .5, 1), (.75, 1, 1)]


@pytest.fixture(scope="module")
def plain(xlow_voice):
    got = [[] for _ in SENTENCES]
    for i, chunk in xlow_voice.stream_synthesis_batch(SENTENCES, 45, 3):
        got[i].append(chunk)
    return got


@pytest.fixture(scope="module")
def want(xlow_voice, plain):
    """apply_prosody_rows of each sentence's concatenated plain stream."""
    sr = xlow_voice.audio_output_info().sample_rate
    out = []
    for chunks, t in zip(plain, E2E_TRIPLES):
        x = np.concatenate(chunks)
        out.append(x if t is None else _one_shot(x, sr, t))
    return out


def _collect(it, n):
    got = [[] for _ in range(n)]
    for i, chunk in it:
        got[i].append(chunk)
    return got


def test_stream_synthesis_batch_with_prosody(xlow_voice, plain, want):
    from sonata_amd.audio.samples import to_i16

    v = xlow_voice
    got = _collect(v.stream_synthesis_batch(SENTENCES, 45, 3,
                                            prosody=E2E_TRIPLES), 4)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(plain[i])  # one chunk per round, empty or not
        _same_bits(np.concatenate(g), w, f"sentence {i}")
    pcm = _collect(v.stream_synthesis_batch(SENTENCES, 45, 3, pcm=True,
                                            prosody=E2E_TRIPLES), 4)
    for g, f in zip(pcm, got):
        assert [len(c) for c in g] == [len(c) for c in f]
        for a, b in zip(g, f):
            assert a.dtype == np.int16
            np.testing.assert_array_equal(a, to_i16(b))
    assert len(v._tail_free) == v._tails.shape[0]
    assert not v._infer_lock.locked()


def test_other_chunk_sizes(xlow_voice, want):
    """Per-row chunk sizes: still the one-shot result of that plain stream
    (which itself depends on where the decode is cut), and the lengths are
    those of any other chunking."""
    v = xlow_voice
    sr = v.audio_output_info().sample_rate
    sizes = [30, 90, 45, 61]
    plain = _collect(v.stream_synthesis_batch(SENTENCES, sizes, 3), 4)
    got = _collect(v.stream_synthesis_batch(SENTENCES, sizes, 3,
                                            prosody=E2E_TRIPLES), 4)
    for i, t in enumerate(E2E_TRIPLES):
        x = np.concatenate(plain[i])
        w = x if t is None else _one_shot(x, sr, t)
        _same_bits(np.concatenate(got[i]), w, f"sentence {i}")
        assert len(w) == len(want[i])


def test_reused_slots_equal_a_fresh_voice(xlow_voice, xlow_voice_path, want):
    """Run one stream to its end, close another midway, then open streams
    that get those slots back: what the earlier streams left in the slots'
    state never reaches the later ones."""
    from sonata_amd.models import load_voice

    v = xlow_voice
    first = v.stream_open(SENTENCES[:2], 45, 3,
                          prosody=[(.5, .3, .5), (2, 1, 1.5)])
    used = {s.slot for s in first}
    v.stream_round(first)
    v.stream_round(first)
    v.stream_close([first[1]])              # abandoned midway
    while not first[0].done:                # run to its end
        v.stream_round(first[:1])
    assert all(s.slot is None for s in first)
    again = v.stream_open(SENTENCES, 45, 3, prosody=E2E_TRIPLES)
    assert used <= {s.slot for s in again}
    got = [[] for _ in SENTENCES]
    while any(not s.done for s in again):
        for s, chunk in v.stream_round(again):
            got[s.index].append(chunk)
    fresh = load_voice(xlow_voice_path)
    ref = _collect(fresh.stream_synthesis_batch(SENTENCES, 45, 3,
                                                prosody=E2E_TRIPLES), 4)
    for i in range(4):
        _same_bits(np.concatenate(got[i]), np.concatenate(ref[i]),
                   f"sentence {i}")
        _same_bits(np.concatenate(got[i]), want[i], f"sentence {i}")


# ------------------------------ StreamBatcher ------------------------------- #
def test_stream_batcher_staggered_mixed_triples(xlow_voice):
    from sonata_amd.synth.batcher import StreamBatcher

    v = xlow_voice
    order = [3, 0, 1, 2]
    triples = [E2E_TRIPLES[i] for i in order]
    solo = []
    for i, t in zip(order, triples):
        sb = StreamBatcher(v)
        try:
            solo.append(list(sb.open(SENTENCES[i], 45, 3, prosody=t)))
        finally:
            sb.close()
    sb = StreamBatcher(v, max_streams=8, max_wait_ms=1.0)
    try:
        started = [threading.Event() for _ in order]
        results, errors = {}, []

        def consumer(k):
            try:
                if k:
                    assert started[k - 1].wait(60)
                chunks = []
                for c in sb.open(SENTENCES[order[k]], 45, 3,
                                 prosody=triples[k]):
                    chunks.append(c)
                    started[k].set()
                started[k].set()
                results[k] = chunks
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
                started[k].set()

        threads = [threading.Thread(target=consumer, args=(k,))
                   for k in range(len(order))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(120)
        assert not errors, errors
    finally:
        sb.close()
    for k in range(len(order)):
        assert all(len(c) for c in results[k])  # empty chunks stay inside
        got, ref = np.concatenate(results[k]), np.concatenate(solo[k])
        assert got.dtype == np.float32 and got.shape == ref.shape
        assert float(np.abs(got - ref).max()) <= TOL, f"stream {k}"
    assert len(v._tail_free) == v._tails.shape[0]


# --------------------------- synthesize_streamed ---------------------------- #
TEXT = ("This is a long test of the streaming path, with many words in "
        "it. One two three four five six seven eight nine ten.")


def _per_sentence_want(v, cfg):
    """One-shot prosody of each sentence's concatenated plain stream (chunk
    size grows per sentence, as synthesize_streamed does), then silence."""
    from sonata_amd.audio.samples import generate_silence

    sr = v.audio_output_info().sample_rate
    out = []
    for k, sent in enumerate(v.phonemize_text(TEXT)):
        x = np.concatenate([c for _, c in v.stream_synthesis_batch(
            [sent], min(45 * (k + 1), 1024), 3)])
        out.append(_one_shot(x, sr, cfg.prosody_triple()))
        if cfg.appended_silence_ms:
            out.append(generate_silence(cfg.appended_silence_ms, sr))
    return np.concatenate(out)


def test_synthesize_streamed_default_is_per_chunk(xlow_voice, monkeypatch):
    from sonata_amd.synth import AudioOutputConfig, SonataSpeechSynthesizer

    monkeypatch.delenv("SONATA_STREAM_PROSODY", raising=False)
    v = xlow_voice
    sr = v.audio_output_info().sample_rate
    cfg = AudioOutputConfig(rate=16, volume=80, pitch=55)
    synth = SonataSpeechSynthesizer(v)
    assert synth.stream_prosody == "chunk"
    got = list(synth.synthesize_streamed(TEXT, cfg))
    want = []
    for k, sent in enumerate(v.phonemize_text(TEXT)):
        for chunk in v.stream_synthesis(sent, min(45 * (k + 1), 1024), 3):
            want.append(cfg.apply(chunk, sr))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        _same_bits(g, w)


@pytest.mark.parametrize("batcher", [False, True])
def test_synthesize_streamed_continuous(xlow_voice, batcher):
    from sonata_amd.synth import (AudioOutputConfig, SonataSpeechSynthesizer,
                                  StreamBatcher)

    v = xlow_voice
    cfg = AudioOutputConfig(rate=16, volume=80, pitch=55,
                            appended_silence_ms=20)
    synth = SonataSpeechSynthesizer(v)
    synth.stream_prosody = "continuous"
    if batcher:
        synth.stream_batcher = StreamBatcher(v)
    try:
        got = list(synth.synthesize_streamed(TEXT, cfg))
    finally:
        if batcher:
            synth.stream_batcher.close()
    assert all(len(c) for c in got)
    _same_bits(np.concatenate(got), _per_sentence_want(v, cfg))


def test_stream_prosody_knob(xlow_voice, monkeypatch):
    from sonata_amd.synth import AudioOutputConfig, SonataSpeechSynthesizer

    monkeypatch.setenv("SONATA_STREAM_PROSODY", "continuous")
    synth = SonataSpeechSynthesizer(xlow_voice)
    assert synth.stream_prosody == "continuous"
    cfg = AudioOutputConfig(rate=16)
    got = np.concatenate(list(synth.synthesize_streamed(TEXT, cfg)))
    _same_bits(got, _per_sentence_want(xlow_voice, cfg))
    monkeypatch.setenv("SONATA_STREAM_PROSODY", "sometimes")
    with pytest.raises(ValueError):
        SonataSpeechSynthesizer(xlow_voice)
