"""Output sample rate for realtime streams on the CPU: the streaming plan of
audio.resample (PolyStreamPlan / PolyStream) against resample_poly on the
whole row, bit for bit and for every chunking; then the op's CPU path, the
voice API, the StreamBatcher and the synthesizer's stream_resample knob.

PolyStream forms every output from the same float64 products in the same
order as resample_poly, so all comparisons are on the int32 views of the
float samples."""

import numpy as np
import pytest
import torch

from stream_oracle import SENTENCES

import stream_resample_oracle as so

from sonata_amd.audio import resample as R


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(got, want, what=""):
    assert got.dtype == np.float32, what
    assert got.shape == want.shape, f"{what}: {got.shape} != {want.shape}"
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


def _signal(n):
    return np.random.default_rng(n).uniform(-1, 1, n).astype(np.float32)


@pytest.mark.parametrize("pair", so.ALL_PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_plan_streaming_equals_resample_poly(pair):
    rate_in, rate_out = pair
    d = R.design(rate_in, rate_out)
    worst = 0
    for n in so.lengths(d):
        x = _signal(n)
        want = R.resample_poly(x, rate_in, rate_out)
        assert len(want) == R.out_len(n, rate_in, rate_out)
        all_sizes = so.chunkings(n, d.K)
        assert len(all_sizes) >= 4
        for sizes in all_sizes:
            what = f"{pair} n {n} chunks {sizes[:8]}"
            ps = R.PolyStream(n, rate_in, rate_out)
            parts, at = [], 0
            for i, c in enumerate(sizes):
                parts.append(ps.push(x[at : at + c], i == len(sizes) - 1))
                at += c
                assert len(ps._carry) <= d.K - 1, what
                worst = max(worst, len(ps._carry))
            assert ps.n_out == len(want), what
            assert sum(len(p) for p in parts) == len(want), what
            _same_bits(np.concatenate(parts), want, what)
    assert worst == d.K - 1, "the carry reaches K - 1"


def test_plan_lengths_and_parity():
    d = R.design(22050, 8000)
    plan = R.PolyStreamPlan(4000, 22050, 8000)
    assert plan.carry_cap == d.K - 1 == 88
    pushes = [plan.push(c, last) for c, last in
              [(10, False), (0, False), (50, False), (3000, False),
               (940, True)]]
    assert [p.parity for p in pushes] == [0, 1, 0, 1, 0]
    assert pushes[0].carry_len == 0  # a first push names no carry
    assert pushes[0].e1 == 0 and pushes[0].keep_len == 10  # nothing ready
    assert pushes[1].e1 == pushes[1].e0 and pushes[1].keep_len == 10
    assert pushes[2].carry_len == 10 and pushes[2].keep_len == 60
    for a, b in zip(pushes, pushes[1:]):
        assert b.e0 == a.e1 and b.a0 == a.a0 + a.m
        assert (b.carry_pos, b.carry_len) == (a.keep_pos, a.keep_len)
    assert pushes[-1].e1 == plan.n_out == R.out_len(4000, 22050, 8000)
    with pytest.raises(AssertionError):
        plan.push(0)  # after the last chunk
    with pytest.raises(AssertionError):
        R.PolyStreamPlan(100, 22050, 8000).push(101)
    with pytest.raises(AssertionError):
        R.PolyStreamPlan(100, 22050, 8000).push(99, last=True)


def test_op_cpu_rows_through_their_streams():
    from sonata_amd import ops

    rate_in, rate_out = 22050, 8000
    lens = [3000, 1200, 37]
    xs = [_signal(n + 1)[:n] for n in lens]
    sizes = [[1000, 0, 1500, 500], [50, 60, 70, 1020], [37]]
    streams = [R.PolyStream(n, rate_in, rate_out) for n in lens[:2]] + [None]
    got = [[] for _ in lens]
    at = [0, 0, 0]
    for rnd in range(4):
        rows = [r for r in range(3) if rnd < len(sizes[r])]
        cl = [sizes[r][rnd] for r in rows]
        x = torch.full((len(rows), max(cl) + 3), float("nan"))
        for i, r in enumerate(rows):
            x[i, : cl[i]] = torch.from_numpy(xs[r][at[r] : at[r] + cl[i]])
            at[r] += cl[i]
        y, out = ops.resample_poly_stream_rows(
            x, cl, [streams[r] for r in rows], rows, None,
            last=[rnd == len(sizes[r]) - 1 for r in rows])
        assert y.shape[1] % 8 == 0 and y.shape[1] >= 8
        y = y.numpy()
        assert np.isfinite(y).all()
        for i, r in enumerate(rows):
            assert not y[i, int(out[i]):].any()
            got[r].append(y[i, : int(out[i])])
    for r in range(2):
        _same_bits(np.concatenate(got[r]),
                   R.resample_poly(xs[r], rate_in, rate_out), f"row {r}")
    _same_bits(np.concatenate(got[2]), xs[2], "copy row")


# ------------------------------ the voice API ------------------------------- #
S3 = SENTENCES[:3]
TRIPLES = [(1.3, .8, 1.05), None, (.75, 1, 1)]


def _collect(it, n):
    got = [[] for _ in range(n)]
    for i, chunk in it:
        got[i].append(chunk)
    return got


@pytest.fixture(scope="module")
def plain(xlow_voice):
    return _collect(xlow_voice.stream_synthesis_batch(S3, 45, 3), 3)


@pytest.fixture(scope="module")
def plain_prosody(xlow_voice):
    return _collect(xlow_voice.stream_synthesis_batch(
        S3, 45, 3, prosody=TRIPLES), 3)


def test_stream_synthesis_batch_at_8k(xlow_voice, plain):
    from sonata_amd.audio.samples import to_i16

    v = xlow_voice
    sr = v.audio_output_info().sample_rate
    got = _collect(v.stream_synthesis_batch(S3, 45, 3, sample_rate=8000), 3)
    for i in range(3):
        assert len(got[i]) == len(plain[i])  # one chunk per round
        _same_bits(np.concatenate(got[i]),
                   R.resample_poly(np.concatenate(plain[i]), sr, 8000),
                   f"sentence {i}")
    pcm = _collect(v.stream_synthesis_batch(S3, 45, 3, pcm=True,
                                            sample_rate=8000), 3)
    for g, f in zip(pcm, got):
        assert [len(c) for c in g] == [len(c) for c in f]
        for a, b in zip(g, f):
            assert a.dtype == np.int16
            np.testing.assert_array_equal(a, to_i16(b))
    assert len(v._tail_free) == v._tails.shape[0]
    assert not v._infer_lock.locked()


def test_stream_synthesis_batch_rate_after_prosody(xlow_voice, plain_prosody):
    v = xlow_voice
    sr = v.audio_output_info().sample_rate
    got = _collect(v.stream_synthesis_batch(
        S3, 45, 3, prosody=TRIPLES, sample_rate=8000), 3)
    for i in range(3):
        _same_bits(np.concatenate(got[i]),
                   R.resample_poly(np.concatenate(plain_prosody[i]), sr,
                                   8000), f"sentence {i}")


def test_stream_synthesis_batch_mixed_rates(xlow_voice, plain):
    v = xlow_voice
    sr = v.audio_output_info().sample_rate
    rates = [None, 8000, 48000]
    got = _collect(v.stream_synthesis_batch(S3, 45, 3, sample_rate=rates), 3)
    for i, rate in enumerate(rates):
        _same_bits(np.concatenate(got[i]),
                   R.resample_poly(np.concatenate(plain[i]), sr, rate),
                   f"sentence {i}")
    # the voice's own rate is the identity; a bad rate is refused at open
    same = _collect(v.stream_synthesis_batch(S3, 45, 3, sample_rate=sr), 3)
    for i in range(3):
        _same_bits(np.concatenate(same[i]), np.concatenate(plain[i]))
    with pytest.raises(ValueError):
        v.stream_open(S3, 45, 3, sample_rate=[None, 1000, None])
    assert len(v._tail_free) == v._tails.shape[0]


def test_stream_batcher_open_with_rate(xlow_voice, plain):
    from sonata_amd.synth.batcher import StreamBatcher

    v = xlow_voice
    sr = v.audio_output_info().sample_rate
    sb = StreamBatcher(v)
    try:
        for i, rate in ((0, 8000), (2, 48000), (1, sr)):
            chunks = list(sb.open(S3[i], 45, 3, sample_rate=rate))
            assert all(len(c) for c in chunks)  # empty chunks stay inside
            # alone in its rounds: the same decode as a batch of one
            x = np.concatenate([c for _, c in v.stream_synthesis_batch(
                [S3[i]], 45, 3)])
            _same_bits(np.concatenate(chunks), R.resample_poly(x, sr, rate),
                       f"sentence {i}")
        with pytest.raises(ValueError):
            sb.open(S3[0], 45, 3, sample_rate=1000)
    finally:
        sb.close()
    assert not sb._worker.is_alive()
    assert len(v._tail_free) == v._tails.shape[0]


# --------------------------- synthesize_streamed ---------------------------- #
TEXT = ("This is a long test of the streaming path, with many words in "
        "it. One two three four five six seven eight nine ten.")


def test_stream_resample_knob(xlow_voice, monkeypatch):
    from sonata_amd.synth import (AudioOutputConfig, SonataSpeechSynthesizer,
                                  StreamBatcher)
    from sonata_amd.synth import synthesizer as synth_mod

    v = xlow_voice
    cfg = AudioOutputConfig(sample_rate=8000, appended_silence_ms=20)
    monkeypatch.delenv("SONATA_STREAM_RESAMPLE", raising=False)
    assert SonataSpeechSynthesizer(v).stream_resample == "host"
    monkeypatch.setenv("SONATA_STREAM_RESAMPLE", "sometimes")
    with pytest.raises(ValueError):
        SonataSpeechSynthesizer(v)
    monkeypatch.setenv("SONATA_STREAM_RESAMPLE", "device")
    assert SonataSpeechSynthesizer(v).stream_resample == "device"
    monkeypatch.delenv("SONATA_STREAM_RESAMPLE")

    calls = []
    real_open = v.stream_open

    def spy_open(*a, **kw):
        calls.append(kw)
        return real_open(*a, **kw)

    monkeypatch.setattr(v, "stream_open", spy_open)
    built = []
    real_rs = synth_mod.StreamResampler

    def spy_rs(*a, **kw):
        built.append(a)
        return real_rs(*a, **kw)

    monkeypatch.setattr(synth_mod, "StreamResampler", spy_rs)

    out = {}
    for knob in ("host", "device"):
        for batcher in (True, False):
            synth = SonataSpeechSynthesizer(v)
            synth.stream_resample = knob
            if batcher:
                synth.stream_batcher = StreamBatcher(v)
            del calls[:], built[:]
            try:
                got = list(synth.synthesize_streamed(TEXT, cfg))
            finally:
                if batcher:
                    synth.stream_batcher.close()
            assert all(len(c) for c in got)
            out[knob, batcher] = np.concatenate(got)
            if knob == "host":
                assert built and all(
                    "sample_rate" not in kw for kw in calls)
            else:
                assert not built and calls and all(
                    kw.get("sample_rate") is not None for kw in calls)
    # through the batcher both knobs see the same decode: equal bit for bit
    _same_bits(out["device", True], out["host", True])
    # without it "host" streams through stream_synthesis, whose chunks equal
    # the batched path's: the same samples again
    _same_bits(out["device", False], out["host", False])
    _same_bits(out["device", False], out["device", True])
    # silence is counted at the output rate
    n_sil = int(0.020 * 8000)
    assert not out["device", True][-n_sil:].any()


def test_device_knob_leaves_host_prosody_alone(xlow_voice):
    """Per-chunk prosody runs on the host and must come before the rate
    conversion: the knob then changes nothing."""
    from sonata_amd.synth import AudioOutputConfig, SonataSpeechSynthesizer

    cfg = AudioOutputConfig(rate=16, sample_rate=8000)
    got = {}
    for knob in ("host", "device"):
        synth = SonataSpeechSynthesizer(xlow_voice)
        synth.stream_resample = knob
        got[knob] = list(synth.synthesize_streamed(TEXT, cfg))
    assert len(got["host"]) == len(got["device"])
    for a, b in zip(got["host"], got["device"]):
        _same_bits(a, b)
