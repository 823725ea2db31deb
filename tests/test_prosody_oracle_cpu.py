"""Batched prosody on the CPU: the replay oracle has teeth, the batched ops
equal the per-row NumPy functions bit for bit, and the prosody triple
travels through speak_batch / DynamicBatcher / the synthesizer.

The GPU counterpart (tests/test_gpu_prosody.py) judges the HIP kernels
with the same oracle and the same inputs."""

import numpy as np
import pytest
import torch

import prosody_oracle as po
from sonata_amd import ops
from sonata_amd.audio.prosody import (apply_prosody, resample_linear,
                                      resample_out_len, time_stretch_wsola,
                                      wsola_plan)
from sonata_amd.audio.window import hann_window
from sonata_amd.synth import DynamicBatcher
from sonata_amd.synth.synthesizer import (AudioOutputConfig,
                                          SonataSpeechSynthesizer)


def _plan_win(n, speed, sr, **kw):
    plan = wsola_plan(n, speed, sr, **kw)
    return plan, hann_window(plan[0])


# --------------------------------------------------------------------------- #
# shared arithmetic
# --------------------------------------------------------------------------- #
def test_plan_matches_the_numpy_functions():
    """wsola_plan / resample_out_len give the lengths the NumPy functions
    produce (22050 Hz: the odd 661-sample frame becomes 660)."""
    assert wsola_plan(9001, 1.37, 22050)[:3] == (660, 330, 220)
    assert wsola_plan(9001, 1.37, 16000)[:3] == (480, 240, 160)
    for sr in (16000, 22050):
        for n in (700, 1500, 4000, 9001):
            x = po.noise(n, n)
            for speed in (0.5, 0.75, 1.37, 2.0, 5.5):
                assert len(time_stretch_wsola(x, speed, sr)) == \
                    wsola_plan(n, speed, sr)[5]
            for ratio in (0.5, 0.75, 1.3, 1.5):
                assert len(resample_linear(x, ratio)) == \
                    resample_out_len(n, ratio)


# --------------------------------------------------------------------------- #
# the oracle has teeth
# --------------------------------------------------------------------------- #
def _matrix():
    for sr in (16000, 22050):
        frame, _, search = wsola_plan(0, 1.0, sr)[:3]
        for n in po.matrix_lengths(frame, search):
            if n < frame:
                continue  # pass-through rows: no WSOLA to replay
            for speed in po.SPEEDS:
                if abs(speed - 1.0) < 1e-3:
                    continue
                yield sr, n, speed


def test_restatement_is_the_numpy_algorithm_and_is_accepted():
    """wsola_f32 without a planted defect IS time_stretch_wsola (bitwise),
    and the oracle accepts it on every matrix input, noise and voiced."""
    n_cases = 0
    for sr, n, speed in _matrix():
        for x in (po.noise(n, n), po.voiced(n, n, sr)):
            plan, w = _plan_win(n, speed, sr)
            y, t = po.wsola_f32(x, plan, w)
            assert np.array_equal(y, time_stretch_wsola(x, speed, sr))
            po.wsola_check(x, plan, w, t, y, what=f"{sr}/{n}/{speed}")
            n_cases += 1
    assert n_cases == 2 * 6 * 5 * 2


def test_search_ms_30_restatement_accepted():
    x = po.noise(3, 9001)
    plan, w = _plan_win(9001, 0.75, 22050, search_ms=30.0)
    assert plan[2] == 661
    y, t = po.wsola_f32(x, plan, w)
    assert np.array_equal(
        y, time_stretch_wsola(x, 0.75, 22050, search_ms=30.0))
    po.wsola_check(x, plan, w, t, y)


def _decisive_frame(rp):
    ks = [k for k in range(len(rp.margin))
          if rp.searched[k] and rp.margin[k] >= 2]
    assert ks, "no frame with margin >= 2"
    return ks[len(ks) // 2]


@pytest.mark.parametrize("d", [1, -1])
def test_rejects_target_moved_by_one(d):
    x = po.noise(0, 4000)
    plan, w = _plan_win(4000, 0.5, 16000)
    y, t = po.wsola_f32(x, plan, w)
    k = _decisive_frame(po.wsola_replay(x, plan, w, t))
    y2, t2 = po.wsola_f32(x, plan, w, move_target=(k, d))
    assert t2[k] == t[k] + d
    rp = po.wsola_replay(x, plan, w, t2)
    assert any(p.startswith(f"frame {k}:") for p in rp.problems), rp.problems


@pytest.mark.parametrize("value", [0.0, 0.25])
def test_rejects_last_index_tie_break(value):
    x = np.full(4000, value, dtype=np.float32)
    plan, w = _plan_win(4000, 0.75, 16000)
    y, t = po.wsola_f32(x, plan, w)
    rp = po.wsola_check(x, plan, w, t, y)
    assert rp.searched.any()
    assert (t[rp.searched] == rp.lo[rp.searched]).all()
    y2, t2 = po.wsola_f32(x, plan, w, tie_last=True)
    assert (t2 != t).any()
    assert po.wsola_replay(x, plan, w, t2).problems


def _assert_output_rejected(x, plan, w, y, t):
    assert not po.wsola_replay(x, plan, w, t).problems  # targets are fine
    with pytest.raises(AssertionError):
        po.wsola_check(x, plan, w, t, y)


def test_rejects_skipped_normalisation():
    x = po.noise(0, 4000)
    plan, w = _plan_win(4000, 1.37, 16000)
    _assert_output_rejected(x, plan, w, *po.wsola_f32(x, plan, w,
                                                      skip_norm=True))


def test_rejects_window_shifted_by_one():
    x = po.noise(0, 4000)
    plan, w = _plan_win(4000, 1.37, 16000)
    _assert_output_rejected(x, plan, w, *po.wsola_f32(x, plan, w,
                                                      window_shift=1))


def test_rejects_dropped_lo_clamp():
    x = po.noise(0, 4000)
    plan, w = _plan_win(4000, 0.5, 16000)
    # frame 1 sits at t = 120 < search = 160: the clamp is live there
    assert po.frame_window(1, plan, 4000)[1] == 0
    y, t = po.wsola_f32(x, plan, w)
    y2, t2 = po.wsola_f32(x, plan, w, drop_lo_clamp=True)
    assert t2[1] != t[1]
    rp = po.wsola_replay(x, plan, w, t2)
    assert any(p.startswith("frame 1:") for p in rp.problems), rp.problems


def test_rejects_output_cut_at_frames():
    x = po.noise(0, 4000)
    plan, w = _plan_win(4000, 2.0, 16000)
    frame, half, _, _, K, n_out = plan
    assert n_out < K * half + frame  # int(n/speed) is the binding length
    y, t = po.wsola_f32(x, plan, w, cut_at_frames=True)
    assert len(y) == K * half + frame
    _assert_output_rejected(x, plan, w, y, t)


def test_rejects_f32_frame_positions():
    """Pinned by a CPU search: at 16 kHz and speed 1.37 (ana_hop 328.8),
    frame 45 sits at 14796 in double and at 14795 in f32 arithmetic.  On a
    constant input every searched frame must choose lo, so the shifted
    window shows."""
    n, sr, speed, k = 16000, 16000, 1.37, 45
    plan, w = _plan_win(n, speed, sr)
    hop = plan[3]
    assert int(k * hop) == 14796
    assert int(np.float32(k) * np.float32(hop)) == 14795
    assert plan[4] > k
    x = np.full(n, 0.25, dtype=np.float32)
    y, t = po.wsola_f32(x, plan, w)
    po.wsola_check(x, plan, w, t, y)
    y2, t2 = po.wsola_f32(x, plan, w, f32_positions=True)
    assert t2[k] != t[k]
    rp = po.wsola_replay(x, plan, w, t2)
    assert any(p.startswith(f"frame {k}:") for p in rp.problems), rp.problems


def test_exact_cases_are_decisive():
    """Precondition of the exact-equality tests (here and on the GPU):
    every searched frame of every EXACT_CASES input has margin >= 2."""
    assert len(po.EXACT_CASES) >= 8
    for seed, sr, n, speed in po.EXACT_CASES:
        x = po.noise(seed, n)
        plan, w = _plan_win(n, speed, sr)
        y, t = po.wsola_f32(x, plan, w)
        rp = po.wsola_check(x, plan, w, t, y)
        assert rp.searched.sum() >= 2
        assert rp.margin[rp.searched].min() >= 2.0, (seed, sr, n, speed)


def test_resample_ref_accepts_numpy_and_rejects_f32_positions():
    for n in (1, 2, 3, 1000, 4097):
        x = po.noise(n, n)
        for ratio in (0.5, 0.75, 1.5):
            y = resample_linear(x, ratio)
            ref, bound = po.resample_ref(x, len(y))
            po.assert_within(y, ref, bound, f"resample {n}/{ratio}")
    # positions in f32 land on other samples: far out of bound
    n, n_out = 4097, 8194
    x = po.noise(1, n)
    pos = (np.arange(n_out, dtype=np.float32) * np.float32(n - 1)
           / np.float32(n_out - 1))
    i0 = np.floor(pos).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    fr = pos - i0.astype(np.float32)
    bad = x[i0] * (1 - fr) + x[i1] * fr
    ref, bound = po.resample_ref(x, n_out)
    with pytest.raises(AssertionError):
        po.assert_within(bad, ref, bound)


# --------------------------------------------------------------------------- #
# CPU batched ops == per-row NumPy functions, bit for bit
# --------------------------------------------------------------------------- #
SR = 22050
FRAME = wsola_plan(0, 1.0, SR)[0]

# (n, speed, volume, pitch)
ROWS = [
    (5000, 1.0, 1.0, 1.0),          # nothing
    (4000, 1.0005, 1.0, 1.0),       # speed ~ 1: below the threshold
    (3000, 1.0, 0.8, 1.0),          # volume only
    (4100, 1.0, 1.0, 1.3),          # pitch only
    (4500, 0.75, 1.0, 1.0),         # speed only
    (6001, 3.75, 0.8, 1.05),        # all three
    (5200, 1.37, 0.5, 0.8),         # all three, pitch down
    (0, 1.37, 0.5, 0.8),            # empty row
    (FRAME - 1, 2.0, 0.5, 1.0),     # shorter than a frame: pass-through
    (FRAME - 1, 1.0, 1.0, 1.3),     # pitch on a short row
    (FRAME, 0.5, 1.0, 1.0),         # exactly one frame
]


def _batch(rows):
    lens = [r[0] for r in rows]
    x = np.zeros((len(rows), max(lens)), dtype=np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = po.noise(100 + b, n)
    return torch.from_numpy(x), lens


def _host_row(x, speed, volume, pitch):
    """apply_prosody plus the two pass-through rules of the batched API."""
    def stretch(r, s):
        if len(r) == 0 or len(r) < FRAME:
            return r.copy()
        return time_stretch_wsola(r, s, SR)

    if len(x) >= 2 * FRAME:  # no short row anywhere in the chain
        return apply_prosody(x, SR, speed=speed, volume=volume, pitch=pitch)
    y = x
    if abs(pitch - 1.0) >= 1e-3:
        y = stretch(resample_linear(y, pitch), 1.0 / pitch)
    if abs(speed - 1.0) >= 1e-3:
        y = stretch(y, speed)
    if abs(volume - 1.0) >= 1e-6:
        y = y * np.float32(volume)
    return y


def test_cpu_apply_prosody_rows_bitwise():
    x, lens = _batch(ROWS)
    y, out = ops.apply_prosody_rows(
        x, torch.tensor(lens), SR, speed=[r[1] for r in ROWS],
        volume=[r[2] for r in ROWS], pitch=[r[3] for r in ROWS])
    assert y.dtype == torch.float32 and y.shape[0] == len(ROWS)
    for b, (n, s, v, p) in enumerate(ROWS):
        want = _host_row(x[b, :n].numpy(), s, v, p)
        assert int(out[b]) == len(want), b
        assert np.array_equal(y[b, : len(want)].numpy(), want), b
        assert not y[b, len(want):].any(), b
    assert int(out[7]) == 0                      # empty stays empty
    assert int(out[8]) == FRAME - 1              # short row: copied, scaled
    assert np.array_equal(y[8, : FRAME - 1].numpy(),
                          x[8, : FRAME - 1].numpy() * np.float32(0.5))
    # rows 0-6 are long enough to go through apply_prosody itself
    assert all(r[0] >= 2 * FRAME for r in ROWS[:7])


def test_cpu_wsola_rows_and_resample_rows_bitwise():
    rows = [(4000, 0.5), (9001, 1.37), (3000, 1.0), (0, 2.0),
            (FRAME - 1, 2.0), (FRAME, 5.5)]
    x, lens = _batch([(n, s, 1.0, 1.0) for n, s in rows])
    y, out = ops.wsola_rows(x, lens, SR, [s for _, s in rows])
    for b, (n, s) in enumerate(rows):
        r = x[b, :n].numpy()
        want = r if (n < FRAME or s == 1.0) else time_stretch_wsola(r, s, SR)
        assert int(out[b]) == len(want)
        assert np.array_equal(y[b, : len(want)].numpy(), want), b
    ratios = [0.5, 0.75, 1.0, 1.5, 1.3, 0.9]
    y, out = ops.resample_linear_rows(x, lens, ratios)
    for b, ((n, _), ratio) in enumerate(zip(rows, ratios)):
        want = resample_linear(x[b, :n].numpy(), ratio)
        assert int(out[b]) == len(want)
        assert np.array_equal(y[b, : len(want)].numpy(), want), b


# --------------------------------------------------------------------------- #
# plumbing on the CPU x_low voice
# --------------------------------------------------------------------------- #
PHONEMES = ["hˈɛloʊ wˈɝld.", "wˈʌn tˈuː θɹˈiː fˈoːɹ fˈaɪv.", "ɡˈʊd mˈɔːnɪŋ."]
CONFIGS = [AudioOutputConfig(rate=65, volume=80, pitch=55),
           AudioOutputConfig(volume=50),
           AudioOutputConfig(rate=10)]


def test_prosody_triple_is_what_apply_uses():
    cfg = AudioOutputConfig(rate=65, volume=80, pitch=55)
    speed, volume, pitch = cfg.prosody_triple()
    assert (speed, volume, pitch) == (0.5 + 5.0 * 0.65, 0.8, 0.5 + 0.55)
    assert AudioOutputConfig().prosody_triple() == (1.0, 1.0, 1.0)
    x = po.noise(5, 6000)
    assert np.array_equal(
        cfg.apply(x, SR),
        apply_prosody(x, SR, speed=speed, volume=volume, pitch=pitch))


def test_speak_batch_prosody_equals_host_apply(xlow_voice):
    v = xlow_voice
    assert v.supports_device_prosody
    sr = v.audio_output_info().sample_rate
    plain = v.speak_batch(PHONEMES)
    triples = [c.prosody_triple() for c in CONFIGS]
    got = v.speak_batch(PHONEMES, prosody=triples)
    for a, g, c in zip(plain, got, CONFIGS):
        want = c.apply(a.samples, sr)
        assert g.samples.dtype == np.float32
        assert np.array_equal(g.samples, want)
    # a None row is left as it is
    got = v.speak_batch(PHONEMES, prosody=[None, triples[1], None])
    assert np.array_equal(got[0].samples, plain[0].samples)
    assert np.array_equal(got[1].samples, CONFIGS[1].apply(plain[1].samples,
                                                           sr))


class _RowModel:
    """Batch-invariant stand-in: the audio of a row depends on its
    phonemes alone, so whatever the batcher coalesces, a request must get
    what it gets alone — exactly."""

    def __init__(self, voice):
        self.voice = voice
        self.calls = []

    def speak_batch(self, phonemes, prosody=None):
        from sonata_amd.core import Audio

        self.calls.append((list(phonemes), prosody))
        info = self.voice.audio_output_info()
        rows = [po.noise(len(p), 3000 + 37 * len(p)) for p in phonemes]
        if prosody is not None:
            lens = [len(r) for r in rows]
            x = np.zeros((len(rows), max(lens)), dtype=np.float32)
            for b, r in enumerate(rows):
                x[b, : len(r)] = r
            tr = [p or (1.0, 1.0, 1.0) for p in prosody]
            y, out = ops.apply_prosody_rows(
                torch.from_numpy(x), lens, info.sample_rate,
                speed=[t[0] for t in tr], volume=[t[1] for t in tr],
                pitch=[t[2] for t in tr])
            rows = [y[b, : int(out[b])].numpy() for b in range(len(rows))]
        return [Audio(r, info) for r in rows]


def test_batcher_carries_per_row_prosody(xlow_voice):
    model = _RowModel(xlow_voice)
    sr = xlow_voice.audio_output_info().sample_rate
    phons = ["a" * (3 + i) for i in range(9)]
    cfgs = [CONFIGS[i % 3] if i % 4 else None for i in range(9)]
    alone = []
    for p, c in zip(phons, cfgs):
        a = model.speak_batch([p])[0].samples
        alone.append(a if c is None else c.apply(a, sr))
    model.calls.clear()
    batcher = DynamicBatcher(model, max_batch=16, max_wait_ms=200)
    futures = [batcher.submit(p, c.prosody_triple() if c else None)
               for p, c in zip(phons, cfgs)]
    got = [f.result(timeout=60).samples for f in futures]
    batcher.close()
    assert max(len(c[0]) for c in model.calls) > 1, "nothing coalesced"
    for g, want in zip(got, alone):
        assert np.array_equal(g, want)


def test_batcher_on_the_voice_mixed_prosody(xlow_voice):
    """The real voice behind the batcher: a coalesced mixed-prosody batch
    equals speak_batch of the same rows followed by the host prosody per
    row, exactly; against each request alone, lengths are exact and rows
    that are not stretched agree to the batch-padding tolerance the
    batcher tests use (a stretched row amplifies that 1e-5 into other
    frame choices, so only its length is compared)."""
    v = xlow_voice
    sr = v.audio_output_info().sample_rate
    cfgs = [CONFIGS[0], None, CONFIGS[1]]
    batcher = DynamicBatcher(v, max_batch=8, max_wait_ms=500)
    futures = [batcher.submit(p, c.prosody_triple() if c else None)
               for p, c in zip(PHONEMES, cfgs)]
    got = [f.result(timeout=120).samples for f in futures]
    batcher.close()
    order = sorted(range(3), key=lambda i: len(PHONEMES[i]))
    same_batch = v.speak_batch([PHONEMES[i] for i in order])
    for a, i in zip(same_batch, order):
        want = a.samples if cfgs[i] is None else cfgs[i].apply(a.samples, sr)
        if len(got[i]) == len(want) and np.array_equal(got[i], want):
            continue
        # the requests did not coalesce into one bucket: compare alone
        alone = v.speak_one_sentence(PHONEMES[i]).samples
        want = alone if cfgs[i] is None else cfgs[i].apply(alone, sr)
        assert len(got[i]) == len(want)
        if cfgs[i] is None or cfgs[i].rate is None and cfgs[i].pitch is None:
            np.testing.assert_allclose(got[i], want, atol=1e-5)


class _FakeCudaModel:
    """Looks like a cuda voice to the synthesizer; records what it is
    asked."""
    supports_device_prosody = True
    device = torch.device("cuda")

    def __init__(self, voice):
        self.voice = voice
        self.prosody_seen = []

    def phonemize_text(self, text):
        return self.voice.phonemize_text(text)

    def audio_output_info(self):
        return self.voice.audio_output_info()

    def speak_batch(self, phonemes, prosody=None):
        self.prosody_seen.append(prosody)
        return self.voice.speak_batch(phonemes, prosody=prosody)

    def speak_one_sentence(self, phonemes):
        return self.speak_batch([phonemes])[0]


TEXT = "Hello world. Good morning."


def test_synthesizer_device_path_selection(xlow_voice, monkeypatch, tmp_path):
    cfg = AudioOutputConfig(rate=65, volume=80, pitch=55,
                            appended_silence_ms=20)
    monkeypatch.delenv("SONATA_DEVICE_PROSODY", raising=False)
    # a CPU model never takes the device path
    cpu = SonataSpeechSynthesizer(xlow_voice)
    assert not cpu.device_prosody(cfg)
    host = [a.samples for a in cpu.synthesize_parallel(TEXT, cfg)]
    assert len(host) == 2

    fake = _FakeCudaModel(xlow_voice)
    synth = SonataSpeechSynthesizer(fake)
    assert synth.device_prosody(cfg)
    assert not synth.device_prosody(None)
    assert not synth.device_prosody(AudioOutputConfig(appended_silence_ms=5))
    dev = [a.samples for a in synth.synthesize_parallel(TEXT, cfg)]
    assert fake.prosody_seen == [[cfg.prosody_triple()] * 2]
    # same batch, same arithmetic on the CPU: identical, silence included
    for d, h in zip(dev, host):
        assert np.array_equal(d, h)
    lazy = [a.samples for a in synth.synthesize_lazy(TEXT, cfg)]
    assert [len(a) for a in lazy] == [len(a) for a in host]
    assert all(p == [cfg.prosody_triple()] for p in fake.prosody_seen[1:])
    out = synth.synthesize_to_file(str(tmp_path / "o.wav"), TEXT, cfg)
    assert np.array_equal(out.samples, np.concatenate(host))

    # SONATA_DEVICE_PROSODY=0: today's path, prosody never reaches the model
    monkeypatch.setenv("SONATA_DEVICE_PROSODY", "0")
    fake.prosody_seen.clear()
    assert not synth.device_prosody(cfg)
    off = [a.samples for a in synth.synthesize_parallel(TEXT, cfg)]
    assert fake.prosody_seen == [None]
    for o, h in zip(off, host):
        assert np.array_equal(o, h)
