"""Streaming prosody kernels (csrc/prosody.hip: wsola_stream_rows,
resample_stream_rows) and the voice's continuous stream prosody on the GPU.

The stages are judged as the one-shot kernels are (tests/prosody_oracle.py):
the concatenation of what a row emits over its rounds, with the concatenated
targets, must be an acceptable WSOLA of the WHOLE input under
wsola_plan(n, ...), every sample within the derived bound.  On decisive
inputs (margin >= 2, asserted) and for the resample stage the streamed result
is the one-shot kernel's bit for bit, for every chunking.  Shapes are the
smallest that reach every branch: rows that run several, one or no frame in
a round, rows that finish early and drop out, skipped input at speed 5.5,
pass-through rows, one-sample chunks."""

import numpy as np
import pytest
import torch

import prosody_oracle as po
from sonata_amd import ops
from sonata_amd.audio.prosody import (ResampleStreamPlan, StreamProsodyPlan,
                                      WsolaStreamPlan, wsola_plan)
from sonata_amd.audio.window import hann_window

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = np.float32(1e3)


def _chunking(kind, n, half):
    if kind == "whole":
        return [n] if n else [0]
    if kind == "ones":
        return [1] * n
    if kind == "768":
        return [768] * (n // 768) + ([n % 768] if n % 768 else [])
    sizes, left = [], n
    for c in (1, half - 1, half + 1, 700, 1100, 2048):
        c = min(c, left)
        if c:
            sizes.append(c)
            left -= c
    if left:
        sizes.append(left)
    return sizes


def _round_rows(rows, sizes, at, r, pad):
    """Rows still fed in round r: (row indices, chunk tensor, lengths).  The
    valid part of each chunk row is followed by the canary."""
    live = [b for b in range(len(rows)) if r < len(sizes[b])]
    lens = [sizes[b][r] for b in live]
    x = np.full((len(live), max(lens) + pad), CANARY, dtype=np.float32)
    for i, b in enumerate(live):
        x[i, : lens[i]] = rows[b][at[b]: at[b] + lens[i]]
        at[b] += lens[i]
    return live, torch.from_numpy(x).to(DEV), lens


def _canary_state(sr, n_slots):
    """A state whose every buffer starts full of the canary: what an earlier
    stream left in a slot, and the slots no row names."""
    st = ops.ProsodyStreamState(sr, DEV)
    st.reserve(n_slots)
    for t in [st.rs_carry] + st.carry + st.tails:
        t.fill_(float(CANARY))
    return st


def _unnamed_untouched(st, slots, which):
    free = [s for s in range(st.slots) if s not in slots]
    assert free
    for t in which:
        assert (t[free].cpu().numpy() == CANARY).all()


def _stream_wsola(rows, speeds, gains, slots, sizes, sr, st, stage=1):
    """Feed rows[b] in chunks of sizes[b] through one streaming WSOLA stage.
    Returns per row (output, targets, plan object)."""
    plans = [WsolaStreamPlan(len(x), s, sr) for x, s in zip(rows, speeds)]
    outs = [[] for _ in rows]
    tgts = [[] for _ in rows]
    at = [0] * len(rows)
    for r in range(max(len(s) for s in sizes)):
        live, xd, lens = _round_rows(rows, sizes, at, r, pad=5)
        pushes = [plans[b].push(n) for b, n in zip(live, lens)]
        y, out, t = ops.wsola_stream_rows(
            xd, lens, pushes, [slots[b] for b in live], st.carry[stage],
            st.tails[stage], st.window, st.half, st.search,
            gain=[gains[b] for b in live], return_targets=True)
        assert y.shape[1] % 8 == 0
        y, t = y.cpu().numpy(), t.cpu().numpy()
        for i, (b, p) in enumerate(zip(live, pushes)):
            n = int(out[i])
            assert n == p.e1 - p.e0
            assert not y[i, n:].any(), f"row {b} round {r}: padding"
            nk = 0 if p.passthrough else p.nk
            assert (t[i, nk:] == -1).all() and (t[i, :nk] >= 0).all()
            outs[b].append(y[i, :n])
            tgts[b].append(t[i, :nk])
    for b, pl in enumerate(plans):
        assert pl.received == len(rows[b]) and pl.emitted == pl.n_out
    return ([np.concatenate(o) for o in outs],
            [np.concatenate(t) for t in tgts], plans)


# --------------------------------------------------------------------------- #
# the WSOLA stage alone
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("sr", [16000, 22050])
def test_wsola_stage_streams(sr):
    frame, half, search = wsola_plan(0, 1.0, sr)[:3]
    w = hann_window(frame)
    rows = [po.noise(1, 4000), po.voiced(2, 3000, sr), po.noise(3, 3500),
            po.voiced(4, 4000, sr), po.noise(5, 3900),
            po.noise(6, 3100),            # speed 1: pass-through
            po.noise(7, frame - 1),       # shorter than a frame
            po.voiced(8, 1200, sr)]       # fed one sample at a time
    speeds = [0.5, 0.75, 1.37, 2.0, 5.5, 1.0, 0.75, 0.75]
    gains = [1.0, 0.5, 0.3, 1.0, 0.8, 0.5, 0.7, 1.0]
    kinds = ["mixed", "768", "whole", "mixed", "768", "mixed", "768",
             "ones" if sr == 16000 else "mixed"]
    sizes = [_chunking(k, len(x), half) for k, x in zip(kinds, rows)]
    assert len({len(s) for s in sizes}) >= 3  # rows leave in different rounds
    slots = [5, 2, 9, 0, 7, 3, 11, 8]
    st = _canary_state(sr, 13)
    ys, ts, plans = _stream_wsola(rows, speeds, gains, slots, sizes, sr, st)
    for b, (x, s, g) in enumerate(zip(rows, speeds, gains)):
        tag = f"sr {sr} row {b} (n={len(x)}, speed {s})"
        if plans[b].passthrough:
            assert np.array_equal(ys[b], x * np.float32(g)), tag
            assert len(ts[b]) == 0
            continue
        plan = wsola_plan(len(x), s, sr)
        assert len(ts[b]) == plan[4], tag
        po.wsola_check(x, plan, w, ts[b], ys[b], gain=g, what=tag)
    _unnamed_untouched(st, slots, [st.carry[1], st.tails[1]])
    # the other stage's buffers were never named at all
    assert (st.carry[0].cpu().numpy() == CANARY).all()
    assert (st.tails[0].cpu().numpy() == CANARY).all()


@pytest.mark.parametrize("sr", [16000, 22050])
def test_wsola_stage_is_the_one_shot_kernel_on_decisive_inputs(sr):
    frame, half, search = wsola_plan(0, 1.0, sr)[:3]
    w = hann_window(frame)
    cases = [c for c in po.EXACT_CASES if c[1] == sr]
    assert len(cases) >= 4
    rows = [po.noise(seed, n) for seed, _, n, _ in cases]
    speeds = [c[3] for c in cases]
    gains = [1.0, 0.5] * 3
    gains = gains[: len(rows)]
    for x, speed in zip(rows, speeds):  # the precondition
        plan = wsola_plan(len(x), speed, sr)
        _, t_np = po.wsola_f32(x, plan, w)
        rp = po.wsola_replay(x, plan, w, t_np)
        assert rp.margin[rp.searched].min() >= 2.0
    x_all = np.zeros((len(rows), max(len(x) for x in rows)), np.float32)
    for b, x in enumerate(rows):
        x_all[b, : len(x)] = x
    lens = [len(x) for x in rows]
    y1, out1, t1 = ops.wsola_rows(torch.from_numpy(x_all).to(DEV), lens, sr,
                                  speeds, gain=gains, return_targets=True)
    y1, t1 = y1.cpu().numpy(), t1.cpu().numpy()
    slots = [4, 1, 6, 0, 3, 2][: len(rows)]
    for kind in ("whole", "mixed", "768"):
        sizes = [_chunking(kind, n, half) for n in lens]
        st = _canary_state(sr, 8)
        ys, ts, _ = _stream_wsola(rows, speeds, gains, slots, sizes, sr, st)
        for b in range(len(rows)):
            tag = f"{cases[b]} {kind}"
            K, n_out = wsola_plan(lens[b], speeds[b], sr)[4:6]
            assert int(out1[b]) == n_out == len(ys[b]), tag
            assert np.array_equal(ts[b], t1[b, :K]), tag
            assert ys[b].tobytes() == y1[b, :n_out].tobytes(), tag


# --------------------------------------------------------------------------- #
# the resample stage
# --------------------------------------------------------------------------- #
def _stream_resample(rows, ratios, slots, sizes, st):
    plans = [ResampleStreamPlan(len(x), r) for x, r in zip(rows, ratios)]
    outs = [[] for _ in rows]
    at = [0] * len(rows)
    for r in range(max(len(s) for s in sizes)):
        live, xd, lens = _round_rows(rows, sizes, at, r, pad=3)
        pushes = [plans[b].push(n) for b, n in zip(live, lens)]
        y, out = ops.resample_stream_rows(
            xd, lens, pushes, [slots[b] for b in live], st.rs_carry)
        assert y.shape[1] % 8 == 0
        y = y.cpu().numpy()
        for i, (b, p) in enumerate(zip(live, pushes)):
            n = int(out[i])
            assert n == p.e1 - p.e0
            assert not y[i, n:].any()
            outs[b].append(y[i, :n])
    for b, pl in enumerate(plans):
        assert pl.emitted == pl.n_out
    return [np.concatenate(o) for o in outs]


def test_resample_stage_is_the_one_shot_kernel():
    sr = 22050
    half = wsola_plan(0, 1.0, sr)[1]
    ratios = [0.5, 0.8, 1.3, 1.5, 1.0, 1.3]
    rows = [po.noise(1, 3000), po.voiced(2, 4000, sr), po.noise(3, 3501),
            po.voiced(4, 3999, sr), po.noise(5, 3000), po.noise(6, 700)]
    lens = [len(x) for x in rows]
    x_all = np.zeros((len(rows), max(lens)), np.float32)
    for b, x in enumerate(rows):
        x_all[b, : len(x)] = x
    y1, out1 = ops.resample_linear_rows(torch.from_numpy(x_all).to(DEV),
                                        lens, ratios)
    y1 = y1.cpu().numpy()
    slots = [3, 0, 5, 1, 6, 4]
    kinds = [["whole"] * 6, ["mixed"] * 6, ["768"] * 6,
             ["mixed", "768", "whole", "768", "mixed", "ones"]]
    for ks in kinds:
        sizes = [_chunking(k, n, half) for k, n in zip(ks, lens)]
        st = _canary_state(sr, 8)
        ys = _stream_resample(rows, ratios, slots, sizes, st)
        for b in range(len(rows)):
            n = int(out1[b])
            assert len(ys[b]) == n, (b, ks[b])
            assert ys[b].tobytes() == y1[b, :n].tobytes(), (b, ks[b])
        _unnamed_untouched(st, slots, [st.rs_carry])


def test_wrappers_refuse_what_would_read_outside():
    sr = 16000
    st = ops.ProsodyStreamState(sr, DEV)
    st.reserve(2)
    x = torch.zeros((1, 2000), device=DEV)
    pl = WsolaStreamPlan(4000, 0.75, sr)
    p = pl.push(2000)
    assert p.nk > 0
    args = (st.carry[1], st.tails[1], st.window, st.half, st.search)
    with pytest.raises(RuntimeError, match="outside"):  # frames need 2000
        ops.wsola_stream_rows(x[:, :1500], [1500],
                              [p._replace(m=1500)], [0], *args)
    with pytest.raises(RuntimeError, match="carry"):
        ops.wsola_stream_rows(x, [2000], [p._replace(carry_len=9999)], [0],
                              *args)
    with pytest.raises(RuntimeError, match="slot"):
        ops.wsola_stream_rows(x, [2000], [p], [2], *args)
    rp = ResampleStreamPlan(4000, 1.3).push(2000)
    with pytest.raises(RuntimeError, match="outside"):
        ops.resample_stream_rows(x[:, :1000], [1000], [rp._replace(m=1000)],
                                 [0], st.rs_carry)
    with pytest.raises(RuntimeError, match="LDS"):
        ops.wsola_stream_rows(
            x, [2000], [p], [0], torch.zeros((1, 18000), device=DEV),
            torch.zeros((1, 6000), device=DEV),
            torch.zeros(12000, device=DEV), 6000, 3000)


# --------------------------------------------------------------------------- #
# end to end on an x_low voice
# --------------------------------------------------------------------------- #
SENTENCES = ["hˈɛloʊ wˈɝld, ðɪs ɪz ɐ lˈɔŋɡɚ sˈɛntəns tə stɹˈiːm.",
             "ɡˈʊd mˈɔːnɪŋ tʊ jˈuː.", "wˈʌn tˈuː θɹˈiː fˈɔːɹ fˈaɪv sˈɪks.",
             "hˈɛloʊ."]
TRIPLES = [(1.3, 0.8, 1.05), (0.75, 0.5, 0.9), None, (1.0, 0.5, 1.0)]


def _staged(chunks, triple, sr):
    """One stream's plain chunks through the stage ops by hand, keeping every
    stage's whole input, output and targets: judged by replay, and what the
    voice emits must be exactly this chain."""
    st = _canary_state(sr, 2)
    pl = StreamProsodyPlan(sum(len(c) for c in chunks), sr, *triple)
    w = hann_window(pl.frame)
    g_pitch = pl.gain if pl.do_pitch and not pl.do_speed else 1.0
    g_speed = pl.gain if pl.do_speed or not pl.do_pitch else 1.0
    keep = {k: [] for k in ("rs", "wp", "tp", "ws", "ts", "in_s")}
    outs = []
    for i, c in enumerate(chunks):
        step = pl.push(len(c), i == len(chunks) - 1)
        y = torch.from_numpy(np.ascontiguousarray(c)).reshape(1, -1).to(DEV)
        n = torch.tensor([len(c)])
        if pl.do_pitch:
            y, n = ops.resample_stream_rows(y, n, [step.resample], [1],
                                            st.rs_carry)
            keep["rs"].append(y[0, : int(n[0])].cpu().numpy())
            y, n, t = ops.wsola_stream_rows(
                y, n, [step.wsola_pitch], [1], st.carry[0], st.tails[0],
                st.window, st.half, st.search, gain=[g_pitch],
                return_targets=True)
            keep["wp"].append(y[0, : int(n[0])].cpu().numpy())
            keep["tp"].append(t[0, : step.wsola_pitch.nk].cpu().numpy())
        keep["in_s"].append(y[0, : int(n[0])].cpu().numpy())
        if pl.do_speed or not pl.do_pitch:
            y, n, t = ops.wsola_stream_rows(
                y, n, [step.wsola_speed], [1], st.carry[1], st.tails[1],
                st.window, st.half, st.search, gain=[g_speed],
                return_targets=True)
            if step.wsola_speed is not None:
                keep["ts"].append(t[0, : step.wsola_speed.nk].cpu().numpy())
        outs.append(y[0, : int(n[0])].cpu().numpy())
    x = np.concatenate(chunks)
    decisive = True
    cur = x
    if pl.do_pitch:
        rs = np.concatenate(keep["rs"])
        ref, bound = po.resample_ref(x, pl.resample.n_out)
        po.assert_within(rs, ref, bound, "resample stage")
        wp = np.concatenate(keep["wp"])
        if pl.wsola_pitch.passthrough:
            assert np.array_equal(wp, rs * np.float32(g_pitch))
        else:
            plan = wsola_plan(len(rs), 1.0 / triple[2], sr)
            rp = po.wsola_check(rs, plan, w, np.concatenate(keep["tp"]), wp,
                                gain=g_pitch, what="pitch stretch")
            decisive &= bool((rp.margin[rp.searched] >= 2.0).all())
        cur = wp
    out = np.concatenate(outs)
    if pl.do_speed and not pl.wsola_speed.passthrough:
        plan = wsola_plan(len(cur), triple[0], sr)
        rp = po.wsola_check(cur, plan, w, np.concatenate(keep["ts"]), out,
                            gain=g_speed, what="speed stretch")
        decisive &= bool((rp.margin[rp.searched] >= 2.0).all())
    else:
        assert np.array_equal(out, cur * np.float32(g_speed))
    assert len(out) == pl.n_out
    return outs, decisive


@pytest.mark.parametrize("engine", ["auto", "python"])
def test_voice_streams_with_continuous_prosody(xlow_voice_path, engine):
    from sonata_amd.audio.samples import to_i16
    from sonata_amd.models import load_voice

    v = load_voice(xlow_voice_path, device=DEV, engine=engine)
    assert (v._engine is not None) == (engine == "auto")
    sr = v.audio_output_info().sample_rate
    n = len(SENTENCES)

    def run(**kw):
        got = [[] for _ in range(n)]
        for i, chunk in v.stream_synthesis_batch(SENTENCES, 45, 3, **kw):
            got[i].append(chunk)
        return got

    plain = run()
    again = run()
    got = run(prosody=TRIPLES)
    pcm = run(prosody=TRIPLES, pcm=True)
    assert max(len(p) for p in plain) >= 3  # several rounds, rows drop out
    for b in range(n):
        tag = f"sentence {b}"
        x = np.concatenate(plain[b])
        assert x.tobytes() == np.concatenate(again[b]).tobytes(), tag
        assert len(got[b]) == len(plain[b]), tag  # one chunk per round
        y = np.concatenate(got[b])
        for a, f in zip(pcm[b], got[b]):
            assert a.dtype == np.int16
            assert np.array_equal(a, to_i16(f)), tag
        if TRIPLES[b] is None:
            assert y.tobytes() == x.tobytes(), tag
            continue
        sp, vo, pi = TRIPLES[b]
        xd = torch.from_numpy(x).reshape(1, -1).to(DEV)
        one, one_len = ops.apply_prosody_rows(xd, [len(x)], sr, [sp], [vo],
                                              [pi])
        _, cpu_len = ops.apply_prosody_rows(xd.cpu(), [len(x)], sr, [sp],
                                            [vo], [pi])
        assert len(y) == int(one_len[0]) == int(cpu_len[0]), tag
        staged, decisive = _staged(plain[b], TRIPLES[b], sr)
        assert [len(c) for c in got[b]] == [len(c) for c in staged], tag
        assert y.tobytes() == np.concatenate(staged).tobytes(), tag
        if decisive:
            assert y.tobytes() == one[0, : len(y)].cpu().numpy().tobytes(), \
                tag
    assert len(v._tail_free) == v._tails.shape[0]

    # slots are reused: a stream closed midway leaves nothing a later one reads
    first = v.stream_open(SENTENCES[:2], 45, 3, prosody=[(0.5, 0.3, 0.5),
                                                         (2.0, 1.0, 1.5)])
    v.stream_round(first)
    v.stream_close(first)
    redo = run(prosody=TRIPLES)
    for b in range(n):
        assert np.concatenate(redo[b]).tobytes() == \
            np.concatenate(got[b]).tobytes()


def test_synthesize_streamed_continuous_on_the_device(xlow_voice_path):
    from sonata_amd.models import load_voice
    from sonata_amd.synth import (AudioOutputConfig, SonataSpeechSynthesizer,
                                  StreamBatcher)

    v = load_voice(xlow_voice_path, device=DEV)
    sr = v.audio_output_info().sample_rate
    text = "This is a test of the streaming path. One two three four five."
    cfg = AudioOutputConfig(rate=16, volume=80, pitch=55)
    synth = SonataSpeechSynthesizer(v)
    synth.stream_prosody = "continuous"
    want = []
    for k, sent in enumerate(v.phonemize_text(text)):
        chunks = [c for _, c in v.stream_synthesis_batch(
            [sent], min(45 * (k + 1), 1024), 3)]
        want.append(np.concatenate(_staged(chunks, cfg.prosody_triple(),
                                           sr)[0]))
    want = np.concatenate(want)
    alone = list(synth.synthesize_streamed(text, cfg))
    synth.stream_batcher = StreamBatcher(v)
    try:
        through = list(synth.synthesize_streamed(text, cfg))
    finally:
        synth.stream_batcher.close()
    for got in (alone, through):
        assert all(len(c) for c in got)
        assert np.concatenate(got).tobytes() == want.tobytes()
