"""Output sample rate for realtime streams on the device
(csrc/resample.hip, resample_poly_stream_rows): a round's outputs are those
of the one-shot kernel on the whole row, so per row the concatenated chunks
must equal ops.resample_rows BITWISE (same tap loop, same bank, tolerance 0)
and lie within resample_oracle.bound of the dense float64 oracle.  The state
is ping-pong: a round never writes the buffer it reads, and never touches a
slot it does not name.  Then the voice path on both engines, and one
StreamBatcher run with mixed rates."""

import threading

import numpy as np
import pytest
import torch

import resample_oracle as ro
import stream_resample_oracle as so
from sonata_amd import ops
from sonata_amd.audio import resample as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# M > L, L > M, L = 1, M = 1, and the ratio at which several tiles of one
# row read the carry
GPU_PAIRS = [(22050, 8000), (22050, 48000), (16000, 8000), (22050, 44100),
             (8000, 192000)]
SLOTS = [6, 2, 7, 0, 3]  # of an 8-slot state
N_SLOTS = 8


def _ibits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _row_sizes(d):
    """Chunk lengths of the five rows (3000 .. 6000 samples each).
    Row 0: pushes that emit exactly one tile, one tile + 1 (or the nearest
    counts the ratio reaches) and three tiles + 5.  Row 1 finishes early.
    Row 2 starts with rounds that emit nothing (less than the look-ahead).
    Row 3 has zero-length chunks.  Row 4 has three chunks in a row shorter
    than K - 1."""
    tile = ops.functional.RESAMPLE_TILE
    first = d.K + 10
    seen, done = first, so.ready(d, first)
    row0 = [first]
    for target, over in ((tile, False), (tile + 1, True),
                         (3 * tile + 5, True)):
        c = so.chunk_emitting(d, seen, done, target, over)
        row0.append(c)
        seen += c
        done = so.ready(d, seen)
    assert seen < 6000
    row0.append(6000 - seen)
    short = [20, 9, 31]
    assert all(c < d.K - 1 for c in short)
    sizes = [row0,
             [2000, 1000],
             [5, 7, 2, 1986, 1500, 500],
             [1500, 0, 1200, 0, 1800],
             [1000] + short + [1, 2000, 1339]]
    assert so.ready(d, 5 + 7 + 2) == 0
    for s in sizes:
        assert 3000 <= sum(s) <= 6000
    return sizes


@pytest.mark.parametrize("pair", GPU_PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_rounds_equal_the_one_shot_kernel(pair):
    rate_in, rate_out = pair
    d = R.design(rate_in, rate_out)
    sizes = _row_sizes(d)
    lens = [sum(s) for s in sizes]
    rng = np.random.default_rng(rate_out)
    xs = [rng.uniform(-1.0, 1.0, n).astype(np.float32) for n in lens]
    whole = torch.zeros((5, max(lens)))
    for r, x in enumerate(xs):
        whole[r, : lens[r]] = torch.from_numpy(x)
    one, one_len = ops.resample_rows(whole.to(DEV), lens, rate_in, rate_out)
    one = one.cpu().numpy()

    st = ops.PolyStreamState(rate_in, rate_out, DEV)
    st.reserve(N_SLOTS)
    assert tuple(st.carry.shape) == (N_SLOTS, 2, (d.K - 1 + 3) // 4 * 4)
    st.carry.fill_(float("nan"))  # a first push names no carry
    streams = [R.PolyStream(n, rate_in, rate_out) for n in lens]
    got = [[] for _ in lens]
    at = [0] * 5
    emitted = set()
    for rnd in range(max(len(s) for s in sizes)):
        rows = [r for r in range(5) if rnd < len(sizes[r])]
        cl = [sizes[r][rnd] for r in rows]
        x = torch.full((len(rows), max(cl) + 3), float("nan"))
        for i, r in enumerate(rows):
            x[i, : cl[i]] = torch.from_numpy(xs[r][at[r] : at[r] + cl[i]])
            at[r] += cl[i]
        before = _ibits(st.carry)
        parity = [streams[r].plan.parity for r in rows]
        y, out = ops.resample_poly_stream_rows(
            x.to(DEV), cl, [streams[r] for r in rows],
            [SLOTS[r] for r in rows], st,
            last=[rnd == len(sizes[r]) - 1 for r in rows])
        out = out.tolist()
        assert y.dtype == torch.float32 and y.shape[0] == len(rows)
        assert y.shape[1] % 8 == 0 and y.shape[1] >= 8
        assert y.shape[1] == max(-(-max(out) // 8) * 8, 8)
        y = y.cpu().numpy()
        assert np.isfinite(y).all(), "NaN behind a chunk's length was read"
        after = _ibits(st.carry)
        named = {SLOTS[r] for r in rows}
        for s in range(N_SLOTS):
            if s not in named:
                assert np.array_equal(after[s], before[s]), f"slot {s}"
        for i, r in enumerate(rows):
            assert not y[i, out[i]:].any(), "padding is zero"
            got[r].append(y[i, : out[i]])
            emitted.add(out[i])
            # the buffer this push read is not written
            assert np.array_equal(after[SLOTS[r], parity[i]],
                                  before[SLOTS[r], parity[i]]), f"row {r}"
    tile = ops.functional.RESAMPLE_TILE
    print(f"{pair}: row 0 emitted {[len(c) for c in got[0]]}")
    assert 0 in emitted
    if d.M >= d.L:  # every count is reached
        assert {tile, tile + 1, 3 * tile + 5} <= emitted
    assert any(tile - d.L // d.M - 1 <= n <= tile for n in emitted)
    assert any(n > 3 * tile for n in emitted)
    for r in range(5):
        y = np.concatenate(got[r])
        n_out = int(one_len[r])
        assert len(y) == n_out == R.out_len(lens[r], rate_in, rate_out)
        assert y.tobytes() == one[r, :n_out].tobytes(), f"row {r}"
        ref = ro.dense_oracle(xs[r], rate_in, rate_out)
        peak = float(np.abs(xs[r]).max())
        err = float(np.abs(y - ref).max())
        tol = ro.bound(d, peak)
        print(f"{pair} row {r} n={lens[r]} err={err:.3e} bound={tol:.3e}")
        assert err <= tol, (r, err, tol)


def test_copy_rows_ride_along():
    """Rows without a stream are copied by the same launch and touch no
    state; a round with no stream at all is x itself."""
    rate_in, rate_out = 22050, 8000
    st = ops.PolyStreamState(rate_in, rate_out, DEV)
    st.reserve(4)
    st.carry.fill_(float("nan"))
    before = _ibits(st.carry)
    rng = np.random.default_rng(5)
    x = torch.full((3, 1000), float("nan"))
    lens = [999, 700, 0]
    for b, n in enumerate(lens):
        x[b, :n] = torch.from_numpy(rng.uniform(-1, 1, n).astype(np.float32))
    ps = R.PolyStream(700, rate_in, rate_out)
    y, out = ops.resample_poly_stream_rows(
        x.to(DEV), lens, [None, ps, None], [0, 3, 1], st,
        last=[False, True, False])
    y = y.cpu().numpy()
    assert out.tolist() == [999, R.out_len(700, rate_in, rate_out), 0]
    assert y.shape[1] == 1000 and np.isfinite(y).all()
    assert y[0, :999].tobytes() == x[0, :999].numpy().tobytes()
    assert not y[0, 999:].any() and not y[2].any()
    one, _ = ops.resample_rows(x[1:2, :700].to(DEV), [700], rate_in, rate_out)
    assert y[1, : int(out[1])].tobytes() == one[0].cpu().numpy().tobytes()
    after = _ibits(st.carry)
    for s in (0, 1, 2):
        assert np.array_equal(after[s], before[s])
    xd = x.to(DEV)
    same, n = ops.resample_poly_stream_rows(xd, lens, [None] * 3, [0, 1, 2],
                                            st)
    assert same is xd and n.tolist() == lens


def test_binding_refuses_before_any_launch():
    ext = ops.hip_ext(required=True)
    rate_in, rate_out = 22050, 8000
    d = R.design(rate_in, rate_out)
    Kc = (d.K - 1 + 3) // 4 * 4
    st = ops.PolyStreamState(rate_in, rate_out, DEV)
    st.reserve(4)
    st.carry.copy_(torch.randn(st.carry.shape))
    before = _ibits(st.carry)
    bank = ops.functional._resample_bank(d, torch.device(DEV))
    x = torch.randn((2, 2000), device=DEV)
    p0 = R.PolyStreamPlan(4000, rate_in, rate_out).push(2000)
    p1 = R.PolyStreamPlan(2000, rate_in, rate_out).push(2000, True)
    n_out = -(-max(p0.e1, p1.e1) // 8) * 8

    def par(rows, slots=(1, 2)):
        flat = []
        for p, s in zip(rows, slots):
            flat += [s, p.m, p.a0, p.carry_pos, p.carry_len, p.n, p.e0, p.e1,
                     0, p.keep_pos, p.keep_len, p.parity]
        return flat

    def call(x=x, rows=(p0, p1), slots=(1, 2), state=st.carry, bank=bank,
             L=d.L, M=d.M, H=d.H, n_out=n_out):
        return ext.resample_poly_stream_rows(x, par(rows, slots), state,
                                             bank, L, M, H, n_out)

    y = call()  # the arguments are good as they stand
    assert tuple(y.shape) == (2, n_out)
    st.carry.copy_(torch.from_numpy(before).view(torch.float32))
    bad = {
        "cpu x": dict(x=x.cpu()),
        "non-contiguous x": dict(x=torch.randn((2000, 2), device=DEV).t()),
        "bf16 x": dict(x=x.to(torch.bfloat16)),
        "cpu state": dict(state=st.carry.cpu()),
        "non-contiguous state": dict(
            state=torch.zeros((4, 2, 2 * Kc), device=DEV)[:, :, ::2]),
        "state width": dict(state=torch.zeros((4, 2, Kc + 4), device=DEV)),
        "cpu bank": dict(bank=bank.cpu()),
        "bf16 bank": dict(bank=bank.to(torch.bfloat16)),
        "bank length": dict(bank=bank[:-1].contiguous()),
        "bank shape": dict(bank=bank.reshape(d.K, d.L)),
        "L above 1024": dict(L=1025, M=1, H=16 * 1025,
                             bank=torch.zeros(1025 * 33, device=DEV)),
        # span_cap = 255*64 + 2049 floats = 73 KB
        "LDS": dict(L=1, M=64, H=1024, bank=torch.zeros(2049, device=DEV),
                    state=torch.zeros((4, 2, 2048), device=DEV)),
        "m above N": dict(x=x[:, :1999].contiguous()),
        "carry_len above Kc": dict(rows=(p0._replace(carry_len=Kc + 1), p1)),
        "keep_len above Kc": dict(rows=(p0._replace(keep_len=Kc + 1), p1)),
        "emits more than n_out": dict(n_out=n_out - 8),
        "n_out not a multiple of 8": dict(n_out=n_out + 4),
        "duplicate slots": dict(slots=(2, 2)),
        "slot out of range": dict(slots=(1, 4)),
        "negative slot": dict(slots=(-1, 2)),
        # outputs [0, 100) need input up to j(99), far past a 10-sample chunk
        "reads past the chunk": dict(rows=(
            p0._replace(m=10, e1=100, keep_pos=0, keep_len=10), p1)),
        # a second push that names no carry reads below its chunk
        "reads before the carry": dict(rows=(
            p0._replace(a0=2000, e0=p0.e1, e1=p0.e1 + 50, keep_pos=3990,
                        keep_len=10, carry_pos=2000, carry_len=0), p1)),
        "new carry outside": dict(rows=(
            p0._replace(keep_pos=p0.keep_pos - 1), p1)),
        "one par row short": None,
    }
    for name, kw in bad.items():
        with pytest.raises(RuntimeError, match="resample_poly_stream_rows"):
            if kw is None:
                ext.resample_poly_stream_rows(x, par((p0,), (1,)), st.carry,
                                              bank, d.L, d.M, d.H, n_out)
            else:
                call(**kw)
            pytest.fail(f"{name}: not refused")
        torch.cuda.synchronize()
        assert np.array_equal(_ibits(st.carry), before), name


# --------------------------------------------------------------------------- #
# end to end on an x_low voice
# --------------------------------------------------------------------------- #
SENTENCES = ["hˈɛloʊ wˈɝld, ðɪs ɪz ɐ lˈɔŋɡɚ sˈɛntəns tə stɹˈiːm.",
             "ɡˈʊd mˈɔːnɪŋ tʊ jˈuː.", "hˈɛloʊ."]


@pytest.mark.parametrize("engine", ["auto", "python"])
def test_voice_streams_at_8k(xlow_voice_path, engine):
    from sonata_amd.audio.samples import to_i16
    from sonata_amd.models import load_voice

    v = load_voice(xlow_voice_path, device=DEV, engine=engine)
    assert (v._engine is not None) == (engine == "auto")
    sr = v.audio_output_info().sample_rate
    n = len(SENTENCES)

    def run(**kw):
        got = [[] for _ in range(n)]
        for i, chunk in v.stream_synthesis_batch(SENTENCES, 8, 1, **kw):
            got[i].append(chunk)
        return got

    plain = run()
    got = run(sample_rate=8000)
    pcm = run(sample_rate=8000, pcm=True)
    mixed = run(sample_rate=[None, 8000, 48000],
                prosody=[None, (1.3, 0.8, 1.05), None])
    plain_p = run(prosody=[None, (1.3, 0.8, 1.05), None])
    assert max(len(p) for p in plain) >= 3  # several rounds, rows drop out

    def one_shot(x, rate):
        xd = torch.from_numpy(x).reshape(1, -1).to(DEV)
        y, yl = ops.resample_rows(xd, [len(x)], sr, rate)
        return y[0, : int(yl[0])].cpu().numpy()

    for b in range(n):
        tag = f"sentence {b}"
        x = np.concatenate(plain[b])
        assert len(got[b]) == len(plain[b]), tag  # one chunk per round
        y = np.concatenate(got[b])
        assert y.dtype == np.float32
        assert y.tobytes() == one_shot(x, 8000).tobytes(), tag
        assert [len(c) for c in pcm[b]] == [len(c) for c in got[b]], tag
        for a, f in zip(pcm[b], got[b]):
            assert a.dtype == np.int16
            assert np.array_equal(a, to_i16(f)), tag
        rate = [None, 8000, 48000][b]
        xp = np.concatenate(plain_p[b])
        want = xp if rate is None else one_shot(xp, rate)
        assert np.concatenate(mixed[b]).tobytes() == want.tobytes(), tag
    assert len(v._tail_free) == v._tails.shape[0]

    # slots are reused: a stream closed midway leaves nothing a later one reads
    first = v.stream_open(SENTENCES[:2], 8, 1, sample_rate=[48000, 8000])
    v.stream_round(first)
    v.stream_round(first)
    v.stream_close(first)
    redo = run(sample_rate=8000)
    for b in range(n):
        assert np.concatenate(redo[b]).tobytes() == \
            np.concatenate(got[b]).tobytes()


def test_stream_batcher_mixed_rates_leaves_no_thread(xlow_voice_path):
    from sonata_amd.models import load_voice
    from sonata_amd.synth.batcher import StreamBatcher

    v = load_voice(xlow_voice_path, device=DEV)
    sr = v.audio_output_info().sample_rate
    rates = [8000, None, 48000]
    threads_before = set(threading.enumerate())
    sb = StreamBatcher(v, max_streams=8, max_wait_ms=20.0)
    results, errors = {}, []

    def consumer(k):
        try:
            results[k] = list(sb.open(SENTENCES[k], 8, 1,
                                      sample_rate=rates[k]))
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    try:
        threads = [threading.Thread(target=consumer, args=(k,))
                   for k in range(3)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(120)
        assert not errors, errors
    finally:
        sb.close()
    assert not sb._worker.is_alive()
    assert set(threading.enumerate()) <= threads_before
    for k, rate in enumerate(rates):
        assert all(len(c) for c in results[k])  # empty chunks stay inside
        y = np.concatenate(results[k])
        # lengths are exact whatever the stream shared its rounds with
        x = np.concatenate([c for _, c in v.stream_synthesis_batch(
            [SENTENCES[k]], 8, 1)])
        assert len(y) == R.out_len(len(x), sr, rate), f"stream {k}"
        assert np.isfinite(y).all()
    assert len(v._tail_free) == v._tails.shape[0]
