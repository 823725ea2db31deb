"""Per-row synthesis scales on the GPU: the three kernels of
csrc/elementwise.hip bit for bit against their scalar counterparts run on
one row at a time, the engine's and the Python graph's per-row entries
against the scalar ones, and the voice's batch and stream routes against
single calls with the config set voice-wide."""

import numpy as np
import pytest
import torch

from sonata_amd import ops
from sonata_amd.models import SynthesisConfig, create_random_voice, load_voice

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float32]


def _mask(lens, T, dtype):
    t = torch.arange(T, device=DEV)
    return (t[None, :] < torch.tensor(lens, device=DEV)[:, None]) \
        .to(dtype).unsqueeze(1)


def _bits(a, b):
    """Bit equality (signed zeros and NaN payloads included)."""
    assert a.dtype == b.dtype and a.shape == b.shape
    view = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


# --------------------------------- kernels ---------------------------------- #
@pytest.mark.parametrize("halves", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_prior_sample_rows_bitwise(dtype, halves):
    ext = ops.hip_ext(required=True)
    B, C, T = 3, 24, 77
    lens, scales = [77, 40, 0], [0.667, 0.0, 1.3]
    torch.manual_seed(5)
    stats = torch.randn(B, 2 * C, T, device=DEV).to(dtype)
    m, logs = stats[:, :C], stats[:, C:]
    if not halves:
        m, logs = m.contiguous(), logs.contiguous()
    else:
        assert m.stride(0) == 2 * C * T and not m.is_contiguous()
    mask = _mask(lens, T, dtype)
    noise = torch.randn(B, C, T, device=DEV).to(dtype) * mask
    ns = torch.tensor(scales, dtype=torch.float32, device=DEV)
    got = ops.prior_sample_rows(m, logs, mask, noise, ns)
    assert got.shape == (B, C, T) and got.is_contiguous()
    for b in range(B):
        want = ext.prior_sample(m[b:b + 1].contiguous(),
                                logs[b:b + 1].contiguous(),
                                mask[b:b + 1].contiguous(),
                                noise[b:b + 1].contiguous(), scales[b])
        assert _bits(got[b:b + 1], want), f"row {b}"
        assert not got[b, :, lens[b]:].any()  # padded tail: exactly zero


def test_row_kernels_refuse_bad_scales():
    ext = ops.hip_ext(required=True)
    x = torch.zeros(2, 2, 8, device=DEV)
    mask = torch.ones(2, 1, 8, device=DEV)
    ok = torch.ones(2, device=DEV)
    for bad in (torch.ones(3, device=DEV), torch.ones(2),
                ok.to(torch.bfloat16)):
        with pytest.raises(RuntimeError, match="f32"):
            ext.scale_mask_rows(x, mask, bad)
        with pytest.raises(RuntimeError, match="f32"):
            ext.prior_sample_rows(x, x, mask, x, bad)
        with pytest.raises(RuntimeError, match="f32"):
            ext.duration_rows(x[:, :1], mask, bad)
    with pytest.raises(RuntimeError, match="x_mask"):
        ext.duration_rows(x[:, :1], mask[:, :, :4].contiguous(), ok)


@pytest.mark.parametrize("T", [37, 130])
@pytest.mark.parametrize("dtype", DTYPES)
def test_duration_rows_bitwise(dtype, T):
    B = 4
    lens, scales = [T, 20, 1, 0], [1.0, 0.5, 2.0, 1.37]
    torch.manual_seed(T)
    # the narrow of a 2-channel flow state, as the graph hands it over
    state = (torch.rand(B, 2, T, device=DEV) * 5.0 - 2.0).to(dtype)
    logw = state[:, :1]
    mask = _mask(lens, T, dtype)
    ls = torch.tensor(scales, dtype=torch.float32, device=DEV)
    durs, y_lengths = ops.duration_rows(logw, mask, ls)
    assert durs.dtype == torch.int32 and durs.shape == (B, T)
    assert y_lengths.dtype == torch.int64 and y_lengths.shape == (B,)
    sums = []
    for b in range(B):
        w = torch.exp(logw[b:b + 1]) * mask[b:b + 1] * scales[b]
        w_ceil = torch.ceil(w)
        want_len = torch.clamp_min(torch.sum(w_ceil, [1, 2]), 1).long()
        want_durs = w_ceil.squeeze(1).to(torch.int32)
        assert torch.equal(durs[b:b + 1], want_durs), f"row {b}"
        assert torch.equal(y_lengths[b:b + 1], want_len), f"row {b}"
        sums.append(int(w_ceil.double().sum()))
    assert int(y_lengths[3]) == 1  # the empty row
    if T == 130:
        assert sums[0] > 256  # past bf16's integer range: the sum rounds
    # contiguous logw takes the same kernel
    d2, y2 = ops.duration_rows(logw.contiguous(), mask, ls)
    assert torch.equal(d2, durs) and torch.equal(y2, y_lengths)


@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_mask_rows_bitwise(dtype):
    B, T = 3, 77
    lens, scales = [77, 40, 0], [0.8, 0.0, 0.333]
    torch.manual_seed(9)
    noise = torch.randn(B, 2, T, device=DEV).to(dtype)
    mask = _mask(lens, T, dtype)
    s = torch.tensor(scales, dtype=torch.float32, device=DEV)
    got = ops.scale_mask_rows(noise, mask, s)
    for b in range(B):
        want = noise[b:b + 1] * scales[b] * mask[b:b + 1]
        assert _bits(got[b:b + 1], want), f"row {b}"
    if dtype == torch.bfloat16:
        # the trap: scales held in bf16 give other bits (0.8 -> 0.80078)
        wrong = noise * s.to(dtype).view(-1, 1, 1) * mask
        assert not _bits(got, wrong)


# ------------------------------ engine, graph ------------------------------- #
SENTS = ["tˈuː θɹˈiː.", "fˈaɪv sˈɪks ˈeɪt nˈaɪn.",
         "ðɪs ɪz ə lˈɔŋɡɚ sˈɛntəns wɪθ mˈɔɹ wˈɝdz."]


@pytest.fixture(scope="module")
def pack(tmp_path_factory):
    return create_random_voice(str(tmp_path_factory.mktemp("rows_gpu")),
                               "rows_gpu", quality="x_low", num_speakers=3)


@pytest.fixture(scope="module")
def voice(pack):
    v = load_voice(pack, device=DEV)
    assert v._engine is not None
    return v


@pytest.fixture(scope="module")
def voice_py(pack):
    return load_voice(pack, device=DEV, engine="python")


def _ids(voice):
    id_lists = [voice._encode_ids(p) for p in SENTS]
    T = max(len(i) for i in id_lists)
    ids = torch.zeros((len(SENTS), T), dtype=torch.long)
    for b, il in enumerate(id_lists):
        ids[b, :len(il)] = torch.tensor(il)
    lengths = torch.tensor([len(i) for i in id_lists])
    return ids.to(DEV), lengths.to(DEV)


def test_engine_rows_uniform_is_the_scalar_path_bitwise(voice):
    ids, lengths = _ids(voice)
    sid = torch.tensor([0, 2, 1], device=DEV)
    seeds = [101, 202, 303]
    ns, ls, nw = 0.667, 1.3, 0.8
    z, y_mask, g = voice._engine.infer_encoder(ids, lengths, sid, ns, ls, nw,
                                               seeds)
    zr, mr, gr = voice._engine.infer_encoder_rows(
        ids, lengths, sid, [ns] * 3, [ls] * 3, [nw] * 3, seeds)
    assert zr.shape == z.shape and z.dtype == torch.bfloat16
    assert _bits(zr, z) and _bits(mr, y_mask) and _bits(gr, g)
    # and the whole graph
    a, al = voice._engine.infer(ids, lengths, sid, ns, ls, nw, seeds)
    ar, alr = voice._engine.infer_rows(ids, lengths, sid, [ns] * 3, [ls] * 3,
                                       [nw] * 3, seeds)
    assert torch.equal(al, alr) and _bits(ar, a)
    with pytest.raises(RuntimeError, match="per-row"):
        voice._engine.infer_encoder_rows(ids, lengths, sid, [ns] * 2,
                                         [ls] * 3, [nw] * 3, seeds)


def test_python_graph_rows_uniform_is_the_scalar_path_bitwise(voice_py):
    v = voice_py
    ids, lengths = _ids(v)
    sid = torch.tensor([0, 2, 1], device=DEV)
    ns, ls, nw = 0.667, 1.3, 0.8

    def run(scales):
        gens = v._generators(SENTS, 0)
        with torch.no_grad():
            return v.net.infer_encoder(ids, lengths, sid=sid,
                                       noise_scale=scales[0],
                                       length_scale=scales[1],
                                       noise_w=scales[2], generators=gens)

    z, y_mask, g = run((ns, ls, nw))
    f32 = dict(dtype=torch.float32, device=DEV)
    zr, mr, gr = run(tuple(torch.full((3,), s, **f32) for s in (ns, ls, nw)))
    assert zr.shape == z.shape
    assert _bits(zr.contiguous(), z.contiguous())
    assert _bits(mr, y_mask) and _bits(gr, g)


# --------------------------------- the voice -------------------------------- #
def _alone(voice, sentence, cfg):
    base = voice.get_synthesis_config()
    if cfg is not None:
        voice.set_synthesis_config(cfg)
    try:
        return voice.speak_one_sentence(sentence).samples
    finally:
        voice.set_synthesis_config(base)


ROWS = [SynthesisConfig(0, 0.667, 1.0, 0.8),
        SynthesisConfig(2, 0.667, 1.3, 0.8), None]


@pytest.mark.parametrize("which", ["cpp", "python"])
def test_mixed_batch_matches_single_calls(which, voice, voice_py):
    """Batch against single on this path: equal lengths and max|diff| < 2e-2,
    as tests/test_gpu_ops.py::test_ragged_batch_matches_single."""
    v = voice if which == "cpp" else voice_py
    base = v.get_synthesis_config()
    default = SynthesisConfig(1, base.noise_scale, base.length_scale,
                              base.noise_w)
    v.set_synthesis_config(default)  # the voice's speaker: neither 0 nor 2
    try:
        batch = v.speak_batch(SENTS, synthesis=ROWS)
        assert v.get_synthesis_config() == default
        singles = [_alone(v, s, r) for s, r in zip(SENTS, ROWS)]
        plain = [_alone(v, s, None) for s in SENTS[:2]]
        pcm = v.speak_batch_pcm(SENTS, synthesis=ROWS)
    finally:
        v.set_synthesis_config(base)
    for k, (one, b) in enumerate(zip(singles, batch)):
        d = (float(np.abs(one - b.samples).max())
             if len(one) == len(b.samples) else None)
        print(f"{which} row {k}: single {len(one)} batch {len(b.samples)} "
              f"max|diff| {d}")
        assert len(one) == len(b.samples)
        assert d < 2e-2
    for k in (0, 1):  # other speakers than the voice's own
        assert (len(plain[k]) != len(batch[k].samples)
                or float(np.abs(plain[k] - batch[k].samples).max()) > 2e-2)
    for a, p in zip(batch, pcm):
        assert p.as_wave_bytes() == a.as_wave_bytes()


def test_stream_open_rows(voice):
    """One stream_open with a config per stream, advanced by stream_round.
    Against stream_synthesis of each stream alone: the chunk lengths, and
    max|a - b| / max|b| < 0.05 (tests/test_gpu_stream_batch.py); against the
    batch rows: the same timeline, and with one window per stream the same
    bound on the samples."""
    v = voice
    rows = [ROWS[0], ROWS[1], SynthesisConfig(1, 0.5, 0.9, 0.6)]
    batch = v.speak_batch(SENTS, synthesis=rows)
    for chunk_size in (45, 4096):
        states = v.stream_open(SENTS, chunk_size, 3, synthesis=rows)
        got = [[] for _ in SENTS]
        while any(not s.done for s in states):
            for s, chunk in v.stream_round(states):
                got[s.index].append(chunk)
        for k, (s, r, g, b) in enumerate(zip(SENTS, rows, got, batch)):
            a = np.concatenate(g)
            assert len(a) == len(b.samples)
            if chunk_size == 45:
                want = list(v.stream_synthesis(s, 45, 3, synthesis=r))
                assert [len(c) for c in g] == [len(c) for c in want]
                ref = np.concatenate(want)
            else:
                assert len(g) == 1
                ref = b.samples
            ratio = float(np.abs(a - ref).max() / np.abs(ref).max())
            print(f"chunk_size {chunk_size} stream {k}: {len(g)} chunks, "
                  f"max|d|/max|ref| {ratio:.3e}")
            assert ratio < 0.05
    assert max(len(list(v.stream_synthesis(s, 45, 3))) for s in SENTS) >= 2


def test_out_of_range_speaker_never_reaches_the_device(voice):
    bad = SynthesisConfig(3, 0.667, 1.0, 0.8)
    with pytest.raises(ValueError, match="speaker_id 3"):
        voice.speak_batch(SENTS, synthesis=[None, bad, None])
    with pytest.raises(ValueError, match="speaker_id 3"):
        voice.stream_open(SENTS, synthesis=[None, bad, None])
    torch.cuda.synchronize()
