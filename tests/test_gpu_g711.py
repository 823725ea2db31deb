"""csrc/pcm.hip g711_rows on the GPU against
g711.encode(to_i16(...)), bit for bit: the kernel alone, every int16 value
through the device compander, VitsVoice.speak_batch_pcm(encoding=...) on
both engines and one batched stream.  No tolerance anywhere."""

import numpy as np
import pytest
import torch

from sonata_amd import ops
from sonata_amd.audio import g711
from sonata_amd.audio.samples import to_i16
from sonata_amd.ops.functional import PCM_TILE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTENCES = ["wˈʌn.", "wˈʌn tˈuː θɹˈiː fˈoːɹ.", "hˈɛloʊ ðˈɛr ˈɛvɹiwˌʌn."]
LAW_ID = {"ulaw": 0, "alaw": 1}


def _amps(rng, n):
    """Per-sample amplitudes log-uniform over 1e-6 .. 10."""
    return (10.0 ** rng.uniform(-6.0, 1.0, n)).astype(np.float32)


def _noise(rng, n):
    return (_amps(rng, n) * rng.standard_normal(n)).astype(np.float32)


def _codes(x, lens, sil=None, **kw):
    """ops.g711_rows on the device for a host [B, N] array or a tensor."""
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    codes, out = ops.g711_rows(x.to(DEV), lens, sil, **kw)
    assert codes.dtype == torch.uint8 and codes.is_cuda
    assert codes.shape[1] % 16 == 0
    return codes.cpu().numpy(), out.tolist()


def _check_row(got_row, x_row, n, law, peak_normalize=True, msg=""):
    np.testing.assert_array_equal(
        got_row[:n], g711.encode(to_i16(x_row[:n], peak_normalize), law),
        err_msg=msg)
    assert (got_row[n:] == g711.ZERO[law]).all(), msg


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("peak_normalize", [True, False])
@pytest.mark.parametrize("law", g711.LAWS)
def test_single_row_small(law, peak_normalize, dtype):
    for n in (0, 1, 2, 15, 16, 17, 31, 33, 255, 256, 257):
        rng = np.random.default_rng(n)
        x = torch.from_numpy(_noise(rng, n).reshape(1, n)).to(dtype)
        ref = x.float().numpy()  # widening bf16 is exact
        got, out = _codes(x, [n], law=law, peak_normalize=peak_normalize)
        assert out == [n] and got.shape == (1, (n + 15) // 16 * 16)
        _check_row(got[0], ref[0], n, law, peak_normalize, msg=f"n {n}")
        if n >= 255:  # both signs, and clamping without normalisation
            want = to_i16(ref[0], peak_normalize)
            assert (want > 0).any() and (want < 0).any()
            assert peak_normalize or (abs(want.astype(int)) >= 32767).any()


def test_every_int16_value_through_the_device_compander():
    v = np.arange(-32767, 32768)
    x = v.astype(np.float32).reshape(1, -1)
    # the peak is 32767, the scale exactly 1: to_i16 is the identity
    np.testing.assert_array_equal(to_i16(x[0]), v.astype(np.int16))
    for law, distinct in (("ulaw", 255), ("alaw", 256)):
        want = g711.encode(v.astype(np.int16), law)
        assert len(np.unique(want)) == distinct  # no segment is missed
        got, _ = _codes(x, [x.shape[1]], law=law)
        np.testing.assert_array_equal(got[0, : x.shape[1]], want, err_msg=law)
        # -32768 and 32767 by clamping at the fixed scale
        ends = np.array([[-2.0, 2.0]], dtype=np.float32)
        assert to_i16(ends[0], False).tolist() == [-32768, 32767]
        got, _ = _codes(ends, [2], law=law, peak_normalize=False)
        np.testing.assert_array_equal(
            got[0, :2], g711.encode([-32768, 32767], law))


def _ragged():
    lens = [4097, 1, 1000, 0, 3]
    rng = np.random.default_rng(3)
    x = np.full((len(lens), 4097), 1e3, dtype=np.float32)  # garbage past len
    for b, n in enumerate(lens):
        x[b, :n] = _noise(rng, n)
    return x, lens


def test_ragged_batch_pads_with_the_rows_zero_code():
    x, lens = _ragged()
    sil = [0, 5, 0, 7, 1]
    laws = ["ulaw", "alaw", "ulaw", "alaw", "ulaw"]
    for pn in (True, False):
        got, out = _codes(x, lens, sil, law=laws, peak_normalize=pn)
        assert out == [n + s for n, s in zip(lens, sil)]
        assert got.shape == (5, 4112)
        for b, n in enumerate(lens):
            _check_row(got[b], x[b], n, laws[b], pn, msg=f"row {b}")
    # the other way round: every row under both laws
    flip = [{"ulaw": "alaw", "alaw": "ulaw"}[w] for w in laws]
    got, _ = _codes(x, lens, sil, law=flip)
    for b, n in enumerate(lens):
        _check_row(got[b], x[b], n, flip[b], msg=f"flipped row {b}")


def test_binding_odd_strides_on_both_sides():
    x, lens = _ragged()
    ext = ops.hip_ext(required=True)
    laws = ["alaw", "ulaw", "alaw", "ulaw", "alaw"]
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    wd = torch.tensor([LAW_ID[w] for w in laws], dtype=torch.int32,
                      device=DEV)
    # rows 4099 floats apart and starting one float in: the row starts fall
    # on every 4-byte offset from a 16-byte boundary; n_out odd: the output
    # rows start at every odd and even byte offset as well
    wide = torch.full((len(lens), 4099), 7e2, dtype=torch.float32, device=DEV)
    wide[:, 1:4098] = torch.from_numpy(x).to(DEV)
    view = wide[:, 1:4098]
    assert view.stride(0) == 4099 and view.data_ptr() % 16 == 4
    for n_out in (4097, 4113, 1001):
        y, peaks = ext.g711_rows(view, ld, wd, n_out, True)
        assert y.dtype == torch.uint8 and y.shape == (len(lens), n_out)
        y, peaks = y.cpu().numpy(), peaks.cpu().numpy()
        for b, n in enumerate(lens):
            m = min(n, n_out)  # a row longer than n_out is cut, as in pcm16
            want = g711.encode(to_i16(x[b, :n]), laws[b])[:m]
            np.testing.assert_array_equal(y[b, :m], want,
                                          err_msg=f"n_out {n_out} row {b}")
            assert (y[b, m:] == g711.ZERO[laws[b]]).all()
            assert peaks[b] == (np.abs(x[b, :n]).max() if n else 0), b
    # argument checks, as strict as pcm16_rows's
    with pytest.raises(RuntimeError):
        ext.g711_rows(view, ld, wd.long(), 4097, True)
    with pytest.raises(RuntimeError):
        ext.g711_rows(view, ld, wd[:4], 4097, True)
    with pytest.raises(RuntimeError):
        ext.g711_rows(view, ld, wd.cpu(), 4097, True)
    with pytest.raises(RuntimeError):
        ext.g711_rows(view.double(), ld, wd, 4097, True)
    with pytest.raises(RuntimeError):
        ext.g711_rows(wide[:, ::2], ld, wd, 100, True)
    with pytest.raises(RuntimeError):
        ext.g711_rows(view, ld, wd, -1, True)
    # the wrapper refuses a law it does not know before anything is uploaded
    with pytest.raises(ValueError):
        ops.g711_rows(view, lens, law=["ulaw"] * 4 + ["pcm16"])


def test_bf16_channel_view_is_taken_as_it_is():
    rng = np.random.default_rng(5)
    B, T = 3, 2 * PCM_TILE + 77   # odd row stride in 2-byte elements
    lens = [T, 900, PCM_TILE + 1]
    laws = ["ulaw", "alaw", "alaw"]
    x = torch.from_numpy(
        np.clip(_noise(rng, B * T), -8, 8).reshape(B, 1, T)).to(DEV)
    xb = x.to(torch.bfloat16)
    view = xb[:, 0, :]
    assert view.data_ptr() == xb.data_ptr()
    ext = ops.hip_ext(required=True)
    y, _ = ext.g711_rows(
        view, torch.tensor(lens, dtype=torch.int32, device=DEV),
        torch.tensor([LAW_ID[w] for w in laws], dtype=torch.int32,
                     device=DEV), T, True)
    ref = xb.float().cpu().numpy()[:, 0, :]
    y = y.cpu().numpy()
    for b, n in enumerate(lens):
        _check_row(y[b], ref[b], n, laws[b], msg=f"bf16 row {b}")
    got, _ = _codes(x[:, 0, :], lens, [0, 3, 0], law=laws)
    ref32 = x.cpu().numpy()[:, 0, :]
    for b, n in enumerate(lens):
        _check_row(got[b], ref32[b], n, laws[b], msg=f"f32 row {b}")


@pytest.mark.parametrize("where", ["first", "middle", "last", "very_last"])
def test_peak_in_each_tile(where):
    n = 3 * PCM_TILE + 5
    rng = np.random.default_rng(7)
    x = np.clip(_noise(rng, n), -8.0, 8.0)
    at = {"first": 11, "middle": PCM_TILE + 123, "last": 3 * PCM_TILE + 1,
          "very_last": n - 1}[where]
    x[at] = -32.0  # 32767/32 is exact in f32: the peak maps to -32767
    for law in g711.LAWS:
        got, _ = _codes(x.reshape(1, n), [n], law=law)
        _check_row(got[0], x, n, law, msg=where)
        assert got[0, at] == g711.encode([-32767], law)[0]


# ------------------------------ whole voice -------------------------------- #
@pytest.fixture(scope="module", params=["auto", "python"])
def gpu_voice(request, xlow_voice_path):
    from sonata_amd.models import load_voice

    v = load_voice(xlow_voice_path, device=DEV, engine=request.param)
    assert (v._engine is not None) == (request.param == "auto")
    return v


def test_speak_batch_pcm_encoding(gpu_voice, monkeypatch):
    monkeypatch.setenv("SONATA_DEVICE_PCM", "1")
    v = gpu_voice
    ref = {rate: v.speak_batch_pcm(SENTENCES, silence_ms=30, sample_rate=rate)
           for rate in (None, 8000)}
    assert len({len(r.pcm) for r in ref[None]}) > 1  # a ragged batch
    calls = []
    real16, real8 = ops.pcm16_rows, ops.g711_rows
    monkeypatch.setattr(ops, "pcm16_rows",
                        lambda *a, **k: calls.append(16) or real16(*a, **k))
    monkeypatch.setattr(ops, "g711_rows",
                        lambda *a, **k: calls.append(8) or real8(*a, **k))
    for law in g711.LAWS:
        got = v.speak_batch_pcm(SENTENCES, silence_ms=30, encoding=law)
        for g, r in zip(got, ref[None]):
            assert g.encoding == law and g.info.sample_width == 1
            np.testing.assert_array_equal(g.pcm, g711.encode(r.pcm, law))
            assert g.info.sample_rate == r.info.sample_rate
            assert g.inference_ms > 0
    assert calls == [8, 8]  # one launch per batch, and no int16 pass
    # a mixed batch: three encodings, two rates, silence
    del calls[:]
    encs, rates = ["alaw", "pcm16", "ulaw"], [8000, 8000, None]
    got = v.speak_batch_pcm(SENTENCES, silence_ms=30, sample_rate=rates,
                            encoding=encs)
    assert sorted(calls) == [8, 8, 16]  # per rate: one launch per kind
    for b, (g, e, rate) in enumerate(zip(got, encs, rates)):
        r = ref[rate][b]
        assert g.encoding == e and g.info.sample_rate == r.info.sample_rate
        np.testing.assert_array_equal(
            g.pcm, r.pcm if e == "pcm16" else g711.encode(r.pcm, e))
    # the host route gives the same bytes and runs neither op
    del calls[:]
    monkeypatch.setenv("SONATA_DEVICE_PCM", "0")
    host = v.speak_batch_pcm(SENTENCES, silence_ms=30, sample_rate=rates,
                             encoding=encs)
    assert not calls
    for g, h in zip(got, host):
        assert g.encoding == h.encoding and g.info == h.info
        np.testing.assert_array_equal(g.pcm, h.pcm)


def test_stream_chunks_are_the_codes_of_the_int16_chunks(xlow_voice_path):
    from sonata_amd.models import load_voice

    v = load_voice(xlow_voice_path, device=DEV)
    two = SENTENCES[1:]
    want = [[] for _ in two]
    for i, chunk in v.stream_synthesis_batch(two, 20, 2, pcm=True):
        want[i].append(chunk)
    assert sum(len(w) for w in want) > 2
    laws = ["alaw", "ulaw"]
    got = [[] for _ in two]
    for i, chunk in v.stream_synthesis_batch(two, 20, 2, encoding=laws):
        assert chunk.dtype == np.uint8
        got[i].append(chunk)
    for g, w, law in zip(got, want, laws):
        assert len(g) == len(w)
        for a, b in zip(g, w):
            np.testing.assert_array_equal(a, g711.encode(b, law))
