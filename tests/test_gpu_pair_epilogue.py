"""Epilogue 2 of the resblock pair kernel through LDS (csrc/resblock_cl.hip,
SONATA_RB_EPILOGUE=staged) against the element-wise one (=direct).

Both run the same f32 operations in the same order, so their outputs are
equal bit for bit; both are held to the per-element bound of
tests/kernel_oracle.py; rows at t >= out_lens[b] are +0 bit for bit; and with
x and accum NaN from out_lens[b] + 64 on the output stays finite (what
test_gpu_dead_tiles.py pins, here on the 16-byte store path).  Running staged
twice on one input screens the aliased LDS for a race.

Shapes: every pair geometry the host dispatches (and the SONATA_RB_GEOM
variants), B = 4, T = 3*BM + 7, out_lens = [T, 2*BM, 2*BM + 1, 0]; channel
counts that mask part of a 16-byte column group or are no multiple of 8 (the
fallback); T around one tile.  All calls go through sonata_amd.ops.functional.
"""

import pytest
import torch

import kernel_oracle as ko

pytestmark = pytest.mark.gpu

NAN_GAP = 64  # the largest halo is 31 rows


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gen(*key):
    seed = 31
    for k in key:
        seed = (seed * 1000003 + int(k * 1000)) % (2 ** 31 - 1)
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _to(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def _nan_past(t, lens, gap=NAN_GAP):
    idx = torch.arange(t.shape[1]).unsqueeze(0)
    far = (idx >= (lens.unsqueeze(1) + gap)).unsqueeze(-1)
    return t.masked_fill(far, float("nan"))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


_assert_plus_zero = ko.assert_plus_zero


def _xtr(C, geom):
    """xt tile rows of resblock_pair_cl_fused's dispatch (C pads to CP)."""
    if C <= 32:
        return 256
    if geom == "xtr64":
        return 64 if C >= 128 else 128
    if geom == "xtr128":
        return 128
    return 64 if C >= 256 else 128


def _run_both(monkeypatch, geom, fn):
    """fn() under direct, staged and staged again."""
    if geom:
        monkeypatch.setenv("SONATA_RB_GEOM", geom)
    else:
        monkeypatch.delenv("SONATA_RB_GEOM", raising=False)
    out = []
    for mode in ("direct", "staged", "staged"):
        monkeypatch.setenv("SONATA_RB_EPILOGUE", mode)
        out.append(fn())
    torch.cuda.synchronize()
    return out


def _check_pair(dev, monkeypatch, C, k, dil, geom, B, T, lens, with_accum,
                scale, nan):
    from sonata_amd.ops.functional import resblock_pair_cl

    BM = _xtr(C, geom) - (k - 1)
    g = _gen(C, k, dil, T, with_accum, scale)
    x = ko.rounding_free((B, T, C), g)
    w1 = ko.rounding_free((C, C, k), g, (C * k) ** -0.5)
    w2 = ko.rounding_free((C, C, k), g, (C * k) ** -0.5)
    b1, b2 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    acc = ko.rounding_free((B, T, C), g) if with_accum else None
    # the oracle sees the clean inputs; no live element depends on a row at
    # or past out_lens + 64, where the kernel gets NaN
    oracle = ko.resblock_pair_oracle(x, w1, b1, w2, b2, dil, lens, acc, scale)
    xn = _nan_past(x, lens) if nan else x
    an = _nan_past(acc, lens) if (nan and with_accum) else acc
    xd, w1d, b1d, w2d, b2d, ld, ad = _to(dev, xn, w1, b1, w2, b2, lens, an)
    direct, staged, again = _run_both(
        monkeypatch, geom,
        lambda: resblock_pair_cl(xd, w1d, b1d, w2d, b2d, dil, out_lens=ld,
                                 accum=ad, out_scale=scale))
    what = (f"pair C={C} k={k} d={dil} geom={geom} T={T} accum={with_accum} "
            f"scale={scale:.3f}")
    assert torch.isfinite(staged.float()).all(), f"{what}: staged not finite"
    assert torch.isfinite(direct.float()).all(), f"{what}: direct not finite"
    ne = _bits(staged) != _bits(direct)
    assert not ne.any(), (
        f"{what}: staged != direct at {int(ne.sum())} elements, first "
        f"{tuple(int(i) for i in ne.nonzero()[0])}")
    assert torch.equal(_bits(staged), _bits(again)), \
        f"{what}: two staged runs differ"
    ko.assert_within(staged, oracle, tile=BM, what=what + " staged")
    ko.assert_within(direct, oracle, tile=BM, what=what + " direct")
    if lens is not None:
        _assert_plus_zero(staged, lens, what)


GEOM_CASES = [(C, None) for C in (32, 64, 128, 256)] + \
    [(128, "xtr64"), (256, "xtr128")]


@pytest.mark.parametrize("with_accum,scale",
                         [(False, 1.0), (True, 1.0), (False, 1.0 / 3.0),
                          (True, 1.0 / 3.0)])
@pytest.mark.parametrize("k,dil", [(3, 1), (7, 3), (11, 5)])
@pytest.mark.parametrize("C,geom", GEOM_CASES)
def test_staged_equals_direct(dev, monkeypatch, C, geom, k, dil, with_accum,
                              scale):
    BM = _xtr(C, geom) - (k - 1)
    T = 3 * BM + 7
    lens = torch.tensor([T, 2 * BM, 2 * BM + 1, 0])
    _check_pair(dev, monkeypatch, C, k, dil, geom, 4, T, lens, with_accum,
                scale, nan=True)


# C = 16 / 24 pad to CP = 32: half / a quarter of the 16-byte column groups
# lie outside C.  C = 20 is no multiple of 8: element-wise under both settings.
@pytest.mark.parametrize("T_off", [None, -1, 0, 1])
@pytest.mark.parametrize("C", [16, 24, 20])
def test_edge_channels_and_one_tile(dev, monkeypatch, C, T_off):
    k, dil = 3, 1
    BM = 256 - (k - 1)
    T = 1 if T_off is None else BM + T_off
    _check_pair(dev, monkeypatch, C, k, dil, None, 1, T, None, True,
                1.0 / 3.0, nan=False)


@pytest.mark.parametrize("C,k,dil", [(64, 7, 3), (128, 3, 1), (256, 11, 5)])
@pytest.mark.parametrize("T_off", [None, -1, 0, 1])
def test_one_tile_wide_channels(dev, monkeypatch, C, k, dil, T_off):
    BM = _xtr(C, None) - (k - 1)
    T = 1 if T_off is None else BM + T_off
    _check_pair(dev, monkeypatch, C, k, dil, None, 1, T, None, False, 1.0,
                nan=False)


# leaky_conv1d_cl: two shapes of the existing matrix (a 2-column last tile at
# Cout 130, full tiles at 256), residual + tanh, ragged.  The conv kernel has
# one store path so far (bias in registers, residuals batched); the knob must
# not move its bits either way.
@pytest.mark.parametrize("Cout", [130, 256])
def test_conv1d_cl_epilogue(dev, monkeypatch, Cout):
    from sonata_amd.ops.functional import leaky_conv1d_cl

    Cin, k, dil = 64, 7, 3
    B, T = 4, 3 * 256 + 7
    pad = (k - 1) * dil // 2
    lens = torch.tensor([T, 2 * 256, 2 * 256 + 1, 0])
    g = _gen(Cin, Cout, k, dil)
    x = ko.rounding_free((B, T, Cin), g)
    w = ko.rounding_free((Cout, Cin, k), g, (Cin * k) ** -0.5)
    bias = torch.randn(Cout, generator=g)
    res = ko.rounding_free((B, T, Cout), g)
    oracle = ko.conv_cl_oracle(x, w, bias, pad, dil, 0.1, "tanh", 0.0, res,
                               lens)
    xd, wd, bd, rd, ld = _to(dev, _nan_past(x, lens), w, bias,
                             _nan_past(res, lens), lens)
    direct, staged, again = _run_both(
        monkeypatch, None,
        lambda: leaky_conv1d_cl(xd, wd, bd, padding=pad, dilation=dil,
                                pre_lrelu=0.1, post_tanh=True, residual=rd,
                                out_lens=ld))
    what = f"conv1d_cl Cout={Cout}"
    assert torch.isfinite(staged.float()).all(), f"{what}: not finite"
    assert torch.equal(_bits(staged), _bits(direct)), f"{what}: staged != direct"
    assert torch.equal(_bits(staged), _bits(again)), f"{what}: runs differ"
    ko.assert_within(staged, oracle, tile=256, what=what)
    _assert_plus_zero(staged, lens, what)
