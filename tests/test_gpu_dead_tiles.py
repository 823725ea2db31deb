"""Dead-tile early exit and the sliced weight layout of the channel-last
decoder kernels (csrc/resblock_cl.hip, csrc/conv1d_cl.hip).

A block whose whole output tile lies at or past out_lens[b] stores zeros and
returns without reading anything.  The shapes put the ragged boundary where
that path can go wrong: T = 3*BM + 7 gives three full tiles and a short
fourth, and the four rows of the batch have

    out_lens = [T, 2*BM, 2*BM + 1, 0]

    T         nothing dead
    2*BM      the boundary exactly on a tile seam: tiles 2 and 3 dead
    2*BM + 1  one live row in tile 2, tile 3 (the short one) dead
    0         every tile dead

BM is the output tile of the geometry the host dispatcher picks.  All calls
go through sonata_amd.ops.functional; every tolerance is the derived bound of
tests/kernel_oracle.py, and rows at t >= out_lens[b] must be +0 bit for bit.
"""

import pytest
import torch

import kernel_oracle as ko

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN_GAP = 64  # inputs are NaN from out_lens[b] + 64 on; the largest halo is 31


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gen(*key):
    seed = 29
    for k in key:
        seed = (seed * 1000003 + int(k * 1000)) % (2 ** 31 - 1)
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _to(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def _four_lens(T, seam):
    return torch.tensor([T, seam, seam + 1, 0])


def _nan_past(t, lens, gap=NAN_GAP):
    """Copy of t [B, T, C] with NaN in every row >= lens[b] + gap."""
    idx = torch.arange(t.shape[1]).unsqueeze(0)
    far = (idx >= (lens.unsqueeze(1) + gap)).unsqueeze(-1)
    return t.masked_fill(far, float("nan"))


_assert_plus_zero = ko.assert_plus_zero


def _pair_bm(C, k):
    """Output tile of resblock_pair_cl_fused's default geometry."""
    xtr = 256 if C <= 32 else (64 if C >= 256 else 128)
    return xtr - (k - 1)


# --------------------------------------------------------------------------- #
# resblock pair
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("with_accum", [False, True])
@pytest.mark.parametrize("k,dil", [(3, 1), (11, 5)])
@pytest.mark.parametrize("C", [32, 64, 128, 256])
def test_pair_dead_tiles(dev, C, k, dil, with_accum):
    from sonata_amd.ops.functional import resblock_pair_cl

    BM = _pair_bm(C, k)
    B, T = 4, 3 * BM + 7
    lens = _four_lens(T, 2 * BM)
    g = _gen(C, k, dil, with_accum)
    x = ko.rounding_free((B, T, C), g)
    w1 = ko.rounding_free((C, C, k), g, (C * k) ** -0.5)
    w2 = ko.rounding_free((C, C, k), g, (C * k) ** -0.5)
    b1, b2 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    acc = ko.rounding_free((B, T, C), g) if with_accum else None
    scale = 1.0 / 3.0
    # The oracle sees the clean inputs.  No live element depends on a row at
    # or past out_lens + 64 (halo <= 31), so the kernel, which gets NaN
    # there, has to produce the same numbers without touching those rows.
    oracle = ko.resblock_pair_oracle(x, w1, b1, w2, b2, dil, lens, acc, scale)
    xn = _nan_past(x, lens)
    an = _nan_past(acc, lens) if with_accum else None
    xd, w1d, b1d, w2d, b2d, ld, ad = _to(dev, xn, w1, b1, w2, b2, lens, an)
    got = resblock_pair_cl(xd, w1d, b1d, w2d, b2d, dil, out_lens=ld,
                           accum=ad, out_scale=scale)
    what = f"pair C={C} k={k} d={dil} accum={with_accum}"
    assert torch.isfinite(got.float()).all(), f"{what}: output not finite"
    ko.assert_within(got, oracle, tile=BM, what=what)
    _assert_plus_zero(got, lens, what)


# --------------------------------------------------------------------------- #
# leaky_conv1d_cl: BM = 256, Cout 130 = one full 128-column tile + a 2-column
# one (a dead tile there is zeroed row by row, not as one span)
# --------------------------------------------------------------------------- #
def test_conv1d_cl_dead_tiles(dev):
    from sonata_amd.ops.functional import leaky_conv1d_cl

    Cin, Cout, k, dil = 64, 130, 7, 3
    B, T = 4, 3 * 256 + 7
    pad = (k - 1) * dil // 2
    lens = _four_lens(T, 2 * 256)
    g = _gen(Cin, Cout, k, dil)
    x = ko.rounding_free((B, T, Cin), g)
    w = ko.rounding_free((Cout, Cin, k), g, (Cin * k) ** -0.5)
    bias = torch.randn(Cout, generator=g)
    res = ko.rounding_free((B, T, Cout), g)
    oracle = ko.conv_cl_oracle(x, w, bias, pad, dil, 0.1, "tanh", 0.0, res,
                               lens)
    xd, wd, bd, rd, ld = _to(dev, x, w, bias, res, lens)
    got = leaky_conv1d_cl(xd, wd, bd, padding=pad, dilation=dil,
                          pre_lrelu=0.1, post_tanh=True, residual=rd,
                          out_lens=ld)
    ko.assert_within(got, oracle, tile=256, what="conv1d_cl dead tiles")
    _assert_plus_zero(got, lens, "conv1d_cl dead tiles")


# --------------------------------------------------------------------------- #
# leaky_convtranspose1d_cl: a block covers 128 input rows = out rows
# [128*s*i - pad, 128*s*(i+1) - pad), so the seam is at 2*128*s - pad; the
# fifth batch row puts the boundary at 2*128*s as well
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("Cin,Cout,stride", [(128, 64, 8), (64, 96, 2)])
def test_convt1d_cl_dead_tiles(dev, Cin, Cout, stride):
    from sonata_amd.ops.functional import leaky_convtranspose1d_cl

    k, pad = 2 * stride, stride // 2
    Tin = 3 * 128 + 7
    Tout = (Tin - 1) * stride - 2 * pad + k
    seam = 2 * 128 * stride - pad
    lens = torch.cat([_four_lens(Tout, seam),
                      torch.tensor([2 * 128 * stride])])
    B = lens.numel()
    g = _gen(Cin, Cout, stride)
    x = ko.rounding_free((B, Tin, Cin), g)
    w = ko.rounding_free((Cin, Cout, k), g, (Cin * 2) ** -0.5)
    bias = torch.randn(Cout, generator=g)
    oracle = ko.convt_cl_oracle(x, w, bias, stride, pad, 0.1, lens)
    xd, wd, bd, ld = _to(dev, x, w, bias, lens)
    got = leaky_convtranspose1d_cl(xd, wd, bd, stride, pad, pre_lrelu=0.1,
                                   out_lens=ld)
    what = f"convt1d_cl s={stride} dead tiles"
    ko.assert_within(got, oracle, tile=128 * stride, what=what)
    _assert_plus_zero(got, lens, what)


# --------------------------------------------------------------------------- #
# both weight layouts of the pair kernel: the same arithmetic in the same
# order, so the outputs are equal bit for bit
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("k,dil", [(3, 1), (7, 3), (11, 5)])
@pytest.mark.parametrize("C", [64, 128, 256])
def test_pair_layouts_bitwise_equal(dev, monkeypatch, C, k, dil):
    from sonata_amd.ops import hip_ext
    from sonata_amd.ops.functional import resblock_pair_cl

    B, T = 4, 300
    lens = torch.tensor([300, 171, 64, 0])
    g = _gen(C, k, dil, 7)
    x = ko.rounding_free((B, T, C), g)
    w1 = ko.rounding_free((C, C, k), g, (C * k) ** -0.5)
    w2 = ko.rounding_free((C, C, k), g, (C * k) ** -0.5)
    b1, b2 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    acc = ko.rounding_free((B, T, C), g)
    xd, w1d, b1d, w2d, b2d, ld, ad = _to(dev, x, w1, b1, w2, b2, lens, acc)
    ext = hip_ext(required=True)
    out = {}
    for layout in ("rows", "sliced"):
        monkeypatch.setenv("SONATA_RB_WLAYOUT", layout)
        assert ext.resblock_wlayout_sliced(C) == (layout == "sliced")
        out[layout] = resblock_pair_cl(xd, w1d, b1d, w2d, b2d, dil,
                                       out_lens=ld, accum=ad, out_scale=0.5)
    assert getattr(w1d, "_sonata_perm_sliced").shape == (k, C // 32, C, 32)
    assert torch.equal(out["rows"].view(torch.int16),
                       out["sliced"].view(torch.int16))
    oracle = ko.resblock_pair_oracle(x, w1, b1, w2, b2, dil, lens, acc, 0.5)
    ko.assert_within(out["sliced"], oracle, tile=_pair_bm(C, k),
                     what=f"pair sliced C={C} k={k} d={dil}")
