"""Every dispatched variant of the channel-last serving kernels against the
fp64 oracle of tests/kernel_oracle.py, element by element.

The shapes are chosen from the host dispatchers: more than one time tile
(interior fast path + both seams), partial channel tiles in every BN class,
Cin that is no multiple of the 32-deep K slice, every XR bucket of every
channel class of the fused resblock pair, both layer-norm kernels.  All
calls go through sonata_amd.ops.functional so the weight-layout caches are
exercised too.  Every tolerance is the oracle's derived bound.
"""

import os

import pytest
import torch

import kernel_oracle as ko

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gen(*key):
    """CPU generator seeded by the case's parameters."""
    seed = 17
    for k in key:
        seed = (seed * 1000003 + int(k * 1000)) % (2 ** 31 - 1)
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _to(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def _ragged(Tout, seam):
    """0, == T, > T, and 3 rows past a tile seam (or 3 short of the end when
    the output has no seam)."""
    return torch.tensor([0, Tout, Tout + 5,
                         seam + 3 if Tout > seam + 3 else max(Tout - 3, 0)])


# --------------------------------------------------------------------------- #
# leaky_conv1d_cl — conv1d_cl_kernel<256, {128,64,32}, ...>
# --------------------------------------------------------------------------- #
SAME, BIG = "same", "big"
# (T, Cin, Cout, k, dil, pad, pre_slope, act, post_slope, bias, resid, ragged)
CONV_CASES = [
    (700, 192, 256, 3, 1, SAME, 0.125, "none", 0.0, True, True, True),
    (700, 192, 130, 7, 3, SAME, 0.125, "lrelu", 0.25, True, False, False),
    (700, 40, 80, 11, 5, SAME, 0.125, "none", 0.0, True, True, True),
    (700, 24, 33, 5, 16, SAME, 0.25, "none", 0.0, False, False, True),
    (700, 8, 1, 7, 1, SAME, 0.125, "tanh", 0.0, True, False, False),
    (700, 40, 256, 1, 1, 0, 0.0, "relu", 0.0, True, False, False),
    (700, 192, 80, 3, 1, 0, 0.1, "none", 0.0, True, True, True),
    (700, 24, 130, 7, 3, BIG, 0.125, "none", 0.0, True, False, False),
    (700, 8, 33, 11, 5, SAME, 0.1, "lrelu", 0.1, False, True, False),
    (700, 40, 1, 5, 16, 0, 0.25, "tanh", 0.0, False, False, False),
    (700, 192, 33, 7, 3, SAME, 0.25, "relu", 0.0, True, True, True),
    (700, 8, 80, 3, 1, SAME, 0.0, "none", 0.0, False, False, False),
    (700, 24, 256, 11, 5, SAME, 0.125, "lrelu", 0.125, True, False, True),
    (1, 24, 33, 3, 1, SAME, 0.125, "none", 0.0, True, False, False),
    (1, 192, 130, 11, 5, SAME, 0.25, "none", 0.0, True, True, False),
    (255, 40, 80, 7, 3, SAME, 0.125, "none", 0.0, True, False, True),
    (255, 8, 130, 5, 16, BIG, 0.25, "none", 0.0, True, False, False),
    (256, 8, 256, 3, 1, SAME, 0.125, "relu", 0.0, True, False, False),
    (256, 192, 1, 5, 16, SAME, 0.125, "none", 0.0, True, False, True),
    (256, 40, 130, 3, 1, SAME, 0.25, "tanh", 0.0, True, False, True),
    (257, 24, 130, 11, 5, SAME, 0.125, "none", 0.0, True, True, True),
    (257, 40, 33, 1, 1, 0, 0.125, "tanh", 0.0, True, False, False),
    (257, 192, 80, 7, 3, 0, 0.125, "lrelu", 0.25, False, False, False),
    (257, 8, 1, 3, 1, SAME, 0.1, "tanh", 0.0, True, False, True),
    (700, 40, 130, 5, 16, SAME, 0.125, "none", 0.0, True, True, False),
]


@pytest.mark.parametrize(
    "T,Cin,Cout,k,dil,pad,pre,act,post,has_bias,has_res,ragged", CONV_CASES)
def test_conv1d_cl_matrix(dev, T, Cin, Cout, k, dil, pad, pre, act, post,
                          has_bias, has_res, ragged):
    from sonata_amd.ops.functional import leaky_conv1d_cl

    g = _gen(T, Cin, Cout, k, dil)
    halo = (k - 1) * dil
    padding = {SAME: halo // 2, BIG: halo // 2 + 2}.get(pad, pad)
    Tout = T + 2 * padding - halo
    B = 4 if ragged else 2
    x = ko.rounding_free((B, T, Cin), g)
    w = ko.rounding_free((Cout, Cin, k), g, (Cin * k) ** -0.5)
    bias = torch.randn(Cout, generator=g) if has_bias else None
    res = ko.rounding_free((B, Tout, Cout), g) if has_res else None
    lens = _ragged(Tout, 256) if ragged else None
    oracle = ko.conv_cl_oracle(x, w, bias, padding, dil, pre, act, post, res,
                               lens)
    xd, wd, bd, rd, ld = _to(dev, x, w, bias, res, lens)
    got = leaky_conv1d_cl(
        xd, wd, bd, padding=padding, dilation=dil, pre_lrelu=pre,
        post_lrelu=post if act == "lrelu" else 0.0,
        post_tanh=(act == "tanh"), post_relu=(act == "relu"),
        residual=rd, out_lens=ld)
    ko.assert_within(got, oracle, tile=256, what="conv1d_cl")
    # second call hits the cached weight layout: bit-identical
    got2 = leaky_conv1d_cl(
        xd, wd, bd, padding=padding, dilation=dil, pre_lrelu=pre,
        post_lrelu=post if act == "lrelu" else 0.0,
        post_tanh=(act == "tanh"), post_relu=(act == "relu"),
        residual=rd, out_lens=ld)
    assert torch.equal(got, got2)


# --------------------------------------------------------------------------- #
# leaky_convtranspose1d_cl — convt1d_cl_kernel<128, {64,32}, 4, 2, {8,2}, 2>
# --------------------------------------------------------------------------- #
CONVT_SHAPES = [
    (512, 256, 16, 8), (256, 128, 16, 8), (128, 64, 4, 2), (64, 32, 4, 2),
    (96, 48, 16, 8), (40, 16, 4, 2), (72, 80, 16, 8),
]
# every Tin and both paddings appear for both strides; ~2 cases per shape
CONVT_CASES = [
    (0, 129, True, True, True), (0, 1, False, False, False),
    (1, 300, True, True, True), (1, 127, False, True, False),
    (2, 300, True, True, True), (2, 128, False, False, False),
    (3, 129, False, True, True), (3, 1, True, True, False),
    (4, 128, True, False, True), (4, 127, False, True, False),
    (5, 300, False, True, True), (5, 127, True, False, True),
    (5, 1, False, True, False),
    (6, 300, True, True, True), (6, 129, False, False, False),
    (6, 128, True, True, False),
]


@pytest.mark.parametrize("shape,Tin,same_pad,has_bias,ragged", CONVT_CASES)
def test_convtranspose1d_cl_matrix(dev, shape, Tin, same_pad, has_bias,
                                   ragged):
    from sonata_amd.ops.functional import leaky_convtranspose1d_cl

    Cin, Cout, k, s = CONVT_SHAPES[shape]
    g = _gen(Cin, Cout, k, Tin, same_pad)
    pad = (k - s) // 2 if same_pad else 0
    Tout = (Tin - 1) * s - 2 * pad + k
    B = 4 if ragged else 2
    pre = 0.1 if shape == 2 or shape == 6 else 0.125
    x = ko.rounding_free((B, Tin, Cin), g)
    w = ko.rounding_free((Cin, Cout, k), g, (Cin * 2) ** -0.5)
    bias = torch.randn(Cout, generator=g) if has_bias else None
    lens = _ragged(Tout, 128 * s) if ragged else None
    oracle = ko.convt_cl_oracle(x, w, bias, s, pad, pre, lens)
    xd, wd, bd, ld = _to(dev, x, w, bias, lens)
    got = leaky_convtranspose1d_cl(xd, wd, bd, s, pad, pre_lrelu=pre,
                                   out_lens=ld)
    ko.assert_within(got, oracle, tile=128 * s, what="convt1d_cl")


# --------------------------------------------------------------------------- #
# resblock_pair_cl — every channel class x XR bucket, geometries, fallback
# --------------------------------------------------------------------------- #
def _pair_inputs(C, k, dil, T, B, use_accum, key=0):
    g = _gen(C, k, dil, key)
    x = ko.rounding_free((B, T, C), g)
    w1 = ko.rounding_free((C, C, k), g, (C * k) ** -0.5)
    w2 = ko.rounding_free((C, C, k), g, (C * k) ** -0.5)
    b1 = torch.randn(C, generator=g) * 0.3
    b2 = torch.randn(C, generator=g) * 0.3
    accum = ko.rounding_free((B, T, C), g) if use_accum else None
    return x, w1, b1, w2, b2, accum


def _pair_check(dev, C, k, dil, xtr, use_accum, what):
    from sonata_amd.ops.functional import resblock_pair_cl

    T = 600 if C <= 32 else 300
    BM = xtr - (k - 1)              # output rows per block
    assert T >= 2 * BM + 1          # at least 3 time tiles
    x, w1, b1, w2, b2, accum = _pair_inputs(C, k, dil, T, 2, use_accum)
    lens = torch.tensor([T, BM + 3])  # 3 rows past the first tile seam
    scale = 1.0 / 3 if use_accum else 1.0
    oracle = ko.resblock_pair_oracle(x, w1, b1, w2, b2, dil, lens, accum,
                                     scale)
    xd, w1d, b1d, w2d, b2d, ad, ld = _to(dev, x, w1, b1, w2, b2, accum, lens)
    got = resblock_pair_cl(xd, w1d, b1d, w2d, b2d, dilation=dil, out_lens=ld,
                           accum=ad, out_scale=scale)
    ko.assert_within(got, oracle, tile=BM, what=what)


PAIR_CASES = [(C, k, d) for C in (32, 64, 128, 256) for k in (3, 7, 11)
              for d in (1, 3, 5)] + [(16, 7, 3)]


@pytest.mark.parametrize("C,k,dil", PAIR_CASES)
def test_resblock_pair_cl_matrix(dev, C, k, dil):
    xtr = 256 if C <= 32 else (64 if C == 256 else 128)  # default geometry
    use_accum = (PAIR_CASES.index((C, k, dil)) % 2) == 0
    _pair_check(dev, C, k, dil, xtr, use_accum, f"pair C{C} k{k} d{dil}")


@pytest.mark.parametrize("C,geom,xtr", [(128, "xtr64", 64),
                                        (256, "xtr128", 128)])
@pytest.mark.parametrize("k,dil", [(3, 1), (11, 5)])
def test_resblock_pair_cl_geometry(dev, C, geom, xtr, k, dil):
    old = os.environ.get("SONATA_RB_GEOM")
    os.environ["SONATA_RB_GEOM"] = geom
    try:
        _pair_check(dev, C, k, dil, xtr, k == 3, f"pair {geom} C{C} k{k}")
    finally:
        if old is None:
            os.environ.pop("SONATA_RB_GEOM", None)
        else:
            os.environ["SONATA_RB_GEOM"] = old


@pytest.mark.parametrize("C,k,dil", [(96, 3, 1), (64, 11, 6)])
def test_resblock_pair_cl_fallback(dev, C, k, dil):
    """Shapes the fused kernel refuses (C=96 pads to a non-square 128x96
    weight; (k-1)*dil = 60 > 52) take the two-conv path.  It rounds the
    intermediate to bf16 once more than the fused kernel (before and after
    the re-activation); the oracle's one-ulp allowance on the intermediate
    times the headroom covers that, so the same bound applies."""
    from sonata_amd.ops.functional import resblock_pair_cl

    T = 300
    x, w1, b1, w2, b2, _ = _pair_inputs(C, k, dil, T, 2, False, key=1)
    lens = torch.tensor([T, 259])
    oracle = ko.resblock_pair_oracle(x, w1, b1, w2, b2, dil, lens)
    xd, w1d, b1d, w2d, b2d, ld = _to(dev, x, w1, b1, w2, b2, lens)
    got = resblock_pair_cl(xd, w1d, b1d, w2d, b2d, dilation=dil, out_lens=ld)
    ko.assert_within(got, oracle, tile=256, what=f"pair fallback C{C}")


# --------------------------------------------------------------------------- #
# gates
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("g_mode", ["none", "b2c", "b12c", "full"])
@pytest.mark.parametrize("B,Fr,C", [(3, 37, 24), (2, 300, 192)])
def test_fused_gate_cl_matrix(dev, B, Fr, C, g_mode, dtype):
    from sonata_amd.ops.functional import fused_gate_cl

    gen = _gen(B, Fr, C, len(g_mode))
    x = ko.rounding_free((B, Fr, 2 * C), gen, 1.5, dtype)
    g_shape = {"none": None, "b2c": (B, 2 * C), "b12c": (B, 1, 2 * C),
               "full": (B, Fr, 2 * C)}[g_mode]
    g = None if g_shape is None else ko.rounding_free(g_shape, gen, 1.0, dtype)
    oracle = ko.gate_cl_oracle(x, g, C)
    xd, gd = _to(dev, x, g)
    ko.assert_within(fused_gate_cl(xd, gd, C), oracle, what="fused_gate_cl")


@pytest.mark.parametrize("g_mode", ["none", "full", "bcast"])
def test_fused_gate_f32(dev, g_mode):
    from sonata_amd.ops.functional import fused_gate

    B, C, T = 3, 24, 37
    gen = _gen(B, C, T, len(g_mode))
    x = torch.randn((B, 2 * C, T), generator=gen) * 1.5
    g = {"none": None, "full": torch.randn((B, 2 * C, T), generator=gen),
         "bcast": torch.randn((B, 2 * C, 1), generator=gen)}[g_mode]
    oracle = ko.gate_ct_oracle(x, g, C)
    xd, gd = _to(dev, x, g)
    ko.assert_within(fused_gate(xd, gd, C), oracle, time_dim=2, chan_dim=1,
                     what="fused_gate")


# --------------------------------------------------------------------------- #
# depthwise_conv1d_cl
# --------------------------------------------------------------------------- #
DW_CASES = [(C, k, d, T) for C in (8, 192)
            for k, d in ((3, 1), (3, 3), (3, 9), (5, 2)) for T in (1, 5, 300)]


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("C,k,dil,T", DW_CASES)
def test_depthwise_cl_matrix(dev, C, k, dil, T, dtype):
    from sonata_amd.ops.functional import depthwise_conv1d_cl

    i = DW_CASES.index((C, k, dil, T)) + (dtype == F32)
    gen = _gen(C, k, dil, T)
    pad = (k - 1) * dil // 2
    x = ko.rounding_free((2, T, C), gen, 1.0, dtype)
    w = ko.rounding_free((C, 1, k), gen, 0.5, dtype)
    bias = [None, torch.randn(C, generator=gen),
            torch.randn(C, generator=gen).to(BF)][i % 3]
    oracle = ko.depthwise_cl_oracle(x, w, bias, dil, pad)
    xd, wd, bd = _to(dev, x, w, bias)
    ko.assert_within(depthwise_conv1d_cl(xd, wd, bd, dil, pad), oracle,
                     what="depthwise_cl")


# --------------------------------------------------------------------------- #
# layer norms
# --------------------------------------------------------------------------- #
# B*T <= 16384 -> layer_norm_ct_split_kernel, else layer_norm_ct_kernel
LN_CASES = [
    (2, 20, 8200, 0.0), (3, 5, 100, 0.0), (3, 190, 100, 0.0),
]


@pytest.mark.parametrize("resid", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("B,C,T,mu", LN_CASES)
def test_layer_norm_ct_matrix(dev, B, C, T, mu, dtype, resid):
    from sonata_amd.ops.functional import layer_norm_ct

    gen = _gen(B, C, T)
    x = (torch.randn((B, C, T), generator=gen) + mu).to(dtype)
    r = torch.randn((B, C, T), generator=gen).to(dtype) if resid else None
    gamma = torch.randn(C, generator=gen)
    beta = torch.randn(C, generator=gen)
    oracle = ko.layer_norm_ct_oracle(x, gamma, beta, 1e-5, r)
    xd, rd, gd, bd = _to(dev, x, r, gamma, beta)
    got = layer_norm_ct(xd, gd, bd, 1e-5, residual=rd)
    ko.assert_within(got, oracle, time_dim=2, chan_dim=1,
                     what="layer_norm_ct")


@pytest.mark.parametrize("B,C,T", [(2, 192, 8200), (3, 192, 2000)])
def test_layer_norm_ct_offset_f32(dev, B, C, T):
    """N(32,1) inputs in f32 through the unsplit and the split kernel must
    meet the project's f32 tolerance (1e-4 of max|ref|) against fp64.  The
    former one-pass variance ss/C - mean^2 measured ~6e-4 in a CPU emulation
    of its arithmetic at C=192."""
    from sonata_amd.ops.functional import layer_norm_ct

    gen = _gen(B, C, T, 32)
    x = torch.randn((B, C, T), generator=gen) + 32.0
    gamma = torch.randn(C, generator=gen)
    beta = torch.randn(C, generator=gen)
    oracle = ko.layer_norm_ct_oracle(x, gamma, beta, 1e-5)
    xd, gd, bd = _to(dev, x, gamma, beta)
    ko.assert_within(layer_norm_ct(xd, gd, bd, 1e-5), oracle, time_dim=2,
                     chan_dim=1, what="layer_norm_ct offset")


@pytest.mark.parametrize("mu", [0.0, 32.0])
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("rows", [1, 7])
@pytest.mark.parametrize("C", [8, 80, 512])
def test_row_ln_cl_matrix(dev, C, rows, dtype, mu):
    from sonata_amd.ops.functional import row_ln_cl

    gen = _gen(C, rows, mu)
    x = (torch.randn((1, rows, C), generator=gen) + mu).to(dtype)
    r = torch.randn((1, rows, C), generator=gen).to(dtype) \
        if rows == 7 else None
    gamma = torch.randn(C, generator=gen)
    beta = torch.randn(C, generator=gen)
    oracle = ko.row_ln_cl_oracle(x, gamma, beta, 1e-5, r)
    xd, rd, gd, bd = _to(dev, x, r, gamma, beta)
    ko.assert_within(row_ln_cl(xd, gd, bd, 1e-5, residual=rd), oracle,
                     what="row_ln_cl")


# --------------------------------------------------------------------------- #
# small fills
# --------------------------------------------------------------------------- #
def test_prior_sample_f32_ragged(dev):
    from sonata_amd.ops.functional import prior_sample

    gen = _gen(7)
    B, C, T = 3, 24, 77
    m = torch.randn((B, C, T), generator=gen)
    logs = torch.randn((B, C, T), generator=gen) * 0.5
    noise = torch.randn((B, C, T), generator=gen)
    lens = torch.tensor([T, 40, 0])
    mask = (torch.arange(T).unsqueeze(0) < lens.unsqueeze(1)).float() \
        .unsqueeze(1)
    oracle = ko.prior_sample_oracle(m, logs, mask, noise, 0.667)
    md, ld, kd, nd = _to(dev, m, logs, mask, noise)
    got = prior_sample(md, ld, kd, nd, 0.667)
    ko.assert_within(got, oracle, time_dim=2, chan_dim=1, what="prior_sample")
    assert got[1, :, 40:].abs().max().item() == 0
    assert got[2].abs().max().item() == 0


@pytest.mark.parametrize("dtype", [F32, BF])
def test_mask_tail_long_length(dev, dtype):
    from sonata_amd.ops.functional import mask_tail_

    gen = _gen(8)
    B, C, T = 3, 5, 300
    x = torch.randn((B, C, T), generator=gen).to(dtype)
    lens = torch.tensor([T + 7, 257, 0])   # one length greater than T
    ref = x.clone()
    ref[1, :, 257:] = 0
    ref[2] = 0
    xd, ld = _to(dev, x, lens)
    got = mask_tail_(xd, ld)
    assert got.data_ptr() == xd.data_ptr()  # in place
    assert torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("dtype", [F32, BF])
def test_expand_states_edges(dev, dtype):
    """Leading zero duration, trailing zero duration, an all-zero row, and
    F_max smaller than a row's sum.  The gather is a copy: exact."""
    from sonata_amd.ops.functional import expand_states

    gen = _gen(9)
    durs = torch.tensor([[0, 3, 1, 0, 2, 0],     # leading + trailing zero
                         [0, 0, 0, 0, 0, 0],     # all zero
                         [4, 4, 4, 4, 4, 4],     # sum 24 > F_max
                         [1, 0, 0, 5, 0, 1]])
    B, T_ph = durs.shape
    C, F_max = 7, 10
    stats = torch.randn((B, C, T_ph), generator=gen).to(dtype)
    y_len = durs.sum(1).clamp(max=F_max)
    sd, dd, yd = _to(dev, stats, durs, y_len)
    got = expand_states(sd, dd, yd, F_max=F_max).cpu()
    assert got.shape == (B, C, F_max)
    for b in range(B):
        idx = torch.repeat_interleave(torch.arange(T_ph), durs[b])[:F_max]
        n = int(y_len[b])
        assert idx.numel() == n
        assert torch.equal(got[b, :, :n], stats[b][:, idx])


def test_expand_states_single_phoneme(dev):
    from sonata_amd.ops.functional import expand_states

    stats = torch.randn((2, 5, 1), generator=_gen(10))
    durs = torch.tensor([[6], [2]])
    y_len = torch.tensor([6, 2])
    sd, dd, yd = _to(dev, stats, durs, y_len)
    got = expand_states(sd, dd, yd).cpu()
    assert got.shape == (2, 5, 6)
    assert torch.equal(got[0], stats[0].expand(5, 6))
    assert torch.equal(got[1, :, :2], stats[1].expand(5, 2))
