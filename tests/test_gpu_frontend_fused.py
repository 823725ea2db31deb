"""Fused front-end glue of the C++ engine (csrc/elementwise.hip wn_step,
coupling_tail, flow_split_rev; the strided prior_sample; the dense spline)
against the eager chains it replaces.

Every comparison is BITWISE (torch.equal on the bf16 tensors, and on their
int16 views where the sign of a zero matters): the fused kernels restate the
eager chain's f32 operations in the same order and round to bf16 wherever
the chain materialised a bf16 tensor, so there is no tolerance to derive.
The eager references are composed from the same torch ops the engine's
SONATA_FUSED_FRONT=0 path runs.
"""

import os

import pytest
import torch

from sonata_amd.models import create_random_voice
from sonata_amd.ops import functional as Fn
from sonata_amd.ops import hip_ext

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
H, HALF = 192, 96
FS = (1, 7, 300)
B = 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gen(*key):
    seed = 41
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _mask(F, dev):
    """[B,F,1] bf16 mask of ragged lengths [F, F//2, 0]."""
    lens = torch.tensor([F, F // 2, 0])
    m = (torch.arange(F).unsqueeze(0) < lens.unsqueeze(1)).unsqueeze(-1)
    return m.to(BF).to(dev)


def _rand(g, dev, *shape):
    """bf16 normal values with exact and negative zeros sprinkled in."""
    t = torch.randn(*shape, generator=g)
    flat = t.view(-1)
    flat[::7] = -0.0
    flat[3::11] = 0.0
    return t.to(BF).to(dev)


def _bits_equal(a, b):
    return (a.shape == b.shape and a.dtype == b.dtype and
            torch.equal(a.contiguous().view(torch.int16),
                        b.contiguous().view(torch.int16)))


# ------------------------------------------------------------------ wn_step
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("layer", (0, 1, 2))
def test_wn_step_bitwise(dev, F, layer):
    g = _gen(1, F, layer)
    mc = _mask(F, dev)
    h = _rand(g, dev, B, F, H)
    rs = _rand(g, dev, B, F, H if layer == 2 else 2 * H)
    out = torch.zeros_like(h) if layer == 0 else _rand(g, dev, B, F, H)
    # the eager chain (vits_engine.cpp flow_reverse, SONATA_FUSED_FRONT=0)
    if layer < 2:
        h_ref = (h + rs.narrow(-1, 0, H)) * mc
        out_ref = out + rs.narrow(-1, H, H)
    else:
        out_ref = (out + rs) * mc
        h_ref = None
    hk = h.clone()
    ok = Fn.wn_step(hk, None if layer == 0 else out.clone(), rs, mc, layer)
    assert _bits_equal(ok, out_ref)
    if h_ref is not None:
        assert _bits_equal(hk, h_ref)
    if layer == 0:
        # 0 + (-0) is +0: the first layer must not copy rs through
        neg0 = rs.narrow(-1, H, H).view(torch.int16) == -32768
        assert bool(neg0.any())
        assert bool((ok.view(torch.int16)[neg0] == 0).all())


# ------------------------------------------------------------ coupling tail
@pytest.mark.parametrize("F", FS)
def test_flow_split_rev_bitwise(dev, F):
    xc = _rand(_gen(2, F), dev, B, F, 2 * HALF)
    fl = torch.flip(xc, [-1])
    x0, x1 = Fn.flow_split_rev(xc)
    assert x0.is_contiguous() and x1.is_contiguous()
    assert _bits_equal(x0, fl.narrow(-1, 0, HALF).contiguous())
    assert _bits_equal(x1, fl.narrow(-1, HALF, HALF).contiguous())


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("last", (False, True))
def test_coupling_tail_bitwise(dev, F, last):
    g = _gen(3, F, last)
    mc = _mask(F, dev)
    x0 = _rand(g, dev, B, F, HALF)
    x1 = _rand(g, dev, B, F, HALF)
    post = _rand(g, dev, B, F, HALF)
    m = post * mc
    xc = torch.cat([x0, (x1 - m) * mc], -1)
    if last:
        got = Fn.coupling_tail(x0, x1, post, mc, True)
        assert _bits_equal(got, xc)
        return
    fl = torch.flip(xc, [-1])
    n0, n1 = Fn.coupling_tail(x0, x1, post, mc, False)
    assert _bits_equal(n0, fl.narrow(-1, 0, HALF).contiguous())
    assert _bits_equal(n1, fl.narrow(-1, HALF, HALF).contiguous())


# --------------------------------------------------- four flows, end to end
def _flow_weights(dev):
    g = _gen(4)

    def w(o, i):
        return (torch.randn(o, i, generator=g) / i ** 0.5).to(BF).to(dev)

    flows = []
    for _ in range(4):
        flows.append({
            "pre": w(H, HALF), "post": w(HALF, H),
            "rs": [w(2 * H, H), w(2 * H, H), w(2 * H, H), w(H, H)],
        })
    return flows


def _flow_eager(x, mc, flows):
    """vits_engine.cpp flow_reverse, eager glue; the gated conv stack of each
    WaveNet layer is stood in for by tanh (the glue cannot tell)."""
    lin = torch.nn.functional.linear
    xc = x.transpose(1, 2).contiguous()
    for fw in flows:
        xc = torch.flip(xc, [-1])
        x0 = xc.narrow(-1, 0, HALF).contiguous()
        x1 = xc.narrow(-1, HALF, HALF)
        h = lin(x0, fw["pre"]) * mc
        output = torch.zeros_like(h)
        for i in range(4):
            rs = lin(torch.tanh(h), fw["rs"][i])
            if i < 3:
                h = (h + rs.narrow(-1, 0, H)) * mc
                output = output + rs.narrow(-1, H, H)
            else:
                output = output + rs
        h = output * mc
        m = lin(h, fw["post"]) * mc
        x1 = (x1 - m) * mc
        xc = torch.cat([x0, x1], -1)
    return xc.transpose(1, 2).contiguous()


def _flow_fused(x, mc, flows):
    lin = torch.nn.functional.linear
    x0, x1 = Fn.flow_split_rev(x.transpose(1, 2).contiguous())
    for n, fw in enumerate(flows):
        h = lin(x0, fw["pre"]) * mc
        output = None
        for i in range(4):
            rs = lin(torch.tanh(h), fw["rs"][i])
            if i == 0:
                output = Fn.wn_step(h, None, rs, mc, 0)
            elif i < 3:
                Fn.wn_step(h, output, rs, mc, 1)
            else:
                h = Fn.wn_step(h, output, rs, mc, 2)
        post = lin(h, fw["post"])
        if n == len(flows) - 1:
            return Fn.coupling_tail(x0, x1, post, mc, True) \
                .transpose(1, 2).contiguous()
        x0, x1 = Fn.coupling_tail(x0, x1, post, mc, False)


@pytest.mark.parametrize("F", FS)
def test_four_flows_chained_bitwise(dev, F):
    flows = _flow_weights(dev)
    mc = _mask(F, dev)
    x = _rand(_gen(5, F), dev, B, 2 * HALF, F)
    want = _flow_eager(x, mc, flows)
    got = _flow_fused(x, mc, flows)
    assert bool(torch.isfinite(want.float()).all())
    assert _bits_equal(got, want)


# ------------------------------------------------------------- DDS kernels
DDS_CT = [(C, T) for C in (192, 8) for T in (1, 5, 70)]


def _dds_params(g, dev, C):
    """Depthwise weight [C,1,3] bf16; bias, gamma, beta as the engine holds
    them: f32 copies of bf16 parameters."""
    w = (torch.randn(C, 1, 3, generator=g) * 0.5).to(BF).to(dev)
    f32 = [(torch.randn(C, generator=g) * s + o).to(BF).float().to(dev)
           for s, o in ((0.1, 0.0), (0.2, 1.0), (0.1, 0.0))]
    return w, f32[0], f32[1], f32[2]


@pytest.mark.parametrize("C,T", DDS_CT)
@pytest.mark.parametrize("dil", (1, 3, 9))
@pytest.mark.parametrize("with_g", (False, True))
def test_dds_sep_ln_gelu_bitwise(dev, C, T, dil, with_g):
    """T=1, and T=5 at dilation 9, leave only the centre tap inside [0,T)."""
    g = _gen(8, C, T, dil, with_g)
    mc = _mask(T, dev)
    x = _rand(g, dev, B, T, C)
    gc = _rand(g, dev, B, T, C) if with_g else None
    w, bias, gamma, beta = _dds_params(g, dev, C)
    # the eager chain (vits_engine.cpp dds_cl, SONATA_FUSED_FRONT=0)
    t_ref = x + gc if with_g else x
    y_ref = Fn.depthwise_conv1d_cl((t_ref * mc).contiguous(), w, bias, dil,
                                   dil)
    y_ref = torch.nn.functional.gelu(Fn.row_ln_cl(y_ref, gamma, beta))
    y, t = Fn.dds_sep_ln_gelu(x, gc, mc, w, bias, gamma, beta, dil)
    assert bool(torch.isfinite(y_ref.float()).all())
    assert _bits_equal(t, t_ref)
    assert _bits_equal(y, y_ref)


@pytest.mark.parametrize("C,T", DDS_CT)
@pytest.mark.parametrize("last", (False, True))
def test_ln_gelu_add_bitwise(dev, C, T, last):
    g = _gen(9, C, T, last)
    mc = _mask(T, dev)
    y = _rand(g, dev, B, T, C)
    t = _rand(g, dev, B, T, C)
    _, _, gamma, beta = _dds_params(g, dev, C)
    ref = t + torch.nn.functional.gelu(Fn.row_ln_cl(y, gamma, beta))
    if last:
        ref = ref * mc
    got = Fn.ln_gelu_add(y, t, mc, gamma, beta, last)
    assert _bits_equal(got, ref)


# ------------------------------------------------------ strided prior_sample
@pytest.mark.parametrize("F", FS)
def test_prior_sample_stats_halves_bitwise(dev, F):
    """m and logs as the two channel halves of one [B,2C,F] tensor (what one
    expand over the unchunked stats hands over) against contiguous copies."""
    g = _gen(6, F)
    C = HALF
    stats = _rand(g, dev, B, 2 * C, F)
    noise = _rand(g, dev, B, C, F)
    mask = _mask(F, dev).transpose(1, 2).contiguous()
    ext = hip_ext(required=True)
    m, logs = stats.narrow(1, 0, C), stats.narrow(1, C, C)
    want = ext.prior_sample(m.contiguous(), logs.contiguous(), mask, noise,
                            0.667)
    got = ext.prior_sample(m, logs, mask, noise, 0.667)
    assert _bits_equal(got, want)


# ---------------------------------------------------------------- the spline
def test_dense_spline_matches_python_dense_form(dev):
    """3x70 bf16 elements with tails and exact +-5: the engine's dense form
    against vits.rational_quadratic_spline (the same dense ATen operations,
    issued from Python)."""
    from sonata_amd.models.vits import rational_quadratic_spline

    g = _gen(7)
    Bq, T = 3, 70
    z = torch.randn(Bq, 1, T, generator=g) * 2.5
    z[0, 0, 0], z[0, 0, 1], z[0, 0, 2], z[0, 0, 3] = 5.0, -5.0, 7.25, -6.5
    z[2] = torch.linspace(5.5, 40.0, T)
    z = z.to(BF).to(dev)
    uw = torch.randn(Bq, 1, T, 10, generator=g).to(BF).to(dev)
    uh = torch.randn(Bq, 1, T, 10, generator=g).to(BF).to(dev)
    ud = torch.randn(Bq, 1, T, 9, generator=g).to(BF).to(dev)
    want, _ = rational_quadratic_spline(z, uw, uh, ud, inverse=True,
                                        tail_bound=5.0)
    got = Fn.rq_spline_inverse(z, uw, uh, ud, 5.0)
    assert _bits_equal(got, want)
    outside = (z < -5.0) | (z > 5.0)
    assert bool(outside[2].all())
    assert torch.equal(got[outside], z[outside])
    # the HIP tail kernel against the dense ATen form, contiguous inputs and
    # the engine's strided ones (z1 is channel 1 of a [B,2,T] state)
    assert bool(torch.isfinite(got.float()).all())
    tail = Fn.rq_spline_inverse(z, uw, uh, ud, 5.0, tail_kernel=True)
    assert _bits_equal(tail, got)
    z2 = torch.cat([torch.zeros_like(z), z], 1)
    tail = Fn.rq_spline_inverse(z2.narrow(1, 1, 1), uw, uh, ud, 5.0,
                                tail_kernel=True)
    assert _bits_equal(tail, got)


# ------------------------------------------------------------- whole engine
def test_engine_fused_front_bitwise(dev, tmp_path):
    """x_low random voice, 3 ragged sentences: infer under the default and
    under SONATA_FUSED_FRONT=0 (read per call) gives equal audio_lengths and
    bitwise-equal audio."""
    ext = hip_ext(required=True)
    pack = create_random_voice(str(tmp_path), "ff_voice", quality="x_low")
    eng = ext.VitsEngine(pack, "cuda:0", "bf16")
    rows = [eng.phonemes_to_ids(p) for p in
            ("wˈʌn.", "tˈuː θɹˈiː fˈoːɹ.",
             "hˈɛloʊ ˈɛvɹiwˌʌn, haʊ ˈɑːɹ juː tʊdˈeɪ?")]
    ids = torch.zeros(len(rows), max(map(len, rows)), dtype=torch.long)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = torch.tensor(r)
    lengths = torch.tensor([len(r) for r in rows])
    old = os.environ.get("SONATA_FUSED_FRONT")
    try:
        os.environ.pop("SONATA_FUSED_FRONT", None)
        a1, l1 = eng.infer(ids, lengths, None, 0.667, 1.0, 0.8, [3, 4, 5])
        os.environ["SONATA_FUSED_FRONT"] = "0"
        a0, l0 = eng.infer(ids, lengths, None, 0.667, 1.0, 0.8, [3, 4, 5])
    finally:
        if old is None:
            os.environ.pop("SONATA_FUSED_FRONT", None)
        else:
            os.environ["SONATA_FUSED_FRONT"] = old
    assert torch.equal(l0.cpu(), l1.cpu())
    assert int(l1.min()) > 0 and len(set(l1.cpu().tolist())) == 3
    assert a0.dtype == a1.dtype and a0.shape == a1.shape
    assert bool(torch.isfinite(a1.float()).all())
    assert _bits_equal(a0, a1)
