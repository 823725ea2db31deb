"""attn_relpos_cl (csrc/attention_cl.hip) against the fp64 oracle of
tests/attention_oracle.py, element by element on every valid row.

The matrix (attention_oracle.MATRIX, also run through an f32 emulation of
the kernel on the CPU by tests/test_attention_oracle_cpu.py) reaches all
four DPAD instantiations at every head size the binding admits per class,
1/2/4 heads, T on both sides of the 64-key tile seams, window 0/1/4/7,
lens None and ragged (T, T-1, 65, 64, w, 1, 0, T+5), three input regimes
and two isolating probes.  The extension is called directly so that the
oracle sees exactly the kernel's inputs; a few cases go through
ops.attn_relpos_cl for the cached fused-projection path.  Exact properties
(padding independence, batch invariance, determinism) are asserted bitwise,
and every refusal of the binding is walked.
"""

import pytest
import torch

import attention_oracle as ao

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from sonata_amd.ops import hip_ext

    return hip_ext(required=True)


def _run(ext, dev, case, inp):
    lens = None if inp.lens is None else inp.lens.to(dev)
    out = ext.attn_relpos_cl(inp.qkv.to(dev), inp.rel_k.to(dev),
                             inp.rel_v.to(dev), lens, heads=case.H,
                             window=case.w, scale=case.scale)
    return out.cpu()


# --------------------------------------------------------------------------- #
# the matrix
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("case", ao.MATRIX, ids=lambda c: c.id)
def test_attn_relpos_cl_matrix(dev, ext, case):
    inp = ao.make_case(case)
    oracle = ao.case_oracle(case, inp)
    got = _run(ext, dev, case, inp)
    assert got.dtype == BF and got.shape == oracle.ref.shape
    worst = ao.assert_within(got, oracle, case.D,
                             f"attn_relpos_cl {case.id}")
    print(f"ATTN_RATIO {case.regime} {case.id} {worst:.4f}")


# --------------------------------------------------------------------------- #
# through the wrapper: cached fused projection and tables
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("C,h,T,ragged", [(192, 2, 129, True),
                                          (96, 2, 200, True),
                                          (96, 2, 65, False)])
def test_ops_wrapper_cached_path(dev, ext, C, h, T, ragged):
    """ops.attn_relpos_cl with a sharpened RelativeAttention whose conv_o is
    the identity (bf16 x·1 summed with zeros in f32 is exact), so the
    wrapper's output IS the kernel's output: bitwise equal to the direct
    call on the same fused projection, within the oracle bound, and the
    second call (served from the module's cache) gives the same bits."""
    import torch.nn.functional as F
    from sonata_amd.models.vits import RelativeAttention
    from sonata_amd.ops import attn_relpos_cl

    torch.manual_seed(C + T)
    m = RelativeAttention(C, h).eval()
    with torch.no_grad():
        m.conv_q.weight.mul_(8.0)
        m.emb_rel_k.mul_(8.0)
        m.emb_rel_v.mul_(8.0)
        m.conv_o.weight.copy_(torch.eye(C).unsqueeze(-1))
        m.conv_o.bias.zero_()
    rel_k_ref = m.emb_rel_k[0].detach().to(BF)
    m = m.to(dev, BF)
    B = 3 if ragged else 1
    lens = torch.tensor(ao.ragged(T, 4, 1)) if ragged else None  # int64
    x = torch.randn(B, T, C).to(BF).to(dev)
    lens_d = None if lens is None else lens.to(dev)
    with torch.no_grad():
        got = attn_relpos_cl(x, m, lens_d)
        assert m._rel_k.cpu().equal(rel_k_ref)
        qkv = F.linear(x, m._qkv_w, m._qkv_b)
        direct = ext.attn_relpos_cl(
            qkv, m._rel_k, m._rel_v,
            None if lens is None else lens_d.to(torch.int32), heads=h,
            window=m.window_size, scale=m.head_dim ** -0.5)
        again = attn_relpos_cl(x, m, lens_d)
    assert torch.equal(got, direct) and torch.equal(got, again)
    oracle = ao.attention_oracle(qkv.cpu(), m._rel_k.cpu(), m._rel_v.cpu(),
                                 lens, h, m.window_size, m.head_dim ** -0.5)
    worst = ao.assert_within(got.cpu(), oracle, C // h,
                             f"ops.attn_relpos_cl C={C} h={h} T={T}")
    print(f"ATTN_RATIO wrapper C{C}-h{h}-T{T} {worst:.4f}")


# --------------------------------------------------------------------------- #
# exact properties, read from the kernel
# --------------------------------------------------------------------------- #
PROPERTY_CASES = [
    ao.Case("peaked", 3, 129, 2, 96, 4, (128, 64, 1)),
    ao.Case("planted", 3, 200, 2, 48, 4, (4, 205, 65)),
    ao.Case("peaked", 3, 65, 4, 8, 7, (65, 0, 7)),
    ao.Case("flat", 3, 130, 1, 128, 1, (129, 65, 0)),
]


@pytest.mark.parametrize("case", PROPERTY_CASES, ids=lambda c: c.id)
def test_padding_batch_invariance_and_determinism(dev, ext, case):
    """Masked scores are overwritten with -1e4 before the row max, so p is
    exactly 0 for padded keys whatever they hold, and blocks share nothing
    across the batch: tolerance 0 throughout."""
    inp = ao.make_case(case)
    valid = ao.case_oracle(case, inp).valid
    base = _run(ext, dev, case, inp)
    assert torch.equal(base, _run(ext, dev, case, inp)), "not deterministic"

    # every qkv row at or past lens[b] filled with +-1e3
    L = ao.live_lengths(inp.lens, case.B, case.T)
    pad = torch.arange(case.T).unsqueeze(0) >= L.unsqueeze(1)       # [B,T]
    sign = torch.where(torch.arange(inp.qkv.shape[-1]) % 2 == 0, 1e3, -1e3)
    loud = torch.where(pad.unsqueeze(-1), sign.to(BF), inp.qkv)
    got = _run(ext, dev, case, inp._replace(qkv=loud.contiguous()))
    assert bool(torch.isfinite(got.float()).all()), "non-finite padded row"
    assert bool(torch.isfinite(base.float()).all())
    assert torch.equal(got[valid], base[valid]), \
        "valid rows depend on what the padded rows hold"

    # each row of the ragged batch alone
    for b in range(case.B):
        one = case._replace(B=1, lens=(case.lens[b],))
        alone = _run(ext, dev, one, ao.Inputs(
            inp.qkv[b:b + 1].contiguous(), inp.rel_k, inp.rel_v,
            inp.lens[b:b + 1]))
        assert torch.equal(alone[0], base[b]), f"row {b} differs run alone"


def test_empty_row_and_lens_none_equivalence(dev, ext):
    """len = 0: no valid row, every output finite.  lens = None equals
    lens = [T] bitwise."""
    case = ao.Case("peaked", 3, 129, 2, 48, 4, (0, 0, 0))
    inp = ao.make_case(case)
    got = _run(ext, dev, case, inp)
    assert bool(torch.isfinite(got.float()).all())
    full = case._replace(lens=(129, 134, 129))
    a = _run(ext, dev, full, inp._replace(
        lens=torch.tensor(full.lens, dtype=torch.int32)))
    b = _run(ext, dev, full, inp._replace(lens=None))
    assert torch.equal(a, b)


# --------------------------------------------------------------------------- #
# the binding refuses, before any launch, what the kernel would read out of
# bounds or from the wrong memory
# --------------------------------------------------------------------------- #
def test_binding_refusals(dev, ext):
    B, T, H, D, w = 2, 5, 2, 16, 4
    g = torch.Generator().manual_seed(3)

    def bf(*shape):
        return torch.randn(*shape, generator=g).to(BF).to(dev)

    ok = dict(qkv=bf(B, T, 3 * H * D), rel_k=bf(2 * w + 1, D),
              rel_v=bf(2 * w + 1, D),
              lens=torch.tensor([5, 3], dtype=torch.int32, device=dev),
              heads=H, window=w, scale=D ** -0.5)
    out = ext.attn_relpos_cl(**ok)
    assert out.shape == (B, T, H * D)

    def refused(**change):
        with pytest.raises(RuntimeError):
            ext.attn_relpos_cl(**{**ok, **change})
            torch.cuda.synchronize()

    # qkv
    refused(qkv=ok["qkv"][0])                                  # 2-D
    refused(qkv=ok["qkv"].cpu())
    refused(qkv=bf(B, T, 6 * H * D)[:, :, ::2])                # strided
    refused(qkv=ok["qkv"].float())
    refused(qkv=bf(B, T, 3 * H * D + 2))                       # not 3*H*D
    refused(qkv=bf(B, T, 3 * H * 12), rel_k=bf(2 * w + 1, 12),
            rel_v=bf(2 * w + 1, 12))                           # 8 !| D
    refused(qkv=bf(1, 2, 3 * 136), heads=1, rel_k=bf(2 * w + 1, 136),
            rel_v=bf(2 * w + 1, 136))                          # D > 128
    # heads / window
    refused(heads=0)
    refused(heads=-2)
    refused(window=-1)
    refused(window=8, rel_k=bf(17, D), rel_v=bf(17, D))        # > 16 slots
    # tables: shape
    refused(rel_k=bf(2 * w, D))                                # short table
    refused(rel_v=bf(2 * w, D))
    refused(rel_k=bf(2 * w + 2, D))
    refused(rel_k=bf(1, 2 * w + 1, D))                         # 3-D
    refused(rel_v=bf(1, 2 * w + 1, D))
    refused(rel_k=bf(2 * w + 1, D + 8))                        # wrong D
    refused(rel_v=bf(2 * w + 1, D - 8))
    refused(window=3)                                          # 9 rows, w = 3
    # tables: memory
    refused(rel_k=bf(2 * w + 1, 2 * D)[:, ::2])                # strided
    refused(rel_v=bf(2 * w + 1, 2 * D)[:, ::2])
    refused(rel_k=ok["rel_k"].float())
    refused(rel_v=ok["rel_v"].float())
    refused(rel_k=ok["rel_k"].cpu())                           # host pointer
    refused(rel_v=ok["rel_v"].cpu())
    # lens
    refused(lens=ok["lens"].long())
    refused(lens=ok["lens"].cpu())                             # host pointer
    refused(lens=ok["lens"][:1])                               # B-1 elements
    refused(lens=torch.zeros(B + 1, dtype=torch.int32, device=dev))
    refused(lens=torch.zeros(B, 1, dtype=torch.int32, device=dev))
    refused(lens=torch.zeros(2 * B, dtype=torch.int32, device=dev)[::2])
    # an empty batch still validates lens and tables, and launches nothing
    refused(qkv=bf(0, T, 3 * H * D))                           # lens has 2
    empty = ext.attn_relpos_cl(**{**ok, "qkv": bf(0, T, 3 * H * D),
                                  "lens": None})
    assert empty.shape == (0, T, H * D)
    # and the conforming call still gives the same bits afterwards
    assert torch.equal(ext.attn_relpos_cl(**ok), out)
