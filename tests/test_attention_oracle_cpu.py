"""The attention oracle (tests/attention_oracle.py) checked without a GPU:

* its sign/slot convention against the model's own definition (fp64
  RelativeAttention, both layouts);
* an honest f32 emulation of the kernel's schedule stays under the bound
  on every case of the GPU matrix;
* every listed way of getting the kernel subtly wrong is rejected by the
  bound on a matrix case (the two seam mutants on a case with T > 64);
* the global metric of the older attention tests accepts zeroed and
  mirrored relative tables at T = 200 while the bound rejects them.
"""

import pytest
import torch

import attention_oracle as ao

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64

HANDFUL = 16   # "more than a handful" of elements over the bound


# --------------------------------------------------------------------------- #
# f32 emulation of the kernel's schedule, with switchable defects
# --------------------------------------------------------------------------- #
MUTANTS = (
    "seam_band_drop",      # band entry not recorded for the first key column
                           # of a later tile
    "band_stale_max",      # band probabilities against the max at recording
    "acco_not_rescaled",
    "relk_slot_shift",     # rel_k slot delta+w+1 used for delta
    "relv_mirrored",
    "mask_off_by_one",     # j > len instead of j >= len
    "masked_logit_zero",   # 0 instead of -1e4
    "heads_swapped",
    "scale_omitted",
    "l_from_bf16_p",       # row sum from the rounded P + unrounded band p
)


def _bf(x):
    return x.to(BF).to(F32)


def emulate_kernel(qkv, rel_k, rel_v, lens, H, w, scale, mutant=None):
    """csrc/attention_cl.hip in f32 torch on the CPU: bf16 scaled Q, f32
    logits, 64-key tiles with a running max and rescale, P rounded to bf16
    for PV, f32 row sum from the unrounded p, band scores recorded per tile
    and exponentiated against the final max, one bf16 store."""
    B, T, _ = qkv.shape
    nslot = 2 * w + 1
    q, k, v = (x.to(F32) for x in ao.split_heads(qkv, H))
    D = q.shape[-1]
    rk, rv = rel_k.to(F32), rel_v.to(F32)
    qs = q if mutant == "scale_omitted" else \
        _bf(q * torch.tensor(scale, dtype=F32))
    delta, inband, slot = ao.band_index(T, w)
    bqk = qs @ rk.t()                                   # [B,H,T,nslot]
    if mutant == "relk_slot_shift":
        bqk = torch.cat([bqk[..., 1:], torch.zeros_like(bqk[..., :1])], -1)
    s_all = qs @ k.transpose(-1, -2) + ao._band_scatter(bqk, inband, slot)
    L = ao.live_lengths(lens, B, T).view(B, 1, 1, 1)
    j = torch.arange(T).view(1, 1, 1, T)
    masked = (j > L) if mutant == "mask_off_by_one" else (j >= L)
    fill = 0.0 if mutant == "masked_logit_zero" else -1e4
    s_all = torch.where(masked, torch.tensor(fill, dtype=F32), s_all)

    m_run = torch.full((B, H, T), -3.0e38, dtype=F32)
    l_run = torch.zeros(B, H, T, dtype=F32)
    acc = torch.zeros(B, H, T, D, dtype=F32)
    sband = torch.full((B, H, T, nslot), float("-inf"), dtype=F32)
    mrec = torch.zeros(B, H, T, nslot, dtype=F32)
    rows = torch.arange(T)
    for j0 in range(0, T, 64):
        j1 = min(j0 + 64, T)
        s = s_all[..., j0:j1]
        m_new = torch.maximum(m_run, s.max(-1).values)
        fscale = torch.exp(m_run - m_new)
        m_run = m_new
        p = torch.exp(s - m_run.unsqueeze(-1))
        pb = _bf(p)
        tsum = (pb if mutant == "l_from_bf16_p" else p).sum(-1)
        l_run = l_run * fscale + tsum
        if mutant != "acco_not_rescaled":
            acc = acc * fscale.unsqueeze(-1)
        acc = acc + pb @ v[..., j0:j1, :]
        for dlt in range(-w, w + 1):
            key = rows + dlt
            ok = (key >= j0) & (key < j1)
            if mutant == "seam_band_drop":
                ok &= ~((key % 64 == 0) & (key > 0))
            r = rows[ok]
            sband[:, :, r, dlt + w] = s_all[:, :, r, r + dlt]
            mrec[:, :, r, dlt + w] = m_run[:, :, r]
    m_fin = mrec if mutant == "band_stale_max" else m_run.unsqueeze(-1)
    pband = torch.where(torch.isfinite(sband), torch.exp(sband - m_fin),
                        torch.zeros((), dtype=F32))
    if mutant == "relv_mirrored":
        rv = rv.flip(0)
    out = (acc + pband @ rv) * (1.0 / l_run).unsqueeze(-1)
    if mutant == "heads_swapped":
        out = out.flip(1)
    return out.to(BF).permute(0, 2, 1, 3).reshape(B, T, H * D)


_CACHE = {}


def _prepared(case):
    """Inputs and oracle of a matrix case, computed once and left alone."""
    if case not in _CACHE:
        inp = ao.make_case(case)
        _CACHE[case] = (inp, ao.case_oracle(case, inp))
    return _CACHE[case]


# --------------------------------------------------------------------------- #
# sign and slot convention: the oracle is the model
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("w", [0, 1, 4, 7])
@pytest.mark.parametrize("T", [1, 3, 5, 64, 65, 130])
def test_oracle_equals_fp64_module(T, w):
    """qkv projection -> oracle (q rounding off) -> conv_o in fp64 equals
    RelativeAttention.double().forward_cl and .forward on valid rows to
    1e-10.  T <= w exercises the table crop in _rel_embeddings; ties
    'slot = delta + w, delta = key - query' to the model, not the kernel."""
    from sonata_amd.models.vits import RelativeAttention

    torch.manual_seed(1000 + 10 * T + w)
    C, H = 32, 2
    m = RelativeAttention(C, H, window_size=w).double().eval()
    with torch.no_grad():   # sharpen: default init gives near-flat softmax
        m.conv_q.weight.mul_(6.0)
        m.emb_rel_k.mul_(4.0)
        m.emb_rel_v.mul_(4.0)
    lens = torch.tensor([T, 1, max(T - 1, 1), max(T // 2, 1)])
    B = len(lens)
    x = torch.randn(B, T, C, dtype=F64)
    mask = (torch.arange(T).unsqueeze(0) < lens.unsqueeze(1)).to(F64)
    x = x * mask.unsqueeze(-1)
    attn_mask = (mask.unsqueeze(2) * mask.unsqueeze(1)).unsqueeze(1)
    with torch.no_grad():
        ref_cl = m.forward_cl(x, attn_mask)                       # [B,T,C]
        ref_cf = m.forward(x.transpose(1, 2), attn_mask).transpose(1, 2)
        wq = torch.cat([m.conv_q.weight, m.conv_k.weight,
                        m.conv_v.weight]).squeeze(-1)
        bq = torch.cat([m.conv_q.bias, m.conv_k.bias, m.conv_v.bias])
        qkv = torch.nn.functional.linear(x, wq, bq)
        o = ao.attention_oracle(qkv, m.emb_rel_k[0], m.emb_rel_v[0], lens,
                                H, w, m.head_dim ** -0.5, round_q=False)
        got = torch.nn.functional.linear(o.ref, m.conv_o.weight.squeeze(-1),
                                         m.conv_o.bias)
    assert o.valid.equal(mask.bool())
    for name, ref in (("forward_cl", ref_cl), ("forward", ref_cf)):
        err = ((got - ref).abs() * mask.unsqueeze(-1)).max()
        assert float(err) < 1e-10, (name, T, w, float(err))


def test_oracle_bound_is_positive_and_padded_rows_are_excluded():
    case = ao.Case("peaked", 3, 65, 2, 8, 4, (65, 3, 0))
    inp, o = _prepared(case)
    assert bool((o.bound > 0).all()) and bool(torch.isfinite(o.bound).all())
    assert o.valid.sum(1).tolist() == [65, 3, 0]
    junk = torch.full_like(o.ref, 7.0)
    junk = torch.where(o.valid.unsqueeze(-1), o.ref, junk)
    assert ao.count_over(junk, o) == 0
    with pytest.raises(AssertionError, match="non-finite"):
        bad = junk.clone()
        bad[2, 5, 1] = float("nan")
        ao.assert_within(bad, o, case.D, "nan in a padded row")


# --------------------------------------------------------------------------- #
# the honest emulation passes everywhere
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("case", ao.MATRIX, ids=lambda c: c.id)
def test_honest_emulation_within_bound(case):
    inp, o = _prepared(case)
    got = emulate_kernel(inp.qkv, inp.rel_k, inp.rel_v, inp.lens, case.H,
                         case.w, case.scale)
    worst = ao.assert_within(got, o, case.D, f"emulation {case.id}")
    print(f"{case.id}: max |got-ref|/bound = {worst:.3f}")


def test_matrix_covers_what_it_claims():
    """Every DPAD class and head size, every time edge, every window, every
    length value, all regimes and probes: the matrix is what the GPU test
    runs, so its coverage is asserted here where it is cheap."""
    M = ao.MATRIX
    assert {c.D for c in M} >= {8, 24, 32, 40, 48, 64, 72, 96, 104, 128}
    assert {c.H for c in M} == {1, 2, 4}
    assert {c.T for c in M} >= {1, 3, 63, 64, 65, 127, 128, 129, 200}
    assert {c.w for c in M} == {0, 1, 4, 7}
    assert {c.regime for c in M} == set(ao.REGIMES + ao.PROBES)
    assert any(c.lens is None for c in M)
    for T, w in ((129, 4), (200, 4)):
        seen = {v for c in M if c.T == T and c.w == w and c.lens
                for v in c.lens}
        assert seen >= {T, T - 1, 65, 64, w, 1, 0, T + 5}
    for regime in ao.REGIMES:
        for D in (32, 48, 64, 96, 128):
            assert any(c.regime == regime and c.D == D for c in M)
    assert all(c.T <= 200 and c.B <= 3 for c in M)


# --------------------------------------------------------------------------- #
# mutants
# --------------------------------------------------------------------------- #
def _rejections(mutant, cases):
    out = []
    for case in cases:
        if mutant == "heads_swapped" and case.H < 2:
            continue
        inp, o = _prepared(case)
        got = emulate_kernel(inp.qkv, inp.rel_k, inp.rel_v, inp.lens, case.H,
                             case.w, case.scale, mutant=mutant)
        n = ao.count_over(got, o)
        if n > HANDFUL:
            out.append((case.id, n))
    return out


SHARP = [c for c in ao.MATRIX if c.regime in ("peaked", "planted")]


@pytest.mark.parametrize("mutant", [m for m in MUTANTS
                                    if m != "l_from_bf16_p"])
def test_mutant_is_rejected(mutant):
    cases = SHARP
    if mutant in ("seam_band_drop", "band_stale_max"):
        cases = [c for c in SHARP if c.T > 64]
    if mutant in ("mask_off_by_one", "masked_logit_zero"):
        cases = [c for c in cases if c.lens is not None]
    hit = _rejections(mutant, cases)
    print(f"{mutant}: rejected on {len(hit)} of {len(cases)} sharp cases; "
          f"first {hit[:3]}")
    assert hit, f"{mutant} passes the bound on every sharp matrix case"


def test_mutant_l_from_bf16_p_is_at_the_margin_of_the_bound():
    """Summing l from the bf16-rounded P (with unrounded band p) is NOT
    rejected, and the bound says why it cannot be.  l' = sum bf16(p_j) =
    l·(1+e) with |e| <= 2^-9 (a weighted mean of the individual relative
    roundings, usually far smaller), so every output element moves by at
    most 2^-9·|out| before its final rounding.  The bound carries
    2·2^-9·|ref| for the output rounding alone, so this defect adds at most
    half of the bound to an honest kernel's error: the ratio can reach 1.5
    at worst and the defect is no larger than a rounding the kernel is
    allowed to make.  On the PV part it even cancels part of the P rounding.

    Which way it went, measured over the whole matrix: accepted.  No case
    has more than a handful of elements over the bound; only the v = 0 probe
    at (T=129, H=4, D=32), where the band term stands alone and nothing
    cancels, shows any at all (9 of 24704, worst ratio 1.13)."""
    worst, most = 0.0, 0
    for case in ao.MATRIX:
        inp, o = _prepared(case)
        got = emulate_kernel(inp.qkv, inp.rel_k, inp.rel_v, inp.lens, case.H,
                             case.w, case.scale, mutant="l_from_bf16_p")
        honest = emulate_kernel(inp.qkv, inp.rel_k, inp.rel_v, inp.lens,
                                case.H, case.w, case.scale)
        # the derivation: nothing moves by more than 2^-9·|out| plus one
        # bf16 ulp (2^-7) where the final rounding lands elsewhere
        move = (got.to(F64) - honest.to(F64)).abs()
        lim = (2.0 ** -9 + 2.0 ** -7) * honest.to(F64).abs() + 1e-30
        assert bool((move <= lim)[o.valid].all()), case.id
        worst = max(worst, float(ao.ratio_to_bound(got, o).max()))
        most = max(most, ao.count_over(got, o))
    print(f"l_from_bf16_p: max |got-ref|/bound over the matrix = {worst:.3f},"
          f" at most {most} elements of a case over the bound")
    assert most <= HANDFUL
    assert worst <= 1.5


# --------------------------------------------------------------------------- #
# why the older tests stay smoke tests
# --------------------------------------------------------------------------- #
def _old_metric(got, ref):
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6))


def test_global_metric_accepts_broken_tables_the_bound_rejects_them():
    """(B,T,C,h) = (3,200,192,2), the seed, lengths and metric of
    test_gpu_ops.test_attn_relpos_kernel_parity, f32 module.  Measured:
    emb_rel_k zeroed 0.0115, emb_rel_v zeroed 0.0244, emb_rel_k flipped
    0.0206, emb_rel_v flipped 0.0219, emb_rel_v slot delta=+4 zeroed 0.0109
    - all under that test's 0.03, so a kernel that ignored or mirrored a
    table would pass it.  The per-element bound rejects every one."""
    from sonata_amd.models.vits import RelativeAttention

    B, T, C, h = 3, 200, 192, 2
    torch.manual_seed(100 + B + T)
    m = RelativeAttention(C, h).eval()
    lens = torch.full((B,), T, dtype=torch.long)
    lens[1:] = torch.randint(max(T // 2, 1), T + 1, (B - 1,))
    x = torch.randn(B, T, C)
    mask = (torch.arange(T).unsqueeze(0) < lens.unsqueeze(1)).float()
    x = x * mask.unsqueeze(-1)
    attn_mask = (mask.unsqueeze(2) * mask.unsqueeze(1)).unsqueeze(1)
    w = m.window_size

    def lin(t, *convs):
        return torch.nn.functional.linear(
            t, torch.cat([c.weight.squeeze(-1) for c in convs]),
            torch.cat([c.bias for c in convs]))

    with torch.no_grad():
        ref = m.forward_cl(x, attn_mask)
        qkv = lin(x, m.conv_q, m.conv_k, m.conv_v).to(BF)
    rk0, rv0 = m.emb_rel_k.detach().clone(), m.emb_rel_v.detach().clone()
    rv_slot = rv0.clone()
    rv_slot[0, 4 + w] = 0
    mutations = {
        "rel_k zeroed": (torch.zeros_like(rk0), rv0),
        "rel_v zeroed": (rk0, torch.zeros_like(rv0)),
        "rel_k flipped": (rk0.flip(1), rv0),
        "rel_v flipped": (rk0, rv0.flip(1)),
        "rel_v slot +4 zeroed": (rk0, rv_slot),
    }
    oracle = ao.attention_oracle(qkv, rk0[0].to(BF), rv0[0].to(BF), lens, h,
                                 w, m.head_dim ** -0.5)
    for name, (rk, rv) in mutations.items():
        with torch.no_grad():
            m.emb_rel_k.copy_(rk)
            m.emb_rel_v.copy_(rv)
            got = m.forward_cl(x, attn_mask)
        old = max(_old_metric(got[b, :ln], ref[b, :ln])
                  for b, ln in enumerate(lens.tolist()))
        broken = ao.attention_oracle(qkv, rk[0].to(BF), rv[0].to(BF), lens,
                                     h, w, m.head_dim ** -0.5).ref.to(BF)
        n = ao.count_over(broken, oracle)
        print(f"{name}: old metric {old:.4f} (< 0.03 passes), "
              f"{n} elements over the per-element bound")
        assert 0.002 < old < 0.03, (name, old)
        assert n > HANDFUL, (name, n)
    # and the unbroken tables, rounded like the kernel's output, pass
    assert ao.count_over(oracle.ref.to(BF), oracle) == 0
