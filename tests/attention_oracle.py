"""fp64 reference and derived per-element error bound for the fused
relative-position attention kernel (csrc/attention_cl.hip,
``attn_relpos_cl``), the input regimes that make the bound bite, and the
case matrix shared by the CPU and the GPU tests.

Reference (``attention_oracle``)
--------------------------------
Direct banded form on what the kernel is handed (qkv [B,T,3·H·D] bf16,
rel_k/rel_v [2w+1,D] bf16, lens, H, w, scale), all arithmetic in float64:

  scaled query   qs = bf16( f32(q) · f32(scale) ).  The ONE rounding the
                 reference mirrors: the kernel's Qs staging and the bf16
                 eager chain (``q * scale``) both perform it.
                 ``round_q=False`` switches it off for the comparison with
                 the float64 module.
  logits         key j, query t, δ = j − t:
                   s = qs·k_j + [|δ| ≤ w] · qs·rel_k[δ+w]
                 keys j ≥ min(lens[b], T) get exactly −1e4
  weights        a = softmax_j(s)
  output         out[t] = Σ_j a_j·v_j
                        + Σ_{|δ|≤w, 0≤t+δ<T} a_{t+δ} · rel_v[δ+w]

So slot = δ + w with δ = key − query.  Rows t ≥ lens[b] are reported in
``valid`` as False and are not compared: the kernel masks keys only, the
eager chain masks the whole row, and the encoder multiplies those rows by
zero.  They must be finite (a NaN survives a multiply by zero).

Error model
-----------
u32 = 2^-24 (f32 unit roundoff).  For query row t, per output element d:

  logit error    All operands are bf16, so each product is exact in f32 and
                 any f32 summation order over D terms, plus the add of the
                 band logit and of the band logit's own accumulation, errs
                 by at most
                   E_t = (D+2)·u32·max_j( Σ|qs||k_j| + band Σ|qs||rel_k| )
                 over live keys j.  Masked keys are exactly −1e4 on both
                 sides.  A uniform logit error of ≤ E perturbs every
                 normalised weight a_j by a relative 2·E (numerator and
                 denominator each move by e^{±E}).
  __expf         ε_t = max_j (min(|x_j|,104) + 4)·u32, x = s − m: the
                 rounding of the argument multiply by log2(e) (relative u32
                 on |x|·log2e) plus the hardware exp2 (a few ulp).  Below
                 x = −104 the f32 result is exactly 0 and the true weight is
                 < 1e-45.  ε is two orders of magnitude below the bf16 terms
                 (|x| ≲ 30 where weights matter ⇒ ε ≲ 2e-6 against 2e-3), so
                 its exact constant decides no outcome.
  row sum        (T+2)·u32 for the f32 sum of T non-negative terms, the
                 running rescale and the reciprocal.
  P rounding     P is rounded to bf16 before the PV MFMA while the row sum l
                 and the band term use the unrounded f32 p:
                 2^-9·Σ_j a_j|v_jd| on the PV part only.
  PV accumulate  T·u32·Σ_j a_j|v_jd|.
  band multiply  (2w+1)·u32·Σ a_band|rel_v| for the ≤ 2w+1 f32 FMAs.
  output         2^-9·|ref| for the final bf16 store.

With r = 2·E_t + 2·ε_t + (T+2)·u32 (every normalised weight's relative
error; numerator and denominator carry one ε each):

  bound = HEADROOM · [ (r + 2^-9)·Σa|v| + (r + (2w+1)·u32)·Σa_band|rel_v|
                       + T·u32·Σa|v| + 2^-9·|ref| + 1e-30 ]

HEADROOM = 2 is the single slack factor.  It is not fitted to the kernel:
it covers (a) the bf16 roundings at their worst, which is 2^-8 relative
just above a power of two against the 2^-9 carried above, (b) the running
rescale chain (each of the ≤ ceil(T/64)−1 later tiles multiplies l and accO
by the SAME f32 fscale, so its error cancels in PV/l and enters only the
band term, at ≤ ε per tile), and (c) second-order products of the terms.

Input regimes (``make_case``)
-----------------------------
  flat      the statistics of a default-initialised module on unit-normal
            input: q, k, v at std 3^-1/2, logits at std ≈ 0.3, tables at
            D^-1/2.  Production-like control; the softmax is almost uniform
            so the relative terms hardly move the output.
  peaked    q at std 4, k, v and both tables at std 1: logits at std ≈ 4,
            band logits move weights by O(1).
  planted   every query row gets one key, drawn uniformly from the live
            keys, whose logit is planted 12 above a flat background
            (q_t = noise + 12/scale · k_c/|k_c|²).  The cross-talk
            12·(k_j·k_c)/|k_c|² has std ≈ 12/√D, so the margin is ≈ 12 at
            D ≥ 48 and the row merely sharp at D = 8; either way the winner
            falls in the first, a middle and the last key tile and inside
            and outside the band, so the running max rises late for some
            rows and early for others.
  probe_v0    peaked with v = 0: the output is the rel-v band term alone.
  probe_relk  peaked with k = 0 and rel_v = 0: the scores are the rel-k band
              alone over a flat background.
"""

from __future__ import annotations

from typing import List, NamedTuple, Optional

import torch

U32 = 2.0 ** -24        # f32 unit roundoff
U_BF16 = 2.0 ** -9      # bf16 rounding carried by the model (see HEADROOM)
HEADROOM = 2.0          # the single headroom factor
MASKED_LOGIT = -1e4
EXP_CAP = 104.0         # exp(-104) is exactly 0 in f32
TINY = 1e-30

F64 = torch.float64
BF = torch.bfloat16

REGIMES = ("flat", "peaked", "planted")
PROBES = ("probe_v0", "probe_relk")


class AttnOracle(NamedTuple):
    ref: torch.Tensor     # fp64 [B, T, H*D], NOT rounded to bf16
    bound: torch.Tensor   # fp64 [B, T, H*D] allowed |got - ref|
    valid: torch.Tensor   # bool [B, T]: t < min(lens[b], T)


# --------------------------------------------------------------------------- #
# reference
# --------------------------------------------------------------------------- #
def split_heads(qkv: torch.Tensor, H: int):
    """qkv [B,T,3*H*D] -> q, k, v each [B,H,T,D] (same dtype)."""
    B, T, C3 = qkv.shape
    D = C3 // (3 * H)
    x = qkv.reshape(B, T, 3, H, D).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def live_lengths(lens, B: int, T: int) -> torch.Tensor:
    if lens is None:
        return torch.full((B,), T, dtype=torch.long)
    return torch.as_tensor(lens).detach().cpu().long().clamp(max=T)


def scaled_query(q: torch.Tensor, scale: float) -> torch.Tensor:
    """bf16( f32(q) * f32(scale) ) as fp64."""
    s32 = torch.tensor(scale, dtype=torch.float32)
    return (q.to(torch.float32) * s32).to(BF).to(F64)


def band_index(T: int, w: int):
    """delta = key - query [T,T], the in-band mask and the slot delta + w
    (clamped to a legal index outside the band)."""
    t = torch.arange(T)
    delta = t.unsqueeze(0) - t.unsqueeze(1)       # [t, j] = j - t
    inband = delta.abs() <= w
    slot = (delta + w).clamp(0, 2 * w)
    return delta, inband, slot


def _band_scatter(R: torch.Tensor, inband, slot) -> torch.Tensor:
    """R [B,H,T,2w+1] per-slot values -> [B,H,T,T], zero off the band."""
    B, H, T, _ = R.shape
    full = torch.gather(R, 3, slot.expand(B, H, T, T))
    return torch.where(inband, full, torch.zeros((), dtype=R.dtype))


def _band_gather(a: torch.Tensor, inband, slot, nslot: int) -> torch.Tensor:
    """a [B,H,T,T] -> [B,H,T,2w+1]: a[t, t+delta] per slot, 0 past the
    ends of the sequence."""
    B, H, T, _ = a.shape
    out = torch.zeros(B, H, T, nslot, dtype=a.dtype)
    out.scatter_add_(3, slot.expand(B, H, T, T),
                     torch.where(inband, a, torch.zeros((), dtype=a.dtype)))
    return out


def attention_oracle(qkv: torch.Tensor, rel_k: torch.Tensor,
                     rel_v: torch.Tensor, lens, H: int, w: int, scale: float,
                     round_q: bool = True) -> AttnOracle:
    """Reference, bound and valid mask as derived in the module docstring.
    qkv/rel_k/rel_v may be any float dtype (bf16 for the kernel, fp64 for
    the comparison with the module)."""
    qkv = qkv.detach().cpu()
    B, T, C3 = qkv.shape
    D = C3 // (3 * H)
    nslot = 2 * w + 1
    assert rel_k.shape == (nslot, D) and rel_v.shape == (nslot, D)
    q, k, v = split_heads(qkv, H)
    qs = scaled_query(q, scale) if round_q else q.to(F64) * scale
    k, v = k.to(F64), v.to(F64)
    rk, rv = rel_k.detach().cpu().to(F64), rel_v.detach().cpu().to(F64)
    L = live_lengths(lens, B, T)
    _, inband, slot = band_index(T, w)
    masked = (torch.arange(T).view(1, 1, 1, T) >= L.view(B, 1, 1, 1))
    valid = torch.arange(T).unsqueeze(0) < L.unsqueeze(1)

    s = qs @ k.transpose(-1, -2) + _band_scatter(qs @ rk.t(), inband, slot)
    s = torch.where(masked, torch.full((), MASKED_LOGIT, dtype=F64), s)
    m = s.max(dim=-1, keepdim=True).values
    a = torch.softmax(s, dim=-1)
    a_band = _band_gather(a, inband, slot, nslot)
    pv = a @ v
    ref = pv + a_band @ rv

    # ---- bound ----------------------------------------------------------- #
    mag = qs.abs() @ k.abs().transpose(-1, -2) \
        + _band_scatter(qs.abs() @ rk.abs().t(), inband, slot)
    mag = torch.where(masked, torch.zeros((), dtype=F64), mag)
    E = (D + 2) * U32 * mag.max(dim=-1, keepdim=True).values
    eps = ((s - m).abs().clamp(max=EXP_CAP) + 4.0).max(
        dim=-1, keepdim=True).values * U32
    r = 2 * E + 2 * eps + (T + 2) * U32
    av = a @ v.abs()
    bv = a_band @ rv.abs()
    bound = HEADROOM * ((r + U_BF16) * av + (r + nslot * U32) * bv
                        + T * U32 * av + U_BF16 * ref.abs() + TINY)

    def merge(x):   # [B,H,T,D] -> [B,T,H*D]
        return x.permute(0, 2, 1, 3).reshape(B, T, H * D)

    return AttnOracle(merge(ref), merge(bound), valid)


# --------------------------------------------------------------------------- #
# comparison
# --------------------------------------------------------------------------- #
SEAM_ROWS = ((60, 68), (124, 132))   # query rows astride the 64-key seams


def ratio_to_bound(got: torch.Tensor, oracle: AttnOracle) -> torch.Tensor:
    """|got - ref| / bound on valid rows, 0 elsewhere.  Non-finite values
    in `got` come back as inf."""
    g = got.detach().cpu().to(F64)
    ratio = (g - oracle.ref).abs() / oracle.bound
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    return torch.where(oracle.valid.unsqueeze(-1), ratio,
                       torch.zeros((), dtype=F64))


def count_over(got: torch.Tensor, oracle: AttnOracle) -> int:
    return int((ratio_to_bound(got, oracle) > 1.0).sum())


def _describe(ratio, got, oracle, rows, D, what):
    sub = ratio[:, rows[0]:rows[1]]
    if sub.numel() == 0 or not (sub > 1.0).any():
        return None
    flat = int(sub.argmax())
    b, t, c = (int(i) for i in
               torch.unravel_index(torch.tensor(flat), sub.shape))
    t += rows[0]
    return (f"{what}: {int((sub > 1.0).sum())} of "
            f"{int(oracle.valid[:, rows[0]:rows[1]].sum()) * sub.shape[2]} "
            f"valid elements out of bound; worst at batch {b}, query row {t} "
            f"(row {t % 64} of query tile {t // 64}), head {c // D}, d "
            f"{c % D}: got {float(got[b, t, c])!r}, ref "
            f"{float(oracle.ref[b, t, c])!r}, bound "
            f"{float(oracle.bound[b, t, c]):.3e}, ratio "
            f"{float(ratio[b, t, c]):.2f}")


def assert_within(got: torch.Tensor, oracle: AttnOracle, D: int,
                  what: str = "") -> float:
    """Every element of a valid row within its bound, every element of every
    row finite.  The rows astride the 64-key seams are asserted first and on
    their own so that a seam failure is named.  Returns the largest ratio."""
    g = got.detach().cpu().to(F64)
    assert g.shape == oracle.ref.shape, (what, tuple(g.shape))
    assert bool(torch.isfinite(g).all()), \
        f"{what}: {int((~torch.isfinite(g)).sum())} non-finite outputs " \
        f"(padded rows included)"
    ratio = ratio_to_bound(g, oracle)
    T = g.shape[1]
    for lo, hi in SEAM_ROWS:
        if lo < T:
            msg = _describe(ratio, g, oracle, (lo, min(hi, T)), D,
                            f"{what} SEAM rows {lo}..{hi - 1}")
            assert msg is None, msg
    msg = _describe(ratio, g, oracle, (0, T), D, what)
    assert msg is None, msg
    return float(ratio.max()) if ratio.numel() else 0.0


# --------------------------------------------------------------------------- #
# input regimes
# --------------------------------------------------------------------------- #
class Case(NamedTuple):
    regime: str
    B: int
    T: int
    H: int
    D: int
    w: int
    lens: Optional[tuple]     # None or B ints

    @property
    def id(self) -> str:
        ln = "none" if self.lens is None else "-".join(map(str, self.lens))
        return (f"{self.regime}-B{self.B}-T{self.T}-H{self.H}-D{self.D}"
                f"-w{self.w}-L{ln}")

    @property
    def scale(self) -> float:
        return self.D ** -0.5


class Inputs(NamedTuple):
    qkv: torch.Tensor        # [B,T,3*H*D] bf16
    rel_k: torch.Tensor      # [2w+1,D] bf16
    rel_v: torch.Tensor      # [2w+1,D] bf16
    lens: Optional[torch.Tensor]   # int32 [B] or None


def _generator(case: Case) -> torch.Generator:
    seed = 29
    for x in (REGIMES + PROBES).index(case.regime), case.B, case.T, case.H, \
            case.D, case.w, *(case.lens or (-1,)):
        seed = (seed * 1000003 + int(x) + 7) % (2 ** 31 - 1)
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def make_case(case: Case) -> Inputs:
    """Generate the bf16 inputs of one case; rows past lens[b] hold data of
    the same statistics (the kernel must ignore them as keys)."""
    g = _generator(case)
    B, T, H, D, w = case.B, case.T, case.H, case.D, case.w
    nslot = 2 * w + 1

    def rn(*shape):
        return torch.randn(*shape, generator=g, dtype=F64)

    regime = case.regime
    if regime == "flat":
        sd = 3.0 ** -0.5
        q, k, v = rn(B, H, T, D) * sd, rn(B, H, T, D) * sd, rn(B, H, T, D) * sd
        rk, rv = rn(nslot, D) * D ** -0.5, rn(nslot, D) * D ** -0.5
    elif regime in ("peaked",) + PROBES:
        q, k, v = rn(B, H, T, D) * 4.0, rn(B, H, T, D), rn(B, H, T, D)
        rk, rv = rn(nslot, D), rn(nslot, D)
        if regime == "probe_v0":
            v = torch.zeros_like(v)
        if regime == "probe_relk":
            k = torch.zeros_like(k)
            rv = torch.zeros_like(rv)
    elif regime == "planted":
        k, v = rn(B, H, T, D), rn(B, H, T, D)
        rk, rv = rn(nslot, D) * D ** -0.5, rn(nslot, D) * D ** -0.5
        L = live_lengths(case.lens, B, T).clamp(min=1)
        u = torch.rand(B, H, T, generator=g, dtype=F64)
        c = (u * L.view(B, 1, 1).to(F64)).long().clamp(max=T - 1)  # [B,H,T]
        kc = torch.gather(k, 2, c.unsqueeze(-1).expand(B, H, T, D))
        q = rn(B, H, T, D) * 3.0 ** -0.5 \
            + (12.0 / case.scale) * kc / (kc * kc).sum(-1, keepdim=True)
    else:
        raise ValueError(regime)
    qkv = torch.stack([q, k, v]).permute(1, 3, 0, 2, 4).reshape(
        B, T, 3 * H * D).to(torch.float32).to(BF).contiguous()
    lens = None if case.lens is None else torch.tensor(case.lens,
                                                       dtype=torch.int32)
    return Inputs(qkv, rk.to(torch.float32).to(BF).contiguous(),
                  rv.to(torch.float32).to(BF).contiguous(), lens)


def case_oracle(case: Case, inp: Inputs) -> AttnOracle:
    return attention_oracle(inp.qkv, inp.rel_k, inp.rel_v, inp.lens, case.H,
                            case.w, case.scale)


# --------------------------------------------------------------------------- #
# the case matrix (shared by the honest-emulation CPU test and the GPU test)
# --------------------------------------------------------------------------- #
def ragged(T: int, w: int, kind: int) -> tuple:
    """B = 3 lengths; the three kinds together cover
    {T, T-1, 65, 64, w, 1, 0, T+5}."""
    return ((T, 65, 0), (max(T - 1, 0), 64, 1), (w, T + 5, T))[kind]


def _matrix() -> List[Case]:
    cases: List[Case] = []

    def add(regime, T, H, D, w=4, lens="r0"):
        ln = None if lens is None else ragged(T, w, int(lens[1]))
        c = Case(regime, 1 if ln is None else 3, T, H, D, w, ln)
        if c not in cases:
            cases.append(c)

    # every head size of every DPAD instantiation, heads cycling 1/2/4
    for i, D in enumerate((8, 24, 32, 40, 48, 64, 72, 96, 104, 128)):
        add("peaked", 129, (1, 2, 4)[i % 3], D, lens=("r0", "r1", "r2")[i % 3])
    # time edges at the two shipped head shapes
    for T in (1, 3, 63, 64, 65, 127, 128, 129, 200):
        add("planted", T, 2, 96, lens=None)
        add("planted", T, 2, 48, lens="r1")
        add("peaked", T, 2, 96, lens="r2")
    # window: nslot 1 .. 15 of the 16 slots
    for w in (0, 1, 4, 7):
        add("peaked", 129, 2, 48, w=w, lens="r2")
        add("planted", 65, 2, 96, w=w, lens=None)
    # all three regimes at the shipped head shapes and one shape per DPAD
    for regime in REGIMES:
        for i, (H, D) in enumerate(((2, 96), (2, 48), (4, 32), (1, 64),
                                    (1, 128))):
            add(regime, 200, H, D, lens=("r0", "r1", "r2")[i % 3])
            add(regime, 129, H, D, lens=None)
    # isolating probes
    for probe in PROBES:
        add(probe, 129, 2, 96, lens="r0")
        add(probe, 129, 2, 48, lens=None)
        add(probe, 129, 4, 32, lens="r1")
    return cases


MATRIX: List[Case] = _matrix()
