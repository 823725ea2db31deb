"""tests/decoder_oracle.py is right, and it would catch what it is for.

No GPU.  The shapes are those of tests/test_gpu_decoder_stages.py, case A
and B: B=3, F=24, lengths [24, 13, 5], `medium` and `x_low`, one speaker
and three.

Agreement     ``exact`` equals the channel-first fp64 ``Generator.forward``
              (the path test_engine_matches_python_exactly pins to the
              engine) to 1e-9 of the row maximum.
Consistency   the rounded chain passes its own teacher-forced check at every
              stage: shapes, masks, 42 stages for `medium`, unique names.
Mutations     a "recorded" trace is the rounded chain with the named stages
              computed by a mutant Stage and everything after teacher-forced
              from the wrong tensor, as it would be on the device.  The check
              must fail at exactly the mutated stages.  A mutation that is
              one slip in the code but changes two launches (swapped
              dilations, the 1/3 on the wrong resblock) mutates both, and
              both must fail.

The subtle mutation, +1 bf16 ulp on every tap of conv_post's weight, IS seen
by the derived bound at case A (`medium`, one speaker): 481 of the 10752
live output samples leave their bound, the worst by 1.2e-4 against a bound
of 9.0e-5.  The bound is about one bf16 ulp of the output; moving all 224
taps away from zero shifts the pre-tanh sum by 0.4-0.8 % of sum |x||w|,
which exceeds one ulp of the sum only where the taps cancel, hence the
4 %.  No doubling was needed.
"""

import dataclasses

import pytest
import torch

import decoder_oracle as do
import kernel_oracle as ko
from sonata_amd.models import create_random_voice, load_voice

BF = torch.bfloat16
FRAMES, LENGTHS = 24, [24, 13, 5]


class Case:
    def __init__(self, root, quality, speakers):
        path = create_random_voice(str(root), f"{quality}_{speakers}",
                                   quality=quality, num_speakers=speakers)
        self.voice = load_voice(path, device="cpu", engine="python")
        net = self.voice.net
        self.arch = net.arch
        self.state = {k: v.detach().clone()
                      for k, v in net.dec.state_dict().items()}
        self.lens = torch.tensor(LENGTHS)
        z, y_mask = do.make_input(self.arch, FRAMES, LENGTHS, seed=11)
        self.z = z * y_mask
        self.g = None
        if speakers > 1:
            sid = torch.arange(len(LENGTHS)) % speakers
            self.g = net.emb_g(sid).unsqueeze(-1).detach()
        self.stages = do.walk(self.arch, self.state, len(LENGTHS), self.lens,
                              self.g)
        self.by_name = {s.name: s for s in self.stages}
        self.memo = do.Memo()
        self.trace = do.chain(self.stages, self.z, memo=self.memo)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    root = tmp_path_factory.mktemp("decoder_oracle")
    made = {}

    def get(quality, speakers):
        if (quality, speakers) not in made:
            made[quality, speakers] = Case(root, quality, speakers)
        return made[quality, speakers]

    return get


# --------------------------------------------------------------------------- #
# agreement with the model
# --------------------------------------------------------------------------- #
def _model_fp64(case):
    """Generator(arch).double() on CPU holding the bf16-rounded
    parameters."""
    from sonata_amd.models.vits import Generator

    gen = Generator(case.arch,
                    gin_channels=case.arch.gin_channels
                    if case.g is not None else 0).double().eval()
    gen.load_state_dict({k: v.float().to(BF).double()
                         for k, v in case.state.items()})
    return gen


@pytest.mark.parametrize("speakers", [1, 3])
@pytest.mark.parametrize("quality", ["medium", "x_low"])
def test_exact_matches_channel_first_model(cases, quality, speakers):
    case = cases(quality, speakers)
    g64 = None if case.g is None else case.g.to(BF).double()
    with torch.no_grad():
        want = _model_fp64(case)(case.z.to(BF).double(), g64, case.lens)
    got = do.exact(case.arch, case.state, case.z, case.lens, case.g)
    assert got.shape == want.shape == (3, 1, FRAMES * case.arch.hop_length)
    for b in range(3):
        top = float(want[b].abs().max())
        assert top > 0
        err = float((got[b] - want[b]).abs().max())
        assert err <= 1e-9 * top, f"row {b}: {err:.3e} > 1e-9 * {top:.3e}"
    # a batch of one drops its lengths on both sides
    one = do.exact(case.arch, case.state, case.z[1:2], case.lens[1:2],
                   None if case.g is None else case.g[1:2])
    with torch.no_grad():
        want1 = _model_fp64(case)(case.z[1:2].to(BF).double(),
                                  None if g64 is None else g64[1:2],
                                  case.lens[1:2])
    assert float((one - want1).abs().max()) <= 1e-9 * float(want1.abs().max())


# --------------------------------------------------------------------------- #
# self-consistency
# --------------------------------------------------------------------------- #
def _expected_names(arch, with_g):
    names = ["conv_pre"] + (["cond.proj", "cond"] if with_g else [])
    nk = len(arch.resblock_kernel_sizes)
    for i in range(len(arch.upsample_rates)):
        names.append(f"ups.{i}")
        for j in range(nk):
            names += [f"resblocks.{i * nk + j}.pair{d}"
                      for d in arch.resblock_dilation_sizes[j]]
    return names + ["conv_post"]


@pytest.mark.parametrize("speakers", [1, 3])
@pytest.mark.parametrize("quality", ["medium", "x_low"])
def test_rounded_chain_is_self_consistent(cases, quality, speakers):
    case = cases(quality, speakers)
    names = [s.name for s in case.stages]
    assert names == _expected_names(case.arch, speakers > 1)
    assert len(set(names)) == len(names)
    launches = [s for s in case.stages if s.kind != "cond"]
    assert len(launches) - (speakers > 1) == 42  # 1 + 4*(1+9) + 1
    assert all(s.kind == "pair" for s in case.stages if ".pair" in s.name)
    assert do.check(case.stages, case.trace, case.memo) == {}
    # shapes, lengths and masks stage by stage
    T, ch, lens = FRAMES, case.arch.upsample_initial_channel, case.lens
    for st in case.stages:
        if st.kind == "proj":
            assert case.trace[st.name].shape == (3, ch, 1)
            continue
        if st.kind == "convt":
            r = st.p["stride"]
            T, ch, lens = T * r, ch // 2, lens * r
        C = 1 if st.name == "conv_post" else ch
        out = case.trace[st.name]
        assert out.shape == (3, T, C) and out.dtype == BF, st.name
        assert torch.equal(st.lens, lens), st.name
        for b, n in enumerate(lens.tolist()):
            assert not out[b, n:].any(), st.name
            assert out[b, :n].any(), st.name
    assert T == FRAMES * case.arch.hop_length


def test_plus_zero_check_sees_minus_zero():
    lens = torch.tensor([3, 1])
    x = torch.ones(2, 4, 5, dtype=BF)
    x[0, 3:] = 0.0
    x[1, 1:] = 0.0
    ko.assert_plus_zero(x, lens, "clean")
    ko.assert_plus_zero(x.transpose(1, 2), lens, "clean", time_dim=2)
    for bad in (-0.0, 2.0 ** -130):
        y = x.clone()
        y[1, 2, 4] = bad
        with pytest.raises(AssertionError, match=r"\(1, 2, 4\)"):
            ko.assert_plus_zero(y, lens, "leak")
        with pytest.raises(AssertionError, match="not \\+0"):
            ko.assert_plus_zero(y.transpose(1, 2), lens, "leak", time_dim=2)


def test_batch_of_one_drops_lengths(cases):
    case = cases("x_low", 1)
    stages = do.walk(case.arch, case.state, 1, case.lens[1:2])
    assert all(s.lens is None for s in stages)


def test_unfused_pairs_are_two_launches():
    """Channel counts that do not pad to a square weight (96 -> 128x96) and
    halos past 52 run as two convs plus the eager MRF arithmetic."""
    from sonata_amd.models.config import VitsArchitecture
    from sonata_amd.models.vits import Generator

    assert do.pair_is_fused(16, 11, 5) and do.pair_is_fused(256, 11, 5)
    assert not do.pair_is_fused(96, 3, 1)       # 128 x 96
    assert not do.pair_is_fused(64, 11, 6)      # halo 60
    assert do.pair_is_fused(48, 3, 1)           # 64 x 64
    arch = VitsArchitecture(
        inter_channels=32, upsample_initial_channel=192,
        upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4],
        resblock_kernel_sizes=[3, 11],
        resblock_dilation_sizes=[[1, 3], [1, 6]])
    torch.manual_seed(3)
    gen = Generator(arch)
    state = {k: v.detach().clone() for k, v in gen.state_dict().items()}
    lens = torch.tensor([9, 4])
    z, y_mask = do.make_input(arch, 9, lens, seed=2)
    stages = do.walk(arch, state, 2, lens)
    names = [s.name for s in stages]
    # stage 0 has 96 channels: every pair unfused; stage 1 has 48: only the
    # halo-60 pair is
    assert names == [
        "conv_pre", "ups.0",
        "resblocks.0.pair1.conv1", "resblocks.0.pair1.conv2",
        "resblocks.0.pair3.conv1", "resblocks.0.pair3.conv2",
        "resblocks.1.pair1.conv1", "resblocks.1.pair1.conv2",
        "resblocks.1.pair6.conv1", "resblocks.1.pair6.conv2",
        "resblocks.1.pair6.mrf",
        "ups.1", "resblocks.2.pair1", "resblocks.2.pair3",
        "resblocks.3.pair1",
        "resblocks.3.pair6.conv1", "resblocks.3.pair6.conv2",
        "resblocks.3.pair6.mrf", "conv_post"]
    memo = do.Memo()
    trace = do.chain(stages, z * y_mask, memo=memo)
    assert do.check(stages, trace, memo) == {}
    gen64 = Generator(arch).double().eval()
    gen64.load_state_dict({k: v.to(BF).double() for k, v in state.items()})
    with torch.no_grad():
        want = gen64((z * y_mask).double(), None, lens)
    got = do.exact(arch, state, z * y_mask, lens)
    assert float((got - want).abs().max()) <= 1e-9 * float(want.abs().max())


# --------------------------------------------------------------------------- #
# mutations
# --------------------------------------------------------------------------- #
def _mutated(case, mutants):
    """Failures of the trace in which `mutants` {name: Stage} replace the
    walk's stages and the rest is teacher-forced."""
    memo = do.Memo(case.memo)
    trace = do.chain(case.stages, case.z, replace=mutants, memo=memo)
    return do.check(case.stages, trace, memo)


def _mut(case, name, *, p=None, **fields):
    st = case.by_name[name]
    if p is not None:
        fields["p"] = {**st.p, **p}
    return dataclasses.replace(st, **fields)


def test_mutation_swapped_dilations(cases):
    case = cases("medium", 1)
    a, b = "resblocks.10.pair3", "resblocks.10.pair5"
    failed = _mutated(case, {a: _mut(case, a, p=dict(dilation=5)),
                             b: _mut(case, b, p=dict(dilation=3))})
    assert sorted(failed) == [a, b], failed


def test_mutation_accum_dropped(cases):
    case = cases("medium", 1)
    name = "resblocks.1.pair5"
    st = case.by_name[name]
    assert st.srcs == ("resblocks.1.pair3", "resblocks.0.pair5")
    failed = _mutated(case, {name: _mut(case, name, srcs=st.srcs[:1])})
    assert list(failed) == [name], failed


def test_mutation_scale_on_wrong_resblock(cases):
    case = cases("medium", 1)
    a, b = "resblocks.1.pair5", "resblocks.2.pair5"
    assert case.by_name[a].p["scale"] == 1.0
    assert case.by_name[b].p["scale"] == 1.0 / 3
    failed = _mutated(case, {a: _mut(case, a, p=dict(scale=1.0 / 3)),
                             b: _mut(case, b, p=dict(scale=1.0))})
    assert sorted(failed) == [a, b], failed


def test_mutation_lengths_not_multiplied(cases):
    case = cases("medium", 1)
    name = "ups.2"
    before = case.by_name["ups.1"].lens
    assert torch.equal(case.by_name[name].lens, before * 2)
    failed = _mutated(case, {name: _mut(case, name, lens=before)})
    assert list(failed) == [name], failed
    assert "out of bound" in failed[name]


def test_mutation_lengths_one_too_long(cases):
    case = cases("medium", 1)
    name = "ups.2"
    longer = case.by_name[name].lens + 1
    failed = _mutated(case, {name: _mut(case, name, lens=longer)})
    assert list(failed) == [name], failed
    assert "masked row not exactly zero" in failed[name]


def test_mutation_convs_swapped_in_one_pair(cases):
    """resblocks.4 (k=7) and resblocks.5 (k=11) cannot trade weights, so
    convs1 and convs2 trade places inside the dilation-1 pair, where the
    weights are the only thing that differs."""
    case = cases("medium", 1)
    assert case.by_name["resblocks.4.pair1"].p["w1"].shape != \
        case.by_name["resblocks.5.pair1"].p["w1"].shape
    name = "resblocks.4.pair1"
    p = case.by_name[name].p
    failed = _mutated(case, {name: _mut(case, name, p=dict(
        w1=p["w2"], b1=p["b2"], w2=p["w1"], b2=p["b1"]))})
    assert list(failed) == [name], failed


def test_mutation_convt_tap_shifted(cases):
    """Phase r tap m reads W[:, :, r + s*m]; here (r, m) = (0, 1) of ups.3
    (s = 2, k = 4) reads the tap of residue r + 1."""
    case = cases("medium", 1)
    name = "ups.3"
    st = case.by_name[name]
    s, r, m = st.p["stride"], 0, 1
    assert (s, st.p["w"].shape[2]) == (2, 4)
    w = st.p["w"].clone()
    w[:, :, r + s * m] = st.p["w"][:, :, r + 1 + s * m]
    failed = _mutated(case, {name: _mut(case, name, p=dict(w=w))})
    assert list(failed) == [name], failed


def test_mutation_cond_not_remasked(cases):
    case = cases("medium", 3)
    failed = _mutated(case, {"cond": _mut(case, "cond", lens=None)})
    assert list(failed) == ["cond"], failed
    assert "masked row not exactly zero" in failed["cond"]


def test_mutation_cond_projection_of_wrong_speaker(cases):
    case = cases("medium", 3)
    st = case.by_name["cond.proj"]
    failed = _mutated(case, {"cond.proj": _mut(
        case, "cond.proj", p=dict(g=st.p["g"].roll(1, 0)))})
    assert list(failed) == ["cond.proj"], failed


def _ulp_up(w):
    """Every element one bf16 ulp further from zero."""
    return (w.view(torch.int16) + 1).view(BF)


def test_mutation_conv_post_one_ulp(cases):
    """The subtle one; see the module docstring for what it measures."""
    case = cases("medium", 1)
    w = case.by_name["conv_post"].p["w"]
    up = _ulp_up(w)
    rel = ((up.double() - w.double()) / w.double()).abs()
    assert float(rel.min()) >= 2.0 ** -8 and float(rel.max()) <= 2.0 ** -7
    failed = _mutated(case, {"conv_post": _mut(case, "conv_post",
                                               p=dict(w=up))})
    assert list(failed) == ["conv_post"], failed
    print(failed["conv_post"])
