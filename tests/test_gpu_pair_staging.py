"""LDS staging of the channel-last conv kernels with every load of a staging
group in flight at once (csrc/common.h: stage_w_window, stage_x_interior;
used by resblock_pair_cl_kernel, conv1d_cl_kernel's 128-column tile and
convt1d_cl_kernel).

Only when loads are issued and waited for differs from the kernels before
it, so the outputs keep their bits: a dozen seeded cases are pinned to
sha256 values recorded from a build of the preceding commit on an MI355X
(tests/golden/pair_staging_parent_sha256.json, written by
tools/record_pair_staging_sha.py; never regenerate them from the code under
test).  Every case is also held, element by element, to the fp64 oracle of
tests/kernel_oracle.py under its derived bound.

Shapes (inputs in tests/pair_staging_cases.py):

  tap-count dispatch   a staging window's tap count selects a compile-time
      instantiation.  C in {32, 64, 128, 256} x (k, d) in {(3,1), (5,2),
      (7,3), (9,1), (11,5)}: windows of TC=3 are 3 / 3+2 / 3+3+1 / 3+3+3 /
      3+3+3+2, TC=2 leaves a 1-tap window at every odd k, TC=1 has full
      windows only.  B = 3, T = 2*BM + 7, out_lens = [T, BM + 1, 0], with
      and without accum, out_scale 1/3, both weight layouts at C >= 64.
  idle staging waves and the guarded path   C = 16 (CP = 32: six of eight
      waves stage no weight rows; no K slice is channel-interior) and
      C = 40 (CP = 64, the second K slice is guarded; the wrapper keeps it
      on the fused kernel), T in {1, BM-1, BM, BM+1}.
  conv1d_cl / convt1d_cl   k in {1, 3, 5, 7, 11} at Cin in {24, 192}, Cout
      in {33, 130}; T = 257 has edge tiles only (except k = 1), T = 769 adds
      an interior tile, which is what the batched x staging needs.  Cin = 24
      has no channel-interior slice.  Transposed: stride 8 and 2 at
      Tin = 129 (edge tiles) and 385 (two interior tiles).
"""

import functools
import json
import os

import pytest
import torch

import kernel_oracle as ko
import pair_staging_cases as pc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "pair_staging_parent_sha256.json")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _pair_case(C, k, dil, B, T, lens, with_accum):
    """Inputs and oracle, built once and shared by the layouts."""
    inp = pc.pair_inputs(C, k, dil, B, T, None if lens is None else list(lens),
                         with_accum)
    oracle = ko.resblock_pair_oracle(inp["x"], inp["w1"], inp["b1"],
                                     inp["w2"], inp["b2"], dil, inp["lens"],
                                     inp["accum"], inp["scale"])
    return inp, oracle


def _check_pair(dev, C, k, dil, B, T, lens, with_accum, layouts):
    inp, oracle = _pair_case(C, k, dil, B, T,
                             None if lens is None else tuple(lens),
                             with_accum)
    BM = pc.xtr(C) - (k - 1)
    outs = []
    for layout in layouts:
        got = pc.run_pair(inp, dev, layout)
        again = pc.run_pair(inp, dev, layout)
        what = (f"pair C={C} k={k} d={dil} T={T} accum={with_accum} "
                f"layout={layout}")
        assert torch.equal(_bits(got), _bits(again)), f"{what}: runs differ"
        ko.assert_within(got, oracle, tile=BM, what=what)
        outs.append(got)
    # the layouts hold the same numbers: same products, same order
    for o in outs[1:]:
        assert torch.equal(_bits(o), _bits(outs[0])), \
            f"pair C={C} k={k} d={dil}: weight layouts differ"


@pytest.mark.parametrize("with_accum", [False, True])
@pytest.mark.parametrize("k,dil", [(3, 1), (5, 2), (7, 3), (9, 1), (11, 5)])
@pytest.mark.parametrize("C", [32, 64, 128, 256])
def test_tap_count_dispatch(dev, C, k, dil, with_accum):
    B, T, lens = pc.dispatch_shape(C, k)
    layouts = ("rows", "sliced") if C >= 64 else (None,)
    _check_pair(dev, C, k, dil, B, T, lens, with_accum, layouts)


@pytest.mark.parametrize("T_off", [None, -1, 0, 1])
@pytest.mark.parametrize("C,k,dil", [(16, 3, 1), (16, 11, 5), (40, 7, 3)])
def test_idle_waves_and_guarded_path(dev, C, k, dil, T_off):
    BM = pc.xtr(C) - (k - 1)
    T = 1 if T_off is None else BM + T_off
    _check_pair(dev, C, k, dil, 1, T, None, True, (None,))


@pytest.mark.parametrize("T", [257, 769])
@pytest.mark.parametrize("k", [1, 3, 5, 7, 11])
@pytest.mark.parametrize("Cout", [33, 130])
@pytest.mark.parametrize("Cin", [24, 192])
def test_conv1d_cl_staging(dev, Cin, Cout, k, T):
    inp = pc.conv_inputs(Cin, Cout, k, T)
    oracle = ko.conv_cl_oracle(inp["x"], inp["w"], inp["bias"], inp["pad"],
                               inp["dil"], inp["pre"], "none", 0.0,
                               inp["res"], inp["lens"])
    got = pc.run_conv(inp, dev)
    what = f"conv1d_cl Cin={Cin} Cout={Cout} k={k} T={T}"
    assert torch.equal(_bits(got), _bits(pc.run_conv(inp, dev))), \
        f"{what}: runs differ"
    ko.assert_within(got, oracle, tile=256, what=what)


@pytest.mark.parametrize("Tin", [129, 385])
@pytest.mark.parametrize("s", [8, 2])
@pytest.mark.parametrize("Cout", [33, 130])
@pytest.mark.parametrize("Cin", [24, 192])
def test_convt1d_cl_staging(dev, Cin, Cout, s, Tin):
    inp = pc.convt_inputs(Cin, Cout, s, Tin)
    oracle = ko.convt_cl_oracle(inp["x"], inp["w"], inp["bias"], s,
                                inp["pad"], inp["pre"], inp["lens"])
    got = pc.run_convt(inp, dev)
    what = f"convt1d_cl Cin={Cin} Cout={Cout} s={s} Tin={Tin}"
    assert torch.equal(_bits(got), _bits(pc.run_convt(inp, dev))), \
        f"{what}: runs differ"
    ko.assert_within(got, oracle, tile=128 * s, what=what)


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_the_cases():
    assert set(_golden()["sha256"]) == set(pc.SHA_CASES)


@pytest.mark.parametrize("name", sorted(pc.SHA_CASES))
def test_bits_match_parent_build(dev, name):
    got = pc.SHA_CASES[name](dev)
    again = pc.SHA_CASES[name](dev)
    assert torch.equal(_bits(got), _bits(again)), f"{name}: runs differ"
    assert pc.sha256_of(got) == _golden()["sha256"][name], (
        f"{name}: output bits differ from the build before the batched "
        f"staging")
