"""The sliced weight layout of the resblock pair kernel, on the CPU.

csrc/resblock_cl.hip stages one (tap, 32-channel K slice c0) window at a
time and reads element (row n, column j of the window) at

    rows    [k][CP][CP]         tap*CP*CP + c0        + n*CP + j
    sliced  [k][CP/32][CP][32]  tap*CP*CP + c0*CP     + n*32 + j

(wpitch / wkstep in the kernel).  Reading the sliced tensor through the
second formula must give back the rows tensor, element for element.
"""

import pytest
import torch

from sonata_amd.ops.functional import _slice_weight_windows


@pytest.mark.parametrize("CP", [64, 128, 256])
@pytest.mark.parametrize("k", [3, 11])
def test_sliced_index_formula_reproduces_rows(CP, k):
    # distinct values, all exact in bf16's 8-bit significand pattern space:
    # compare raw int16 patterns instead of floats
    n_el = k * CP * CP
    rows = (torch.arange(n_el, dtype=torch.int64) % 65521).to(torch.int16) \
        .view(k, CP, CP).view(torch.bfloat16)
    sliced = _slice_weight_windows(rows)
    assert sliced.shape == (k, CP // 32, CP, 32)
    assert sliced.is_contiguous()
    flat = sliced.view(torch.int16).reshape(-1)

    tap = torch.arange(k).view(k, 1, 1)
    n = torch.arange(CP).view(1, CP, 1)
    ci = torch.arange(CP).view(1, 1, CP)
    c0, j = (ci // 32) * 32, ci % 32
    wpitch, wkstep = 32, CP
    idx = tap * CP * CP + c0 * wkstep + n * wpitch + j
    assert int(idx.max()) == n_el - 1 and idx.unique().numel() == n_el
    back = flat[idx.reshape(-1)].view(k, CP, CP)
    assert torch.equal(back, rows.view(torch.int16))
    # every window is one contiguous block of CP*32 elements
    first = tap * CP * CP + c0 * wkstep
    assert torch.equal(idx - first, (n * 32 + j).expand_as(idx))


def test_sliced_weight_is_cached_on_the_parameter():
    from sonata_amd.ops.functional import (_conv_weight_mfma,
                                           _conv_weight_sliced)

    w = torch.randn(64, 64, 3)
    s1 = _conv_weight_sliced(w)
    assert _conv_weight_sliced(w) is s1
    perm = _conv_weight_mfma(w)
    assert torch.equal(s1.permute(0, 2, 1, 3).reshape(perm.shape), perm)
