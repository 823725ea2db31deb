"""The engine's dense, sync-free inverse spline (csrc/engine/vits_engine.cpp
rq_spline_inverse) against vits.rational_quadratic_spline(inverse=True) on
CPU f32, and the engine with and without SONATA_FUSED_FRONT on CPU.

Both sides run the same ATen operations in the same order, so the outputs
agree to f32 rounding; the bound is the atol=1e-4 test_engine.py uses for
the same pair of paths.  Elements outside [-5, 5] must pass through
bit for bit.
"""

import os

import pytest
import torch

from sonata_amd.models import create_random_voice
from sonata_amd.models.vits import rational_quadratic_spline
from sonata_amd.ops import hip_ext

B, T, BINS = 3, 17, 10


@pytest.fixture(scope="module")
def ext():
    e = hip_ext(required=False)
    if e is None or not hasattr(e, "rq_spline_inverse"):
        pytest.skip("HIP extension not built")
    return e


def _inputs():
    g = torch.Generator().manual_seed(5)
    z = torch.randn(B, 1, T, generator=g) * 2.5
    z[0, 0, 0] = 5.0          # exactly on the upper tail bound
    z[0, 0, 1] = -5.0         # exactly on the lower one
    z[0, 0, 2] = 7.25         # beyond
    z[0, 0, 3] = -6.5
    z[0, 0, 4] = 0.0
    z[1, 0, 5] = 5.0000005    # next f32 above 5
    z[2] = torch.linspace(5.5, 40.0, T) * torch.where(
        torch.arange(T) % 2 == 0, 1.0, -1.0)  # a row entirely outside
    uw = torch.randn(B, 1, T, BINS, generator=g)
    uh = torch.randn(B, 1, T, BINS, generator=g)
    ud = torch.randn(B, 1, T, BINS - 1, generator=g)
    return z, uw, uh, ud


def test_rq_spline_inverse_matches_python(ext):
    z, uw, uh, ud = _inputs()
    want, _ = rational_quadratic_spline(z, uw, uh, ud, inverse=True,
                                        tail_bound=5.0)
    got = ext.rq_spline_inverse(z, uw, uh, ud, 5.0)
    assert got.shape == z.shape and got.dtype == torch.float32
    diff = float((got - want).abs().max())
    print(f"rq_spline_inverse vs python: max abs diff {diff:.3e}")
    assert torch.isfinite(got).all()
    assert diff <= 1e-4
    outside = (z < -5.0) | (z > 5.0)
    assert bool(outside[2].all()) and int(outside.sum()) >= T + 3
    assert torch.equal(got[outside], z[outside])
    # inside elements moved (the spline is not the identity there)
    assert not torch.equal(got[~outside], z[~outside])


def test_rq_spline_inverse_all_outside(ext):
    """No element inside: the compacted form returned early here; the dense
    form must hand the inputs back untouched."""
    z, uw, uh, ud = _inputs()
    z = z.abs() + 5.5
    got = ext.rq_spline_inverse(z, uw, uh, ud, 5.0)
    assert torch.equal(got, z)


def test_engine_cpu_fused_front_equals_eager(ext, tmp_path):
    """CPU f32 engine: the dense spline (default) against the compacted
    one (SONATA_FUSED_FRONT=0), the knob read per call."""
    pack = create_random_voice(str(tmp_path), "ff_voice", quality="x_low")
    eng = ext.VitsEngine(pack, "cpu", "f32")
    rows = [eng.phonemes_to_ids(p) for p in
            ("wˈʌn.", "tˈuː θɹˈiː fˈoːɹ.", "hˈɛloʊ wˈɜːld tʊdˈeɪ.")]
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
    assert torch.equal(l0, l1)
    diff = float((a0 - a1).abs().max())
    print(f"cpu engine fused vs eager front end: max abs diff {diff:.3e}")
    assert diff <= 1e-4
