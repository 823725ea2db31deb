"""csrc/stream.hip and the batched-stream route on the GPU.

The kernels are compared bit for bit with the host oracle (stream_oracle.py:
slicing plus audio.samples.crossfade), and so is a whole stream_round against
the same inputs taken through ops.gather_windows, the voice's decode and the
host oracle.  Against the single-stream path only the project's bound for two
streaming routes of one sentence is claimed (max|a - b| / max|b| < 0.05, as
test_stream_graphed_matches_eager): a batch-of-one and a batch-of-R decode
may pick different tile variants."""

import threading

import numpy as np
import pytest
import torch

from sonata_amd import ops
from sonata_amd.audio.samples import to_i16
from stream_oracle import (SENTENCES, XF, run_gather_cases, run_seam_cases,
                           seam_oracle)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# --------------------------------- kernels ---------------------------------- #
def test_crossfade_constant_matches_the_kernel():
    from sonata_amd.models.voice import CROSSFADE_SAMPLES
    from sonata_amd.ops.functional import SEAM_CROSSFADE

    assert ops.hip_ext(required=True).SEAM_CROSSFADE == SEAM_CROSSFADE \
        == CROSSFADE_SAMPLES == XF


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [96, 192])
def test_gather_windows_bitwise(C, dtype):
    run_gather_cases(DEV, C, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_stream_seam_rows_bitwise(dtype):
    run_seam_cases(DEV, dtype)


def test_bindings_refuse_what_would_read_out_of_bounds():
    ext = ops.hip_ext(required=True)
    z = torch.zeros((1, 4, 10), device=DEV)
    with pytest.raises(RuntimeError, match="outside its source row"):
        ext.gather_windows([z], [0], [0], [3], [8], 8)
    wav = torch.zeros((1, 512), device=DEV)
    tails = torch.zeros((2, XF), device=DEV)
    ramp = torch.zeros(XF, device=DEV)
    with pytest.raises(RuntimeError, match="outside the row"):
        ext.stream_seam_rows(wav, [0], [500], [XF], [0], [0], tails, tails,
                             ramp, 504)
    with pytest.raises(RuntimeError, match="slot"):
        ext.stream_seam_rows(wav, [0], [400], [XF], [0], [2], tails, tails,
                             ramp, 400)


# ------------------------------- whole voice -------------------------------- #
@pytest.fixture(scope="module")
def voice_path(tmp_path_factory):
    from sonata_amd.models import create_random_voice

    return create_random_voice(str(tmp_path_factory.mktemp("stream_voice")),
                               "xlow_stream", quality="x_low")


@pytest.fixture(scope="module", params=["cpp", "python"])
def gpu_voice(request, voice_path):
    from sonata_amd.models import load_voice

    v = load_voice(voice_path, device=DEV, engine=request.param)
    assert (v._engine is not None) == (request.param == "cpp")
    return v


@pytest.fixture(scope="module")
def single(gpu_voice):
    return [list(gpu_voice.stream_synthesis(s, 45, 3)) for s in SENTENCES]


def _lens(chunks):
    return [len(c) for c in chunks]


def test_stream_round_is_gather_decode_oracle_bit_for_bit(gpu_voice):
    v = gpu_voice
    hop = v.net.arch.hop_length
    states = v.stream_open(SENTENCES, 45, 3)
    assert len({s.slot for s in states}) == len(states)
    host_tails = np.zeros((len(states), XF), dtype=np.float32)
    prev_ext = [0] * len(states)
    floats = [[] for _ in states]
    n_rounds = 0
    assert len([s for s in states if not s.done]) >= 3
    while any(not s.done for s in states):
        live = [s for s in states if not s.done]
        specs = [s.next_spec for s in live]
        length = [sp.mel_end - sp.mel_start for sp in specs]
        # the round's inputs once more, by hand
        z_c = ops.gather_windows([s.z for s in live], list(range(len(live))),
                                 [s.row for s in live],
                                 [sp.mel_start for sp in specs], length,
                                 max(length))
        for r, (s, sp) in enumerate(zip(live, specs)):
            assert torch.equal(z_c[r, :, : length[r]],
                               s.z[s.row, :, sp.mel_start : sp.mel_end])
        wav = v._decode_windows(z_c, length, None)
        rows = [(sp.trim_left_frames * hop,
                 (n - sp.trim_right_frames) * hop,
                 0 if sp.is_last else XF, prev_ext[s.index])
                for s, sp, n in zip(live, specs, length)]
        want, host_tails = seam_oracle(wav, rows, [s.index for s in live],
                                       host_tails)
        got = v.stream_round(states)
        assert [s for s, _ in got] == live
        for (s, chunk), w, row in zip(got, want, rows):
            assert chunk.dtype == np.float32
            np.testing.assert_array_equal(chunk.view(np.int32),
                                          w.view(np.int32))
            prev_ext[s.index] = row[2]
            floats[s.index].append(chunk)
        n_rounds += 1
    # streams left at different rounds, one of them after a single chunk
    assert n_rounds == max(len(f) for f in floats) >= 3
    assert min(len(f) for f in floats) == 1
    assert len(v._tail_free) == v._tails.shape[0]
    # pcm=True: the bytes of to_i16 of the float chunk
    got = [[] for _ in SENTENCES]
    for i, chunk in v.stream_synthesis_batch(SENTENCES, 45, 3, pcm=True):
        assert chunk.dtype == np.int16
        got[i].append(chunk)
    for g, f in zip(got, floats):
        assert _lens(g) == _lens(f)
        for a, b in zip(g, f):
            np.testing.assert_array_equal(a, to_i16(b))
    assert not v._infer_lock.locked()


def test_batched_streams_match_the_single_stream_path(gpu_voice, single):
    v = gpu_voice
    got = [[] for _ in SENTENCES]
    for i, chunk in v.stream_synthesis_batch(SENTENCES, 45, 3):
        got[i].append(chunk)
    ratios = []
    for g, w in zip(got, single):
        assert _lens(g) == _lens(w)
        a, b = np.concatenate(g), np.concatenate(w)
        assert np.isfinite(a).all()
        ratios.append(float(np.abs(a - b).max() / np.abs(b).max()))
    print("batched vs single stream, max|d|/max|single| per sentence:",
          ["%.3e" % r for r in ratios],
          "engine" if v._engine is not None else "python")
    assert max(ratios) < 0.05


def test_stream_batcher_on_the_gpu(gpu_voice, single):
    from sonata_amd.synth.batcher import StreamBatcher

    v = gpu_voice
    sb = StreamBatcher(v, max_streams=8, max_wait_ms=1.0)
    try:
        # eight streams; stream k opens when stream k-1 has its first chunk
        which = [3, 0, 1, 2, 3, 1, 0, 2]
        started = [threading.Event() for _ in which]
        results, errors = {}, []

        def consumer(k):
            try:
                if k:
                    assert started[k - 1].wait(60)
                it = sb.open(SENTENCES[which[k]], 45, 3)
                chunks = []
                for c in it:
                    chunks.append(c)
                    started[k].set()
                    if k == 4 and len(chunks) == 2:
                        it.close()  # abandoned midway
                        break
                results[k] = chunks
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
                started[k].set()

        threads = [threading.Thread(target=consumer, args=(k,))
                   for k in range(len(which))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(120)
        assert not errors, errors
        for k, i in enumerate(which):
            want = _lens(single[i])
            assert _lens(results[k]) == (want[:2] if k == 4 else want)
    finally:
        sb.close()
    assert not sb._worker.is_alive()
    assert not [t for t in threading.enumerate()
                if t.name == "sonata_stream_batcher"]
    assert len(v._tail_free) == v._tails.shape[0]
