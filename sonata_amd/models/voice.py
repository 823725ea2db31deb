"""VitsVoice: a loaded voice pack implementing the SonataModel interface.

Parity: reference crates/sonata/models/piper/src/lib.rs —
`from_config_path` (:88-110), `VitsModel`/`VitsStreamingModel` (:291,480),
trait `VitsModelCommons` (:168-289: phonemize, id-encode, speaker maps,
fallback synthesis config), `SpeechStreamer` chunked decoding with
42-sample crossfade (:765-858).

Voice-pack format: `<name>.json` (Piper-compatible config schema) +
`<name>.safetensors` (weights).  A real Piper `.onnx` voice can be
converted via sonata_amd.models.onnx_import (weights-only importer).
"""

from __future__ import annotations

import math
import os
import threading
import time
from typing import Dict, Iterator, List, Optional, Sequence

import numpy as np
import torch

from ..audio.samples import crossfade, silence_samples
from ..utils.trace import stage_timer
from ..core import (Audio, AudioInfo, ModelError, PcmAudio, Phonemes,
                    SonataModel)
from ..text.ids import phonemes_to_ids
from ..text.phonemizer import text_to_phonemes
from .chunker import chunk_plan
from .config import ModelConfig, SynthesisConfig
from .vits import VitsModel

CROSSFADE_SAMPLES = 42  # reference: piper/src/lib.rs:838


def _utterance_seed(phonemes: str, sid: Optional[int]) -> int:
    """Deterministic per-utterance seed: same text -> same audio on any
    rank (SURVEY.md §7 hard part 7: seed per utterance, not per rank)."""
    import hashlib

    h = hashlib.sha256(
        (phonemes + "|" + str(sid if sid is not None else -1)).encode("utf-8")
    ).digest()
    return int.from_bytes(h[:8], "little") & 0x7FFFFFFFFFFFFFFF


class VitsVoice(SonataModel):
    def __init__(
        self,
        config: ModelConfig,
        net: VitsModel,
        device: str = "cpu",
        dtype: torch.dtype = torch.float32,
        engine=None,
    ):
        self.config = config
        self.net = net.eval().to(device=device, dtype=dtype)
        self.device = torch.device(device)
        self.dtype = dtype
        # optional C++ VitsEngine runtime (csrc/engine): when attached,
        # speak_batch/stream_synthesis execute through it (same kernels,
        # same per-utterance seeds -> identical audio; no Python in the
        # graph loop).  NOTE: the engine holds its own weight copy — it
        # attaches at load time, after which parallel.broadcast_module
        # only affects self.net (ranks load identical packs anyway).
        self._engine = engine
        self._synth_config = config.default_synthesis_config()
        self._cfg_lock = threading.Lock()
        # Serializes GPU inference on THIS voice: the hipGraph caches
        # (capture + replay via shared capture buffers), the pinned
        # staging buffers of the stream pipeline, and the C++ engine's
        # lazily-built weight cache are all per-voice mutable state.
        # Concurrent callers on one voice otherwise race (a 4-minute
        # mixed-load soak surfaced rare hipErrorInvalidConfiguration).
        # Cross-voice concurrency is unaffected; the gRPC batcher
        # already funnels per-voice work through one thread.
        self._infer_lock = threading.Lock()
        # batched streams (stream_open / stream_round): one kept crossfade
        # tail per live stream, [S, CROSSFADE_SAMPLES] f32 on the device
        self._tail_lock = threading.Lock()
        self._tail_free: List[int] = []
        self._tails: Optional[torch.Tensor] = None
        self._ramp: Optional[torch.Tensor] = None
        # device state of continuous stream prosody (ops.ProsodyStreamState),
        # indexed by tail slot; allocated with the first stream that asks
        self._prosody_state = None
        # ops.PolyStreamState per output sample rate streams were opened at
        self._poly_states: Dict[int, object] = {}
        self._tashkeel = None
        if config.espeak_voice.startswith("ar"):
            from ..text.tashkeel import TashkeelModel

            self._tashkeel = TashkeelModel.default(device="cpu")

    # ------------------------------------------------------------------ #
    # SonataModel interface
    # ------------------------------------------------------------------ #
    def audio_output_info(self) -> AudioInfo:
        return AudioInfo(sample_rate=self.config.sample_rate)

    @property
    def language(self) -> Optional[str]:
        return self.config.language_code

    def get_speakers(self) -> Optional[Dict[int, str]]:
        if self.config.num_speakers <= 1:
            return None
        return {v: k for k, v in self.config.speaker_id_map.items()}

    def get_synthesis_config(self) -> SynthesisConfig:
        with self._cfg_lock:
            return self._synth_config.copy()

    def set_synthesis_config(self, config: SynthesisConfig) -> None:
        with self._cfg_lock:
            self._synth_config = config.copy()

    def phonemize_text(self, text: str) -> Phonemes:
        with stage_timer("phonemize"):
            if self._tashkeel is not None:
                text = self._tashkeel.diacritize(text)
            sentences = text_to_phonemes(text, voice=self.config.espeak_voice)
            return Phonemes(sentences)

    # ------------------------------------------------------------------ #
    # inference
    # ------------------------------------------------------------------ #
    def _encode_ids(self, phonemes: str) -> List[int]:
        return phonemes_to_ids(phonemes, self.config.phoneme_id_map)

    def _generators(
        self, phonemes_batch: Sequence[str], sid: Optional[int]
    ) -> List[torch.Generator]:
        """One deterministic generator per utterance — same text gives the
        same audio regardless of batch composition or rank."""
        gens = []
        for p in phonemes_batch:
            gen = torch.Generator(device=self.device)
            gen.manual_seed(_utterance_seed(p, sid))
            gens.append(gen)
        return gens

    def _sid_tensor(self, batch: int, sid: Optional[int]):
        if self.config.num_speakers <= 1:
            return None
        s = sid if sid is not None else 0
        return torch.full((batch,), s, dtype=torch.long, device=self.device)

    @property
    def supports_row_synthesis(self) -> bool:
        """speak_batch / speak_batch_pcm / stream_open / stream_synthesis*
        take synthesis=: a SynthesisConfig (speaker and the three scales)
        per row, all rows in one padded batch."""
        return True

    def check_synthesis_config(self, cfg: SynthesisConfig) -> None:
        """Raise ValueError for a config no request may carry.  Run on the
        host before any tensor is built: an out-of-range speaker would be
        an out-of-range embedding index on the device."""
        n = self.config.num_speakers
        sid = cfg.speaker_id
        if n > 1 and sid is not None:
            if isinstance(sid, bool) or not isinstance(sid, (int, np.integer)):
                raise ValueError(f"speaker_id {sid!r} is not an integer")
            if not 0 <= int(sid) < n:
                raise ValueError(
                    f"speaker_id {sid} is outside [0, {n}) for this voice")
        for name, lo_open in (("length_scale", True), ("noise_scale", False),
                              ("noise_w", False)):
            v = getattr(cfg, name)
            try:
                v = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"{name} {v!r} is not a number") from None
            if not math.isfinite(v):
                raise ValueError(f"{name} must be finite, got {v}")
            if v < 0 or (lo_open and v == 0):
                raise ValueError(
                    f"{name} must be {'> 0' if lo_open else '>= 0'}, got {v}")

    def _resolve_synthesis(self, synthesis, B: int):
        """(cfg, rows) for a batch of B.  rows is None when one config holds
        for every row (synthesis=None, or rows that resolve to the same four
        values): the batch then runs through the scalar entry with cfg,
        exactly as without synthesis=.  Otherwise rows is one validated
        SynthesisConfig per row, None entries filled with the voice's."""
        base = self.get_synthesis_config()
        if synthesis is None:
            return base, None
        if isinstance(synthesis, SynthesisConfig):
            synthesis = [synthesis] * B
        if len(synthesis) != B:
            raise ValueError("one SynthesisConfig (or None) per row")
        rows = []
        for s in synthesis:
            if s is None:
                rows.append(base)
                continue
            self.check_synthesis_config(s)
            rows.append(s.copy())
        if not rows:
            return base, None
        key = lambda c: (c.speaker_id, float(c.noise_scale),  # noqa: E731
                         float(c.length_scale), float(c.noise_w))
        if all(key(r) == key(rows[0]) for r in rows[1:]):
            return rows[0], None
        return base, rows

    def _encoder_rows(self, phonemes_batch, ids, lengths, rows, decode: bool):
        """One batch with a speaker and three scales per row.  Row b's seed
        is _utterance_seed(phonemes, rows[b].speaker_id): the audio a row
        gets is the audio of that sentence alone with its config set
        voice-wide.  decode=True runs the whole graph (audio, lengths);
        False stops at the latent (z, y_mask, g)."""
        B = len(rows)
        sid_t = None
        if self.config.num_speakers > 1:
            sid_t = torch.tensor(
                [int(r.speaker_id) if r.speaker_id is not None else 0
                 for r in rows], dtype=torch.long, device=self.device)
        ns = [float(r.noise_scale) for r in rows]
        ls = [float(r.length_scale) for r in rows]
        nw = [float(r.noise_w) for r in rows]
        if self._engine is not None:
            seeds = [_utterance_seed(p, r.speaker_id)
                     for p, r in zip(phonemes_batch, rows)]
            fn = (self._engine.infer_rows if decode
                  else self._engine.infer_encoder_rows)
            return fn(ids, lengths, sid_t, ns, ls, nw, seeds)
        gens = []
        for p, r in zip(phonemes_batch, rows):
            gens.extend(self._generators([p], r.speaker_id))
        f32 = dict(dtype=torch.float32, device=self.device)
        fn = self.net.infer if decode else self.net.infer_encoder
        return fn(ids, lengths, sid=sid_t,
                  noise_scale=torch.tensor(ns, **f32),
                  length_scale=torch.tensor(ls, **f32),
                  noise_w=torch.tensor(nw, **f32), generators=gens)

    @torch.no_grad()
    def speak_one_sentence(self, phonemes: str) -> Audio:
        return self.speak_batch([phonemes])[0]

    @property
    def supports_device_prosody(self) -> bool:
        """speak_batch(prosody=...) applies rate / volume / pitch to the
        batch on the model's device, before the copy to the host."""
        return True

    def _prosody_rows(self, audio, audio_lengths, prosody):
        """Per-row (speed, volume, pitch) on the [B, 1, T] decoder output;
        rows given as None are left as they are."""
        from ..ops import apply_prosody_rows

        rows = [p if p is not None else (1.0, 1.0, 1.0) for p in prosody]
        assert len(rows) == audio.shape[0], "one prosody triple per row"
        y, out_lengths = apply_prosody_rows(
            audio.float()[:, 0, :], audio_lengths, self.config.sample_rate,
            speed=[r[0] for r in rows], volume=[r[1] for r in rows],
            pitch=[r[2] for r in rows])
        return y.unsqueeze(1), out_lengths

    @torch.no_grad()
    def _infer_batch(self, phonemes_batch: Sequence[str], synthesis=None):
        """Id-encode and run one padded batch.  Returns the decoder output
        [B, 1, T] and per-row lengths, both on the model's device, and the
        wall time of the inference in ms."""
        cfg, rows = self._resolve_synthesis(synthesis, len(phonemes_batch))
        id_lists = [self._encode_ids(p) for p in phonemes_batch]
        B = len(id_lists)
        T = max((len(i) for i in id_lists), default=1)
        ids = torch.zeros((B, T), dtype=torch.long)
        lengths = torch.zeros((B,), dtype=torch.long)
        for b, il in enumerate(id_lists):
            ids[b, : len(il)] = torch.tensor(il, dtype=torch.long)
            lengths[b] = len(il)
        ids = ids.to(self.device)
        lengths = lengths.to(self.device)
        if rows is not None:
            t0 = time.perf_counter()
            with self._infer_lock, stage_timer("infer", self.device):
                audio, audio_lengths = self._encoder_rows(
                    phonemes_batch, ids, lengths, rows, decode=True)
                if self.device.type == "cuda":
                    torch.cuda.synchronize(self.device)
            infer_ms = (time.perf_counter() - t0) * 1000.0
            return audio, audio_lengths, infer_ms
        gens = self._generators(phonemes_batch, cfg.speaker_id)

        t0 = time.perf_counter()
        if self._engine is not None:
            seeds = [_utterance_seed(p, cfg.speaker_id)
                     for p in phonemes_batch]
            sid_t = self._sid_tensor(B, cfg.speaker_id)
            with self._infer_lock, stage_timer("infer", self.device):
                audio, audio_lengths = self._engine.infer(
                    ids, lengths, sid_t, cfg.noise_scale, cfg.length_scale,
                    cfg.noise_w, seeds)
                if self.device.type == "cuda":
                    torch.cuda.synchronize(self.device)
            infer_ms = (time.perf_counter() - t0) * 1000.0
            return audio, audio_lengths, infer_ms
        with self._infer_lock, stage_timer("infer", self.device):
            audio, audio_lengths = self.net.infer(
            ids,
            lengths,
            sid=self._sid_tensor(B, cfg.speaker_id),
            noise_scale=cfg.noise_scale,
            length_scale=cfg.length_scale,
            noise_w=cfg.noise_w,
            generators=gens,
            )
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        infer_ms = (time.perf_counter() - t0) * 1000.0
        return audio, audio_lengths, infer_ms

    @property
    def supports_output_rate(self) -> bool:
        """speak_batch / speak_batch_pcm take sample_rate= and convert each
        row to its rate on the model's device (ops.resample_rows)."""
        return True

    def _row_rates(self, sample_rate, B: int) -> List[int]:
        """One output rate per row (None: the voice's own), each checked
        against the filter's limits."""
        from ..audio.resample import check_rate, is_identity

        native = self.config.sample_rate
        if sample_rate is None or isinstance(sample_rate, int):
            sample_rate = [sample_rate] * B
        assert len(sample_rate) == B, "one sample rate per row"
        rates = []
        for r in sample_rate:
            if is_identity(native, r):
                rates.append(native)
            else:
                check_rate(native, r)
                rates.append(int(r))
        return rates

    def _resample_groups(self, audio2d, audio_lengths, rates):
        """ops.resample_rows once per distinct rate, on that rate's rows.
        Yields (rate, row indices, y [b, n], out_lengths); rows at the
        voice's own rate pass through untouched."""
        from ..ops import resample_rows

        lens = [int(n) for n in audio_lengths.tolist()]
        for rate in sorted(set(rates)):
            idx = [b for b, r in enumerate(rates) if r == rate]
            if len(idx) == len(rates):
                rows, rl = audio2d, lens
            else:
                sel = torch.tensor(idx, dtype=torch.long,
                                   device=audio2d.device)
                rl = [lens[b] for b in idx]
                rows = audio2d.index_select(0, sel)[:, : max(rl, default=0)]
            y, out_lengths = resample_rows(
                rows, rl, self.config.sample_rate, rate)
            yield rate, idx, y, out_lengths

    @torch.no_grad()
    def speak_batch(self, phonemes_batch: Sequence[str],
                    prosody=None, sample_rate=None,
                    synthesis=None) -> List[Audio]:
        """True padded [B, T] batching (the reference loops batch=1:
        piper/src/lib.rs:425-437 — batching is a headline improvement).

        `prosody`: optional per-row sequence of (speed, volume, pitch) or
        None; applied on the device tensor before the single host copy.
        `sample_rate`: optional output rate, one int or one int-or-None per
        row; each distinct rate is converted on the device after prosody
        (ops.resample_rows) and copied on its own.
        `synthesis`: optional per-row sequence of SynthesisConfig or None
        (None: the voice's config when the call runs).  Rows with different
        speakers or scales share the one batch; each row is rendered as it
        would be alone with its config set voice-wide."""
        audio, audio_lengths, infer_ms = self._infer_batch(
            phonemes_batch, synthesis)
        B = len(phonemes_batch)
        info = self.audio_output_info()
        out: List[Audio] = []
        if prosody is not None:
            audio, audio_lengths = self._prosody_rows(
                audio, audio_lengths, prosody)
        rates = self._row_rates(sample_rate, B)
        if any(r != info.sample_rate for r in rates):
            out = [None] * B
            for rate, idx, y, out_lengths in self._resample_groups(
                    audio[:, 0, :], audio_lengths, rates):
                y = y.float().cpu().numpy()
                rinfo = AudioInfo(sample_rate=rate)
                for i, b in enumerate(idx):
                    out[b] = Audio(y[i, : int(out_lengths[i])], rinfo,
                                   inference_ms=infer_ms / B)
            return out
        audio = audio.float().cpu().numpy()
        audio_lengths = audio_lengths.cpu().numpy()
        for b in range(B):
            n = int(audio_lengths[b])
            out.append(Audio(audio[b, 0, :n], info, inference_ms=infer_ms / B))
        return out

    @property
    def supports_device_pcm(self) -> bool:
        """speak_batch_pcm converts the batch to int16 PCM on the model's
        device (when it is a GPU), before the copy to the host."""
        return True

    def _device_pcm(self) -> bool:
        return (self.device.type == "cuda"
                and os.environ.get("SONATA_DEVICE_PCM", "1") != "0")

    @staticmethod
    def _row_encodings(encoding, B: int):
        """Per-row wire encoding: "pcm16", "ulaw" or "alaw"."""
        from ..audio.g711 import check_encoding

        if encoding is None or isinstance(encoding, str):
            encoding = [encoding] * B
        assert len(encoding) == B, "one encoding per row"
        return [check_encoding(e) for e in encoding]

    @staticmethod
    def _wire_rows(y, lengths, sil, encs):
        """Wire-format rows of y [b, n] on the device: ops.pcm16_rows for
        the int16 rows and ONE ops.g711_rows (per-row laws) for the 8-bit
        rows, each followed by its own host copy.  Returns one NumPy row per
        input row, silence included."""
        from ..ops import g711_rows, pcm16_rows

        lens = [int(n) for n in (lengths.tolist()
                                 if isinstance(lengths, torch.Tensor)
                                 else lengths)]
        rows = [None] * len(encs)
        lin = [i for i, e in enumerate(encs) if e == "pcm16"]
        comp = [i for i, e in enumerate(encs) if e != "pcm16"]
        for idx in (lin, comp):
            if not idx:
                continue
            if len(idx) == len(encs):
                part, pl = y, lens
            else:
                sel = torch.tensor(idx, dtype=torch.long, device=y.device)
                pl = [lens[i] for i in idx]
                part = y.index_select(0, sel)[:, : max(pl, default=0)]
            ps = [sil[i] for i in idx]
            if idx is lin:
                wire, wl = pcm16_rows(part, pl, ps)
            else:
                wire, wl = g711_rows(part, pl, ps, [encs[i] for i in idx])
            wire = wire.cpu().numpy()
            for r, i in enumerate(idx):
                rows[i] = wire[r, : int(wl[r])]
        return rows

    @torch.no_grad()
    def speak_batch_pcm(self, phonemes_batch: Sequence[str], prosody=None,
                        silence_ms=None, sample_rate=None,
                        encoding=None, synthesis=None) -> List[PcmAudio]:
        """speak_batch whose results are wire-format int16: what
        `Audio.as_wave_bytes` gives for speak_batch's samples with
        `silence_ms` of silence merged on (per row or one value; rounded to
        samples as generate_silence does, at the row's output rate).  On
        cuda the order is optional device prosody, optional
        ops.resample_rows, ops.pcm16_rows, then ONE host copy of the int16
        batch per distinct rate: half the bytes of the float copy, and no
        per-row NumPy passes.  A CPU voice, or SONATA_DEVICE_PCM=0, converts
        speak_batch's samples on the host: same bytes.
        `encoding` (one value or one per row: None, "pcm16", "ulaw",
        "alaw") makes a row 8-bit G.711: audio.g711.encode of its int16.
        On cuda the 8-bit rows of a rate are one ops.g711_rows launch with
        per-row laws and one host copy of a quarter of the float bytes; a
        batch that is all one kind costs the launches and copies of the
        int16 path.
        `synthesis` is speak_batch's: one SynthesisConfig or None per row."""
        B = len(phonemes_batch)
        if silence_ms is None or isinstance(silence_ms, (int, float)):
            silence_ms = [silence_ms] * B
        assert len(silence_ms) == B, "one silence value per row"
        encs = self._row_encodings(encoding, B)
        rates = self._row_rates(sample_rate, B)
        native = self.config.sample_rate
        converts = any(r != native for r in rates)
        sil = [silence_samples(ms, r) if ms else 0
               for ms, r in zip(silence_ms, rates)]
        if not self._device_pcm():
            kw = {}
            if prosody is not None:
                kw["prosody"] = prosody
            if converts:
                kw["sample_rate"] = rates
            if synthesis is not None:
                kw["synthesis"] = synthesis
            audios = self.speak_batch(phonemes_batch, **kw)
            return [PcmAudio.from_audio(a, s, e)
                    for a, s, e in zip(audios, sil, encs)]

        audio, audio_lengths, infer_ms = self._infer_batch(
            phonemes_batch, synthesis)
        if prosody is not None:
            audio, audio_lengths = self._prosody_rows(
                audio, audio_lengths, prosody)
        if converts:
            out = [None] * B
            for rate, idx, y, out_lengths in self._resample_groups(
                    audio[:, 0, :], audio_lengths, rates):
                rows = self._wire_rows(y, out_lengths, [sil[b] for b in idx],
                                       [encs[b] for b in idx])
                rinfo = AudioInfo(sample_rate=rate)
                for i, b in enumerate(idx):
                    out[b] = PcmAudio(rows[i], rinfo,
                                      inference_ms=infer_ms / B,
                                      encoding=encs[b])
            return out
        # bf16 decoder output is read as it is (widening is exact)
        rows = self._wire_rows(audio[:, 0, :], audio_lengths, sil, encs)
        info = self.audio_output_info()
        return [PcmAudio(rows[b], info, inference_ms=infer_ms / B,
                         encoding=encs[b]) for b in range(B)]

    # ------------------------------------------------------------------ #
    # streaming decode (encoder once, HiFi-GAN chunked)
    # ------------------------------------------------------------------ #
    @property
    def supports_streaming_output(self) -> bool:
        return True

    @torch.no_grad()
    def stream_synthesis(
        self, phonemes: str, chunk_size: int = 45, chunk_padding: int = 3,
        synthesis: Optional[SynthesisConfig] = None,
    ) -> Iterator[np.ndarray]:
        """Yield waveform chunks: encoder runs once, the HiFi-GAN decoder
        runs per adaptive chunk with overlap-discard + crossfade seams
        (reference SpeechStreamer, piper/src/lib.rs:765-858).
        `synthesis`: this stream's speaker and scales (None: the voice's).
        The graph-replayed phase 1 bakes none of them in: noise_w scales the
        noise before the replay, the other two act in the eager phase 2."""
        from ..utils.graphs import phase1_enabled

        if synthesis is not None:
            self.check_synthesis_config(synthesis)
            cfg = synthesis.copy()
        else:
            cfg = self.get_synthesis_config()
        ids_l = self._encode_ids(phonemes)
        ids = torch.tensor([ids_l], dtype=torch.long, device=self.device)
        lengths = torch.tensor([len(ids_l)], dtype=torch.long, device=self.device)
        # the lock spans the whole stream (graph caches + pinned staging
        # are per-voice state); released when the generator finishes or
        # is closed/GC'd
        with self._infer_lock:
            if (phase1_enabled() and self.device.type == "cuda"
                    and self.config.num_speakers <= 1):
                # hipGraph-replayed encoder phase 1 (default ON: 9.1 ->
                # 6.8 ms first chunk at B=1; the sync-free spline made
                # capture legal).  Gated to single-speaker voices: the
                # captured phase-1 closure runs with g=None, which would
                # drop speaker conditioning.
                yield from self._stream_graphed(
                    phonemes, cfg, ids, lengths, chunk_size, chunk_padding)
                return
            yield from self._stream_eager(phonemes, cfg, ids, lengths,
                                          chunk_size, chunk_padding)

    @torch.no_grad()
    def _stream_eager(self, phonemes, cfg, ids, lengths, chunk_size,
                      chunk_padding):
        with stage_timer("encode", self.device):
            if self._engine is not None:
                # C++ engine encoder: same kernels/seeds, no per-launch
                # Python overhead on the first-chunk latency path
                z, y_mask, g = self._engine.infer_encoder(
                    ids, lengths, self._sid_tensor(1, cfg.speaker_id),
                    cfg.noise_scale, cfg.length_scale, cfg.noise_w,
                    [_utterance_seed(phonemes, cfg.speaker_id)])
                if g is not None and (not g.numel()):
                    g = None
            else:
                gens = self._generators([phonemes], cfg.speaker_id)
                z, y_mask, g = self.net.infer_encoder(
                    ids, lengths, sid=self._sid_tensor(1, cfg.speaker_id),
                    noise_scale=cfg.noise_scale,
                    length_scale=cfg.length_scale,
                    noise_w=cfg.noise_w, generators=gens,
                )
        yield from self._stream_decode(z, y_mask, g, chunk_size,
                                       chunk_padding)

    @torch.no_grad()
    def _stream_graphed(self, phonemes, cfg, ids, lengths, chunk_size,
                        chunk_padding):
        """Realtime path with hipGraph-captured encoder phase 1 (text
        encoder + duration predictor) per padded-T bucket; phase 2 (frame
        expansion, flow) stays eager (F is data-dependent); chunk decode
        replays per-shape graphs.  Padding invariance is exact (masked
        everywhere), so bucketing ids costs nothing numerically."""
        from ..utils.graphs import TupleGraphCache
        from .vits import masked_noise_rows

        T = ids.shape[1]
        Tpad = (T + 31) // 32 * 32
        if Tpad != T:
            ids = torch.nn.functional.pad(ids, (0, Tpad - T))
        gens = self._generators([phonemes], cfg.speaker_id)
        noise = masked_noise_rows(1, 2, Tpad, lengths, gens,
                                  self.device, self.dtype)
        noise = noise * cfg.noise_w  # pre-scale: graph runs noise_w=1
        if not hasattr(self, "_phase1_graphs"):
            self._phase1_graphs = TupleGraphCache(
                lambda i, l, n: self.net.encode_phase1(i, l, None, 1.0, n))
        with stage_timer("encode_graph", self.device):
            x, m_p, logs_p, x_mask, logw = self._phase1_graphs(
                ids, lengths, noise)
            z, y_mask, g = self.net.encode_phase2(
                m_p, logs_p, x_mask, logw, None, cfg.noise_scale,
                cfg.length_scale, gens)
        yield from self._stream_decode(z, y_mask, g, chunk_size,
                                       chunk_padding)

    @torch.no_grad()
    def warmup(self) -> None:
        """Pay one-time costs (hipGraph captures for the default stream
        path, kernel/module caches) at LOAD time so the first real
        request doesn't (cold first request measured ~36 ms of capture;
        profiles/r02_modes_final.json).  Safe no-op on CPU."""
        if self.device.type != "cuda":
            return
        try:
            for _ in self.stream_synthesis("wˈɔːm ˈʌp sˈɛntəns.", 45, 3):
                pass
            self.speak_one_sentence("wˈɔːm.")
        except Exception:  # warmup must never break loading
            pass

    def _stream_decode(self, z, y_mask, g, chunk_size: int,
                       chunk_padding: int) -> Iterator[np.ndarray]:
        from ..utils.graphs import DecodeGraphCache, enabled as graphs_on

        graph_cache = None
        if (graphs_on() and self.device.type == "cuda" and g is None):
            # hipGraph replay per chunk shape (launch-bound at small B);
            # decode is capture-safe (no host syncs inside)
            if not hasattr(self, "_decode_graphs"):
                if self._engine is not None:
                    self._decode_graphs = DecodeGraphCache(
                        lambda zc, mc: self._engine.decode(zc, mc, None,
                                                           None))
                else:
                    self._decode_graphs = DecodeGraphCache(
                        lambda zc, mc: self.net.decode(zc, mc, None))
            graph_cache = self._decode_graphs
        hop = self.net.arch.hop_length
        num_frames = z.shape[-1]
        # Overlap-crossfade at seams without changing the timeline: each
        # interior chunk keeps `ext` extra decoded samples (taken from its
        # right padding region); the next chunk's first `ext` samples cover
        # the same timeline window, so the sine-ramp mix preserves total
        # length exactly (streamed output == one-shot length).
        tail: Optional[np.ndarray] = None
        prev_ext = 0

        def decode_one(spec):
            z_c = z[:, :, spec.mel_start : spec.mel_end].contiguous()
            m_c = y_mask[:, :, spec.mel_start : spec.mel_end].contiguous()
            with stage_timer("decode_chunk", self.device):
                if graph_cache is not None:
                    return graph_cache(z_c, m_c)
                if self._engine is not None:
                    return self._engine.decode(z_c, m_c, g, None)
                return self.net.decode(z_c, m_c, g)

        def trim_and_emit(spec, wav):
            nonlocal tail, prev_ext
            lo = spec.trim_left_frames * hop
            hi = len(wav) - spec.trim_right_frames * hop
            ext = 0 if spec.is_last else min(
                CROSSFADE_SAMPLES, spec.trim_right_frames * hop
            )
            cur = wav[lo : hi + ext]
            if tail is not None:
                cur = crossfade(tail, cur, prev_ext)
            cut = len(cur) - ext
            tail_next = cur[cut:] if ext else None
            out = cur[:cut].astype(np.float32)
            tail = tail_next
            prev_ext = ext
            return out

        if self.device.type != "cuda":
            for spec in chunk_plan(num_frames, chunk_size, chunk_padding):
                wav = decode_one(spec)[0, 0].float().cpu().numpy()
                yield trim_and_emit(spec, wav)
                if spec.is_last:
                    return
            return

        # GPU: 1-deep pipeline — chunk i+1's decode is enqueued before
        # chunk i's host copy is consumed, so GPU decode overlaps the
        # D2H transfer + Python trim/crossfade/emit of the previous
        # chunk.  Double-buffered pinned staging; stream order makes the
        # graph-replay output safe (the copy is enqueued before the next
        # replay can overwrite its capture buffer).
        if not hasattr(self, "_pin_bufs"):
            max_samples = (1024 + 2 * 16) * hop
            self._pin_bufs = [
                torch.empty(max_samples, dtype=torch.float32,
                            pin_memory=True) for _ in range(2)]
            self._pin_events = [torch.cuda.Event(), torch.cuda.Event()]
        pending = None  # (spec, buf_idx, n_samples)
        which = 0
        first = True
        for spec in chunk_plan(num_frames, chunk_size, chunk_padding):
            audio = decode_one(spec)
            n = audio.shape[-1]
            buf = self._pin_bufs[which]
            if n > buf.shape[0]:  # defensive: unexpected chunk size
                buf = torch.empty(n, dtype=torch.float32, pin_memory=True)
                self._pin_bufs[which] = buf
            buf[:n].copy_(audio[0, 0].float(), non_blocking=True)
            self._pin_events[which].record()
            if first:
                # latency priority: emit chunk 0 before enqueuing chunk
                # 1's ~150 eager launches; pipeline from chunk 1 on
                self._pin_events[which].synchronize()
                wav = self._pin_bufs[which][:n].numpy().copy()
                yield trim_and_emit(spec, wav)
                first = False
            else:
                if pending is not None:
                    pspec, pwhich, pn = pending
                    self._pin_events[pwhich].synchronize()
                    wav = self._pin_bufs[pwhich][:pn].numpy().copy()
                    yield trim_and_emit(pspec, wav)
                pending = (spec, which, n)
            which ^= 1
            if spec.is_last:
                break
        if pending is not None:
            pspec, pwhich, pn = pending
            self._pin_events[pwhich].synchronize()
            wav = self._pin_bufs[pwhich][:pn].numpy().copy()
            yield trim_and_emit(pspec, wav)

    # ------------------------------------------------------------------ #
    # batched streams: many realtime streams share one chunk decode
    # ------------------------------------------------------------------ #
    @torch.no_grad()
    def stream_open(self, phonemes_batch: Sequence[str], chunk_size=45,
                    chunk_padding: int = 3, prosody=None,
                    sample_rate=None, synthesis=None) -> List["StreamState"]:
        """Encode a list of sentences in ONE batched encoder call and return
        one StreamState per sentence, to be advanced by stream_round.
        `chunk_size` is an int or one int per sentence.  Speaker and scales
        are those of the current synthesis config; seeds are per utterance,
        as in stream_synthesis.  Holds the inference lock for this call
        only.  Release unfinished states with stream_close.
        `prosody`: one (speed, volume, pitch) or None per sentence.  A
        stream with a triple emits, over all its chunks, what
        ops.apply_prosody_rows gives on its whole plain audio (frames * hop
        samples, known here): the stretcher's state stays on the device
        between rounds, and a round may emit an empty chunk.
        `sample_rate`: one output rate, or one rate or None per sentence
        (checked as speak_batch's).  A stream with a rate emits, over all
        its chunks, what ops.resample_rows gives on its whole audio (after
        prosody): the filter's carry stays on the device between rounds
        (ops.resample_poly_stream_rows), and a round may emit an empty
        chunk.
        `synthesis`: one SynthesisConfig or None per sentence, as in
        speak_batch: streams of different speakers and scales share the one
        encoder call."""
        B = len(phonemes_batch)
        native = self.config.sample_rate
        rates = [None if r == native else r
                 for r in self._row_rates(sample_rate, B)]
        if prosody is None:
            prosody = [None] * B
        assert len(prosody) == B, "one prosody triple (or None) per sentence"
        if isinstance(chunk_size, int):
            chunk_size = [chunk_size] * B
        chunk_size = [int(c) for c in chunk_size]
        assert len(chunk_size) == B, "one chunk_size per sentence"
        cfg, rows = self._resolve_synthesis(synthesis, B)
        if B == 0:
            return []
        id_lists = [self._encode_ids(p) for p in phonemes_batch]
        T = max(len(i) for i in id_lists)
        ids = torch.zeros((B, T), dtype=torch.long)
        lengths = torch.zeros((B,), dtype=torch.long)
        for b, il in enumerate(id_lists):
            ids[b, : len(il)] = torch.tensor(il, dtype=torch.long)
            lengths[b] = len(il)
        ids = ids.to(self.device)
        lengths = lengths.to(self.device)
        sid = self._sid_tensor(B, cfg.speaker_id)
        with self._infer_lock:
            with stage_timer("encode", self.device):
                if rows is not None:
                    z, y_mask, g = self._encoder_rows(
                        phonemes_batch, ids, lengths, rows, decode=False)
                    if g is not None and (not g.numel()):
                        g = None
                elif self._engine is not None:
                    z, y_mask, g = self._engine.infer_encoder(
                        ids, lengths, sid, cfg.noise_scale, cfg.length_scale,
                        cfg.noise_w,
                        [_utterance_seed(p, cfg.speaker_id)
                         for p in phonemes_batch])
                    if g is not None and (not g.numel()):
                        g = None
                else:
                    z, y_mask, g = self.net.infer_encoder(
                        ids, lengths, sid=sid, noise_scale=cfg.noise_scale,
                        length_scale=cfg.length_scale, noise_w=cfg.noise_w,
                        generators=self._generators(phonemes_batch,
                                                    cfg.speaker_id))
                # one host sync: every row's frame count
                frames = (y_mask[:, 0, :] > 0).sum(-1).tolist()
            slots = self._tail_slots_take(B)
            if any(t is not None for t in prosody):
                self._prosody_reserve()
            self._poly_reserve(rates)
        from ..audio.prosody import StreamProsody
        from ..audio.resample import PolyStream

        hop = self.net.arch.hop_length
        states = []
        for b in range(B):
            pros = None if prosody[b] is None else StreamProsody(
                int(frames[b]) * hop, native, *prosody[b])
            # the resampler's input length: what the stages before it emit
            n_in = int(frames[b]) * hop if pros is None else pros.n_out
            states.append(StreamState(
                index=b, z=z, row=b, frames=int(frames[b]),
                g=g[b : b + 1] if g is not None else None,
                plan=chunk_plan(int(frames[b]), chunk_size[b], chunk_padding),
                slot=slots[b], prosody=pros,
                resample=None if rates[b] is None else PolyStream(
                    n_in, native, rates[b])))
        return states

    def _poly_reserve(self, rates) -> None:
        """Device state of the streams' output rates for every tail slot
        (cuda only; on the CPU each PolyStream keeps its own carry).
        Called under _infer_lock, like _prosody_reserve."""
        if self.device.type != "cuda":
            return
        from ..ops import PolyStreamState

        for rate in set(rates) - {None}:
            if rate not in self._poly_states:
                self._poly_states[rate] = PolyStreamState(
                    self.config.sample_rate, rate, self.device)
        for st in self._poly_states.values():
            st.reserve(self._tails.shape[0])

    def _prosody_reserve(self) -> None:
        """Device state of stream prosody for every tail slot (cuda only;
        on the CPU each StreamProsody keeps its own).  Called under
        _infer_lock, like _tail_slots_take: rounds see either buffer
        whole."""
        if self.device.type != "cuda":
            return
        from ..ops import ProsodyStreamState

        if self._prosody_state is None:
            self._prosody_state = ProsodyStreamState(
                self.config.sample_rate, self.device)
        self._prosody_state.reserve(self._tails.shape[0])

    def stream_close(self, states) -> None:
        """Release the tail slots of states that will not be advanced any
        further (finished states have released theirs already).  The slot's
        prosody state needs no cleaning: a stream's plan dies with it here,
        and the next stream on the slot starts at frame 0 with an empty
        carry, so it reads nothing the slot still holds."""
        with self._tail_lock:
            for s in states:
                if s.slot is not None:
                    self._tail_free.append(s.slot)
                    s.slot = None
                s.prosody = None
                s.resample = None
                s.done = True

    def _tail_slots_take(self, n: int) -> List[int]:
        """n free tail slots; grows the device buffer when they run out
        (called under _infer_lock: rounds see either buffer whole)."""
        from ..audio.samples import _quarter_sine_ramp

        with self._tail_lock:
            if self._ramp is None:
                self._ramp = torch.from_numpy(
                    _quarter_sine_ramp(CROSSFADE_SAMPLES).copy()
                ).to(self.device)
            have = 0 if self._tails is None else self._tails.shape[0]
            if len(self._tail_free) < n:
                grow = max(64, n - len(self._tail_free), have)
                tails = torch.zeros((have + grow, CROSSFADE_SAMPLES),
                                    dtype=torch.float32, device=self.device)
                if have:
                    tails[:have].copy_(self._tails)
                self._tails = tails
                self._tail_free.extend(range(have + grow - 1, have - 1, -1))
            return [self._tail_free.pop() for _ in range(n)]

    @torch.no_grad()
    def _round_enqueue(self, states, pcm: bool, pins=None, encoding=None):
        """Take each live state's next chunk and enqueue gather -> decode ->
        seam (-> pcm) and the copy of the packed rows to the host.  Caller
        holds _infer_lock.  Returns what _round_collect needs, or None when
        no state is live."""
        from ..ops import (g711_rows, gather_windows, pcm16_rows,
                           prosody_stream_rows, resample_poly_stream_rows,
                           stream_seam_rows)

        laws = self._round_laws(states, encoding)
        if laws is not None:
            laws = [w for s, w in zip(states, laws) if not s.done]
        live = [s for s in states if not s.done]
        if not live:
            return None
        hop = self.net.arch.hop_length
        specs = [s.take_spec() for s in live]
        length = [sp.mel_end - sp.mel_start for sp in specs]
        l_max = max(length)
        zs: list = []
        src = []
        for s in live:
            for i, z in enumerate(zs):
                if z is s.z:
                    src.append(i)
                    break
            else:
                src.append(len(zs))
                zs.append(s.z)
        with stage_timer("decode_round", self.device):
            z_c = gather_windows(zs, src, [s.row for s in live],
                                 [sp.mel_start for sp in specs], length,
                                 l_max)
            g = None
            if live[0].g is not None:
                g = (live[0].g if len(live) == 1
                     else torch.cat([s.g for s in live], dim=0))
            wav = self._decode_windows(z_c, length, g)
            lo = [sp.trim_left_frames * hop for sp in specs]
            hi = [n * hop - sp.trim_right_frames * hop
                  for n, sp in zip(length, specs)]
            ext = [0 if sp.is_last else min(CROSSFADE_SAMPLES,
                                            sp.trim_right_frames * hop)
                   for sp in specs]
            out, out_len, _ = stream_seam_rows(
                wav, lo, hi, ext, [s.prev_ext for s in live],
                [s.slot for s in live], self._tails, self._ramp,
                tails_out=self._tails)
            if any(s.prosody is not None for s in live):
                if self._prosody_state is not None:
                    # slots taken by prosody-free opens since the last grow
                    self._prosody_state.reserve(self._tails.shape[0])
                out, out_len = prosody_stream_rows(
                    out, out_len, [s.prosody for s in live],
                    [s.slot for s in live], self._prosody_state,
                    last=[sp.is_last for sp in specs])
            # one launch per output rate; the other rows ride as copies
            for rate in sorted({s.resample.rate_out for s in live
                                if s.resample is not None}):
                st = self._poly_states.get(rate)
                if st is not None:
                    st.reserve(self._tails.shape[0])
                out, out_len = resample_poly_stream_rows(
                    out, out_len,
                    [s.resample if s.resample is not None
                     and s.resample.rate_out == rate else None for s in live],
                    [s.slot for s in live], st,
                    last=[sp.is_last for sp in specs])
            if laws is not None:
                out, _ = g711_rows(out, out_len, law=laws)
            elif pcm:
                out, _ = pcm16_rows(out, out_len)
        finished = []
        for s, sp, e in zip(live, specs, ext):
            s.prev_ext = e
            if sp.is_last:
                finished.append(s)
        if finished:
            self.stream_close(finished)
        event = None
        if self.device.type == "cuda":
            host = (pins if pins is not None else self._round_pins()).take(
                out.shape, out.dtype)
            host.copy_(out, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
        else:
            host = out
        return live, out_len.tolist(), host, event

    def _decode_windows(self, z_c, length, g):
        """Eager ragged decode of packed windows [R, C, l_max] with
        `length[r]` valid frames each -> [R, 1, l_max * hop]."""
        lens_t = torch.tensor(length, dtype=torch.long, device=self.device)
        # inside its valid frames a stream's y_mask is 1
        m_c = (torch.arange(z_c.shape[-1], device=self.device)[None, :]
               < lens_t[:, None]).to(z_c.dtype).unsqueeze(1)
        if self._engine is not None:
            return self._engine.decode(z_c, m_c, g, lens_t)
        return self.net.decode(z_c, m_c, g, lengths=lens_t)

    @classmethod
    def _round_laws(cls, states, encoding):
        """One G.711 law per state, or None for a round that is not 8-bit.
        A round has one output dtype: its rows share one host copy."""
        encs = cls._row_encodings(encoding, len(states))
        if all(e == "pcm16" for e in encs):
            return None
        if any(e == "pcm16" for e in encs):
            raise ValueError(
                "a stream round is all pcm16 or all G.711: its rows share "
                "one host copy")
        return encs

    def _round_pins(self):
        if not hasattr(self, "_round_pin_bufs"):
            self._round_pin_bufs = _PinnedPair()
        return self._round_pin_bufs

    @staticmethod
    def _round_collect(pending):
        """Wait for a round's host copy and slice it per stream."""
        live, out_len, host, event = pending
        if event is not None:
            event.synchronize()
        rows = host.numpy()
        return [(s, rows[r, : out_len[r]].copy())
                for r, s in enumerate(live)]

    def stream_round(self, states, pcm: bool = False, encoding=None):
        """Advance every live state by one chunk in ONE decode: gather the
        latent windows, decode them as a ragged batch, trim and crossfade
        per stream on the device, copy the packed rows to the host once.
        Returns [(state, chunk)] for the states that were live: float32
        chunks, or int16 (ops.pcm16_rows of the float chunk) with pcm=True.
        A state opened with a prosody triple has it applied before the copy
        (and before the PCM conversion); its chunk may then be empty.
        `encoding` ("ulaw" / "alaw", one value or one per state) makes the
        chunks uint8 G.711 instead: ops.g711_rows of the float chunk, peak-
        normalised per chunk as the int16 chunks are.  Both laws share a
        round; G.711 and pcm16 states do not (ValueError).
        A state whose chunk was its last is finished (state.done).  Holds
        the inference lock for the round only, and always decodes eagerly
        (R and the window length change from round to round)."""
        with self._infer_lock:
            pending = self._round_enqueue(states, pcm, encoding=encoding)
            if pending is None:
                return []
            # collected under the lock: the pinned pair belongs to the voice
            return self._round_collect(pending)

    def stream_synthesis_batch(self, phonemes_batch: Sequence[str],
                               chunk_size=45, chunk_padding: int = 3,
                               pcm: bool = False, prosody=None,
                               sample_rate=None, encoding=None,
                               synthesis=None):
        """stream_synthesis for a list of sentences at once: yields (index,
        chunk) with, per index, the chunk boundaries, total length and seams
        of stream_synthesis.  One encoder call, then one decode per round
        for all streams still running.  On cuda round r+1 is enqueued before
        round r's host copy is consumed (the first round is emitted first).
        The inference lock is held per call and per round, never across a
        yield; closing the iterator releases the streams' slots.
        `prosody` is stream_open's: with a triple, an index's chunks
        concatenate to the one-shot prosody of its plain stream, and a chunk
        may be empty (every live stream still yields one per round).
        `sample_rate` is stream_open's too: an index's chunks then
        concatenate to ops.resample_rows of its stream without a rate, and
        a chunk may be empty.
        `encoding` is stream_round's, one value or one per sentence.
        `synthesis` is stream_open's, one SynthesisConfig or None per
        sentence."""
        self._round_laws(phonemes_batch, encoding)  # checked before opening
        states = self.stream_open(phonemes_batch, chunk_size, chunk_padding,
                                  prosody=prosody, sample_rate=sample_rate,
                                  synthesis=synthesis)
        pins = _PinnedPair() if self.device.type == "cuda" else None
        try:
            with self._infer_lock:
                pending = self._round_enqueue(states, pcm, pins, encoding)
            pipelined = self.device.type == "cuda"
            first = True
            while pending is not None:
                ahead = pipelined and not first
                nxt = None
                if ahead:
                    with self._infer_lock:
                        nxt = self._round_enqueue(states, pcm, pins, encoding)
                for s, chunk in self._round_collect(pending):
                    yield s.index, chunk
                if not ahead:
                    with self._infer_lock:
                        nxt = self._round_enqueue(states, pcm, pins, encoding)
                first = False
                pending = nxt
        finally:
            self.stream_close(states)


class StreamState:
    """One stream of VitsVoice.stream_open: its latent tensor and row, frame
    count, conditioning row, chunk plan, tail slot and the crossfade length
    its previous chunk left."""

    __slots__ = ("index", "z", "row", "frames", "g", "slot", "prev_ext",
                 "done", "prosody", "resample", "_plan", "_next")

    def __init__(self, index, z, row, frames, g, plan, slot, prosody=None,
                 resample=None):
        self.index = index
        self.z = z
        self.row = row
        self.frames = frames
        self.g = g
        self.slot = slot
        self.prosody = prosody  # audio.prosody.StreamProsody or None
        self.resample = resample  # audio.resample.PolyStream or None
        self.prev_ext = 0
        self.done = False
        self._plan = plan
        self._next = next(plan, None)
        if self._next is None:
            self.done = True

    @property
    def next_spec(self):
        """The ChunkSpec the next round decodes (None when finished)."""
        return None if self.done else self._next

    def take_spec(self):
        spec = self._next
        self._next = None if spec.is_last else next(self._plan, None)
        return spec


class _PinnedPair:
    """Two pinned host buffers handed out in turn, grown on demand: a round's
    rows stay valid while the next round is enqueued."""

    def __init__(self):
        self._bufs = [None, None]
        self._which = 0

    def take(self, shape, dtype) -> torch.Tensor:
        n = 1
        for d in shape:
            n *= int(d)
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        buf = self._bufs[self._which]
        if buf is None or buf.shape[0] < nbytes:
            buf = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8,
                              pin_memory=True)
            self._bufs[self._which] = buf
        self._which ^= 1
        return buf[:nbytes].view(dtype).view(*shape)


# --------------------------------------------------------------------------- #
# loading / creation
# --------------------------------------------------------------------------- #
def _weights_path_for(config_path: str) -> str:
    stem = config_path
    if stem.endswith(".json"):
        stem = stem[: -len(".json")]
    if stem.endswith(".onnx"):
        stem = stem[: -len(".onnx")]
    return stem + ".safetensors"


def load_voice(
    config_path: str, device: str = "cpu",
    dtype: Optional[torch.dtype] = None, engine: str = "auto"
) -> VitsVoice:
    """Load a voice pack: `<stem>.json` + `<stem>.safetensors`.

    Mirrors the reference loader dispatch (piper/src/lib.rs:88-110); the
    `streaming` config key only changes default synthesis mode — the same
    net serves one-shot and streaming here (encoder/decoder split is a
    method boundary, not two files)."""
    config = ModelConfig.from_json_path(config_path)
    if dtype is None:
        dtype = torch.bfloat16 if device.startswith("cuda") else torch.float32
    net = VitsModel(config.num_symbols, config.architecture,
                    n_speakers=max(config.num_speakers, 1))
    wpath = _weights_path_for(config_path)
    if os.path.exists(wpath):
        from safetensors.torch import load_file

        state = load_file(wpath)
        missing, unexpected = net.load_state_dict(state, strict=False)
        if missing or unexpected:
            raise ModelError(
                f"voice weights mismatch: missing={missing[:5]} "
                f"unexpected={unexpected[:5]}"
            )
    else:
        raise ModelError(f"voice weights not found: {wpath}")
    # serving runtime: the C++ VitsEngine by default (same kernels, same
    # per-utterance seeds -> identical audio); SONATA_ENGINE=python or
    # engine="python" keeps the torch-module path.
    #
    # warmup(): see VitsVoice.warmup — capture/compile costs paid at
    # load time instead of the first request.
    eng = None
    choice = os.environ.get("SONATA_ENGINE", engine)
    if choice == "auto" and not device.startswith("cuda"):
        choice = "python"  # CPU stays on the torch oracle path
    if choice in ("auto", "cpp"):
        try:
            from ..ops import hip_ext

            ext = hip_ext(required=False)
            if ext is not None and hasattr(ext, "VitsEngine"):
                eng = ext.VitsEngine(
                    config_path, device,
                    "bf16" if (dtype == torch.bfloat16) else "f32")
        except Exception:
            if choice == "cpp":
                raise
            eng = None
    return VitsVoice(config, net, device=device, dtype=dtype, engine=eng)


def create_random_voice(
    out_dir: str,
    name: str = "test_voice",
    quality: str = "medium",
    language: str = "en-us",
    num_speakers: int = 1,
    seed: int = 0,
) -> str:
    """Create a random-init voice pack (tests / synthetic benches — there is
    no network for real checkpoints).  Returns the config path."""
    from .config import QUALITY_PRESETS, VitsArchitecture

    preset = QUALITY_PRESETS[quality]
    arch = VitsArchitecture(**preset["arch"])
    if num_speakers > 1:
        arch.gin_channels = 256
    config = ModelConfig(
        key=name,
        language_code=language,
        sample_rate=preset["sample_rate"],
        quality=quality,
        num_speakers=num_speakers,
        speaker_id_map={f"spk{i}": i for i in range(num_speakers)}
        if num_speakers > 1 else {},
        espeak_voice=language,
        architecture=arch,
    )
    torch.manual_seed(seed)
    net = VitsModel(config.num_symbols, arch, n_speakers=max(num_speakers, 1))
    os.makedirs(out_dir, exist_ok=True)
    cfg_path = os.path.join(out_dir, f"{name}.json")
    config.save_json(cfg_path)
    from safetensors.torch import save_file

    save_file(net.state_dict(), _weights_path_for(cfg_path))
    return cfg_path
