"""Synthesizer facade: stream modes + prosody post-processing.

Parity: reference crates/sonata/synth/src/lib.rs —
`SYNTHESIS_THREAD_POOL` (:17-26, rayon num_cpus*4) -> a shared
ThreadPoolExecutor; `AudioOutputConfig` percent->param mapping with ranges
RATE (0.5,5.5) VOLUME (0,1) PITCH (0.5,1.5) (:13-15, utils.rs:6-8) and
sonic application (:55-105) -> sonata_amd.audio.prosody;
`SonataSpeechSynthesizer` (:119-203) with synthesize_lazy (:138),
synthesize_parallel (:145), synthesize_streamed realtime (:152),
synthesize_to_file (:170); streams Lazy/Parallel/Realtime (:282-430)
including the realtime producer thread + queue and growing chunk size
(:350-358), per-chunk prosody (:392-407), appended silence (:408-412).
"""

from __future__ import annotations

import os
import queue
import threading
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Iterator, List, Optional

import numpy as np

from ..audio.prosody import apply_prosody
from ..audio.resample import (StreamResampler, check_rate, is_identity,
                              resample_poly)
from ..audio.g711 import check_encoding
from ..audio.g711 import encode as g711_encode
from ..audio.samples import (generate_silence, merge, silence_samples,
                             to_i16)
from ..audio.wav import write_wav_file, write_wav_file_g711
from ..core import Audio, AudioInfo, PcmAudio, SonataModel
from .batcher import _config_set, _StreamIter

# percent(0-100) -> parameter ranges (reference synth/src/lib.rs:13-15)
RATE_RANGE = (0.5, 5.5)
VOLUME_RANGE = (0.0, 1.0)
PITCH_RANGE = (0.5, 1.5)

_POOL: Optional[ThreadPoolExecutor] = None
_POOL_LOCK = threading.Lock()


def synthesis_pool() -> ThreadPoolExecutor:
    """Global synthesis thread pool (reference SYNTHESIS_THREAD_POOL:
    rayon pool of num_cpus*4 threads, synth/src/lib.rs:17-26)."""
    global _POOL
    with _POOL_LOCK:
        if _POOL is None:
            n = (os.cpu_count() or 4) * 4
            _POOL = ThreadPoolExecutor(
                max_workers=n, thread_name_prefix="sonata_synth"
            )
        return _POOL


def device_prosody_enabled(model) -> bool:
    """Device prosody is available for `model`: it advertises
    supports_device_prosody, lives on cuda, and SONATA_DEVICE_PROSODY is
    not 0."""
    if os.environ.get("SONATA_DEVICE_PROSODY", "1") == "0":
        return False
    if not getattr(model, "supports_device_prosody", False):
        return False
    dev = getattr(model, "device", None)
    return getattr(dev, "type", None) == "cuda"


def _percent(value: float, lo: float, hi: float) -> float:
    v = min(max(value, 0.0), 100.0)
    return lo + (hi - lo) * (v / 100.0)


@dataclass
class AudioOutputConfig:
    """Prosody knobs in percent (0-100) + appended silence, mirroring the
    reference AudioOutputConfig (synth/src/lib.rs:28-117).  `sample_rate`
    (Hz, not percent) asks for the result at another rate than the voice's
    own; it is no part of `is_noop`, which speaks of prosody alone.
    `encoding` (None, "pcm16", "ulaw" or "alaw") chooses the wire format of
    PcmAudio results and written files: 16-bit linear PCM, or 8-bit G.711
    (audio.g711.encode of that PCM).  Float results never change, and it
    is no part of `is_noop` either."""

    rate: Optional[float] = None
    volume: Optional[float] = None
    pitch: Optional[float] = None
    appended_silence_ms: Optional[float] = None
    sample_rate: Optional[int] = None
    encoding: Optional[str] = None

    def prosody_triple(self):
        """(speed, volume, pitch) as parameters (not percent) — what `apply`
        hands to apply_prosody; the form speak_batch(prosody=...) takes."""
        speed = _percent(self.rate, *RATE_RANGE) if self.rate is not None else 1.0
        volume = (
            _percent(self.volume, *VOLUME_RANGE)
            if self.volume is not None else 1.0
        )
        pitch = (
            _percent(self.pitch, *PITCH_RANGE) if self.pitch is not None else 1.0
        )
        return speed, volume, pitch

    def apply(self, samples: np.ndarray, sample_rate: int) -> np.ndarray:
        speed = _percent(self.rate, *RATE_RANGE) if self.rate is not None else 1.0
        volume = (
            _percent(self.volume, *VOLUME_RANGE)
            if self.volume is not None else 1.0
        )
        pitch = (
            _percent(self.pitch, *PITCH_RANGE) if self.pitch is not None else 1.0
        )
        return apply_prosody(samples, sample_rate, speed=speed, volume=volume,
                             pitch=pitch)

    @property
    def is_noop(self) -> bool:
        return (
            self.rate is None and self.volume is None and self.pitch is None
        )


class SonataSpeechSynthesizer:
    """Facade over a SonataModel: phonemize + synthesize in three modes."""

    def __init__(self, model: SonataModel):
        self.model = model
        # optional synth.batcher.StreamBatcher on the same model: when set,
        # synthesize_streamed opens its sentences through it, so concurrent
        # realtime streams share chunk decodes
        self.stream_batcher = None
        # prosody of synthesize_streamed: "chunk" applies the output config
        # to every chunk on its own, on the host (the reference's
        # behaviour); "continuous" hands the triple to the model's stream
        # path, which stretches the sentence as a whole with its state kept
        # between chunks (on the device for a cuda voice)
        self.stream_prosody = os.environ.get("SONATA_STREAM_PROSODY",
                                             "chunk") or "chunk"
        if self.stream_prosody not in ("chunk", "continuous"):
            raise ValueError(
                "SONATA_STREAM_PROSODY must be 'chunk' or 'continuous', "
                f"not {self.stream_prosody!r}")
        # output sample rate of synthesize_streamed: "host" converts every
        # chunk here with one audio.resample.StreamResampler per sentence;
        # "device" hands the rate to the model's batched stream path, which
        # converts inside the shared round (other chunk boundaries, and the
        # last bits of f32 accumulation instead of f64)
        self.stream_resample = os.environ.get("SONATA_STREAM_RESAMPLE",
                                              "host") or "host"
        if self.stream_resample not in ("host", "device"):
            raise ValueError(
                "SONATA_STREAM_RESAMPLE must be 'host' or 'device', "
                f"not {self.stream_resample!r}")

    # ------------------------------------------------------------------ #
    def audio_output_info(self) -> AudioInfo:
        return self.model.audio_output_info()

    def device_prosody(self, cfg: Optional[AudioOutputConfig]) -> bool:
        """True when `cfg`'s rate / volume / pitch run on the device inside
        speak_batch: the model offers it, lives on cuda, and
        SONATA_DEVICE_PROSODY is not 0 (0 = host prosody, for A/B runs)."""
        return device_prosody_enabled(self.model) and cfg is not None \
            and not cfg.is_noop

    def output_rate(self, cfg: Optional[AudioOutputConfig]) -> Optional[int]:
        """The rate `cfg` asks for when it differs from the voice's own,
        else None.  Raises ValueError for a rate the filter does not serve."""
        if cfg is None or getattr(cfg, "sample_rate", None) is None:
            return None
        native = self.model.audio_output_info().sample_rate
        if is_identity(native, cfg.sample_rate):
            return None
        check_rate(native, cfg.sample_rate)
        return int(cfg.sample_rate)

    @staticmethod
    def output_encoding(cfg: Optional[AudioOutputConfig]) -> str:
        """The wire encoding `cfg` asks for: "pcm16" (also for None),
        "ulaw" or "alaw".  Raises ValueError for anything else."""
        return check_encoding(getattr(cfg, "encoding", None)
                              if cfg is not None else None)

    def device_rate(self, cfg: Optional[AudioOutputConfig]) -> bool:
        """True when the conversion to cfg's rate runs inside speak_batch*:
        the model offers it and lives on cuda, and prosody, which comes
        first, does not have to run on the host."""
        dev = getattr(self.model, "device", None)
        return (getattr(self.model, "supports_output_rate", False)
                and getattr(dev, "type", None) == "cuda"
                and (cfg.is_noop or self.device_prosody(cfg)))

    def _model_batch(self, name: str, sentences: List[str], synthesis,
                     **kw):
        """model.speak_batch / speak_batch_pcm for one request.  Its
        SynthesisConfig (speaker and scales; None: the model's own) goes in
        as the rows' synthesis=; a model without supports_row_synthesis has
        it set voice-wide around the call."""
        fn = getattr(self.model, name)
        if synthesis is None:
            return fn(sentences, **kw)
        if getattr(self.model, "supports_row_synthesis", False):
            return fn(sentences, synthesis=[synthesis] * len(sentences),
                      **kw)
        with _config_set(self.model, synthesis):
            return fn(sentences, **kw)

    def _speak_device_prosody(self, sentences: List[str],
                              cfg: AudioOutputConfig,
                              synthesis=None) -> List[Audio]:
        """One speak_batch with cfg's prosody applied on the device; _post
        then only appends silence."""
        triple = cfg.prosody_triple()
        batch = self._model_batch(
            "speak_batch", sentences, synthesis,
            prosody=[triple] * len(sentences))
        return [self._post(a, cfg, prosody_done=True) for a in batch]

    def _speak_rate(self, sentences: List[str], cfg: AudioOutputConfig,
                    rate: int, synthesis=None) -> List[Audio]:
        """One batch at another output rate.  On the device: prosody and the
        conversion inside speak_batch, silence here.  Else the float batch
        is finished on the host: prosody, resample_poly, silence."""
        if self.device_rate(cfg):
            kw = {}
            if not cfg.is_noop:
                kw["prosody"] = [cfg.prosody_triple()] * len(sentences)
            batch = self._model_batch("speak_batch", sentences, synthesis,
                                      sample_rate=rate, **kw)
            return [self._post(a, cfg, prosody_done=True) for a in batch]
        if self.device_prosody(cfg):
            batch = self._model_batch(
                "speak_batch", sentences, synthesis,
                prosody=[cfg.prosody_triple()] * len(sentences))
            return [self._post(a, cfg, prosody_done=True, rate=rate)
                    for a in batch]
        batch = self._model_batch("speak_batch", sentences, synthesis)
        return [self._post(a, cfg, rate=rate) for a in batch]

    @staticmethod
    def _to_rate(audio: Audio, rate: Optional[int]) -> Audio:
        if rate is None or audio.info.sample_rate == rate:
            return audio
        return Audio(resample_poly(audio.samples, audio.info.sample_rate, rate),
                     AudioInfo(sample_rate=rate), audio.inference_ms)

    def _post(self, audio: Audio, cfg: Optional[AudioOutputConfig],
              prosody_done: bool = False,
              rate: Optional[int] = None) -> Audio:
        if cfg is None:
            return audio
        samples = audio.samples
        if not cfg.is_noop and not prosody_done:
            samples = cfg.apply(samples, audio.info.sample_rate)
        if rate is not None:
            audio = self._to_rate(
                Audio(samples, audio.info, audio.inference_ms), rate)
            samples = audio.samples
        if cfg.appended_silence_ms:
            samples = merge(
                samples,
                generate_silence(cfg.appended_silence_ms,
                                 audio.info.sample_rate),
            )
        return Audio(samples, audio.info, audio.inference_ms)

    def _speak_pcm(self, sentences: List[str],
                   cfg: Optional[AudioOutputConfig],
                   synthesis=None) -> List[PcmAudio]:
        """One batch as wire-format PcmAudio, bytes equal to
        as_wave_bytes() of the float path.  A model with speak_batch_pcm
        gets prosody (when the device path is on), appended silence and the
        int16 conversion in that one call; it decides itself between the
        device and the host conversion (SONATA_DEVICE_PCM).  Prosody that
        has to run on the host keeps the float path up to the conversion."""
        host_prosody = (cfg is not None and not cfg.is_noop
                        and not self.device_prosody(cfg))
        rate = self.output_rate(cfg)
        enc = self.output_encoding(cfg)
        if rate is not None and not self.device_rate(cfg):
            # the conversion runs on the host, so the float path is kept up
            # to it (device prosody first, where it is on)
            if self.device_prosody(cfg):
                batch = self._model_batch(
                    "speak_batch", sentences, synthesis,
                    prosody=[cfg.prosody_triple()] * len(sentences))
                return [self.to_pcm(a, cfg, prosody_done=True, rate=rate)
                        for a in batch]
            batch = self._model_batch("speak_batch", sentences, synthesis)
            return [self.to_pcm(a, cfg, rate=rate) for a in batch]
        if getattr(self.model, "supports_device_pcm", False) \
                and not host_prosody:
            triple = (cfg.prosody_triple()
                      if cfg is not None and not cfg.is_noop else None)
            kw = {"sample_rate": rate} if rate is not None else {}
            if enc != "pcm16":
                kw["encoding"] = enc
            return self._model_batch(
                "speak_batch_pcm", sentences, synthesis,
                prosody=[triple] * len(sentences) if triple else None,
                silence_ms=cfg.appended_silence_ms if cfg else None, **kw)
        if rate is not None:
            return [PcmAudio.from_audio(a, encoding=enc)
                    for a in self._speak_rate(sentences, cfg, rate,
                                              synthesis)]
        batch = self._model_batch("speak_batch", sentences, synthesis)
        return [self.to_pcm(a, cfg) for a in batch]

    def to_pcm(self, audio: Audio, cfg: Optional[AudioOutputConfig],
               prosody_done: bool = False,
               rate: Optional[int] = None) -> PcmAudio:
        """Host finish of one float result: prosody unless done, the
        conversion to `rate` when one is given, then the int16 conversion
        with cfg's silence appended (counted at the result's rate), then
        cfg's G.711 encoding when it names one."""
        if cfg is not None and not cfg.is_noop and not prosody_done:
            audio = Audio(cfg.apply(audio.samples, audio.info.sample_rate),
                          audio.info, audio.inference_ms)
        audio = self._to_rate(audio, rate)
        sil = (silence_samples(cfg.appended_silence_ms,
                               audio.info.sample_rate)
               if cfg is not None and cfg.appended_silence_ms else 0)
        return PcmAudio.from_audio(audio, sil, self.output_encoding(cfg))

    # ------------------------------------------------------------------ #
    def synthesize_lazy(
        self, text: str, output_config: Optional[AudioOutputConfig] = None,
        pcm: bool = False, synthesis=None,
    ) -> Iterator[Audio]:
        """Pull-based: each sentence synthesized when consumed
        (reference SonataSpeechStreamLazy, synth/src/lib.rs:282-307).
        `pcm=True` yields PcmAudio (int16, converted on the device when the
        model can) instead of float Audio; the wire bytes are the same.
        `synthesis`: optional SynthesisConfig (speaker and scales) of this
        request alone; the model's own config is neither read nor changed."""
        rate = self.output_rate(output_config)
        self.output_encoding(output_config)
        phonemes = self.model.phonemize_text(text)
        for sent in phonemes:
            if pcm:
                yield self._speak_pcm([sent], output_config, synthesis)[0]
                continue
            if rate is not None:
                yield self._speak_rate([sent], output_config, rate,
                                       synthesis)[0]
                continue
            if self.device_prosody(output_config):
                yield self._speak_device_prosody([sent], output_config,
                                                 synthesis)[0]
                continue
            if synthesis is not None:
                yield self._post(self._model_batch(
                    "speak_batch", [sent], synthesis)[0], output_config)
                continue
            yield self._post(self.model.speak_one_sentence(sent), output_config)

    def synthesize_parallel(
        self, text: str, output_config: Optional[AudioOutputConfig] = None,
        pcm: bool = False, synthesis=None,
    ) -> Iterator[Audio]:
        """Eager batched synthesis of all sentences.  The reference fans
        out per-sentence rayon tasks (synth/src/lib.rs:316-320); here the
        model's true padded batch path does the fan-out on-device.
        `pcm=True` yields PcmAudio, as in synthesize_lazy; `synthesis` is
        synthesize_lazy's too."""
        self.output_encoding(output_config)
        phonemes = self.model.phonemize_text(text)
        if len(phonemes) == 0:
            return iter(())
        if pcm:
            return iter(self._speak_pcm(list(phonemes), output_config,
                                        synthesis))
        rate = self.output_rate(output_config)
        if rate is not None:
            return iter(self._speak_rate(list(phonemes), output_config, rate,
                                         synthesis))
        if self.device_prosody(output_config):
            return iter(self._speak_device_prosody(list(phonemes),
                                                   output_config, synthesis))
        batch = self._model_batch("speak_batch", list(phonemes), synthesis)
        return iter([self._post(a, output_config) for a in batch])

    def synthesize_streamed(
        self,
        text: str,
        output_config: Optional[AudioOutputConfig] = None,
        chunk_size: int = 45,
        chunk_padding: int = 3,
        synthesis=None,
    ) -> Iterator[np.ndarray]:
        """Realtime mode: producer thread pushes waveform chunks through a
        queue while the caller consumes (reference RealtimeSpeechStream,
        synth/src/lib.rs:335-430).  Chunk size grows per processed chunk
        (:352-356).  Yields float32 sample chunks.
        With stream_prosody == "continuous" (and a model with batched
        streams) rate / pitch / volume run inside the model's stream path:
        a sentence's chunks concatenate to its one-shot prosody, nothing is
        applied here and empty chunks are dropped.
        An output sample rate is served by one audio.resample
        StreamResampler per sentence, on the host, after prosody in either
        mode: it is flushed at the end of the sentence, its empty chunks are
        dropped and silence is counted at the output rate.
        With stream_resample == "device" (and a model with batched streams)
        the rate rides into the model's stream path instead, after prosody
        there: no StreamResampler is built and empty chunks are dropped.
        It applies when no prosody is left to run here, on the host, which
        would have to come before the conversion.
        `synthesis` is synthesize_lazy's: it rides into whichever stream
        path serves the request (the stream batcher, the model's batched
        streams or its single stream)."""
        rate = self.output_rate(output_config)
        check = getattr(self.model, "check_synthesis_config", None)
        if synthesis is not None and check is not None:
            check(synthesis)
        rows = getattr(self.model, "supports_row_synthesis", False)
        # one request's config for a model call: as synthesis= where the
        # model takes it, else set voice-wide while the stream runs
        syn_one = ({"synthesis": synthesis}
                   if synthesis is not None and rows else {})
        syn_rows = ({"synthesis": [synthesis]}
                    if synthesis is not None and rows else {})
        syn_open = {"synthesis": synthesis} if synthesis is not None else {}
        held = None if rows else synthesis
        phonemes = self.model.phonemize_text(text)
        info = self.model.audio_output_info()
        q: "queue.Queue" = queue.Queue()
        DONE, ERROR = object(), object()
        if self.stream_prosody not in ("chunk", "continuous"):
            raise ValueError(f"stream_prosody {self.stream_prosody!r}")
        triple = None
        if (self.stream_prosody == "continuous" and output_config is not None
                and not output_config.is_noop
                and self.model.supports_streaming_output
                and hasattr(self.model, "stream_synthesis_batch")):
            triple = output_config.prosody_triple()
        if self.stream_resample not in ("host", "device"):
            raise ValueError(f"stream_resample {self.stream_resample!r}")
        host_prosody = (triple is None and output_config is not None
                        and not output_config.is_noop)
        model_rate = (rate is not None and self.stream_resample == "device"
                      and not host_prosody
                      and self.model.supports_streaming_output
                      and hasattr(self.model, "stream_synthesis_batch"))

        def producer():
            try:
                for n_done, sent in enumerate(phonemes):
                    # Chunk size grows with each processed SENTENCE —
                    # a deliberate bounded-linear variant of the
                    # reference's compounding growth (reference
                    # RealtimeSpeechStream, synth/src/lib.rs:350-358,
                    # multiplies by cumulative processed CHUNK count,
                    # unbounded).  Intent is identical: first sentence
                    # streams with low latency, later ones with bigger
                    # (faster) chunks; the in-sentence chunker grows
                    # further.  The 1024 cap matches MAX_CHUNK_SIZE.
                    cs = min(chunk_size * (n_done + 1), 1024)
                    if triple is not None or model_rate:
                        kw = {"sample_rate": rate} if model_rate else {}
                        if self.stream_batcher is not None:
                            it = self.stream_batcher.open(
                                sent, cs, chunk_padding, prosody=triple,
                                **kw, **syn_open)
                        else:
                            it = (c for _, c in
                                  self.model.stream_synthesis_batch(
                                      [sent], cs, chunk_padding,
                                      prosody=(None if triple is None
                                               else [triple]), **kw,
                                      **syn_rows))
                    elif (self.stream_batcher is not None
                            and self.model.supports_streaming_output):
                        it = self.stream_batcher.open(sent, cs, chunk_padding,
                                                      **syn_open)
                    elif self.model.supports_streaming_output:
                        it = self.model.stream_synthesis(
                            sent, cs, chunk_padding, **syn_one
                        )
                    else:
                        it = iter([self._model_batch(
                            "speak_batch", [sent], synthesis)[0].samples])
                    # (the stream batcher sets the config itself for a model
                    # that takes none per stream)
                    if held is not None and not isinstance(it, _StreamIter):
                        it = self._held(it, held)
                    rs = (StreamResampler(info.sample_rate, rate)
                          if rate is not None and not model_rate else None)
                    for chunk in it:
                        if triple is None and output_config is not None \
                                and not output_config.is_noop:
                            chunk = output_config.apply(chunk, info.sample_rate)
                        if rs is not None:
                            chunk = rs.push(chunk)
                        if (triple is not None or rs is not None
                                or model_rate) and not len(chunk):
                            continue
                        q.put(chunk)
                    if rs is not None:
                        chunk = rs.flush()
                        if len(chunk):
                            q.put(chunk)
                    if output_config is not None and output_config.appended_silence_ms:
                        q.put(generate_silence(
                            output_config.appended_silence_ms,
                            rate if rate is not None else info.sample_rate
                        ))
                q.put(DONE)
            except BaseException as e:  # propagate to consumer
                q.put(ERROR)
                q.put(e)

        synthesis_pool().submit(producer)
        while True:
            item = q.get()
            if item is DONE:
                return
            if item is ERROR:
                raise q.get()
            yield item

    def _held(self, it, synthesis):
        """Run a model stream with `synthesis` set voice-wide while it
        lasts: a model without supports_row_synthesis reads its config when
        the stream starts."""
        with _config_set(self.model, synthesis):
            yield from it

    def synthesize_to_file(
        self,
        path: str,
        text: str,
        output_config: Optional[AudioOutputConfig] = None,
        synthesis=None,
    ) -> Audio:
        """Collect parallel synthesis into one WAV (reference
        synthesize_to_file, synth/src/lib.rs:170-198).  With a G.711
        encoding in the output config the file holds the codes of the int16
        it would hold otherwise."""
        enc = self.output_encoding(output_config)
        pieces: List[np.ndarray] = []
        info = self.model.audio_output_info()
        inference_ms = 0.0
        for audio in self.synthesize_parallel(text, output_config,
                                              synthesis=synthesis):
            info = audio.info  # the result's own rate
            pieces.append(audio.samples)
            inference_ms += audio.inference_ms
        samples = (
            np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.float32)
        )
        if enc != "pcm16":
            write_wav_file_g711(path, g711_encode(to_i16(samples), enc),
                                info.sample_rate, enc)
        else:
            write_wav_file(path, samples, info.sample_rate)
        return Audio(samples, info, inference_ms)

    # delegation (reference re-implements SonataModel by delegation,
    # synth/src/lib.rs:205-247)
    def phonemize_text(self, text: str):
        return self.model.phonemize_text(text)

    def get_synthesis_config(self):
        return self.model.get_synthesis_config()

    def set_synthesis_config(self, cfg) -> None:
        self.model.set_synthesis_config(cfg)
