"""Core types: errors, phonemes, audio containers, model interface.

Parity: reference crates/sonata/core/src/lib.rs (SonataError :15-50,
Phonemes :53-79, trait SonataModel :82-131) and
crates/audio/ops/src/samples.rs (Audio :208-271, AudioInfo :10-14).
Re-designed as idiomatic Python ABCs over numpy/torch rather than a
trait-object hierarchy.
"""

from __future__ import annotations

import abc
import dataclasses
from dataclasses import dataclass, field
from typing import Dict, Iterator, List, Optional, Sequence

import numpy as np


# --------------------------------------------------------------------------- #
# Errors (reference: core/src/lib.rs:20-24 — 3-variant enum)
# --------------------------------------------------------------------------- #
class SonataError(Exception):
    """Base error for the engine."""


class ModelError(SonataError):
    """Voice pack loading / inference errors."""


class OperationError(SonataError):
    """Invalid operation / bad configuration."""


class PhonemizationError(SonataError):
    """Text front-end errors."""


# --------------------------------------------------------------------------- #
# Phonemes (reference: core/src/lib.rs:53-79 — Vec of per-sentence IPA)
# --------------------------------------------------------------------------- #
@dataclass
class Phonemes:
    """Per-sentence IPA phoneme strings for one utterance."""

    sentences: List[str] = field(default_factory=list)

    def __iter__(self) -> Iterator[str]:
        return iter(self.sentences)

    def __len__(self) -> int:
        return len(self.sentences)

    def __getitem__(self, i):
        return self.sentences[i]

    def append(self, s: str) -> None:
        self.sentences.append(s)

    def to_string(self) -> str:
        return " ".join(self.sentences)


# --------------------------------------------------------------------------- #
# Audio containers (reference: ops/src/samples.rs:10-14, 208-271)
# --------------------------------------------------------------------------- #
@dataclass(frozen=True)
class AudioInfo:
    sample_rate: int
    num_channels: int = 1
    sample_width: int = 2  # bytes per sample on the wire (i16)


@dataclass
class Audio:
    """A synthesized waveform plus timing metadata.

    `samples` is float32 mono in [-1, 1] (model output scale).
    `inference_ms` is the wall time spent in neural inference, used for the
    real-time factor (reference: samples.rs:253-260).
    """

    samples: np.ndarray
    info: AudioInfo
    inference_ms: float = 0.0

    def __post_init__(self):
        self.samples = np.asarray(self.samples, dtype=np.float32).reshape(-1)

    @property
    def duration_ms(self) -> float:
        return len(self.samples) * 1000.0 / self.info.sample_rate

    @property
    def real_time_factor(self) -> float:
        d = self.duration_ms
        return (self.inference_ms / d) if d > 0 else 0.0

    def as_wave_bytes(self) -> bytes:
        from .audio.samples import to_i16_bytes

        return to_i16_bytes(self.samples)

    def save_to_file(self, path: str) -> None:
        from .audio.wav import write_wav_file

        write_wav_file(path, self.samples, self.info.sample_rate)


@dataclass
class PcmAudio:
    """A synthesized waveform already converted to wire format: `pcm` is
    the peak-normalised int16 that `Audio.as_wave_bytes` would produce for
    the float samples it came from (converted on the device by
    speak_batch_pcm when available).  Offers front ends what Audio does.

    With `encoding` "ulaw" or "alaw", `pcm` is the uint8 G.711 codes of
    that int16 (audio.g711.encode) and `info.sample_width` is 1."""

    pcm: np.ndarray
    info: AudioInfo
    inference_ms: float = 0.0
    encoding: str = "pcm16"

    def __post_init__(self):
        if self.encoding == "pcm16":
            self.pcm = np.asarray(self.pcm, dtype=np.int16).reshape(-1)
            return
        from .audio.g711 import check_law

        check_law(self.encoding)
        self.pcm = np.asarray(self.pcm, dtype=np.uint8).reshape(-1)
        if self.info.sample_width != 1:
            self.info = dataclasses.replace(self.info, sample_width=1)

    @classmethod
    def from_audio(cls, audio: Audio, silence_samples: int = 0,
                   encoding: str = "pcm16") -> "PcmAudio":
        """Host conversion: to_i16 of audio.samples followed by
        `silence_samples` zeros (equal to to_i16 of the samples with that
        silence merged: zeros neither move the peak nor scale), then
        g711.encode of it for a G.711 `encoding`."""
        from .audio.samples import to_i16

        pcm = to_i16(audio.samples)
        if silence_samples > 0:
            pcm = np.concatenate(
                [pcm, np.zeros(silence_samples, dtype=np.int16)])
        if encoding != "pcm16":
            from .audio.g711 import encode

            pcm = encode(pcm, encoding)
        return cls(pcm, audio.info, audio.inference_ms, encoding)

    def to_int16(self) -> np.ndarray:
        """The samples as int16: `pcm` itself, or the decoded codes."""
        if self.encoding == "pcm16":
            return self.pcm
        from .audio.g711 import decode

        return decode(self.pcm, self.encoding)

    @property
    def duration_ms(self) -> float:
        return len(self.pcm) * 1000.0 / self.info.sample_rate

    @property
    def real_time_factor(self) -> float:
        d = self.duration_ms
        return (self.inference_ms / d) if d > 0 else 0.0

    def as_wave_bytes(self) -> bytes:
        if self.encoding != "pcm16":
            return self.pcm.tobytes()
        return self.pcm.astype("<i2", copy=False).tobytes()

    def save_to_file(self, path: str) -> None:
        if self.encoding != "pcm16":
            from .audio.wav import write_wav_file_g711

            write_wav_file_g711(path, self.pcm, self.info.sample_rate,
                                self.encoding)
            return
        from .audio.wav import write_wav_file_pcm

        write_wav_file_pcm(path, self.pcm, self.info.sample_rate)


# --------------------------------------------------------------------------- #
# Model interface (reference: core/src/lib.rs:82-131 trait SonataModel)
# --------------------------------------------------------------------------- #
class SonataModel(abc.ABC):
    """Abstract voice model: phonemization + synthesis.

    Concrete impl: sonata_amd.models.voice.VitsVoice.
    """

    # -- required ----------------------------------------------------------- #
    @abc.abstractmethod
    def audio_output_info(self) -> AudioInfo:
        ...

    @abc.abstractmethod
    def phonemize_text(self, text: str) -> Phonemes:
        ...

    @abc.abstractmethod
    def speak_one_sentence(self, phonemes: str) -> Audio:
        ...

    def speak_batch(self, phonemes_batch: Sequence[str]) -> List[Audio]:
        """True padded batching (the reference's speak_batch loops batch=1,
        piper/src/lib.rs:425-437 — here a real [B, T] batch is the default)."""
        return [self.speak_one_sentence(p) for p in phonemes_batch]

    @property
    def supports_device_pcm(self) -> bool:
        """True when the model offers speak_batch_pcm(phonemes_batch,
        prosody=None, silence_ms=None) -> List[PcmAudio]."""
        return False

    @property
    def supports_output_rate(self) -> bool:
        """True when speak_batch / speak_batch_pcm take sample_rate= (one
        int, or one int-or-None per row) and return each row converted to
        its rate, with AudioInfo(sample_rate=<its rate>)."""
        return False

    @property
    def supports_row_synthesis(self) -> bool:
        """True when speak_batch / speak_batch_pcm / stream_open /
        stream_synthesis_batch take synthesis= (one synthesis config or
        None per row; stream_synthesis takes one): every row is rendered
        with its own speaker and scales inside the one batch, and the
        model's own config is left alone."""
        return False

    # -- synthesis config (reference get/set_fallback..., typed not Any) ---- #
    @abc.abstractmethod
    def get_synthesis_config(self):
        ...

    @abc.abstractmethod
    def set_synthesis_config(self, config) -> None:
        ...

    # -- speaker helpers (reference: core/src/lib.rs:92-116 default impls) -- #
    def get_speakers(self) -> Optional[Dict[int, str]]:
        return None

    def speaker_id_to_name(self, sid: int) -> Optional[str]:
        speakers = self.get_speakers()
        if not speakers:
            return None
        return speakers.get(sid)

    def speaker_name_to_id(self, name: str) -> Optional[int]:
        speakers = self.get_speakers()
        if not speakers:
            return None
        for sid, sname in speakers.items():
            if sname == name:
                return sid
        return None

    @property
    def language(self) -> Optional[str]:
        return None

    # -- streaming capability (reference: core/src/lib.rs:118-130) ---------- #
    @property
    def supports_streaming_output(self) -> bool:
        return False

    def stream_synthesis(
        self, phonemes: str, chunk_size: int, chunk_padding: int
    ) -> Iterator[np.ndarray]:
        raise OperationError("this model does not support streaming output")
