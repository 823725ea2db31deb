"""Dynamic request batcher: coalesce concurrent synthesis requests into
padded GPU batches.

The reference serves one ort session.run per sentence (rayon threads,
synth/src/lib.rs:316-320).  On an MI355X the GPU wants batched work:
this scheduler queues incoming sentences and a worker drains up to
`max_batch` of them (or whatever arrived within `max_wait_ms`) into ONE
`speak_batch` call — the serving-side counterpart of SURVEY.md §7 step 5
("scheduler balancing 512 concurrent utterances").  Per-utterance
seeding keeps every result independent of batch composition, so
batching is invisible to callers.
"""

from __future__ import annotations

import queue
import threading
from concurrent.futures import Future
from typing import List, Optional, Sequence

from ..audio.g711 import check_encoding
from ..audio.resample import check_rate, is_identity, resample_poly
from ..audio.samples import silence_samples
from ..core import Audio, AudioInfo, PcmAudio, SonataModel


def _check_synthesis(model, synthesis):
    """A request's own SynthesisConfig, validated by the model at submit
    time (ValueError) and copied; None stays None: the model's config at
    the time the batch runs."""
    if synthesis is None:
        return None
    check = getattr(model, "check_synthesis_config", None)
    if check is not None:
        check(synthesis)
    return synthesis.copy()


def _synthesis_key(cfg):
    if cfg is None:
        return None
    return (cfg.speaker_id, float(cfg.noise_scale), float(cfg.length_scale),
            float(cfg.noise_w))


def _by_synthesis(items, cfg_of):
    """items grouped by config, first-seen order: [(cfg or None, [items])]"""
    groups = {}
    for it in items:
        cfg = cfg_of(it)
        groups.setdefault(_synthesis_key(cfg), (cfg, []))[1].append(it)
    return list(groups.values())


class _config_set:
    """Set the model's voice-wide config around one call: the route for a
    model without supports_row_synthesis."""

    def __init__(self, model, cfg):
        self.model, self.cfg = model, cfg

    def __enter__(self):
        if self.cfg is not None:
            self.saved = self.model.get_synthesis_config()
            self.model.set_synthesis_config(self.cfg)

    def __exit__(self, *exc):
        if self.cfg is not None:
            self.model.set_synthesis_config(self.saved)
        return False


class DynamicBatcher:
    def __init__(self, model: SonataModel, max_batch: int = 64,
                 max_wait_ms: float = 3.0):
        self.model = model
        self.max_batch = max_batch
        self.max_wait = max_wait_ms / 1000.0
        # items: (phonemes, future, prosody triple or None, pcm,
        #         silence_ms or None, output sample rate or None,
        #         wire encoding, SynthesisConfig or None)
        self._q: "queue.Queue[Optional[tuple]]" = queue.Queue()
        self._worker = threading.Thread(target=self._run, daemon=True,
                                        name="sonata_batcher")
        self._closed = False
        self._worker.start()

    def submit(self, phonemes: str,
               prosody: Optional[Sequence[float]] = None,
               pcm: bool = False,
               silence_ms: Optional[float] = None,
               sample_rate: Optional[int] = None,
               encoding: Optional[str] = None,
               synthesis=None) -> "Future[Audio]":
        """Queue one sentence; the future resolves with its Audio.
        `prosody`: optional (speed, volume, pitch) applied to this request's
        row by the model (speak_batch(prosody=...)); rows of one batch may
        each carry their own.
        `pcm=True`: the future resolves with a PcmAudio (wire-format int16)
        with `silence_ms` of silence appended.  A bucket whose requests all
        want PCM runs one speak_batch_pcm; in a mixed bucket the PCM rows
        are converted on the host.  The bytes are the same either way.
        `sample_rate`: optional output rate of this request's row; it rides
        with the request as the prosody triple does, and requests with
        different rates still share one speak_batch* call.  A rate the
        filter does not serve raises ValueError here.
        `encoding`: optional wire encoding of a pcm request ("pcm16",
        "ulaw", "alaw"); it rides with the request too, and requests with
        different encodings still share one speak_batch_pcm.  Anything else
        raises ValueError here.
        `synthesis`: optional SynthesisConfig (speaker and scales) of this
        request alone; it rides with the request as the prosody triple does,
        and requests with different speakers or scales still share one
        speak_batch* call (speak_batch(synthesis=...)).  None: the model's
        config when the batch runs.  A speaker or scale the model refuses
        raises ValueError here.  A model without supports_row_synthesis gets
        the bucket group by group, each with its config set around it."""
        if self._closed:
            raise RuntimeError("batcher closed")
        synthesis = _check_synthesis(self.model, synthesis)
        assert pcm or not silence_ms, "silence_ms rides with pcm requests"
        encoding = check_encoding(encoding)
        assert pcm or encoding == "pcm16", "encoding rides with pcm requests"
        if sample_rate is not None:
            native = self.model.audio_output_info().sample_rate
            if is_identity(native, sample_rate):
                sample_rate = None
            else:
                check_rate(native, sample_rate)
                sample_rate = int(sample_rate)
        f: "Future[Audio]" = Future()
        self._q.put((phonemes, f, tuple(prosody) if prosody is not None
                     else None, bool(pcm), silence_ms, sample_rate,
                     encoding, synthesis))
        return f

    def synthesize(self, phonemes: str) -> Audio:
        return self.submit(phonemes).result()

    def close(self) -> None:
        self._closed = True
        self._q.put(None)
        self._worker.join(timeout=10)

    # ------------------------------------------------------------------ #
    def _run(self) -> None:
        while True:
            item = self._q.get()
            if item is None:
                return
            batch: List[tuple] = [item]
            # drain whatever arrives within the wait window
            deadline = None
            while len(batch) < self.max_batch:
                try:
                    timeout = self.max_wait if deadline is None else deadline
                    nxt = self._q.get(timeout=timeout)
                except queue.Empty:
                    break
                if nxt is None:
                    self._flush(batch)
                    return
                batch.append(nxt)
                deadline = 0.0  # after the first wait, drain non-blocking
            self._flush(batch)

    def _flush(self, batch: List[tuple]) -> None:
        # Length-bucketed sub-batches: padded batching costs compute
        # proportional to the LONGEST utterance, so a 3-word request
        # coalesced with a 40-word one would pay 10x.  Sort by length
        # and cut where the next item is >2x the bucket's minimum.
        batch = sorted(batch, key=lambda it: len(it[0]))
        start = 0
        for i in range(1, len(batch) + 1):
            if i == len(batch) or (
                    len(batch[i][0]) > 2 * max(len(batch[start][0]), 8)):
                self._run_bucket(batch[start:i])
                start = i

    def _run_bucket(self, bucket: List[tuple]) -> None:
        synth = [it[7] for it in bucket]
        if all(c is None for c in synth):
            return self._run_rows(bucket)
        if getattr(self.model, "supports_row_synthesis", False):
            return self._run_rows(bucket, synth)
        for cfg, group in _by_synthesis(bucket, lambda it: it[7]):
            try:
                with _config_set(self.model, cfg):
                    self._run_rows(group)
            except BaseException as e:  # noqa: BLE001 - propagate to callers
                for it in group:
                    if not it[1].done():
                        it[1].set_exception(e)

    def _run_rows(self, bucket: List[tuple], synthesis=None) -> None:
        phonemes = [it[0] for it in bucket]
        prosody = [it[2] for it in bucket]
        kw = {"prosody": prosody} if any(
            p is not None for p in prosody) else {}
        if synthesis is not None:
            kw["synthesis"] = synthesis
        rates = [it[5] for it in bucket]
        host_rate = False
        if any(r is not None for r in rates):
            if getattr(self.model, "supports_output_rate", False):
                kw["sample_rate"] = rates
            else:
                host_rate = True  # converted below, after the float batch
        try:
            if all(it[3] for it in bucket) and not host_rate and getattr(
                    self.model, "supports_device_pcm", False):
                encs = [it[6] for it in bucket]
                if any(e != "pcm16" for e in encs):
                    kw["encoding"] = encs
                audios = self.model.speak_batch_pcm(
                    phonemes, silence_ms=[it[4] for it in bucket], **kw)
            else:
                audios = self.model.speak_batch(phonemes, **kw)
                if host_rate:
                    audios = [self._host_rate(a, r)
                              for a, r in zip(audios, rates)]
                audios = [self._host_pcm(a, it[4], it[6]) if it[3] else a
                          for it, a in zip(bucket, audios)]
            for it, audio in zip(bucket, audios):
                it[1].set_result(audio)
        except BaseException as e:  # noqa: BLE001 - propagate to callers
            for it in bucket:
                if not it[1].done():
                    it[1].set_exception(e)

    @staticmethod
    def _host_rate(audio: Audio, rate: Optional[int]) -> Audio:
        if rate is None:
            return audio
        return Audio(resample_poly(audio.samples, audio.info.sample_rate,
                                   rate),
                     AudioInfo(sample_rate=rate), audio.inference_ms)

    @staticmethod
    def _host_pcm(audio: Audio, silence_ms: Optional[float],
                  encoding: str = "pcm16") -> PcmAudio:
        sil = (silence_samples(silence_ms, audio.info.sample_rate)
               if silence_ms else 0)
        return PcmAudio.from_audio(audio, sil, encoding)


class _StreamHandle:
    """One stream of a StreamBatcher: its request, its chunk queue and,
    once opened, its model state."""

    __slots__ = ("phonemes", "chunk_size", "chunk_padding", "pcm", "q",
                 "cancelled", "state", "prosody", "sample_rate", "encoding",
                 "synthesis")

    def __init__(self, phonemes, chunk_size, chunk_padding, pcm,
                 prosody=None, sample_rate=None, encoding="pcm16",
                 synthesis=None):
        self.phonemes = phonemes
        self.synthesis = synthesis
        self.encoding = encoding
        self.prosody = tuple(prosody) if prosody is not None else None
        self.sample_rate = sample_rate
        self.chunk_size = int(chunk_size)
        self.chunk_padding = int(chunk_padding)
        self.pcm = bool(pcm)
        self.q: "queue.Queue" = queue.Queue()
        self.cancelled = False
        self.state = None

    @property
    def kind(self) -> int:
        """Output dtype of the stream's chunks: 0 float32, 1 int16, 2 uint8
        (G.711, either law)."""
        if self.encoding != "pcm16":
            return 2
        return 1 if self.pcm else 0

    def window(self) -> int:
        spec = self.state.next_spec
        return spec.mel_end - spec.mel_start


class _StreamIter:
    """Iterator over one stream's chunks.  close() (or dropping the
    iterator) takes the stream out of the batcher at its next tick."""

    _DONE = object()

    def __init__(self, handle: _StreamHandle):
        self._h = handle
        self._ended = False

    def __iter__(self):
        return self

    def __next__(self):
        if self._ended:
            raise StopIteration
        item = self._h.q.get()
        if item is self._DONE:
            self._ended = True
            raise StopIteration
        if isinstance(item, BaseException):
            self._ended = True
            raise item
        return item

    def close(self) -> None:
        self._ended = True
        self._h.cancelled = True

    def __del__(self):
        if not self._ended:
            self._h.cancelled = True


class StreamBatcher:
    """Coalesce concurrent realtime streams on one voice into shared chunk
    decodes: the streaming counterpart of DynamicBatcher.

    `open` queues a sentence and returns the iterator of its chunks.  One
    worker owns the live streams.  Each tick it admits what is queued
    (waiting `max_wait_ms` for company only when nothing is live), opens the
    newcomers in ONE model.stream_open (one batched encoder call), and
    advances every live stream by one chunk with model.stream_round: one
    decode per bucket of similar window length.  Streams join and leave
    between ticks; per-utterance seeding keeps each stream's audio
    independent of what it shares a round with."""

    def __init__(self, model: SonataModel, max_streams: int = 64,
                 max_wait_ms: float = 2.0):
        self.model = model
        self.max_streams = max_streams
        self.max_wait = max_wait_ms / 1000.0
        self._q: "queue.Queue[Optional[_StreamHandle]]" = queue.Queue()
        self._closed = False
        self._worker = threading.Thread(target=self._run, daemon=True,
                                        name="sonata_stream_batcher")
        self._worker.start()

    def open(self, phonemes: str, chunk_size: int = 45,
             chunk_padding: int = 3, pcm: bool = False, prosody=None,
             sample_rate: Optional[int] = None,
             encoding: Optional[str] = None, synthesis=None):
        """Start one stream; returns the iterator of its chunks (float32
        arrays, or int16 with pcm=True), those model.stream_synthesis
        yields for the same arguments.
        `prosody`: optional (speed, volume, pitch) applied continuously
        over the stream by the model (stream_open(prosody=...)); streams of
        one round may each carry their own.  The chunks then concatenate to
        the one-shot prosody of the plain stream; rounds in which the
        stretcher emits nothing yield no chunk.
        `sample_rate`: optional output rate of this stream, converted by
        the model inside the shared round (stream_open(sample_rate=...));
        streams of one round may each carry their own.  The chunks then
        concatenate to the conversion of the whole stream, and rounds in
        which the filter emits nothing yield no chunk.  A rate the filter
        does not serve raises ValueError here.
        `encoding`: "ulaw" or "alaw" makes the chunks uint8 G.711 codes
        (model.stream_round(encoding=...): the codes of the int16 chunks
        pcm=True gives); mu-law and A-law streams share a round.  None or
        "pcm16" changes nothing; anything else raises ValueError here.
        `synthesis`: optional SynthesisConfig of this stream alone; streams
        with different speakers or scales still share one model.stream_open
        (stream_open(synthesis=...)).  None: the model's config when the
        stream is opened.  What the model refuses raises ValueError here.  A
        model without supports_row_synthesis opens the newcomers group by
        group, each with its config set around the call."""
        if self._closed:
            raise RuntimeError("stream batcher closed")
        synthesis = _check_synthesis(self.model, synthesis)
        encoding = check_encoding(encoding)
        if sample_rate is not None:
            native = self.model.audio_output_info().sample_rate
            if is_identity(native, sample_rate):
                sample_rate = None
            else:
                check_rate(native, sample_rate)
                sample_rate = int(sample_rate)
        h = _StreamHandle(phonemes, chunk_size, chunk_padding, pcm, prosody,
                          sample_rate, encoding, synthesis)
        self._q.put(h)
        return _StreamIter(h)

    def close(self) -> None:
        """End the worker; streams still running end with an error."""
        self._closed = True
        self._q.put(None)
        self._worker.join(timeout=10)

    # ------------------------------------------------------------------ #
    def _admit(self, n_live: int):
        """Handles to open this tick, and whether close() was seen."""
        room = self.max_streams - n_live
        new: List[_StreamHandle] = []
        if room <= 0:
            return new, False
        if n_live == 0:
            first = self._q.get()  # idle: sleep until somebody arrives
            if first is None:
                return new, True
            new.append(first)
        wait = self.max_wait if n_live == 0 else 0.0
        while len(new) < room:
            try:
                nxt = self._q.get(timeout=wait) if wait else \
                    self._q.get_nowait()
            except queue.Empty:
                break
            if nxt is None:
                return new, True
            new.append(nxt)
            wait = 0.0  # after the first wait, drain non-blocking
        return new, False

    def _fail(self, handles, exc: BaseException) -> None:
        states = [h.state for h in handles if h.state is not None]
        if states:
            try:
                self.model.stream_close(states)
            except Exception:  # noqa: BLE001 - the first error is the news
                pass
        for h in handles:
            h.q.put(exc)

    def _open(self, new: List[_StreamHandle]) -> List[_StreamHandle]:
        new = [h for h in new if not h.cancelled]
        opened: List[_StreamHandle] = []
        # one stream_open per chunk_padding (in practice: one)
        rows = getattr(self.model, "supports_row_synthesis", False)
        for pad in sorted({h.chunk_padding for h in new}):
            padded = [h for h in new if h.chunk_padding == pad]
            if rows or all(h.synthesis is None for h in padded):
                groups = [(None, padded)]
            else:
                groups = _by_synthesis(padded, lambda h: h.synthesis)
            for cfg, group in groups:
                try:
                    kw = {"prosody": [h.prosody for h in group]} if any(
                        h.prosody is not None for h in group) else {}
                    if any(h.sample_rate is not None for h in group):
                        kw["sample_rate"] = [h.sample_rate for h in group]
                    if rows and any(h.synthesis is not None for h in group):
                        kw["synthesis"] = [h.synthesis for h in group]
                    with _config_set(self.model, cfg):
                        states = self.model.stream_open(
                            [h.phonemes for h in group],
                            [h.chunk_size for h in group], pad, **kw)
                except BaseException as e:  # noqa: BLE001 - reaches callers
                    self._fail(group, e)
                    continue
                for h, s in zip(group, states):
                    h.state = s
                opened.extend(group)
        return opened

    @staticmethod
    def _buckets(live: List[_StreamHandle]) -> List[List[_StreamHandle]]:
        """Shortest windows first, cut where the next window is more than
        twice the bucket's shortest (DynamicBatcher._flush's rule on window
        length): a newcomer's 45-frame chunk neither pays for nor waits
        behind a 225-frame one.  Float, int16 and 8-bit streams decode
        apart (a round has one output dtype); both laws share a round."""
        out = []
        for kind in (0, 1, 2):
            part = sorted((h for h in live if h.kind == kind),
                          key=_StreamHandle.window)
            start = 0
            for i in range(1, len(part) + 1):
                if i == len(part) or (
                        part[i].window() > 2 * max(part[start].window(), 8)):
                    out.append(part[start:i])
                    start = i
        out.sort(key=lambda b: b[0].window())
        return out

    def _round(self, bucket: List[_StreamHandle]) -> List[_StreamHandle]:
        """One decode for the bucket; returns the handles still live."""
        try:
            kw = ({"encoding": [h.encoding for h in bucket]}
                  if bucket[0].kind == 2 else {})
            chunks = self.model.stream_round([h.state for h in bucket],
                                             pcm=bucket[0].pcm, **kw)
        except BaseException as e:  # noqa: BLE001 - reaches the callers
            self._fail(bucket, e)
            return []
        by_state = {id(h.state): h for h in bucket}
        for state, chunk in chunks:
            h = by_state[id(state)]
            if len(chunk) or (h.prosody is None
                              and h.sample_rate is None):
                h.q.put(chunk)
        still = []
        for h in bucket:
            if h.state.done:
                h.q.put(_StreamIter._DONE)
            else:
                still.append(h)
        return still

    def _run(self) -> None:
        live: List[_StreamHandle] = []
        while True:
            new, closing = self._admit(len(live))
            if new:
                live.extend(self._open(new))
            gone = [h for h in live if h.cancelled]
            if gone:
                self.model.stream_close([h.state for h in gone])
                live = [h for h in live if not h.cancelled]
            if closing:
                self._fail(live, RuntimeError("stream batcher closed"))
                return
            nxt: List[_StreamHandle] = []
            for bucket in self._buckets(live):
                nxt.extend(self._round(bucket))
            live = nxt
