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

from ..audio.samples import silence_samples
from ..core import Audio, PcmAudio, SonataModel


class DynamicBatcher:
    def __init__(self, model: SonataModel, max_batch: int = 64,
                 max_wait_ms: float = 3.0):
        self.model = model
        self.max_batch = max_batch
        self.max_wait = max_wait_ms / 1000.0
        # items: (phonemes, future, prosody triple or None, pcm,
        #         silence_ms or None)
        self._q: "queue.Queue[Optional[tuple]]" = queue.Queue()
        self._worker = threading.Thread(target=self._run, daemon=True,
                                        name="sonata_batcher")
        self._closed = False
        self._worker.start()

    def submit(self, phonemes: str,
               prosody: Optional[Sequence[float]] = None,
               pcm: bool = False,
               silence_ms: Optional[float] = None) -> "Future[Audio]":
        """Queue one sentence; the future resolves with its Audio.
        `prosody`: optional (speed, volume, pitch) applied to this request's
        row by the model (speak_batch(prosody=...)); rows of one batch may
        each carry their own.
        `pcm=True`: the future resolves with a PcmAudio (wire-format int16)
        with `silence_ms` of silence appended.  A bucket whose requests all
        want PCM runs one speak_batch_pcm; in a mixed bucket the PCM rows
        are converted on the host.  The bytes are the same either way."""
        if self._closed:
            raise RuntimeError("batcher closed")
        assert pcm or not silence_ms, "silence_ms rides with pcm requests"
        f: "Future[Audio]" = Future()
        self._q.put((phonemes, f, tuple(prosody) if prosody is not None
                     else None, bool(pcm), silence_ms))
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
        phonemes = [it[0] for it in bucket]
        prosody = [it[2] for it in bucket]
        kw = {"prosody": prosody} if any(
            p is not None for p in prosody) else {}
        try:
            if all(it[3] for it in bucket) and getattr(
                    self.model, "supports_device_pcm", False):
                audios = self.model.speak_batch_pcm(
                    phonemes, silence_ms=[it[4] for it in bucket], **kw)
            else:
                audios = self.model.speak_batch(phonemes, **kw)
                audios = [self._host_pcm(a, it[4]) if it[3] else a
                          for it, a in zip(bucket, audios)]
            for it, audio in zip(bucket, audios):
                it[1].set_result(audio)
        except BaseException as e:  # noqa: BLE001 - propagate to callers
            for it in bucket:
                if not it[1].done():
                    it[1].set_exception(e)

    @staticmethod
    def _host_pcm(audio: Audio, silence_ms: Optional[float]) -> PcmAudio:
        sil = (silence_samples(silence_ms, audio.info.sample_rate)
               if silence_ms else 0)
        return PcmAudio.from_audio(audio, sil)
