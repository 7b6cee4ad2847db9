"""Drop-in replacement for the onnxruntime.InferenceSession the reference builds at
vosk_tts/model.py:46 and calls at vosk_tts/synth.py:123-126:

    audio = self.model.onnx.run(None, args)[0]

`VitsSession.run(output_names, input_feed)` accepts the same feed dict — "input" int64 [B,T_x],
"input_lengths" int64 [B], "scales" float32 [3], "sid" int64 [B], and None-valued "bert" /
"phone_duration_extra" (synth.py:113-120; onnxruntime skips None feeds) — and returns
[float32 [B,1,1,S]] like the exported graph (training/vits2/onnx_export.py:65-72).
The arithmetic runs in hand-written HIP kernels behind the C ABI (include/vits_mi355.h); there
is no CPU path.  Thread-safe: the gRPC server shares one Synth across worker threads
(server/tts_server.py:39-40) and ctypes releases the GIL during the call.
"""
import itertools
import logging
import os
import threading

import numpy as np

from .capi import VitsLib
from .outopts import DOCUMENT_FEEDS, Tail, document_from_feed

log = logging.getLogger(__name__)


class _Pending:
    """one request waiting in the coalescer: its owner sleeps on `event` until a result (or an exception) is posted, or until it
    is handed a batch to lead"""
    __slots__ = ("key", "ids", "sid", "seed", "extra", "event", "result", "error", "lead")

    def __init__(self, key, ids, sid, seed, extra=None):
        self.key, self.ids, self.sid, self.seed, self.extra = key, ids, sid, seed, extra
        self.event = threading.Event()
        self.result = self.error = self.lead = None


class RequestCoalescer:
    """Merges concurrent single-utterance requests into solo batches (server shape: one Synth shared by a thread pool,
    server/tts_server.py:35-57 -- N threads each calling .run() for ONE utterance).

    Natural batching: a request that finds fewer than `max_inflight` engine calls running runs at once (the first of them on the
    persistent single-utterance path; nothing added to a lone client's latency).  Requests that arrive while `max_inflight` calls are in
    flight queue up; when one of those calls returns, its thread hands the queue's compatible requests (same output kind /
    conversion scale / output sample rate, at most `max_batch`; a request's scales ride with it as `extra`, include/vits_prosody.h) to the first waiter, which runs them as ONE padded VITS_FLAG_SOLO_BATCH call with per-request
    item seeds -- every item of a solo batch is its own single-utterance synthesis (own Philox streams, zeros beyond its own end), so
    what a request gets does not depend on what it was batched with -- and scatters the results.

    Gathering (`gather_us` > 0): a pool of N closed-loop clients otherwise settles into two alternating half-size batches (the clients of
    the batch that just returned are still on their way back when the next one is launched), and a batch of 8 costs 0.39 ms per request on
    the device where a batch of 16 costs 0.33.  So a leader that is about to launch FEWER requests than were recently present at the same
    time (`_peak`: the largest number of requests in flight + queued during the last 50 ms) waits up to `gather_us` for the stragglers.
    A lone client never waits (peak 1), a burst waits at most once per batch."""

    def __init__(self, run_batch, max_batch=32, max_inflight=1, gather_us=0):
        self._run_batch = run_batch  # (key, [(ids, sid, seed, extra), ...]) -> list of per-request results
        self.max_batch = int(max_batch)
        self.max_inflight = max(1, int(max_inflight))  # engine calls that may run at the same time (the GPU overlaps a few small forwards)
        self.gather_us = float(gather_us)
        self._lock = threading.Lock()
        self._cond = threading.Condition(self._lock)  # a gathering leader sleeps here; arrivals notify
        self._busy = 0
        self._queue = []
        self._in_calls = 0     # requests inside engine calls right now
        self._gathering = False  # a leader is waiting for stragglers: arrivals join its queue instead of starting calls of their own
        self._in_key = {}      # ... per key
        self._peaks = {}       # key -> (most requests of that key present at once recently, when that was last seen)
        self.calls = 0        # engine calls issued
        self.requests = 0     # requests served
        self.largest = 0      # largest batch so far
        self.split_retries = 0  # merged batches that failed and were re-run member by member
        self.gathered = 0     # launches that waited for stragglers

    # (lock held) requests of `key` present at once (inside engine calls + queued): a leader only ever takes its own key, so the
    # stragglers it may wait for are counted per key
    def _note_presence(self, now, key):
        present = self._in_key.get(key, 0) + sum(1 for p in self._queue if p.key == key)
        peak, t = self._peaks.get(key, (1, 0.0))
        if present >= peak or now - t > 0.05:
            self._peaks[key] = (max(present, 1), now)
        if len(self._peaks) > 64:  # (keys are (kind, scale, rate, marks, tail) tuples: bounded in practice, bounded here for good)
            self._peaks = {key: self._peaks[key]}

    def _gather(self, me, batch):
        """(lock held) `batch` (containing `me`) is about to be launched: wait for stragglers while it is smaller than the recent peak.
        Returns the batch to launch."""
        if self.gather_us <= 0:
            return batch
        import time

        now = time.perf_counter()
        self._note_presence(now, me.key)
        target = min(self.max_batch, self._peaks[me.key][0] - self._in_key.get(me.key, 0))
        if len(batch) >= target:
            return batch
        deadline = now + self.gather_us * 1e-6
        self.gathered += 1
        self._gathering = True
        try:
            return self._gather_wait(me, batch, target, deadline)
        finally:
            self._gathering = False

    def _gather_wait(self, me, batch, target, deadline):
        import time

        while True:
            more = [p for p in self._queue if p.key == me.key][:max(target, 1) - len(batch)]
            if more:
                taken = set(map(id, more))
                self._queue = [p for p in self._queue if id(p) not in taken]
                batch = batch + more
            now = time.perf_counter()
            if len(batch) >= target or now >= deadline:
                return batch
            self._cond.wait(deadline - now)

    def _promote(self):
        """(lock held) a leader has just taken its batch: requests it left in the queue (beyond its target, or of another key) must not
        wait for a call to finish when a call slot is free -- the queue's head becomes a leader of its own (and gathers in turn)."""
        if not self._queue or self._busy >= self.max_inflight or self._gathering:
            return None
        head = self._queue.pop(0)
        self._busy += 1
        head.lead = [head]
        return head

    def submit(self, key, ids, sid, seed, extra=None):
        """extra: what rides with the request into its batch without deciding which batch that is (the adapter: its scales)"""
        import time

        me = _Pending(key, ids, sid, seed, extra)
        promote = None
        with self._lock:
            if self._busy >= self.max_inflight or self._gathering:
                self._queue.append(me)
                if self.gather_us > 0:
                    self._note_presence(time.perf_counter(), key)
                self._cond.notify_all()
                batch = None
            else:
                self._busy += 1
                batch = self._gather(me, [me])
                self._in_calls += len(batch)
                if self.gather_us > 0:
                    self._in_key[key] = self._in_key.get(key, 0) + len(batch)
                promote = self._promote()
        if batch is not None and promote is not None:
            promote.event.set()
        if batch is None:
            me.event.wait()
            if me.lead is None:  # somebody else ran it
                if me.error is not None:
                    raise me.error
                return me.result
            with self._lock:
                batch = self._gather(me, me.lead)
                self._in_calls += len(batch)
                if self.gather_us > 0:
                    self._in_key[key] = self._in_key.get(key, 0) + len(batch)
                promote = self._promote()
            if promote is not None:
                promote.event.set()
        # this thread leads `batch` (which contains its own request)
        try:
            try:
                outs = self._run_batch(batch[0].key, [(p.ids, p.sid, p.seed, p.extra) for p in batch])
                for p, o in zip(batch, outs):
                    p.result = o
            except Exception as e:
                if len(batch) == 1:
                    me.error = e
                else:
                    # a merged batch failed: one bad request (token / speaker id out of range, ...) must not fail the unrelated
                    # requests it was merged with -- run the members one by one, each gets its own result or its own exception
                    self.split_retries += 1
                    try:
                        for p in batch:
                            try:
                                p.result = self._run_batch(p.key, [(p.ids, p.sid, p.seed, p.extra)])[0]
                            except Exception as e1:
                                p.error = e1
                    except BaseException as e2:  # interrupted in the middle of the retries (the sibling handler below does not cover this one)
                        for p in batch:
                            if p.result is None and p.error is None:
                                p.error = RuntimeError(f"batch leader interrupted: {e2!r}") if p is not me else e2
            except BaseException as e:  # KeyboardInterrupt / SystemExit in the leader: nobody may be left waiting
                for p in batch:
                    p.error = RuntimeError(f"batch leader interrupted: {e!r}") if p is not me else e
        finally:
            with self._lock:
                self.calls += 1
                self.requests += len(batch)
                self.largest = max(self.largest, len(batch))
                self._in_calls -= len(batch)
                if self.gather_us > 0:  # (the per-key presence count only feeds the gather window)
                    left = self._in_key.get(batch[0].key, 0) - len(batch)
                    if left > 0:
                        self._in_key[batch[0].key] = left
                    else:
                        self._in_key.pop(batch[0].key, None)  # a server that forwards client-chosen speech rates sees unboundedly many keys
                for p in batch:
                    if p.result is None and p.error is None:  # whatever happened above: a member never wakes up with nothing
                        p.error = RuntimeError("coalesced batch ended without a result for this request")
                nxt = None
                if self._queue:
                    head = self._queue[0]
                    take = [p for p in self._queue if p.key == head.key][:self.max_batch]
                    taken = set(map(id, take))
                    self._queue = [p for p in self._queue if id(p) not in taken]
                    head.lead = take
                    nxt = head
                else:
                    self._busy -= 1
            for p in batch:
                if p is not me:
                    p.event.set()
            if nxt is not None:
                nxt.event.set()
        if me.error is not None:
            raise me.error
        return me.result

# frame-bucket ("back") contexts the engine keeps per T_x bucket before it evicts the least recently used one (mirror of csrc/ctx_cache.hip.h VITS_BACKS_PER_FRONT)
BACK_SESSIONS_PER_FRONT = 6

_GRAPH_INPUTS = ("input", "input_lengths", "scales", "sid")
_OPTIONAL_NONE = ("bert", "phone_duration_extra")
# extension feeds (not part of the ONNX graph) used by parity tests
_EXT = ("vits.noise_dp", "vits.noise_prior", "vits.forced_durations", "vits.seed", "vits.solo", "vits.item_seeds", "vits.sample_rate", "vits.marks",
        "vits.loudness", "vits.peak", "vits.peak_ceiling", "vits.pitch", "vits.pitch_formants", "vits.limit", "vits.limit_lookahead_ms",
        "vits.limit_release_ms", "vits.item_scales", "vits.token_length_scale", "vits.token_pause", "vits.fit_frames", "vits.token_pitch",
        "vits.token_gain_db", "vits.pitch_range", "vits.watermark_key", "vits.watermark_depth_db",
        "vits.watermark_payload") + tuple(DOCUMENT_FEEDS)
# the prosody controls of a request (include/vits_prosody.h): feed key -> keyword of capi.VitsModel.synthesize*
_PROSODY = {"vits.item_scales": "item_scales", "vits.token_length_scale": "token_length_scale", "vits.token_pause": "token_pause",
            "vits.fit_frames": "fit_frames"}
# the contour of a request (include/vits_contour.h): feed key -> keyword of capi.VitsModel.synthesize*
_CONTOUR = {"vits.token_pitch": "token_pitch", "vits.token_gain_db": "token_gain_db"}


class RequestExtra(tuple):
    """What rides with a request through the coalescer without deciding its batch: the scales (the tuple itself) and, as an attribute,
    the payload of its mark (include/vits_watermark_payload.h; None: none)"""

    payload = None

    @classmethod
    def of(cls, scales, payload=None):
        me = cls(scales)
        me.payload = None if payload is None else int(np.asarray(payload).reshape(-1)[0])  # (one request: one value)
        return me


def ride_payloads(pk, tail, reqs, n_real):
    """the keywords of a coalesced call whose Tail says its payloads ride with the requests: one value for a lone request, one per item
    (the one-token dummies behind n_real: 0) for a batch"""
    from .capi import PAYLOAD_RIDES

    if tail.payload != PAYLOAD_RIDES:
        return pk
    vals = [getattr(r[3], "payload", None) or 0 for r in reqs[:n_real]] + [0] * (len(reqs) - n_real)
    return dict(pk, watermark_payload=vals[0] if len(reqs) == 1 else vals)


class _Arg:
    def __init__(self, name, typ, shape):
        self.name, self.type, self.shape = name, typ, shape


class VitsSession:
    def __init__(self, blob, device=0, lib=None, coalesce=True, max_batch=32, max_inflight=None):
        self._lib = lib or VitsLib()
        self._model = self._lib.create(blob, device)
        self.hp = self._model.hp
        self._seed = itertools.count(1)
        self._seed_lock = threading.Lock()
        # concurrent single-utterance run() / run_pcm16() calls are merged into solo batches (RequestCoalescer); coalesce=False:
        # every call goes to the engine on its own, as in rounds 1-3
        if max_inflight is None:
            # measured on MI355X (16 threads, 47-token requests, bench.py host_api.concurrent): 1 call in flight 1520 requests/s, 2-4: ~2000,
            # 8: 2200, no coalescing: 2110 -- the device overlaps a handful of single-utterance forwards (one of them on the persistent
            # programs); merging only starts beyond that, which also bounds the workspaces and streams a burst can pin
            max_inflight = int(os.environ.get("VITS_COALESCE_INFLIGHT", "8"))
        gather_us = float(os.environ.get("VITS_COALESCE_GATHER_US", "0"))
        self.coalescer = RequestCoalescer(self._run_solo_batch, max_batch, max_inflight, gather_us) if coalesce else None
        self._ps_timeouts = 0  # persistent-program timeouts already reported (persist_state)

    def persist_state(self, with_device=True):
        """State of the single-utterance persistent programs in this process (vits_persist_state): a poll timeout -- the device shared
        with another process, a transient -- puts single utterances on the ~1.5x slower launch path for a bounded interval, after which
        the programs are re-armed.  Logged at WARNING whenever the timeout count has grown since the last look."""
        st = self._model.persist_state(with_device)
        if st["timeouts"] > self._ps_timeouts:
            # process_owns_device is the outcome of the LAST call's lock lease (1 got it, -1 was refused, 0 not asked yet) and is only
            # known with a model handle: the periodic watcher (with_device=False) says nothing about it
            lock = (", last call " + {1: "got", -1: "was refused", 0: "has not asked for"}.get(st["process_owns_device"], "?") +
                    " the device's program lock") if with_device else ""
            log.warning("persistent programs timed out %d time(s) so far (re-armed %d time(s)); launch path for another %d ms%s",
                        st["timeouts"], st["rearms"], st["off_for_ms"], lock)
            self._ps_timeouts = st["timeouts"]
        return st

    def _watch(self):
        # cheap (process-wide counters, no device access): read through the C ABI every 256 requests
        self._n_req = getattr(self, "_n_req", 0) + 1
        if self._n_req & 255 == 0 and self._lib.is_device:
            try:
                self.persist_state(with_device=False)
            except Exception:  # diagnostics must never cost a request
                pass

    def _coalescable(self, feed, ids):
        """plain single-utterance requests only: no injected tensors, no pinned durations, no caller-chosen batch semantics.
        Returns the request's token count (> 0) when it may be merged, 0 otherwise -- a length outside (0, T] is NOT sliced here:
        such a request takes the direct call, whose C-side check answers VITS_ERR_ARG as it always did."""
        if not (self.coalescer is not None and ids.shape[0] == 1 and self.hp.bert_dim == 0 and
                not any(k in feed for k in ("vits.noise_dp", "vits.noise_prior", "vits.forced_durations", "vits.solo", "vits.item_seeds", "bert") + tuple(_PROSODY) + tuple(_CONTOUR))):
            return 0
        lens = np.asarray(feed["input_lengths"]).reshape(-1)
        if lens.shape[0] != 1:
            return 0
        n = int(lens[0])
        return n if 0 < n <= ids.shape[1] else 0

    def _run_solo_batch(self, key, reqs):
        """reqs: [(ids [1,T] int64, sid, seed, scales)] -> per request (audio-or-pcm [1,S_b], lengths [1]); one request: the plain call.
        The scales ride with the request (include/vits_prosody.h): requests that agree on them run as the batch they always were, requests
        that differ run as ONE solo batch with their scales as its item_scales."""
        # key: (kind "pcm" / "f32", pcm scale, rate: output sample rate in Hz, 0 = the voice's own, marks: the requests want their token
        # ends, include/vits_marks.h, tail: the outopts.Tail of the batch).  A batch has one rate, either every request of it gets a third
        # value or none does, and one tail, whose stages measure and apply per item: a request's result does not depend on what it
        # was batched with
        kind, scale, rate, marks, tail = key
        pk = ride_payloads(tail.kw(), tail, reqs, len(reqs))
        scales = np.array(reqs[0][3], np.float32)
        if len(reqs) == 1:
            ids, sid, seed = reqs[0][:3]
            lens = np.array([ids.shape[1]], np.int64)
            if kind == "pcm":
                return [self._model.synthesize_pcm16(ids, lens, scales, np.array([sid], np.int64), pcm_scale=scale, seed=seed, sample_rate=rate,
                                                     marks=marks, **pk)]
            return [self._model.synthesize(ids, lens, scales, np.array([sid], np.int64), seed=seed, sample_rate=rate, marks=marks, **pk)]
        # batch sizes come in powers of two (filled up with one-token dummies, whose padding tiles the ragged solo batch never
        # computes): every (batch size, length bucket) is a workspace and two captured graphs inside the engine, and a thread pool
        # produces every batch size between 1 and its own size
        n_real = len(reqs)
        n_pad = 1
        while n_pad < n_real:
            n_pad *= 2
        reqs = list(reqs) + [(np.ones((1, 1), np.int64), 0, 0, reqs[0][3])] * (n_pad - n_real)
        pk = ride_payloads(tail.kw(), tail, reqs, n_real)  # (requests of one key with different payloads: one call, watermark_payloads [B])
        if any(tuple(r[3]) != tuple(reqs[0][3]) for r in reqs):  # every item its own [noise_scale, length_scale, noise_scale_w]
            pk = dict(pk, item_scales=np.array([r[3] for r in reqs], np.float32))
        lens = np.array([r[0].shape[1] for r in reqs], np.int64)
        batch = np.zeros((len(reqs), int(lens.max())), np.int64)
        for b, r in enumerate(reqs):
            batch[b, :lens[b]] = r[0][0]
        sids = np.array([r[1] for r in reqs], np.int64)
        seeds = np.array([r[2] for r in reqs], np.uint64)
        if kind == "pcm":
            res = self._model.synthesize_pcm16(batch, lens, scales, sids, pcm_scale=scale, seed=int(seeds[0]), solo=True, item_seeds=seeds,
                                               sample_rate=rate, marks=marks, **pk)
        else:
            res = self._model.synthesize(batch, lens, scales, sids, seed=int(seeds[0]), solo=True, item_seeds=seeds, sample_rate=rate, marks=marks,
                                         **pk)
        out, ol = res[0], res[1]
        if marks:  # each request its own tokens' ends
            return [(out[b:b + 1, :int(ol[b])].copy(), ol[b:b + 1].copy(), res[2][b:b + 1, :int(lens[b])].copy()) for b in range(n_real)]
        return [(out[b:b + 1, :int(ol[b])].copy(), ol[b:b + 1].copy()) for b in range(n_real)]

    # -- onnxruntime.InferenceSession surface used by the reference ------------------------
    def get_inputs(self):
        args = [_Arg("input", "tensor(int64)", ["batch_size", "phonemes"]),
                _Arg("input_lengths", "tensor(int64)", ["batch_size"]),
                _Arg("scales", "tensor(float)", [3]),
                _Arg("sid", "tensor(int64)", ["batch_size"])]
        if self.hp.bert_dim > 0:  # BERT-conditioned flavour (vosk_tts/synth.py:88-99)
            args.append(_Arg("bert", "tensor(float)", ["batch_size", self.hp.bert_dim, "phonemes"]))
        return args

    def get_outputs(self):
        return [_Arg("output", "tensor(float)", ["batch_size", 1, 1, "time"])]

    def get_providers(self):
        return ["MI355XExecutionProvider"]

    def _validated(self, output_names, input_feed):
        if output_names is not None and list(output_names) != ["output"]:
            raise ValueError(f"unknown output names {output_names}")
        feed = {k: v for k, v in input_feed.items() if v is not None}  # ORT ignores None feeds
        for k in feed:
            if k == "bert" and self.hp.bert_dim > 0:
                continue  # this graph declares the input (BERT-conditioned VITS flavour)
            if k in _OPTIONAL_NONE:
                raise NotImplementedError(
                    f"feed '{k}': this VITS graph declares no such input (bert: voices whose blob carries enc_p.bert_proj; "
                    "phone_duration_extra: multistream voices only, SURVEY.md §8f rank 2-3)")
            if k not in _GRAPH_INPUTS and k not in _EXT:
                raise ValueError(f"Invalid input name: {k}")
        for k in _GRAPH_INPUTS + (("bert",) if self.hp.bert_dim > 0 else ()):
            if k not in feed and not (k == "sid" and self.hp.n_speakers <= 1):
                raise ValueError(f"Required input {k} is missing")
        ids = np.asarray(feed["input"])
        if ids.ndim != 2:
            raise ValueError("input must be int64 [batch, phonemes] (multistream [B,5,T] flavours are out of scope)")
        B = ids.shape[0]
        sid = np.asarray(feed.get("sid", np.zeros(B, np.int64))).reshape(-1)
        if sid.shape[0] == 1 and B > 1:
            sid = np.repeat(sid, B)
        seed = feed.get("vits.seed")
        if seed is None:
            with self._seed_lock:
                seed = next(self._seed)
        return feed, ids, sid, int(seed)

    def _rate(self, sample_rate):
        """output sample rate of a request -> 0 for None / 0 / the voice's own rate (those take the calls without a rate)"""
        rate = int(sample_rate or 0)
        if rate < 0:
            raise ValueError(f"sample_rate {rate}: must be positive, or None for the voice's own {self.hp.sampling_rate} Hz")
        return 0 if rate == self.hp.sampling_rate else rate

    def run_document(self, input_feed, scale=1.0, pcm16=True):
        """A document (include/vits_document.h): the feed of a batch -- "input" [B, T], "input_lengths" [B], "sid" [B], "bert" -- with at
        least one of the document feeds "vits.doc_gap_frames" int [B], "vits.doc_lead_frames", "vits.doc_fade_samples",
        "vits.doc_trim_db", "vits.doc_trim_keep"; its items are synthesised as a SOLO batch and joined on the device in front of the
        resampler, the loudness stage, the limiter and the int16 conversion.  -> (audio int16 or float32 [S], info): info["seg_start"] /
        ["seg_end"] int64 [B] in output samples, info["trim"] int32 [B, 2], and with "vits.marks" info["token_ends"] int64 [B, T].
        Every other extension feed of run() applies: the per-item ones per item, the output tail to the whole document."""
        feed, ids, sid, seed = self._validated(None, input_feed)
        doc = document_from_feed(self._lib, feed)
        if doc is None:
            raise ValueError("run_document: the feed names no document key (\"vits.doc_gap_frames\", ...)")
        for k in ("vits.noise_dp", "vits.noise_prior"):
            if k in feed:
                raise ValueError(f"feed '{k}' with a document: injected noise belongs to the parity calls")
        self._watch()
        audio, info = self._model.synthesize_document(
            ids, np.asarray(feed["input_lengths"]).reshape(-1), np.asarray(feed["scales"], np.float32).reshape(-1), sid, pcm=bool(pcm16),
            pcm_scale=float(scale), forced_durations=feed.get("vits.forced_durations"), seed=int(seed), item_seeds=feed.get("vits.item_seeds"),
            bert=feed.get("bert"), sample_rate=self._rate(feed.get("vits.sample_rate")), marks=self._marks(feed),
            **Tail.from_feed(self._lib, feed).kw(), **self._prosody(feed), **self._contour(feed), **doc)
        self.last_lengths = np.array([audio.shape[0]], np.int64)
        return audio, info

    def run(self, output_names, input_feed, run_options=None):
        """The document feeds ("vits.doc_gap_frames", ...; run_document): the batch of the feed comes back as ONE row [1, 1, 1, S].
        Extension feed "vits.sample_rate" (next to "vits.seed"): output rate in Hz; the time axis of the output is then in output
        samples (include/vits_resample.h).  Extension feed "vits.marks": True -- the result list gets a second entry, token_ends int64
        [B, T_x] in output samples (include/vits_marks.h).  Extension feeds "vits.loudness" / "vits.peak" / "vits.peak_ceiling": every
        item normalised to a LUFS or a peak target on the device, last in the chain (include/vits_loudness.h)."""
        feed, ids, sid, seed = self._validated(output_names, input_feed)
        if any(k in feed for k in DOCUMENT_FEEDS):
            audio, info = self.run_document(input_feed, pcm16=False)
            return [audio[None, None, None, :]] + ([info["token_ends"]] if "token_ends" in info else [])
        self._watch()
        rate = self._rate(feed.get("vits.sample_rate"))
        marks = self._marks(feed)
        n = self._coalescable(feed, ids)
        # (the loudness, limiter, pitch, intonation and watermark feeds; outopts.TAIL_FEEDS.  A coalesced request's payload rides with it)
        tail = Tail.from_feed(self._lib, feed, payload_rides=bool(n))
        if n:
            key = ("f32", 1.0, rate, marks, tail)
            res = self.coalescer.submit(key, np.ascontiguousarray(ids[:, :n], np.int64), int(sid[0]), int(seed), self._scales(feed))
            self.last_lengths = res[1]
            if marks:  # (the request's own tokens; columns beyond its length repeat the last end, as the C ABI pads them)
                return [res[0][:, None, None, :], self._pad_ends(res[2], ids.shape[1])]
            return [res[0][:, None, None, :]]
        res = self._model.synthesize(
            ids, np.asarray(feed["input_lengths"]).reshape(-1), np.asarray(feed["scales"], np.float32).reshape(-1), sid,
            noise_dp=feed.get("vits.noise_dp"), noise_prior=feed.get("vits.noise_prior"),
            forced_durations=feed.get("vits.forced_durations"), seed=int(seed), solo=bool(feed.get("vits.solo", False)),
            item_seeds=feed.get("vits.item_seeds"), bert=feed.get("bert"), sample_rate=rate, marks=marks,
            **tail.kw(), **self._prosody(feed), **self._contour(feed))
        self.last_lengths = res[1]
        return [res[0][:, None, None, :], res[2]] if marks else [res[0][:, None, None, :]]

    @staticmethod
    def _scales(feed):
        """the request's scales as the tuple that rides with it through the coalescer, and with them the payload of its mark"""
        return RequestExtra.of((float(v) for v in np.asarray(feed["scales"], np.float32).reshape(-1)), feed.get("vits.watermark_payload"))

    def _prosody(self, feed):
        """The prosody controls of a request (include/vits_prosody.h) -> keywords of the model's calls, none without one (the call as it
        was).  Feeds "vits.item_scales" float [B, 3], "vits.token_length_scale" float [B, T_x], "vits.token_pause" int32 [B, T_x] frames,
        "vits.fit_frames" int32 [B]; values the engine would refuse are refused here, before any device work (ValueError naming them)."""
        kw = {v: feed[k] for k, v in _PROSODY.items() if k in feed}
        if kw:
            from .prosody import check_controls

            self._lib._need_prosody()
            check_controls(np.asarray(feed["input_lengths"]).reshape(-1), forced="vits.forced_durations" in feed, **kw)
        return kw

    def _contour(self, feed):
        """The contour of a request (include/vits_contour.h) -> keywords of the model's calls, none without one (the call as it was).
        Feeds "vits.token_pitch" float [B, T_x] semitones and "vits.token_gain_db" float [B, T_x] dB; the model's call refuses values out
        of range before any device work (ValueError naming item, token and value)."""
        kw = {v: feed[k] for k, v in _CONTOUR.items() if k in feed}
        if kw:
            self._lib._need_contour()
        return kw

    def _marks(self, feed):
        """the "vits.marks" feed of a request -> bool; the CPU oracle has no marks, and says so"""
        marks = bool(feed.get("vits.marks", False))
        if marks:
            self._lib._need_marks()
        return marks

    @staticmethod
    def _pad_ends(ends, T):
        """token ends [1, n] of a request cut at its length -> [1, T], padded by the rule of include/vits_marks.h"""
        n = ends.shape[1]
        if n >= T:
            return ends
        return np.concatenate([ends, np.repeat(ends[:, -1:] if n else np.zeros((1, 1), np.int64), T - n, axis=1)], axis=1)

    def run_pcm16(self, input_feed, scale=1.0, return_lengths=False, sample_rate=None):
        """run() followed by `audio.squeeze() * scale` and Synth.audio_float_to_int16 (vosk_tts/synth.py:127-130), with the
        conversion done on the device (vits_synthesize_pcm16): returns int16 [B, S] -- bit-identical to converting run()'s
        float output with numpy, half the bytes over PCIe.  return_lengths: also return the per-item sample counts
        (concurrent callers must take them from the call, not from the shared `last_lengths` attribute).
        sample_rate: output rate in Hz (default: the feed's "vits.sample_rate", else the voice's own): the resampler converts in its
        epilogue, so the call launches as many kernels as at the voice's rate and copies rate_out / rate_in as many bytes.
        With the feed "vits.marks": True the result is a tuple that ends with token_ends int64 [B, T_x]: (pcm, token_ends), or
        (pcm, lengths, token_ends) with return_lengths.  The loudness feeds: as for run(); `scale` multiplies the normalised audio."""
        feed, ids, sid, seed = self._validated(None, input_feed)
        if any(k in feed for k in DOCUMENT_FEEDS):  # (run_document: the batch comes back as one row)
            if sample_rate is not None:
                input_feed = dict(input_feed, **{"vits.sample_rate": sample_rate})
            pcm, info = self.run_document(input_feed, scale=scale)
            res = (pcm[None, :],) + ((self.last_lengths,) if return_lengths else ()) + ((info["token_ends"],) if "token_ends" in info else ())
            return res if len(res) > 1 else res[0]
        self._watch()
        rate = self._rate(sample_rate if sample_rate is not None else feed.get("vits.sample_rate"))
        marks = self._marks(feed)
        n = self._coalescable(feed, ids)
        tail = Tail.from_feed(self._lib, feed, payload_rides=bool(n))
        if n:
            key = ("pcm", float(scale), rate, marks, tail)
            res = self.coalescer.submit(key, np.ascontiguousarray(ids[:, :n], np.int64), int(sid[0]), int(seed), self._scales(feed))
            pcm, lengths = res[0], res[1]
            self.last_lengths = lengths
            if marks:
                ends = self._pad_ends(res[2], ids.shape[1])
                return (pcm, lengths, ends) if return_lengths else (pcm, ends)
            return (pcm, lengths) if return_lengths else pcm
        res = self._model.synthesize_pcm16(
            ids, np.asarray(feed["input_lengths"]).reshape(-1), np.asarray(feed["scales"], np.float32).reshape(-1), sid,
            pcm_scale=float(scale), noise_dp=feed.get("vits.noise_dp"), noise_prior=feed.get("vits.noise_prior"),
            forced_durations=feed.get("vits.forced_durations"), seed=int(seed), solo=bool(feed.get("vits.solo", False)),
            item_seeds=feed.get("vits.item_seeds"), bert=feed.get("bert"), sample_rate=rate, marks=marks,
            **tail.kw(), **self._prosody(feed), **self._contour(feed))
        pcm, lengths = res[0], res[1]
        self.last_lengths = lengths
        if marks:
            return (pcm, lengths, res[2]) if return_lengths else (pcm, res[2])
        return (pcm, lengths) if return_lengths else pcm

    def run_stream(self, output_names, input_feed, chunk_frames=64, sample_rate=None, on_marks=None):
        """on_marks: called once with token_ends int64 [T_x] in the stream's output samples before the first chunk (vits_stream_marks).
        Streaming form of run() for ONE utterance (extension; the reference's transport is already
        `stream AudioChunk`, server/tts_service.proto:46-54): yields float32 [n] chunks of chunk_frames*256
        samples whose concatenation equals run(...)[0].squeeze() for the same feed (same "vits.seed").
        sample_rate (default: the feed's "vits.sample_rate"): output rate in Hz; chunk sizes then vary by one sample."""
        feed, ids, sid, seed = self._validated(output_names, input_feed)
        if any(k in feed for k in DOCUMENT_FEEDS):
            raise ValueError("a stream cannot take a document: the join and the stages behind it need every segment before the first chunk "
                             "(run() / run_pcm16() / run_document() take the \"vits.doc_*\" feeds)")
        Tail.from_feed(self._lib, feed).refuse_stream("VITS", "run() / run_pcm16() take")
        if any(k in feed for k in _CONTOUR):
            raise ValueError("a stream cannot be contoured: the position recurrence and the phase recursion need the whole utterance before "
                             "the first chunk (run() / run_pcm16() take \"vits.token_pitch\" / \"vits.token_gain_db\")")
        rate = self._rate(sample_rate if sample_rate is not None else feed.get("vits.sample_rate"))
        if ids.shape[0] != 1:
            raise ValueError("run_stream takes one utterance")
        n = int(np.asarray(feed["input_lengths"]).reshape(-1)[0])
        fd = feed.get("vits.forced_durations")
        nd = feed.get("vits.noise_dp")
        bert = feed.get("bert")  # BERT-conditioned flavour (synth.py:88-99): vits_stream_open takes it through opts->bert
        return self._model.stream(
            ids[:, :n], np.asarray(feed["scales"], np.float32).reshape(-1), int(sid[0]), chunk_frames=chunk_frames,
            noise_dp=None if nd is None else np.asarray(nd)[:, :, :n], noise_prior=feed.get("vits.noise_prior"),
            forced_durations=None if fd is None else np.asarray(fd)[:, :n], seed=seed,
            bert=None if bert is None else np.ascontiguousarray(np.asarray(bert, np.float32)[:, :, :n]), sample_rate=rate,
            on_marks=on_marks, **{k: (np.asarray(v)[:, :n] if k in ("token_length_scale", "token_pause") else v) for k, v in self._prosody(feed).items()})

    def warmup(self, max_tokens=128, frames_per_token=(2.0, 5.0), speaker_id=0, freeze_gc=False, typical_frames_per_token=3.0,
               stream_chunk_frames=None):
        """Pay the one-off costs of the graph-replayed host path before the first real request does (extension; onnxruntime has the same
        need and no such call): for every T_x bucket (multiples of 8) up to `max_tokens`, the frame buckets (multiples of 32) between
        frames_per_token[0] and [1] frames per token that lie closest to `typical_frames_per_token` -- at most BACK_SESSIONS_PER_FRONT - 1
        of them, the engine's per-T_x cap less one -- are synthesized once with pinned durations -- which lays out the workspaces, builds
        the persistent programs and captures the front / back graphs of those (T_x, T_y) buckets -- plus one free-running call.
        Returns (calls, seconds).  Requests outside the warmed buckets still work; they pay their bucket's capture (tens of
        milliseconds) on first use.
        stream_chunk_frames=<n> also opens and drains a stream (run_stream's engine path) of every T_x bucket TWICE, at the typical frame
        count: streams run the eager stage path on a pooled session, and the first two opens of a size cost 15 - 40 ms instead of the
        steady 5 (workspace allocation, then one more slow open after the first graph-replayed call: tools/stream_warm_probe.py).
        freeze_gc=True additionally runs gc.collect() + gc.freeze() at the end: CPython's older-generation passes over the heap of a
        process that has loaded its models stop every thread for tens of milliseconds (25-60 ms measured beside 1 ms requests,
        profiles/r5_m2_gc.txt); frozen, that heap is no longer traversed and the collector only looks at what requests allocate.
        Process-wide, hence opt-in."""
        import time

        t0 = time.perf_counter()
        calls = 0
        scales = np.array([0.8, 1.0, 0.8], np.float32)
        sid = np.array([speaker_id], np.int64)
        lo, hi = float(frames_per_token[0]), float(frames_per_token[1])
        for tx in range(8, max(int(max_tokens), 8) + 1, 8):
            ids = np.ones((1, tx), np.int64)
            lens = np.array([tx], np.int64)
            bert = np.zeros((1, self.hp.bert_dim, tx), np.float32) if self.hp.bert_dim > 0 else None
            first = max(32, (int(lo * tx) + 31) // 32 * 32)
            last = max(first, (int(hi * tx) + 31) // 32 * 32)
            # The engine keeps at most BACK_SESSIONS_PER_FRONT frame-bucket contexts per T_x bucket and evicts the least recently used
            # (engine_fastpath.hip.h back_get): warming more than that frees the first ones again (from T_x = 64 on there are 7+
            # buckets between 2 and 5 frames per token).  So: the buckets closest to `typical_frames_per_token`, at most one fewer
            # than the cap (the free-running call below may open one more), walked from the farthest to the closest -- the
            # likeliest bucket is the most recently used one when warm-up ends.
            centre = typical_frames_per_token * tx
            buckets = sorted(range(first, last + 1, 32), key=lambda ty: abs(ty - centre))[:BACK_SESSIONS_PER_FRONT - 1]
            for ty in sorted(buckets, key=lambda ty: -abs(ty - centre)) + [None]:
                dur = None
                if ty is not None:  # exactly ty frames over the tx tokens
                    dur = np.full((1, tx), ty // tx, np.int32)
                    dur[0, :ty % tx] += 1
                self._model.synthesize_pcm16(ids, lens, scales, sid, forced_durations=dur, seed=1, bert=bert)
                calls += 1
            if stream_chunk_frames:
                ty = max(1, int(round(typical_frames_per_token * tx)))
                dur = np.full((1, tx), ty // tx, np.int32)
                dur[0, :ty % tx] += 1
                for _ in range(2):
                    for _chunk in self._model.stream(ids, scales, speaker_id, chunk_frames=int(stream_chunk_frames), forced_durations=dur, seed=1, bert=bert):
                        pass
                    calls += 1
        if freeze_gc:
            import gc

            gc.collect()
            gc.freeze()
        return calls, time.perf_counter() - t0

    def close(self):
        self._model.close()
