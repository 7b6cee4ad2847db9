"""Host-side batching for multi-utterance synthesis: the path shards by utterance
with no exchange step, so multi-GPU means independent replicas fed with balanced shards.

`plan_shards` sorts requests by token count and deals them greedily (longest first) to the shard
with the least predicted work, so padded batches stay tight and ranks finish together;
`pad_batch` builds the [B,T_x] feed of one shard; `scatter_results` restores request order.
No collective is needed on the data path: each rank reads the same request list and keeps its
own shard; only the small int16 PCM results travel back (over the launcher's channel of choice).
"""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np


def predicted_cost(n_tokens, frames_per_token=3.0):
    """Relative work of one utterance: decoder+flow scale with frames, encoder with tokens
    (SURVEY.md §8a totals: 162.4 MFLOP/frame vs 14.4 MFLOP/token)."""
    n_tokens = np.asarray(n_tokens, dtype=np.float64)
    return 162.4 * frames_per_token * n_tokens + 14.4 * n_tokens


def plan_shards(lengths, n_shards, max_batch=None):
    """lengths: tokens per request.  Returns n_shards lists of request indices (each sorted by
    descending length), balanced by predicted cost; max_batch caps items per shard per round."""
    lengths = np.asarray(lengths)
    order = np.argsort(-lengths, kind="stable")
    cost = predicted_cost(lengths)
    load = np.zeros(n_shards)
    shards = [[] for _ in range(n_shards)]
    for i in order:
        cand = [s for s in range(n_shards) if max_batch is None or len(shards[s]) < max_batch]
        if not cand:
            raise ValueError("max_batch * n_shards < number of requests")
        s = min(cand, key=lambda k: (load[k], k))
        shards[s].append(int(i))
        load[s] += cost[i]
    return shards


def pad_batch(token_lists, indices, pad_id=0):
    """-> ids int64 [B,T_x] (padded), lengths int64 [B] for the requests `indices`."""
    lens = np.array([len(token_lists[i]) for i in indices], dtype=np.int64)
    Tx = int(lens.max()) if len(indices) else 0
    ids = np.full((len(indices), Tx), pad_id, dtype=np.int64)
    for r, i in enumerate(indices):
        ids[r, :lens[r]] = token_lists[i]
    return ids, lens


def scatter_results(n_requests, shards, shard_outputs):
    """shard_outputs[s][r] is the result of request shards[s][r]; returns them in request order."""
    out = [None] * n_requests
    for idx, res in zip(shards, shard_outputs):
        for i, r in zip(idx, res):
            out[i] = r
    if any(o is None for o in out):
        raise ValueError("some requests were not assigned to any shard")
    return out


# Smallest part of a shard whose front end runs as one batched BERT call (Synth.front_batch).  profiles/bert_batch_bench.txt
# (tools/bert_batch_bench.py, rubert-base geometry, sentences of 9 - 40 tokens): one sentence is a tie (0.83 ms either way: the solo
# call replays a captured graph, the batched one launches eagerly), from two sentences on the batched call wins (1.5x at 2, 2.0x at 4,
# 2.9x at 8, 4.0x at 16, 3.5x at 32 against as many solo calls), so a part of one request keeps the per-request front end.
BATCHED_FRONT_MIN = 2


def tail_part(tail_feed, part):
    """the tail's feed fragment for the requests `part` of a call: what is one value per call as it is, a per-request
    "vits.watermark_payload" cut to the part"""
    feed = dict(tail_feed or {})
    payload = feed.get("vits.watermark_payload")
    if isinstance(payload, tuple):
        feed["vits.watermark_payload"] = [payload[i] for i in part]
    return feed


class MultiDeviceSynth:
    """Batched multi-utterance synthesis over N device replicas in ONE process (BASELINE north_star: "Batched multi-utterance
    synthesis shards across the 8 GPUs of one node as embarrassingly-parallel data replicas"; SURVEY.md 8e: "one host thread
    per device; results gathered on host in original order").  The seam is where the reference's gRPC server shares one Synth
    across a thread pool (server/tts_server.py:37-40,56-63): here each device holds its own `Model` replica (weights resident
    once per device) and a worker thread; a list of requests is front-ended on the host (the same g2p as `Synth`), sharded by
    predicted cost (`plan_shards`), every shard runs as padded batches of at most `max_batch` through the C ABI
    (vits_synthesize_pcm16, int16 conversion on the device) and the results come back in request order.

    Every request is synthesized as an independent utterance (VITS_FLAG_SOLO_BATCH) with its own noise seed, so the samples a
    request gets do not depend on how many devices there are or on what else was in its batch.  No collective anywhere: ctypes
    drops the GIL during the call, the devices run concurrently.

        mds = MultiDeviceSynth(model_path, devices=[0, 1, 2, 3, 4, 5, 6, 7])
        pcm = mds.synth_batch(["...", "..."], speaker_ids=2)        # list of int16 arrays, request order
    """

    def __init__(self, model_path=None, devices=None, model_name=None, lang=None, max_batch=32, batched_front=True):
        from .model import Model
        from .synth import Synth

        if devices is None:
            from .capi import VitsLib

            n = VitsLib().device_count()
            devices = list(range(max(n, 1)))
        if not devices:
            raise ValueError("no devices")
        self.devices = list(devices)
        self.max_batch = int(max_batch)
        # BERT-conditioned families: front end of a whole part in one Synth.front_batch call (one padded BERT forward, the phoneme
        # feed gathered on the device) where the voice's BERT session has the batched entry points; False keeps the per-request
        # front end (get_word_bert per text)
        self.batched_front = bool(batched_front)
        self.models = [Model(model_path=model_path, model_name=model_name, lang=lang, device=d) for d in self.devices]
        # the three voice families of vosk_tts/synth.py:64-103 behind the same door:
        #   "vits"        plain VITS (g2p_noembed -> token ids)                              -> vits_synthesize_pcm16, solo batch
        #   "vits_bert"   BERT-conditioned VITS (get_word_bert + g2p / g2p_noblank, synth.py:88-99) -> the same with a padded `bert` feed
        #   "multistream" StableTTS / Matcha voices (five id streams + BERT rows, synth.py:64-87)  -> stts_synthesize_batch per replica
        m0 = self.models[0]
        mt = str(m0.config.get("model_type") or "")
        if mt.startswith("multistream"):
            self.family = "multistream"
        elif getattr(m0.onnx, "hp", None) is not None and m0.onnx.hp.bert_dim > 0:
            if m0.tokenizer is None:
                raise NotImplementedError("this voice is BERT-conditioned (hparams.bert_dim > 0) but has no bert/ directory next to it")
            self.family = "vits_bert"
        else:
            self.family = "vits"
        self.synths = [Synth(m) for m in self.models]
        self._replica_locks = [threading.Lock() for _ in self.models]  # one batch at a time per replica (shared pool threads)
        self._pool = ThreadPoolExecutor(max_workers=len(self.devices), thread_name_prefix="vits-dev")
        self._seed = 0
        self._lock = threading.Lock()

    def close(self):
        self._pool.shutdown(wait=True)
        for m in self.models:
            m.onnx.close()
            if getattr(m, "bert_onnx", None) is not None and hasattr(m.bert_onnx, "close"):
                m.bert_onnx.close()

    @staticmethod
    def _pcm16_marks(sess, feed, scale, sample_rate, marks):
        """run_pcm16 of one padded batch -> (pcm, lengths, token_ends or None); marks: the feed gets "vits.marks" (include/vits_marks.h)"""
        if not marks:
            return sess.run_pcm16(feed, scale, return_lengths=True, sample_rate=sample_rate) + (None,)
        return sess.run_pcm16(dict(feed, **{"vits.marks": True}), scale, return_lengths=True, sample_rate=sample_rate)

    @staticmethod
    def _scales_feed(scales, part):
        """the feed entries of the scales for the requests `part`: one triple for the call, or -- where noise_level / speech_rate /
        duration_noise_level came per request -- every request's own triple as the item scales of the solo batch (include/vits_prosody.h)"""
        if scales.ndim == 1:
            return {"scales": scales}
        return {"scales": scales[part[0]], "vits.item_scales": np.ascontiguousarray(scales[list(part)])}

    @staticmethod
    def _item(pcm, n, ends, n_tokens):
        """one request's result: its samples, and with marks (samples, its own tokens' ends)"""
        a = pcm[:int(n)].copy()
        return a if ends is None else (a, ends[:int(n_tokens)].copy())

    def _run_shard(self, r, token_lists, idx, sids, scales, scale, seeds, sample_rate=None, marks=False, tail_feed=None):
        """the requests `idx` on replica r, in batches of <= max_batch (already sorted by descending length) -> list of int16 arrays
        (marks: of (int16 array, token ends)).  tail_feed: the tail's feed fragment of the batch (outopts.TAIL_FEEDS: "vits.loudness",
        "vits.pitch", "vits.watermark_key", ...), merged into every feed; the engine applies every stage per item"""
        out = []
        sess = self.models[r].onnx
        for k in range(0, len(idx), self.max_batch):
            part = idx[k:k + self.max_batch]
            ids, lens = pad_batch(token_lists, part)
            feed = {"input": ids, "input_lengths": lens, **self._scales_feed(scales, part), "sid": np.array([sids[i] for i in part], np.int64),
                    "bert": None, "phone_duration_extra": None, "vits.solo": True,
                    "vits.item_seeds": np.array([seeds[i] for i in part], np.uint64), **tail_part(tail_feed, part)}
            with self._replica_locks[r]:  # concurrent synth_batch() calls do not interleave on one replica
                pcm, lengths, ends = self._pcm16_marks(sess, feed, scale, sample_rate, marks)  # lengths of THIS call (not the shared attribute)
            out.extend(self._item(pcm[j], lengths[j], None if ends is None else ends[j], lens[j]) for j in range(len(part)))
        return out

    def synth_batch(self, texts, speaker_ids=0, noise_level=None, speech_rate=None, duration_noise_level=None, scale=None, seeds=None,
                    sample_rate=None, denoiser_strength=None, marks=False, loudness=None, peak=None, peak_ceiling=None, pitch=None,
                    preserve_formants=None, limit=None, limit_lookahead_ms=None, limit_release_ms=None, pitch_range=None, watermark=None,
                    watermark_depth_db=None, watermark_payload=None):
        """`watermark_payload`: 16 bits inside the mark (include/vits_watermark_payload.h), one int for the call or one per request: the
        requests of a shard still share their batches, each item with its own payload.
        texts: list of str -> list of int16 PCM arrays (22.05 kHz), one per request, in request order.  marks=True: a list of
        (audio, marks.SpeechMarks) per request instead (as Synth.synth_audio(..., marks=True)), through every shard path.  `seeds`: optional
        per-request noise seeds (default: a running counter), `speaker_ids`: one id or one per request.  `noise_level` / `speech_rate` /
        `duration_noise_level`: one value or one per request (VITS-family voices: the requests still share their batches, each with its own
        scales, include/vits_prosody.h).  `sample_rate`: output rate
        in Hz for the whole batch (default: the voice's own; include/vits_resample.h).  `denoiser_strength`: the vocoder-bias
        denoiser of a multistream voice for the whole batch (default: the voice's inference.denoiser_strength, else off; as
        Synth.synth_audio, a VITS-family voice raises ValueError), every item denoised from its own length before any resampling.
        `loudness` / `peak` / `peak_ceiling`: a LUFS or a peak target for every request of the batch (defaults and rules of
        Synth.synth_audio): each request is measured and normalised on its own, so it equals its single call with the same seed.
        `limit` / `limit_lookahead_ms` / `limit_release_ms`: the look-ahead peak limiter (include/vits_limit.h), one setting per call and a
        gain per request; `peak_ceiling` is then the limiter's ceiling.
        `pitch_range`: the intonation range (include/vits_intonation.h), one value per call; every request is tracked and scaled about
        its own median, so it equals its single call with the same seed.
        `watermark` / `watermark_depth_db`: the audio watermark (include/vits_watermark.h; Synth._watermark), one key per call; every
        request is marked from its own samples, so it equals its single call with the same seed."""
        s0 = self.synths[0]
        tail_feed = {}  # (the tail's feed keys, one setting for the whole batch: merged into every shard's feed)
        s0._loudness(tail_feed, loudness, peak, peak_ceiling)
        s0._limit(tail_feed, limit, peak_ceiling, limit_lookahead_ms, limit_release_ms)
        s0._pitch(tail_feed, pitch, preserve_formants)
        s0._range(tail_feed, pitch_range)
        per_request = isinstance(watermark_payload, (list, tuple, np.ndarray))
        if per_request and len(watermark_payload) != len(texts):
            raise ValueError(f"watermark_payload: {len(watermark_payload)} values for {len(texts)} requests")
        s0._watermark(tail_feed, watermark, watermark_depth_db, list(watermark_payload) if per_request else watermark_payload)
        dn = {}
        s0._denoiser(dn, denoiser_strength)
        denoiser_strength = dn.get("vits.denoiser_strength")
        rate = int(sample_rate) if sample_rate else s0.native_rate()
        with_marks = (lambda res: [(a, s0._marks(t, e, rate)) for t, (a, e) in zip(texts, res)]) if marks else (lambda res: res)
        if self.family == "vits":
            token_lists = [s0.g2p_noembed(s0.normalize(t)) for t in texts]
            return with_marks(self.synth_tokens(token_lists, speaker_ids, noise_level, speech_rate, duration_noise_level, scale, seeds, sample_rate,
                                                marks=marks, tail_feed=tail_feed))
        # BERT-conditioned families: the front end needs the replica's BERT encoder, so it runs on the replica that gets the request;
        # requests are sharded by a cheap length estimate (phoneme count, no BERT needed)
        n = len(texts)
        if n == 0:
            return []
        texts = [s0.normalize(t) for t in texts]
        scales, scale, sids, seeds = self._call_params(n, speaker_ids, noise_level, speech_rate, duration_noise_level, scale, seeds)
        est = [len(s0.phonemize(t.replace("_", " "))) for t in texts]
        shards = plan_shards(est, len(self.devices))
        run = self._run_shard_bert if self.family == "vits_bert" else self._run_shard_multistream
        kw = {"denoiser_strength": denoiser_strength} if self.family == "multistream" else {}
        futs = [self._pool.submit(run, r, texts, idx, sids, scales, scale, seeds, sample_rate=sample_rate, marks=marks, tail_feed=tail_feed, **kw) if idx else None
                for r, idx in enumerate(shards)]
        return with_marks(scatter_results(n, [idx for idx in shards if idx], [f.result() for f in futs if f is not None]))

    def synth_documents(self, docs, seeds=None, **kw):
        """docs: a list of documents, each a string or a list of document.Segment -> a list of Synth.synth_document's results, in request
        order (marks=True: (audio, SpeechMarks) each).  A document goes whole to ONE replica -- its join and the stages behind it need every
        segment on one device -- and the documents are spread over the replicas by their total token counts (plan_shards; a cheap
        phoneme count, no BERT needed).  `seeds`: one noise seed per document (default: a running counter; segment b draws seed + b);
        **kw: the keywords of Synth.synth_document, one setting for all."""
        from . import document as D

        n = len(docs)
        if n == 0:
            return []
        s0 = self.synths[0]
        est = []
        for d in docs:
            segs = D.split(d) if isinstance(d, str) else list(d)
            est.append(sum(len(s0.phonemize(s0.normalize(s.text).replace("_", " "))) for s in segs))
        if seeds is None:
            with self._lock:
                seeds = [self._seed + 1 + 1000 * i for i in range(n)]
                self._seed += 1000 * n
        seeds = list(seeds)
        if len(seeds) != n:
            raise ValueError(f"seeds: one per document ({n})")
        shards = plan_shards(est, len(self.devices))

        def run(r, idx):
            out = []
            for i in idx:
                with self._replica_locks[r]:
                    out.append(self.synths[r].synth_document(docs[i], seed=seeds[i], **kw))
            return out

        futs = [self._pool.submit(run, r, idx) if idx else None for r, idx in enumerate(shards)]
        return scatter_results(n, [idx for idx in shards if idx], [f.result() for f in futs if f is not None])

    def _call_params(self, n, speaker_ids, noise_level, speech_rate, duration_noise_level, scale, seeds):
        """runtime defaults (synth.py:50-56,106) and per-request speaker ids / seeds.  noise_level / speech_rate / duration_noise_level:
        one value, or one per request -- `scales` is then float32 [n, 3], every request's own triple (the reference server hands every
        request its own speech_rate hint, server/tts_service.proto Hints.speech_rate)"""
        inf = self.synths[0].model.config.get("inference", {})
        noise_level = inf.get("noise_level", 0.8) if noise_level is None else noise_level
        speech_rate = inf.get("speech_rate", 1.0) if speech_rate is None else speech_rate
        duration_noise_level = inf.get("duration_noise_level", 0.8) if duration_noise_level is None else duration_noise_level
        scale = inf.get("scale", 1.0) if scale is None else scale
        if all(np.isscalar(v) for v in (noise_level, speech_rate, duration_noise_level)):
            scales = np.array([noise_level, 1.0 / speech_rate, duration_noise_level], np.float32)  # synth.py:106
        else:
            if self.family == "multistream":
                raise ValueError("noise_level / speech_rate / duration_noise_level per request: the VITS-family voices only (include/vits_prosody.h)")
            cols = []
            for name, v in (("noise_level", noise_level), ("speech_rate", speech_rate), ("duration_noise_level", duration_noise_level)):
                a = np.full(n, v, np.float64) if np.isscalar(v) else np.asarray(list(v), np.float64)
                if a.shape != (n,):
                    raise ValueError(f"{name}: one value, or one per request ({n})")
                cols.append(a)
            scales = np.stack([cols[0], 1.0 / cols[1], cols[2]], axis=1).astype(np.float32)
        sids = [speaker_ids] * n if np.isscalar(speaker_ids) or speaker_ids is None else list(speaker_ids)
        sids = [0 if v is None else int(v) for v in sids]
        if seeds is None:
            with self._lock:
                seeds = [self._seed + 1 + i for i in range(n)]
                self._seed += n
        return scales, scale, sids, list(seeds)

    def _front_is_batched(self, r, n):
        """whether a part of n requests on replica r takes Synth.front_batch"""
        enc = getattr(self.models[r], "bert_onnx", None)
        return self.batched_front and n >= BATCHED_FRONT_MIN and (self.models[r].tokenizer is None or getattr(enc, "has_batch", False))

    def _run_parts(self, r, idx, run_part, per_request):
        """`idx` (sorted by descending estimated length by plan_shards) in parts of <= max_batch: run_part(part) for every part that
        takes front_batch, per_request(rest) once for the requests of all the others -> results in the order of idx"""
        out, rest = {}, []
        for k in range(0, len(idx), self.max_batch):
            part = idx[k:k + self.max_batch]
            if self._front_is_batched(r, len(part)):
                out.update(zip(part, run_part(part)))
            else:
                rest.extend(part)
        if rest:
            out.update(zip(rest, per_request(rest)))
        return [out[i] for i in idx]

    def _run_shard_bert(self, r, texts, idx, sids, scales, scale, seeds, per_request=False, sample_rate=None, marks=False, tail_feed=None):
        """BERT-conditioned VITS requests `idx` on replica r: get_word_bert + g2p / g2p_noblank per request (synth.py:88-99), then padded
        solo batches with a padded `bert` feed [B, 768, T]"""
        synth, sess = self.synths[r], self.models[r].onnx
        if not per_request:
            def run_part(part):
                f = synth.front_batch([texts[i] for i in part], [sids[i] for i in part])
                feed = {"input": f["input"], "input_lengths": f["input_lengths"], **self._scales_feed(scales, part), "sid": f["sid"], "bert": f["bert"],
                        "phone_duration_extra": None, "vits.solo": True, "vits.item_seeds": np.array([seeds[i] for i in part], np.uint64),
                        **tail_part(tail_feed, part)}
                with self._replica_locks[r]:
                    pcm, lengths, ends = self._pcm16_marks(sess, feed, scale, sample_rate, marks)
                return [self._item(pcm[b], lengths[b], None if ends is None else ends[b], f["input_lengths"][b]) for b in range(len(part))]

            return self._run_parts(r, idx, run_part, lambda rest: self._run_shard_bert(r, texts, rest, sids, scales, scale, seeds, per_request=True,
                                                                                      sample_rate=sample_rate, marks=marks, tail_feed=tail_feed))
        fe = synth.g2p_noblank if synth.model.config.get("no_blank", 0) != 0 else synth.g2p
        fronts = []
        for i in idx:
            ids, emb = fe(texts[i], synth.get_word_bert(texts[i]))
            fronts.append((np.array(ids, np.int64), np.transpose(np.array(emb, np.float32))))  # [T], [768, T]
        order = sorted(range(len(idx)), key=lambda k: -len(fronts[k][0]))
        out = [None] * len(idx)
        for k0 in range(0, len(order), self.max_batch):
            part = order[k0:k0 + self.max_batch]
            lens = np.array([len(fronts[k][0]) for k in part], np.int64)
            T = int(lens.max())
            ids = np.zeros((len(part), T), np.int64)
            bert = np.zeros((len(part), sess.hp.bert_dim, T), np.float32)
            for b, k in enumerate(part):
                ids[b, :lens[b]] = fronts[k][0]
                bert[b, :, :lens[b]] = fronts[k][1]
            feed = {"input": ids, "input_lengths": lens, **self._scales_feed(scales, [idx[k] for k in part]),
                    "sid": np.array([sids[idx[k]] for k in part], np.int64), "bert": bert, "phone_duration_extra": None, "vits.solo": True,
                    "vits.item_seeds": np.array([seeds[idx[k]] for k in part], np.uint64), **tail_part(tail_feed, [idx[k] for k in part])}
            with self._replica_locks[r]:
                pcm, lengths, ends = self._pcm16_marks(sess, feed, scale, sample_rate, marks)
            for b, k in enumerate(part):
                out[k] = self._item(pcm[b], lengths[b], None if ends is None else ends[b], lens[b])
        return out

    @staticmethod
    def _stts_batch(sess, args, kw, sample_rate, marks, tail_feed=None):
        """stts_synthesize_batch of one padded part and the tail behind it (SttsSession.tail_chain) -> (audio, lengths, token_ends or None)
        at `sample_rate`.  tail_feed: the tail's feed fragment; every item is marked and normalised on its own, behind the resampler"""
        from .outopts import Tail

        res = sess.tail_chain(lambda **t: sess._model.synthesize_batch(*args, **kw, **t), Tail.from_feed(sess._lib, tail_feed or {}), sample_rate, marks)
        return res if marks else res + (None,)

    def _run_shard_multistream(self, r, texts, idx, sids, scales, scale, seeds, per_request=False, sample_rate=None, denoiser_strength=None,
                               marks=False, tail_feed=None):
        """multistream (StableTTS / Matcha) requests `idx` on replica r: the five-stream front end of Synth._feed per request
        (synth.py:64-87), then stts_synthesize_batch with per-request seeds (and the denoiser, where a strength is given);
        float -> int16 as Synth.audio_float_to_int16"""
        synth, sess = self.synths[r], self.models[r].onnx
        if not per_request:
            def run_part(part):
                f = synth.front_batch([texts[i] for i in part], [sids[i] for i in part])
                with self._replica_locks[r]:
                    audio, ol, ends = self._stts_batch(
                        sess, (f["input"], f["input_lengths"], scales, f["sid"], f["bert"], f["phone_duration_extra"]),
                        dict(seed=0, item_seeds=np.array([seeds[i] for i in part], np.uint64), denoiser_strength=denoiser_strength), sample_rate, marks,
                        tail_part(tail_feed, part))
                pcm = [synth.audio_float_to_int16(audio[b, :int(ol[b])] * scale) for b in range(len(part))]
                return pcm if ends is None else [(pcm[b], ends[b, :int(f["input_lengths"][b])].copy()) for b in range(len(part))]

            return self._run_parts(r, idx, run_part, lambda rest: self._run_shard_multistream(r, texts, rest, sids, scales, scale, seeds, per_request=True,
                                                                                             sample_rate=sample_rate, denoiser_strength=denoiser_strength,
                                                                                             marks=marks, tail_feed=tail_feed))
        fronts = []
        for i in idx:
            feed, _ = synth._feed(texts[i], sids[i], None, None, None, None)
            pde = feed["phone_duration_extra"]
            fronts.append((feed["input"][0], feed["bert"][0], None if pde is None else np.asarray(pde, np.float32).reshape(-1)))
        order = sorted(range(len(idx)), key=lambda k: -fronts[k][0].shape[1])
        out = [None] * len(idx)
        for k0 in range(0, len(order), self.max_batch):
            part = order[k0:k0 + self.max_batch]
            lens = np.array([fronts[k][0].shape[1] for k in part], np.int64)
            T = int(lens.max())
            ids = np.zeros((len(part), 5, T), np.int64)
            bert = np.zeros((len(part), sess.hp.bert_dim, T), np.float32)
            any_pde = any(fronts[k][2] is not None for k in part)
            pde = np.zeros((len(part), T), np.float32) if any_pde else None
            for b, k in enumerate(part):
                ids[b, :, :lens[b]] = fronts[k][0]
                bert[b, :, :lens[b]] = fronts[k][1]
                if fronts[k][2] is not None:
                    pde[b, :lens[b]] = fronts[k][2]
            with self._replica_locks[r]:
                audio, ol, ends = self._stts_batch(
                    sess, (ids, lens, scales, np.array([sids[idx[k]] for k in part], np.int64), bert, pde),
                    dict(seed=0, item_seeds=np.array([seeds[idx[k]] for k in part], np.uint64), denoiser_strength=denoiser_strength), sample_rate, marks,
                    tail_part(tail_feed, [idx[k] for k in part]))
            for b, k in enumerate(part):
                out[k] = synth.audio_float_to_int16(audio[b, :int(ol[b])] * scale)
                if ends is not None:
                    out[k] = (out[k], ends[b, :int(lens[b])].copy())
        return out

    def synth_tokens(self, token_lists, speaker_ids=0, noise_level=None, speech_rate=None, duration_noise_level=None, scale=None, seeds=None,
                     sample_rate=None, marks=False, tail_feed=None):
        """synth_batch() behind the front end: token id lists in, int16 PCM arrays out (request order).  marks=True: (PCM, token ends
        int64 [len(tokens)] in output samples) per request.  tail_feed: the tail's feed fragment of the batch (Synth._loudness, _limit, ...)."""
        n = len(token_lists)
        if n == 0:
            return []
        if self.family != "vits":
            raise NotImplementedError("synth_tokens takes plain VITS token ids; BERT-conditioned and multistream voices need the text (synth_batch)")
        scales, scale, sids, seeds = self._call_params(n, speaker_ids, noise_level, speech_rate, duration_noise_level, scale, seeds)
        shards = plan_shards([len(t) for t in token_lists], len(self.devices))
        futs = [self._pool.submit(self._run_shard, r, token_lists, idx, sids, scales, scale, seeds, sample_rate, marks, tail_feed) if idx else None
                for r, idx in enumerate(shards)]
        return scatter_results(n, [idx for idx in shards if idx], [f.result() for f in futs if f is not None])
