"""Drop-in for the onnxruntime session of a `multistream_v*` voice (vosk_tts/model.py:46, synth.py:113-126):
`SttsSession.run(None, feed)` takes the feed of the StableTTS export (training/stabletts/matcha/onnx/export.py:64-98)
    input [1,5,T] int64, input_lengths [1], scales [3] = [noise_level, 1/speech_rate, duration_noise_level],
    sid [1], bert [1,768,T] or None (-> zeros, synth.py:79), phone_duration_extra [1,T] or None
and returns [wav float32 [1,S], wav_lengths int64 [1]] like the exported graph (export.py:21-32,58-59).
The arithmetic runs in HIP kernels behind include/stts_mi355.h; there is no CPU path."""
import itertools
import threading
from dataclasses import replace

import numpy as np

from .capi import VitsLib
from .capi_stts import SttsModel
from .outopts import DOCUMENT_FEEDS, Tail, document_from_feed

_INPUTS = ("input", "input_lengths", "scales", "sid", "bert", "phone_duration_extra")
_EXT = ("vits.noise", "vits.seed", "vits.n_timesteps", "vits.sample_rate", "vits.denoiser_strength", "vits.denoiser_filter_length",
        "vits.marks", "vits.loudness", "vits.peak", "vits.peak_ceiling", "vits.pitch", "vits.pitch_formants",
        "vits.limit", "vits.limit_lookahead_ms", "vits.limit_release_ms", "vits.token_pitch", "vits.token_gain_db",
        "vits.pitch_range", "vits.watermark_key", "vits.watermark_depth_db", "vits.watermark_payload") + tuple(DOCUMENT_FEEDS)


class SttsSession:
    def __init__(self, blob, vocoder_blob, device=0, lib=None):
        self._lib = lib or VitsLib()
        self._vocoder = self._lib.create(vocoder_blob, device)
        self._model = SttsModel(self._lib, blob, self._vocoder, device)
        self.hp = self._model.hp
        self._seed = itertools.count(1)
        self._seed_lock = threading.Lock()

    def get_providers(self):
        return ["MI355XExecutionProvider"]

    def _parse(self, output_names, input_feed):
        if output_names is not None and not set(output_names) <= {"wav", "wav_lengths"}:
            raise ValueError(f"unknown output names {output_names}")
        feed = {k: v for k, v in input_feed.items() if v is not None}
        for k in feed:
            if k not in _INPUTS and k not in _EXT:
                raise ValueError(f"Invalid input name: {k}")
        for k in ("input", "input_lengths", "scales"):
            if k not in feed:
                raise ValueError(f"Required input {k} is missing")
        ids = np.asarray(feed["input"])
        if ids.ndim != 3 or ids.shape[0] != 1 or ids.shape[1] != 5:
            raise ValueError("input must be int64 [1, 5, T] (one utterance, five streams)")
        T = ids.shape[2]
        if int(np.asarray(feed["input_lengths"]).reshape(-1)[0]) != T:
            raise ValueError("input_lengths must equal T (the graph is driven with B = 1, synth.py:69-70)")
        sid = int(np.asarray(feed.get("sid", [0])).reshape(-1)[0])
        bert = feed.get("bert")
        if bert is not None:
            bert = np.asarray(bert, np.float32).reshape(self.hp.bert_dim, T)
        pde = feed.get("phone_duration_extra")
        if pde is not None:
            pde = np.asarray(pde, np.float32).reshape(T)
        seed = feed.get("vits.seed")
        if seed is None:
            with self._seed_lock:
                seed = next(self._seed)
        return feed, ids[0], np.asarray(feed["scales"], np.float32).reshape(-1), sid, bert, pde, int(seed)

    @staticmethod
    def _denoiser(feed):
        """the extension feeds "vits.denoiser_strength" (absent / None = off) and "vits.denoiser_filter_length" (absent / 0 = 1024) ->
        keyword arguments of the SttsModel calls; values the library would refuse are refused here, by name, before any work"""
        strength = feed.get("vits.denoiser_strength")
        n = feed.get("vits.denoiser_filter_length")
        if strength is None:
            if n is not None:
                raise ValueError("vits.denoiser_filter_length needs vits.denoiser_strength")
            return {}
        strength = float(np.asarray(strength).reshape(-1)[0])
        if not strength >= 0:
            raise ValueError(f"vits.denoiser_strength {strength}: must be >= 0")
        n = int(np.asarray(n).reshape(-1)[0]) if n is not None else 0
        if n and (n < 64 or n > 1024 or n & (n - 1)):
            raise ValueError(f"vits.denoiser_filter_length {n}: must be a power of two in [64, 1024] (0 = 1024)")
        return {"denoiser_strength": strength, "denoiser_filter_length": n}

    def _rate(self, sample_rate):
        """output sample rate of a request -> 0 for None / 0 / the vocoder's own rate"""
        rate = int(sample_rate or 0)
        if rate < 0:
            raise ValueError(f"sample_rate {rate}: must be positive, or None for the voice's own {self._vocoder.hp.sampling_rate} Hz")
        return 0 if rate == self._vocoder.hp.sampling_rate else rate

    def resample(self, audio, lengths, sample_rate):
        """audio float32 [B, S] with per-item sample counts -> (audio, lengths) at `sample_rate` (vits_op_resample on the host
        buffer, every item from its own samples only); None / the vocoder's own rate: unchanged"""
        rate = self._rate(sample_rate)
        if not rate:
            return audio, lengths
        native = self._vocoder.hp.sampling_rate
        lengths = np.asarray(lengths, np.int64).reshape(-1)
        out = self._lib.op_resample(audio, lengths, native, rate, device=self._vocoder.device)
        return out, np.array([self._lib.out_samples(n, native, rate) for n in lengths], np.int64)

    @staticmethod
    def _contour(feed):
        """the contour feeds "vits.token_pitch" / "vits.token_gain_db" (float [1, T], include/vits_contour.h) as the keywords of the model's
        single-utterance call: empty without a contour"""
        return {k[5:]: np.asarray(feed[k], np.float32).reshape(-1) for k in ("vits.token_pitch", "vits.token_gain_db") if k in feed}

    def mark(self, audio, lengths, wm):
        """audio float32 [B, S] with per-item sample counts -> the audio marked per item (vits_op_watermark on the host buffer); wm: a
        capi.watermark_spec() (key, depth) or (key, depth, payload: vits_op_watermark_payload), None: unchanged.  What tail_chain() does
        behind resample() and in front of normalize(): the mark goes in at the rate returned"""
        if wm is None or audio.shape[-1] == 0:
            return audio
        if len(wm) > 2:
            payloads = wm[2] if isinstance(wm[2], tuple) else (wm[2],) * audio.shape[0]
            return self._lib.op_watermark_payload(audio, lengths, wm[0], payloads, wm[1], device=self._vocoder.device)
        return self._lib.op_watermark(audio, lengths, *wm, device=self._vocoder.device)

    def normalize(self, audio, lengths, sample_rate, spec, limit=None):
        """audio float32 [B, S] at `sample_rate` Hz (None / 0 = the vocoder's own) with per-item sample counts -> the audio normalised
        per item by `spec` (vits_op_loudness_normalize on the host buffer) and / or limited by `limit` (vits_op_loudness_limit,
        vits_op_limit); both None: unchanged.  What tail_chain() does behind resample(): the order is decode, clamp, denoise,
        resample, mark, normalise + limit"""
        if (spec is None and limit is None) or audio.shape[-1] == 0:
            return audio
        rate = int(sample_rate or 0) or self._vocoder.hp.sampling_rate
        if limit is not None:
            mode, ceiling, la, rel, gain = limit
            if spec is None:
                return self._lib.op_limit(audio, lengths, rate, mode, ceiling, la, rel, gain, device=self._vocoder.device)[0]
            return self._lib.op_loudness_limit(audio, lengths, rate, spec[1], mode, ceiling, la, rel, device=self._vocoder.device)[0]
        return self._lib.op_loudness_normalize(audio, lengths, rate, *spec, device=self._vocoder.device)[0]

    def run(self, output_names, input_feed, run_options=None):
        """Extension feeds: "vits.sample_rate", output rate in Hz (the finished waveform is resampled, include/vits_resample.h);
        "vits.denoiser_strength" / "vits.denoiser_filter_length", the vocoder-bias denoiser behind the clamp (include/vits_denoise.h),
        applied at the vocoder's own rate, before any resampling; "vits.marks": True appends token_ends int64 [1, T] in output samples
        to the result list (include/vits_marks.h; stts_synthesize_marks takes the rate itself); "vits.loudness" / "vits.peak" /
        "vits.peak_ceiling": the audio normalised to a LUFS or a peak target, last in the chain -- at another rate the resampled audio
        is what is measured (include/vits_loudness.h)."""
        if any(input_feed.get(k) is not None for k in DOCUMENT_FEEDS):  # (run_document: the batch of the feed comes back as one row)
            if output_names is not None and not set(output_names) <= {"wav", "wav_lengths"}:
                raise ValueError(f"unknown output names {output_names}")
            audio, info = self.run_document(input_feed)
            outs = {"wav": audio[None, :], "wav_lengths": np.array([audio.shape[0]], np.int64)}
            return [outs[n] for n in (output_names or ["wav", "wav_lengths"])] + ([info["token_ends"]] if "token_ends" in info else [])
        feed, ids, scales, sid, bert, pde, seed = self._parse(output_names, input_feed)
        n_steps = int(feed.get("vits.n_timesteps", 0))
        marks = bool(feed.get("vits.marks"))

        def call(**kw):  # (the single-utterance call in the batch door's form)
            res = self._model.synthesize(ids, scales, sid, bert, pde, noise=feed.get("vits.noise"), seed=seed, n_timesteps=n_steps, want_mel=False,
                                         **kw, **self._contour(feed), **self._denoiser(feed))
            return (res[0][None, :], np.array([res[0].shape[0]], np.int64)) + ((res[2][None, :],) if marks else ())

        res = self.tail_chain(call, Tail.from_feed(self._lib, feed), feed.get("vits.sample_rate"), marks)
        outs = {"wav": res[0], "wav_lengths": np.array([res[0].shape[1]], np.int64)}
        return [outs[n] for n in (output_names or ["wav", "wav_lengths"])] + list(res[2:])

    def tail_chain(self, call, tail, sample_rate, marks):
        """One synthesize call and the tail behind it -> what the call returns, (audio float32 [B, S], lengths int64 [B]) and with marks
        token_ends, at `sample_rate`.  call(**keywords): the model's batch call, taking the tail's keywords (Tail.kw()) and, for marks,
        marks=True with the rate (the marks entry points resample inside the library, tail and all).  Without marks the library has
        no rate: the call keeps the stages in front of the resampler (pitch, intonation range), and the resampler, the mark and the
        normalisation / limiter follow it here on the host buffer, in the library's order."""
        rate = self._rate(sample_rate)
        if marks:
            return call(marks=True, sample_rate=rate, **tail.kw())
        if not rate:
            return call(**tail.kw())
        audio, ol = call(**replace(tail, loudness=None, limit=None, watermark=None).kw())
        audio, ol = self.resample(audio, ol, rate)
        return self.normalize(self.mark(audio, ol, tail.watermark), ol, rate, tail.loudness, tail.limit), ol

    def run_stream(self, output_names, input_feed, chunk_frames=64, sample_rate=None, on_marks=None):
        """on_marks: called once with token_ends int64 [T] in the stream's output samples, before the first chunk.
        Streaming form of run() (extension; the reference's transport is already `stream AudioChunk`,
        server/tts_service.proto:46-54): yields float32 [n] chunks of chunk_frames * hop samples whose concatenation equals
        run(...)[0].squeeze() for the same feed (same "vits.seed").  The acoustic model runs once, the vocoder is streamed."""
        if any(input_feed.get(k) is not None for k in DOCUMENT_FEEDS):
            raise ValueError("a stream cannot take a document: the join and the stages behind it need every segment before the first chunk "
                             "(run() / run_document() take the \"vits.doc_*\" feeds)")
        feed, ids, scales, sid, bert, pde, seed = self._parse(output_names, input_feed)
        if "vits.noise" in feed:
            raise NotImplementedError("run_stream draws the CFM noise on the device (vits.seed)")
        tail = Tail.from_feed(self._lib, feed)
        (replace(tail, pitch=0.0) if self._contour(feed) else tail).refuse_stream("STTS", "run() takes")  # (a contour: the pitch stage's refusal)
        rate = self._rate(sample_rate if sample_rate is not None else feed.get("vits.sample_rate"))
        dn = self._denoiser(feed)
        if rate and dn:
            from .capi import VitsError

            raise VitsError(4, f"a stream with a denoiser (strength {dn['denoiser_strength']}) at sample_rate {rate} Hz is not supported: "
                               f"only the voice's own {self._vocoder.hp.sampling_rate} Hz")
        if rate:  # the acoustic model's mel, then the vocoder streamed at the rate asked for (vits_stream_open_latent_rate; clamped like the export)
            res = self._model.synthesize(ids, scales, sid, bert, pde, seed=seed, n_timesteps=int(feed.get("vits.n_timesteps", 0)),
                                         want_audio=False, want_mel=True, marks=on_marks is not None, sample_rate=rate if on_marks else None)
            mel = res[1]
            if on_marks is not None:
                on_marks(res[2])
            return self._vocoder.stream_latent(mel, chunk_frames=chunk_frames, clamp=True, sample_rate=rate)
        return self._model.stream(ids, scales, sid, bert, pde, seed=seed, n_timesteps=int(feed.get("vits.n_timesteps", 0)),
                                  chunk_frames=chunk_frames, on_marks=on_marks, **dn)

    def run_batch(self, input_feed):
        """The batch door as a feed (stts_synthesize_batch; MultiDeviceSynth calls the model's synthesize_batch with the same
        keywords): "input" int64 [B, 5, T], "input_lengths" [B], "scales" [3],
        "sid" [B], "bert" [B, 768, T] or None, "phone_duration_extra" [B, T] or None, "vits.item_seeds" [B] (or "vits.seed"), and the
        extension feeds of run() -> (audio float32 [B, S] zero beyond each item, lengths int64 [B] in output samples).  Every item is
        denoised from its own length, then resampled from its own samples.  "vits.marks": True -> a third value, token_ends int64
        [B, T] in output samples (stts_synthesize_batch_marks)."""
        feed = {k: v for k, v in input_feed.items() if v is not None}
        for k in feed:
            if k not in _INPUTS and k not in _EXT and k != "vits.item_seeds":
                raise ValueError(f"Invalid input name: {k}")
        if "vits.noise" in feed:
            raise NotImplementedError("injected noise is a single-utterance option")
        if any(k in feed for k in DOCUMENT_FEEDS):
            raise ValueError("run_batch returns the items of a batch; a document feed (\"vits.doc_*\") belongs to run_document() / run()")
        for k in ("input", "input_lengths", "scales"):
            if k not in feed:
                raise ValueError(f"Required input {k} is missing")
        dn = self._denoiser(feed)
        tail = Tail.from_feed(self._lib, feed)  # (per-item gains, last in the chain like run())
        ids = np.asarray(feed["input"])
        if ids.ndim != 3 or ids.shape[1] != 5:
            raise ValueError("input must be int64 [B, 5, T]")
        sid = np.asarray(feed.get("sid", np.zeros(ids.shape[0])), np.int64).reshape(-1)
        return self.tail_chain(
            lambda **kw: self._model.synthesize_batch(ids, feed["input_lengths"], np.asarray(feed["scales"], np.float32).reshape(-1), sid,
                                                      feed.get("bert"), feed.get("phone_duration_extra"), seed=int(feed.get("vits.seed", 0)),
                                                      n_timesteps=int(feed.get("vits.n_timesteps", 0)), item_seeds=feed.get("vits.item_seeds"),
                                                      **kw, **self._contour(feed), **dn),
            tail, feed.get("vits.sample_rate"), bool(feed.get("vits.marks")))

    def run_document(self, input_feed, scale=1.0, pcm16=False):
        """A document (include/vits_document.h): run_batch's feed with at least one of the document feeds "vits.doc_gap_frames" int [B],
        "vits.doc_lead_frames", "vits.doc_fade_samples", "vits.doc_trim_db", "vits.doc_trim_keep": the items of the batch joined into
        one piece of audio behind the pitch stage (stts_synthesize_document), in front of the resampler and the loudness / limiter
        stage.  -> (audio float32 [S], info) as VitsSession.run_document; pcm16=True converts on the host, as Synth does for this
        family (audio * scale, then Synth.audio_float_to_int16's rule)."""
        feed = {k: v for k, v in input_feed.items() if v is not None}
        for k in feed:
            if k not in _INPUTS and k not in _EXT and k != "vits.item_seeds":
                raise ValueError(f"Invalid input name: {k}")
        if "vits.noise" in feed:
            raise NotImplementedError("injected noise is a single-utterance option")
        for k in ("input", "input_lengths", "scales"):
            if k not in feed:
                raise ValueError(f"Required input {k} is missing")
        doc = document_from_feed(self._lib, feed)
        if doc is None:
            raise ValueError("run_document: the feed names no document key (\"vits.doc_gap_frames\", ...)")
        ids = np.asarray(feed["input"])
        if ids.ndim != 3 or ids.shape[1] != 5:
            raise ValueError("input must be int64 [B, 5, T]")
        sid = np.asarray(feed.get("sid", np.zeros(ids.shape[0])), np.int64).reshape(-1)
        if sid.shape[0] == 1 and ids.shape[0] > 1:
            sid = np.repeat(sid, ids.shape[0])
        seed = feed.get("vits.seed")
        if seed is None and "vits.item_seeds" not in feed:
            with self._seed_lock:
                seed = next(self._seed)
        con = {k: a.reshape(ids.shape[0], -1) for k, a in self._contour(feed).items()}  # ([B, T] here, not the single utterance's [T])
        audio, info = self._model.synthesize_document(
            ids, feed["input_lengths"], np.asarray(feed["scales"], np.float32).reshape(-1), sid, feed.get("bert"), feed.get("phone_duration_extra"),
            seed=int(seed or 0), n_timesteps=int(feed.get("vits.n_timesteps", 0)), item_seeds=feed.get("vits.item_seeds"),
            marks=bool(feed.get("vits.marks")), sample_rate=self._rate(feed.get("vits.sample_rate")), **Tail.from_feed(self._lib, feed).kw(),
            **con, **self._denoiser(feed), **doc)
        if pcm16:
            audio = np.clip((audio * scale) * 32767.0, -32767.0, 32767.0).astype("int16")
        return audio, info

    def close(self):
        self._model.close()
        self._vocoder.close()
