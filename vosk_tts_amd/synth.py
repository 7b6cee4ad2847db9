"""`Synth` — mirror of vosk_tts.Synth (vosk_tts/synth.py:11-150) for the VITS flavour
(`g2p_noembed`, synth.py:223-255): same signature, defaults, feed construction, int16 conversion,
RTF log line and WAV output.  The only change is what sits behind `self.model.onnx.run`.
"""
import logging
import math
import re
import time
import wave

import numpy as np

from .g2p import convert

_SPLIT = "([,.?!;:\"() ])"


class Synth:
    def __init__(self, model):
        self.model = model

    def audio_float_to_int16(self, audio, max_wav_value=32767.0):
        """Normalize audio and convert to int16 range (synth.py:16-23)"""
        audio_norm = np.clip(audio * max_wav_value, -max_wav_value, max_wav_value)
        return audio_norm.astype("int16")

    @staticmethod
    def normalize(text):
        """the two text fix-ups synth_audio applies before any front-end (synth.py:58-59)"""
        return re.sub("—", "-", text.strip())

    def _feed(self, text, speaker_id, noise_level, speech_rate, duration_noise_level, scale):
        """Runtime defaults and the six-key feed of synth.py:50-56,100-120."""
        inf = self.model.config.get("inference", {})
        if noise_level is None:
            noise_level = inf.get("noise_level", 0.8)
        if speech_rate is None:
            speech_rate = inf.get("speech_rate", 1.0)
        if duration_noise_level is None:
            duration_noise_level = inf.get("duration_noise_level", 0.8)
        if scale is None:
            scale = inf.get("scale", 1.0)

        text = self.normalize(text)
        model_type = self.model.config.get("model_type") or ""
        bert_embs = None
        phone_duration_extra = None
        have_bert = self.model.tokenizer is not None
        if model_type.startswith("multistream"):
            # synth.py:64-87: v3 = lower-cased text for BERT + '_' pause marks, v2 = word positions, v1 = plain phonemes;
            # v2 also runs without a tokenizer (zero BERT vectors, synth.py:77-81)
            from .multistream import g2p_multistream

            idmap = self.model.config["phoneme_id_map"]
            if model_type == "multistream_v3" and have_bert:
                bert = self.get_word_bert(text.lower(), nopunc=True)
                stream_ids, per_symbol, extra = g2p_multistream(text, self.model.dic, idmap, bert, pause_marks=True)
                phone_duration_extra = np.expand_dims(np.array(extra, dtype=np.float32), 0)
            elif model_type in ("multistream_v1", "multistream_v2") and have_bert:
                bert = self.get_word_bert(text, nopunc=True)
                stream_ids, per_symbol = g2p_multistream(text, self.model.dic, idmap, bert, word_pos=model_type == "multistream_v2")
            elif model_type == "multistream_v2":
                stream_ids, _ = g2p_multistream(text, self.model.dic, idmap, None, word_pos=True)
                per_symbol = None
            else:
                # without a tokenizer the reference falls through to g2p_noembed for v1/v3 (synth.py:100-103), which a
                # five-stream graph cannot take
                raise NotImplementedError(f"{model_type} needs bert/ (vocab.txt + model.bertw) next to the model")
            ids = np.expand_dims(np.transpose(np.array(stream_ids, dtype=np.int64)), 0)  # [1, 5, T]
            if per_symbol is None:
                bert_embs = np.zeros((1, 768, ids.shape[2]), dtype=np.float32)
            else:
                bert_embs = np.expand_dims(np.transpose(np.array(per_symbol, dtype=np.float32)), 0)  # [1, 768, T]
            lengths = np.array([ids.shape[2]], dtype=np.int64)
        elif have_bert:
            # BERT-conditioned VITS flavours (synth.py:88-99): per-word vectors fanned out to the phonemes of each word,
            # with (g2p) or without (g2p_noblank, config "no_blank") the interspersed blank
            bert = self.get_word_bert(text)
            fe = self.g2p_noblank if self.model.config.get("no_blank", 0) != 0 else self.g2p
            phoneme_ids, emb = fe(text, bert)
            bert_embs = np.expand_dims(np.transpose(np.array(emb, dtype=np.float32)), 0)
            ids = np.expand_dims(np.array(phoneme_ids, dtype=np.int64), 0)
            lengths = np.array([ids.shape[1]], dtype=np.int64)
        else:
            phoneme_ids = self.g2p_noembed(text)
            ids = np.expand_dims(np.array(phoneme_ids, dtype=np.int64), 0)
            lengths = np.array([ids.shape[1]], dtype=np.int64)
        scales = np.array([noise_level, 1.0 / speech_rate, duration_noise_level], dtype=np.float32)
        if speaker_id is None:
            speaker_id = 0
        sid = np.array([speaker_id], dtype=np.int64)
        args = {"input": ids, "input_lengths": lengths, "scales": scales, "sid": sid, "bert": bert_embs,
                "phone_duration_extra": phone_duration_extra}
        return args, scale

    def get_word_bert(self, text, nopunc=False):
        """Word-level BERT vectors (synth.py:25-44): encode the text without stress marks, run the encoder, keep the
        rows of first word pieces (optionally dropping punctuation tokens).  -> float32 [n_words + 2, 768]"""
        from .multistream import word_bert_rows

        tokens = self.model.tokenizer.encode(text.replace("+", "").replace("_", ""))
        bert = self.model.bert_onnx.run(None, {"input_ids": [tokens.ids], "attention_mask": [tokens.attention_mask],
                                               "token_type_ids": [tokens.type_ids]})[0]
        return bert[word_bert_rows(tokens.tokens, nopunc)]

    def _front_rows(self, text):
        """One text through the front end that _feed would pick, with the BERT vectors replaced by their indices: -> (ids int64 [T] or
        [5, T], token ids + type ids of the sentence for BERT or None, rows int32 [T] = the BERT token whose hidden state phoneme t
        takes (-1: none), phone_duration_extra float32 [T] or None).  The front ends are called as they are, with
        embeddings = np.arange(number of word rows) -- an array, so that -1 for '$' still means the last row -- and what they return is
        composed with word_bert_rows to token indices."""
        from .multistream import word_bert_rows

        model_type = self.model.config.get("model_type") or ""
        have_bert = self.model.tokenizer is not None

        def encode(t, nopunc):
            tokens = self.model.tokenizer.encode(t.replace("+", "").replace("_", ""))
            return tokens, np.asarray(word_bert_rows(tokens.tokens, nopunc), np.int32)

        pde = None
        if model_type.startswith("multistream"):
            from .multistream import g2p_multistream

            idmap = self.model.config["phoneme_id_map"]
            tokens = None
            if model_type == "multistream_v3" and have_bert:
                tokens, word_rows = encode(text.lower(), True)
                stream_ids, per_symbol, extra = g2p_multistream(text, self.model.dic, idmap, np.arange(len(word_rows)), pause_marks=True)
                pde = np.array(extra, dtype=np.float32)
            elif model_type in ("multistream_v1", "multistream_v2") and have_bert:
                tokens, word_rows = encode(text, True)
                stream_ids, per_symbol = g2p_multistream(text, self.model.dic, idmap, np.arange(len(word_rows)),
                                                         word_pos=model_type == "multistream_v2")
            elif model_type == "multistream_v2":
                stream_ids, _ = g2p_multistream(text, self.model.dic, idmap, None, word_pos=True)
            else:
                raise NotImplementedError(f"{model_type} needs bert/ (vocab.txt + model.bertw) next to the model")
            ids = np.transpose(np.array(stream_ids, dtype=np.int64))  # [5, T]
            rows = np.full(ids.shape[1], -1, np.int32) if tokens is None else word_rows[np.asarray(per_symbol, np.int64)]
        elif have_bert:
            tokens, word_rows = encode(text, False)
            fe = self.g2p_noblank if self.model.config.get("no_blank", 0) != 0 else self.g2p
            phoneme_ids, emb = fe(text, np.arange(len(word_rows)))
            ids = np.array(phoneme_ids, dtype=np.int64)
            rows = word_rows[np.asarray(emb, np.int64)]
        else:
            raise NotImplementedError("front_batch is the front end of BERT-conditioned and multistream voices")
        tok = None if tokens is None else (np.asarray(tokens.ids, np.int64), np.asarray(tokens.type_ids, np.int64))
        return ids, tok, rows, pde

    def front_batch(self, texts, speaker_ids=0):
        """The front end of _feed for a list of texts as ONE padded set, with one batched BERT call (BertEncoder.feed_batch: all
        sentences in one padded forward, the per-phoneme feed gathered on the device) instead of an encoder call, a row selection, a
        fan-out and a transpose per text.  Covers _feed's BERT-conditioned branches: g2p, g2p_noblank, multistream_v1 / v2 / v3
        (a tokenizer-less v2 gets a zero feed and makes no BERT call).
        -> {"input": int64 [B, T] ([B, 5, T] multistream), "input_lengths": int64 [B], "bert": float32 [B, 768, T],
            "phone_duration_extra": float32 [B, T] or None, "sid": int64 [B]}; item b, cut at its length, is _feed's feed of texts[b]."""
        n = len(texts)
        if n == 0:
            raise ValueError("empty batch")
        sids = [speaker_ids] * n if np.isscalar(speaker_ids) or speaker_ids is None else list(speaker_ids)
        if len(sids) != n:
            raise ValueError("one speaker id per text")
        fronts = [self._front_rows(self.normalize(t)) for t in texts]
        lens = np.array([f[0].shape[-1] for f in fronts], np.int64)
        T = int(lens.max())
        ids = np.zeros((n,) + fronts[0][0].shape[:-1] + (T,), np.int64)
        any_pde = any(f[3] is not None for f in fronts)
        pde = np.zeros((n, T), np.float32) if any_pde else None
        for b, (i, _, _, p) in enumerate(fronts):
            ids[b, ..., :lens[b]] = i
            if p is not None:
                pde[b, :lens[b]] = p
        if fronts[0][1] is None:  # tokenizer-less multistream_v2 (the branch depends on the voice, not on the text): zero vectors
            bert = np.zeros((n, 768, T), np.float32)
        else:
            enc = self.model.bert_onnx
            if not getattr(enc, "has_batch", False):
                raise NotImplementedError("the BERT session of this voice has no batched entry point (BertEncoder.has_batch)")
            bert = enc.feed_batch([f[1][0] for f in fronts], [f[2] for f in fronts], T_x=T, token_type_ids=[f[1][1] for f in fronts])
        return {"input": ids, "input_lengths": lens, "bert": bert, "phone_duration_extra": pde,
                "sid": np.array([0 if v is None else int(v) for v in sids], np.int64)}

    def native_rate(self):
        """the voice's own sample rate (the session's hparams; 22050 for sessions that do not say)"""
        sess = self.model.onnx
        hp = getattr(getattr(sess, "_vocoder", None), "hp", None) or getattr(sess, "hp", None)
        return int(getattr(hp, "sampling_rate", 0) or 22050)

    def _denoiser(self, args, denoiser_strength):
        """The vocoder-bias denoiser of the multistream (StableTTS / Matcha) voices (matcha/cli.py:105-108,253-256): `denoiser_strength`,
        or the config key inference.denoiser_strength, goes into the feed as "vits.denoiser_strength"; None and no config key = off.
        A VITS-family voice has no separate vocoder stage to put it behind (its decoder runs inside the fused forward): ValueError."""
        if denoiser_strength is None:
            denoiser_strength = self.model.config.get("inference", {}).get("denoiser_strength")
        if denoiser_strength is None:
            return
        if not (self.model.config.get("model_type") or "").startswith("multistream"):
            raise ValueError(f"denoiser_strength {denoiser_strength}: the denoiser belongs to the multistream (StableTTS / Matcha) voices; "
                             "this is a VITS-family voice")
        args["vits.denoiser_strength"] = float(denoiser_strength)

    def _loudness(self, args, loudness, peak, peak_ceiling):
        """Loudness normalisation of the request (include/vits_loudness.h): `loudness`, a LUFS target (ITU-R BS.1770 integrated loudness),
        or `peak`, a max-|sample| target in (0, 1], each defaulting to the config keys inference.loudness / inference.peak; peak_ceiling
        (inference.peak_ceiling, else 1.0; 0 = none) caps the peak a LUFS target may produce.  They go into the feed as "vits.loudness" /
        "vits.peak" / "vits.peak_ceiling"; none given and no config key = off, the reference's behaviour.  An argument overrides the
        config as a whole (peak=0.9 on a voice whose config names a loudness is a peak request); both arguments at once is ValueError.
        The engine measures and applies the gain on the device, last in the chain; `scale` multiplies afterwards, as before."""
        from .capi import loudness_spec

        inf = self.model.config.get("inference", {})
        if loudness is None and peak is None:
            loudness, peak = inf.get("loudness"), inf.get("peak")
        if peak_ceiling is None:
            peak_ceiling = inf.get("peak_ceiling")
        if loudness_spec(loudness, peak, peak_ceiling) is None:  # (raises on both at once and on values out of range)
            return False
        if loudness is not None:
            args["vits.loudness"] = float(loudness)
            if peak_ceiling is not None:
                args["vits.peak_ceiling"] = float(peak_ceiling)
        else:
            args["vits.peak"] = float(peak)
        return True

    def _limit(self, args, limit, peak_ceiling=None, lookahead_ms=None, release_ms=None):
        """The look-ahead peak limiter of the request (include/vits_limit.h): `limit`, None, "sample" or "true" (4x oversampled peaks),
        defaulting to the config key inference.limit; `lookahead_ms` / `release_ms` default to inference.limit_lookahead_ms /
        inference.limit_release_ms, else 5 and 50 ms.  peak_ceiling (inference.peak_ceiling, else 1.0) is the limiter's ceiling: with a
        limiter the loudness gain is not capped, the peaks above the ceiling are taken down around themselves and the LUFS target is met
        in two passes.  Without a loudness target it is a plain limiter at gain 1.  The feed gets "vits.limit", "vits.limit_lookahead_ms",
        "vits.limit_release_ms" (and "vits.peak_ceiling"); none given and no config key = off.  A peak target next to a limiter is
        ValueError."""
        from .capi import limit_spec

        inf = self.model.config.get("inference", {})
        if limit is None:
            limit = inf.get("limit")
        if limit is None:
            return False
        if peak_ceiling is None:
            peak_ceiling = inf.get("peak_ceiling")
        la = inf.get("limit_lookahead_ms", 5.0) if lookahead_ms is None else lookahead_ms
        rel = inf.get("limit_release_ms", 50.0) if release_ms is None else release_ms
        limit_spec(limit, peak_ceiling, la, rel)  # (raises on a value out of range)
        if "vits.peak" in args:
            raise ValueError(f"peak={args['vits.peak']} with limit={limit!r}: a peak target leaves a limiter nothing to do (a LUFS target, or the "
                             "limiter alone)")
        args["vits.limit"] = str(limit)
        args["vits.limit_lookahead_ms"] = float(la)
        args["vits.limit_release_ms"] = float(rel)
        if peak_ceiling is not None:
            args["vits.peak_ceiling"] = float(peak_ceiling)
        return True

    def _pitch(self, args, pitch, preserve_formants=None):
        """Pitch shift of the request (include/vits_pitch.h): `pitch` in semitones, [-12, 12], defaulting to the config key
        inference.pitch; it goes into the feed as "vits.pitch".  None and no config key, or a shift that reduces to the identity = off,
        the reference's behaviour.  The engine shifts the finished waveform on the device, behind the decoder and the denoiser and before
        the resampler; duration, sample counts and marks do not change.  Formants move with the pitch unless `preserve_formants`
        (default: the config key inference.pitch_formants, else False) is set: then the feed gets "vits.pitch_formants" and the engine
        keeps the spectral envelope where it was (VITS_FLAG_PITCH_FORMANT).  It modifies a shift: without one in effect the request is
        the request it was, so a voice's config can set it for every request."""
        from .capi import pitch_spec

        if pitch is None:
            pitch = self.model.config.get("inference", {}).get("pitch")
        p = pitch_spec(pitch)  # (raises on a value out of range)
        if p is None:
            return False
        args["vits.pitch"] = p
        if preserve_formants is None:
            preserve_formants = self.model.config.get("inference", {}).get("pitch_formants", False)
        if preserve_formants:
            args["vits.pitch_formants"] = True
        return True

    def _range(self, args, pitch_range):
        """Intonation range of the request (include/vits_intonation.h; both voice families): `pitch_range` r in [0, 4], defaulting to the
        config key inference.pitch_range; it goes into the feed as "vits.pitch_range".  The engine tracks the F0 of the finished waveform
        on the device and scales its movement about the utterance's own median by r: 0 is a monotone, 0.5 a calm reading, 1.5 a lively
        one.  None and no config key, or a value within 0.0005 of 1 = off, the request as it was.  Duration, sample counts and marks do
        not change; a value out of range is a ValueError naming it."""
        from .capi import range_spec

        if pitch_range is None:
            pitch_range = self.model.config.get("inference", {}).get("pitch_range")
        r = range_spec(pitch_range)
        if r is None:
            return False
        args["vits.pitch_range"] = r
        return True

    def _watermark_key(self, watermark):
        """a watermark= / key= argument -> the 32-bit key: True (or None where a key is needed) takes the config key
        inference.watermark_key, a ValueError where the voice's config names none"""
        if watermark is True or watermark is None:
            watermark = self.model.config.get("inference", {}).get("watermark_key")
            if watermark is None:
                raise ValueError("watermark=True needs the config key inference.watermark_key (or pass the key itself)")
        return int(watermark)

    def _watermark(self, args, watermark, watermark_depth_db=None, watermark_payload=None):
        """watermark_payload: an int in [0, 65535] that the mark carries and read_watermark returns (include/vits_watermark_payload.h; the
        feed gets "vits.watermark_payload", and the default depth is then 2 dB); without watermark= it is a ValueError, as is a value out of
        range, before any device work.
        The audio watermark of the request (include/vits_watermark.h; both voice families): `watermark`, a 32-bit key (a selector, not
        a secret) or True for the config key inference.watermark_key; None / False = off, the reference's behaviour (a config key alone
        marks nothing).  watermark_depth_db in (0, 2], default 1 dB.  The feed gets "vits.watermark_key" / "vits.watermark_depth_db"; the
        engine marks the audio on the device behind the resampler, in front of the loudness stage, the limiter and the int16 conversion.
        Sample counts and marks do not change; a value out of range is a ValueError naming it."""
        from .capi import watermark_spec

        if watermark is None or watermark is False:
            if watermark_depth_db is not None:
                raise ValueError("watermark_depth_db needs watermark=")
            if watermark_payload is not None:
                raise ValueError("watermark_payload needs watermark=: VITS_FLAG_WATERMARK_PAYLOAD modifies a watermark request")
            return False
        key, depth, *payload = watermark_spec(self._watermark_key(watermark), watermark_depth_db, watermark_payload)
        args["vits.watermark_key"] = key
        if payload:
            args["vits.watermark_payload"] = payload[0]  # (an int; MultiDeviceSynth.synth_batch: or a tuple, one per request)
        if depth:
            args["vits.watermark_depth_db"] = depth
        return True

    def detect_watermark(self, audio, key=None):
        """(detected, z, offset_samples) of one piece of audio under `key` (default: the config key inference.watermark_key), by the
        engine's own detector (vits_op_watermark_detect): z is the best normalised correlation over the 128 pattern offsets, detected iff
        z >= 6 (a false-alarm bound of 1.9e-6 per item, include/vits_watermark.h), offset_samples how far into the 16384-sample pattern
        the audio starts (a multiple of 128: a crop is found where it was cut).  audio: int16 PCM or float, at the rate it was returned
        at; audio below 513 samples is never detected."""
        from .capi import WATERMARK_THRESHOLD

        k = self._watermark_key(key)
        a = np.asarray(audio)
        x = a.astype(np.float32) / np.float32(32767.0) if a.dtype == np.int16 else a.astype(np.float32)
        x = x.reshape(1, -1)
        sess = self.model.onnx
        lib = getattr(sess, "_lib", None)
        if lib is None or not getattr(lib, "has_watermark", False):
            raise NotImplementedError("this session type has no watermark detector (include/vits_watermark.h)")
        if x.shape[1] == 0:
            return False, 0.0, 0
        dev = getattr(getattr(sess, "_vocoder", None) or getattr(sess, "_model", None), "device", 0)
        z, off, _, _ = lib.op_watermark_detect(x, [x.shape[1]], k, device=dev)
        return bool(z[0] >= WATERMARK_THRESHOLD), float(z[0]), int(off[0])

    def read_watermark(self, audio, key=None):
        """(detected, z, offset_samples, payload_or_None, bit_z) of one piece of audio under `key` (default: the config key
        inference.watermark_key), by the engine's reader (vits_op_watermark_read, include/vits_watermark_payload.h): z is the best
        correlation of the PILOT chips over the 128 pattern offsets, detected iff z >= 6 (the same false-alarm bound of 1.9e-6 per item);
        payload is the 16-bit value the mark carries, None unless the read is valid (detected, and the word's CRC holds: a plain mark
        of the same key is detected and has no payload); bit_z float64 [24]: the score of every coded bit, negative = 1, near 0 = weak.
        audio as for detect_watermark, which is unchanged and is NOT the detector of a payload mark."""
        from .capi import WATERMARK_CODED_BITS, WATERMARK_THRESHOLD

        k = self._watermark_key(key)
        a = np.asarray(audio)
        x = a.astype(np.float32) / np.float32(32767.0) if a.dtype == np.int16 else a.astype(np.float32)
        x = x.reshape(1, -1)
        sess = self.model.onnx
        lib = getattr(sess, "_lib", None)
        if lib is None or not getattr(lib, "has_watermark_payload", False):
            raise NotImplementedError("this session type has no watermark reader (include/vits_watermark_payload.h)")
        if x.shape[1] == 0:
            return False, 0.0, 0, None, np.zeros(WATERMARK_CODED_BITS)
        dev = getattr(getattr(sess, "_vocoder", None) or getattr(sess, "_model", None), "device", 0)
        z, off, _, payload, valid, _, bit_z = lib.op_watermark_read(x, [x.shape[1]], k, device=dev)
        return bool(z[0] >= WATERMARK_THRESHOLD), float(z[0]), int(off[0]), int(payload[0]) if valid[0] else None, bit_z[0]

    def locate_watermark(self, audio, key=None, span=4, payload=False):
        """[WatermarkSegment] (vosk_tts_amd/watermark_scan.py), sorted by start: where in a recording the mark of `key` (default: the
        config key inference.watermark_key) sits, for audio in which marked speech stands between other speech or several marked
        pieces are joined, where the whole-item score of detect_watermark dilutes.  The engine scores every window of `span` pattern
        periods (0.74 s each at 22050 Hz; 1 to 8) at every offset (vits_op_watermark_scan, include/vits_watermark_scan.h); the windows
        over the derived threshold t(Wmax) -- the detector's false-alarm bound of 1.9e-6 per item, spread over all windows -- are
        grouped into segments with start, end (samples; each good to about a span), z and offset_samples.  payload=True: for audio
        marked with a payload -- the scan scores the pilot positions only, each segment's crop goes through read_watermark, and the
        segment carries payload (None unless that read is valid) and bit_z.  audio as for detect_watermark; audio shorter than span
        periods has no window and no segment."""
        from .watermark_scan import segments, span_arg

        k = self._watermark_key(key)
        S = span_arg(span)
        a = np.asarray(audio)
        x = a.astype(np.float32) / np.float32(32767.0) if a.dtype == np.int16 else a.astype(np.float32)
        x = x.reshape(1, -1)
        sess = self.model.onnx
        lib = getattr(sess, "_lib", None)
        if lib is None or not getattr(lib, "has_watermark_scan", False):
            raise NotImplementedError("this session type has no watermark scan (include/vits_watermark_scan.h)")
        if x.shape[1] == 0:
            return []
        dev = getattr(getattr(sess, "_vocoder", None) or getattr(sess, "_model", None), "device", 0)
        z_scan, first, wins = lib.op_watermark_scan(x, [x.shape[1]], k, span=S, pilots=bool(payload), device=dev)
        segs = segments(z_scan[0], first[0], wins[0], S, x.shape[1])
        if payload:
            for s in segs:
                _, _, _, s.payload, s.bit_z = self.read_watermark(x[0, s.start:s.end], k)
        return segs

    def measure_pitch(self, audio, rate=None):
        """(hz, median_hz) of one utterance: hz float32 [1 + n // 256], the F0 of every analysis frame of include/vits_intonation.h (hop
        256, 0 where unvoiced) as the engine's own tracker finds it (vits_op_f0_track, the track `pitch_range` scales), and the median of
        the voiced frames (0.0 without one).  audio: int16 PCM or float; rate: its sample rate in Hz (default: the voice's own), tracked at
        that rate if the tracker takes it (8 to 32 kHz)."""
        a = np.asarray(audio)
        x = a.astype(np.float32) / np.float32(32767.0) if a.dtype == np.int16 else a.astype(np.float32)
        x = x.reshape(1, -1)
        sess = self.model.onnx
        lib = getattr(sess, "_lib", None)
        if lib is None or not getattr(lib, "has_intonation", False):
            raise NotImplementedError("this session type has no F0 tracker (include/vits_intonation.h)")
        if x.shape[1] == 0:
            return np.zeros(1, np.float32), 0.0
        dev = getattr(getattr(sess, "_vocoder", None) or getattr(sess, "_model", None), "device", 0)
        cents = lib.op_f0_track(x, [x.shape[1]], int(rate or self.native_rate()), device=dev)[0]
        voiced = cents > 0
        hz = np.where(voiced, 27.5 * 2.0 ** (cents / 1200.0), 0.0).astype(np.float32)
        med = float(27.5 * 2.0 ** (np.sort(cents[voiced])[(int(voiced.sum()) - 1) // 2] / 1200.0)) if voiced.any() else 0.0
        return hz, med

    def measure_loudness(self, audio, rate=None, true_peak=False):
        """(lufs, peak) of one utterance: BS.1770 integrated loudness (-inf for silence) and max |sample| in full-scale units, measured
        by the engine's own kernels (vits_op_loudness).  audio: int16 PCM (scaled by 1 / 32767, the conversion's own factor) or float;
        rate: its sample rate in Hz (default: the voice's own).  true_peak=True: (lufs, peak, true_peak), the last the 4x oversampled
        peak of include/vits_limit.h (vits_op_true_peak)."""
        a = np.asarray(audio)
        x = a.astype(np.float32) / np.float32(32767.0) if a.dtype == np.int16 else a.astype(np.float32)
        x = x.reshape(1, -1)
        sess = self.model.onnx
        lib = getattr(sess, "_lib", None)
        if lib is None or not getattr(lib, "has_loudness", False):
            raise NotImplementedError("this session type has no loudness measurement (include/vits_loudness.h)")
        if true_peak and not getattr(lib, "has_limit", False):
            raise NotImplementedError("this session type has no true-peak measurement (include/vits_limit.h)")
        if x.shape[1] == 0:
            return (float("-inf"), 0.0, 0.0) if true_peak else (float("-inf"), 0.0)
        dev = getattr(getattr(sess, "_vocoder", None) or getattr(sess, "_model", None), "device", 0)
        loud, pk = lib.op_loudness(x, [x.shape[1]], int(rate or self.native_rate()), device=dev)
        if true_peak:
            return float(loud[0]), float(pk[0]), float(lib.op_true_peak(x, [x.shape[1]], int(rate or self.native_rate()), device=dev)[0])
        return float(loud[0]), float(pk[0])

    def hop_length(self):
        """frames to samples at the voice's own rate (the session's hparams; 256 for sessions that do not say)"""
        sess = self.model.onnx
        hp = getattr(getattr(sess, "_vocoder", None), "hp", None) or getattr(sess, "hp", None)
        return int(getattr(hp, "hop_length", 0) or 256)

    def _prosody_text(self, text, word_rates, pauses, duration):
        """Before the front end sees the text: a multistream voice refuses the prosody keywords (that family keeps its own '_' markup),
        and with the config key inference.pause_markup a VITS voice accepts the reference's '_' behind a word as a pause of
        inference.pause_frames frames (default 20, the reference's value; off by default: '_' then reaches the front end as before).
        -> (text, pauses)"""
        multistream = (self.model.config.get("model_type") or "").startswith("multistream")
        if multistream:
            if word_rates or pauses or duration is not None:
                raise ValueError("word_rates / pauses / duration are the prosody controls of the VITS-family voices; a multistream voice keeps "
                                 "its own '_' pause markup")
            return text, pauses
        inf = self.model.config.get("inference", {})
        if inf.get("pause_markup") and "_" in text:
            from .prosody import PAUSE_FRAMES, split_pause_markup

            text, after = split_pause_markup(text)
            sec = int(inf.get("pause_frames", PAUSE_FRAMES)) * self.hop_length() / self.native_rate()
            pauses = dict(pauses or {})
            for w in after:
                pauses[w] = pauses.get(w, 0.0) + sec
        return text, pauses

    def _prosody(self, args, text, word_rates=None, pauses=None, duration=None):
        """Prosody controls of the request (include/vits_prosody.h; VITS-family voices): word_rates {word index: rate}, pauses {word
        index: seconds behind that word}, duration = seconds the whole utterance is fitted to.  Words are counted as the speech marks
        count them.  The feed gets "vits.token_length_scale", "vits.token_pause" (vosk_tts_amd/prosody.py token_controls) and
        "vits.fit_frames" = round(duration * rate / hop); none given = off, the reference's behaviour."""
        if not word_rates and not pauses and duration is None:
            return False
        from . import prosody as P

        rate, hop = self.native_rate(), self.hop_length()
        tls, pause = P.token_controls(self.marks_layout(text), word_rates, pauses, rate, hop)
        T = np.asarray(args["input"]).shape[-1]
        for name, a in (("vits.token_length_scale", tls), ("vits.token_pause", pause)):
            if a is None:
                continue
            if a.shape[0] != T:
                raise ValueError(f"token layout does not match: {a.shape[0]} tokens laid out for {T} ids")
            args[name] = a[None]
        if duration is not None:
            F = P.frames(duration, rate, hop)
            if F <= 0:
                raise ValueError(f"duration {duration} s is less than one frame ({hop} samples at {rate} Hz)")
            args["vits.fit_frames"] = np.array([F], np.int32)
        return True

    def _contour(self, args, text, word_pitch=None, word_gains=None):
        """Per-word pitch and volume of the request (include/vits_contour.h; both voice families): word_pitch {word index: semitones},
        word_gains {word index: dB}, words counted as the speech marks count them.  A word's setting covers the tokens of its phonemes
        and the blank in front of each; the engine ramps between neighbours over about 100 ms.  The feed gets "vits.token_pitch" /
        "vits.token_gain_db" (vosk_tts_amd/prosody.py token_contour); none given = off.  Values out of range are a ValueError here."""
        if not word_pitch and not word_gains:
            return False
        from . import prosody as P

        tp, tg = P.token_contour(self.marks_layout(text), word_pitch, word_gains)
        T = np.asarray(args["input"]).shape[-1]
        for name, a in (("vits.token_pitch", tp), ("vits.token_gain_db", tg)):
            if a is None:
                continue
            if a.shape[0] != T:
                raise ValueError(f"token layout does not match: {a.shape[0]} tokens laid out for {T} ids")
            args[name] = a[None]
        return True

    def marks_layout(self, text):
        """The token layout of `text` under the front end _feed picks, for speech marks (vosk_tts_amd/marks.py):
        -> (symbols, ids per symbol, blank layout?, word_of per symbol, word_texts).  Needs the voice's config and dictionary only."""
        from . import marks as M

        text = self.normalize(text)
        model_type = self.model.config.get("model_type") or ""
        have_bert = self.model.tokenizer is not None
        if model_type.startswith("multistream"):
            from .multistream import g2p_multistream

            v3 = model_type == "multistream_v3" and have_bert
            res = g2p_multistream(text, self.model.dic, self.model.config["phoneme_id_map"], None, word_pos=model_type == "multistream_v2",
                                  pause_marks=v3, return_words=True)
            symbols, word_of, word_texts = M.multistream_layout(*res[-1])
            return symbols, [1] * len(symbols), False, word_of, word_texts
        symbols, word_of, word_texts = M.vits_layout(
            text, lambda w: (self.model.dic[w] if w in self.model.dic else convert(w)).split())
        if have_bert:
            return symbols, [1] * len(symbols), self.model.config.get("no_blank", 0) == 0, word_of, word_texts
        id_map = self.model.config["phoneme_id_map"]
        return symbols, [len(id_map[p]) if isinstance(id_map[p], list) else 1 for p in symbols], True, word_of, word_texts

    def _marks(self, text, token_ends, rate):
        from .marks import build_marks

        symbols, counts, blank, word_of, word_texts = self.marks_layout(text)
        return build_marks(rate, np.asarray(token_ends).reshape(-1), symbols, counts, blank, word_of, word_texts)

    def synth_audio(self, text, speaker_id=0, noise_level=None, speech_rate=None, duration_noise_level=None, scale=None, sample_rate=None,
                    denoiser_strength=None, marks=False, loudness=None, peak=None, peak_ceiling=None, pitch=None,
                    preserve_formants=None, limit=None, limit_lookahead_ms=None, limit_release_ms=None, word_rates=None, pauses=None,
                    duration=None, word_pitch=None, word_gains=None, pitch_range=None, watermark=None, watermark_depth_db=None,
                    watermark_payload=None):
        """watermark_payload (extension): 16 bits inside the mark, which read_watermark returns, see _watermark.
        watermark / watermark_depth_db (extension): a keyed mark in the returned audio that detect_watermark recognises, see _watermark.
        pitch_range (extension): the intonation range, 0 (monotone) to 4, 1 = unchanged, see _range.
        word_pitch / word_gains (extension): per-word semitones and decibels, see _contour.
        word_rates / pauses / duration (extension): per-word tempo, pauses behind words and the length of the whole utterance in
        seconds, see _prosody.
        limit / limit_lookahead_ms / limit_release_ms (extension): the look-ahead peak limiter, see _limit; peak_ceiling is then its
        ceiling.
        pitch / preserve_formants (extension): semitones by which the returned audio is shifted, and whether its formants stay where
        they were, see _pitch.
        sample_rate: output rate in Hz (extension; default None = the voice's own rate, the reference's behaviour): the feed gets
        "vits.sample_rate" and the engine resamples on the device.  denoiser_strength: see _denoiser.
        loudness / peak / peak_ceiling (extension): a LUFS or a peak target for the returned audio, see _loudness.
        marks=True (extension): returns (audio, marks) -- marks.SpeechMarks with rate, token_ends, phonemes [(symbol, start, end)] and
        words [(text, start, end)] in samples of the returned audio, and seconds(); the default returns the array alone."""
        text, pauses = self._prosody_text(text, word_rates, pauses, duration)
        args, scale = self._feed(text, speaker_id, noise_level, speech_rate, duration_noise_level, scale)
        self._prosody(args, self.normalize(text), word_rates, pauses, duration)
        self._contour(args, self.normalize(text), word_pitch, word_gains)
        self._denoiser(args, denoiser_strength)
        self._loudness(args, loudness, peak, peak_ceiling)
        self._limit(args, limit, peak_ceiling, limit_lookahead_ms, limit_release_ms)
        self._pitch(args, pitch, preserve_formants)
        self._range(args, pitch_range)
        self._watermark(args, watermark, watermark_depth_db, watermark_payload)
        rate = self.native_rate()
        if sample_rate and int(sample_rate) != rate:
            rate = int(sample_rate)
            args["vits.sample_rate"] = rate
        if marks:
            args["vits.marks"] = True

        start_time = time.perf_counter()
        run_pcm16 = getattr(self.model.onnx, "run_pcm16", None)
        ends = None
        if run_pcm16 is not None:
            # same three steps as below (squeeze, * scale, audio_float_to_int16) fused behind the boundary: the device
            # converts and only int16 crosses PCIe (vits_synthesize_pcm16)
            audio = run_pcm16(args, scale)
            if marks:
                audio, ends = audio
            audio = audio.squeeze()
        else:
            audio = self.model.onnx.run(None, args)
            if marks:
                ends = audio[-1]
            audio = audio[0]
            audio = audio.squeeze()
            audio = audio * scale
            audio = self.audio_float_to_int16(audio)
        end_time = time.perf_counter()

        audio_duration_sec = audio.shape[-1] / rate
        infer_sec = end_time - start_time
        real_time_factor = infer_sec / audio_duration_sec if audio_duration_sec > 0 else 0.0
        logging.info("Real-time factor: %0.2f (infer=%0.2f sec, audio=%0.2f sec)" % (real_time_factor, infer_sec, audio_duration_sec))
        if marks:
            return audio, self._marks(text, ends, rate)
        return audio

    def synth_ssml(self, ssml, **kw):
        """synth_audio for an SSML document (vosk_tts_amd/ssml.py: speak, p, s, sub, break, prosody rate / pitch / volume, mark): the
        document becomes the text and the word_rates / pauses / word_pitch / word_gains keywords, so those four are not accepted next
        to it; every other keyword of synth_audio is (a `range` on a prosody element that covers the whole document becomes pitch_range,
        and a pitch_range keyword next to it is refused the same way).  With marks=True the returned marks carry `named`: {mark name: start sample of the
        next word, or the end of the audio behind the last one}.  Whatever the subset does not cover is a ValueError before the model
        is touched; on a multistream voice rate and break raise that family's own refusal."""
        from . import ssml as S

        plan = S.parse(ssml)
        for k in ("word_rates", "pauses", "word_pitch", "word_gains") + (("pitch_range",) if plan.pitch_range is not None else ()):
            if kw.get(k) is not None:
                raise ValueError(f"synth_ssml takes {k} from the document's markup, not as a keyword")
        res = self.synth_audio(plan.text, **dict(kw, **plan.keywords()))
        if kw.get("marks"):
            audio, sm = res
            sm.named = {name: (int(sm.words[w][1]) if w < len(sm.words) else int(audio.shape[-1])) for name, w in plan.marks}
        return res

    # ---- documents (include/vits_document.h; vosk_tts_amd/document.py) ---------------------------------------------------------
    def count_tokens(self, text):
        """how many tokens the front end _feed picks makes of `text` (what document.split counts sentences in)"""
        text = self.normalize(text)
        if self.model.tokenizer is None and not (self.model.config.get("model_type") or "").startswith("multistream"):
            return len(self.g2p_noembed(text))
        return int(self._front_rows(text)[0].shape[-1])

    def _document_feed(self, segments, speaker_id, noise_level, speech_rate, duration_noise_level, scale):
        """The batch feed of a document's segments: one front end (front_batch for the BERT-conditioned and multistream voices, else
        g2p_noembed per segment, padded), per-segment speakers, rates (-> "vits.item_scales") and per-word controls
        (-> "vits.token_length_scale" / "vits.token_pause" / "vits.token_pitch" / "vits.token_gain_db", rows padded with their neutral
        values).  -> (feed, scale)"""
        from . import prosody as P

        inf = self.model.config.get("inference", {})
        noise_level = inf.get("noise_level", 0.8) if noise_level is None else noise_level
        speech_rate = inf.get("speech_rate", 1.0) if speech_rate is None else speech_rate
        duration_noise_level = inf.get("duration_noise_level", 0.8) if duration_noise_level is None else duration_noise_level
        scale = inf.get("scale", 1.0) if scale is None else scale
        multistream = (self.model.config.get("model_type") or "").startswith("multistream")
        texts = [self.normalize(s.text) for s in segments]
        sids = [int((speaker_id or 0) if s.speaker_id is None else s.speaker_id) for s in segments]
        B = len(segments)
        if multistream or self.model.tokenizer is not None:
            fb = self.front_batch(texts, sids)
            ids, lens, bert, pde = fb["input"], fb["input_lengths"], fb["bert"], fb["phone_duration_extra"]
        else:
            rows = [np.array(self.g2p_noembed(t), np.int64) for t in texts]
            lens = np.array([r.shape[0] for r in rows], np.int64)
            ids = np.zeros((B, int(lens.max())), np.int64)
            for b, r in enumerate(rows):
                ids[b, :lens[b]] = r
            bert = pde = None
        T = ids.shape[-1]
        feed = {"input": ids, "input_lengths": lens, "scales": np.array([noise_level, 1.0 / speech_rate, duration_noise_level], np.float32),
                "sid": np.array(sids, np.int64), "bert": bert, "phone_duration_extra": pde}
        if any(s.speech_rate is not None for s in segments):
            if multistream:
                raise ValueError("Segment.speech_rate is a prosody control of the VITS-family voices (\"vits.item_scales\"); a multistream "
                                 "voice has one rate per call")
            feed["vits.item_scales"] = np.array([[noise_level, 1.0 / (speech_rate if s.speech_rate is None else s.speech_rate),
                                                  duration_noise_level] for s in segments], np.float32)
        rate, hop = self.native_rate(), self.hop_length()
        rows = {"vits.token_length_scale": (np.ones((B, T), np.float32), False), "vits.token_pause": (np.zeros((B, T), np.int32), False),
                "vits.token_pitch": (np.zeros((B, T), np.float32), False), "vits.token_gain_db": (np.zeros((B, T), np.float32), False)}
        for b, (s, text) in enumerate(zip(segments, texts)):
            if multistream and (s.word_rates or s.pauses):
                self._prosody_text(text, s.word_rates, s.pauses, None)  # (that family's own refusal)
            vals = {}
            if s.word_rates or s.pauses:
                vals["vits.token_length_scale"], vals["vits.token_pause"] = P.token_controls(self.marks_layout(text), s.word_rates, s.pauses, rate, hop)
            if s.word_pitch or s.word_gains:
                vals["vits.token_pitch"], vals["vits.token_gain_db"] = P.token_contour(self.marks_layout(text), s.word_pitch, s.word_gains)
            for k, a in vals.items():
                if a is None:
                    continue
                if a.shape[0] != int(lens[b]):
                    raise ValueError(f"token layout of segment {b} does not match: {a.shape[0]} tokens laid out for {int(lens[b])} ids")
                rows[k][0][b, :a.shape[0]] = a
                rows[k] = (rows[k][0], True)
        for k, (a, used) in rows.items():
            if used:
                feed[k] = a
        return feed, scale

    def synth_document(self, doc, speaker_id=0, sentence_pause=0.2, paragraph_pause=0.6, lead=0.0, fade_ms=2.0, trim_db=None, trim_keep=1,
                       marks=False, seed=None, noise_level=None, speech_rate=None, duration_noise_level=None, scale=None, sample_rate=None,
                       denoiser_strength=None, loudness=None, peak=None, peak_ceiling=None, pitch=None, preserve_formants=None, limit=None,
                       limit_lookahead_ms=None, limit_release_ms=None, pitch_range=None, max_tokens=None, watermark=None,
                       watermark_depth_db=None, watermark_payload=None, **refused):
        """Many sentences and speakers in one call (extension; include/vits_document.h).  doc: a string -- split by document.split into
        sentences and paragraphs under the documented rule, sentences longer than max_tokens (default 512) tokens cut at clause marks --
        or a list of document.Segment(text, speaker_id=None, pause_after=None, speech_rate=None, word_rates=, pauses=, word_pitch=,
        word_gains=).  The segments are synthesised as one batch, every one as if alone, and joined on the device: `lead` seconds of
        silence in front, sentence_pause (default 0.2 s) / paragraph_pause (default 0.6 s; both design choices, not measurements) or a
        segment's own pause_after behind each, the last one trailing; fade_ms raised-cosine fades at both ends of every segment (at most
        half a frame); trim_db (None = off, else a negative dBFS value) cuts the frames below it from both ends of every segment, keeping
        trim_keep frames.  Seconds become frames as floor(sec * rate / hop + 0.5).  The resampler (sample_rate), the loudness target, the
        limiter and the int16 conversion then see ONE piece of audio, as does the watermark (watermark=, see _watermark) in front of them;
        pitch and pitch_range are one value per call, applied per segment.
        Returns int16 audio; with marks=True (audio, SpeechMarks) whose words and phonemes run over the whole document, plus
        marks.segments = [(start, end)] in samples.  The call-wide per-word keywords of synth_audio (word_rates, pauses, duration,
        word_pitch, word_gains) index one utterance and are refused by name: they belong to a Segment."""
        from . import document as D

        for k in refused:
            if k in ("word_rates", "pauses", "duration", "word_pitch", "word_gains"):
                raise ValueError(f"synth_document takes no {k}=: it indexes the words of one utterance (give it to a document.Segment)")
            raise TypeError(f"synth_document() got an unexpected keyword argument {k!r}")
        segments = D.split(doc, max_tokens or D.MAX_TOKENS, self.count_tokens) if isinstance(doc, str) else list(doc)
        if not segments:
            raise ValueError("an empty document")
        for b, s in enumerate(segments):
            if not isinstance(s, D.Segment):
                raise TypeError(f"segment {b} is {type(s).__name__}: a document is a string or a list of document.Segment")
            if not D.has_word(s.text):
                raise ValueError(f"segment {b} ({s.text!r}) has no word")
        rate, hop = self.native_rate(), self.hop_length()
        args, scale = self._document_feed(segments, speaker_id, noise_level, speech_rate, duration_noise_level, scale)
        args["vits.doc_gap_frames"] = D.gap_frames(segments, sentence_pause, paragraph_pause, rate, hop)
        args["vits.doc_lead_frames"] = D.frames(lead, rate, hop)
        fade = int(math.floor(float(fade_ms) * rate / 1000.0 + 0.5))
        if fade < 0 or fade > hop // 2:
            raise ValueError(f"fade_ms {fade_ms}: {fade} samples at {rate} Hz, outside [0, half a frame = {hop // 2}]")
        args["vits.doc_fade_samples"] = fade
        if trim_db is not None:
            if not (math.isfinite(float(trim_db)) and float(trim_db) < 0):
                raise ValueError(f"trim_db {trim_db}: None (off) or a negative finite dBFS value")
            args["vits.doc_trim_db"] = float(trim_db)
            args["vits.doc_trim_keep"] = int(trim_keep)
        if seed is not None:
            args["vits.seed"] = int(seed)
        self._denoiser(args, denoiser_strength)
        self._loudness(args, loudness, peak, peak_ceiling)
        self._limit(args, limit, peak_ceiling, limit_lookahead_ms, limit_release_ms)
        self._pitch(args, pitch, preserve_formants)
        self._range(args, pitch_range)
        self._watermark(args, watermark, watermark_depth_db, watermark_payload)
        out_rate = rate
        if sample_rate and int(sample_rate) != rate:
            out_rate = int(sample_rate)
            args["vits.sample_rate"] = out_rate
        if marks:
            args["vits.marks"] = True
        run = getattr(self.model.onnx, "run_document", None)
        if run is None:
            raise NotImplementedError("this session type has no run_document (VitsSession: vits_synthesize_document_pcm16, SttsSession: "
                                      "stts_synthesize_document)")
        start_time = time.perf_counter()
        audio, info = run(args, scale=scale, pcm16=True)
        infer_sec = time.perf_counter() - start_time
        sec = audio.shape[-1] / out_rate
        logging.info("Real-time factor: %0.2f (infer=%0.2f sec, audio=%0.2f sec)" % (infer_sec / sec if sec > 0 else 0.0, infer_sec, sec))
        if not marks:
            return audio
        sm = D.stitch_marks(out_rate, info["token_ends"], args["input_lengths"], [self.marks_layout(s.text) for s in segments],
                            info["seg_start"], info["seg_end"])
        return audio, sm

    def synth_document_ssml(self, ssml, **kw):
        """synth_document for an SSML document (ssml.parse_document): <s>, <p> and <voice name="N"> (N an integer speaker id) end a
        segment, a <break> at a segment boundary becomes the silence there, prosody / sub / mark work per segment as in synth_ssml, and a
        prosody `range` around the whole document becomes pitch_range.  With marks=True the marks carry `named` as synth_ssml's do."""
        from . import ssml as S

        plan = S.parse_document(ssml)
        if plan.pitch_range is not None:
            if kw.get("pitch_range") is not None:
                raise ValueError("synth_document_ssml takes pitch_range from the document's markup, not as a keyword")
            kw = dict(kw, pitch_range=plan.pitch_range)
        if plan.lead:
            if kw.get("lead"):
                raise ValueError("synth_document_ssml takes lead from the <break> in front of the first segment, not as a keyword")
            kw = dict(kw, lead=plan.lead)
        res = self.synth_document(plan.segments, **kw)
        if kw.get("marks"):
            audio, sm = res
            sm.named = {name: (int(sm.words[w][1]) if w < len(sm.words) else int(audio.shape[-1])) for name, w in plan.marks}
        return res

    def synth_stream(self, text, speaker_id=0, noise_level=None, speech_rate=None, duration_noise_level=None, scale=None,
                     chunk_frames=64, sample_rate=None, denoiser_strength=None, on_marks=None, loudness=None, peak=None, peak_ceiling=None,
                     pitch=None, limit=None, word_rates=None, pauses=None, duration=None, pitch_range=None, document=None, watermark=None,
                     watermark_payload=None):
        """watermark_payload: ValueError naming VITS_FLAG_WATERMARK_PAYLOAD, as for watermark.
        watermark: ValueError naming VITS_FLAG_WATERMARK -- the mark is a stage of the output tail, and a stream has none.
        document: ValueError -- the join and the stages behind it need every segment before the first chunk (synth_document).
        word_rates / pauses / duration: as for synth_audio (the stream's open runs the controlled regulator; chunking is untouched).
        pitch_range: ValueError -- the median of the F0 track needs the whole utterance (a voice whose config names
        inference.pitch_range streams with the range it has).
        limit: ValueError -- the limiter's look-ahead and its loudness passes need the whole utterance (a voice whose config names
        inference.limit streams unlimited).
        pitch: ValueError -- the phase recursion needs the frames before a chunk (a voice whose config names inference.pitch streams
        unshifted).
        Generator of int16 PCM chunks (chunk_frames*256 samples each, ~0.74 s at the default): what a streaming
        `SynthesizeStream` handler would put into successive AudioChunk messages (tts_service.proto:46-54) instead
        of the single whole-utterance chunk of tts_server.py:54.  Same conversion as synth_audio per chunk.
        on_marks: a callable that receives the utterance's marks.SpeechMarks once, before the first chunk is yielded.
        loudness / peak: ValueError -- an integrated-loudness or peak target needs the whole utterance before the first chunk (a voice
        whose config names inference.loudness / inference.peak streams un-normalised)."""
        if document is not None:
            raise ValueError("synth_stream cannot take document=: the join and the stages behind it need every segment before the first "
                             "chunk (synth_document takes a document)")
        if watermark_payload is not None:
            raise ValueError("synth_stream cannot carry a watermark payload (VITS_FLAG_WATERMARK_PAYLOAD): the mark is a stage of the output "
                             "tail, and a stream has none (synth_audio takes watermark= and watermark_payload=)")
        if watermark is not None and watermark is not False:
            raise ValueError("synth_stream cannot watermark (VITS_FLAG_WATERMARK): the mark is a stage of the output tail, and a stream has "
                             "none (synth_audio takes watermark=)")
        if loudness is not None or peak is not None:
            raise ValueError("synth_stream cannot normalise loudness: an integrated-loudness or peak target needs the whole utterance "
                             "before the first chunk (synth_audio takes loudness= / peak=)")
        if limit is not None:
            raise ValueError("synth_stream cannot limit: the limiter's look-ahead and its loudness passes need the whole utterance before the "
                             "first chunk (synth_audio takes limit=)")
        if pitch_range is not None:
            raise ValueError("synth_stream cannot change the intonation range: the median of the F0 track needs the whole utterance before "
                             "the first chunk (synth_audio takes pitch_range=)")
        if pitch is not None:
            raise ValueError("synth_stream cannot shift the pitch: the phase recursion needs the frames before a chunk, and its state is "
                             "not carried across chunks (synth_audio takes pitch=)")
        text, pauses = self._prosody_text(text, word_rates, pauses, duration)
        args, scale = self._feed(text, speaker_id, noise_level, speech_rate, duration_noise_level, scale)
        self._prosody(args, self.normalize(text), word_rates, pauses, duration)
        self._denoiser(args, denoiser_strength)
        if not hasattr(self.model.onnx, "run_stream"):
            raise NotImplementedError("this session type has no run_stream (VitsSession: vits_stream_open, SttsSession: stts_stream_open)")
        rate = self.native_rate()
        if sample_rate and int(sample_rate) != rate:
            rate = int(sample_rate)
            args["vits.sample_rate"] = rate
        kw = {}
        if on_marks is not None:
            kw["on_marks"] = lambda ends: on_marks(self._marks(text, ends, rate))
        for chunk in self.model.onnx.run_stream(None, args, chunk_frames=chunk_frames, **kw):
            yield self.audio_float_to_int16(chunk * scale)

    def synth(self, text, oname, speaker_id=0, noise_level=None, speech_rate=None, duration_noise_level=None, scale=None, sample_rate=None,
              denoiser_strength=None, marks=False, loudness=None, peak=None, peak_ceiling=None, pitch=None, preserve_formants=None,
              limit=None, limit_lookahead_ms=None, limit_release_ms=None, word_rates=None, pauses=None, duration=None, word_pitch=None,
              word_gains=None, pitch_range=None, watermark=None, watermark_depth_db=None, watermark_payload=None):
        """marks=True: the utterance's marks.SpeechMarks are returned (the default returns None, as the reference does)"""
        audio = self.synth_audio(text, speaker_id, noise_level, speech_rate, duration_noise_level, scale, sample_rate, denoiser_strength, marks=marks,
                                 loudness=loudness, peak=peak, peak_ceiling=peak_ceiling, pitch=pitch,
                                 preserve_formants=preserve_formants, limit=limit, limit_lookahead_ms=limit_lookahead_ms,
                                 limit_release_ms=limit_release_ms, **{k: v for k, v in (("word_rates", word_rates), ("pauses", pauses), ("duration", duration),
                                                                                           ("word_pitch", word_pitch), ("word_gains", word_gains),
                                                                                           ("pitch_range", pitch_range), ("watermark", watermark),
                                                                                           ("watermark_depth_db", watermark_depth_db),
                                                                                           ("watermark_payload", watermark_payload))
                                                                      if v is not None})
        sm = None
        if marks:
            audio, sm = audio
        with wave.open(oname, "w") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(int(sample_rate) if sample_rate else self.native_rate())
            f.writeframes(audio.tobytes())
        return sm

    def _phonemes_and_words(self, text):
        """One pass over the split text: the phoneme string ('^' ... '$', punctuation kept, dictionary or rule G2P per word) and,
        per phoneme, the index of the token it belongs to in get_word_bert's row order: 0 = '^' ([CLS]), tokens counted from 1,
        spaces emit a phoneme but do not advance the count, -1 = '$' ([SEP])  (synth.py:152-171 / 190-209 / 224-236)."""
        phonemes, words = ["^"], [0]
        w = 1
        for token in re.split(_SPLIT, text.lower()):
            if token == "":
                continue
            if re.match(_SPLIT, token) or token == "-":
                ps = [token]
            elif token in self.model.dic:
                ps = self.model.dic[token].split()
            else:
                ps = convert(token).split()
            phonemes.extend(ps)
            words.extend([w] * len(ps))
            if token != " ":
                w += 1
        phonemes.append("$")
        words.append(-1)
        return phonemes, words

    def phonemize(self, text):
        """Words -> dictionary lookup or rule G2P, punctuation kept, '^' ... '$' (synth.py:224-236)."""
        return self._phonemes_and_words(text)[0]

    def g2p_noblank(self, text, embeddings):
        """BERT-conditioned front-end without blanks (synth.py:190-220): ids of the phoneme string and, per phoneme, the BERT row
        of its word (embeddings[0] for '^', embeddings[-1] for '$')."""
        phonemes, words = self._phonemes_and_words(text)
        id_map = self.model.config["phoneme_id_map"]
        logging.info(f"Text: {text}")
        logging.info(f"Phonemes: {phonemes}")
        return [id_map[p] for p in phonemes], [embeddings[w] for w in words]

    def g2p(self, text, embeddings):
        """BERT-conditioned front-end with the interspersed blank 0 (synth.py:152-188): every blank carries the BERT row of the
        phoneme that FOLLOWS it."""
        ids, emb = self.g2p_noblank(text, embeddings)
        out_ids, out_emb = [ids[0]], [emb[0]]
        for i, e in zip(ids[1:], emb[1:]):
            out_ids += [0, i]
            out_emb += [e, e]
        return out_ids, out_emb

    def g2p_noembed(self, text):
        phonemes = self.phonemize(text)
        # ids interspersed with blank 0; id-map values may be lists (synth.py:238-251)
        id_map = self.model.config["phoneme_id_map"]
        as_list = (lambda v: list(v)) if isinstance(id_map[phonemes[0]], list) else (lambda v: [v])
        phoneme_ids = as_list(id_map[phonemes[0]])
        for p in phonemes[1:]:
            phoneme_ids.append(0)
            phoneme_ids.extend(as_list(id_map[p]))
        logging.info(f"Text: {text}")
        logging.info(f"Phonemes: {phonemes}")
        return phoneme_ids
