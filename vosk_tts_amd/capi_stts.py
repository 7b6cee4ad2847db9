"""ctypes binding of include/stts_mi355.h (StableTTS / Matcha "multistream" path).  Like capi.VitsLib the class
takes an explicit (library, prefix) so the tests can point it at the CPU oracle; the product default is the HIP
library and there is no CPU fallback."""
import ctypes

import numpy as np

from .capi import (LIMIT_FIELDS, Contour, TailFamily, VitsError, VitsLib, _f32, _i32, _i64, _p, c_f32p, c_i32p, c_i64p, contour_arrays,
                   pitch_spec, set_contour, tail_of, watermark_spec)
from .weights_stts import SttsHParams


STTS_FLAG_ITEM_SEEDS = 1  # include/stts_mi355.h
STTS_FLAG_DENOISE = 2     # include/vits_denoise.h


class SttsOpts(ctypes.Structure):
    _fields_ = [("noise", c_f32p), ("noise_stride", ctypes.c_int64), ("seed", ctypes.c_uint64),
                ("n_timesteps", ctypes.c_int32), ("flags", ctypes.c_int32), ("item_seeds", ctypes.POINTER(ctypes.c_uint64)),
                ("denoiser_strength", ctypes.c_float), ("denoiser_filter_length", ctypes.c_int32)]


class SttsLoudnessOpts(SttsOpts):
    """mirror of `struct stts_synth_opts_loudness` (include/vits_loudness.h): SttsOpts followed by the five loudness fields, which the
    library reads only under STTS_FLAG_LOUDNESS; passed where a POINTER(SttsOpts) is declared"""

    _fields_ = [("loudness_mode", ctypes.c_int32), ("loudness_target", ctypes.c_float), ("loudness_ceiling", ctypes.c_float),
                ("out_loudness", c_f32p), ("out_gain", c_f32p)]


STTS_FLAG_LOUDNESS = 4    # include/vits_loudness.h
STTS_FLAG_PITCH = 8       # include/vits_pitch.h
STTS_FLAG_PITCH_FORMANT = 16  # ... keep the spectral envelope where it was; modifies a pitch request
FLAG_PITCH_FORMANT = STTS_FLAG_PITCH_FORMANT


class SttsPitchOpts(SttsLoudnessOpts):
    """mirror of `struct stts_synth_opts_pitch` (include/vits_pitch.h): SttsLoudnessOpts followed by pitch_semitones, which the library
    reads only under STTS_FLAG_PITCH (the loudness fields inside still only under their own flag)"""

    _fields_ = [("pitch_semitones", ctypes.c_float)]


STTS_FLAG_LIMIT = 32      # include/vits_limit.h


class SttsLimitOpts(SttsPitchOpts):
    """mirror of `struct stts_synth_opts_limit` (include/vits_limit.h): SttsPitchOpts followed by the six limiter fields, which the library
    reads only under STTS_FLAG_LIMIT"""

    _fields_ = LIMIT_FIELDS


STTS_FLAG_CONTOUR = 64    # include/vits_contour.h


class SttsContourOpts(SttsLimitOpts):
    """mirror of `struct stts_synth_opts_contour` (include/vits_contour.h): SttsLimitOpts followed by the pointer to the contour, which
    the library reads only under STTS_FLAG_CONTOUR"""

    _fields_ = [("contour", ctypes.POINTER(Contour))]


STTS_FLAG_INTONATION = 128    # include/vits_intonation.h


class SttsIntonationOpts(SttsContourOpts):
    """mirror of `struct stts_synth_opts_intonation` (include/vits_intonation.h): SttsContourOpts followed by pitch_range, which the
    library reads only under STTS_FLAG_INTONATION"""

    _fields_ = [("pitch_range", ctypes.c_float)]


STTS_FLAG_WATERMARK = 256     # include/vits_watermark.h


class SttsWatermarkOpts(SttsIntonationOpts):
    """mirror of `struct stts_synth_opts_watermark` (include/vits_watermark.h): SttsIntonationOpts followed by the key and the depth, which
    the library reads only under STTS_FLAG_WATERMARK"""

    _fields_ = [("watermark_key", ctypes.c_uint32), ("watermark_depth_db", ctypes.c_float)]


STTS_FLAG_WATERMARK_PAYLOAD = 512     # include/vits_watermark_payload.h


class SttsWatermarkPayloadOpts(SttsWatermarkOpts):
    """mirror of `struct stts_synth_opts_watermark_payload` (include/vits_watermark_payload.h): SttsWatermarkOpts followed by the payload
    and the per-item payloads, which the library reads only under STTS_FLAG_WATERMARK_PAYLOAD"""

    _fields_ = [("watermark_payload", ctypes.c_uint32), ("watermark_payloads", ctypes.POINTER(ctypes.c_uint32))]


STTS_TAIL = TailFamily("STTS", (SttsOpts, SttsLoudnessOpts, SttsPitchOpts, SttsLimitOpts, SttsContourOpts, SttsIntonationOpts, SttsWatermarkOpts,
                                SttsWatermarkPayloadOpts),
                       loudness=STTS_FLAG_LOUDNESS, limit=STTS_FLAG_LIMIT, pitch=STTS_FLAG_PITCH, formant=STTS_FLAG_PITCH_FORMANT,
                       contour=STTS_FLAG_CONTOUR, intonation=STTS_FLAG_INTONATION, watermark=STTS_FLAG_WATERMARK,
                       watermark_payload=STTS_FLAG_WATERMARK_PAYLOAD)


class SttsModel:
    """Owns one stts_model* ; `vocoder` is a capi.VitsModel created from a vocoder-only blob (kept alive here)."""

    def __init__(self, vlib: VitsLib, blob, vocoder=None, device=0, prefix=None):
        self.vlib = vlib
        self.prefix = prefix or ("stts_" if vlib.prefix == "vits_" else "sttsref_")
        L = vlib.lib
        f = self._fn
        vp = ctypes.c_void_p
        f("create").argtypes = [vp, ctypes.c_size_t, vp, ctypes.c_int, ctypes.POINTER(vp)]
        f("destroy").argtypes = [vp]
        f("destroy").restype = None
        f("last_error").restype = ctypes.c_char_p
        f("get_hparams").argtypes = [vp, ctypes.POINTER(SttsHParams)]
        f("synthesize").argtypes = [vp, c_i64p, ctypes.c_int32, c_f32p, ctypes.c_int64, c_f32p, c_f32p, ctypes.POINTER(SttsOpts),
                                    ctypes.POINTER(c_f32p), c_i64p, ctypes.POINTER(c_f32p), c_i64p]
        f("synthesize_batch").argtypes = [vp, c_i64p, c_i64p, ctypes.c_int32, ctypes.c_int32, c_f32p, c_i64p, c_f32p, c_f32p,
                                          ctypes.POINTER(SttsOpts), ctypes.POINTER(c_f32p), c_i64p, c_i64p]
        if hasattr(L, self.prefix + "stream_open"):
            f("stream_open").argtypes = [vp, c_i64p, ctypes.c_int32, c_f32p, ctypes.c_int64, c_f32p, c_f32p, ctypes.POINTER(SttsOpts),
                                         ctypes.c_int32, ctypes.POINTER(vp), c_i64p]
        # include/vits_marks.h: speech marks, declared where the symbols exist (the CPU oracle has none)
        self.has_marks = hasattr(L, self.prefix + "synthesize_marks")
        if self.has_marks:
            f("synthesize_marks").argtypes = [vp, c_i64p, ctypes.c_int32, c_f32p, ctypes.c_int64, c_f32p, c_f32p, ctypes.POINTER(SttsOpts),
                                              ctypes.c_int32, ctypes.POINTER(c_f32p), c_i64p, ctypes.POINTER(c_f32p), c_i64p, c_i64p]
            f("synthesize_batch_marks").argtypes = [vp, c_i64p, c_i64p, ctypes.c_int32, ctypes.c_int32, c_f32p, c_i64p, c_f32p, c_f32p,
                                                    ctypes.POINTER(SttsOpts), ctypes.c_int32, ctypes.POINTER(c_f32p), c_i64p, c_i64p, c_i64p]
        # include/vits_document.h: the batch call joined into one piece of audio
        self.has_document = hasattr(L, self.prefix + "synthesize_document")
        if self.has_document:
            from .capi import Document

            f("synthesize_document").argtypes = [vp, c_i64p, c_i64p, ctypes.c_int32, ctypes.c_int32, c_f32p, c_i64p, c_f32p, c_f32p,
                                                 ctypes.POINTER(SttsOpts), ctypes.POINTER(Document), ctypes.c_int32, ctypes.POINTER(c_f32p),
                                                 c_i64p, c_i64p]
        f("stage_encoder").argtypes = [vp, c_i64p, c_i64p, ctypes.c_int32, ctypes.c_int32, c_i64p, c_f32p, c_f32p, c_f32p]
        f("stage_durations").argtypes = [vp, c_f32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_float, c_f32p, c_i32p, c_i64p]
        f("stage_estimator").argtypes = [vp, c_f32p, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int32, ctypes.c_float, c_f32p, c_f32p]
        f("stage_cfm").argtypes = [vp, c_f32p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, c_f32p, ctypes.c_float, ctypes.c_int32,
                                   c_f32p]
        self._vocoder = vocoder
        self._h = vp()
        buf = (ctypes.c_char * len(blob)).from_buffer_copy(blob)
        self.check(f("create")(ctypes.cast(buf, vp), len(blob), vocoder._h if vocoder is not None else None, device,
                               ctypes.byref(self._h)))
        self.hp = SttsHParams()
        self.check(f("get_hparams")(self._h, ctypes.byref(self.hp)))

    def _fn(self, name):
        return getattr(self.vlib.lib, self.prefix + name)

    def check(self, rc):
        if rc != 0:
            raise VitsError(rc, self._fn("last_error")().decode(errors="replace"))

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _denoise(self, opts, denoiser_strength, denoiser_filter_length):
        """STTS_FLAG_DENOISE and its two fields (include/vits_denoise.h); None = off.  Only the device library has the denoiser: the CPU
        oracle would ignore the flag, which is refused here instead"""
        if denoiser_strength is None:
            return
        self.vlib._need_denoise()
        opts.flags |= STTS_FLAG_DENOISE
        opts.denoiser_strength = float(denoiser_strength)
        opts.denoiser_filter_length = int(denoiser_filter_length or 0)

    def _opts_for(self, loudness, pitch, preserve_formants=False, limit=None, contour=None, pitch_range=None, watermark=None, B=1, keep=None,
                  out=None):
        """The options struct of a call, with the tail's flags and fields written (capi.TailFamily: the plain struct for a plain call, else
        the first of the chain that has every field asked for).  loudness, limit, watermark: their specs; pitch, pitch_range: as tail_of()
        takes them; contour: the arrays of contour_arrays().  B, keep, out: the result arrays of the loudness stage and the limiter
        (TailFamily.fill).  A stage the library does not export is refused: the CPU oracle would ignore the flag"""
        tail = tail_of(loudness, limit, pitch, preserve_formants, pitch_range, watermark)
        if contour is not None:
            self.vlib._need_contour()
        self.vlib._need_tail(tail, STTS_TAIL.word)
        opts = STTS_TAIL.opts(tail, contour=contour)
        STTS_TAIL.fill(opts, [] if keep is None else keep, tail, B, out)
        return opts

    def _need_marks(self):
        if not self.has_marks:
            raise VitsError(4, "this backend has no speech marks (include/vits_marks.h): the CPU oracle returns audio only")

    # ---- hot path ----------------------------------------------------------------------------
    def synthesize(self, ids, scales, sid, bert=None, phone_duration_extra=None, noise=None, seed=0, n_timesteps=0,
                   want_audio=True, want_mel=True, denoiser_strength=None, denoiser_filter_length=0, marks=False, sample_rate=None,
                   loudness=None, loudness_out=None, pitch=None, preserve_formants=False, limit=None, token_pitch=None, token_gain_db=None,
                   pitch_range=None, watermark=None, watermark_depth_db=None, watermark_payload=None):
        """watermark_payload: an int in [0, 65535] (STTS_FLAG_WATERMARK_PAYLOAD, include/vits_watermark_payload.h): the mark carries it;
        needs watermark=, and watermark_depth_db then defaults to 2.
        watermark: a 32-bit key (STTS_FLAG_WATERMARK, include/vits_watermark.h): the audio marked behind the resampler, in front of the
        loudness stage and the limiter; watermark_depth_db in (0, 2], default 1.
        pitch_range: r in [0, 4] (STTS_FLAG_INTONATION, include/vits_intonation.h): the utterance's movement about its own median pitch
        times r; 1 is the call as it was.
        token_pitch / token_gain_db: float [T] semitones / dB per token (STTS_FLAG_CONTOUR, include/vits_contour.h): every token raised
        or lowered by its own amount, in the pitch stage's place; `pitch` is added to every token.  Lengths and marks do not change.
        limit: a capi.limit_spec() (STTS_FLAG_LIMIT, include/vits_limit.h): the peak limiter with the loudness gain or alone;
        loudness_out then also receives "reduction".
        pitch: semitones in [-12, 12] (STTS_FLAG_PITCH, include/vits_pitch.h): the audio shifted behind the denoiser, before any
        resampling; its length and the marks do not change.  preserve_formants (STTS_FLAG_PITCH_FORMANT): the spectral envelope stays
        where it was; without a pitch in effect it changes nothing.
        One utterance.  ids int64 [5,T]; returns (audio float32 [S] or None, mel float32 [n_feats,T_y] or None).
        denoiser_strength (None = off) / denoiser_filter_length (0 = 1024): the vocoder-bias denoiser behind the clamp.
        marks=True (stts_synthesize_marks): a third value, token_ends int64 [T]; audio and marks are then at `sample_rate`
        (None / 0 = the voice's own).  loudness: a capi.loudness_spec() (STTS_FLAG_LOUDNESS): the audio normalised last in the chain
        (after the denoiser and, in the marks call, the resampler); loudness_out: a dict that receives "loudness" and "gain" [1]."""
        if marks:
            self._need_marks()
        elif sample_rate:
            raise ValueError("sample_rate is an argument of the marks call (SttsSession.resample serves the call without marks)")
        ids = _i64(ids)
        if ids.ndim != 2 or ids.shape[0] != 5:
            raise ValueError("ids must be [5, T]")
        T = ids.shape[1]
        scales = _f32(scales)
        keep = []
        con = None
        if want_audio and (token_pitch is not None or token_gain_db is not None):
            con = contour_arrays(1, T, None if token_pitch is None else _f32(token_pitch).reshape(1, -1),
                                 None if token_gain_db is None else _f32(token_gain_db).reshape(1, -1), None, pitch_spec(pitch))
        if want_audio:
            opts = self._opts_for(loudness, pitch, preserve_formants, limit, con, pitch_range,
                                  watermark_spec(watermark, watermark_depth_db, watermark_payload), 1, keep, loudness_out)
        else:  # (the mel alone: no stage of the tail applies)
            opts = self._opts_for(None, None)
        set_contour(opts, keep, con, STTS_TAIL.contour)
        if noise is not None:
            a = _f32(noise); keep.append(a)
            if a.ndim != 2 or a.shape[0] != self.hp.n_feats:
                raise ValueError("noise must be [n_feats, T]")
            opts.noise = _p(a, c_f32p)
            opts.noise_stride = a.shape[1]
        opts.seed = seed
        opts.n_timesteps = n_timesteps
        self._denoise(opts, denoiser_strength, denoiser_filter_length)
        b = None if bert is None else _f32(bert)
        if b is not None and b.shape != (self.hp.bert_dim, T):
            raise ValueError("bert must be [768, T]")
        p = None if phone_duration_extra is None else _f32(phone_duration_extra)
        if p is not None and p.shape != (T,):
            raise ValueError("phone_duration_extra must be [T]")
        au, mel = c_f32p(), c_f32p()
        ns, nf = ctypes.c_int64(), ctypes.c_int64()
        ends = np.zeros(T, np.int64) if marks else None
        tail = (ctypes.byref(au) if want_audio else None, ctypes.byref(ns) if want_audio else None,
                ctypes.byref(mel) if want_mel else None, ctypes.byref(nf) if want_mel else None)
        head = (self._h, _p(ids, c_i64p), T, _p(scales, c_f32p), int(sid), None if b is None else _p(b, c_f32p),
                None if p is None else _p(p, c_f32p), ctypes.byref(opts))
        if marks:
            self.check(self._fn("synthesize_marks")(*head, int(sample_rate or 0), *tail, _p(ends, c_i64p)))
        else:
            self.check(self._fn("synthesize")(*head, *tail))
        free = self.vlib._fn("free_output")
        audio = melo = None
        if want_audio:
            audio = np.ctypeslib.as_array(au, shape=(ns.value,)).copy(); free(au)
        if want_mel:
            melo = np.ctypeslib.as_array(mel, shape=(self.hp.n_feats, nf.value)).copy(); free(mel)
        return (audio, melo, ends) if marks else (audio, melo)

    def stream(self, ids, scales, sid, bert=None, phone_duration_extra=None, seed=0, n_timesteps=0, chunk_frames=64,
               denoiser_strength=None, denoiser_filter_length=0, on_marks=None, loudness=None, pitch=None, limit=None, watermark=None,
               watermark_payload=None):
        """pitch, limit, watermark, watermark_payload: refused, as loudness is.
        Streaming form of synthesize() (stts_stream_open): a generator of float32 chunks of chunk_frames*hop samples whose
        concatenation equals synthesize()'s audio for the same arguments.  on_marks: called once with token_ends int64 [T]
        (vits_stream_marks) as soon as the stream is open.  loudness: refused (stts_stream_open refuses STTS_FLAG_LOUDNESS the same
        way; here before any device work)."""
        tail_of(loudness, limit, pitch, watermark=watermark_spec(watermark, None, watermark_payload)).refuse_stream(STTS_TAIL.word, None, lambda msg: VitsError(4, msg))
        if on_marks is not None:
            self._need_marks()
        if self._vocoder is None:
            raise ValueError("no vocoder attached")
        ids = _i64(ids)
        if ids.ndim != 2 or ids.shape[0] != 5:
            raise ValueError("ids must be [5, T]")
        T = ids.shape[1]
        scales = _f32(scales)
        opts = SttsOpts(); opts.seed = seed; opts.n_timesteps = n_timesteps
        self._denoise(opts, denoiser_strength, denoiser_filter_length)
        b = None if bert is None else _f32(bert)
        if b is not None and b.shape != (self.hp.bert_dim, T):
            raise ValueError("bert must be [768, T]")
        p = None if phone_duration_extra is None else _f32(phone_duration_extra)
        if p is not None and p.shape != (T,):
            raise ValueError("phone_duration_extra must be [T]")
        st = ctypes.c_void_p()
        total = ctypes.c_int64()
        self.check(self._fn("stream_open")(self._h, _p(ids, c_i64p), T, _p(scales, c_f32p), int(sid), None if b is None else _p(b, c_f32p),
                                           None if p is None else _p(p, c_f32p), ctypes.byref(opts), int(chunk_frames),
                                           ctypes.byref(st), ctypes.byref(total)))
        if on_marks is not None:
            try:
                ends = self.vlib.stream_marks(st)
            except Exception:
                self.vlib._fn("stream_close")(st)
                raise
            on_marks(ends)
        return self._vocoder._drain(st, chunk_frames)

    def synthesize_batch(self, ids, lengths, scales, sid, bert=None, phone_duration_extra=None, seed=0, n_timesteps=0, item_seeds=None,
                         denoiser_strength=None, denoiser_filter_length=0, marks=False, sample_rate=None, loudness=None, loudness_out=None,
                         pitch=None, preserve_formants=False, limit=None, token_pitch=None, token_gain_db=None, pitch_range=None,
                         watermark=None, watermark_depth_db=None, watermark_payload=None):
        """watermark_payload: as for synthesize, or one value per item.
        token_pitch / token_gain_db: float [B, T], as for synthesize; pitch_range, watermark: as for synthesize, one value for the batch.
        pitch, preserve_formants, limit: as for synthesize, one value for the batch; every item is shifted from its own length.
        B independent utterances in one pass (stts_synthesize_batch): ids [B,5,T], lengths [B], sid [B];
        returns (audio float32 [B,S] zero-padded, out_lengths int64 [B] in samples).  Item b equals
        synthesize(ids[b][:, :lengths[b]], ..., seed=item_seeds[b]) (seed + b without item seeds).  marks=True
        (stts_synthesize_batch_marks): a third value, token_ends int64 [B,T]; everything is then at `sample_rate`."""
        if marks:
            self._need_marks()
        elif sample_rate:
            raise ValueError("sample_rate is an argument of the marks call (SttsSession.resample serves the call without marks)")
        B, T, head, keep = self._batch_head(ids, lengths, scales, sid, bert, phone_duration_extra, seed, n_timesteps, item_seeds, denoiser_strength,
                                            denoiser_filter_length, loudness, loudness_out, pitch, preserve_formants, limit, token_pitch,
                                            token_gain_db, pitch_range, watermark=watermark_spec(watermark, watermark_depth_db, watermark_payload))
        au = c_f32p(); ns = ctypes.c_int64(); ol = np.zeros(B, np.int64)
        ends = np.zeros((B, T), np.int64) if marks else None
        if marks:
            self.check(self._fn("synthesize_batch_marks")(*head, int(sample_rate or 0), ctypes.byref(au), ctypes.byref(ns), _p(ol, c_i64p),
                                                          _p(ends, c_i64p)))
        else:
            self.check(self._fn("synthesize_batch")(*head, ctypes.byref(au), ctypes.byref(ns), _p(ol, c_i64p)))
        audio = np.ctypeslib.as_array(au, shape=(B, ns.value)).copy()
        self.vlib._fn("free_output")(au)
        return (audio, ol, ends) if marks else (audio, ol)

    def _batch_head(self, ids, lengths, scales, sid, bert, phone_duration_extra, seed, n_timesteps, item_seeds, denoiser_strength,
                    denoiser_filter_length, loudness, loudness_out, pitch, preserve_formants, limit, token_pitch, token_gain_db, pitch_range,
                    results=None, watermark=None):
        """the leading arguments of the batch entry points -> (B, T, head, keep); results: how many result values the loudness / limiter
        outputs hold (default B; 1 for a document)"""
        ids = _i64(ids); lengths = _i64(lengths); sid = _i64(sid); scales = _f32(scales)
        B, five, T = ids.shape
        b = None if bert is None else _f32(bert)
        p = None if phone_duration_extra is None else _f32(phone_duration_extra)
        con = contour_arrays(B, T, token_pitch, token_gain_db, lengths, pitch_spec(pitch))
        keep = [ids, lengths, sid, scales, b, p]
        opts = self._opts_for(loudness, pitch, preserve_formants, limit, con, pitch_range, watermark, results or B, keep,
                              loudness_out)  # (per-item gains; loudness_out as for synthesize, [B])
        opts.seed = seed; opts.n_timesteps = n_timesteps
        self._denoise(opts, denoiser_strength, denoiser_filter_length)
        keep.append(opts)
        set_contour(opts, keep, con, STTS_TAIL.contour)
        if item_seeds is not None:
            sd = np.ascontiguousarray(item_seeds, dtype=np.uint64)
            if sd.shape != (B,):
                raise ValueError("item_seeds must be [B]")
            keep.append(sd)
            opts.item_seeds = sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
            opts.flags |= STTS_FLAG_ITEM_SEEDS  # (the trailing field is only read under this flag: include/stts_mi355.h)
        head = (self._h, _p(ids, c_i64p), _p(lengths, c_i64p), B, T, _p(scales, c_f32p), _p(sid, c_i64p),
                None if b is None else _p(b, c_f32p), None if p is None else _p(p, c_f32p), ctypes.byref(opts))
        return B, T, head, keep

    def synthesize_document(self, ids, lengths, scales, sid, bert=None, phone_duration_extra=None, seed=0, n_timesteps=0, item_seeds=None,
                            denoiser_strength=None, denoiser_filter_length=0, marks=False, sample_rate=None, loudness=None, loudness_out=None,
                            pitch=None, preserve_formants=False, limit=None, token_pitch=None, token_gain_db=None, pitch_range=None,
                            lead_frames=0, gap_frames=None, fade_samples=0, trim_db=None, trim_keep_frames=0, watermark=None,
                            watermark_depth_db=None, watermark_payload=None):
        """stts_synthesize_document (include/vits_document.h): the items of synthesize_batch joined into one piece of audio behind the
        pitch stage, in front of the resampler and the loudness / limiter stage, which see one item.  Returns (audio float32 [S], info):
        info["seg_start"] / ["seg_end"] int64 [B] in output samples, info["trim"] int32 [B, 2] frames, and with marks=True
        info["token_ends"] int64 [B, T].  The other keywords are those of synthesize_batch; loudness_out receives one value per key."""
        from .capi import document_struct

        if not self.has_document:
            raise VitsError(4, "this backend has no documents (include/vits_document.h)")
        if isinstance(watermark_payload, (list, tuple, np.ndarray)):
            raise ValueError("watermark_payload of a document: one value, it is marked as the one item it has become")
        B, T, head, keep = self._batch_head(ids, lengths, scales, sid, bert, phone_duration_extra, seed, n_timesteps, item_seeds, denoiser_strength,
                                            denoiser_filter_length, loudness, loudness_out, pitch, preserve_formants, limit, token_pitch,
                                            token_gain_db, pitch_range, results=1, watermark=watermark_spec(watermark, watermark_depth_db, watermark_payload))
        d, dkeep, info = document_struct(B, lead_frames, gap_frames, fade_samples, trim_db, trim_keep_frames)
        au = c_f32p(); ns = ctypes.c_int64()
        ends = np.zeros((B, T), np.int64) if marks else None
        self.check(self._fn("synthesize_document")(*head, ctypes.byref(d), int(sample_rate or 0), ctypes.byref(au), ctypes.byref(ns), _p(ends, c_i64p)))
        audio = np.ctypeslib.as_array(au, shape=(ns.value,)).copy() if ns.value else np.zeros(0, np.float32)
        self.vlib._fn("free_output")(au)
        if marks:
            info["token_ends"] = ends
        return audio, info

    # ---- stages --------------------------------------------------------------------------------
    def encoder(self, ids, lengths, sid, bert=None):
        ids = _i64(ids); lengths = _i64(lengths); sid = _i64(sid)
        B, five, T = ids.shape
        b = None if bert is None else _f32(bert)
        x = np.empty((B, self.hp.enc_hidden, T), np.float32); mu = np.empty((B, self.hp.dp_out, T), np.float32)
        self.check(self._fn("stage_encoder")(self._h, _p(ids, c_i64p), _p(lengths, c_i64p), B, T, _p(sid, c_i64p),
                                             None if b is None else _p(b, c_f32p), _p(x, c_f32p), _p(mu, c_f32p)))
        return x, mu

    def durations(self, mu_dp, length_scale, phone_duration_extra=None):
        mu_dp = _f32(mu_dp)
        B, K, T = mu_dp.shape
        p = None if phone_duration_extra is None else _f32(phone_duration_extra)
        d = np.empty((B, T), np.int32); yl = np.empty(B, np.int64)
        self.check(self._fn("stage_durations")(self._h, _p(mu_dp, c_f32p), B, T, float(length_scale),
                                               None if p is None else _p(p, c_f32p), _p(d, c_i32p), _p(yl, c_i64p)))
        return d, yl

    def estimator(self, x, mu, y_lengths, t, c):
        x = _f32(x); mu = _f32(mu); c = _f32(c); yl = _i64(y_lengths)
        B, NF, T = x.shape
        out = np.empty_like(x)
        self.check(self._fn("stage_estimator")(self._h, _p(x, c_f32p), _p(mu, c_f32p), _p(yl, c_i64p), B, T, float(t), _p(c, c_f32p),
                                               _p(out, c_f32p)))
        return out

    def cfm(self, mu_y, y_length, sid, noise, temperature, n_timesteps=0):
        mu_y = _f32(mu_y); noise = _f32(noise)
        T = mu_y.shape[1]
        out = np.empty((self.hp.n_feats, T), np.float32)
        self.check(self._fn("stage_cfm")(self._h, _p(mu_y, c_f32p), int(y_length), T, int(sid), _p(noise, c_f32p), float(temperature),
                                         int(n_timesteps), _p(out, c_f32p)))
        return out


class BertEncoder:
    """stts_bert_* : the word-embedding BERT encoder (`bert/model.onnx` of the reference, vosk_tts/model.py:61).
    `run(None, {"input_ids": [ids], "attention_mask": [...], "token_type_ids": [...]})[0]` -> float32 [T, hidden]
    mirrors the onnxruntime call at synth.py:27-34."""

    def __init__(self, vlib: VitsLib, blob, device=0, prefix=None):
        from .weights_bert import BertHParams

        self.vlib = vlib
        self.prefix = prefix or ("stts_bert_" if vlib.prefix == "vits_" else "sttsref_bert_")
        vp = ctypes.c_void_p
        f = self._fn
        f("create").argtypes = [vp, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(vp)]
        f("destroy").argtypes = [vp]
        f("destroy").restype = None
        f("get_hparams").argtypes = [vp, ctypes.POINTER(BertHParams)]
        f("encode").argtypes = [vp, c_i64p, c_i64p, ctypes.c_int32, c_f32p]
        # include/stts_bert_batch.h: padded batches, an extension of the product library (the CPU oracle encodes one sentence)
        self.has_batch = hasattr(vlib.lib, self.prefix + "encode_batch") and hasattr(vlib.lib, self.prefix + "feed_batch")
        if self.has_batch:
            f("encode_batch").argtypes = [vp, c_i64p, c_i64p, c_i32p, ctypes.c_int32, ctypes.c_int32, c_f32p]
            f("feed_batch").argtypes = [vp, c_i64p, c_i64p, c_i32p, ctypes.c_int32, ctypes.c_int32, c_i32p, ctypes.c_int32, c_f32p]
        self._err = getattr(vlib.lib, "stts_last_error" if vlib.prefix == "vits_" else "sttsref_last_error")
        self._err.restype = ctypes.c_char_p
        self._h = vp()
        buf = (ctypes.c_char * len(blob)).from_buffer_copy(blob)
        self._check(f("create")(ctypes.cast(buf, vp), len(blob), device, ctypes.byref(self._h)))
        self.hp = BertHParams()
        self._check(f("get_hparams")(self._h, ctypes.byref(self.hp)))

    def _fn(self, name):
        return getattr(self.vlib.lib, self.prefix + name)

    def _check(self, rc):
        if rc != 0:
            raise VitsError(rc, self._err().decode(errors="replace"))

    def encode(self, input_ids, token_type_ids=None):
        ids = _i64(input_ids).reshape(-1)
        ty = None if token_type_ids is None else _i64(token_type_ids).reshape(-1)
        out = np.empty((ids.shape[0], self.hp.hidden), np.float32)
        self._check(self._fn("encode")(self._h, _p(ids, c_i64p), None if ty is None else _p(ty, c_i64p), ids.shape[0], _p(out, c_f32p)))
        return out

    def _pad_ids(self, id_lists, token_type_ids):
        """-> ids int64 [B, T], types int64 [B, T] or None, lengths int32 [B] (padding entries are never read by the library)"""
        if not self.has_batch:
            raise NotImplementedError("this library has no batched BERT entry points (include/stts_bert_batch.h)")
        seqs = [_i64(a).reshape(-1) for a in id_lists]
        if not seqs:
            raise ValueError("empty batch")
        lens = np.array([a.shape[0] for a in seqs], np.int32)
        B, T = len(seqs), max(int(lens.max()), 1)
        ids = np.zeros((B, T), np.int64)
        for b, a in enumerate(seqs):
            ids[b, :lens[b]] = a
        ty = None
        if token_type_ids is not None:
            if len(token_type_ids) != B:
                raise ValueError("token_type_ids must hold one array per sentence")
            ty = np.zeros((B, T), np.int64)
            for b, a in enumerate(token_type_ids):
                a = _i64(a).reshape(-1)
                if a.shape[0] != lens[b]:
                    raise ValueError(f"token_type_ids[{b}] has {a.shape[0]} entries for {lens[b]} tokens")
                ty[b, :lens[b]] = a
        return ids, ty, lens

    def encode_batch(self, id_lists, token_type_ids=None):
        """stts_bert_encode_batch: B sentences of any lengths in ONE padded forward -> list of float32 [T_b, hidden], item b what
        encode(id_lists[b]) returns (to rounding: the batch takes other conv / attention tiles than a lone sentence)."""
        ids, ty, lens = self._pad_ids(id_lists, token_type_ids)
        out = self.encode_batch_padded(ids, ty, lens)
        return [out[b, :lens[b]].copy() for b in range(len(lens))]

    def encode_batch_padded(self, ids, token_type_ids, lengths):
        """the call itself on padded arrays: ids / token_type_ids [B, T] (types may be None), lengths [B] -> float32 [B, T, hidden],
        rows beyond lengths[b] zero"""
        ids = _i64(ids); lens = _i32(lengths)
        ty = None if token_type_ids is None else _i64(token_type_ids)
        if ids.ndim != 2 or lens.shape != (ids.shape[0],) or (ty is not None and ty.shape != ids.shape):
            raise ValueError("ids / token_type_ids must be [B, T], lengths [B]")
        B, T = ids.shape
        out = np.empty((B, T, self.hp.hidden), np.float32)
        self._check(self._fn("encode_batch")(self._h, _p(ids, c_i64p), _p(ty, c_i64p), _p(lens, c_i32p), B, T, _p(out, c_f32p)))
        return out

    def feed_batch(self, id_lists, row_lists, T_x=None, token_type_ids=None):
        """stts_bert_feed_batch: the same forward and, still on the device, the phoneme feed of the acoustic models:
        -> float32 [B, hidden, T_x] with out[b, :, t] = hidden state of token row_lists[b][t] of sentence b; a negative row and
        every column beyond len(row_lists[b]) is zero.  T_x defaults to the longest row list."""
        ids, ty, lens = self._pad_ids(id_lists, token_type_ids)
        if len(row_lists) != len(lens):
            raise ValueError("one row list per sentence")
        rl = [_i32(r).reshape(-1) for r in row_lists]
        longest = max(r.shape[0] for r in rl)
        T_x = max(longest, 1) if T_x is None else int(T_x)
        if T_x < longest:
            raise ValueError(f"T_x = {T_x} is shorter than the longest row list ({longest})")
        rows = np.full((len(rl), T_x), -1, np.int32)
        for b, r in enumerate(rl):
            rows[b, :r.shape[0]] = r
        return self.feed_batch_padded(ids, ty, lens, rows)

    def feed_batch_padded(self, ids, token_type_ids, lengths, rows):
        ids = _i64(ids); lens = _i32(lengths); rows = _i32(rows)
        ty = None if token_type_ids is None else _i64(token_type_ids)
        if ids.ndim != 2 or rows.ndim != 2 or rows.shape[0] != ids.shape[0] or lens.shape != (ids.shape[0],) or (ty is not None and ty.shape != ids.shape):
            raise ValueError("ids / token_type_ids must be [B, T], lengths [B], rows [B, T_x]")
        B, T = ids.shape
        out = np.empty((B, self.hp.hidden, rows.shape[1]), np.float32)
        self._check(self._fn("feed_batch")(self._h, _p(ids, c_i64p), _p(ty, c_i64p), _p(lens, c_i32p), B, T, _p(rows, c_i32p), rows.shape[1],
                                           _p(out, c_f32p)))
        return out

    def run(self, output_names, feed):
        mask = np.asarray(feed.get("attention_mask", [[1]]))
        if not np.all(mask == 1):
            raise NotImplementedError("padded BERT batches are not part of the path (synth.py:27-34 encodes one sentence)")
        ids = np.asarray(feed["input_ids"])
        if ids.ndim != 2 or ids.shape[0] != 1:
            raise ValueError("input_ids must be [1, T]")
        ty = feed.get("token_type_ids")
        return [self.encode(ids[0], None if ty is None else np.asarray(ty)[0])]

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
