"""ctypes binding of the C ABI declared in include/vits_mi355.h.

`VitsLib()` loads the product library (vosk_tts_amd/csrc/libvits_mi355.so, the
hand-written HIP kernels) and fails loudly when it is missing — there is no CPU
fallback in the product path.  The class takes an explicit (path, prefix) only
so that tests can drive the CPU oracle (oracle/libvits_oracle.so, prefix
"vitsref_") through the very same wrapper and compare results.
"""
import ctypes
import os

import numpy as np

from .outopts import PLAIN, Tail
from .weights import HParams

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "csrc", "libvits_mi355.so")

c_i64p = ctypes.POINTER(ctypes.c_int64)
c_i32p = ctypes.POINTER(ctypes.c_int32)
c_f32p = ctypes.POINTER(ctypes.c_float)


class SynthOpts(ctypes.Structure):
    """mirror of `struct vits_synth_opts`"""

    _fields_ = [
        ("noise_dp", c_f32p),
        ("noise_prior", c_f32p),
        ("noise_prior_stride", ctypes.c_int64),
        ("forced_durations", c_i32p),
        ("seed", ctypes.c_uint64),
        ("max_frames", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("item_seeds", ctypes.POINTER(ctypes.c_uint64)),
        ("bert", c_f32p),
        # include/vits_loudness.h: read only under VITS_FLAG_LOUDNESS
        ("loudness_mode", ctypes.c_int32),
        ("loudness_target", ctypes.c_float),
        ("loudness_ceiling", ctypes.c_float),
        ("out_loudness", c_f32p),
        ("out_gain", c_f32p),
    ]


# include/vits_loudness.h
FLAG_LOUDNESS = 2       # VITS_FLAG_LOUDNESS
LOUDNESS_LUFS = 1       # VITS_LOUDNESS_LUFS
LOUDNESS_PEAK = 2       # VITS_LOUDNESS_PEAK
LOUDNESS_MIN_RATE = 4000
# include/vits_limit.h
LIMIT_SAMPLE = 1        # VITS_LIMIT_SAMPLE
LIMIT_TRUE = 2          # VITS_LIMIT_TRUE
LIMIT_TILE = 2048
LIMIT_MAX_LOOKAHEAD = 1024


def loudness_spec(loudness=None, peak=None, peak_ceiling=None):
    """The normalisation a call asks for -> None (none) or (mode, target, ceiling) as vits_synth_opts carries it.  loudness: a LUFS
    target (BS.1770 integrated loudness) with peak_ceiling as the cap on the resulting peak (default 1.0: an int16 result never clips
    harder than it did; 0 = no cap); peak: a max-|sample| target.  Both at once is a ValueError, as is a value out of range (the
    library refuses the same values, VITS_ERR_ARG: here they are refused before any device work)."""
    if loudness is not None and peak is not None:
        raise ValueError(f"loudness={loudness} and peak={peak}: a request is normalised to a LUFS target or to a peak target, not both")
    if loudness is not None:
        t, c = float(loudness), 1.0 if peak_ceiling is None else float(peak_ceiling)
        if not -70.0 <= t <= 0.0:
            raise ValueError(f"loudness target {t} LUFS outside [-70, 0]")
        if not 0.0 <= c < float("inf"):
            raise ValueError(f"peak_ceiling {c} must be >= 0 (0 = none)")
        return (LOUDNESS_LUFS, t, c)
    if peak is not None:
        t = float(peak)
        if not 0.0 < t <= 1.0:
            raise ValueError(f"peak target {t} outside (0, 1]")
        return (LOUDNESS_PEAK, t, 0.0)
    return None


# include/vits_pitch.h
FLAG_PITCH = 4          # VITS_FLAG_PITCH
FLAG_PITCH_FORMANT = 8  # VITS_FLAG_PITCH_FORMANT: keep the spectral envelope where it was; modifies a pitch request
PITCH_FRAME = 1024      # VITS_PITCH_FRAME
PITCH_MAX_SEMITONES = 12.0


class SynthPitchOpts(SynthOpts):
    """mirror of `struct vits_synth_opts_pitch` (include/vits_pitch.h): SynthOpts followed by pitch_semitones, which the library reads
    only under VITS_FLAG_PITCH; passed where a POINTER(SynthOpts) is declared"""

    _fields_ = [("pitch_semitones", ctypes.c_float)]


def pitch_ratio(semitones):
    """(P, Q) of a shift as include/vits_pitch.h defines it; ValueError names a value out of range (NaN included), as the library's
    VITS_ERR_ARG does: here it is refused before any device work"""
    import math
    s = float(semitones)
    if not abs(s) <= PITCH_MAX_SEMITONES:
        raise ValueError(f"pitch {s} semitones outside [-{PITCH_MAX_SEMITONES:g}, {PITCH_MAX_SEMITONES:g}]")
    p0 = int(math.floor(1000.0 * 2.0 ** (s / 12.0) + 0.5))
    g = math.gcd(p0, 1000)
    return p0 // g, 1000 // g


def pitch_spec(pitch=None):
    """The shift a call asks for -> None (none, or one that reduces to P = Q) or the semitones as a float"""
    if pitch is None:
        return None
    P, Q = pitch_ratio(pitch)
    return None if P == Q else float(pitch)


# include/vits_limit.h
FLAG_LIMIT = 16         # VITS_FLAG_LIMIT
LIMIT_MODES = {"sample": LIMIT_SAMPLE, "true": LIMIT_TRUE}
LIMIT_FIELDS = [("limit_mode", ctypes.c_int32), ("limit_ceiling", ctypes.c_float), ("limit_lookahead_ms", ctypes.c_float),
                ("limit_release_ms", ctypes.c_float), ("limit_gain", ctypes.c_float), ("out_reduction", c_f32p)]


class SynthLimitOpts(SynthPitchOpts):
    """mirror of `struct vits_synth_opts_limit` (include/vits_limit.h): SynthPitchOpts followed by the six limiter fields, which the
    library reads only under VITS_FLAG_LIMIT (the loudness and pitch fields inside still only under their own flags)"""

    _fields_ = LIMIT_FIELDS


def limit_spec(limit=None, ceiling=None, lookahead_ms=5.0, release_ms=50.0, gain=1.0):
    """The limiter a call asks for -> None (none) or (mode, ceiling, lookahead_ms, release_ms, gain) as vits_synth_opts_limit carries it.
    limit: None, "sample" (sample peaks) or "true" (4x oversampled peaks); ceiling in (0, 1] (default 1.0); gain: the pre-gain of a call
    without a loudness target.  A value out of range is a ValueError naming it (the library refuses the same values, VITS_ERR_ARG: here
    they are refused before any device work)."""
    if limit is None:
        return None
    if limit not in LIMIT_MODES:
        raise ValueError(f"limit={limit!r}: None, 'sample' or 'true'")
    c, la, rel, g = 1.0 if ceiling is None else float(ceiling), float(lookahead_ms), float(release_ms), float(gain)
    if not 0.0 < c <= 1.0:
        raise ValueError(f"limiter ceiling {c} outside (0, 1]")
    if not 0.0 < la <= 10.0:
        raise ValueError(f"limit_lookahead_ms {la} outside (0, 10]")
    if not 1.0 <= rel <= 1000.0:
        raise ValueError(f"limit_release_ms {rel} outside [1, 1000]")
    if not 0.0 <= g <= 64.0:
        raise ValueError(f"limiter gain {g} outside [0, 64]")
    return (LIMIT_MODES[limit], c, la, rel, g)


# include/vits_prosody.h
FLAG_PROSODY = 32                # VITS_FLAG_PROSODY
PROSODY_MAX_TOKEN_SCALE = 16.0   # VITS_PROSODY_MAX_TOKEN_SCALE
PROSODY_FIT_RATIO = (0.25, 4.0)  # VITS_PROSODY_MIN_FIT_RATIO, VITS_PROSODY_MAX_FIT_RATIO


class Prosody(ctypes.Structure):
    """mirror of `struct vits_prosody` (include/vits_prosody.h)"""

    _fields_ = [("item_scales", c_f32p), ("token_length_scale", c_f32p), ("token_pause", c_i32p), ("fit_frames", c_i32p),
                ("out_fit_ratio", c_f32p)]


class SynthProsodyOpts(SynthLimitOpts):
    """mirror of `struct vits_synth_opts_prosody` (include/vits_prosody.h): SynthLimitOpts followed by the pointer to the controls, which
    the library reads only under VITS_FLAG_PROSODY (the loudness, pitch and limiter fields inside still only under their own flags)"""

    _fields_ = [("prosody", ctypes.POINTER(Prosody))]


def prosody_arrays(B, Tx, item_scales=None, token_length_scale=None, token_pause=None, fit_frames=None):
    """The controls a call asks for -> None (none) or a dict of contiguous arrays of the shapes include/vits_prosody.h states.  Only the
    shapes are checked here (ValueError): the values are the library's to refuse, by name (VITS_ERR_ARG)."""
    if item_scales is None and token_length_scale is None and token_pause is None and fit_frames is None:
        return None
    out = {}
    for name, a, conv, shape in (("item_scales", item_scales, _f32, (B, 3)), ("token_length_scale", token_length_scale, _f32, (B, Tx)),
                                 ("token_pause", token_pause, _i32, (B, Tx)), ("fit_frames", fit_frames, _i32, (B,))):
        if a is None:
            continue
        a = conv(a)
        if a.shape != shape:
            raise ValueError(f"{name} must be {list(shape)} (got {list(a.shape)})")
        out[name] = a
    return out


def prosody_struct(arrays):
    """a Prosody whose input pointers name the arrays of prosody_arrays() (which the caller keeps alive); absent ones are NULL"""
    P = Prosody()
    for name, typ in (("item_scales", c_f32p), ("token_length_scale", c_f32p), ("token_pause", c_i32p), ("fit_frames", c_i32p)):
        setattr(P, name, _p(arrays.get(name), typ))
    return P


def set_prosody(opts, keep, arrays, B, flag, out=None):
    """Points a SynthProsodyOpts at the controls of prosody_arrays() and sets the family's flag; the struct, the arrays and the [B] result
    array are kept alive in `keep` and, when `out` is a dict, the result is published there as out["fit_ratio"]."""
    if arrays is None:
        return
    P = prosody_struct(arrays)
    ratio = np.full(B, np.nan, np.float32)
    keep += [P, ratio] + list(arrays.values())
    P.out_fit_ratio = _p(ratio, c_f32p)
    opts.prosody = ctypes.pointer(P)
    opts.flags |= flag
    if out is not None:
        out["fit_ratio"] = ratio


# include/vits_contour.h
FLAG_CONTOUR = 64                # VITS_FLAG_CONTOUR (STTS_FLAG_CONTOUR has the same value)
CONTOUR_DB = (-40.0, 12.0)       # VITS_CONTOUR_MIN_DB, VITS_CONTOUR_MAX_DB
CONTOUR_RAMP = 4                 # VITS_CONTOUR_RAMP


class Contour(ctypes.Structure):
    """mirror of `struct vits_contour` (include/vits_contour.h)"""

    _fields_ = [("token_semitones", c_f32p), ("token_gain_db", c_f32p)]


class SynthContourOpts(SynthProsodyOpts):
    """mirror of `struct vits_synth_opts_contour` (include/vits_contour.h): SynthProsodyOpts followed by the pointer to the contour, which
    the library reads only under VITS_FLAG_CONTOUR"""

    _fields_ = [("contour", ctypes.POINTER(Contour))]


def contour_arrays(B, Tx, token_pitch=None, token_gain_db=None, lengths=None, pitch=None):
    """The contour a call asks for -> None (none, or one whose every token is neutral) or a dict of contiguous float32 [B, T_x] arrays.
    Values out of range (NaN included) are a ValueError naming item, token and value, as the library's VITS_ERR_ARG does: here they are
    refused before any device work.  lengths: the items' token counts (values beyond them are not looked at); pitch: the call's own
    shift, which the library adds to every token."""
    if token_pitch is None and token_gain_db is None:
        return None
    out = {}
    live = np.ones((B, Tx), bool) if lengths is None else np.arange(Tx)[None, :] < np.asarray(lengths).reshape(B, 1)
    add = 0.0 if pitch is None else float(pitch)
    for name, a, lo, hi, unit, off in (("token_semitones", token_pitch, -PITCH_MAX_SEMITONES, PITCH_MAX_SEMITONES, "semitones", add),
                                       ("token_gain_db", token_gain_db, CONTOUR_DB[0], CONTOUR_DB[1], "dB", 0.0)):
        if a is None:
            continue
        a = _f32(a)
        if a.shape != (B, Tx):
            raise ValueError(f"{name} must be {[B, Tx]} (got {list(a.shape)})")
        v = a.astype(np.float64) + off
        bad = live & ~((v >= lo) & (v <= hi))
        if bad.any():
            b, t = (int(i) for i in np.argwhere(bad)[0])
            raise ValueError(f"contour: {v[b, t]:g} {unit} at item {b}, token {t} outside [{lo:g}, {hi:g}]")
        out[name] = a
    if all(not np.any(a[live]) for a in out.values()):
        return None
    return out


def set_contour(opts, keep, arrays, flag):
    """Points a SynthContourOpts / SttsContourOpts at the arrays of contour_arrays() and sets the flag; everything is kept alive in `keep`"""
    if arrays is None:
        return
    C = Contour()
    C.token_semitones = _p(arrays.get("token_semitones"), c_f32p)
    C.token_gain_db = _p(arrays.get("token_gain_db"), c_f32p)
    keep += [C] + list(arrays.values())
    opts.contour = ctypes.pointer(C)
    opts.flags |= flag


# include/vits_intonation.h
FLAG_INTONATION = 128            # VITS_FLAG_INTONATION (STTS_FLAG_INTONATION has the same value)
INTONATION_MAX_RANGE = 4.0       # VITS_INTONATION_MAX_RANGE
INTONATION_RATES = (8000, 32000)  # VITS_INTONATION_MIN_RATE, VITS_INTONATION_MAX_RATE


class SynthIntonationOpts(SynthContourOpts):
    """mirror of `struct vits_synth_opts_intonation` (include/vits_intonation.h): SynthContourOpts followed by pitch_range, which the
    library reads only under VITS_FLAG_INTONATION"""

    _fields_ = [("pitch_range", ctypes.c_float)]


def range_spec(pitch_range=None):
    """The intonation range a call asks for -> None (none, or one whose r_m = lround(1000 r) is 1000: the call as it was) or r as a
    float.  ValueError names a value out of range (NaN included), as the library's VITS_ERR_ARG does: here before any device work"""
    if pitch_range is None:
        return None
    import math
    r = float(np.float32(pitch_range))  # (the value the library is handed)
    if not 0.0 <= r <= INTONATION_MAX_RANGE:
        raise ValueError(f"pitch_range {float(pitch_range)} outside [0, {INTONATION_MAX_RANGE:g}]")
    return None if int(math.floor(1000.0 * r + 0.5)) == 1000 else r


# include/vits_watermark.h
FLAG_WATERMARK = 256             # VITS_FLAG_WATERMARK (STTS_FLAG_WATERMARK has the same value)
WATERMARK_MAX_DEPTH_DB = 2.0     # VITS_WATERMARK_MAX_DEPTH_DB
WATERMARK_THRESHOLD = 6.0        # VITS_WATERMARK_THRESHOLD
WATERMARK_OFFSETS = 128          # VITS_WATERMARK_OFFSETS
WATERMARK_FIELDS = [("watermark_key", ctypes.c_uint32), ("watermark_depth_db", ctypes.c_float)]


class SynthWatermarkOpts(SynthIntonationOpts):
    """mirror of `struct vits_synth_opts_watermark` (include/vits_watermark.h): SynthIntonationOpts followed by the key and the depth,
    which the library reads only under VITS_FLAG_WATERMARK"""

    _fields_ = WATERMARK_FIELDS


# include/vits_watermark_payload.h
FLAG_WATERMARK_PAYLOAD = 512     # VITS_FLAG_WATERMARK_PAYLOAD (STTS_FLAG_WATERMARK_PAYLOAD has the same value)
WATERMARK_PAYLOAD_MAX = 65535    # VITS_WATERMARK_PAYLOAD_MAX
WATERMARK_CODED_BITS = 24        # VITS_WATERMARK_CODED_BITS
WATERMARK_PAYLOAD_FIELDS = [("watermark_payload", ctypes.c_uint32), ("watermark_payloads", ctypes.POINTER(ctypes.c_uint32))]
PAYLOAD_RIDES = "rides"  # in a session's Tail, in the payload's place: the value rides with the request (it does not decide the batch)


class SynthWatermarkPayloadOpts(SynthWatermarkOpts):
    """mirror of `struct vits_synth_opts_watermark_payload` (include/vits_watermark_payload.h): SynthWatermarkOpts followed by the
    payload and the per-item payloads, which the library reads only under VITS_FLAG_WATERMARK_PAYLOAD"""

    _fields_ = WATERMARK_PAYLOAD_FIELDS


# include/vits_watermark_scan.h
WATERMARK_SCAN_MAX_SPAN = 8        # VITS_WATERMARK_SCAN_MAX_SPAN
WATERMARK_SCAN_DEFAULT_SPAN = 4    # VITS_WATERMARK_SCAN_DEFAULT_SPAN
WATERMARK_SCAN_PILOTS = 1          # VITS_WATERMARK_SCAN_PILOTS
WATERMARK_PERIOD_SAMPLES = 16384   # VITS_WATERMARK_PERIOD_SAMPLES


def payload_spec(payload):
    """watermark_payload= -> None, an int, or a tuple of ints (one per item of a batch); a value outside [0, 65535] is a ValueError
    naming it, as the library's VITS_ERR_ARG does: here before any device work"""
    if payload is None:
        return None

    def one(v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= WATERMARK_PAYLOAD_MAX:
            raise ValueError(f"watermark_payload {v!r} outside [0, {WATERMARK_PAYLOAD_MAX}]")
        return int(v)

    if isinstance(payload, (list, tuple, np.ndarray)):
        return tuple(one(v) for v in np.asarray(payload).reshape(-1).tolist()) if isinstance(payload, np.ndarray) else tuple(one(v) for v in payload)
    return one(payload)


def watermark_spec(watermark=None, depth_db=None, payload=None):
    """The mark a call asks for -> None (none) or (key, depth_db) as vits_synth_opts_watermark carries it (depth 0 = the default,
    1 dB), or (key, depth_db, payload) with a payload_spec() (include/vits_watermark_payload.h; depth 0 is then 2 dB).  watermark: the
    32-bit key (a selector, not a secret).  ValueError names a key outside [0, 2^32), a depth outside (0, 2] dB (NaN included) or a
    payload outside [0, 65535], as the library's VITS_ERR_ARG does, and a payload without a key: here before any device work."""
    if watermark is None or watermark is False:
        if payload is not None:
            raise ValueError("watermark_payload needs watermark=: VITS_FLAG_WATERMARK_PAYLOAD modifies a watermark request")
        return None
    if isinstance(watermark, bool) or not isinstance(watermark, (int, np.integer)):
        raise ValueError(f"watermark={watermark!r}: a key is an integer in [0, 2^32)")
    key = int(watermark)
    if not 0 <= key < 1 << 32:
        raise ValueError(f"watermark key {key} outside [0, 2^32)")
    d = 0.0 if depth_db is None else float(depth_db)
    if depth_db is not None and not 0.0 < d <= WATERMARK_MAX_DEPTH_DB:
        raise ValueError(f"watermark_depth_db {d} outside (0, {WATERMARK_MAX_DEPTH_DB:g}]")
    if payload is not None:
        return (key, d, payload if payload is PAYLOAD_RIDES else payload_spec(payload))
    return (key, d)


def tail_payload(tail):
    """the payload of a Tail's mark: None, an int, a tuple of ints, or PAYLOAD_RIDES"""
    return tail.watermark[2] if tail.watermark is not None and len(tail.watermark) > 2 else None


def tail_of(loudness=None, limit=None, pitch=None, preserve_formants=False, pitch_range=None, watermark=None):
    """The Tail of a model's call: loudness, limit and watermark as their specs, pitch and pitch_range as the caller gave them (a shift
    that reduces to P = Q and a range whose r_m is 1000 are none; preserve_formants counts only with a shift in effect)"""
    if loudness is None and limit is None and pitch is None and pitch_range is None and watermark is None:
        return PLAIN
    pitch = pitch_spec(pitch)
    return Tail(loudness, limit, pitch, pitch is not None and bool(preserve_formants), range_spec(pitch_range), watermark)


class TailFamily:
    """What differs between the two APIs in how a call's options carry the tail; the Python twin of TailFamily in csrc/out_tail.hip.h.
    flags: the flag bit of every stage; chain: the options structs in the order each extends the one before."""

    FIELDS = ("loudness_mode", "pitch_semitones", "limit_mode", "prosody", "contour", "pitch_range", "watermark_key",
              "watermark_payload")  # one per stage, in opts()'s order

    def __init__(self, word, chain, loudness, limit, pitch, formant, contour, intonation, watermark, prosody=0, watermark_payload=FLAG_WATERMARK_PAYLOAD):
        self.word, self.chain, self.watermark_payload = word, chain, watermark_payload
        self.loudness, self.limit, self.pitch, self.formant = loudness, limit, pitch, formant
        self.contour, self.intonation, self.watermark, self.prosody = contour, intonation, watermark, prosody

    def opts(self, tail, prosody=None, contour=None):
        """the options struct of a call: the first of the chain that has every field asked for (a plain call: the plain struct)"""
        if tail is PLAIN and prosody is None and contour is None:  # (the hot path: not worth a search)
            return self.chain[0]()
        asked = (tail.loudness, tail.pitch, tail.limit, prosody, contour, tail.pitch_range, tail.watermark, tail_payload(tail))
        need = [f for f, v in zip(self.FIELDS, asked) if v is not None]
        return next(c for c in self.chain if all(hasattr(c, f) for f in need))()

    def fill(self, opts, keep, tail, B, out=None):
        """Writes the flags and fields of `tail` into an opts() struct.  The [B] result arrays of the loudness stage and the limiter are
        kept alive in `keep` and, when `out` is a dict, published there: out["loudness"] (LUFS of the un-normalised item, -inf for
        silence), out["gain"], out["reduction"] (min of the limiter's gain curve per item, 1 = not limited)."""
        if tail.loudness is not None:
            opts.flags |= self.loudness
            opts.loudness_mode, opts.loudness_target, opts.loudness_ceiling = tail.loudness
            results = ("loudness", "out_loudness"), ("gain", "out_gain")
        else:
            results = ()
        if tail.limit is not None:
            opts.flags |= self.limit
            opts.limit_mode, opts.limit_ceiling, opts.limit_lookahead_ms, opts.limit_release_ms, opts.limit_gain = tail.limit
            results += (("reduction", "out_reduction"),)
        for name, field in results:
            a = np.full(B, np.nan, np.float32)
            keep.append(a)
            setattr(opts, field, _p(a, c_f32p))
            if out is not None:
                out[name] = a
        if tail.pitch is not None:
            opts.flags |= self.pitch | (self.formant if tail.formants else 0)
            opts.pitch_semitones = tail.pitch
        if tail.pitch_range is not None:
            opts.flags |= self.intonation
            opts.pitch_range = tail.pitch_range
        if tail.watermark is not None:
            opts.flags |= self.watermark
            opts.watermark_key, opts.watermark_depth_db = tail.watermark[:2]
            payload = tail_payload(tail)
            if payload is PAYLOAD_RIDES:
                raise ValueError("a session's Tail reached the options struct with its payload still riding with the request")
            if isinstance(payload, tuple):  # one per item; it overrides the scalar
                if len(payload) != B:
                    raise ValueError(f"watermark_payload: {len(payload)} values for a batch of {B}")
                a = np.array(payload, np.uint32)
                keep.append(a)
                opts.flags |= self.watermark_payload
                opts.watermark_payloads = a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
            elif payload is not None:
                opts.flags |= self.watermark_payload
                opts.watermark_payload = payload


VITS_TAIL = TailFamily("VITS", (SynthOpts, SynthPitchOpts, SynthLimitOpts, SynthProsodyOpts, SynthContourOpts, SynthIntonationOpts, SynthWatermarkOpts,
                                SynthWatermarkPayloadOpts),
                       loudness=FLAG_LOUDNESS, limit=FLAG_LIMIT, pitch=FLAG_PITCH, formant=FLAG_PITCH_FORMANT, contour=FLAG_CONTOUR,
                       intonation=FLAG_INTONATION, watermark=FLAG_WATERMARK, prosody=FLAG_PROSODY)


class PersistInfo(ctypes.Structure):
    """mirror of `struct vits_persist_info` (vits_persist_state)"""

    _fields_ = [(n, ctypes.c_int32) for n in ("configured_mask", "active_mask", "off_for_ms", "timeouts", "rearms", "launches",
                                               "process_owns_device", "reserved")]


class VitsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"vits error {code}: {msg}")
        self.code = code


class Document(ctypes.Structure):
    """mirror of `struct vits_document` (include/vits_document.h)"""

    _fields_ = [
        ("lead_frames", ctypes.c_int32),
        ("gap_frames", c_i32p),
        ("fade_samples", ctypes.c_int32),
        ("trim_db", ctypes.c_float),
        ("trim_keep_frames", ctypes.c_int32),
        ("out_seg_start", c_i64p),
        ("out_seg_end", c_i64p),
        ("out_trim", c_i32p),
    ]


def document_struct(B, lead_frames=0, gap_frames=None, fade_samples=0, trim_db=None, trim_keep_frames=0, outputs=True):
    """-> (Document, keep, out): the controls of include/vits_document.h for B segments.  gap_frames: None, one int for every segment or
    [B]; trim_db None / 0 = off.  out (with outputs): the arrays the call fills, "seg_start" / "seg_end" int64 [B], "trim" int32 [B, 2].
    Values are passed as they are: the library refuses what the header refuses."""
    d = Document()
    keep, out = [], {}
    d.lead_frames = int(lead_frames)
    if gap_frames is not None:
        g = _i32(np.broadcast_to(np.asarray(gap_frames), (B,)) if np.ndim(gap_frames) == 0 else gap_frames)
        if g.shape != (B,):
            raise ValueError(f"gap_frames must be one value or [B = {B}] (got {g.shape})")
        keep.append(g)
        d.gap_frames = _p(g, c_i32p)
    d.fade_samples = int(fade_samples)
    d.trim_db = 0.0 if trim_db is None else float(trim_db)
    d.trim_keep_frames = int(trim_keep_frames)
    if outputs:
        out = {"seg_start": np.zeros(B, np.int64), "seg_end": np.zeros(B, np.int64), "trim": np.zeros((B, 2), np.int32)}
        d.out_seg_start = _p(out["seg_start"], c_i64p)
        d.out_seg_end = _p(out["seg_end"], c_i64p)
        d.out_trim = _p(out["trim"], c_i32p)
    return d, keep, out


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p(a, typ):
    return a.ctypes.data_as(typ) if a is not None else None


EXPORTED = [
    "create", "destroy", "last_error", "get_hparams", "is_device_backend", "synthesize", "free_output",
    "stage_text_encoder", "stage_duration", "stage_regulate", "stage_flow", "stage_decoder", "op_conv1d",
    "algorithmic_flops",
]
DEVICE_ONLY = ["session_create", "session_destroy", "session_synthesize_device", "session_last_ms"]


class VitsLib:
    def __init__(self, path=None, prefix="vits_"):
        path = path or os.environ.get("VITS_MI355_LIB", DEFAULT_LIB)
        if not os.path.exists(path):
            raise ImportError(
                f"{path} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback in the product path."
            )
        self.path = path
        self.prefix = prefix
        self.lib = ctypes.CDLL(path)
        L = self.lib
        f = self._fn
        f("create").argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        f("destroy").argtypes = [ctypes.c_void_p]
        f("destroy").restype = None
        f("last_error").restype = ctypes.c_char_p
        f("get_hparams").argtypes = [ctypes.c_void_p, ctypes.POINTER(HParams)]
        f("synthesize").argtypes = [ctypes.c_void_p, c_i64p, c_i64p, ctypes.c_int32, ctypes.c_int32, c_f32p, c_i64p,
                                    ctypes.POINTER(SynthOpts), ctypes.POINTER(c_f32p), c_i64p, c_i64p]
        f("free_output").argtypes = [c_f32p]
        f("free_output").restype = None
        f("stage_text_encoder").argtypes = [ctypes.c_void_p, c_i64p, c_i64p, ctypes.c_int32, ctypes.c_int32, c_i64p,
                                            c_f32p, c_f32p, c_f32p]
        f("stage_duration").argtypes = [ctypes.c_void_p, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int32, c_i64p, c_f32p,
                                        ctypes.c_float, c_f32p]
        f("stage_regulate").argtypes = [ctypes.c_void_p, c_f32p, c_i32p, c_i64p, ctypes.c_int32, ctypes.c_int32,
                                        ctypes.c_float, c_f32p, c_f32p, c_f32p, ctypes.c_float, ctypes.c_int32, c_i32p,
                                        c_i64p, c_f32p]
        f("stage_flow").argtypes = [ctypes.c_void_p, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int32, c_i64p, c_f32p]
        f("stage_decoder").argtypes = [ctypes.c_void_p, c_f32p, ctypes.c_int32, ctypes.c_int32, c_i64p, c_f32p, c_f32p]
        f("op_conv1d").argtypes = [ctypes.c_int, c_f32p, c_f32p, c_f32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                   ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_float, c_f32p]
        f("algorithmic_flops").argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
        f("algorithmic_flops").restype = ctypes.c_double
        f("mas_maximum_path").argtypes = [ctypes.c_int, c_f32p, c_i32p, c_i32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                          c_i32p]
        self.is_device = bool(f("is_device_backend")())
        self.has_resample = False
        self.has_denoise = False
        self.has_marks = False
        self.has_loudness = False
        self.has_pitch = False
        self.has_pitch_formant = False
        self.has_limit = False
        self.has_prosody = False
        self.has_contour = False
        self.has_document = False
        self.has_intonation = False
        self.has_watermark = False
        self.has_watermark_payload = False
        self.has_watermark_scan = False
        if self.is_device:
            c_i16p = ctypes.POINTER(ctypes.c_int16)
            f("synthesize_pcm16").argtypes = [ctypes.c_void_p, c_i64p, c_i64p, ctypes.c_int32, ctypes.c_int32, c_f32p, c_i64p,
                                              ctypes.POINTER(SynthOpts), ctypes.c_float, ctypes.POINTER(c_i16p), c_i64p, c_i64p]
            f("free_pcm16").argtypes = [c_i16p]
            f("free_pcm16").restype = None
            f("session_set_sdp_always").argtypes = [ctypes.c_void_p, ctypes.c_int]
            f("session_create").argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                            ctypes.POINTER(ctypes.c_void_p)]
            f("session_destroy").argtypes = [ctypes.c_void_p]
            f("session_destroy").restype = None
            f("session_synthesize_device").argtypes = [
                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, c_f32p,
                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64,
                ctypes.c_void_p]
            f("session_last_ms").argtypes = [ctypes.c_void_p, c_f32p]
            f("debug_decoder_needs").argtypes = [ctypes.POINTER(HParams), c_i32p, ctypes.c_int32]
            f("stream_open").argtypes = [ctypes.c_void_p, c_i64p, ctypes.c_int32, c_f32p, ctypes.c_int64,
                                         ctypes.POINTER(SynthOpts), ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p), c_i64p]
            f("stream_open_latent").argtypes = [ctypes.c_void_p, c_f32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32,
                                                ctypes.POINTER(ctypes.c_void_p), c_i64p]
            f("stream_next").argtypes = [ctypes.c_void_p, c_f32p, ctypes.c_int64, c_i64p]
            f("stream_close").argtypes = [ctypes.c_void_p]
            f("stream_close").restype = None
            f("persist_state").argtypes = [ctypes.c_void_p, ctypes.POINTER(PersistInfo)]
            # include/vits_resample.h: an extension of the product library (the oracle has no counterpart), declared where it exists
            self.has_resample = self.has("resample_plan")
            if self.has_resample:
                f("resample_plan").argtypes = [ctypes.c_int32, ctypes.c_int32, c_i32p, c_i32p, c_i32p, c_i32p]
                f("resample_table").argtypes = [ctypes.c_int32, ctypes.c_int32, c_f32p, ctypes.c_int64]
                f("op_resample").argtypes = [ctypes.c_int, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                             c_f32p]
                f("synthesize_rate").argtypes = [ctypes.c_void_p, c_i64p, c_i64p, ctypes.c_int32, ctypes.c_int32, c_f32p, c_i64p,
                                                 ctypes.POINTER(SynthOpts), ctypes.c_int32, ctypes.POINTER(c_f32p), c_i64p, c_i64p]
                f("synthesize_pcm16_rate").argtypes = [ctypes.c_void_p, c_i64p, c_i64p, ctypes.c_int32, ctypes.c_int32, c_f32p, c_i64p,
                                                       ctypes.POINTER(SynthOpts), ctypes.c_float, ctypes.c_int32,
                                                       ctypes.POINTER(c_i16p), c_i64p, c_i64p]
                f("stream_open_rate").argtypes = [ctypes.c_void_p, c_i64p, ctypes.c_int32, c_f32p, ctypes.c_int64,
                                                  ctypes.POINTER(SynthOpts), ctypes.c_int32, ctypes.c_int32,
                                                  ctypes.POINTER(ctypes.c_void_p), c_i64p]
                f("stream_open_latent_rate").argtypes = [ctypes.c_void_p, c_f32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32,
                                                         ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p), c_i64p]
            # include/vits_denoise.h: the vocoder-bias denoiser, an extension of the product library like the resampler
            self.has_denoise = self.has("op_denoise")
            if self.has_denoise:
                f("denoise_bias").argtypes = [ctypes.c_void_p, ctypes.c_int32, c_f32p, ctypes.c_int64]
                f("op_denoise").argtypes = [ctypes.c_int, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, c_f32p, ctypes.c_int32, ctypes.c_float,
                                            c_f32p]
                f("stream_open_latent_denoise").argtypes = [ctypes.c_void_p, c_f32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32,
                                                            ctypes.c_float, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p), c_i64p]
            # include/vits_marks.h: speech marks, an extension of the product library like the two above
            self.has_marks = self.has("synthesize_marks")
            if self.has_marks:
                f("synthesize_marks").argtypes = [ctypes.c_void_p, c_i64p, c_i64p, ctypes.c_int32, ctypes.c_int32, c_f32p, c_i64p,
                                                  ctypes.POINTER(SynthOpts), ctypes.c_int32, ctypes.POINTER(c_f32p), c_i64p, c_i64p, c_i64p]
                f("synthesize_pcm16_marks").argtypes = [ctypes.c_void_p, c_i64p, c_i64p, ctypes.c_int32, ctypes.c_int32, c_f32p, c_i64p,
                                                        ctypes.POINTER(SynthOpts), ctypes.c_float, ctypes.c_int32,
                                                        ctypes.POINTER(c_i16p), c_i64p, c_i64p, c_i64p]
                f("stream_marks").argtypes = [ctypes.c_void_p, c_i64p, ctypes.c_int32, c_i32p]
            # include/vits_loudness.h: loudness normalisation, an extension of the product library like the three above
            self.has_loudness = self.has("op_loudness")
            if self.has_loudness:
                f("loudness_plan").argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_double), c_i32p]
                f("op_loudness").argtypes = [ctypes.c_int, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, c_f32p, c_f32p]
                f("op_loudness_normalize").argtypes = [ctypes.c_int, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                                       ctypes.c_int32, ctypes.c_float, ctypes.c_float, c_f32p, c_f32p, c_f32p]
            # include/vits_limit.h: the look-ahead peak limiter (kernel-level doors and the host-only plan)
            self.has_limit = self.has("op_limit")
            if self.has_limit:
                lim = [ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_float]  # mode, ceiling, lookahead_ms, release_ms
                door = [ctypes.c_int, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32]
                f("limit_plan").argtypes = [ctypes.c_int32, ctypes.c_float, ctypes.c_float, c_i32p, ctypes.POINTER(ctypes.c_double)]
                f("op_true_peak").argtypes = door + [c_f32p]
                f("op_limit_gain").argtypes = door + lim + [ctypes.c_float, c_f32p]
                f("op_limit").argtypes = door + lim + [ctypes.c_float, c_f32p, c_f32p]
                f("op_loudness_limit").argtypes = door + [ctypes.c_float] + lim + [c_f32p, c_f32p, c_f32p, c_f32p]
            # include/vits_pitch.h: pitch-shifted output, an extension of the product library like the four above
            self.has_pitch = self.has("op_pitch_shift")
            if self.has_pitch:
                f("pitch_plan").argtypes = [ctypes.c_float, c_i32p, c_i32p]
                for name in ("op_pitch_shift", "op_pitch_stretch"):
                    f(name).argtypes = [ctypes.c_int, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, c_f32p]
                # include/vits_pitch_formant.h: the doors of the formant-preserving shift
                self.has_pitch_formant = self.has("op_pitch_formant_gain")
                if self.has_pitch_formant:
                    for name in ("op_pitch_shift_formant", "op_pitch_stretch_formant", "op_pitch_formant_gain"):
                        f(name).argtypes = [ctypes.c_int, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, c_f32p]
            # include/vits_prosody.h: prosody controls (the flag of the synthesize calls and the regulator's own door)
            self.has_prosody = self.has("op_regulate")
            if self.has_prosody:
                f("op_regulate").argtypes = [ctypes.c_int, c_f32p, c_i32p, c_i64p, ctypes.c_int32, ctypes.c_int32, ctypes.c_float,
                                             ctypes.POINTER(Prosody), c_i32p, c_i32p, c_i64p, c_f32p]
            # include/vits_contour.h: per-token pitch and volume contours (the flag of the synthesize calls and the two doors)
            self.has_contour = self.has("op_contour")
            if self.has_contour:
                door = [ctypes.c_int, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, c_i32p, c_i64p, ctypes.c_int32, ctypes.c_int32, c_f32p, c_f32p]
                f("op_contour").argtypes = door + [c_f32p]
                f("op_contour_stretch").argtypes = door + [c_f32p, c_i64p]
            # include/vits_intonation.h: the intonation range (the flag of the synthesize calls and the three doors)
            self.has_intonation = self.has("op_intonation")
            if self.has_intonation:
                door = [ctypes.c_int, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, c_i32p, c_i64p, ctypes.c_int32, ctypes.c_int32,
                        c_f32p, c_f32p, ctypes.c_float]
                f("op_f0_track").argtypes = [ctypes.c_int, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, c_i32p]
                f("op_intonation").argtypes = door + [c_f32p]
                f("op_intonation_stretch").argtypes = door + [c_f32p, c_i64p, c_i32p]
            # include/vits_document.h: documents (the two joined synthesize calls and the join's own door)
            self.has_document = self.has("op_document_join")
            if self.has_document:
                f("synthesize_document").argtypes = [ctypes.c_void_p, c_i64p, c_i64p, ctypes.c_int32, ctypes.c_int32, c_f32p, c_i64p,
                                                     ctypes.POINTER(SynthOpts), ctypes.POINTER(Document), ctypes.c_int32, ctypes.POINTER(c_f32p),
                                                     c_i64p, c_i64p]
                f("synthesize_document_pcm16").argtypes = [ctypes.c_void_p, c_i64p, c_i64p, ctypes.c_int32, ctypes.c_int32, c_f32p, c_i64p,
                                                           ctypes.POINTER(SynthOpts), ctypes.POINTER(Document), ctypes.c_float, ctypes.c_int32,
                                                           ctypes.POINTER(c_i16p), c_i64p, c_i64p]
                f("op_document_join").argtypes = [ctypes.c_int, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                                  ctypes.POINTER(Document), c_f32p, ctypes.c_int64, c_i64p, c_i32p, c_i32p]
            # include/vits_watermark.h: the keyed audio watermark (the flag of the synthesize calls and the two doors)
            self.has_watermark = self.has("op_watermark")
            if self.has_watermark:
                f("op_watermark").argtypes = [ctypes.c_int, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_float, c_f32p]
                f("op_watermark_detect").argtypes = [ctypes.c_int, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32,
                                                     ctypes.POINTER(ctypes.c_double), c_i32p, c_i32p, ctypes.POINTER(ctypes.c_double)]
            # include/vits_watermark_payload.h: 16 payload bits in the mark (the flag of the synthesize calls and the two doors)
            self.has_watermark_payload = self.has("op_watermark_payload")
            if self.has_watermark_payload:
                c_u32p, c_f64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)
                f("op_watermark_payload").argtypes = [ctypes.c_int, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_float,
                                                      c_u32p, c_f32p]
                f("op_watermark_read").argtypes = [ctypes.c_int, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, c_f64p, c_i32p,
                                                   c_i32p, c_u32p, c_i32p, c_f64p, c_f64p]
            # include/vits_watermark_scan.h: windowed detector scores (the localiser's door)
            self.has_watermark_scan = self.has("op_watermark_scan")
            if self.has_watermark_scan:
                f("watermark_scan_windows").argtypes = [ctypes.c_int64, ctypes.c_int32]
                f("watermark_scan_windows").restype = ctypes.c_int64
                f("op_watermark_scan").argtypes = [ctypes.c_int, c_f32p, c_i64p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_int32,
                                                   ctypes.c_uint32, ctypes.c_int64, ctypes.POINTER(ctypes.c_double), c_i32p, c_i32p]
            if self.has("debug_clock_probe"):
                f("debug_clock_probe").argtypes = [ctypes.c_int, ctypes.c_int32, ctypes.POINTER(ctypes.c_double), ctypes.c_int32]

    def _fn(self, name):
        return getattr(self.lib, self.prefix + name)

    def device_count(self):
        """HIP devices visible to this process (0 for the CPU oracle)"""
        if not self.is_device or not self.has("device_count"):
            return 0
        self._fn("device_count").restype = ctypes.c_int
        return int(self._fn("device_count")())

    def has(self, name):
        return hasattr(self.lib, self.prefix + name)

    def check(self, rc):
        if rc != 0:
            raise VitsError(rc, self._fn("last_error")().decode(errors="replace"))

    def create(self, blob, device=0):
        return VitsModel(self, blob, device)

    def _need_marks(self):
        if not self.has_marks:
            raise VitsError(4, "this backend has no speech marks (include/vits_marks.h): the CPU oracle returns audio only")

    def _need_tail(self, tail, family="VITS"):
        """every stage `tail` asks for must be one this library exports (VitsError 4 names the first that is not)"""
        if tail.watermark is not None:
            self._need_watermark()
            if tail_payload(tail) is not None:
                self._need_watermark_payload()
        if tail.pitch_range is not None:
            self._need_intonation()
        if tail.limit is not None:
            self._need_limit()
        if tail.pitch is not None:
            self._need_pitch_formant(family) if tail.formants else self._need_pitch()
        if tail.loudness is not None:
            self._need_loudness()

    def stream_marks(self, st):
        """vits_stream_marks of an open stream handle -> int64 [T_x] (empty for a latent stream)"""
        self._need_marks()
        n = ctypes.c_int32()
        self.check(self._fn("stream_marks")(st, None, 0, ctypes.byref(n)))  # (NULL, capacity 0: the count only)
        ends = np.zeros(n.value, np.int64)
        if n.value:
            self.check(self._fn("stream_marks")(st, _p(ends, c_i64p), n.value, ctypes.byref(n)))
        return ends

    def clock_probe(self, device=0, duration_us=20000, n=64):
        """vits_debug_clock_probe (include/vits_mi355_debug.h): shader clock in GHz seen by `n` one-wave workgroups that sit on the device
        for `duration_us` NEXT to whatever the caller has in flight on other streams -> sorted list.  Blocks for the duration."""
        out = (ctypes.c_double * n)()
        rc = self._fn("debug_clock_probe")(device, duration_us, out, n)
        if rc < 0:
            raise VitsError(-rc, self._fn("last_error")().decode(errors="replace"))
        return sorted(float(v) for v in out[:rc])

    def decoder_needs(self, hp):
        """vits_debug_decoder_needs (host arithmetic, no device): the decoder's per-layer limits in a ragged batch for the hparams struct
        `hp` -> dict(z_frames, pre_out, post_out, tail_cols, stages=[dict(ups_q, c1_out=[...], c2_out=[...])])"""
        buf = np.zeros(4 + 4 * 9, np.int32)
        n = self._fn("debug_decoder_needs")(ctypes.byref(hp), _p(buf, c_i32p), buf.shape[0])
        if n < 0:
            raise VitsError(-n, self._fn("last_error")().decode(errors="replace"))
        v = buf[:n].tolist()
        out = dict(z_frames=v[0], pre_out=v[1], post_out=v[2], tail_cols=v[3], stages=[])
        k, nd = 4, hp.n_resd
        for _ in range(hp.n_ups):
            out["stages"].append(dict(ups_q=v[k], c1_out=v[k + 1:k + 1 + nd], c2_out=v[k + 1 + nd:k + 1 + 2 * nd]))
            k += 1 + 2 * nd
        return out

    def rag_halo(self, hp):
        """vits_debug_rag_halo (host arithmetic, no device): the ragged / streaming halo in frames vits_create derives for `hp`"""
        n = self._fn("debug_rag_halo")(ctypes.byref(hp))
        if n < 0:
            raise VitsError(-n, self._fn("last_error")().decode(errors="replace"))
        return int(n)

    def launch_log(self, on):
        """vits_debug_launch_log: start (clearing the counters) or stop counting eager launches by (operation, kernel)"""
        self._fn("debug_launch_log")(int(on))

    def launch_count(self, op, kernel_prefix):
        """vits_debug_launch_count: launches of operation `op` counted so far whose kernel name starts with `kernel_prefix`"""
        return int(self._fn("debug_launch_count")(op.encode(), kernel_prefix.encode()))

    def launch_dump(self):
        """vits_debug_launch_dump: the whole launch log as {"op|kernel": count}"""
        buf = ctypes.create_string_buffer(1 << 16)
        self._fn("debug_launch_dump")(buf, ctypes.c_size_t(len(buf)))
        return {k: int(n) for k, n in (line.rsplit(" ", 1) for line in buf.value.decode().splitlines())}

    def _items_door(self, name, x, lengths, device, scalars, outs):
        """One kernel-level door over B items: vits_<name>(device, x, lengths, B, N, *scalars, *outputs) with x float32 [B, N] and
        lengths [B] checked here and float32 outputs of the shapes outs(B, N) -> the outputs (a lone one as itself)"""
        x = _f32(x)
        if x.ndim != 2:
            raise ValueError("x must be [B, N]")
        B, N = x.shape
        lengths = _i64(lengths).reshape(-1)
        if lengths.shape != (B,):
            raise ValueError("lengths must be [B]")
        ys = [np.empty(shape, np.float32) for shape in outs(B, N)]
        self.check(self._fn(name)(device, _p(x, c_f32p), _p(lengths, c_i64p), B, N, *scalars, *[_p(y, c_f32p) for y in ys]))
        return ys[0] if len(ys) == 1 else tuple(ys)

    # ---- output sample rate (include/vits_resample.h) -----------------------
    def _need_resample(self):
        if not self.has_resample:
            raise VitsError(4, "this backend has no resampler (include/vits_resample.h): only the voice's own sample rate")

    def resample_plan(self, rate_in, rate_out):
        """vits_resample_plan (host only): dict(L, M, taps, half) of rate_in -> rate_out; VitsError(4) names a refused pair"""
        self._need_resample()
        v = [ctypes.c_int32() for _ in range(4)]
        self.check(self._fn("resample_plan")(int(rate_in), int(rate_out), *[ctypes.byref(c) for c in v]))
        return dict(L=v[0].value, M=v[1].value, taps=v[2].value, half=v[3].value)

    def resample_table(self, rate_in, rate_out):
        """vits_resample_table (host only): the fp32 phase table [L, taps]"""
        P = self.resample_plan(rate_in, rate_out)
        tab = np.empty((P["L"], P["taps"]), np.float32)
        self.check(self._fn("resample_table")(int(rate_in), int(rate_out), _p(tab, c_f32p), tab.size))
        return tab

    def out_samples(self, n, rate_in, rate_out):
        """ceil(n * L / M): samples at rate_out of n samples at rate_in (rate_out 0 / None / rate_in: n)"""
        if not rate_out or rate_out == rate_in:
            return int(n)
        P = self.resample_plan(rate_in, rate_out)
        return -(-int(n) * P["L"] // P["M"])

    def op_resample(self, x, lengths, rate_in, rate_out, device=0):
        """vits_op_resample: x float32 [B, N], lengths [B] -> y float32 [B, ceil(N*L/M)]; item b from x[b, :lengths[b]] only"""
        self._need_resample()
        return self._items_door("op_resample", x, lengths, device, (int(rate_in), int(rate_out)),
                                lambda B, N: [(B, self.out_samples(N, rate_in, rate_out))])

    # ---- vocoder-bias denoiser (include/vits_denoise.h) ---------------------
    def _need_denoise(self):
        if not self.has_denoise:
            raise VitsError(4, "this backend has no denoiser (include/vits_denoise.h)")

    def op_denoise(self, x, lengths, bias, strength, filter_length=1024, device=0):
        """vits_op_denoise: x float32 [B, N], lengths [B], bias [filter_length / 2 + 1] -> y float32 [B, hop * (N // hop)], hop =
        filter_length / 4; item b from x[b, :lengths[b]] only, zero at and beyond hop * (lengths[b] // hop)"""
        self._need_denoise()
        n = int(filter_length)
        bias = _f32(bias).reshape(-1)
        if 0 < n <= 4096 and bias.shape[0] != n // 2 + 1:  # (a filter length the library refuses is refused there, by name)
            raise ValueError(f"bias must hold filter_length / 2 + 1 = {n // 2 + 1} values")
        hop = max(n // 4, 1)
        return self._items_door("op_denoise", x, lengths, device, (_p(bias, c_f32p), n, float(strength)), lambda B, N: [(B, hop * (N // hop))])

    # ---- loudness normalisation (include/vits_loudness.h) --------------------
    def _need_loudness(self):
        if not self.has_loudness:
            raise VitsError(4, "this backend has no loudness normalisation (include/vits_loudness.h)")

    def loudness_plan(self, rate):
        """vits_loudness_plan (host only): (sos float64 [2, 6] = rows of b0 b1 b2 1 a1 a2, hop); VitsError(4) names a refused rate"""
        self._need_loudness()
        sos = np.zeros((2, 6), np.float64)
        hop = ctypes.c_int32()
        self.check(self._fn("loudness_plan")(int(rate), sos.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(hop)))
        return sos, hop.value

    def op_loudness(self, x, lengths, rate, device=0):
        """vits_op_loudness: x float32 [B, N], lengths [B] -> (loudness float32 [B] in LUFS, -inf for silence; peak float32 [B]);
        item b from x[b, :lengths[b]] only"""
        self._need_loudness()
        return self._items_door("op_loudness", x, lengths, device, (int(rate),), lambda B, N: [(B,), (B,)])

    def op_loudness_normalize(self, x, lengths, rate, mode, target, ceiling=0.0, device=0):
        """vits_op_loudness_normalize -> (y float32 [B, N] = gain[b] * x[b], zero at and beyond lengths[b]; loudness [B]; gain [B])"""
        self._need_loudness()
        return self._items_door("op_loudness_normalize", x, lengths, device, (int(rate), int(mode), float(target), float(ceiling)),
                                lambda B, N: [(B, N), (B,), (B,)])

    # ---- look-ahead peak limiter (include/vits_limit.h) ------------------------
    def _need_limit(self):
        if not self.has_limit:
            raise VitsError(4, "this backend has no peak limiter (include/vits_limit.h)")

    def limit_plan(self, rate, lookahead_ms=5.0, release_ms=50.0):
        """vits_limit_plan (host only): (W samples of look-ahead, a = the release coefficient per sample); VitsError names a refused value"""
        self._need_limit()
        W, a = ctypes.c_int32(), ctypes.c_double()
        self.check(self._fn("limit_plan")(int(rate), float(lookahead_ms), float(release_ms), ctypes.byref(W), ctypes.byref(a)))
        return W.value, a.value

    def op_true_peak(self, x, lengths, rate, device=0):
        """vits_op_true_peak: x float32 [B, N], lengths [B] -> the 4x oversampled peak of every item, float32 [B]; item b from
        x[b, :lengths[b]] only"""
        self._need_limit()
        return self._items_door("op_true_peak", x, lengths, device, (int(rate),), lambda B, N: [(B,)])

    def op_limit_gain(self, x, lengths, rate, mode, ceiling, lookahead_ms=5.0, release_ms=50.0, gain=1.0, device=0):
        """vits_op_limit_gain -> s float32 [B, N]: the limiter's gain curve, 1 at and beyond lengths[b]"""
        self._need_limit()
        return self._items_door("op_limit_gain", x, lengths, device,
                                (int(rate), int(mode), float(ceiling), float(lookahead_ms), float(release_ms), float(gain)), lambda B, N: [(B, N)])

    def op_limit(self, x, lengths, rate, mode, ceiling, lookahead_ms=5.0, release_ms=50.0, gain=1.0, device=0):
        """vits_op_limit -> (y float32 [B, N] = fp32(gain s) x, zero at and beyond lengths[b]; reduction float32 [B] = min s)"""
        self._need_limit()
        return self._items_door("op_limit", x, lengths, device,
                                (int(rate), int(mode), float(ceiling), float(lookahead_ms), float(release_ms), float(gain)),
                                lambda B, N: [(B, N), (B,)])

    def op_loudness_limit(self, x, lengths, rate, target, mode, ceiling, lookahead_ms=5.0, release_ms=50.0, device=0):
        """vits_op_loudness_limit, the two-pass LUFS form -> (y float32 [B, N]; loudness [B] of the items as given; gain [B] = g_1;
        reduction [B] = min s of the last pass)"""
        self._need_limit()
        return self._items_door("op_loudness_limit", x, lengths, device,
                                (int(rate), float(target), int(mode), float(ceiling), float(lookahead_ms), float(release_ms)),
                                lambda B, N: [(B, N), (B,), (B,), (B,)])

    # ---- pitch-shifted output (include/vits_pitch.h) ---------------------------
    def _need_pitch(self):
        if not self.has_pitch:
            raise VitsError(4, "this backend has no pitch shifter (include/vits_pitch.h)")

    def pitch_plan(self, semitones):
        """vits_pitch_plan (host only): (P, Q) of a shift; VitsError(1) names a refused value"""
        self._need_pitch()
        P, Q = ctypes.c_int32(), ctypes.c_int32()
        self.check(self._fn("pitch_plan")(float(semitones), ctypes.byref(P), ctypes.byref(Q)))
        return P.value, Q.value

    def _need_pitch_formant(self, family="VITS"):
        self._need_pitch()
        if not self.has_pitch_formant:
            raise VitsError(4, f"this backend has no formant-preserving pitch shift (include/vits_pitch.h, {family}_FLAG_PITCH_FORMANT)")

    def op_pitch_shift(self, x, lengths, semitones, device=0, _door="op_pitch_shift"):
        """vits_op_pitch_shift: x float32 [B, N], lengths [B] -> y float32 [B, N]; item b from x[b, :lengths[b]] only, zero beyond"""
        self._need_pitch()
        return self._items_door(_door, x, lengths, device, (float(semitones),), lambda B, N: [(B, N)])

    def op_pitch_shift_formant(self, x, lengths, semitones, device=0):
        """vits_op_pitch_shift_formant: op_pitch_shift with the envelope correction (steps 3a-3d of include/vits_pitch.h)"""
        self._need_pitch_formant()
        return self.op_pitch_shift(x, lengths, semitones, device, "op_pitch_shift_formant")

    def op_pitch_stretch_formant(self, x, lengths, semitones, device=0):
        """vits_op_pitch_stretch_formant: op_pitch_stretch with the envelope correction"""
        self._need_pitch_formant()
        return self.op_pitch_stretch(x, lengths, semitones, device, "op_pitch_stretch_formant")

    def op_pitch_formant_gain(self, x, lengths, semitones, device=0):
        """vits_op_pitch_formant_gain: the gains of step 3d, float32 [B, N // 256 + 3, 513]; row f of item b is g_f for f < F_a[b], every
        other row exactly 0"""
        self._need_pitch_formant()
        return self._items_door("op_pitch_formant_gain", x, lengths, device, (float(semitones),),
                                lambda B, N: [(B, N // 256 + 3, PITCH_FRAME // 2 + 1)])

    def op_pitch_stretch(self, x, lengths, semitones, device=0, _door="op_pitch_stretch"):
        """vits_op_pitch_stretch: the vocoder's output before the resampler, float32 [B, 256 * (ceil((N // 256 + 2) * P / Q) - 1)]"""
        self._need_pitch()

        def outs(B, N):
            P, Q = self.pitch_plan(semitones)
            return [(B, 256 * (-(-(N // 256 + 2) * P // Q) - 1))]

        return self._items_door(_door, x, lengths, device, (float(semitones),), outs)

    # ---- per-token contours (include/vits_contour.h) ----------------------------
    def _need_document(self):
        if not self.has_document:
            raise VitsError(4, "this backend has no documents (include/vits_document.h)")

    def op_document_join(self, x, len_frames, hop, y=None, y_cap=None, device=0, **doc):
        """vits_op_document_join: x float32 [B, N], len_frames [B] -> (y float32 [y_cap], F, start int32 [B], trim int32 [B, 2]).  y: the
        buffer the join writes into (its samples at and beyond F * hop come back as they went), default NaN-filled, of y_cap samples
        (default: the untrimmed bound).  **doc: the controls of document_struct()."""
        self._need_document()
        x = _f32(x)
        if x.ndim != 2:
            raise ValueError("x must be [B, N]")
        B, N = x.shape
        lf = _i64(len_frames).reshape(-1)
        if lf.shape != (B,):
            raise ValueError("len_frames must be [B]")
        d, keep, _ = document_struct(B, outputs=False, **doc)
        if y is None:
            if y_cap is None:
                g = keep[0] if keep else np.zeros(B, np.int32)
                y_cap = (int(d.lead_frames) + int(lf.sum()) + int(g.sum())) * int(hop)
            y = np.full(max(int(y_cap), 0), np.nan, np.float32)
        else:
            y = _f32(y).copy()
        F = ctypes.c_int64()
        start = np.zeros(B, np.int32)
        trim = np.zeros((B, 2), np.int32)
        self.check(self._fn("op_document_join")(device, _p(x, c_f32p), _p(lf, c_i64p), B, N, int(hop), ctypes.byref(d), _p(y, c_f32p), y.shape[0],
                                                ctypes.byref(F), _p(start, c_i32p), _p(trim, c_i32p)))
        return y, int(F.value), start, trim

    def _need_contour(self):
        if not self.has_contour:
            raise VitsError(4, "this backend has no pitch / volume contours (include/vits_contour.h)")

    def _contour_door(self, name, x, lengths, cum, tok_lengths, hop, token_semitones, token_gain_db, device, outs):
        self._need_contour()
        x = _f32(x)
        if x.ndim != 2:
            raise ValueError("x must be [B, N]")
        B, N = x.shape
        lengths = _i64(lengths).reshape(-1)
        cum = _i32(cum)
        tok_lengths = _i64(tok_lengths).reshape(-1)
        if lengths.shape != (B,) or tok_lengths.shape != (B,) or cum.ndim != 2 or cum.shape[0] != B:
            raise ValueError("lengths and tok_lengths must be [B], cum [B, T_x]")
        Tx = cum.shape[1]
        st = None if token_semitones is None else _f32(token_semitones)
        db = None if token_gain_db is None else _f32(token_gain_db)
        for a in (st, db):
            if a is not None and a.shape != (B, Tx):
                raise ValueError("token_semitones / token_gain_db must be [B, T_x]")
        ys = outs(B, N)
        self.check(self._fn(name)(device, _p(x, c_f32p), _p(lengths, c_i64p), B, N, _p(cum, c_i32p), _p(tok_lengths, c_i64p), Tx, int(hop),
                                  _p(st, c_f32p), _p(db, c_f32p), *[_p(y, c_f32p if y.dtype == np.float32 else c_i64p) for y in ys]))
        return ys

    def op_contour(self, x, lengths, cum, tok_lengths, hop, token_semitones=None, token_gain_db=None, device=0):
        """vits_op_contour: x float32 [B, N], lengths [B], cum int32 [B, T_x] (inclusive frame counts), tok_lengths [B], hop samples per
        frame, token_semitones / token_gain_db float32 [B, T_x] or None -> y float32 [B, N]; item b from x[b, :lengths[b]] only"""
        return self._contour_door("op_contour", x, lengths, cum, tok_lengths, hop, token_semitones, token_gain_db, device,
                                  lambda B, N: [np.empty((B, N), np.float32)])[0]

    def op_contour_stretch(self, x, lengths, cum, tok_lengths, hop, token_semitones=None, token_gain_db=None, device=0):
        """vits_op_contour_stretch: (u float32 [B, 256 * (2 * (N // 256 + 2) - 1)], steps int64 [B, 2 * (N // 256 + 2) + 2]); row b of steps
        is F_s, a_0 .. a_{F_s}, then zeros"""
        return tuple(self._contour_door("op_contour_stretch", x, lengths, cum, tok_lengths, hop, token_semitones, token_gain_db, device,
                                        lambda B, N: [np.empty((B, 256 * (2 * (N // 256 + 2) - 1)), np.float32),
                                                      np.empty((B, 2 * (N // 256 + 2) + 2), np.int64)]))

    # ---- intonation range (include/vits_intonation.h) ----------------------------
    def _need_intonation(self):
        if not self.has_intonation:
            raise VitsError(4, "this backend has no intonation control (include/vits_intonation.h)")

    def op_f0_track(self, x, lengths, rate, device=0):
        """vits_op_f0_track: x float32 [B, N], lengths [B], rate in Hz -> cents int32 [B, 1 + N // 256]: 1200 log2(f0 / 27.5) of every
        analysis row, 0 where unvoiced, behind an item's rows and for an item below 513 samples"""
        self._need_intonation()
        x = _f32(x)
        if x.ndim != 2:
            raise ValueError("x must be [B, N]")
        B, N = x.shape
        lengths = _i64(lengths).reshape(-1)
        if lengths.shape != (B,):
            raise ValueError("lengths must be [B]")
        cents = np.empty((B, 1 + N // 256), np.int32)
        self.check(self._fn("op_f0_track")(device, _p(x, c_f32p), _p(lengths, c_i64p), B, N, int(rate), _p(cents, c_i32p)))
        return cents

    def _intonation_door(self, name, x, lengths, rate, pitch_range, cum, tok_lengths, hop, token_semitones, token_gain_db, device, outs):
        self._need_intonation()
        x = _f32(x)
        if x.ndim != 2:
            raise ValueError("x must be [B, N]")
        B, N = x.shape
        lengths = _i64(lengths).reshape(-1)
        if lengths.shape != (B,):
            raise ValueError("lengths must be [B]")
        Tx, st, db = 0, None, None
        if cum is not None:
            cum = _i32(cum)
            tok_lengths = _i64(tok_lengths).reshape(-1)
            if tok_lengths.shape != (B,) or cum.ndim != 2 or cum.shape[0] != B:
                raise ValueError("tok_lengths must be [B], cum [B, T_x]")
            Tx = cum.shape[1]
            st = None if token_semitones is None else _f32(token_semitones)
            db = None if token_gain_db is None else _f32(token_gain_db)
            for a in (st, db):
                if a is not None and a.shape != (B, Tx):
                    raise ValueError("token_semitones / token_gain_db must be [B, T_x]")
        elif tok_lengths is not None or token_semitones is not None or token_gain_db is not None:
            raise ValueError("tok_lengths, token_semitones and token_gain_db need cum")
        else:
            tok_lengths = None
        ys = outs(B, N)
        typ = {np.dtype(np.float32): c_f32p, np.dtype(np.int64): c_i64p, np.dtype(np.int32): c_i32p}
        self.check(self._fn(name)(device, _p(x, c_f32p), _p(lengths, c_i64p), B, N, int(rate), _p(cum, c_i32p), _p(tok_lengths, c_i64p), Tx, int(hop),
                                  _p(st, c_f32p), _p(db, c_f32p), float(pitch_range), *[_p(y, typ[y.dtype]) for y in ys]))
        return ys

    def op_intonation(self, x, lengths, rate, pitch_range, cum=None, tok_lengths=None, hop=256, token_semitones=None, token_gain_db=None, device=0):
        """vits_op_intonation: x float32 [B, N], lengths [B], rate in Hz, pitch_range r in [0, 4]; optionally the tokens of op_contour (cum
        int32 [B, T_x], tok_lengths [B], hop, token_semitones / token_gain_db) -> y float32 [B, N]; item b from x[b, :lengths[b]] only"""
        return self._intonation_door("op_intonation", x, lengths, rate, pitch_range, cum, tok_lengths, hop, token_semitones, token_gain_db, device,
                                     lambda B, N: [np.empty((B, N), np.float32)])[0]

    def op_intonation_stretch(self, x, lengths, rate, pitch_range, cum=None, tok_lengths=None, hop=256, token_semitones=None, token_gain_db=None,
                              device=0):
        """vits_op_intonation_stretch: (u, steps) with the shapes of op_contour_stretch and cents int32 [B, 1 + N // 256], the track the
        ratios came from"""
        return tuple(self._intonation_door("op_intonation_stretch", x, lengths, rate, pitch_range, cum, tok_lengths, hop, token_semitones,
                                           token_gain_db, device,
                                           lambda B, N: [np.empty((B, 256 * (2 * (N // 256 + 2) - 1)), np.float32),
                                                         np.empty((B, 2 * (N // 256 + 2) + 2), np.int64), np.empty((B, 1 + N // 256), np.int32)]))

    # ---- keyed audio watermark (include/vits_watermark.h) ---------------------------
    def _need_watermark(self):
        if not self.has_watermark:
            raise VitsError(4, "this backend has no audio watermark (include/vits_watermark.h)")

    def op_watermark(self, x, lengths, key, depth_db=0.0, device=0):
        """vits_op_watermark: x float32 [B, N], lengths [B], key uint32, depth_db (0 = 1 dB) -> y float32 [B, N]; item b marked on
        [0, 256 * (lengths[b] // 256)), x from there up to lengths[b], zero beyond; an item below 513 samples as it went in"""
        self._need_watermark()
        return self._items_door("op_watermark", x, lengths, device, (int(key) & 0xFFFFFFFF, float(depth_db)), lambda B, N: [(B, N)])

    def op_watermark_detect(self, x, lengths, key, device=0):
        """vits_op_watermark_detect: x float32 [B, N], lengths [B] -> (z float64 [B], offset int32 [B] in samples, rows int32 [B],
        z_all float64 [B, 128]); detected iff z >= WATERMARK_THRESHOLD"""
        self._need_watermark()
        x = _f32(x)
        if x.ndim != 2:
            raise ValueError("x must be [B, N]")
        B, N = x.shape
        lengths = _i64(lengths).reshape(-1)
        if lengths.shape != (B,):
            raise ValueError("lengths must be [B]")
        z, z_all = np.empty(B, np.float64), np.empty((B, WATERMARK_OFFSETS), np.float64)
        off, rows = np.empty(B, np.int32), np.empty(B, np.int32)
        c_f64p = ctypes.POINTER(ctypes.c_double)
        self.check(self._fn("op_watermark_detect")(device, _p(x, c_f32p), _p(lengths, c_i64p), B, N, int(key) & 0xFFFFFFFF, _p(z, c_f64p),
                                                   _p(off, c_i32p), _p(rows, c_i32p), _p(z_all, c_f64p)))
        return z, off, rows, z_all

    # ---- watermark payload (include/vits_watermark_payload.h) ------------------------
    def _need_watermark_payload(self):
        if not self.has_watermark_payload:
            raise VitsError(4, "this backend has no watermark payload (include/vits_watermark_payload.h)")

    def op_watermark_payload(self, x, lengths, key, payloads, depth_db=0.0, device=0):
        """vits_op_watermark_payload: op_watermark with one payload in [0, 65535] per item (payloads [B]; depth_db 0 = 2 dB)"""
        self._need_watermark_payload()
        pl = np.ascontiguousarray(np.asarray(payloads).reshape(-1), np.uint32)
        if pl.shape[0] != np.shape(x)[0]:
            raise ValueError("payloads must be [B]")
        return self._items_door("op_watermark_payload", x, lengths, device,
                                (int(key) & 0xFFFFFFFF, float(depth_db), pl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))), lambda B, N: [(B, N)])

    def op_watermark_read(self, x, lengths, key, device=0):
        """vits_op_watermark_read: x float32 [B, N], lengths [B] -> (z float64 [B], offset int32 [B] in samples, rows int32 [B],
        payload uint32 [B], valid int32 [B], z_all float64 [B, 128], bit_z float64 [B, 24]); detected iff z >= WATERMARK_THRESHOLD, the
        payload is to be believed iff valid"""
        self._need_watermark_payload()
        x = _f32(x)
        if x.ndim != 2:
            raise ValueError("x must be [B, N]")
        B, N = x.shape
        lengths = _i64(lengths).reshape(-1)
        if lengths.shape != (B,):
            raise ValueError("lengths must be [B]")
        z, z_all, bit_z = np.empty(B, np.float64), np.empty((B, WATERMARK_OFFSETS), np.float64), np.empty((B, WATERMARK_CODED_BITS), np.float64)
        off, rows, valid, payload = np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.uint32)
        c_f64p = ctypes.POINTER(ctypes.c_double)
        self.check(self._fn("op_watermark_read")(device, _p(x, c_f32p), _p(lengths, c_i64p), B, N, int(key) & 0xFFFFFFFF, _p(z, c_f64p),
                                                 _p(off, c_i32p), _p(rows, c_i32p), payload.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                 _p(valid, c_i32p), _p(z_all, c_f64p), _p(bit_z, c_f64p)))
        return z, off, rows, payload, valid, z_all, bit_z

    # ---- watermark localisation (include/vits_watermark_scan.h) ----------------------
    def _need_watermark_scan(self):
        if not self.has_watermark_scan:
            raise VitsError(4, "this backend has no watermark scan (include/vits_watermark_scan.h)")

    def watermark_scan_windows(self, n_samples, span=0):
        """vits_watermark_scan_windows: the most windows of `span` periods any offset of an item of n_samples holds"""
        self._need_watermark_scan()
        n = self._fn("watermark_scan_windows")(int(n_samples), int(span))
        if n < 0:
            self.check(1)  # VITS_ERR_ARG, named by vits_last_error
        return int(n)

    def op_watermark_scan(self, x, lengths, key, span=0, pilots=False, device=0, w_cap=None):
        """vits_op_watermark_scan: x float32 [B, N], lengths [B], span 1 .. 8 (0 = 4) -> (z_scan float64 [B, 128, w_cap], the score of
        window w of `span` pattern periods at offset index o, exactly 0 beyond windows[b, o]; first_period int32 [B, 128], p0;
        windows int32 [B, 128], W_o).  pilots: score the pilot positions only (audio marked with a payload).  w_cap: default what the
        longest item needs, at least 1.  vosk_tts_amd.watermark_scan turns the three into segments."""
        self._need_watermark_scan()
        x = _f32(x)
        if x.ndim != 2:
            raise ValueError("x must be [B, N]")
        B, N = x.shape
        lengths = _i64(lengths).reshape(-1)
        if lengths.shape != (B,):
            raise ValueError("lengths must be [B]")
        if w_cap is None:
            w_cap = max([1] + [self.watermark_scan_windows(n, span) for n in lengths if 0 <= n <= N])
        w_cap = int(w_cap)
        z = np.empty((B, WATERMARK_OFFSETS, max(w_cap, 0)), np.float64)
        p0, wins = np.empty((B, WATERMARK_OFFSETS), np.int32), np.empty((B, WATERMARK_OFFSETS), np.int32)
        self.check(self._fn("op_watermark_scan")(device, _p(x, c_f32p), _p(lengths, c_i64p), B, N, int(key) & 0xFFFFFFFF, int(span),
                                                 WATERMARK_SCAN_PILOTS if pilots else 0, w_cap, _p(z, ctypes.POINTER(ctypes.c_double)),
                                                 _p(p0, c_i32p), _p(wins, c_i32p)))
        return z, p0, wins

    # ---- prosody controls (include/vits_prosody.h) ------------------------------
    def _need_prosody(self):
        if not self.has_prosody:
            raise VitsError(4, "this backend has no prosody controls (include/vits_prosody.h)")

    def op_regulate(self, logw, forced, lengths, length_scale=1.0, item_scales=None, token_length_scale=None, token_pause=None,
                    fit_frames=None, device=0):
        """vits_op_regulate, the controlled length regulator alone: logw float32 [B, T_x] or None with forced int32 [B, T_x], lengths [B]
        -> (durations int32 [B, T_x], cum int32 [B, T_x], y_lengths int64 [B], fit_ratio float32 [B])"""
        self._need_prosody()
        logw = _f32(logw) if logw is not None else None
        forced = _i32(forced) if forced is not None else None
        src = logw if logw is not None else forced
        if src is None or src.ndim != 2 or (logw is not None and forced is not None and logw.shape != forced.shape):
            raise ValueError("logw / forced must be [B, T_x]")
        B, Tx = src.shape
        lengths = _i64(lengths).reshape(-1)
        if lengths.shape != (B,):
            raise ValueError("lengths must be [B]")
        arrays = prosody_arrays(B, Tx, item_scales, token_length_scale, token_pause, fit_frames)
        P = prosody_struct(arrays) if arrays is not None else None
        dur, cum = np.zeros((B, Tx), np.int32), np.zeros((B, Tx), np.int32)
        ylen, ratio = np.zeros(B, np.int64), np.zeros(B, np.float32)
        self.check(self._fn("op_regulate")(device, _p(logw, c_f32p), _p(forced, c_i32p), _p(lengths, c_i64p), B, Tx, float(length_scale),
                                           ctypes.byref(P) if P is not None else None, _p(dur, c_i32p), _p(cum, c_i32p), _p(ylen, c_i64p),
                                           _p(ratio, c_f32p)))
        return dur, cum, ylen, ratio

    def mas_maximum_path(self, values, t_ys, t_xs, device=0):
        """monotonic_align.maximum_path_c (core.pyx:35-42): values float32 [B,T_y,T_x] -> paths int32 [B,T_y,T_x]."""
        values = _f32(values)
        if values.ndim != 3:
            raise ValueError("values must be [B,T_y,T_x]")
        B, Ty, Tx = values.shape
        t_ys = _i32(t_ys).reshape(-1); t_xs = _i32(t_xs).reshape(-1)
        if t_ys.shape != (B,) or t_xs.shape != (B,):
            raise ValueError("t_ys/t_xs must be [B]")
        paths = np.empty((B, Ty, Tx), np.int32)
        self.check(self._fn("mas_maximum_path")(device, _p(values, c_f32p), _p(t_ys, c_i32p), _p(t_xs, c_i32p), B, Ty, Tx,
                                                _p(paths, c_i32p)))
        return paths


class VitsModel:
    """Owns one vits_model* (weights resident on one device)."""

    def __init__(self, lib, blob, device=0):
        self.lib = lib
        self._h = ctypes.c_void_p()
        buf = (ctypes.c_char * len(blob)).from_buffer_copy(blob)
        lib.check(lib._fn("create")(ctypes.cast(buf, ctypes.c_void_p), len(blob), device, ctypes.byref(self._h)))
        self.hp = HParams()
        lib.check(lib._fn("get_hparams")(self._h, ctypes.byref(self.hp)))
        self.device = device

    def persist_state(self, with_device=True):
        """vits_persist_state: dict of the persistent-program state of this process (masks, timeouts, re-arms, completed launches).
        with_device=False: process-wide counters only (no device synchronisation; `launches` / `process_owns_device` are -1)."""
        info = PersistInfo()
        self.lib.check(self.lib._fn("persist_state")(self._h if with_device else None, ctypes.byref(info)))
        return {n: int(getattr(info, n)) for n, _ in PersistInfo._fields_ if n != "reserved"}

    def close(self):
        if self._h:
            self.lib._fn("destroy")(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _opts(self, B, Tx, noise_dp, noise_prior, forced_durations, seed, max_frames, solo=False, item_seeds=None, bert=None, loudness_out=None,
              prosody=None, prosody_out=None, contour=None, tail=None, **tail_kw):
        """the options struct of a call and what it points at -> (opts, keep).  tail: the call's Tail, or **tail_kw: the keywords of
        tail_of() (loudness, limit, pitch, preserve_formants, pitch_range, watermark)"""
        tail = tail or tail_of(**tail_kw)
        if contour is not None:
            self.lib._need_contour()
        if prosody is not None:
            self.lib._need_prosody()
        if tail is not PLAIN:
            self.lib._need_tail(tail)
        opts = VITS_TAIL.opts(tail, prosody, contour)
        keep = []
        if bert is not None:
            a = _f32(bert); keep.append(a)
            if a.shape != (B, self.hp.bert_dim, Tx):
                raise ValueError(f"bert must be [B, {self.hp.bert_dim}, T_x] (got {a.shape})")
            opts.bert = _p(a, c_f32p)
        if item_seeds is not None:
            a = np.ascontiguousarray(item_seeds, dtype=np.uint64); keep.append(a)
            if a.shape != (B,) or not solo:
                raise ValueError("item_seeds must be [B] and needs solo=True")
            opts.item_seeds = a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        if noise_dp is not None:
            a = _f32(noise_dp); keep.append(a)
            if a.shape != (B, 2, Tx):
                raise ValueError("noise_dp must be [B,2,T_x]")
            opts.noise_dp = _p(a, c_f32p)
        if noise_prior is not None:
            a = _f32(noise_prior); keep.append(a)
            if a.ndim != 3 or a.shape[0] != B or a.shape[1] != self.hp.inter_channels:
                raise ValueError("noise_prior must be [B,inter,T]")
            opts.noise_prior = _p(a, c_f32p)
            opts.noise_prior_stride = a.shape[2]
        if forced_durations is not None:
            a = _i32(forced_durations); keep.append(a)
            if a.shape != (B, Tx):
                raise ValueError("forced_durations must be [B,T_x]")
            opts.forced_durations = _p(a, c_i32p)
        opts.seed = seed
        opts.max_frames = max_frames
        opts.flags = 1 if solo else 0  # VITS_FLAG_SOLO_BATCH
        if tail is not PLAIN:
            VITS_TAIL.fill(opts, keep, tail, B, loudness_out)
        if prosody is not None:
            set_prosody(opts, keep, prosody, B, VITS_TAIL.prosody, prosody_out)
        if contour is not None:
            set_contour(opts, keep, contour, VITS_TAIL.contour)
        return opts, keep

    # ---- the hot path -----------------------------------------------------
    def _rate(self, sample_rate):
        """None / 0 / the voice's own rate -> 0 (the entry points without a rate); anything else needs the resampler"""
        rate = int(sample_rate or 0)
        if rate == self.hp.sampling_rate:
            rate = 0
        if rate:
            self.lib._need_resample()
        return rate

    def _call(self, ids, lengths, scales, sid, pcm, pcm_scale, document, sample_rate, marks, fit_ratio, loudness_out, inputs, tail, prosody, contour):
        """The body of synthesize / synthesize_pcm16 / synthesize_document: shape checks, options, one of the eight entry points
        vits_synthesize[_pcm16][_rate | _marks] and vits_synthesize_document[_pcm16] by (pcm, rate, marks, document), copy out, free.
        document: None, or the controls of document_struct(); inputs: the arguments of _opts from noise_dp to bert; prosody:
        (item_scales, token_length_scale, token_pause, fit_frames); contour: (token_pitch, token_gain_db)"""
        ids = _i64(ids)
        B, Tx = ids.shape
        lengths = _i64(lengths); sid = _i64(sid); scales = _f32(scales)
        if lengths.shape != (B,) or sid.shape != (B,) or scales.shape != (3,):
            raise ValueError("bad feed shapes")
        pros_out = {}
        opts, keep = self._opts(B, Tx, *inputs, loudness_out, prosody_arrays(B, Tx, *prosody), pros_out,
                                contour_arrays(B, Tx, *contour, lengths, tail.pitch), tail)
        head = (self._h, _p(ids, c_i64p), _p(lengths, c_i64p), B, Tx, _p(scales, c_f32p), _p(sid, c_i64p), ctypes.byref(opts))
        out = ctypes.POINTER(ctypes.c_int16)() if pcm else c_f32p()
        ns = ctypes.c_int64()
        scale = (float(pcm_scale),) if pcm else ()
        name = "_pcm16" if pcm else ""
        if document is not None:
            d, dkeep, info = document_struct(B, *document)
            rate = self._rate(sample_rate)
            ends = np.zeros((B, Tx), np.int64) if marks else None
            self.lib.check(self.lib._fn("synthesize_document" + name)(*head, ctypes.byref(d), *scale, rate, ctypes.byref(out), ctypes.byref(ns),
                                                                      _p(ends, c_i64p)))
        else:
            olen = np.zeros(B, dtype=np.int64)
            rate = self._rate(sample_rate)
            ends = None
            if marks:  # (token_ends int64 [B,T_x] as a third value)
                self.lib._need_marks()
                ends = np.zeros((B, Tx), np.int64)
            name += "_marks" if marks else "_rate" if rate else ""
            self.lib.check(self.lib._fn("synthesize" + name)(*head, *scale, *((rate,) if marks or rate else ()), ctypes.byref(out), ctypes.byref(ns),
                                                             _p(olen, c_i64p), *((_p(ends, c_i64p),) if marks else ())))
        try:
            if document is None:
                audio = np.ctypeslib.as_array(out, shape=(B, ns.value)).copy()
            else:
                audio = np.ctypeslib.as_array(out, shape=(ns.value,)).copy() if ns.value else np.zeros(0, np.int16 if pcm else np.float32)
        finally:
            self.lib._fn("free_pcm16" if pcm else "free_output")(out)
        if document is not None:
            if marks:
                info["token_ends"] = ends
            if loudness_out:  # (one item behind the join)
                for k in list(loudness_out):
                    loudness_out[k] = np.asarray(loudness_out[k])[:1]
            return audio, info
        res = (audio, olen, ends) if marks else (audio, olen)
        return res + (pros_out.get("fit_ratio", np.ones(B, np.float32)),) if fit_ratio else res

    def synthesize(self, ids, lengths, scales, sid, noise_dp=None, noise_prior=None, forced_durations=None, seed=0,
                   max_frames=0, solo=False, item_seeds=None, bert=None, sample_rate=None, marks=False, loudness=None, loudness_out=None,
                   pitch=None, preserve_formants=False, limit=None, item_scales=None, token_length_scale=None, token_pause=None,
                   fit_frames=None, fit_ratio=False, token_pitch=None, token_gain_db=None, pitch_range=None, watermark=None,
                   watermark_depth_db=None, watermark_payload=None):
        """watermark_payload: an int in [0, 65535], or one per item (VITS_FLAG_WATERMARK_PAYLOAD, include/vits_watermark_payload.h): the mark
        carries it, and op_watermark_read returns it; needs watermark=, and watermark_depth_db then defaults to 2.
        watermark: a 32-bit key (VITS_FLAG_WATERMARK, include/vits_watermark.h): every item marked on the device behind the resampler,
        in front of the loudness stage, the limiter and the int16 conversion; watermark_depth_db in (0, 2], default 1.  Lengths and marks
        do not change.
        pitch_range: r in [0, 4] (VITS_FLAG_INTONATION, include/vits_intonation.h): how far every item moves about its own median pitch,
        times r, from an F0 track of the finished waveform on the device; 0 is a monotone, 1 the call as it was.  Lengths and marks do not
        change.  Not with preserve_formants.
        token_pitch / token_gain_db: float [B, T_x] semitones / dB per token (VITS_FLAG_CONTOUR, include/vits_contour.h): every token
        raised or lowered by its own amount on the device, in the pitch stage's place; `pitch` is added to every token; lengths and marks
        do not change.  Not with preserve_formants.
        item_scales float [B, 3], token_length_scale float [B, T_x], token_pause int32 [B, T_x] frames, fit_frames int32 [B]
        (VITS_FLAG_PROSODY, include/vits_prosody.h): per-item [noise_scale, length_scale, noise_scale_w], per-token rates, pauses appended
        to a token's own span, and the frame count an item is fitted to (0: not fitted); fit_ratio=True appends the ratio s of every item,
        float32 [B] (1 where nothing was fitted), to the returned tuple.
        limit: a limit_spec() (VITS_FLAG_LIMIT, include/vits_limit.h): the look-ahead peak limiter with the loudness gain (a LUFS
        spec whose ceiling is 0) or alone; loudness_out then also receives "reduction" float32 [B].
        pitch: semitones in [-12, 12] (VITS_FLAG_PITCH, include/vits_pitch.h): every item shifted on the device behind the decoder,
        before the resampler; lengths and marks do not change.  preserve_formants (VITS_FLAG_PITCH_FORMANT): the spectral envelope stays
        where it was; without a pitch in effect it changes nothing.
        One .run(): returns (audio float32 [B,S], out_lengths int64 [B]); with marks=True (vits_synthesize_marks) a third value,
        token_ends int64 [B,T_x] in output samples (include/vits_marks.h).  solo=True (VITS_FLAG_SOLO_BATCH): every
        item equals its own single-utterance call with seed + b instead of the reference's padded-batch result.
        sample_rate: output rate in Hz (vits_synthesize_rate; S and out_lengths are then in output samples).
        loudness: a loudness_spec() (VITS_FLAG_LOUDNESS, include/vits_loudness.h): every item normalised on the device, last in the
        chain; loudness_out: a dict that receives "loudness" (LUFS of each un-normalised item) and "gain" float32 [B]."""
        return self._call(ids, lengths, scales, sid, False, 1.0, None, sample_rate, marks, fit_ratio, loudness_out,
                          (noise_dp, noise_prior, forced_durations, seed, max_frames, solo, item_seeds, bert),
                          tail_of(loudness, limit, pitch, preserve_formants, pitch_range, watermark_spec(watermark, watermark_depth_db, watermark_payload)),
                          (item_scales, token_length_scale, token_pause, fit_frames), (token_pitch, token_gain_db))

    def synthesize_pcm16(self, ids, lengths, scales, sid, pcm_scale=1.0, noise_dp=None, noise_prior=None, forced_durations=None,
                         seed=0, max_frames=0, solo=False, item_seeds=None, bert=None, sample_rate=None, marks=False, loudness=None,
                         loudness_out=None, pitch=None, preserve_formants=False, limit=None, item_scales=None, token_length_scale=None,
                         token_pause=None, fit_frames=None, fit_ratio=False, token_pitch=None, token_gain_db=None, pitch_range=None,
                         watermark=None, watermark_depth_db=None, watermark_payload=None):
        """watermark, watermark_depth_db, watermark_payload, pitch, preserve_formants, limit, item_scales, token_length_scale, token_pause, fit_frames, fit_ratio, token_pitch,
        token_gain_db, pitch_range: as for synthesize.
        synthesize() with Synth.synth_audio's `* scale` and audio_float_to_int16 (vosk_tts/synth.py:127-130) done on the
        device: returns (pcm int16 [B,S], out_lengths int64 [B]).  sample_rate: as for synthesize (vits_synthesize_pcm16_rate:
        the resampler does the conversion in its epilogue).  loudness / loudness_out: as for synthesize (pcm_scale multiplies the
        normalised audio, as before)."""
        return self._call(ids, lengths, scales, sid, True, pcm_scale, None, sample_rate, marks, fit_ratio, loudness_out,
                          (noise_dp, noise_prior, forced_durations, seed, max_frames, solo, item_seeds, bert),
                          tail_of(loudness, limit, pitch, preserve_formants, pitch_range, watermark_spec(watermark, watermark_depth_db, watermark_payload)),
                          (item_scales, token_length_scale, token_pause, fit_frames), (token_pitch, token_gain_db))

    def synthesize_document(self, ids, lengths, scales, sid, pcm=False, pcm_scale=1.0, lead_frames=0, gap_frames=None, fade_samples=0,
                            trim_db=None, trim_keep_frames=0, marks=False, seed=0, max_frames=0, item_seeds=None, bert=None, sample_rate=None,
                            loudness=None, loudness_out=None, pitch=None, preserve_formants=False, limit=None, item_scales=None,
                            token_length_scale=None, token_pause=None, fit_frames=None, token_pitch=None, token_gain_db=None, pitch_range=None,
                            forced_durations=None, watermark=None, watermark_depth_db=None, watermark_payload=None):
        """vits_synthesize_document / _pcm16 (include/vits_document.h): the B items of one SOLO batch call joined on the device into one
        piece of audio, in front of the resampler, the loudness stage, the limiter and the int16 conversion.  Returns (audio float32 or
        int16 [S], info): info["seg_start"] / ["seg_end"] int64 [B] in output samples, info["trim"] int32 [B, 2] frames, and with
        marks=True info["token_ends"] int64 [B, T_x].  The per-item keywords are those of synthesize; loudness_out receives ONE value per
        key, of the whole document.  watermark: the document is marked as the one item it has become; watermark_payload: ONE value."""
        self.lib._need_document()
        if isinstance(watermark_payload, (list, tuple, np.ndarray)):
            raise ValueError("watermark_payload of a document: one value, it is marked as the one item it has become")
        return self._call(ids, lengths, scales, sid, bool(pcm), pcm_scale, (lead_frames, gap_frames, fade_samples, trim_db, trim_keep_frames),
                          sample_rate, marks, False, loudness_out, (None, None, forced_durations, seed, max_frames, True, item_seeds, bert),
                          tail_of(loudness, limit, pitch, preserve_formants, pitch_range, watermark_spec(watermark, watermark_depth_db, watermark_payload)),
                          (item_scales, token_length_scale, token_pause, fit_frames), (token_pitch, token_gain_db))

    def stream(self, ids, scales, sid, chunk_frames=64, noise_dp=None, noise_prior=None, forced_durations=None, seed=0, bert=None,
               sample_rate=None, on_marks=None, loudness=None, pitch=None, limit=None, item_scales=None, token_length_scale=None,
               token_pause=None, fit_frames=None, fit_ratio=None, watermark=None, watermark_payload=None):
        """watermark_payload: refused, naming VITS_FLAG_WATERMARK_PAYLOAD.
        watermark: refused (vits_stream_open* refuse VITS_FLAG_WATERMARK the same way: a stream has no tail).
        item_scales [1, 3], token_length_scale [1, T_x], token_pause [1, T_x], fit_frames [1]: the prosody controls of synthesize
        (the open runs the controlled regulator; total_samples and the marks reflect them); fit_ratio: called once with the ratio,
        float32 [1], as soon as the stream is open.
        limit: refused, as loudness is (vits_stream_open* refuse VITS_FLAG_LIMIT).
        pitch: refused (vits_stream_open* refuse VITS_FLAG_PITCH the same way; here before any device work).
        Streaming synthesis of ONE utterance (vits_stream_*): a generator of float32 chunks of
        chunk_frames*hop_length samples (the last one shorter); their concatenation equals synthesize().
        sample_rate: output rate in Hz (vits_stream_open_rate): the chunk that covers input samples [a, b) holds the outputs
        ceil(a*L/M) <= n < ceil(b*L/M), so chunk sizes vary by one sample.
        on_marks: called once with token_ends int64 [T_x] (vits_stream_marks, the stream's own output samples) as soon as the
        stream is open, before the first chunk."""
        # (vits_stream_open* refuse the flags the same way; here before any device work)
        tail_of(loudness, limit, pitch, watermark=watermark_spec(watermark, None, watermark_payload)).refuse_stream(VITS_TAIL.word, None, lambda msg: VitsError(4, msg))
        if on_marks is not None:
            self.lib._need_marks()
        if not self.lib.has("stream_open"):
            raise VitsError(-1, "this backend has no streaming entry points")
        ids = _i64(ids).reshape(1, -1)
        Tx = ids.shape[1]
        scales = _f32(scales)
        pros_out = {}
        opts, keep = self._opts(1, Tx, noise_dp, noise_prior, forced_durations, seed, 0, bert=bert,
                                prosody=prosody_arrays(1, Tx, item_scales, token_length_scale, token_pause, fit_frames), prosody_out=pros_out)
        L = self.lib
        st = ctypes.c_void_p()
        total = ctypes.c_int64()
        rate = self._rate(sample_rate)
        if rate:
            L.check(L._fn("stream_open_rate")(self._h, _p(ids, c_i64p), Tx, _p(scales, c_f32p), int(sid), ctypes.byref(opts),
                                              int(chunk_frames), rate, ctypes.byref(st), ctypes.byref(total)))
        else:
            L.check(L._fn("stream_open")(self._h, _p(ids, c_i64p), Tx, _p(scales, c_f32p), int(sid), ctypes.byref(opts),
                                         int(chunk_frames), ctypes.byref(st), ctypes.byref(total)))
        if on_marks is not None:
            try:
                ends = L.stream_marks(st)
            except Exception:
                L._fn("stream_close")(st)
                raise
            on_marks(ends)
        if fit_ratio is not None:
            fit_ratio(pros_out.get("fit_ratio", np.ones(1, np.float32)))
        return self._drain(st, chunk_frames, rate)

    def denoise_bias(self, filter_length=1024):
        """vits_denoise_bias: float32 [filter_length / 2 + 1], the magnitudes of frame 0 of this vocoder's output for an all-zero
        input (computed once per filter length and cached in the model)"""
        self.lib._need_denoise()
        n = int(filter_length) or 1024
        bias = np.empty(max(n // 2 + 1, 1), np.float32)
        self.lib.check(self.lib._fn("denoise_bias")(self._h, int(filter_length), _p(bias, c_f32p), bias.shape[0]))
        return bias

    def stream_latent(self, z, chunk_frames=64, clamp=False, sample_rate=None, denoiser_strength=None, denoiser_filter_length=0):
        """Streams the decoder over a latent the caller holds (vits_stream_open_latent): z float32 [inter_channels, T_y].
        sample_rate: as for stream (vits_stream_open_latent_rate).  denoiser_strength (None = off): every chunk goes through the
        vocoder-bias denoiser (vits_stream_open_latent_denoise), chunk sizes unchanged; not together with another sample rate."""
        z = _f32(z)
        if z.ndim != 2 or z.shape[0] != self.hp.inter_channels:
            raise ValueError("z must be [inter_channels, T_y]")
        L = self.lib
        st = ctypes.c_void_p()
        total = ctypes.c_int64()
        rate = self._rate(sample_rate)
        if denoiser_strength is not None:
            L._need_denoise()
            if rate:
                raise VitsError(4, f"a stream with a denoiser (strength {denoiser_strength}) at sample_rate {rate} Hz is not supported: "
                                   f"only the voice's own {self.hp.sampling_rate} Hz")
            L.check(L._fn("stream_open_latent_denoise")(self._h, _p(z, c_f32p), z.shape[1], int(chunk_frames), 1 if clamp else 0,
                                                        float(denoiser_strength), int(denoiser_filter_length), ctypes.byref(st), ctypes.byref(total)))
            return self._drain(st, chunk_frames, 0)
        if rate:
            L.check(L._fn("stream_open_latent_rate")(self._h, _p(z, c_f32p), z.shape[1], int(chunk_frames), 1 if clamp else 0, rate,
                                                     ctypes.byref(st), ctypes.byref(total)))
        else:
            L.check(L._fn("stream_open_latent")(self._h, _p(z, c_f32p), z.shape[1], int(chunk_frames), 1 if clamp else 0,
                                                ctypes.byref(st), ctypes.byref(total)))
        return self._drain(st, chunk_frames, rate)

    def _drain(self, st, chunk_frames, rate=0):
        """generator over an open vits_stream; closes it when exhausted or dropped"""
        L = self.lib
        cap = int(chunk_frames) * self.hp.hop_length
        if rate:  # chunk sizes vary by one sample around chunk * hop * L / M
            cap = L.out_samples(cap, self.hp.sampling_rate, rate) + 1
        n = ctypes.c_int64()
        try:
            while True:
                buf = np.empty(cap, np.float32)
                L.check(L._fn("stream_next")(st, _p(buf, c_f32p), cap, ctypes.byref(n)))
                if n.value == 0:
                    break
                yield buf[:n.value]
        finally:
            L._fn("stream_close")(st)

    # ---- stage-level entry points (parity tests) ---------------------------
    def text_encoder(self, ids, lengths, sid):
        ids = _i64(ids); lengths = _i64(lengths); sid = _i64(sid)
        B, T = ids.shape
        H, I = self.hp.hidden_channels, self.hp.inter_channels
        x = np.empty((B, H, T), np.float32); m_p = np.empty((B, I, T), np.float32); logs_p = np.empty((B, I, T), np.float32)
        self.lib.check(self.lib._fn("stage_text_encoder")(self._h, _p(ids, c_i64p), _p(lengths, c_i64p), B, T,
                                                          _p(sid, c_i64p), _p(x, c_f32p), _p(m_p, c_f32p), _p(logs_p, c_f32p)))
        return x, m_p, logs_p

    def duration(self, x, lengths, sid, noise, noise_scale_w):
        x = _f32(x); lengths = _i64(lengths); sid = _i64(sid); noise = _f32(noise)
        B, _, T = x.shape
        logw = np.empty((B, T), np.float32)
        self.lib.check(self.lib._fn("stage_duration")(self._h, _p(x, c_f32p), _p(lengths, c_i64p), B, T, _p(sid, c_i64p),
                                                      _p(noise, c_f32p), noise_scale_w, _p(logw, c_f32p)))
        return logw

    def regulate(self, logw, forced, lengths, length_scale, m_p, logs_p, noise, noise_scale, T_cap):
        lengths = _i64(lengths)
        B = lengths.shape[0]
        logw = _f32(logw) if logw is not None else None
        forced = _i32(forced) if forced is not None else None
        T = (logw if logw is not None else forced).shape[-1]
        m_p = _f32(m_p); logs_p = _f32(logs_p)
        noise = _f32(noise) if noise is not None else None
        I = self.hp.inter_channels
        dur = np.zeros((B, T), np.int32); ylen = np.zeros(B, np.int64)
        z_p = np.zeros((B, I, T_cap), np.float32)
        self.lib.check(self.lib._fn("stage_regulate")(self._h, _p(logw, c_f32p), _p(forced, c_i32p), _p(lengths, c_i64p), B, T,
                                                      length_scale, _p(m_p, c_f32p), _p(logs_p, c_f32p), _p(noise, c_f32p),
                                                      noise_scale, T_cap, _p(dur, c_i32p), _p(ylen, c_i64p), _p(z_p, c_f32p)))
        return dur, ylen, z_p

    def flow(self, z_p, y_lengths, sid):
        z_p = _f32(z_p); y_lengths = _i64(y_lengths); sid = _i64(sid)
        B, _, T = z_p.shape
        z = np.empty_like(z_p)
        self.lib.check(self.lib._fn("stage_flow")(self._h, _p(z_p, c_f32p), _p(y_lengths, c_i64p), B, T, _p(sid, c_i64p),
                                                  _p(z, c_f32p)))
        return z

    def decoder(self, z, want_mb=True, sid=None):
        z = _f32(z)
        B, _, T = z.shape
        sid = _i64(sid) if sid is not None else None
        hop = self.hp.hop_length
        audio = np.empty((B, T * hop), np.float32)
        mb = None
        if want_mb and self.hp.dec_type in (0, 2):  # type 2: the sub-band signal before zero-stuffing, as for type 0
            mb = np.empty((B, self.hp.subbands, T * hop // self.hp.subbands), np.float32)
        self.lib.check(self.lib._fn("stage_decoder")(self._h, _p(z, c_f32p), B, T, _p(sid, c_i64p), _p(audio, c_f32p), _p(mb, c_f32p)))
        return audio, mb

    def algorithmic_flops(self, B, Tx, Ty):
        return float(self.lib._fn("algorithmic_flops")(self._h, B, Tx, Ty))


def op_conv1d(lib, x, w, bias, dilation=1, lrelu_slope=1.0, device=0):
    x = _f32(x); w = _f32(w)
    bias = _f32(bias) if bias is not None else None
    B, Cin, T = x.shape
    Cout, Cin2, K = w.shape
    assert Cin == Cin2
    y = np.empty((B, Cout, T), np.float32)
    lib.check(lib._fn("op_conv1d")(device, _p(x, c_f32p), _p(w, c_f32p), _p(bias, c_f32p), B, Cin, Cout, T, K, dilation,
                                   lrelu_slope, _p(y, c_f32p)))
    return y


class VitsDeviceSession:
    """Device-resident serving loop (vits_session_*): inputs and outputs are raw HBM pointers
    (e.g. torch tensors' data_ptr()); the forward runs asynchronously on the session's own HIP
    stream and is replayed as a cached hipGraph."""

    def __init__(self, model, max_B, max_Tx, max_Ty):
        self.model = model
        self.lib = model.lib
        if not self.lib.is_device:
            raise RuntimeError("device sessions exist only in the HIP library")
        self._h = ctypes.c_void_p()
        self.lib.check(self.lib._fn("session_create")(model._h, max_B, max_Tx, max_Ty, ctypes.byref(self._h)))
        L = self.lib
        L._fn("session_sync").argtypes = [ctypes.c_void_p]
        L._fn("session_set_options").argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        L._fn("session_profile_report").argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]

    def close(self):
        if self._h:
            self.lib._fn("session_destroy")(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synthesize_device(self, d_ids, d_lengths, B, Tx, scales, d_sid, d_forced, Ty, seed, d_audio, audio_capacity):
        scales = _f32(scales)
        self.lib.check(self.lib._fn("session_synthesize_device")(
            self._h, ctypes.c_void_p(d_ids), ctypes.c_void_p(d_lengths), B, Tx, _p(scales, c_f32p),
            ctypes.c_void_p(d_sid) if d_sid else None, ctypes.c_void_p(d_forced) if d_forced else None, Ty, seed,
            ctypes.c_void_p(d_audio), audio_capacity, None))

    def last_ms(self):
        ms = ctypes.c_float()
        self.lib.check(self.lib._fn("session_last_ms")(self._h, ctypes.byref(ms)))
        return ms.value

    def sync(self):
        self.lib.check(self.lib._fn("session_sync")(self._h))

    def set_options(self, use_graph=True, profile=False):
        self.lib.check(self.lib._fn("session_set_options")(self._h, int(use_graph), int(profile)))

    def graph_nodes(self):
        """kernel launches (graph nodes) of the captured forward, 0 before the first graph capture"""
        fn = self.lib._fn("session_graph_nodes")
        fn.argtypes = [ctypes.c_void_p]
        return int(fn(self._h))

    def set_sdp_always(self, on=True):
        """run the duration predictor even when durations are forced (fixed-work benchmark of the whole infer())"""
        self.lib.check(self.lib._fn("session_set_sdp_always")(self._h, int(on)))

    def profile_report(self):
        """-> {(op_name, kernel_instantiation): (launches, total_ms, flops)}"""
        buf = ctypes.create_string_buffer(1 << 16)
        self.lib.check(self.lib._fn("session_profile_report")(self._h, buf, len(buf)))
        out = {}
        for line in buf.value.decode().splitlines():
            name, kern, n, ms, fl = line.split()
            out[(name, kern)] = (int(n), float(ms), float(fl))
        return out
