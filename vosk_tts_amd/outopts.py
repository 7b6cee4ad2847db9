"""The extension feeds of the output tail (pitch -> resample -> normalise / limit, DESIGN.md "Output tail"), read once for both session
types: what a request's feed asks of the loudness, limiter, pitch and intonation stages, checked before any device work.  `lib` is the session's
library: a stage the loaded library does not export is refused here (its _need_* check)."""
from .capi import limit_spec, loudness_spec, pitch_spec, range_spec, watermark_spec


def loudness_from_feed(lib, feed):
    """"vits.loudness" (LUFS target), "vits.peak" (peak target) and "vits.peak_ceiling" -> capi.loudness_spec() (None = none); both
    targets at once and values out of range are ValueError"""
    limited = feed.get("vits.limit") is not None  # (then "vits.peak_ceiling" is the limiter's ceiling and the gain has no cap)
    spec = loudness_spec(feed.get("vits.loudness"), feed.get("vits.peak"), 0.0 if limited else feed.get("vits.peak_ceiling"))
    if spec is not None:
        lib._need_loudness()
    return spec


def limit_from_feed(lib, feed):
    """"vits.limit" ("sample" or "true"), "vits.limit_lookahead_ms", "vits.limit_release_ms" and, as the limiter's ceiling,
    "vits.peak_ceiling" -> capi.limit_spec() (None = none; include/vits_limit.h); values out of range and a peak target next to a
    limiter are ValueError"""
    spec = limit_spec(feed.get("vits.limit"), feed.get("vits.peak_ceiling"), feed.get("vits.limit_lookahead_ms", 5.0),
                      feed.get("vits.limit_release_ms", 50.0))
    if spec is not None:
        if feed.get("vits.peak") is not None:
            raise ValueError("\"vits.peak\" with \"vits.limit\": a peak target leaves a limiter nothing to do (a LUFS target, or the limiter alone)")
        lib._need_limit()
    return spec


def pitch_from_feed(lib, feed):
    """"vits.pitch" (semitones in [-12, 12]; include/vits_pitch.h) and "vits.pitch_formants" (bool) -> (the shift as a float, or None
    for none and for one that reduces to the identity; whether it keeps the spectral envelope).  The second modifies a shift: without
    one in effect it is False, the request as it was.  A value out of range is ValueError"""
    p = pitch_spec(feed.get("vits.pitch"))
    if p is None:
        return None, False
    lib._need_pitch()
    formants = bool(feed.get("vits.pitch_formants", False))
    if formants:
        lib._need_pitch_formant()
    return p, formants


def range_from_feed(lib, feed):
    """"vits.pitch_range" (r in [0, 4]; include/vits_intonation.h) -> r as a float, or None for none and for one whose
    lround(1000 r) is 1000 (the request as it was).  A value out of range is ValueError"""
    r = range_spec(feed.get("vits.pitch_range"))
    if r is not None:
        lib._need_intonation()
    return r


def watermark_from_feed(lib, feed):
    """"vits.watermark_key" (a 32-bit key; include/vits_watermark.h) and "vits.watermark_depth_db" (in (0, 2], default 1) -> the
    keywords of the models' calls, {} without a key (the request as it was).  A depth without a key and values out of range are
    ValueError"""
    key = feed.get("vits.watermark_key")
    if key is None:
        if feed.get("vits.watermark_depth_db") is not None:
            raise ValueError("\"vits.watermark_depth_db\" needs \"vits.watermark_key\"")
        return {}
    key, depth = watermark_spec(int(key), feed.get("vits.watermark_depth_db"))
    lib._need_watermark()
    return {"watermark": key} if not depth else {"watermark": key, "watermark_depth_db": depth}


# the document feeds (include/vits_document.h): feed key -> keyword of the models' synthesize_document
DOCUMENT_FEEDS = {"vits.doc_gap_frames": "gap_frames", "vits.doc_lead_frames": "lead_frames", "vits.doc_fade_samples": "fade_samples",
                  "vits.doc_trim_db": "trim_db", "vits.doc_trim_keep": "trim_keep_frames"}


def document_from_feed(lib, feed):
    """"vits.doc_gap_frames" (int [B] or one int), "vits.doc_lead_frames", "vits.doc_fade_samples", "vits.doc_trim_db" (None = off),
    "vits.doc_trim_keep" -> the keywords of synthesize_document; None when the feed names none of them (the request is no document).
    The library refuses values out of range, naming segment and value, before anything is launched."""
    kw = {v: feed[k] for k, v in DOCUMENT_FEEDS.items() if k in feed}
    if not kw:
        return None
    lib._need_document()
    return kw
