"""The output tail of a request (pitch -> resample -> mark -> normalise / limit, DESIGN.md "Output tail") as ONE value, `Tail`, between a
session's feed and the options struct of the C call: what the request asks of the stages behind the decoder, in the forms capi defines
(loudness_spec, limit_spec, pitch_spec, range_spec, watermark_spec).  Frozen and hashable: it is the last entry of a coalescer key.

What stays out of it, and why:
  - the output rate and `marks`: explicit arguments at every layer already, and the two families treat the rate differently (the VITS
    calls take it, the multistream session resamples on the host; SttsSession._tail_chain);
  - the per-token and per-item arrays (contour, prosody): unhashable, and they keep a request out of the coalescer anyway;
  - the document controls: another entry point (document_from_feed below);
  - the denoiser: it sits in front of the tail and has fields of its own.
"""
from dataclasses import dataclass

# the feed keys Tail.from_feed reads
TAIL_FEEDS = ("vits.loudness", "vits.peak", "vits.peak_ceiling", "vits.pitch", "vits.pitch_formants", "vits.limit", "vits.limit_lookahead_ms",
              "vits.limit_release_ms", "vits.pitch_range", "vits.watermark_key", "vits.watermark_depth_db",
              "vits.watermark_payload")

# why a stream has no tail: (field, what it cannot be, why, the feed a whole-utterance call takes)
_STREAM = (("loudness", "be loudness-normalised", "an integrated-loudness or peak target needs the whole utterance before the first chunk",
            "the loudness feeds"),
           ("limit", "be limited", "the limiter's look-ahead and its loudness passes need the whole utterance before the first chunk",
            "\"vits.limit\""),
           ("pitch", "be pitch-shifted", "the phase recursion needs the frames before a chunk", "\"vits.pitch\""),
           ("pitch_range", "take an intonation range", "the median of the F0 track needs the whole utterance before the first chunk",
            "\"vits.pitch_range\""),
           ("payload", "carry a watermark payload ({family}_FLAG_WATERMARK_PAYLOAD)", "the mark is a stage of the output tail, and a stream has none",
            "\"vits.watermark_payload\""),
           ("watermark", "be watermarked ({family}_FLAG_WATERMARK)", "the mark is a stage of the output tail, and a stream has none",
            "\"vits.watermark_key\""))


@dataclass(frozen=True)
class Tail:
    loudness: tuple = None     # capi.loudness_spec(): (mode, target, ceiling); include/vits_loudness.h
    limit: tuple = None        # capi.limit_spec(): (mode, ceiling, lookahead_ms, release_ms, gain); include/vits_limit.h
    pitch: float = None        # semitones, already reduced by capi.pitch_spec() (None: none, or one that is the identity)
    formants: bool = False     # that shift with the spectral envelope kept; False whenever pitch is None
    pitch_range: float = None  # capi.range_spec(); include/vits_intonation.h
    watermark: tuple = None    # capi.watermark_spec(): (key, depth_db, 0 = the default); include/vits_watermark.h.  A third entry: the
    #                            mark carries a payload (include/vits_watermark_payload.h): an int, one int per item, or, in a session's
    #                            Tail, capi.PAYLOAD_RIDES: the value rides with the request and does not decide its batch

    @property
    def payload(self):
        return self.watermark[2] if self.watermark is not None and len(self.watermark) > 2 else None

    @classmethod
    def from_feed(cls, lib, feed, payload_rides=False):
        """payload_rides: "vits.watermark_payload" is checked here and then kept OUT of the Tail (capi.PAYLOAD_RIDES in its place): the
        caller hands the value on with the request, so requests of one key with different payloads share a coalescer key.
        The tail a feed asks for, checked before any device work, in the order loudness, pitch, limit, range, watermark.  `lib` is the
        session's library: a stage it does not export is refused here (its _need_* check).  Values out of range, both loudness targets
        at once, "vits.peak" next to "vits.limit" and a depth without a key are ValueError.  "vits.pitch_formants" modifies a shift:
        without one in effect it changes nothing.  With "vits.limit", "vits.peak_ceiling" is the limiter's ceiling and the gain has no cap."""
        if feed.keys().isdisjoint(TAIL_FEEDS):
            return PLAIN
        from .capi import limit_spec, loudness_spec, pitch_spec, range_spec, watermark_spec  # (capi builds its options from a Tail)

        limited = feed.get("vits.limit") is not None
        loudness = loudness_spec(feed.get("vits.loudness"), feed.get("vits.peak"), 0.0 if limited else feed.get("vits.peak_ceiling"))
        if loudness is not None:
            lib._need_loudness()
        pitch = pitch_spec(feed.get("vits.pitch"))
        formants = pitch is not None and bool(feed.get("vits.pitch_formants", False))
        if pitch is not None:
            lib._need_pitch_formant() if formants else lib._need_pitch()
        limit = limit_spec(feed.get("vits.limit"), feed.get("vits.peak_ceiling"), feed.get("vits.limit_lookahead_ms", 5.0),
                           feed.get("vits.limit_release_ms", 50.0))
        if limit is not None:
            if feed.get("vits.peak") is not None:
                raise ValueError("\"vits.peak\" with \"vits.limit\": a peak target leaves a limiter nothing to do (a LUFS target, or the limiter alone)")
            lib._need_limit()
        pitch_range = range_spec(feed.get("vits.pitch_range"))
        if pitch_range is not None:
            lib._need_intonation()
        key = feed.get("vits.watermark_key")
        if key is None and feed.get("vits.watermark_depth_db") is not None:
            raise ValueError("\"vits.watermark_depth_db\" needs \"vits.watermark_key\"")
        payload = feed.get("vits.watermark_payload")
        if key is None and payload is not None:
            raise ValueError("\"vits.watermark_payload\" needs \"vits.watermark_key\": watermark_payload without watermark")
        watermark = None if key is None else watermark_spec(int(key), feed.get("vits.watermark_depth_db"), payload)
        if watermark is not None:
            lib._need_watermark()
            if payload is not None:
                lib._need_watermark_payload()
                if payload_rides:
                    from .capi import PAYLOAD_RIDES

                    watermark = watermark[:2] + (PAYLOAD_RIDES,)
        return cls(loudness, limit, pitch, formants, pitch_range, watermark)

    def kw(self):
        """the keywords of the models' synthesize calls; a stage that is not asked for adds none (a plain request: {})"""
        kw = {}
        if self.loudness is not None:
            kw["loudness"] = self.loudness
        if self.limit is not None:
            kw["limit"] = self.limit
        if self.pitch is not None:
            kw["pitch"] = self.pitch
            if self.formants:
                kw["preserve_formants"] = True
        if self.pitch_range is not None:
            kw["pitch_range"] = self.pitch_range
        if self.watermark is not None:
            kw["watermark"] = self.watermark[0]
            if self.watermark[1]:
                kw["watermark_depth_db"] = self.watermark[1]
            if self.payload is not None and not isinstance(self.payload, str):  # (capi.PAYLOAD_RIDES: the request's caller adds the value)
                kw["watermark_payload"] = self.payload
        return kw

    def refuse_stream(self, family, hint, error=ValueError):
        """A stream has no tail: raises for the first stage asked for.  family: "VITS" / "STTS", the word of the flag the message names;
        hint: the calls that do take the feed ("run() / run_pcm16() take"; None: the models' form, without one); error: message ->
        exception, ValueError for the sessions, a VitsError(4, ...) for the models"""
        for field, what, why, feeds in _STREAM:
            if getattr(self, field) is not None:
                raise error(f"a stream cannot {what.format(family=family)}: {why}" + (f" ({hint} {feeds})" if hint else ""))


PLAIN = Tail()

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
