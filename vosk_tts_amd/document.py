"""Documents: many sentences and speakers in one call (include/vits_document.h).  This module is the text side: the segments of a
document, the splitter that makes them from plain text, seconds -> frames, and the marks of the segments stitched into one
SpeechMarks.  Pure functions; nothing touches the engine.

Splitting rule (split): paragraphs end at blank lines.  Inside a paragraph a sentence ends behind a run of `. ! ? …` plus any closing
quotes or brackets, when white space or the end of the text follows.  Abbreviations are not recognised: "Dr. Smith" is two pieces, as
the rule says.  A piece without a word (only punctuation, only a dash) merges into its neighbour: the one in front of it in the same
paragraph, else the one behind it.  A sentence whose token count -- as counted by the voice's own front end, `count(text)` -- exceeds
max_tokens is cut at the last `, ; : —` that fits (the mark stays with the piece in front of it), else at the last space that fits,
else where it must.  512 is the limit of the single-utterance programs.
"""
import math
import re

import numpy as np

_SENT_END = re.compile(r"[.!?…]+[\"'»”’)\]]*(?=\s|$)")
_CLAUSE = ",;:—"
_WORD = re.compile(r"\w", re.UNICODE)

SENTENCE_PAUSE = 0.2   # seconds behind a sentence (a design choice, not a measurement)
PARAGRAPH_PAUSE = 0.6  # seconds behind a paragraph (likewise)
MAX_TOKENS = 512       # the single-utterance programs' limit


class Segment:
    """One segment of a document: its text, and what may differ between segments.  speaker_id None = the call's; pause_after None = the
    call's sentence / paragraph pause (by `kind`), else seconds; speech_rate None = the call's; word_rates / pauses / word_pitch /
    word_gains: the per-word keywords of Synth.synth_audio, counted over this segment's words."""

    def __init__(self, text, speaker_id=None, pause_after=None, speech_rate=None, word_rates=None, pauses=None, word_pitch=None,
                 word_gains=None, kind="sentence"):
        if kind not in ("sentence", "paragraph-end"):
            raise ValueError(f"segment kind {kind!r}: 'sentence' or 'paragraph-end'")
        self.text, self.speaker_id, self.pause_after, self.speech_rate = text, speaker_id, pause_after, speech_rate
        self.word_rates, self.pauses, self.word_pitch, self.word_gains, self.kind = word_rates, pauses, word_pitch, word_gains, kind

    def __repr__(self):
        return f"Segment({self.text!r}, kind={self.kind!r}, speaker_id={self.speaker_id!r}, pause_after={self.pause_after!r})"

    def __eq__(self, other):
        return isinstance(other, Segment) and self.__dict__ == other.__dict__


def has_word(text):
    return _WORD.search(text) is not None


def _sentences(paragraph):
    """the pieces of one paragraph under the sentence rule, pieces without a word merged into a neighbour"""
    pieces, at = [], 0
    for m in _SENT_END.finditer(paragraph):
        pieces.append(paragraph[at:m.end()].strip())
        at = m.end()
    if paragraph[at:].strip():
        pieces.append(paragraph[at:].strip())
    out = []
    for p in pieces:
        if not p:
            continue
        if out and (not has_word(p) or not has_word(out[-1])):
            out[-1] = out[-1] + " " + p
        else:
            out.append(p)
    return out


def _last_that_fits(rest, places, max_tokens, count):
    """the largest position of the ascending `places` whose prefix counts at most max_tokens, or None: the token count does not fall as
    a prefix grows, so the positions that fit are a prefix of the list and a bisection finds its end in log2(n) calls of count"""
    lo, hi = 0, len(places)  # places[:lo] fit, places[hi:] do not
    while lo < hi:
        mid = (lo + hi) // 2
        if count(rest[:places[mid]].strip()) <= max_tokens:
            lo = mid + 1
        else:
            hi = mid
    return places[lo - 1] if lo else None


def _cut(sentence, max_tokens, count):
    """a sentence of more than max_tokens tokens -> pieces that fit"""
    out, rest = [], sentence
    while count(rest) > max_tokens:
        cut = None
        for marks in ([i + 1 for i, ch in enumerate(rest) if ch in _CLAUSE], [i for i, ch in enumerate(rest) if ch.isspace()]):
            places = [i for i in marks if 0 < i < len(rest) and has_word(rest[:i]) and has_word(rest[i:])]
            cut = _last_that_fits(rest, places, max_tokens, count)
            if cut is not None:
                break
        if cut is None:  # one word longer than the limit: the longest prefix that fits
            cut = _last_that_fits(rest, list(range(1, len(rest))), max_tokens, count) or 1
        out.append(rest[:cut].strip())
        rest = rest[cut:].strip()
    out.append(rest)
    return [p for p in out if p]


def split(text, max_tokens=MAX_TOKENS, count=len):
    """text -> [Segment] with kind 'sentence' or 'paragraph-end' (the last segment of every paragraph).  count(text) -> the number of
    tokens the voice's front end makes of it (default: characters)."""
    if max_tokens < 1:
        raise ValueError(f"max_tokens {max_tokens}: at least 1")
    segs = []
    for para in re.split(r"\n[ \t\r]*\n\s*", text.strip()):
        pieces = _sentences(re.sub(r"\s+", " ", para).strip())
        pieces = [q for p in pieces for q in (_cut(p, max_tokens, count) if count(p) > max_tokens else [p])]
        if len(pieces) == 1 and not has_word(pieces[0]) and segs:  # a paragraph without a word: behind the paragraph in front of it
            segs[-1].text += " " + pieces[0]
            continue
        for k, p in enumerate(pieces):
            segs.append(Segment(p, kind="paragraph-end" if k == len(pieces) - 1 else "sentence"))
    return [s for s in segs if s.text]


def frames(seconds, rate, hop):
    """seconds -> frames of `hop` samples at `rate` Hz: floor(sec * rate / hop + 0.5)"""
    sec = float(seconds)
    if not (math.isfinite(sec) and sec >= 0.0):
        raise ValueError(f"a pause of {seconds} s: a finite number of seconds, not negative")
    return int(math.floor(sec * rate / hop + 0.5))


def gap_frames(segments, sentence_pause, paragraph_pause, rate, hop):
    """the silence behind every segment in frames: its own pause_after, else the call's pause for its kind"""
    return np.array([frames(s.pause_after if s.pause_after is not None else paragraph_pause if s.kind == "paragraph-end" else sentence_pause,
                            rate, hop) for s in segments], np.int32)


def stitch_marks(rate, token_ends, lengths, layouts, seg_start, seg_end):
    """The marks of a document: token_ends int64 [B, T_x] on the document's time axis, lengths [B] tokens per segment, layouts [B] of
    Synth.marks_layout, seg_start / seg_end [B] -> SpeechMarks whose phonemes and words run over the whole document, with
    .segments = [(start, end)] and .word_segment = the segment of every word.  The first token of a segment starts where the segment
    starts (not at the end of the segment in front of it: the gap belongs to nobody)."""
    from .marks import SpeechMarks, build_marks

    phonemes, words, owner, ends = [], [], [], []
    for b, lay in enumerate(layouts):
        s0 = int(seg_start[b])
        e = np.asarray(token_ends[b][:int(lengths[b])], np.int64)
        sm = build_marks(rate, e - s0, *lay)
        phonemes += [(s, a + s0, z + s0) for s, a, z in sm.phonemes]
        words += [(t, a + s0, z + s0) for t, a, z in sm.words]
        owner += [b] * len(sm.words)
        ends.append(e)
    out = SpeechMarks(rate, np.concatenate(ends) if ends else np.zeros(0, np.int64), phonemes, words)
    out.segments = [(int(a), int(z)) for a, z in zip(seg_start, seg_end)]
    out.word_segment = owner
    return out
