"""An SSML front end for Synth: the subset of the markup whose every attribute maps onto something the engine runs
(include/vits_prosody.h, include/vits_contour.h, include/vits_marks.h).  Parsed with xml.etree.ElementTree; no device, no model.

    <speak>, <p>, <s>          transparent
    <sub alias="...">          its text is replaced by the alias
    <break time="250ms|0.25s"/> a pause behind the preceding word (`pauses`); in front of the first word it is a ValueError
    <prosody rate= pitch= volume=>   nested elements compose: rates multiply, semitones and decibels add
        rate    N%  (100% = unchanged)               or  x-slow 0.5, slow 0.75, medium 1.0, fast 1.5, x-fast 2.0
        pitch   +Nst / -Nst, +N% / -N% (12 log2(1 + N / 100) semitones)  or  x-low -6, low -3, medium 0, high +3, x-high +6 semitones
        volume  +NdB / -NdB                          or  x-soft -12, soft -6, medium 0, loud +6, x-loud +12 dB
        range   N% / +N% / -N% (100% = +0% = unchanged)  or  x-low 0.25, low 0.5, medium / default 1, high 1.5, x-high 2: the intonation
                range of include/vits_intonation.h, one value per utterance -- accepted only on a prosody element that covers every
                word of the document (`pitch_range` of the plan); a range for some of the words is a ValueError
    <mark name="..."/>         with marks=True, marks.named[name] = the start sample of the next word, or the end of the audio

Anything else is a ValueError that names it, raised before a model is touched: another element, an unknown attribute, a tag that starts
or ends inside a word, malformed XML.  Words are counted as the speech marks count them (marks.vits_layout).
"""
import math
import re
import xml.etree.ElementTree as ET

from .capi import CONTOUR_DB, INTONATION_MAX_RANGE, PITCH_MAX_SEMITONES, PROSODY_MAX_TOKEN_SCALE
from .marks import _SPLIT

RATE_LABELS = {"x-slow": 0.5, "slow": 0.75, "medium": 1.0, "fast": 1.5, "x-fast": 2.0}
PITCH_LABELS = {"x-low": -6.0, "low": -3.0, "medium": 0.0, "high": 3.0, "x-high": 6.0}
VOLUME_LABELS = {"x-soft": -12.0, "soft": -6.0, "medium": 0.0, "loud": 6.0, "x-loud": 12.0}
RANGE_LABELS = {"x-low": 0.25, "low": 0.5, "medium": 1.0, "high": 1.5, "x-high": 2.0, "default": 1.0}

_NUM = r"[0-9]+(?:\.[0-9]*)?|\.[0-9]+"
_XML_LANG = "{http://www.w3.org/XML/1998/namespace}lang"
_ATTRS = {"speak": {"version", _XML_LANG}, "p": {_XML_LANG}, "s": {_XML_LANG}, "sub": {"alias"}, "break": {"time"},
          "prosody": {"rate", "pitch", "volume", "range"}, "mark": {"name"}}


class Plan:
    """What a document asks for: text, word_rates {word: rate}, pauses {word: seconds}, word_pitch {word: semitones}, word_gains
    {word: dB}, pitch_range (the keywords of Synth.synth_audio; empty ones are None) and marks [(name, index of the next word)]."""

    def __init__(self, text, word_rates, pauses, word_pitch, word_gains, marks, pitch_range=None):
        self.text, self.word_rates, self.pauses, self.word_pitch, self.word_gains, self.marks = text, word_rates, pauses, word_pitch, word_gains, marks
        self.pitch_range = pitch_range

    def keywords(self):
        kw = {k: v for k, v in (("word_rates", self.word_rates), ("pauses", self.pauses), ("word_pitch", self.word_pitch),
                                ("word_gains", self.word_gains)) if v}
        if self.pitch_range is not None:
            kw["pitch_range"] = self.pitch_range
        return kw


def count_words(text):
    return sum(1 for piece in re.split(_SPLIT, text.lower()) if piece != "" and piece != "-" and not re.match(_SPLIT, piece))


def _is_sep(ch):
    return re.match(_SPLIT, ch) is not None


def parse_rate(v):
    v = v.strip()
    if v in RATE_LABELS:
        return RATE_LABELS[v]
    m = re.fullmatch(rf"({_NUM})%", v)
    if not m or float(m.group(1)) <= 0:
        raise ValueError(f"prosody rate={v!r}: a positive percentage such as '80%' or one of {', '.join(RATE_LABELS)}")
    return float(m.group(1)) / 100.0


def parse_pitch(v):
    v = v.strip()
    if v in PITCH_LABELS:
        return PITCH_LABELS[v]
    m = re.fullmatch(rf"([+-])({_NUM})(st|%)", v)
    if not m:
        raise ValueError(f"prosody pitch={v!r}: '+2st', '-10%' or one of {', '.join(PITCH_LABELS)}")
    x = float(m.group(2)) * (1.0 if m.group(1) == "+" else -1.0)
    if m.group(3) == "st":
        return x
    if x <= -100.0:
        raise ValueError(f"prosody pitch={v!r}: a change of -100% or more has no pitch")
    return 12.0 * math.log2(1.0 + x / 100.0)


def parse_volume(v):
    v = v.strip()
    if v in VOLUME_LABELS:
        return VOLUME_LABELS[v]
    m = re.fullmatch(rf"([+-])({_NUM})dB", v)
    if not m:
        raise ValueError(f"prosody volume={v!r}: '+6dB', '-3dB' or one of {', '.join(VOLUME_LABELS)}")
    return float(m.group(2)) * (1.0 if m.group(1) == "+" else -1.0)


def parse_range(v):
    v = v.strip()
    if v in RANGE_LABELS:
        return RANGE_LABELS[v]
    m = re.fullmatch(rf"([+-]?)({_NUM})%", v)
    if not m:
        raise ValueError(f"prosody range={v!r}: '50%', '+20%' or one of {', '.join(RANGE_LABELS)}")
    x = float(m.group(2))
    r = x / 100.0 if m.group(1) == "" else 1.0 + x / 100.0 if m.group(1) == "+" else 1.0 - x / 100.0
    if not 0.0 <= r <= INTONATION_MAX_RANGE:
        raise ValueError(f"prosody range={v!r}: {r:g} times the voice's own range is outside [0, {INTONATION_MAX_RANGE:g}]")
    return r


def parse_time(v):
    m = re.fullmatch(rf"({_NUM})(ms|s)", v.strip())
    if not m:
        raise ValueError(f"break time={v!r}: a duration such as '250ms' or '0.25s'")
    return float(m.group(1)) / (1000.0 if m.group(2) == "ms" else 1.0)


def _local(tag):
    return tag.rsplit("}", 1)[-1] if isinstance(tag, str) else str(tag)


def parse(ssml):
    """SSML text -> Plan; ValueError names whatever is refused"""
    try:
        root = ET.fromstring(ssml)
    except ET.ParseError as e:
        raise ValueError(f"malformed SSML: {e}") from None
    if _local(root.tag) != "speak":
        raise ValueError(f"the root element must be <speak>, not <{_local(root.tag)}>")
    text = []        # the pieces of the spoken text
    runs = []        # (start, end, rate, semitones, dB) per piece under a prosody element
    edges = []       # (position in the text, tag) of every tag boundary
    breaks, marks = [], []
    ranges = []      # (start, end, r, raw value) of every prosody element with a range

    def pos():
        return sum(len(t) for t in text)

    def say(chunk, ctx):
        chunk = re.sub(r"\s+", " ", chunk or "")
        so_far = "".join(text)
        if chunk.startswith(" ") and (so_far == "" or so_far.endswith(" ")):
            chunk = chunk[1:]
        if not chunk:
            return
        a = pos()
        text.append(chunk)
        if ctx != (1.0, 0.0, 0.0):
            runs.append((a, a + len(chunk)) + ctx)

    def walk(el, ctx):
        tag = _local(el.tag)
        if tag not in _ATTRS:
            raise ValueError(f"SSML element <{tag}> is not supported (speak, p, s, sub, break, prosody, mark)")
        for k in el.attrib:
            if k not in _ATTRS[tag]:
                raise ValueError(f"<{tag}> has no attribute {_local(k)!r} here ({', '.join(sorted(_local(a) for a in _ATTRS[tag])) or 'none'})")
        if el is not root:
            edges.append((pos(), tag))
        if tag in ("break", "mark", "sub") and len(el):
            raise ValueError(f"<{tag}> cannot contain <{_local(el[0].tag)}>")
        if tag == "break":
            if (el.text or "").strip():
                raise ValueError("<break> cannot contain text")
            breaks.append((pos(), parse_time(el.attrib.get("time", "250ms"))))
        elif tag == "mark":
            if "name" not in el.attrib:
                raise ValueError("<mark> needs a name")
            marks.append((el.attrib["name"], pos()))
        elif tag == "sub":
            if "alias" not in el.attrib:
                raise ValueError("<sub> needs an alias")
            say(el.attrib["alias"], ctx)
        else:
            if tag == "prosody":
                r, s, g = ctx
                if "rate" in el.attrib:
                    r *= parse_rate(el.attrib["rate"])
                if "pitch" in el.attrib:
                    s += parse_pitch(el.attrib["pitch"])
                if "volume" in el.attrib:
                    g += parse_volume(el.attrib["volume"])
                ctx = (r, s, g)
            a0 = pos()
            say(el.text, ctx)
            for child in el:
                walk(child, ctx)
                say(child.tail, ctx)
            if tag == "prosody" and "range" in el.attrib:
                ranges.append((a0, pos(), parse_range(el.attrib["range"]), el.attrib["range"]))
        if el is not root:
            edges.append((pos(), tag))

    walk(root, (1.0, 0.0, 0.0))
    full = "".join(text)
    for p, tag in edges:
        if 0 < p < len(full) and not _is_sep(full[p - 1]) and not _is_sep(full[p]):
            raise ValueError(f"<{tag}> starts or ends inside the word {full[:p].split(' ')[-1] + full[p:].split(' ')[0]!r}")
    words_before = lambda p: count_words(full[:p])
    word_rates, word_pitch, word_gains, pauses = {}, {}, {}, {}
    for a, b, r, s, g in runs:
        for w in range(words_before(a), words_before(b)):
            if r != 1.0:
                if not (math.isfinite(r) and r > 0.0 and 1.0 / r <= PROSODY_MAX_TOKEN_SCALE):
                    raise ValueError(f"prosody rate of word {w} composes to {r:g}: at least {1.0 / PROSODY_MAX_TOKEN_SCALE:g}")
                word_rates[w] = r
            if s != 0.0:
                if not abs(s) <= PITCH_MAX_SEMITONES:
                    raise ValueError(f"prosody pitch of word {w} composes to {s:g} semitones: outside [-{PITCH_MAX_SEMITONES:g}, {PITCH_MAX_SEMITONES:g}]")
                word_pitch[w] = s
            if g != 0.0:
                if not CONTOUR_DB[0] <= g <= CONTOUR_DB[1]:
                    raise ValueError(f"prosody volume of word {w} composes to {g:g} dB: outside [{CONTOUR_DB[0]:g}, {CONTOUR_DB[1]:g}]")
                word_gains[w] = g
    pitch_range = None
    for a, b, r, raw in ranges:  # one intonation range per utterance: the element must hold every word
        if words_before(a) != 0 or words_before(b) != count_words(full):
            raise ValueError(f"prosody range={raw!r} covers words {words_before(a)} to {words_before(b) - 1} of {count_words(full)}: the "
                             "intonation range is one value per utterance, so `range` is accepted only on a prosody element around every word")
        pitch_range = r if pitch_range is None else pitch_range * r
        if not 0.0 <= pitch_range <= INTONATION_MAX_RANGE:
            raise ValueError(f"prosody range composes to {pitch_range:g}: outside [0, {INTONATION_MAX_RANGE:g}]")
    for p, sec in breaks:
        w = words_before(p) - 1
        if w < 0:
            raise ValueError("<break> in front of the first word: a pause follows a word")
        pauses[w] = pauses.get(w, 0.0) + sec
    return Plan(full.strip(), word_rates or None, pauses or None, word_pitch or None, word_gains or None,
                [(name, words_before(p)) for name, p in marks], pitch_range)
