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


def _root(ssml):
    try:
        root = ET.fromstring(ssml)
    except ET.ParseError as e:
        raise ValueError(f"malformed SSML: {e}") from None
    if _local(root.tag) != "speak":
        raise ValueError(f"the root element must be <speak>, not <{_local(root.tag)}>")
    return root


def parse(ssml):
    """SSML text -> Plan; ValueError names whatever is refused"""
    return _plan(_root(ssml))


def _plan(root):
    """the Plan of one <speak> tree"""
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


# ---- documents (include/vits_document.h; Synth.synth_document_ssml) ---------------------------------------------------------------------
_DOC_ATTRS = dict(_ATTRS, voice={"name", _XML_LANG})


class DocumentPlan:
    """What an SSML document asks of Synth.synth_document: segments [document.Segment], lead (seconds of silence in front, from a <break>
    ahead of the first word), pitch_range (from a prosody `range` around every word, else None) and marks [(name, index of the next word,
    counted over the whole document)]."""

    def __init__(self, segments, lead, pitch_range, marks):
        self.segments, self.lead, self.pitch_range, self.marks = segments, lead, pitch_range, marks


def parse_document(ssml):
    """SSML text -> DocumentPlan.  On top of parse()'s subset: <s>, <p> and <voice name="N"> (N an integer speaker id) end a segment, both
    where they open and where they close; the segment in front of a </p> is a paragraph's last.  A <break> with no word between it and
    a segment boundary becomes the silence at that boundary (in front of the first segment: the lead) in place of the default pause;
    anywhere else it stays a pause behind its word.  prosody, sub and mark work as in parse(), per segment: a prosody element that spans
    several segments applies to each.  `range` is accepted on a prosody element around every word of the document only.  Anything else
    is a ValueError that names it."""
    from .document import Segment

    root = _root(ssml)
    events = []  # ("text", str) | ("open", attrib) | ("close",) | ("leaf", element) | ("bound", tag, opening?, speaker or None)

    def walk(el):
        tag = _local(el.tag)
        if tag not in _DOC_ATTRS:
            raise ValueError(f"SSML element <{tag}> is not supported in a document (speak, p, s, voice, sub, break, prosody, mark)")
        for k in el.attrib:
            if k not in _DOC_ATTRS[tag]:
                raise ValueError(f"<{tag}> has no attribute {_local(k)!r} here ({', '.join(sorted(_local(a) for a in _DOC_ATTRS[tag])) or 'none'})")
        if tag in ("break", "mark", "sub"):
            if len(el):
                raise ValueError(f"<{tag}> cannot contain <{_local(el[0].tag)}>")
            if tag == "break":
                if (el.text or "").strip():
                    raise ValueError("<break> cannot contain text")
                parse_time(el.attrib.get("time", "250ms"))
            if tag == "mark" and "name" not in el.attrib:
                raise ValueError("<mark> needs a name")
            if tag == "sub" and "alias" not in el.attrib:
                raise ValueError("<sub> needs an alias")
            events.append(("leaf", el))
            return
        sid = None
        if tag == "voice":
            name = el.attrib.get("name", "").strip()
            if not re.fullmatch(r"[0-9]+", name):
                raise ValueError(f"<voice name={el.attrib.get('name')!r}>: the name is an integer speaker id of the voice, such as '1'")
            sid = int(name)
        if tag in ("p", "s", "voice"):
            events.append(("bound", tag, True, sid))
        elif tag == "prosody":
            events.append(("open", dict(el.attrib)))
        events.append(("text", el.text or ""))
        for child in el:
            walk(child)
            events.append(("text", child.tail or ""))
        if tag in ("p", "s", "voice"):
            events.append(("bound", tag, False, sid))
        elif tag == "prosody":
            events.append(("close",))

    walk(root)
    segments, marks, ranges = [], [], []
    state = {"lead": 0.0, "words": 0}
    voices, open_pros = [None], []     # the speakers and the prosody attributes in effect
    pending, pending_pros = [], []     # the events of the segment being collected, and the prosody stack where it began

    def words_in(evs):
        return count_words(re.sub(r"\s+", " ", " ".join(e[1] if e[0] == "text" else e[1].attrib["alias"] for e in evs
                                                        if e[0] == "text" or (e[0] == "leaf" and _local(e[1].tag) == "sub"))))

    def boundary_pause(sec):
        if segments:
            segments[-1].pause_after = (segments[-1].pause_after or 0.0) + sec
        else:
            state["lead"] += sec

    def finish(kind):
        evs = list(pending)
        del pending[:]
        spoken = [i for i, e in enumerate(evs) if words_in([e])]
        is_break = lambda e: e[0] == "leaf" and _local(e[1].tag) == "break"
        if not spoken:  # no word: its breaks belong to the boundary, its punctuation to nobody
            for e in evs:
                if is_break(e):
                    boundary_pause(parse_time(e[1].attrib.get("time", "250ms")))
            return
        after = None
        keep = []
        for i, e in enumerate(evs):
            if is_break(e) and (i < spoken[0] or i > spoken[-1]):
                sec = parse_time(e[1].attrib.get("time", "250ms"))
                if i < spoken[0]:
                    boundary_pause(sec)
                else:
                    after = (after or 0.0) + sec
            else:
                keep.append(e)
        seg_root = ET.Element("speak")
        stack = [seg_root]
        for attrib in pending_pros:
            stack.append(ET.SubElement(stack[-1], "prosody", attrib))
        for e in keep:
            if e[0] == "text":
                top = stack[-1]
                if len(top):
                    top[-1].tail = (top[-1].tail or "") + e[1]
                else:
                    top.text = (top.text or "") + e[1]
            elif e[0] == "open":
                stack.append(ET.SubElement(stack[-1], "prosody", e[1]))
            elif e[0] == "close":
                stack.pop()
            else:
                leaf = ET.SubElement(stack[-1], e[1].tag, dict(e[1].attrib))
                leaf.text = e[1].text
        plan = _plan(seg_root)
        segments.append(Segment(plan.text, speaker_id=voices[-1], pause_after=after, word_rates=plan.word_rates, pauses=plan.pauses,
                                word_pitch=plan.word_pitch, word_gains=plan.word_gains, kind=kind))
        state["words"] += count_words(plan.text)

    range_open = []
    for e in events:
        if e[0] == "bound":
            _, tag, opening, sid = e
            had = bool(pending) and words_in(pending) > 0
            finish("paragraph-end" if (tag == "p" and not opening) else "sentence")
            if tag == "p" and not opening and not had and segments:
                segments[-1].kind = "paragraph-end"
            if tag == "voice":
                voices.append(sid) if opening else voices.pop()
            pending_pros[:] = [dict(a) for a in open_pros]
            continue
        if e[0] == "leaf" and _local(e[1].tag) == "mark":
            marks.append((e[1].attrib["name"], state["words"] + words_in(pending)))
            continue
        if e[0] == "open":
            attrib = dict(e[1])
            if "range" in attrib:
                range_open.append((state["words"] + words_in(pending), parse_range(attrib["range"]), attrib.pop("range")))
            else:
                range_open.append(None)
            open_pros.append(attrib)
            e = ("open", attrib)
        elif e[0] == "close":
            open_pros.pop()
            r = range_open.pop()
            if r is not None:
                ranges.append((r[0], state["words"] + words_in(pending), r[1], r[2]))
        if not pending:
            pending_pros[:] = [dict(a) for a in (open_pros[:-1] if e[0] == "open" else open_pros + [{}] if e[0] == "close" else open_pros)]
        pending.append(e)
    finish("paragraph-end")
    if not segments:
        raise ValueError("the document has no word")
    segments[-1].kind = "paragraph-end"  # (the end of the document ends a paragraph)
    total = state["words"]
    pitch_range = None
    for a, b, r, raw in ranges:
        if a != 0 or b != total:
            raise ValueError(f"prosody range={raw!r} covers words {a} to {b - 1} of {total}: the intonation range is one value per call, so "
                             "`range` is accepted only on a prosody element around every word of the document")
        pitch_range = r if pitch_range is None else pitch_range * r
        if not 0.0 <= pitch_range <= INTONATION_MAX_RANGE:
            raise ValueError(f"prosody range composes to {pitch_range:g}: outside [0, {INTONATION_MAX_RANGE:g}]")
    return DocumentPlan(segments, state["lead"], pitch_range, marks)
