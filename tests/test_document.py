"""Documents (include/vits_document.h) without a device: the restatement (tests/document_ref.py) against hand-written cases, the
splitter's documented rule, ssml.parse_document, Synth.synth_document with a stub in place of the session, and the ctypes mirrors
against the header."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import document_ref as R
from vosk_tts_amd import document as D
from vosk_tts_amd import ssml as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 4


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _frames(*peaks):
    """one item whose frame f is HOP samples with the largest magnitude peaks[f] (at an odd place, negative)"""
    x = np.zeros(len(peaks) * HOP, np.float32)
    for f, p in enumerate(peaks):
        x[f * HOP + 1] = -np.float32(p)
        x[f * HOP + 2] = np.float32(p) / 2
    return x


def test_a_peak_exactly_at_the_threshold_is_not_loud():
    thr = R.threshold(-20.0)
    assert thr == np.float32(10.0 ** -1.0) and thr.dtype == np.float32
    above = np.nextafter(thr, np.float32(1))
    assert R.trim_item(_frames(thr, above, thr), 3, HOP, thr, 0) == (1, 2)
    assert R.trim_item(_frames(thr, thr, thr), 3, HOP, thr, 0) == (0, 0)
    assert R.trim_item(_frames(thr, thr), 2, HOP, None, 0) == (0, 2)  # off
    assert R.threshold(None) is None and R.threshold(0) is None


def test_an_all_quiet_item_is_empty_and_keeps_its_gap():
    rows = [_frames(0.5, 0.5), _frames(0.01, 0.01, 0.01), _frames(0.5)]
    j = R.join(rows, [2, 3, 1], HOP, lead=1, gaps=[2, 3, 1], trim_db=-20.0)
    assert j["lo"] == [0, 0, 0] and j["hi"] == [2, 0, 1] and j["n"] == [2, 0, 1]
    assert j["start"] == [1, 5, 8] and j["F"] == 10  # 1 + (2 + 2) + (0 + 3) + (1 + 1)
    y = j["y"].reshape(-1, HOP)
    assert not y[0].any() and np.array_equal(y[1:3].reshape(-1), rows[0]) and not y[3:8].any()
    assert np.array_equal(y[8], rows[2]) and not y[9].any()


def test_keep_is_clamped_at_both_ends():
    x = _frames(0.01, 0.01, 0.5, 0.01, 0.5, 0.01)
    thr = R.threshold(-20.0)
    assert R.trim_item(x, 6, HOP, thr, 0) == (2, 5)  # a quiet frame between loud ones stays
    assert R.trim_item(x, 6, HOP, thr, 1) == (1, 6)
    assert R.trim_item(x, 6, HOP, thr, 2) == (0, 6)
    assert R.trim_item(x, 6, HOP, thr, 100) == (0, 6)


def test_fades_are_one_multiply_and_fade_zero_is_a_copy():
    rng = np.random.default_rng(1)
    rows = [rng.standard_normal(3 * 8).astype(np.float32), rng.standard_normal(8).astype(np.float32)]
    j0 = R.join(rows, [3, 1], 8, gaps=[1, 0])
    assert j0["y"].tobytes() == np.concatenate([rows[0], np.zeros(8, np.float32), rows[1]]).tobytes()
    w = R.fade_table(4)
    assert w.dtype == np.float32 and np.all(np.diff(w) > 0) and 0 < w[0] and w[-1] < 1
    assert w[1] == np.float32(0.5 - 0.5 * np.cos(np.pi * 1.5 / 4))
    j = R.join(rows, [3, 1], 8, gaps=[1, 0], fade=4)
    seg = j["y"][32:40]  # the one-frame segment: head and tail fades meet at hop / 2 and do not overlap
    assert seg[:4].tobytes() == (rows[1][:4] * w).tobytes() and seg[4:].tobytes() == (rows[1][4:] * w[::-1]).tobytes()
    assert j["y"][4:20].tobytes() == rows[0][4:20].tobytes()


def test_marks_follow_the_layout():
    lay = {"start": [2, 9], "lo": [1, 0], "n": [3, 2], "F": 12}
    cum = np.array([[1, 2, 6, 6], [1, 2, 2, 2]])
    s0, s1, ends, total = R.marks(lay, cum, [3, 2], 256)
    assert s0 == [512, 9 * 256] and s1 == [5 * 256, 11 * 256] and total == 12 * 256
    # cum - lo clamped to [0, n]: frame counts 1, 2, 6 of a segment trimmed to [1, 4) become 0, 1, 3
    assert ends.tolist() == [[512, 768, 1280, 1280], [2560, 2816, 2816, 2816]]
    s0, s1, ends, total = R.marks(lay, cum, [3, 2], 256, 22050, 8000)
    assert s0[0] == -(-512 * 160 // 441) and total == -(-12 * 256 * 160 // 441)
    assert R.frames(0.2, 22050, 256) == 17 and R.frames(0.6, 22050, 256) == 52 and D.frames(0.2, 22050, 256) == 17


# ---- the splitter ----------------------------------------------------------------------------------------------------------------------
def _texts(segs):
    return [(s.text, s.kind) for s in segs]


def test_split_follows_the_documented_rule():
    # abbreviations are not recognised: the rule, not a goal
    assert _texts(D.split("Dr. Smith came. He left!")) == [("Dr.", "sentence"), ("Smith came.", "sentence"), ("He left!", "paragraph-end")]
    # closing quotes and brackets stay with their sentence; no white space behind the mark, no end
    assert _texts(D.split('He said "go." (Really?) Version 2.5 is out…')) == [
        ('He said "go."', "sentence"), ("(Really?)", "sentence"), ("Version 2.5 is out…", "paragraph-end")]
    # a blank line ends a paragraph; a single newline does not
    assert _texts(D.split("one.\ntwo.\n\n  \nthree")) == [("one.", "sentence"), ("two.", "paragraph-end"), ("three", "paragraph-end")]


def test_split_merges_pieces_without_a_word():
    assert _texts(D.split("... Hello. !!! World. ?")) == [("... Hello. !!!", "sentence"), ("World. ?", "paragraph-end")]
    assert _texts(D.split("Hello.\n\n - \n\nWorld.")) == [("Hello. -", "paragraph-end"), ("World.", "paragraph-end")]
    assert _texts(D.split("?!")) == [("?!", "paragraph-end")]  # nothing to merge into: the caller's refusal, not the splitter's


def test_split_cuts_an_over_long_sentence_at_the_last_clause_mark_that_fits():
    count = lambda t: len(t.split())  # a front end that makes one token per word
    s = "a b c, d e f; g h: i j k l m n o"
    assert _texts(D.split(s, 6, count)) == [("a b c, d e f;", "sentence"), ("g h:", "sentence"), ("i j k l m n", "sentence"), ("o", "paragraph-end")]
    assert _texts(D.split(s, 100, count)) == [(s, "paragraph-end")]
    assert _texts(D.split("a b — c d", 3, count)) == [("a b —", "sentence"), ("c d", "paragraph-end")]
    assert [t for t, _ in _texts(D.split("abcdefgh", 3))] == ["abc", "def", "gh"]  # (characters: one word longer than the limit)
    with pytest.raises(ValueError, match="max_tokens 0"):
        D.split("a", 0)


# ---- SSML ------------------------------------------------------------------------------------------------------------------------------
def test_parse_document_segments_speakers_and_gaps():
    p = S.parse_document('<speak><break time="300ms"/><p><s>Hello there.</s><break time="1s"/><s>How <prosody pitch="+2st">are you</prosody>?</s></p>'
                         '<voice name="1"><s>I am<break time="200ms"/> fine.</s></voice> <mark name="m"/><voice name="2">bye</voice></speak>')
    assert [(s.text, s.kind, s.speaker_id, s.pause_after) for s in p.segments] == [
        ("Hello there.", "sentence", None, 1.0), ("How are you?", "paragraph-end", None, None), ("I am fine.", "sentence", 1, None),
        ("bye", "paragraph-end", 2, None)]
    assert p.lead == pytest.approx(0.3) and p.pitch_range is None and p.marks == [("m", 8)]
    assert p.segments[1].word_pitch == {1: 2.0, 2: 2.0} and p.segments[0].word_pitch is None
    assert p.segments[2].pauses == {1: 0.2}  # a break inside a segment stays a pause behind its word


def test_parse_document_prosody_applies_per_segment_and_range_around_everything():
    p = S.parse_document('<speak><prosody range="high" rate="fast"><s>one <prosody rate="50%" volume="+3dB">two</prosody></s><s>three</s></prosody></speak>')
    assert [s.text for s in p.segments] == ["one two", "three"] and p.pitch_range == 1.5
    assert p.segments[0].word_rates == {0: 1.5, 1: 0.75} and p.segments[0].word_gains == {1: 3.0} and p.segments[1].word_rates == {0: 1.5}
    with pytest.raises(ValueError, match="range='low' covers words 0 to 0 of 2"):
        S.parse_document('<speak><s><prosody range="low">a</prosody></s><s>b</s></speak>')


@pytest.mark.parametrize("doc, match", [
    ("<speak><emphasis>a</emphasis></speak>", "<emphasis> is not supported in a document"),
    ("<speak><voice name='bob'>a</voice></speak>", "<voice name='bob'>: the name is an integer speaker id"),
    ("<speak><voice>a</voice></speak>", "integer speaker id"),
    ("<speak><voice name='1' age='3'>a</voice></speak>", "no attribute 'age'"),
    ("<speak><s>a <break time='soon'/> b</s></speak>", "break time='soon'"),
    ("<speak><s> , </s></speak>", "the document has no word"),
    ("<talk>a</talk>", "root element must be <speak>"),
])
def test_parse_document_refusals_name_their_cause(doc, match):
    with pytest.raises(ValueError, match=match):
        S.parse_document(doc)


def test_parse_still_refuses_voice_and_keeps_s_and_p_transparent():
    with pytest.raises(ValueError, match="<voice> is not supported"):
        S.parse("<speak><voice name='1'>a</voice></speak>")
    assert S.parse("<speak><p><s>one two</s> <s>three</s></p></speak>").text == "one two three"


# ---- Synth.synth_document with a stub session -------------------------------------------------------------------------------------------
class _Session:
    """records the feed; answers as run_document does: every token 256 samples long, segments laid out by the feed's own gaps"""

    def __init__(self):
        self.feeds = []

    def run_document(self, feed, scale=1.0, pcm16=True):
        self.feeds.append((dict(feed), scale, pcm16))
        lens, gaps = feed["input_lengths"], feed["vits.doc_gap_frames"]
        at = int(feed["vits.doc_lead_frames"]) * 256
        B, T = feed["input"].shape
        info = {"seg_start": np.zeros(B, np.int64), "seg_end": np.zeros(B, np.int64), "trim": np.zeros((B, 2), np.int32)}
        ends = np.zeros((B, T), np.int64)
        for b in range(B):
            info["seg_start"][b] = at
            ends[b] = at + 256 * np.minimum(np.arange(1, T + 1), lens[b])
            at += 256 * int(lens[b])
            info["seg_end"][b] = at
            at += 256 * int(gaps[b])
        if feed.get("vits.marks"):
            info["token_ends"] = ends
        return np.zeros(at, np.int16), info


def _synth():
    from vosk_tts_amd.synth import Synth

    ids = {p: i + 1 for i, p in enumerate("^$ .,!?abcdefghijklmnopqrstuvwxyz-")}
    s = Synth.__new__(Synth)
    sess = _Session()
    s.model = type("M", (), {"config": {"model_type": "vits", "inference": {}, "phoneme_id_map": ids}, "tokenizer": None,
                             "dic": {w: " ".join(w) for w in ("hello", "there", "how", "are", "you", "fine", "bye")}, "onnx": sess})()
    return s, sess


def test_synth_document_builds_one_feed():
    s, sess = _synth()
    audio = s.synth_document("Hello there. How are you?\n\nFine.", speaker_id=3, seed=7, fade_ms=1.0, trim_db=-50.0, loudness=-19.0)
    feed, scale, pcm16 = sess.feeds[0]
    assert len(sess.feeds) == 1 and pcm16 and scale == 1.0 and audio.dtype == np.int16
    lens = [len(s.g2p_noembed(t)) for t in ("hello there.", "how are you?", "fine.")]
    assert feed["input"].shape == (3, max(lens)) and feed["input_lengths"].tolist() == lens and feed["sid"].tolist() == [3, 3, 3]
    assert feed["input"][2, :lens[2]].tolist() == s.g2p_noembed("fine.") and not feed["input"][2, lens[2]:].any()
    # seconds -> frames: floor(sec * 22050 / 256 + 0.5); sentence 0.2 s, paragraph 0.6 s, the last segment ends a paragraph
    assert feed["vits.doc_gap_frames"].tolist() == [17, 52, 52] and feed["vits.doc_gap_frames"].dtype == np.int32
    assert feed["vits.doc_lead_frames"] == 0 and feed["vits.doc_fade_samples"] == 22 and feed["vits.doc_trim_db"] == -50.0
    assert feed["vits.doc_trim_keep"] == 1 and feed["vits.seed"] == 7 and feed["vits.loudness"] == -19.0 and "vits.marks" not in feed
    assert not any(k in feed for k in ("vits.item_scales", "vits.token_pause", "vits.token_pitch", "vits.solo"))
    assert audio.shape == ((sum(lens) + 17 + 52 + 52) * 256,)


def test_synth_document_segments_carry_their_own_controls():
    s, sess = _synth()
    segs = [D.Segment("hello there", speaker_id=1, pause_after=0.0, word_pitch={1: 2.0}), D.Segment("how are you", speech_rate=2.0, pauses={0: 0.1}),
            D.Segment("bye", kind="paragraph-end")]
    s.synth_document(segs, speaker_id=5, lead=0.5, sentence_pause=0.3, paragraph_pause=1.0, speech_rate=1.0, noise_level=0.5)
    feed = sess.feeds[0][0]
    assert feed["sid"].tolist() == [1, 5, 5] and feed["vits.doc_gap_frames"].tolist() == [0, 26, 86] and feed["vits.doc_lead_frames"] == 43
    assert feed["vits.item_scales"].tolist() == [[0.5, 1.0, np.float32(0.8)], [0.5, 0.5, np.float32(0.8)], [0.5, 1.0, np.float32(0.8)]]
    tp, pause = feed["vits.token_pitch"], feed["vits.token_pause"]
    assert tp.shape == feed["input"].shape and tp[0].any() and not tp[1:].any() and set(np.unique(tp[0])) == {0.0, 2.0}
    assert pause[1].sum() == R.frames(0.1, 22050, 256) and not pause[0].any() and not pause[2].any()
    assert "vits.token_gain_db" not in feed and "vits.doc_trim_db" not in feed


def test_synth_document_refuses_the_per_utterance_keywords_by_name():
    s, sess = _synth()
    for k, v in (("word_rates", {0: 2.0}), ("pauses", {0: 1.0}), ("duration", 3.0), ("word_pitch", {0: 1.0}), ("word_gains", {0: 1.0})):
        with pytest.raises(ValueError, match=f"no {k}="):
            s.synth_document("hello there.", **{k: v})
    with pytest.raises(TypeError, match="unexpected keyword argument 'volume'"):
        s.synth_document("hello there.", volume=1)
    with pytest.raises(ValueError, match="fade_ms 10"):
        s.synth_document("hello there.", fade_ms=10.0)
    with pytest.raises(ValueError, match="trim_db 3"):
        s.synth_document("hello there.", trim_db=3.0)
    with pytest.raises(ValueError, match=r"segment 0 \('\?!'\) has no word"):
        s.synth_document("?!")
    with pytest.raises(ValueError, match="synth_stream cannot take document="):
        next(s.synth_stream("hello", document="hello there."))
    assert not sess.feeds
    assert "document" in inspect.signature(type(s).synth_stream).parameters


def test_synth_document_stitches_the_marks():
    s, sess = _synth()
    audio, sm = s.synth_document("Hello there. Bye.", marks=True, lead=0.1)
    feed = sess.feeds[0][0]
    assert feed["vits.marks"] is True
    lead = R.frames(0.1, 22050, 256) * 256
    n0 = len(s.g2p_noembed("hello there."))
    assert sm.segments == [(lead, lead + 256 * n0), (lead + 256 * (n0 + 17), audio.shape[0] - 52 * 256)]
    assert [w[0] for w in sm.words] == ["hello", "there", "bye"] and sm.word_segment == [0, 0, 1]
    # the first phoneme of a segment starts where the segment starts, and words stay inside their segment
    assert sm.phonemes[0][:2] == ("^", lead) and [p for p in sm.phonemes if p[0] == "^"][1][1] == sm.segments[1][0]
    assert all(sm.segments[b][0] <= a and z <= sm.segments[b][1] for (_, a, z), b in zip(sm.words, sm.word_segment))
    starts = [w[1] for w in sm.words]
    assert starts == sorted(starts) and sm.token_ends.shape == (n0 + len(s.g2p_noembed("bye.")),) and sm.rate == 22050


def test_synth_document_ssml_maps_the_plan():
    s, sess = _synth()
    audio, sm = s.synth_document_ssml('<speak><break time="100ms"/><prosody range="low"><s>hello there<break time="1s"/></s><mark name="x"/>'
                                      '<voice name="4">bye</voice></prosody></speak>', marks=True)
    feed = sess.feeds[0][0]
    assert feed["sid"].tolist() == [0, 4] and feed["vits.doc_gap_frames"].tolist() == [R.frames(1.0, 22050, 256), 52]
    assert feed["vits.doc_lead_frames"] == R.frames(0.1, 22050, 256) and feed["vits.pitch_range"] == 0.5
    assert sm.named == {"x": sm.words[2][1]} and sm.words[2][0] == "bye"
    with pytest.raises(ValueError, match="pitch_range from the document"):
        s.synth_document_ssml('<speak><prosody range="low">hello</prosody></speak>', pitch_range=2.0)


# ---- the C side ------------------------------------------------------------------------------------------------------------------------
def test_ctypes_mirror_matches_the_header(tmp_path, hip_lib):
    from vosk_tts_amd import capi
    from vosk_tts_amd.outopts import DOCUMENT_FEEDS

    fields = [n for n, _ in capi.Document._fields_]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vits_document.h"', 'int main(void) {',
             '  printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(vits_document), ' + ", ".join(f"offsetof(vits_document, {n})" for n in fields) + ');',
             '  return 0;', '}']
    src = tmp_path / "d.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "d"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert out == [ctypes.sizeof(capi.Document)] + [getattr(capi.Document, n).offset for n in fields]
    assert fields == ["lead_frames", "gap_frames", "fade_samples", "trim_db", "trim_keep_frames", "out_seg_start", "out_seg_end", "out_trim"]
    # the library exports the entry points with the binding's argument lists; the two ABI headers tied to the oracle do not name them
    assert hip_lib.has_document
    assert [len(hip_lib._fn(n).argtypes) for n in ("synthesize_document", "synthesize_document_pcm16", "op_document_join")] == [13, 14, 12]
    assert hasattr(hip_lib.lib, "stts_synthesize_document")
    for h in ("vits_mi355.h", "stts_mi355.h"):
        assert "document" not in open(os.path.join(ROOT, "include", h)).read()
    assert sorted(DOCUMENT_FEEDS) == ["vits.doc_fade_samples", "vits.doc_gap_frames", "vits.doc_lead_frames", "vits.doc_trim_db", "vits.doc_trim_keep"]
    d, keep, out = capi.document_struct(3, lead_frames=2, gap_frames=[1, 0, 4], fade_samples=5, trim_db=-40.0, trim_keep_frames=1)
    assert (d.lead_frames, d.fade_samples, d.trim_db, d.trim_keep_frames) == (2, 5, -40.0, 1) and [d.gap_frames[i] for i in range(3)] == [1, 0, 4]
    assert out["trim"].shape == (3, 2) and capi.document_struct(2, gap_frames=7)[1][0].tolist() == [7, 7]


def test_synth_documents_sends_every_document_whole_to_one_replica():
    import threading
    from concurrent.futures import ThreadPoolExecutor

    from vosk_tts_amd.batching import MultiDeviceSynth

    class _Replica:
        def __init__(self, r):
            self.r, self.calls = r, []

        normalize = staticmethod(lambda t: t.strip())
        phonemize = staticmethod(lambda t: list(t))

        def synth_document(self, doc, **kw):
            self.calls.append((doc, kw))
            return (self.r, doc if isinstance(doc, str) else [s.text for s in doc])

    mds = MultiDeviceSynth.__new__(MultiDeviceSynth)
    mds.devices, mds.synths = [0, 1], [_Replica(0), _Replica(1)]
    mds._replica_locks = [threading.Lock() for _ in mds.synths]
    mds._pool, mds._seed, mds._lock = ThreadPoolExecutor(max_workers=2), 0, threading.Lock()
    docs = ["short one. two.", "a much longer document. " * 6, [D.Segment("third"), D.Segment("document", speaker_id=1)]]
    out = mds.synth_documents(docs, seeds=[5, 6, 7], fade_ms=1.0)
    mds._pool.shutdown()
    # request order; the longest document alone on one replica, the two short ones together on the other (plan_shards by tokens)
    assert [o[1] for o in out] == [docs[0], docs[1], ["third", "document"]]
    assert out[1][0] != out[0][0] == out[2][0]
    calls = {c[0] if isinstance(c[0], str) else "segments": c[1] for s in mds.synths for c in s.calls}
    assert calls[docs[1]] == {"seed": 6, "fade_ms": 1.0} and calls["segments"]["seed"] == 7 and sum(len(s.calls) for s in mds.synths) == 3
    with pytest.raises(ValueError, match="one per document"):
        mds.synth_documents(docs, seeds=[1])
    assert mds.synth_documents([]) == []


def test_a_nan_sample_is_left_out_of_the_peak():
    x = _frames(0.01, 0.5, 0.01)
    x[0] = np.nan
    x[2 * HOP:] = np.nan  # a frame of NaNs has peak 0: never loud
    assert R.frame_peaks(x, 3, HOP).tolist() == [np.float32(0.01), 0.5, 0.0]
    assert R.trim_item(x, 3, HOP, R.threshold(-20.0), 0) == (1, 2)


def test_cut_asks_the_front_end_a_logarithmic_number_of_times():
    calls = []

    def count(t):
        calls.append(t)
        return len(t.split())

    s = " ".join(f"w{i}," for i in range(400))
    segs = D.split(s, 100, count)
    assert [len(x.text.split()) for x in segs] == [100, 100, 100, 100] and " ".join(x.text for x in segs) == s
    assert len(calls) < 4 * 16
