"""The SSML front end (vosk_tts_amd/ssml.py): every accepted form and label against the keywords it maps to, nesting, refusals by name,
and Synth.synth_ssml with a stub in place of the model.  No device."""
import math

import numpy as np
import pytest

from vosk_tts_amd import ssml as S


def test_transparent_elements_sub_and_text():
    p = S.parse('<speak version="1.1" xml:lang="ru"><p><s>one two</s> <s>three</s></p></speak>')
    assert p.text == "one two three" and p.keywords() == {} and p.marks == []
    p = S.parse('<speak>say <sub alias="forty five">45</sub> now</speak>')
    assert p.text == "say forty five now"
    p = S.parse("<speak>\n  a\n  b\n</speak>")
    assert p.text == "a b"
    assert S.count_words("ab, c - d") == 3


def test_the_issue_example_maps_to_its_keywords():
    p = S.parse('<speak>a <prosody pitch="+3st" volume="+6dB">b</prosody><break time="250ms"/> c</speak>')
    assert p.text == "a b c"
    assert p.keywords() == {"word_pitch": {1: 3.0}, "word_gains": {1: 6.0}, "pauses": {1: 0.25}}


def test_labels_are_the_documented_values():
    assert S.RATE_LABELS == {"x-slow": 0.5, "slow": 0.75, "medium": 1.0, "fast": 1.5, "x-fast": 2.0}
    assert S.PITCH_LABELS == {"x-low": -6.0, "low": -3.0, "medium": 0.0, "high": 3.0, "x-high": 6.0}
    assert S.VOLUME_LABELS == {"x-soft": -12.0, "soft": -6.0, "medium": 0.0, "loud": 6.0, "x-loud": 12.0}
    for table in (S.RATE_LABELS, S.PITCH_LABELS, S.VOLUME_LABELS):
        for label, v in table.items():
            assert f"{label} {v:g}" in S.__doc__ or f"{label} {v:+g}" in S.__doc__, (label, v)  # the docstring states the values
    for label, v in S.RATE_LABELS.items():
        kw = S.parse(f'<speak><prosody rate="{label}">w</prosody></speak>').keywords()
        assert kw == ({} if v == 1.0 else {"word_rates": {0: v}})
    for label, v in S.PITCH_LABELS.items():
        kw = S.parse(f'<speak><prosody pitch="{label}">w</prosody></speak>').keywords()
        assert kw == ({} if v == 0.0 else {"word_pitch": {0: v}})
    for label, v in S.VOLUME_LABELS.items():
        kw = S.parse(f'<speak><prosody volume="{label}">w</prosody></speak>').keywords()
        assert kw == ({} if v == 0.0 else {"word_gains": {0: v}})


def test_numeric_forms():
    assert S.parse_rate("80%") == 0.8 and S.parse_rate("150%") == 1.5
    assert S.parse_pitch("+2st") == 2.0 and S.parse_pitch("-1.5st") == -1.5
    assert S.parse_pitch("+100%") == pytest.approx(12.0) and S.parse_pitch("-50%") == pytest.approx(-12.0)
    assert S.parse_pitch("+10%") == pytest.approx(12 * math.log2(1.1))
    assert S.parse_volume("+6dB") == 6.0 and S.parse_volume("-3.5dB") == -3.5
    assert S.parse_time("250ms") == 0.25 and S.parse_time("0.25s") == 0.25 and S.parse_time("2s") == 2.0
    for fn, bad in ((S.parse_rate, "fastish"), (S.parse_rate, "0%"), (S.parse_rate, "+10%"), (S.parse_pitch, "3st"), (S.parse_pitch, "+3"),
                    (S.parse_pitch, "-100%"), (S.parse_volume, "6dB"), (S.parse_volume, "+6"), (S.parse_time, "250"), (S.parse_time, "-1s")):
        with pytest.raises(ValueError, match=bad.replace("+", r"\+")):
            fn(bad)


def test_nesting_composes_and_is_checked_against_the_ranges():
    p = S.parse('<speak>one <prosody rate="fast" pitch="+2st" volume="-3dB">two <prosody rate="50%" pitch="+3st" volume="-3dB">three</prosody> four'
                '</prosody></speak>')
    assert p.text == "one two three four"
    assert p.word_rates == {1: 1.5, 2: 0.75, 3: 1.5} and p.word_pitch == {1: 2.0, 2: 5.0, 3: 2.0} and p.word_gains == {1: -3.0, 2: -6.0, 3: -3.0}
    with pytest.raises(ValueError, match="pitch of word 0 composes to 14"):
        S.parse('<speak><prosody pitch="+7st"><prosody pitch="+7st">w</prosody></prosody></speak>')
    with pytest.raises(ValueError, match="volume of word 1 composes to 18 dB"):
        S.parse('<speak>a <prosody volume="x-loud"><prosody volume="+6dB">w</prosody></prosody></speak>')
    with pytest.raises(ValueError, match="rate of word 0"):
        S.parse('<speak><prosody rate="5%"><prosody rate="5%">w</prosody></prosody></speak>')


def test_breaks_and_marks():
    p = S.parse('<speak>a<break time="0.5s"/><break time="100ms"/> b c<break time="1s"/><mark name="end"/></speak>')
    assert p.text == "a b c" and p.pauses == {0: pytest.approx(0.6), 2: 1.0} and p.marks == [("end", 3)]
    p = S.parse('<speak><mark name="start"/>a <mark name="mid"/>b</speak>')
    assert p.marks == [("start", 0), ("mid", 1)]
    with pytest.raises(ValueError, match="in front of the first word"):
        S.parse('<speak><break time="1s"/>a</speak>')


@pytest.mark.parametrize("doc, match", [
    ("<speak>a", "malformed SSML"),
    ("<talk>a</talk>", "root element must be <speak>"),
    ("<speak><voice name='x'>a</voice></speak>", "<voice> is not supported"),
    ("<speak><emphasis>a</emphasis></speak>", "<emphasis> is not supported"),
    ("<speak><prosody contour='(0%,+1st)'>a</prosody></speak>", "no attribute 'contour'"),
    ("<speak><break strength='weak'/>a</speak>", "no attribute 'strength'"),
    ("<speak>ab<prosody pitch='+1st'>cd</prosody></speak>", "inside the word 'abcd'"),
    ("<speak><prosody pitch='+1st'>ab</prosody>cd</speak>", "inside the word 'abcd'"),
    ("<speak>a<break time='1s'/>b</speak>", "inside the word 'ab'"),
    ("<speak>a <sub>b</sub></speak>", "<sub> needs an alias"),
    ("<speak>a <mark/></speak>", "<mark> needs a name"),
    ("<speak>a <break time='soon'/></speak>", "break time='soon'"),
    ("<speak>a <prosody rate='quick'>b</prosody></speak>", "rate='quick'"),
])
def test_refusals_name_their_cause(doc, match):
    with pytest.raises(ValueError, match=match):
        S.parse(doc)


# ---- through Synth, with a stub in place of the model -------------------------------------------------------------------------------------
def _synth(multistream=False):
    from vosk_tts_amd.marks import SpeechMarks
    from vosk_tts_amd.synth import Synth

    s = Synth.__new__(Synth)
    s.model = type("M", (), {"config": {"model_type": "multistream_v2" if multistream else "vits", "inference": {}}})()
    s.calls = []

    def synth_audio(text, **kw):
        s._prosody_text(text, kw.get("word_rates"), kw.get("pauses"), kw.get("duration"))  # (the family's own refusal)
        s.calls.append((text, kw))
        audio = np.zeros(1000, np.int16)
        if kw.get("marks"):
            return audio, SpeechMarks(22050, [100, 400, 900], [], [("a", 0, 100), ("b", 100, 400), ("c", 400, 900)])
        return audio

    s.synth_audio = synth_audio
    return s


def test_synth_ssml_is_the_keyword_call_and_names_its_marks():
    s = _synth()
    doc = '<speak><mark name="m0"/>a <prosody pitch="+3st" volume="+6dB">b</prosody><break time="250ms"/> <mark name="m2"/>c<mark name="end"/></speak>'
    out = s.synth_ssml(doc, speaker_id=2)
    assert out.shape == (1000,)
    assert s.calls == [("a b c", {"speaker_id": 2, "word_pitch": {1: 3.0}, "word_gains": {1: 6.0}, "pauses": {1: 0.25}})]
    audio, sm = s.synth_ssml(doc, marks=True)
    assert sm.named == {"m0": 0, "m2": 400, "end": 1000}
    with pytest.raises(ValueError, match="word_pitch from the document"):
        s.synth_ssml(doc, word_pitch={0: 1.0})
    n = len(s.calls)
    with pytest.raises(ValueError, match="<voice> is not supported"):
        s.synth_ssml("<speak><voice>a</voice></speak>")
    assert len(s.calls) == n  # refused before the model is touched


def test_multistream_voices_take_pitch_and_volume_and_refuse_rate_and_break():
    s = _synth(multistream=True)
    s.synth_ssml('<speak>a <prosody pitch="high" volume="soft">b</prosody></speak>')
    assert s.calls == [("a b", {"word_pitch": {1: 3.0}, "word_gains": {1: -6.0}})]
    for doc in ('<speak>a <prosody rate="slow">b</prosody></speak>', '<speak>a<break time="1s"/> b</speak>'):
        with pytest.raises(ValueError, match="multistream"):
            s.synth_ssml(doc)
    assert len(s.calls) == 1
