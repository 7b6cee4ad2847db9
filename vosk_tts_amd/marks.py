"""Speech marks: token ends (include/vits_marks.h) mapped back to the phonemes and words the caller wrote.

Everything here is a pure function of ids / token ends; nothing touches the engine.

Token t occupies the output samples [token_ends[t-1], token_ends[t]) (token_ends[-1] = 0).  Three layouts of tokens per phoneme:
  * interspersed blank (`g2p`, `g2p_noembed`; ids [p0, 0, p1, 0, p2, ...]): phoneme 0 is its own id(s); phoneme k >= 1 covers the
    blank in front of it plus its own id(s) -- a list-valued id map gives a phoneme several ids, and it covers them all.  The
    phoneme spans therefore tile [0, token_ends[-1]) without gaps;
  * `g2p_noblank`: one token per phoneme;
  * multistream: one token per symbol.
Words cover the union of their phonemes' spans; '^', '$', spaces and punctuation appear among the phonemes only.
"""
import json
import math
import re

import numpy as np

_SPLIT = "([,.?!;:\"() ])"  # (synth.py's word splitter)


def rate_ratio(native_rate, rate):
    """(L, M): `rate` / `native_rate` in lowest terms; (1, 1) for None / 0 / the native rate"""
    if not rate or int(rate) == int(native_rate):
        return 1, 1
    g = math.gcd(int(native_rate), int(rate))
    return int(rate) // g, int(native_rate) // g


def n_out(x, L=1, M=1):
    """the resampler's length rule ceil(x * L / M) in integers"""
    return (int(x) * L + M - 1) // M


def token_spans(token_ends):
    ends = [int(v) for v in np.asarray(token_ends).reshape(-1)]
    return list(zip([0] + ends[:-1], ends))


def phoneme_spans(token_ends, ids_per_phoneme, blank):
    """-> [(start, end)] per phoneme.  ids_per_phoneme: how many ids the id map gives each phoneme (1, or the length of a list value);
    blank: the interspersed-blank layout, where every phoneme but the first also covers the blank token in front of it"""
    spans = token_spans(token_ends)
    out, pos = [], 0
    for k, n in enumerate(ids_per_phoneme):
        width = n + (1 if blank and k > 0 else 0)
        if width <= 0 or pos + width > len(spans):
            raise ValueError(f"token layout does not match: phoneme {k} needs tokens [{pos}, {pos + width}) of {len(spans)}")
        out.append((spans[pos][0], spans[pos + width - 1][1]))
        pos += width
    if pos != len(spans):
        raise ValueError(f"token layout does not match: {len(spans)} tokens for {pos} laid out")
    return out


def word_spans(spans, word_of, word_texts):
    """spans per phoneme, word_of per phoneme (a key of word_texts, or None for a phoneme outside every word) -> [(text, start, end)]
    in order of first appearance; consecutive phonemes only (a key met again after another word starts a new entry)"""
    out, cur = [], None
    for (a, b), w in zip(spans, word_of):
        if w is None:
            cur = None
            continue
        if w == cur:
            t, s, e = out[-1]
            out[-1] = (t, min(s, a), max(e, b))
        else:
            out.append((word_texts[w], a, b))
            cur = w
    return out


def vits_layout(text, phonemize_word):
    """The phoneme string of the VITS front ends with, per phoneme, the word it belongs to: -> (phonemes, word_of, word_texts).
    Words are the pieces of re.split(_SPLIT, text.lower()) that are neither separators nor '-', in order, each with its own text.
    phonemize_word(piece) -> list of phonemes (dictionary lookup or rule G2P)."""
    phonemes, word_of, word_texts = ["^"], [None], {}
    for piece in re.split(_SPLIT, text.lower()):
        if piece == "":
            continue
        if re.match(_SPLIT, piece) or piece == "-":
            phonemes.append(piece)
            word_of.append(None)
            continue
        ps = list(phonemize_word(piece))
        w = len(word_texts)
        word_texts[w] = piece
        phonemes.extend(ps)
        word_of.extend([w] * len(ps))
    phonemes.append("$")
    word_of.append(None)
    return phonemes, word_of, word_texts


def multistream_layout(symbols, word_index, word_texts):
    """g2p_multistream(..., return_words=True)'s last value -> (symbols, word_of, word_texts): ' ', '^' and '$' belong to no word (the
    space behind a word already carries the NEXT word's index)"""
    word_of = [None if s in (" ", "^", "$") or w not in word_texts else w for s, w in zip(symbols, word_index)]
    return list(symbols), word_of, dict(word_texts)


class SpeechMarks:
    """rate (Hz of the time axis), token_ends int64 [T], phonemes [(symbol, start_sample, end_sample)], words [(text, start, end)]"""

    def __init__(self, rate, token_ends, phonemes, words):
        self.rate = int(rate)
        self.token_ends = np.asarray(token_ends, np.int64).reshape(-1)
        self.phonemes = list(phonemes)
        self.words = list(words)
        self.named = {}  # {mark name: sample} of an SSML document's <mark> elements (Synth.synth_ssml)

    def seconds(self):
        """the same two lists with the offsets in seconds"""
        r = float(self.rate)
        return {"phonemes": [(s, a / r, b / r) for s, a, b in self.phonemes], "words": [(t, a / r, b / r) for t, a, b in self.words]}

    def to_dict(self):
        r = float(self.rate)
        row = lambda key, t, a, b: {key: t, "start_sample": int(a), "end_sample": int(b), "start": a / r, "end": b / r}
        return {"rate": self.rate, "phonemes": [row("symbol", *p) for p in self.phonemes], "words": [row("text", *w) for w in self.words]}

    def to_json(self, **kw):
        return json.dumps(self.to_dict(), ensure_ascii=False, **kw)

    def __eq__(self, other):
        return (isinstance(other, SpeechMarks) and self.rate == other.rate and np.array_equal(self.token_ends, other.token_ends) and
                self.phonemes == other.phonemes and self.words == other.words)

    def __repr__(self):
        return f"SpeechMarks(rate={self.rate}, tokens={self.token_ends.shape[0]}, phonemes={len(self.phonemes)}, words={len(self.words)})"


def build_marks(rate, token_ends, symbols, ids_per_symbol, blank, word_of, word_texts):
    spans = phoneme_spans(token_ends, ids_per_symbol, blank)
    phonemes = [(s, a, b) for s, (a, b) in zip(symbols, spans)]
    return SpeechMarks(rate, token_ends, phonemes, word_spans(spans, word_of, word_texts))
