"""Prosody controls of the VITS family on the host (include/vits_prosody.h): from words, seconds and rates to the per-token arrays the
engine takes.  Pure functions of the token layout `Synth.marks_layout` returns -- no device, no model.

A word's rate r gives 1 / r to every token of the word's phonemes, the blank in front of a phoneme included (the cover of
marks.phoneme_spans).  A pause of `sec` seconds after word w is round(sec * native_rate / hop) frames on the last token of the first
symbol behind w that belongs to no word -- a space, punctuation, or '$' at the end -- which is where the reference's multistream v3
markup puts its 20 frames ('_' in g2p_multistream_scales, vosk_tts/synth.py:361-454)."""
import math
import re

import numpy as np

from .capi import PROSODY_FIT_RATIO as FIT_RATIO  # noqa: F401  (the header's constants, mirrored once)
from .capi import PROSODY_MAX_TOKEN_SCALE as MAX_TOKEN_SCALE

PAUSE_FRAMES = 20          # the reference's '_' (vosk_tts/synth.py:432-433)
_SPLIT_PAUSE = "([,.?!;:\"() _])"


def frames(seconds, native_rate, hop):
    """seconds -> frames of the voice: round(seconds * native_rate / hop)"""
    s = float(seconds)
    if not (math.isfinite(s) and s >= 0.0):
        raise ValueError(f"{seconds} seconds: a duration must be finite and >= 0")
    return int(round(s * native_rate / hop))


def symbol_tokens(ids_per_symbol, blank):
    """-> [(first, end)] token range per symbol, the cover of marks.phoneme_spans: every symbol but the first also owns the blank in
    front of it in the interspersed-blank layout"""
    out, pos = [], 0
    for k, n in enumerate(ids_per_symbol):
        width = int(n) + (1 if blank and k > 0 else 0)
        if width <= 0:
            raise ValueError(f"token layout does not match: symbol {k} has no tokens")
        out.append((pos, pos + width))
        pos += width
    return out


def token_controls(layout, word_rates=None, pauses=None, native_rate=22050, hop=256):
    """layout: (symbols, ids per symbol, blank layout?, word_of per symbol, word_texts) as Synth.marks_layout returns it.
    word_rates {word index: rate > 0}, pauses {word index: seconds >= 0}
    -> (token_length_scale float32 [T] or None, token_pause int32 [T] or None); ValueError names a word that does not exist, a rate whose
    inverse the engine refuses, or a pause with no symbol behind the word to carry it."""
    symbols, counts, blank, word_of, word_texts = layout
    ranges = symbol_tokens(counts, blank)
    T = ranges[-1][1] if ranges else 0
    tls = pause = None
    if word_rates:
        tls = np.ones(T, np.float32)
        for w, r in word_rates.items():
            if w not in word_texts:
                raise ValueError(f"word_rates: no word {w!r} (the text has {len(word_texts)} words)")
            r = float(r)
            if not (math.isfinite(r) and r > 0.0 and 1.0 / r <= MAX_TOKEN_SCALE):
                raise ValueError(f"word_rates[{w!r}] = {r}: a rate must be finite and at least {1.0 / MAX_TOKEN_SCALE}")
            for (a, b), wo in zip(ranges, word_of):
                if wo == w:
                    tls[a:b] = np.float32(1.0 / r)
    if pauses:
        pause = np.zeros(T, np.int32)
        for w, sec in pauses.items():
            if w not in word_texts:
                raise ValueError(f"pauses: no word {w!r} (the text has {len(word_texts)} words)")
            last = max(k for k, wo in enumerate(word_of) if wo == w)
            carrier = next((k for k in range(last + 1, len(word_of)) if word_of[k] is None), None)
            if carrier is None:
                raise ValueError(f"pauses[{w!r}]: no symbol outside a word behind word {w!r} to carry the pause")
            pause[ranges[carrier][1] - 1] += frames(sec, native_rate, hop)
    return tls, pause


def token_contour(layout, word_pitch=None, word_gains=None):
    """layout as for token_controls; word_pitch {word index: semitones}, word_gains {word index: dB} (include/vits_contour.h)
    -> (token_pitch float32 [T] or None, token_gain_db float32 [T] or None): a word's setting covers the tokens of its phonemes and the
    blank in front of each, as a word's rate does.  ValueError names a word that does not exist or a value the engine refuses."""
    from .capi import CONTOUR_DB, PITCH_MAX_SEMITONES

    symbols, counts, blank, word_of, word_texts = layout
    ranges = symbol_tokens(counts, blank)
    T = ranges[-1][1] if ranges else 0
    out = []
    for name, unit, values, lo, hi in (("word_pitch", "semitones", word_pitch, -PITCH_MAX_SEMITONES, PITCH_MAX_SEMITONES),
                                       ("word_gains", "dB", word_gains, CONTOUR_DB[0], CONTOUR_DB[1])):
        if not values:
            out.append(None)
            continue
        a = np.zeros(T, np.float32)
        for w, v in values.items():
            if w not in word_texts:
                raise ValueError(f"{name}: no word {w!r} (the text has {len(word_texts)} words)")
            v = float(v)
            if not lo <= v <= hi:  # (NaN fails the comparison)
                raise ValueError(f"{name}[{w!r}] = {v}: {unit} must lie in [{lo:g}, {hi:g}]")
            for (i, j), wo in zip(ranges, word_of):
                if wo == w:
                    a[i:j] = np.float32(v)
        out.append(a)
    return out[0], out[1]


def split_pause_markup(text):
    """The reference's '_' pause markup in VITS text (config inference.pause_markup): -> (text without the marks, [index of the word each
    mark follows]).  Words are counted as marks.vits_layout counts them; a mark in front of the first word is dropped."""
    out, after, n_words = [], [], 0
    for piece in re.split(_SPLIT_PAUSE, text):
        if piece == "":
            continue
        if piece == "_":
            if n_words:
                after.append(n_words - 1)
            continue
        if not re.match(_SPLIT_PAUSE, piece) and piece != "-":
            n_words += 1
        out.append(piece)
    return "".join(out), after


def check_controls(lengths, item_scales=None, token_length_scale=None, token_pause=None, fit_frames=None, forced=False):
    """The refusals of include/vits_prosody.h that need no device, as ValueError naming item, token and value (the library returns
    VITS_ERR_ARG for the same values).  Arrays as the C ABI takes them: [B, 3], [B, T], [B, T], [B]."""
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    if token_length_scale is not None and forced:
        raise ValueError("token_length_scale with forced durations: a forced duration is the caller's own number and is not scaled")
    if item_scales is not None:
        a = np.asarray(item_scales, np.float64).reshape(len(lengths), 3)
        for b, k in zip(*np.nonzero(~(np.isfinite(a) & (a >= 0)))):
            raise ValueError(f"item_scales[{b}, {k}] = {a[b, k]}: an item scale must be finite and >= 0")
    if fit_frames is not None:
        a = np.asarray(fit_frames, np.int64).reshape(len(lengths))
        for b in np.nonzero(a < 0)[0]:
            raise ValueError(f"fit_frames[{b}] = {a[b]}: must be >= 0 (0 = the item is not fitted)")
    for b, L in enumerate(lengths):
        if token_length_scale is not None:
            a = np.asarray(token_length_scale, np.float64).reshape(len(lengths), -1)[b, :L]
            for t in np.nonzero(~(np.isfinite(a) & (a >= 0) & (a <= MAX_TOKEN_SCALE)))[0]:
                raise ValueError(f"token_length_scale[{b}, {t}] = {a[t]}: must be finite and in [0, {MAX_TOKEN_SCALE:g}]")
        if token_pause is not None:
            a = np.asarray(token_pause, np.int64).reshape(len(lengths), -1)[b, :L]
            for t in np.nonzero(a < 0)[0]:
                raise ValueError(f"token_pause[{b}, {t}] = {a[t]}: a pause must be >= 0 frames")
