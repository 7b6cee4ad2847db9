"""Integer restatement of include/vits_marks.h and of the token -> phoneme -> word mapping rules, written from the definition.
Never calls the library (plain Python integers, so nothing can overflow or round).

    token_end[b, t] = n_out(cum[b, t] * hop)            0 <= t < lengths[b]
    token_end[b, t] = token_end[b, lengths[b] - 1]      lengths[b] <= t < T_x   (0 when lengths[b] == 0)
    n_out(x) = ceil(x * L / M),  L / M = rate_out / rate_in in lowest terms
"""
import math
import re

import numpy as np

SPLIT = "([,.?!;:\"() ])"


def ratio(rate_in, rate_out):
    if not rate_out or rate_out == rate_in:
        return 1, 1
    g = math.gcd(rate_in, rate_out)
    return rate_out // g, rate_in // g


def n_out(x, L=1, M=1):
    return -((-int(x) * L) // M)  # ceil without floats (another spelling than the library's (x*L + M - 1) / M)


def token_ends(durations, lengths, hop, rate_in=22050, rate_out=None):
    """durations [B, T_x] (entries at and beyond lengths[b] are ignored), lengths [B] -> int64 [B, T_x]"""
    L, M = ratio(rate_in, rate_out)
    d = np.asarray(durations)
    B, T = d.shape
    out = np.zeros((B, T), np.int64)
    for b in range(B):
        n = int(lengths[b])
        cum, last = 0, 0
        for t in range(T):
            if t < n:
                cum += max(int(d[b, t]), 0)
                last = n_out(cum * hop, L, M)
            out[b, t] = last
    return out


def out_lengths(durations, lengths, hop, rate_in=22050, rate_out=None, clamp_min=1):
    """samples of audio per item: the reference's clamp_min(y_lengths, 1) gives an all-zero item one frame"""
    L, M = ratio(rate_in, rate_out)
    d = np.asarray(durations)
    return [n_out(max(sum(max(int(v), 0) for v in d[b, :int(lengths[b])]), clamp_min) * hop, L, M) for b in range(d.shape[0])]


# ---- mapping rules -------------------------------------------------------------------------------------------------
def _spans(ends):
    ends = [int(v) for v in ends]
    return [(0 if t == 0 else ends[t - 1], ends[t]) for t in range(len(ends))]


def phonemes_blank(ends, symbols, ids_per_symbol=None):
    """interspersed blank: ids [p0, 0, p1, 0, p2, ...]; phoneme 0 is token 0 (all of its ids where the map is list-valued), phoneme
    k >= 1 the blank before it plus its own id(s)"""
    sp = _spans(ends)
    n = ids_per_symbol or [1] * len(symbols)
    out, pos = [], 0
    for k, s in enumerate(symbols):
        first = pos
        pos += n[k] + (1 if k else 0)
        out.append((s, sp[first][0], sp[pos - 1][1]))
    assert pos == len(sp), (pos, len(sp))
    return out


def phonemes_plain(ends, symbols):
    """one token per symbol (g2p_noblank, multistream)"""
    sp = _spans(ends)
    assert len(sp) == len(symbols)
    return [(s, a, b) for s, (a, b) in zip(symbols, sp)]


def vits_words(text, phonemes_of_word):
    """-> (symbols, word index per symbol or None, [word texts]): the pieces of re.split(SPLIT, text.lower()) that are neither
    separators nor '-' are the words"""
    symbols, owner, words = ["^"], [None], []
    for piece in re.split(SPLIT, text.lower()):
        if piece == "":
            continue
        if re.match(SPLIT, piece) or piece == "-":
            symbols.append(piece)
            owner.append(None)
        else:
            ps = phonemes_of_word(piece)
            symbols += ps
            owner += [len(words)] * len(ps)
            words.append(piece)
    symbols.append("$")
    owner.append(None)
    return symbols, owner, words


def words_from(phonemes, owner, words):
    """each word covers the union of its phonemes' spans, in text order"""
    out = []
    for w, text in enumerate(words):
        mine = [p for p, o in zip(phonemes, owner) if o == w]
        out.append((text, min(p[1] for p in mine), max(p[2] for p in mine)))
    return out


def multistream_words(phonemes, word_index, word_texts):
    """a word is the run of non-space symbols ('^' and '$' are no words either) sharing one bert_word_index"""
    out, cur = [], None
    for (s, a, b), w in zip(phonemes, word_index):
        if s in (" ", "^", "$") or w not in word_texts:
            cur = None
            continue
        if w == cur:
            out[-1] = (out[-1][0], out[-1][1], b)
        else:
            out.append((word_texts[w], a, b))
            cur = w
    return out
