"""NumPy restatement of include/vits_document.h, written from the definition.  Never calls the library.  Integers are Python integers;
the only floating-point operations are the ones the definition names: |x| > thr in fp32, and one fp32 multiply per faded sample.

    trim     thr = float32(10 ** (trim_db / 20));  frame f of item b is loud iff max |x_b[f*hop .. (f+1)*hop)| > thr
             lo = max(f0 - keep, 0), hi = min(f1 + 1 + keep, len); no loud frame: lo = hi = 0; off: lo = 0, hi = len
    layout   start_0 = lead, start_{b+1} = start_b + n_b + gap_b, F = start_{B-1} + n_{B-1} + gap_{B-1}
    join     d[start_b*hop + i] = x_b[lo_b*hop + i] * h(i) * t(i), zeros elsewhere
    marks    seg_start = n_out(start*hop), seg_end = n_out((start + n)*hop), token_end = n_out((start + clamp(cum - lo, 0, n))*hop)
"""
import math

import numpy as np

from marks_ref import n_out, ratio


def threshold(trim_db):
    """None / 0: off (None); else the fp32 threshold"""
    if not trim_db:
        return None
    return np.float32(10.0 ** (float(trim_db) / 20.0))


def fade_table(fade):
    return np.array([np.float32(0.5 - 0.5 * math.cos(math.pi * (j + 0.5) / fade)) for j in range(fade)], np.float32)


def frame_peaks(x, n_frames, hop):
    """float32 [n_frames]: the largest magnitude of every frame, a NaN sample left out (fmax from 0, as the header defines it)"""
    x = np.asarray(x, np.float32)
    if not n_frames:
        return np.zeros(0, np.float32)
    return np.fmax.reduce(np.abs(x[:n_frames * hop].reshape(n_frames, hop)), axis=1, initial=np.float32(0))


def trim_item(x, n_frames, hop, thr, keep):
    """-> (lo, hi) in frames"""
    if thr is None:
        return 0, int(n_frames)
    loud = np.nonzero(frame_peaks(x, n_frames, hop) > np.float32(thr))[0]
    if loud.size == 0:
        return 0, 0
    return max(int(loud[0]) - keep, 0), min(int(loud[-1]) + 1 + keep, int(n_frames))


def layout(n, gaps, lead):
    """n, gaps: frames per segment -> (start [B], F)"""
    start, at = [], int(lead)
    for nb, g in zip(n, gaps):
        start.append(at)
        at += int(nb) + int(g)
    return start, at


def join(rows, len_frames, hop, lead=0, gaps=None, fade=0, trim_db=None, keep=0):
    """rows: B arrays (or [B, N]) of float32 samples, item b being rows[b][:len_frames[b]*hop].
    -> dict(y float32 [F*hop], F, start [B], lo [B], hi [B], n [B])"""
    B = len(rows)
    gaps = [0] * B if gaps is None else [int(g) for g in np.broadcast_to(np.asarray(gaps), (B,))]
    assert 0 <= fade <= hop // 2 and lead >= 0 and keep >= 0 and all(g >= 0 for g in gaps)
    thr = threshold(trim_db)
    lo, hi = [], []
    for b in range(B):
        a, e = trim_item(rows[b], int(len_frames[b]), hop, thr, keep)
        lo.append(a)
        hi.append(e)
    n = [e - a for a, e in zip(lo, hi)]
    start, F = layout(n, gaps, lead)
    y = np.zeros(F * hop, np.float32)
    w = fade_table(fade)
    for b in range(B):
        if not n[b]:
            continue
        seg = np.asarray(rows[b], np.float32)[lo[b] * hop:hi[b] * hop].copy()
        if fade:
            seg[:fade] = seg[:fade] * w            # one fp32 multiply each
            seg[-fade:] = seg[-fade:] * w[::-1]    # t(i) = w[n*hop - 1 - i]
        y[start[b] * hop:(start[b] + n[b]) * hop] = seg
    return {"y": y, "F": F, "start": start, "lo": lo, "hi": hi, "n": n}


def marks(lay, cum, lengths, hop, rate_in=22050, rate_out=None):
    """lay: what join() or layout gives (start, lo, n, F); cum int [B, T_x] inclusive cumulative frame counts of the batch
    -> (seg_start [B], seg_end [B], token_ends int64 [B, T_x], total output samples)"""
    L, M = ratio(rate_in, rate_out)
    cum = np.asarray(cum)
    B, T = cum.shape
    seg_start = [n_out(s * hop, L, M) for s in lay["start"]]
    seg_end = [n_out((s + n) * hop, L, M) for s, n in zip(lay["start"], lay["n"])]
    ends = np.zeros((B, T), np.int64)
    for b in range(B):
        ln = min(int(lengths[b]), T)
        last = 0
        for t in range(T):
            if t < ln:
                c = min(max(int(cum[b, t]) - lay["lo"][b], 0), lay["n"][b])
                last = n_out((lay["start"][b] + c) * hop, L, M)
            ends[b, t] = last
    return seg_start, seg_end, ends, n_out(lay["F"] * hop, L, M)


def pcm16(x, scale=1.0):
    """the int16 conversion of the plain int16 call: v*scale, *32767, clamp to +-32767, truncate (each step in fp32)"""
    v = np.asarray(x, np.float32) * np.float32(scale)
    v = v * np.float32(32767.0)
    v = np.minimum(np.maximum(v, np.float32(-32767.0)), np.float32(32767.0))
    return v.astype(np.int32).astype(np.int16)


def frames(seconds, rate, hop):
    """seconds -> frames, as Synth.synth_document turns pauses into gaps: floor(sec * rate / hop + 0.5)"""
    return int(math.floor(float(seconds) * rate / hop + 0.5))
