"""float64 restatement of the watermark scan (include/vits_watermark_scan.h), the definition the device kernel and
vosk_tts_amd/watermark_scan.py are checked against, on top of tests/watermark_ref.py (which it imports and does not change), and an
fp32 run of the same code (dtype=np.float32, with the meaning it has there: the transform, ln and the four-bin mean in fp32; T, D, the
window sums and the scores in float64).  Plain numpy."""
from collections import namedtuple

import numpy as np

import watermark_payload_ref as P
import watermark_ref as R

MAX_SPAN = 8
DEFAULT_SPAN = 4
PERIOD = 16384  # samples: 16 tile rows of 4 frames at hop 256

Segment = namedtuple("Segment", "start end z offset_samples")


def span_arg(span):
    """1 .. 8, 0 = the default 4; anything else is refused by name"""
    if isinstance(span, bool) or not isinstance(span, (int, np.integer)) or not 0 <= int(span) <= MAX_SPAN:
        raise ValueError(f"watermark scan: span {span!r} outside [1, {MAX_SPAN}] (0 = the default, {DEFAULT_SPAN})")
    return int(span) or DEFAULT_SPAN


# ---- S1, S2: the row differences of the complete periods ----------------------------------------------------------------------------
def periods(Lb, o):
    """(Gp float64 [p1 - p0 + 1, 16, 96] with columns 0 and 95 zero, p0) of offset index o; no complete period: ([0, 16, 96], p0)"""
    Lb = np.asarray(Lb, np.float64)
    F = Lb.shape[0]
    g0 = o & 1
    pbase = (o + g0) // 2
    nf = (F - g0 + 1) // 2 if F > g0 else 0
    r0, r1 = (pbase + 3) // 4, (pbase + nf) // 4 - 1
    p0, p1 = -(-r0 // R.ROWS), (r1 + 1) // R.ROWS - 1
    n = max(0, p1 - p0 + 1)
    Gp = np.zeros((n, R.ROWS, R.GROUPS))
    if n:
        rho = R.ROWS * p0 + np.arange(R.ROWS * n)
        gf = g0 + 2 * (4 * rho - pbase)
        T = (((Lb[gf] + Lb[gf + 2]) + Lb[gf + 4]) + Lb[gf + 6]) * 0.25
        Gp[:, :, 1:-1] = (T[:, 1:-1] - 0.5 * (T[:, :-2] + T[:, 2:])).reshape(n, R.ROWS, R.GROUPS - 2)
    return Gp, p0


# ---- S3: the windows ---------------------------------------------------------------------------------------------------------------
def window_sums(Gp, span):
    """G float64 [W, 16, 96] of every window of `span` periods: ((Gp[w] + Gp[w + 1]) + ...), ascending, each window on its own"""
    W = max(0, Gp.shape[0] + 1 - span)
    G = Gp[:W].copy()
    for k in range(1, span):
        G = G + Gp[k:k + W]
    return G


# ---- S4: the scores ----------------------------------------------------------------------------------------------------------------
def scan(Lb, key, o, span=0, pilots=False):
    """(z float64 [W_o], p0, W_o) of offset index o from Lb"""
    S = span_arg(span)
    Gp, p0 = periods(Lb, o)
    G = window_sums(Gp, S)
    sel = np.zeros((R.ROWS, R.GROUPS), bool)
    sel[:, 1:-1] = True
    if pilots:
        sel &= P.pilots()
    c = R.chips(key)
    z = np.zeros(G.shape[0])
    for w in range(G.shape[0]):
        den = float(np.sum(G[w][sel] ** 2))
        if den > 0.0:
            z[w] = float(np.sum((c * G[w])[sel])) / np.sqrt(den)
    return z, p0, G.shape[0]


def scan_all(x, key, span=0, pilots=False, dtype=np.float64):
    """-> (z_scan float64 [128, max(1, Wmax)] with 0 beyond W_o, first_period int32 [128], windows int32 [128]) of the audio x"""
    return scan_bands(R.band_logs(x, dtype), key, span, pilots)


def scan_bands(Lb, key, span=0, pilots=False):
    """scan_all from the Lb of the audio (R.band_logs, of either dtype)"""
    Lb = np.asarray(Lb, np.float64)
    res = [scan(Lb, key, o, span, pilots) for o in range(R.OFFSETS)]
    first = np.array([r[1] for r in res], np.int32)
    wins = np.array([r[2] for r in res], np.int32)
    z = np.zeros((R.OFFSETS, max(1, int(wins.max()))))
    for o, r in enumerate(res):
        z[o, :r[2]] = r[0]
    return z, first, wins


def windows_of(n_samples, span=0):
    """max_o W_o of an item of n_samples"""
    S = span_arg(span)
    F = 1 + n_samples // R.DETECT_HOP if n_samples >= R.M + 1 else 0
    Lb = np.zeros((F, R.GROUPS))
    return max(max(0, periods(Lb, o)[0].shape[0] + 1 - S) for o in range(R.OFFSETS))


# ---- S5, S6 and the segments ---------------------------------------------------------------------------------------------------------
def threshold(wmax):
    """t(Wmax) = sqrt(36 + 2 ln(max(1, Wmax))): 128 Wmax e^(-t^2 / 2) = 128 e^(-18)"""
    return float(np.sqrt(36.0 + 2.0 * np.log(max(1, int(wmax)))))


def window_range(o, p0, w, span, length):
    """the nominal range [start, end) of window (o, w) in samples, clipped to [0, length)"""
    a = PERIOD * (int(p0) + int(w)) - R.DETECT_HOP * int(o)
    return min(max(a, 0), int(length)), min(max(a + PERIOD * int(span), 0), int(length))


def segments(z_scan, first_period, windows, span, length):
    """The marked segments of one item, sorted by start.  Every (o, w) with z >= t(Wmax) is a candidate.  The best candidate (o*, w*)
    grows over the candidates at offset indices o* - 1 .. o* + 1 whose first period p0 + w continues its own in steps of one period,
    on either side; the segment is the union of their nominal ranges with the best window's z and 128 o*.  Every candidate left whose
    nominal range overlaps the segment is dropped, and the best of the rest is next."""
    S = span_arg(span)
    z_scan, first_period, windows = np.asarray(z_scan, np.float64), np.asarray(first_period), np.asarray(windows)
    t = threshold(int(windows.max()) if windows.size else 0)
    cand = [(float(z_scan[o, w]), o, w) for o in range(R.OFFSETS) for w in range(int(windows[o])) if z_scan[o, w] >= t]
    cand.sort(key=lambda c: (-c[0], c[1], c[2]))
    out = []
    while cand:
        z, o, w = cand[0]
        near = {}  # first period -> the candidates of the three offsets that start there
        for c in cand:
            if abs(c[1] - o) <= 1:
                near.setdefault(int(first_period[c[1]]) + c[2], []).append(c)
        lo = hi = int(first_period[o]) + w
        while lo - 1 in near:
            lo -= 1
        while hi + 1 in near:
            hi += 1
        ranges = [window_range(c[1], first_period[c[1]], c[2], S, length) for p in range(lo, hi + 1) for c in near[p]]
        start, end = min(r[0] for r in ranges), max(r[1] for r in ranges)
        out.append(Segment(start, end, z, R.DETECT_HOP * o))
        keep = []
        for c in cand[1:]:
            a, b = window_range(c[1], first_period[c[1]], c[2], S, length)
            if b <= start or a >= end:
                keep.append(c)
        cand = keep
    return sorted(out, key=lambda s: s.start)


# ---- the test signal of the issue: marked speech between unmarked speech --------------------------------------------------------------
SPLICE_MARKED = (88200, 187425)


def spliced_signal(key, depth_db=1.0, marked=True):
    """voiced_signal(4 s, seed 3), then 4.5 s of the 6 s signal of seed 7 cut from sample 5000 (marked with `key` before the cut, unless
    marked=False: the control), then voiced_signal(4 s, seed 11): float32 [275625], marked on SPLICE_MARKED, offset index 118"""
    mid = R.voiced_signal(6.0, seed=7)
    if marked:
        mid = R.embed(mid, key, depth_db).astype(np.float32)
    x = np.concatenate([R.voiced_signal(4.0, seed=3), mid[5000:5000 + SPLICE_MARKED[1] - SPLICE_MARKED[0]], R.voiced_signal(4.0, seed=11)])
    return x.astype(np.float32)
