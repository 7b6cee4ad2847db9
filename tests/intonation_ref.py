"""Restatement of the intonation control defined in include/vits_intonation.h: a YIN F0 track at the pitch stage's frame geometry, integer
offsets that scale the track's deviation from its median by r, and the contour stage of include/vits_contour.h run on the per-frame
ratios that come of it (tests/contour_ref.py and tests/pitch_ref.py hold everything behind P_f).  numpy only.

`dtype` is the working precision of the tracker's difference function and of the vocoder: float64 is the reference the device is checked
against, float32 the yardstick.  Everything behind the track is integer arithmetic, the same here, on the host and on the device.

  geometry   n = 1024, H = 256, reflect-pad n/2, F = 1 + len // H rows, row f = xp[f H .. f H + n); len < n/2 + 1: no track
  track      W = 512, tau_min = max(2, sr // 550), tau_max = min(ceil(sr / 55), 511), 8000 <= sr <= 32000
             d(tau) = sum_{j < W} (fr[j] - fr[j + tau])^2 in ascending j, tau = 1 .. tau_max + 1 (the direct form)
             d'(tau) = d(tau) tau / sum_{i <= tau} d(i), 1 where the sum is 0
             the first tau in [tau_min, tau_max] with d' < 0.15, walked forward while d'(tau + 1) < d'(tau) and tau + 1 <= tau_max;
             off = (y0 - y2) / (2 (y0 - 2 y1 + y2)) through d'(tau - 1), d'(tau), d'(tau + 1) in double, clamped to +-0.5, 0 where the
             curvature y0 - 2 y1 + y2 is not positive; cents = lround(1200 log2(sr / (tau + off) / 27.5)) in double; none: cents = 0
  offsets    r_m = lround(1000 r); c_med = the lower median of the voiced cents; voiced: o = rha((r_m - 1000)(cents - c_med) / 1000);
             unvoiced between voiced rows l < f < g: o = o_l + rha((o_g - o_l)(f - l) / (g - l)); held at the ends; no voiced row: 0;
             then clamped to +-1200.  rha(a / b), b > 0 = sign(a) ((2 |a| + b) // (2 b)): round half away from zero.
  ratios     R_f = TAB[o_rho(f) + 1200], rho(f) = min(f H, len - 1) // H (the row of the sample the contour stage finds tok(f) by),
             TAB[j] = lround(1000 2^((j - 1200) / 1200)); P_f = clamp((P_tok(f) R_f + 500) // 1000, 500, 2000)
  the rest   contour_ref with P_f in place of P_tok(f): Sigma_f, inc_f, positions, vocoder, warp, gain; every P_f == 1000: y = fp32(G x)
"""
import math

import numpy as np

import contour_ref
import pitch_ref

FRAME = pitch_ref.FRAME
HOP = pitch_ref.HOP
MIN_LEN = pitch_ref.MIN_LEN
W = 512
THRESHOLD = 0.15
MIN_RATE, MAX_RATE = 8000, 32000
MAX_RANGE = 4.0
MAX_CENTS = 1200
REF_HZ = 27.5
TAB = np.floor(1000.0 * 2.0 ** ((np.arange(2 * MAX_CENTS + 1) - MAX_CENTS) / 1200.0) + 0.5).astype(np.int64)


def lags(rate):
    """-> (tau_min, tau_max); ValueError names a refused rate"""
    rate = int(rate)
    if not MIN_RATE <= rate <= MAX_RATE:
        raise ValueError(f"intonation: rate {rate} outside [{MIN_RATE}, {MAX_RATE}]")
    return max(2, rate // 550), min(-(-rate // 55), W - 1)


def range_milli(r):
    """r_m; ValueError names a refused value"""
    r = float(r)
    if not 0.0 <= r <= MAX_RANGE:  # (NaN fails the comparison)
        raise ValueError(f"intonation: pitch_range {r} outside [0, {MAX_RANGE:g}]")
    return int(math.floor(1000.0 * r + 0.5))


def frames(length):
    return 1 + int(length) // HOP if length >= MIN_LEN else 0


def normalised_difference(x, rate, dtype=np.float64):
    """d' dtype [F, tau_max + 2]: column tau, columns 0 unused (1)"""
    x = np.asarray(x, np.float32).astype(dtype).reshape(-1)
    F = frames(x.shape[0])
    _, tmax = lags(rate)
    if F == 0:
        return np.ones((0, tmax + 2), dtype)
    xp = np.pad(x, FRAME // 2, mode="reflect")
    fr = xp[HOP * np.arange(F)[:, None] + np.arange(FRAME)[None, :]]
    d = np.zeros((F, tmax + 1), dtype)  # tau = 1 .. tmax + 1
    for j in range(W):  # ascending j, one accumulator per lag, as the device sums
        df = fr[:, j:j + 1] - fr[:, j + 1:j + tmax + 2]
        d = d + df * df
    cs = np.cumsum(d, axis=1, dtype=dtype)
    tau = np.arange(1, tmax + 2).astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        dn = np.where(cs == 0, dtype(1), (d * tau[None, :]) / cs)
    return np.concatenate([np.ones((F, 1), dtype), dn.astype(dtype)], axis=1)


def decide(dn, rate):
    """d' [F, tau_max + 2] -> (cents int64 [F], margin float64 [F]): the decision of every row and its smallest |d' - 0.15| examined"""
    tmin, tmax = lags(rate)
    F = dn.shape[0]
    cents = np.zeros(F, np.int64)
    margin = np.zeros(F, np.float64)
    thr = dn.dtype.type(THRESHOLD)
    for f in range(F):
        row = dn[f]
        under = np.nonzero(row[tmin:tmax + 1] < thr)[0]
        if not len(under):
            margin[f] = float(np.abs(row[tmin:tmax + 1].astype(np.float64) - THRESHOLD).min())
            continue
        t = tmin + int(under[0])
        margin[f] = float(np.abs(row[tmin:t + 1].astype(np.float64) - THRESHOLD).min())
        while t + 1 <= tmax and row[t + 1] < row[t]:
            t += 1
        y0, y1, y2 = float(row[t - 1]), float(row[t]), float(row[t + 1])
        curv = y0 - 2.0 * y1 + y2
        off = 0.0
        if curv > 0.0:
            off = min(0.5, max(-0.5, (y0 - y2) / (2.0 * curv)))
        cents[f] = int(math.floor(1200.0 * math.log2(float(rate) / (t + off) / REF_HZ) + 0.5))
    return cents, margin


def track(x, rate, dtype=np.float64, report=None):
    """ONE item -> cents int64 [1 + len // H] (zeros below n/2 + 1 samples).  report: margin [F], dn"""
    x = np.asarray(x, np.float32).reshape(-1)
    dn = normalised_difference(x, rate, dtype)
    cents, margin = decide(dn, rate)
    if report is not None:
        report.update(dn=dn, margin=margin)
    out = np.zeros(contour_ref.frames(x.shape[0]), np.int64)
    out[:cents.shape[0]] = cents
    return out


def track_figures(x, rate):
    """the float64 and float32 tracks of one item with what the GPU test's exclusion rule needs:
    -> dict(c64, c32, margin (float64 decision margins), yardstick (largest |d'_32 - d'_64| of the item))"""
    r64, r32 = {}, {}
    c64 = track(x, rate, np.float64, r64)
    c32 = track(x, rate, np.float32, r32)
    F = r64["dn"].shape[0]
    yard = float(np.abs(r32["dn"].astype(np.float64) - r64["dn"]).max()) if F else 0.0
    margin = np.full(c64.shape[0], np.inf)
    margin[:F] = r64["margin"]
    return dict(c64=c64, c32=c32, margin=margin, yardstick=yard)


def rha(a, b):
    """round half away from zero of a / b for integer arrays, b > 0"""
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    return np.sign(a) * ((2 * np.abs(a) + b) // (2 * b))


def offsets(cents, r_m):
    """cents int [F] (0: unvoiced) -> o int64 [F] in [-1200, 1200]"""
    cents = np.asarray(cents, np.int64)
    F = cents.shape[0]
    v = np.nonzero(cents > 0)[0]
    if not len(v):
        return np.zeros(F, np.int64)
    c_med = int(np.sort(cents[v])[(len(v) - 1) // 2])
    ov = rha((int(r_m) - 1000) * (cents[v] - c_med), 1000)
    f = np.arange(F)
    r = np.searchsorted(v, f, side="left")  # the first voiced row >= f
    li = np.clip(r - 1, 0, len(v) - 1)
    gi = np.clip(r, 0, len(v) - 1)
    l, g = v[li], v[gi]
    ol, og = ov[li], ov[gi]
    between = (r > 0) & (r < len(v)) & (g != f)
    o = np.where(r == 0, og, ol)  # held before the first voiced row and behind the last
    o = np.where(g == f, og, o)
    den = np.where(between, g - l, 1)
    o = np.where(between, ol + rha((og - ol) * (f - l), den), o)
    return np.clip(o, -MAX_CENTS, MAX_CENTS)


def row_tokens(length, cum, tok_len, hop, P_tok, g_tok):
    """the contour stage's token ratio and gain of every row: -> P int64 [F], g float64 [F]"""
    F = contour_ref.frames(length)
    tok_len = int(tok_len)
    if tok_len <= 0:
        return np.full(F, 1000, np.int64), np.ones(F, np.float64)
    ends = np.asarray(cum, np.int64)[:tok_len] * int(hop)
    pos = np.minimum(np.arange(F, dtype=np.int64) * HOP, max(int(length) - 1, 0))
    tok = np.searchsorted(ends, pos, side="right")
    have = tok < tok_len
    tc = np.minimum(tok, tok_len - 1)
    P = np.where(have, np.asarray(P_tok, np.int64)[:tok_len][tc], 1000)
    g = np.where(have, np.asarray(g_tok, np.float32)[:tok_len][tc].astype(np.float64), 1.0)
    return P, g


def row_of(length):
    """the analysis row whose offset row f takes: the one that holds the sample min(f H, len - 1) by which the contour stage finds the row's
    token (f itself, except the last row of a length that is a multiple of H)"""
    F = contour_ref.frames(length)
    return np.minimum(np.arange(F, dtype=np.int64) * HOP, max(int(length) - 1, 0)) // HOP


def frame_ratios(P_row, o):
    return np.clip((np.asarray(P_row, np.int64) * TAB[np.asarray(o, np.int64) + MAX_CENTS] + 500) // 1000, 500, 2000)


def tracks(Pf, gf):
    """Sigma int64 [F], gbar float32 [F + 1] from the per-row ratios and gains (contour_ref.tracks behind its token lookup)"""
    F = Pf.shape[0]
    Sigma = np.zeros(F, np.int64)
    gsum = np.zeros(F, np.float64)
    for j in range(-contour_ref.RAMP, contour_ref.RAMP + 1):
        idx = np.clip(np.arange(F) + j, 0, F - 1)
        Sigma += Pf[idx]
        gsum = gsum + gf[idx]
    gbar = (gsum / float(contour_ref.K)).astype(np.float32)
    return Sigma, np.concatenate([gbar, gbar[-1:]])


def intonation(x, rate, pitch_range, cum=None, tok_len=0, hop=HOP, semitones=None, gain_db=None, add_semitones=0.0, dtype=np.float64,
               cents=None, report=None):
    """ONE item: x [len] -> y dtype [len].  cents: a track to use in place of this restatement's own (the device's, in the GPU tests)"""
    x = np.asarray(x, np.float32).reshape(-1)
    length = x.shape[0]
    r_m = range_milli(pitch_range)
    tok_len = int(tok_len)
    s_tok = (np.zeros(tok_len) if semitones is None else np.asarray(semitones, np.float64)[:tok_len]) + float(add_semitones)
    P_tok = contour_ref.token_ratios(s_tok)
    g_tok = contour_ref.token_gains(np.zeros(tok_len) if gain_db is None else np.asarray(gain_db)[:tok_len])
    if length == 0:
        return np.zeros(0, dtype)
    if cents is None:
        cents = track(x, rate, dtype)
    cents = np.asarray(cents, np.int64)[:contour_ref.frames(length)]
    o = offsets(cents, r_m) if length >= MIN_LEN else np.zeros(cents.shape[0], np.int64)
    P_row, g_row = row_tokens(length, cum, tok_len, hop, P_tok, g_tok)
    Pf = frame_ratios(P_row, o[row_of(length)])
    Sigma, gbar = tracks(Pf, g_row)
    G = contour_ref.gain_curve(gbar, length)
    shifted = bool((Pf != 1000).any()) and length >= MIN_LEN
    if report is not None:
        report.update(cents=cents, o=o, Pf=Pf, Sigma=Sigma, gbar=gbar, shifted=shifted)
    if not shifted:
        return (G.astype(np.float64) * x.astype(np.float64)).astype(np.float32).astype(dtype)
    a, Fs = contour_ref.positions(Sigma, pitch_ref.frames_a(length))
    u = contour_ref.stretch(x, a, Fs, dtype)
    v = contour_ref.warp(u, a, Fs, length, dtype)
    if report is not None:
        report.update(a=a, Fs=Fs, u=u, v=v)
    return G.astype(dtype) * v


# ---- the test signals ------------------------------------------------------------------------------------------------------------------
def glide(n=12288, rate=22050, f_lo=120.0, f_hi=200.0, seed=0):
    """24 harmonics 1/h gliding linearly from f_lo to f_hi, a 1e-3 noise floor, and 0.02 * randn alone from 0.4 n to 0.5 n; float32 [n]"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    f = f_lo + (f_hi - f_lo) * np.arange(n) / n
    ph = 2 * np.pi * np.cumsum(f) / rate
    x = np.zeros(n)
    for h in range(1, 25):
        x += np.sin(h * ph + rng.uniform(0, 2 * np.pi)) / h
    x = 0.28 * x / np.abs(x).max() + 1e-3 * rng.standard_normal(n)
    a, b = int(0.4 * n), int(0.5 * n)
    x[a:b] = 0.02 * rng.standard_normal(b - a)
    del t
    return x.astype(np.float32)


def noise(n, seed=0):
    return (0.2 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def hz(cents):
    """cents int [F] -> Hz float64, 0 where unvoiced"""
    c = np.asarray(cents, np.float64)
    return np.where(c > 0, REF_HZ * 2.0 ** (c / 1200.0), 0.0)


def slope(x, y, rate, skip):
    """the regression slope of the output's tracked deviation (cents about its median) on the input's, over the rows voiced in both that
    `skip` (bool [F]) does not leave out; -> (slope, largest |output deviation| in cents)"""
    cx, cy = track(x, rate), track(y, rate)
    keep = (cx > 0) & (cy > 0) & ~skip
    dx = cx[keep] - np.median(cx[keep])
    dy = cy[keep] - np.median(cy[keep])
    return float((dx * dy).sum() / (dx * dx).sum()), float(np.abs(dy).max())


def glide_skip(n):
    """rows of glide(n) the slope leaves out: 6 at each end and 5 either side of the noise stretch"""
    F = contour_ref.frames(n)
    f = np.arange(F)
    lo, hi = int(0.4 * n), int(0.5 * n)
    # a row's frame covers samples [f H - n/2, f H + n/2) of the item
    touches = (f * HOP + FRAME // 2 > lo) & (f * HOP - FRAME // 2 < hi)
    idx = np.nonzero(touches)[0]
    skip = (f < 6) | (f >= F - 6)
    skip[max(idx[0] - 5, 0):idx[-1] + 6] = True
    return skip


# ---- the inputs of tests/test_intonation_gpu.py (tests/test_intonation.py checks their decision margins on the CPU) ---------------------
GPU_RATE = 22050


def gpu_cases():
    """name -> list of items (float32 arrays; an empty array is an empty item)"""
    return {
        "513": [pitch_ref.voiced(8192, seed=1)[500:500 + MIN_LEN]],  # (two voiced rows a cent apart: it is shifted at r = 4)
        "1024": [pitch_ref.voiced(8192, seed=1)[1000:1000 + 1024]],
        "ragged": [pitch_ref.voiced(4352, seed=0), noise(2048, seed=3), np.zeros(0, np.float32), pitch_ref.voiced(8192, seed=1)[:769]],
        "glide": [glide(8192)],
    }
