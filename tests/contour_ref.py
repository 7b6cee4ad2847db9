"""Restatement of the per-token pitch and volume contour defined in include/vits_contour.h: frame tracks from the tokens, an integer
position recurrence, the phase-locked vocoder of include/vits_pitch.h driven by it (tests/pitch_ref.py holds its pieces), a warping
windowed-sinc resampler and a gain curve.  numpy only.

`dtype` is the working precision: float64 is the reference the device is checked against, float32 the yardstick that says how far an
fp32 implementation of the same definition may sit from it.  Everything that decides WHICH rows and samples are read is integer or
double arithmetic in both: the tracks Sigma, the positions a_t, tau_n and the tap bounds.

  per token    P_t = lround(1000 * 2^(s_t / 12)), g_t = float32(10^(v_t / 20))
  tracks       F = 1 + len // H rows; tok(f) = the first t with cum[t] * hop > min(f H, len - 1), none: P = 1000, g = 1;
               Sigma_f = sum_{|j| <= R} P_tok(clamp(f + j)); gbar_f = float32(mean of g_tok(clamp(f + j)) in double); gbar_F = gbar_{F-1}
  positions    inc_f = (2^24 * 1000 * K) // Sigma_f; a_0 = 0, a_{t+1} = a_t + inc[min(a_t >> 24, F_a - 1)];
               F_s = #{t: a_t < (F_a + 1) << 24}; alpha_t = (a_t & (2^24 - 1)) * 2^-24
  vocoder      steps 1-4 of pitch_ref with i_t = a_t >> 24 and alpha_t: u[0 .. H (F_s - 1))
  warp         A = n << 16, t = the largest index with a_t <= A, d = a_{t+1} - a_t, tau = H (t + (A - a_t) / d), s = min(1, d 2^-24);
               v[n] = sum_k u[k] h_s(tau - k), ceil(tau - Z / s) <= k <= floor(tau + Z / s), ascending k; 0 where tau >= N_u;
               h_s(x) = s * lerp(T, |x| s RES), T[j] = float32(h_1(j / RES)), T[Z RES + 1] = 0
  output       G[n] = (1 - fr) gbar_f + fr gbar_{f+1} in float32 (f = n >> 8, fr = (n & 255) / 256); y[n] = G[n] v[n]
  exact cases  every P_t == 1000 in the item, or len < n/2 + 1: y = float32(G x)
"""
import math

import numpy as np

import pitch_ref
import resample_ref

FRAME = pitch_ref.FRAME
HOP = pitch_ref.HOP
NB = pitch_ref.NB
MIN_LEN = pitch_ref.MIN_LEN
RAMP = 4
K = 2 * RAMP + 1
MIN_DB, MAX_DB = -40.0, 12.0
MAX_SEMITONES = pitch_ref.MAX_SEMITONES
RES = 256
Z = resample_ref.Z
ONE = 1 << 24
MASK = ONE - 1


def token_ratios(semitones):
    """P_t int64 of an array of semitones; ValueError names a refused value"""
    s = np.asarray(semitones, np.float64)
    bad = ~(np.abs(s) <= MAX_SEMITONES)
    if bad.any():
        i = np.argwhere(bad)[0]
        raise ValueError(f"contour: {s[tuple(i)]} semitones at {tuple(int(v) for v in i)} outside [-{MAX_SEMITONES:g}, {MAX_SEMITONES:g}]")
    return np.floor(1000.0 * 2.0 ** (s / 12.0) + 0.5).astype(np.int64)


def token_gains(gain_db):
    """g_t float32 of an array of decibels; ValueError names a refused value"""
    v = np.asarray(gain_db, np.float64)
    bad = ~((v >= MIN_DB) & (v <= MAX_DB))
    if bad.any():
        i = np.argwhere(bad)[0]
        raise ValueError(f"contour: {v[tuple(i)]} dB at {tuple(int(x) for x in i)} outside [{MIN_DB:g}, {MAX_DB:g}]")
    return (10.0 ** (v / 20.0)).astype(np.float32)


def frames(length):
    return 1 + int(length) // HOP


def tracks(length, cum, tok_len, hop, P_tok, g_tok):
    """-> Sigma int64 [F], gbar float32 [F + 1] of ONE item"""
    F = frames(length)
    ends = np.asarray(cum, np.int64)[:int(tok_len)] * int(hop)
    pos = np.minimum(np.arange(F, dtype=np.int64) * HOP, max(int(length) - 1, 0))
    tok = np.searchsorted(ends, pos, side="right")  # the first t with ends[t] > pos
    have = tok < int(tok_len)
    tc = np.minimum(tok, max(int(tok_len) - 1, 0))
    if int(tok_len) > 0:
        Pf = np.where(have, np.asarray(P_tok, np.int64)[:int(tok_len)][tc], 1000)
        gf = np.where(have, np.asarray(g_tok, np.float32)[:int(tok_len)][tc].astype(np.float64), 1.0)
    else:
        Pf = np.full(F, 1000, np.int64)
        gf = np.ones(F, np.float64)
    Sigma = np.zeros(F, np.int64)
    gsum = np.zeros(F, np.float64)
    for j in range(-RAMP, RAMP + 1):  # ascending j
        idx = np.clip(np.arange(F) + j, 0, F - 1)
        Sigma += Pf[idx]
        gsum = gsum + gf[idx]
    gbar = (gsum / float(K)).astype(np.float32)
    return Sigma, np.concatenate([gbar, gbar[-1:]])


def positions(Sigma, Fa):
    """-> (a int64 [F_s + 1], F_s)"""
    inc = (ONE * 1000 * K) // np.asarray(Sigma, np.int64)
    end = (Fa + 1) << 24
    a = [0]
    while a[-1] < end:
        i = min(a[-1] >> 24, Fa - 1)
        a.append(a[-1] + int(inc[i]))
    return np.asarray(a, np.int64), len(a) - 1


def stretch(x, a, Fs, dtype=np.float64, report=None):
    """steps 1-4 of pitch_ref.stretch with the step table -> u dtype [H (F_s - 1)]"""
    x = np.asarray(x, dtype).reshape(-1)
    mag, theta = pitch_ref.analysis(x, dtype)
    m_all = np.zeros((Fs, NB), dtype)
    phi_all = np.zeros((Fs, NB), np.uint32)
    gap = np.inf
    phi = theta[0].copy()
    for t in range(Fs):
        i = int(a[t]) >> 24
        alpha = dtype(int(a[t]) & MASK) * dtype(2.0 ** -24)
        m = (dtype(1) - alpha) * mag[i] + alpha * mag[i + 1]
        if t >= 1:
            j = int(a[t - 1]) >> 24
            adv = phi + theta[j + 1] - theta[j]  # uint32: wraps
            pk = pitch_ref.peaks_of(m)
            gap = min(gap, pitch_ref.min_gap(m))
            if len(pk):
                own = pitch_ref.owners(pk)
                phi = adv[own] + theta[i] - theta[i][own]
            else:
                phi = adv
        m_all[t], phi_all[t] = m, phi
    turn = phi_all.astype(np.int32).astype(dtype) * dtype(2.0 ** -32)
    ang = dtype(2.0 * np.pi) * turn
    Y = (m_all * np.cos(ang)).astype(dtype) + 1j * (m_all * np.sin(ang)).astype(dtype)
    Y[:, 0] = Y[:, 0].real
    Y[:, -1] = Y[:, -1].real
    w64 = pitch_ref.window()
    y = np.fft.irfft(Y, n=FRAME, axis=1).astype(dtype) * w64.astype(dtype)[None, :]
    total = HOP * (Fs - 1) + FRAME
    acc = np.zeros(total, dtype)
    env = np.zeros(total, np.float64)
    for f in range(Fs):
        acc[f * HOP:f * HOP + FRAME] += y[f]
        env[f * HOP:f * HOP + FRAME] += w64 * w64
    keep = slice(FRAME // 2, FRAME // 2 + HOP * (Fs - 1))
    if report is not None:
        report.update(min_gap=gap, phi=phi_all, m=m_all)
    return acc[keep] * (1.0 / env[keep]).astype(dtype)


def h1(y):
    """h_1(y) = 0.9 sinc(0.9 y) I0(beta sqrt(1 - (y / Z)^2)) / I0(beta) in float64, 0 <= y <= Z"""
    y = np.asarray(y, np.float64)
    v = resample_ref.RHO * y
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(v == 0, 1.0, np.sin(math.pi * v) / (math.pi * v))
    r2 = np.maximum(1.0 - (y / Z) ** 2, 0.0)
    return resample_ref.RHO * sinc * resample_ref.bessel_i0(resample_ref.BETA * np.sqrt(r2)) / resample_ref.bessel_i0(resample_ref.BETA)


def filter_table():
    """T float32 [Z RES + 2]"""
    T = np.zeros(Z * RES + 2, np.float32)
    T[:Z * RES + 1] = h1(np.arange(Z * RES + 1) / float(RES)).astype(np.float32)
    return T


def warp_positions(a, Fs, length):
    """-> tau float64 [len], s float64 [len]"""
    a = np.asarray(a, np.int64)
    A = np.arange(int(length), dtype=np.int64) << 16
    t = np.searchsorted(a[:Fs + 1], A, side="right") - 1
    d = a[t + 1] - a[t]
    tau = HOP * (t.astype(np.float64) + (A - a[t]).astype(np.float64) / d.astype(np.float64))
    s = np.minimum(1.0, d.astype(np.float64) * 2.0 ** -24)
    return tau, s


def warp(u, a, Fs, length, dtype=np.float64):
    """v dtype [len]"""
    u = np.asarray(u, dtype)
    Nu = u.shape[0]
    T = filter_table()
    Tw = T.astype(dtype)
    tau, s = warp_positions(a, Fs, length)
    hw = Z / s
    klo = np.ceil(tau - hw).astype(np.int64)
    khi = np.floor(tau + hw).astype(np.int64)
    live = tau < Nu
    up = np.concatenate([u, np.zeros(1, dtype)])
    acc = np.zeros(int(length), dtype)
    sR = s * RES
    s_w = s.astype(dtype)
    for j in range(int((khi - klo).max()) + 1 if length else 0):  # ascending k
        k = klo + j
        ok = live & (k <= khi) & (k >= 0) & (k < Nu)
        p = np.abs(tau - k) * sR
        jj = np.minimum(p.astype(np.int64), Z * RES)
        fr = (p - jj).astype(dtype)
        h = s_w * (Tw[jj] + fr * (Tw[jj + 1] - Tw[jj]))
        acc = acc + np.where(ok, up[np.where(ok, k, Nu)] * h, dtype(0))
    return acc


def gain_curve(gbar, length):
    """G float32 [len]"""
    n = np.arange(int(length), dtype=np.int64)
    f = n >> 8
    fr = ((n & 255).astype(np.float32) / np.float32(256))
    gbar = np.asarray(gbar, np.float32)
    return (np.float32(1) - fr) * gbar[f] + fr * gbar[f + 1]


def contour(x, cum, tok_len, hop, semitones=None, gain_db=None, dtype=np.float64, report=None):
    """ONE item: x [len], cum int [>= tok_len], semitones / gain_db [>= tok_len] or None -> y dtype [len]"""
    x = np.asarray(x, np.float32).reshape(-1)
    length = x.shape[0]
    tok_len = int(tok_len)
    P_tok = token_ratios(np.zeros(tok_len) if semitones is None else np.asarray(semitones)[:tok_len])
    g_tok = token_gains(np.zeros(tok_len) if gain_db is None else np.asarray(gain_db)[:tok_len])
    if length == 0:
        return np.zeros(0, dtype)
    Sigma, gbar = tracks(length, cum, tok_len, hop, P_tok, g_tok)
    G = gain_curve(gbar, length)
    shifted = bool((P_tok != 1000).any()) and length >= MIN_LEN
    if report is not None:
        report.update(Sigma=Sigma, gbar=gbar, G=G, shifted=shifted)
    if not shifted:
        return (G.astype(np.float64) * x.astype(np.float64)).astype(np.float32).astype(dtype)  # one rounding: the product is exact in double
    a, Fs = positions(Sigma, pitch_ref.frames_a(length))
    u = stretch(x, a, Fs, dtype, report)
    v = warp(u, a, Fs, length, dtype)
    if report is not None:
        report.update(a=a, Fs=Fs, u=u, v=v)
    return G.astype(dtype) * v


def stretch_samples(N):
    """row length of u in vits_op_contour_stretch for items of at most N samples"""
    return HOP * (2 * (N // HOP + 2) - 1)


def steps_columns(N):
    return 2 * (N // HOP + 2) + 2


def tone(n=16384, f0=200.0, harmonics=8, rate=22050, amp=0.25):
    t = np.arange(n) / rate
    x = sum(np.sin(2 * np.pi * f0 * h * t + 0.7 * h) / h for h in range(1, harmonics + 1))
    return (amp * x / np.abs(x).max()).astype(np.float32)


def fundamental(seg, rate=22050, lo=80.0, hi=500.0):
    """the frequency of the strongest spectral peak in [lo, hi]: Hann window, 8x zero-padded FFT, parabolic interpolation"""
    seg = np.asarray(seg, np.float64)
    n = seg.shape[0]
    sp = np.abs(np.fft.rfft(seg * np.hanning(n), 8 * n))
    fq = np.arange(sp.shape[0]) * rate / (8.0 * n)
    band = np.nonzero((fq >= lo) & (fq <= hi))[0]
    k = band[np.argmax(sp[band])]
    a, b, c = np.log(sp[k - 1]), np.log(sp[k]), np.log(sp[k + 1])
    return (k + 0.5 * (a - c) / (a - 2 * b + c)) * rate / (8.0 * n)
