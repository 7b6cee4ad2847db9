"""Restatement of the pitch shifter defined in include/vits_pitch.h: an identity-phase-locked vocoder (Laroche & Dolson 1999) that
stretches the waveform by P/Q, then the resampler of include/vits_resample.h (P -> Q) that brings it back to its length.  numpy only.

`dtype` is the working precision: float64 is the reference the device is checked against, float32 the yardstick that says how far an
fp32 implementation of the same definition may sit from it.  The phases are 32-bit fixed-point turns in both: every phase operation
after the analysis is a wrapping unsigned addition, exact and associative, the same here and on the device.

  ratio     P0 = lround(1000 * 2^(s/12)), Q0 = 1000, reduced by their gcd; |s| <= 12; P == Q is the identity
  geometry  n = 1024, H = 256, w[i] = sin^2(pi i / n), NB = 513
  1 analysis   reflect-pad n/2, F_a = 1 + len // H frames, X_f = rFFT(frame f * w); mag_f = sqrt(re^2 + im^2),
               theta_f = low 32 bits of rint(atan2(im, re) / 2 pi * 2^32), atan2(0, 0) = 0; rows f >= F_a are zero
  2 steps      F_s = ceil((F_a + 1) P / Q); i_t = (t Q) // P, alpha_t = ((t Q) mod P) / P (one division in `dtype`);
               m_t = (1 - alpha_t) mag_i + alpha_t mag_(i+1)
  3 phase      Phi_0 = theta_0; t >= 1, j = i_(t-1), i = i_t: adv = Phi_(t-1) + theta_(j+1) - theta_j;
               k is a peak of m_t iff m[k] > m[k-1], m[k] > m[k-2], m[k] >= m[k+1], m[k] >= m[k+2] (outside [0, NB): -1);
               own(k) = the nearest peak, the lower one on a tie; Phi_t[k] = adv[own(k)] + theta_i[k] - theta_i[own(k)]
  4 synthesis  turn = int32(Phi) * 2^-32; Y = m (cos 2 pi turn, sin 2 pi turn), imaginary parts of bins 0 and n/2 dropped;
               y = irFFT(Y) * w, overlap-added at H, times 1 / (overlap-added w^2) (formed in double, rounded once), n/2 dropped from
               both ends: N_u = H (F_s - 1) samples
  5 resample   tests/resample_ref.py with rate_in = P, rate_out = Q: N_v = ceil(N_u Q / P)
  6 output     y[n] = v[n] for n < min(len, N_v), 0 up to len.  An item shorter than n/2 + 1 is returned as it is.
"""
import math

import numpy as np

import resample_ref

FRAME = 1024
HOP = FRAME // 4
NB = FRAME // 2 + 1
MAX_SEMITONES = 12.0
MIN_LEN = FRAME // 2 + 1


def plan(semitones):
    """-> (P, Q); ValueError names a refused value"""
    s = float(semitones)
    if not abs(s) <= MAX_SEMITONES:  # (NaN fails the comparison)
        raise ValueError(f"pitch {s} semitones outside [-{MAX_SEMITONES:g}, {MAX_SEMITONES:g}]")
    p0 = int(math.floor(1000.0 * 2.0 ** (s / 12.0) + 0.5))  # lround of a positive value
    g = math.gcd(p0, 1000)
    return p0 // g, 1000 // g


def window():
    return np.sin(np.pi * np.arange(FRAME, dtype=np.float64) / FRAME) ** 2


def frames_a(length):
    return 1 + int(length) // HOP if length >= MIN_LEN else 0


def frames_s(length, P, Q):
    return -(-(frames_a(length) + 1) * P // Q)


def n_u(length, P, Q):
    return HOP * (frames_s(length, P, Q) - 1)


def n_v(length, P, Q):
    return -(-n_u(length, P, Q) * Q // P)


def stretch_samples(N, P, Q):
    """row length of vits_op_pitch_stretch for items of at most N samples"""
    return HOP * (-(-(N // HOP + 2) * P // Q) - 1)


def analysis(x, dtype):
    """-> mag dtype [F_a + 2, NB], theta uint32 [F_a + 2, NB]"""
    x = np.asarray(x, dtype).reshape(-1)
    Fa = frames_a(x.shape[0])
    xp = np.pad(x, FRAME // 2, mode="reflect")
    idx = HOP * np.arange(Fa)[:, None] + np.arange(FRAME)[None, :]
    X = np.fft.rfft(xp[idx] * window().astype(dtype)[None, :], axis=1)
    re, im = X.real.astype(dtype), X.imag.astype(dtype)
    mag = np.zeros((Fa + 2, NB), dtype)
    theta = np.zeros((Fa + 2, NB), np.uint32)
    mag[:Fa] = np.sqrt(re * re + im * im)
    t = np.arctan2(im, re) / dtype(2.0 * np.pi)
    t = np.where((re == 0) & (im == 0), dtype(0), t)
    theta[:Fa] = (np.rint(t.astype(np.float64) * 2.0 ** 32).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)  # (* 2^32 is exact)
    return mag, theta


def peaks_of(m):
    e = np.concatenate([[-1.0, -1.0], np.asarray(m, np.float64), [-1.0, -1.0]])  # (comparisons of dtype values: exact in double)
    c = e[2:-2]
    return np.nonzero((c > e[1:-3]) & (c > e[:-4]) & (c >= e[3:-1]) & (c >= e[4:]))[0]


def owners(pk):
    """own(k) for k in [0, NB) given the ascending peak indices (at least one)"""
    k = np.arange(NB)
    r = np.searchsorted(pk, k)  # first peak >= k
    lo = pk[np.clip(r - 1, 0, len(pk) - 1)]
    hi = pk[np.clip(r, 0, len(pk) - 1)]
    use_hi = (r == 0) | ((r < len(pk)) & (hi - k < k - lo))
    return np.where(use_hi, hi, lo)


def min_gap(m):
    """smallest |m[a] - m[b]| over the comparisons of the peak test, |a - b| in {1, 2}; pairs of exact zeros (frames of exact
    silence, the same in every precision) are left out"""
    m = np.asarray(m, np.float64)
    g = np.inf
    for d in (1, 2):
        a, b = m[d:], m[:-d]
        live = (a != 0) | (b != 0)
        if live.any():
            g = min(g, float(np.abs(a - b)[live].min()))
    return g


def stretch(x, P, Q, dtype=np.float64, report=None):
    """steps 1-4 -> u dtype [N_u].  report (a dict) receives m [F_s, NB], phi uint32 [F_s, NB], min_gap and peaks (a count)"""
    x = np.asarray(x, dtype).reshape(-1)
    if x.shape[0] < MIN_LEN:
        raise ValueError(f"{x.shape[0]} samples: the vocoder needs at least n/2 + 1 = {MIN_LEN}")
    mag, theta = analysis(x, dtype)
    Fs = frames_s(x.shape[0], P, Q)
    m_all = np.zeros((Fs, NB), dtype)
    phi_all = np.zeros((Fs, NB), np.uint32)
    gap, n_peaks = np.inf, 0
    phi = theta[0].copy()
    for t in range(Fs):
        i, r = (t * Q) // P, (t * Q) % P
        alpha = dtype(r) / dtype(P)
        m = (dtype(1) - alpha) * mag[i] + alpha * mag[i + 1]
        if t >= 1:
            j = ((t - 1) * Q) // P
            adv = phi + theta[j + 1] - theta[j]  # uint32: wraps
            pk = peaks_of(m)
            gap = min(gap, min_gap(m))
            n_peaks += len(pk)
            if len(pk):
                own = owners(pk)
                phi = adv[own] + theta[i] - theta[i][own]
            else:
                phi = adv
        m_all[t], phi_all[t] = m, phi
    turn = phi_all.astype(np.int32).astype(dtype) * dtype(2.0 ** -32)
    ang = dtype(2.0 * np.pi) * turn
    Y = (m_all * np.cos(ang)).astype(dtype) + 1j * (m_all * np.sin(ang)).astype(dtype)
    Y[:, 0] = Y[:, 0].real
    Y[:, -1] = Y[:, -1].real
    w64 = window()
    y = np.fft.irfft(Y, n=FRAME, axis=1).astype(dtype) * w64.astype(dtype)[None, :]
    total = HOP * (Fs - 1) + FRAME
    acc = np.zeros(total, dtype)
    env = np.zeros(total, np.float64)
    for f in range(Fs):  # ascending frame order, as the device adds them
        acc[f * HOP:f * HOP + FRAME] += y[f]
        env[f * HOP:f * HOP + FRAME] += w64 * w64
    keep = slice(FRAME // 2, FRAME // 2 + HOP * (Fs - 1))
    u = acc[keep] * (1.0 / env[keep]).astype(dtype)
    if report is not None:
        report.update(m=m_all, phi=phi_all, min_gap=gap, peaks=n_peaks, mag=mag, theta=theta)
    return u


def resample(u, P, Q, dtype=np.float64):
    """step 5.  float64: straight from h; float32: the fp32-rounded phase table and an fp32 sum in tap order (the device's form)"""
    if dtype == np.float64:
        return resample_ref.resample(u, P, Q)
    pl = resample_ref.plan(P, Q)
    L, M, W, taps = pl["L"], pl["M"], pl["W"], pl["taps"]
    tab = resample_ref.table(P, Q).astype(np.float32)
    u = np.asarray(u, np.float32)
    N = resample_ref.n_out(u.shape[0], L, M)
    n = np.arange(N, dtype=np.int64)
    nm = n * M
    q, p = nm // L, nm % L
    base = q - (W - p) // L
    up = np.concatenate([u, np.zeros(1, np.float32)])
    acc = np.zeros(N, np.float32)
    for i in range(taps):
        k = base + i
        ok = (k >= 0) & (k < u.shape[0])
        acc = acc + tab[p, i] * up[np.where(ok, k, u.shape[0])]
    return acc


def pitch_shift(x, semitones, dtype=np.float64, report=None):
    """x [len] -> y dtype [len]"""
    x = np.asarray(x, dtype).reshape(-1)
    P, Q = plan(semitones)
    if P == Q or x.shape[0] < MIN_LEN:
        return x.copy()
    u = stretch(x, P, Q, dtype, report)
    v = resample(u, P, Q, dtype)
    y = np.zeros(x.shape[0], dtype)
    c = min(x.shape[0], v.shape[0])
    y[:c] = v[:c]
    return y


def voiced(n, rate=22050, seed=0, f0=140.0):
    """a synthetic voiced signal: 24 harmonics with vibrato, a noise floor and a pause of exact zeros; float32 [n], peak about 0.28"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    ph = 2 * np.pi * (f0 * t + (3.0 / (2 * np.pi * 5.0)) * np.sin(2 * np.pi * 5.0 * t))
    x = np.zeros(n)
    for h in range(1, 25):
        x += np.sin(h * ph + rng.uniform(0, 2 * np.pi)) / h
    x = 0.28 * x / np.abs(x).max() + 1e-3 * rng.standard_normal(n)
    a, b = int(0.55 * n), int(0.7 * n)
    x[a:b] = 0.0
    return x.astype(np.float32)


# ---- the inputs of tests/test_pitch_gpu.py (tests/test_pitch.py checks their peak margins on the CPU) ----------------------------------
GPU_SEMITONES = (-12.0, -4.0, 3.0, 12.0)
GPU_N = 4352
GPU_LENGTHS = (MIN_LEN, 2048, 4173)
GPU_SEED = 0


def gpu_items(seed=GPU_SEED):
    """the three ragged items of the parity test: two seeded 0.2 * randn items (the shortest the vocoder takes, and 2048 samples) and the
    voiced generator for the longest"""
    rng = np.random.default_rng(seed)
    a = (0.2 * rng.standard_normal(GPU_LENGTHS[0])).astype(np.float32)
    b = (0.2 * rng.standard_normal(GPU_LENGTHS[1])).astype(np.float32)
    return [a, b, voiced(GPU_LENGTHS[2], seed=seed)]


def sine(n=16384, f=440.0, amp=0.3, rate=22050):
    return (amp * np.sin(2 * np.pi * f * np.arange(n) / rate)).astype(np.float32)


def sine_figures(y, rate=22050):
    """(peak bin of the 8192-point Hann spectrum of the middle, RMS over [2048, -2048)) of a shifted sine()"""
    y = np.asarray(y, np.float64)
    sp = np.abs(np.fft.rfft(y[4096:4096 + 8192] * np.hanning(8192)))
    return int(np.argmax(sp)), float(np.sqrt(np.mean(y[2048:-2048] ** 2)))
