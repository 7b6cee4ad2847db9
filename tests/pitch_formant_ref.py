"""Restatement of the formant-preserving pitch shift, steps 3a-3d of include/vits_pitch.h (VITS_FLAG_PITCH_FORMANT), on top of
tests/pitch_ref.py: the analysis, the phase recursion, the resampler, the plan and the GPU items are that module's.  numpy only.

`dtype` is the working precision, as there: float64 is the reference the device is checked against, float32 the yardstick -- in it
every operation of 3a-3d (the logarithm, the differences, the sums, the division of the angle, the cosine, the exponential) is a
float32 operation; only the n-entry cosine table is a constant formed in double and rounded once, like pitch_ref's window.

For every analysis row f < F_a (C = 40, floor = 1e-4, g_max = 30 dB in nepers, n = 1024):
  3a  L[k] = ln(max(mag[k], floor)), k = 0 .. n/2
  3b  c[q] = (D[0] + (-1)^q D[n/2] + 2 sum_{k=1}^{n/2-1} D[k] tab[(k q) mod n]) / n, q = 0 .. C, D = L - L[0], tab[j] = cos(2 pi j / n)
  3c  e(k) = c[0] + 2 sum_{q=1}^{C} c[q] tab[(k q) mod n];  e(kappa_k) the same with cos(pi * (2 r / (Q n))), r = (k P q) mod (Q n),
      and with (-1)^q where k P >= (n/2) Q (kappa_k = min(k P / Q, n/2))
  3d  g[k] = exp(clamp(e(kappa_k) - e(k), -g_max, g_max)); mag'[k] = mag[k] g[k]
The phases come from the unscaled mag (they are pitch_ref.stretch's); step 4 takes m'_t = (1 - alpha_t) mag'_i + alpha_t mag'_(i+1).
"""
import numpy as np

import pitch_ref as R

LIFTER = 40
LOG_FLOOR = 1e-4
MAX_DB = 30.0
G_MAX = MAX_DB * np.log(10.0) / 20.0


def kappa_clamped(P, Q):
    """bool [NB]: the bins whose shifted position is clamped to n/2"""
    k = np.arange(R.NB, dtype=np.int64)
    return k * P >= (R.FRAME // 2) * Q


def gains(mag, P, Q, dtype=np.float64):
    """mag [F, NB] (or [NB]) -> g of the same shape, every operation in `dtype`"""
    mag = np.asarray(mag, dtype)
    one = mag.ndim == 1
    mag = np.atleast_2d(mag)
    n, h, C = R.FRAME, R.FRAME // 2, LIFTER
    tab = np.cos(2.0 * np.pi * np.arange(n) / n).astype(dtype)
    L = np.log(np.maximum(mag, dtype(LOG_FLOOR)))
    D = L - L[:, :1]
    k = np.arange(R.NB, dtype=np.int64)
    q = np.arange(C + 1, dtype=np.int64)
    sign = np.where(q % 2 == 1, dtype(-1), dtype(1))
    s = D[:, 1:h] @ tab[(k[1:h, None] * q[None, :]) % n]  # [F, C + 1]: products and sums in dtype
    c = (D[:, :1] + sign[None, :] * D[:, h:h + 1] + dtype(2) * s) / dtype(n)
    ek = c[:, :1] + dtype(2) * (c[:, 1:] @ tab[(q[1:, None] * k[None, :]) % n])
    qn = Q * n
    r = (k[None, :] * P * q[1:, None]) % qn  # [C, NB], integers
    cx = np.cos(dtype(np.pi) * ((2 * r).astype(dtype) / dtype(qn)))
    cx = np.where(kappa_clamped(P, Q)[None, :], sign[1:, None], cx).astype(dtype)
    ex = c[:, :1] + dtype(2) * (c[:, 1:] @ cx)
    g = np.exp(np.clip(ex - ek, dtype(-G_MAX), dtype(G_MAX)))
    assert g.dtype == dtype
    return g[0] if one else g


def stretch_formant(x, P, Q, dtype=np.float64, report=None):
    """steps 1-4 with 3a-3d -> u dtype [N_u].  report (a dict) receives pitch_ref.stretch's entries (phi among them: the plain call's),
    and gain [F_a, NB], magf [F_a + 2, NB], mf [F_s, NB]"""
    x = np.asarray(x, dtype).reshape(-1)
    rep = {}
    R.stretch(x, P, Q, dtype, rep)
    mag, phi_all = rep["mag"], rep["phi"]
    Fa, Fs = R.frames_a(x.shape[0]), R.frames_s(x.shape[0], P, Q)
    g = gains(mag[:Fa], P, Q, dtype)
    magf = np.zeros_like(mag)
    magf[:Fa] = mag[:Fa] * g
    m_all = np.zeros((Fs, R.NB), dtype)
    for t in range(Fs):
        i, r = (t * Q) // P, (t * Q) % P
        alpha = dtype(r) / dtype(P)
        m_all[t] = (dtype(1) - alpha) * magf[i] + alpha * magf[i + 1]
    # step 4, as pitch_ref.stretch has it
    turn = phi_all.astype(np.int32).astype(dtype) * dtype(2.0 ** -32)
    ang = dtype(2.0 * np.pi) * turn
    Y = (m_all * np.cos(ang)).astype(dtype) + 1j * (m_all * np.sin(ang)).astype(dtype)
    Y[:, 0] = Y[:, 0].real
    Y[:, -1] = Y[:, -1].real
    w64 = R.window()
    y = np.fft.irfft(Y, n=R.FRAME, axis=1).astype(dtype) * w64.astype(dtype)[None, :]
    total = R.HOP * (Fs - 1) + R.FRAME
    acc = np.zeros(total, dtype)
    env = np.zeros(total, np.float64)
    for f in range(Fs):
        acc[f * R.HOP:f * R.HOP + R.FRAME] += y[f]
        env[f * R.HOP:f * R.HOP + R.FRAME] += w64 * w64
    keep = slice(R.FRAME // 2, R.FRAME // 2 + R.HOP * (Fs - 1))
    u = acc[keep] * (1.0 / env[keep]).astype(dtype)
    if report is not None:
        report.update(rep, gain=g, magf=magf, mf=m_all)
    return u


def pitch_shift_formant(x, semitones, dtype=np.float64, report=None):
    """x [len] -> y dtype [len]"""
    x = np.asarray(x, dtype).reshape(-1)
    P, Q = R.plan(semitones)
    if P == Q or x.shape[0] < R.MIN_LEN:
        return x.copy()
    u = stretch_formant(x, P, Q, dtype, report)
    v = R.resample(u, P, Q, dtype)
    y = np.zeros(x.shape[0], dtype)
    c = min(x.shape[0], v.shape[0])
    y[:c] = v[:c]
    return y


def gain_rows(N):
    """rows of vits_op_pitch_formant_gain for items of at most N samples"""
    return N // R.HOP + 3


# ---- the synthetic vowel of the CPU test: three formants over harmonics of f0 ---------------------------------------------------------
FORMANTS = ((700.0, 80.0), (1300.0, 90.0), (2700.0, 150.0))


def formant_curve(f):
    f = np.asarray(f, np.float64)
    return sum(1.0 / (1.0 + ((f - F) / B) ** 2) for F, B in FORMANTS) + 0.02


def vowel(f0=110.0, n=16384, rate=22050, seed=1):
    """-> (x float32 [n] at peak 0.3, the scale sc that brought it there)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    x = np.zeros(n)
    h = 1
    while h * f0 < 5000:
        x += formant_curve(h * f0) * np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 2 * np.pi))
        h += 1
    sc = 0.3 / np.abs(x).max()
    return (sc * x).astype(np.float32), sc


def envelope_deviation(y, P, Q, sc, f0=110.0, rate=22050):
    """mean |err - median(err)| in dB of the harmonic amplitudes of a shifted vowel() against the formant curve at their new places"""
    y = np.asarray(y, np.float64)
    S = np.abs(np.fft.rfft(y[2048:10240] * np.hanning(8192))) / 2048
    err = []
    h = 1
    while h * f0 * P / Q < 4000:
        f = h * f0 * P / Q
        b = int(round(f * 8192 / rate))
        err.append(20 * np.log10(S[b - 3:b + 4].max() / (sc * formant_curve(f))))
        h += 1
    err = np.array(err)
    return float(np.mean(np.abs(err - np.median(err))))
