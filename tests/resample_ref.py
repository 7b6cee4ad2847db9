"""float64 restatement of the resampler defined in include/vits_resample.h, numpy only.

    g = gcd(rate_in, rate_out), L = rate_out / g, M = rate_in / g, s = min(1, L / M)
    N_out = ceil(len * L / M)
    y[n]  = sum_k x[k] * h(n*M/L - k)
    h(t)  = c * sinc(c*t) * I0(beta * sqrt(1 - (t/Hw)^2)) / I0(beta)   for |t| <= Hw, else 0
    c = rho * s,  Hw = Z / s,  Z = 16,  rho = 0.9,  beta = 10

Everything that decides WHICH samples a tap touches is integer arithmetic on t = num / L and Hw = W / L, W = Z * max(L, M); the
window's argument 1 - (t/Hw)^2 = (W - num)(W + num) / W^2 is formed from those integers, so the two sides of a comparison at fp32
round the same double.
"""
import math

import numpy as np

Z, RHO, BETA = 16, 0.9, 10.0
TILE = 256  # VITS_RESAMPLE_TILE: outputs of one workgroup (the tests place item lengths around its input span)
MAX_TABLE = 65536

# (rate_in, rate_out) pairs every test walks
PAIRS = [(22050, r) for r in (8000, 11025, 12000, 16000, 24000, 32000, 44100, 48000)] + [(16000, 8000)]


def bessel_i0(x):
    """I0 by its power series (all terms positive): a few ulp for 0 <= x <= beta"""
    x = np.asarray(x, np.float64)
    q = x * x / 4
    term = np.ones_like(q)
    total = np.ones_like(q)
    for k in range(1, 200):
        term = term * (q / (float(k) * k))
        total = total + term
        if np.all(term < total * 1e-18):
            break
    return total


def plan(rate_in, rate_out):
    """-> dict(L, M, W, taps, half): the geometry of include/vits_resample.h (no acceptance rules)"""
    g = math.gcd(rate_in, rate_out)
    L, M = rate_out // g, rate_in // g
    W = Z * max(L, M)
    taps = max((W - p) // L + (W + p) // L + 1 for p in range(L))
    return dict(L=L, M=M, W=W, taps=taps, half=-(-W // L))


def h_num(num, L, M):
    """h(num / L) in float64 for integer numerators `num` (array)"""
    num = np.asarray(num, np.int64)
    W = Z * max(L, M)
    s = L / M if L < M else 1.0
    c = RHO * s
    t = num.astype(np.float64) / float(L)
    v = c * t
    pv = math.pi * v
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(num == 0, 1.0, np.sin(pv) / pv)
    inside = np.abs(num) <= W
    r2 = np.where(inside, ((W - num) * (W + num)).astype(np.float64) / float(W * W), 0.0)
    w = bessel_i0(BETA * np.sqrt(r2)) / bessel_i0(BETA)
    return np.where(inside, c * sinc * w, 0.0)


def table(rate_in, rate_out):
    """the phase table [L][taps] in float64: table[p][i] = h(lo(p) - i + p/L), lo(p) = (W - p) // L"""
    P = plan(rate_in, rate_out)
    L, M, W, taps = P["L"], P["M"], P["W"], P["taps"]
    p = np.arange(L, dtype=np.int64)[:, None]
    i = np.arange(taps, dtype=np.int64)[None, :]
    lo = (W - p) // L
    return h_num((lo - i) * L + p, L, M)


def n_out(length, L, M):
    return -(-int(length) * L // M)


def resample(x, rate_in, rate_out, n_from=0, n_to=None):
    """y[n_from:n_to] of the definition for ONE signal x (1-D, zero outside), float64; straight from h, not from the table"""
    x = np.asarray(x, np.float64)
    P = plan(rate_in, rate_out)
    L, M, W = P["L"], P["M"], P["W"]
    N = n_out(x.shape[0], L, M)
    n_to = N if n_to is None else min(n_to, N)
    y = np.zeros(max(n_to - n_from, 0), np.float64)
    half = P["half"]
    xp = np.concatenate([np.zeros(half + 1), x, np.zeros(half + 1)])
    j = np.arange(-half, half + 1, dtype=np.int64)  # k = q + j
    for a in range(n_from, n_to, 4096):
        n = np.arange(a, min(a + 4096, n_to), dtype=np.int64)
        nm = n * M
        q = nm // L
        k = q[:, None] + j[None, :]
        num = nm[:, None] - k * L  # t = n*M/L - k = num / L
        kk = np.clip(k + half + 1, 0, xp.shape[0] - 1)
        valid = (k >= 0) & (k < x.shape[0])
        y[a - n_from:a - n_from + n.shape[0]] = np.sum(np.where(valid, xp[kk], 0.0) * h_num(num, L, M), axis=1)
    return y


def fp32_bound(tab32, xmax):
    """worst-case error of an fp32 sum of `taps` products against the exact one: taps * 2^-24 * max_p sum_i |table[p][i]| * max|x|"""
    t = np.abs(np.asarray(tab32, np.float64))
    return t.shape[1] * 2.0 ** -24 * t.sum(axis=1).max() * float(xmax)


def pcm16(y64, scale):
    """trunc(clip(y * scale * 32767)) as int16 (audio_float_to_int16 of the reference after `* scale`)"""
    return np.trunc(np.clip(np.asarray(y64, np.float64) * scale * 32767.0, -32767.0, 32767.0)).astype(np.int16)
