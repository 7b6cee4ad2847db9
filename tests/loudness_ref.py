"""float64 restatement of include/vits_loudness.h (ITU-R BS.1770 K-weighting, gated integrated loudness, peak, gain) -- the reference
the loudness tests compare the library with -- and the signals those tests use.  Nothing here imports the package."""
import math

import numpy as np

RATES = (8000, 16000, 22050, 44100, 48000)
MIN_RATE = 4000
LUFS, PEAK = 1, 2
# ITU-R BS.1770-4, table 1 and table 2 (48 kHz): stage 1 b0 b1 b2 a1 a2, stage 2 a1 a2
BS1770_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
              -1.99004745483398, 0.99007225036621)


def hop(rate):
    return (int(rate) + 5) // 10


def sos(rate):
    """float64 [2, 6]: rows of b0 b1 b2 1 a1 a2"""
    out = np.zeros((2, 6))
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    out[0] = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
              1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / rate)
    a0 = 1.0 + K / Q + K * K
    out[1] = [1.0, -2.0, 1.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return out


def kweight(x, rate):
    """x float [..., n] -> the K-weighted signal in float64: the two biquads in cascade, zero initial state, coefficients rounded once
    to fp32 as the definition says, every operation in float64.  scipy.signal.lfilter where scipy is present, else the same recurrence
    (transposed direct form II) over time, vectorised over the leading axes."""
    y = np.asarray(x, np.float64)
    c = sos(rate).astype(np.float32).astype(np.float64)
    try:
        from scipy.signal import lfilter
    except ImportError:
        lfilter = None
    for b0, b1, b2, _, a1, a2 in c:
        if lfilter is not None:
            y = lfilter([b0, b1, b2], [1.0, a1, a2], y, axis=-1)
            continue
        out = np.empty_like(y)
        s1 = np.zeros(y.shape[:-1])
        s2 = np.zeros(y.shape[:-1])
        for n in range(y.shape[-1]):
            v = y[..., n]
            o = b0 * v + s1
            s1 = b1 * v - a1 * o + s2
            s2 = b2 * v - a2 * o
            out[..., n] = o
        y = out
    return y


def blocks(x, rate):
    """z_j of one item x [len] (float64 [n_blocks])"""
    x = np.asarray(x, np.float64).reshape(-1)
    n, h = x.shape[0], hop(rate)
    if n == 0:
        return np.zeros(0)
    q = kweight(x, rate) ** 2
    nh = n // h
    if nh < 4:
        return np.array([q.sum() / n])
    E = q[:nh * h].reshape(nh, h).sum(axis=1)
    return (E[:-3] + E[1:-2] + E[2:-1] + E[3:]) / (4.0 * h)


def _l(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def integrated(x, rate, details=False):
    """L of one item (-inf for silence or no block); details: (L, l_j, Gamma)"""
    z = blocks(x, rate)
    l = _l(z) if z.size else np.zeros(0)
    ja = l > -70.0
    if not ja.any():
        return (-math.inf, l, None) if details else -math.inf
    gamma = -0.691 + 10.0 * math.log10(z[ja].mean()) - 10.0
    j = ja & (l > gamma)
    L = -0.691 + 10.0 * math.log10(z[j].mean())
    return (L, l, gamma) if details else L


def gate_margin(x, rate):
    """the least distance in LU of any block's l_j from -70 or from Gamma (inf where there is no such block / no Gamma)"""
    _, l, gamma = integrated(x, rate, details=True)
    l = l[np.isfinite(l)]
    if l.size == 0:
        return math.inf
    m = np.abs(l + 70.0).min()
    if gamma is not None:
        m = min(m, np.abs(l - gamma).min())
    return float(m)


def peak(x):
    x = np.asarray(x).reshape(-1)
    return float(np.abs(x).max()) if x.size else 0.0


def gain(L, pk, mode, target, ceiling=0.0):
    if mode == LUFS:
        g = 1.0 if L == -math.inf else 10.0 ** ((target - L) / 20.0)
        if ceiling > 0 and g * pk > ceiling:
            g = ceiling / pk
        return g
    return target / pk if pk > 0 else 1.0


# ---- signals ------------------------------------------------------------------------------------------------------------------------
def sine(rate, n, amp=0.1, freq=1000.0):
    return amp * np.sin(2.0 * np.pi * freq * np.arange(n) / rate)


def enveloped_noise(rate, n, seed=1):
    t = np.arange(n) / rate
    return 0.3 * (0.6 + 0.4 * np.sin(2.0 * np.pi * 0.7 * t)) * np.random.default_rng(seed).uniform(-1.0, 1.0, n)


def gated_sequence(rate, n):
    """a 440 Hz tone whose amplitude changes per 100 ms hop: loud, quiet, four hops at 1e-5, one hop of exact zeros, repeating.  Blocks made
    of the 1e-5 hops fail the absolute gate, blocks led by the quiet hop the relative one."""
    amps = np.array([0.5, 0.01, 1e-5, 1e-5, 1e-5, 1e-5, 0.0])
    h = hop(rate)
    a = amps[(np.arange(n) // h) % amps.shape[0]]
    return a * np.sin(2.0 * np.pi * 440.0 * np.arange(n) / rate)


def dc_step_tone(rate, n):
    """0.5 DC from sample 0 plus a 30 Hz tone: the high-pass stage's transient is longest here"""
    return 0.5 + 0.25 * np.sin(2.0 * np.pi * 30.0 * np.arange(n) / rate)


SIGNALS = (("sine", sine), ("noise", enveloped_noise), ("gated", gated_sequence), ("dc30", dc_step_tone))


def op_lengths(rate, tile):
    h = hop(rate)
    return [0, 1, h - 1, 4 * h - 1, 4 * h, 4 * h + 1, 7 * h + 3, tile - 1, tile + 1, 3 * tile + 17]


def op_batch(rate, tile):
    """The ragged batch of the kernel-level GPU test at `rate`: every signal at every length of op_lengths, plus one all-zero item.
    -> (x float32 [B, N] with NaN at and beyond each length, lengths int64 [B], names)"""
    lens, names, rows = [], [], []
    for name, fn in SIGNALS:
        for n in op_lengths(rate, tile):
            rows.append(fn(rate, n).astype(np.float32))
            lens.append(n)
            names.append(f"{name}/{n}")
    rows.append(np.zeros(5 * hop(rate), np.float32))
    lens.append(5 * hop(rate))
    names.append("zeros")
    N = max(lens)
    x = np.full((len(rows), N), np.nan, np.float32)
    for b, r in enumerate(rows):
        x[b, :r.shape[0]] = r
    return x, np.array(lens, np.int64), names


def normalize_batch(rate, tile):
    """The batch of the normalisation test: the four signals at 3 * tile + 17 samples, one short item and one all-zero item"""
    n = 3 * tile + 17
    rows = [fn(rate, n).astype(np.float32) for _, fn in SIGNALS] + [sine(rate, hop(rate) - 1).astype(np.float32), np.zeros(n, np.float32)]
    lens = [r.shape[0] for r in rows]
    x = np.full((len(rows), n), np.nan, np.float32)
    for b, r in enumerate(rows):
        x[b, :r.shape[0]] = r
    return x, np.array(lens, np.int64)
