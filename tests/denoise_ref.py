"""float64 restatement of the vocoder-bias denoiser (include/vits_denoise.h), the definition the device kernels are checked against.

filter_length n (a power of two), hop = n / 4, window w[i] = sin^2(pi i / n) (the periodic Hann), win_length = n.  For x[0 .. len):
  1. reflect-pad n/2 on both sides (needs len >= n/2 + 1)
  2. F = 1 + len // hop frames, frame f = xp[f hop .. f hop + n) * w, X_f = rFFT(frame f)           (n/2 + 1 bins)
  3. X'_f[k] = X_f[k] * max(|X_f[k]| - strength * bias[k], 0) / |X_f[k]|, and 0 where |X_f[k]| = 0
  4. y_f = irFFT(X'_f) * w, overlap-added, divided by the overlap-added w^2, n/2 dropped from both ends: hop * (F - 1) samples
bias[k] = |X_0[k]| of the vocoder's output for an all-zero mel.  Plain numpy, no torch: tests/test_denoise.py holds the comparison
with torch.stft / torch.istft."""
import numpy as np


def window(n):
    return np.sin(np.pi * np.arange(n, dtype=np.float64) / n) ** 2


def check_filter_length(n):
    n = int(n)
    if n < 64 or n > 1024 or n & (n - 1):
        raise ValueError(f"filter_length {n}: must be a power of two in [64, 1024]")
    return n


def out_length(length, n=1024):
    hop = n // 4
    return hop * (int(length) // hop)


def frames(x, n):
    """the windowed frames [F, n] of the reflect-padded signal"""
    x = np.asarray(x, np.float64).reshape(-1)
    hop = n // 4
    if x.shape[0] < n // 2 + 1:
        raise ValueError(f"{x.shape[0]} samples: reflect padding needs at least n/2 + 1 = {n // 2 + 1}")
    xp = np.pad(x, n // 2, mode="reflect")
    F = 1 + x.shape[0] // hop
    idx = hop * np.arange(F)[:, None] + np.arange(n)[None, :]
    return xp[idx] * window(n)[None, :]


def bias_of(audio, n=1024):
    """|rFFT| of frame 0 (the frame centred on sample 0) of `audio`: float64 [n/2 + 1]"""
    n = check_filter_length(n)
    return np.abs(np.fft.rfft(frames(audio, n)[0]))


def gain(X, bias, strength):
    """step 3; also returns the share of bins clamped to zero"""
    mag = np.abs(X)
    new = np.maximum(mag - float(strength) * np.asarray(bias, np.float64)[None, :], 0.0)
    g = np.divide(new, mag, out=np.zeros_like(mag), where=mag > 0)
    return X * g, float(np.mean(new == 0.0))


def denoise(x, bias, strength, n=1024, return_clamped=False):
    """x float [len] -> float64 [hop * (len // hop)]"""
    n = check_filter_length(n)
    if strength < 0:
        raise ValueError(f"strength {strength}: must be >= 0")
    hop = n // 4
    w = window(n)
    X = np.fft.rfft(frames(x, n), axis=1)
    X, clamped = gain(X, bias, strength)
    y = np.fft.irfft(X, n=n, axis=1) * w[None, :]
    F = y.shape[0]
    total = hop * (F - 1) + n
    acc = np.zeros(total)
    env = np.zeros(total)
    for f in range(F):
        acc[f * hop:f * hop + n] += y[f]
        env[f * hop:f * hop + n] += w * w
    keep = slice(n // 2, n // 2 + hop * (F - 1))  # (the overlap-added w^2 is positive on all of it: at least three frames cover a sample)
    out = acc[keep] / env[keep]
    return (out, clamped) if return_clamped else out
