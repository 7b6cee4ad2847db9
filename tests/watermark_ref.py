"""float64 restatement of the keyed audio watermark (include/vits_watermark.h), the definition the device kernels are checked against,
and an fp32 run of the same code (dtype=np.float32: the transforms, the gains, ln and the four-bin mean in fp32; T, D, G and the score in
float64, as the header states the device's arithmetic).  Plain numpy.

Geometry: the denoiser's transform (tests/denoise_ref.py) at n = 1024, H = 256; band bins [16, 400) in 96 groups of 4; tile rows of 4
frames, 16 rows per pattern period.  Also here: the deterministic voiced test signal of tests/test_watermark*.py."""
import numpy as np

N = 1024
H = 256
M = N // 2
BIN_LO, BIN_HI = 16, 400
GROUPS = 96
ROWS = 16
OFFSETS = 128
DETECT_HOP = 128
DEFAULT_DEPTH_DB = 1.0
MAX_DEPTH_DB = 2.0
THRESHOLD = 6.0


# ---- chips (uint32 arithmetic only) -------------------------------------------------------------------------------------------
def mix(x):
    x = np.asarray(x, np.uint64) & 0xFFFFFFFF  # (uint64 with masks: no overflow warnings, the same bits as uint32)
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x.astype(np.uint32)


def chips(key):
    """c(key, q, j) as float64 [16, 96] of +1 / -1"""
    mk = np.uint64(mix(int(key) & 0xFFFFFFFF))
    idx = (GROUPS * np.arange(ROWS)[:, None] + np.arange(GROUPS)[None, :] + 1).astype(np.uint64)
    return np.where(mix(mk ^ idx) & 1, 1.0, -1.0)


def depth_arg(depth_db):
    """0 = the default; anything outside (0, 2] dB, NaN included, is refused by name -> a in double"""
    d = float(depth_db)
    if d == 0.0:
        d = DEFAULT_DEPTH_DB
    if not 0.0 < d <= MAX_DEPTH_DB:
        raise ValueError(f"watermark: depth {float(depth_db):g} dB outside (0, {MAX_DEPTH_DB:g}]")
    return 10.0 ** (d / 20.0) - 1.0


# ---- the transform -------------------------------------------------------------------------------------------------------------
def window(dtype=np.float64):
    return (np.sin(np.pi * np.arange(N, dtype=np.float64) / N) ** 2).astype(dtype)


def frames(x, hop, dtype=np.float64):
    """the windowed frames [1 + len // hop, n] of the reflect-padded signal; frame g is centred on sample g * hop"""
    x = np.asarray(x, dtype).reshape(-1)
    xp = np.pad(x, M, mode="reflect")
    F = 1 + x.shape[0] // hop
    idx = hop * np.arange(F)[:, None] + np.arange(N)[None, :]
    return xp[idx] * window(dtype)[None, :]


# ---- embed ---------------------------------------------------------------------------------------------------------------------
def embed(x, key, depth_db=0.0, dtype=np.float64):
    """x float [len] -> y [len] of `dtype`: marked on [0, H (len // H)), x from there on; an item below n/2 + 1 samples as it went in"""
    a = depth_arg(depth_db)
    x = np.asarray(x, dtype).reshape(-1)
    n_in = x.shape[0]
    if n_in < M + 1:
        return x.copy()
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    a = dtype(np.float32(a)) if dtype == np.float32 else a
    gp, gm = dtype(1.0) + a, dtype(1.0) - a
    w = window(dtype)
    X = np.fft.rfft(frames(x, H, dtype), axis=1).astype(ctype)
    F = X.shape[0]
    c = chips(key)
    g = np.ones((F, M + 1), dtype)
    q = (np.arange(F) >> 2) & (ROWS - 1)
    k = np.arange(BIN_LO, BIN_HI)
    g[:, BIN_LO:BIN_HI] = np.where(c[q][:, (k - BIN_LO) >> 2] > 0, gp, gm)
    y = np.fft.irfft(X * g, n=N, axis=1).astype(dtype) * w[None, :]
    total = H * (F - 1) + N
    acc = np.zeros(total, dtype)
    env = np.zeros(total, np.float64)
    w2 = window() ** 2
    for f in range(F):
        acc[f * H:f * H + N] += y[f]
        env[f * H:f * H + N] += w2
    keep = slice(M, M + H * (F - 1))
    out = x.copy()
    out[:H * (F - 1)] = acc[keep] * (1.0 / env[keep]).astype(dtype)
    return out


# ---- detect --------------------------------------------------------------------------------------------------------------------
def band_logs(x, dtype=np.float64):
    """Lb [F', 96] of `dtype` (steps 1 to 3); no frames for an item below n/2 + 1 samples"""
    x = np.asarray(x, dtype).reshape(-1)
    if x.shape[0] < M + 1:
        return np.zeros((0, GROUPS), dtype)
    X = np.fft.rfft(frames(x, DETECT_HOP, dtype), axis=1)
    A = np.abs(X[:, BIN_LO:BIN_HI]).astype(dtype)
    m = A.max(axis=1)
    floor = (dtype(1e-4) * m)[:, None]
    with np.errstate(divide="ignore"):
        ln = np.log(np.maximum(A, floor)).astype(dtype)
    ln = ln.reshape(-1, GROUPS, 4)
    Lb = (((ln[:, :, 0] + ln[:, :, 1]) + ln[:, :, 2]) + ln[:, :, 3]) * dtype(0.25)
    Lb[m == 0] = 0
    return Lb


def score(Lb, key, o):
    """(z_o, complete rows) of offset index o from Lb (steps 4 to 6), in float64"""
    Lb = np.asarray(Lb, np.float64)
    F = Lb.shape[0]
    g0 = o & 1
    pbase = (o + g0) // 2
    nf = (F - g0 + 1) // 2 if F > g0 else 0
    r0, r1 = (pbase + 3) // 4, (pbase + nf) // 4 - 1
    if r1 < r0:
        return 0.0, 0
    G = np.zeros((ROWS, GROUPS - 2))
    for rho in range(r0, r1 + 1):
        gf = g0 + 2 * (4 * rho - pbase)
        T = (((Lb[gf] + Lb[gf + 2]) + Lb[gf + 4]) + Lb[gf + 6]) * 0.25
        G[rho & (ROWS - 1)] += T[1:-1] - 0.5 * (T[:-2] + T[2:])
    den = float(np.sum(G * G))
    if den <= 0.0:
        return 0.0, r1 - r0 + 1
    return float(np.sum(chips(key)[:, 1:-1] * G)) / np.sqrt(den), r1 - r0 + 1


def detect(x, key, dtype=np.float64):
    """-> dict(z, offset (samples), rows, z_all float64 [128], rows_all, detected)"""
    Lb = band_logs(x, dtype)
    res = [score(Lb, key, o) for o in range(OFFSETS)]
    z_all = np.array([r[0] for r in res])
    rows_all = np.array([r[1] for r in res], np.int32)
    o = int(np.argmax(z_all))  # (the lowest o on a tie)
    return dict(z=float(z_all[o]), offset=DETECT_HOP * o, rows=int(rows_all[o]), z_all=z_all, rows_all=rows_all,
                detected=bool(z_all[o] >= THRESHOLD))


# ---- the test signal -----------------------------------------------------------------------------------------------------------
def voiced_signal(seconds=3.0, rate=22050, seed=7):
    """Deterministic synthetic speech, float32 [rate * seconds]: harmonics of a slowly moving 90 - 160 Hz fundamental through four
    resonances, a syllable-rate envelope with gaps, a little noise."""
    rng = np.random.default_rng(seed)
    n = int(round(rate * seconds))
    t = np.arange(n) / rate
    f0 = 125.0 + 35.0 * np.sin(2 * np.pi * 0.37 * t + 0.4) * np.cos(2 * np.pi * 0.11 * t)  # 90 .. 160 Hz
    phase = 2 * np.pi * np.cumsum(f0) / rate
    x = np.zeros(n)
    formants = [(600.0, 110.0, 1.0), (1400.0, 160.0, 0.7), (2600.0, 240.0, 0.45), (3700.0, 320.0, 0.3)]
    for h in range(1, 70):
        fh = h * f0
        amp = sum(g / (1.0 + ((fh - fc) / bw) ** 2) for fc, bw, g in formants) + 0.02
        amp = np.where(fh < 0.45 * rate, amp, 0.0)
        x += amp * np.sin(h * phase + rng.uniform(0, 2 * np.pi))
    syl = 0.5 * (1.0 - np.cos(2 * np.pi * 3.7 * t))          # syllable rate
    gate = (np.sin(2 * np.pi * 0.8 * t + 1.0) > -0.75)       # gaps
    env = syl ** 1.5 * gate
    x = x / np.abs(x).max() * env + 0.03 * rng.standard_normal(n) * (0.3 + env)  # (the noise: -30 dB of the voiced peak, -40 dB in the gaps)
    x *= 0.5 / np.abs(x).max()
    return x.astype(np.float32)
