"""float64 restatement of the watermark payload (include/vits_watermark_payload.h), the definition the device kernels are checked
against, on top of tests/watermark_ref.py (which it imports and does not change), and an fp32 run of the same code (dtype=np.float32,
with the meaning it has there: the transforms, the gains, ln and the four-bin mean in fp32; T, D, G and every score in float64).
Plain numpy."""
import numpy as np

import watermark_ref as R

PAYLOAD_MAX = 0xFFFF
CODED_BITS = 24
DEFAULT_DEPTH_DB = 2.0


# ---- the code (integer arithmetic only) ---------------------------------------------------------------------------------------
def crc8(p, init=0xFF):
    """over the 16 bits of p, MSB first: polynomial 0x07, no final xor"""
    c = init
    for i in range(15, -1, -1):
        fb = ((c >> 7) & 1) ^ ((int(p) >> i) & 1)
        c = (c << 1) & 0xFF
        if fb:
            c ^= 0x07
    return c


def payload_arg(p):
    """the payload as an int; anything outside [0, 65535] is refused by name"""
    if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not 0 <= int(p) <= PAYLOAD_MAX:
        raise ValueError(f"watermark payload {p!r} outside [0, {PAYLOAD_MAX}]")
    return int(p)


def word(p):
    """W = (p << 8) | crc8(p)"""
    p = payload_arg(p)
    return (p << 8) | crc8(p)


def word_bits(W):
    """coded bit i = (W >> (23 - i)) & 1, int [24]"""
    return np.array([(int(W) >> (CODED_BITS - 1 - i)) & 1 for i in range(CODED_BITS)], np.int64)


# ---- positions -----------------------------------------------------------------------------------------------------------------
def pilots():
    """bool [16, 96]: (q + j) odd"""
    return ((np.arange(R.ROWS)[:, None] + np.arange(R.GROUPS)[None, :]) & 1) == 1


def bit_index(key):
    """i(q, j) int [16, 96] (meaningful on the payload positions only)"""
    mk = np.uint64(R.mix(int(key) & 0xFFFFFFFF))
    idx = (R.GROUPS * np.arange(R.ROWS)[:, None] + np.arange(R.GROUPS)[None, :] + 1).astype(np.uint64) | np.uint64(0x80000000)
    return (R.mix(mk ^ idx).astype(np.int64)) % CODED_BITS


def payload_chips(key, p):
    """c'(q, j) as float64 [16, 96] of +1 / -1"""
    c = R.chips(key)
    flip = word_bits(word(p))[bit_index(key)] == 1
    return np.where(~pilots() & flip, -c, c)


def depth_arg(depth_db):
    """0 = the payload default, 2 dB; the range is that of the plain mark"""
    return R.depth_arg(DEFAULT_DEPTH_DB if float(depth_db) == 0.0 else depth_db)


# ---- embed ---------------------------------------------------------------------------------------------------------------------
def embed(x, key, p, depth_db=0.0, dtype=np.float64):
    """the embed of watermark_ref, line by line, with c' in place of c"""
    a = depth_arg(depth_db)
    c = payload_chips(key, p)
    x = np.asarray(x, dtype).reshape(-1)
    if x.shape[0] < R.M + 1:
        return x.copy()
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    a = dtype(np.float32(a)) if dtype == np.float32 else a
    gp, gm = dtype(1.0) + a, dtype(1.0) - a
    w = R.window(dtype)
    X = np.fft.rfft(R.frames(x, R.H, dtype), axis=1).astype(ctype)
    F = X.shape[0]
    g = np.ones((F, R.M + 1), dtype)
    q = (np.arange(F) >> 2) & (R.ROWS - 1)
    k = np.arange(R.BIN_LO, R.BIN_HI)
    g[:, R.BIN_LO:R.BIN_HI] = np.where(c[q][:, (k - R.BIN_LO) >> 2] > 0, gp, gm)
    y = np.fft.irfft(X * g, n=R.N, axis=1).astype(dtype) * w[None, :]
    total = R.H * (F - 1) + R.N
    acc = np.zeros(total, dtype)
    env = np.zeros(total, np.float64)
    w2 = R.window() ** 2
    for f in range(F):
        acc[f * R.H:f * R.H + R.N] += y[f]
        env[f * R.H:f * R.H + R.N] += w2
    keep = slice(R.M, R.M + R.H * (F - 1))
    out = x.copy()
    out[:R.H * (F - 1)] = acc[keep] * (1.0 / env[keep]).astype(dtype)
    return out


# ---- read ----------------------------------------------------------------------------------------------------------------------
def g_of(Lb, o):
    """(G float64 [16, 96] with columns 0 and 95 zero, complete rows) of offset index o: steps 4 and 5 of Detect"""
    F = Lb.shape[0]
    g0 = o & 1
    pbase = (o + g0) // 2
    nf = (F - g0 + 1) // 2 if F > g0 else 0
    r0, r1 = (pbase + 3) // 4, (pbase + nf) // 4 - 1
    G = np.zeros((R.ROWS, R.GROUPS))
    if r1 < r0:
        return G, 0
    for rho in range(r0, r1 + 1):
        gf = g0 + 2 * (4 * rho - pbase)
        T = (((Lb[gf] + Lb[gf + 2]) + Lb[gf + 4]) + Lb[gf + 6]) * 0.25
        G[rho & (R.ROWS - 1), 1:-1] += T[1:-1] - 0.5 * (T[:-2] + T[2:])
    return G, r1 - r0 + 1


def read(x, key, dtype=np.float64):
    """-> dict(z, offset (samples), rows, detected, payload, valid, word, z_all float64 [128], bit_z float64 [24])"""
    Lb = np.asarray(R.band_logs(x, dtype), np.float64)
    c = R.chips(key)
    scored = np.zeros((R.ROWS, R.GROUPS), bool)
    scored[:, 1:-1] = True
    pil = pilots() & scored
    z_all = np.zeros(R.OFFSETS)
    rows_all = np.zeros(R.OFFSETS, np.int32)
    Gs = []
    for o in range(R.OFFSETS):
        G, rows = g_of(Lb, o)
        Gs.append(G)
        rows_all[o] = rows
        den = float(np.sum(G[pil] ** 2))
        if rows > 0 and den > 0.0:
            z_all[o] = float(np.sum((c * G)[pil])) / np.sqrt(den)
    o = int(np.argmax(z_all))  # (the lowest o on a tie)
    G = Gs[o]
    bi = bit_index(key)
    bit_z = np.zeros(CODED_BITS)
    for i in range(CODED_BITS):
        sel = ~pilots() & scored & (bi == i)
        n = float(np.sum(G[sel] ** 2))
        if n > 0.0:
            bit_z[i] = float(np.sum((c * G)[sel])) / np.sqrt(n)
    W = 0
    for i in range(CODED_BITS):
        W = (W << 1) | int(bit_z[i] < 0)
    detected = bool(z_all[o] >= R.THRESHOLD)
    return dict(z=float(z_all[o]), offset=R.DETECT_HOP * o, rows=int(rows_all[o]), detected=detected, payload=W >> 8,
                valid=bool(detected and crc8(W >> 8) == (W & 0xFF)), word=W, z_all=z_all, rows_all=rows_all, bit_z=bit_z)
