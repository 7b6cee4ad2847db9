"""float64 restatement of include/vits_limit.h (envelope, required gain, look-ahead minimum, release, box attack, output and the two-pass
LUFS form) -- the reference the limiter tests compare the library with -- and the signals those tests use.  Nothing here imports the
package.  Every step takes a dtype, so that the same code run in float32 gives the yardstick for a different order of operations."""
import math

import numpy as np

import loudness_ref
import resample_ref

SAMPLE, TRUE = 1, 2
TILE = 2048           # VITS_LIMIT_TILE
MAX_LOOKAHEAD = 1024  # VITS_LIMIT_MAX_LOOKAHEAD
HALF = 16             # half width of the 4x interpolator, input samples
RATES = (8000, 22050, 48000)


def plan(rate, lookahead_ms, release_ms):
    """(W, a): W = round(lookahead_ms * rate / 1000), halves away from zero; a = exp(-1 / (release_ms * rate / 1000)); both from the fp32
    arguments in double"""
    w = float(np.float32(lookahead_ms)) * rate / 1000.0
    W = int(math.floor(w + 0.5))
    a = math.exp(-1.0 / (float(np.float32(release_ms)) * rate / 1000.0))
    return W, a


def table4(rate):
    """the fp32 table of vits_resample_table(rate, 4 rate): [4, 33]"""
    return resample_ref.table(rate, 4 * rate).astype(np.float32)


def upsample4(x, rate):
    """u [4 len] of step 1 in float64 from the fp32 table: u[4 n + p] = sum_i table[p][i] x[n - lo(p) + i]"""
    x = np.asarray(x, np.float64).reshape(-1)
    n = x.shape[0]
    tab = table4(rate).astype(np.float64)
    P = resample_ref.plan(rate, 4 * rate)
    L, W, taps = P["L"], P["W"], P["taps"]
    assert (L, P["M"], taps, P["half"]) == (4, 1, 33, HALF)
    xp = np.concatenate([np.zeros(HALF), x, np.zeros(taps)])
    u = np.zeros((n, L))
    for p in range(L):
        lo = (W - p) // L
        win = np.lib.stride_tricks.sliding_window_view(xp, taps)[HALF - lo:HALF - lo + n]  # row n: x[n - lo .. n - lo + taps)
        u[:, p] = win @ tab[p]
    return u.reshape(-1)


def envelope(x, rate, mode):
    """p [len] in float64 (the device forms u, and so p, in fp32: resample_ref.fp32_bound of table4 bounds the difference)"""
    x = np.asarray(x, np.float64).reshape(-1)
    p = np.abs(x)
    if mode == TRUE and x.shape[0]:
        p = np.maximum(p, np.abs(upsample4(x, rate)).reshape(-1, 4).max(axis=1))
    return p


def true_peak(x, rate):
    p = envelope(x, rate, TRUE)
    return float(p.max()) if p.size else 0.0


def required(p, c, g, dtype=np.float64):
    """step 2"""
    gp = dtype(g) * np.asarray(p, dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(gp > 0, np.minimum(dtype(1), dtype(c) / gp), dtype(1)).astype(dtype)


def lookahead_min(r, W):
    """step 3: m[k] for k in [-W, len) (index k + W), r = 1 outside [0, len)"""
    one = np.ones(W, r.dtype)
    rp = np.concatenate([one, r, one])
    return np.lib.stride_tricks.sliding_window_view(rp, W + 1).min(axis=1)


def release(m, a, e0=1.0):
    """step 4, sequentially: e[k] = min(m[k], a e[k-1] + (1 - a)) from e[-W-1] = e0"""
    dt = m.dtype.type
    a, b = dt(a), dt(1) - dt(a)
    e = np.empty_like(m)
    v = dt(e0)
    for k in range(m.shape[0]):
        v = min(m[k], a * v + b)
        e[k] = v
    return e


def release_scan(m, a, block=8, tile=TILE):
    """step 4 by composition: a step is the map v -> min(C, A v + B) = (a, 1 - a, m[k]); (A1, B1, C1) then (A2, B2, C2) is
    (A2 A1, A2 B1 + B2, min(C2, A2 C1 + B2)).  Composites per block, per tile of blocks, carries over the tiles, then over the blocks of
    a tile, then the steps of a block from its carry-in: the order the device's launches impose."""
    def comp(f, g):
        return (g[0] * f[0], g[0] * f[1] + g[1], min(g[2], g[0] * f[2] + g[1]))

    def ap(f, v):
        return min(f[2], f[0] * v + f[1])

    n = m.shape[0]
    steps = [(a, 1.0 - a, float(m[k])) for k in range(n)]
    ident = (1.0, 0.0, math.inf)
    blocks = []
    for k0 in range(0, n, block):
        f = ident
        for s in steps[k0:k0 + block]:
            f = comp(f, s)
        blocks.append(f)
    per_tile = tile // block
    tiles = []
    for t0 in range(0, len(blocks), per_tile):
        f = ident
        for bl in blocks[t0:t0 + per_tile]:
            f = comp(f, bl)
        tiles.append(f)
    e = np.empty(n)
    v_tile = 1.0
    for ti, tf in enumerate(tiles):
        v_blk = v_tile
        for bi in range(ti * per_tile, min((ti + 1) * per_tile, len(blocks))):
            v = v_blk
            for k in range(bi * block, min((bi + 1) * block, n)):
                v = ap(steps[k], v)
                e[k] = v
            v_blk = ap(blocks[bi], v_blk)
        v_tile = ap(tf, v_tile)
    return e


def attack(e, W, n):
    """step 5: s[n] = (e[n-W] + ... + e[n]) / (W + 1), e indexed by k + W"""
    if n == 0:
        return np.zeros(0, e.dtype)
    return np.lib.stride_tricks.sliding_window_view(e, W + 1)[:n].sum(axis=1, dtype=e.dtype) / e.dtype.type(W + 1)


def curve(p, c, g, W, a, dtype=np.float64):
    """steps 2-5 from an envelope -> (r, s)"""
    r = required(p, c, g, dtype)
    e = release(lookahead_min(r, W), a)
    return r, attack(e, W, r.shape[0])


def apply(x, s, g):
    """step 6: fp32(fp32(g s) x)"""
    gs = (np.float64(np.float32(g)) * np.asarray(s, np.float64)).astype(np.float32)
    return gs * np.asarray(x, np.float32)


def limit(x, rate, mode, c, lookahead_ms, release_ms, g, dtype=np.float64):
    """one item -> dict(p, r, s, y, reduction)"""
    x = np.asarray(x, np.float32).reshape(-1)
    W, a = plan(rate, lookahead_ms, release_ms)
    p = envelope(x, rate, mode).astype(np.float32)  # (fp32 p, as on the device; in sample mode the same bits)
    r, s = curve(p, np.float32(c), np.float32(g), W, a, dtype)
    s32 = s.astype(np.float32)
    return dict(p=p, r=r, s=s, y=apply(x, s, g), reduction=float(s32.min()) if s32.size else 1.0)


def loudness_limit(x, rate, target, mode, c, lookahead_ms, release_ms):
    """the two-pass LUFS form of one item -> dict(L, g0, y0, L0, g1, y, s)"""
    x = np.asarray(x, np.float32).reshape(-1)
    L = loudness_ref.integrated(x, rate)
    g0 = np.float32(1.0 if L == -math.inf else 10.0 ** ((target - L) / 20.0))
    one = limit(x, rate, mode, c, lookahead_ms, release_ms, g0)
    L0 = loudness_ref.integrated(one["y"], rate)
    g1 = g0
    if L0 != -math.inf and (one["r"] < 1).any():
        g1 = np.float32(np.float64(g0) * np.float64(np.float32(10.0 ** ((target - L0) / 20.0))))
    two = limit(x, rate, mode, c, lookahead_ms, release_ms, g1)
    return dict(L=L, g0=float(g0), y0=one["y"], L0=L0, g1=float(g1), y=two["y"], s=two["s"], reduction=two["reduction"])


# ---- signals ------------------------------------------------------------------------------------------------------------------------
def gated_noise(rate, n, seed=1):
    """loudness_ref.enveloped_noise times a 2.5 Hz square gate: bursts between silences, as plosives between vowels"""
    t = np.arange(n) / rate
    return loudness_ref.enveloped_noise(rate, n, seed) * (np.floor(t * 5.0) % 2 == 0)


def alternating(n):
    """a full-scale +1 / -1 run: the sample peak is 1, the interpolated peak lies between the samples' sign changes"""
    return np.where(np.arange(n) % 2 == 0, 1.0, -1.0)


def spiky(n, W, seed=3):
    """low noise with single-sample peaks at: sample 0, the last sample, W before every tile edge, on every tile edge, and a pair W + 2
    apart (the release runs between them)"""
    x = 0.05 * np.random.default_rng(seed).uniform(-1.0, 1.0, n)
    at = {0, n - 1}
    for k in range(1, n // TILE + 1):
        at |= {k * TILE - W, k * TILE, k * TILE - 1}
    at |= {n // 3, n // 3 + W + 2}
    for i, q in enumerate(sorted(q for q in at if 0 <= q < n)):
        x[q] = (0.95 - 0.1 * (i % 3)) * (-1.0) ** i
    return x


def op_lengths(W):
    return [0, 1, W, W + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + W]


def op_batches(W):
    """The ragged batches of the kernel-level GPU tests at look-ahead W: B = 4 items of at most 3 tiles each, the lengths of op_lengths;
    the first batch spiky (limits), the second holds a quiet item (never reaches the ceiling) and zeros.
    -> [(x float32 [4, N] with NaN at and beyond each length, lengths int64 [4])]"""
    lens = op_lengths(W)
    out = []
    for half, group in enumerate((lens[:4], lens[4:])):
        rows = [spiky(n, W, seed=3 + i + 4 * half).astype(np.float32) if n else np.zeros(0, np.float32) for i, n in enumerate(group)]
        N = max(max(group), 1)
        x = np.full((4, N), np.nan, np.float32)
        for b, r in enumerate(rows):
            x[b, :r.shape[0]] = r
        out.append((x, np.array(group, np.int64)))
    n = 2 * TILE + W
    quiet = np.stack([0.01 * spiky(n, W, 11), np.zeros(n), gated_noise(22050, n), 0.4 * alternating(n)]).astype(np.float32)
    out.append((quiet, np.array([n, n, n - 5, TILE + 3], np.int64)))
    out[-1][0][2, n - 5:] = np.nan
    out[-1][0][3, TILE + 3:] = np.nan
    return out


def two_pass_items(rate):
    """The items of the two-pass GPU test at `rate`, 2 s each: gated noise (limits hard at a loud target) and a sine (reaches a
    moderate target without limiting) -> x float32 [2, N], lengths"""
    n = 2 * rate
    x = np.stack([gated_noise(rate, n), loudness_ref.sine(rate, n, amp=0.1)]).astype(np.float32)
    x[1, n - 7:] = np.nan
    return x, np.array([n, n - 7], np.int64)


TWO_PASS_TARGET = -10.0   # gated noise at 0.3 peak sits near -18.5 LUFS: + 8.5 dB drives its bursts to 0.8, past the ceiling; the sine stays at 0.45
TWO_PASS_CEILING = 0.5
