"""The relative-position attention kernels (relpos_attention_kernel: impl 1, relpos_attention_mfma_kernel: impl 2,
relpos_attention16_kernel: impl 3, the engine's own choice: impl 0) on their own, through vits_debug_relpos_attention, against a
float64 numpy restatement of MultiHeadAttention.attention (attentions.py:165-260).  The reference computes the relative terms the way
the reference does (_get_relative_embeddings pad / slice, then the _relative_position_to_absolute_position /
_absolute_position_to_relative_position reshapes), not in the band form the kernels and the C oracle use, and masks keys with
masked_fill(-1e4).  Head dims 32 / 64 / 96, windows 0-4 and no tables (the StableTTS / BERT form), 1-4 heads (12 for the BERT shape),
ragged lengths T, T-1, ~T/2, 1 and 0."""
import ctypes
import itertools

import numpy as np
import pytest

from conftest import assert_close

pytestmark = pytest.mark.gpu

TOL = 1e-5
# Logits of magnitude S ~ 50-100 carry an fp32 rounding error of ~S * 2^-24 per accumulated term (100 * 6e-8 = 6e-6), which exp()
# turns into a relative error of the same size in every probability.  The scalar kernel (impl 1) recomputes the logits of the
# relative-value band in another order (q.E_k first, then q.k), so its band probabilities and its softmax sum carry independent
# roundings of that size: measured ~1.4e-5 there at max |S| ~ 75 (5.6e-5 at max |S| ~ 290, where the 1e-5 of every other case fails).
SHARP_TOL = 2e-5
IMPLS = (1, 2, 3, 0)
DKS = (32, 64, 96)
WINDOWS = (0, 1, 2, 3, 4, None)
TS = (1, 2, 4, 5, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 300, 513, 1100)


# --------------------------------------------------------------------------- float64 reference (attentions.py:165-260)

def _rel_embeddings(emb, W, length):
    """_get_relative_embeddings: emb [2W+1, dk] -> [2 length - 1, dk]"""
    pad = max(length - (W + 1), 0)
    start = max((W + 1) - length, 0)
    if pad > 0:
        emb = np.pad(emb, ((pad, pad), (0, 0)))
    return emb[start:start + 2 * length - 1]


def _rel_to_abs(x):
    """_relative_position_to_absolute_position: [h, l, 2l-1] -> [h, l, l]"""
    h, n, _ = x.shape
    x = np.pad(x, ((0, 0), (0, 0), (0, 1)))
    x = np.pad(x.reshape(h, n * 2 * n), ((0, 0), (0, n - 1)))
    return x.reshape(h, n + 1, 2 * n - 1)[:, :n, n - 1:]


def _abs_to_rel(x):
    """_absolute_position_to_relative_position: [h, l, l] -> [h, l, 2l-1]"""
    h, n, _ = x.shape
    x = np.pad(x, ((0, 0), (0, 0), (0, n - 1)))
    x = np.pad(x.reshape(h, n * n + n * (n - 1)), ((0, 0), (n, 0)))
    return x.reshape(h, n, 2 * n)[:, :, 1:]


def attention_ref(qkv, lengths, C, nh, ek=None, ev=None, W=None, mask=True):
    """float64 [B, C, T]; query columns >= len are left 0 (the reference's uniform-softmax values there are masked away by x_mask)"""
    B, _, T = qkv.shape
    dk = C // nh
    out = np.zeros((B, C, T))
    x = qkv.astype(np.float64)
    for b in range(B):
        n = int(lengths[b])
        if n == 0:
            continue
        q = x[b, :C].reshape(nh, dk, T).transpose(0, 2, 1) / np.sqrt(dk)  # [h, t, d]
        k = x[b, C:2 * C].reshape(nh, dk, T).transpose(0, 2, 1)
        v = x[b, 2 * C:].reshape(nh, dk, T).transpose(0, 2, 1)
        s = q @ k.transpose(0, 2, 1)
        if ek is not None:
            s = s + _rel_to_abs(q @ _rel_embeddings(np.asarray(ek, np.float64), W, T).T)
        if mask:
            valid = np.arange(T) < n
            s = np.where(valid[:, None] & valid[None, :], s, -1e4)
        s -= s.max(axis=-1, keepdims=True)
        p = np.exp(s)
        p /= p.sum(axis=-1, keepdims=True)
        o = p @ v
        if ev is not None:
            o = o + _abs_to_rel(p) @ _rel_embeddings(np.asarray(ev, np.float64), W, T)
        out[b, :, :n] = o.transpose(0, 2, 1).reshape(C, T)[:, :n]
    return out


# --------------------------------------------------------------------------- the hook

def relpos_attention(lib, qkv, lengths, C, nh, ek=None, ev=None, W=0):
    fn = lib.vits_debug_relpos_attention
    fn.restype = ctypes.c_int
    fp = ctypes.POINTER(ctypes.c_float)
    i32 = ctypes.c_int32
    fn.argtypes = [ctypes.c_int, fp, fp, fp, ctypes.POINTER(ctypes.c_int64), i32, i32, i32, i32, i32, fp]
    B, _, T = qkv.shape
    qkv = np.ascontiguousarray(qkv, np.float32)
    ln = np.ascontiguousarray(lengths, np.int64)
    out = np.empty((B, C, T), np.float32)
    tabs = [None if e is None else np.ascontiguousarray(e, np.float32) for e in (ek, ev)]
    ptr = [None if e is None else e.ctypes.data_as(fp) for e in tabs]
    rc = fn(0, qkv.ctypes.data_as(fp), ptr[0], ptr[1], ln.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), B, C, T, nh, W,
            out.ctypes.data_as(fp))
    return rc, out


def _tables(rng, W, dk):
    """~3x the reference's rel_stddev (k_channels^-0.5, attentions.py:143-145), plus a ramp along the offset axis: the terms carry
    weight and the tables are not symmetric under j - i <-> i - j"""
    nw = 2 * W + 1
    ramp = np.linspace(-1.0, 1.5, nw)[:, None] * (2.0 / np.sqrt(dk))
    ek = rng.standard_normal((nw, dk)) * (3.0 / np.sqrt(dk)) + ramp
    ev = rng.standard_normal((nw, dk)) * 3.0 + 4.0 * ramp * np.sqrt(dk)
    return ek.astype(np.float32), ev.astype(np.float32)


def _lengths(T):
    """T, T-1, about T/2, 1, and an empty item"""
    return np.array(list(dict.fromkeys([T, max(T - 1, 0), T // 2 + 1 if T > 2 else T, 1, 0])), np.int64)


def _cases():
    """Every (impl, dk, window-or-none) cell at least once, every T at least once, each impl at T = 2048 once; heads 1-4 drawn from
    a seeded generator, and one 12-head no-table case at dk 64 (the BERT shape)."""
    rng = np.random.default_rng(20261016)
    cells = list(itertools.product(IMPLS, DKS, WINDOWS))
    order = rng.permutation(len(cells))
    cheap = [t for t in TS if t <= 300]
    cases = []
    for n, c in enumerate(order):
        impl, dk, W = cells[c]
        T = TS[n] if n < len(TS) else int(rng.choice(cheap))
        nh = 12 if (dk == 64 and W is None and impl == 0) else int(rng.integers(1, 5))
        cases.append((impl, dk, W, nh, T))
    for impl in IMPLS:
        dk = int(rng.choice(DKS))
        cases.append((impl, dk, 4 if impl % 2 else None, 2, 2048))
    return cases


CASES = _cases()


def _run(hip_lib, impl, qkv, lengths, C, nh, ek, ev, W):
    try:
        hip_lib.lib.vits_debug_attention_impl(impl)
        rc, got = relpos_attention(hip_lib.lib, qkv, lengths, C, nh, ek, ev, W if W is not None else 0)
    finally:
        hip_lib.lib.vits_debug_attention_impl(0)
    assert rc == 0, rc
    return got


def _check(name, want, got, lengths, tol):
    assert np.isfinite(got).all(), f"{name}: non-finite output (a column the kernel never wrote holds NaN)"
    for b, n in enumerate(lengths):
        assert np.all(got[b, :, int(n):] == 0.0), f"{name}: item {b}: query columns past len {n} are not 0"
    cols = [(b, int(n)) for b, n in enumerate(lengths) if n > 0]
    ref = np.concatenate([want[b, :, :n] for b, n in cols], axis=1)
    out = np.concatenate([got[b, :, :n] for b, n in cols], axis=1)
    return assert_close(name, ref, out, tol)


def test_the_matrix_reaches_every_cell():
    assert {(i, d, w) for i, d, w, _, _ in CASES} == set(itertools.product(IMPLS, DKS, WINDOWS))
    assert {t for *_, t in CASES} >= set(TS)
    assert sorted(i for i, _, _, _, t in CASES if t == 2048) == sorted(IMPLS)
    assert {nh for *_, nh, _ in CASES} >= {1, 2, 3, 4, 12}


@pytest.mark.parametrize("impl,dk,W,nh,T", CASES, ids=[f"impl{i}-dk{d}-{'W%d' % w if w is not None else 'notab'}-h{h}-T{t}"
                                                       for i, d, w, h, t in CASES])
def test_relpos_attention_against_float64(hip_lib, impl, dk, W, nh, T):
    rng = np.random.default_rng([impl, dk, 9 if W is None else W, nh, T])
    C = nh * dk
    lengths = _lengths(T)
    qkv = (rng.standard_normal((len(lengths), 3 * C, T)) * 1.5).astype(np.float32)
    ek, ev = _tables(rng, W, dk) if W is not None else (None, None)
    got = _run(hip_lib, impl, qkv, lengths, C, nh, ek, ev, W)
    _check(f"impl {impl} dk {dk} W {W} heads {nh} T {T}", attention_ref(qkv, lengths, C, nh, ek, ev, W), got, lengths, TOL)


@pytest.mark.parametrize("impl", IMPLS)
def test_sharp_logits(hip_lib, impl):
    """logits of order 50-100: the online-softmax rescale across key tiles and the merge of the waves' (m, l, O) carry the result"""
    rng = np.random.default_rng(77 + impl)
    dk, nh, T, W = 64, 2, 300, 4
    C = nh * dk
    lengths = np.array([T, 257, 150], np.int64)
    qkv = rng.standard_normal((3, 3 * C, T)).astype(np.float32)
    qkv[:, :2 * C] *= 4.0  # q.k / sqrt(dk) ~ N(0, 16^2): max |S| ~ 75 over the 300 x 300 scores
    ek, ev = _tables(rng, W, dk)
    ek *= 4.0
    got = _run(hip_lib, impl, qkv, lengths, C, nh, ek, ev, W)
    x = qkv.astype(np.float64)
    s = np.einsum("dt,ds->ts", x[0, :dk], x[0, C:C + dk]) / np.sqrt(dk)
    assert 50 < np.abs(s).max() < 100, np.abs(s).max()
    err = _check(f"sharp impl {impl}", attention_ref(qkv, lengths, C, nh, ek, ev, W), got, lengths, SHARP_TOL)
    print(f"sharp logits (max |S| {np.abs(s).max():.0f}), impl {impl}: relative error {err:.2e}")


def test_the_reference_would_see_a_misread_kernel(hip_lib):
    """The comparison has power: the reference with the relative offset's sign flipped, with window W-1 instead of W, or with keys
    past len left unmasked misses the kernel's output by at least 100x the tolerance on this case."""
    rng = np.random.default_rng(5)
    dk, nh, T, W = 64, 2, 24, 4
    C = nh * dk
    lengths = np.array([T, 13], np.int64)
    qkv = (rng.standard_normal((2, 3 * C, T)) * 1.5).astype(np.float32)
    ek, ev = _tables(rng, W, dk)
    got = _run(hip_lib, 0, qkv, lengths, C, nh, ek, ev, W)
    _check("fixed case", attention_ref(qkv, lengths, C, nh, ek, ev, W), got, lengths, TOL)

    def miss(want):
        ref = np.concatenate([want[b, :, :n] for b, n in enumerate(lengths)], axis=1)
        out = np.concatenate([got[b, :, :n] for b, n in enumerate(lengths)], axis=1).astype(np.float64)
        return np.abs(ref - out).max() / np.abs(ref).max() / TOL

    flipped = miss(attention_ref(qkv, lengths, C, nh, ek[::-1], ev[::-1], W))  # E[j - i] read as E[i - j]
    narrow = miss(attention_ref(qkv, lengths, C, nh, ek[1:-1], ev[1:-1], W - 1))
    unmasked = miss(attention_ref(qkv, lengths, C, nh, ek, ev, W, mask=False))
    print(f"misreadings / tolerance: flipped offset {flipped:.0f}x, window W-1 {narrow:.0f}x, unmasked keys {unmasked:.0f}x")
    assert flipped >= 100 and narrow >= 100 and unmasked >= 100, (flipped, narrow, unmasked)


def test_hook_arguments(hip_lib):
    rng = np.random.default_rng(1)
    qkv = rng.standard_normal((1, 3 * 64, 8)).astype(np.float32)
    ek, ev = _tables(rng, 4, 32)
    lengths = np.array([8], np.int64)
    assert relpos_attention(hip_lib.lib, qkv, lengths, 64, 2, ek, None, 4)[0] == 1  # exactly one table: VITS_ERR_ARG
    assert relpos_attention(hip_lib.lib, qkv, lengths, 64, 2, None, ev, 4)[0] == 1
    assert relpos_attention(hip_lib.lib, qkv, lengths, 64, 4, None, None, 4)[0] == 4  # head dim 16: VITS_ERR_UNSUPPORTED
    assert relpos_attention(hip_lib.lib, qkv, lengths, 64, 2, ek, ev, 5)[0] == 4  # window 5
    assert relpos_attention(hip_lib.lib, qkv, lengths, 64, 2, ek, ev, -1)[0] == 4
    assert relpos_attention(hip_lib.lib, qkv, np.array([9], np.int64), 64, 2, ek, ev, 4)[0] == 1  # len > T
