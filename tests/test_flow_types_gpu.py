"""GPU tests of the `pre_conv` (flow_type 1) and plain (flow_type 2) flows: the attention without relative positions on its own
against float64 numpy, the flow stage and the whole path against fixtures computed by the reference's own SynthesizerTrn
(tools/gen_golden_flow_types.py), ragged batches on poisoned workspaces, the fast path, streaming, split-bf16 convs and the
persistent flow program (type 0 only).  (The C oracle computes flow_type 0 only: these types are pinned to the goldens.)"""
import ctypes

import numpy as np
import pytest

from conftest import assert_close, golden

pytestmark = pytest.mark.gpu

STAGE_TOL = 1e-4
E2E_TOL = 5e-4
KINDS = ("preconv", "plain")


def _hp(kind, default=False):
    from vosk_tts_amd import weights as W

    if kind == "preconv":
        return W.pre_conv_hparams() if default else W.tiny_pre_conv_hparams()
    return W.plain_flow_hparams() if default else W.tiny_plain_flow_hparams()


@pytest.fixture(scope="module")
def models(hip_lib):
    from vosk_tts_amd import weights as W

    ms = {k: hip_lib.create(W.synthetic_blob(_hp(k), 1234), 0) for k in KINDS}
    yield ms
    for m in ms.values():
        m.close()


@pytest.fixture(scope="module")
def default_models(hip_lib):
    from vosk_tts_amd import weights as W

    ms = {k: hip_lib.create(W.synthetic_blob(_hp(k, True), 1234), 0) for k in KINDS}
    yield ms
    for m in ms.values():
        m.close()


def _attn_ref(qkv, lengths, C, nh):
    """MultiHeadAttention.attention, window_size=None (attentions.py:165-196), float64; rows past len are 0"""
    B, _, T = qkv.shape
    dk = C // nh
    out = np.zeros((B, C, T))
    for b in range(B):
        n = int(lengths[b])
        for h in range(nh):
            q = qkv[b, h * dk:(h + 1) * dk, :n].astype(np.float64)
            k = qkv[b, C + h * dk:C + (h + 1) * dk, :n].astype(np.float64)
            v = qkv[b, 2 * C + h * dk:2 * C + (h + 1) * dk, :n].astype(np.float64)
            s = (q / np.sqrt(dk)).T @ k
            s -= s.max(axis=1, keepdims=True)
            p = np.exp(s)
            p /= p.sum(axis=1, keepdims=True)
            out[b, h * dk:(h + 1) * dk, :n] = (p @ v.T).T
    return out


def _plain_attention(lib, qkv, lengths, C, nh):
    fn = lib.vits_debug_plain_attention
    fn.restype = ctypes.c_int
    fp = ctypes.POINTER(ctypes.c_float)
    fn.argtypes = [ctypes.c_int, fp, ctypes.POINTER(ctypes.c_int64), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, fp]
    B, _, T = qkv.shape
    qkv = np.ascontiguousarray(qkv, np.float32)
    ln = np.ascontiguousarray(lengths, np.int64)
    out = np.empty((B, C, T), np.float32)
    rc = fn(0, qkv.ctypes.data_as(fp), ln.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), B, C, T, nh, out.ctypes.data_as(fp))
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("dk", [16, 32, 48, 64, 96])
@pytest.mark.parametrize("impl", [2, 3])
def test_plain_attention_against_float64(hip_lib, dk, impl):
    """Both tile variants (2: 32-query tiles, 3: 16-query tiles), ragged lengths including 1, rows past len exactly 0."""
    rng = np.random.default_rng(dk * 10 + impl)
    nh = 2
    C = nh * dk
    try:
        hip_lib.lib.vits_debug_attention_impl(impl)
        for T in (1, 5, 16, 17, 33, 64, 65, 300, 2048):
            lengths = np.array(sorted({T, max(1, T // 2 + 1), 1}, reverse=True), np.int64)
            qkv = rng.standard_normal((len(lengths), 3 * C, T)).astype(np.float32) * 1.5
            got = _plain_attention(hip_lib.lib, qkv, lengths, C, nh)
            assert_close(f"attention dk {dk} T {T} impl {impl}", _attn_ref(qkv, lengths, C, nh), got, 1e-5)
            for b, n in enumerate(lengths):
                assert np.all(got[b, :, int(n):] == 0.0)
    finally:
        hip_lib.lib.vits_debug_attention_impl(0)


def test_unsupported_flow_geometries_are_refused(hip_lib):
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.capi import VitsError

    hp = W.tiny_hparams()
    t = W.make_synthetic_weights(hp, 1)
    raw = bytearray(W.pack_blob(hp, t))
    off = 12 + W.HParams.flow_type.offset
    raw[off:off + 4] = (3).to_bytes(4, "little")  # (pack_blob validates; a hand-edited blob reaches vits_create)
    with pytest.raises(VitsError) as e:
        hip_lib.create(bytes(raw), 0)
    assert e.value.code == 4
    hp = W.tiny_pre_conv_hparams()
    hp.inter_channels = 96  # head dim 24
    raw = bytearray(W.pack_blob(W.tiny_hparams(), t))
    raw[12:12 + len(bytes(hp))] = bytes(hp)
    with pytest.raises(VitsError) as e:
        hip_lib.create(bytes(raw), 0)
    assert e.value.code == 4


@pytest.mark.parametrize("kind", KINDS)
def test_flow_stage_tiny_ragged_b3(models, kind):
    g = golden(f"flow_{kind}_tiny_b3")
    z = models[kind].flow(g["z_p"], g["y_lengths"], g["sid"])
    for b, n in enumerate(g["y_lengths"]):
        assert_close(f"z[{b}]", g["z"][b, :, :n], z[b, :, :n], STAGE_TOL)


@pytest.mark.parametrize("kind", KINDS)
def test_flow_stage_default_size(default_models, kind):
    """Default geometry (pre_conv: head dim 48) at B=2 ragged and each item alone at B=1."""
    g = golden(f"flow_{kind}_default_b2")
    m = default_models[kind]
    z = m.flow(g["z_p"], g["y_lengths"], g["sid"])
    for b, n in enumerate(g["y_lengths"]):
        n = int(n)
        assert_close(f"B=2 z[{b}]", g["z"][b, :, :n], z[b, :, :n], STAGE_TOL)
        z1 = m.flow(np.ascontiguousarray(g["z_p"][b:b + 1, :, :n]), g["y_lengths"][b:b + 1], g["sid"][b:b + 1])
        assert_close(f"B=1 z[{b}]", g["z"][b, :, :n], z1[0], STAGE_TOL)


def _valid(audio, olen):
    a = np.array(audio, copy=True)
    for b, n in enumerate(olen):
        a[b, int(n):] = 0.0
    return a


@pytest.mark.parametrize("kind", KINDS)
def test_end_to_end_ragged_batch_on_poisoned_workspace(hip_lib, kind):
    from vosk_tts_amd import weights as W

    g = golden(f"flow_{kind}_e2e_b3")
    hip_lib.lib.vits_debug_poison_workspace(1)
    try:
        m = hip_lib.create(W.synthetic_blob(_hp(kind), 1234), 0)
        try:
            audio, olen = m.synthesize(g["ids"], g["lengths"], g["scales"], g["sid"], noise_dp=g["noise_dp"], noise_prior=g["noise_prior"],
                                       forced_durations=g["forced_durations"])
        finally:
            m.close()
    finally:
        hip_lib.lib.vits_debug_poison_workspace(0)
    assert np.array_equal(olen, g["y_lengths"] * 256)
    assert np.isfinite(audio).all()
    assert_close("audio(e2e, golden)", _valid(g["audio"], olen), _valid(audio, olen), E2E_TOL)


def _batch(rng, B=3, Tx=30):
    lengths = np.array([Tx, 9, 17, 1, 22, 30, 5, 12][:B], np.int64)
    ids = rng.integers(1, 20, size=(B, Tx)).astype(np.int64)
    dur = rng.integers(0, 5, size=(B, Tx)).astype(np.int32)
    return ids, lengths, (np.arange(B) % 5).astype(np.int64), dur


@pytest.mark.parametrize("kind", KINDS)
def test_fast_path_equals_eager(hip_lib, models, kind):
    rng = np.random.default_rng(3)
    ids, lengths, sid, dur = _batch(rng)
    out = []
    try:
        for on in (0, 1, 1):
            hip_lib.lib.vits_debug_fast_path(on)
            out.append(models[kind].synthesize(ids, lengths, [0.667, 1.0, 0.8], sid, forced_durations=dur, seed=6))
    finally:
        hip_lib.lib.vits_debug_fast_path(1)
    for a, la in out[1:]:
        assert np.array_equal(la, out[0][1])
        assert np.array_equal(_valid(a, la), _valid(out[0][0], la))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("chunk", [16, 37])
def test_streaming_chunks_equal_one_shot(models, kind, chunk):
    m = models[kind]
    rng = np.random.default_rng(11)
    Tx = 40
    ids = rng.integers(1, 20, size=(1, Tx)).astype(np.int64)
    dur = rng.integers(1, 6, size=(1, Tx)).astype(np.int32)
    Ty = int(dur.sum())
    scales = [0.667, 1.0, 0.8]
    one, _ = m.synthesize(ids, [Tx], scales, [2], forced_durations=dur, seed=5)
    chunks = list(m.stream(ids, scales, 2, chunk_frames=chunk, forced_durations=dur, seed=5))
    got = np.concatenate(chunks)[None]
    assert got.shape == one.shape == (1, Ty * 256)
    assert_close("stream vs one-shot", one, got, 2e-5)


@pytest.mark.parametrize("kind", KINDS)
def test_split_bf16_convs_stay_within_5e5_at_batch(hip_lib, kind):
    from vosk_tts_amd import weights as W

    hp = _hp(kind)
    t = W.make_synthetic_weights(hp, 1234)
    hp1 = W.HParams.from_buffer_copy(bytes(hp))
    hp1.conv_precision = 1
    m0, m1 = hip_lib.create(W.pack_blob(hp, t), 0), hip_lib.create(W.pack_blob(hp1, t), 0)
    try:
        rng = np.random.default_rng(21)
        ids, lengths, sid, dur = _batch(rng, B=8, Tx=60)
        a0, l0 = m0.synthesize(ids, lengths, [0.667, 1.0, 0.8], sid, forced_durations=dur, seed=2)
        a1, l1 = m1.synthesize(ids, lengths, [0.667, 1.0, 0.8], sid, forced_durations=dur, seed=2)
        assert np.array_equal(l0, l1)
        assert_close("bf16x3 vs fp32", _valid(a0, l0), _valid(a1, l1), 5e-5)
    finally:
        m0.close()
        m1.close()


def test_only_flow_type_0_runs_the_persistent_flow_program(hip_lib, hip_default, default_models):
    fn = hip_lib.lib.vits_debug_persist_runs
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p]
    rng = np.random.default_rng(4)
    z_p = rng.standard_normal((1, 192, 150)).astype(np.float32)
    for m, want in ((hip_default, True), (default_models["preconv"], False), (default_models["plain"], False)):
        r0 = int(fn(m._h))
        m.flow(z_p, np.array([150], np.int64), np.array([3], np.int64))
        took = int(fn(m._h)) - r0
        assert (took > 0) == want, (m.hp.flow_type, took)
