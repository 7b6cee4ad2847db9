"""GPU tests of voices whose n_heads is not 2 (weights.heads3_hparams: text encoder 3 heads of 64; heads4_hparams: 4 heads of 32),
whose pre_conv2 flow keeps 2 heads (models.py:352-360): the text encoder, duration, regulation and flow stages against fixtures
computed by the reference's own SynthesizerTrn (tools/gen_golden_heads.py) and the oracle under every attention kernel, the
persistent text encoder and flow programs, the fast path and a ragged batch on a poisoned workspace."""
import ctypes

import numpy as np
import pytest

from conftest import assert_close, golden

pytestmark = pytest.mark.gpu

STAGE_TOL = 1e-4
VARIANTS = ("heads3", "heads4")


def _hp(v):
    from vosk_tts_amd import weights as W

    return {"heads3": W.heads3_hparams, "heads4": W.heads4_hparams}[v]()


@pytest.fixture(scope="module")
def models(hip_lib):
    from vosk_tts_amd import weights as W

    ms = {v: hip_lib.create(W.synthetic_blob(_hp(v), 1234), 0) for v in VARIANTS}
    yield ms
    for m in ms.values():
        m.close()


@pytest.fixture(scope="module")
def oracles(oracle_lib):
    from vosk_tts_amd import weights as W

    ms = {v: oracle_lib.create(W.synthetic_blob(_hp(v), 1234)) for v in VARIANTS}
    yield ms
    for m in ms.values():
        m.close()


def _persist_runs(hip_lib, model):
    fn = hip_lib.lib.vits_debug_persist_runs
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p]
    return int(fn(model._h))


@pytest.mark.parametrize("impl", [0, 1, 2, 3])
@pytest.mark.parametrize("v", VARIANTS)
def test_stages_against_the_reference_and_the_oracle(hip_lib, models, oracles, v, impl):
    g = golden(f"{v}_b2")
    m, o = models[v], oracles[v]
    ids, lengths, sid, scales = g["ids"], g["lengths"], g["sid"], g["scales"]
    Ty = int(g["y_lengths"].max())
    try:
        hip_lib.lib.vits_debug_attention_impl(impl)
        hip_lib.lib.vits_debug_persist(0)  # the launch path's kernels (the programs have their own attention blocks)
        x, m_p, logs_p = m.text_encoder(ids, lengths, sid)
        logw = m.duration(g["x"], lengths, sid, g["noise_dp"], float(scales[2]))
        _, ylen, z_p = m.regulate(None, g["forced_durations"], lengths, float(scales[1]), g["m_p_tok"], g["logs_p_tok"], g["noise_prior"],
                                  float(scales[0]), Ty)
        z = m.flow(g["z_p"], g["y_lengths"], sid)
    finally:
        hip_lib.lib.vits_debug_attention_impl(0)
        hip_lib.lib.vits_debug_persist(7)
    ox, _, _ = o.text_encoder(ids, lengths, sid)
    oz = o.flow(g["z_p"], g["y_lengths"], sid)
    for b, n in enumerate(lengths):
        n = int(n)
        assert_close(f"x[{b}]", g["x"][b, :, :n], x[b, :, :n], STAGE_TOL)
        assert_close(f"x[{b}] vs oracle", ox[b, :, :n], x[b, :, :n], STAGE_TOL)
        assert_close(f"m_p[{b}]", g["m_p_tok"][b, :, :n], m_p[b, :, :n], STAGE_TOL)
        assert_close(f"logs_p[{b}]", g["logs_p_tok"][b, :, :n], logs_p[b, :, :n], STAGE_TOL)
        assert_close(f"logw[{b}]", g["logw"][b, :n], logw[b, :n], 5 * STAGE_TOL)
    assert np.array_equal(ylen, g["y_lengths"])
    assert_close("z_p", g["z_p"], z_p, STAGE_TOL)
    for b, n in enumerate(g["y_lengths"]):
        n = int(n)
        assert_close(f"z[{b}]", g["z"][b, :, :n], z[b, :, :n], STAGE_TOL)
        assert_close(f"z[{b}] vs oracle", oz[b, :, :n], z[b, :, :n], STAGE_TOL)


@pytest.mark.parametrize("T", [1, 5, 17])
@pytest.mark.parametrize("v", VARIANTS)
def test_text_encoder_edge_lengths(models, v, T):
    g = golden(f"{v}_enc_T{T}")
    x, m_p, logs_p = models[v].text_encoder(g["ids"], g["lengths"], g["sid"])
    assert_close("x", g["x"], x, STAGE_TOL)
    assert_close("m_p", g["m_p_tok"], m_p, STAGE_TOL)
    assert_close("logs_p", g["logs_p_tok"], logs_p, STAGE_TOL)


@pytest.mark.parametrize("T", [1, 16, 17, 50, 257, 512])
@pytest.mark.parametrize("v", VARIANTS)
def test_persistent_text_encoder_and_flow(hip_lib, models, oracles, v, T):
    """The single-utterance programs, each encoder with its own heads (text encoder: n_heads; flow: 2), against the oracle and the
    launch path (vits_debug_persist(0))"""
    m, o, hp = models[v], oracles[v], _hp(v)
    rng = np.random.default_rng(4000 + T)
    L = max(1, T - 3)
    lens = np.array([L], np.int64)
    sid = np.array([7], np.int64)
    ids = rng.integers(1, hp.n_vocab, size=(1, T)).astype(np.int64)
    z_p = rng.standard_normal((1, hp.inter_channels, T)).astype(np.float32)
    mask = np.arange(T)[None, None, :] < L
    want_enc, want_z = o.text_encoder(ids, lens, sid), o.flow(z_p, lens, sid)
    try:
        hip_lib.lib.vits_debug_persist(7)
        r0 = _persist_runs(hip_lib, m)
        enc = m.text_encoder(ids, lens, sid)
        z = m.flow(z_p, lens, sid)
        assert _persist_runs(hip_lib, m) == r0 + 2, "the persistent programs did not run"
        hip_lib.lib.vits_debug_persist(0)
        base_enc = m.text_encoder(ids, lens, sid)
        base_z = m.flow(z_p, lens, sid)
    finally:
        hip_lib.lib.vits_debug_persist(7)
    for name, w, got, b in zip(("x", "m_p", "logs_p"), want_enc, enc, base_enc):
        assert_close(f"{name} persistent vs oracle", w * mask, got * mask, STAGE_TOL)
        assert_close(f"{name} persistent vs launch path", b * mask, got * mask, STAGE_TOL)
        assert np.all(got * ~mask == 0), f"{name}: padding columns must be zero"
    assert_close("z persistent vs oracle", want_z * mask, z * mask, STAGE_TOL)
    assert_close("z persistent vs launch path", base_z * mask, z * mask, STAGE_TOL)


def _valid(audio, olen):
    a = np.array(audio, copy=True)
    for b, n in enumerate(olen):
        a[b, int(n):] = 0.0
    return a


@pytest.mark.parametrize("v", VARIANTS)
def test_fast_path_equals_eager(hip_lib, models, v):
    rng = np.random.default_rng(8)
    B, Tx = 3, 30
    ids = rng.integers(1, 62, size=(B, Tx)).astype(np.int64)
    lengths = np.array([Tx, 9, 17], np.int64)
    dur = rng.integers(0, 5, size=(B, Tx)).astype(np.int32)
    sid = np.array([0, 7, 199], np.int64)
    out = []
    try:
        for on in (0, 1, 1):
            hip_lib.lib.vits_debug_fast_path(on)
            out.append(models[v].synthesize(ids, lengths, [0.667, 1.0, 0.8], sid, forced_durations=dur, seed=6))
    finally:
        hip_lib.lib.vits_debug_fast_path(1)
    for a, la in out[1:]:
        assert np.array_equal(la, out[0][1])
        assert np.array_equal(_valid(a, la), _valid(out[0][0], la))


@pytest.mark.parametrize("v", VARIANTS)
def test_ragged_batch_on_poisoned_workspace_equals_items_alone(hip_lib, v):
    from vosk_tts_amd import weights as W

    g = golden(f"{v}_b2")
    hip_lib.lib.vits_debug_poison_workspace(1)
    try:
        m = hip_lib.create(W.synthetic_blob(_hp(v), 1234), 0)  # fresh session pool -> fresh (poisoned) workspaces
        try:
            x, _, _ = m.text_encoder(g["ids"], g["lengths"], g["sid"])
            z = m.flow(g["z_p"], g["y_lengths"], g["sid"])
            assert np.isfinite(x).all() and np.isfinite(z).all()
            for b in range(2):
                n, ny = int(g["lengths"][b]), int(g["y_lengths"][b])
                x1, _, _ = m.text_encoder(np.ascontiguousarray(g["ids"][b:b + 1, :n]), g["lengths"][b:b + 1], g["sid"][b:b + 1])
                z1 = m.flow(np.ascontiguousarray(g["z_p"][b:b + 1, :, :ny]), g["y_lengths"][b:b + 1], g["sid"][b:b + 1])
                assert_close(f"x[{b}] batch vs alone", x1[0], x[b, :, :n], STAGE_TOL)
                assert_close(f"z[{b}] batch vs alone", z1[0], z[b, :, :ny], STAGE_TOL)
                assert_close(f"z[{b}] vs reference", g["z"][b, :, :ny], z[b, :, :ny], STAGE_TOL)
        finally:
            m.close()
    finally:
        hip_lib.lib.vits_debug_poison_workspace(0)
