"""Tests of the fused attention half of the encoder layers in the step programs (csrc/persist.hip.h PK_MERGE | PF_MV,
csrc/persist_plan.hip.h persist_attn_form): the merge column step also runs conv_o + the residual on its column as a matrix-vector
product.  Form A: up to 4 workers per column, each with ceil(H / w) <= 64 output channels, LayerNorm 1 stays a step (H = 192 with 256
workers: 4 x 48 channels up to 64 padded columns, 3 x 64 up to 80).  Form B: one worker per column runs all H channels in passes of 64
and ends with LayerNorm 1 (up to 256 columns).  vits_debug_persist_attn_fused picks the form: 0 = the planner's rule, 1 = never,
2 = form A only, 3 = form B wherever it fits; where a mode cannot apply the three-step form runs and the case still has to pass.

Every comparison: the program (twice, bit-equal) against the CPU oracle and against the launch path (vits_debug_persist(0)) at the
tolerance of the existing stage tests, masked columns exactly zero, lengths T, T - 1 and (T + 1) // 2 inside a T-wide tensor."""
import ctypes

import numpy as np
import pytest

from conftest import assert_close

STAGE_TOL = 1e-4
SCALES = np.array([0.667, 1.0, 0.8], np.float32)
gpu = pytest.mark.gpu


def _persist_runs(hip_lib, model):
    lib = hip_lib.lib
    lib.vits_debug_persist_runs.restype = ctypes.c_int
    lib.vits_debug_persist_runs.argtypes = [ctypes.c_void_p]
    return int(lib.vits_debug_persist_runs(model._h))


def _last_steps(hip_lib):
    fn = hip_lib.lib.vits_debug_persist_last_steps
    fn.restype = ctypes.c_int
    fn.argtypes = []
    return int(fn())


def _form(hip_lib, H, T, mode, P=256):
    fn = hip_lib.lib.vits_debug_persist_attn_form
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 4
    return int(fn(H, (T + 15) // 16 * 16, P, mode))


_plain_steps = {}  # (model key, stage, T) -> steps of the stage's program with no fused step (mode 1)


def _assert_steps(hip_lib, key, stage, hip, T, mode, layers, run):
    """The program that just ran (`run` runs the stage once more under the mode in effect) has the steps of the form the planner's rule
    names: against the never-fused program of the same model and length, form A saves one step per encoder layer (conv_o), form B two
    (conv_o and LayerNorm 1).  Fails when a fused form silently falls back to the three steps."""
    k = (key, stage, T)
    if k not in _plain_steps:
        hip_lib.lib.vits_debug_persist_attn_fused(1)
        run()
        _plain_steps[k] = _last_steps(hip_lib)
        hip_lib.lib.vits_debug_persist_attn_fused(mode)
    run()
    form = _form(hip_lib, hip.hp.hidden_channels, T, mode)
    saved = layers * (0 if form == 0 else (1 if form > 0 else 2))
    assert _last_steps(hip_lib) == _plain_steps[k] - saved, (
        f"{stage} T={T} mode={mode}: {_last_steps(hip_lib)} steps, never-fused program {_plain_steps[k]}, form {form} saves {saved}")


def _lengths(T):
    return sorted({T, max(1, T - 1), (T + 1) // 2}, reverse=True)


_enc_refs = {}  # (model key, T, L) -> (inputs, oracle outputs, launch-path outputs): computed once, shared by the four modes


def _enc_reference(hip_lib, key, hip, oracle, T, L, it):
    k = (key, T, L)
    if k not in _enc_refs:
        rng = np.random.default_rng(9100 + 7 * T + L)
        ids = rng.integers(1, hip.hp.n_vocab, size=(1, T)).astype(np.int64)
        lens = np.array([L], np.int64)
        sid = np.array([it + 2], np.int64)
        want = oracle.text_encoder(ids, lens, sid)
        try:
            hip_lib.lib.vits_debug_persist(0)
            base = hip.text_encoder(ids, lens, sid)
        finally:
            hip_lib.lib.vits_debug_persist(7)
        _enc_refs[k] = (ids, lens, sid, want, base)
    return _enc_refs[k]


def _check_encoder(hip_lib, key, hip, oracle, T, mode):
    for it, L in enumerate(_lengths(T)):
        ids, lens, sid, want, base = _enc_reference(hip_lib, key, hip, oracle, T, L, it)
        try:
            hip_lib.lib.vits_debug_persist_attn_fused(mode)
            hip_lib.lib.vits_debug_persist(7)
            r0 = _persist_runs(hip_lib, hip)
            got = hip.text_encoder(ids, lens, sid)
            got2 = hip.text_encoder(ids, lens, sid)
            assert _persist_runs(hip_lib, hip) == r0 + 2, "the persistent program did not run"
            if it == 0:
                _assert_steps(hip_lib, key, "enc", hip, T, mode, hip.hp.n_layers, lambda: hip.text_encoder(ids, lens, sid))
        finally:
            hip_lib.lib.vits_debug_persist_attn_fused(0)
        mask = np.arange(T)[None, None, :] < L
        for name, w, g, g2, b in zip(("x", "m_p", "logs_p"), want, got, got2, base):
            tag = f"{name} (T={T}, L={L}, mode={mode})"
            assert np.array_equal(g, g2), f"{tag}: two forwards on the same inputs differ"
            assert np.all(g[np.broadcast_to(~mask, g.shape)] == 0), f"{tag}: masked columns are not zero"
            assert_close(f"{tag} program vs oracle", w * mask, g * mask, STAGE_TOL)
            assert_close(f"{tag} program vs launch path", b * mask, g * mask, STAGE_TOL)


_sid = [1]


def _next_sid():
    """a speaker id that differs from the previous comparison's"""
    _sid[0] = _sid[0] % 9 + 2
    return np.array([_sid[0]], np.int64)


def _check_flow(hip_lib, hip, oracle, T, mode, key="default"):
    I = hip.hp.inter_channels
    for it, L in enumerate(_lengths(T)):
        rng = np.random.default_rng(9300 + 7 * T + L)
        z_p = rng.standard_normal((1, I, T)).astype(np.float32)
        lens = np.array([L], np.int64)
        sid = _next_sid()
        want = oracle.flow(z_p, lens, sid)
        try:
            hip_lib.lib.vits_debug_persist_attn_fused(mode)
            hip_lib.lib.vits_debug_persist(7)
            r0 = _persist_runs(hip_lib, hip)
            got = hip.flow(z_p, lens, sid)
            got2 = hip.flow(z_p, lens, sid)
            assert _persist_runs(hip_lib, hip) == r0 + 2, "the persistent program did not run"
            if it == 0:
                _assert_steps(hip_lib, key, "flow", hip, T, mode, hip.hp.flow_n_flows, lambda: hip.flow(z_p, lens, sid))
            hip_lib.lib.vits_debug_persist(0)
            base = hip.flow(z_p, lens, sid)
        finally:
            hip_lib.lib.vits_debug_persist(7)
            hip_lib.lib.vits_debug_persist_attn_fused(0)
        mask = np.arange(T)[None, None, :] < L
        tag = f"z (T={T}, L={L}, mode={mode})"
        assert np.array_equal(got, got2), f"{tag}: two forwards on the same inputs differ"
        assert np.all(got[np.broadcast_to(~mask, got.shape)] == 0), f"{tag}: masked columns are not zero"
        assert_close(f"{tag} program vs oracle", want * mask, got * mask, STAGE_TOL)
        assert_close(f"{tag} program vs launch path", base * mask, got * mask, STAGE_TOL)


# 15 | 16 | 17, 64 | 65, 80 | 81: column tiles end; 4 workers of 48 channels up to 64 columns, 3 workers of 64 channels at 65 ... 80, 81 is
# the first length outside form A; 129: form B where the rule picks it, the three-step form otherwise
@gpu
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("T", [1, 2, 15, 16, 17, 50, 64, 65, 80, 81, 129])
def test_fused_text_encoder(hip_lib, hip_default, oracle_default, T, mode):
    _check_encoder(hip_lib, "default", hip_default, oracle_default, T, mode)


# 256 | 257: the last length of form B (one round of columns) and the first no fused form takes
@gpu
@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("T", [1, 16, 17, 64, 65, 80, 81, 150, 256, 257])
def test_fused_flow(hip_lib, hip_default, oracle_default, T, mode):
    _check_flow(hip_lib, hip_default, oracle_default, T, mode)


@gpu
def test_step_counts_of_the_default_voice(hip_lib, hip_default):
    """the absolute figures: 6 text-encoder layers of 8 / 7 / 6 steps + embedding and proj, 4 coupling layers of 17 / 16 / 15 steps"""
    rng = np.random.default_rng(9400)
    sid = np.array([3], np.int64)

    def steps(mode, run):
        try:
            hip_lib.lib.vits_debug_persist_attn_fused(mode)
            hip_lib.lib.vits_debug_persist(7)
            run()
            return _last_steps(hip_lib)
        finally:
            hip_lib.lib.vits_debug_persist_attn_fused(0)

    ids = rng.integers(1, 62, size=(1, 50)).astype(np.int64)
    enc = lambda: hip_default.text_encoder(ids, np.array([50], np.int64), sid)
    assert [steps(m, enc) for m in (1, 2, 0, 3)] == [50, 44, 38, 38]
    for T, want in ((150, [68, 68, 60, 60]), (64, [68, 64, 60, 60]), (257, None)):
        z_p = rng.standard_normal((1, hip_default.hp.inter_channels, T)).astype(np.float32)
        flow = lambda: hip_default.flow(z_p, np.array([T], np.int64), sid)
        got = [steps(m, flow) for m in (1, 2, 0, 3)]
        if want is None:
            assert len(set(got)) == 1, f"no fused form fits {T} columns: {got}"
        else:
            assert got == want, (T, got)


def _h128_hparams():
    from vosk_tts_amd import weights as W

    hp = W.heads4_hparams()
    hp.n_heads = 2
    return hp


def _heads4_hparams():
    from vosk_tts_amd import weights as W

    return W.heads4_hparams()


# hidden 128, 2 heads of 64: form A has 4 x 32 channels (up to 64 columns) or 2 x 64, form B two passes;  4 heads of 32 at hidden 128:
# the merge's (head, d) threads against the conv's channel threads
GEOMETRIES = {"H128": _h128_hparams, "heads4": _heads4_hparams}
_models = {}


@pytest.fixture
def geometry_models(request, hip_lib, oracle_lib):
    from vosk_tts_amd import weights as W

    name = request.param
    if name not in _models:
        blob = W.synthetic_blob(GEOMETRIES[name](), 4321)
        _models[name] = (hip_lib.create(blob, 0), oracle_lib.create(blob))
    return (name,) + _models[name]


@gpu
@pytest.mark.parametrize("mode", [0, 2, 3])
@pytest.mark.parametrize("geometry_models,T", [(g, T) for g in GEOMETRIES for T in (5, 17, 50)], indirect=["geometry_models"])
def test_fused_other_geometries(hip_lib, geometry_models, T, mode):
    name, hip, oracle = geometry_models
    _check_encoder(hip_lib, name, hip, oracle, T, mode)
    _check_flow(hip_lib, hip, oracle, T, mode, name)


@gpu
def test_synthesize_program_vs_launch_path(hip_lib, hip_default):
    """one whole forward of 50 tokens with pinned durations (150 frames; the rule's form in the text encoder and in the flow)"""
    rng = np.random.default_rng(9500)
    Tx = 50
    ids = rng.integers(1, 62, size=(1, Tx)).astype(np.int64)
    lens = np.array([Tx], np.int64)
    sid = np.array([6], np.int64)
    dur = np.full((1, Tx), 3, np.int32)
    try:
        hip_lib.lib.vits_debug_persist(7)
        r0 = _persist_runs(hip_lib, hip_default)
        got, gl = hip_default.synthesize(ids, lens, SCALES, sid, forced_durations=dur, seed=33)
        got2, gl2 = hip_default.synthesize(ids, lens, SCALES, sid, forced_durations=dur, seed=33)
        assert _persist_runs(hip_lib, hip_default) >= r0 + 2, "the programs did not run"
        hip_lib.lib.vits_debug_persist(0)
        base, bl = hip_default.synthesize(ids, lens, SCALES, sid, forced_durations=dur, seed=33)
    finally:
        hip_lib.lib.vits_debug_persist(7)
    assert int(gl[0]) == 150 * hip_default.hp.hop_length
    assert np.array_equal(gl, bl) and np.array_equal(gl, gl2)
    assert np.array_equal(got, got2), "two forwards on the same inputs differ"
    assert_close("audio program vs launch path", base, got, 2e-4)


# ---- the planner's rule (host arithmetic, no device): every (H, padded columns) the cases above run, 256 workers
def _rule(H, Tp, P, mode):
    """the forms as the issue states them: form A with w = min(4, workers / padded columns) workers of ceil(H / w) <= 64 channels, form B
    (-1) with one worker per column up to one round of columns, else the three steps (0)"""
    w = min(4, P // Tp) if Tp <= P else 0
    a = w if w >= 1 and -(-H // w) <= 64 else 0
    b = -1 if Tp <= P and H % 32 == 0 and H <= 256 else 0
    if mode == 1:
        return 0
    return a if mode == 2 else b  # modes 0 and 3: the rule is form B wherever it fits (form A alone measured slower than the parent at c2)


@pytest.mark.parametrize("H", [128, 192])
def test_planner_rule(hip_lib, H):
    for T in (1, 2, 5, 15, 16, 17, 50, 64, 65, 80, 81, 129, 150, 256, 257):
        Tp = (T + 15) // 16 * 16
        for mode in (0, 1, 2, 3):
            assert _form(hip_lib, H, T, mode) == _rule(H, Tp, 256, mode), (H, T, mode)
    # the figures of the default voice (H = 192): 4 x 48 channels up to 64 columns, 3 x 64 up to 80, nothing of form A beyond
    if H == 192:
        assert [_form(hip_lib, H, T, 2) for T in (1, 64, 65, 80, 81, 129)] == [4, 4, 3, 3, 0, 0]
        assert [_form(hip_lib, H, T, 3) for T in (1, 150, 256, 257)] == [-1, -1, -1, 0]
    else:
        # H = 128: 4 x 32 channels up to 64 columns, 3 x 43 up to 80, 2 x 64 up to 128
        assert [_form(hip_lib, H, T, 2) for T in (5, 64, 65, 97, 128, 129)] == [4, 4, 3, 2, 2, 0]
