"""GPU tests of the fused column steps of the duration predictor's step program (csrc/persist.hip.h PF_MV, csrc/persist_plan.hip.h
seg_sdp): one step per DDSConv layer (finish the previous layer, depthwise conv, LN1, GELU and the layer's 1x1 conv as a matrix-vector
product of the worker's column), dp.proj behind the last finish, ConvFlow.proj + the inverse spline of one column behind the last
finish of a ConvFlow stack.

The fused form needs ceil(dp_filter_channels / 64) workers per column and uses min(4, workers / padded columns) of them
(persist_sdp_split): with 256 workers, 256 channels are fused up to 64 tokens (4 workers per column), 192 channels up to 80 (4 per column up
to 64 tokens, 3 from 65 on), 64 channels at every length of one round.  Longer sequences keep the two-step form; both are checked
against the CPU oracle and the launch path (vits_debug_persist(0))."""
import ctypes

import numpy as np
import pytest

from conftest import assert_close

pytestmark = pytest.mark.gpu

STAGE_TOL = 1e-4
SCALES = np.array([0.667, 1.0, 0.8], np.float32)


def _persist_runs(hip_lib, model):
    """completed persistent launches of `model` so far: a stage that fell back to launches adds none"""
    lib = hip_lib.lib
    lib.vits_debug_persist_runs.restype = ctypes.c_int
    lib.vits_debug_persist_runs.argtypes = [ctypes.c_void_p]
    return int(lib.vits_debug_persist_runs(model._h))


def _check_duration(hip_lib, hip, oracle, T, seed):
    """lengths T, T - 1 and (T + 1) // 2, another speaker in every call, two forwards of the program, the launch path, the oracle"""
    H = hip.hp.hidden_channels
    rng = np.random.default_rng(seed)
    for it, L in enumerate(sorted({T, max(1, T - 1), (T + 1) // 2}, reverse=True)):
        x = rng.standard_normal((1, H, T)).astype(np.float32)
        lens = np.array([L], np.int64)
        x *= (np.arange(T)[None, None, :] < L)
        sid = np.array([it + 2], np.int64)
        noise = rng.standard_normal((1, 2, T)).astype(np.float32)
        want = oracle.duration(x, lens, sid, noise, 0.8)
        try:
            hip_lib.lib.vits_debug_persist(7)
            r0 = _persist_runs(hip_lib, hip)
            got = hip.duration(x, lens, sid, noise, 0.8)
            got2 = hip.duration(x, lens, sid, noise, 0.8)
            assert _persist_runs(hip_lib, hip) == r0 + 2, "the persistent program did not run"
            hip_lib.lib.vits_debug_persist(0)
            base = hip.duration(x, lens, sid, noise, 0.8)
        finally:
            hip_lib.lib.vits_debug_persist(7)
        m = np.arange(T)[None, :] < L
        assert np.array_equal(got, got2), f"T={T} L={L}: two forwards on the same inputs differ"
        assert np.all(got[~m] == 0), f"T={T} L={L}: logw is not zero on masked columns"
        assert_close(f"logw (T={T}, L={L}) program vs oracle", want * m, got * m, STAGE_TOL)
        assert_close(f"logw (T={T}, L={L}) program vs launch path", base * m, got * m, STAGE_TOL)


# 1 ... 28: with dilations 1 / 3 / 9 the t +- d neighbours fall outside the sequence, on the mask edge and just inside.
# 64 | 65: the last length of the fused form at the default 256 filter channels (4 workers per column need 64 padded columns) and the
# first of the two-step form; 80 | 81 and 128 | 129: column tiles end, two-step form.
@pytest.mark.parametrize("T", [1, 2, 4, 9, 10, 19, 28, 64, 65, 80, 81, 128, 129])
def test_fused_duration_stage(hip_lib, hip_default, oracle_default, T):
    _check_duration(hip_lib, hip_default, oracle_default, T, 7100 + T)


GEOMETRIES = {
    "D64": dict(dp_filter_channels=64),                        # 2 dwordx4 rows per wave, 16 output channels per worker
    "D192_L2": dict(dp_filter_channels=192, dp_dds_layers=2),  # 48 output channels per worker; 3 workers per column from 65 tokens on
    "L1": dict(dp_dds_layers=1),                               # a stack is one layer step + its end
    "F2": dict(dp_n_flows=2),                                  # one ConvFlow: its spline step is the last one and writes logw
}
_models = {}


@pytest.fixture
def geometry_models(request, hip_lib, oracle_lib):
    """(HIP model, oracle model) of default_hparams() with the named changes, both from the same synthetic blob; built once"""
    from vosk_tts_amd import weights as W

    name = request.param
    if name not in _models:
        hp = W.default_hparams()
        for k, v in GEOMETRIES[name].items():
            setattr(hp, k, v)
        blob = W.synthetic_blob(hp, 4321)
        _models[name] = (hip_lib.create(blob, 0), oracle_lib.create(blob))
    return _models[name]


# (the default voice is the 256-channel, 3-layer, 4-flow geometry: 256 channels = PS_MAXC, 8 dwordx4 rows per wave = all the registers of
# the request.)  192 channels at 65 / 80 tokens: three workers per column, 64 output channels each; at 81 the two-step form.  256 channels
# at 65 and more (above) and 192 at 81: models the fused form cannot take at that length still match through the old form.
@pytest.mark.parametrize("geometry_models,T", [(g, T) for g in GEOMETRIES for T in (5, 17, 50)] + [("D192_L2", 65), ("D192_L2", 80), ("D192_L2", 81)],
                         indirect=["geometry_models"])
def test_fused_duration_other_geometries(hip_lib, geometry_models, T):
    hip, oracle = geometry_models
    _check_duration(hip_lib, hip, oracle, T, 7300 + T)


# seeds for which every duration of the oracle is decided at least 1e-3 away from an integer (checked below from the oracle's logw)
FREE_SEEDS = {1: 8101, 17: 8217, 50: 8150}  # (closest pre-ceil value of the oracle: 0.35 / 0.049 / 0.024 from an integer)


@pytest.mark.parametrize("Tx", [1, 17, 50])
def test_free_running_durations_through_fused_front_program(hip_lib, hip_default, oracle_default, Tx):
    """vits_synthesize without pinned durations: the front program (text encoder, fused duration predictor, PK_DUR) decides the frame
    count.  Durations are ceil(exp(logw) * length_scale): a sum in another order may flip a ceil that sits on an integer, so the inputs
    are chosen (and checked here, from the oracle's logw) to keep every pre-ceil value >= 1e-3 away from one."""
    rng = np.random.default_rng(FREE_SEEDS[Tx])
    ids = rng.integers(1, 62, size=(1, Tx)).astype(np.int64)
    lens = np.array([Tx], np.int64)
    sid = np.array([6], np.int64)
    noise_dp = rng.standard_normal((1, 2, Tx)).astype(np.float32)
    x, _, _ = oracle_default.text_encoder(ids, lens, sid)
    w = np.exp(oracle_default.duration(x, lens, sid, noise_dp, float(SCALES[2])).astype(np.float64)) * float(SCALES[1])
    assert np.abs(w - np.round(w)).min() >= 1e-3, f"a duration of this input sits on an integer: {w}"
    try:
        hip_lib.lib.vits_debug_persist(7)
        r0 = _persist_runs(hip_lib, hip_default)
        got, gl = hip_default.synthesize(ids, lens, SCALES, sid, noise_dp=noise_dp, seed=33)
        got2, gl2 = hip_default.synthesize(ids, lens, SCALES, sid, noise_dp=noise_dp, seed=33)
        assert _persist_runs(hip_lib, hip_default) >= r0 + 2, "the front program did not run"
        hip_lib.lib.vits_debug_persist(0)
        base, bl = hip_default.synthesize(ids, lens, SCALES, sid, noise_dp=noise_dp, seed=33)
    finally:
        hip_lib.lib.vits_debug_persist(7)
    assert int(gl[0]) == int(np.ceil(w).sum()) * hip_default.hp.hop_length, f"frame count {gl} against the oracle's durations {np.ceil(w).sum()}"
    assert np.array_equal(gl, bl) and np.array_equal(gl, gl2), f"frame counts differ: {gl} (program) / {bl} (launch path)"
    assert np.array_equal(got, got2), "two forwards on the same inputs differ"
    assert_close(f"audio (T_x={Tx}) program vs launch path", base, got, 2e-4)
