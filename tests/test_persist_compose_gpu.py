"""GPU tests of the shortened chain of dependent steps in the single-utterance step programs (csrc/persist_plan.hip.h):

* the flow's q | k | v composed with the coupling layer's `pre` conv (CouplingW::qkv_pre), `pre` itself sharing that step's slot;
* the text encoder's proj and the duration predictor's pre in one slot of the programs that run both.

Against the launch path (vits_debug_persist(0)) and, stage by stage, the CPU oracle, at the sizes where a column tile ends, the length
mask falls inside a tile, and the items of a shared slot stop fitting the workers without coarser row-block groups."""
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


@pytest.mark.parametrize("T", [1, 15, 16, 17, 33])
def test_flow_with_composed_qkv(hip_lib, hip_default, oracle_default, T):
    """The flow program whose q | k | v reads the previous coupling output through (W_qkv W_pre): lengths at the tile edge and with the
    mask inside a tile (on masked columns the composed bias differs from qkv(0): nothing of it may reach a valid column)."""
    rng = np.random.default_rng(4100 + T)
    for it, L in enumerate(sorted({T, max(1, T - 1), (T + 1) // 2}, reverse=True)):
        z_p = rng.standard_normal((1, 192, T)).astype(np.float32)
        lens = np.array([L], np.int64)
        sid = np.array([it + 4], np.int64)
        want = oracle_default.flow(z_p, lens, sid)
        try:
            hip_lib.lib.vits_debug_persist(7)
            r0 = _persist_runs(hip_lib, hip_default)
            got = hip_default.flow(z_p, lens, sid)
            got2 = hip_default.flow(z_p, lens, sid)
            assert _persist_runs(hip_lib, hip_default) == r0 + 2, "the persistent program did not run"
            hip_lib.lib.vits_debug_persist(0)
            base = hip_default.flow(z_p, lens, sid)
        finally:
            hip_lib.lib.vits_debug_persist(7)
        m = (np.arange(T)[None, None, :] < L)
        assert np.array_equal(got, got2), "two forwards on the same inputs differ"
        assert_close(f"z (T={T}, L={L}) program vs oracle", want * m, got * m, STAGE_TOL)
        assert_close(f"z (T={T}, L={L}) program vs launch path", base * m, got * m, STAGE_TOL)


@pytest.mark.parametrize("Tx", [1, 16, 17, 100, 200])
def test_front_program_with_proj_and_dp_pre_in_one_slot(hip_lib, hip_default, Tx):
    """A free-running utterance through the host entry point: its front program runs the text encoder's proj and the duration
    predictor's pre (both read the encoder output, neither needs the other) in one slot.  The durations it decides and the audio must
    be the launch path's: 16 / 17 tokens end and begin a column tile, from 100 tokens on the two steps fit the workers only with coarser
    row-block groups."""
    rng = np.random.default_rng(6300 + Tx)
    ids = rng.integers(1, 62, size=(1, Tx)).astype(np.int64)
    lens = np.array([Tx], np.int64)
    sid = np.array([5], np.int64)
    try:
        hip_lib.lib.vits_debug_persist(7)
        r0 = _persist_runs(hip_lib, hip_default)
        got, gl = hip_default.synthesize(ids, lens, SCALES, sid, seed=21)
        got2, gl2 = hip_default.synthesize(ids, lens, SCALES, sid, seed=21)
        assert _persist_runs(hip_lib, hip_default) >= r0 + 2, "the front program did not run"
        hip_lib.lib.vits_debug_persist(0)
        base, bl = hip_default.synthesize(ids, lens, SCALES, sid, seed=21)
    finally:
        hip_lib.lib.vits_debug_persist(7)
    assert np.array_equal(gl, bl) and np.array_equal(gl, gl2), f"frame counts differ: {gl} (program) / {bl} (launch path)"
    assert np.array_equal(got, got2), "two forwards on the same inputs differ"
    assert_close(f"audio (T_x={Tx}) program vs launch path", base, got, 2e-4)
