"""GPU tests of the mono_layer_* flows (flow_type 4 = mono_layer_inter_residual, 5 = mono_layer_post_residual):
mono_couple_kernel on its own against float64 numpy, the flow stage against the float64 restatement tests/flow_ref.py at 1, 3 and
4 flows (the Flip parity) and against fixtures computed by the reference's own SynthesizerTrn (tools/gen_golden_mono_flows.py), the
whole path on a poisoned workspace, the fast path, streaming, split-bf16 convs, the persistent flow program (never taken) and the
loader's refusals.  Tolerances are those of tests/test_flow_types_gpu.py."""
import ctypes
import os
import tempfile

import numpy as np
import pytest

from conftest import assert_close, golden

pytestmark = pytest.mark.gpu

STAGE_TOL = 1e-4
E2E_TOL = 5e-4
KINDS = ("monointer", "monopost")
FLOW_TYPE = {"monointer": 4, "monopost": 5}


def _hp(kind, default=False, n_flows=None):
    from vosk_tts_amd import weights as W

    if kind == "monointer":
        hp = W.mono_inter_hparams() if default else W.tiny_mono_inter_hparams()
    else:
        hp = W.mono_post_hparams() if default else W.tiny_mono_post_hparams()
    if n_flows is not None:
        hp.flow_n_flows = n_flows
    return hp


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


def _mono_couple(lib, h, u, Wm, bias, lengths, mode):
    fn = lib.vits_debug_mono_couple
    fn.restype = ctypes.c_int
    fp = ctypes.POINTER(ctypes.c_float)
    fn.argtypes = [ctypes.c_int, fp, fp, fp, fp, ctypes.POINTER(ctypes.c_int64), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                   ctypes.c_int32, fp]
    B, C, T = h.shape
    h, u, Wm, bias = (np.ascontiguousarray(a, np.float32) for a in (h, u, Wm, bias))
    ln = np.ascontiguousarray(lengths, np.int64)
    z = np.empty((B, 2 * C, T), np.float32)
    rc = fn(0, h.ctypes.data_as(fp), u.ctypes.data_as(fp), Wm.ctypes.data_as(fp), bias.ctypes.data_as(fp),
            ln.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), B, C, T, mode, z.ctypes.data_as(fp))
    assert rc == 0, rc
    return z


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("half", [32, 96, 160, 192])
def test_mono_couple_against_float64(hip_lib, half, mode):
    """One row tile per wave pair (32), the default size (96), an odd tile count (160), the maximum (192); T below, at and across the
    32-column tile; ragged B=3 with one item of length 1.  The x1 half past len is exactly 0; the x0 half passes through everywhere."""
    rng = np.random.default_rng(half * 10 + mode)
    s = 0.5 if mode else 1.0
    Wm = rng.standard_normal((half, half)).astype(np.float32) / np.sqrt(half)
    bias = rng.standard_normal(half).astype(np.float32) * 0.1
    for T in (1, 5, 33, 65, 300):
        lengths = np.array([T, 1, max(1, T // 2 + 1)], np.int64)
        h = rng.standard_normal((3, half, T)).astype(np.float32)
        u = rng.standard_normal((3, 2 * half, T)).astype(np.float32)
        got = _mono_couple(hip_lib.lib, h, u, Wm, bias, lengths, mode)
        m = np.einsum("rk,bkt->brt", Wm.astype(np.float64), h.astype(np.float64)) + bias.astype(np.float64)[None, :, None]
        want = np.concatenate([u[:, :half].astype(np.float64) * s, (u[:, half:].astype(np.float64) - m) * s], axis=1)
        for b, n in enumerate(lengths):
            want[b, half:, int(n):] = 0.0
        assert_close(f"mono couple half {half} T {T} mode {mode}", want, got, 1e-5)
        for b, n in enumerate(lengths):
            assert np.all(got[b, half:, int(n):] == 0.0)
            assert np.array_equal(got[b, :half], u[b, :half] * np.float32(s))


LENGTHS_B3 = np.array([70, 1, 33], np.int64)
SID_B3 = np.array([1, 4, 2], np.int64)


@pytest.fixture(scope="module")
def flow_ref_cases():
    """(kind, n_flows) -> (z_p, float64 z of tests/flow_ref.py), computed once and shared by the B=3 and the B=1 test"""
    import flow_ref

    from vosk_tts_amd import weights as W

    cache = {}

    def get(kind, n_flows):
        if (kind, n_flows) not in cache:
            hp = _hp(kind, n_flows=n_flows)
            rng = np.random.default_rng(100 + n_flows)
            z_p = rng.standard_normal((3, hp.inter_channels, int(LENGTHS_B3.max()))).astype(np.float32)
            z = flow_ref.flow_reverse(hp, W.make_synthetic_weights(hp, 1234), z_p, LENGTHS_B3, SID_B3)
            z.setflags(write=False)
            cache[(kind, n_flows)] = (z_p, z)
        return cache[(kind, n_flows)]

    return get


@pytest.mark.parametrize("n_flows", [1, 3, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_flow_stage_against_flow_ref(hip_lib, flow_ref_cases, kind, n_flows):
    """An odd and an even number of flows, and one: a Flip on the wrong side of a mono layer cannot cancel out.  Ragged B=3 with an
    item of length 1, then every item alone at B=1."""
    from vosk_tts_amd import weights as W

    z_p, want = flow_ref_cases(kind, n_flows)
    m = hip_lib.create(W.synthetic_blob(_hp(kind, n_flows=n_flows), 1234), 0)
    try:
        z = m.flow(z_p, LENGTHS_B3, SID_B3)
        for b, n in enumerate(int(v) for v in LENGTHS_B3):
            assert_close(f"B=3 z[{b}]", want[b, :, :n], z[b, :, :n], STAGE_TOL)
            z1 = m.flow(np.ascontiguousarray(z_p[b:b + 1, :, :n]), LENGTHS_B3[b:b + 1], SID_B3[b:b + 1])
            assert_close(f"B=1 z[{b}]", want[b, :, :n], z1[0], STAGE_TOL)
    finally:
        m.close()


@pytest.mark.parametrize("kind", KINDS)
def test_flow_stage_tiny_ragged_b3(models, kind):
    g = golden(f"flow_{kind}_tiny_b3")
    z = models[kind].flow(g["z_p"], g["y_lengths"], g["sid"])
    for b, n in enumerate(g["y_lengths"]):
        assert_close(f"z[{b}]", g["z"][b, :, :n], z[b, :, :n], STAGE_TOL)


@pytest.mark.parametrize("kind", KINDS)
def test_flow_stage_default_size(default_models, kind):
    """Default geometry (mono layer: 96 channels, head dim 48) at B=2 ragged and each item alone at B=1."""
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


def test_mono_flows_never_run_the_persistent_flow_program(hip_lib, default_models):
    fn = hip_lib.lib.vits_debug_persist_runs
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p]
    rng = np.random.default_rng(4)
    z_p = rng.standard_normal((1, 192, 150)).astype(np.float32)
    for kind in KINDS:
        m = default_models[kind]
        r0 = int(fn(m._h))
        z = m.flow(z_p, np.array([150], np.int64), np.array([3], np.int64))
        assert np.isfinite(z).all()
        assert int(fn(m._h)) == r0, (m.hp.flow_type, int(fn(m._h)) - r0)


def test_unsupported_mono_geometries_are_refused(hip_lib):
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.capi import VitsError

    hp = W.tiny_mono_post_hparams()
    t = W.make_synthetic_weights(hp, 1)
    raw = bytearray(W.pack_blob(hp, t))
    off = 12 + W.HParams.flow_type.offset
    raw[off:off + 4] = (6).to_bytes(4, "little")  # (pack_blob validates; a hand-edited blob reaches vits_create)
    with pytest.raises(VitsError) as e:
        hip_lib.create(bytes(raw), 0)
    assert e.value.code == 4
    for kind in KINDS:
        bad = _hp(kind)
        bad.inter_channels = 96  # head dim 24
        raw = bytearray(W.pack_blob(hp, t))
        raw[12:12 + len(bytes(bad))] = bytes(bad)
        with pytest.raises(VitsError) as e:
            hip_lib.create(bytes(raw), 0)
        assert e.value.code == 4


@pytest.mark.parametrize("kind", KINDS)
def test_a_mono_voice_synthesizes_through_the_public_api(kind):
    """Model -> Synth.synth_audio / synth_stream on a voice directory whose blob has the mono flow."""
    from vosk_tts_amd import Model, Synth
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.toymodel import PHONEMES, write_toy_model

    hp = W.tiny_hparams(n_vocab=len(PHONEMES))
    hp.flow_type = FLOW_TYPE[kind]
    with tempfile.TemporaryDirectory() as d:
        write_toy_model(d, hp)
        assert W.unpack_blob(open(os.path.join(d, "model.vitsw"), "rb").read())[0].flow_type == FLOW_TYPE[kind]
        synth = Synth(Model(model_path=d, device=0))
        pcm = synth.synth_audio("прив+ет, м+ир!", speaker_id=2)
        assert pcm.dtype == np.int16 and pcm.ndim == 1 and pcm.size > 0 and pcm.size % 256 == 0 and np.abs(pcm).max() > 0
        chunks = list(synth.synth_stream("прив+ет, м+ир!", speaker_id=2, chunk_frames=16))
        assert chunks and all(c.dtype == np.int16 for c in chunks) and sum(c.size for c in chunks) % 256 == 0
