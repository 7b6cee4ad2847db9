"""GPU tests of the deterministic duration predictor (use_sdp false: DurationPredictor, models.py:104-139; hparams.dp_n_flows == 0):
the duration stage against fixtures computed by the reference's own SynthesizerTrn(use_sdp=False) (tools/gen_golden_dp_types.py) and
against a float64 numpy restatement, the whole path, ragged batches on poisoned workspaces, the fast path, device sessions, streaming,
split-bf16 convs, the ignored duration noise, the persistent programs and the Model / Synth API.  (The C oracle computes the stochastic
predictor only: these voices are pinned to the goldens and to the restatement below.)"""
import ctypes
import json
import os
import tempfile

import numpy as np
import pytest

from conftest import assert_close, golden

pytestmark = pytest.mark.gpu

STAGE_TOL = 1e-4
E2E_TOL = 5e-4
SCALES = [0.667, 1.0, 0.8]


def _variant(name):
    from vosk_tts_amd import weights as W

    hp = W.tiny_deterministic_dp_hparams()
    if name == "nocond":  # a single-speaker voice: no emb_g, no dp.cond
        hp.gin_channels, hp.n_speakers = 0, 0
    elif name == "d128":  # conv_2 narrow enough for norm_1 to be folded into its staging at few columns
        hp.dp_filter_channels = 128
    return hp


@pytest.fixture(scope="module")
def tiny(hip_lib):
    from vosk_tts_amd import weights as W

    m = hip_lib.create(W.synthetic_blob(W.tiny_deterministic_dp_hparams(), 1234), 0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def default_det(hip_lib):
    from vosk_tts_amd import weights as W

    m = hip_lib.create(W.synthetic_blob(W.deterministic_dp_hparams(), 1234), 0)
    yield m
    m.close()


def _conv(x, w, b):
    """Conv1d with 'same' zero padding, float64: x [B, C, T], w [O, C, K]"""
    K = w.shape[2]
    T = x.shape[2]
    xp = np.pad(x, ((0, 0), (0, 0), (K // 2, K // 2)))
    y = sum(np.einsum("oc,bct->bot", w[:, :, k], xp[:, :, k:k + T]) for k in range(K))
    return y + b[None, :, None]


def _ln(x, g, b):
    mu = x.mean(axis=1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=1, keepdims=True)
    return (x - mu) / np.sqrt(var + 1e-5) * g[None, :, None] + b[None, :, None]


def _dp_ref(t, x, lengths, sid):
    """DurationPredictor.forward (models.py:123-139) in float64"""
    t = {k: v.astype(np.float64) for k, v in t.items()}
    B, _, T = x.shape
    mask = (np.arange(T)[None, :] < np.asarray(lengths)[:, None]).astype(np.float64)[:, None, :]
    x = x.astype(np.float64)
    if "emb_g.weight" in t:
        g = t["emb_g.weight"][np.asarray(sid)]
        x = x + (g @ t["dp.cond.weight"][:, :, 0].T + t["dp.cond.bias"])[:, :, None]
    h = _ln(np.maximum(_conv(x * mask, t["dp.conv_1.weight"], t["dp.conv_1.bias"]), 0), t["dp.norm_1.gamma"], t["dp.norm_1.beta"])
    h = _ln(np.maximum(_conv(h * mask, t["dp.conv_2.weight"], t["dp.conv_2.bias"]), 0), t["dp.norm_2.gamma"], t["dp.norm_2.beta"])
    return (_conv(h * mask, t["dp.proj.weight"], t["dp.proj.bias"]) * mask)[:, 0]


def _noise(B, T, seed=0):
    return np.random.default_rng(seed).standard_normal((B, 2, T)).astype(np.float32)


@pytest.mark.parametrize("name", ["dp_det_tiny_b3", "dp_det_default_b2"])
def test_duration_stage_against_the_reference_module(tiny, default_det, name):
    g = golden(name)
    m = tiny if "tiny" in name else default_det
    logw = m.duration(g["x"], g["lengths"], g["sid"], _noise(*g["logw"].shape), 0.8)
    for b, n in enumerate(g["lengths"]):
        assert_close(f"{name} logw[{b}]", g["logw"][b, :n], logw[b, :n], STAGE_TOL)
        assert np.all(logw[b, n:] == 0.0)


@pytest.mark.parametrize("variant", ["tiny", "nocond", "d128"])
def test_duration_stage_against_float64(hip_lib, variant):
    from vosk_tts_amd import weights as W

    hp = _variant(variant)
    t = W.make_synthetic_weights(hp, 1234)
    m = hip_lib.create(W.pack_blob(hp, t), 0)
    try:
        rng = np.random.default_rng(17)
        for T in (1, 2, 3, 17, 50, 129, 512):
            for lengths in ([T], [T, max(1, T // 2), 1, max(1, T - 1)][: 4 if T > 2 else 2]):
                B = len(lengths)
                x = rng.standard_normal((B, hp.hidden_channels, T)).astype(np.float32)
                sid = np.arange(B, dtype=np.int64) % max(hp.n_speakers, 1)
                got = m.duration(x, np.asarray(lengths, np.int64), sid, _noise(B, T), 0.8)
                want = _dp_ref(t, x, lengths, sid)
                for b, n in enumerate(lengths):
                    assert_close(f"{variant} T {T} B {B} logw[{b}]", want[b, :n], got[b, :n], 1e-5)
                    assert np.all(got[b, n:] == 0.0), (variant, T, b)
    finally:
        m.close()


def _valid(audio, olen):
    a = np.array(audio, copy=True)
    for b, n in enumerate(olen):
        a[b, int(n):] = 0.0
    return a


def test_end_to_end_against_the_reference_module(hip_lib):
    """Forced durations with injected prior noise: the audio.  Free-running: the integer durations and y_lengths (the fixture's
    w * length_scale are all >= 1e-3 from an integer)."""
    from vosk_tts_amd import weights as W

    g = golden("dp_det_e2e_b3")
    hip_lib.lib.vits_debug_poison_workspace(1)
    try:
        m = hip_lib.create(W.synthetic_blob(W.tiny_deterministic_dp_hparams(), 1234), 0)
        try:
            audio, olen = m.synthesize(g["ids"], g["lengths"], g["scales"], g["sid"], noise_prior=g["noise_prior"],
                                       forced_durations=g["forced_durations"])
            x, m_p, logs_p = m.text_encoder(g["ids"], g["lengths"], g["sid"])
            logw = m.duration(x, g["lengths"], g["sid"], _noise(3, 14), 0.8)
            dur, ylen, _ = m.regulate(logw, None, g["lengths"], float(g["scales"][1]), m_p, logs_p, None, 0.0, int(g["y_lengths_free"].max()))
            _, olen_free = m.synthesize(g["ids"], g["lengths"], g["scales"], g["sid"], seed=3)
        finally:
            m.close()
    finally:
        hip_lib.lib.vits_debug_poison_workspace(0)
    assert np.array_equal(olen, g["y_lengths"] * 256)
    assert_close("audio (forced durations)", _valid(g["audio"], olen), _valid(audio, olen), E2E_TOL)
    for b, n in enumerate(g["lengths"]):
        assert_close(f"logw[{b}]", g["logw"][b, :n], logw[b, :n], STAGE_TOL)
    assert np.array_equal(dur, g["durations_free"])
    assert np.array_equal(ylen, g["y_lengths_free"])
    assert np.array_equal(olen_free, g["y_lengths_free"] * 256)


def _batch(rng, B=3, Tx=30):
    lengths = np.array([Tx, 9, 17, 1, 22, 30, 5, 12][:B], np.int64)
    ids = rng.integers(1, 20, size=(B, Tx)).astype(np.int64)
    return ids, lengths, (np.arange(B) % 5).astype(np.int64)


def test_ragged_batch_on_poisoned_workspace_equals_items_alone(hip_lib):
    from vosk_tts_amd import weights as W

    ids, lengths, sid = _batch(np.random.default_rng(8), B=4, Tx=40)
    hip_lib.lib.vits_debug_poison_workspace(1)
    try:
        m = hip_lib.create(W.synthetic_blob(W.tiny_deterministic_dp_hparams(), 1234), 0)
        try:
            a, la = m.synthesize(ids, lengths, SCALES, sid, seed=5, solo=True)
            for b, n in enumerate(lengths):
                a1, l1 = m.synthesize(ids[b:b + 1, :n], lengths[b:b + 1], SCALES, sid[b:b + 1], seed=5 + b)
                assert l1[0] == la[b], (b, l1, la)
                assert_close(f"item {b} in the batch vs alone", a1[0, :l1[0]], a[b, :la[b]], 1e-5)
        finally:
            m.close()
    finally:
        hip_lib.lib.vits_debug_poison_workspace(0)


def test_fast_path_equals_eager(hip_lib, tiny):
    for B in (1, 3):
        ids, lengths, sid = _batch(np.random.default_rng(3), B=B)
        out = []
        try:
            for on in (0, 1, 1):
                hip_lib.lib.vits_debug_fast_path(on)
                out.append(tiny.synthesize(ids, lengths, SCALES, sid, seed=6))
        finally:
            hip_lib.lib.vits_debug_fast_path(1)
        for a, la in out[1:]:
            assert np.array_equal(la, out[0][1])
            assert np.array_equal(_valid(a, la), _valid(out[0][0], la)), B


def test_device_session_equals_eager(tiny):
    """Free-running on a device session (the caller's frame capacity): the predictor runs inside the captured forward."""
    import torch

    from vosk_tts_amd.capi import VitsDeviceSession

    ids, lengths, sid = _batch(np.random.default_rng(12), B=3)
    B, Tx = ids.shape
    want, wl = tiny.synthesize(ids, lengths, np.asarray(SCALES, np.float32), sid, seed=9)
    Ty = int(wl.max()) // 256 + 8
    dev = torch.device("cuda", 0)
    d_ids, d_len, d_sid = (torch.from_numpy(a).to(dev) for a in (ids, lengths, sid))
    d_audio = torch.zeros((B, Ty * 256), dtype=torch.float32, device=dev)
    s = VitsDeviceSession(tiny, B, Tx, Ty)
    try:
        for use_graph in (True, False, True):
            s.set_options(use_graph=use_graph)
            d_audio.zero_()
            for _ in range(2):
                s.synthesize_device(d_ids.data_ptr(), d_len.data_ptr(), B, Tx, np.asarray(SCALES, np.float32), d_sid.data_ptr(), 0, Ty, 9,
                                    d_audio.data_ptr(), Ty * 256)
            s.sync()
            got = d_audio.cpu().numpy()
            for b in range(B):
                assert_close(f"device session item {b}", want[b, :wl[b]], got[b, :wl[b]], 1e-6)
    finally:
        s.close()


@pytest.mark.parametrize("chunk", [16, 37])
def test_streaming_chunks_equal_one_shot(tiny, chunk):
    rng = np.random.default_rng(11)
    Tx = 40
    ids = rng.integers(1, 20, size=(1, Tx)).astype(np.int64)
    one, lo = tiny.synthesize(ids, [Tx], SCALES, [2], seed=5)
    got = np.concatenate(list(tiny.stream(ids, SCALES, 2, chunk_frames=chunk, seed=5)))[None]
    assert got.shape == one.shape == (1, int(lo[0]))
    assert_close("stream vs one-shot", one, got, 2e-5)


def test_split_bf16_convs_stay_within_5e5_at_batch(hip_lib):
    from vosk_tts_amd import weights as W

    hp = W.tiny_deterministic_dp_hparams()
    t = W.make_synthetic_weights(hp, 1234)
    hp1 = W.HParams.from_buffer_copy(bytes(hp))
    hp1.conv_precision = 1
    m0, m1 = hip_lib.create(W.pack_blob(hp, t), 0), hip_lib.create(W.pack_blob(hp1, t), 0)
    try:
        rng = np.random.default_rng(21)
        ids, lengths, sid = _batch(rng, B=8, Tx=60)
        x, _, _ = m0.text_encoder(ids, lengths, sid)
        l0 = m0.duration(x, lengths, sid, _noise(8, 60), 0.8)
        l1 = m1.duration(x, lengths, sid, _noise(8, 60), 0.8)
        assert np.abs(l0 - l1).max() <= 5e-5
        dur = rng.integers(0, 5, size=ids.shape).astype(np.int32)
        a0, o0 = m0.synthesize(ids, lengths, SCALES, sid, forced_durations=dur, seed=2)
        a1, o1 = m1.synthesize(ids, lengths, SCALES, sid, forced_durations=dur, seed=2)
        assert np.array_equal(o0, o1)
        assert_close("bf16x3 vs fp32", _valid(a0, o0), _valid(a1, o1), 5e-5)
    finally:
        m0.close()
        m1.close()


def test_duration_noise_is_ignored(tiny):
    rng = np.random.default_rng(5)
    ids, lengths, sid = _batch(rng, B=2, Tx=20)
    a, la = tiny.synthesize(ids, lengths, [0.667, 1.0, 0.8], sid, seed=4)
    for scales, nd in (([0.667, 1.0, 0.0], None), ([0.667, 1.0, 1.7], _noise(2, 20, 1) * 3), ([0.667, 1.0, 0.8], _noise(2, 20, 2))):
        b, lb = tiny.synthesize(ids, lengths, scales, sid, seed=4, noise_dp=nd)
        assert np.array_equal(la, lb) and np.array_equal(a, b)
    x = rng.standard_normal((2, 64, 20)).astype(np.float32)
    w0 = tiny.duration(x, lengths, sid, _noise(2, 20, 3), 0.8)
    w1 = tiny.duration(x, lengths, sid, _noise(2, 20, 4) * 5, 0.0)
    assert np.array_equal(w0, w1)


def test_no_persistent_duration_program_for_deterministic_voices(hip_lib, hip_default, default_det):
    fn = hip_lib.lib.vits_debug_persist_runs
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p]
    rng = np.random.default_rng(4)
    x = rng.standard_normal((1, 192, 50)).astype(np.float32)
    for m, want in ((hip_default, True), (default_det, False)):
        r0 = int(fn(m._h))
        logw = m.duration(x, np.array([50], np.int64), np.array([3], np.int64), _noise(1, 50), 0.8)
        took = int(fn(m._h)) - r0
        assert np.isfinite(logw).all()
        assert (took > 0) == want, (m.hp.dp_n_flows, took)
    # the whole single-utterance forward still takes the text-encoder / flow programs
    ids = rng.integers(1, 62, size=(1, 50)).astype(np.int64)
    r0 = int(fn(default_det._h))
    default_det.synthesize(ids, [50], SCALES, [3], seed=1)
    assert int(fn(default_det._h)) > r0


def test_model_directory_with_use_sdp_false(hip_lib):
    """model.onnx + config.json {"model": {"use_sdp": false}} loads through Model and runs through Synth.synth_audio."""
    from vosk_tts_amd import Model, Synth
    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.session import VitsSession
    from vosk_tts_amd.toymodel import PHONEMES, write_toy_model

    hp = W.tiny_deterministic_dp_hparams(n_vocab=len(PHONEMES))
    with tempfile.TemporaryDirectory() as d:
        write_toy_model(d, hp)
        blob_path = os.path.join(d, "model.vitsw")
        _, tens = W.unpack_blob(open(blob_path, "rb").read())
        oi.write_minimal_onnx(os.path.join(d, "model.onnx"), dict(tens))
        os.remove(blob_path)
        with open(os.path.join(d, "config.json")) as f:
            cfg = json.load(f)
        cfg["model"] = {"use_sdp": False, "upsample_rates": [4, 4], "gen_istft_hop_size": 4, "subbands": 4}
        with open(os.path.join(d, "config.json"), "w") as f:
            json.dump(cfg, f, ensure_ascii=False)
        model = Model(model_path=d, device=0)
        synth = Synth(model)
        pcm = synth.synth_audio("привет мир", speaker_id=2)
        args, scale = synth._feed("привет мир", 2, None, None, None, None)
        ref = VitsSession(W.pack_blob(hp, tens), device=0)
        want = ref.run_pcm16(args, scale).squeeze()
        assert pcm.dtype == np.int16 and pcm.size > 0
        assert np.array_equal(pcm, want)
        cfg["model"]["use_sdp"] = True
        with open(os.path.join(d, "config.json"), "w") as f:
            json.dump(cfg, f, ensure_ascii=False)
        with pytest.raises(ValueError, match="use_sdp"):
            Model(model_path=d, device=0)
