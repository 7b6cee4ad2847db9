"""GPU tests of loudness normalisation (include/vits_loudness.h): the kernels through vits_op_loudness / vits_op_loudness_normalize
against the float64 restatement (tests/loudness_ref.py), the flag through the VITS and multistream entry points against the op on the
unflagged call's audio, and the Python layers.

Bounds.  |L_gpu - L_ref| <= 0.01 LU, a tenth of the meter tolerance of EBU Tech 3341; the peak is bit-equal to max |x| in fp32; a gain
that follows L is within 10^(0.01/20) - 1 of the restatement's, a gain that is a quotient of two fp32 numbers (ceiling / peak, P / peak)
within 4 fp32 ulp.  tests/test_loudness.py asserts, on the restatement alone, that no block of any input used here lies within 0.05 LU
of either gate, so no case is skipped or retried."""
import math

import numpy as np
import pytest

import loudness_ref as R

pytestmark = pytest.mark.gpu

L_TOL = 0.01                              # LU
G_TOL = 10.0 ** (L_TOL / 20.0) - 1.0      # relative, of a gain that follows L
ULP4 = 4 * 2.0 ** -23                     # relative, of a gain that is one fp32 quotient
SCALES = [0.667, 1.0, 0.8]
SC = np.array([0.8, 1.0, 0.8], np.float32)
NATIVE = 22050


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert hip_lib.has_loudness, "libvits_mi355.so exports no vits_op_loudness"
    return hip_lib


@pytest.fixture(scope="module")
def tile():
    """VITS_LOUDNESS_TILE, the constant the kernels use (the lengths straddle it)"""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return int(re.search(r"#define\s+VITS_LOUDNESS_TILE\s+(\d+)", open(os.path.join(root, "include", "vits_loudness.h")).read()).group(1))


def _spec(**kw):
    from vosk_tts_amd.capi import loudness_spec

    return loudness_spec(**kw)


def _pcm16(audio, scale):
    """the conversion of vits_synthesize_pcm16 in fp32: scale, * 32767, clip, truncating cast"""
    v = np.asarray(audio, np.float32) * np.float32(scale)
    v = v * np.float32(32767.0)
    return np.trunc(np.clip(v, np.float32(-32767.0), np.float32(32767.0))).astype(np.int16)


# ---- the kernels against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", (8000, 22050, 48000))
def test_op_loudness_against_float64(lib, tile, rate):
    x, lens, names = R.op_batch(rate, tile)
    loud, peak = lib.op_loudness(x, lens, rate)
    assert loud.shape == peak.shape == lens.shape and loud.dtype == peak.dtype == np.float32
    worst = 0.0
    for b, name in enumerate(names):
        xi = x[b, :lens[b]]
        want = R.integrated(xi, rate)
        assert peak[b] == (np.abs(xi).max() if lens[b] else np.float32(0)), name  # bit-equal (NaN beyond the length would poison it)
        if want == -math.inf:
            assert loud[b] == -np.inf, (name, loud[b])
            continue
        err = abs(float(loud[b]) - want)
        worst = max(worst, err)
        assert err <= L_TOL, f"{rate} Hz {name}: {loud[b]:.5f} vs {want:.5f} LUFS ({err:.2e} LU)"
    print(f"{rate} Hz: max |L_gpu - L_ref| = {worst:.2e} LU over {len(names)} items")
    assert loud[names.index("zeros")] == -np.inf and loud[names.index("sine/0")] == -np.inf and peak[names.index("sine/0")] == 0
    l2, p2 = lib.op_loudness(x, lens, rate)
    assert l2.tobytes() == loud.tobytes() and p2.tobytes() == peak.tobytes()  # fixed slots, fixed order: the same bits twice


@pytest.mark.parametrize("case", ("lufs-19", "lufs-10-ceiling", "peak0.5"))
@pytest.mark.parametrize("rate", (8000, 22050))
def test_op_normalize_against_float64(lib, tile, rate, case):
    mode, target, ceiling = {"lufs-19": (R.LUFS, -19.0, 1.0), "lufs-10-ceiling": (R.LUFS, -10.0, 1.0), "peak0.5": (R.PEAK, 0.5, 0.0)}[case]
    x, lens = R.normalize_batch(rate, tile)
    y, loud, gain = lib.op_loudness_normalize(x, lens, rate, mode, target, ceiling)
    assert y.shape == x.shape and y.dtype == np.float32
    capped = []
    for b in range(x.shape[0]):
        xi = x[b, :lens[b]]
        L, pk = R.integrated(xi, rate), R.peak(xi)
        if pk == 0:  # silence: returned unchanged, gain 1
            assert gain[b] == 1.0 and loud[b] == -np.inf and not y[b].any()
            continue
        assert abs(float(loud[b]) - L) <= L_TOL
        if mode == R.PEAK:
            want, tol = target / pk, ULP4
        else:
            free = R.gain(L, pk, mode, target, 0.0)
            assert abs(free * pk / ceiling - 1.0) > 10 * G_TOL, "the restatement cannot tell whether this item reaches the ceiling"
            capped.append(free * pk > ceiling)
            want, tol = (ceiling / pk, ULP4) if capped[-1] else (free, G_TOL)
        rel = abs(float(gain[b]) / want - 1.0)
        print(f"{rate} Hz {case} item {b}: gain {gain[b]:.6f} vs {want:.6f} (rel {rel:.2e}, bound {tol:.2e})")
        assert rel <= tol
        assert np.array_equal(y[b, :lens[b]], np.float32(gain[b]) * xi)  # exactly fp32(gain * x), given the returned gain
        assert not y[b, lens[b]:].any()
    if case == "lufs-19":
        assert capped.count(False) >= 4  # the ceiling not reached (the DC + 30 Hz item, all crest, does reach it)
    if case == "lufs-10-ceiling":
        assert capped.count(True) >= 1
    again = lib.op_loudness_normalize(x, lens, rate, mode, target, ceiling)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((y, loud, gain), again))


# ---- VITS entry points ------------------------------------------------------------------------------------------------------------
def _ragged(rng, B, Tx=24, n_vocab=20):
    lens = np.array([Tx, Tx - 9, 5][:B], np.int64)
    ids = rng.integers(1, n_vocab, size=(B, Tx)).astype(np.int64)
    sid = rng.integers(0, 4, size=B).astype(np.int64)
    return ids, lens, sid


@pytest.fixture(scope="module")
def launch_path(hip_lib):
    """single utterances on the launch path for this module's bit-for-bit comparisons of two calls (whether a call takes the persistent
    programs depends on how busy the device is as it starts)"""
    hip_lib.lib.vits_debug_persist(0)
    yield
    hip_lib.lib.vits_debug_persist(7)


@pytest.mark.parametrize("solo", (False, True), ids=("padded", "solo"))
@pytest.mark.parametrize("rate", (None, 8000), ids=("native", "8000"))
@pytest.mark.parametrize("B", (3, 1))
def test_flagged_synthesize_is_the_op_on_the_unflagged_audio(lib, hip_tiny, launch_path, B, rate, solo):
    ids, lens, sid = _ragged(np.random.default_rng(41), B)
    hz = rate or NATIVE
    kw = dict(seed=7, solo=solo, sample_rate=rate)
    plain, ol, ends = hip_tiny.synthesize(ids, lens, SCALES, sid, marks=True, **kw)
    assert ol.min() > 0
    for spec in (_spec(loudness=-19.0), _spec(peak=0.5)):
        want, wl, wg = lib.op_loudness_normalize(plain, ol, hz, *spec)
        out = {}
        got, gl = hip_tiny.synthesize(ids, lens, SCALES, sid, loudness=spec, loudness_out=out, **kw)
        assert np.array_equal(gl, ol) and got.shape == plain.shape
        assert np.array_equal(got, want)
        assert out["loudness"].tobytes() == wl.tobytes() and out["gain"].tobytes() == wg.tobytes()
        assert np.isfinite(wl).all() and (wg != 1).all()
        scale = float(1.25 / np.abs(want).max())  # the loudest samples clip
        pcm, pl = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=scale, loudness=spec, **kw)
        assert np.array_equal(pl, ol) and np.array_equal(pcm, _pcm16(want, scale))
        g3, l3, e3 = hip_tiny.synthesize(ids, lens, SCALES, sid, marks=True, loudness=spec, **kw)
        assert np.array_equal(g3, want) and np.array_equal(l3, ol) and np.array_equal(e3, ends)  # lengths and marks do not change
        p3, _, e4 = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=scale, marks=True, loudness=spec, **kw)
        assert np.array_equal(p3, pcm) and np.array_equal(e4, ends)


def test_eager_path_agrees_with_the_fast_path(lib, hip_tiny, launch_path):
    ids, lens, sid = _ragged(np.random.default_rng(42), 3)
    spec = _spec(loudness=-19.0)
    fast = hip_tiny.synthesize(ids, lens, SCALES, sid, seed=5, solo=True, sample_rate=8000, loudness=spec)
    fast16 = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=0.7, seed=5, solo=True, loudness=spec)
    lib.lib.vits_debug_fast_path(0)
    try:
        plain, ol = hip_tiny.synthesize(ids, lens, SCALES, sid, seed=5, solo=True, sample_rate=8000)
        out = {}
        got, gl = hip_tiny.synthesize(ids, lens, SCALES, sid, seed=5, solo=True, sample_rate=8000, loudness=spec, loudness_out=out)
        want, wl, wg = lib.op_loudness_normalize(plain, ol, 8000, *spec)
        assert np.array_equal(got, want) and out["gain"].tobytes() == wg.tobytes() and out["loudness"].tobytes() == wl.tobytes()
        p0, l0 = hip_tiny.synthesize(ids, lens, SCALES, sid, seed=5, solo=True)
        w16 = _pcm16(lib.op_loudness_normalize(p0, l0, NATIVE, *spec)[0], 0.7)
        e16, _ = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=0.7, seed=5, solo=True, loudness=spec)
        assert np.array_equal(e16, w16)
    finally:
        lib.lib.vits_debug_fast_path(1)
    # the two paths run the decoder on different launch shapes: equal within what their unflagged outputs differ by
    assert fast[0].shape == got.shape and np.array_equal(fast[1], gl)
    assert np.abs(fast[0] - got).max() <= 1e-4 * np.abs(got).max()
    assert np.abs(fast16[0].astype(np.int32) - e16.astype(np.int32)).max() <= 2


def test_a_call_without_the_flag_launches_what_it_did(lib, hip_tiny, launch_path):
    ids = np.random.default_rng(43).integers(1, 20, size=(1, 16)).astype(np.int64)

    def dump(**kw):
        lib.launch_log(1)
        try:
            hip_tiny.synthesize_pcm16(ids, [16], SCALES, [1], seed=3, **kw)
        finally:
            lib.launch_log(0)
        return lib.launch_dump()

    lib.lib.vits_debug_fast_path(0)  # the eager path: one counted launch per kernel
    try:
        before = dump()
        flagged = dump(loudness=_spec(loudness=-19.0))
        after = dump()
    finally:
        lib.lib.vits_debug_fast_path(1)
    assert not any("loud" in k for k in before) and before == after
    mine = {k: n for k, n in flagged.items() if "loud" in k}
    assert sorted(mine) == ["out.loudness|loud_apply_kernel<int16>", "out.loudness|loud_carry_kernel", "out.loudness|loud_final_kernel",
                            "out.loudness|loud_square_kernel", "out.loudness|loud_tile_kernel"] and set(mine.values()) == {1}
    rest = {k: n for k, n in flagged.items() if "loud" not in k}
    assert rest == {k: n for k, n in before.items() if k != "out.pcm16|pcm16_kernel"}  # (the gain kernel converts)


def test_streams_refuse_the_flag_and_the_process_goes_on(lib, hip_tiny):
    import ctypes

    from vosk_tts_amd.capi import FLAG_LOUDNESS, SynthOpts, VitsError, _p, c_f32p, c_i64p

    ids = np.random.default_rng(44).integers(1, 20, size=(1, 12)).astype(np.int64)
    with pytest.raises(VitsError, match="whole utterance") as e:
        hip_tiny.stream(ids, SCALES, 1, loudness=_spec(loudness=-19.0))
    assert e.value.code == 4
    opts = SynthOpts()
    opts.flags = FLAG_LOUDNESS
    opts.loudness_mode, opts.loudness_target, opts.loudness_ceiling = 1, -19.0, 1.0
    sc = np.array(SCALES, np.float32)
    st, total = ctypes.c_void_p(), ctypes.c_int64()
    for name, extra in (("stream_open", ()), ("stream_open_rate", (8000,))):
        rc = lib._fn(name)(hip_tiny._h, _p(ids, c_i64p), 12, _p(sc, c_f32p), 1, ctypes.byref(opts), 8, *extra, ctypes.byref(st), ctypes.byref(total))
        assert rc == 4 and not st.value  # VITS_ERR_UNSUPPORTED
        with pytest.raises(VitsError, match="whole utterance"):
            lib.check(rc)
    for bad, word in ((dict(loudness_mode=3), "mode 3"), (dict(loudness_target=2.0), "2"), (dict(loudness_ceiling=-1.0), "-1")):
        o = SynthOpts()
        o.flags = FLAG_LOUDNESS
        o.loudness_mode, o.loudness_target, o.loudness_ceiling = 1, -19.0, 1.0
        for k, v in bad.items():
            setattr(o, k, v)
        out, ns, ol = c_f32p(), ctypes.c_int64(), np.zeros(1, np.int64)
        rc = lib._fn("synthesize")(hip_tiny._h, _p(ids, c_i64p), _p(np.array([12], np.int64), c_i64p), 1, 12, _p(sc, c_f32p),
                                   _p(np.array([1], np.int64), c_i64p), ctypes.byref(o), ctypes.byref(out), ctypes.byref(ns), _p(ol, c_i64p))
        assert rc == 1  # VITS_ERR_ARG
        with pytest.raises(VitsError, match=word):
            lib.check(rc)
    audio, ol = hip_tiny.synthesize(ids, [12], SCALES, [1], seed=2)  # a normal request afterwards
    assert ol[0] > 0 and np.isfinite(audio).all()
    chunks = list(hip_tiny.stream(ids, SCALES, 1, chunk_frames=8, seed=2))
    assert sum(c.shape[0] for c in chunks) == ol[0]


# ---- multistream entry points ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def voice(tmp_path_factory):
    from vosk_tts_amd import Model
    from vosk_tts_amd.toymodel import write_toy_multistream_model

    d = str(tmp_path_factory.mktemp("ms"))
    write_toy_multistream_model(d)
    model = Model(model_path=d, device=0)
    yield model
    model.onnx.close()


def _ms_ids(T, seed, n_vocab=40):
    return np.random.default_rng(seed).integers(1, n_vocab, size=(5, T)).astype(np.int64)


@pytest.mark.parametrize("denoise", (None, 0.01), ids=("plain", "denoised"))
def test_stts_flag_is_the_op_on_the_unflagged_audio(lib, voice, denoise):
    sess = voice.onnx
    native = sess._vocoder.hp.sampling_rate
    T = 14
    ids, pde = _ms_ids(T, 3), np.full(T, 3.0, np.float32)
    kw = dict(seed=9, n_timesteps=2, want_mel=False, denoiser_strength=denoise)
    plain, _ = sess._model.synthesize(ids, SC, 2, None, pde, **kw)
    assert plain.shape == (T * 3 * sess._vocoder.hp.hop_length,)
    for spec in (_spec(loudness=-19.0), _spec(peak=0.5)):
        want, wl, wg = lib.op_loudness_normalize(plain[None], [plain.shape[0]], native, *spec)
        out = {}
        got, _ = sess._model.synthesize(ids, SC, 2, None, pde, loudness=spec, loudness_out=out, **kw)
        assert np.array_equal(got, want[0]) and out["gain"].tobytes() == wg.tobytes() and out["loudness"].tobytes() == wl.tobytes()
        assert wg[0] != 1
        # the marks form at another rate: after its resample
        p8, _, e8 = sess._model.synthesize(ids, SC, 2, None, pde, marks=True, sample_rate=8000, **kw)
        w8 = lib.op_loudness_normalize(p8[None], [p8.shape[0]], 8000, *spec)[0][0]
        g8, _, f8 = sess._model.synthesize(ids, SC, 2, None, pde, marks=True, sample_rate=8000, loudness=spec, **kw)
        assert np.array_equal(g8, w8) and np.array_equal(e8, f8)
    # the batch door: ragged, a gain per item
    B = 3
    lens = np.array([T, 9, 4], np.int64)
    bids = np.stack([_ms_ids(T, 10 + b) for b in range(B)])
    bpde = np.full((B, T), 3.0, np.float32)
    bkw = dict(seed=0, n_timesteps=2, item_seeds=[5, 6, 7], denoiser_strength=denoise)
    spec = _spec(loudness=-19.0)
    plain, ol = sess._model.synthesize_batch(bids, lens, SC, [0, 1, 2], None, bpde, **bkw)
    want, wl, wg = lib.op_loudness_normalize(plain, ol, native, *spec)
    out = {}
    got, gl = sess._model.synthesize_batch(bids, lens, SC, [0, 1, 2], None, bpde, loudness=spec, loudness_out=out, **bkw)
    assert np.array_equal(gl, ol) and np.array_equal(got, want) and out["gain"].tobytes() == wg.tobytes()
    assert len(set(wg.tolist())) == B
    p8, l8, e8 = sess._model.synthesize_batch(bids, lens, SC, [0, 1, 2], None, bpde, marks=True, sample_rate=8000, **bkw)
    g8, m8, f8 = sess._model.synthesize_batch(bids, lens, SC, [0, 1, 2], None, bpde, marks=True, sample_rate=8000, loudness=spec, **bkw)
    assert np.array_equal(g8, lib.op_loudness_normalize(p8, l8, 8000, *spec)[0]) and np.array_equal(l8, m8) and np.array_equal(e8, f8)


def test_stts_session_normalises_the_resampled_audio(lib, voice):
    from vosk_tts_amd.capi import VitsError

    sess = voice.onnx
    T = 14
    feed = {"input": _ms_ids(T, 3)[None], "input_lengths": np.array([T], np.int64), "scales": SC, "sid": np.array([2], np.int64),
            "phone_duration_extra": np.full((1, T), 3.0, np.float32), "vits.seed": 9, "vits.n_timesteps": 2, "vits.sample_rate": 8000}
    plain8 = sess.run(None, feed)[0][0]
    got = sess.run(None, dict(feed, **{"vits.loudness": -19.0}))[0][0]
    spec = _spec(loudness=-19.0)
    want = lib.op_loudness_normalize(plain8[None], [plain8.shape[0]], 8000, *spec)[0][0]
    assert np.array_equal(got, want)
    # ... and not the normalised native audio resampled: that one is measured with another filter on another signal
    native = sess.run(None, dict({k: v for k, v in feed.items() if k != "vits.sample_rate"}, **{"vits.loudness": -19.0}))[0][0]
    other = sess.resample(native[None], [native.shape[0]], 8000)[0][0]
    assert other.shape == got.shape and not np.array_equal(other, got)
    batch = {"input": np.stack([_ms_ids(T, 10 + b) for b in range(2)]), "input_lengths": np.array([T, 9], np.int64), "scales": SC,
             "sid": np.array([0, 1], np.int64), "phone_duration_extra": np.full((2, T), 3.0, np.float32), "vits.item_seeds": [5, 6],
             "vits.n_timesteps": 2, "vits.sample_rate": 8000}
    pa, pl = sess.run_batch(batch)
    ga, gl = sess.run_batch(dict(batch, **{"vits.peak": 0.5}))
    assert np.array_equal(gl, pl) and np.array_equal(ga, lib.op_loudness_normalize(pa, pl, 8000, *_spec(peak=0.5))[0])
    with pytest.raises(ValueError, match="whole utterance"):
        sess.run_stream(None, dict(feed, **{"vits.loudness": -19.0}))
    with pytest.raises(VitsError, match="whole utterance") as e:
        sess._model.stream(_ms_ids(T, 3), SC, 2, loudness=spec)
    assert e.value.code == 4
    with pytest.raises(ValueError, match="not both"):
        sess.run(None, dict(feed, **{"vits.loudness": -19.0, "vits.peak": 0.5}))
    assert np.array_equal(sess.run(None, feed)[0][0], plain8)  # a normal request afterwards


def test_stts_stream_open_refuses_the_flag(lib, voice):
    import ctypes

    from vosk_tts_amd.capi import VitsError, _p, c_f32p, c_i64p
    from vosk_tts_amd.capi_stts import STTS_FLAG_LOUDNESS, SttsLoudnessOpts

    m = voice.onnx._model
    ids = _ms_ids(8, 1)
    o = SttsLoudnessOpts()
    o.flags = STTS_FLAG_LOUDNESS
    o.loudness_mode, o.loudness_target, o.loudness_ceiling = 2, 0.5, 0.0
    st, total = ctypes.c_void_p(), ctypes.c_int64()
    rc = m._fn("stream_open")(m._h, _p(ids, c_i64p), 8, _p(SC, c_f32p), 0, None, None, ctypes.byref(o), 8, ctypes.byref(st), ctypes.byref(total))
    assert rc == 4 and not st.value
    with pytest.raises(VitsError, match="whole utterance"):
        m.check(rc)


# ---- through Synth ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from vosk_tts_amd import Model, Synth
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.toymodel import PHONEMES, write_toy_model

    d = write_toy_model(str(tmp_path_factory.mktemp("vits") / "m"), W.default_hparams(n_vocab=len(PHONEMES)))
    model = Model(model_path=d, device=0)
    yield d, Synth(model)
    model.onnx.close()


TEXT = "прив+ет прив+ет прив+ет м+ир, м+ир."


def test_synth_audio_reaches_the_target(toy):
    _, synth = toy
    plain = synth.synth_audio(TEXT, speaker_id=2, scale=1.0)
    l0, p0 = synth.measure_loudness(plain)
    assert math.isfinite(l0) and 0 < p0 <= 1 and p0 == np.float32(np.abs(plain.astype(np.int32)).max()) / np.float32(32767)
    # half the level of the un-normalised voice: the ceiling cannot be reached, so the target must be met.  0.05 LU = the 0.01 LU bound of
    # the measurement plus int16 quantisation (far below 0.01 LU at these levels), rounded up
    target = max(round(l0 - 6.0), -60)
    pcm = synth.synth_audio(TEXT, speaker_id=2, scale=1.0, loudness=float(target))
    lufs, pk = synth.measure_loudness(pcm)
    print(f"un-normalised {l0:.2f} LUFS peak {p0:.3f}; target {target}: {lufs:.3f} LUFS peak {pk:.3f}")
    assert pcm.dtype == np.int16 and pk < 0.99 and abs(lufs - target) <= 0.05
    pcm = synth.synth_audio(TEXT, speaker_id=2, scale=1.0, loudness=-19.0)
    lufs, pk = synth.measure_loudness(pcm)
    print(f"target -19: {lufs:.3f} LUFS peak {pk:.3f}")
    if pk < 0.999:  # the default ceiling 1.0 was not reached
        assert abs(lufs - (-19.0)) <= 0.05
    else:
        assert lufs < -19.0 and np.abs(pcm.astype(np.int32)).max() in (32766, 32767)
    # at another rate the returned audio is what is measured
    pcm8 = synth.synth_audio(TEXT, speaker_id=2, scale=1.0, loudness=float(target), sample_rate=8000)
    lufs8, pk8 = synth.measure_loudness(pcm8, 8000)
    assert pk8 < 0.99 and abs(lufs8 - target) <= 0.05
    pcm = synth.synth_audio(TEXT, speaker_id=2, scale=1.0, peak=0.5)
    assert int(np.abs(pcm.astype(np.int32)).max()) in (16382, 16383)
    with pytest.raises(ValueError, match="not both"):
        synth.synth_audio(TEXT, loudness=-19.0, peak=0.5)
    with pytest.raises(ValueError, match="whole utterance"):
        next(synth.synth_stream(TEXT, loudness=-19.0))
    assert sum(c.size for c in synth.synth_stream(TEXT, speaker_id=2)) > 0  # a normal stream afterwards


def test_session_feeds_and_stream_refusal(toy):
    _, synth = toy
    sess = synth.model.onnx
    ids = np.array([synth.g2p_noembed(TEXT)], np.int64)
    feed = {"input": ids, "input_lengths": np.array([ids.shape[1]], np.int64), "scales": SC, "sid": np.array([2], np.int64), "bert": None,
            "phone_duration_extra": None, "vits.seed": 11}
    plain = sess.run(None, feed)[0].reshape(1, -1)
    got = sess.run(None, dict(feed, **{"vits.peak": 0.25}))[0].reshape(1, -1)
    assert got.shape == plain.shape and np.abs(got).max() == pytest.approx(0.25, rel=1e-6)
    pcm = sess.run_pcm16(dict(feed, **{"vits.peak": 0.25}), 2.0)
    assert np.array_equal(pcm, _pcm16(got, 2.0))  # `scale` multiplies afterwards, as before
    with pytest.raises(ValueError, match="whole utterance"):
        sess.run_stream(None, dict(feed, **{"vits.loudness": -19.0}))
    with pytest.raises(ValueError, match="not both"):
        sess.run(None, dict(feed, **{"vits.loudness": -19.0, "vits.peak": 0.5}))


def test_synth_batch_items_equal_their_single_calls(toy):
    """Every request of a batch is measured and normalised on its own.  int16, at most one LSB apart, as for the un-normalised batch
    (tests/test_host_api.py: batch composition changes which conv kernel runs; the gains then differ by parts in 1e6)."""
    from vosk_tts_amd.batching import MultiDeviceSynth

    d, synth = toy
    texts = ["прив+ет, м+ир!", "м+ир", TEXT, "м+ир прив+ет?"]
    sids, seeds = [2, 0, 5, 2], [101, 7, 33, 58]
    mds = MultiDeviceSynth(d, devices=[0], max_batch=4)
    try:
        plain = mds.synth_batch(texts, speaker_ids=sids, seeds=seeds, scale=1.0)
        got = mds.synth_batch(texts, speaker_ids=sids, seeds=seeds, scale=1.0, peak=0.5)
        for i, t in enumerate(texts):
            ids = np.array([synth.g2p_noembed(t)], np.int64)
            feed = {"input": ids, "input_lengths": np.array([ids.shape[1]], np.int64), "scales": np.array([0.8, 1.0, 0.8], np.float32),
                    "sid": np.array([sids[i]], np.int64), "bert": None, "phone_duration_extra": None, "vits.seed": seeds[i], "vits.peak": 0.5}
            solo = synth.model.onnx.run_pcm16(feed, 1.0)[0]
            assert got[i].shape == solo.shape == plain[i].shape
            assert np.abs(got[i].astype(np.int32) - solo.astype(np.int32)).max() <= 1, i
            assert int(np.abs(got[i].astype(np.int32)).max()) in (16382, 16383)  # its own peak, not the batch's
        with pytest.raises(ValueError, match="not both"):
            mds.synth_batch(texts, loudness=-19.0, peak=0.5)
    finally:
        mds.close()
