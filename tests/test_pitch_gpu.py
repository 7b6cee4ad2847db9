"""Pitch-shifted output on the device (include/vits_pitch.h): the kernels against the float64 restatement (tests/pitch_ref.py) through the
parity doors, padding / batching / determinism, and the flag through the entry points of both model families.

Tolerance of the sample-wise comparisons: the float32 run of the restatement is an fp32 implementation of the same definition with
another FFT order, another atan2 and another sincos; its largest deviation from the float64 run on the very same item is the yardstick,
and the device may sit 4 times that far from float64.  Measured on an MI355X (the worst of the four shifts, device / yardstick):
    vits_op_pitch_shift    item 513: 1.8e-7 / 1.2e-7,  item 2048: 2.5e-7 / 1.1e-7,  item 4173 (voiced): 1.9e-7 / 8.2e-8   (at most 2.3 x)
    vits_op_pitch_stretch  item 2048: 2.4e-7 / 1.0e-7                                                                    (at most 2.4 x)
"""
import ctypes
import math

import numpy as np
import pytest

import pitch_ref as R

pytestmark = pytest.mark.gpu

SCALES = [0.667, 1.0, 0.8]
SC = np.array([0.8, 1.0, 0.8], np.float32)
NATIVE = 22050


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert hip_lib.has_pitch, "libvits_mi355.so exports no vits_op_pitch_shift"
    return hip_lib


@pytest.fixture(scope="module")
def items():
    """the ragged batch: x [3, N] poisoned with NaN beyond every length"""
    its = R.gpu_items()
    x = np.full((len(its), R.GPU_N), np.nan, np.float32)
    for b, v in enumerate(its):
        x[b, :v.shape[0]] = v
    return its, x, np.array([v.shape[0] for v in its], np.int64)


@pytest.fixture(scope="module")
def refs(items):
    """per shift: the float64 and float32 runs of the restatement on every item, computed once"""
    its = items[0]
    cache = {}

    def get(s):
        if s not in cache:
            P, Q = R.plan(s)
            cache[s] = dict(y64=[R.pitch_shift(v, s, np.float64) for v in its], y32=[R.pitch_shift(v, s, np.float32) for v in its],
                            u64=R.stretch(its[1], P, Q, np.float64), u32=R.stretch(its[1], P, Q, np.float32))
        return cache[s]

    return get


def _pcm16(audio, scale):
    """the conversion of vits_synthesize_pcm16 in fp32: scale, * 32767, clip, truncating cast"""
    v = np.asarray(audio, np.float32) * np.float32(scale)
    v = v * np.float32(32767.0)
    return np.trunc(np.clip(v, np.float32(-32767.0), np.float32(32767.0))).astype(np.int16)


# ---- the kernels against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", R.GPU_SEMITONES)
def test_op_shift_against_float64(lib, items, refs, s):
    its, x, lens = items
    y = lib.op_pitch_shift(x, lens, s)
    assert y.shape == x.shape and np.isfinite(y).all()
    r = refs(s)
    for b, v in enumerate(its):
        n = v.shape[0]
        yard = np.abs(r["y32"][b].astype(np.float64) - r["y64"][b]).max()
        dev = np.abs(y[b, :n].astype(np.float64) - r["y64"][b]).max()
        print(f"s={s} item {b} ({n} samples): device {dev:.3g}, float32 restatement {yard:.3g} from float64 (x{dev / yard:.2f})")
        assert yard > 0 and dev <= 4 * yard, (s, b, dev, yard)
        assert not y[b, n:].any()  # exactly zero beyond the length
        assert np.abs(y[b, :R.HOP * (n // R.HOP)]).max() > 0.05  # (and not silence inside it)


@pytest.mark.parametrize("s", R.GPU_SEMITONES)
def test_op_stretch_against_float64(lib, items, refs, s):
    """u, the vocoder's output before the resampler, for the 2048-sample item: a difference in the test above is placed with it"""
    its, x, lens = items
    P, Q = R.plan(s)
    u = lib.op_pitch_stretch(x[1:2, :2048], lens[1:2], s)
    r = refs(s)
    n_u = R.n_u(2048, P, Q)
    assert u.shape == (1, R.stretch_samples(2048, P, Q)) and r["u64"].shape == (n_u,) and np.isfinite(u).all()
    yard = np.abs(r["u32"].astype(np.float64) - r["u64"]).max()
    dev = np.abs(u[0, :n_u].astype(np.float64) - r["u64"]).max()
    print(f"s={s}: device {dev:.3g}, float32 restatement {yard:.3g} from float64 (x{dev / yard:.2f})")
    assert yard > 0 and dev <= 4 * yard, (s, dev, yard)
    assert not u[0, n_u:].any()


@pytest.mark.parametrize("s", (-12.0, -3.0, 4.0, 12.0))
def test_device_shifts_a_sine_and_keeps_its_level(lib, s):
    """the property the plain phase vocoder fails (it returns a tenth of the level); tolerant of any flipped peak by construction"""
    P, Q = R.plan(s)
    x = R.sine()
    y = lib.op_pitch_shift(x[None], [x.shape[0]], s)[0]
    peak, rms = R.sine_figures(y)
    assert abs(peak - 440.0 * P / Q * 8192 / 22050) <= 1.0, peak
    assert abs(rms - 0.3 / math.sqrt(2)) <= 0.01 * 0.3 / math.sqrt(2), rms


# ---- lengths, padding, batching ------------------------------------------------------------------------------------------------------
def test_padding_is_never_read_and_short_items_come_back(lib):
    rng = np.random.default_rng(3)
    N = 1100
    x = np.full((4, N), np.nan, np.float32)
    lens = np.array([512, 0, 1100, 769], np.int64)  # below n/2 + 1; empty; the whole row; one sample past a hop
    for b, n in enumerate(lens):
        x[b, :n] = 0.2 * rng.standard_normal(n)
    for s in (5.0, -7.0):
        y = lib.op_pitch_shift(x, lens, s)
        assert np.isfinite(y).all()
        for b, n in enumerate(lens):
            assert not y[b, n:].any()
        assert y[0, :512].tobytes() == x[0, :512].tobytes()  # a 512-sample item: bit-identical
        assert np.abs(y[2, :1024]).max() > 0.05 and np.abs(y[3, :768]).max() > 0.05
        u = lib.op_pitch_stretch(x, lens, s)
        P, Q = R.plan(s)
        assert np.isfinite(u).all() and not u[0].any() and not u[1].any() and not u[2, R.n_u(1100, P, Q):].any()


def test_items_do_not_depend_on_their_batch_and_calls_repeat(lib, items):
    its, x, lens = items
    for s in (3.0, -12.0):
        y = lib.op_pitch_shift(x, lens, s)
        assert y.tobytes() == lib.op_pitch_shift(x, lens, s).tobytes()  # the same call twice: the same bits
        for b, v in enumerate(its):
            alone = lib.op_pitch_shift(v[None], [v.shape[0]], s)  # another row length, another batch
            assert alone[0].tobytes() == y[b, :v.shape[0]].tobytes(), (s, b)


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
@pytest.mark.parametrize("B", (3, 1))
def test_flagged_synthesize_is_the_op_chain_on_the_unflagged_audio(lib, hip_tiny, launch_path, B, solo):
    from vosk_tts_amd.capi import loudness_spec

    ids, lens, sid = _ragged(np.random.default_rng(41), B)
    kw = dict(seed=7, solo=solo)
    plain, ol, ends = hip_tiny.synthesize(ids, lens, SCALES, sid, marks=True, **kw)
    assert ol.max() >= R.MIN_LEN
    for s in (3.0, -12.0):
        want = lib.op_pitch_shift(plain, ol, s)  # the same kernels on the same samples
        got, gl = hip_tiny.synthesize(ids, lens, SCALES, sid, pitch=s, **kw)
        assert np.array_equal(gl, ol) and got.shape == plain.shape
        assert got.tobytes() == want.tobytes() and not np.array_equal(got, plain)
        scale = float(1.25 / np.abs(want).max())  # the loudest samples clip
        pcm, pl = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=scale, pitch=s, **kw)
        assert np.array_equal(pl, ol) and np.array_equal(pcm, _pcm16(want, scale))
        g3, l3, e3 = hip_tiny.synthesize(ids, lens, SCALES, sid, marks=True, pitch=s, **kw)
        assert g3.tobytes() == want.tobytes() and np.array_equal(l3, ol) and np.array_equal(e3, ends)  # lengths and marks do not change
        # at 8000 Hz with a loudness target: pitch -> resample -> normalise
        spec = loudness_spec(loudness=-19.0)
        p8, l8, e8 = hip_tiny.synthesize(ids, lens, SCALES, sid, marks=True, sample_rate=8000, **kw)
        w8 = lib.op_loudness_normalize(lib.op_resample(want, ol, NATIVE, 8000), l8, 8000, *spec)[0]
        out = {}
        g8, m8, f8 = hip_tiny.synthesize(ids, lens, SCALES, sid, marks=True, sample_rate=8000, pitch=s, loudness=spec, loudness_out=out, **kw)
        assert np.array_equal(m8, l8) and np.array_equal(f8, e8) and g8.tobytes() == w8.tobytes()
        assert np.isfinite(out["gain"]).all()
        p16, _ = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=0.7, sample_rate=8000, pitch=s, loudness=spec, **kw)
        assert np.array_equal(p16, _pcm16(w8, 0.7))
        # at 8000 Hz without one: the resampler converts
        r16, _ = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=0.7, sample_rate=8000, pitch=s, **kw)
        assert np.array_equal(r16, _pcm16(lib.op_resample(want, ol, NATIVE, 8000), 0.7))


def test_eager_path_agrees_with_the_fast_path(lib, hip_tiny, launch_path):
    ids, lens, sid = _ragged(np.random.default_rng(42), 3)
    fast, fl = hip_tiny.synthesize(ids, lens, SCALES, sid, seed=5, solo=True, pitch=-4.0)
    lib.lib.vits_debug_fast_path(0)
    try:
        plain, ol = hip_tiny.synthesize(ids, lens, SCALES, sid, seed=5, solo=True)
        got, gl = hip_tiny.synthesize(ids, lens, SCALES, sid, seed=5, solo=True, pitch=-4.0)
        assert got.tobytes() == lib.op_pitch_shift(plain, ol, -4.0).tobytes() and np.array_equal(gl, ol)
        e16, _ = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=0.7, seed=5, solo=True, pitch=-4.0)
        assert np.array_equal(e16, _pcm16(got, 0.7))
    finally:
        lib.lib.vits_debug_fast_path(1)
    # the two paths run the decoder on different launch shapes (their unflagged outputs differ by parts in 1e5) and the shifter is not
    # continuous in its input, so the samples of the two are not compared: each path is held to the op on its own audio, here and above
    assert fast.shape == got.shape and np.array_equal(fl, gl) and np.isfinite(fast).all()


def test_no_shift_is_the_call_it_was(lib, hip_tiny, launch_path):
    """pitch=0 and a shift that reduces to P = Q set no flag: the bytes and the launches of the call without the argument"""
    ids = np.random.default_rng(43).integers(1, 20, size=(1, 16)).astype(np.int64)

    def dump(**kw):
        lib.launch_log(1)
        try:
            out = hip_tiny.synthesize_pcm16(ids, [16], SCALES, [1], seed=3, **kw)[0]
        finally:
            lib.launch_log(0)
        return out, lib.launch_dump()

    lib.lib.vits_debug_fast_path(0)  # the eager path: one counted launch per kernel
    try:
        before, d0 = dump()
        zero, d1 = dump(pitch=0.0)
        tiny, d2 = dump(pitch=0.0004)
    finally:
        lib.lib.vits_debug_fast_path(1)
    assert before.tobytes() == zero.tobytes() == tiny.tobytes() and d0 == d1 == d2
    a, _ = hip_tiny.synthesize(ids, [16], SCALES, [1], seed=3)
    b, _ = hip_tiny.synthesize(ids, [16], SCALES, [1], seed=3, pitch=0.0)
    assert a.tobytes() == b.tobytes()
    # the flag itself with 0 semitones, through the C ABI: still the identity
    from vosk_tts_amd.capi import FLAG_PITCH, SynthPitchOpts, _p, c_f32p, c_i64p

    o = SynthPitchOpts()
    o.flags, o.seed, o.pitch_semitones = FLAG_PITCH, 3, 0.0
    out, ns, ol = c_f32p(), ctypes.c_int64(), np.zeros(1, np.int64)
    sc = np.array(SCALES, np.float32)
    lib.check(lib._fn("synthesize")(hip_tiny._h, _p(ids, c_i64p), _p(np.array([16], np.int64), c_i64p), 1, 16, _p(sc, c_f32p),
                                    _p(np.array([1], np.int64), c_i64p), ctypes.byref(o), ctypes.byref(out), ctypes.byref(ns), _p(ol, c_i64p)))
    try:
        assert np.ctypeslib.as_array(out, shape=(1, ns.value)).tobytes() == a.tobytes()
    finally:
        lib._fn("free_output")(out)


def test_streams_and_unfit_voices_refuse_and_the_process_goes_on(lib, hip_lib, hip_tiny):
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.capi import FLAG_PITCH, SynthPitchOpts, VitsError, _p, c_f32p, c_i64p

    ids = np.random.default_rng(44).integers(1, 20, size=(1, 12)).astype(np.int64)
    with pytest.raises(VitsError, match="pitch-shifted") as e:
        hip_tiny.stream(ids, SCALES, 1, pitch=2.0)
    assert e.value.code == 4
    opts = SynthPitchOpts()
    opts.flags, opts.pitch_semitones = FLAG_PITCH, 2.0
    sc = np.array(SCALES, np.float32)
    st, total = ctypes.c_void_p(), ctypes.c_int64()
    for name, extra in (("stream_open", ()), ("stream_open_rate", (8000,))):
        rc = lib._fn(name)(hip_tiny._h, _p(ids, c_i64p), 12, _p(sc, c_f32p), 1, ctypes.byref(opts), 8, *extra, ctypes.byref(st), ctypes.byref(total))
        assert rc == 4 and not st.value  # VITS_ERR_UNSUPPORTED
        with pytest.raises(VitsError, match="VITS_FLAG_PITCH on a stream"):
            lib.check(rc)
    with pytest.raises(VitsError, match="12.5") as e:  # a value out of range through the flag: VITS_ERR_ARG naming it
        o = SynthPitchOpts()
        o.flags, o.pitch_semitones = FLAG_PITCH, 12.5
        out, ns, ol = c_f32p(), ctypes.c_int64(), np.zeros(1, np.int64)
        lib.check(lib._fn("synthesize")(hip_tiny._h, _p(ids, c_i64p), _p(np.array([12], np.int64), c_i64p), 1, 12, _p(sc, c_f32p),
                                        _p(np.array([1], np.int64), c_i64p), ctypes.byref(o), ctypes.byref(out), ctypes.byref(ns), _p(ol, c_i64p)))
    assert e.value.code == 1
    # a voice whose hop_length (128) is not a multiple of the pitch stage's hop (256)
    hp = W.plain_hparams()
    hp.n_ups = 3
    hp.up_rates[3] = hp.up_kernels[3] = 0
    hp.hop_length = 128
    small = hip_lib.create(W.synthetic_blob(hp, 7), 0)
    try:
        with pytest.raises(VitsError, match="128.*256") as e:
            small.synthesize(ids, [12], SCALES, [1], seed=2, pitch=2.0)
        assert e.value.code == 4
        a, al = small.synthesize(ids, [12], SCALES, [1], seed=2)
        assert al[0] > 0 and al[0] % 128 == 0
    finally:
        small.close()
    audio, ol = hip_tiny.synthesize(ids, [12], SCALES, [1], seed=2)  # a normal request afterwards
    assert ol[0] > 0 and np.isfinite(audio).all()
    assert sum(c.shape[0] for c in hip_tiny.stream(ids, SCALES, 1, chunk_frames=8, seed=2)) == ol[0]


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
def test_stts_flag_is_the_op_chain_on_the_unflagged_audio(lib, voice, denoise):
    from vosk_tts_amd.capi import loudness_spec

    sess = voice.onnx
    native = sess._vocoder.hp.sampling_rate
    T, s = 14, -5.0
    ids, pde = _ms_ids(T, 3), np.full(T, 3.0, np.float32)
    kw = dict(seed=9, n_timesteps=2, want_mel=False, denoiser_strength=denoise)
    plain, _ = sess._model.synthesize(ids, SC, 2, None, pde, **kw)
    assert plain.shape[0] >= R.MIN_LEN
    want = lib.op_pitch_shift(plain[None], [plain.shape[0]], s)[0]
    got, _ = sess._model.synthesize(ids, SC, 2, None, pde, pitch=s, **kw)
    assert got.tobytes() == want.tobytes() and not np.array_equal(got, plain)
    assert sess._model.synthesize(ids, SC, 2, None, pde, pitch=0.0, **kw)[0].tobytes() == plain.tobytes()
    # the marks form at another rate with a loudness target: pitch -> resample -> normalise; the marks do not move
    spec = loudness_spec(peak=0.5)
    p8, _, e8 = sess._model.synthesize(ids, SC, 2, None, pde, marks=True, sample_rate=8000, **kw)
    w8 = lib.op_loudness_normalize(lib.op_resample(want[None], [want.shape[0]], native, 8000), [p8.shape[0]], 8000, *spec)[0][0]
    g8, _, f8 = sess._model.synthesize(ids, SC, 2, None, pde, marks=True, sample_rate=8000, pitch=s, loudness=spec, **kw)
    assert g8.tobytes() == w8.tobytes() and np.array_equal(e8, f8)
    # the batch door: ragged, every item from its own length
    B = 3
    lens = np.array([T, 9, 4], np.int64)
    bids = np.stack([_ms_ids(T, 10 + b) for b in range(B)])
    bpde = np.full((B, T), 3.0, np.float32)
    bkw = dict(seed=0, n_timesteps=2, item_seeds=[5, 6, 7], denoiser_strength=denoise)
    plain, ol = sess._model.synthesize_batch(bids, lens, SC, [0, 1, 2], None, bpde, **bkw)
    got, gl = sess._model.synthesize_batch(bids, lens, SC, [0, 1, 2], None, bpde, pitch=s, **bkw)
    assert np.array_equal(gl, ol) and got.tobytes() == lib.op_pitch_shift(plain, ol, s).tobytes()
    p8, l8, e8 = sess._model.synthesize_batch(bids, lens, SC, [0, 1, 2], None, bpde, marks=True, sample_rate=8000, **bkw)
    g8, m8, f8 = sess._model.synthesize_batch(bids, lens, SC, [0, 1, 2], None, bpde, marks=True, sample_rate=8000, pitch=s, **bkw)
    assert np.array_equal(l8, m8) and np.array_equal(e8, f8)
    assert g8.tobytes() == lib.op_resample(lib.op_pitch_shift(plain, ol, s), ol, native, 8000).tobytes()


def test_stts_session_and_stream_refusals(lib, voice):
    from vosk_tts_amd.capi import VitsError, _p, c_f32p, c_i64p
    from vosk_tts_amd.capi_stts import STTS_FLAG_PITCH, SttsPitchOpts

    sess = voice.onnx
    T = 14
    feed = {"input": _ms_ids(T, 3)[None], "input_lengths": np.array([T], np.int64), "scales": SC, "sid": np.array([2], np.int64),
            "phone_duration_extra": np.full((1, T), 3.0, np.float32), "vits.seed": 9, "vits.n_timesteps": 2}
    plain = sess.run(None, feed)[0][0]
    got = sess.run(None, dict(feed, **{"vits.pitch": 2.0}))[0][0]
    assert got.tobytes() == lib.op_pitch_shift(plain[None], [plain.shape[0]], 2.0)[0].tobytes()
    got8 = sess.run(None, dict(feed, **{"vits.pitch": 2.0, "vits.sample_rate": 8000}))[0][0]  # shifted at the native rate, then resampled
    assert got8.tobytes() == sess.resample(got[None], [got.shape[0]], 8000)[0][0].tobytes()
    with pytest.raises(ValueError, match="frames before a chunk"):
        sess.run_stream(None, dict(feed, **{"vits.pitch": 2.0}))
    with pytest.raises(VitsError, match="pitch-shifted") as e:
        sess._model.stream(_ms_ids(T, 3), SC, 2, pitch=2.0)
    assert e.value.code == 4
    m = sess._model
    ids = _ms_ids(8, 1)
    o = SttsPitchOpts()
    o.flags, o.pitch_semitones = STTS_FLAG_PITCH, 2.0
    st, total = ctypes.c_void_p(), ctypes.c_int64()
    rc = m._fn("stream_open")(m._h, _p(ids, c_i64p), 8, _p(SC, c_f32p), 0, None, None, ctypes.byref(o), 8, ctypes.byref(st), ctypes.byref(total))
    assert rc == 4 and not st.value
    with pytest.raises(VitsError, match="STTS_FLAG_PITCH on a stream"):
        m.check(rc)
    assert sess.run(None, feed)[0][0].tobytes() == plain.tobytes()  # a normal request afterwards


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


def test_synth_audio_and_the_batch_door_take_pitch(lib, toy):
    from vosk_tts_amd.batching import MultiDeviceSynth

    d, synth = toy
    sess = synth.model.onnx
    ids = np.array([synth.g2p_noembed(TEXT)], np.int64)
    feed = {"input": ids, "input_lengths": np.array([ids.shape[1]], np.int64), "scales": SC, "sid": np.array([2], np.int64), "bert": None,
            "phone_duration_extra": None, "vits.seed": 11}
    plain = sess.run(None, feed)[0].reshape(1, -1)
    got = sess.run(None, dict(feed, **{"vits.pitch": 2.0}))[0].reshape(1, -1)
    assert got.tobytes() == lib.op_pitch_shift(plain, [plain.shape[1]], 2.0).tobytes()
    assert np.array_equal(sess.run_pcm16(dict(feed, **{"vits.pitch": 2.0}), 2.0), _pcm16(got, 2.0))
    w0, e0 = sess.run(None, dict(feed, **{"vits.marks": True}))
    w1, e1 = sess.run(None, dict(feed, **{"vits.marks": True, "vits.pitch": -3.0}))
    assert w1.shape == w0.shape and np.array_equal(e0, e1) and not np.array_equal(w0, w1)  # the duration and the marks do not change
    a1, m1 = synth.synth_audio(TEXT, speaker_id=2, scale=1.0, marks=True, pitch=-3.0)  # (free-running durations: its own length)
    assert a1.dtype == np.int16 and a1.shape[0] == m1.token_ends[-1] > 0 and np.abs(a1.astype(np.int32)).max() > 0
    with pytest.raises(ValueError, match="frames before a chunk"):
        next(synth.synth_stream(TEXT, pitch=2.0))
    texts = ["прив+ет, м+ир!", TEXT]
    mds = MultiDeviceSynth(d, devices=[0], max_batch=4)
    try:
        shifted = mds.synth_batch(texts, speaker_ids=[2, 0], seeds=[101, 7], scale=1.0, pitch=2.0)
        for i, t in enumerate(texts):
            one = np.array([synth.g2p_noembed(t)], np.int64)
            f = {"input": one, "input_lengths": np.array([one.shape[1]], np.int64), "scales": np.array([0.8, 1.0, 0.8], np.float32),
                 "sid": np.array([[2, 0][i]], np.int64), "bert": None, "phone_duration_extra": None, "vits.seed": [101, 7][i], "vits.pitch": 2.0}
            solo = sess.run_pcm16(f, 1.0)[0]
            assert shifted[i].shape == solo.shape
    finally:
        mds.close()
