"""Intonation range on the device (include/vits_intonation.h): the F0 tracker against the float64 restatement
(tests/intonation_ref.py), the integer offsets and positions from the device's own track, the samples, the exact cases, and the flag
through the entry points of both model families.

The track.  A frame is compared unless its float64 decision margin (the smallest |d' - 0.15| over the lags the decision looked at) is
below 4 times the item's yardstick (the largest |d'_float32 - d'_float64|); at most one frame in 16 of an item may be left out that way
(tests/test_intonation.py shows that none is, on these inputs).  On every other frame the voicing is equal and the cents within 1.

The samples, as in tests/test_contour_gpu.py: the float64 restatement is fed the device's own track, so what is compared is the stage
behind it; the float32 run of the restatement on the same track is the yardstick and the device may sit 4 times that far from float64.

Measured on an MI355X.  Track: no frame left out, largest difference 0 cents on every input (smallest margin 2.7e-4, yardsticks 1.5e-6
to 4.9e-6).  Samples (largest distance from float64: device / float32 restatement; r = 4 for 513, 0.5 for 1024 and the ragged batch,
1.5 for the glide; the other items of the ragged batch are exact cases):
    y  513: 6.30e-8 / 7.61e-8   1024: 1.18e-7 / 1.48e-7   ragged item 0: 9.21e-8 / 1.01e-7   glide: 1.19e-7 / 1.36e-7   (at most 0.91 x)
    u  513: 5.18e-8 / 5.41e-8   1024: 5.23e-8 / 5.99e-8   ragged item 0: 5.27e-8 / 5.39e-8   glide: 4.67e-8 / 1.43e-7   (at most 0.98 x)
Slope of the device's output on the 12288-sample glide at r = 0.5: 0.494.
"""
import ctypes

import numpy as np
import pytest

import contour_ref as C
import intonation_ref as I
import pitch_ref as R

pytestmark = pytest.mark.gpu

HOP = 256
RATE = I.GPU_RATE
SCALES = [0.667, 1.0, 0.8]
SC = np.array([0.8, 1.0, 0.8], np.float32)
CASES = I.gpu_cases()
RANGES = {"513": 4.0, "1024": 0.5, "ragged": 0.5, "glide": 1.5}  # (the shortest item's track moves by one cent: only a large r shifts it)


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert hip_lib.has_intonation, "libvits_mi355.so exports no vits_op_intonation"
    return hip_lib


def _pad(items):
    """-> x [B, N] poisoned with NaN beyond every length, lengths [B]"""
    N = max(max(v.shape[0] for v in items), 1)
    x = np.full((len(items), N), np.nan, np.float32)
    lens = np.zeros(len(items), np.int64)
    for b, v in enumerate(items):
        x[b, :v.shape[0]] = v
        lens[b] = v.shape[0]
    return x, lens


@pytest.fixture(scope="module")
def figures():
    cache = {}

    def get(key, x, rate=RATE):
        if key not in cache:
            cache[key] = I.track_figures(x, rate)
        return cache[key]

    return get


def _check_track(name, b, v, cents_row, fg):
    F = C.frames(v.shape[0])
    assert not cents_row[F:].any(), (name, b)  # rows beyond the item's are zero
    if v.shape[0] < R.MIN_LEN:
        assert not cents_row.any(), (name, b)
        return
    c64 = fg["c64"]
    skip = fg["margin"] < 4 * fg["yardstick"]
    assert skip.sum() * 16 <= F, (name, b, int(skip.sum()), F)
    keep = ~skip
    dev = cents_row[:F].astype(np.int64)
    print(f"{name} item {b}: {F} rows, {int((c64 > 0).sum())} voiced, {int(skip.sum())} left out, largest |dcents| "
          f"{int(np.abs(dev - c64)[keep].max()) if keep.any() else 0}, smallest margin {fg['margin'].min():.3g}, yardstick {fg['yardstick']:.3g}")
    assert np.array_equal((dev > 0)[keep], (c64 > 0)[keep]), (name, b)
    assert (np.abs(dev - c64)[keep] <= 1).all(), (name, b, dev, c64)


@pytest.mark.parametrize("name", list(CASES))
def test_track_against_float64(lib, figures, name):
    items = CASES[name]
    x, lens = _pad(items)
    cents = lib.op_f0_track(x, lens, RATE)
    assert cents.shape == (len(items), 1 + x.shape[1] // HOP) and cents.dtype == np.int32
    for b, v in enumerate(items):
        _check_track(name, b, v, cents[b], figures((name, b), v))
    assert cents.tobytes() == lib.op_f0_track(x, lens, RATE).tobytes()  # the same call twice: the same words


def test_track_at_another_rate_and_refused_rates(lib, figures):
    from vosk_tts_amd.capi import VitsError

    v = R.voiced(4352, rate=16000, seed=0)
    cents = lib.op_f0_track(v[None], [v.shape[0]], 16000)
    fg = figures(("16k", 0), v, 16000)
    assert (fg["c64"] > 0).sum() >= 4
    _check_track("16k", 0, v, cents[0], fg)
    for rate in (48000, 7999):
        with pytest.raises(VitsError, match=str(rate)) as e:
            lib.op_f0_track(v[None], [v.shape[0]], rate)
        assert e.value.code == 4
    with pytest.raises(VitsError, match="48000"):
        lib.op_intonation(v[None], [v.shape[0]], 48000, 0.5)
    for r in (-0.1, 4.5, float("nan")):
        with pytest.raises(VitsError, match="pitch_range") as e:
            lib.op_intonation(v[None], [v.shape[0]], 16000, r)
        assert e.value.code == 1
    assert lib.op_f0_track(v[None], [v.shape[0]], 16000).tobytes() == cents.tobytes()  # a normal call afterwards


# ---- the integers: offsets, ratios and positions from the device's own track ------------------------------------------------------------
def _tokens(F, kind):
    """a token contour over an item of F rows at hop 256: (cum, semitones, gain_db) or None"""
    if kind == "none":
        return None
    cum = np.array([max(F // 3, 1), max(F // 3, 1), max(2 * F // 3, 2), F + 1], np.int32)  # (a zero-frame token among them)
    st = np.array([3.0, 9.0, -2.0, 5.0], np.float32) + (2.0 if kind == "tokens+shift" else 0.0)
    return cum, st, np.array([0.0, 0.0, 3.0, -3.0], np.float32)


def _door_args(items, kind):
    x, lens = _pad(items)
    if kind == "none":
        return x, lens, {}
    toks = [_tokens(C.frames(v.shape[0]), kind) for v in items]
    cum = np.stack([t[0] for t in toks])
    return x, lens, dict(cum=cum, tok_lengths=np.full(len(items), 4, np.int64), hop=HOP, token_semitones=np.stack([t[1] for t in toks]),
                         token_gain_db=np.stack([t[2] for t in toks]))


def _ref(v, r, kind, cents, dtype=np.float64):
    rep = {}
    t = _tokens(C.frames(v.shape[0]), kind)
    kw = {} if t is None else dict(cum=t[0], tok_len=4, hop=HOP, semitones=t[1], gain_db=t[2])
    y = I.intonation(v, RATE, r, dtype=dtype, cents=cents, report=rep, **kw)
    return y, rep


@pytest.mark.parametrize("kind", ("none", "tokens", "tokens+shift"))
@pytest.mark.parametrize("name", ("ragged", "glide"))
def test_positions_equal_the_recurrence_from_the_device_track(lib, name, kind):
    items = CASES[name]
    r = RANGES[name]
    x, lens, kw = _door_args(items, kind)
    u, steps, cents = lib.op_intonation_stretch(x, lens, RATE, r, **kw)
    assert steps.shape == (len(items), C.steps_columns(x.shape[1])) and u.shape == (len(items), C.stretch_samples(x.shape[1]))
    assert np.isfinite(u).all()
    assert cents.tobytes() == lib.op_f0_track(x, lens, RATE).tobytes()  # the track the ratios came from is the door's
    shifted = 0
    for b, v in enumerate(items):
        if v.shape[0] == 0:
            assert not steps[b].any() and not u[b].any()
            continue
        _, rep = _ref(v, r, kind, cents[b])
        if not rep["shifted"]:
            assert not steps[b].any() and not u[b].any(), (name, kind, b)
            continue
        shifted += 1
        Fs, Fa = rep["Fs"], R.frames_a(v.shape[0])
        assert steps[b, 0] == Fs and Fs <= 2 * (Fa + 1)
        assert np.array_equal(steps[b, 1:Fs + 2], rep["a"]) and not steps[b, Fs + 2:].any()
        assert not u[b, HOP * (Fs - 1):].any()
    assert shifted >= 1


# ---- the samples --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_stretch_and_output_against_float64(lib, name):
    items = CASES[name]
    r = RANGES[name]
    x, lens = _pad(items)
    u, steps, cents = lib.op_intonation_stretch(x, lens, RATE, r)
    y = lib.op_intonation(x, lens, RATE, r)
    assert y.shape == x.shape and np.isfinite(y).all()
    for b, v in enumerate(items):
        n = v.shape[0]
        assert not y[b, n:].any()  # exactly zero from the length on
        y64, r64 = _ref(v, r, "none", cents[b])
        if n == 0 or not r64["shifted"]:
            assert y[b, :n].tobytes() == v.tobytes(), (name, b)  # no voiced row, a constant track or a short item: x bit for bit
            continue
        y32, r32 = _ref(v, r, "none", cents[b], np.float32)
        n_u = HOP * (r64["Fs"] - 1)
        assert np.array_equal(steps[b, 1:r64["Fs"] + 2], r64["a"])
        for what, dev, ref64, ref32 in (("u", u[b, :n_u], r64["u"], r32["u"]), ("y", y[b, :n], y64, y32)):
            yard = np.abs(ref32.astype(np.float64) - ref64).max()
            dist = np.abs(dev.astype(np.float64) - ref64).max()
            print(f"{name} item {b} {what}: device {dist:.3g}, float32 restatement {yard:.3g} from float64 (x{dist / yard:.2f})")
            assert yard > 0 and dist <= 4 * yard, (name, b, what, dist, yard)
        assert np.abs(y[b, :n]).max() > 0.01


# ---- the exact cases -----------------------------------------------------------------------------------------------------------------
def test_exact_cases_batches_and_repeats(lib):
    items = [I.noise(2048, seed=5), np.zeros(1500, np.float32), R.voiced(8192, seed=1)[:400], R.voiced(4352, seed=0), np.zeros(0, np.float32)]
    x, lens = _pad(items)
    y = lib.op_intonation(x, lens, RATE, 0.0)
    for b in (0, 1, 2):  # noise, zeros, an item below n/2 + 1 samples: x bit for bit
        assert y[b, :lens[b]].tobytes() == items[b].tobytes() and not y[b, lens[b]:].any(), b
    assert not np.array_equal(y[3, :lens[3]], items[3]) and not y[4].any()
    assert y.tobytes() == lib.op_intonation(x, lens, RATE, 0.0).tobytes()  # the same call twice: the same bits
    for b, v in enumerate(items[:4]):  # an item alone: another row length, another batch, the same bits
        alone = lib.op_intonation(v[None], [v.shape[0]], RATE, 0.0)
        assert alone[0].tobytes() == y[b, :v.shape[0]].tobytes(), b
    # r_m == 1000 through the door: every R_f is 1000, every item is x
    y1 = lib.op_intonation(x, lens, RATE, 1.0004)
    for b, v in enumerate(items):
        assert y1[b, :v.shape[0]].tobytes() == v.tobytes()


def test_device_halves_the_movement_of_a_glide(lib):
    x = I.glide(12288)
    y = lib.op_intonation(x[None], [x.shape[0]], RATE, 0.5)[0]
    s, _ = I.slope(x, y, RATE, I.glide_skip(x.shape[0]))
    print(f"slope of the device's output deviation on the input's at r = 0.5: {s:.4f}")
    assert abs(s - 0.5) <= 0.05


# ---- VITS entry points ------------------------------------------------------------------------------------------------------------
def _pcm16(audio, scale):
    v = np.asarray(audio, np.float32) * np.float32(scale)
    v = v * np.float32(32767.0)
    return np.trunc(np.clip(v, np.float32(-32767.0), np.float32(32767.0))).astype(np.int16)


def _cum(ends, hop):
    assert not (ends % hop).any()
    return (ends // hop).astype(np.int32)


@pytest.fixture(scope="module")
def launch_path(hip_lib):
    """single utterances on the launch path for this module's bit-for-bit comparisons of two calls"""
    hip_lib.lib.vits_debug_persist(0)
    yield
    hip_lib.lib.vits_debug_persist(7)


@pytest.mark.parametrize("B", (3, 1))
def test_flagged_synthesize_is_the_door_on_the_unflagged_audio(lib, hip_tiny, launch_path, B):
    rng = np.random.default_rng(61)
    Tx = 24
    lens = np.array([Tx, Tx - 9, 5][:B], np.int64)
    ids = rng.integers(1, 20, size=(B, Tx)).astype(np.int64)
    sid = rng.integers(0, 4, size=B).astype(np.int64)
    hop, native = hip_tiny.hp.hop_length, hip_tiny.hp.sampling_rate
    kw = dict(seed=7, solo=True)
    plain, ol, ends = hip_tiny.synthesize(ids, lens, SCALES, sid, marks=True, **kw)
    assert ol.max() >= R.MIN_LEN
    want = lib.op_intonation(plain, ol, native, 0.0)  # the same kernels on the same samples
    through = lib.op_intonation_stretch(plain, ol, native, 0.0)[1][:, 0] > 0  # the items the device sent through the vocoder
    print(f"B = {B}: items through the vocoder {through.tolist()}")
    got, gl, ge = hip_tiny.synthesize(ids, lens, SCALES, sid, marks=True, pitch_range=0.0, **kw)
    assert got.shape == plain.shape and np.array_equal(gl, ol) and np.array_equal(ge, ends)  # out_samples, lengths and marks do not change
    assert got.tobytes() == want.tobytes()
    for b in range(B):  # (on the toy voice the tracker finds no voiced row: the range alone is the exact case, x bit for bit; with the
        assert np.array_equal(got[b], plain[b]) == (not through[b]), b  # tokens below the same call runs the vocoder on the stage's table)
    # r_m == 1000: the unflagged call's bytes
    same, _ = hip_tiny.synthesize(ids, lens, SCALES, sid, pitch_range=1.0004, **kw)
    assert same.tobytes() == plain.tobytes()
    # int16, and another rate: the plain conversion and the plain resampler on the door's audio
    scale = float(1.25 / np.abs(want).max())
    pcm, pl = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=scale, pitch_range=0.0, **kw)
    assert np.array_equal(pl, ol) and np.array_equal(pcm, _pcm16(want, scale))
    g8, _ = hip_tiny.synthesize(ids, lens, SCALES, sid, sample_rate=8000, pitch_range=0.0, **kw)
    assert g8.tobytes() == lib.op_resample(want, ol, native, 8000).tobytes()
    # with a contour and the call's own shift: the door with the tokens, the shift added to every one
    st = rng.choice([-3.0, 0.0, 4.0], size=(B, Tx)).astype(np.float32)
    db = rng.choice([-6.0, 0.0, 3.0], size=(B, Tx)).astype(np.float32)
    w2 = lib.op_intonation(plain, ol, native, 1.5, cum=_cum(ends, hop), tok_lengths=lens, hop=hop, token_semitones=st + np.float32(2.0), token_gain_db=db)
    g2, _ = hip_tiny.synthesize(ids, lens, SCALES, sid, pitch=2.0, token_pitch=st, token_gain_db=db, pitch_range=1.5, **kw)
    assert g2.tobytes() == w2.tobytes()
    # the call's shift alone: every token carries it
    w3 = lib.op_intonation(plain, ol, native, 1.5, cum=_cum(ends, hop), tok_lengths=lens, hop=hop, token_semitones=np.full((B, Tx), 2.0, np.float32))
    g3, _ = hip_tiny.synthesize(ids, lens, SCALES, sid, pitch=2.0, pitch_range=1.5, **kw)
    assert g3.tobytes() == w3.tobytes()


def test_session_feed_and_eager_path(lib, hip_tiny, launch_path):
    rng = np.random.default_rng(62)
    ids = rng.integers(1, 20, size=(2, 20)).astype(np.int64)
    lens = np.array([20, 11], np.int64)
    sid = np.array([1, 2], np.int64)
    native = hip_tiny.hp.sampling_rate
    lib.lib.vits_debug_fast_path(0)
    try:
        plain, ol = hip_tiny.synthesize(ids, lens, SCALES, sid, seed=5, solo=True)
        got, gl = hip_tiny.synthesize(ids, lens, SCALES, sid, seed=5, solo=True, pitch_range=0.25)
        assert got.tobytes() == lib.op_intonation(plain, ol, native, 0.25).tobytes() and np.array_equal(gl, ol)
    finally:
        lib.lib.vits_debug_fast_path(1)


def test_refusals_by_name_and_the_process_goes_on(lib, hip_tiny):
    from vosk_tts_amd.capi import FLAG_INTONATION, SynthIntonationOpts, VitsError, _p, c_f32p, c_i64p

    ids = np.random.default_rng(63).integers(1, 20, size=(1, 12)).astype(np.int64)
    with pytest.raises(VitsError, match="VITS_FLAG_INTONATION with VITS_FLAG_PITCH_FORMANT") as e:
        hip_tiny.synthesize(ids, [12], SCALES, [1], seed=2, pitch=1.0, preserve_formants=True, pitch_range=0.5)
    assert e.value.code == 4
    with pytest.raises(ValueError, match="pitch_range 4.5"):
        hip_tiny.synthesize(ids, [12], SCALES, [1], seed=2, pitch_range=4.5)
    o = SynthIntonationOpts()
    o.flags, o.pitch_range = FLAG_INTONATION, 0.5
    sc = np.array(SCALES, np.float32)
    stream, total = ctypes.c_void_p(), ctypes.c_int64()
    for name, extra in (("stream_open", ()), ("stream_open_rate", (8000,))):
        rc = lib._fn(name)(hip_tiny._h, _p(ids, c_i64p), 12, _p(sc, c_f32p), 1, ctypes.byref(o), 8, *extra, ctypes.byref(stream), ctypes.byref(total))
        assert rc == 4 and not stream.value
        with pytest.raises(VitsError, match="VITS_FLAG_INTONATION on a stream"):
            lib.check(rc)
    o.pitch_range = float("nan")  # through the C ABI itself: the value is named
    out, ns, ol = c_f32p(), ctypes.c_int64(), np.zeros(1, np.int64)
    with pytest.raises(VitsError, match="pitch_range nan") as e:
        lib.check(lib._fn("synthesize")(hip_tiny._h, _p(ids, c_i64p), _p(np.array([12], np.int64), c_i64p), 1, 12, _p(sc, c_f32p),
                                        _p(np.array([1], np.int64), c_i64p), ctypes.byref(o), ctypes.byref(out), ctypes.byref(ns), _p(ol, c_i64p)))
    assert e.value.code == 1
    audio, ol = hip_tiny.synthesize(ids, [12], SCALES, [1], seed=2)  # a plain request afterwards
    assert ol[0] > 0 and np.isfinite(audio).all()
    assert sum(ch.shape[0] for ch in hip_tiny.stream(ids, SCALES, 1, chunk_frames=8, seed=2)) == ol[0]


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


def test_stts_flag_is_the_door_on_the_unflagged_audio(lib, voice):
    from vosk_tts_amd.capi import VitsError, _p, c_f32p, c_i64p
    from vosk_tts_amd.capi_stts import STTS_FLAG_INTONATION, STTS_FLAG_PITCH, STTS_FLAG_PITCH_FORMANT, SttsIntonationOpts

    sess = voice.onnx
    native = sess._vocoder.hp.sampling_rate
    T = 14
    ids = np.random.default_rng(3).integers(1, 40, size=(5, T)).astype(np.int64)
    pde = np.full(T, 3.0, np.float32)
    kw = dict(seed=9, n_timesteps=2, want_mel=False)
    plain, _, ends = sess._model.synthesize(ids, SC, 2, None, pde, marks=True, **kw)
    assert plain.shape[0] >= R.MIN_LEN
    want = lib.op_intonation(plain[None], [plain.shape[0]], native, 0.0)[0]
    got, _, ge = sess._model.synthesize(ids, SC, 2, None, pde, marks=True, pitch_range=0.0, **kw)
    assert got.tobytes() == want.tobytes() and np.array_equal(ge, ends)
    assert sess._model.synthesize(ids, SC, 2, None, pde, pitch_range=1.0004, **kw)[0].tobytes() == plain.tobytes()  # r_m == 1000
    g8, _, _ = sess._model.synthesize(ids, SC, 2, None, pde, marks=True, sample_rate=8000, pitch_range=0.0, **kw)
    assert g8.tobytes() == lib.op_resample(want[None], [want.shape[0]], native, 8000)[0].tobytes()
    # the session's feed key
    feed = {"input": ids[None], "input_lengths": np.array([T], np.int64), "scales": SC, "sid": np.array([2], np.int64),
            "phone_duration_extra": pde[None], "vits.seed": 9, "vits.n_timesteps": 2}
    assert sess.run(None, dict(feed, **{"vits.pitch_range": 0.0}))[0][0].tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="intonation range"):
        next(iter(sess.run_stream(None, dict(feed, **{"vits.pitch_range": 0.5}))))
    # refusals through the C ABI: the formant flag next to the range, and a stream open with the flag; then a plain call
    m = sess._model
    o = SttsIntonationOpts()
    o.flags, o.pitch_semitones, o.pitch_range = STTS_FLAG_INTONATION | STTS_FLAG_PITCH | STTS_FLAG_PITCH_FORMANT, 1.0, 0.5
    au, ns = c_f32p(), ctypes.c_int64()
    rc = m._fn("synthesize")(m._h, _p(ids, c_i64p), T, _p(SC, c_f32p), 2, None, _p(pde, c_f32p), ctypes.byref(o), ctypes.byref(au), ctypes.byref(ns), None, None)
    assert rc == 4
    with pytest.raises(VitsError, match="STTS_FLAG_INTONATION with STTS_FLAG_PITCH_FORMANT"):
        m.check(rc)
    o.flags = STTS_FLAG_INTONATION
    stream, total = ctypes.c_void_p(), ctypes.c_int64()
    rc = m._fn("stream_open")(m._h, _p(ids, c_i64p), T, _p(SC, c_f32p), 2, None, _p(pde, c_f32p), ctypes.byref(o), 8, ctypes.byref(stream), ctypes.byref(total))
    assert rc == 4 and not stream.value
    with pytest.raises(VitsError, match="STTS_FLAG_INTONATION on a stream"):
        m.check(rc)
    assert sess._model.synthesize(ids, SC, 2, None, pde, **kw)[0].shape == want.shape  # a plain request afterwards


# ---- through Synth ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from vosk_tts_amd import Model, Synth
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.toymodel import PHONEMES, write_toy_model

    d = write_toy_model(str(tmp_path_factory.mktemp("vits") / "m"), W.default_hparams(n_vocab=len(PHONEMES)))
    model = Model(model_path=d, device=0)
    yield Synth(model)
    model.onnx.close()


def test_synth_keyword_session_feed_and_measure_pitch(lib, toy, launch_path):
    import itertools

    text = "прив+ет м+ир др+уг"

    def pinned(fn, *args, **kw):  # (every request draws the session's next seed: the calls compared here draw the same one)
        toy.model.onnx._seed = itertools.count(77)
        return fn(*args, **kw)

    plain, pm = pinned(toy.synth_audio, text, marks=True)
    got, gm = pinned(toy.synth_audio, text, pitch_range=0.0, marks=True)
    assert gm == pm and got.shape == plain.shape  # the marks of the plain call
    via_ssml = pinned(toy.synth_ssml, f'<speak><prosody range="0%">{text}</prosody></speak>')
    assert via_ssml.tobytes() == got.tobytes()
    assert pinned(toy.synth_audio, text, pitch_range=1.0).tobytes() == plain.tobytes()
    with pytest.raises(ValueError, match="intonation range"):
        next(iter(toy.synth_stream(text, pitch_range=0.5)))
    # the session's feed key (through the coalescer, whose key carries the range): the door on the plain request's audio
    sess = toy.model.onnx
    feed = dict(toy._feed(text, 0, None, None, None, None)[0], **{"vits.seed": 5})
    plain_f = sess.run(None, feed)[0]
    got_f = sess.run(None, dict(feed, **{"vits.pitch_range": 0.0}))[0]
    assert got_f.shape == plain_f.shape and plain_f.shape[-1] >= R.MIN_LEN
    want = lib.op_intonation(plain_f.reshape(1, -1), [plain_f.shape[-1]], toy.native_rate(), 0.0)
    assert got_f.tobytes() == want.tobytes()
    assert sess.run(None, dict(feed, **{"vits.pitch_range": 1.0004}))[0].tobytes() == plain_f.tobytes()
    # measure_pitch: the door's track, in Hz
    x = I.glide(8192)
    hz, med = toy.measure_pitch(x)
    cents = lib.op_f0_track(x[None], [x.shape[0]], toy.native_rate())[0]
    assert hz.dtype == np.float32 and hz.shape == cents.shape and np.array_equal(hz > 0, cents > 0)
    assert np.allclose(hz[cents > 0], 27.5 * 2.0 ** (cents[cents > 0] / 1200.0), rtol=1e-6)
    assert 120.0 < med < 200.0 and abs(med - np.median(hz[hz > 0])) < 3.0
    pcm = np.round(x * 32767.0).astype(np.int16)
    hz16, _ = toy.measure_pitch(pcm, rate=toy.native_rate())
    assert np.array_equal(hz16 > 0, hz > 0)
    with pytest.raises(Exception, match="48000"):
        toy.measure_pitch(x, rate=48000)
