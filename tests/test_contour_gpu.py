"""Per-token pitch and volume contours on the device (include/vits_contour.h): the kernels against the float64 restatement
(tests/contour_ref.py) through the parity doors, the exact cases, padding / batching / determinism, and the flag through the entry points
of both model families.

Tolerance of the sample-wise comparisons, as in tests/test_pitch_gpu.py: the float32 run of the restatement is an fp32 implementation of
the same definition; its largest deviation from the float64 run on the very same item is the yardstick, and the device may sit 4 times
that far from float64.  The positions are integers and must be equal.

Measured on an MI355X (largest distance from float64: device / float32 restatement):
    y  513: 1.00e-7 / 8.37e-8   1024: 9.33e-8 / 9.33e-8   ragged: 1.11e-7 / 1.31e-7, 1.53e-7 / 1.83e-7, 2.46e-7 / 2.01e-7
       8192: 1.76e-7 / 2.36e-7                                                                                    (at most 1.2 x)
    u  513: 9.96e-8 / 5.48e-8   1024: 9.39e-8 / 1.06e-7   ragged: 4.32e-8 / 8.0e-8, 8.75e-8 / 8.9e-8, 7.2e-8 / 1.08e-7
       8192: 5.44e-8 / 2.51e-7                                                                                    (at most 1.8 x)
With the fp32 analysis transform of the pitch stage u sat at 4.9 x (513) and 4.8 x (8192): the contour stage transforms its frames in
double (contour_analysis_kernel).
"""
import ctypes

import numpy as np
import pytest

import contour_ref as C
import pitch_ref as R

pytestmark = pytest.mark.gpu

HOP = 256
SCALES = [0.667, 1.0, 0.8]
SC = np.array([0.8, 1.0, 0.8], np.float32)
NATIVE = 22050


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert hip_lib.has_contour, "libvits_mi355.so exports no vits_op_contour"
    return hip_lib


def _noise(n, seed):
    return (0.2 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _case(items):
    """items: [(x, cum, semitones, gain_db)] -> the padded arrays of a door call (x poisoned with NaN beyond every length)"""
    B = len(items)
    N = max(max(it[0].shape[0] for it in items), 1)
    Tx = max(max(len(it[1]) for it in items), 1)
    x = np.full((B, N), np.nan, np.float32)
    cum = np.zeros((B, Tx), np.int32)
    st = np.zeros((B, Tx), np.float32)
    db = np.zeros((B, Tx), np.float32)
    lens = np.zeros(B, np.int64)
    tl = np.zeros(B, np.int64)
    for b, (v, c, s, g) in enumerate(items):
        x[b, :v.shape[0]] = v
        lens[b], tl[b] = v.shape[0], len(c)
        cum[b, :len(c)] = c
        cum[b, len(c):] = c[-1] if len(c) else 0
        st[b, :len(c)] = s
        db[b, :len(c)] = g
    return x, lens, cum, tl, st, db


def _ref(item, dtype=np.float64):
    v, c, s, g = item
    rep = {}
    y = C.contour(v, np.asarray(c, np.int64), len(c), HOP, s, g, dtype, rep)
    return y, rep


# the parity cases: (name, items)
PARITY = {
    "513": [(_noise(513, 1), [1, 3], [5.0, -7.0], [3.0, -6.0])],
    "1024": [(_noise(1024, 2), [1, 2, 4], [-12.0, 12.0, 2.0], [0.0, 6.0, -12.0])],
    "ragged": [(R.voiced(4352, seed=0), [3, 3, 9, 17], [2.0, 9.0, -3.0, 4.0], [0.0, 0.0, 4.0, -3.0]),
               (_noise(2048, 3), [8], [-5.0], [2.0]),
               (_noise(769, 4), [2, 4], [12.0, -12.0], [-40.0, 12.0])],
    "8192": [(R.voiced(8192, seed=1), [8, 20, 26, 32], [-12.0, 12.0, 0.0, 5.0], [0.0, 3.0, -3.0, 0.0])],
}


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = [(_ref(it, np.float64), _ref(it, np.float32)) for it in PARITY[name]]
        return cache[name]

    return get


# ---- positions ---------------------------------------------------------------------------------------------------------------------
POSITIONS = {
    "adjacent_extremes": [(_noise(4096, 5), [8, 16], [-12.0, 12.0], [0.0, 0.0])],
    "zero_frame_token": [(_noise(4096, 6), [4, 4, 10, 16], [3.0, 9.0, -2.0, 5.0], [0.0, 0.0, 0.0, 0.0])],
    "single_token": [(_noise(4173, 7), [17], [7.0], [0.0])],
    "boundaries_near_the_ends": [(_noise(4096, 8), [2, 14, 16], [6.0, 0.0, -6.0], [0.0, 0.0, 0.0])],
    "ragged_with_an_empty_item": [(_noise(4352, 9), [5, 17], [-4.0, 11.0], [0.0, 0.0]), (_noise(0, 0), [], [], []),
                                  (_noise(1024, 10), [1, 4], [1.0, -1.0], [0.0, 0.0])],
}


@pytest.mark.parametrize("name", list(POSITIONS))
def test_positions_equal_the_restatement(lib, name):
    items = POSITIONS[name]
    x, lens, cum, tl, st, db = _case(items)
    u, steps = lib.op_contour_stretch(x, lens, cum, tl, HOP, st, db)
    assert steps.shape == (len(items), C.steps_columns(x.shape[1])) and u.shape == (len(items), C.stretch_samples(x.shape[1]))
    assert np.isfinite(u).all()
    for b, it in enumerate(items):
        if it[0].shape[0] == 0:
            assert not steps[b].any() and not u[b].any()
            continue
        _, rep = _ref(it)
        Fs = rep["Fs"]
        assert steps[b, 0] == Fs and Fs <= 2 * (R.frames_a(it[0].shape[0]) + 1)
        assert np.array_equal(steps[b, 1:Fs + 2], rep["a"]) and not steps[b, Fs + 2:].any()
        assert not u[b, HOP * (Fs - 1):].any()


# ---- parity, u then y --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PARITY))
def test_stretch_against_float64(lib, refs, name):
    items = PARITY[name]
    x, lens, cum, tl, st, db = _case(items)
    u, steps = lib.op_contour_stretch(x, lens, cum, tl, HOP, st, db)
    for b, ((y64, r64), (y32, r32)) in enumerate(refs(name)):
        n_u = HOP * (r64["Fs"] - 1)
        assert np.array_equal(steps[b, 1:r64["Fs"] + 2], r64["a"])
        yard = np.abs(r32["u"].astype(np.float64) - r64["u"]).max()
        dev = np.abs(u[b, :n_u].astype(np.float64) - r64["u"]).max()
        print(f"{name} item {b} u: device {dev:.3g}, float32 restatement {yard:.3g} from float64 (x{dev / yard:.2f})")
        assert yard > 0 and dev <= 4 * yard, (name, b, dev, yard)
        assert not u[b, n_u:].any()


@pytest.mark.parametrize("name", list(PARITY))
def test_contour_against_float64(lib, refs, name):
    items = PARITY[name]
    x, lens, cum, tl, st, db = _case(items)
    y = lib.op_contour(x, lens, cum, tl, HOP, st, db)
    assert y.shape == x.shape and np.isfinite(y).all()
    for b, ((y64, r64), (y32, r32)) in enumerate(refs(name)):
        n = items[b][0].shape[0]
        yard = np.abs(y32.astype(np.float64) - y64).max()
        dev = np.abs(y[b, :n].astype(np.float64) - y64).max()
        print(f"{name} item {b} y: device {dev:.3g}, float32 restatement {yard:.3g} from float64 (x{dev / yard:.2f})")
        assert yard > 0 and dev <= 4 * yard, (name, b, dev, yard)
        assert not y[b, n:].any()  # exactly zero from the length on
        assert np.abs(y[b, :n]).max() > 0.01


# ---- the exact cases ---------------------------------------------------------------------------------------------------------------
def test_exact_cases(lib):
    v = _noise(2048, 11)
    x, lens, cum, tl, st, db = _case([(v, [3, 8], [0.0, 0.0], [0.0, 0.0])])
    assert lib.op_contour(x, lens, cum, tl, HOP, st, db)[0].tobytes() == v.tobytes()  # all neutral: x bit for bit
    assert lib.op_contour(x, lens, cum, tl, HOP, None, None)[0].tobytes() == v.tobytes()
    it = (v, [3, 8], [0.0, 0.0], [6.0, -9.0])
    x, lens, cum, tl, st, db = _case([it])
    want = _ref(it)[0].astype(np.float32)
    got = lib.op_contour(x, lens, cum, tl, HOP, st, db)[0]
    assert got.tobytes() == want.tobytes() and not np.array_equal(got, v)  # gain only: the restatement bit for bit
    short = (_noise(300, 12), [1, 2], [7.0, -7.0], [6.0, 0.0])  # below n/2 + 1: gain only
    x, lens, cum, tl, st, db = _case([short])
    assert lib.op_contour(x, lens, cum, tl, HOP, st, db)[0].tobytes() == _ref(short)[0].astype(np.float32).tobytes()
    assert _ref(short)[1]["shifted"] is False


def test_items_do_not_depend_on_their_batch_and_calls_repeat(lib):
    items = PARITY["ragged"] + [(_noise(300, 13), [2], [3.0], [-3.0]), (_noise(1500, 14), [2, 6], [0.0, 0.0], [3.0, -3.0])]
    x, lens, cum, tl, st, db = _case(items)
    y = lib.op_contour(x, lens, cum, tl, HOP, st, db)
    assert y.tobytes() == lib.op_contour(x, lens, cum, tl, HOP, st, db).tobytes()  # the same call twice: the same bytes
    for b, it in enumerate(items):
        n = it[0].shape[0]
        assert not y[b, n:].any()
        alone = lib.op_contour(*_case([it])[:4], HOP, *_case([it])[4:])  # another row length, another batch
        assert alone[0].tobytes() == y[b, :n].tobytes(), b


def test_device_moves_the_fundamental_of_every_token(lib):
    x = C.tone()
    st = [0.0, 4.0, -5.0, 12.0]
    y = lib.op_contour(x[None], [x.shape[0]], np.array([[16, 32, 48, 64]], np.int32), [4], HOP, np.array([st], np.float32), None)[0]
    P = C.token_ratios(st)
    for t in range(4):
        f = C.fundamental(y[t * 4096 + 1024:t * 4096 + 3072])
        want = 200.0 * P[t] / 1000.0
        assert abs(f - want) <= 0.01 * want, (t, f, want)


def test_doors_refuse_by_name(lib):
    from vosk_tts_amd.capi import VitsError

    x, lens, cum, tl, st, db = _case([(_noise(1024, 15), [2, 4], [0.0, 12.5], [0.0, 0.0])])
    with pytest.raises(VitsError, match="12.5 semitones at item 0, token 1") as e:
        lib.op_contour(x, lens, cum, tl, HOP, st, db)
    assert e.value.code == 1
    st[0, 1], db[0, 0] = 0.0, np.nan
    with pytest.raises(VitsError, match="dB at item 0, token 0"):
        lib.op_contour(x, lens, cum, tl, HOP, st, db)
    db[0, 0] = 0.0
    assert lib.op_contour(x, lens, cum, tl, HOP, st, db)[0].tobytes() == x[0].tobytes()


# ---- VITS entry points ------------------------------------------------------------------------------------------------------------
def _pcm16(audio, scale):
    """the conversion of vits_synthesize_pcm16 in fp32: scale, * 32767, clip, truncating cast"""
    v = np.asarray(audio, np.float32) * np.float32(scale)
    v = v * np.float32(32767.0)
    return np.trunc(np.clip(v, np.float32(-32767.0), np.float32(32767.0))).astype(np.int16)


def _ragged(rng, B, Tx=24, n_vocab=20):
    lens = np.array([Tx, Tx - 9, 5][:B], np.int64)
    ids = rng.integers(1, n_vocab, size=(B, Tx)).astype(np.int64)
    sid = rng.integers(0, 4, size=B).astype(np.int64)
    return ids, lens, sid


def _tokens(rng, B, Tx):
    st = rng.choice([-12.0, -3.0, 0.0, 4.0, 12.0], size=(B, Tx)).astype(np.float32)
    db = rng.choice([-9.0, 0.0, 6.0], size=(B, Tx)).astype(np.float32)
    return st, db


def _cum(ends, hop):
    """token_ends at the native rate -> the inclusive frame counts"""
    assert not (ends % hop).any()
    return (ends // hop).astype(np.int32)


@pytest.fixture(scope="module")
def launch_path(hip_lib):
    """single utterances on the launch path for this module's bit-for-bit comparisons of two calls"""
    hip_lib.lib.vits_debug_persist(0)
    yield
    hip_lib.lib.vits_debug_persist(7)


@pytest.mark.parametrize("solo", (False, True), ids=("padded", "solo"))
@pytest.mark.parametrize("B", (3, 1))
def test_flagged_synthesize_is_the_door_on_the_unflagged_audio(lib, hip_tiny, launch_path, B, solo):
    ids, lens, sid = _ragged(np.random.default_rng(51), B)
    st, db = _tokens(np.random.default_rng(52), B, ids.shape[1])
    hop = hip_tiny.hp.hop_length
    kw = dict(seed=7, solo=solo)
    plain, ol, ends = hip_tiny.synthesize(ids, lens, SCALES, sid, marks=True, **kw)
    assert ol.max() >= R.MIN_LEN
    want = lib.op_contour(plain, ol, _cum(ends, hop), lens, hop, st, db)  # the same kernels on the same samples, with the plain call's marks
    got, gl, ge = hip_tiny.synthesize(ids, lens, SCALES, sid, marks=True, token_pitch=st, token_gain_db=db, **kw)
    assert got.shape == plain.shape and np.array_equal(gl, ol) and np.array_equal(ge, ends)  # out_samples, lengths and marks do not change
    assert got.tobytes() == want.tobytes() and not np.array_equal(got, plain)
    g2, _ = hip_tiny.synthesize(ids, lens, SCALES, sid, token_pitch=st, token_gain_db=db, **kw)
    assert g2.tobytes() == want.tobytes()
    # VITS_FLAG_PITCH plus a contour: the contour with the semitones added
    st2 = np.clip(st, -10.0, 10.0)
    w2 = lib.op_contour(plain, ol, _cum(ends, hop), lens, hop, st2 + np.float32(2.0), db)
    g3, _ = hip_tiny.synthesize(ids, lens, SCALES, sid, pitch=2.0, token_pitch=st2, token_gain_db=db, **kw)
    assert g3.tobytes() == w2.tobytes()
    # int16: the float output converted
    scale = float(1.25 / np.abs(want).max())
    pcm, pl = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=scale, token_pitch=st, token_gain_db=db, **kw)
    assert np.array_equal(pl, ol) and np.array_equal(pcm, _pcm16(want, scale))
    # at 8000 Hz: the plain resampler on the contoured native audio
    g8, l8 = hip_tiny.synthesize(ids, lens, SCALES, sid, sample_rate=8000, token_pitch=st, token_gain_db=db, **kw)
    assert g8.tobytes() == lib.op_resample(want, ol, NATIVE, 8000).tobytes()
    p8, _ = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=0.7, sample_rate=8000, token_pitch=st, token_gain_db=db, **kw)
    assert np.array_equal(p8, _pcm16(lib.op_resample(want, ol, NATIVE, 8000), 0.7))
    # gain only
    g4, _ = hip_tiny.synthesize(ids, lens, SCALES, sid, token_gain_db=db, **kw)
    assert g4.tobytes() == lib.op_contour(plain, ol, _cum(ends, hop), lens, hop, None, db).tobytes()


def test_eager_path_and_neutral_contours(lib, hip_tiny, launch_path):
    ids, lens, sid = _ragged(np.random.default_rng(53), 3)
    st, db = _tokens(np.random.default_rng(54), 3, ids.shape[1])
    hop = hip_tiny.hp.hop_length
    lib.lib.vits_debug_fast_path(0)
    try:
        plain, ol, ends = hip_tiny.synthesize(ids, lens, SCALES, sid, seed=5, solo=True, marks=True)
        got, gl = hip_tiny.synthesize(ids, lens, SCALES, sid, seed=5, solo=True, token_pitch=st, token_gain_db=db)
        assert got.tobytes() == lib.op_contour(plain, ol, _cum(ends, hop), lens, hop, st, db).tobytes() and np.array_equal(gl, ol)
        e16, _ = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=0.7, seed=5, solo=True, token_pitch=st, token_gain_db=db)
        assert np.array_equal(e16, _pcm16(got, 0.7))
    finally:
        lib.lib.vits_debug_fast_path(1)
    # an all-neutral contour is the call it was: through the binding (no flag) and through the flag itself
    from vosk_tts_amd.capi import FLAG_CONTOUR, Contour, SynthContourOpts, _p, c_f32p, c_i64p

    a, al = hip_tiny.synthesize(ids, lens, SCALES, sid, seed=5)
    b, _ = hip_tiny.synthesize(ids, lens, SCALES, sid, seed=5, token_pitch=np.zeros_like(st), token_gain_db=np.zeros_like(db))
    assert a.tobytes() == b.tobytes()
    zeros = np.zeros_like(st)
    c = Contour()
    c.token_semitones = _p(zeros, c_f32p)
    o = SynthContourOpts()
    o.flags, o.seed, o.contour = FLAG_CONTOUR, 5, ctypes.pointer(c)
    out, ns, ol2 = c_f32p(), ctypes.c_int64(), np.zeros(3, np.int64)
    sc = np.array(SCALES, np.float32)
    lib.check(lib._fn("synthesize")(hip_tiny._h, _p(ids, c_i64p), _p(lens, c_i64p), 3, ids.shape[1], _p(sc, c_f32p), _p(sid, c_i64p), ctypes.byref(o),
                                    ctypes.byref(out), ctypes.byref(ns), _p(ol2, c_i64p)))
    try:
        assert np.ctypeslib.as_array(out, shape=(3, ns.value)).tobytes() == a.tobytes()
    finally:
        lib._fn("free_output")(out)


def test_refusals_by_name_and_the_process_goes_on(lib, hip_tiny):
    from vosk_tts_amd.capi import FLAG_CONTOUR, Contour, SynthContourOpts, VitsError, _p, c_f32p, c_i64p

    ids = np.random.default_rng(55).integers(1, 20, size=(1, 12)).astype(np.int64)
    st = np.full((1, 12), 2.0, np.float32)
    with pytest.raises(VitsError, match="VITS_FLAG_CONTOUR with VITS_FLAG_PITCH_FORMANT") as e:
        hip_tiny.synthesize(ids, [12], SCALES, [1], seed=2, pitch=1.0, preserve_formants=True, token_pitch=st)
    assert e.value.code == 4
    with pytest.raises(ValueError, match="14 semitones at item 0, token 0"):
        hip_tiny.synthesize(ids, [12], SCALES, [1], seed=2, token_pitch=st + 12.0)
    c = Contour()
    c.token_semitones = _p(st, c_f32p)
    o = SynthContourOpts()
    o.flags, o.contour = FLAG_CONTOUR, ctypes.pointer(c)
    sc = np.array(SCALES, np.float32)
    stream, total = ctypes.c_void_p(), ctypes.c_int64()
    for name, extra in (("stream_open", ()), ("stream_open_rate", (8000,))):
        rc = lib._fn(name)(hip_tiny._h, _p(ids, c_i64p), 12, _p(sc, c_f32p), 1, ctypes.byref(o), 8, *extra, ctypes.byref(stream), ctypes.byref(total))
        assert rc == 4 and not stream.value
        with pytest.raises(VitsError, match="VITS_FLAG_CONTOUR on a stream"):
            lib.check(rc)
    o2 = SynthContourOpts()
    o2.flags = FLAG_CONTOUR  # the flag with a NULL contour
    out, ns, ol = c_f32p(), ctypes.c_int64(), np.zeros(1, np.int64)
    with pytest.raises(VitsError, match="NULL contour") as e:
        lib.check(lib._fn("synthesize")(hip_tiny._h, _p(ids, c_i64p), _p(np.array([12], np.int64), c_i64p), 1, 12, _p(sc, c_f32p),
                                        _p(np.array([1], np.int64), c_i64p), ctypes.byref(o2), ctypes.byref(out), ctypes.byref(ns), _p(ol, c_i64p)))
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


def _ms_ids(T, seed, n_vocab=40):
    return np.random.default_rng(seed).integers(1, n_vocab, size=(5, T)).astype(np.int64)


def test_stts_flag_is_the_door_on_the_unflagged_audio(lib, voice):
    from vosk_tts_amd.capi import VitsError, _p, c_f32p, c_i64p
    from vosk_tts_amd.capi_stts import STTS_FLAG_CONTOUR, STTS_FLAG_PITCH, STTS_FLAG_PITCH_FORMANT, SttsContourOpts
    from vosk_tts_amd.capi import Contour

    sess = voice.onnx
    hop = sess._vocoder.hp.hop_length
    native = sess._vocoder.hp.sampling_rate
    T = 14
    ids, pde = _ms_ids(T, 3), np.full(T, 3.0, np.float32)
    st, db = _tokens(np.random.default_rng(56), 1, T)
    kw = dict(seed=9, n_timesteps=2, want_mel=False)
    plain, _, ends = sess._model.synthesize(ids, SC, 2, None, pde, marks=True, **kw)
    assert plain.shape[0] >= R.MIN_LEN
    want = lib.op_contour(plain[None], [plain.shape[0]], _cum(ends, hop)[None], [T], hop, st, db)[0]
    got, _, ge = sess._model.synthesize(ids, SC, 2, None, pde, marks=True, token_pitch=st[0], token_gain_db=db[0], **kw)
    assert got.tobytes() == want.tobytes() and np.array_equal(ge, ends) and not np.array_equal(got, plain)
    assert sess._model.synthesize(ids, SC, 2, None, pde, token_pitch=st[0], token_gain_db=db[0], **kw)[0].tobytes() == want.tobytes()
    g8, _, e8 = sess._model.synthesize(ids, SC, 2, None, pde, marks=True, sample_rate=8000, token_pitch=st[0], token_gain_db=db[0], **kw)
    assert g8.tobytes() == lib.op_resample(want[None], [want.shape[0]], native, 8000)[0].tobytes()
    # the session's feed keys
    feed = {"input": ids[None], "input_lengths": np.array([T], np.int64), "scales": SC, "sid": np.array([2], np.int64),
            "phone_duration_extra": pde[None], "vits.seed": 9, "vits.n_timesteps": 2}
    assert sess.run(None, dict(feed, **{"vits.token_pitch": st, "vits.token_gain_db": db}))[0][0].tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="stream"):
        next(iter(sess.run_stream(None, dict(feed, **{"vits.token_pitch": st}))))
    # the batch door: ragged, every item from its own tokens
    B = 3
    lens = np.array([T, 9, 4], np.int64)
    bids = np.stack([_ms_ids(T, 10 + b) for b in range(B)])
    bpde = np.full((B, T), 3.0, np.float32)
    bst, bdb = _tokens(np.random.default_rng(57), B, T)
    bkw = dict(seed=0, n_timesteps=2, item_seeds=[5, 6, 7])
    plain, ol, ends = sess._model.synthesize_batch(bids, lens, SC, [0, 1, 2], None, bpde, marks=True, **bkw)
    got, gl = sess._model.synthesize_batch(bids, lens, SC, [0, 1, 2], None, bpde, token_pitch=bst, token_gain_db=bdb, **bkw)
    assert np.array_equal(gl, ol) and got.tobytes() == lib.op_contour(plain, ol, _cum(ends, hop), lens, hop, bst, bdb).tobytes()
    # refusals through the C ABI: the formant flag next to the contour, and a stream open with the flag; then a plain call
    m = sess._model
    c = Contour()
    c.token_semitones = _p(st, c_f32p)
    o = SttsContourOpts()
    o.flags, o.pitch_semitones, o.contour = STTS_FLAG_CONTOUR | STTS_FLAG_PITCH | STTS_FLAG_PITCH_FORMANT, 1.0, ctypes.pointer(c)
    au, ns = c_f32p(), ctypes.c_int64()
    rc = m._fn("synthesize")(m._h, _p(ids, c_i64p), T, _p(SC, c_f32p), 2, None, _p(pde, c_f32p), ctypes.byref(o), ctypes.byref(au), ctypes.byref(ns), None, None)
    assert rc == 4
    with pytest.raises(VitsError, match="STTS_FLAG_CONTOUR with STTS_FLAG_PITCH_FORMANT"):
        m.check(rc)
    o.flags = STTS_FLAG_CONTOUR
    stream, total = ctypes.c_void_p(), ctypes.c_int64()
    rc = m._fn("stream_open")(m._h, _p(ids, c_i64p), T, _p(SC, c_f32p), 2, None, _p(pde, c_f32p), ctypes.byref(o), 8, ctypes.byref(stream), ctypes.byref(total))
    assert rc == 4 and not stream.value
    with pytest.raises(VitsError, match="STTS_FLAG_CONTOUR on a stream"):
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


def test_synth_keywords_and_ssml(lib, toy, launch_path):
    import itertools

    text = "прив+ет м+ир др+уг"

    def pinned(fn, *args, **kw):  # (every request draws the session's next seed: the calls compared here draw the same one)
        toy.model.onnx._seed = itertools.count(77)
        return fn(*args, **kw)

    plain, pm = pinned(toy.synth_audio, text, marks=True)
    got, gm = pinned(toy.synth_audio, text, word_pitch={1: 3.0}, marks=True)
    assert gm == pm and got.shape == plain.shape and not np.array_equal(got, plain)  # the marks of the plain call
    doc = '<speak>прив+ет <prosody pitch="+3st" volume="+6dB">м+ир</prosody><break time="250ms"/> др+уг<mark name="end"/></speak>'
    a = pinned(toy.synth_ssml, doc)
    b = pinned(toy.synth_audio, text, word_pitch={1: 3.0}, word_gains={1: 6.0}, pauses={1: 0.25})
    assert a.tobytes() == b.tobytes() and a.shape[0] > plain.shape[0]
    a2, am = pinned(toy.synth_ssml, doc, marks=True)
    assert a2.tobytes() == a.tobytes() and am.named == {"end": a.shape[0]}
    with pytest.raises(ValueError, match="contoured"):
        next(iter(toy.model.onnx.run_stream(None, dict(toy._feed(text, 0, None, None, None, None)[0], **{"vits.token_pitch": np.zeros((1, 4), np.float32)}))))
