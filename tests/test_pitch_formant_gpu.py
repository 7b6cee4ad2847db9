"""Formant-preserving pitch shift on the device (steps 3a-3d of include/vits_pitch.h): pitch_formant_kernel against the float64
restatement (tests/pitch_formant_ref.py) through the parity doors, determinism, and VITS_FLAG_PITCH_FORMANT / STTS_FLAG_PITCH_FORMANT
through the entry points of both model families.  The shapes are those of tests/test_pitch_gpu.py: three ragged items of 513, 2048
and 4173 samples in rows of 4352, NaN behind every length, at -12, -4, +3 and +12 semitones (an F_a = 3 item, F_s = 2 at -12, the clamp
of kappa at +3 and +12, Q n near its maximum at the ratios with gcd 1).

Tolerance, as there: the float32 run of the restatement is an fp32 implementation of the same definition; its largest deviation from
the float64 run on the very same item is the yardstick, and the device may sit 4 times that far from float64.  For the gains the
deviation is the relative error per bin.  Measured on an MI355X (the worst of the four shifts, device / yardstick):
    vits_op_pitch_formant_gain     item 513: 4.2e-7 / 9.8e-7,  item 2048: 5.4e-7 / 2.5e-6,  item 4173 (voiced): 2.7e-6 / 3.3e-5   (at most 0.5 x)
    vits_op_pitch_shift_formant    item 513: 2.0e-7 / 1.6e-7,  item 2048: 2.4e-7 / 2.2e-7,  item 4173 (voiced): 1.0e-6 / 7.0e-7   (at most 1.5 x)
    vits_op_pitch_stretch_formant  item 2048: 2.5e-7 / 2.4e-7                                                              (at most 1.1 x)
(The gains come out closer than the yardstick because the kernel forms the magnitudes under its logarithm in double; with the fp32
analysis rows they read 1.8 to 4.5 x: DESIGN.md "Formant-preserving pitch".)
"""
import ctypes

import numpy as np
import pytest

import pitch_formant_ref as F
import pitch_ref as R

pytestmark = pytest.mark.gpu

SCALES = [0.667, 1.0, 0.8]
SC = np.array([0.8, 1.0, 0.8], np.float32)
NATIVE = 22050


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert hip_lib.has_pitch_formant, "libvits_mi355.so exports no vits_op_pitch_formant_gain"
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
    """per shift: the float64 and float32 runs of the restatement on every item (y, the gains) and u of the 2048-sample item, once"""
    its = items[0]
    cache = {}

    def get(s):
        if s not in cache:
            P, Q = R.plan(s)
            c = dict(y64=[], y32=[], g64=[], g32=[])
            for v in its:
                for dt, tag in ((np.float64, "64"), (np.float32, "32")):
                    rep = {}
                    c["y" + tag].append(F.pitch_shift_formant(v, s, dt, rep))
                    c["g" + tag].append(rep["gain"])
            c["u64"] = F.stretch_formant(its[1], P, Q, np.float64)
            c["u32"] = F.stretch_formant(its[1], P, Q, np.float32)
            cache[s] = c
        return cache[s]

    return get


def _pcm16(audio, scale):
    """the conversion of vits_synthesize_pcm16 in fp32: scale, * 32767, clip, truncating cast"""
    v = np.asarray(audio, np.float32) * np.float32(scale)
    v = v * np.float32(32767.0)
    return np.trunc(np.clip(v, np.float32(-32767.0), np.float32(32767.0))).astype(np.int16)


# ---- the kernel against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", R.GPU_SEMITONES)
def test_op_gain_against_float64(lib, items, refs, s):
    its, x, lens = items
    g = lib.op_pitch_formant_gain(x, lens, s)
    assert g.shape == (3, F.gain_rows(R.GPU_N), R.NB) and np.isfinite(g).all()
    r = refs(s)
    for b, v in enumerate(its):
        Fa = R.frames_a(v.shape[0])
        g64 = r["g64"][b]
        assert g64.shape == (Fa, R.NB)
        yard = np.abs(r["g32"][b].astype(np.float64) / g64 - 1).max()
        dev = np.abs(g[b, :Fa].astype(np.float64) / g64 - 1).max()
        print(f"s={s} item {b} ({v.shape[0]} samples): device {dev:.3g}, float32 restatement {yard:.3g} from float64, relative (x{dev / yard:.2f})")
        assert yard > 0 and dev <= 4 * yard, (s, b, dev, yard)
        assert not g[b, Fa:].any()  # exactly zero behind the last frame
        assert (g[b, :Fa, 0] == 1).all()  # bin 0 stays where it is


@pytest.mark.parametrize("s", R.GPU_SEMITONES)
def test_op_shift_and_stretch_against_float64(lib, items, refs, s):
    its, x, lens = items
    P, Q = R.plan(s)
    y = lib.op_pitch_shift_formant(x, lens, s)
    assert y.shape == x.shape and np.isfinite(y).all()
    r = refs(s)
    for b, v in enumerate(its):
        n = v.shape[0]
        yard = np.abs(r["y32"][b].astype(np.float64) - r["y64"][b]).max()
        dev = np.abs(y[b, :n].astype(np.float64) - r["y64"][b]).max()
        print(f"s={s} shift, item {b} ({n} samples): device {dev:.3g}, float32 restatement {yard:.3g} from float64 (x{dev / yard:.2f})")
        assert yard > 0 and dev <= 4 * yard, (s, b, dev, yard)
        assert not y[b, n:].any()  # exactly zero beyond the length
        assert np.abs(y[b, :R.HOP * (n // R.HOP)]).max() > 0.05  # (and not silence inside it)
    u = lib.op_pitch_stretch_formant(x[1:2, :2048], lens[1:2], s)
    n_u = R.n_u(2048, P, Q)
    assert u.shape == (1, R.stretch_samples(2048, P, Q)) and r["u64"].shape == (n_u,) and np.isfinite(u).all()
    yard = np.abs(r["u32"].astype(np.float64) - r["u64"]).max()
    dev = np.abs(u[0, :n_u].astype(np.float64) - r["u64"]).max()
    print(f"s={s} stretch, 2048 samples: device {dev:.3g}, float32 restatement {yard:.3g} from float64 (x{dev / yard:.2f})")
    assert yard > 0 and dev <= 4 * yard, (s, dev, yard)
    assert not u[0, n_u:].any()
    assert not np.array_equal(y, lib.op_pitch_shift(x, lens, s))  # (the correction does something)


def test_padding_is_never_read_and_short_items_come_back(lib):
    rng = np.random.default_rng(3)
    N = 1100
    x = np.full((4, N), np.nan, np.float32)
    lens = np.array([512, 0, 1100, 769], np.int64)  # below n/2 + 1; empty; the whole row; one sample past a hop
    for b, n in enumerate(lens):
        x[b, :n] = 0.2 * rng.standard_normal(n)
    for s in (5.0, -7.0):
        P, Q = R.plan(s)
        y = lib.op_pitch_shift_formant(x, lens, s)
        assert np.isfinite(y).all()
        for b, n in enumerate(lens):
            assert not y[b, n:].any()
        assert y[0, :512].tobytes() == x[0, :512].tobytes()  # a 512-sample item: bit-identical
        assert np.abs(y[2, :1024]).max() > 0.05 and np.abs(y[3, :768]).max() > 0.05
        u = lib.op_pitch_stretch_formant(x, lens, s)
        assert np.isfinite(u).all() and not u[0].any() and not u[1].any() and not u[2, R.n_u(1100, P, Q):].any()
        g = lib.op_pitch_formant_gain(x, lens, s)
        assert g.shape == (4, F.gain_rows(N), R.NB) and np.isfinite(g).all()
        assert not g[0].any() and not g[1].any()  # an item below n/2 + 1 samples: every row exactly 0
        for b in (2, 3):
            Fa = R.frames_a(lens[b])
            assert (g[b, :Fa] > 0).all() and not g[b, Fa:].any()
    # frames of exact zeros (frame f covers the samples [256 f - 512, 256 f + 512): 0 .. 4 here): their gain is exactly 1
    z = np.zeros((1, 2048), np.float32)
    z[0, 1600:] = 0.2 * rng.standard_normal(448)
    g = lib.op_pitch_formant_gain(z, [2048], 3.0)
    assert (g[0, :5] == 1).all() and (g[0, :9] > 0).all() and not (g[0, 8] == 1).all() and not g[0, 9:].any()


def test_items_do_not_depend_on_their_batch_and_calls_repeat(lib, items):
    its, x, lens = items
    for s in (3.0, -12.0):
        y = lib.op_pitch_shift_formant(x, lens, s)
        g = lib.op_pitch_formant_gain(x, lens, s)
        assert y.tobytes() == lib.op_pitch_shift_formant(x, lens, s).tobytes()  # the same call twice: the same bits
        assert g.tobytes() == lib.op_pitch_formant_gain(x, lens, s).tobytes()
        for b, v in enumerate(its):
            n = v.shape[0]
            alone = lib.op_pitch_shift_formant(v[None], [n], s)  # another row length, another batch
            assert alone[0].tobytes() == y[b, :n].tobytes(), (s, b)
            ga = lib.op_pitch_formant_gain(v[None], [n], s)
            assert ga[0].tobytes() == g[b, :ga.shape[1]].tobytes(), (s, b)


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
    fk = dict(kw, preserve_formants=True)
    plain, ol, ends = hip_tiny.synthesize(ids, lens, SCALES, sid, marks=True, **kw)
    assert ol.max() >= R.MIN_LEN
    s = 4.0
    want = lib.op_pitch_shift_formant(plain, ol, s)  # the same kernels on the same samples
    got, gl, ge = hip_tiny.synthesize(ids, lens, SCALES, sid, marks=True, pitch=s, **fk)
    assert np.array_equal(gl, ol) and np.array_equal(ge, ends) and got.shape == plain.shape  # lengths and marks do not change
    assert got.tobytes() == want.tobytes()
    shifted, _ = hip_tiny.synthesize(ids, lens, SCALES, sid, pitch=s, **kw)
    assert shifted.tobytes() == lib.op_pitch_shift(plain, ol, s).tobytes()  # VITS_FLAG_PITCH alone: the plain path has not moved
    assert not np.array_equal(got, shifted)  # a corrected call differs from the plain pitch call
    scale = float(1.25 / np.abs(want).max())  # the loudest samples clip
    pcm, pl = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=scale, pitch=s, **fk)
    assert np.array_equal(pl, ol) and np.array_equal(pcm, _pcm16(want, scale))
    # at 8000 Hz with a loudness target: pitch -> resample -> normalise -> int16
    spec = loudness_spec(loudness=-19.0)
    p8, l8, e8 = hip_tiny.synthesize(ids, lens, SCALES, sid, marks=True, sample_rate=8000, **kw)
    w8 = lib.op_loudness_normalize(lib.op_resample(want, ol, NATIVE, 8000), l8, 8000, *spec)[0]
    g8, m8, f8 = hip_tiny.synthesize(ids, lens, SCALES, sid, marks=True, sample_rate=8000, pitch=s, loudness=spec, **fk)
    assert np.array_equal(m8, l8) and np.array_equal(f8, e8) and g8.tobytes() == w8.tobytes()
    p16, q8, h8 = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=0.7, sample_rate=8000, marks=True, pitch=s, loudness=spec, **fk)
    assert np.array_equal(p16, _pcm16(w8, 0.7)) and np.array_equal(q8, l8) and np.array_equal(h8, e8)
    r16, _ = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=0.7, sample_rate=8000, pitch=s, **fk)  # the resampler converts
    assert np.array_equal(r16, _pcm16(lib.op_resample(want, ol, NATIVE, 8000), 0.7))


def test_eager_path_takes_the_flag(lib, hip_tiny, launch_path):
    ids, lens, sid = _ragged(np.random.default_rng(42), 3)
    lib.lib.vits_debug_fast_path(0)
    try:
        plain, ol = hip_tiny.synthesize(ids, lens, SCALES, sid, seed=5, solo=True)
        got, gl = hip_tiny.synthesize(ids, lens, SCALES, sid, seed=5, solo=True, pitch=-4.0, preserve_formants=True)
        assert got.tobytes() == lib.op_pitch_shift_formant(plain, ol, -4.0).tobytes() and np.array_equal(gl, ol)
        e16, _ = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=0.7, seed=5, solo=True, pitch=-4.0, preserve_formants=True)
        assert np.array_equal(e16, _pcm16(got, 0.7))
    finally:
        lib.lib.vits_debug_fast_path(1)


def _c_synthesize(lib, model, ids, flags, semitones, seed=3):
    """vits_synthesize through the C ABI with the flags as given -> (status, audio or None)"""
    from vosk_tts_amd.capi import SynthPitchOpts, _p, c_f32p, c_i64p

    o = SynthPitchOpts()
    o.flags, o.seed, o.pitch_semitones = flags, seed, semitones
    out, ns, ol = c_f32p(), ctypes.c_int64(), np.zeros(1, np.int64)
    sc = np.array(SCALES, np.float32)
    T = ids.shape[1]
    rc = lib._fn("synthesize")(model._h, _p(ids, c_i64p), _p(np.array([T], np.int64), c_i64p), 1, T, _p(sc, c_f32p),
                               _p(np.array([1], np.int64), c_i64p), ctypes.byref(o), ctypes.byref(out), ctypes.byref(ns), _p(ol, c_i64p))
    if rc:
        return rc, None
    try:
        return 0, np.ctypeslib.as_array(out, shape=(1, ns.value)).copy()
    finally:
        lib._fn("free_output")(out)


def test_flag_handling_and_the_plain_paths_have_not_moved(lib, hip_tiny, launch_path):
    from vosk_tts_amd.capi import FLAG_PITCH, FLAG_PITCH_FORMANT, VitsError, _p, c_f32p, c_i64p, SynthPitchOpts

    ids = np.random.default_rng(43).integers(1, 20, size=(1, 16)).astype(np.int64)
    a, al = hip_tiny.synthesize(ids, [16], SCALES, [1], seed=3)
    rc, _ = _c_synthesize(lib, hip_tiny, ids, FLAG_PITCH_FORMANT, 4.0)  # the formant flag without the pitch flag
    assert rc == 1  # VITS_ERR_ARG
    with pytest.raises(VitsError, match="VITS_FLAG_PITCH_FORMANT without VITS_FLAG_PITCH"):
        lib.check(rc)
    o = SynthPitchOpts()
    o.flags, o.pitch_semitones = FLAG_PITCH_FORMANT, 4.0
    st, total = ctypes.c_void_p(), ctypes.c_int64()
    sc = np.array(SCALES, np.float32)
    assert lib._fn("stream_open")(hip_tiny._h, _p(ids, c_i64p), 16, _p(sc, c_f32p), 1, ctypes.byref(o), 8, ctypes.byref(st), ctypes.byref(total)) == 1
    assert not st.value
    o.flags = FLAG_PITCH | FLAG_PITCH_FORMANT  # a stream keeps refusing pitch
    assert lib._fn("stream_open")(hip_tiny._h, _p(ids, c_i64p), 16, _p(sc, c_f32p), 1, ctypes.byref(o), 8, ctypes.byref(st), ctypes.byref(total)) == 4
    with pytest.raises(VitsError, match="pitch-shifted"):
        hip_tiny.stream(ids, SCALES, 1, pitch=2.0)
    rc, b = _c_synthesize(lib, hip_tiny, ids, 0, 0.0)  # a normal request afterwards
    assert rc == 0 and b.tobytes() == a.tobytes()
    rc, b = _c_synthesize(lib, hip_tiny, ids, FLAG_PITCH | FLAG_PITCH_FORMANT, 0.0004)  # P = Q: the bytes of the unflagged call
    assert rc == 0 and b.tobytes() == a.tobytes()
    rc, b = _c_synthesize(lib, hip_tiny, ids, FLAG_PITCH, 4.0)  # VITS_FLAG_PITCH alone: what vits_op_pitch_shift gives
    assert rc == 0 and b.tobytes() == lib.op_pitch_shift(a, al, 4.0).tobytes()
    rc, b = _c_synthesize(lib, hip_tiny, ids, FLAG_PITCH | FLAG_PITCH_FORMANT, 4.0)
    assert rc == 0 and b.tobytes() == lib.op_pitch_shift_formant(a, al, 4.0).tobytes()
    # through Python the bit is set only with a pitch in effect: the call as it was, launches included
    lib.lib.vits_debug_fast_path(0)  # the eager path: one counted launch per kernel
    try:
        dumps = []
        for kw in ({}, dict(preserve_formants=True), dict(pitch=0.0, preserve_formants=True)):
            lib.launch_log(1)
            try:
                out = hip_tiny.synthesize_pcm16(ids, [16], SCALES, [1], seed=3, **kw)[0]
            finally:
                lib.launch_log(0)
            dumps.append((out.tobytes(), lib.launch_dump()))
    finally:
        lib.lib.vits_debug_fast_path(1)
    assert dumps[0] == dumps[1] == dumps[2]


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


def test_stts_flag_is_the_op_chain_on_the_unflagged_audio(lib, voice):
    from vosk_tts_amd.capi import VitsError, _p, c_f32p, c_i64p, loudness_spec
    from vosk_tts_amd.capi_stts import STTS_FLAG_PITCH_FORMANT, SttsPitchOpts

    sess = voice.onnx
    native = sess._vocoder.hp.sampling_rate
    T, s = 14, -5.0
    ids, pde = _ms_ids(T, 3), np.full(T, 3.0, np.float32)
    kw = dict(seed=9, n_timesteps=2, want_mel=False)
    fk = dict(kw, pitch=s, preserve_formants=True)
    plain, _ = sess._model.synthesize(ids, SC, 2, None, pde, **kw)
    assert plain.shape[0] >= R.MIN_LEN
    want = lib.op_pitch_shift_formant(plain[None], [plain.shape[0]], s)[0]
    got, _ = sess._model.synthesize(ids, SC, 2, None, pde, **fk)
    assert got.tobytes() == want.tobytes()
    shifted, _ = sess._model.synthesize(ids, SC, 2, None, pde, pitch=s, **kw)
    assert shifted.tobytes() == lib.op_pitch_shift(plain[None], [plain.shape[0]], s)[0].tobytes() and not np.array_equal(got, shifted)
    assert sess._model.synthesize(ids, SC, 2, None, pde, preserve_formants=True, **kw)[0].tobytes() == plain.tobytes()  # no pitch: as it was
    assert sess._model.synthesize(ids, SC, 2, None, pde, pitch=0.0, preserve_formants=True, **kw)[0].tobytes() == plain.tobytes()
    # the marks form at another rate with a peak target: pitch -> resample -> normalise; the marks do not move
    spec = loudness_spec(peak=0.5)
    p8, _, e8 = sess._model.synthesize(ids, SC, 2, None, pde, marks=True, sample_rate=8000, **kw)
    w8 = lib.op_loudness_normalize(lib.op_resample(want[None], [want.shape[0]], native, 8000), [p8.shape[0]], 8000, *spec)[0][0]
    g8, _, f8 = sess._model.synthesize(ids, SC, 2, None, pde, marks=True, sample_rate=8000, loudness=spec, **fk)
    assert g8.tobytes() == w8.tobytes() and np.array_equal(e8, f8)
    # the batch doors: ragged, every item from its own length
    B = 3
    lens = np.array([T, 9, 4], np.int64)
    bids = np.stack([_ms_ids(T, 10 + b) for b in range(B)])
    bpde = np.full((B, T), 3.0, np.float32)
    bkw = dict(seed=0, n_timesteps=2, item_seeds=[5, 6, 7])
    plain_b, ol = sess._model.synthesize_batch(bids, lens, SC, [0, 1, 2], None, bpde, **bkw)
    got, gl = sess._model.synthesize_batch(bids, lens, SC, [0, 1, 2], None, bpde, pitch=s, preserve_formants=True, **bkw)
    assert np.array_equal(gl, ol) and got.tobytes() == lib.op_pitch_shift_formant(plain_b, ol, s).tobytes()
    p8, l8, e8 = sess._model.synthesize_batch(bids, lens, SC, [0, 1, 2], None, bpde, marks=True, sample_rate=8000, **bkw)
    g8, m8, f8 = sess._model.synthesize_batch(bids, lens, SC, [0, 1, 2], None, bpde, marks=True, sample_rate=8000, pitch=s, preserve_formants=True, **bkw)
    assert np.array_equal(l8, m8) and np.array_equal(e8, f8)
    assert g8.tobytes() == lib.op_resample(lib.op_pitch_shift_formant(plain_b, ol, s), ol, native, 8000).tobytes()
    # the flag without the pitch flag, through the C ABI: VITS_ERR_ARG naming both, and a normal request afterwards
    m = sess._model
    o = SttsPitchOpts()
    o.flags, o.seed, o.n_timesteps, o.pitch_semitones = STTS_FLAG_PITCH_FORMANT, 9, 2, s
    out, ns = c_f32p(), ctypes.c_int64()
    rc = m._fn("synthesize")(m._h, _p(ids, c_i64p), T, _p(SC, c_f32p), 2, None, _p(pde, c_f32p), ctypes.byref(o), ctypes.byref(out), ctypes.byref(ns),
                             None, None)
    assert rc == 1
    with pytest.raises(VitsError, match="STTS_FLAG_PITCH_FORMANT without STTS_FLAG_PITCH"):
        m.check(rc)
    assert sess._model.synthesize(ids, SC, 2, None, pde, **kw)[0].tobytes() == plain.tobytes()


def test_stts_session_takes_the_feed_key(lib, voice):
    sess = voice.onnx
    T = 14
    feed = {"input": _ms_ids(T, 3)[None], "input_lengths": np.array([T], np.int64), "scales": SC, "sid": np.array([2], np.int64),
            "phone_duration_extra": np.full((1, T), 3.0, np.float32), "vits.seed": 9, "vits.n_timesteps": 2}
    plain = sess.run(None, feed)[0][0]
    got = sess.run(None, dict(feed, **{"vits.pitch": 2.0, "vits.pitch_formants": True}))[0][0]
    assert got.tobytes() == lib.op_pitch_shift_formant(plain[None], [plain.shape[0]], 2.0)[0].tobytes()
    assert sess.run(None, dict(feed, **{"vits.pitch_formants": True}))[0][0].tobytes() == plain.tobytes()
    with pytest.raises(ValueError, match="frames before a chunk"):
        sess.run_stream(None, dict(feed, **{"vits.pitch": 2.0, "vits.pitch_formants": True}))


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


def test_synth_audio_the_session_and_the_batch_door_take_the_option(lib, toy):
    from vosk_tts_amd.batching import MultiDeviceSynth

    d, synth = toy
    sess = synth.model.onnx
    ids = np.array([synth.g2p_noembed(TEXT)], np.int64)
    feed = {"input": ids, "input_lengths": np.array([ids.shape[1]], np.int64), "scales": SC, "sid": np.array([2], np.int64), "bert": None,
            "phone_duration_extra": None, "vits.seed": 11}
    plain = sess.run(None, feed)[0].reshape(1, -1)
    both = {"vits.pitch": 4.0, "vits.pitch_formants": True}
    got = sess.run(None, dict(feed, **both))[0].reshape(1, -1)
    assert got.tobytes() == lib.op_pitch_shift_formant(plain, [plain.shape[1]], 4.0).tobytes()
    assert np.array_equal(sess.run_pcm16(dict(feed, **both), 2.0), _pcm16(got, 2.0))
    assert sess.run(None, dict(feed, **{"vits.pitch_formants": True}))[0].tobytes() == plain.tobytes()  # no pitch: the plain call
    w0, e0 = sess.run(None, dict(feed, **{"vits.marks": True}))
    w1, e1 = sess.run(None, dict(feed, **{"vits.marks": True}, **both))
    assert w1.shape == w0.shape and np.array_equal(e0, e1) and w1.reshape(1, -1).tobytes() == got.tobytes()
    a1 = synth.synth_audio(TEXT, speaker_id=2, scale=1.0, preserve_formants=True)  # (free-running durations: its own length)
    assert a1.dtype == np.int16 and a1.shape[0] > 0
    a2, m2 = synth.synth_audio(TEXT, speaker_id=2, scale=1.0, marks=True, pitch=4, preserve_formants=True)
    assert a2.dtype == np.int16 and a2.shape[0] == m2.token_ends[-1] > 0 and np.abs(a2.astype(np.int32)).max() > 0
    texts = ["прив+ет, м+ир!", TEXT]
    mds = MultiDeviceSynth(d, devices=[0], max_batch=4)
    try:
        kept = mds.synth_batch(texts, speaker_ids=[2, 0], seeds=[101, 7], scale=1.0, pitch=4.0, preserve_formants=True)
        moved = mds.synth_batch(texts, speaker_ids=[2, 0], seeds=[101, 7], scale=1.0, pitch=4.0)
        same = mds.synth_batch(texts, speaker_ids=[2, 0], seeds=[101, 7], scale=1.0, preserve_formants=True)
        base = mds.synth_batch(texts, speaker_ids=[2, 0], seeds=[101, 7], scale=1.0)
        for i, t in enumerate(texts):
            one = np.array([synth.g2p_noembed(t)], np.int64)
            f = {"input": one, "input_lengths": np.array([one.shape[1]], np.int64), "scales": np.array([0.8, 1.0, 0.8], np.float32),
                 "sid": np.array([[2, 0][i]], np.int64), "bert": None, "phone_duration_extra": None, "vits.seed": [101, 7][i], **both}
            solo = sess.run_pcm16(f, 1.0)[0]
            assert kept[i].shape == solo.shape == moved[i].shape and not np.array_equal(kept[i], moved[i])
            assert same[i].tobytes() == base[i].tobytes()
    finally:
        mds.close()
