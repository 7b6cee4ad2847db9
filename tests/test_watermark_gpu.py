"""GPU tests of the audio watermark (include/vits_watermark.h): the two doors against the float64 restatement
(tests/watermark_ref.py), determinism, where the stage sits in the output tail of both voice families on both host paths, the whole way
from Synth.synth_audio to Synth.detect_watermark, and the refusals.

Bounds.  The embed door and the detector's z_all are allowed four times the distance of the restatement's own fp32 run from its float64
run (the limiter's rule, tests/test_limit_gpu.py): the device runs another FFT factorisation with an fp32 twiddle table, and its ln is
the device's.  offset and rows are compared as integers; tests/test_watermark.py keeps every input of the detector at least 2 away
from the threshold, six orders of magnitude more than that distance."""
import ctypes
import hashlib
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import watermark_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = 0x5EED1234
SCALES = [0.667, 1.0, 0.8]
SC = np.array([0.8, 1.0, 0.8], np.float32)
SEED = 31
LUFS = -23.0


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert hip_lib.has_watermark
    return hip_lib


@pytest.fixture(scope="module")
def signal():
    """the test signal, marked by the restatement: computed once, never written to"""
    x = R.voiced_signal(3.0)
    y = R.embed(x, KEY).astype(np.float32)
    for a in (x, y):
        a.setflags(write=False)
    return x, y


# ---- the doors ----------------------------------------------------------------------------------------------------------------------
def test_op_against_float64(lib, signal):
    x1 = signal[0][:22050]
    lengths = np.array([600, 5000, 22050], np.int64)
    x = np.stack([x1, x1[::-1], x1]).astype(np.float32)
    for b, n in enumerate(lengths):
        x[b, n:] = 1e30  # never read
    for depth in (0.0, 2.0):
        y = lib.op_watermark(x, lengths, KEY, depth)
        assert y.shape == x.shape and y.dtype == np.float32
        for b, n in enumerate(lengths):
            n = int(n)
            ref64 = R.embed(x[b, :n], KEY, depth)
            ref32 = R.embed(x[b, :n], KEY, depth, dtype=np.float32)
            yard = np.abs(ref32.astype(np.float64) - ref64).max()
            dist = np.abs(y[b, :n].astype(np.float64) - ref64).max()
            print(f"depth {depth or 1.0} dB len {n}: device {dist:.3g}, float32 restatement {yard:.3g} from float64 (x{dist / yard:.2f})")
            assert yard > 0 and dist <= 4 * yard, (depth, n, dist, yard)
            assert not y[b, n:].any()  # exactly zero from the length on
            tail = 256 * (n // 256)
            assert y[b, tail:n].tobytes() == x[b, tail:n].tobytes()  # the samples behind the last whole hop: x bit for bit
            assert np.abs(y[b, :tail] - x[b, :tail]).max() > 1e-3  # and marked in front of them
        assert y.tobytes() == lib.op_watermark(x, lengths, KEY, depth).tobytes()  # no atomics: the same bits twice
    assert lib.op_watermark(x, lengths, KEY, 0.0).tobytes() == lib.op_watermark(x, lengths, KEY, 1.0).tobytes()  # 0 = the default
    short = x[:1, :400]
    assert lib.op_watermark(short, [400], KEY).tobytes() == short.tobytes()  # below n/2 + 1 samples: as it went in
    y512 = lib.op_watermark(x[:1, :600], [512], KEY)
    assert y512[0, :512].tobytes() == x[0, :512].tobytes() and not y512[0, 512:].any()


def test_detector_against_float64(lib, signal):
    x, y = signal
    items = [y, x, y[5000:]]
    lens = np.array([a.shape[0] for a in items], np.int64)
    xs = np.full((3, int(lens.max())), 1e30, np.float32)  # (beyond an item: never read)
    for b, a in enumerate(items):
        xs[b, :lens[b]] = a
    z, off, rows, z_all = lib.op_watermark_detect(xs, lens, KEY)
    assert z_all.shape == (3, 128) and z_all.dtype == np.float64 and np.isfinite(z_all).all()
    yard = dist = 0.0
    for b, a in enumerate(items):
        d64, d32 = R.detect(a, KEY), R.detect(a, KEY, dtype=np.float32)
        yard = max(yard, np.abs(d32["z_all"] - d64["z_all"]).max())
        dist = max(dist, np.abs(z_all[b] - d64["z_all"]).max())
        assert (int(off[b]), int(rows[b])) == (d64["offset"], d64["rows"]), b
        assert z[b] == z_all[b].max() and bool(z[b] >= R.THRESHOLD) == d64["detected"] and abs(z[b] - R.THRESHOLD) >= 2.0
        print(f"item {b}: z {z[b]:.4f} (float64 {d64['z']:.4f}) offset {off[b]} rows {rows[b]}")
    print(f"z_all: device {dist:.3g}, float32 restatement {yard:.3g} from float64 (x{dist / yard:.2f})")
    assert yard > 0 and dist <= 4 * yard
    assert [bool(v >= R.THRESHOLD) for v in z] == [True, False, True]
    # the wrong key, silence, and an item without a frame
    assert lib.op_watermark_detect(xs[:1], lens[:1], KEY + 1)[0][0] < 4.0
    z0, o0, r0, za0 = lib.op_watermark_detect(np.zeros((2, 4096), np.float32), [4096, 400], KEY)
    assert not z0.any() and not o0.any() and not za0.any() and r0.tolist() == [R.detect(np.zeros(4096), KEY)["rows"], 0]


def test_items_do_not_depend_on_their_batch_and_calls_repeat(lib, signal):
    x, y = signal
    items = [y[:22050], x[3000:9000], y[12345:40000], x[:400], x[:513]]
    lens = np.array([a.shape[0] for a in items], np.int64)
    xs = np.zeros((len(items), int(lens.max())), np.float32)
    for b, a in enumerate(items):
        xs[b, :lens[b]] = a
    m = lib.op_watermark(xs, lens, KEY, 1.5)
    d = lib.op_watermark_detect(xs, lens, KEY)
    assert m.tobytes() == lib.op_watermark(xs, lens, KEY, 1.5).tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(d, lib.op_watermark_detect(xs, lens, KEY)))
    for b, a in enumerate(items):  # an item alone: another row length, another batch, the same bits
        alone = lib.op_watermark(a[None], [a.shape[0]], KEY, 1.5)
        assert alone[0].tobytes() == m[b, :a.shape[0]].tobytes(), b
        da = lib.op_watermark_detect(a[None], [a.shape[0]], KEY)
        assert all(u[0].tobytes() == v[b].tobytes() for u, v in zip(da, d)), b


def test_op_refusals_name_the_value(lib):
    from vosk_tts_amd.capi import VitsError

    x = np.zeros((1, 4096), np.float32)
    for bad, match in ((-0.5, "-0.5"), (2.5, "2.5"), (float("nan"), "nan")):
        with pytest.raises(VitsError, match=match) as e:
            lib.op_watermark(x, [4096], KEY, bad)
        assert e.value.code == 1  # VITS_ERR_ARG
    with pytest.raises(VitsError, match="4097") as e:
        lib.op_watermark(x, [4097], KEY)
    assert e.value.code == 1
    with pytest.raises(VitsError, match="4097"):
        lib.op_watermark_detect(x, [4097], KEY)


# ---- VITS entry points: where the stage sits ----------------------------------------------------------------------------------------
def _pcm16(audio, scale):
    v = np.asarray(audio, np.float32) * np.float32(scale)
    v = v * np.float32(32767.0)
    return np.trunc(np.clip(v, np.float32(-32767.0), np.float32(32767.0))).astype(np.int16)


class _Path:
    """one host path: the fast one as it is, the eager one with vits_debug_fast_path(0) around every call"""

    def __init__(self, lib, fast):
        self.lib, self.fast = lib, fast

    def call(self, fn, *a, **kw):
        self.lib.lib.vits_debug_fast_path(1 if self.fast else 0)
        try:
            return fn(*a, **kw)
        finally:
            self.lib.lib.vits_debug_fast_path(1)


@pytest.fixture(scope="module")
def launch_path(hip_lib):
    """single utterances on the launch path for this module's bit-for-bit comparisons of two calls"""
    hip_lib.lib.vits_debug_persist(0)
    yield
    hip_lib.lib.vits_debug_persist(7)


def _feed(B):
    rng = np.random.default_rng(61)
    Tx = 24
    lens = np.array([Tx, Tx - 9, 5][:B], np.int64)
    ids = rng.integers(1, 20, size=(B, Tx)).astype(np.int64)
    sid = rng.integers(0, 4, size=B).astype(np.int64)
    return ids, lens, sid


@pytest.mark.parametrize("fast", (True, False), ids=("fast", "eager"))
@pytest.mark.parametrize("B", (3, 1))
def test_flagged_synthesize_is_the_door_on_the_unflagged_audio(lib, hip_tiny, launch_path, B, fast):
    from vosk_tts_amd.capi import LOUDNESS_LUFS

    ids, lens, sid = _feed(B)
    native = hip_tiny.hp.sampling_rate
    path = _Path(lib, fast)
    kw = dict(seed=SEED, solo=True)
    plain, ol, ends = path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, marks=True, **kw)
    assert ol.max() >= 513
    want = lib.op_watermark(plain, ol, KEY)  # the same kernels on the same samples
    got, gl, ge = path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, marks=True, watermark=KEY, **kw)
    assert got.shape == plain.shape and np.array_equal(gl, ol) and np.array_equal(ge, ends)  # out_samples, lengths and marks do not change
    assert got.tobytes() == want.tobytes() and not np.array_equal(got, plain)
    d2 = path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, watermark=KEY, watermark_depth_db=2.0, **kw)[0]
    assert d2.tobytes() == lib.op_watermark(plain, ol, KEY, 2.0).tobytes()
    # another rate: marked at the rate it is returned at
    p8, ol8 = path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, sample_rate=8000, **kw)
    g8, gl8 = path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, sample_rate=8000, watermark=KEY, **kw)
    assert np.array_equal(gl8, ol8) and g8.tobytes() == lib.op_watermark(p8, ol8, KEY).tobytes()
    # a loudness target: the gain is measured on, and applied to, the marked audio
    for rate, marked, n in ((None, want, ol), (8000, lib.op_watermark(p8, ol8, KEY), ol8)):
        gn, _ = path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, sample_rate=rate, watermark=KEY, loudness=(LOUDNESS_LUFS, LUFS, 0.0), **kw)
        assert gn.tobytes() == lib.op_loudness_normalize(marked, n, rate or native, LOUDNESS_LUFS, LUFS, 0.0)[0].tobytes(), rate
    # int16: the conversion of the marked float audio with the call's scale (the stage's own epilogue, the resampled form, and behind the gain)
    scale = float(1.25 / np.abs(want).max())
    pcm, pl = path.call(hip_tiny.synthesize_pcm16, ids, lens, SCALES, sid, pcm_scale=scale, watermark=KEY, **kw)
    assert np.array_equal(pl, ol) and np.array_equal(pcm, _pcm16(want, scale))
    pcm8, _ = path.call(hip_tiny.synthesize_pcm16, ids, lens, SCALES, sid, pcm_scale=scale, sample_rate=8000, watermark=KEY, **kw)
    assert np.array_equal(pcm8, _pcm16(lib.op_watermark(p8, ol8, KEY), scale))
    pcmn, _ = path.call(hip_tiny.synthesize_pcm16, ids, lens, SCALES, sid, pcm_scale=0.5, watermark=KEY, loudness=(LOUDNESS_LUFS, LUFS, 0.0), **kw)
    assert np.array_equal(pcmn, _pcm16(lib.op_loudness_normalize(want, ol, native, LOUDNESS_LUFS, LUFS, 0.0)[0], 0.5))
    # behind the pitch stage: the door on the shifted call's audio
    ps, _ = path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, pitch=2.0, **kw)
    gs, _ = path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, pitch=2.0, watermark=KEY, **kw)
    assert gs.tobytes() == lib.op_watermark(ps, ol, KEY).tobytes()
    # the unflagged call afterwards: the bytes of before
    assert path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, **kw)[0].tobytes() == plain.tobytes()


@pytest.mark.parametrize("fast", (True, False), ids=("fast", "eager"))
def test_flagged_document_is_the_door_on_the_unflagged_document(lib, hip_tiny, fast):
    ids, lens, sid = _feed(3)
    path = _Path(lib, fast)
    kw = dict(seed=SEED, lead_frames=2, gap_frames=[3, 0, 2], fade_samples=9)
    for rate in (None, 8000):
        plain, info = path.call(hip_tiny.synthesize_document, ids, lens, SCALES, sid, sample_rate=rate, **kw)
        got, gi = path.call(hip_tiny.synthesize_document, ids, lens, SCALES, sid, sample_rate=rate, watermark=KEY, **kw)
        assert got.shape == plain.shape and np.array_equal(gi["seg_end"], info["seg_end"])
        # marked as the one item it has become
        assert got.tobytes() == lib.op_watermark(plain[None], [plain.shape[0]], KEY)[0].tobytes(), rate
    scale = float(1.25 / np.abs(got).max())
    pcm, _ = path.call(hip_tiny.synthesize_document, ids, lens, SCALES, sid, sample_rate=8000, pcm=True, pcm_scale=scale, watermark=KEY, **kw)
    assert np.array_equal(pcm, _pcm16(got, scale))


def test_refusals_by_name_and_the_process_goes_on(lib, hip_tiny, tiny_blob, launch_path, tmp_path):
    from vosk_tts_amd.capi import FLAG_WATERMARK, SynthWatermarkOpts, VitsError, _p, c_f32p, c_i64p

    ids = np.random.default_rng(63).integers(1, 20, size=(1, 12)).astype(np.int64)
    with pytest.raises(ValueError, match="watermark_depth_db 2.5"):
        hip_tiny.synthesize(ids, [12], SCALES, [1], seed=2, watermark=KEY, watermark_depth_db=2.5)
    with pytest.raises(VitsError, match="FLAG_WATERMARK") as e:
        hip_tiny.stream(ids, SCALES, 1, chunk_frames=8, seed=2, watermark=KEY)
    assert e.value.code == 4
    o = SynthWatermarkOpts()
    o.flags, o.watermark_key = FLAG_WATERMARK, KEY
    sc = np.array(SCALES, np.float32)
    stream, total = ctypes.c_void_p(), ctypes.c_int64()
    for name, extra in (("stream_open", ()), ("stream_open_rate", (8000,))):  # both stream opens, through the C ABI itself
        rc = lib._fn(name)(hip_tiny._h, _p(ids, c_i64p), 12, _p(sc, c_f32p), 1, ctypes.byref(o), 8, *extra, ctypes.byref(stream), ctypes.byref(total))
        assert rc == 4 and not stream.value
        with pytest.raises(VitsError, match="VITS_FLAG_WATERMARK on a stream"):
            lib.check(rc)
    o.watermark_depth_db = float("nan")  # the value is named
    out, ns, ol = c_f32p(), ctypes.c_int64(), np.zeros(1, np.int64)
    with pytest.raises(VitsError, match="depth nan") as e:
        lib.check(lib._fn("synthesize")(hip_tiny._h, _p(ids, c_i64p), _p(np.array([12], np.int64), c_i64p), 1, 12, _p(sc, c_f32p),
                                        _p(np.array([1], np.int64), c_i64p), ctypes.byref(o), ctypes.byref(out), ctypes.byref(ns), _p(ol, c_i64p)))
    assert e.value.code == 1
    hip_tiny.synthesize(ids, [12], SCALES, [1], seed=2, watermark=KEY)  # this process has seen the flag
    audio, ol = hip_tiny.synthesize(ids, [12], SCALES, [1], seed=2)  # a plain request afterwards
    assert ol[0] > 0 and np.isfinite(audio).all()
    assert sum(ch.shape[0] for ch in hip_tiny.stream(ids, SCALES, 1, chunk_frames=8, seed=2)) == ol[0]
    # the unflagged call's digest equals the one a process takes whose library never saw the flag
    blob = tmp_path / "tiny.vitsw"
    blob.write_bytes(tiny_blob)
    child = ("import sys, hashlib, numpy as np, torch\n"
             f"sys.path.insert(0, {ROOT!r})\n"
             "from vosk_tts_amd.capi import VitsLib\n"
             "lib = VitsLib(); lib.lib.vits_debug_persist(0)\n"
             f"m = lib.create(open({str(blob)!r}, 'rb').read(), 0)\n"
             f"ids = np.random.default_rng(63).integers(1, 20, size=(1, 12)).astype(np.int64)\n"
             f"a, ol = m.synthesize(ids, [12], {SCALES!r}, [1], seed=2)\n"
             "print(hashlib.sha256(a.tobytes()).hexdigest())\n")
    fresh = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=120)
    assert fresh.returncode == 0, fresh.stderr[-2000:]
    assert fresh.stdout.split()[-1] == hashlib.sha256(audio.tobytes()).hexdigest()


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
    from vosk_tts_amd.capi import LOUDNESS_LUFS, VitsError, _p, c_f32p, c_i64p
    from vosk_tts_amd.capi_stts import STTS_FLAG_WATERMARK, SttsWatermarkOpts

    sess = voice.onnx
    m = sess._model
    native = sess._vocoder.hp.sampling_rate
    T = 14
    ids = np.random.default_rng(3).integers(1, 40, size=(5, T)).astype(np.int64)
    pde = np.full(T, 3.0, np.float32)
    kw = dict(seed=9, n_timesteps=2, want_mel=False)
    for dn in ({}, {"denoiser_strength": 0.05}):  # with and without the denoiser in front
        plain, _, ends = m.synthesize(ids, SC, 2, None, pde, marks=True, **kw, **dn)
        n = plain.shape[0]
        assert n >= 513
        want = lib.op_watermark(plain[None], [n], KEY)[0]
        got, _, ge = m.synthesize(ids, SC, 2, None, pde, marks=True, watermark=KEY, **kw, **dn)
        assert got.tobytes() == want.tobytes() and np.array_equal(ge, ends) and not np.array_equal(got, plain)
        p8, _, _ = m.synthesize(ids, SC, 2, None, pde, marks=True, sample_rate=8000, **kw, **dn)
        g8, _, _ = m.synthesize(ids, SC, 2, None, pde, marks=True, sample_rate=8000, watermark=KEY, **kw, **dn)
        assert g8.tobytes() == lib.op_watermark(p8[None], [p8.shape[0]], KEY)[0].tobytes()
        gn, _ = m.synthesize(ids, SC, 2, None, pde, watermark=KEY, loudness=(LOUDNESS_LUFS, LUFS, 0.0), **kw, **dn)
        assert gn.tobytes() == lib.op_loudness_normalize(want[None], [n], native, LOUDNESS_LUFS, LUFS, 0.0)[0][0].tobytes()
    # the batch call: every item from its own length (the last plain / want are those with the denoiser)
    B = 3
    bids = np.random.default_rng(4).integers(1, 40, size=(B, 5, T)).astype(np.int64)
    blens = np.array([T, T - 5, 6], np.int64)
    bpde = np.full((B, T), 3.0, np.float32)
    bkw = dict(seed=9, n_timesteps=2)
    bp, bl = m.synthesize_batch(bids, blens, SC, [0, 1, 2], None, bpde, **bkw)
    bg, bgl = m.synthesize_batch(bids, blens, SC, [0, 1, 2], None, bpde, watermark=KEY, **bkw)
    assert np.array_equal(bgl, bl) and bg.tobytes() == lib.op_watermark(bp, bl, KEY).tobytes()
    dp, _ = m.synthesize_document(bids, blens, SC, [0, 1, 2], None, bpde, gap_frames=[2, 0, 1], **bkw)
    dg, _ = m.synthesize_document(bids, blens, SC, [0, 1, 2], None, bpde, gap_frames=[2, 0, 1], watermark=KEY, **bkw)
    assert dg.tobytes() == lib.op_watermark(dp[None], [dp.shape[0]], KEY)[0].tobytes()
    # the session's feed keys, at the native rate (inside the library) and at another (behind the session's resampler)
    feed = {"input": ids[None], "input_lengths": np.array([T], np.int64), "scales": SC, "sid": np.array([2], np.int64),
            "phone_duration_extra": pde[None], "vits.seed": 9, "vits.n_timesteps": 2}
    for rate in (None, 8000):
        f = dict(feed, **({"vits.sample_rate": rate} if rate else {}))
        p = sess.run(None, f)[0]
        g = sess.run(None, dict(f, **{"vits.watermark_key": KEY}))[0]
        assert g.tobytes() == lib.op_watermark(p, [p.shape[1]], KEY).tobytes(), rate
    with pytest.raises(ValueError, match="FLAG_WATERMARK"):
        next(iter(sess.run_stream(None, dict(feed, **{"vits.watermark_key": KEY}))))
    bfeed = {"input": bids, "input_lengths": blens, "scales": SC, "sid": np.array([0, 1, 2], np.int64), "phone_duration_extra": bpde,
             "vits.seed": 9, "vits.n_timesteps": 2}
    for rate in (None, 8000):  # the batch door as a feed: marked behind the session's resampler, in front of its normalisation
        f = dict(bfeed, **({"vits.sample_rate": rate} if rate else {}))
        p, pl = sess.run_batch(f)
        g, gl = sess.run_batch(dict(f, **{"vits.watermark_key": KEY}))
        marked = lib.op_watermark(p, pl, KEY)
        assert np.array_equal(gl, pl) and g.tobytes() == marked.tobytes(), rate
        gn, _ = sess.run_batch(dict(f, **{"vits.watermark_key": KEY, "vits.loudness": LUFS, "vits.peak_ceiling": 0.0}))
        assert gn.tobytes() == lib.op_loudness_normalize(marked, pl, rate or native, LOUDNESS_LUFS, LUFS, 0.0)[0].tobytes(), rate
    # the stream open through the C ABI refuses by name; then a plain call
    o = SttsWatermarkOpts()
    o.flags, o.watermark_key = STTS_FLAG_WATERMARK, KEY
    stream, total = ctypes.c_void_p(), ctypes.c_int64()
    rc = m._fn("stream_open")(m._h, _p(ids, c_i64p), T, _p(SC, c_f32p), 2, None, _p(pde, c_f32p), ctypes.byref(o), 8, ctypes.byref(stream), ctypes.byref(total))
    assert rc == 4 and not stream.value
    with pytest.raises(VitsError, match="STTS_FLAG_WATERMARK on a stream"):
        m.check(rc)
    assert m.synthesize(ids, SC, 2, None, pde, **kw)[0].shape[0] > 0


# ---- through Synth ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from vosk_tts_amd import Model, Synth
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.toymodel import PHONEMES, write_toy_model

    d = write_toy_model(str(tmp_path_factory.mktemp("vits") / "m"), W.default_hparams(n_vocab=len(PHONEMES)))
    model = Model(model_path=d, device=0)
    synth = Synth(model)
    synth.model_dir = d
    yield synth
    model.onnx.close()


def test_synth_audio_then_detect_watermark(lib, toy, launch_path):
    text = " ".join(["прив+ет м+ир др+уг"] * 10)

    def pinned(fn, *args, **kw):  # (every request draws the session's next seed: the calls compared here draw the same one)
        toy.model.onnx._seed = itertools.count(77)
        return fn(*args, **kw)

    plain = pinned(toy.synth_audio, text)
    marked = pinned(toy.synth_audio, text, watermark=KEY)
    assert marked.dtype == np.int16 and marked.shape == plain.shape and not np.array_equal(marked, plain)
    ref = R.detect(marked.astype(np.float64) / 32767.0, KEY)
    print(f"{marked.shape[0]} samples: the restatement scores z = {ref['z']:.2f} at offset {ref['offset']}")
    assert ref["z"] >= 8.0  # the text is long enough
    detected, z, offset = toy.detect_watermark(marked, KEY)
    assert detected and abs(z - ref["z"]) < 1e-3 and offset == ref["offset"]
    for audio, key in ((plain, KEY), (marked, KEY + 1)):  # the unflagged audio, and the wrong key
        detected, z, _ = toy.detect_watermark(audio, key)
        assert not detected and z < R.THRESHOLD - 2.0, (key, z)
    assert toy.detect_watermark(marked[:400], KEY) == (False, 0.0, 0)
    # True takes the config key; the session's feed key is the door on the plain request's audio
    toy.model.config.setdefault("inference", {})["watermark_key"] = KEY
    try:
        assert pinned(toy.synth_audio, text, watermark=True).tobytes() == marked.tobytes()
        assert toy.detect_watermark(marked)[0]
    finally:
        del toy.model.config["inference"]["watermark_key"]
    sess = toy.model.onnx
    feed = dict(toy._feed("прив+ет м+ир др+уг", 0, None, None, None, None)[0], **{"vits.seed": 5})
    plain_f = sess.run(None, feed)[0]
    got_f = sess.run(None, dict(feed, **{"vits.watermark_key": KEY, "vits.watermark_depth_db": 1.5}))[0]
    assert got_f.tobytes() == lib.op_watermark(plain_f.reshape(1, -1), [plain_f.shape[-1]], KEY, 1.5).tobytes()
    with pytest.raises(ValueError, match="FLAG_WATERMARK"):
        next(iter(toy.synth_stream(text, watermark=KEY)))


def test_multi_device_batch_takes_the_key(lib, toy, voice, tmp_path_factory):
    from vosk_tts_amd.batching import MultiDeviceSynth
    from vosk_tts_amd.toymodel import write_toy_multistream_model

    texts = [" ".join(["прив+ет м+ир др+уг"] * 6), "прив+ет, м+ир!"]
    ms = str(tmp_path_factory.mktemp("ms_batch"))
    write_toy_multistream_model(ms)
    for d, rates in ((toy.model_dir, (None,)), (ms, (None, 8000))):  # (the multistream family marks behind the session's resampler)
        mds = MultiDeviceSynth(d, devices=[0], max_batch=4)
        try:
            for rate in rates:
                kw = dict(speaker_ids=[2, 0], seeds=[101, 7], scale=1.0, sample_rate=rate)
                plain = mds.synth_batch(texts, **kw)
                marked = mds.synth_batch(texts, watermark=KEY, **kw)
                for a, b in zip(plain, marked):
                    assert b.dtype == np.int16 and b.shape == a.shape and (a.shape[0] < 513 or not np.array_equal(a, b))
                zp, zm = (toy.detect_watermark(x[0], KEY)[1] for x in (plain, marked))
                print(f"{os.path.basename(d)} at {rate or 'its own rate'}: {marked[0].shape[0]} samples, z {zp:.2f} plain, {zm:.2f} marked")
                assert zm > zp + 2.0
                if rate is None:  # (at 8000 Hz the toy vocoder's 11 s score 4.3: marked, but below the threshold; DESIGN.md "Watermark")
                    assert zm >= R.THRESHOLD + 2.0 and zp < R.THRESHOLD - 2.0
        finally:
            mds.close()
