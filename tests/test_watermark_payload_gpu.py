"""GPU tests of the watermark payload (include/vits_watermark_payload.h): the two doors against the float64 restatement
(tests/watermark_payload_ref.py), the flagged calls of both voice families against the embed door on the unflagged audio, that no
payload outlives its call, and the refusals.

Bounds.  The embed door, z_all and bit_z are allowed four times the distance of the restatement's own fp32 run from its float64 run,
the rule and the factor of tests/test_watermark_gpu.py.  offset, rows, payload and valid are compared as integers, on inputs whose two
conditions tests/test_watermark_payload.py asserts on the restatement: every |z_i| >= 1 and the best offset ahead of every other by
>= 1e-3, both orders of magnitude more than that distance."""
import ctypes
import itertools

import numpy as np
import pytest

import watermark_payload_ref as P
import watermark_ref as R

pytestmark = pytest.mark.gpu
KEY = 0x5EED1234
PAYLOADS = (0xBEEF, 0x1234, 0xA5A5)
SCALES = [0.667, 1.0, 0.8]
SC = np.array([0.8, 1.0, 0.8], np.float32)
SEED = 31
LUFS = -23.0


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert hip_lib.has_watermark_payload
    return hip_lib


@pytest.fixture(scope="module")
def signal():
    """the 4 s test signal: computed once, never written to"""
    x = R.voiced_signal(4.0)
    x.setflags(write=False)
    return x


# ---- the doors ----------------------------------------------------------------------------------------------------------------------
def test_embed_door_against_float64(lib, signal):
    from vosk_tts_amd.capi import VitsError

    lengths = np.array([600, 5000, 88200], np.int64)
    x = np.stack([signal, signal[::-1], signal]).astype(np.float32)
    for b, n in enumerate(lengths):
        x[b, n:] = 1e30  # never read
    worst = 0.0
    for depth in (1.0, 2.0):
        y = lib.op_watermark_payload(x, lengths, KEY, PAYLOADS, depth)
        assert y.shape == x.shape and y.dtype == np.float32
        for b, n in enumerate(lengths):
            n = int(n)
            ref64 = P.embed(x[b, :n], KEY, PAYLOADS[b], depth)
            ref32 = P.embed(x[b, :n], KEY, PAYLOADS[b], depth, dtype=np.float32)
            yard = np.abs(ref32.astype(np.float64) - ref64).max()
            dist = np.abs(y[b, :n].astype(np.float64) - ref64).max()
            worst = max(worst, dist / yard)
            print(f"depth {depth} dB len {n} payload {PAYLOADS[b]:#06x}: device {dist:.3g}, float32 restatement {yard:.3g} from float64 (x{dist / yard:.2f})")
            assert yard > 0 and dist <= 4 * yard, (depth, n, dist, yard)
            assert not y[b, n:].any()  # exactly zero from the length on
            tail = 256 * (n // 256)
            assert y[b, tail:n].tobytes() == x[b, tail:n].tobytes()
        assert y.tobytes() == lib.op_watermark_payload(x, lengths, KEY, PAYLOADS, depth).tobytes()  # the same bits twice
    print(f"embed door: worst ratio x{worst:.2f}")
    assert lib.op_watermark_payload(x, lengths, KEY, PAYLOADS, 0.0).tobytes() == y.tobytes()  # 0 = the payload default, 2 dB
    assert not np.array_equal(y[2], lib.op_watermark(x[2:], lengths[2:], KEY, 2.0)[0])  # a payload mark is not the plain mark
    assert not np.array_equal(y[2], lib.op_watermark_payload(x[2:], lengths[2:], KEY, [PAYLOADS[0]], 2.0)[0])  # nor another payload's
    short = x[:1, :400]
    assert lib.op_watermark_payload(short, [400], KEY, [7]).tobytes() == short.tobytes()  # below n/2 + 1 samples: as it went in
    with pytest.raises(VitsError, match="65536") as e:
        lib.op_watermark_payload(x, lengths, KEY, (1, 65536, 2))
    assert e.value.code == 1  # VITS_ERR_ARG
    with pytest.raises(VitsError, match="2.5"):
        lib.op_watermark_payload(x, lengths, KEY, PAYLOADS, 2.5)


def test_reader_against_float64(lib, signal):
    x = signal
    marked = [P.embed(x, KEY, p, 2.0).astype(np.float32) for p in PAYLOADS]
    plain = R.embed(x, KEY, 2.0).astype(np.float32)
    # (name, audio, the payload a valid read returns or None)
    items = [("marked", marked[0], PAYLOADS[0]), ("crop 5000", marked[1][5000:], PAYLOADS[1]), ("crop 12345", marked[2][12345:], PAYLOADS[2]),
             ("int16", np.round(marked[0] * 32767.0).astype(np.int16).astype(np.float32) / np.float32(32767.0), PAYLOADS[0]),
             ("x 1e-3", marked[1] * np.float32(1e-3), PAYLOADS[1]), ("600 samples", marked[0][:600], None), ("plain mark", plain, None),
             ("unmarked", x, None)]
    lens = np.array([a.shape[0] for _, a, _ in items], np.int64)
    xs = np.full((len(items), int(lens.max())), 1e30, np.float32)  # (beyond an item: never read)
    for b, (_, a, _) in enumerate(items):
        xs[b, :lens[b]] = a
    z, off, rows, payload, valid, z_all, bit_z = lib.op_watermark_read(xs, lens, KEY)
    assert z_all.shape == (len(items), 128) and bit_z.shape == (len(items), 24) and np.isfinite(z_all).all() and np.isfinite(bit_z).all()
    yard_z = dist_z = yard_b = dist_b = 0.0
    for b, (name, a, want) in enumerate(items):
        d64, d32 = P.read(a, KEY), P.read(a, KEY, dtype=np.float32)
        yard_z = max(yard_z, np.abs(d32["z_all"] - d64["z_all"]).max())
        dist_z = max(dist_z, np.abs(z_all[b] - d64["z_all"]).max())
        print(f"{name}: z {z[b]:.4f} (float64 {d64['z']:.4f}) offset {off[b]} rows {rows[b]} payload {int(payload[b]):#06x} valid {valid[b]} "
              f"min |z_i| {np.abs(bit_z[b]).min():.3f}")
        if want is not None or name == "plain mark":  # (the inputs whose margins the CPU test asserts; the others have no best offset to speak of)
            assert (int(off[b]), int(rows[b]), int(payload[b]), int(valid[b])) == (d64["offset"], d64["rows"], d64["payload"], int(d64["valid"])), name
            if d32["offset"] == d64["offset"]:  # (bit_z is of the best offset: a yardstick only where the fp32 run chose the same one)
                yard_b = max(yard_b, np.abs(d32["bit_z"] - d64["bit_z"]).max())
            dist_b = max(dist_b, np.abs(bit_z[b] - d64["bit_z"]).max())
        assert z[b] == z_all[b].max() and int(rows[b]) == d64["rows_all"][int(off[b]) // 128]
        assert (bool(valid[b]), int(payload[b]) if valid[b] else None) == (want is not None, want), name
    print(f"z_all: device {dist_z:.3g}, float32 restatement {yard_z:.3g} from float64 (x{dist_z / yard_z:.2f})")
    print(f"bit_z: device {dist_b:.3g}, float32 restatement {yard_b:.3g} from float64 (x{dist_b / yard_b:.2f})")
    assert yard_z > 0 and dist_z <= 4 * yard_z
    assert yard_b > 0 and dist_b <= 4 * yard_b
    names = [n for n, _, _ in items]
    b600, bplain, bun = names.index("600 samples"), names.index("plain mark"), names.index("unmarked")
    assert (z[b600], off[b600], rows[b600], valid[b600]) == (0.0, 0, 0, 0) and not z_all[b600].any()
    assert z[bplain] >= R.THRESHOLD and payload[bplain] == 0 and not valid[bplain]  # detected, word 0x000000: not a codeword
    assert z[bun] < 4.0 and not valid[bun]
    assert lib.op_watermark_read(xs[:1], lens[:1], KEY + 1)[0][0] < 4.0  # the wrong key
    # the same call twice, and an item alone: the same bits
    again = lib.op_watermark_read(xs, lens, KEY)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(again, (z, off, rows, payload, valid, z_all, bit_z)))
    alone = lib.op_watermark_read(items[1][1][None], [lens[1]], KEY)
    assert all(u[0].tobytes() == v[1].tobytes() for u, v in zip(alone, again))
    # the plain detector is untouched by the reader's templates: it still scores all 1504 chips of a plain mark
    zd = lib.op_watermark_detect(plain[None], [plain.shape[0]], KEY)[0][0]
    assert zd > z[bplain]


# ---- VITS entry points: the flagged call is the door on the unflagged audio ----------------------------------------------------------
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
def test_flagged_synthesize_is_the_payload_door_on_the_unflagged_audio(lib, hip_tiny, launch_path, B, fast):
    from vosk_tts_amd.capi import LOUDNESS_LUFS

    ids, lens, sid = _feed(B)
    native = hip_tiny.hp.sampling_rate
    path = _Path(lib, fast)
    kw = dict(seed=SEED, solo=True)
    pl = list(PAYLOADS[:B])
    plain, ol, ends = path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, marks=True, **kw)
    assert ol.max() >= 513
    want = lib.op_watermark_payload(plain, ol, KEY, pl)  # the same kernels on the same samples, at the payload default of 2 dB
    got, gl, ge = path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, marks=True, watermark=KEY, watermark_payload=pl, **kw)
    assert got.shape == plain.shape and np.array_equal(gl, ol) and np.array_equal(ge, ends)
    assert got.tobytes() == want.tobytes() and not np.array_equal(got, plain)
    assert got.tobytes() != path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, watermark=KEY, watermark_depth_db=2.0, **kw)[0].tobytes()
    # one value for the call: every item carries it; and another depth
    one = path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, watermark=KEY, watermark_payload=0x0F0F, watermark_depth_db=1.0, **kw)[0]
    assert one.tobytes() == lib.op_watermark_payload(plain, ol, KEY, [0x0F0F] * B, 1.0).tobytes()
    # another rate: marked at the rate it is returned at
    p8, ol8 = path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, sample_rate=8000, **kw)
    g8, gl8 = path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, sample_rate=8000, watermark=KEY, watermark_payload=pl, **kw)
    want8 = lib.op_watermark_payload(p8, ol8, KEY, pl)
    assert np.array_equal(gl8, ol8) and g8.tobytes() == want8.tobytes()
    # a loudness target: the gain is measured on, and applied to, the marked audio
    gn, _ = path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, watermark=KEY, watermark_payload=pl, loudness=(LOUDNESS_LUFS, LUFS, 0.0), **kw)
    assert gn.tobytes() == lib.op_loudness_normalize(want, ol, native, LOUDNESS_LUFS, LUFS, 0.0)[0].tobytes()
    # int16: the conversion of the marked float audio with the call's scale, at both rates
    scale = float(1.25 / np.abs(want).max())
    pcm, ql = path.call(hip_tiny.synthesize_pcm16, ids, lens, SCALES, sid, pcm_scale=scale, watermark=KEY, watermark_payload=pl, **kw)
    assert np.array_equal(ql, ol) and np.array_equal(pcm, _pcm16(want, scale))
    pcm8, _ = path.call(hip_tiny.synthesize_pcm16, ids, lens, SCALES, sid, pcm_scale=scale, sample_rate=8000, watermark=KEY, watermark_payload=pl, **kw)
    assert np.array_equal(pcm8, _pcm16(want8, scale))
    # the plain mark and the unflagged call afterwards: the bytes of their doors and of before
    assert path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, watermark=KEY, **kw)[0].tobytes() == lib.op_watermark(plain, ol, KEY).tobytes()
    assert path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, **kw)[0].tobytes() == plain.tobytes()


@pytest.mark.parametrize("fast", (True, False), ids=("fast", "eager"))
def test_flagged_document_takes_the_scalar(lib, hip_tiny, fast):
    ids, lens, sid = _feed(3)
    path = _Path(lib, fast)
    kw = dict(seed=SEED, lead_frames=2, gap_frames=[3, 0, 2], fade_samples=9)
    for rate in (None, 8000):
        plain, info = path.call(hip_tiny.synthesize_document, ids, lens, SCALES, sid, sample_rate=rate, **kw)
        got, gi = path.call(hip_tiny.synthesize_document, ids, lens, SCALES, sid, sample_rate=rate, watermark=KEY, watermark_payload=0xBEEF, **kw)
        assert got.shape == plain.shape and np.array_equal(gi["seg_end"], info["seg_end"])
        assert got.tobytes() == lib.op_watermark_payload(plain[None], [plain.shape[0]], KEY, [0xBEEF])[0].tobytes(), rate  # the one item it has become
    with pytest.raises(ValueError, match="one value"):
        hip_tiny.synthesize_document(ids, lens, SCALES, sid, watermark=KEY, watermark_payload=[1, 2, 3], **kw)


# ---- no payload outlives its call, and the read returns it ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from vosk_tts_amd import Model, Synth
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.toymodel import PHONEMES, write_toy_model

    d = write_toy_model(str(tmp_path_factory.mktemp("vits") / "m"), W.default_hparams(n_vocab=len(PHONEMES)))
    model = Model(model_path=d, device=0)
    synth = Synth(model)
    yield synth
    model.onnx.close()


def test_two_calls_of_one_bucket_carry_their_own_payloads(lib, toy, launch_path):
    """Two consecutive B = 1 calls of the same bucket with payloads 0x1234 and 0xBEEF: each equals its own door output, and each reads
    back its own payload from about 3 s of toy-voice audio at 2 dB.  The read is compared with the restatement where the restatement's
    own two conditions hold on this audio (they are asserted: printed first)."""
    sess = toy.model.onnx
    text = "прив+ет м+ир др+уг"
    feed = dict(toy._feed(text, 0, None, None, None, None)[0], **{"vits.seed": 5})
    plain = sess.run(None, feed)[0].reshape(1, -1)
    n = plain.shape[1]
    print(f"{n} samples, {n / toy.native_rate():.2f} s")
    for p in (0x1234, 0xBEEF):
        got = sess.run(None, dict(feed, **{"vits.watermark_key": KEY, "vits.watermark_payload": p}))[0].reshape(1, -1)
        assert got.tobytes() == lib.op_watermark_payload(plain, [n], KEY, [p]).tobytes(), hex(p)
        d = P.read(got[0], KEY)
        za = d["z_all"].copy()
        za[d["offset"] // 128] = -np.inf
        print(f"payload {p:#06x}: the restatement reads {d['payload']:#06x} valid {d['valid']} z {d['z']:.2f}, min |z_i| {np.abs(d['bit_z']).min():.2f}, "
              f"lead {d['z'] - za.max():.4f}")
        assert np.abs(d["bit_z"]).min() >= 1.0 and d["z"] - za.max() >= 1e-3 and d["valid"] and d["payload"] == p
        z, off, rows, payload, valid, _, _ = lib.op_watermark_read(got, [n], KEY)
        assert (int(payload[0]), int(valid[0]), int(off[0]), int(rows[0])) == (p, 1, d["offset"], d["rows"])
        detected, zs, offset, pay, bit_z = toy.read_watermark(got[0], KEY)
        assert detected and pay == p and offset == d["offset"] and bit_z.shape == (24,)
    # through Synth, as int16: the payload of the request, then none for the plain mark and for the unmarked audio
    toy.model.onnx._seed = itertools.count(77)
    pcm = toy.synth_audio(text, watermark=KEY, watermark_payload=0xA5A5)
    assert pcm.dtype == np.int16 and toy.read_watermark(pcm, KEY)[3] == 0xA5A5
    toy.model.onnx._seed = itertools.count(77)
    detected, _, _, pay, _ = toy.read_watermark(toy.synth_audio(text, watermark=KEY, watermark_depth_db=2.0), KEY)
    assert detected and pay is None
    toy.model.onnx._seed = itertools.count(77)
    assert toy.read_watermark(toy.synth_audio(text), KEY)[::3] == (False, None)
    with pytest.raises(ValueError, match="VITS_FLAG_WATERMARK_PAYLOAD"):
        next(iter(toy.synth_stream(text, watermark=KEY, watermark_payload=1)))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name(lib, hip_tiny, launch_path):
    from vosk_tts_amd.capi import FLAG_WATERMARK, FLAG_WATERMARK_PAYLOAD, SynthWatermarkPayloadOpts, VitsError, _p, c_f32p, c_i64p

    ids = np.random.default_rng(63).integers(1, 20, size=(1, 12)).astype(np.int64)
    sc = np.array(SCALES, np.float32)
    with pytest.raises(ValueError, match="65536"):
        hip_tiny.synthesize(ids, [12], SCALES, [1], seed=2, watermark=KEY, watermark_payload=65536)
    with pytest.raises(ValueError, match="needs watermark"):
        hip_tiny.synthesize(ids, [12], SCALES, [1], seed=2, watermark_payload=5)
    with pytest.raises(VitsError, match="FLAG_WATERMARK_PAYLOAD") as e:
        hip_tiny.stream(ids, SCALES, 1, chunk_frames=8, seed=2, watermark=KEY, watermark_payload=5)
    assert e.value.code == 4

    def synthesize(o):  # the C ABI itself
        out, ns, ol = c_f32p(), ctypes.c_int64(), np.zeros(1, np.int64)
        return lib._fn("synthesize")(hip_tiny._h, _p(ids, c_i64p), _p(np.array([12], np.int64), c_i64p), 1, 12, _p(sc, c_f32p),
                                     _p(np.array([1], np.int64), c_i64p), ctypes.byref(o), ctypes.byref(out), ctypes.byref(ns), _p(ol, c_i64p))

    o = SynthWatermarkPayloadOpts()
    o.flags, o.watermark_key, o.watermark_payload = FLAG_WATERMARK_PAYLOAD, KEY, 5  # the payload flag alone
    with pytest.raises(VitsError, match="VITS_FLAG_WATERMARK_PAYLOAD without VITS_FLAG_WATERMARK") as e:
        lib.check(synthesize(o))
    assert e.value.code == 1  # VITS_ERR_ARG
    o.flags, o.watermark_payload = FLAG_WATERMARK | FLAG_WATERMARK_PAYLOAD, 65536
    with pytest.raises(VitsError, match="payload 65536") as e:
        lib.check(synthesize(o))
    assert e.value.code == 1
    bad = np.array([70000], np.uint32)
    o.watermark_payload, o.watermark_payloads = 5, bad.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    with pytest.raises(VitsError, match="payload 70000 of item 0"):
        lib.check(synthesize(o))
    o.watermark_payloads = None
    stream, total = ctypes.c_void_p(), ctypes.c_int64()
    for name, extra in (("stream_open", ()), ("stream_open_rate", (8000,))):  # both stream opens
        rc = lib._fn(name)(hip_tiny._h, _p(ids, c_i64p), 12, _p(sc, c_f32p), 1, ctypes.byref(o), 8, *extra, ctypes.byref(stream), ctypes.byref(total))
        assert rc == 4 and not stream.value
        with pytest.raises(VitsError, match="VITS_FLAG_WATERMARK_PAYLOAD on a stream"):
            lib.check(rc)
    audio, ol = hip_tiny.synthesize(ids, [12], SCALES, [1], seed=2)  # a plain request afterwards
    assert ol[0] > 0 and np.isfinite(audio).all()


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


def test_stts_flag_is_the_payload_door_on_the_unflagged_audio(lib, voice):
    from vosk_tts_amd.capi import VitsError, _p, c_f32p, c_i64p
    from vosk_tts_amd.capi_stts import STTS_FLAG_WATERMARK, STTS_FLAG_WATERMARK_PAYLOAD, SttsWatermarkPayloadOpts

    sess = voice.onnx
    m = sess._model
    T = 14
    ids = np.random.default_rng(3).integers(1, 40, size=(5, T)).astype(np.int64)
    pde = np.full(T, 3.0, np.float32)
    kw = dict(seed=9, n_timesteps=2, want_mel=False)
    plain, _, ends = m.synthesize(ids, SC, 2, None, pde, marks=True, **kw)
    n = plain.shape[0]
    assert n >= 513
    got, _, ge = m.synthesize(ids, SC, 2, None, pde, marks=True, watermark=KEY, watermark_payload=0xBEEF, **kw)
    assert got.tobytes() == lib.op_watermark_payload(plain[None], [n], KEY, [0xBEEF])[0].tobytes() and np.array_equal(ge, ends)
    p8, _, _ = m.synthesize(ids, SC, 2, None, pde, marks=True, sample_rate=8000, **kw)
    g8, _, _ = m.synthesize(ids, SC, 2, None, pde, marks=True, sample_rate=8000, watermark=KEY, watermark_payload=0xBEEF, **kw)
    assert g8.tobytes() == lib.op_watermark_payload(p8[None], [p8.shape[0]], KEY, [0xBEEF])[0].tobytes()
    # the batch call: every item its own payload, from its own length; one value for the batch; a document takes the scalar
    B = 3
    bids = np.random.default_rng(4).integers(1, 40, size=(B, 5, T)).astype(np.int64)
    blens = np.array([T, T - 5, 6], np.int64)
    bpde = np.full((B, T), 3.0, np.float32)
    bkw = dict(seed=9, n_timesteps=2)
    bp, bl = m.synthesize_batch(bids, blens, SC, [0, 1, 2], None, bpde, **bkw)
    bg, bgl = m.synthesize_batch(bids, blens, SC, [0, 1, 2], None, bpde, watermark=KEY, watermark_payload=list(PAYLOADS), **bkw)
    assert np.array_equal(bgl, bl) and bg.tobytes() == lib.op_watermark_payload(bp, bl, KEY, PAYLOADS).tobytes()
    b1, _ = m.synthesize_batch(bids, blens, SC, [0, 1, 2], None, bpde, watermark=KEY, watermark_payload=7, watermark_depth_db=1.0, **bkw)
    assert b1.tobytes() == lib.op_watermark_payload(bp, bl, KEY, [7, 7, 7], 1.0).tobytes()
    dp, _ = m.synthesize_document(bids, blens, SC, [0, 1, 2], None, bpde, gap_frames=[2, 0, 1], **bkw)
    dg, _ = m.synthesize_document(bids, blens, SC, [0, 1, 2], None, bpde, gap_frames=[2, 0, 1], watermark=KEY, watermark_payload=0x1234, **bkw)
    assert dg.tobytes() == lib.op_watermark_payload(dp[None], [dp.shape[0]], KEY, [0x1234])[0].tobytes()
    # the session's feed keys, at the native rate (inside the library) and at another (behind the session's resampler)
    feed = {"input": ids[None], "input_lengths": np.array([T], np.int64), "scales": SC, "sid": np.array([2], np.int64),
            "phone_duration_extra": pde[None], "vits.seed": 9, "vits.n_timesteps": 2}
    for rate in (None, 8000):
        f = dict(feed, **({"vits.sample_rate": rate} if rate else {}))
        p = sess.run(None, f)[0]
        g = sess.run(None, dict(f, **{"vits.watermark_key": KEY, "vits.watermark_payload": 0xA5A5}))[0]
        assert g.tobytes() == lib.op_watermark_payload(p, [p.shape[1]], KEY, [0xA5A5]).tobytes(), rate
    with pytest.raises(ValueError, match="STTS_FLAG_WATERMARK_PAYLOAD"):
        next(iter(sess.run_stream(None, dict(feed, **{"vits.watermark_key": KEY, "vits.watermark_payload": 1}))))
    # the C ABI: the flag alone, and the stream open, refuse by name; then a plain call
    o = SttsWatermarkPayloadOpts()
    o.flags, o.watermark_key, o.watermark_payload = STTS_FLAG_WATERMARK | STTS_FLAG_WATERMARK_PAYLOAD, KEY, 3
    stream, total = ctypes.c_void_p(), ctypes.c_int64()
    rc = m._fn("stream_open")(m._h, _p(ids, c_i64p), T, _p(SC, c_f32p), 2, None, _p(pde, c_f32p), ctypes.byref(o), 8, ctypes.byref(stream), ctypes.byref(total))
    assert rc == 4 and not stream.value
    with pytest.raises(VitsError, match="STTS_FLAG_WATERMARK_PAYLOAD on a stream"):
        m.check(rc)
    o.flags = STTS_FLAG_WATERMARK_PAYLOAD
    au, ns = c_f32p(), ctypes.c_int64()
    rc = m._fn("synthesize")(m._h, _p(ids, c_i64p), T, _p(SC, c_f32p), 2, None, _p(pde, c_f32p), ctypes.byref(o), ctypes.byref(au), ctypes.byref(ns), None, None)
    assert rc == 1
    with pytest.raises(VitsError, match="STTS_FLAG_WATERMARK_PAYLOAD without STTS_FLAG_WATERMARK"):
        m.check(rc)
    assert m.synthesize(ids, SC, 2, None, pde, **kw)[0].shape[0] > 0
