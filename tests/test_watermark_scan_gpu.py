"""GPU tests of the watermark scan (include/vits_watermark_scan.h): the door against the float64 restatement
(tests/watermark_scan_ref.py), the segments made from the device's scores, the chunk seams of wm_scan_kernel, the whole way from
Synth.synth_audio to Synth.locate_watermark, and the refusals.

Bounds.  z_scan is allowed four times the distance of the restatement's own fp32 run from its float64 run on the same inputs, the rule
and the factor of z_all in tests/test_watermark_gpu.py; first_period and windows are compared as integers; what lies beyond W_o is
exactly 0.  The segments are decisions against the threshold: tests/test_watermark_scan.py asserts that no window of the spliced
signal or of its control lies within 1e-3 of it, three orders of magnitude more than that distance."""
import itertools

import numpy as np
import pytest

import watermark_ref as R
import watermark_scan_ref as S

pytestmark = pytest.mark.gpu
KEY = 0x5EED1234
PERIOD = 16384


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert hip_lib.has_watermark_scan
    return hip_lib


@pytest.fixture(scope="module")
def items():
    """the spliced signal (tests/test_watermark_scan.py), a 60000-sample piece of its marked part (windows at span 1 and 2, none at 4
    and 8), 600 samples (no frame with a complete row), and the unmarked control: computed once, never written to; with the Lb of both
    dtypes, which every case shares"""
    x = S.spliced_signal(KEY, 1.0)
    audio = [x, x[100000:160000], x[:600], S.spliced_signal(KEY, marked=False)]
    for a in audio:
        a.setflags(write=False)
    return audio, [R.band_logs(a) for a in audio], [R.band_logs(a, np.float32) for a in audio]


def _batch(audio, pad=0):
    lens = np.array([a.shape[0] for a in audio], np.int64)
    xs = np.full((len(audio), int(lens.max()) + pad), 1e30, np.float32)  # (beyond an item: never read)
    for b, a in enumerate(audio):
        xs[b, :lens[b]] = a
    return xs, lens


# ---- parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", (1, 2, 4, 8))
def test_scan_against_float64(lib, items, span):
    audio, lb64, lb32 = items
    xs, lens = _batch(audio[:3])
    assert lens.tolist() == [275625, 60000, 600]
    for pilots in (False, True):
        z, first, wins = lib.op_watermark_scan(xs, lens, KEY, span=span, pilots=pilots)
        assert z.dtype == np.float64 and z.shape[:2] == (3, 128) and first.shape == wins.shape == (3, 128) and np.isfinite(z).all()
        assert z.shape[2] == max(1, lib.watermark_scan_windows(275625, span)) == max(1, S.windows_of(275625, span))
        yard = dist = 0.0
        for b in range(3):
            z64, f64, w64 = S.scan_bands(lb64[b], KEY, span, pilots)
            z32, f32, w32 = S.scan_bands(lb32[b], KEY, span, pilots)
            assert np.array_equal(first[b], f64) and np.array_equal(wins[b], w64)
            W = z64.shape[1]
            yard = max(yard, np.abs(z32 - z64).max())
            dist = max(dist, np.abs(z[b, :, :W] - z64).max())
            assert not z[b, :, W:].any()
            for o in range(128):
                assert not z[b, o, wins[b, o]:].any()  # exactly 0 beyond W_o
        print(f"span {span} pilots {pilots}: device {dist:.3g}, float32 restatement {yard:.3g} from float64 (x{dist / yard:.2f})")
        assert yard > 0 and dist <= 4 * yard
        assert {1: (3, 0), 2: (2, 0), 4: (0, 0), 8: (0, 0)}[span] == (int(wins[1].max()), int(wins[2].max()))
        # the same call twice: the same bits
        again = lib.op_watermark_scan(xs, lens, KEY, span=span, pilots=pilots)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(again, (z, first, wins)))
    assert lib.op_watermark_scan(xs, lens, KEY, span=0)[0].tobytes() == lib.op_watermark_scan(xs, lens, KEY, span=4)[0].tobytes()  # 0 = the default


# ---- decisions --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", (4, 2))
def test_segments_from_the_device_scores(lib, items, span):
    from vosk_tts_amd.watermark_scan import segments

    audio, lb64, _ = items
    xs, lens = _batch([audio[0], audio[3]])
    z, first, wins = lib.op_watermark_scan(xs, lens, KEY, span=span)
    want = S.segments(*S.scan_bands(lb64[0], KEY, span), span, 275625)
    got = segments(z[0], first[0], wins[0], span, 275625)
    print(f"span {span}: {got}")
    assert len(want) == 1 and [(g.start, g.end, g.offset_samples) for g in got] == [(s.start, s.end, s.offset_samples) for s in want]
    assert abs(got[0].z - want[0].z) < 1e-4 and got[0].z >= S.threshold(wins[0].max()) + 1.0
    assert segments(z[1], first[1], wins[1], span, 275625) == [] and z[1].max() < 4.0  # the control


# ---- chunk seams ------------------------------------------------------------------------------------------------------------------------
def test_chunk_seams(lib, items):
    """wm_scan_kernel gives a workgroup 8 consecutive windows of one offset (WM_SCAN_CHUNK).  The item: the spliced signal twice in a
    row, 551250 samples = 33.6 periods, so 29 or 30 windows of span 4 at every offset: chunks 0 .. 7, 8 .. 15, 16 .. 23 and a ragged
    fourth, three seams.  The windows on both sides of every seam are checked against the restatement by index; the item alone, with
    another row length, and inside a batch gives the same bits."""
    audio = items[0]
    x = np.concatenate([audio[0], audio[0]])
    span = 4
    xs, lens = _batch([audio[1], x, audio[2]], pad=1000)
    z, first, wins = lib.op_watermark_scan(xs, lens, KEY, span=span)
    assert 24 < wins[1].min() <= wins[1].max() == z.shape[2] <= 32
    alone = lib.op_watermark_scan(x[None], [x.shape[0]], KEY, span=span)
    assert all(u[0].tobytes() == v[1].tobytes() for u, v in zip(alone, (z, first, wins)))
    lb64, lb32 = R.band_logs(x), R.band_logs(x, np.float32)
    seams = (7, 8, 15, 16, 23, 24)
    yard = dist = 0.0
    for o in (0, 1, 63, 118, 127):
        z64, p0, W = S.scan(lb64, KEY, o, span)
        z32 = S.scan(lb32, KEY, o, span)[0]
        assert (p0, W) == (first[1, o], wins[1, o]) and W > max(seams)
        yard = max(yard, np.abs(z32 - z64).max())
        dist = max(dist, np.abs(z[1, o, :W] - z64).max())
        for w in seams:
            assert abs(z[1, o, w] - z64[w]) <= 4 * np.abs(z32 - z64).max(), (o, w)
    print(f"seams: device {dist:.3g}, float32 restatement {yard:.3g} from float64 (x{dist / yard:.2f})")
    assert yard > 0 and dist <= 4 * yard
    # the signal repeats after 275625 samples, which is no multiple of 128: the second copy is found at another offset, as a second segment
    from vosk_tts_amd.watermark_scan import segments

    a, b = segments(z[1], first[1], wins[1], span, x.shape[0])
    assert a.end <= b.start and abs(a.offset_samples // 128 - 118) <= 1 and a.offset_samples != b.offset_samples


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
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


def test_synth_audio_then_locate_watermark(lib, toy):
    """Three toy-voice requests of about 12 s each, the middle one marked at the default 1 dB, joined on the host as a recording
    would hold them, located at the default span.  The restatement on this audio (258048 + 269568 + 288768 samples): the whole-item
    detector scores 6.07, the best window of four periods 13.35 against a threshold of 6.61, and no window lies within 0.019 of the
    threshold."""
    text = " ".join(["прив+ет м+ир др+уг"] * 3)
    toy.model.onnx._seed = itertools.count(77)
    a = toy.synth_audio(text)
    b = toy.synth_audio(text, watermark=KEY)
    c = toy.synth_audio(text)
    x = np.concatenate([a, b, c])
    lo, hi = a.shape[0], a.shape[0] + b.shape[0]
    assert x.dtype == np.int16
    span = 4
    segs = toy.locate_watermark(x, KEY, span=span)
    print(f"pieces of {a.shape[0]}, {b.shape[0]}, {c.shape[0]} samples; marked on [{lo}, {hi}); segments {segs}")
    assert len(segs) == 1
    (s,) = segs
    assert s.start < hi and s.end > lo  # it overlaps the middle piece
    assert s.start > lo - span * PERIOD and s.end < hi + span * PERIOD  # and neither neighbour by more than `span` periods
    assert s.z > toy.detect_watermark(x, KEY)[1] + 2.0  # the whole-item score dilutes on this audio
    assert s.offset_samples % 128 == 0 and abs((s.offset_samples - (-lo) % PERIOD + PERIOD // 2) % PERIOD - PERIOD // 2) <= 128
    assert toy.locate_watermark(x, KEY + 1, span=span) == [] and toy.locate_watermark(np.concatenate([a, c]), KEY, span=span) == []
    toy.model.config.setdefault("inference", {})["watermark_key"] = KEY  # key=None takes the config key
    try:
        assert toy.locate_watermark(x, span=span) == segs
    finally:
        del toy.model.config["inference"]["watermark_key"]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi_and_the_detector_goes_on(lib, items):
    import ctypes

    from vosk_tts_amd.capi import VitsError, _p, c_f32p, c_i32p, c_i64p

    audio = items[0]
    x = np.ascontiguousarray(audio[1][None])
    lens = np.array([60000], np.int64)
    z, p0, w = np.zeros((1, 128, 8)), np.zeros((1, 128), np.int32), np.zeros((1, 128), np.int32)

    def scan(span, flags, w_cap):
        return lib._fn("op_watermark_scan")(0, _p(x, c_f32p), _p(lens, c_i64p), 1, 60000, KEY, span, flags, w_cap,
                                            _p(z, ctypes.POINTER(ctypes.c_double)), _p(p0, c_i32p), _p(w, c_i32p))

    for args, match in (((9, 0, 8), "span 9"), ((-1, 0, 8), "span -1"), ((1, 0, 2), "w_cap 2 below the 3 windows"), ((1, 2, 8), "flags 0x2")):
        rc = scan(*args)
        assert rc == 1  # VITS_ERR_ARG
        with pytest.raises(VitsError, match=match):
            lib.check(rc)
    assert scan(1, 0, 8) == 0 and w.max() == 3 and not z[0, :, 3:].any() and z.max() > 6.0
    zd, off, rows, z_all = lib.op_watermark_detect(x, lens, KEY)  # a plain detect afterwards
    assert zd[0] >= R.THRESHOLD and rows[0] > 0
