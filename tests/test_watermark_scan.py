"""Watermark localisation on the CPU (include/vits_watermark_scan.h): the conditions the float64 restatement
(tests/watermark_scan_ref.py) has to meet on the spliced test signal -- which are also the decision margins of
tests/test_watermark_scan_gpu.py -- the restatement against the detector's own G, vosk_tts_amd/watermark_scan.py against the
restatement and on hand-made score arrays, the refusals of the C ABI (host-side: they need no device), and Synth.locate_watermark
and the command line against stubs.  The device is checked in tests/test_watermark_scan_gpu.py.

The spliced signal: voiced_signal(4 s, seed 3), 4.5 s of the marked 6 s signal of seed 7 cut from sample 5000, voiced_signal(4 s,
seed 11): 275625 samples, marked on [88200, 187425); the crop predicts offset index (5000 - 88200) mod 16384 / 128 = 118.  Figures of
the float64 restatement (printed by the tests): the whole-item detector scores 7.59 at 1 dB and 16.05 at 2 dB, the best window of four
periods 13.61 and 23.61; the unmarked control's window maxima are 3.14 (span 2) and 1.99 (span 4) against thresholds of 6.44 and 6.41."""
import inspect
import json
import wave

import numpy as np
import pytest

import watermark_payload_ref as P
import watermark_ref as R
import watermark_scan_ref as S

KEY = 0x5EED1234
PERIOD = 16384
LO, HI = S.SPLICE_MARKED


@pytest.fixture(scope="module")
def spliced():
    """{depth: signal} and the control at None: computed once, never written to"""
    out = {1.0: S.spliced_signal(KEY, 1.0), 2.0: S.spliced_signal(KEY, 2.0), None: S.spliced_signal(KEY, marked=False)}
    for a in out.values():
        assert a.shape == (275625,) and a.dtype == np.float32
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def scans(spliced):
    """{(depth, span): (z_scan, first_period, windows)} of the restatement"""
    return {(d, s): S.scan_all(spliced[d], KEY, s) for d in (1.0, 2.0, None) for s in (2, 4)}


# ---- the point of the feature ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", (4, 2))
@pytest.mark.parametrize("depth", (1.0, 2.0))
def test_one_segment_where_the_mark_is(spliced, scans, depth, span):
    z, first, wins = scans[depth, span]
    n = spliced[depth].shape[0]
    segs = S.segments(z, first, wins, span, n)
    t = S.threshold(wins.max())
    print(f"{depth} dB span {span}: Wmax {wins.max()} t {t:.3f} best {z.max():.2f} segments {segs}; smallest margin {np.abs(z - t).min():.4f}")
    assert len(segs) == 1
    seg = segs[0]
    assert abs(seg.offset_samples // 128 - 118) <= 1 and seg.offset_samples % 128 == 0
    assert LO - span * PERIOD < seg.start < LO + PERIOD
    assert HI - PERIOD < seg.end < HI + span * PERIOD
    assert seg.z == z.max() >= t
    # the whole-item detector dilutes on this audio: it stays below the best window
    whole = R.detect(spliced[depth], KEY)["z"]
    print(f"  the detector on the whole item: {whole:.2f}")
    assert whole < seg.z
    # the margins of the GPU test's decisions: no window within 1e-3 of the threshold (the fp32 distance is of order 1e-6)
    assert np.abs(z - t).min() >= 1e-3
    # the product's grouping is the restatement's
    from vosk_tts_amd import watermark_scan as W

    got = W.segments(z, first, wins, span, n)
    assert [(g.start, g.end, g.z, g.offset_samples) for g in got] == [tuple(s) for s in segs]


@pytest.mark.parametrize("span", (4, 2))
def test_the_unmarked_control_has_no_segment(spliced, scans, span):
    from vosk_tts_amd import watermark_scan as W

    z, first, wins = scans[None, span]
    print(f"control span {span}: window maximum {z.max():.2f} against {S.threshold(wins.max()):.3f}")
    assert z.max() < 4.0
    assert S.segments(z, first, wins, span, spliced[None].shape[0]) == [] == W.segments(z, first, wins, span, spliced[None].shape[0])


# ---- the restatement against the detector it extends ---------------------------------------------------------------------------------
def test_scan_over_every_period_is_the_detectors_G_on_complete_periods(spliced):
    x = spliced[1.0][:120000]
    Lb = R.band_logs(x)
    F = Lb.shape[0]
    for o in (0, 1, 64, 117, 127):
        Gp, p0 = S.periods(Lb, o)
        n = Gp.shape[0]
        assert 1 <= n <= S.MAX_SPAN
        G = S.window_sums(Gp, n)
        assert G.shape == (1, R.ROWS, R.GROUPS)
        # score()'s own loop (tests/watermark_ref.py), over the rows of the complete periods only
        g0 = o & 1
        pbase = (o + g0) // 2
        nf = (F - g0 + 1) // 2
        r0, r1 = (pbase + 3) // 4, (pbase + nf) // 4 - 1
        assert r0 <= R.ROWS * p0 and R.ROWS * (p0 + n) - 1 <= r1 and R.ROWS * (p0 - 1) < r0 and r1 < R.ROWS * (p0 + n + 1) - 1
        want = np.zeros((R.ROWS, R.GROUPS - 2))
        for rho in range(R.ROWS * p0, R.ROWS * (p0 + n)):
            gf = g0 + 2 * (4 * rho - pbase)
            T = (((Lb[gf] + Lb[gf + 2]) + Lb[gf + 4]) + Lb[gf + 6]) * 0.25
            want[rho & (R.ROWS - 1)] += T[1:-1] - 0.5 * (T[:-2] + T[2:])
        assert np.array_equal(G[0][:, 1:-1], want) and not G[0][:, 0].any() and not G[0][:, -1].any()
        z, zp0, W = S.scan(Lb, KEY, o, n)
        assert (zp0, W) == (p0, 1)
        assert abs(z[0] - float(np.sum(R.chips(KEY)[:, 1:-1] * want)) / np.sqrt(float(np.sum(want * want)))) < 1e-12  # (numpy's sum order)
        # a window is the written sum of its own periods: the scores at span 2 do not depend on what lies in front of the window
        if n >= 3:
            z2 = S.scan(Lb, KEY, o, 2)[0]
            G1 = Gp[1] + Gp[2]
            sel = np.s_[:, 1:-1]
            assert abs(z2[1] - float(np.sum((R.chips(KEY) * G1)[sel])) / np.sqrt(float(np.sum(G1[sel] ** 2)))) < 1e-12


def test_pilots_score_the_odd_positions_only(spliced):
    Lb = R.band_logs(spliced[2.0][80000:200000])
    Gp, _ = S.periods(Lb, 0)
    G = S.window_sums(Gp, 2)[1]
    sel = P.pilots().copy()
    sel[:, 0] = sel[:, -1] = False
    assert sel.sum() == 752  # include/vits_watermark_payload.h: the scored pilot chips
    want = float(np.sum((R.chips(KEY) * G)[sel])) / np.sqrt(float(np.sum(G[sel] ** 2)))
    assert S.scan(Lb, KEY, 0, 2, pilots=True)[0][1] == want != S.scan(Lb, KEY, 0, 2)[0][1]


def test_threshold_and_ranges():
    from vosk_tts_amd import watermark_scan as W

    for mod in (S, W):
        assert mod.threshold(1) == 6.0 == mod.threshold(0) == R.THRESHOLD
        for wmax in (2, 13, 80, 5000):
            t = mod.threshold(wmax)
            assert abs(128 * wmax * np.exp(-t * t / 2) - 128 * np.exp(-18.0)) < 1e-18  # the detector's bound, spread over the windows
        assert mod.threshold(13) == S.threshold(13) and 6.41 < mod.threshold(13) < 6.42
        # pattern frame p is centred on sample 256 p - 128 o: window (o, w) starts 16384 (p0 + w) - 128 o samples into the audio
        assert mod.window_range(0, 0, 0, 4, 10 ** 6) == (0, 65536)
        assert mod.window_range(118, 1, 7, 4, 275625) == (8 * PERIOD - 118 * 128, 12 * PERIOD - 118 * 128)
        assert mod.window_range(127, 0, 0, 1, 10 ** 6) == (0, PERIOD - 127 * 128)  # clipped at the front
        assert mod.window_range(3, 1, 14, 2, 275625) == (15 * PERIOD - 384, 275625)  # and at the end
    for bad in (-1, 9, 1.5, True, "4"):
        with pytest.raises(ValueError, match="span"):
            W.span_arg(bad)
        with pytest.raises(ValueError, match="span"):
            S.span_arg(bad)
    assert W.span_arg(0) == W.span_arg(None) == S.span_arg(0) == 4 and W.span_arg(8) == 8


def test_window_counts_against_the_library(hip_lib):
    """vits_watermark_scan_windows is host arithmetic: it is compared here, without a device, with the restatement's count"""
    assert hip_lib.has_watermark_scan
    for n in (0, 512, 513, 600, 16383, 16384 + 512, 32768, 60000, 275625, 22050 * 60):
        for span in (0, 1, 2, 4, 8):
            assert hip_lib.watermark_scan_windows(n, span) == S.windows_of(n, span), (n, span)
    assert S.windows_of(275625, 4) == 13 and S.windows_of(60000, 1) == 3 and S.windows_of(60000, 2) == 2
    assert S.windows_of(60000, 4) == 0 == S.windows_of(60000, 8) and S.windows_of(600, 1) == 0


def test_refusals_name_their_values(hip_lib):
    from vosk_tts_amd.capi import VitsError

    x = np.zeros((1, 60000), np.float32)
    for bad, match in ((9, "span 9"), (-1, "span -1")):
        with pytest.raises(VitsError, match=match) as e:
            hip_lib.op_watermark_scan(x, [60000], KEY, span=bad, w_cap=8)
        assert e.value.code == 1  # VITS_ERR_ARG
        with pytest.raises(VitsError, match=match):
            hip_lib.watermark_scan_windows(60000, bad)
    with pytest.raises(VitsError, match="w_cap 2 below the 3 windows") as e:
        hip_lib.op_watermark_scan(x, [60000], KEY, span=1, w_cap=2)
    assert e.value.code == 1
    with pytest.raises(VitsError, match="60001"):
        hip_lib.op_watermark_scan(x, [60001], KEY, span=1, w_cap=8)
    assert len(hip_lib._fn("op_watermark_scan").argtypes) == 12


# ---- segments on hand-made scores -------------------------------------------------------------------------------------------------------
def _blank(W=20):
    return np.zeros((128, W)), np.zeros(128, np.int32), np.full(128, W, np.int32)


@pytest.mark.parametrize("mod", ("restatement", "product"))
def test_segments_on_hand_made_scores(mod):
    from vosk_tts_amd import watermark_scan as Wm

    seg = S.segments if mod == "restatement" else Wm.segments
    n = 24 * PERIOD
    t = S.threshold(20)
    # nothing over the threshold, and a score just below it
    z, first, wins = _blank()
    z[5, 3] = t - 1e-9
    assert seg(z, first, wins, 2, n) == []
    # two separated runs at different offsets: two segments, sorted by start, each with its best window's score
    z, first, wins = _blank()
    z[10, 2:5] = (7.0, 9.0, 8.0)
    z[40, 12:14] = (11.0, 7.5)
    a, b = seg(z, first, wins, 2, n)
    assert (a.start, a.end, a.z, a.offset_samples) == (2 * PERIOD - 1280, 6 * PERIOD - 1280, 9.0, 1280)
    assert (b.start, b.end, b.z, b.offset_samples) == (12 * PERIOD - 5120, 15 * PERIOD - 5120, 11.0, 5120)
    # a window beyond windows[o] is not a candidate, whatever its score
    wins[40] = 12
    assert len(seg(z, first, wins, 2, n)) == 1
    # one run seen at two neighbouring offsets, whose first periods differ: one segment, the union of both
    z, first, wins = _blank()
    first[:64] = 1  # (as in a real scan: the low offsets start one period later)
    z[63, 3:6] = (8.0, 10.0, 8.5)     # periods 4 .. 6
    z[64, 4:8] = (7.0, 9.5, 8.0, 7.2)  # periods 4 .. 7
    (one,) = seg(z, first, wins, 1, n)
    assert (one.start, one.end, one.z, one.offset_samples) == (4 * PERIOD - 64 * 128, 8 * PERIOD - 64 * 128, 10.0, 63 * 128)
    # the same run at an offset further away is not grown into, but it overlaps the segment and is dropped: still one
    z[70, 5] = 7.7
    assert len(seg(z, first, wins, 1, n)) == 1
    # a hole in the run ends the growth; what lies behind the hole does not overlap and is its own segment
    z, first, wins = _blank()
    z[0, 1:3] = 9.0
    z[0, 4] = 8.0
    a, b = seg(z, first, wins, 1, n)
    assert (a.start, a.end, b.start, b.end) == (PERIOD, 3 * PERIOD, 4 * PERIOD, 5 * PERIOD)


# ---- two joined items, each with its own payload -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def joined():
    a = P.embed(R.voiced_signal(6.0, seed=7), KEY, 0xBEEF, 2.0).astype(np.float32)
    b = P.embed(R.voiced_signal(6.0, seed=11), KEY, 0x1234, 2.0).astype(np.float32)
    x = np.concatenate([a, b])
    x.setflags(write=False)
    return x, a.shape[0]


@pytest.mark.parametrize("span", (4, 2))
def test_two_joined_items_read_their_own_payloads(joined, span):
    x, cut = joined
    z, first, wins = S.scan_all(x, KEY, span, pilots=True)
    segs = S.segments(z, first, wins, span, x.shape[0])
    print(f"span {span}: {segs}")
    assert len(segs) == 2
    a, b = segs
    assert a.start == 0 and cut - PERIOD < a.end < cut + span * PERIOD and a.end <= b.start < cut + span * PERIOD and b.end > x.shape[0] - PERIOD
    assert a.offset_samples == 0 and abs(b.offset_samples - (-cut) % PERIOD) <= 128
    for seg, want in ((a, 0xBEEF), (b, 0x1234)):
        d = P.read(x[seg.start:seg.end], KEY)
        print(f"  [{seg.start}, {seg.end}): payload {d['payload']:#06x} valid {d['valid']} min |z_i| {np.abs(d['bit_z']).min():.2f}")
        assert d["valid"] and d["payload"] == want


# ---- Synth.locate_watermark and the command line against stubs ---------------------------------------------------------------------------
class _LibStub:
    """stands where the session's library does: the restatement behind the two doors locate_watermark calls, and a record of the calls"""

    has_watermark_scan = has_watermark_payload = True

    def __init__(self):
        self.calls = []

    def op_watermark_scan(self, x, lengths, key, span=0, pilots=False, device=0):
        assert x.dtype == np.float32 and x.ndim == 2 and list(lengths) == [x.shape[1]]
        self.calls.append(("scan", x.shape[1], key, span, pilots, device))
        z, first, wins = S.scan_all(x[0], key, span, pilots)
        return z[None], first[None], wins[None]

    def op_watermark_read(self, x, lengths, key, device=0):
        self.calls.append(("read", x.shape[1], key, device))
        d = P.read(x[0], key)
        return (np.array([d["z"]]), np.array([d["offset"]], np.int32), np.array([d["rows"]], np.int32), np.array([d["payload"]], np.uint32),
                np.array([int(d["valid"])], np.int32), d["z_all"][None], d["bit_z"][None])


def _synth(config, lib):
    from vosk_tts_amd.synth import Synth

    s = Synth.__new__(Synth)
    s.model = type("M", (), {})()
    s.model.config = config
    s.model.onnx = type("Sess", (), {"_lib": lib, "_model": type("Mod", (), {"device": 3})()})()
    return s


def test_locate_watermark_through_synth(spliced, scans, joined):
    from vosk_tts_amd.synth import Synth
    from vosk_tts_amd.watermark_scan import WatermarkSegment

    sig = inspect.signature(Synth.locate_watermark).parameters
    assert (sig["key"].default, sig["span"].default, sig["payload"].default) == (None, 4, False)
    lib = _LibStub()
    s = _synth({"inference": {"watermark_key": KEY}}, lib)
    x = spliced[1.0]
    # the config key, float audio, the default span
    (seg,) = s.locate_watermark(x)
    want = S.segments(*scans[1.0, 4], 4, x.shape[0])[0]
    assert isinstance(seg, WatermarkSegment) and (seg.start, seg.end, seg.z, seg.offset_samples) == tuple(want)
    assert seg.payload is None and seg.bit_z is None
    assert lib.calls == [("scan", x.shape[0], KEY, 4, False, 3)]
    # int16 audio goes in as x / 32767, and the keyword key wins over the config's
    pcm = np.round(x * 32767.0).astype(np.int16)
    lib.calls.clear()
    (seg16,) = s.locate_watermark(pcm, key=KEY, span=2)
    assert lib.calls == [("scan", x.shape[0], KEY, 2, False, 3)]
    assert abs(seg16.z - S.segments(*scans[1.0, 2], 2, x.shape[0])[0].z) < 0.1 and seg16.offset_samples // 128 in (117, 118, 119)
    assert s.locate_watermark(x, key=KEY + 1) == [] and lib.calls[-1][2] == KEY + 1
    assert s.locate_watermark(np.zeros(0, np.float32)) == [] and s.locate_watermark(x[:400]) == []
    # payload=True: the scan on pilots, then the reader once per segment, on the segment's crop
    y, cut = joined
    lib.calls.clear()
    a, b = s.locate_watermark(y, payload=True)
    assert lib.calls == [("scan", y.shape[0], KEY, 4, True, 3), ("read", a.end - a.start, KEY, 3), ("read", b.end - b.start, KEY, 3)]
    assert (a.payload, b.payload) == (0xBEEF, 0x1234) and a.bit_z.shape == (24,) and b.bit_z.shape == (24,)
    # a plain mark located with payload=True: found on its pilots, and it carries no payload
    (p,) = s.locate_watermark(spliced[2.0], payload=True)
    assert p.payload is None and p.bit_z.shape == (24,)
    # refusals before the library is touched
    lib.calls.clear()
    for bad in (9, -1, 2.5):
        with pytest.raises(ValueError, match="span"):
            s.locate_watermark(x, span=bad)
    with pytest.raises(ValueError, match="inference.watermark_key"):
        _synth({"inference": {}}, lib).locate_watermark(x)
    with pytest.raises(NotImplementedError, match="watermark scan"):
        _synth({"inference": {}}, None).locate_watermark(x, KEY)
    assert lib.calls == []


def test_command_line(tmp_path, capsys):
    from vosk_tts_amd import cli
    from vosk_tts_amd.watermark_scan import WatermarkSegment

    p = cli.build_parser()
    o = p.parse_args(["--locate-watermark", "a.wav", "--watermark", "0x5EED1234", "--watermark-span", "2", "--read-payload"])
    assert (o.locate_watermark, o.watermark, o.watermark_span, o.read_payload, o.input) == ("a.wav", KEY, 2, True, None)
    o = p.parse_args(["-i", "x"])
    assert (o.locate_watermark, o.watermark_span, o.read_payload) == (None, 4, False)
    path = str(tmp_path / "a.wav")
    with wave.open(path, "w") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(np.arange(1000, dtype=np.int16).tobytes())
    seen = []

    class Syn:
        def locate_watermark(self, audio, key, span=4, payload=False):
            seen.append((audio.dtype, audio.shape, key, span, payload))
            return [WatermarkSegment(16000, 48000, 9.1234, 640, 0xBEEF if payload else None), WatermarkSegment(64000, 80000, 7.5, 0)]

    assert cli.locate_watermark(Syn(), path, 5, 2, True) == 0
    assert seen == [(np.dtype(np.int16), (1000,), 5, 2, True)]
    lines = [json.loads(line) for line in capsys.readouterr().out.splitlines()]
    assert lines == [{"start_s": 1.0, "end_s": 3.0, "z": 9.123, "offset_samples": 640, "payload": 0xBEEF},
                     {"start_s": 4.0, "end_s": 5.0, "z": 7.5, "offset_samples": 0, "payload": None}]
    assert cli.locate_watermark(Syn(), path, None) == 0
    assert "payload" not in json.loads(capsys.readouterr().out.splitlines()[0])
