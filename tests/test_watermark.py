"""The audio watermark on the CPU (include/vits_watermark.h): the header against its ctypes mirrors, the chips against a table, the
conditions the float64 restatement (tests/watermark_ref.py) has to meet on the test signal -- which are also the decision margins of
every input of tests/test_watermark_gpu.py -- and the plumbing from Synth, the sessions and the command line down to the engine call,
against stubs.  The device is checked in tests/test_watermark_gpu.py.

How the conditions are read.  "z >= 8 at o" is the score OF THAT OFFSET INDEX, z_all[o] >= 8.  The arg-max may sit one index away: two
neighbouring indices are 128 samples = 1/8 of a tile row apart, their scores differ by a few per cent, and a crop of 12345 = 96.45 * 128
samples lies between two of them.  So the arg-max is asserted to be within one index of o, and its offset is what the GPU test compares
as an integer.  Figures of the float64 restatement on voiced_signal(3.0) (printed by the test): marked z_all[0] = 10.05; int16 and
1e-3-scaled within 0.03 of it; crop 5000: z_all[39] = 9.21; crop 12345: z_all[96] = 11.31; unmarked at most 0.62 and three other keys at
most 2.41 over all 128 offsets."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import watermark_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = 0x5EED1234
OTHER_KEYS = (KEY + 1, 1, 0xDEADBEEF)
MIX_IN = (0, 1, 2, 0xDEADBEEF, 0x5EED1234, 0xFFFFFFFF, 12345, 1 << 31)
MIX_OUT = (0x0, 0x688990C0, 0xD1132181, 0xE628C683, 0x6BBB11B0, 0x6768824A, 0x912EFCF7, 0xCC4B4124)
CHIPS_Q0 = (-1, 1, 1, -1, 1, -1, -1, 1)  # c(KEY, 0, 0 .. 7)


def test_header_layout_flags_and_export(tmp_path, hip_lib):
    from vosk_tts_amd import capi, capi_stts

    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vits_watermark.h"',
             # the header's own words for mix, in C's uint32
             'static uint32_t mix(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }',
             'int main(void) {',
             '  printf("%d %d %d %d %d %d %d %d %d %g %g %g\\n", VITS_FLAG_WATERMARK, STTS_FLAG_WATERMARK, VITS_WATERMARK_FRAME, VITS_WATERMARK_BIN_LO, '
             'VITS_WATERMARK_BIN_HI, VITS_WATERMARK_GROUPS, VITS_WATERMARK_ROWS, VITS_WATERMARK_OFFSETS, VITS_WATERMARK_DETECT_HOP, '
             '(double)VITS_WATERMARK_DEFAULT_DEPTH_DB, (double)VITS_WATERMARK_MAX_DEPTH_DB, (double)VITS_WATERMARK_THRESHOLD);',
             '  printf("%zu %zu %zu %zu %zu\\n", sizeof(vits_synth_opts_watermark), offsetof(vits_synth_opts_watermark, base), '
             'offsetof(vits_synth_opts_watermark, watermark_key), offsetof(vits_synth_opts_watermark, watermark_depth_db), '
             'sizeof(vits_synth_opts_intonation));',
             '  printf("%zu %zu %zu %zu %zu\\n", sizeof(stts_synth_opts_watermark), offsetof(stts_synth_opts_watermark, base), '
             'offsetof(stts_synth_opts_watermark, watermark_key), offsetof(stts_synth_opts_watermark, watermark_depth_db), '
             'sizeof(stts_synth_opts_intonation));',
             '  ' + " ".join(f'printf("%u ", mix({v}u));' for v in MIX_IN) + ' printf("\\n");',
             '  return 0;', '}']
    src = tmp_path / "c.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "c"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert [float(v) for v in out[0]] == [capi.FLAG_WATERMARK, capi_stts.STTS_FLAG_WATERMARK, R.N, R.BIN_LO, R.BIN_HI, R.GROUPS, R.ROWS, R.OFFSETS,
                                         R.DETECT_HOP, R.DEFAULT_DEPTH_DB, R.MAX_DEPTH_DB, R.THRESHOLD]
    assert (capi.FLAG_WATERMARK, capi_stts.STTS_FLAG_WATERMARK, capi.WATERMARK_THRESHOLD, capi.WATERMARK_MAX_DEPTH_DB, capi.WATERMARK_OFFSETS) == (256, 256, 6.0, 2.0, 128)
    for row, W, I in ((out[1], capi.SynthWatermarkOpts, capi.SynthIntonationOpts), (out[2], capi_stts.SttsWatermarkOpts, capi_stts.SttsIntonationOpts)):
        assert [int(v) for v in row] == [ctypes.sizeof(W), 0, W.watermark_key.offset, W.watermark_depth_db.offset, ctypes.sizeof(I)]
        assert issubclass(W, I)
    assert [int(v) for v in out[3]] == list(MIX_OUT)  # the C of the header's words, the table and (below) the restatement agree
    # the bit is free in both families, and the library exports the doors with the binding's argument lists
    assert capi.FLAG_WATERMARK not in (1, capi.FLAG_LOUDNESS, capi.FLAG_PITCH, capi.FLAG_PITCH_FORMANT, capi.FLAG_LIMIT, capi.FLAG_PROSODY, capi.FLAG_CONTOUR,
                                       capi.FLAG_INTONATION)
    assert capi_stts.STTS_FLAG_WATERMARK not in (capi_stts.STTS_FLAG_ITEM_SEEDS, capi_stts.STTS_FLAG_DENOISE, capi_stts.STTS_FLAG_LOUDNESS,
                                                 capi_stts.STTS_FLAG_PITCH, capi_stts.STTS_FLAG_PITCH_FORMANT, capi_stts.STTS_FLAG_LIMIT,
                                                 capi_stts.STTS_FLAG_CONTOUR, capi_stts.STTS_FLAG_INTONATION)
    assert hip_lib.has_watermark
    assert [len(hip_lib._fn(n).argtypes) for n in ("op_watermark", "op_watermark_detect")] == [8, 10]


def test_mix_and_chips_equal_the_table():
    assert [int(v) for v in R.mix(np.array(MIX_IN, np.uint64))] == list(MIX_OUT)
    c = R.chips(KEY)
    assert c.shape == (16, 96) and set(np.unique(c)) == {-1.0, 1.0}
    assert tuple(int(v) for v in c[0, :8]) == CHIPS_Q0
    # c(key, q, j) from the definition's words, element by element, for the written-out row
    mk = int(R.mix(KEY))
    assert [1 if int(R.mix(mk ^ (96 * 0 + j + 1))) & 1 else -1 for j in range(8)] == list(CHIPS_Q0)
    for key in (KEY, 0, 1, 0xDEADBEEF, KEY + 1):
        ones = int((R.chips(key) > 0).sum())
        assert 700 <= ones <= 836, (key, ones)  # 768 +- 3.5 sigma (sigma = sqrt(1536) / 2 = 19.6): a sanity bound, not a measurement
    assert not np.array_equal(R.chips(KEY), R.chips(KEY + 1))


# ---- the conditions on the restatement ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def signal():
    x = R.voiced_signal(3.0)
    return x, R.embed(x, KEY)


def test_the_signal_is_what_the_issue_describes(signal):
    x, _ = signal
    assert x.dtype == np.float32 and x.shape == (66150,) and abs(float(np.abs(x).max()) - 0.5) < 1e-6
    assert np.array_equal(x, R.voiced_signal(3.0))  # seeded
    env = np.abs(x.astype(np.float64)).reshape(-1, 441).max(axis=1)  # 20 ms blocks
    assert (env < 0.02).mean() > 0.1 and (env > 0.1).mean() > 0.3  # gaps and syllables


def test_restatement_detects_marked_audio_and_only_that(signal):
    x, y = signal
    assert y.shape == x.shape and 0.01 < np.abs(y - x).max() / np.abs(x).max() < 0.2  # a ripple of about 1 dB, not a rewrite
    cases = {"marked": (y, 0), "int16": (np.round(y * 32767.0).astype(np.int16).astype(np.float64) / 32767.0, 0), "scaled 1e-3": (y * 1e-3, 0),
             "crop 5000": (y[5000:], 39), "crop 12345": (y[12345:], 96)}
    zs = {}
    for name, (a, o) in cases.items():
        d = R.detect(a, KEY)
        zs[name] = d["z_all"][o]
        print(f"{name}: z_all[{o}] = {d['z_all'][o]:.3f}, arg-max index {d['offset'] // 128} with z = {d['z']:.3f}, rows {d['rows']}")
        assert d["z_all"][o] >= 8.0, (name, d["z_all"][o])
        assert d["detected"] and min((d["offset"] // 128 - o) % 128, (o - d["offset"] // 128) % 128) <= 1, (name, d["offset"])
        assert d["z"] - R.THRESHOLD >= 2.0  # the GPU test's inputs stay at least 2 away from the threshold
    assert abs(zs["int16"] - zs["marked"]) < 1.0
    assert abs(zs["scaled 1e-3"] - zs["marked"]) < 1e-9  # the floor is relative to the frame: the score does not move with gain
    d = R.detect(x, KEY)
    print(f"unmarked: max z = {d['z_all'].max():.3f}")
    assert d["z_all"].max() < 4.0 and not d["detected"]
    for key in OTHER_KEYS:
        d = R.detect(y, key)
        print(f"key {key:#x}: max z = {d['z_all'].max():.3f}")
        assert d["z_all"].max() < 4.0 and not d["detected"]


def test_embed_edges_of_the_restatement(signal):
    x, _ = signal
    for n in (400, 512):  # below n/2 + 1: as it went in
        assert np.array_equal(R.embed(x[:n], KEY), x[:n].astype(np.float64))
    for n in (513, 600, 5000):
        y = R.embed(x[:n], KEY)
        assert y.shape == (n,) and np.array_equal(y[256 * (n // 256):], x[256 * (n // 256):n].astype(np.float64))
        assert not np.array_equal(y[:256 * (n // 256)], x[:256 * (n // 256)])
    assert np.array_equal(R.embed(x[:5000], KEY, 0.0), R.embed(x[:5000], KEY, 1.0))  # 0 = the default
    d = R.detect(x[:400], KEY)  # no frames: never detected
    assert (d["z"], d["offset"], d["rows"], d["detected"]) == (0.0, 0, 0, False) and not d["z_all"].any()
    for bad, match in ((-0.5, "-0.5"), (2.5, "2.5"), (float("nan"), "nan")):
        with pytest.raises(ValueError, match=match):
            R.embed(x[:5000], KEY, bad)
    # the fp32 run of the same code stays close: it is the yardstick of the GPU test
    y64, y32 = R.embed(x[:22050], KEY), R.embed(x[:22050], KEY, dtype=np.float32)
    assert y32.dtype == np.float32 and 0 < np.abs(y32 - y64).max() < 1e-6


# ---- plumbing against stubs -----------------------------------------------------------------------------------------------------
def test_watermark_spec_and_the_options_struct(hip_lib):
    from vosk_tts_amd import capi, capi_stts

    assert capi.watermark_spec(None) is None and capi.watermark_spec(False) is None
    assert capi.watermark_spec(KEY) == (KEY, 0.0) and capi.watermark_spec(0) == (0, 0.0) and capi.watermark_spec(np.uint32(7), 1.5) == (7, 1.5)
    for bad, match in ((-1, "-1"), (1 << 32, str(1 << 32)), ("k", "'k'"), (True, "True"), (1.5, "1.5")):
        with pytest.raises(ValueError, match=match):
            capi.watermark_spec(bad)
    for bad, match in ((0.0, "0.0"), (-1.0, "-1.0"), (2.01, "2.01"), (float("nan"), "nan")):
        with pytest.raises(ValueError, match=match):
            capi.watermark_spec(KEY, bad)
    m = capi.VitsModel.__new__(capi.VitsModel)
    m.lib = hip_lib
    opts, _ = m._opts(1, 4, None, None, None, 0, 0)
    assert type(opts) is capi.SynthOpts and opts.flags == 0  # the options of before
    opts, _ = m._opts(1, 4, None, None, None, 0, 0, watermark=(KEY, 0.0))
    assert type(opts) is capi.SynthWatermarkOpts and opts.flags == capi.FLAG_WATERMARK and opts.watermark_key == KEY and opts.watermark_depth_db == 0.0
    opts, _ = m._opts(1, 4, None, None, None, 0, 0, pitch=2.0, pitch_range=0.5, watermark=(3, 1.5))
    assert opts.flags == capi.FLAG_WATERMARK | capi.FLAG_INTONATION | capi.FLAG_PITCH and (opts.watermark_key, opts.watermark_depth_db, opts.pitch_range) == (3, 1.5, 0.5)
    s = capi_stts.SttsModel.__new__(capi_stts.SttsModel)
    s.vlib = hip_lib
    assert type(s._opts_for(None, None)) is capi_stts.SttsOpts
    o = s._opts_for(None, 3.0, watermark=(KEY, 2.0))
    assert type(o) is capi_stts.SttsWatermarkOpts and o.flags == capi_stts.STTS_FLAG_WATERMARK | capi_stts.STTS_FLAG_PITCH
    assert (o.watermark_key, o.watermark_depth_db) == (KEY, 2.0)
    for fn in (capi.VitsModel.synthesize, capi.VitsModel.synthesize_pcm16, capi.VitsModel.synthesize_document, capi_stts.SttsModel.synthesize,
               capi_stts.SttsModel.synthesize_batch, capi_stts.SttsModel.synthesize_document):
        p = inspect.signature(fn).parameters
        assert p["watermark"].default is None and p["watermark_depth_db"].default is None
    # the streams refuse by name before any device work
    for st, args in ((m.stream, (np.ones((1, 4), np.int64), [0.8, 1.0, 0.8], 0)), (s.stream, (np.ones((5, 4), np.int64), [0.8, 1.0, 0.8], 0))):
        with pytest.raises(capi.VitsError, match="FLAG_WATERMARK") as e:
            st(*args, watermark=KEY)
        assert e.value.code == 4


class _Hp:
    sampling_rate, hop_length, bert_dim, n_speakers = 22050, 256, 0, 4


class _EngineStub:
    """stands where capi.VitsModel stands: records the keywords of every engine call"""

    def __init__(self):
        self.hp = _Hp()
        self.calls = []

    def synthesize_pcm16(self, ids, lens, scales, sid, pcm_scale=1.0, seed=0, solo=False, item_seeds=None, sample_rate=None, **kw):
        self.calls.append((ids.shape[0], {k: v for k, v in kw.items() if k in ("pitch_range", "watermark", "watermark_depth_db")}))
        B = ids.shape[0]
        return np.zeros((B, 8), np.int16), np.full(B, 8, np.int64)

    def close(self):
        pass


class _LibStub:
    is_device = True
    has_watermark = has_intonation = True

    def __init__(self):
        self.model = _EngineStub()

    def create(self, blob, device):
        return self.model

    def _need_watermark(self):
        pass

    def _need_intonation(self):
        pass


def _feed(**ext):
    return dict({"input": np.ones((1, 5), np.int64), "input_lengths": np.array([5]), "scales": np.array([0.8, 1.0, 0.8], np.float32),
                 "sid": np.array([1])}, **ext)


def test_sessions_take_the_feed_keys_and_a_marked_feed_is_not_coalesced_with_an_unmarked_one():
    from vosk_tts_amd import session, session_stts
    from vosk_tts_amd.outopts import Tail
    from vosk_tts_amd.session import VitsSession

    for mod in (session, session_stts):
        assert "vits.watermark_key" in mod._EXT and "vits.watermark_depth_db" in mod._EXT
    lib = _LibStub()
    sess = VitsSession(b"", lib=lib)
    keys = []
    submit = sess.coalescer.submit
    sess.coalescer.submit = lambda key, *a: (keys.append(key), submit(key, *a))[1]
    sess.run_pcm16(_feed(), 1.0)
    sess.run_pcm16(_feed(**{"vits.watermark_key": KEY}), 1.0)
    sess.run_pcm16(_feed(**{"vits.watermark_key": KEY + 1}), 1.0)
    sess.run_pcm16(_feed(**{"vits.watermark_key": KEY, "vits.watermark_depth_db": 2.0}), 1.0)
    sess.run_pcm16(_feed(**{"vits.watermark_key": KEY, "vits.pitch_range": 0.5}), 1.0)
    assert [c[1] for c in lib.model.calls] == [{}, {"watermark": KEY}, {"watermark": KEY + 1}, {"watermark": KEY, "watermark_depth_db": 2.0},
                                               {"watermark": KEY, "pitch_range": 0.5}]
    assert keys[0] == ("pcm", 1.0, 0, False, Tail()) and len(set(keys)) == 5  # the key of before without a mark; with one, only the same key and depth share a batch
    out = sess._run_solo_batch(keys[3], [(np.ones((1, 4), np.int64), 0, 1, (0.8, 1.0, 0.8)), (np.ones((1, 3), np.int64), 1, 2, (0.8, 1.0, 0.8))])
    assert len(out) == 2 and lib.model.calls[-1] == (2, {"watermark": KEY, "watermark_depth_db": 2.0})
    for bad, match in (({"vits.watermark_key": -1}, "-1"), ({"vits.watermark_key": KEY, "vits.watermark_depth_db": 3.0}, "3.0"),
                       ({"vits.watermark_depth_db": 1.0}, "needs")):
        with pytest.raises(ValueError, match=match):
            sess.run_pcm16(_feed(**bad), 1.0)
    with pytest.raises(ValueError, match="FLAG_WATERMARK"):
        sess.run_stream(None, _feed(**{"vits.watermark_key": KEY}))
    st = session_stts.SttsSession.__new__(session_stts.SttsSession)
    st._lib = lib
    assert Tail.from_feed(lib, {}).kw() == {} and Tail.from_feed(lib, {"vits.watermark_key": KEY}).kw() == {"watermark": KEY}
    assert Tail.from_feed(lib, {"vits.watermark_key": 5, "vits.watermark_depth_db": 0.5}).kw() == {"watermark": 5, "watermark_depth_db": 0.5}
    assert st.mark(np.zeros((1, 8), np.float32), [8], None).shape == (1, 8)  # no key: the audio as it was, no library call


def _synth(config):
    from vosk_tts_amd.synth import Synth

    class M:
        pass

    s = Synth.__new__(Synth)
    s.model = M()
    s.model.config = config
    s.model.onnx = type("Sess", (), {"hp": _Hp()})()
    return s


def test_synth_takes_the_keyword_and_true_takes_the_config_key():
    from vosk_tts_amd.batching import MultiDeviceSynth
    from vosk_tts_amd.synth import Synth

    for fn in (Synth.synth_audio, Synth.synth, Synth.synth_document, Synth.synth_stream, MultiDeviceSynth.synth_batch):
        assert inspect.signature(fn).parameters["watermark"].default is None
    assert hasattr(Synth, "detect_watermark")
    s = _synth({"inference": {}})
    args = {}
    assert not s._watermark(args, None) and not s._watermark(args, False) and args == {}  # the feed of before
    assert s._watermark(args, KEY) and args == {"vits.watermark_key": KEY}
    args = {}
    assert s._watermark(args, 7, 1.5) and args == {"vits.watermark_key": 7, "vits.watermark_depth_db": 1.5}
    with pytest.raises(ValueError, match="inference.watermark_key"):
        s._watermark({}, True)
    c = _synth({"inference": {"watermark_key": 99}})
    args = {}
    assert not c._watermark(args, None) and args == {}  # a config key alone marks nothing
    assert c._watermark(args, True) and args == {"vits.watermark_key": 99}
    assert c._watermark(args, 5) and args == {"vits.watermark_key": 5}  # the keyword wins
    for bad, match in (((-1, None), "-1"), ((1 << 32, None), str(1 << 32)), ((KEY, 2.5), "2.5"), ((KEY, float("nan")), "nan"), ((None, 1.0), "needs")):
        with pytest.raises(ValueError, match=match):
            s._watermark({}, *bad)
    with pytest.raises(ValueError, match="FLAG_WATERMARK"):  # before the model is touched: the stub has none
        next(iter(s.synth_stream("a", watermark=KEY)))
    with pytest.raises(NotImplementedError, match="watermark detector"):
        s.detect_watermark(np.zeros(1024, np.float32), KEY)
    with pytest.raises(ValueError, match="inference.watermark_key"):
        s.detect_watermark(np.zeros(1024, np.float32))


def test_command_line_flags():
    from vosk_tts_amd import cli

    p = cli.build_parser()
    assert p.parse_args(["-i", "x", "--watermark", "0x5EED1234"]).watermark == KEY
    assert p.parse_args(["-i", "x", "--watermark", "77"]).watermark == 77
    o = p.parse_args(["-i", "x"])
    assert o.watermark is None and o.detect_watermark is None
    o = p.parse_args(["--detect-watermark", "a.wav", "--watermark", "5"])
    assert (o.detect_watermark, o.watermark, o.input) == ("a.wav", 5, None)
    for bad in ("-1", "4294967296", "key"):
        with pytest.raises(SystemExit):
            p.parse_args(["-i", "x", "--watermark", bad])


def test_detect_command_prints_the_triple(tmp_path, capsys):
    import json
    import wave

    from vosk_tts_amd import cli

    path = str(tmp_path / "a.wav")
    with wave.open(path, "w") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(22050)
        f.writeframes(np.arange(1000, dtype=np.int16).tobytes())
    seen = []

    class S:
        def detect_watermark(self, audio, key):
            seen.append((audio.dtype, audio.shape, key))
            return True, 9.25, 640

    assert cli.detect_watermark(S(), path, 5) == 0
    assert seen == [(np.dtype(np.int16), (1000,), 5)]
    assert json.loads(capsys.readouterr().out) == {"detected": True, "z": 9.25, "offset_samples": 640}
