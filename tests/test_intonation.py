"""Intonation range on the CPU (include/vits_intonation.h): the header against its ctypes mirrors, the float64 restatement
(tests/intonation_ref.py) against the contour stage it rests on, what the definition does to a glide, the decision margins of every
input of tests/test_intonation_gpu.py, and the plumbing from Synth, the sessions, the command line and SSML down to the engine call,
against stubs.  The device is checked in tests/test_intonation_gpu.py."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import contour_ref as C
import intonation_ref as I
import pitch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_layout_flags_and_export(tmp_path, hip_lib):
    from vosk_tts_amd import capi, capi_stts

    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vits_intonation.h"', 'int main(void) {',
             '  printf("%d %d %d %g %d %d %g %d\\n", VITS_FLAG_INTONATION, STTS_FLAG_INTONATION, VITS_INTONATION_WINDOW, '
             '(double)VITS_INTONATION_THRESHOLD, VITS_INTONATION_MIN_RATE, VITS_INTONATION_MAX_RATE, (double)VITS_INTONATION_MAX_RANGE, '
             'VITS_INTONATION_MAX_CENTS);',
             '  printf("%zu %zu %zu %zu\\n", sizeof(vits_synth_opts_intonation), offsetof(vits_synth_opts_intonation, base), '
             'offsetof(vits_synth_opts_intonation, pitch_range), sizeof(vits_synth_opts_contour));',
             '  printf("%zu %zu %zu %zu\\n", sizeof(stts_synth_opts_intonation), offsetof(stts_synth_opts_intonation, base), '
             'offsetof(stts_synth_opts_intonation, pitch_range), sizeof(stts_synth_opts_contour));',
             '  return 0;', '}']
    src = tmp_path / "c.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "c"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert [float(v) for v in out[0]] == pytest.approx([capi.FLAG_INTONATION, capi_stts.STTS_FLAG_INTONATION, I.W, I.THRESHOLD, *capi.INTONATION_RATES,
                                                        capi.INTONATION_MAX_RANGE, I.MAX_CENTS], rel=1e-6)
    assert (capi.FLAG_INTONATION, capi_stts.STTS_FLAG_INTONATION, I.W, I.MIN_RATE, I.MAX_RATE, I.MAX_RANGE) == (128, 128, 512, 8000, 32000, 4.0)
    assert [int(v) for v in out[1]] == [ctypes.sizeof(capi.SynthIntonationOpts), 0, capi.SynthIntonationOpts.pitch_range.offset,
                                        ctypes.sizeof(capi.SynthContourOpts)]
    assert [int(v) for v in out[2]] == [ctypes.sizeof(capi_stts.SttsIntonationOpts), 0, capi_stts.SttsIntonationOpts.pitch_range.offset,
                                        ctypes.sizeof(capi_stts.SttsContourOpts)]
    assert issubclass(capi.SynthIntonationOpts, capi.SynthContourOpts) and issubclass(capi_stts.SttsIntonationOpts, capi_stts.SttsContourOpts)
    # the flags are free in their families, and the library exports the doors with the binding's argument lists
    assert capi.FLAG_INTONATION not in (1, capi.FLAG_LOUDNESS, capi.FLAG_PITCH, capi.FLAG_PITCH_FORMANT, capi.FLAG_LIMIT, capi.FLAG_PROSODY, capi.FLAG_CONTOUR)
    assert capi_stts.STTS_FLAG_INTONATION not in (capi_stts.STTS_FLAG_ITEM_SEEDS, capi_stts.STTS_FLAG_DENOISE, capi_stts.STTS_FLAG_LOUDNESS,
                                                  capi_stts.STTS_FLAG_PITCH, capi_stts.STTS_FLAG_PITCH_FORMANT, capi_stts.STTS_FLAG_LIMIT,
                                                  capi_stts.STTS_FLAG_CONTOUR)
    assert hip_lib.has_intonation
    assert [len(hip_lib._fn(n).argtypes) for n in ("op_f0_track", "op_intonation", "op_intonation_stretch")] == [7, 14, 16]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (4173, 8192, 12288))
@pytest.mark.parametrize("r", (0.0, 0.5, 1.5))
def test_without_tokens_it_is_the_contour_of_one_token_per_row(n, r):
    """exact: the integers are the same (12288 and 8192 are multiples of H, where the contour stage reads the last row's token at
    len - 1, which is why the ratio of row f is taken from row min(f H, len - 1) // H)"""
    x = I.glide(n) if n != 4173 else R.voiced(n, seed=0)
    rep = {}
    y = I.intonation(x, 22050, r, report=rep)
    F = C.frames(n)
    assert rep["shifted"] and rep["o"].shape == (F,) and np.abs(rep["o"]).max() <= 1200
    want = C.contour(x, np.arange(1, F + 1), F, 256, rep["o"] / 100.0)
    assert np.array_equal(y, want)


def test_offsets_are_integers_with_a_stated_rounding():
    cents = np.array([0, 0, 3000, 3101, 0, 0, 0, 2950, 3000, 0])
    o = I.offsets(cents, 500)
    # the lower median of (2950, 3000, 3000, 3101) is 3000; voiced rows: rha(-500 (c - 3000) / 1000)
    assert o[[2, 3, 7, 8]].tolist() == [0, -51, 25, 0]  # (-50.5 rounds away from zero)
    assert o[:2].tolist() == [0, 0] and o[9] == 0  # held at the ends
    assert o[4:7].tolist() == [-51 + 19, -51 + 38, -51 + 57]  # rha(76 k / 4), k = 1, 2, 3
    assert not I.offsets(np.zeros(7, np.int64), 0).any()  # no voiced row
    # clamped to an octave after the interpolation: the unvoiced row lies halfway to the unclamped 18000, not halfway to 1200
    assert I.offsets(np.array([3000, 0, 9000]), 4000).tolist() == [0, 1200, 1200]
    assert I.offsets(np.array([3000, 0, 0, 0, 3100]), 4000).tolist() == [0, 75, 150, 225, 300]
    assert I.rha([5, -5, 7, -7, 0], 10).tolist() == [1, -1, 1, -1, 0]
    assert (I.TAB[0], I.TAB[1200], I.TAB[2400], I.TAB.shape) == (500, 1000, 2000, (2401,))
    assert I.frame_ratios([1000, 2000, 500, 1000], [0, 1200, -1200, 700]).tolist() == [1000, 2000, 500, I.TAB[1900]]
    with pytest.raises(ValueError, match="4.5"):
        I.range_milli(4.5)
    with pytest.raises(ValueError, match="nan"):
        I.range_milli(float("nan"))
    with pytest.raises(ValueError, match="48000"):
        I.lags(48000)
    assert I.lags(22050) == (40, 401) and I.lags(8000) == (14, 146) and I.lags(32000) == (58, 511)


def test_exact_cases_of_the_restatement():
    for x in (I.noise(2048, seed=3), np.zeros(1500, np.float32), R.voiced(8192, seed=1)[:400]):
        rep = {}
        y = I.intonation(x, 22050, 0.0, report=rep)
        assert not rep["shifted"] and y.astype(np.float32).tobytes() == x.tobytes()
    x = R.voiced(4352, seed=0)
    assert I.intonation(x, 22050, 1.0004).astype(np.float32).tobytes() == x.tobytes()  # r_m == 1000: every R_f is 1000


@pytest.fixture(scope="module")
def glide():
    x = I.glide(12288)
    return x, I.glide_skip(x.shape[0])


@pytest.mark.parametrize("r", (0.5, 1.5))
def test_definition_scales_the_movement_of_a_glide(glide, r):
    x, skip = glide
    s, _ = I.slope(x, I.intonation(x, 22050, r), 22050, skip)
    print(f"r = {r}: slope {s:.4f}")
    assert abs(s - r) <= 0.05


def test_definition_flattens_a_glide_at_zero(glide):
    x, skip = glide
    _, dev = I.slope(x, I.intonation(x, 22050, 0.0), 22050, skip)
    print(f"r = 0: largest deviation {dev:g} cents")
    assert dev < 15


def test_margins_of_the_gpu_inputs():
    """the float32 and float64 trackers agree on every frame of every input of the GPU test, and no frame's margin is below 4 times the
    item's yardstick: the GPU test's exclusion rule leaves out nothing the reference alone would"""
    inputs = [(name, b, v, I.GPU_RATE) for name, items in I.gpu_cases().items() for b, v in enumerate(items)]
    inputs += [("16k", 0, R.voiced(4352, rate=16000, seed=0), 16000), ("glide12288", 0, I.glide(12288), I.GPU_RATE)]
    for name, b, v, rate in inputs:
        fg = I.track_figures(v, rate)
        assert np.array_equal(fg["c64"] > 0, fg["c32"] > 0), (name, b)
        assert np.abs(fg["c64"] - fg["c32"]).max(initial=0) <= 1, (name, b)
        assert (fg["margin"] >= 4 * fg["yardstick"]).all(), (name, b, fg["margin"].min(), fg["yardstick"])
        if v.shape[0] >= R.MIN_LEN:
            assert 0 < fg["yardstick"] < 1e-4 or not v.any()


# ---- plumbing against stubs ---------------------------------------------------------------------------------------------------------------
def test_range_spec_and_the_options_struct(hip_lib):
    from vosk_tts_amd import capi, capi_stts

    assert capi.range_spec(None) is None and capi.range_spec(1.0) is None and capi.range_spec(1.0004) is None and capi.range_spec(0.9996) is None
    assert capi.range_spec(0.5) == 0.5 and capi.range_spec(0) == 0.0 and capi.range_spec(4) == 4.0
    for bad in (-0.01, 4.01, float("nan")):
        with pytest.raises(ValueError, match="pitch_range"):
            capi.range_spec(bad)
    m = capi.VitsModel.__new__(capi.VitsModel)
    m.lib = hip_lib
    opts, _ = m._opts(1, 4, None, None, None, 0, 0, pitch_range=1.0004)
    assert type(opts) is capi.SynthOpts and opts.flags == 0  # r_m == 1000: the options of before
    opts, _ = m._opts(1, 4, None, None, None, 0, 0, pitch_range=0.5)
    assert type(opts) is capi.SynthIntonationOpts and opts.flags == capi.FLAG_INTONATION and opts.pitch_range == 0.5 and not opts.contour
    opts, _ = m._opts(1, 4, None, None, None, 0, 0, pitch=2.0, pitch_range=1.5)
    assert opts.flags == capi.FLAG_INTONATION | capi.FLAG_PITCH and opts.pitch_semitones == 2.0
    s = capi_stts.SttsModel.__new__(capi_stts.SttsModel)
    s.vlib = hip_lib
    assert type(s._opts_for(None, None, pitch_range=None)) is capi_stts.SttsOpts
    o = s._opts_for(None, 3.0, pitch_range=0.25)
    assert type(o) is capi_stts.SttsIntonationOpts and o.flags == capi_stts.STTS_FLAG_INTONATION | capi_stts.STTS_FLAG_PITCH and o.pitch_range == 0.25
    for fn in (capi.VitsModel.synthesize, capi.VitsModel.synthesize_pcm16, capi_stts.SttsModel.synthesize, capi_stts.SttsModel.synthesize_batch):
        assert inspect.signature(fn).parameters["pitch_range"].default is None


class _Hp:
    sampling_rate, hop_length, bert_dim, n_speakers = 22050, 256, 0, 4


class _EngineStub:
    """stands where capi.VitsModel stands: records the keywords of every engine call"""

    def __init__(self):
        self.hp = _Hp()
        self.calls = []

    def synthesize_pcm16(self, ids, lens, scales, sid, pcm_scale=1.0, seed=0, solo=False, item_seeds=None, sample_rate=None, **kw):
        self.calls.append((ids.shape[0], {k: v for k, v in kw.items() if k in ("pitch", "pitch_range")}))
        B = ids.shape[0]
        return np.zeros((B, 8), np.int16), np.full(B, 8, np.int64)

    def close(self):
        pass


class _LibStub:
    is_device = True
    has_pitch = has_intonation = True

    def __init__(self):
        self.model = _EngineStub()

    def create(self, blob, device):
        return self.model

    def _need_pitch(self):
        pass

    def _need_intonation(self):
        pass


def _feed(**ext):
    return dict({"input": np.ones((1, 5), np.int64), "input_lengths": np.array([5]), "scales": np.array([0.8, 1.0, 0.8], np.float32),
                 "sid": np.array([1])}, **ext)


def test_sessions_take_the_feed_key_and_it_is_a_coalescer_key():
    from vosk_tts_amd import session, session_stts
    from vosk_tts_amd.outopts import Tail
    from vosk_tts_amd.session import VitsSession

    for mod in (session, session_stts):
        assert "vits.pitch_range" in mod._EXT
    lib = _LibStub()
    sess = VitsSession(b"", lib=lib)
    keys = []
    submit = sess.coalescer.submit
    sess.coalescer.submit = lambda key, *a: (keys.append(key), submit(key, *a))[1]
    sess.run_pcm16(_feed(), 1.0)
    sess.run_pcm16(_feed(**{"vits.pitch_range": 1.0004}), 1.0)  # r_m == 1000: the request it was, the key it had
    sess.run_pcm16(_feed(**{"vits.pitch_range": 0.5}), 1.0)
    sess.run_pcm16(_feed(**{"vits.pitch_range": 1.5}), 1.0)
    sess.run_pcm16(_feed(**{"vits.pitch_range": 0.5, "vits.pitch": 2.0}), 1.0)
    assert [c[1] for c in lib.model.calls] == [{}, {}, {"pitch_range": 0.5}, {"pitch_range": 1.5}, {"pitch_range": 0.5, "pitch": 2.0}]
    assert keys[0] == keys[1] and keys[0] == ("pcm", 1.0, 0, False, Tail()) and len({keys[0], keys[2], keys[3], keys[4]}) == 4  # different ranges do not share a batch
    # two requests of one key in one batch carry the range once, for the batch
    out = sess._run_solo_batch(keys[2], [(np.ones((1, 4), np.int64), 0, 1, (0.8, 1.0, 0.8)), (np.ones((1, 3), np.int64), 1, 2, (0.8, 1.0, 0.8))])
    assert len(out) == 2 and lib.model.calls[-1] == (2, {"pitch_range": 0.5})
    for bad in (-1.0, 5.0, float("nan")):
        with pytest.raises(ValueError, match="pitch_range"):
            sess.run_pcm16(_feed(**{"vits.pitch_range": bad}), 1.0)
    with pytest.raises(ValueError, match="intonation range"):
        sess.run_stream(None, _feed(**{"vits.pitch_range": 0.5}))
    st = session_stts.SttsSession.__new__(session_stts.SttsSession)
    st._lib = lib
    assert Tail.from_feed(lib, {}).kw() == {} and Tail.from_feed(lib, {"vits.pitch_range": 1.0}).kw() == {}
    assert Tail.from_feed(lib, {"vits.pitch_range": 0.25, "vits.pitch": -5}).kw() == {"pitch": -5.0, "pitch_range": 0.25}


def _synth(config):
    from vosk_tts_amd.synth import Synth

    class M:
        pass

    s = Synth.__new__(Synth)
    s.model = M()
    s.model.config = config
    s.model.onnx = type("Sess", (), {"hp": _Hp()})()
    return s


def test_synth_takes_the_keyword_and_the_config_key():
    from vosk_tts_amd.batching import MultiDeviceSynth
    from vosk_tts_amd.synth import Synth

    for fn in (Synth.synth_audio, Synth.synth, Synth.synth_stream, MultiDeviceSynth.synth_batch):
        assert inspect.signature(fn).parameters["pitch_range"].default is None
    assert hasattr(Synth, "measure_pitch")
    s = _synth({"inference": {}})
    args = {}
    assert not s._range(args, None) and not s._range(args, 1.0) and not s._range(args, 1.0004) and args == {}  # the feed of before
    assert s._range(args, 0.5) and args == {"vits.pitch_range": 0.5}
    c = _synth({"inference": {"pitch_range": 1.5}})
    args = {}
    assert c._range(args, None) and args == {"vits.pitch_range": 1.5}
    assert c._range(args, 0.0) and args == {"vits.pitch_range": 0.0}  # the keyword wins
    for bad, match in ((4.5, "4.5"), (-0.5, "-0.5"), (float("nan"), "nan")):
        with pytest.raises(ValueError, match=match):
            s._range({}, bad)
    with pytest.raises(ValueError, match="intonation range"):  # before the model is touched: the stub has none
        next(iter(s.synth_stream("a", pitch_range=0.5)))
    with pytest.raises(NotImplementedError, match="F0 tracker"):
        s.measure_pitch(np.zeros(1024, np.float32))


def test_command_line_flag():
    from vosk_tts_amd import cli

    assert cli.build_parser().parse_args(["-i", "x", "--pitch-range", "0.5"]).pitch_range == 0.5
    assert cli.build_parser().parse_args(["-i", "x"]).pitch_range is None


# ---- SSML ---------------------------------------------------------------------------------------------------------------------------------
def test_ssml_range_on_the_whole_document():
    from vosk_tts_amd import ssml

    for v, want in (("x-low", 0.25), ("low", 0.5), ("medium", 1.0), ("high", 1.5), ("x-high", 2.0), ("default", 1.0), ("50%", 0.5), ("+20%", 1.2),
                    ("-100%", 0.0), ("0%", 0.0), ("400%", 4.0)):
        plan = ssml.parse(f'<speak><prosody range="{v}">one two</prosody></speak>')
        assert plan.pitch_range == pytest.approx(want) and plan.text == "one two" and plan.keywords() == {"pitch_range": plan.pitch_range}
    plan = ssml.parse('<speak><p><prosody range="low" rate="fast">one <prosody pitch="+2st">two</prosody></prosody></p></speak>')
    assert plan.keywords() == {"pitch_range": 0.5, "word_rates": {0: 1.5, 1: 1.5}, "word_pitch": {1: 2.0}}
    assert ssml.parse("<speak>one two</speak>").pitch_range is None and "pitch_range" not in ssml.parse("<speak>one</speak>").keywords()
    for doc, match in (('<speak>one <prosody range="low">two</prosody></speak>', "range='low' covers words 1 to 1 of 2"),
                       ('<speak><prosody range="high">one</prosody> two</speak>', "range='high'"),
                       ('<speak><prosody range="wide">one</prosody></speak>', "range='wide'"),
                       ('<speak><prosody range="500%">one</prosody></speak>', "range='500%'"),
                       ('<speak><prosody range="-120%">one</prosody></speak>', "range='-120%'")):
        with pytest.raises(ValueError, match=match):
            ssml.parse(doc)


def test_synth_ssml_passes_the_range_on():
    from vosk_tts_amd.synth import Synth

    s = Synth.__new__(Synth)
    seen = {}
    s.synth_audio = lambda text, **kw: seen.update(text=text, **kw) or np.zeros(4, np.int16)
    s.synth_ssml('<speak><prosody range="low">one two</prosody></speak>', speaker_id=2)
    assert seen == {"text": "one two", "speaker_id": 2, "pitch_range": 0.5}
    with pytest.raises(ValueError, match="pitch_range"):
        s.synth_ssml('<speak><prosody range="low">one two</prosody></speak>', pitch_range=0.7)
    seen.clear()
    s.synth_ssml("<speak>one two</speak>", pitch_range=0.7)  # without a range in the document the keyword is the caller's
    assert seen["pitch_range"] == 0.7
