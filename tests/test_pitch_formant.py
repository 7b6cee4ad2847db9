"""Formant-preserving pitch shift (steps 3a-3d of include/vits_pitch.h), the parts that need no GPU: that the correction corrects, on a
synthetic vowel; that the phases are the plain call's; the properties of the gain; the float32 run of the restatement against the
float64 run (the yardstick of tests/test_pitch_formant_gpu.py); the ABI and the Python plumbing."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import pitch_formant_ref as F
import pitch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert hip_lib.has_pitch_formant, "libvits_mi355.so exports no vits_op_pitch_formant_gain"
    return hip_lib


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vowel():
    return F.vowel()


def test_untouched_vowel_reads_its_own_formant_curve(vowel):
    x, sc = vowel
    assert np.abs(x).max() == pytest.approx(0.3, rel=1e-6) and x.dtype == np.float32 and x.shape == (16384,)
    assert F.envelope_deviation(x, 1, 1, sc) < 0.5  # (0.35 dB: what the measure itself leaves)


@pytest.mark.parametrize("s", (-4.0, 4.0, 7.0))
def test_the_correction_corrects(vowel, s):
    """the mean deviation of the shifted vowel's harmonic amplitudes from the formant curve: the corrected shift reads at most half the
    plain shift's, and below 5 dB (float64 restatement: 3.4 / 8.8, 3.5 / 10.4 and 3.2 / 10.7 dB at -4, +4 and +7)"""
    x, sc = vowel
    P, Q = R.plan(s)
    plain = F.envelope_deviation(R.pitch_shift(x, s), P, Q, sc)
    kept = F.envelope_deviation(F.pitch_shift_formant(x, s), P, Q, sc)
    print(f"s={s}: plain {plain:.2f} dB, corrected {kept:.2f} dB ({kept / plain:.2f})")
    assert kept <= 0.5 * plain, (s, kept, plain)
    assert kept < 5.0, (s, kept)


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
def test_phases_are_the_plain_calls(dtype):
    x = R.gpu_items()[2]
    for s in (-4.0, 3.0):
        P, Q = R.plan(s)
        plain, kept = {}, {}
        u0 = R.stretch(x, P, Q, dtype, plain)
        u1 = F.stretch_formant(x, P, Q, dtype, kept)
        assert np.array_equal(plain["phi"], kept["phi"]) and np.array_equal(plain["m"], kept["m"])
        assert u0.shape == u1.shape and not np.array_equal(u0, u1)
        assert not np.array_equal(kept["mf"], kept["m"])


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
def test_gain_properties(dtype):
    rng = np.random.default_rng(5)
    for P, Q in ((1189, 1000), (1, 2), (2, 1), (1999, 1000), (63, 50)):
        g = F.gains(np.zeros((2, R.NB)), P, Q, dtype)
        assert g.dtype == dtype and (g == 1).all(), (P, Q)  # a frame of exact zeros: exactly 1
        assert (F.gains(np.full(R.NB, 3.5), P, Q, dtype) == 1).all()  # ... and any constant row
        # rows whose envelope would ask for far more than 30 dB: steps of 1e6 across the spectrum
        mag = np.where(rng.uniform(size=(4, R.NB)) < 0.5, 1e-3, 1e3) * np.repeat(np.where(np.arange(19) % 2, 1e-3, 1.0), 27)[None, :]
        mag = np.concatenate([mag, np.abs(rng.standard_normal((4, R.NB)))])
        g = F.gains(mag, P, Q, dtype)
        lo, hi = np.exp(dtype(-F.G_MAX)), np.exp(dtype(F.G_MAX))
        assert np.isfinite(g).all() and g.min() >= lo and g.max() <= hi, (P, Q, g.min(), g.max())
        assert (g[:, 0] == 1).all()  # bin 0 stays where it is
    assert hi == pytest.approx(10 ** 1.5, rel=1e-6)
    # at +12 every bin from n/4 on lands at or beyond n/2: clamped
    cl = F.kappa_clamped(2, 1)
    assert cl[256:].all() and not cl[:256].any()
    assert not F.kappa_clamped(1, 2).any() and F.kappa_clamped(1189, 1000)[431:].all() and not F.kappa_clamped(1189, 1000)[:431].any()
    # where the position is clamped the envelope is read at n/2: every clamped bin k gets e(n/2) - e(k)
    mag = np.abs(rng.standard_normal((1, R.NB))) + 0.1
    g = F.gains(mag, 2, 1, np.float64)[0]
    assert g[512] == pytest.approx(1.0, abs=1e-12)


def test_float32_restatement_against_float64():
    """the yardstick of the GPU tests: how far an fp32 implementation of the same definition sits from float64, per item and shift"""
    for s in R.GPU_SEMITONES:
        P, Q = R.plan(s)
        for b, v in enumerate(R.gpu_items()):
            r64, r32 = {}, {}
            y64 = F.pitch_shift_formant(v, s, np.float64, r64)
            y32 = F.pitch_shift_formant(v, s, np.float32, r32)
            assert y32.dtype == np.float32 and r32["gain"].dtype == np.float32
            dy = float(np.abs(y32.astype(np.float64) - y64).max())
            dg = float(np.abs(r32["gain"].astype(np.float64) / r64["gain"] - 1).max())
            print(f"s={s} item {b} ({v.shape[0]} samples): y {dy:.3g}, gain (relative) {dg:.3g}")
            assert np.isfinite(dy) and dy < 1e-5, (s, b, dy)
            assert np.isfinite(dg)
            assert np.array_equal(r32["phi"].shape, r64["phi"].shape)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def test_header_flags_and_constants(tmp_path):
    from vosk_tts_amd import capi, capi_stts

    # the three doors have the signature of vits_op_pitch_shift, as C sees it (compiled, not linked)
    lines = ['#include "vits_pitch.h"', 'typedef int (*door)(int, const float*, const int64_t*, int32_t, int64_t, float, float*);',
             'door doors[] = {vits_op_pitch_shift, vits_op_pitch_shift_formant, vits_op_pitch_stretch_formant, vits_op_pitch_formant_gain};']
    src = tmp_path / "c.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "c.o"), str(src)])
    # the constants, from the preprocessor
    pre = tmp_path / "p.c"
    pre.write_text('#include "vits_pitch.h"\nA VITS_FLAG_PITCH_FORMANT STTS_FLAG_PITCH_FORMANT VITS_PITCH_LIFTER VITS_PITCH_FORMANT_MAX_DB VITS_PITCH_LOG_FLOOR\n')
    out = subprocess.check_output(["gcc", "-E", "-P", "-I", os.path.join(ROOT, "include"), str(pre)], text=True)
    assert out.strip().splitlines()[-1].split() == ["A", "8", "16", "40", "30", "1e-4f"]
    assert capi.FLAG_PITCH_FORMANT == 8 and capi_stts.FLAG_PITCH_FORMANT == capi_stts.STTS_FLAG_PITCH_FORMANT == 16
    assert (F.LIFTER, F.MAX_DB, F.LOG_FLOOR) == (40, 30, 1e-4)
    # no bit of one family is used twice
    assert len({1, 2, capi.FLAG_PITCH, capi.FLAG_PITCH_FORMANT}) == 4
    assert len({1, 2, 4, capi_stts.STTS_FLAG_PITCH, capi_stts.STTS_FLAG_PITCH_FORMANT}) == 5


def test_ctypes_bindings_agree_with_the_header_prototypes(lib):
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "vits_pitch_formant.h")).read(), flags=re.S)
    protos = {m.group(1): [a.strip() for a in m.group(2).split(",")]
              for m in re.finditer(r"\bint\s+(vits_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)}
    assert sorted(protos) == ["vits_op_pitch_formant_gain", "vits_op_pitch_shift_formant", "vits_op_pitch_stretch_formant"]
    for name, args in protos.items():
        fn = getattr(lib.lib, name)
        kinds = ["p" if "*" in a else ("f" if a.startswith("float") else "i") for a in args]
        got = ["f" if t is ctypes.c_float else ("p" if hasattr(t, "contents") or issubclass(t, ctypes._Pointer) else "i") for t in fn.argtypes]
        assert got == kinds, name
    assert '#include "vits_pitch_formant.h"' in open(os.path.join(ROOT, "include", "vits_pitch.h")).read()


def test_doors_refuse_bad_arguments_before_the_device(lib):
    from vosk_tts_amd.capi import VitsError

    x = np.zeros((2, 600), np.float32)
    for door in (lib.op_pitch_shift_formant, lib.op_pitch_stretch_formant, lib.op_pitch_formant_gain):
        with pytest.raises(VitsError, match="601") as e:
            door(x, [600, 601], 3.0)
        assert e.value.code == 1
        with pytest.raises(VitsError, match="12.5") as e:
            door(x, [600, 600], 12.5)
        assert e.value.code == 1
    for door in (lib.op_pitch_stretch_formant, lib.op_pitch_formant_gain):
        with pytest.raises(VitsError, match="identity") as e:
            door(x, [600, 600], 0.0)
        assert e.value.code == 1
    y = lib.op_pitch_shift_formant(np.ones((2, 600), np.float32), [600, 100], 0.0)  # P = Q: a copy, zero beyond the lengths, no device
    assert (y[0] == 1).all() and (y[1, :100] == 1).all() and not y[1, 100:].any()


# ---- Python plumbing ------------------------------------------------------------------------------------------------------------------
def test_model_wrappers_set_the_bit_only_with_a_pitch_in_effect(lib):
    from vosk_tts_amd import capi, capi_stts

    m = capi.VitsModel.__new__(capi.VitsModel)
    m.lib = lib
    for p in (None, 0.0, 0.0004):
        opts, _ = m._opts(1, 4, None, None, None, 0, 0, pitch=p, preserve_formants=True)
        assert type(opts) is capi.SynthOpts and opts.flags == 0
    opts, _ = m._opts(1, 4, None, None, None, 0, 0, solo=True, pitch=-2.0, preserve_formants=True)
    assert type(opts) is capi.SynthPitchOpts and opts.flags == 1 | capi.FLAG_PITCH | capi.FLAG_PITCH_FORMANT and opts.pitch_semitones == -2.0
    opts, _ = m._opts(1, 4, None, None, None, 0, 0, pitch=-2.0)
    assert opts.flags == capi.FLAG_PITCH  # the plain shift: the flags of before
    s = capi_stts.SttsModel.__new__(capi_stts.SttsModel)
    s.vlib = lib
    assert type(s._opts_for(None, None, True)) is capi_stts.SttsOpts and type(s._opts_for(None, 0.0, True)) is capi_stts.SttsOpts
    o = s._opts_for(None, 3.0, True)
    assert type(o) is capi_stts.SttsPitchOpts and o.flags == capi_stts.STTS_FLAG_PITCH | capi_stts.STTS_FLAG_PITCH_FORMANT
    assert s._opts_for(None, 3.0).flags == capi_stts.STTS_FLAG_PITCH
    for fn in (capi.VitsModel.synthesize, capi.VitsModel.synthesize_pcm16, capi_stts.SttsModel.synthesize, capi_stts.SttsModel.synthesize_batch):
        assert inspect.signature(fn).parameters["preserve_formants"].default is False


class _Hp:
    sampling_rate, hop_length, bert_dim, n_speakers = 22050, 256, 0, 4


class _EngineStub:
    """stands where capi.VitsModel stands: records the keywords of every engine call"""

    def __init__(self):
        self.hp = _Hp()
        self.calls = []

    def synthesize_pcm16(self, ids, lens, scales, sid, pcm_scale=1.0, seed=0, solo=False, item_seeds=None, sample_rate=None, **kw):
        self.calls.append({k: v for k, v in kw.items() if k in ("pitch", "preserve_formants")})
        B = ids.shape[0]
        return np.zeros((B, 8), np.int16), np.full(B, 8, np.int64)

    def close(self):
        pass


class _LibStub:
    is_device = True
    has_pitch = has_pitch_formant = True

    def __init__(self):
        self.model = _EngineStub()

    def create(self, blob, device):
        return self.model

    def _need_pitch(self):
        pass

    def _need_pitch_formant(self):
        pass


def _feed(**ext):
    return dict({"input": np.ones((1, 5), np.int64), "input_lengths": np.array([5]), "scales": np.array([0.8, 1.0, 0.8], np.float32),
                 "sid": np.array([1])}, **ext)


def test_sessions_take_the_feed_key_and_it_is_a_coalescer_key():
    from vosk_tts_amd import session, session_stts
    from vosk_tts_amd.outopts import Tail
    from vosk_tts_amd.session import VitsSession

    for mod in (session, session_stts):
        assert "vits.pitch_formants" in mod._EXT
    lib = _LibStub()
    sess = VitsSession(b"", lib=lib)
    keys = []
    submit = sess.coalescer.submit
    sess.coalescer.submit = lambda key, *a: (keys.append(key), submit(key, *a))[1]
    sess.run_pcm16(_feed(), 1.0)
    sess.run_pcm16(_feed(**{"vits.pitch_formants": True}), 1.0)  # no pitch: the request it was, the key it had
    sess.run_pcm16(_feed(**{"vits.pitch": 0.0, "vits.pitch_formants": True}), 1.0)
    sess.run_pcm16(_feed(**{"vits.pitch": 2.0}), 1.0)
    sess.run_pcm16(_feed(**{"vits.pitch": 2.0, "vits.pitch_formants": True}), 1.0)
    sess.run_pcm16(_feed(**{"vits.pitch": 2.0, "vits.pitch_formants": False}), 1.0)
    assert lib.model.calls == [{}, {}, {}, {"pitch": 2.0}, {"pitch": 2.0, "preserve_formants": True}, {"pitch": 2.0}]
    assert keys[0] == keys[1] == keys[2] and keys[3] == keys[5] and len({keys[0], keys[3], keys[4]}) == 3  # they do not share a batch
    with pytest.raises(ValueError, match="frames before a chunk"):
        sess.run_stream(None, _feed(**{"vits.pitch": 2.0, "vits.pitch_formants": True}))
    st = session_stts.SttsSession.__new__(session_stts.SttsSession)
    st._lib = lib
    assert Tail.from_feed(lib, {"vits.pitch_formants": True}).kw() == {} and Tail.from_feed(lib, {"vits.pitch": 0.0, "vits.pitch_formants": True}).kw() == {}
    assert Tail.from_feed(lib, {"vits.pitch": -5}).kw() == {"pitch": -5.0}
    assert Tail.from_feed(lib, {"vits.pitch": -5, "vits.pitch_formants": True}).kw() == {"pitch": -5.0, "preserve_formants": True}


def test_synth_takes_the_argument_and_the_config_key():
    from vosk_tts_amd.batching import MultiDeviceSynth
    from vosk_tts_amd.synth import Synth

    class NoModel:
        config = {"inference": {}}

        def __getattr__(self, name):
            raise AssertionError(f"the model was touched ({name})")

    s = Synth.__new__(Synth)
    s.model = NoModel()
    args = {}
    assert s._pitch(args, None, True) is False and args == {}  # no pitch: the feed of before
    assert s._pitch(args, 0.0, True) is False and args == {}
    assert s._pitch(args, 2.0, True) is True and args == {"vits.pitch": 2.0, "vits.pitch_formants": True}
    args = {}
    assert s._pitch(args, 2.0) is True and args == {"vits.pitch": 2.0}
    s.model.config = {"inference": {"pitch_formants": True}}
    args = {}
    assert s._pitch(args, None) is False and args == {}  # a voice may set it for every request
    assert s._pitch(args, 4) and args == {"vits.pitch": 4.0, "vits.pitch_formants": True}
    args = {}
    assert s._pitch(args, 4, False) and args == {"vits.pitch": 4.0}  # an argument overrides the config
    s.model.config = {"inference": {"pitch": -1.5, "pitch_formants": True}}
    args = {}
    assert s._pitch(args, None) and args == {"vits.pitch": -1.5, "vits.pitch_formants": True}
    with pytest.raises(ValueError, match="frames before a chunk"):
        next(s.synth_stream("x", pitch=2.0))
    for fn in (Synth.synth_audio, Synth.synth, MultiDeviceSynth.synth_batch):
        assert "preserve_formants" in inspect.signature(fn).parameters
    assert "preserve_formants" not in inspect.signature(Synth.synth_stream).parameters


def test_cli_has_the_flag():
    from vosk_tts_amd.cli import build_parser

    assert build_parser().parse_args(["-i", "x", "--pitch", "4", "--preserve-formants"]).preserve_formants is True
    assert build_parser().parse_args(["-i", "x", "--pitch", "4"]).preserve_formants is None  # (the voice's config decides)
