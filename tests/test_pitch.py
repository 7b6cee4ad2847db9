"""Pitch-shifted output (include/vits_pitch.h), the parts that need no GPU: the float64 restatement's own properties (tests/pitch_ref.py),
the host-only plan, the length rule, the ABI of the new header, the Python plumbing through stub sessions, and the check that keeps the
GPU tests' inputs away from the one discontinuous step, the peak picking."""
import ctypes
import math
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import pitch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P0_SWEEP = (500, 501, 667, 749, 999, 1001, 1189, 1498, 1999, 2000)


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert hip_lib.has_pitch, "libvits_mi355.so exports no vits_op_pitch_shift"
    return hip_lib


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", (-12.0, -3.0, 4.0, 12.0))
def test_restatement_shifts_a_sine_and_keeps_its_level(s):
    P, Q = R.plan(s)
    y = R.pitch_shift(R.sine(), s, np.float64)
    assert y.shape == (16384,)
    peak, rms = R.sine_figures(y)
    assert abs(peak - 440.0 * P / Q * 8192 / 22050) <= 1.0, peak
    assert abs(rms - 0.3 / math.sqrt(2)) <= 0.01 * 0.3 / math.sqrt(2), rms  # (the plain vocoder returns a tenth of it)


def test_zero_is_the_identity():
    assert R.plan(0.0) == (1, 1) and R.plan(0.0004) == (1, 1)
    x = R.sine(2048)
    assert np.array_equal(R.pitch_shift(x, 0.0, np.float32), x)
    short = R.sine(512)
    assert np.array_equal(R.pitch_shift(short, 5.0, np.float32), short)  # below n/2 + 1: unshifted


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def test_plan_equals_the_python_formula(lib):
    from vosk_tts_amd.capi import pitch_ratio

    for s in np.concatenate([np.linspace(-12, 12, 481), [0.0, 0.01, -0.01, 11.999, -11.999]]):
        s32 = float(np.float32(s))  # (the C entry takes a float)
        assert lib.pitch_plan(s32) == R.plan(s32) == pitch_ratio(s32), s
    assert lib.pitch_plan(12.0) == (2, 1) and lib.pitch_plan(-12.0) == (1, 2) and lib.pitch_plan(0.0) == (1, 1)
    assert lib.pitch_plan(3.0) == (1189, 1000)


@pytest.mark.parametrize("s,word", ((12.5, "12.5"), (-12.25, "-12.25"), (float("nan"), "nan"), (float("inf"), "inf")))
def test_plan_refuses_values_out_of_range_by_value(lib, s, word):
    from vosk_tts_amd.capi import VitsError, pitch_ratio

    with pytest.raises(VitsError) as e:
        lib.pitch_plan(s)
    assert e.value.code == 1 and word in str(e.value)  # VITS_ERR_ARG
    with pytest.raises(ValueError, match=word):
        pitch_ratio(s)
    with pytest.raises(ValueError, match=word):
        R.plan(s)
    x = np.zeros((1, 600), np.float32)
    with pytest.raises(VitsError) as e:  # the doors refuse the same values before the device is touched
        lib.op_pitch_shift(x, [600], s)
    assert e.value.code == 1 and word in str(e.value)


def test_every_ratio_fits_the_resampler_table(lib):
    """all 1501 values of P0: the resampler P -> Q has a plan, and its table stays inside VITS_RESAMPLE_MAX_TABLE"""
    worst = 0
    for p0 in range(500, 2001):
        g = math.gcd(p0, 1000)
        P, Q = p0 // g, 1000 // g
        if P == Q:
            continue
        pl = lib.resample_plan(P, Q)
        assert (pl["L"], pl["M"]) == (Q, P)
        worst = max(worst, pl["L"] * pl["taps"])
    assert worst <= 65536
    pl = lib.resample_plan(1999, 1000)
    assert pl["L"] == 1000 and pl["taps"] <= 65


def test_doors_refuse_bad_arguments_before_the_device(lib):
    from vosk_tts_amd.capi import VitsError

    x = np.zeros((2, 600), np.float32)
    with pytest.raises(VitsError, match="601") as e:
        lib.op_pitch_shift(x, [600, 601], 3.0)
    assert e.value.code == 1
    with pytest.raises(VitsError, match="identity") as e:
        lib.op_pitch_stretch(x, [600, 600], 0.0)
    assert e.value.code == 1
    y = lib.op_pitch_shift(np.ones((2, 600), np.float32), [600, 100], 0.0)  # P = Q: a copy, zero beyond the lengths, no device
    assert (y[0] == 1).all() and (y[1, :100] == 1).all() and not y[1, 100:].any()


# ---- the length rule ----------------------------------------------------------------------------------------------------------------
def test_the_resampled_stretch_covers_the_item():
    for p0 in P0_SWEEP:
        g = math.gcd(p0, 1000)
        P, Q = p0 // g, 1000 // g
        for n in range(513, 5121):
            assert R.n_v(n, P, Q) >= R.HOP * (n // R.HOP), (p0, n)
            assert R.n_u(n, P, Q) <= R.stretch_samples(n, P, Q)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def test_header_layout_and_flags(tmp_path):
    from vosk_tts_amd import capi, capi_stts

    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vits_pitch.h"', 'int main(void) {',
             '  printf("%d %d %d %d\\n", VITS_FLAG_PITCH, STTS_FLAG_PITCH, VITS_PITCH_FRAME, VITS_PITCH_MAX_SEMITONES);']
    for s in ("vits_synth_opts_pitch", "stts_synth_opts_pitch"):
        lines.append(f'  printf("%zu %zu %zu\\n", sizeof({s}), offsetof({s}, base), offsetof({s}, pitch_semitones));')
    lines += ['  printf("%zu %zu\\n", sizeof(vits_synth_opts), sizeof(stts_synth_opts_loudness));', '  return 0;', '}']
    src = tmp_path / "c.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "c"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [[int(v) for v in line.split()] for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert out[0] == [4, 8, 1024, 12]
    assert capi.FLAG_PITCH == 4 and capi_stts.STTS_FLAG_PITCH == 8 and capi.PITCH_FRAME == R.FRAME == 1024
    assert capi.PITCH_MAX_SEMITONES == R.MAX_SEMITONES == 12
    for row, cls, base in ((out[1], capi.SynthPitchOpts, capi.SynthOpts), (out[2], capi_stts.SttsPitchOpts, capi_stts.SttsLoudnessOpts)):
        assert row == [ctypes.sizeof(cls), 0, cls.pitch_semitones.offset]
        assert issubclass(cls, base) and [n for n, *_ in cls._fields_] == ["pitch_semitones"]
        assert cls.pitch_semitones.offset >= ctypes.sizeof(base)
        for n, *_ in base._fields_:  # base at offset 0: every older field where it was
            assert getattr(cls, n).offset == getattr(base, n).offset
    assert out[3] == [ctypes.sizeof(capi.SynthOpts), ctypes.sizeof(capi_stts.SttsLoudnessOpts)]  # neither older struct grew


def test_ctypes_bindings_agree_with_the_header_prototypes(lib):
    import re

    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "vits_pitch.h")).read(), flags=re.S)
    protos = {m.group(1): [a.strip() for a in m.group(2).split(",")]
              for m in re.finditer(r"\bint\s+(vits_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)}
    assert sorted(protos) == ["vits_op_pitch_shift", "vits_op_pitch_stretch", "vits_pitch_plan"]
    for name, args in protos.items():
        fn = getattr(lib.lib, name)
        kinds = ["p" if "*" in a else ("f" if a.startswith("float") else "i") for a in args]
        got = ["f" if t is ctypes.c_float else ("p" if hasattr(t, "contents") or issubclass(t, ctypes._Pointer) else "i") for t in fn.argtypes]
        assert got == kinds, name


# ---- Python plumbing ------------------------------------------------------------------------------------------------------------------
class _Hp:
    sampling_rate, hop_length, bert_dim, n_speakers = 22050, 256, 0, 4


class _EngineStub:
    """stands where capi.VitsModel stands: records (items, pitch keyword) per engine call; the first call waits for `gate`"""

    def __init__(self):
        self.hp = _Hp()
        self.calls = []
        self.gate = threading.Event()
        self.entered = threading.Event()
        self._lock = threading.Lock()

    def synthesize_pcm16(self, ids, lens, scales, sid, pcm_scale=1.0, seed=0, solo=False, item_seeds=None, sample_rate=None, **kw):
        with self._lock:
            first = not self.calls
            self.calls.append((ids.shape[0], kw.get("pitch"), "pitch" in kw))
        if first:
            self.entered.set()
            assert self.gate.wait(30)
        B = ids.shape[0]
        return np.full((B, 8), int(round(10 * (kw.get("pitch") or 0))), np.int16), np.full(B, 8, np.int64)

    def close(self):
        pass


class _LibStub:
    is_device = True
    has_pitch = True

    def __init__(self):
        self.model = _EngineStub()

    def create(self, blob, device):
        return self.model

    def _need_pitch(self):
        pass

    def _need_loudness(self):
        pass


def _feed(**ext):
    return dict({"input": np.ones((1, 5), np.int64), "input_lengths": np.array([5]), "scales": np.array([0.8, 1.0, 0.8], np.float32),
                 "sid": np.array([1])}, **ext)


def test_coalescer_never_mixes_shifts_and_an_unshifted_request_is_the_call_it_was():
    from vosk_tts_amd.session import VitsSession

    lib = _LibStub()
    sess = VitsSession(b"", lib=lib, max_inflight=1)
    eng = lib.model
    shifts = [None, 2.0, -3.0, 2.0, 0.0, 2.0, -3.0, None]  # (0.0 reduces to P = Q: the same key as None)
    results = [None] * len(shifts)

    def worker(i):
        ext = {} if shifts[i] is None else {"vits.pitch": shifts[i]}
        results[i] = sess.run_pcm16(_feed(**ext), 1.0, return_lengths=True)[0]

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(len(shifts))]
    threads[0].start()
    assert eng.entered.wait(30)
    for t in threads[1:]:
        t.start()
    deadline = time.monotonic() + 30
    while len(sess.coalescer._queue) < len(shifts) - 1 and time.monotonic() < deadline:
        time.sleep(0.001)
    assert len(sess.coalescer._queue) == len(shifts) - 1
    eng.gate.set()
    for t in threads:
        t.join(30)
    for s, out in zip(shifts, results):
        assert out is not None and (out == int(round(10 * (s or 0)))).all(), (s, out)
    assert sorted(set(c[1] for c in eng.calls), key=lambda v: (v is not None, v)) == [None, -3.0, 2.0]
    assert sess.coalescer.calls < len(shifts) and max(c[0] for c in eng.calls) > 1
    # without a shift the engine is called with the keywords it was called with before: no pitch keyword at all
    assert all(not has for _, p, has in eng.calls if p is None)


def test_session_feed_names_and_refusals():
    from vosk_tts_amd import session, session_stts
    from vosk_tts_amd.outopts import Tail
    from vosk_tts_amd.session import VitsSession

    for mod in (session, session_stts):
        assert "vits.pitch" in mod._EXT
    lib = _LibStub()
    sess = VitsSession(b"", lib=lib)
    with pytest.raises(ValueError, match="13"):
        sess.run_pcm16(_feed(**{"vits.pitch": 13.0}), 1.0)
    with pytest.raises(ValueError, match="frames before a chunk"):
        sess.run_stream(None, _feed(**{"vits.pitch": 2.0}))
    assert lib.model.calls == []
    # the multistream session: the same key, turned into the model's keyword; nothing for no shift
    st = session_stts.SttsSession.__new__(session_stts.SttsSession)
    st._lib = lib
    assert Tail.from_feed(lib, {}).kw() == {} and Tail.from_feed(lib, {"vits.pitch": 0.0}).kw() == {} and Tail.from_feed(lib, {"vits.pitch": -5}).kw() == {"pitch": -5.0}
    with pytest.raises(ValueError, match="-12.5"):
        Tail.from_feed(lib, {"vits.pitch": -12.5})


def test_synth_takes_pitch_and_the_config_key_and_streams_refuse():
    from vosk_tts_amd.synth import Synth

    class NoModel:
        config = {"inference": {}}

        def __getattr__(self, name):
            raise AssertionError(f"the model was touched ({name})")

    s = Synth.__new__(Synth)
    s.model = NoModel()
    with pytest.raises(ValueError, match="frames before a chunk"):
        next(s.synth_stream("x", pitch=2.0))
    args = {}
    assert s._pitch(args, None) is False and args == {}  # a request without pitch builds the feed it built before
    assert s._pitch(args, 0.0) is False and args == {}
    assert s._pitch(args, 2.0) is True and args == {"vits.pitch": 2.0}
    with pytest.raises(ValueError, match="12.5"):
        s._pitch({}, 12.5)
    s.model.config = {"inference": {"pitch": -1.5}}
    args = {}
    assert s._pitch(args, None) and args == {"vits.pitch": -1.5}
    args = {}
    assert s._pitch(args, 4) and args == {"vits.pitch": 4.0}  # an argument overrides the config
    import inspect

    for fn in (Synth.synth_audio, Synth.synth, Synth.synth_stream):
        assert "pitch" in inspect.signature(fn).parameters
    from vosk_tts_amd.batching import MultiDeviceSynth

    assert "pitch" in inspect.signature(MultiDeviceSynth.synth_batch).parameters


def test_cli_has_the_flag():
    from vosk_tts_amd.cli import build_parser

    assert build_parser().parse_args(["-i", "x", "--pitch", "-2.5"]).pitch == -2.5
    assert build_parser().parse_args(["-i", "x"]).pitch is None


def test_model_wrappers_pick_the_struct_by_the_request(lib):
    """no shift (or one that reduces to P = Q): the structs of before, flag clear; a shift: the extended struct with the flag"""
    from vosk_tts_amd import capi, capi_stts

    m = capi.VitsModel.__new__(capi.VitsModel)
    m.lib = lib
    for p in (None, 0.0):
        opts, _ = m._opts(1, 4, None, None, None, 0, 0, pitch=p)
        assert type(opts) is capi.SynthOpts and not opts.flags & capi.FLAG_PITCH
    opts, _ = m._opts(1, 4, None, None, None, 0, 0, solo=True, pitch=-2.0)
    assert type(opts) is capi.SynthPitchOpts and opts.flags == 1 | capi.FLAG_PITCH and opts.pitch_semitones == -2.0
    s = capi_stts.SttsModel.__new__(capi_stts.SttsModel)
    s.vlib = lib
    assert type(s._opts_for(None, None)) is capi_stts.SttsOpts and type(s._opts_for((1, -19.0, 1.0), 0.0)) is capi_stts.SttsLoudnessOpts
    o = s._opts_for(None, 3.0)
    assert type(o) is capi_stts.SttsPitchOpts and o.flags == capi_stts.STTS_FLAG_PITCH and o.pitch_semitones == 3.0


# ---- the GPU tests' inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", R.GPU_SEMITONES)
def test_gpu_inputs_keep_their_peaks_apart(s):
    """Peak picking is the one discontinuous step.  For the seeded noise items of tests/test_pitch_gpu.py the smallest gap between two
    magnitudes that a peak test compares (float64 run) is at least 8 times the largest difference between the float32 and the float64
    magnitudes: an fp32 implementation decides every peak as the reference does, and a sample-wise comparison means something.
    (The voiced item cannot meet this -- its noise-floor bins sit 50 dB below harmonics whose rounding error is as large as their gaps
    -- and is not asked to; the figures below are printed for it as well.)"""
    items = R.gpu_items()
    for b, x in enumerate(items):
        r64, r32 = {}, {}
        R.pitch_shift(x, s, np.float64, r64)
        R.pitch_shift(x, s, np.float32, r32)
        err = float(np.abs(r64["m"] - r32["m"].astype(np.float64)).max())
        print(f"s={s} item {b} ({x.shape[0]} samples): min gap {r64['min_gap']:.3g}, |m32 - m64| {err:.3g}, ratio {r64['min_gap'] / err:.1f}")
        if b < 2:
            assert r64["min_gap"] >= 8 * err, (s, b, r64["min_gap"], err)
