"""The look-ahead peak limiter (include/vits_limit.h), the parts that need no GPU: the restatement's own properties (tests/limit_ref.py),
the host-only plan, argument checking and refusals that happen before any device work, the ABI of the new header, and the check that
keeps the two-pass GPU inputs away from the loudness gates."""
import ctypes
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import limit_ref as R
import loudness_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert hip_lib.has_limit, "libvits_mi355.so exports no vits_op_limit"
    return hip_lib


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def _peaky(n, at, seed=5):
    x = 0.02 * np.random.default_rng(seed).uniform(-1.0, 1.0, n)
    for q in at:
        x[q] = 0.9 * (-1.0) ** q
    return x.astype(np.float32)


def _invariant_cases(W):
    T = R.TILE
    cases = [("peak at sample 0", _peaky(3 * W + 7, [0])), ("peak at the last sample", _peaky(3 * W + 7, [3 * W + 6])),
             ("len 1", _peaky(1, [0])), ("len W", _peaky(W, [W // 2])), ("len W + 1", _peaky(W + 1, [0, W]))]
    for n in (T - 1, T, T + 1, T + W, T + W + 1):
        cases.append((f"len {n}", _peaky(n, [0, n // 2, n // 2 + W + 2, n - 1])))
    return cases


@pytest.mark.parametrize("W", (1, 8, 40))
def test_gain_curve_never_exceeds_the_required_gain(W):
    """s[n] <= r[n], hence g s[n] p[n] <= c.  Exactly, for the definition: steps 3-5 evaluated in rational arithmetic from the float64
    r and a (on the cases of at most 3 W + 7 samples: the rationals of a release grow by 53 bits a sample).  The float64 evaluation
    rounds the mean of W + 1 values, so a run of equal e can come out an ulp above them: there the bound is (W + 2) 2^-53 relative, the
    worst case of W additions and one division.  Measured: 0 on the single-sample peaks of these cases, 2.2e-16 (W = 40) and 6.7e-16
    (W = 110) on gated noise driven 19 dB over the ceiling."""
    rate, c, g = 8000, 0.5, 2.0
    la = W * 1000.0 / rate
    assert R.plan(rate, la, 20.0)[0] == W
    a = R.plan(rate, la, 20.0)[1]
    worst = 0.0
    noise = R.gated_noise(rate, R.TILE + W + 1).astype(np.float32)
    for name, x in _invariant_cases(W) + [("gated noise", noise * np.float32(4.0))]:
        o = R.limit(x, rate, R.SAMPLE, c, la, 20.0, g)
        r, s = o["r"], o["s"]
        assert r.min() < 1.0, name  # the case limits
        worst = max(worst, float((s / r).max()) - 1.0)
        assert np.all(s <= r * (1.0 + (W + 2) * 2.0 ** -53)), name
        assert np.all(np.abs(o["y"]) <= np.float32(c) * (1 + 2.0 ** -22)), name  # |y| <= c to the two fp32 roundings of step 6
        if x.shape[0] > 3 * W + 7:
            continue
        # exactly: Fractions of the same r and a
        fa, one = Fraction(a), Fraction(1)
        fr = [Fraction(float(v)) for v in r]
        rp = [one] * W + fr + [one] * W
        e, v = [], one
        for k in range(len(fr) + W):
            v = min(min(rp[k:k + W + 1]), fa * v + (one - fa))
            e.append(v)
        run = sum(e[:W + 1])
        for n in range(len(fr)):
            assert run <= (W + 1) * fr[n], (name, n)
            if n + 1 < len(fr):
                run += e[n + W + 1] - e[n]
    print(f"W {W}: max s / r - 1 in float64 = {worst:.2e}")


@pytest.mark.parametrize("W", (1, 40))
def test_release_by_composition_equals_the_recurrence(W):
    """the tile-composite form ((A, B, C) per block of 8, per tile, then the carries) against the sequential recurrence"""
    rate, la = 8000, W * 1000.0 / 8000
    a = R.plan(rate, la, 20.0)[1]
    for name, x in _invariant_cases(W)[-5:] + [("three tiles", _peaky(3 * R.TILE + 5, [0, 100, 2047, 2048, 4000, 6148]))]:
        m = R.lookahead_min(R.required(np.abs(x), 0.5, 2.0), W)
        seq, scan = R.release(m, a), R.release_scan(m, a)
        assert np.abs(scan / seq - 1.0).max() <= 1e-14, name


@pytest.mark.parametrize("rate", R.RATES)
def test_true_peak_mode_holds_the_true_peak(rate):
    """gated noise driven 10 dB above the level at which it first limits, c = 0.9: the output's true peak in TRUE mode is within 1 % of c
    and below what SAMPLE mode leaves (a trial gave 0.9004-0.9014 against 1.34-1.37)"""
    c = 0.9
    x = R.gated_noise(rate, int(1.2 * rate)).astype(np.float32)
    g = c / float(np.abs(x).max()) * 10.0 ** (10.0 / 20.0)
    tp = {mode: R.true_peak(R.limit(x, rate, mode, c, 5.0, 50.0, g)["y"], rate) for mode in (R.SAMPLE, R.TRUE)}
    print(f"{rate} Hz: output true peak {tp[R.TRUE]:.4f} in TRUE mode, {tp[R.SAMPLE]:.4f} in SAMPLE mode (c = {c})")
    assert tp[R.TRUE] < tp[R.SAMPLE]
    assert abs(tp[R.TRUE] / c - 1.0) <= 0.01


@pytest.mark.parametrize("rate", (8000, 22050))
def test_two_pass_inputs_keep_clear_of_the_gates(rate):
    """no block of x or of the restatement's y_0 lies within 0.05 LU of either gate, for every two-pass input of tests/test_limit_gpu.py
    (the rule of tests/test_loudness.py), so no GPU case is skipped or retried; and the items do what the GPU test says they do"""
    x, lens = R.two_pass_items(rate)
    for mode in (R.SAMPLE, R.TRUE):
        for b in range(x.shape[0]):
            xi = x[b, :lens[b]]
            o = R.loudness_limit(xi, rate, R.TWO_PASS_TARGET, mode, R.TWO_PASS_CEILING, 5.0, 50.0)
            for name, sig in (("x", xi), ("y_0", o["y0"])):
                m = loudness_ref.gate_margin(sig, rate)
                assert m > 0.05, f"{rate} Hz mode {mode} item {b}: a block of {name} lies {m:.4f} LU from a gate"
            if b == 0:
                assert o["reduction"] < 0.9 and o["g1"] > o["g0"]
                assert abs(loudness_ref.integrated(o["y"], rate) - R.TWO_PASS_TARGET) < abs(o["L0"] - R.TWO_PASS_TARGET)  # pass 2 is nearer
            else:
                assert o["reduction"] == 1.0 and o["g1"] == o["g0"]


# ---- the plan and refusals before any device work ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,la,rel", [(8000, 5.0, 50.0), (22050, 5.0, 50.0), (48000, 5.0, 50.0), (8000, 0.125, 1.0), (102400, 10.0, 1000.0),
                                         (22050, 0.3, 20.0)])
def test_plan_equals_the_definition(lib, rate, la, rel):
    W, a = lib.limit_plan(rate, la, rel)
    Wr, ar = R.plan(rate, la, rel)
    assert W == Wr and abs(a - ar) <= 1e-15
    assert 1 <= W <= R.MAX_LOOKAHEAD and 0.0 < a < 1.0


def test_plan_values(lib):
    assert lib.limit_plan(22050, 5.0, 50.0)[0] == 110 and lib.limit_plan(48000, 5.0, 50.0)[0] == 240
    assert lib.limit_plan(102400, 10.0, 50.0)[0] == 1024
    assert abs(lib.limit_plan(8000, 5.0, 50.0)[1] - math.exp(-1.0 / 400.0)) <= 1e-15


@pytest.mark.parametrize("kw,code,word", [
    (dict(ceiling=0.0), 1, "ceiling 0"), (dict(ceiling=1.5), 1, "ceiling 1.5"), (dict(ceiling=float("nan")), 1, "ceiling nan"),
    (dict(lookahead_ms=0.0), 1, "lookahead 0"), (dict(lookahead_ms=11.0), 1, "lookahead 11"), (dict(release_ms=0.5), 1, "release 0.5"),
    (dict(release_ms=2000.0), 1, "release 2000"), (dict(gain=-1.0), 1, "gain -1"), (dict(gain=65.0), 1, "gain 65"), (dict(mode=3), 1, "mode 3"),
    (dict(mode=0), 1, "mode 0"), (dict(lookahead_ms=10.0, rate=200000), 4, "W = 2000"), (dict(lookahead_ms=0.01), 4, "W = 0"),
])
def test_op_refuses_values_out_of_range_by_value(lib, kw, code, word):
    """VITS_ERR_ARG naming the value (VITS_ERR_UNSUPPORTED naming W), answered before the device is touched"""
    from vosk_tts_amd.capi import VitsError

    a = dict(rate=8000, mode=R.SAMPLE, ceiling=0.9, lookahead_ms=5.0, release_ms=50.0, gain=1.0)
    a.update(kw)
    x = np.zeros((1, 64), np.float32)
    for door in ("op_limit", "op_limit_gain"):
        with pytest.raises(VitsError) as e:
            getattr(lib, door)(x, [64], a["rate"], a["mode"], a["ceiling"], a["lookahead_ms"], a["release_ms"], a["gain"])
        assert e.value.code == code and word in str(e.value), str(e.value)
    if "gain" not in kw:
        with pytest.raises(VitsError) as e:
            lib.op_loudness_limit(x, [64], a["rate"], -16.0, a["mode"], a["ceiling"], a["lookahead_ms"], a["release_ms"])
        assert e.value.code == code and word in str(e.value), str(e.value)


def test_op_refuses_bad_targets_lengths_and_rates_before_the_device(lib):
    from vosk_tts_amd.capi import VitsError

    x = np.zeros((2, 100), np.float32)
    for args, code, word in (((x, [100, 101], 22050, R.SAMPLE, 0.9), 1, "101"), ((x, [100, -1], 22050, R.SAMPLE, 0.9), 1, "-1")):
        with pytest.raises(VitsError) as e:
            lib.op_limit(*args)
        assert e.value.code == code and word in str(e.value)
    with pytest.raises(VitsError) as e:
        lib.op_true_peak(x, [100, 101], 22050)
    assert e.value.code == 1 and "101" in str(e.value)
    with pytest.raises(VitsError) as e:
        lib.op_loudness_limit(x, [100, 100], 22050, 0.5, R.TRUE, 0.9)
    assert e.value.code == 1 and "0.5" in str(e.value)  # the LUFS target, by the loudness rule
    with pytest.raises(VitsError) as e:
        lib.op_loudness_limit(x, [100, 100], 3000, -16.0, R.TRUE, 0.9)
    assert e.value.code == 4 and "3000" in str(e.value)  # the loudness kernels' lowest rate


def test_limit_spec():
    from vosk_tts_amd.capi import LIMIT_SAMPLE, LIMIT_TRUE, limit_spec

    assert limit_spec() is None and limit_spec(None, 0.5) is None
    assert limit_spec("true") == (LIMIT_TRUE, 1.0, 5.0, 50.0, 1.0)
    assert limit_spec("sample", 0.89, 2.0, 100.0, 3.0) == (LIMIT_SAMPLE, 0.89, 2.0, 100.0, 3.0)
    for args, word in ((("peak",), "'peak'"), (("true", 0.0), "0.0"), (("true", 1.5), "1.5"), (("true", 0.9, 0.0), "0.0"), (("true", 0.9, 10.5), "10.5"),
                       (("true", 0.9, 5.0, 0.5), "0.5"), (("true", 0.9, 5.0, 1001.0), "1001.0"), (("true", 0.9, 5.0, 50.0, 65.0), "65.0"),
                       (("true", float("nan")), "nan")):
        with pytest.raises(ValueError) as e:
            limit_spec(*args)
        assert word in str(e.value)


def test_synth_refuses_before_any_session_call():
    """Synth.synth_stream with a limiter, a peak target next to one and values out of range raise without touching the model"""
    from vosk_tts_amd.synth import Synth

    class NoModel:
        config = {"inference": {}}

        def __getattr__(self, name):
            raise AssertionError(f"the model was touched ({name})")

    s = Synth.__new__(Synth)
    s.model = NoModel()
    with pytest.raises(ValueError, match="whole utterance"):
        next(s.synth_stream("x", limit="true"))
    args = {}
    assert s._limit(args, None) is False and args == {}
    assert s._limit(args, "true", 0.89) is True
    assert args == {"vits.limit": "true", "vits.limit_lookahead_ms": 5.0, "vits.limit_release_ms": 50.0, "vits.peak_ceiling": 0.89}
    with pytest.raises(ValueError, match="peak"):
        s._limit({"vits.peak": 0.5}, "true")
    with pytest.raises(ValueError, match="12.0"):
        s._limit({}, "sample", None, 12.0)
    s.model.config = {"inference": {"limit": "sample", "limit_lookahead_ms": 2.0, "limit_release_ms": 80.0, "peak_ceiling": 0.9}}
    args = {}
    assert s._limit(args, None) and args == {"vits.limit": "sample", "vits.limit_lookahead_ms": 2.0, "vits.limit_release_ms": 80.0,
                                              "vits.peak_ceiling": 0.9}


def test_sessions_read_the_feeds_before_any_device_work():
    """the feed names, and what the two session types make of them: with a limiter the loudness gain has no cap and "vits.peak_ceiling" is
    the limiter's ceiling"""
    from vosk_tts_amd import session, session_stts
    from vosk_tts_amd.capi import LIMIT_TRUE, LOUDNESS_LUFS
    from vosk_tts_amd.outopts import Tail

    class Lib:
        has_limit = has_loudness = True

        def _need_limit(self):
            pass

        def _need_loudness(self):
            pass

    for mod, cls in ((session, session.VitsSession), (session_stts, session_stts.SttsSession)):
        assert {"vits.limit", "vits.limit_lookahead_ms", "vits.limit_release_ms"} <= set(mod._EXT)
        s = cls.__new__(cls)
        s._lib = Lib()
        feed = {"vits.loudness": -16.0, "vits.peak_ceiling": 0.89, "vits.limit": "true", "vits.limit_release_ms": 80.0}
        assert Tail.from_feed(s._lib, feed).limit == (LIMIT_TRUE, 0.89, 5.0, 80.0, 1.0)
        assert Tail.from_feed(s._lib, feed).loudness == (LOUDNESS_LUFS, -16.0, 0.0)
        assert Tail.from_feed(s._lib, {"vits.loudness": -16.0}).limit is None and Tail.from_feed(s._lib, {"vits.loudness": -16.0, "vits.peak_ceiling": 0.89}).loudness[2] == 0.89
        with pytest.raises(ValueError, match="vits.peak"):
            Tail.from_feed(s._lib, {"vits.limit": "sample", "vits.peak": 0.5})
        with pytest.raises(ValueError, match="bogus"):
            Tail.from_feed(s._lib, {"vits.limit": "bogus"})


def test_cli_has_the_flag():
    from vosk_tts_amd.cli import build_parser

    assert build_parser().parse_args(["-i", "x", "--limit", "true", "--loudness", "-16"]).limit == "true"
    assert build_parser().parse_args(["-i", "x", "--limit", "sample"]).limit == "sample"
    assert build_parser().parse_args(["-i", "x"]).limit is None
    with pytest.raises(SystemExit):
        build_parser().parse_args(["-i", "x", "--limit", "peak"])


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def _kinds(args):
    out = []
    for a in args:
        a = a.strip()
        out.append("p" if ("*" in a or "[" in a) else ("f" if re.match(r"(const\s+)?(float|double)\b", a) else "i"))
    return out


def _ctypes_kind(t):
    if t in (ctypes.c_float, ctypes.c_double):
        return "f"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or hasattr(t, "contents") or issubclass(t, ctypes._Pointer):
        return "p"
    return "i"


def test_ctypes_bindings_agree_with_the_header_prototypes(lib):
    text = open(os.path.join(ROOT, "include", "vits_limit.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = {m.group(1): _kinds(m.group(2).split(","))
              for m in re.finditer(r"\bint\s+(vits_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)}
    assert sorted(protos) == ["vits_limit_plan", "vits_op_limit", "vits_op_limit_gain", "vits_op_loudness_limit", "vits_op_true_peak"]
    for name, kinds in protos.items():
        fn = getattr(lib.lib, name)  # (exported)
        assert fn.argtypes is not None, name
        assert [_ctypes_kind(t) for t in fn.argtypes] == kinds, name
    assert protos["vits_op_limit"] == list("ippiiiiffffpp") and protos["vits_op_loudness_limit"] == list("ippiiififffpppp")


def test_header_constants_and_the_two_new_structs(tmp_path):
    """the flags, modes and sizes as C sees them against the Python mirrors; the six fields sit behind an unchanged vits_synth_opts_pitch /
    stts_synth_opts_pitch, in the same order; the header compiles as C on its own"""
    from vosk_tts_amd import capi, capi_stts

    names = ("limit_mode", "limit_ceiling", "limit_lookahead_ms", "limit_release_ms", "limit_gain", "out_reduction")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vits_limit.h"', 'int main(void) {',
             '  printf("%d %d %d %d %d %d %d %d\\n", VITS_FLAG_LIMIT, STTS_FLAG_LIMIT, VITS_LIMIT_SAMPLE, VITS_LIMIT_TRUE, VITS_LIMIT_TILE, '
             'VITS_LIMIT_MAX_LOOKAHEAD, VITS_LIMIT_OVERSAMPLE, VITS_LIMIT_PASSES);']
    for s, base in (("vits_synth_opts_limit", "vits_synth_opts_pitch"), ("stts_synth_opts_limit", "stts_synth_opts_pitch")):
        lines.append(f'  printf("%zu %zu %zu", sizeof({s}), sizeof({base}), offsetof({s}, base));')
        for n in names:
            lines.append(f'  printf(" %zu", offsetof({s}, {n}));')
        lines.append('  printf("\\n");')
    lines += ['  return 0;', '}']
    src = tmp_path / "c.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "c"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    assert [int(v) for v in out[0].split()] == [capi.FLAG_LIMIT, capi_stts.STTS_FLAG_LIMIT, capi.LIMIT_SAMPLE, capi.LIMIT_TRUE, capi.LIMIT_TILE,
                                                 capi.LIMIT_MAX_LOOKAHEAD, 4, 2]
    assert (capi.FLAG_LIMIT, capi_stts.STTS_FLAG_LIMIT) == (16, 32) and (capi.LIMIT_TILE, capi.LIMIT_MAX_LOOKAHEAD) == (R.TILE, R.MAX_LOOKAHEAD)
    for line, cls, base in ((out[1], capi.SynthLimitOpts, capi.SynthPitchOpts), (out[2], capi_stts.SttsLimitOpts, capi_stts.SttsPitchOpts)):
        v = [int(t) for t in line.split()]
        assert v[0] == ctypes.sizeof(cls) and v[1] == ctypes.sizeof(base) and v[2] == 0
        assert v[3:] == [getattr(cls, n).offset for n in names]
        assert issubclass(cls, base) and [n for n, *_ in cls._fields_] == list(names)
        for n, *_ in base._fields_:  # the older fields where they were
            assert getattr(cls, n).offset == getattr(base, n).offset
    # no flag bit is used twice
    flags = [1, capi.FLAG_LOUDNESS, capi.FLAG_PITCH, capi.FLAG_PITCH_FORMANT, capi.FLAG_LIMIT]
    assert len(set(flags)) == len(flags) and all(f & (f - 1) == 0 for f in flags)
    sflags = [capi_stts.STTS_FLAG_ITEM_SEEDS, capi_stts.STTS_FLAG_DENOISE, capi_stts.STTS_FLAG_LOUDNESS, capi_stts.STTS_FLAG_PITCH,
              capi_stts.STTS_FLAG_PITCH_FORMANT, capi_stts.STTS_FLAG_LIMIT]
    assert len(set(sflags)) == len(sflags) and all(f & (f - 1) == 0 for f in sflags)
