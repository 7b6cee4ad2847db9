"""Loudness normalisation (include/vits_loudness.h), the parts that need no GPU: the host-only plan against the float64 restatement
(tests/loudness_ref.py) and the BS.1770-4 table, the restatement's own figures, argument checking and refusals that happen before any
device work, the ABI of the new header, and the check that keeps the GPU tests' inputs away from the gates."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import loudness_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_RATES = (8000, 22050, 48000)  # the rates tests/test_loudness_gpu.py measures at


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert hip_lib.has_loudness, "libvits_mi355.so exports no vits_op_loudness"
    return hip_lib


def _tile():
    text = open(os.path.join(ROOT, "include", "vits_loudness.h")).read()
    return int(re.search(r"#define\s+VITS_LOUDNESS_TILE\s+(\d+)", text).group(1))


@pytest.mark.parametrize("rate", R.RATES)
def test_plan_equals_the_float64_definition(lib, rate):
    sos, hop = lib.loudness_plan(rate)
    assert hop == (rate + 5) // 10 == R.hop(rate)
    assert sos.shape == (2, 6)
    assert np.abs(sos - R.sos(rate)).max() <= 1e-12


def test_plan_at_48k_is_the_bs1770_table(lib):
    sos, hop = lib.loudness_plan(48000)
    got = (sos[0, 0], sos[0, 1], sos[0, 2], sos[0, 4], sos[0, 5], sos[1, 4], sos[1, 5])
    assert np.abs(np.array(got) - np.array(R.BS1770_48K)).max() <= 1e-12
    assert list(sos[1, :3]) == [1.0, -2.0, 1.0] and sos[0, 3] == sos[1, 3] == 1.0
    assert hop == 4800
    assert np.abs(R.sos(48000) - sos).max() <= 1e-12


def test_hop_at_22050_is_odd(lib):
    assert lib.loudness_plan(22050)[1] == 2205


@pytest.mark.parametrize("rate", R.RATES)
def test_restatement_reads_the_reference_sine(rate):
    """1 kHz, amplitude 0.1, mono: -23.01 LUFS; the lower rates differ by the bilinear transform's warping, inside 0.05 LU"""
    L = R.integrated(R.sine(rate, 5 * rate), rate)
    print(f"{rate} Hz: {L:.4f} LUFS")
    assert abs(L - (-23.01)) <= 0.05


def test_restatement_reads_the_tech3341_gating_sequence():
    """mono, 48 kHz: 10 s at -36, 30 s at -23, 20 s at -36 dBFS -> -26.01 within the meter tolerance of EBU Tech 3341"""
    r = 48000
    x = np.concatenate([R.sine(r, 10 * r, 10 ** (-36 / 20)), R.sine(r, 30 * r, 10 ** (-23 / 20)), R.sine(r, 20 * r, 10 ** (-36 / 20))])
    L = R.integrated(x, r)
    print(f"{L:.4f} LUFS")
    assert abs(L - (-26.01)) <= 0.1


def test_restatement_edges():
    assert R.integrated(np.zeros(0), 22050) == -math.inf and R.peak(np.zeros(0)) == 0.0
    assert R.integrated(np.zeros(30000), 22050) == -math.inf
    one = R.integrated(np.array([0.5]), 22050)  # one sample is one block
    assert math.isfinite(one)
    assert R.blocks(R.sine(22050, 4 * 2205 - 1), 22050).shape == (1,) and R.blocks(R.sine(22050, 4 * 2205), 22050).shape == (1,)
    assert R.blocks(R.sine(22050, 5 * 2205 + 7), 22050).shape == (2,)  # the incomplete tail is dropped
    assert R.gain(-math.inf, 0.0, R.LUFS, -19.0, 1.0) == 1.0 and R.gain(-20.0, 0.0, R.PEAK, 0.5) == 1.0
    assert R.gain(-23.0, 0.5, R.LUFS, -3.0, 1.0) == 2.0  # capped: 10 x 0.5 > 1
    assert R.gain(-23.0, 0.5, R.LUFS, -3.0, 0.0) == pytest.approx(10.0)


@pytest.mark.parametrize("rate", GPU_RATES)
def test_gpu_inputs_stay_clear_of_both_gates(rate):
    """The gates are discontinuous: a block whose l_j lies on -70 or on Gamma would flip on rounding.  Every input the GPU tests measure
    keeps every block at least 0.05 LU from both, so those tests skip and retry nothing."""
    tile = _tile()
    x, lens, names = R.op_batch(rate, tile)
    assert sorted(set(lens.tolist())) == sorted(set(R.op_lengths(rate, tile) + [5 * R.hop(rate)]))
    for b, name in enumerate(names):
        assert np.isnan(x[b, lens[b]:]).all() and np.isfinite(x[b, :lens[b]]).all()
        m = R.gate_margin(x[b, :lens[b]], rate)
        assert m >= 0.05, f"{rate} Hz {name}: a block {m:.4f} LU from a gate"
    xn, ln = R.normalize_batch(rate, tile)
    for b in range(xn.shape[0]):
        m = R.gate_margin(xn[b, :ln[b]], rate)
        assert m >= 0.05, f"{rate} Hz normalize item {b}: a block {m:.4f} LU from a gate"


@pytest.mark.parametrize("rate", GPU_RATES)
def test_the_gated_signal_exercises_both_gates(rate):
    h = R.hop(rate)
    L, l, gamma = R.integrated(R.gated_sequence(rate, 7 * h + 3).astype(np.float32), rate, details=True)
    assert l.shape == (4,)
    assert (l <= -70.0).sum() == 2, l                      # the blocks of the 1e-5 hops
    assert ((l > -70.0) & (l <= gamma)).sum() == 1, (l, gamma)  # the block led by the quiet hop
    assert math.isfinite(L)


# ---- argument checking and refusals before any device work ----------------------------------------------------------------------------
def test_loudness_spec():
    from vosk_tts_amd.capi import LOUDNESS_LUFS, LOUDNESS_PEAK, loudness_spec

    assert loudness_spec() is None
    assert loudness_spec(loudness=-19.0) == (LOUDNESS_LUFS, -19.0, 1.0)  # the default ceiling: an int16 result never clips harder
    assert loudness_spec(loudness=-19.0, peak_ceiling=0) == (LOUDNESS_LUFS, -19.0, 0.0)
    assert loudness_spec(peak=0.9) == (LOUDNESS_PEAK, 0.9, 0.0)
    with pytest.raises(ValueError, match="not both"):
        loudness_spec(loudness=-19.0, peak=0.9)
    for kw, word in ((dict(loudness=1.0), "1.0"), (dict(loudness=-71.0), "-71.0"), (dict(peak=0.0), "0.0"), (dict(peak=1.5), "1.5"),
                     (dict(loudness=-19.0, peak_ceiling=-1.0), "-1.0")):
        with pytest.raises(ValueError) as e:
            loudness_spec(**kw)
        assert word in str(e.value)


@pytest.mark.parametrize("rate", (3999, 0, -8000))
def test_plan_refuses_low_rates_by_value(lib, rate):
    from vosk_tts_amd.capi import VitsError

    with pytest.raises(VitsError) as e:
        lib.loudness_plan(rate)
    assert e.value.code == 4 and str(rate) in str(e.value)  # VITS_ERR_UNSUPPORTED
    assert lib.loudness_plan(4000)[1] == 400


@pytest.mark.parametrize("mode,target,ceiling,word", [
    (1, 0.5, 1.0, "0.5"), (1, -70.5, 1.0, "-70.5"), (1, -19.0, -0.25, "-0.25"), (1, float("nan"), 1.0, "nan"),
    (2, 0.0, 0.0, "0"), (2, 1.25, 0.0, "1.25"), (3, 0.5, 0.0, "mode 3"), (0, 0.5, 0.0, "mode 0"),
])
def test_op_refuses_values_out_of_range_by_value(lib, mode, target, ceiling, word):
    """VITS_ERR_ARG naming the value, answered before the device is touched"""
    from vosk_tts_amd.capi import VitsError

    x = np.zeros((1, 100), np.float32)
    with pytest.raises(VitsError) as e:
        lib.op_loudness_normalize(x, [100], 22050, mode, target, ceiling)
    assert e.value.code == 1 and word in str(e.value), str(e.value)


def test_op_refuses_bad_lengths_and_rates_before_the_device(lib):
    from vosk_tts_amd.capi import VitsError

    x = np.zeros((2, 100), np.float32)
    with pytest.raises(VitsError) as e:
        lib.op_loudness(x, [100, 101], 22050)
    assert e.value.code == 1 and "101" in str(e.value)
    with pytest.raises(VitsError) as e:
        lib.op_loudness(x, [100, -1], 22050)
    assert e.value.code == 1
    with pytest.raises(VitsError) as e:
        lib.op_loudness(x, [100, 100], 3000)
    assert e.value.code == 4 and "3000" in str(e.value)


def test_synth_refuses_before_any_session_call():
    """Synth.synth_stream with a target, and both targets at once, raise without touching the model"""
    from vosk_tts_amd.synth import Synth

    class NoModel:
        config = {"inference": {}}

        def __getattr__(self, name):
            raise AssertionError(f"the model was touched ({name})")

    s = Synth.__new__(Synth)
    s.model = NoModel()
    with pytest.raises(ValueError, match="whole utterance"):
        next(s.synth_stream("x", loudness=-19.0))
    with pytest.raises(ValueError, match="whole utterance"):
        next(s.synth_stream("x", peak=0.5))
    with pytest.raises(ValueError, match="not both"):
        s._loudness({}, -19.0, 0.9, None)
    args = {}
    assert s._loudness(args, None, None, None) is False and args == {}
    assert s._loudness(args, -19.0, None, None) is True and args == {"vits.loudness": -19.0}
    args = {}
    s.model.config = {"inference": {"loudness": -16.0, "peak_ceiling": 0.9}}
    assert s._loudness(args, None, None, None) and args == {"vits.loudness": -16.0, "vits.peak_ceiling": 0.9}
    args = {}
    assert s._loudness(args, None, 0.5, None) and args == {"vits.peak": 0.5}  # an argument overrides the config as a whole


def test_cli_has_the_two_flags():
    from vosk_tts_amd.cli import build_parser

    o = build_parser().parse_args(["-i", "x", "--loudness", "-19", "--peak", "0.5"])
    assert o.loudness == -19.0 and o.peak == 0.5
    o = build_parser().parse_args(["-i", "x"])
    assert o.loudness is None and o.peak is None


def test_session_feed_names():
    from vosk_tts_amd import session, session_stts

    for mod in (session, session_stts):
        assert {"vits.loudness", "vits.peak", "vits.peak_ceiling"} <= set(mod._EXT)


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
    text = open(os.path.join(ROOT, "include", "vits_loudness.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = {m.group(1): _kinds(m.group(2).split(","))
              for m in re.finditer(r"\bint\s+(vits_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)}
    assert sorted(protos) == ["vits_loudness_plan", "vits_op_loudness", "vits_op_loudness_normalize"]
    for name, kinds in protos.items():
        fn = getattr(lib.lib, name)  # (exported)
        assert fn.argtypes is not None, name
        assert [_ctypes_kind(t) for t in fn.argtypes] == kinds, name
    assert protos["vits_op_loudness_normalize"] == list("ippiiiiffppp")


def test_header_constants_and_appended_fields(tmp_path):
    """the flags, modes and the tile as C sees them against the Python mirrors; the five fields sit behind the last older field of
    vits_synth_opts and, for the multistream family, behind an unchanged stts_synth_opts in stts_synth_opts_loudness, in the same order;
    the header compiles as C on its own"""
    from vosk_tts_amd import capi, capi_stts

    names = ("loudness_mode", "loudness_target", "loudness_ceiling", "out_loudness", "out_gain")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vits_loudness.h"', 'int main(void) {',
             '  printf("%d %d %d %d %d %d\\n", VITS_FLAG_LOUDNESS, STTS_FLAG_LOUDNESS, VITS_LOUDNESS_LUFS, VITS_LOUDNESS_PEAK, VITS_LOUDNESS_TILE, '
             'VITS_LOUDNESS_MIN_RATE);']
    for s in ("vits_synth_opts", "stts_synth_opts_loudness"):
        lines.append(f'  printf("%zu", sizeof({s}));')
        for n in names:
            lines.append(f'  printf(" %zu", offsetof({s}, {n}));')
        lines.append('  printf("\\n");')
    lines += ['  printf("%zu %zu\\n", sizeof(stts_synth_opts), offsetof(stts_synth_opts_loudness, base));', '  return 0;', '}']
    src = tmp_path / "c.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "c"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    assert [int(v) for v in out[0].split()] == [capi.FLAG_LOUDNESS, capi_stts.STTS_FLAG_LOUDNESS, capi.LOUDNESS_LUFS, capi.LOUDNESS_PEAK, _tile(),
                                                 capi.LOUDNESS_MIN_RATE]
    assert capi.FLAG_LOUDNESS == 2 and capi_stts.STTS_FLAG_LOUDNESS == 4 and capi.LOUDNESS_MIN_RATE == R.MIN_RATE
    for line, cls in ((out[1], capi.SynthOpts), (out[2], capi_stts.SttsLoudnessOpts)):
        v = [int(t) for t in line.split()]
        assert v[0] == ctypes.sizeof(cls)
        assert v[1:] == [getattr(cls, n).offset for n in names]
    fields = [n for n, *_ in capi.SynthOpts._fields_]
    assert fields[-5:] == list(names) and fields[-6] == "bert"
    # the multistream struct itself keeps its size and its last fields; the extension begins with it and adds exactly the five
    assert [int(v) for v in out[3].split()] == [ctypes.sizeof(capi_stts.SttsOpts), 0]
    assert issubclass(capi_stts.SttsLoudnessOpts, capi_stts.SttsOpts)
    assert [n for n, *_ in capi_stts.SttsLoudnessOpts._fields_] == list(names)
    assert [n for n, *_ in capi_stts.SttsOpts._fields_][-1] == "denoiser_filter_length"
    for n, *_ in capi_stts.SttsOpts._fields_:
        assert getattr(capi_stts.SttsLoudnessOpts, n).offset == getattr(capi_stts.SttsOpts, n).offset
