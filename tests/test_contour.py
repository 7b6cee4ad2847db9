"""Per-token pitch and volume contours on the CPU (include/vits_contour.h): the header against its ctypes mirrors, the self-checks of the
float64 restatement (tests/contour_ref.py), the frequency property of the definition, and Synth's word-to-token mapping with a stub
model.  The device is checked in tests/test_contour_gpu.py."""
import ctypes
import inspect
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import contour_ref as C
import pitch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_layout_flags_and_export(tmp_path, hip_lib):
    from vosk_tts_amd import capi, capi_stts

    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vits_contour.h"', 'int main(void) {',
             '  printf("%d %d %d %g %g %d %d\\n", VITS_FLAG_CONTOUR, STTS_FLAG_CONTOUR, VITS_CONTOUR_RAMP, (double)VITS_CONTOUR_MIN_DB, '
             '(double)VITS_CONTOUR_MAX_DB, VITS_CONTOUR_TABLE_RES, VITS_PITCH_MAX_SEMITONES);',
             '  printf("%zu %zu %zu %zu\\n", sizeof(vits_synth_opts_contour), offsetof(vits_synth_opts_contour, base), '
             'offsetof(vits_synth_opts_contour, contour), sizeof(vits_synth_opts_prosody));',
             '  printf("%zu %zu %zu %zu\\n", sizeof(stts_synth_opts_contour), offsetof(stts_synth_opts_contour, base), '
             'offsetof(stts_synth_opts_contour, contour), sizeof(stts_synth_opts_limit));',
             '  printf("%zu %zu %zu\\n", sizeof(vits_contour), offsetof(vits_contour, token_semitones), offsetof(vits_contour, token_gain_db));',
             '  printf("%zu %zu %zu %zu %zu\\n", sizeof(vits_synth_opts), sizeof(vits_synth_opts_pitch), sizeof(vits_synth_opts_limit), '
             'sizeof(stts_synth_opts_loudness), sizeof(stts_synth_opts_pitch));',
             '  return 0;', '}']
    src = tmp_path / "c.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "c"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert [float(v) for v in out[0]] == [capi.FLAG_CONTOUR, capi_stts.STTS_FLAG_CONTOUR, capi.CONTOUR_RAMP, *capi.CONTOUR_DB, C.RES,
                                         capi.PITCH_MAX_SEMITONES] == [64, 64, 4, -40, 12, 256, 12]
    assert (C.RAMP, C.MIN_DB, C.MAX_DB) == (capi.CONTOUR_RAMP, *capi.CONTOUR_DB)
    assert [int(v) for v in out[1]] == [ctypes.sizeof(capi.SynthContourOpts), 0, capi.SynthContourOpts.contour.offset, ctypes.sizeof(capi.SynthProsodyOpts)]
    assert [int(v) for v in out[2]] == [ctypes.sizeof(capi_stts.SttsContourOpts), 0, capi_stts.SttsContourOpts.contour.offset,
                                        ctypes.sizeof(capi_stts.SttsLimitOpts)]
    assert [int(v) for v in out[3]] == [ctypes.sizeof(capi.Contour), capi.Contour.token_semitones.offset, capi.Contour.token_gain_db.offset]
    # the older structs did not grow
    assert [int(v) for v in out[4]] == [ctypes.sizeof(t) for t in (capi.SynthOpts, capi.SynthPitchOpts, capi.SynthLimitOpts, capi_stts.SttsLoudnessOpts,
                                                                   capi_stts.SttsPitchOpts)]
    assert issubclass(capi.SynthContourOpts, capi.SynthProsodyOpts) and issubclass(capi_stts.SttsContourOpts, capi_stts.SttsLimitOpts)
    # the flags are free in their families, and the library exports the doors with the binding's argument lists
    assert capi.FLAG_CONTOUR not in (1, capi.FLAG_LOUDNESS, capi.FLAG_PITCH, capi.FLAG_PITCH_FORMANT, capi.FLAG_LIMIT, capi.FLAG_PROSODY)
    assert capi_stts.STTS_FLAG_CONTOUR not in (capi_stts.STTS_FLAG_ITEM_SEEDS, capi_stts.STTS_FLAG_DENOISE, capi_stts.STTS_FLAG_LOUDNESS,
                                               capi_stts.STTS_FLAG_PITCH, capi_stts.STTS_FLAG_PITCH_FORMANT, capi_stts.STTS_FLAG_LIMIT)
    assert hip_lib.has_contour and len(hip_lib._fn("op_contour").argtypes) == 12 and len(hip_lib._fn("op_contour_stretch").argtypes) == 13


# ---- the restatement's own arithmetic --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", (-12.0, -5.0, 3.0, 7.0, 12.0))
def test_positions_of_a_constant_contour_against_fractions(s):
    """a_t against t * 1000 / P in exact rationals: the integer division of inc loses less than 2^-24 frames a step"""
    P = int(C.token_ratios([s])[0])
    Fa = 40
    a, Fs = C.positions(np.full(Fa, P * C.K, np.int64), Fa)
    assert a[0] == 0 and a[Fs - 1] < (Fa + 1) << 24 <= a[Fs] and Fs <= 2 * (Fa + 1)
    slack = Fraction(Fs, 1 << 24)
    for t in range(Fs):
        exact = Fraction(1000 * t, P)
        got = Fraction(int(a[t]), 1 << 24)
        assert exact - slack <= got <= exact
        near = exact - int(exact) < slack or int(exact) + 1 - exact <= slack  # within F_s 2^-24 frames of a boundary
        assert (int(a[t]) >> 24) == (1000 * t) // P or near, (t, a[t])
    assert Fs in (-(-(Fa + 1) * P // 1000), -(-(Fa + 1) * P // 1000) + 1)


def test_steps_are_bounded_and_tau_stays_inside_u():
    rng = np.random.default_rng(0)
    for trial in range(40):
        frames = int(rng.integers(3, 60))
        n_tok = int(rng.integers(1, 9))
        cuts = np.sort(rng.integers(0, frames + 1, size=n_tok - 1))
        cum = np.concatenate([cuts, [frames]]).astype(np.int64)
        st = rng.choice([-12.0, 12.0, 0.0, 5.5, -7.25], size=n_tok)
        length = frames * 256 if trial % 2 == 0 else int(rng.integers(513, frames * 256 + 1))
        if length < C.MIN_LEN:
            continue
        Sigma, gbar = C.tracks(length, cum, n_tok, 256, C.token_ratios(st), C.token_gains(np.zeros(n_tok)))
        Fa = R.frames_a(length)
        assert Sigma.shape == (Fa,) and (Sigma >= 500 * C.K).all() and (Sigma <= 2000 * C.K).all() and (gbar == 1).all()
        a, Fs = C.positions(Sigma, Fa)
        assert Fs <= 2 * (Fa + 1) and (np.diff(a) >= 1 << 23).all() and (np.diff(a) <= 1 << 25).all()
        tau, s = C.warp_positions(a, Fs, length)
        assert (np.diff(tau) > 0).all() and (s > 0).all() and (s <= 1).all()
        if length % 256 == 0:
            assert tau.max() < 256 * (Fs - 1), (trial, tau.max(), Fs)


def test_tracks_ramp_between_tokens_and_neutral_rows_without_a_token():
    P, g = C.token_ratios([12.0, 0.0]), C.token_gains([6.0, 0.0])
    Sigma, gbar = C.tracks(20 * 256, [10, 20], 2, 256, P, g)
    assert Sigma[0] == 2000 * C.K and Sigma[-1] == 1000 * C.K
    assert (np.diff(Sigma[:5]) == 0).all() and (np.diff(Sigma[5:15]) <= 0).all() and Sigma[10] == 2000 * 4 + 1000 * 5
    assert gbar[0] == g[0] and gbar[-1] == 1 and gbar.shape == (22,)
    # all durations zero, or no tokens at all: P = 1000, g = 1
    for cum, n in (([0, 0], 2), ([], 0)):
        Sigma, gbar = C.tracks(700, cum, n, 256, P[:n], g[:n])
        assert (Sigma == 1000 * C.K).all() and (gbar == 1).all()
    with pytest.raises(ValueError, match="12.5 semitones"):
        C.token_ratios([0.0, 12.5])
    with pytest.raises(ValueError, match="dB"):
        C.token_gains([np.nan])
    assert C.token_ratios([0.0, 12.0, -12.0]).tolist() == [1000, 2000, 500]


def test_exact_cases_of_the_restatement():
    x = (0.2 * np.random.default_rng(1).standard_normal(2048)).astype(np.float32)
    assert C.contour(x, [3, 8], 2, 256, [0.0, 0.0], [0.0, 0.0]).astype(np.float32).tobytes() == x.tobytes()
    rep = {}
    y = C.contour(x, [3, 8], 2, 256, None, [6.0, -6.0], report=rep)
    assert not rep["shifted"] and y.astype(np.float32).tobytes() == (rep["G"] * x).tobytes()
    assert C.contour(x[:300], [1, 2], 2, 256, [5.0, -5.0], None).astype(np.float32).tobytes() == x[:300].tobytes()  # too short to shift
    T = C.filter_table()
    assert T.shape == (C.Z * C.RES + 2,) and T[0] == np.float32(0.9) and T[-1] == 0 and abs(T[-2]) < 1e-5


def test_definition_moves_the_fundamental_of_every_token():
    """f0 = 200 Hz, 8 harmonics, four tokens of 16 frames: in the middle of each the fundamental sits within 1 % of 200 P_t / 1000"""
    x = C.tone()
    st = [0.0, 4.0, -5.0, 12.0]
    y = C.contour(x, [16, 32, 48, 64], 4, 256, st, None, np.float64)
    assert y.shape == x.shape
    P = C.token_ratios(st)
    for t in range(4):
        f = C.fundamental(y[t * 4096 + 1024:t * 4096 + 3072])
        want = 200.0 * P[t] / 1000.0
        assert abs(f - want) <= 0.01 * want, (t, f, want)
    assert abs(C.fundamental(x[1024:3072]) - 200.0) < 0.5


# ---- Synth with a stub model -------------------------------------------------------------------------------------------------------------
class _Hp:
    sampling_rate, hop_length, bert_dim, n_speakers = 22050, 256, 0, 4


def _synth(config, layout):
    from vosk_tts_amd.synth import Synth

    class M:
        pass

    s = Synth.__new__(Synth)
    s.model = M()
    s.model.config = config
    s.model.onnx = type("Sess", (), {"hp": _Hp()})()
    s.marks_layout = lambda text: layout
    return s


def _layout(blank):
    """'^ a b , c $' with words {0: 'ab', 1: 'c'}"""
    return ["^", "a", "b", ",", "c", "$"], [1] * 6, blank, [None, 0, 0, None, 1, None], {0: "ab", 1: "c"}


def test_keywords_are_on_synth_audio_and_synth_and_not_on_synth_stream():
    from vosk_tts_amd.synth import Synth

    for name in ("synth_audio", "synth"):
        assert {"word_pitch", "word_gains"} <= set(inspect.signature(getattr(Synth, name)).parameters)
    assert not {"word_pitch", "word_gains"} & set(inspect.signature(Synth.synth_stream).parameters)
    assert hasattr(Synth, "synth_ssml")


def test_words_map_to_tokens_in_both_layouts_and_bad_values_stop_before_the_model():
    # interspersed blanks: ids [^ _ a _ b _ , _ c _ $]: a word covers its phonemes and the blank in front of each
    s = _synth({"inference": {}}, _layout(True))
    args = {"input": np.ones((1, 11), np.int64)}
    assert not s._contour(args, "ab, c") and list(args) == ["input"]
    assert s._contour(args, "ab, c", word_pitch={0: 3.0}, word_gains={1: -6.0})
    assert args["vits.token_pitch"].tolist() == [[0, 3, 3, 3, 3, 0, 0, 0, 0, 0, 0]] and args["vits.token_pitch"].dtype == np.float32
    assert args["vits.token_gain_db"].tolist() == [[0, 0, 0, 0, 0, 0, 0, -6, -6, 0, 0]]
    # a multistream layout: one token per symbol, and the keywords are accepted there
    ms = _synth({"model_type": "multistream_v2", "inference": {}}, _layout(False))
    args = {"input": np.ones((1, 5, 6), np.int64)}
    assert ms._contour(args, "ab, c", word_pitch={1: -2.0})
    assert args["vits.token_pitch"].tolist() == [[0, 0, 0, 0, -2, 0]] and "vits.token_gain_db" not in args
    # refused before the model is called (the stub has none to call)
    for kw, match in ((dict(word_pitch={0: 12.5}), "12.5"), (dict(word_pitch={0: float("nan")}), "semitones"), (dict(word_gains={1: 13.0}), "dB"),
                      (dict(word_gains={0: -41.0}), "dB"), (dict(word_pitch={7: 1.0}), "no word 7")):
        with pytest.raises(ValueError, match=match):
            s._contour({"input": np.ones((1, 11), np.int64)}, "ab, c", **kw)
    with pytest.raises(ValueError, match="layout does not match"):
        s._contour({"input": np.ones((1, 12), np.int64)}, "ab, c", word_pitch={0: 1.0})


def test_contour_arrays_refuse_by_name_and_neutral_ones_are_no_contour():
    from vosk_tts_amd.capi import contour_arrays

    assert contour_arrays(1, 4) is None and contour_arrays(1, 4, np.zeros((1, 4)), np.zeros((1, 4))) is None
    a = contour_arrays(2, 3, [[0, 1, 0], [0, 0, 0]], None, [3, 2])
    assert list(a) == ["token_semitones"] and a["token_semitones"].dtype == np.float32
    assert contour_arrays(2, 3, [[0, 0, 0], [0, 0, 99]], None, [3, 2]) is None  # beyond an item's tokens nothing is looked at
    with pytest.raises(ValueError, match="13 semitones at item 1, token 0"):
        contour_arrays(2, 3, [[0, 1, 0], [10, 0, 0]], None, [3, 2], pitch=3.0)
    with pytest.raises(ValueError, match="dB at item 0, token 2"):
        contour_arrays(1, 3, None, [[0, 0, 12.5]])
    with pytest.raises(ValueError, match=r"must be \[1, 3\]"):
        contour_arrays(1, 3, [[0, 0]])


def test_sessions_take_the_feed_keys_and_streams_refuse_them():
    from vosk_tts_amd import session, session_stts

    assert {"vits.token_pitch", "vits.token_gain_db"} <= set(session._EXT) and {"vits.token_pitch", "vits.token_gain_db"} <= set(session_stts._EXT)
    assert set(session._CONTOUR.values()) == {"token_pitch", "token_gain_db"}


def test_command_line_flags():
    from vosk_tts_amd import cli

    o = cli.build_parser().parse_args(["-i", "x", "--word-pitch", "1=-3", "--word-pitch", "0=2.5", "--word-gain", "2=6", "--ssml"])
    assert cli._indexed(o.word_pitch, "--word-pitch", "=") == {1: -3.0, 0: 2.5} and cli._indexed(o.word_gain, "--word-gain", "=") == {2: 6.0} and o.ssml
    o = cli.build_parser().parse_args(["-i", "x"])
    assert o.word_pitch is None and o.word_gain is None and o.ssml is False
    with pytest.raises(SystemExit, match="INDEX=VALUE"):
        cli._indexed(["1:3"], "--word-pitch", "=")
