"""CPU tests of the prosody controls (include/vits_prosody.h): the restatement's own invariants, the host-side layout arithmetic
(vosk_tts_amd/prosody.py), the ABI mirrors, the refusals that need no device, and the serving path -- requests with different scales
share a batch."""
import ctypes
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import prosody_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def _inputs(seed=3, B=4, T=13, lens=(13, 5, 1, 0)):
    rng = np.random.default_rng(seed)
    logw = rng.normal(0.6, 0.7, size=(B, T)).astype(np.float32)
    forced = rng.integers(0, 7, size=(B, T)).astype(np.int32)
    forced[:, 0] = np.maximum(forced[:, 0], 1)
    pause = (rng.integers(0, 4, size=(B, T)) * (rng.random((B, T)) < 0.4)).astype(np.int32)
    return logw, forced, np.array(lens, np.int64), pause


def test_fitted_items_have_exactly_their_frame_count():
    logw, forced, lens, pause = _inputs()
    mask = np.arange(13)[None] < lens[:, None]
    P = np.where(mask, pause, 0).sum(1)
    for src in (dict(logw=logw, forced=None), dict(logw=None, forced=forced)):
        for factor in (0.4, 1.0, 1.7, 3.1):
            _, _, natural, _ = R.regulate(src["logw"], src["forced"], lens)
            fit = np.where(lens > 0, np.maximum(np.rint(natural * factor), 1) + P, 0).astype(np.int32)
            fit[1] = 0  # one item is not fitted
            d, cum, ylen, ratio = R.regulate(src["logw"], src["forced"], lens, token_pause=pause, fit_frames=fit)
            plain = R.regulate(src["logw"], src["forced"], lens, token_pause=pause)
            for b in range(4):
                if fit[b] > 0:
                    assert ylen[b] == fit[b] == d[b].sum() and 0.25 <= ratio[b] <= 4.0
                    assert (d[b] >= np.where(mask[b], pause[b], 0)).all()  # c_t is non-decreasing: a pause is never eaten
                else:
                    assert np.array_equal(d[b], plain[0][b]) and ratio[b] == 1.0
            assert np.array_equal(cum, np.cumsum(d, axis=1)) and not d[~mask].any()


def test_neutral_controls_are_the_plain_rule():
    logw, forced, lens, _ = _inputs(4)
    mask = np.arange(13)[None] < lens[:, None]
    for ls in (1.0, 0.8, 1.37):
        want = np.where(mask, np.maximum(np.ceil(np.exp(logw).astype(np.float32) * np.float32(ls)), 0), 0).astype(np.int32)
        plain = R.regulate(logw, None, lens, ls)
        assert np.array_equal(plain[0], want) and np.array_equal(plain[2], np.maximum(want.sum(1), 1))
        neutral = R.regulate(logw, None, lens, ls, token_length_scale=np.ones((4, 13), np.float32), token_pause=np.zeros((4, 13), np.int32),
                             fit_frames=np.zeros(4, np.int32))
        scales = R.regulate(logw, None, lens, 99.0, item_scales=np.tile(np.array([0.3, ls, 0.1], np.float32), (4, 1)))
        for got in (neutral, scales):
            assert all(np.array_equal(a, b) for a, b in zip(plain, got))


def test_a_pause_is_a_longer_forced_duration():
    _, forced, lens, pause = _inputs(5)
    a = R.regulate(None, forced, lens, token_pause=pause)
    b = R.regulate(None, forced + pause, lens)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_fit_refusals_and_margins():
    _, forced, lens, pause = _inputs(6)
    P0 = int(pause[0].sum())
    for fit in ([P0, 0, 0, 0], [0, 0, 0, 5], [100 * int(forced[0].sum()), 0, 0, 0], [1 + P0, 0, 0, 0]):
        with pytest.raises(R.FitRefused):
            R.regulate(None, forced, lens, token_pause=pause, fit_frames=np.array(fit, np.int32))
    with pytest.raises(ValueError):
        R.regulate(None, forced, lens, token_length_scale=np.ones((4, 13), np.float32))
    # s = 1.5 over odd prefixes is an exact tie; the margin says so, and rint resolves it half-to-even
    d = np.array([[1, 2, 2]], np.int32)
    assert R.fit_margin(None, d, [3], [int(1.5 * 5)]) > 0 and R.fit_margin(None, d, [3], [15]) == 0.5
    assert R.fit_margin(None, np.array([[1, 1]], np.int32), [2], [3]) == 0.0
    assert R.regulate(None, np.array([[1, 1]], np.int32), [2], fit_frames=[3])[0].tolist() == [[2, 1]]  # rint(1.5) = 2, rint(3) = 3
    assert R.ceil_margin(np.array([[2.0, 2.5, 0.0]])) == 0.0 and abs(R.ceil_margin(np.array([[2.5]])) - 0.2) < 1e-12


# ---- words, seconds, rates -> tokens ------------------------------------------------------------------------------------------------
def _layout(blank, counts=None):
    """'^ a b , c $' with words {0: 'ab', 1: 'c'} -- symbols 1, 2 are word 0, symbol 4 word 1"""
    symbols = ["^", "a", "b", ",", "c", "$"]
    return symbols, counts or [1] * 6, blank, [None, 0, 0, None, 1, None], {0: "ab", 1: "c"}


def test_token_controls_blank_and_no_blank_layouts():
    from vosk_tts_amd import marks as M
    from vosk_tts_amd import prosody as P

    # no blank: one token per symbol
    tls, pause = P.token_controls(_layout(False), {0: 2.0}, {0: 0.5}, 22050, 256)
    assert tls.tolist() == [1, 0.5, 0.5, 1, 1, 1] and tls.dtype == np.float32
    assert pause.tolist() == [0, 0, 0, 43, 0, 0] and pause.dtype == np.int32 and P.frames(0.5, 22050, 256) == 43
    # interspersed blank: symbol k > 0 owns the blank in front of it (tokens 2k-1, 2k), the cover of marks.phoneme_spans
    tls, pause = P.token_controls(_layout(True), {1: 0.25}, {0: 0.1, 1: 0.2}, 22050, 256)
    assert tls.tolist() == [1, 1, 1, 1, 1, 1, 1, 4, 4, 1, 1] and pause.tolist() == [0, 0, 0, 0, 0, 0, 9, 0, 0, 0, 17]  # word 1's pause lands on '$'
    spans = M.phoneme_spans(np.arange(1, 12), [1] * 6, True)
    assert [(a, b) for a, b in P.symbol_tokens([1] * 6, True)] == [(a, b) for a, b in spans]
    # list-valued id maps: a symbol of several ids; the pause goes on the LAST token of the carrier
    tls, pause = P.token_controls(_layout(True, [1, 2, 1, 3, 1, 1]), {0: 2.0}, {0: 1.0}, 16000, 200)
    assert tls.tolist() == [1, .5, .5, .5, .5, .5, 1, 1, 1, 1, 1, 1, 1, 1] and pause.tolist() == [0] * 9 + [80] + [0] * 4
    assert P.token_controls(_layout(True)) == (None, None)
    for bad in (dict(word_rates={2: 1.0}), dict(pauses={5: 0.1}), dict(word_rates={0: 0.0}), dict(word_rates={0: 1e-3}),
                dict(word_rates={0: float("nan")}), dict(pauses={0: -0.1})):
        with pytest.raises(ValueError):
            P.token_controls(_layout(True), **bad)


def test_pause_markup_is_split_off_the_text():
    from vosk_tts_amd import prosody as P

    assert P.split_pause_markup("прив+ет_ м+ир, да_") == ("прив+ет м+ир, да", [0, 2])
    assert P.split_pause_markup("_а - б_в") == ("а - бв", [1])  # in front of the first word: dropped; '-' is no word
    assert P.split_pause_markup("no marks here.") == ("no marks here.", [])
    assert P.PAUSE_FRAMES == 20


def test_controls_are_checked_before_any_device_work():
    from vosk_tts_amd import capi
    from vosk_tts_amd import prosody as P

    lens = [3, 2]
    ok = dict(item_scales=np.ones((2, 3)), token_length_scale=np.ones((2, 3)), token_pause=np.zeros((2, 3), int), fit_frames=[0, 9])
    P.check_controls(lens, **ok)
    junk = np.ones((2, 3))
    junk[1, 2] = np.nan  # beyond item 1's length: not looked at
    P.check_controls(lens, token_length_scale=junk)
    for name, value, pattern in (("token_length_scale", np.array([[1, np.nan, 1], [1, 1, 1.]]), r"token_length_scale\[0, 1\] = nan"),
                                 ("token_length_scale", np.array([[1, 1, 1], [1, 17.0, 1]]), r"token_length_scale\[1, 1\] = 17"),
                                 ("token_pause", np.array([[0, 0, -4], [0, 0, 0]]), r"token_pause\[0, 2\] = -4"),
                                 ("fit_frames", [0, -1], r"fit_frames\[1\] = -1"),
                                 ("item_scales", np.array([[1, 1, 1], [1, -0.5, 1]]), r"item_scales\[1, 1\] = -0.5"),
                                 ("item_scales", np.array([[np.inf, 1, 1], [1, 1, 1]]), r"item_scales\[0, 0\] = inf")):
        with pytest.raises(ValueError, match=pattern):
            P.check_controls(lens, **{name: value})
    with pytest.raises(ValueError, match="forced"):
        P.check_controls(lens, token_length_scale=np.ones((2, 3)), forced=True)
    # shapes, at the binding
    assert capi.prosody_arrays(2, 3) is None
    a = capi.prosody_arrays(2, 3, token_pause=[[0, 1, 2], [3, 4, 5]], fit_frames=[7, 0])
    assert a["token_pause"].dtype == np.int32 and a["fit_frames"].dtype == np.int32 and set(a) == {"token_pause", "fit_frames"}
    for kw in (dict(item_scales=np.ones(3)), dict(token_length_scale=np.ones((2, 4))), dict(token_pause=np.ones((3, 3))), dict(fit_frames=[1])):
        with pytest.raises(ValueError, match="must be"):
            capi.prosody_arrays(2, 3, **kw)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def test_header_layout_flag_and_export(tmp_path, hip_lib):
    from vosk_tts_amd import capi
    from vosk_tts_amd import prosody as P

    names = [n for n, _ in capi.Prosody._fields_]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vits_prosody.h"', 'int main(void) {',
             '  printf("%d %g %g %g\\n", VITS_FLAG_PROSODY, (double)VITS_PROSODY_MAX_TOKEN_SCALE, VITS_PROSODY_MIN_FIT_RATIO, VITS_PROSODY_MAX_FIT_RATIO);',
             '  printf("%zu %zu %zu %zu\\n", sizeof(vits_synth_opts_prosody), offsetof(vits_synth_opts_prosody, base), '
             'offsetof(vits_synth_opts_prosody, prosody), sizeof(vits_synth_opts_limit));',
             '  printf("%zu' + " %zu" * len(names) + '\\n", sizeof(vits_prosody)' + "".join(f", offsetof(vits_prosody, {n})" for n in names) + ');',
             '  return 0;', '}']
    src = tmp_path / "c.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "c"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert [float(v) for v in out[0]] == [capi.FLAG_PROSODY, capi.PROSODY_MAX_TOKEN_SCALE, *capi.PROSODY_FIT_RATIO] == [32, 16, 0.25, 4]
    assert (P.MAX_TOKEN_SCALE, P.FIT_RATIO) == (R.MAX_TOKEN_SCALE, R.FIT_RATIO) == (capi.PROSODY_MAX_TOKEN_SCALE, capi.PROSODY_FIT_RATIO)
    assert [int(v) for v in out[1]] == [ctypes.sizeof(capi.SynthProsodyOpts), 0, capi.SynthProsodyOpts.prosody.offset, ctypes.sizeof(capi.SynthLimitOpts)]
    assert issubclass(capi.SynthProsodyOpts, capi.SynthLimitOpts) and [n for n, *_ in capi.SynthProsodyOpts._fields_] == ["prosody"]
    assert [int(v) for v in out[2]] == [ctypes.sizeof(capi.Prosody)] + [getattr(capi.Prosody, n).offset for n in names]
    # the flag is free among the VITS flags, and the library exports the door with the binding's argument list
    assert capi.FLAG_PROSODY not in (1, capi.FLAG_LOUDNESS, capi.FLAG_PITCH, capi.FLAG_PITCH_FORMANT, capi.FLAG_LIMIT)
    assert hip_lib.has_prosody and len(hip_lib._fn("op_regulate").argtypes) == 12


# ---- serving --------------------------------------------------------------------------------------------------------------------------
class _Hp:
    sampling_rate, hop_length, bert_dim, n_speakers = 22050, 256, 0, 4


class _EngineStub:
    """stands where capi.VitsModel stands: records the scales of every engine call; the first call waits for the gate"""

    def __init__(self):
        self.hp = _Hp()
        self.calls = []
        self.entered, self.gate = threading.Event(), threading.Event()

    def synthesize_pcm16(self, ids, lens, scales, sid, pcm_scale=1.0, seed=0, solo=False, item_seeds=None, sample_rate=None, **kw):
        first = not self.calls
        self.calls.append((ids.shape[0], np.array(scales).tolist(), None if kw.get("item_scales") is None else np.array(kw["item_scales"]).tolist(),
                           np.array(lens).tolist()))
        if first:
            self.entered.set()
            assert self.gate.wait(30)
        B = ids.shape[0]
        tag = np.array(scales if kw.get("item_scales") is None else kw["item_scales"], np.float32).reshape(-1, 3)[:, 1] * 100
        return np.broadcast_to(np.rint(tag).astype(np.int16)[:, None] if tag.shape[0] == B else np.full((B, 1), np.rint(tag[0]), np.int16), (B, 8)).copy(), \
            np.full(B, 8, np.int64)

    def close(self):
        pass


class _LibStub:
    is_device = True
    has_prosody = True

    def __init__(self):
        self.model = _EngineStub()

    def create(self, blob, device):
        return self.model

    def _need_prosody(self):
        pass


def _feed(speech_rate, n=5, **ext):
    return dict({"input": np.ones((1, n), np.int64), "input_lengths": np.array([n]), "scales": np.array([0.8, 1.0 / speech_rate, 0.8], np.float32),
                 "sid": np.array([1])}, **ext)


def test_requests_with_different_speech_rates_share_a_batch():
    from vosk_tts_amd.session import VitsSession

    lib = _LibStub()
    sess = VitsSession(b"", lib=lib, max_inflight=1)
    eng = lib.model
    rates = [1.0, 0.8, 1.25, 2.0]
    results = [None] * len(rates)

    def worker(i):
        results[i] = sess.run_pcm16(_feed(rates[i], n=5 + i), 1.0)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(len(rates))]
    threads[0].start()
    assert eng.entered.wait(30)  # the first request is inside the engine: the others queue behind it
    for t in threads[1:]:
        t.start()
    deadline = time.monotonic() + 30
    while len(sess.coalescer._queue) < len(rates) - 1 and time.monotonic() < deadline:
        time.sleep(0.001)
    assert len(sess.coalescer._queue) == len(rates) - 1
    assert len({p.key for p in sess.coalescer._queue}) == 1 and not any("scales" in str(k) for k in sess.coalescer._queue[0].key)
    eng.gate.set()
    for t in threads:
        t.join(30)
    # two engine calls: the first request alone, then the three queued ones as ONE solo batch (padded to four) with their own scales
    assert [c[0] for c in eng.calls] == [1, 4] and sess.coalescer.calls == 2
    assert eng.calls[0][1] == pytest.approx([0.8, 1.0, 0.8]) and eng.calls[0][2] is None
    want = [[0.8, 1.0 / r, 0.8] for r in rates[1:]]
    got = sorted(eng.calls[1][2][:3], key=lambda s: -s[1])
    assert np.allclose(got, sorted(want, key=lambda s: -s[1])) and eng.calls[1][2][3] == eng.calls[1][2][0]  # (the dummy rides on the first one's)
    for r, out in zip(rates, results):  # every request got the item that was run with ITS scales
        assert out is not None and (out == int(np.rint(100.0 / r))).all(), (r, out)


def test_requests_with_equal_scales_run_the_call_they_always_ran():
    from vosk_tts_amd.outopts import Tail
    from vosk_tts_amd.session import RequestCoalescer, VitsSession

    lib = _LibStub()
    lib.model.gate.set()
    sess = VitsSession(b"", lib=lib)
    out = sess._run_solo_batch(("pcm", 1.0, 0, False, Tail()),
                               [(np.ones((1, 4), np.int64), 0, 1, (0.8, 1.0, 0.8)), (np.ones((1, 6), np.int64), 1, 2, (0.8, 1.0, 0.8))])
    assert len(out) == 2 and len(lib.model.calls) == 1
    assert lib.model.calls[0][0] == 2 and lib.model.calls[0][1] == pytest.approx([0.8, 1.0, 0.8]) and lib.model.calls[0][2:] == (None, [4, 6])
    # the coalescer's own contract: a trailing `extra` rides with the request, the first three entries are where they were
    seen = []
    co = RequestCoalescer(lambda key, reqs: [seen.append(reqs) or (r[2], r[3]) for r in reqs])
    assert co.submit("k", None, 0, 7) == (7, None) and co.submit("k", None, 0, 8, "mine") == (8, "mine")
    assert [len(r) for reqs in seen for r in reqs] == [4, 4]


def test_prosody_feeds_reach_the_engine_and_keep_out_of_merged_batches():
    from vosk_tts_amd import session
    from vosk_tts_amd.session import VitsSession

    assert {"vits.item_scales", "vits.token_length_scale", "vits.token_pause", "vits.fit_frames"} <= set(session._EXT)
    lib = _LibStub()
    lib.model.gate.set()
    seen = []
    lib.model.synthesize_pcm16 = lambda ids, lens, scales, sid, **kw: (seen.append(kw), (np.zeros((1, 8), np.int16), np.full(1, 8, np.int64)))[1]
    sess = VitsSession(b"", lib=lib)
    sess.coalescer.submit = lambda *a: pytest.fail("a controlled request was handed to the coalescer")
    sess.run_pcm16(_feed(1.0, **{"vits.token_pause": np.zeros((1, 5), np.int32), "vits.fit_frames": np.array([40], np.int32)}), 1.0)
    assert seen[0]["fit_frames"].tolist() == [40] and seen[0]["token_pause"].shape == (1, 5) and "token_length_scale" not in seen[0]
    with pytest.raises(ValueError, match=r"token_pause\[0, 1\] = -3"):
        sess.run_pcm16(_feed(1.0, **{"vits.token_pause": np.array([[0, -3, 0, 0, 0]], np.int32)}), 1.0)
    with pytest.raises(ValueError, match="forced"):
        sess.run_pcm16(_feed(1.0, **{"vits.token_length_scale": np.ones((1, 5), np.float32), "vits.forced_durations": np.ones((1, 5), np.int32)}), 1.0)
    assert len(seen) == 1


def test_multi_device_batcher_takes_one_value_or_one_per_request():
    from vosk_tts_amd.batching import MultiDeviceSynth

    class S:
        class model:
            config = {"inference": {}}

    m = MultiDeviceSynth.__new__(MultiDeviceSynth)
    m.synths, m.family, m._seed, m._lock = [S()], "vits", 0, threading.Lock()
    scales, scale, sids, seeds = m._call_params(3, 0, None, 2.0, None, None, None)
    assert scales.shape == (3,) and np.allclose(scales, [0.8, 0.5, 0.8])
    assert m._scales_feed(scales, [2, 0]).keys() == {"scales"}
    scales, _, _, _ = m._call_params(3, 0, None, [1.0, 2.0, 0.5], [0.1, 0.2, 0.3], None, None)
    assert scales.shape == (3, 3) and np.allclose(scales, [[0.8, 1.0, 0.1], [0.8, 0.5, 0.2], [0.8, 2.0, 0.3]])
    f = m._scales_feed(scales, [2, 0])
    assert np.allclose(f["vits.item_scales"], scales[[2, 0]]) and np.allclose(f["scales"], scales[2])
    with pytest.raises(ValueError, match="speech_rate"):
        m._call_params(3, 0, None, [1.0, 2.0], None, None, None)
    m.family = "multistream"
    with pytest.raises(ValueError, match="VITS-family"):
        m._call_params(3, 0, None, [1.0, 2.0, 0.5], None, None, None)


# ---- Synth and the command line -------------------------------------------------------------------------------------------------------
def _synth(config, layout=None):
    from vosk_tts_amd.synth import Synth

    class M:
        pass

    s = Synth.__new__(Synth)
    s.model = M()
    s.model.config = config
    s.model.onnx = type("Sess", (), {"hp": _Hp()})()
    if layout is not None:
        s.marks_layout = lambda text: layout
    return s


def test_synth_builds_the_feeds_from_words_and_seconds():
    s = _synth({"inference": {}}, _layout(True))
    args = {"input": np.ones((1, 11), np.int64)}
    assert not s._prosody(args, "ab, c") and list(args) == ["input"]
    assert s._prosody(args, "ab, c", word_rates={0: 2.0}, pauses={1: 0.2}, duration=1.5)
    assert args["vits.token_length_scale"].shape == (1, 11) and args["vits.token_length_scale"][0, 1:5].tolist() == [0.5] * 4
    assert args["vits.token_pause"].tolist() == [[0] * 10 + [17]] and args["vits.fit_frames"].tolist() == [129]
    assert args["vits.fit_frames"].dtype == np.int32
    with pytest.raises(ValueError, match="less than one frame"):
        s._prosody({"input": np.ones((1, 11), np.int64)}, "ab, c", duration=0.001)
    with pytest.raises(ValueError, match="layout does not match"):
        s._prosody({"input": np.ones((1, 12), np.int64)}, "ab, c", pauses={0: 0.1})
    # the reference's '_' behind a word: off by default, a pause of inference.pause_frames with the config key
    assert s._prosody_text("ab_ c", None, None, None) == ("ab_ c", None)
    on = _synth({"inference": {"pause_markup": True}})
    text, pauses = on._prosody_text("ab_ c_", None, {1: 0.5}, None)
    assert text == "ab c" and pauses == {0: pytest.approx(20 * 256 / 22050), 1: pytest.approx(0.5 + 20 * 256 / 22050)}
    assert on._prosody_text("ab c", None, None, None) == ("ab c", None)
    on7 = _synth({"inference": {"pause_markup": True, "pause_frames": 7}}, _layout(True))
    text, pauses = on7._prosody_text("ab_, c", None, None, None)
    args = {"input": np.ones((1, 11), np.int64)}
    on7._prosody(args, text, pauses=pauses)
    assert text == "ab, c" and args["vits.token_pause"].tolist() == [[0] * 6 + [7] + [0] * 4]
    # a multistream voice keeps its own markup
    ms = _synth({"model_type": "multistream_v3", "inference": {}})
    assert ms._prosody_text("ab_ c", None, None, None) == ("ab_ c", None)
    for kw in (dict(word_rates={0: 2.0}), dict(pauses={0: 0.1}), dict(duration=2.0)):
        with pytest.raises(ValueError, match="multistream"):
            ms._prosody_text("ab c", kw.get("word_rates"), kw.get("pauses"), kw.get("duration"))


def test_command_line_flags():
    from vosk_tts_amd import cli

    o = cli.build_parser().parse_args(["-i", "x", "--duration", "2.5", "--pause", "0:0.3", "--pause", "2:1", "--word-rate", "1:0.5"])
    assert o.duration == 2.5 and cli._indexed(o.pause, "--pause") == {0: 0.3, 2: 1.0} and cli._indexed(o.word_rate, "--word-rate") == {1: 0.5}
    o = cli.build_parser().parse_args(["-i", "x"])
    assert o.duration is None and cli._indexed(o.pause, "--pause") is None and cli._indexed(o.word_rate, "--word-rate") is None
    with pytest.raises(SystemExit, match="INDEX:VALUE"):
        cli._indexed(["nonsense"], "--pause")
