"""GPU tests of the prosody controls (include/vits_prosody.h) against the NumPy restatement (tests/prosody_ref.py).

Exactness is asserted where the numbers are fixed by the input: the regulator's door on inputs whose roundings are at least 1e-3 away from
a tie (asserted on the restatement before the device is asked -- the device's expf may differ from NumPy's by an ulp), and whole forwards
under forced durations.  Where a controlled single utterance runs other kernels than its uncontrolled twin (launches instead of the
single-utterance program), or a batch item is compared with its own single call, the bound is the suite's figure for a change of kernel
choice, 2e-5 (test_solo_batch_items_equal_their_single_utterance_calls)."""
import ctypes

import numpy as np
import pytest

import marks_ref as MR
import prosody_ref as R
from conftest import assert_close

pytestmark = pytest.mark.gpu

SCALES = np.array([0.667, 1.0, 0.8], np.float32)
NATIVE, HOP = 22050, 256
KERNEL_CHOICE_TOL = 2e-5
E2E_TOL = 5e-4  # the suite's HIP-vs-oracle bound (tests/test_hip_parity.py)
SHAPES = {"ragged": (4, 13, [13, 5, 1, 0]), "long": (1, 300, [300]), "one": (1, 1, [1])}
# seeds of regulate_case() at which every free-running leg has ceil_margin() and fit_margin() >= 1e-3 (found with the restatement)
CASE_SEEDS = {"ragged": 1, "long": 1127, "one": 0}


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert getattr(hip_lib, "has_prosody", False), "libvits_mi355.so exports no prosody symbols (include/vits_prosody.h)"
    return hip_lib


def _persist_runs(lib, model):
    fn = lib.lib.vits_debug_persist_runs
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p]
    return int(fn(model._h))


def _both_paths(lib, fn):
    """fn() through the graph-replayed fast path and through the eager path"""
    out = []
    try:
        for on in (1, 0):
            lib.lib.vits_debug_fast_path(on)
            out.append(fn())
    finally:
        lib.lib.vits_debug_fast_path(1)
    return out


# ---- 1. the regulator's door --------------------------------------------------------------------------------------------------------
def regulate_case(shape, seed):
    """inputs of one shape: logw, forced (with zeros), item scales with different ls_b, token scales in [0.5, 2] with a zero, pauses,
    and per leg the fit targets at about 1.3 x (free-running) / 0.8 x (forced) of the item's own length (0 for an empty item)"""
    B, T, lens = SHAPES[shape]
    rng = np.random.default_rng([seed, B, T])
    c = dict(lens=np.array(lens, np.int64))
    c["logw"] = rng.normal(0.6, 0.7, size=(B, T)).astype(np.float32)
    c["forced"] = rng.integers(0, 7, size=(B, T)).astype(np.int32)
    c["forced"][:, 2::5] = 0
    c["forced"][:, 0] = np.maximum(c["forced"][:, 0], 1)
    c["item_scales"] = np.stack([np.full(B, 0.667), 0.7 + 0.35 * np.arange(B), np.full(B, 0.8)], axis=1).astype(np.float32)
    c["tls"] = rng.uniform(0.5, 2.0, size=(B, T)).astype(np.float32)
    if T > 3:
        c["tls"][:, 3] = 0.0
    c["pause"] = (rng.integers(0, 4, size=(B, T)) * (rng.random((B, T)) < 0.3)).astype(np.int32)
    c["pause"][:, -1] = 2
    return c


def regulate_legs(c):
    """name -> keyword arguments of op_regulate / prosody_ref.regulate: each control alone and all together, free-running and forced"""
    def fit_for(factor, **kw):
        _, _, ylen, _ = R.regulate(kw.get("logw"), kw.get("forced"), c["lens"], 1.0, kw.get("item_scales"), kw.get("token_length_scale"))
        P = np.where(np.arange(c["pause"].shape[1])[None] < c["lens"][:, None], c["pause"], 0).sum(1) if "token_pause" in kw else 0
        return np.where(c["lens"] > 0, np.maximum(np.rint(ylen * factor), 1) + P, 0).astype(np.int32)

    free, forced = dict(logw=c["logw"]), dict(forced=c["forced"])
    legs = {
        "free/tls": dict(free, token_length_scale=c["tls"]),
        "free/pause": dict(free, token_pause=c["pause"]),
        "free/item_scales": dict(free, item_scales=c["item_scales"]),
        "free/fit": dict(free, fit_frames=fit_for(1.3, **free)),
        "forced/pause": dict(forced, token_pause=c["pause"]),
        "forced/fit": dict(forced, fit_frames=fit_for(0.8, **forced)),
    }
    every = dict(free, token_length_scale=c["tls"], token_pause=c["pause"], item_scales=c["item_scales"])
    legs["free/all"] = dict(every, fit_frames=fit_for(1.3, **every))
    every = dict(forced, token_pause=c["pause"], item_scales=c["item_scales"])
    legs["forced/all"] = dict(every, fit_frames=fit_for(0.8, **every))
    return legs


def leg_margins(c, kw):
    """(ceil_margin, fit_margin) of one leg on the restatement; forced legs have no ceil"""
    cm = 0.5
    if kw.get("logw") is not None:
        _, _, w = R.base(kw["logw"], None, c["lens"], 1.0, kw.get("item_scales"), kw.get("token_length_scale"))
        cm = R.ceil_margin(w, c["lens"])
    fm = 0.5
    if "fit_frames" in kw:
        fm = R.fit_margin(kw.get("logw"), kw.get("forced"), c["lens"], kw["fit_frames"], 1.0, kw.get("item_scales"), kw.get("token_length_scale"),
                          kw.get("token_pause"))
    return cm, fm


@pytest.mark.parametrize("shape", list(SHAPES))
def test_regulate_door_equals_the_restatement(lib, shape):
    c = regulate_case(shape, CASE_SEEDS[shape])
    for name, kw in regulate_legs(c).items():
        cm, fm = leg_margins(c, kw)
        if "logw" in kw:
            assert cm >= 1e-3 and fm >= 1e-3, (shape, name, cm, fm)
        else:  # u is exact under forced durations: any distance from a tie will do
            assert fm >= 1e-9, (shape, name, fm)
        want = R.regulate(kw.get("logw"), kw.get("forced"), c["lens"], 1.0, kw.get("item_scales"), kw.get("token_length_scale"),
                          kw.get("token_pause"), kw.get("fit_frames"))
        got = lib.op_regulate(kw.get("logw"), kw.get("forced"), c["lens"], 1.0, kw.get("item_scales"), kw.get("token_length_scale"),
                              kw.get("token_pause"), kw.get("fit_frames"))
        for what, w, g in zip(("durations", "cum", "y_lengths"), want, got):
            assert np.array_equal(w, g), (shape, name, what, w, g)
        assert np.allclose(got[3], want[3], rtol=1e-6, atol=0), (shape, name, got[3], want[3])
        if "fit_frames" in kw:  # the item has exactly F_b frames
            fitted = kw["fit_frames"] > 0
            assert np.array_equal(got[2][fitted], kw["fit_frames"][fitted])
    # no controls at all: the plain rule
    d, cum, ylen, ratio = lib.op_regulate(c["logw"], None, c["lens"], 1.25)
    want = R.regulate(c["logw"], None, c["lens"], 1.25)
    _, _, w = R.base(c["logw"], None, c["lens"], 1.25)
    assert R.ceil_margin(w, c["lens"]) >= 1e-3
    assert np.array_equal(d, want[0]) and np.array_equal(cum, want[1]) and np.array_equal(ylen, want[2]) and (ratio == 1).all()


# ---- the whole forward ---------------------------------------------------------------------------------------------------------------
def _batch_case(seed=61):
    """B = 3, T_x = 13 (no multiple of the bucket of 8), lengths [13, 5, 1]; forced durations with zeros, pauses on a few tokens"""
    rng = np.random.default_rng(seed)
    lens = np.array([13, 5, 1], np.int64)
    ids = rng.integers(1, 20, size=(3, 13)).astype(np.int64)
    sid = np.array([0, 3, 1], np.int64)
    dur = rng.integers(0, 6, size=(3, 13)).astype(np.int32)
    dur[0, [2, 9]] = 0
    dur[2, 0] = 3
    pause = np.zeros((3, 13), np.int32)
    pause[0, [2, 5, 12]] = [4, 1, 7]
    pause[1, 4] = 3
    pause[2, 0] = 2
    return ids, lens, sid, dur, pause


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def test_pauses_equal_longer_forced_durations(lib, hip_tiny):
    ids, lens, sid, dur, pause = _batch_case()
    kw = dict(seed=7, marks=True)
    for solo in (False, True):
        want = _both_paths(lib, lambda: hip_tiny.synthesize(ids, lens, SCALES, sid, forced_durations=dur + pause, solo=solo, **kw))
        got = _both_paths(lib, lambda: hip_tiny.synthesize(ids, lens, SCALES, sid, forced_durations=dur, token_pause=pause, solo=solo, **kw))
        for path, w, g in zip(("fast", "eager"), want, got):
            assert _same(w, g), (solo, path)
    # one utterance: the uncontrolled call may take the single-utterance program, the controlled one runs launches
    one = slice(0, 1)
    want = _both_paths(lib, lambda: hip_tiny.synthesize(ids[one], lens[one], SCALES, sid[one], forced_durations=(dur + pause)[one], **kw))
    got = _both_paths(lib, lambda: hip_tiny.synthesize(ids[one], lens[one], SCALES, sid[one], forced_durations=dur[one], token_pause=pause[one], **kw))
    for path, w, g in zip(("fast", "eager"), want, got):
        assert np.array_equal(w[1], g[1]) and np.array_equal(w[2], g[2]), path
        assert_close(f"B = 1, {path}", w[0], g[0], KERNEL_CHOICE_TOL)


def test_neutral_controls_change_nothing(lib, hip_tiny):
    ids, lens, sid, _, _ = _batch_case(62)
    neutral = dict(token_length_scale=np.ones((3, 13), np.float32), token_pause=np.zeros((3, 13), np.int32))
    kw = dict(seed=11, marks=True)
    for solo in (False, True):
        want = _both_paths(lib, lambda: hip_tiny.synthesize(ids, lens, SCALES, sid, solo=solo, **kw))
        got = _both_paths(lib, lambda: hip_tiny.synthesize(ids, lens, SCALES, sid, solo=solo, fit_ratio=True, **neutral, **kw))
        for path, w, g in zip(("fast", "eager"), want, got):
            assert _same(w, g[:3]) and (g[3] == 1).all(), (solo, path)
    # one utterance; the plain call launches what it launched before a controlled call came by (the same persistent launches)
    one = slice(0, 1)
    n1 = {k: v[one] for k, v in neutral.items()}
    r0 = _persist_runs(lib, hip_tiny)
    want = hip_tiny.synthesize(ids[one], lens[one], SCALES, sid[one], **kw)
    r1 = _persist_runs(lib, hip_tiny)
    got = hip_tiny.synthesize(ids[one], lens[one], SCALES, sid[one], **n1, **kw)
    r2 = _persist_runs(lib, hip_tiny)
    again = hip_tiny.synthesize(ids[one], lens[one], SCALES, sid[one], **kw)
    r3 = _persist_runs(lib, hip_tiny)
    assert r3 - r2 == r1 - r0 and _same(want, again)
    assert np.array_equal(want[1], got[1]) and np.array_equal(want[2], got[2])
    assert_close("B = 1", want[0], got[0], KERNEL_CHOICE_TOL)


ITEM_SCALES = np.array([[0.667, 1.0, 0.8], [0.5, 1.3, 0.6], [0.8, 0.8, 1.0]], np.float32)
ITEM_SEED = 0  # of _item_case(): the oracle's own w of the checked item has ceil_margin() >= 1e-3 there (found with the oracle)


def _item_case(seed):
    rng = np.random.default_rng([seed, 77])
    lens = np.array([30, 12, 21], np.int64)
    ids = rng.integers(1, 62, size=(3, 30)).astype(np.int64)
    sid = np.array([1, 4, 7], np.int64)
    noise_dp = rng.standard_normal((3, 2, 30)).astype(np.float32)
    return ids, lens, sid, noise_dp


def oracle_item_margin(oracle, seed, b=1):
    """ceil_margin() of the oracle's own w = exp(logw) * ls_b of item b under the case's injected duration noise"""
    ids, lens, sid, noise_dp = _item_case(seed)
    L = int(lens[b])
    x, _, _ = oracle.text_encoder(ids[b:b + 1, :L], [L], sid[b:b + 1])
    logw = oracle.duration(x, [L], sid[b:b + 1], noise_dp[b:b + 1, :, :L], float(ITEM_SCALES[b, 2]))
    w = np.exp(logw.astype(np.float32)).astype(np.float32) * ITEM_SCALES[b, 1]
    return R.ceil_margin(w, [L])


def test_item_scales_give_every_item_its_own_call(lib, hip_default, oracle_default):
    ids, lens, sid, noise_dp = _item_case(ITEM_SEED)
    for audio, olen in _both_paths(lib, lambda: hip_default.synthesize(ids, lens, SCALES, sid, seed=50, solo=True, item_scales=ITEM_SCALES)):
        for b in range(3):
            L = int(lens[b])
            one, ol = hip_default.synthesize(ids[b:b + 1, :L], [L], ITEM_SCALES[b], sid[b:b + 1], seed=50 + b)
            assert ol[0] == olen[b], b
            assert_close(f"item {b}", one[0], audio[b, :olen[b]], KERNEL_CHOICE_TOL)
            assert not audio[b, olen[b]:].any()
    # one item against the oracle, under injected noise (the oracle's own durations are then known to be a safe distance from a flip)
    b, L = 1, int(lens[1])
    assert oracle_item_margin(oracle_default, ITEM_SEED, b) >= 1e-3
    rng = np.random.default_rng(78)
    noise_prior = rng.standard_normal((3, hip_default.hp.inter_channels, 1024)).astype(np.float32)
    audio, olen = hip_default.synthesize(ids, lens, SCALES, sid, solo=True, item_scales=ITEM_SCALES, noise_dp=noise_dp, noise_prior=noise_prior)
    want, wl = oracle_default.synthesize(ids[b:b + 1, :L], [L], ITEM_SCALES[b], sid[b:b + 1], noise_dp=noise_dp[b:b + 1, :, :L],
                                         noise_prior=noise_prior[b:b + 1])
    assert wl[0] == olen[b]
    assert_close("item 1 vs oracle", want[0, :wl[0]], audio[b, :olen[b]], E2E_TOL)
    # one utterance: its item scales are the call's scalars
    for b in range(3):
        L = int(lens[b])
        for w, g in zip(_both_paths(lib, lambda: hip_default.synthesize(ids[b:b + 1, :L], [L], ITEM_SCALES[b], sid[b:b + 1], seed=9, marks=True)),
                        _both_paths(lib, lambda: hip_default.synthesize(ids[b:b + 1, :L], [L], SCALES, sid[b:b + 1], seed=9, marks=True,
                                                                        item_scales=ITEM_SCALES[b:b + 1]))):
            assert _same(w, g), b


@pytest.mark.parametrize("rate", (None, 8000), ids=lambda r: f"{r or NATIVE}Hz")
def test_fit_lands_on_the_frame_count(lib, hip_tiny, rate):
    ids, lens, sid, dur, pause = _batch_case(63)
    natural = np.where(np.arange(13)[None] < lens[:, None], dur, 0).sum(1)
    fit = np.array([int(natural[0] * 1.4) + int(pause[0].sum()), 0, 7 + int(pause[2].sum())], np.int32)  # item 1 is not fitted
    assert R.fit_margin(None, dur, lens, fit, token_pause=pause) >= 1e-9
    d, _, ylen, ratio = R.regulate(None, dur, lens, token_pause=pause, fit_frames=fit)
    assert ylen[0] == fit[0] and ylen[2] == fit[2]
    L, M = MR.ratio(NATIVE, rate)
    kw = dict(seed=5, marks=True, sample_rate=rate)
    for solo in (False, True):
        want = _both_paths(lib, lambda: hip_tiny.synthesize(ids, lens, SCALES, sid, forced_durations=d, solo=solo, **kw))
        got = _both_paths(lib, lambda: hip_tiny.synthesize(ids, lens, SCALES, sid, forced_durations=dur, token_pause=pause, fit_frames=fit,
                                                           fit_ratio=True, solo=solo, **kw))
        for path, w, g in zip(("fast", "eager"), want, got):
            assert _same(w, g[:3]), (solo, path)
            audio, olen, ends, s = g
            for b in (0, 2):
                assert olen[b] == MR.n_out(int(fit[b]) * HOP, L, M) == ends[b, lens[b] - 1], (b, olen, ends)
            assert np.allclose(s, ratio, rtol=1e-6, atol=0)
    # free-running, one utterance: the length, and the ratio's range
    one = slice(0, 1)
    _, ol = hip_tiny.synthesize(ids[one], lens[one], SCALES, sid[one], seed=5)
    F = int(round(1.2 * int(ol[0]) / HOP))
    for audio, olen, ends, s in _both_paths(lib, lambda: hip_tiny.synthesize(ids[one], lens[one], SCALES, sid[one], fit_frames=[F], fit_ratio=True, **kw)):
        assert olen[0] == MR.n_out(F * HOP, L, M) == ends[0, 12] == audio.shape[1]
        assert 0.25 <= s[0] <= 4.0


def test_controlled_stream_equals_the_controlled_call(lib, hip_tiny):
    """the chunks against the one-shot call at the suite's figure for stream against one-shot (windows are decoded by other kernel
    choices than the whole utterance, test_streaming_chunks_equal_one_shot); the sample count and the marks exactly"""
    rng = np.random.default_rng(64)
    Tx = 21
    ids = rng.integers(1, 20, size=(1, Tx)).astype(np.int64)
    dur = rng.integers(1, 5, size=(1, Tx)).astype(np.int32)
    pause = np.zeros((1, Tx), np.int32)
    pause[0, [3, 20]] = [5, 9]
    fit = np.array([int(dur.sum() * 1.4) + 14], np.int32)
    assert R.fit_margin(None, dur, [Tx], fit, token_pause=pause) >= 1e-9
    for rate in (None, 8000):
        ctl = dict(forced_durations=dur, token_pause=pause, fit_frames=fit, seed=3, sample_rate=rate)
        one, olen, ends = hip_tiny.synthesize(ids, [Tx], SCALES, [2], marks=True, **ctl)
        assert olen[0] == MR.n_out(int(fit[0]) * HOP, *MR.ratio(NATIVE, rate))
        got_ends, got_ratio = [], []
        chunks = list(hip_tiny.stream(ids, SCALES, 2, chunk_frames=16, on_marks=got_ends.append, fit_ratio=got_ratio.append, **ctl))
        got = np.concatenate(chunks)[None]
        assert got.shape == one.shape and np.array_equal(got_ends[0][None], ends)
        assert 0.25 <= got_ratio[0][0] <= 4.0
        assert_close("stream vs one-shot", one, got, KERNEL_CHOICE_TOL)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _refusals():
    ids, lens, sid, dur, pause = _batch_case(65)
    ones = np.ones((3, 13), np.float32)
    nan, big = ones.copy(), ones.copy()
    nan[1, 2] = np.nan
    big[0, 7] = 17.0
    neg = pause.copy()
    neg[0, 5] = -2
    P = int(pause[0].sum())
    return ids, lens, sid, dur, [
        ("NaN in token_length_scale", dict(token_length_scale=nan), 1, r"token_length_scale\[1, 2\] = -?nan"),
        ("17 in token_length_scale", dict(token_length_scale=big), 1, r"token_length_scale\[0, 7\] = 17"),
        ("negative pause", dict(token_pause=neg), 1, r"token_pause\[0, 5\] = -2"),
        ("fit <= sum of pauses", dict(forced_durations=dur, token_pause=pause, fit_frames=[P, 0, 0]), 4, rf"item 0 .*F = {P} .*P = {P} "),
        ("fit needs s > 4", dict(forced_durations=dur, fit_frames=[0, 10 * int(dur[1, :5].sum()), 0]), 4, r"item 1 .*F = 80 .*s = .* = 10,"),
        ("token_length_scale with forced durations", dict(forced_durations=dur, token_length_scale=ones), 1, r"token_length_scale with forced_durations"),
    ]


def test_refusals_name_the_value_and_leave_the_engine_usable(lib, hip_tiny):
    from vosk_tts_amd import capi
    from vosk_tts_amd.capi import VitsError

    ids, lens, sid, dur, cases = _refusals()
    for fast in (1, 0):
        try:
            lib.lib.vits_debug_fast_path(fast)
            plain = hip_tiny.synthesize(ids, lens, SCALES, sid, forced_durations=dur, seed=2)
            for name, kw, code, pattern in cases:
                with pytest.raises(VitsError, match=pattern) as e:
                    hip_tiny.synthesize(ids, lens, SCALES, sid, seed=2, **kw)
                assert e.value.code == code, (name, fast, str(e.value))
                assert _same(plain, hip_tiny.synthesize(ids, lens, SCALES, sid, forced_durations=dur, seed=2)), (name, fast)  # d_err is cleared
            # the flag with a NULL struct
            opts = capi.SynthProsodyOpts()
            opts.flags = capi.FLAG_PROSODY
            out, ns, olen = capi.c_f32p(), ctypes.c_int64(), np.zeros(3, np.int64)
            rc = lib._fn("synthesize")(hip_tiny._h, capi._p(ids, capi.c_i64p), capi._p(lens, capi.c_i64p), 3, 13, capi._p(SCALES, capi.c_f32p),
                                       capi._p(sid, capi.c_i64p), ctypes.byref(opts), ctypes.byref(out), ctypes.byref(ns), capi._p(olen, capi.c_i64p))
            assert rc == 1 and b"NULL prosody" in lib._fn("last_error")()
        finally:
            lib.lib.vits_debug_fast_path(1)
    # the door refuses the same values, and a stream open too
    with pytest.raises(VitsError, match=r"token_pause\[0, 5\] = -2") as e:
        lib.op_regulate(None, dur, lens, token_pause=cases[2][1]["token_pause"])
    assert e.value.code == 1
    with pytest.raises(VitsError, match=r"item 0 .*s = ") as e:
        lib.op_regulate(None, dur[:1], lens[:1], fit_frames=[100 * int(dur[0].sum())])
    assert e.value.code == 4
    with pytest.raises(VitsError, match=r"item 0 .*s = ") as e:
        next(hip_tiny.stream(ids[:1], SCALES, 0, forced_durations=dur[:1], fit_frames=[100 * int(dur[0].sum())]))
    assert e.value.code == 4
    assert _same(plain, hip_tiny.synthesize(ids, lens, SCALES, sid, forced_durations=dur, seed=2))


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def test_synth_duration_and_pauses_on_the_toy_voice(lib, tmp_path):
    from vosk_tts_amd import Model, Synth
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.toymodel import PHONEMES, write_toy_model

    write_toy_model(str(tmp_path), W.tiny_hparams(n_vocab=len(PHONEMES)))
    model = Model(model_path=str(tmp_path), device=0)
    try:
        synth = Synth(model)
        text = "прив+ет, м+ир!"
        rate, hop = synth.native_rate(), synth.hop_length()
        want = int(round(1.5 * rate / hop)) * hop
        assert synth.synth_audio(text, speaker_id=2, duration=1.5).shape == (want,)
        assert sum(len(c) for c in synth.synth_stream(text, speaker_id=2, duration=1.5, chunk_frames=32)) == want
        pcm8k, marks = synth.synth_audio(text, speaker_id=2, duration=1.5, sample_rate=8000, marks=True)
        assert pcm8k.shape == (MR.n_out(want, *MR.ratio(rate, 8000)),) and marks.words[-1][2] <= pcm8k.shape[0]
        # a pause behind word 0 moves word 1 by that many frames and leaves word 0 where it was (forced durations: nothing else moves)
        args, _ = synth._feed(text, 2, None, None, None, None)
        T = args["input"].shape[1]
        base = dict(args, **{"vits.forced_durations": np.full((1, T), 2, np.int32), "vits.marks": True, "vits.seed": 3})
        ctl = dict(base)
        assert synth._prosody(ctl, synth.normalize(text), pauses={0: 0.2})
        m0 = synth._marks(text, model.onnx.run(None, base)[1], rate)
        m1 = synth._marks(text, model.onnx.run(None, ctl)[1], rate)
        frames = int(round(0.2 * rate / hop))
        assert frames == 17 and [w[0] for w in m0.words] == ["прив+ет", "м+ир"]
        assert m1.words[0] == m0.words[0]
        assert m1.words[1][1] - m0.words[1][1] == frames * hop == m1.words[1][2] - m0.words[1][2]
        # a slower word is longer, the other one keeps its length
        slow = dict(base)
        slow.pop("vits.forced_durations")
        fast = dict(slow)
        synth._prosody(slow, synth.normalize(text), word_rates={1: 0.5})
        synth._prosody(fast, synth.normalize(text), word_rates={1: 1.0})
        ms, mf = synth._marks(text, model.onnx.run(None, slow)[1], rate), synth._marks(text, model.onnx.run(None, fast)[1], rate)
        assert ms.words[0] == mf.words[0] and ms.words[1][2] - ms.words[1][1] > mf.words[1][2] - mf.words[1][1]
    finally:
        model.onnx.close()
