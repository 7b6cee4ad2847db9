"""Eviction and rebuild in the graph-replayed host path (csrc/ctx_cache.hip.h behind engine_fastpath.hip.h and stts.hip.h): one more
context than each cap keeps, then the evicted one again.  The fast path promises exact repeats (test_hip_parity.py, "repeat exactly
for repeated inputs"), so every assertion is bit equality of a repeated call with its own first result: a rebuilt front, back or rate
computes what the first one did.  On the first bucket of each family the existing fast-vs-eager bound keeps garbage from passing.
Smallest shapes that reach the code: B = 1, 5 tokens, forced durations, fixed seeds."""
import hashlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT, assert_close
from vosk_tts_amd.session import BACK_SESSIONS_PER_FRONT

pytestmark = pytest.mark.gpu

SCALES = np.array([0.667, 1.0, 0.8], np.float32)
IDS = np.array([[3, 7, 1, 12, 5]], np.int64)
RATES_PER_BACK = 4  # csrc/ctx_cache.hip.h VITS_RATES_PER_BACK
STTS_BACKS_PER_FRONT = 4  # csrc/ctx_cache.hip.h


def _dur(frames, tokens=5):
    """forced durations of `tokens` tokens that sum to `frames`"""
    d = np.full((1, tokens), frames // tokens, np.int32)
    d[0, 0] += frames - int(d.sum())
    return d


def _eager(hip_lib, fn):
    hip_lib.lib.vits_debug_fast_path(0)
    try:
        return fn()
    finally:
        hip_lib.lib.vits_debug_fast_path(1)


def test_backs_evicted_and_rebuilt(hip_lib, hip_tiny):
    """BACK_SESSIONS_PER_FRONT + 2 frame buckets of one T_x bucket (16, 48, 80, ... frames), the first again, all once more in reverse"""
    frames = [16 + 32 * k for k in range(BACK_SESSIONS_PER_FRONT + 2)]
    call = lambda f: hip_tiny.synthesize(IDS, [5], SCALES, [2], forced_durations=_dur(f), seed=11)
    first = {}
    for f in frames:
        first[f], olen = call(f)
        assert olen[0] == f * 256 and first[f].shape == (1, f * 256) and np.abs(first[f]).max() > 1e-4
    a_e, l_e = _eager(hip_lib, lambda: call(frames[0]))
    assert l_e[0] == frames[0] * 256
    assert_close("fast vs eager, first bucket", a_e, first[frames[0]], 2e-5)
    for f in [frames[0]] + frames[::-1]:
        assert np.array_equal(call(f)[0], first[f]), f"{f} frames: a rebuilt back context computes something else"


def test_rates_evicted_and_rebuilt(hip_tiny):
    """on one frame bucket: one output rate more than a back keeps, then the first again, float and int16; the native rate around them"""
    rates = [8000, 11025, 16000, 24000, 44100]
    assert len(rates) == RATES_PER_BACK + 1
    kw = dict(forced_durations=_dur(16), seed=12)
    native = hip_tiny.synthesize(IDS, [5], SCALES, [1], **kw)[0]
    native16 = hip_tiny.synthesize_pcm16(IDS, [5], SCALES, [1], **kw)[0]
    first = {}
    for r in rates:
        first[r] = (hip_tiny.synthesize(IDS, [5], SCALES, [1], sample_rate=r, **kw)[0], hip_tiny.synthesize_pcm16(IDS, [5], SCALES, [1], sample_rate=r, **kw)[0])
        assert first[r][0].shape == first[r][1].shape and first[r][0].shape[1] == -(-16 * 256 * r // 22050) and np.abs(first[r][0]).max() > 1e-4
    for r in [rates[0]] + rates[::-1]:
        assert np.array_equal(hip_tiny.synthesize(IDS, [5], SCALES, [1], sample_rate=r, **kw)[0], first[r][0]), r
        assert np.array_equal(hip_tiny.synthesize_pcm16(IDS, [5], SCALES, [1], sample_rate=r, **kw)[0], first[r][1]), r
    assert np.array_equal(hip_tiny.synthesize(IDS, [5], SCALES, [1], **kw)[0], native)
    assert np.array_equal(hip_tiny.synthesize_pcm16(IDS, [5], SCALES, [1], **kw)[0], native16)


# The child of test_fronts_*: with VITS_CACHE_MB=0 only one idle front survives a release, so three T_x buckets in round robin rebuild
# their front in every round.  Per call one line "<round> <tokens> <sha256 audio> <sha256 audio of the marks call> <token ends>".
_CHILD = r"""
import hashlib, sys
import numpy as np
import torch  # (before the product library, as tests/conftest.py)
sys.path.insert(0, sys.argv[1])
from vosk_tts_amd import weights as W
from vosk_tts_amd.capi import VitsLib
m = VitsLib().create(W.synthetic_blob(W.tiny_hparams(), 1234), 0)
sc = np.array([0.667, 1.0, 0.8], np.float32)
h = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
for rnd in range(3):
    for T in (5, 13, 21):
        ids = (np.arange(T, dtype=np.int64)[None] * 7 + 3) % 19 + 1
        dur = np.full((1, T), 2, np.int32)
        a, _ = m.synthesize(ids, [T], sc, [2], forced_durations=dur, seed=13)
        am, _, ends = m.synthesize(ids, [T], sc, [2], forced_durations=dur, seed=13, marks=True)
        assert np.abs(a).max() > 1e-4
        print("call", rnd, T, h(a), h(am), ",".join(str(int(e)) for e in ends[0]), flush=True)
"""


@pytest.fixture(scope="module")
def fronts_child():
    env = dict(os.environ, VITS_CACHE_MB="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    calls = {}
    for line in r.stdout.splitlines():
        if line.startswith("call "):
            _, rnd, T, ha, ham, ends = line.split()
            calls[int(rnd), int(T)] = (ha, ham, [int(e) for e in ends.split(",")])
    assert len(calls) == 9, r.stdout
    return calls


def test_fronts_evicted_and_rebuilt(fronts_child):
    for T in (5, 13, 21):
        ha, ham, _ = fronts_child[0, T]
        assert ha == ham  # (the marks call returns the samples of the plain one)
        for rnd in (1, 2):
            assert fronts_child[rnd, T][:2] == (ha, ham), f"round {rnd}, {T} tokens: a rebuilt front context computes something else"
    assert len({fronts_child[0, T][0] for T in (5, 13, 21)}) == 3


def test_marks_on_a_rebuilt_front(fronts_child):
    """the mark buffers are allocated by the first marks request of a front, and again after that front was evicted and rebuilt"""
    for T in (5, 13, 21):
        ends = fronts_child[0, T][2]
        assert ends == [2 * 256 * (t + 1) for t in range(T)]
        for rnd in (1, 2):
            assert fronts_child[rnd, T][2] == ends


@pytest.fixture(scope="module")
def stts_small(hip_lib):
    from vosk_tts_amd import weights as W
    from vosk_tts_amd import weights_stts as S
    from vosk_tts_amd.capi_stts import SttsModel

    hip = SttsModel(hip_lib, S.synthetic_blob(S.default_hparams(30, 1), 99), hip_lib.create(W.synthetic_blob(W.hifigan_v1_vocoder_hparams(), 1234), 0))
    yield hip
    hip.close()


STTS_IDS = np.random.default_rng(5).integers(1, 30, size=(5, 5)).astype(np.int64)
STTS_PDE = np.full(5, 4.0, np.float32)


def test_stts_backs_evicted_and_rebuilt(hip_lib, stts_small):
    """n_timesteps 1..5 at one length: five (frame bucket, n_steps) backs where a front keeps four, then the first again"""
    sc = np.array([0.6, 0.9, 0.8], np.float32)
    call = lambda n: stts_small.synthesize(STTS_IDS, sc, 0, None, STTS_PDE, seed=1, n_timesteps=n)
    first = {n: call(n) for n in range(1, STTS_BACKS_PER_FRONT + 2)}
    a_e, m_e = _eager(hip_lib, lambda: call(1))
    assert_close("mel, fast vs eager", m_e, first[1][1], 2e-5)
    assert_close("audio, fast vs eager", a_e, first[1][0], 5e-5)
    assert np.abs(first[1][0]).max() > 1e-4 and not np.array_equal(first[1][1], first[2][1])
    for n in [1] + list(range(STTS_BACKS_PER_FRONT + 1, 0, -1)):
        a, m = call(n)
        assert np.array_equal(a, first[n][0]) and np.array_equal(m, first[n][1]), f"{n} steps: a rebuilt back context computes something else"


def _two_threads(call, seeds):
    """call(seed) from two threads at once, every seed in each: all results, with what went wrong in a thread"""
    out, errs = [{}, {}], []

    def run(k):
        try:
            for s in seeds:
                out[k][s] = call(s)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    return out


def test_two_threads_on_one_bucket(hip_lib, hip_tiny, stts_small):
    """two threads on the same T_x bucket, four calls each: each takes a front of its own (a second one is built, and both are idle
    afterwards -- kept side by side for VITS, the newer in place of the older for StableTTS); every result is the single-threaded one.
    A single VITS utterance that starts while another call is in flight runs its stages as launches, not as the persistent programs
    (engine_session.hip.h PersistScope: "slower, never wrong"), and the two forms round differently (seen: 1e-8 of the scale, on the
    library before and after this file's change alike).  So "the single-threaded one" is the single-threaded call of the form the
    threaded call took: bit equality with either, nothing in between."""
    seeds = [21, 22, 23, 24]
    vits = lambda s: hip_tiny.synthesize(IDS, [5], SCALES, [3], forced_durations=_dur(16), seed=s)[0]
    sc = np.array([0.6, 0.9, 0.8], np.float32)
    stts = lambda s: stts_small.synthesize(STTS_IDS, sc, 0, None, STTS_PDE, seed=s, n_timesteps=2, want_mel=False)[0]
    for name, call in (("vits", vits), ("stts", stts)):
        want = {s: call(s) for s in seeds}
        hip_lib.lib.vits_debug_persist(0)
        try:
            want_launches = {s: call(s) for s in seeds}
        finally:
            hip_lib.lib.vits_debug_persist(7)
        assert not np.array_equal(want[21], want[22])
        for got in _two_threads(call, seeds):
            for s in seeds:
                assert np.array_equal(got[s], want[s]) or np.array_equal(got[s], want_launches[s]), (name, s)
        for s in seeds:  # and the contexts the threads left behind serve the next calls
            assert np.array_equal(call(s), want[s]), (name, s)
