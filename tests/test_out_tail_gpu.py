"""GPU test of the output tail as a whole (DESIGN.md "Output tail"; csrc/out_tail.hip.h): every combination of the stages behind the
decoder -- pitch x rate x last stage x output type -- on both host paths, against the chained parity doors

    op_pitch_shift -> op_resample -> op_loudness_normalize | op_limit | op_loudness_limit -> _pcm16

applied to the same path's own unflagged, native-rate float output.  That is the reference of the per-feature tests
(tests/test_{resample,loudness,pitch,limit}_gpu.py), which hold single stages and a few pairs; here the cross product is held.

Bounds: none.  Every cell is compared bit for bit (audio, lengths, and the loudness / gain / reduction rows with tobytes()), as the
per-feature tests compare the cells they cover: the tail runs the doors' kernels on the same bytes, and neither path's decoder enters
the comparison because each path is compared with its own unflagged output."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCALES = [0.667, 1.0, 0.8]
NATIVE = 22050
PITCH, RATE, PCM_SCALE = 3.0, 16000, 0.9
KW = dict(seed=6, solo=True)
LAST = ("none", "loudness", "limit", "loudness+limit")


def _pcm16(audio, scale):
    """the conversion of vits_synthesize_pcm16 in fp32: scale, * 32767, clip, truncating cast"""
    v = np.asarray(audio, np.float32) * np.float32(scale)
    v = v * np.float32(32767.0)
    return np.trunc(np.clip(v, np.float32(-32767.0), np.float32(32767.0))).astype(np.int16)


def _ragged(rng, B, Tx=24, n_vocab=20):
    lens = np.array([Tx, Tx - 9, 5][:B], np.int64)
    ids = rng.integers(1, n_vocab, size=(B, Tx)).astype(np.int64)
    sid = rng.integers(0, 4, size=B).astype(np.int64)
    return ids, lens, sid


def _settings(lib, x, ol, hz):
    """settings under which every stage does something to this audio (the idea of tests/test_limit_gpu.py::_settings): a LUFS target
    6 LU above the loudest item, without a cap for the plain gain; a true-peak limiter alone with its ceiling at 0.7 of the quietest
    item's peak; and for the two-pass form the ceiling at 1.2 of that peak (at most 1), which the +6 LU gain exceeds"""
    from vosk_tts_amd.capi import limit_spec, loudness_spec

    loud, peak = lib.op_loudness(x, ol, hz)
    assert np.isfinite(loud).all() and peak.min() > 0
    target = min(0.0, float(loud.max()) + 6.0)
    return dict(loud=loudness_spec(loudness=target, peak_ceiling=0.0), target=target,
                alone=limit_spec("true", min(1.0, 0.7 * float(peak.min())), 2.0, 30.0, 1.0),
                two=limit_spec("true", min(1.0, 1.2 * float(peak.min()))))


class _Path:
    """one host path: the fast one as it is, the eager one with vits_debug_fast_path(0) around every call"""

    def __init__(self, lib, model, fast):
        self.lib, self.model, self.fast = lib, model, fast

    def call(self, fn, *a, **kw):
        self.lib.lib.vits_debug_fast_path(1 if self.fast else 0)
        try:
            return fn(*a, **kw)
        finally:
            self.lib.lib.vits_debug_fast_path(1)


@pytest.fixture(scope="module")
def feed():
    return _ragged(np.random.default_rng(47), 3)


@pytest.fixture(scope="module")
def references(hip_lib, hip_tiny, feed):
    """per path: the unflagged native-rate float output, and from it, per (pitch, rate), the input of the last stage with its lengths,
    the settings and the four last-stage references {name: (audio, result rows)}.  Computed once, never written to."""
    lib = hip_lib
    assert lib.has_limit and lib.has_pitch and lib.has_loudness
    ids, lens, sid = feed
    refs = {}
    for fast in (True, False):
        path = _Path(lib, hip_tiny, fast)
        plain, ol = path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, **KW)
        assert ol.min() > 0
        for pitch, rate in itertools.product((None, PITCH), (None, RATE)):
            x, n, hz = plain, ol, NATIVE
            if pitch:
                x = lib.op_pitch_shift(x, n, pitch)
                assert not np.array_equal(x, plain)
            if rate:
                x = lib.op_resample(x, n, NATIVE, rate)
                n, hz = np.array([lib.out_samples(k, NATIVE, rate) for k in n], np.int64), rate
            st = _settings(lib, x, n, hz)
            yl, ll, gl = lib.op_loudness_normalize(x, n, hz, *st["loud"])
            ya, ra = lib.op_limit(x, n, hz, *st["alone"])
            y2, l2, g2, r2 = lib.op_loudness_limit(x, n, hz, st["target"], *st["two"][:4])
            # every stage did something: 6 LU above the loudest item is a gain of 2 or more for every item (1.5: a target capped at
            # 0 LUFS would still have to gain), and both limiters reduce every item
            assert (gl > 1.5).all() and (g2 > 1.5).all() and (ra < 1).all() and (r2 < 1).all()
            for a in (x, yl, ya, y2, ll, gl, ra, l2, g2, r2):
                a.setflags(write=False)
            refs[fast, pitch, rate] = dict(lengths=n, settings=st, want={
                "none": (x, {}), "loudness": (yl, dict(loudness=ll, gain=gl)), "limit": (ya, dict(reduction=ra)),
                "loudness+limit": (y2, dict(loudness=l2, gain=g2, reduction=r2))})
    return refs


@pytest.mark.parametrize("rate", (None, RATE), ids=("native", "16000"))
@pytest.mark.parametrize("pitch", (None, PITCH), ids=("unshifted", "shifted"))
@pytest.mark.parametrize("fast", (True, False), ids=("fast", "eager"))
def test_every_tail_equals_the_ops_chained(hip_lib, hip_tiny, feed, references, fast, pitch, rate):
    ids, lens, sid = feed
    ref = references[fast, pitch, rate]
    st = ref["settings"]
    flags = {"none": {}, "loudness": dict(loudness=st["loud"]), "limit": dict(limit=st["alone"]),
             "loudness+limit": dict(loudness=st["loud"], limit=st["two"])}
    path = _Path(hip_lib, hip_tiny, fast)
    for last in LAST:
        want, rows = ref["want"][last]
        kw = dict(KW, sample_rate=rate, pitch=pitch, **flags[last])
        out = {}
        got, gl = path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, loudness_out=out, **kw)
        assert gl.tobytes() == ref["lengths"].tobytes(), last
        assert got.shape[1] == int(gl.max()) and got.tobytes() == want[:, :got.shape[1]].tobytes(), last
        assert sorted(out) == sorted(rows), last
        for k, v in rows.items():
            assert out[k].tobytes() == v.tobytes(), (last, k)
        out16 = {}
        pcm, pl = path.call(hip_tiny.synthesize_pcm16, ids, lens, SCALES, sid, pcm_scale=PCM_SCALE, loudness_out=out16, **kw)
        assert pl.tobytes() == gl.tobytes() and pcm.dtype == np.int16, last
        assert pcm.tobytes() == _pcm16(want[:, :got.shape[1]], PCM_SCALE).tobytes(), last
        for k, v in rows.items():
            assert out16[k].tobytes() == v.tobytes(), (last, k)
