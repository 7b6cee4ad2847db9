"""GPU tests of the look-ahead peak limiter (include/vits_limit.h): the kernels through vits_op_true_peak / vits_op_limit_gain /
vits_op_limit / vits_op_loudness_limit against the float64 restatement (tests/limit_ref.py), the flag through the VITS and multistream
entry points against the ops on the unflagged call's audio, and the Python layers.

Bounds.
  True peak: the worst-case error of an fp32 sum of 33 products against the exact one, resample_ref.fp32_bound of the 4 x 33 table at the
  item's max |x| (the restatement sums the same fp32 table in float64).
  Gain curve s: the yardstick is what the restatement run in float32 (steps 2-5) differs from its float64 run by on the same inputs; the
  device forms those steps in double but in another order (a sliding maximum of p in place of a minimum of r, the deficit 1 - e, a prefix
  sum in place of a window sum) and returns fp32(s), so it is allowed 4 times the yardstick, the margin the pitch tests took over theirs
  and for the same reason, in either mode: in true-peak mode the device's envelope is the fp32 sum where the restatement rounds the
  float64 sum, and that difference has to fit inside the same allowance.  Measured on these inputs, max |s32 - s64| of the restatement
  over the three batches: W = 1: 2.7e-6, W = 40: 1.3e-6, W = 1024: 2.0e-7, the same in either mode to two digits (allowed: 1.1e-5,
  5.1e-6, 8.0e-7); the device against float64 on an MI355X: 3.0e-8 in sample mode at every W (the rounding of s to fp32),
  3.2e-7 / 3.3e-7 / 1.3e-7 in true-peak mode (its fp32 envelope).
  Eager against fast path: the decoder runs on other launch shapes, and the limited outputs may differ by what the unflagged outputs of
  the two paths differ by, with the project's floor of 1e-4 of the peak (tests/test_loudness_gpu.py) under it; measured 5.9e-7 unflagged,
  1.0e-6 limited.
  Exact conditions, sample mode (p = |x| is the device's own envelope): |y| <= c (1 + 4 ulp); y = 0 and s = 1 beyond the length;
  reduction = min s; an item that never reaches the ceiling has s = 1 and y = fp32(g x); the same call twice gives the same bits.
  Two-pass form: the returned gain within 10^(0.02/20) - 1 of the restatement's g_1 (two measurements, each inside the 0.01 LU of
  tests/test_loudness_gpu.py); tests/test_limit.py asserts, on the restatement alone, that no block of x or of y_0 lies within 0.05 LU of
  either gate, so no case is skipped or retried."""
import numpy as np
import pytest

import limit_ref as R
import loudness_ref
import resample_ref

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
G2_TOL = 10.0 ** (0.02 / 20.0) - 1.0
C, G = 0.5, 2.0                      # ceiling and pre-gain of the kernel-level cases: the peaks of limit_ref.spiky reach 1.9, its noise 0.1
# W -> (rate, lookahead_ms): W = round(lookahead_ms * rate / 1000), lookahead_ms <= 10
GEOM = {1: (8000, 0.125), 40: (8000, 5.0), 1024: (102400, 10.0)}
RELEASE_MS = 20.0


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert hip_lib.has_limit, "libvits_mi355.so exports no vits_op_limit"
    return hip_lib


def _rows(items):
    lens = np.array([r.shape[0] for r in items], np.int64)
    x = np.full((len(items), max(int(lens.max()), 1)), np.nan, np.float32)
    for b, r in enumerate(items):
        x[b, :r.shape[0]] = r
    return x, lens


@pytest.mark.parametrize("rate", R.RATES)
def test_op_true_peak_against_float64(lib, rate):
    T, H = R.TILE, R.HALF
    items = [np.zeros(T + 1), np.zeros(0), np.array([0.7]), np.array([-0.25])]
    items += [loudness_ref.sine(rate, n, amp=0.8) for n in (H - 1, H, H + 1, T - 1, T, T + 1, T + H, 2 * T + H + 1)]
    items += [R.alternating(n) for n in (H + 1, T + 1, 2 * T - 1)]
    x, lens = _rows([np.asarray(i, np.float32) for i in items])
    tp = lib.op_true_peak(x, lens, rate)
    assert tp.shape == lens.shape and tp.dtype == np.float32
    tab = R.table4(rate)
    worst = 0.0
    for b in range(x.shape[0]):
        xi = x[b, :lens[b]]
        want = R.true_peak(xi, rate)
        bound = resample_ref.fp32_bound(tab, np.abs(xi).max() if lens[b] else 0.0)
        err = abs(float(tp[b]) - want)
        worst = max(worst, err)
        assert err <= bound + 2.0 ** -24 * want, f"{rate} Hz item {b} (len {lens[b]}): {tp[b]:.7f} vs {want:.7f} ({err:.2e} > {bound:.2e})"
        assert tp[b] >= (np.abs(xi).max() if lens[b] else 0)  # the samples themselves are part of the envelope
    print(f"{rate} Hz: max |tp_gpu - tp_ref| = {worst:.2e} over {x.shape[0]} items")
    assert tp[0] == 0 and tp[1] == 0
    assert lib.op_true_peak(x, lens, rate).tobytes() == tp.tobytes()


@pytest.fixture(scope="module")
def yardstick():
    """(mode, W) -> max |s32 - s64| of the restatement over the inputs of test_op_limit_against_float64, computed once"""
    out = {}
    for W, (rate, la) in GEOM.items():
        for mode in (R.SAMPLE, R.TRUE):
            d = 0.0
            for x, lens in R.op_batches(W):
                for b in range(x.shape[0]):
                    xi = x[b, :lens[b]]
                    s64 = R.limit(xi, rate, mode, C, la, RELEASE_MS, G)["s"]
                    s32 = R.limit(xi, rate, mode, C, la, RELEASE_MS, G, dtype=np.float32)["s"]
                    if s64.size:
                        d = max(d, float(np.abs(s32.astype(np.float64) - s64).max()))
            out[(mode, W)] = d
    return out


@pytest.mark.parametrize("W", sorted(GEOM))
@pytest.mark.parametrize("mode", (R.SAMPLE, R.TRUE), ids=("sample", "true"))
def test_op_limit_against_float64(lib, yardstick, mode, W):
    rate, la = GEOM[W]
    assert lib.limit_plan(rate, la, RELEASE_MS)[0] == W == R.plan(rate, la, RELEASE_MS)[0]
    d32 = yardstick[(mode, W)]
    tol = 4.0 * d32
    print(f"W {W} mode {mode}: float32 restatement differs from float64 by {d32:.2e}; the device is allowed {tol:.2e}")
    assert d32 > 0
    worst, limited, free = 0.0, 0, 0
    for x, lens in R.op_batches(W):
        s = lib.op_limit_gain(x, lens, rate, mode, C, la, RELEASE_MS, G)
        y, red = lib.op_limit(x, lens, rate, mode, C, la, RELEASE_MS, G)
        assert s.shape == y.shape == x.shape and s.dtype == y.dtype == np.float32 and red.shape == lens.shape
        for b in range(x.shape[0]):
            n = int(lens[b])
            xi, si, yi = x[b, :n], s[b, :n], y[b, :n]
            assert not y[b, n:].any() and (s[b, n:] == 1).all()          # NaN beyond the length does not leak
            assert np.isfinite(si).all() and np.isfinite(yi).all()
            assert red[b] == (si.min() if n else 1.0)
            ref = R.limit(xi, rate, mode, C, la, RELEASE_MS, G)
            if n:
                err = float(np.abs(si.astype(np.float64) - ref["s"]).max())
                worst = max(worst, err)
                assert err <= tol, f"W {W} mode {mode} len {n}: max |s_gpu - s_ref| = {err:.2e} > {tol:.2e} at {int(np.abs(si - ref['s']).argmax())}"
                # y = fp32(fp32(g s) x): from the returned fp32(s) to within the second rounding of s
                assert np.all(np.abs(yi.astype(np.float64) - G * si.astype(np.float64) * xi) <= 3 * ULP * np.abs(yi) + 1e-45)
            if mode == R.SAMPLE:
                assert np.all(np.abs(yi) <= C * (1 + 4 * ULP))
            never = n == 0 or G * float(ref["p"].max()) * (1 + 1e-5) <= C
            if never:
                free += 1
                assert (si == 1).all() and np.array_equal(yi, np.float32(G) * xi)
            elif (ref["r"] < 1 - 1e-5).any():
                limited += 1
                assert red[b] < 1
        again = lib.op_limit(x, lens, rate, mode, C, la, RELEASE_MS, G)
        assert again[0].tobytes() == y.tobytes() and again[1].tobytes() == red.tobytes()
    print(f"W {W} mode {mode}: max |s_gpu - s_ref| = {worst:.2e}; {limited} items limited, {free} never reach the ceiling")
    assert limited >= 6 and free >= 3


@pytest.mark.parametrize("mode", (R.SAMPLE, R.TRUE), ids=("sample", "true"))
@pytest.mark.parametrize("rate", (8000, 22050))
def test_op_loudness_limit_two_pass(lib, rate, mode):
    x, lens = R.two_pass_items(rate)
    T, c = R.TWO_PASS_TARGET, R.TWO_PASS_CEILING
    y, loud, gain, red = lib.op_loudness_limit(x, lens, rate, T, mode, c)
    assert y.shape == x.shape and y.dtype == np.float32
    for b in range(x.shape[0]):
        n = int(lens[b])
        ref = R.loudness_limit(x[b, :n], rate, T, mode, c, 5.0, 50.0)
        rel = abs(float(gain[b]) / ref["g1"] - 1.0)
        print(f"{rate} Hz mode {mode} item {b}: L {loud[b]:.3f} vs {ref['L']:.3f}, gain {gain[b]:.6f} vs g_1 {ref['g1']:.6f} (g_0 {ref['g0']:.6f}; "
              f"rel {rel:.2e}, bound {G2_TOL:.2e}), reduction {red[b]:.4f} vs {ref['reduction']:.4f}")
        assert abs(float(loud[b]) - ref["L"]) <= 0.01
        assert rel <= G2_TOL
        one, red1 = lib.op_limit(x[b:b + 1], lens[b:b + 1], rate, mode, c, gain=float(gain[b]))
        assert one.tobytes() == y[b:b + 1].tobytes() and red1[0] == red[b]  # the one-pass limiter at the returned gain, bit for bit
        assert not y[b, n:].any()
    # item 0 is limited in both passes; item 1 reaches the target without limiting: the un-capped normalisation, bit for bit
    assert red[0] < 0.95 and red[1] == 1
    yn, ln, gn = lib.op_loudness_normalize(x, lens, rate, loudness_ref.LUFS, T, 0.0)
    assert y[1].tobytes() == yn[1].tobytes() and gain[1] == gn[1] and loud.tobytes() == ln.tobytes()
    again = lib.op_loudness_limit(x, lens, rate, T, mode, c)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((y, loud, gain, red), again))


def test_refusals_by_value(lib):
    from vosk_tts_amd.capi import VitsError

    x, lens = np.zeros((1, 64), np.float32), np.array([64])
    for kw, code, word in ((dict(ceiling=0.0), 1, "ceiling"), (dict(ceiling=1.5), 1, "ceiling"), (dict(lookahead_ms=0.0), 1, "lookahead"),
                           (dict(lookahead_ms=11.0), 1, "lookahead"), (dict(release_ms=0.5), 1, "release"), (dict(release_ms=2000.0), 1, "release"),
                           (dict(gain=-1.0), 1, "gain"), (dict(gain=65.0), 1, "gain"), (dict(mode=3), 1, "mode"),
                           (dict(lookahead_ms=10.0, rate=200000), 4, "W = 2000"), (dict(lookahead_ms=0.01), 4, "W = 0")):
        a = dict(rate=8000, mode=R.SAMPLE, ceiling=0.9, lookahead_ms=5.0, release_ms=50.0, gain=1.0)
        a.update(kw)
        with pytest.raises(VitsError) as e:
            lib.op_limit(x, lens, a["rate"], a["mode"], a["ceiling"], a["lookahead_ms"], a["release_ms"], a["gain"])
        assert e.value.code == code and word in str(e.value), (kw, str(e.value))
    y, red = lib.op_limit(x + 0.5, lens, 8000, R.SAMPLE, 0.9)  # a normal request runs afterwards
    assert (y == 0.5).all() and red[0] == 1


# ---- VITS entry points ------------------------------------------------------------------------------------------------------------
SCALES = [0.667, 1.0, 0.8]
SC = np.array([0.8, 1.0, 0.8], np.float32)
NATIVE = 22050


def _lspec(*a, **kw):
    from vosk_tts_amd.capi import limit_spec

    return limit_spec(*a, **kw)


def _loud(target):
    from vosk_tts_amd.capi import loudness_spec

    return loudness_spec(loudness=target, peak_ceiling=0.0)  # (under the limit flag the loudness gain has no cap)


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


def _settings(lib, plain, ol, hz):
    """a plain limiter and a two-pass request that both limit this audio: the ceiling at 0.7 of the quietest item's peak, and a LUFS
    target 6 LU above the loudest item with the ceiling at 1.2 of that peak (at most 1)"""
    loud, peak = lib.op_loudness(plain, ol, hz)
    assert np.isfinite(loud).all() and peak.min() > 0
    alone = _lspec("sample", min(1.0, 0.7 * float(peak.min())), 2.0, 30.0, 1.0)
    target = min(0.0, float(loud.max()) + 6.0)
    two = _lspec("true", min(1.0, 1.2 * float(peak.min())))
    return alone, target, two


@pytest.fixture(scope="module")
def launch_path(hip_lib):
    """single utterances on the launch path for this module's bit-for-bit comparisons of two calls (whether a call takes the persistent
    programs depends on how busy the device is as it starts)"""
    hip_lib.lib.vits_debug_persist(0)
    yield
    hip_lib.lib.vits_debug_persist(7)


@pytest.mark.parametrize("solo", (False, True), ids=("padded", "solo"))
@pytest.mark.parametrize("rate", (None, 8000), ids=("native", "8000"))
@pytest.mark.parametrize("B", (3, 1))
def test_flagged_synthesize_is_the_op_on_the_unflagged_audio(lib, hip_tiny, launch_path, B, rate, solo):
    ids, lens, sid = _ragged(np.random.default_rng(41), B)
    hz = rate or NATIVE
    kw = dict(seed=7, solo=solo, sample_rate=rate)
    plain, ol, ends = hip_tiny.synthesize(ids, lens, SCALES, sid, marks=True, **kw)
    assert ol.min() > 0
    alone, target, two = _settings(lib, plain, ol, hz)
    want, wred = lib.op_limit(plain, ol, hz, *alone)
    y2, l2, g2, r2 = lib.op_loudness_limit(plain, ol, hz, target, *two[:4])
    assert (wred < 1).all() and (r2 < 1).all()
    for call_kw, w, res in ((dict(limit=alone), want, dict(reduction=wred)),
                            (dict(limit=two, loudness=_loud(target)), y2, dict(reduction=r2, gain=g2, loudness=l2))):
        out = {}
        got, gl = hip_tiny.synthesize(ids, lens, SCALES, sid, loudness_out=out, **call_kw, **kw)
        assert np.array_equal(gl, ol) and got.shape == plain.shape
        assert np.array_equal(got, w)
        for k, v in res.items():
            assert out[k].tobytes() == v.tobytes(), k
        scale = float(1.25 / np.abs(w).max())  # the loudest samples clip
        pcm, pl = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=scale, **call_kw, **kw)
        assert np.array_equal(pl, ol) and np.array_equal(pcm, _pcm16(w, scale))
        g3, l3, e3 = hip_tiny.synthesize(ids, lens, SCALES, sid, marks=True, **call_kw, **kw)
        assert np.array_equal(g3, w) and np.array_equal(l3, ol) and np.array_equal(e3, ends)  # lengths and marks do not change
        p3, _, e4 = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=scale, marks=True, **call_kw, **kw)
        assert np.array_equal(p3, pcm) and np.array_equal(e4, ends)


def test_eager_path_agrees_with_the_fast_path(lib, hip_tiny, launch_path):
    ids, lens, sid = _ragged(np.random.default_rng(42), 3)
    kw = dict(seed=5, solo=True)
    p0, l0 = hip_tiny.synthesize(ids, lens, SCALES, sid, **kw)
    _, target, two = _settings(lib, p0, l0, NATIVE)
    ck = dict(limit=two, loudness=_loud(target))
    fast = hip_tiny.synthesize(ids, lens, SCALES, sid, **ck, **kw)
    fast16 = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=0.7, **ck, **kw)
    lib.lib.vits_debug_fast_path(0)
    try:
        plain, ol = hip_tiny.synthesize(ids, lens, SCALES, sid, **kw)
        out = {}
        got, gl = hip_tiny.synthesize(ids, lens, SCALES, sid, loudness_out=out, **ck, **kw)
        want, wl, wg, wr = lib.op_loudness_limit(plain, ol, NATIVE, target, *two[:4])
        assert np.array_equal(got, want) and out["gain"].tobytes() == wg.tobytes() and out["reduction"].tobytes() == wr.tobytes()
        e16, _ = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=0.7, **ck, **kw)
        assert np.array_equal(e16, _pcm16(want, 0.7))
        # 8000 Hz, the plain limiter, through the eager resampler
        p8, o8 = hip_tiny.synthesize(ids, lens, SCALES, sid, sample_rate=8000, **kw)
        alone = _settings(lib, p8, o8, 8000)[0]
        g8, _ = hip_tiny.synthesize(ids, lens, SCALES, sid, sample_rate=8000, limit=alone, **kw)
        assert np.array_equal(g8, lib.op_limit(p8, o8, 8000, *alone)[0])
    finally:
        lib.lib.vits_debug_fast_path(1)
    # the two paths run the decoder on different launch shapes: equal within what their unflagged outputs differ by
    unflagged = np.abs(p0 - plain).max() / np.abs(plain).max()
    assert fast[0].shape == got.shape and np.array_equal(fast[1], gl)
    print(f"fast vs eager: unflagged {unflagged:.2e}, limited {np.abs(fast[0] - got).max() / np.abs(got).max():.2e}")
    assert np.abs(fast[0] - got).max() <= max(1e-4, unflagged) * np.abs(got).max()
    assert np.abs(fast16[0].astype(np.int32) - e16.astype(np.int32)).max() <= 2


@pytest.mark.parametrize("rate", (None, 16000), ids=("native", "16000"))
def test_pitch_loudness_and_limit_equal_the_ops_chained(lib, hip_tiny, launch_path, rate):
    ids, lens, sid = _ragged(np.random.default_rng(45), 3)
    kw = dict(seed=4, solo=True)
    plain, ol = hip_tiny.synthesize(ids, lens, SCALES, sid, **kw)
    shifted = lib.op_pitch_shift(plain, ol, 3.0)
    hz = rate or NATIVE
    if rate:
        shifted = lib.op_resample(shifted, ol, NATIVE, rate)
        ol = np.array([lib.out_samples(n, NATIVE, rate) for n in ol], np.int64)
    _, target, two = _settings(lib, shifted, ol, hz)
    want, wl, wg, wr = lib.op_loudness_limit(shifted, ol, hz, target, *two[:4])
    out = {}
    got, gl = hip_tiny.synthesize(ids, lens, SCALES, sid, pitch=3.0, loudness=_loud(target), limit=two, loudness_out=out, sample_rate=rate, **kw)
    assert np.array_equal(gl, ol) and np.array_equal(got, want[:, :got.shape[1]])
    assert out["gain"].tobytes() == wg.tobytes() and out["reduction"].tobytes() == wr.tobytes() and (wr < 1).all()
    pcm, _ = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=0.9, pitch=3.0, loudness=_loud(target), limit=two, sample_rate=rate, **kw)
    assert np.array_equal(pcm, _pcm16(got, 0.9))


def test_launches_with_and_without_the_flag(lib, hip_tiny, launch_path):
    ids = np.random.default_rng(43).integers(1, 20, size=(1, 16)).astype(np.int64)

    def dump(**kw):
        lib.launch_log(1)
        try:
            hip_tiny.synthesize_pcm16(ids, [16], SCALES, [1], seed=3, **kw)
        finally:
            lib.launch_log(0)
        return lib.launch_dump()

    lib.lib.vits_debug_fast_path(0)  # the eager path: one counted launch per kernel
    try:
        before = dump()
        loud_only = dump(loudness=_loud(-19.0))
        alone = dump(limit=_lspec("sample", 0.5))
        two = dump(limit=_lspec("true", 0.5), loudness=_loud(-19.0))
        after = dump()
    finally:
        lib.lib.vits_debug_fast_path(1)
    assert not any("loud" in k or "limit" in k for k in before) and before == after
    assert not any("limit" in k for k in loud_only) and loud_only["out.loudness|loud_apply_kernel<int16>"] == 1
    rest = {k: n for k, n in before.items() if k != "out.pcm16|pcm16_kernel"}  # (the limiter's last kernel converts)
    once = {f"out.limit|limit_{k}_kernel": 1 for k in ("env", "gain", "scan", "carry", "final")}
    assert alone == dict(rest, **once, **{"out.limit|limit_apply_kernel<int16>": 1})
    twice = {k: (1 if "env" in k or "final" in k else 2) for k in once}  # the envelope once, a scan / carry / apply per pass
    measure = {f"out.loudness|loud_{k}_kernel": 2 for k in ("tile", "carry", "square", "final")}
    assert two == dict(rest, **twice, **measure, **{"out.limit|limit_apply_kernel<float>": 1, "out.limit|limit_apply_kernel<int16>": 1})
    assert not any("loud_apply" in k for k in two)


def test_streams_and_bad_values_are_refused_and_the_process_goes_on(lib, hip_tiny):
    import ctypes

    from vosk_tts_amd.capi import FLAG_LIMIT, FLAG_LOUDNESS, SynthLimitOpts, VitsError, _p, c_f32p, c_i64p

    ids = np.random.default_rng(44).integers(1, 20, size=(1, 12)).astype(np.int64)
    with pytest.raises(VitsError, match="whole utterance") as e:
        hip_tiny.stream(ids, SCALES, 1, limit=_lspec("true"))
    assert e.value.code == 4

    def opts(flags=FLAG_LIMIT, **kw):
        o = SynthLimitOpts()
        o.flags = flags
        o.loudness_mode, o.loudness_target, o.loudness_ceiling = 1, -19.0, 0.0
        o.limit_mode, o.limit_ceiling, o.limit_lookahead_ms, o.limit_release_ms, o.limit_gain = 2, 0.9, 5.0, 50.0, 1.0
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    sc = np.array(SCALES, np.float32)
    st, total = ctypes.c_void_p(), ctypes.c_int64()
    o = opts()
    for name, extra in (("stream_open", ()), ("stream_open_rate", (8000,))):
        rc = lib._fn(name)(hip_tiny._h, _p(ids, c_i64p), 12, _p(sc, c_f32p), 1, ctypes.byref(o), 8, *extra, ctypes.byref(st), ctypes.byref(total))
        assert rc == 4 and not st.value  # VITS_ERR_UNSUPPORTED
        with pytest.raises(VitsError, match="whole utterance"):
            lib.check(rc)
    both = FLAG_LIMIT | FLAG_LOUDNESS
    for o, words in ((opts(limit_mode=3), ("mode 3",)), (opts(limit_ceiling=0.0), ("ceiling 0",)), (opts(limit_ceiling=1.5), ("ceiling 1.5",)),
                     (opts(limit_lookahead_ms=11.0), ("lookahead 11",)), (opts(limit_release_ms=0.5), ("release 0.5",)),
                     (opts(limit_gain=65.0), ("gain 65",)), (opts(both, loudness_ceiling=1.0), ("loudness_ceiling", "limit_ceiling")),
                     (opts(both, loudness_mode=2, loudness_target=0.5), ("VITS_LOUDNESS_PEAK",))):
        out, ns, ol = c_f32p(), ctypes.c_int64(), np.zeros(1, np.int64)
        rc = lib._fn("synthesize")(hip_tiny._h, _p(ids, c_i64p), _p(np.array([12], np.int64), c_i64p), 1, 12, _p(sc, c_f32p),
                                   _p(np.array([1], np.int64), c_i64p), ctypes.byref(o), ctypes.byref(out), ctypes.byref(ns), _p(ol, c_i64p))
        assert rc == 1  # VITS_ERR_ARG
        for word in words:
            with pytest.raises(VitsError, match=word):
                lib.check(rc)
    audio, ol = hip_tiny.synthesize(ids, [12], SCALES, [1], seed=2)  # a normal request afterwards
    assert ol[0] > 0 and np.isfinite(audio).all()
    # the limit_gain field is not read under the loudness flag
    a1 = hip_tiny.synthesize(ids, [12], SCALES, [1], seed=2, loudness=_loud(-19.0), limit=_lspec("true", 0.5, gain=1.0))[0]
    a2 = hip_tiny.synthesize(ids, [12], SCALES, [1], seed=2, loudness=_loud(-19.0), limit=_lspec("true", 0.5, gain=7.0))[0]
    assert np.array_equal(a1, a2)


# ---- multistream entry points ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def voice(tmp_path_factory):
    from vosk_tts_amd import Model
    from vosk_tts_amd.toymodel import write_toy_multistream_model

    d = str(tmp_path_factory.mktemp("ms"))
    write_toy_multistream_model(d)
    model = Model(model_path=d, device=0)
    yield model
    model.onnx.close()


def _ms_ids(T, seed, n_vocab=40):
    return np.random.default_rng(seed).integers(1, n_vocab, size=(5, T)).astype(np.int64)


@pytest.mark.parametrize("denoise", (None, 0.01), ids=("plain", "denoised"))
def test_stts_flag_is_the_op_on_the_unflagged_audio(lib, voice, denoise):
    sess = voice.onnx
    native = sess._vocoder.hp.sampling_rate
    T = 14
    ids, pde = _ms_ids(T, 3), np.full(T, 3.0, np.float32)
    kw = dict(seed=9, n_timesteps=2, want_mel=False, denoiser_strength=denoise)
    plain, _ = sess._model.synthesize(ids, SC, 2, None, pde, **kw)
    n = np.array([plain.shape[0]], np.int64)
    alone, target, two = _settings(lib, plain[None], n, native)
    out = {}
    got, _ = sess._model.synthesize(ids, SC, 2, None, pde, limit=alone, loudness_out=out, **kw)
    want, wr = lib.op_limit(plain[None], n, native, *alone)
    assert np.array_equal(got, want[0]) and out["reduction"].tobytes() == wr.tobytes() and wr[0] < 1
    out = {}
    got, _ = sess._model.synthesize(ids, SC, 2, None, pde, limit=two, loudness=_loud(target), loudness_out=out, **kw)
    want, wl, wg, wr = lib.op_loudness_limit(plain[None], n, native, target, *two[:4])
    assert np.array_equal(got, want[0]) and wr[0] < 1
    assert out["gain"].tobytes() == wg.tobytes() and out["loudness"].tobytes() == wl.tobytes() and out["reduction"].tobytes() == wr.tobytes()
    # the marks form at another rate: after its resample
    p8, _, e8 = sess._model.synthesize(ids, SC, 2, None, pde, marks=True, sample_rate=8000, **kw)
    a8 = _settings(lib, p8[None], [p8.shape[0]], 8000)[0]
    g8, _, f8 = sess._model.synthesize(ids, SC, 2, None, pde, marks=True, sample_rate=8000, limit=a8, **kw)
    assert np.array_equal(g8, lib.op_limit(p8[None], [p8.shape[0]], 8000, *a8)[0][0]) and np.array_equal(e8, f8)
    # the batch door: ragged, a gain per item
    B = 3
    lens = np.array([T, 9, 4], np.int64)
    bids = np.stack([_ms_ids(T, 10 + b) for b in range(B)])
    bpde = np.full((B, T), 3.0, np.float32)
    bkw = dict(seed=0, n_timesteps=2, item_seeds=[5, 6, 7], denoiser_strength=denoise)
    plain, ol = sess._model.synthesize_batch(bids, lens, SC, [0, 1, 2], None, bpde, **bkw)
    _, target, two = _settings(lib, plain, ol, native)
    want, wl, wg, wr = lib.op_loudness_limit(plain, ol, native, target, *two[:4])
    out = {}
    got, gl = sess._model.synthesize_batch(bids, lens, SC, [0, 1, 2], None, bpde, loudness=_loud(target), limit=two, loudness_out=out, **bkw)
    assert np.array_equal(gl, ol) and np.array_equal(got, want) and out["gain"].tobytes() == wg.tobytes()
    assert out["reduction"].tobytes() == wr.tobytes() and len(set(wg.tolist())) == B
    # the session at another rate limits the resampled audio; streams refuse
    feed = {"input": ids[None], "input_lengths": np.array([T], np.int64), "scales": SC, "sid": np.array([2], np.int64),
            "phone_duration_extra": pde[None], "vits.seed": 9, "vits.n_timesteps": 2, "vits.sample_rate": 8000}
    if denoise is None:
        s8 = sess.run(None, feed)[0][0]
        c8 = min(1.0, 0.7 * float(np.abs(s8).max()))
        got = sess.run(None, dict(feed, **{"vits.limit": "sample", "vits.peak_ceiling": c8}))[0][0]
        assert np.array_equal(got, lib.op_limit(s8[None], [s8.shape[0]], 8000, 1, c8)[0][0])
        with pytest.raises(ValueError, match="whole utterance"):
            sess.run_stream(None, dict(feed, **{"vits.limit": "true"}))


def test_stts_stream_open_refuses_the_flag(lib, voice):
    import ctypes

    from vosk_tts_amd.capi import VitsError, _p, c_f32p, c_i64p
    from vosk_tts_amd.capi_stts import STTS_FLAG_LIMIT, SttsLimitOpts

    m = voice.onnx._model
    ids = _ms_ids(8, 1)
    with pytest.raises(VitsError, match="whole utterance") as e:
        m.stream(ids, SC, 0, limit=_lspec("true"))
    assert e.value.code == 4
    o = SttsLimitOpts()
    o.flags = STTS_FLAG_LIMIT
    o.limit_mode, o.limit_ceiling, o.limit_lookahead_ms, o.limit_release_ms, o.limit_gain = 1, 0.9, 5.0, 50.0, 1.0
    st, total = ctypes.c_void_p(), ctypes.c_int64()
    rc = m._fn("stream_open")(m._h, _p(ids, c_i64p), 8, _p(SC, c_f32p), 0, None, None, ctypes.byref(o), 8, ctypes.byref(st), ctypes.byref(total))
    assert rc == 4 and not st.value
    with pytest.raises(VitsError, match="whole utterance"):
        m.check(rc)


# ---- through Synth ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from vosk_tts_amd import Model, Synth
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.toymodel import PHONEMES, write_toy_model

    d = write_toy_model(str(tmp_path_factory.mktemp("vits") / "m"), W.default_hparams(n_vocab=len(PHONEMES)))
    model = Model(model_path=d, device=0)
    yield d, Synth(model)
    model.onnx.close()


TEXT = "прив+ет прив+ет прив+ет м+ир, м+ир."


def test_synth_audio_meets_the_target_the_cap_misses(toy):
    _, synth = toy
    plain = synth.synth_audio(TEXT, speaker_id=2, scale=1.0)
    l0, p0, t0 = synth.measure_loudness(plain, true_peak=True)
    assert t0 >= p0 > 0
    # 8 LU above the un-normalised voice, so that the peak_ceiling = 1.0 cap is reached (asserted below); the toy voice is loud enough
    # (about -5 LUFS) for that to pass 0 LUFS, the highest target the library takes, which still needs more gain than the cap allows
    target = min(l0 + 8.0, 0.0)
    assert target >= l0 + 3.0
    capped = synth.synth_audio(TEXT, speaker_id=2, scale=1.0, loudness=target)  # the default peak_ceiling = 1.0 cap
    lc, pc = synth.measure_loudness(capped)
    assert pc >= 0.999 and lc < target - 0.05, "the cap is not reached: the case shows nothing"
    pcm = synth.synth_audio(TEXT, speaker_id=2, scale=1.0, loudness=target, limit="true", peak_ceiling=0.89)
    ll, pl, tl = synth.measure_loudness(pcm, true_peak=True)
    print(f"un-normalised {l0:.2f} LUFS, peak {p0:.3f}, true peak {t0:.3f}; target {target:.2f}: capped {lc:.2f} LUFS peak {pc:.3f}; "
          f"limited {ll:.2f} LUFS peak {pl:.3f} true peak {tl:.3f}")
    assert pcm.dtype == np.int16 and pcm.ndim == 1 and pcm.size > 0  # (every call draws its own durations: lengths differ)
    assert abs(ll - target) < abs(lc - target)
    assert int(np.abs(pcm.astype(np.int32)).max()) <= 0.89 * 32767
    with pytest.raises(ValueError, match="whole utterance"):
        next(synth.synth_stream(TEXT, limit="true"))
    with pytest.raises(ValueError, match="peak"):
        synth.synth_audio(TEXT, peak=0.5, limit="sample")
    assert sum(c.size for c in synth.synth_stream(TEXT, speaker_id=2)) > 0  # a normal stream afterwards


def test_synth_batch_items_equal_their_single_calls(toy):
    """Every request of a batch is measured, normalised and limited on its own.  int16, at most one LSB apart, as for the un-limited
    batch (tests/test_loudness_gpu.py)."""
    from vosk_tts_amd.batching import MultiDeviceSynth

    d, synth = toy
    texts = ["прив+ет, м+ир!", "м+ир", TEXT, "м+ир прив+ет?"]
    sids, seeds = [2, 0, 5, 2], [101, 7, 33, 58]
    l0, _ = synth.measure_loudness(synth.synth_audio(TEXT, speaker_id=2, scale=1.0))
    target = min(0.0, l0 + 8.0)
    mds = MultiDeviceSynth(d, devices=[0], max_batch=4)
    try:
        got = mds.synth_batch(texts, speaker_ids=sids, seeds=seeds, scale=1.0, loudness=target, limit="true", peak_ceiling=0.8)
        for i, t in enumerate(texts):
            ids = np.array([synth.g2p_noembed(t)], np.int64)
            feed = {"input": ids, "input_lengths": np.array([ids.shape[1]], np.int64), "scales": np.array([0.8, 1.0, 0.8], np.float32),
                    "sid": np.array([sids[i]], np.int64), "bert": None, "phone_duration_extra": None, "vits.seed": seeds[i],
                    "vits.loudness": target, "vits.limit": "true", "vits.peak_ceiling": 0.8}
            solo = synth.model.onnx.run_pcm16(feed, 1.0)[0]
            assert got[i].shape == solo.shape
            assert np.abs(got[i].astype(np.int32) - solo.astype(np.int32)).max() <= 1, i
            assert int(np.abs(got[i].astype(np.int32)).max()) <= 0.8 * 32767
        with pytest.raises(ValueError, match="peak"):
            mds.synth_batch(texts, peak=0.5, limit="true")
    finally:
        mds.close()
