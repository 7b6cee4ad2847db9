"""Output sample rate (include/vits_resample.h), the parts that need no GPU: the host-only plan / table entry points against the
float64 restatement (tests/resample_ref.py), the filter's own figures, and the Python surface (coalescer key, WAV header, CLI flag)."""
import threading
import time
import wave

import numpy as np
import pytest

import resample_ref as R

# rate_in, rate_out -> (L, M, taps, half_width_in): taps = the most input samples one output reads = 2 floor(Hw) + 1 here,
# half_width_in = ceil(Hw), Hw = 16 / min(1, L / M)
EXPECTED = {
    (22050, 8000): (160, 441, 89, 45),
    (22050, 11025): (1, 2, 65, 32),
    (22050, 12000): (80, 147, 59, 30),
    (22050, 16000): (320, 441, 45, 23),
    (22050, 24000): (160, 147, 33, 16),
    (22050, 32000): (640, 441, 33, 16),
    (22050, 44100): (2, 1, 33, 16),
    (22050, 48000): (320, 147, 33, 16),
    (16000, 8000): (1, 2, 65, 32),
}


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert hip_lib.has_resample, "libvits_mi355.so exports no vits_resample_* symbols"
    return hip_lib


def test_the_pairs_are_the_ones_every_test_walks():
    assert sorted(EXPECTED) == sorted(R.PAIRS)


@pytest.mark.parametrize("pair", R.PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_plan_and_table_equal_the_float64_definition(lib, pair):
    L, M, taps, half = EXPECTED[pair]
    P = lib.resample_plan(*pair)
    assert (P["L"], P["M"], P["taps"], P["half"]) == (L, M, taps, half)
    Q = R.plan(*pair)
    assert (Q["L"], Q["M"], Q["taps"], Q["half"]) == (L, M, taps, half)
    assert L * taps <= R.MAX_TABLE
    got = lib.resample_table(*pair)
    want = R.table(*pair).astype(np.float32)  # rounded once
    assert got.shape == want.shape == (L, taps) and got.dtype == np.float32
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} of {got.size} coefficients differ"


def test_table_capacity_is_checked(lib):
    import ctypes

    from vosk_tts_amd.capi import VitsError, c_f32p

    buf = np.zeros(160 * 89 - 1, np.float32)
    rc = lib._fn("resample_table")(22050, 8000, buf.ctypes.data_as(c_f32p), ctypes.c_int64(buf.size))
    assert rc == 1  # VITS_ERR_ARG
    with pytest.raises(VitsError):
        lib.check(rc)


@pytest.mark.parametrize("pair,words", [
    ((22050, 8003), ("22050", "8003", "8003 phases")),     # gcd 1: 8003 phases x 89 taps, far beyond 65536 floats
    ((22050, 5000), ("22050", "5000")),                    # below rate_in / 4
    ((22050, 88201), ("22050", "88201")),                  # above 4 * rate_in
    ((22050, 0), ("22050", "rate_out 0")),
    ((22050, -8000), ("22050", "-8000")),
    ((0, 8000), ("rate_in 0", "8000")),
])
def test_refusals_name_the_values(lib, pair, words):
    from vosk_tts_amd.capi import VitsError

    with pytest.raises(VitsError) as e:
        lib.resample_plan(*pair)
    assert e.value.code == 4  # VITS_ERR_UNSUPPORTED
    for w in words:
        assert w in str(e.value), str(e.value)


def test_22050_to_8001_is_inside_the_table_limit(lib):
    """gcd(22050, 8001) = 63, so 8001 Hz is 127 phases x 89 taps = 11303 floats: inside the 65536-float rule, hence accepted (and
    exact like every other pair); the pair the table rule refuses is one with a small gcd, 8003 above."""
    P = lib.resample_plan(22050, 8001)
    assert (P["L"], P["M"], P["taps"], P["half"]) == (127, 350, 89, 45)
    assert np.array_equal(lib.resample_table(22050, 8001), R.table(22050, 8001).astype(np.float32))


@pytest.mark.parametrize("pair", R.PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_filter_figures_of_the_float64_prototype(pair):
    """unit DC gain (every phase within 1e-4), at most -90 dB beyond (2 - rho) of the lower Nyquist (measured: -98 to -99 dB)"""
    rate_in, rate_out = pair
    P = R.plan(*pair)
    L, M, W = P["L"], P["M"], P["W"]
    tab = R.table(*pair)
    dc = tab.sum(axis=1)
    assert np.abs(dc - 1.0).max() <= 1e-4, dc
    g = R.h_num(np.arange(-W, W + 1), L, M)  # the prototype at the interpolated rate L * rate_in
    n_fft = 1 << 20
    H = np.abs(np.fft.rfft(g, n_fft)) / L
    f = np.arange(H.shape[0]) * (float(rate_in) * L / n_fft)  # Hz
    stop = (2.0 - R.RHO) * min(rate_in, rate_out) / 2.0
    worst = 20 * np.log10(H[f >= stop].max())
    print(f"{rate_in} -> {rate_out}: DC {dc.min():.7f}..{dc.max():.7f}, stop band {worst:.1f} dB")
    assert abs(H[0] - 1.0) <= 1e-4
    assert worst <= -90.0


@pytest.mark.parametrize("pair", R.PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_restatement_agrees_with_scipy(pair):
    sig = pytest.importorskip("scipy.signal")
    P = R.plan(*pair)
    L, M, W = P["L"], P["M"], P["W"]
    g = R.h_num(np.arange(-W, W + 1), L, M)
    x = np.random.default_rng(3).uniform(-1, 1, 1000)
    want = sig.resample_poly(x, L, M, window=g / L)  # (resample_poly multiplies the window by L)
    got = R.resample(x, *pair)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12


def test_restatement_from_the_table_is_the_restatement_from_h():
    """y[n] = sum_i table[p][i] x[q - lo(p) + i] is the same sum as the definition's, for an item shorter than the filter too"""
    rng = np.random.default_rng(4)
    for pair in ((22050, 8000), (22050, 48000), (22050, 11025)):
        P = R.plan(*pair)
        L, M, W = P["L"], P["M"], P["W"]
        tab = R.table(*pair)
        for n_in in (1, 37, 700):
            x = rng.uniform(-1, 1, n_in)
            want = R.resample(x, *pair)
            got = np.zeros_like(want)
            for n in range(want.shape[0]):
                q, p = divmod(n * M, L)
                lo = (W - p) // L
                for i in range(P["taps"]):
                    k = q - lo + i
                    if 0 <= k < n_in:
                        got[n] += tab[p, i] * x[k]
            assert np.abs(got - want).max() <= 1e-14


# ---- Python surface ----------------------------------------------------------------------------------------------------------
class _Hp:
    sampling_rate, hop_length, bert_dim, n_speakers = 22050, 256, 0, 4


class _EngineStub:
    """stands where capi.VitsModel stands: records (items, sample_rate) per engine call; the first call waits for `gate`"""

    def __init__(self):
        self.hp = _Hp()
        self.calls = []
        self.gate = threading.Event()
        self.entered = threading.Event()
        self._lock = threading.Lock()

    def synthesize_pcm16(self, ids, lens, scales, sid, pcm_scale=1.0, seed=0, solo=False, item_seeds=None, sample_rate=None, **kw):
        with self._lock:
            first = not self.calls
            self.calls.append((ids.shape[0], sample_rate))
        if first:
            self.entered.set()
            assert self.gate.wait(30)
        B = ids.shape[0]
        # every sample says which rate its call ran at
        return np.full((B, 8), (sample_rate or 0) // 100, np.int16), np.full(B, 8, np.int64)

    def close(self):
        pass


class _LibStub:
    is_device = True

    def __init__(self):
        self.model = _EngineStub()

    def create(self, blob, device):
        return self.model


def test_coalescer_never_mixes_rates():
    from vosk_tts_amd.session import VitsSession

    lib = _LibStub()
    sess = VitsSession(b"", lib=lib, max_inflight=1)
    eng = lib.model
    rates = [None, 8000, 16000, 8000, None, 8000, 16000, 22050]  # (22050 is the voice's own: the same key as None)
    results = [None] * len(rates)

    def feed():
        return {"input": np.ones((1, 5), np.int64), "input_lengths": np.array([5]), "scales": np.array([0.8, 1.0, 0.8], np.float32),
                "sid": np.array([1])}

    def worker(i):
        results[i] = sess.run_pcm16(feed(), 1.0, return_lengths=True, sample_rate=rates[i])[0]

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(len(rates))]
    threads[0].start()
    assert eng.entered.wait(30)  # the first request is inside the engine: everybody else queues behind it
    for t in threads[1:]:
        t.start()
    deadline = time.monotonic() + 30
    while len(sess.coalescer._queue) < len(rates) - 1 and time.monotonic() < deadline:
        time.sleep(0.001)
    assert len(sess.coalescer._queue) == len(rates) - 1
    eng.gate.set()
    for t in threads:
        t.join(30)
    for r, out in zip(rates, results):
        want = 0 if r in (None, 22050) else r // 100
        assert out is not None and (out == want).all(), (r, out)
    # one rate per engine call, and the queued requests of one rate did share calls
    assert sorted(set(c[1] for c in eng.calls)) == [0, 8000, 16000]
    assert sess.coalescer.calls < len(rates) and max(c[0] for c in eng.calls) > 1
    # the key itself: same scales / kind / scale, different rate
    assert sum(c[0] for c in eng.calls if c[1] == 8000) == 4  # three requests, padded to a power of two


def test_session_refuses_a_negative_rate_before_the_engine():
    from vosk_tts_amd.session import VitsSession

    lib = _LibStub()
    sess = VitsSession(b"", lib=lib)
    with pytest.raises(ValueError, match="-8000"):
        sess.run_pcm16({"input": np.ones((1, 5), np.int64), "input_lengths": np.array([5]), "scales": np.ones(3, np.float32),
                        "sid": np.array([0])}, sample_rate=-8000)
    assert lib.model.calls == []


class _StubSession:
    """the session stub of tests/test_host_api.py, which also understands "vits.sample_rate" as VitsSession.run does"""

    def __init__(self):
        self.feeds = []

    def run(self, names, feed):
        self.feeds.append((names, feed))
        T = 512 * feed.get("vits.sample_rate", 22050) // 22050
        return [np.linspace(-2.0, 2.0, T, dtype=np.float32)[None, None, None, :]]


class _StubModel:
    def __init__(self, id_map):
        self.onnx = _StubSession()
        self.dic = {}
        self.tokenizer = None
        self.config = {"phoneme_id_map": id_map, "inference": {}}


def test_synth_writes_the_rate_it_used_into_the_wav_header(tmp_path, caplog):
    import logging

    from vosk_tts_amd.synth import Synth
    from vosk_tts_amd.toymodel import phoneme_id_map

    m = _StubModel(phoneme_id_map())
    s = Synth(m)
    # default: the feed and the bytes of before, 22050 in the header
    base = s.synth_audio("м+ир")
    assert set(m.onnx.feeds[-1][1]) == {"input", "input_lengths", "scales", "sid", "bert", "phone_duration_extra"}
    want = np.clip(np.linspace(-2.0, 2.0, 512, dtype=np.float32) * 32767.0, -32767.0, 32767.0).astype("int16")
    assert base.tobytes() == want.tobytes()
    out = tmp_path / "native.wav"
    s.synth("м+ир", str(out))
    with wave.open(str(out)) as f:
        assert (f.getframerate(), f.getnframes()) == (22050, 512)
        assert f.readframes(512) == want.tobytes()
    # the voice's own rate, spelled out, is the default path too
    s.synth("м+ир", str(out), sample_rate=22050)
    assert "vits.sample_rate" not in m.onnx.feeds[-1][1]
    # another rate: asked of the session, written into the header, used by the RTF line
    out8 = tmp_path / "8k.wav"
    with caplog.at_level(logging.INFO):
        s.synth("м+ир", str(out8), sample_rate=8000)
    assert m.onnx.feeds[-1][1]["vits.sample_rate"] == 8000
    with wave.open(str(out8)) as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 8000, 512 * 8000 // 22050)
    n = 512 * 8000 // 22050
    assert any("audio=%0.2f sec" % (n / 8000) in r.getMessage() for r in caplog.records)
    # the stream asks for it the same way
    chunks = list(_stream_stub(s, m, 16000))
    assert m.onnx.stream_feeds[-1]["vits.sample_rate"] == 16000 and chunks[0].dtype == np.int16


def _stream_stub(s, m, rate):
    m.onnx.stream_feeds = []

    def run_stream(names, feed, chunk_frames=64):
        m.onnx.stream_feeds.append(feed)
        yield np.zeros(100, np.float32)

    m.onnx.run_stream = run_stream
    return s.synth_stream("м+ир", sample_rate=rate)


def test_cli_has_a_sample_rate_flag():
    from vosk_tts_amd import cli

    ap = cli.build_parser()
    assert ap.parse_args([]).sample_rate is None
    assert ap.parse_args(["--sample-rate", "8000"]).sample_rate == 8000


def test_bindings_are_declared_only_where_the_symbols_exist(oracle_lib, hip_lib):
    from vosk_tts_amd.capi import VitsError

    assert hip_lib.has_resample and not oracle_lib.has_resample
    with pytest.raises(VitsError):
        oracle_lib.resample_plan(22050, 8000)
    assert hip_lib.out_samples(1000, 22050, 8000) == -(-1000 * 160 // 441)
    assert hip_lib.out_samples(1000, 22050, None) == hip_lib.out_samples(1000, 22050, 22050) == 1000
