"""Output sample rate on the device (include/vits_resample.h): resample_kernel through vits_op_resample against the float64
restatement (tests/resample_ref.py), then the one-shot, batched and streamed entry points against the op."""
import numpy as np
import pytest

import resample_ref as R
from conftest import assert_close

pytestmark = pytest.mark.gpu

SCALES = [0.667, 1.0, 0.8]
NATIVE = 22050
PAD = 1e30  # what lies beyond an item's end in the padded batch: one read of it shows in every comparison


def _item_lengths(L, M):
    """1, 37 (shorter than the filter), the input span of one workgroup's outputs -1 / +1, and 1000"""
    span = R.TILE * M // L
    return [1, 37, span - 1, span + 1, 1000]


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert hip_lib.has_resample, "libvits_mi355.so exports no vits_resample_* symbols"
    return hip_lib


@pytest.mark.parametrize("pair", R.PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_op_resample_against_float64(lib, pair):
    rate_in, rate_out = pair
    P = R.plan(*pair)
    L, M = P["L"], P["M"]
    lens = _item_lengths(L, M)
    N = max(lens) + 77
    rng = np.random.default_rng(L * 1000 + M)
    x = np.full((len(lens), N), PAD, np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = rng.uniform(-1, 1, n)
    y = lib.op_resample(x, lens, rate_in, rate_out)
    assert y.shape == (len(lens), R.n_out(N, L, M)) and np.isfinite(y).all()
    tab = lib.resample_table(*pair)
    for b, n in enumerate(lens):
        want = R.resample(x[b, :n], *pair)
        n_out = R.n_out(n, L, M)
        assert want.shape == (n_out,)
        bound = R.fp32_bound(tab, np.abs(x[b, :n]).max())  # taps * 2^-24 * max_p sum_i |table[p][i]| * max|x|
        err = np.abs(y[b, :n_out] - want).max()
        print(f"{rate_in} -> {rate_out} len {n}: err {err:.3e}, bound {bound:.3e}, max|y| {np.abs(want).max():.3f}")
        assert err <= bound, (b, n, err, bound)
        assert not y[b, n_out:].any(), f"item {b}: nonzero output at or beyond N_out"


def test_op_resample_identity_and_errors(lib):
    from vosk_tts_amd.capi import VitsError

    x = np.random.default_rng(1).uniform(-1, 1, (2, 300)).astype(np.float32)
    y = lib.op_resample(x, [300, 120], NATIVE, NATIVE)
    assert np.array_equal(y[0], x[0]) and np.array_equal(y[1, :120], x[1, :120]) and not y[1, 120:].any()
    with pytest.raises(VitsError) as e:
        lib.op_resample(x, [300, 301], NATIVE, 8000)
    assert e.value.code == 1
    with pytest.raises(VitsError) as e:
        lib.op_resample(x, [300, 120], NATIVE, 8003)
    assert e.value.code == 4 and "8003" in str(e.value)


def test_op_resample_where_n_times_M_passes_2_to_31(lib):
    """n * M is 64-bit in the kernel: at 22050 -> 8000 (M = 441) it passes 2^31 at output 4 869 567, ten minutes into the audio"""
    pair = (NATIVE, 8000)
    P = R.plan(*pair)
    L, M = P["L"], P["M"]
    n_cross = (1 << 31) // M
    N = (n_cross + 3000) * M // L
    x = np.random.default_rng(2).uniform(-1, 1, N).astype(np.float32)
    y = lib.op_resample(x[None], [N], *pair)[0]
    n_out = R.n_out(N, L, M)
    assert y.shape == (n_out,) and n_out > n_cross + 2000
    bound = R.fp32_bound(lib.resample_table(*pair), 1.0)
    for a, b in ((n_cross - 300, n_cross + 300), (n_out - 300, n_out)):
        want = R.resample(x, *pair, n_from=a, n_to=b)
        assert np.abs(y[a:b] - want).max() <= bound


def _ragged(rng, B=3, Tx=24, n_vocab=20):
    lens = np.array([Tx, Tx - 9, 5][:B], np.int64)
    ids = rng.integers(1, n_vocab, size=(B, Tx)).astype(np.int64)
    sid = rng.integers(0, 4, size=B).astype(np.int64)
    return ids, lens, sid


@pytest.fixture(scope="module")
def native_runs(hip_tiny):
    """the native-rate outputs every end-to-end test resamples: computed once, left unchanged"""
    ids, lens, sid = _ragged(np.random.default_rng(31))
    out = {"ids": ids, "lens": lens, "sid": sid}
    for solo in (False, True):
        out[solo] = hip_tiny.synthesize(ids, lens, SCALES, sid, seed=7, solo=solo)
    return out


@pytest.mark.parametrize("solo", (False, True), ids=("padded", "solo"))
@pytest.mark.parametrize("rate", (8000, 48000))
def test_synthesize_rate_is_the_op_on_each_items_own_signal(lib, hip_tiny, native_runs, rate, solo):
    ids, lens, sid = native_runs["ids"], native_runs["lens"], native_runs["sid"]
    audio, ol = native_runs[solo]
    P = R.plan(NATIVE, rate)
    L, M = P["L"], P["M"]
    got, gl = hip_tiny.synthesize(ids, lens, SCALES, sid, seed=7, solo=solo, sample_rate=rate)
    assert gl.tolist() == [R.n_out(n, L, M) for n in ol]
    assert got.shape == (3, int(gl.max()))
    tab = lib.resample_table(NATIVE, rate)
    scale = float(1.25 / np.abs(audio).max())  # the loudest samples clip
    pcm, pl = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=scale, seed=7, solo=solo, sample_rate=rate)
    assert pl.tolist() == gl.tolist() and pcm.shape == got.shape and pcm.dtype == np.int16
    for b in range(3):
        n, n_out = int(ol[b]), int(gl[b])
        via_op = lib.op_resample(audio[b:b + 1, :n], [n], NATIVE, rate)[0]
        want = R.resample(audio[b, :n], NATIVE, rate)
        bound = R.fp32_bound(tab, np.abs(audio[b, :n]).max())
        print(f"{rate} Hz item {b}: vs op {np.abs(got[b, :n_out] - via_op).max():.3e}, vs float64 {np.abs(got[b, :n_out] - want).max():.3e}, bound {bound:.3e}")
        assert np.abs(got[b, :n_out] - via_op).max() <= bound
        assert np.abs(got[b, :n_out] - want).max() <= bound
        assert not got[b, n_out:].any() and not pcm[b, n_out:].any()
        want16 = R.pcm16(want, scale)
        d = np.abs(pcm[b, :n_out].astype(np.int32) - want16.astype(np.int32))
        print(f"{rate} Hz item {b}: int16 differs in {np.count_nonzero(d)} of {n_out}, clipped {np.count_nonzero(np.abs(want16) == 32767)}")
        assert d.max() <= 1
        assert np.count_nonzero(d) <= 0.01 * n_out


def _launches(lib, run):
    lib.launch_log(1)
    try:
        run()
    finally:
        lib.launch_log(0)
    return sum(lib.launch_dump().values())


def test_another_rate_costs_no_launch_at_int16_and_one_at_float(lib, hip_tiny):
    ids = np.random.default_rng(33).integers(1, 20, size=(1, 16)).astype(np.int64)
    lib.lib.vits_debug_fast_path(0)  # the eager path: one counted launch per kernel
    try:
        n = {(kind, rate): _launches(lib, lambda: getattr(hip_tiny, kind)(ids, [16], SCALES, [1], seed=3, sample_rate=rate))
             for kind in ("synthesize", "synthesize_pcm16") for rate in (None, 8000)}
    finally:
        lib.lib.vits_debug_fast_path(1)
    assert n["synthesize_pcm16", 8000] == n["synthesize_pcm16", None] == n["synthesize", None] + 1
    assert n["synthesize", 8000] == n["synthesize", None] + 1
    lib.launch_log(1)
    try:
        lib.lib.vits_debug_fast_path(0)
        hip_tiny.synthesize_pcm16(ids, [16], SCALES, [1], seed=3, sample_rate=8000)
    finally:
        lib.lib.vits_debug_fast_path(1)
        lib.launch_log(0)
    assert lib.launch_count("out.resample", "resample_kernel<int16>") == 1 and lib.launch_count("out.pcm16", "") == 0


@pytest.mark.parametrize("rate", (8000, 48000))
def test_streamed_chunks_follow_the_formula_and_equal_the_one_shot(hip_tiny, rate):
    chunk, hop = 8, hip_tiny.hp.hop_length
    P = R.plan(NATIVE, rate)
    L, M = P["L"], P["M"]
    ids = np.random.default_rng(11).integers(1, 20, size=(1, 40)).astype(np.int64)
    _, nl = hip_tiny.synthesize(ids, [40], SCALES, [2], seed=5)
    Ty = int(nl[0]) // hop
    one, ol = hip_tiny.synthesize(ids, [40], SCALES, [2], seed=5, sample_rate=rate)
    chunks = list(hip_tiny.stream(ids, SCALES, 2, chunk_frames=chunk, seed=5, sample_rate=rate))
    edges = [min(i, Ty) * hop for i in range(0, Ty + chunk, chunk)]
    assert [len(c) for c in chunks] == [R.n_out(b, L, M) - R.n_out(a, L, M) for a, b in zip(edges, edges[1:])]
    got = np.concatenate(chunks)[None]
    assert got.shape == one.shape == (1, int(ol[0])) and int(ol[0]) == R.n_out(Ty * hop, L, M)
    assert_close("stream vs one-shot", one, got, 2e-5)


@pytest.mark.parametrize("rate", (8000, 48000))
def test_streamed_latent_equals_the_resampled_decode(lib, hip_tiny, rate):
    chunk, hop, Ty = 8, hip_tiny.hp.hop_length, 53
    P = R.plan(NATIVE, rate)
    L, M = P["L"], P["M"]
    z = np.random.default_rng(12).standard_normal((hip_tiny.hp.inter_channels, Ty)).astype(np.float32)
    audio, _ = hip_tiny.decoder(z[None], want_mb=False, sid=[0])
    one = lib.op_resample(audio, [Ty * hop], NATIVE, rate)
    chunks = list(hip_tiny.stream_latent(z, chunk_frames=chunk, sample_rate=rate))
    edges = [min(i, Ty) * hop for i in range(0, Ty + chunk, chunk)]
    assert [len(c) for c in chunks] == [R.n_out(b, L, M) - R.n_out(a, L, M) for a, b in zip(edges, edges[1:])]
    got = np.concatenate(chunks)[None]
    assert got.shape == one.shape == (1, R.n_out(Ty * hop, L, M))
    assert_close("latent stream vs resampled decode", one, got, 2e-5)


def test_stream_capacity_is_checked_in_output_samples(lib, hip_tiny):
    import ctypes

    from vosk_tts_amd.capi import c_f32p, c_i64p

    z = np.zeros((hip_tiny.hp.inter_channels, 20), np.float32)
    st, total = ctypes.c_void_p(), ctypes.c_int64()
    lib.check(lib._fn("stream_open_latent_rate")(hip_tiny._h, z.ctypes.data_as(c_f32p), 20, 8, 0, 8000, ctypes.byref(st), ctypes.byref(total)))
    try:
        n_first = R.n_out(8 * hip_tiny.hp.hop_length, 160, 441)
        assert total.value == R.n_out(20 * hip_tiny.hp.hop_length, 160, 441)
        buf, n = np.zeros(n_first, np.float32), ctypes.c_int64()
        assert lib._fn("stream_next")(st, buf.ctypes.data_as(c_f32p), n_first - 1, ctypes.byref(n)) == 1  # VITS_ERR_ARG, nothing consumed
        lib.check(lib._fn("stream_next")(st, buf.ctypes.data_as(c_f32p), n_first, ctypes.byref(n)))
        assert n.value == n_first
    finally:
        lib._fn("stream_close")(st)


def test_the_rate_is_part_of_the_graph_key(hip_tiny):
    """native, 8000 Hz, native again on one model (same shape buckets, same seed): the native output is the same bits both times, and
    so is the 8000 Hz one on a second visit"""
    ids = np.random.default_rng(35).integers(1, 20, size=(1, 21)).astype(np.int64)

    def run(kind, rate):
        return getattr(hip_tiny, kind)(ids, [21], SCALES, [3], seed=9, sample_rate=rate)

    for kind in ("synthesize", "synthesize_pcm16"):
        a0, l0 = run(kind, None)
        b0, m0 = run(kind, 8000)
        a1, l1 = run(kind, None)
        b1, m1 = run(kind, 8000)
        assert np.array_equal(a0, a1) and np.array_equal(l0, l1)
        assert np.array_equal(b0, b1) and np.array_equal(m0, m1)
        assert m0[0] == R.n_out(int(l0[0]), 160, 441) and b0.shape[1] == m0[0] and a0.shape[1] == l0[0]


def test_session_feed_key(lib, hip_tiny, tiny_blob):
    """VitsSession: "vits.sample_rate" next to "vits.seed"; run, run_pcm16 and run_stream agree with the model-level calls"""
    from vosk_tts_amd.session import VitsSession

    sess = VitsSession(tiny_blob, 0, lib=lib)
    try:
        ids = np.random.default_rng(36).integers(1, 20, size=(1, 18)).astype(np.int64)
        feed = {"input": ids, "input_lengths": np.array([18]), "scales": np.array(SCALES, np.float32), "sid": np.array([1]),
                "vits.seed": 4, "vits.sample_rate": 16000}
        want, wl = hip_tiny.synthesize(ids, [18], SCALES, [1], seed=4, sample_rate=16000)
        got = sess.run(None, feed)[0]
        assert got.shape == (1, 1, 1, int(wl[0])) and np.array_equal(got.reshape(1, -1), want)
        pcm = sess.run_pcm16({k: v for k, v in feed.items() if k != "vits.sample_rate"}, 1.0, sample_rate=16000)
        assert np.array_equal(pcm, hip_tiny.synthesize_pcm16(ids, [18], SCALES, [1], seed=4, sample_rate=16000)[0])
        chunks = list(sess.run_stream(None, feed, chunk_frames=8))
        assert sum(len(c) for c in chunks) == int(wl[0])
        assert_close("session stream", want, np.concatenate(chunks)[None], 2e-5)
    finally:
        sess.close()


def test_multistream_session_resamples_on_the_host_buffer_and_streams_the_vocoder_at_the_rate(lib, tmp_path):
    """SttsSession: run() = vits_op_resample of its own native-rate waveform, run_stream() = vits_stream_open_latent_rate"""
    from vosk_tts_amd import Model
    from vosk_tts_amd.multistream import g2p_multistream
    from vosk_tts_amd.toymodel import write_toy_multistream_model

    write_toy_multistream_model(str(tmp_path))
    model = Model(model_path=str(tmp_path), device=0)
    try:
        sess = model.onnx
        native = sess._vocoder.hp.sampling_rate
        ids, _ = g2p_multistream("м+ир.", model.dic, model.config["phoneme_id_map"], None, word_pos=True)
        ids = np.transpose(np.array(ids, np.int64))
        feed = {"input": ids[None], "input_lengths": np.array([ids.shape[1]], np.int64), "scales": np.array([0.7, 1.0, 0.8], np.float32),
                "sid": np.array([1], np.int64), "bert": None, "phone_duration_extra": None, "vits.seed": 3}
        wav, n = sess.run(None, feed)
        P = lib.resample_plan(native, 8000)
        got, gn = sess.run(None, dict(feed, **{"vits.sample_rate": 8000}))
        assert gn.tolist() == [R.n_out(int(n[0]), P["L"], P["M"])] and got.shape == (1, int(gn[0]))
        assert np.array_equal(got, lib.op_resample(wav, n, native, 8000))
        chunks = list(sess.run_stream(None, feed, chunk_frames=8, sample_rate=8000))
        assert sum(len(c) for c in chunks) == int(gn[0])
        assert_close("multistream stream", got, np.concatenate(chunks)[None], 2e-5)
    finally:
        model.onnx.close()
