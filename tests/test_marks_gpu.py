"""GPU tests of the speech marks (include/vits_marks.h) against the integer restatement (tests/marks_ref.py).

Exactness is asserted only where the frame counts are fixed by the input -- forced durations for the VITS family, an all-non-zero
phone_duration_extra for the multistream family -- so that no rounding coincidence decides a test.  Free-running calls are checked
by invariants and by feeding their own marks back as forced durations."""
import ctypes

import numpy as np
import pytest

import marks_ref as R
from conftest import assert_close

pytestmark = pytest.mark.gpu

SCALES = np.array([0.667, 1.0, 0.8], np.float32)
NATIVE, HOP = 22050, 256
RATES = (None, 8000, 48000)


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert hip_lib.has_marks, "libvits_mi355.so exports no speech-mark symbols"
    return hip_lib


def _persist_runs(lib, model):
    fn = lib.lib.vits_debug_persist_runs
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p]
    return int(fn(model._h))


def _ragged_case():
    """B = 3, T_x = 13 (no multiple of the bucket of 8), lengths [13, 5, 1]; durations in [0, 6] with zeros inside; item 1 all zero
    (the clamp exception: one frame of audio, every token end 0)"""
    rng = np.random.default_rng(41)
    lens = np.array([13, 5, 1], np.int64)
    dur = rng.integers(0, 7, size=(3, 13)).astype(np.int32)
    dur[0, [2, 3, 9]] = 0
    dur[1] = 0
    dur[2, 0] = 3
    ids = rng.integers(1, 20, size=(3, 13)).astype(np.int64)
    sid = np.array([0, 3, 1], np.int64)
    return ids, lens, sid, dur


@pytest.mark.parametrize("rate", RATES, ids=lambda r: f"{r or NATIVE}Hz")
def test_forced_durations_ragged_batch(lib, hip_tiny, rate):
    ids, lens, sid, dur = _ragged_case()
    want = R.token_ends(dur, lens, HOP, NATIVE, rate)
    want_len = R.out_lengths(dur, lens, HOP, NATIVE, rate)
    assert not want[1].any() and want_len[1] == R.n_out(HOP, *R.ratio(NATIVE, rate))  # the clamp exception is in the case
    for solo in (False, True):
        kw = dict(forced_durations=dur, seed=7, solo=solo, sample_rate=rate)
        plain, pl = hip_tiny.synthesize(ids, lens, SCALES, sid, **kw)
        audio, ol, ends = hip_tiny.synthesize(ids, lens, SCALES, sid, marks=True, **kw)
        assert ends.dtype == np.int64 and np.array_equal(ends, want), (rate, solo, ends, want)
        assert ol.tolist() == want_len and np.array_equal(ol, pl) and np.array_equal(audio, plain)
        pcm0, pl0 = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=0.9, **kw)
        pcm, ol16, ends16 = hip_tiny.synthesize_pcm16(ids, lens, SCALES, sid, pcm_scale=0.9, marks=True, **kw)
        assert np.array_equal(ends16, want) and np.array_equal(ol16, pl0) and np.array_equal(pcm, pcm0) and pcm.dtype == np.int16
        # items 0 and 2 have frames: their last valid mark is their length
        assert ends[0, 12] == ol[0] and ends[2, 0] == ol[2]


def test_null_token_ends_is_an_argument_error(lib, hip_tiny):
    fn = lib._fn("synthesize_marks")
    ids = np.ones((1, 4), np.int64)
    lens = np.array([4], np.int64)
    out, ns = ctypes.POINTER(ctypes.c_float)(), ctypes.c_int64()
    rc = fn(hip_tiny._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), lens.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1, 4,
            SCALES.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), None, None, 0, ctypes.byref(out), ctypes.byref(ns), None, None)
    assert rc == 1 and b"token_ends" in lib._fn("last_error")()


def test_more_than_256_tokens_in_one_item(lib, hip_tiny):
    """T_x = 300: durations_kernel gives a thread more than one token, token_ends_kernel runs two workgroups per item"""
    rng = np.random.default_rng(42)
    dur = rng.integers(0, 4, size=(1, 300)).astype(np.int32)
    ids = rng.integers(1, 20, size=(1, 300)).astype(np.int64)
    for rate in (None, 8000):
        _, ol, ends = hip_tiny.synthesize(ids, [300], SCALES, [1], forced_durations=dur, seed=3, sample_rate=rate, marks=True)
        assert np.array_equal(ends, R.token_ends(dur, [300], HOP, NATIVE, rate))
        assert ol.tolist() == R.out_lengths(dur, [300], HOP, NATIVE, rate)


def _one_utterance(seed=43, Tx=11, n_vocab=60):
    rng = np.random.default_rng(seed)
    ids = rng.integers(1, n_vocab, size=(1, Tx)).astype(np.int64)
    dur = rng.integers(0, 5, size=(1, Tx)).astype(np.int32)
    dur[0, 4] = 0
    return ids, dur


def test_every_front_variant_gives_the_same_marks(lib, hip_default):
    ids, dur = _one_utterance()
    want = R.token_ends(dur, [11], HOP)
    kw = dict(forced_durations=dur, seed=9, marks=True)
    legs = {}
    try:
        lib.lib.vits_debug_persist(7)
        r0 = _persist_runs(lib, hip_default)
        legs["persistent"] = hip_default.synthesize(ids, [11], SCALES, [5], **kw)
        ran = _persist_runs(lib, hip_default) > r0
        lib.lib.vits_debug_persist(0)
        legs["launch"] = hip_default.synthesize(ids, [11], SCALES, [5], **kw)
        lib.lib.vits_debug_fast_path(0)
        legs["eager"] = hip_default.synthesize(ids, [11], SCALES, [5], **kw)
    finally:
        lib.lib.vits_debug_fast_path(1)
        lib.lib.vits_debug_persist(7)
    got = []
    chunks = list(hip_default.stream(ids, SCALES, 5, chunk_frames=8, forced_durations=dur, seed=9, on_marks=got.append))
    assert len(got) == 1
    legs["stream"] = (np.concatenate(chunks)[None], np.array([sum(len(c) for c in chunks)]), got[0][None])
    for name, (audio, ol, ends) in legs.items():
        if name == "persistent" and not ran:
            continue
        assert np.array_equal(ends, want), (name, ends, want)
        assert int(ol[0]) == int(want[0, -1]) == audio.shape[1]
    if not ran:
        pytest.skip("the persistent front program did not run (token or lock taken): that leg is unchecked, the other three passed")


def test_free_running_marks_fed_back_reproduce_the_call(lib, hip_default):
    ids, _ = _one_utterance(44)
    I = hip_default.hp.inter_channels
    rng = np.random.default_rng(45)
    noise_dp = rng.standard_normal((1, 2, 11)).astype(np.float32)
    noise_prior = rng.standard_normal((1, I, 4096)).astype(np.float32)

    def invariants(ol, ends):
        assert (np.diff(ends[0]) >= 0).all() and ends[0, 0] >= 0
        assert int(ends[0, -1]) == int(ol[0])
        assert not (ends % HOP).any()  # native rate: every span is a whole number of frames
        return np.diff(ends, prepend=0).astype(np.int32) // HOP

    fast = {}
    try:
        for name, mask in (("persistent", 7), ("launch", 0)):
            lib.lib.vits_debug_persist(mask)
            r0 = _persist_runs(lib, hip_default)
            fast[name] = hip_default.synthesize(ids, [11], SCALES, [5], seed=21, marks=True) + (_persist_runs(lib, hip_default) > r0,)
    finally:
        lib.lib.vits_debug_persist(7)
    for name, (audio, ol, ends, ran) in fast.items():
        dur = invariants(ol, ends)
        a2, ol2, ends2 = hip_default.synthesize(ids, [11], SCALES, [5], forced_durations=dur, noise_prior=noise_prior, marks=True)
        assert np.array_equal(ol2, ol) and np.array_equal(ends2, ends), name
    # the eager path with injected noise: the forced call on its own durations is the same call
    a, ol, ends = hip_default.synthesize(ids, [11], SCALES, [5], noise_dp=noise_dp, noise_prior=noise_prior, marks=True)
    dur = invariants(ol, ends)
    b, ol2, ends2 = hip_default.synthesize(ids, [11], SCALES, [5], forced_durations=dur, noise_prior=noise_prior, marks=True)
    assert np.array_equal(ol2, ol) and np.array_equal(ends2, ends)
    assert_close("forced by its own marks vs free-running", a, b, 1e-4)
    if not fast["persistent"][3]:
        pytest.skip("the persistent front program did not run (token or lock taken): that leg ran on launches")


def _captured_launches(lib, blob, ids, dur, marks):
    """launches a FRESH model logs for one call: every graph of it is captured inside the log, and a capture counts each kernel once.
    On the launch path, so that the two counts compared do not depend on who holds the device's program token at the time."""
    m = lib.create(blob, 0)
    lib.lib.vits_debug_persist(0)
    lib.launch_log(1)
    try:
        m.synthesize(ids, [11], SCALES, [1], forced_durations=dur, seed=2, marks=marks)
        return sum(lib.launch_dump().values()), lib.launch_count("marks.token_ends", "token_ends_kernel")
    finally:
        lib.launch_log(0)
        lib.lib.vits_debug_persist(7)
        m.close()


def test_marks_off_replays_the_graphs_of_before(lib, tiny_blob):
    ids, dur = _one_utterance(46, n_vocab=20)
    # the marks variant of a call is the plain one plus exactly one launch
    n_plain, k_plain = _captured_launches(lib, tiny_blob, ids, dur, False)
    n_marks, k_marks = _captured_launches(lib, tiny_blob, ids, dur, True)
    assert (k_plain, k_marks) == (0, 1) and n_marks == n_plain + 1
    m = lib.create(tiny_blob, 0)
    try:
        base = m.synthesize(ids, [11], SCALES, [1], forced_durations=dur, seed=2)  # (captures the plain graphs, outside the log)
        lib.launch_log(1)
        try:
            _, _, ends = m.synthesize(ids, [11], SCALES, [1], forced_durations=dur, seed=2, marks=True)
            n1 = sum(lib.launch_dump().values())
            assert lib.launch_count("marks.token_ends", "token_ends_kernel") == 1
            again = m.synthesize(ids, [11], SCALES, [1], forced_durations=dur, seed=2)
            assert lib.launch_count("marks.token_ends", "token_ends_kernel") == 1  # the call without marks launched none ...
            assert sum(lib.launch_dump().values()) == n1                            # ... and captured nothing: it replayed what it had
            m.synthesize(ids, [11], SCALES, [1], seed=2, marks=True)  # the free-running variant: its own capture, one more launch
            assert lib.launch_count("marks.token_ends", "token_ends_kernel") == 2
            m.synthesize(ids, [11], SCALES, [1], forced_durations=dur, seed=2, marks=True)  # replayed
            assert lib.launch_count("marks.token_ends", "token_ends_kernel") == 2
        finally:
            lib.launch_log(0)
        assert np.array_equal(ends, R.token_ends(dur, [11], HOP))
        assert np.array_equal(again[0], base[0]) and np.array_equal(again[1], base[1])
    finally:
        m.close()


def test_stream_marks_at_another_rate(lib, hip_tiny):
    ids, dur = _one_utterance(47, n_vocab=20)
    dur[0, :] += 2  # 30-odd frames: several chunks of 8
    _, ol, want = hip_tiny.synthesize(ids, [11], SCALES, [2], forced_durations=dur, seed=4, sample_rate=8000, marks=True)
    assert np.array_equal(want, R.token_ends(dur, [11], HOP, NATIVE, 8000))
    got = []
    chunks = list(hip_tiny.stream(ids, SCALES, 2, chunk_frames=8, forced_durations=dur, seed=4, sample_rate=8000, on_marks=got.append))
    assert len(got) == 1 and np.array_equal(got[0], want[0])
    assert len(chunks) > 2 and sum(len(c) for c in chunks) == int(want[0, -1]) == int(ol[0])
    # a latent stream has no tokens
    z = np.zeros((hip_tiny.hp.inter_channels, 20), np.float32)
    st, total = ctypes.c_void_p(), ctypes.c_int64()
    lib.check(lib._fn("stream_open_latent")(hip_tiny._h, z.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 20, 8, 0, ctypes.byref(st),
                                            ctypes.byref(total)))
    try:
        assert lib.stream_marks(st).shape == (0,)
    finally:
        lib._fn("stream_close")(st)


# ---- multistream ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def voice(tmp_path_factory):
    from vosk_tts_amd import Model
    from vosk_tts_amd.toymodel import write_toy_multistream_model

    d = str(tmp_path_factory.mktemp("ms_marks"))
    write_toy_multistream_model(d)
    model = Model(model_path=d, device=0)
    yield model
    model.onnx.close()


def test_multistream_marks(lib, voice):
    sess = voice.onnx
    SC = np.array([0.8, 1.0, 0.8], np.float32)  # length_scale 1
    rng = np.random.default_rng(48)
    ids = rng.integers(2, 40, size=(5, 9)).astype(np.int64)
    pde = rng.integers(1, 6, size=9).astype(np.float32)
    want = (np.cumsum(pde) * 256).astype(np.int64)
    plain, _ = sess._model.synthesize(ids, SC, 2, None, pde, seed=9, n_timesteps=2, want_mel=False)
    audio, _, ends = sess._model.synthesize(ids, SC, 2, None, pde, seed=9, n_timesteps=2, want_mel=False, marks=True)
    assert np.array_equal(ends, want) and np.array_equal(audio, plain) and audio.shape[0] == want[-1]
    L, M = R.ratio(NATIVE, 8000)
    a8, _, e8 = sess._model.synthesize(ids, SC, 2, None, pde, seed=9, n_timesteps=2, want_mel=False, marks=True, sample_rate=8000)
    assert e8.tolist() == [R.n_out(v, L, M) for v in want] and a8.shape[0] == e8[-1]
    ref8 = sess.resample(plain[None], [plain.shape[0]], 8000)[0][0]
    assert np.array_equal(a8, ref8)
    _, _, dn = sess._model.synthesize(ids, SC, 2, None, pde, seed=9, n_timesteps=2, want_mel=False, marks=True, denoiser_strength=0.01)
    assert np.array_equal(dn, want)  # the denoiser moves no samples
    # the session's feed
    out = sess.run(None, {"input": ids[None], "input_lengths": np.array([9], np.int64), "scales": SC, "sid": np.array([2], np.int64),
                          "phone_duration_extra": pde[None], "vits.seed": 9, "vits.n_timesteps": 2, "vits.marks": True, "vits.sample_rate": 8000})
    assert len(out) == 3 and np.array_equal(out[2][0], e8) and out[1][0] == e8[-1]
    # ragged batch
    lens = np.array([9, 4, 1], np.int64)
    bids = rng.integers(2, 40, size=(3, 5, 9)).astype(np.int64)
    bpde = rng.integers(1, 6, size=(3, 9)).astype(np.float32)
    sid = np.array([0, 3, 1], np.int64)
    for rate in (None, 8000):
        p_audio, p_ol = sess._model.synthesize_batch(bids, lens, SC, sid, None, bpde, seed=5, n_timesteps=2)
        b_audio, b_ol, b_ends = sess._model.synthesize_batch(bids, lens, SC, sid, None, bpde, seed=5, n_timesteps=2, marks=True, sample_rate=rate)
        assert np.array_equal(b_ends, R.token_ends(bpde.astype(np.int64), lens, 256, NATIVE, rate))
        assert b_ol.tolist() == [int(b_ends[b, lens[b] - 1]) for b in range(3)]
        if rate is None:
            assert np.array_equal(b_audio, p_audio) and np.array_equal(b_ol, p_ol)
    # the stream records them
    got = []
    chunks = list(sess._model.stream(ids, SC, 2, None, pde, seed=9, n_timesteps=2, chunk_frames=8, on_marks=got.append))
    assert len(got) == 1 and np.array_equal(got[0], want) and sum(len(c) for c in chunks) == want[-1]


# ---- the Python door -----------------------------------------------------------------------------------------------------------
TEXT = "Прив+ет, м+ир - да!"


def _check_marks(marks, audio, text_words):
    assert marks.phonemes[0][1] == 0 and marks.phonemes[-1][2] == len(audio)
    for (_, _, e0), (_, s1, _) in zip(marks.phonemes, marks.phonemes[1:]):
        assert e0 == s1
    assert [w[0] for w in marks.words] == text_words
    starts = [w[1] for w in marks.words]
    assert starts == sorted(starts) and all(a <= b for _, a, b in marks.words)


@pytest.mark.parametrize("family", ["vits", "multistream"])
def test_synth_audio_with_marks(lib, tmp_path, voice, family):
    from vosk_tts_amd import Model, Synth
    from vosk_tts_amd.toymodel import write_toy_model

    if family == "vits":
        model = Model(model_path=write_toy_model(str(tmp_path / "v")), device=0)
    else:
        model = voice
    try:
        s = Synth(model)
        kw = dict(speaker_id=1, duration_noise_level=0.0)  # (no duration noise: the same frame counts in every call below)
        audio, marks = s.synth_audio(TEXT, marks=True, **kw)
        assert audio.dtype == np.int16 and marks.rate == NATIVE
        _check_marks(marks, audio, ["прив+ет", "м+ир", "да"])
        bare = s.synth_audio(TEXT, **kw)
        assert isinstance(bare, np.ndarray) and bare.shape == audio.shape
        a8, m8 = s.synth_audio(TEXT, marks=True, sample_rate=8000, **kw)
        L, M = R.ratio(NATIVE, 8000)
        assert m8.rate == 8000 and m8.token_ends.tolist() == [R.n_out(v, L, M) for v in marks.token_ends]
        assert [p[1:] for p in m8.phonemes] == [(R.n_out(a, L, M), R.n_out(b, L, M)) for _, a, b in marks.phonemes]
        assert [w[1:] for w in m8.words] == [(R.n_out(a, L, M), R.n_out(b, L, M)) for _, a, b in marks.words]
        _check_marks(m8, a8, ["прив+ет", "м+ир", "да"])
        calls, chunks = [], []
        for c in s.synth_stream(TEXT, chunk_frames=8, on_marks=lambda mk: calls.append((mk, len(chunks))), **kw):
            chunks.append(c)
        assert len(calls) == 1 and calls[0][1] == 0
        assert calls[0][0].token_ends.tolist() == marks.token_ends.tolist() and sum(len(c) for c in chunks) == len(audio)
    finally:
        if family == "vits":
            model.onnx.close()


@pytest.mark.parametrize("family", ["vits", "vits_bert", "multistream"])
def test_synth_batch_with_marks(lib, tmp_path, family):
    """every shard path of MultiDeviceSynth: plain, BERT-conditioned (one batched front end), multistream"""
    from vosk_tts_amd.batching import MultiDeviceSynth
    from vosk_tts_amd.toymodel import write_toy_model, write_toy_multistream_model

    d = str(tmp_path / "m")
    write_toy_multistream_model(d) if family == "multistream" else write_toy_model(d, bert=family == "vits_bert")
    mds = MultiDeviceSynth(d, devices=[0])
    assert mds.family == family
    try:
        texts = ["Прив+ет, м+ир!", "да", "м+ир - прив+ет, прив+ет."]
        seeds = [11, 12, 13]
        res = mds.synth_batch(texts, speaker_ids=1, seeds=seeds, marks=True)
        plain = mds.synth_batch(texts, speaker_ids=1, seeds=seeds)
        assert len(res) == 3 and all(isinstance(p, np.ndarray) for p in plain)
        s0, sess = mds.synths[0], mds.models[0].onnx
        for text, (audio, marks), p in zip(texts, res, plain):
            assert np.array_equal(audio, p)
            _check_marks(marks, audio, [w for w in __import__("re").split(r"[ ,.!\-]+", text.lower()) if w])
            # the solo call with the same seed and the batch's own frame counts as forced durations
            feed, scale = s0._feed(text, 1, None, None, None, None)
            assert feed["input"].shape[-1] == marks.token_ends.shape[0]
            dur = np.diff(marks.token_ends, prepend=0) // HOP
            if family != "multistream":
                feed.update({"vits.forced_durations": dur[None].astype(np.int32), "vits.seed": seeds[texts.index(text)], "vits.marks": True})
                pcm, ends = sess.run_pcm16(feed, scale)
            else:
                feed.update({"phone_duration_extra": dur[None].astype(np.float32), "vits.seed": seeds[texts.index(text)], "vits.marks": True})
                out = sess.run(None, feed)
                pcm, ends = out[0], out[2]
            assert np.array_equal(ends[0], marks.token_ends) and pcm.shape[-1] == len(audio)
    finally:
        mds.close()
