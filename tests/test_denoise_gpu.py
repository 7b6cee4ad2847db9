"""GPU tests of the vocoder-bias denoiser (include/vits_denoise.h): the kernels against the float64 restatement
(tests/denoise_ref.py), the bias, the refusals, and the flag through stts_synthesize / _batch / stream_open, SttsSession and Synth.

Bound of the kernel-level test: max|y - ref| <= 4e-6 * max|x| per item.  torch's own fp32 run of the same transform on the CPU is
1.9e-7 .. 3.7e-7 of max|x| from the float64 restatement; the kernel gets about ten times that for another FFT factorisation and an
fp32 twiddle table.  The test prints both figures for every item."""
import numpy as np
import pytest

import denoise_ref as R
from conftest import assert_close

pytestmark = pytest.mark.gpu
OP_TOL = 4e-6
BATCH_TOL = 2e-5   # batch against solo, as tests/test_stts_hip_parity.py
STREAM_TOL = 2e-5  # streamed against one-shot
SC = np.array([0.8, 1.0, 0.8], np.float32)


def _op_case(n):
    hop = n // 4
    lengths = np.array([n // 2 + 1, 3 * hop + 17, 3 * n, 40 * hop, 41 * hop + 1], np.int64)
    rng = np.random.default_rng(1000 + n)
    x = rng.uniform(-0.3, 0.3, (len(lengths), int(lengths.max()))).astype(np.float32)
    for b, length in enumerate(lengths):
        x[b, length:] = 1e30  # never read
    # windowed uniform +-0.3 noise has rms |X| = sqrt(0.03 * 3 n / 8) (3.4 at n = 1024), Rayleigh: median = 0.83 rms.  A positive
    # random bias around 1 and strength = that median put about half of the bins under the threshold
    bias = rng.uniform(0.5, 1.5, n // 2 + 1).astype(np.float32)
    strength = float(np.float32(0.83 * np.sqrt(0.03 * 3 * n / 8)))
    return lengths, x, bias, strength


def _torch_fp32(x, bias, strength, n):
    import torch

    w = torch.hann_window(n, dtype=torch.float32)
    spec = torch.stft(torch.as_tensor(x)[None], n_fft=n, hop_length=n // 4, win_length=n, window=w, return_complex=True)
    mag = spec.abs()
    new = torch.clamp(mag - torch.as_tensor(bias)[None, :, None] * strength, 0.0)
    spec = spec * torch.where(mag > 0, new / mag, torch.zeros_like(mag))
    return torch.istft(spec, n_fft=n, hop_length=n // 4, win_length=n, window=w)[0].numpy()


@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024])  # log2 (n/2) odd: the transform ends in the radix-2 pass; even (128, 512): radix-4 alone
def test_op_against_float64(hip_lib, n):
    lengths, x, bias, strength = _op_case(n)
    hop = n // 4
    refs, shares = [], []
    for b, length in enumerate(lengths):
        y, c = R.denoise(x[b, :length], bias, strength, n, return_clamped=True)
        refs.append(y)
        shares.append(c * (1 + length // hop))
    share = sum(shares) / sum(1 + length // hop for length in lengths)
    assert 0.2 <= share <= 0.8, share  # a gain that never or always clamps cannot pass unnoticed
    for s in (0.0, strength):
        y = hip_lib.op_denoise(x, lengths, bias, s, n)
        assert y.shape == (len(lengths), hop * (x.shape[1] // hop)) and y.dtype == np.float32
        for b, length in enumerate(lengths):
            n_out = hop * (int(length) // hop)
            ref = refs[b] if s else x[b, :n_out].astype(np.float64)
            scale = np.abs(x[b, :length]).max()
            err = np.abs(y[b, :n_out] - ref).max() / scale
            t_err = np.abs(_torch_fp32(x[b, :length], bias, s, n) - (refs[b] if s else R.denoise(x[b, :length], bias, 0.0, n))).max() / scale
            print(f"n {n} strength {s:.4g} len {length}: kernel {err:.3e}  torch fp32 {t_err:.3e}  (of max|x|; clamped share {share:.2f})")
            assert err <= OP_TOL, (n, s, int(length), err)
            assert not y[b, n_out:].any()
        assert np.array_equal(y, hip_lib.op_denoise(x, lengths, bias, s, n))  # no atomics: the same bits twice


@pytest.fixture(scope="module")
def voice(tmp_path_factory):
    from vosk_tts_amd import Model
    from vosk_tts_amd.toymodel import write_toy_multistream_model

    d = str(tmp_path_factory.mktemp("ms"))
    write_toy_multistream_model(d)
    model = Model(model_path=d, device=0)
    yield model
    model.onnx.close()


def _ids(T, seed, n_vocab=40):
    return np.random.default_rng(seed).integers(1, n_vocab, size=(5, T)).astype(np.int64)


def _strength_for(audio, bias, n=1024):
    """a strength that puts the median bin of `audio` at its threshold (worked out on the float64 side only)"""
    X = np.abs(np.fft.rfft(R.frames(audio, n), axis=1))
    return float(np.median(X / np.maximum(np.asarray(bias, np.float64)[None, :], 1e-30)))


@pytest.mark.parametrize("n", [256, 1024])
def test_bias_is_frame_0_of_the_zero_mel(voice, n):
    voc = voice.onnx._vocoder
    audio, _ = voc.decoder(np.zeros((1, voc.hp.inter_channels, 88), np.float32), want_mb=False)
    want = R.bias_of(audio[0], n)
    got = voc.denoise_bias(n)
    assert got.shape == (n // 2 + 1,) and got.dtype == np.float32
    err = np.abs(got - want).max() / want.max()
    print(f"bias n {n}: {err:.3e} of max(bias) = {want.max():.4g}")
    # an fp32 FFT is off by about 2^-24 log2(n) |frame|_2 per bin, and max|X| >= |frame|_2 by Parseval: the bound is over ten times that
    assert err <= 1e-5
    assert np.array_equal(got, voc.denoise_bias(n))  # the cached copy
    if n == 1024:
        assert np.array_equal(got, voc.denoise_bias(0))  # 0 = 1024


def test_refusals_name_the_value(hip_lib, voice):
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.capi import VitsError

    x = np.zeros((1, 4096), np.float32)
    for bad in (100, 2048):
        with pytest.raises(VitsError, match=str(bad)) as e:
            hip_lib.op_denoise(x, [4096], np.ones(bad // 2 + 1), 0.1, bad)
        assert e.value.code == 4
        with pytest.raises(VitsError, match=str(bad)):
            voice.onnx._vocoder.denoise_bias(bad)
    with pytest.raises(VitsError, match="512") as e:  # below n/2 + 1 = 513
        hip_lib.op_denoise(x, [512], np.ones(513), 0.1, 1024)
    assert e.value.code == 1  # VITS_ERR_ARG
    with pytest.raises(VitsError, match="4097"):
        hip_lib.op_denoise(x, [4097], np.ones(513), 0.1, 1024)
    with pytest.raises(VitsError, match="-0.5") as e:
        hip_lib.op_denoise(x, [4096], np.ones(513), -0.5, 1024)
    assert e.value.code == 1  # VITS_ERR_ARG
    sess = voice.onnx
    with pytest.raises(VitsError, match="-0.5"):
        sess._model.synthesize(_ids(4, 1), SC, 0, None, np.full(4, 3.0, np.float32), seed=1, denoiser_strength=-0.5)
    with pytest.raises(VitsError, match="2048"):
        sess._model.synthesize_batch(_ids(4, 1)[None], [4], SC, [0], denoiser_strength=0.1, denoiser_filter_length=2048)
    # a vocoder whose hop_length (32) is not a multiple of the denoiser's hop (256)
    hp = W.decoder_hparams(1, ((8, 16), (4, 8)), (3, 7), (1, 3), None, 128, 32)
    assert hp.hop_length == 32
    small = hip_lib.create(W.synthetic_blob(hp, 7), 0)
    try:
        with pytest.raises(VitsError, match="32.*256") as e:
            small.stream_latent(np.zeros((32, 40), np.float32), chunk_frames=8, denoiser_strength=0.1)
        assert e.value.code == 4
    finally:
        small.close()
    # a stream with both a strength and another rate
    with pytest.raises(VitsError, match="8000") as e:
        sess._vocoder.stream_latent(np.zeros((80, 40), np.float32), chunk_frames=8, sample_rate=8000, denoiser_strength=0.1)
    assert e.value.code == 4
    feed = {"input": _ids(4, 1)[None], "input_lengths": np.array([4], np.int64), "scales": SC, "sid": np.array([0], np.int64),
            "vits.denoiser_strength": 0.1, "vits.sample_rate": 8000}
    with pytest.raises(VitsError, match="8000"):
        sess.run_stream(None, feed)


@pytest.fixture(scope="module")
def one_shot(voice):
    """one utterance of 53 frames: (ids, pde, plain audio, mel, bias, strength, denoised audio) shared by the tests below"""
    sess = voice.onnx
    ids, pde = _ids(53, 21), np.ones(53, np.float32)
    plain, mel = sess._model.synthesize(ids, SC, 2, None, pde, seed=9)
    bias = sess._vocoder.denoise_bias(1024)
    strength = _strength_for(plain, bias)
    got, mel2 = sess._model.synthesize(ids, SC, 2, None, pde, seed=9, denoiser_strength=strength)
    for a in (plain, mel, bias, got, mel2):
        a.setflags(write=False)
    return dict(ids=ids, pde=pde, plain=plain, mel=mel, bias=bias, strength=strength, got=got, mel2=mel2)


def test_one_shot(voice, hip_lib, one_shot):
    o = one_shot
    sess = voice.onnx
    plain, got = o["plain"], o["got"]
    assert plain.shape == got.shape == (53 * 256,) and np.array_equal(o["mel"], o["mel2"])
    scale = np.abs(plain).max()
    ref, clamped = R.denoise(plain, o["bias"], o["strength"], 1024, return_clamped=True)
    assert 0.2 <= clamped <= 0.8
    assert np.abs(ref - plain).max() > 100 * OP_TOL * scale  # the denoiser does something at this strength
    op = hip_lib.op_denoise(plain[None], [plain.shape[0]], o["bias"], o["strength"], 1024)[0]
    e_op, e_ref = np.abs(got - op).max() / scale, np.abs(got - ref).max() / scale
    print(f"one-shot: against op_denoise {e_op:.3e}, against float64 {e_ref:.3e} (of max|x| = {scale:.4g}; clamped share {clamped:.2f})")
    assert e_op <= OP_TOL and e_ref <= OP_TOL
    # the eager path (an injected noise tensor bypasses the captured graphs) carries the flag too
    noise = np.random.default_rng(2).standard_normal((80, 56)).astype(np.float32)
    p2, _ = sess._model.synthesize(o["ids"], SC, 2, None, o["pde"], noise=noise)
    g2, _ = sess._model.synthesize(o["ids"], SC, 2, None, o["pde"], noise=noise, denoiser_strength=o["strength"])
    want = hip_lib.op_denoise(p2[None], [p2.shape[0]], o["bias"], o["strength"], 1024)[0]
    assert np.abs(g2 - want).max() <= OP_TOL * np.abs(p2).max()
    # another filter length: hop 64 divides the vocoder's 256
    g3, _ = sess._model.synthesize(o["ids"], SC, 2, None, o["pde"], seed=9, denoiser_strength=o["strength"], denoiser_filter_length=256)
    want = hip_lib.op_denoise(plain[None], [plain.shape[0]], sess._vocoder.denoise_bias(256), o["strength"], 256)[0]
    assert np.abs(g3 - want).max() <= OP_TOL * scale
    # flag unset: today's bits; a one-frame utterance (256 samples < 513) is returned undenoised, bit for bit
    again, _ = sess._model.synthesize(o["ids"], SC, 2, None, o["pde"], seed=9)
    assert np.array_equal(again, plain)
    ids1, pde1 = _ids(1, 5), np.ones(1, np.float32)
    a, _ = sess._model.synthesize(ids1, SC, 1, None, pde1, seed=4)
    b, _ = sess._model.synthesize(ids1, SC, 1, None, pde1, seed=4, denoiser_strength=0.0)
    c, _ = sess._model.synthesize(ids1, SC, 1, None, pde1, seed=4, denoiser_strength=50.0)
    assert a.shape == (256,) and np.array_equal(a, b) and np.array_equal(a, c)


def test_batch_items_equal_their_solo_runs(voice, one_shot):
    sess = voice.onnx
    rng = np.random.default_rng(77)
    B, Tx = 3, 20
    lengths = np.array([20, 1, 9], np.int64)  # the middle item (2 frames = 512 samples) is too short for n = 1024: passed through
    ids = rng.integers(1, 40, size=(B, 5, Tx)).astype(np.int64)
    pde = np.full((B, Tx), 2.0, np.float32)
    sid = np.array([0, 3, 1], np.int64)
    s = one_shot["strength"]
    audio, olen = sess._model.synthesize_batch(ids, lengths, SC, sid, None, pde, seed=50, n_timesteps=3, denoiser_strength=s)
    plain, plen = sess._model.synthesize_batch(ids, lengths, SC, sid, None, pde, seed=50, n_timesteps=3)
    assert np.array_equal(olen, plen) and olen.tolist() == [40 * 256, 2 * 256, 18 * 256] and audio.shape == plain.shape
    for b in range(B):
        L = int(lengths[b])
        one, _ = sess._model.synthesize(ids[b][:, :L], SC, int(sid[b]), None, pde[b][:L], seed=50 + b, n_timesteps=3, want_mel=False, denoiser_strength=s)
        assert_close(f"item {b}", one, audio[b, :olen[b]], BATCH_TOL)
        assert not audio[b, olen[b]:].any()
    assert np.array_equal(audio[1], plain[1])
    assert np.abs(audio[0] - plain[0]).max() > 100 * BATCH_TOL * np.abs(plain[0]).max()
    # the session's batch door
    a2, l2 = sess.run_batch({"input": ids, "input_lengths": lengths, "scales": SC, "sid": sid, "phone_duration_extra": pde, "vits.seed": 50,
                             "vits.n_timesteps": 3, "vits.denoiser_strength": s})
    assert np.array_equal(a2, audio) and np.array_equal(l2, olen)


def test_streamed_chunks_equal_the_one_shot_call(voice, one_shot):
    o = one_shot
    sess = voice.onnx
    sizes = [8 * 256] * 6 + [5 * 256]
    plain_parts = list(sess._model.stream(o["ids"], SC, 2, None, o["pde"], seed=9, chunk_frames=8))
    assert [len(p) for p in plain_parts] == sizes
    parts = list(sess._model.stream(o["ids"], SC, 2, None, o["pde"], seed=9, chunk_frames=8, denoiser_strength=o["strength"]))
    assert [len(p) for p in parts] == sizes
    assert_close("stts_stream_open", o["got"], np.concatenate(parts), STREAM_TOL)
    parts = list(sess._vocoder.stream_latent(o["mel"], chunk_frames=8, clamp=True, denoiser_strength=o["strength"]))
    assert [len(p) for p in parts] == sizes
    assert_close("stream_latent", o["got"], np.concatenate(parts), STREAM_TOL)
    # a one-frame utterance streams undenoised
    ids1, pde1 = _ids(1, 5), np.ones(1, np.float32)
    a, _ = sess._model.synthesize(ids1, SC, 1, None, pde1, seed=4)
    got = np.concatenate(list(sess._model.stream(ids1, SC, 1, None, pde1, seed=4, chunk_frames=8, denoiser_strength=50.0)))
    assert_close("short stream", a, got, STREAM_TOL)


@pytest.mark.parametrize("n", [1024, 256])
def test_long_stream_decodes_in_windows_with_the_wider_halo(voice, hip_lib, n):
    """300 frames at chunk_frames 8 (and 16): longer than the wide window of 8 chunks plus both halos, so the first chunk's own window,
    wide windows that start inside the utterance (slot offset > 0), the decode-ahead into the other slot and the last window shifted
    inward all run, and every chunk's frames read the ceil(n / hop_length) extra halo frames either side"""
    sess = voice.onnx
    voc = sess._vocoder
    Ty, halo = 300, hip_lib.rag_halo(voc.hp) + -(-n // voc.hp.hop_length)
    assert Ty > 8 * 16 + 2 * halo  # more than one wide window at both chunk sizes
    ids, pde = _ids(100, 33), np.full(100, 3.0, np.float32)
    plain, mel = sess._model.synthesize(ids, SC, 1, None, pde, seed=12)
    assert mel.shape == (80, Ty)
    strength = _strength_for(plain, voc.denoise_bias(n), n)
    want, _ = sess._model.synthesize(ids, SC, 1, None, pde, seed=12, denoiser_strength=strength, denoiser_filter_length=n)
    assert np.abs(want - plain).max() > 100 * STREAM_TOL * np.abs(plain).max()
    for cf in (8, 16):
        sizes = [cf * 256] * (Ty // cf) + ([(Ty % cf) * 256] if Ty % cf else [])
        parts = list(sess._model.stream(ids, SC, 1, None, pde, seed=12, chunk_frames=cf, denoiser_strength=strength, denoiser_filter_length=n))
        assert [len(p) for p in parts] == sizes
        assert_close(f"stts_stream_open n={n} chunk={cf}", want, np.concatenate(parts), STREAM_TOL)
        parts = list(voc.stream_latent(mel, chunk_frames=cf, clamp=True, denoiser_strength=strength, denoiser_filter_length=n))
        assert [len(p) for p in parts] == sizes
        assert_close(f"stream_latent n={n} chunk={cf}", want, np.concatenate(parts), STREAM_TOL)


def test_multi_device_synth_applies_the_config_default(tmp_path):
    """the batched serving door: inference.denoiser_strength of the voice's config (or the argument) reaches stts_synthesize_batch:
    same seeds, the config default and the argument give the same bits, and they differ from the undenoised ones"""
    from vosk_tts_amd.batching import MultiDeviceSynth
    from vosk_tts_amd.toymodel import write_toy_multistream_model

    inf = {"noise_level": 0.8, "speech_rate": 1.0, "duration_noise_level": 0.8, "scale": 1.0}
    write_toy_multistream_model(str(tmp_path / "plain"), inference=dict(inf))
    write_toy_multistream_model(str(tmp_path / "dn"), inference=dict(inf, denoiser_strength=0.4))
    texts = ["прив+ет, м+ир!", "м+ир."]
    out = {}
    for name, kw in (("plain", {}), ("dn", {}), ("arg", {"denoiser_strength": 0.4})):
        mds = MultiDeviceSynth(model_path=str(tmp_path / ("dn" if name == "dn" else "plain")), devices=[0])
        try:
            out[name] = mds.synth_batch(texts, speaker_ids=1, seeds=[5, 6], **kw)
        finally:
            mds.close()
    for a, b, c in zip(out["plain"], out["dn"], out["arg"]):
        assert a.shape == b.shape and np.array_equal(b, c) and not np.array_equal(a, b)


def test_session_and_synth_reach_the_model_level_call(voice, hip_lib, one_shot):
    from vosk_tts_amd import Synth

    o = one_shot
    sess = voice.onnx
    feed = {"input": o["ids"][None], "input_lengths": np.array([53], np.int64), "scales": SC, "sid": np.array([2], np.int64),
            "phone_duration_extra": o["pde"][None], "vits.seed": 9, "vits.denoiser_strength": o["strength"]}
    wav, n = sess.run(None, feed)
    assert n[0] == 53 * 256 and np.array_equal(wav[0], o["got"])
    got = np.concatenate(list(sess.run_stream(None, feed, chunk_frames=8)))
    assert_close("run_stream", o["got"], got, STREAM_TOL)
    feed["vits.denoiser_filter_length"] = 256
    w256, _ = sess.run(None, feed)
    want, _ = sess._model.synthesize(o["ids"], SC, 2, None, o["pde"], seed=9, denoiser_strength=o["strength"], denoiser_filter_length=256)
    assert np.array_equal(w256[0], want)
    del feed["vits.denoiser_filter_length"]
    # another rate: the denoised native buffer, resampled
    feed["vits.sample_rate"] = 8000
    w8, n8 = sess.run(None, feed)
    want = hip_lib.op_resample(o["got"][None], [o["got"].shape[0]], sess._vocoder.hp.sampling_rate, 8000)[0]
    assert n8[0] == want.shape[0] and np.array_equal(w8[0], want)
    # Synth: the argument reaches the feed; same text and seed counter position -> compare through the feed the Synth builds
    synth = Synth(voice)
    args, scale = synth._feed("м+ир.", 1, None, None, None, None)
    args["vits.seed"] = 77
    plain = sess.run(None, args)[0][0]
    strength = _strength_for(plain, o["bias"])
    args["vits.denoiser_strength"] = strength
    want = synth.audio_float_to_int16(sess.run(None, args)[0].squeeze() * scale)
    seen = {}
    real = sess.run
    sess.run = lambda names, f, *a, **kw: real(names, dict(seen.setdefault("feed", f), **{"vits.seed": 77}), *a, **kw)
    try:
        pcm = synth.synth_audio("м+ир.", speaker_id=1, denoiser_strength=strength)
    finally:
        sess.run = real
    assert seen["feed"]["vits.denoiser_strength"] == strength and pcm.dtype == np.int16 and np.array_equal(pcm, want)
    assert not np.array_equal(pcm, synth.audio_float_to_int16(plain * scale))
