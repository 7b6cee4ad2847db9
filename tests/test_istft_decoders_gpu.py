"""GPU tests of the multi-stream (dec_type 2) and single-band (dec_type 3) iSTFT decoders: the decoder stage and the whole
path against fixtures computed by the reference's own modules (tools/gen_golden_istft_heads.py), the fused decoder tail
against the separately written iSTFT / synthesis kernels, ragged batches, streaming, and the multi-stream decoder with the
PQMF filter as its learned filter against the multi-band decoder.  (The C oracle decodes types 0 and 1 only.)"""
import numpy as np
import pytest

from conftest import assert_close, golden

pytestmark = pytest.mark.gpu

STAGE_TOL = 1e-4
E2E_TOL = 5e-4
TYPES = ("ms", "istft")


def _hparams(kind):
    from vosk_tts_amd import weights as W

    return W.tiny_multistream_hparams() if kind == "ms" else W.tiny_istft_hparams()


@pytest.fixture(scope="module")
def models(hip_lib):
    from vosk_tts_amd import weights as W

    ms = {k: hip_lib.create(W.synthetic_blob(_hparams(k), 1234), 0) for k in TYPES}
    yield ms
    for m in ms.values():
        m.close()


def _valid(audio, olen):
    a = np.array(audio, copy=True)
    for b, n in enumerate(olen):
        a[b, int(n):] = 0.0
    return a


def _batch(rng, B=3, Tx=30):
    lengths = np.array([Tx, 9, 17][:B], np.int64)
    ids = rng.integers(1, 20, size=(B, Tx)).astype(np.int64)
    dur = rng.integers(0, 5, size=(B, Tx)).astype(np.int32)
    return ids, lengths, np.array([1, 4, 2][:B], np.int64), dur


def test_new_dec_types_report_themselves(models):
    assert models["ms"].hp.dec_type == 2 and models["istft"].hp.dec_type == 3
    assert models["ms"].hp.hop_length == models["istft"].hp.hop_length == 256


@pytest.mark.parametrize("kind", TYPES)
def test_decoder_stage_matches_reference_module(models, kind):
    g = golden(f"{kind}_dec_b2")
    audio, mb = models[kind].decoder(g["z"])
    assert_close("audio(golden)", g["audio"], audio, STAGE_TOL)
    if kind == "ms":
        S = models[kind].hp.subbands
        ymb = g["y_mb_hat"]
        assert mb.shape == (2, S, ymb.shape[2] // S)
        assert_close("audio_mb(golden y_mb_hat on every S-th sample / S)", ymb[:, :, ::S] / S, mb, STAGE_TOL)
    else:
        assert mb is None


@pytest.mark.parametrize("kind", TYPES)
def test_fused_tail_equals_separate_kernels(hip_lib, models, kind):
    """istft_tail_kernel<true / false> against istft_kernel (+ pqmf_synthesis_kernel): dense with T_y = 70 (70 tail blocks),
    and a ragged batch through the full path (defined zeros beyond each item's decoded tail on both)."""
    m = models[kind]
    rng = np.random.default_rng(8)
    z = rng.standard_normal((2, 64, 70)).astype(np.float32)
    ids, lengths, sid, dur = _batch(rng)
    try:
        dense, full = [], []
        for impl in (1, 0):
            hip_lib.lib.vits_debug_tail_impl(impl)
            dense.append(m.decoder(z))
            full.append(m.synthesize(ids, lengths, [0.667, 1.0, 0.8], sid, forced_durations=dur, seed=4))
    finally:
        hip_lib.lib.vits_debug_tail_impl(0)
    assert_close("dense audio, fused vs separate", dense[0][0], dense[1][0], 1e-5)
    if kind == "ms":
        assert_close("dense audio_mb, fused vs separate", dense[0][1], dense[1][1], 1e-5)
    assert np.array_equal(full[0][1], full[1][1])
    assert_close("ragged batch, fused vs separate", full[0][0], full[1][0], 1e-5)
    tail = hip_lib.decoder_needs(m.hp)["tail_cols"]
    per_col = 256 // (m.hp.up_rates[0] * m.hp.up_rates[1])
    for a, olen in full:
        assert np.isfinite(a).all()
        for b in range(3):
            assert np.all(a[b, int(olen[b]) + tail * per_col:] == 0.0)


@pytest.mark.parametrize("kind", TYPES)
def test_end_to_end_ragged_batch_matches_reference(models, kind):
    g = golden(f"{kind}_e2e_b3")
    m = models[kind]
    ids, lengths, sid, scales = g["ids"], g["lengths"], g["sid"], g["scales"]
    Ty = int(g["y_lengths"].max())
    _dur, ylen, z_p = m.regulate(None, g["forced_durations"], lengths, float(scales[1]), *m.text_encoder(ids, lengths, sid)[1:],
                                 g["noise_prior"], float(scales[0]), Ty)
    assert np.array_equal(ylen, g["y_lengths"])
    assert_close("z(golden)", g["z"], m.flow(z_p, ylen, sid), STAGE_TOL)
    audio, olen = m.synthesize(ids, lengths, scales, sid, noise_dp=g["noise_dp"], noise_prior=g["noise_prior"],
                               forced_durations=g["forced_durations"])
    assert np.array_equal(olen, g["y_lengths"] * 256)
    assert_close("audio(e2e, golden)", _valid(g["audio"], olen), _valid(audio, olen), E2E_TOL)


@pytest.mark.parametrize("kind", TYPES)
def test_ragged_batch_with_poisoned_workspace(hip_lib, models, kind):
    """NaN-filled fresh workspaces: a valid sample that reads anything the ragged limits (decoder_needs / rag_halo) left
    unwritten would surface as NaN or a mismatch."""
    from vosk_tts_amd import weights as W

    rng = np.random.default_rng(31)
    ids, lengths, sid, dur = _batch(rng)
    want, wlen = models[kind].synthesize(ids, lengths, [0.667, 1.0, 0.8], sid, forced_durations=dur, seed=9)
    hip_lib.lib.vits_debug_poison_workspace(1)
    try:
        fresh = hip_lib.create(W.synthetic_blob(_hparams(kind), 1234), 0)
        try:
            got, glen = fresh.synthesize(ids, lengths, [0.667, 1.0, 0.8], sid, forced_durations=dur, seed=9)
        finally:
            fresh.close()
    finally:
        hip_lib.lib.vits_debug_poison_workspace(0)
    assert np.array_equal(wlen, glen)
    assert np.isfinite(got).all()
    assert_close("poisoned workspace", _valid(want, wlen), _valid(got, glen), 1e-6)


@pytest.mark.parametrize("kind", TYPES)
@pytest.mark.parametrize("chunk", [16, 37, 200])
def test_streaming_chunks_equal_one_shot(models, kind, chunk):
    m = models[kind]
    rng = np.random.default_rng(11)
    Tx = 40
    ids = rng.integers(1, 20, size=(1, Tx)).astype(np.int64)
    dur = rng.integers(1, 6, size=(1, Tx)).astype(np.int32)
    Ty = int(dur.sum())
    scales = [0.667, 1.0, 0.8]
    one, _ = m.synthesize(ids, [Tx], scales, [2], forced_durations=dur, seed=5)
    chunks = list(m.stream(ids, scales, 2, chunk_frames=chunk, forced_durations=dur, seed=5))
    assert len(chunks) == -(-Ty // chunk)
    got = np.concatenate(chunks)[None]
    assert got.shape == one.shape == (1, Ty * 256)
    assert_close("stream vs one-shot", one, got, 2e-5)


def _pqmf_synthesis_filter(S=4, taps=62, cutoff=0.15, beta=9.0):
    """PQMF.synthesis_filter (the Kaiser-window prototype and its cosine modulation, pqmf.py:15-75) in numpy -> [S, taps + 1]"""
    n = np.arange(taps + 1)
    x = n - 0.5 * taps
    with np.errstate(invalid="ignore", divide="ignore"):
        h = np.sin(np.pi * cutoff * x) / (np.pi * x)
    h[taps // 2] = cutoff
    proto = h * np.kaiser(taps + 1, beta)
    k = np.arange(S)[:, None]
    return 2 * proto[None] * np.cos((2 * k + 1) * (np.pi / (2 * S)) * (n[None] - (taps - 1) / 2) - (-1.0) ** k * np.pi / 4)


def test_multistream_with_the_pqmf_filter_is_the_multiband_decoder(hip_lib):
    """Default size, no golden needed: a type-2 blob whose post-conv bias is zero and whose learned filter is the PQMF
    synthesis filter computes what the type-0 blob with the same other weights computes -- one utterance at the c2 size and
    a ragged batch of 8."""
    from vosk_tts_amd import weights as W

    filt = _pqmf_synthesis_filter()
    assert_close("numpy PQMF filter vs the reference's", golden("consts")["pqmf_synthesis_filter"], filt, 1e-6)
    hp0, hp2 = W.default_hparams(), W.multistream_hparams()
    t0 = W.make_synthetic_weights(hp0, 1234)
    t2 = dict(t0)
    t2["dec.subband_conv_post.bias"] = np.zeros(72, np.float32)
    t2["dec.multistream_conv_post.weight"] = filt.astype(np.float32)[None]
    m0, m2 = hip_lib.create(W.pack_blob(hp0, t0), 0), hip_lib.create(W.pack_blob(hp2, t2), 0)
    try:
        rng = np.random.default_rng(1234)
        ids = rng.integers(1, 62, size=(1, 50)).astype(np.int64)
        dur = np.full((1, 50), 3, np.int32)
        a0, l0 = m0.synthesize(ids, [50], [0.667, 1.0, 0.8], [2], forced_durations=dur, seed=3)
        a2, l2 = m2.synthesize(ids, [50], [0.667, 1.0, 0.8], [2], forced_durations=dur, seed=3)
        assert a0.shape == (1, 38400) and np.array_equal(l0, l2)
        assert_close("c2: type 2 with PQMF filter vs type 0", a0, a2, 1e-5)
        lengths = rng.integers(10, 61, size=8).astype(np.int64)
        ids = rng.integers(1, 62, size=(8, int(lengths.max()))).astype(np.int64)
        dur = rng.integers(0, 5, size=ids.shape).astype(np.int32)
        sid = rng.integers(0, 200, size=8).astype(np.int64)
        a0, l0 = m0.synthesize(ids, lengths, [0.667, 1.0, 0.8], sid, forced_durations=dur, seed=4)
        a2, l2 = m2.synthesize(ids, lengths, [0.667, 1.0, 0.8], sid, forced_durations=dur, seed=4)
        assert np.array_equal(l0, l2)
        assert_close("B=8 ragged: type 2 with PQMF filter vs type 0", a0, a2, 1e-5)
    finally:
        m0.close()
        m2.close()


def test_multistream_model_onnx_through_the_user_api(tmp_path):
    """A model directory whose model.onnx is a multi-stream graph loads through vosk_tts_amd.Model; Synth.synth_audio gives
    the int16 PCM of synthesize_pcm16 on the same inputs."""
    import os

    from vosk_tts_amd import Model, Synth
    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.toymodel import PHONEMES, write_toy_model

    hp = W.tiny_multistream_hparams(n_vocab=len(PHONEMES))
    d = write_toy_model(str(tmp_path / "m"), hp)
    _hp, tensors = W.unpack_blob(open(os.path.join(d, "model.vitsw"), "rb").read())
    oi.write_minimal_onnx(os.path.join(d, "model.onnx"), tensors)
    os.remove(os.path.join(d, "model.vitsw"))
    model = Model(model_path=d, device=0)
    assert model.onnx._model.hp.dec_type == 2
    synth = Synth(model)
    text = "прив+ет, м+ир!"
    pcm = synth.synth_audio(text, speaker_id=2, noise_level=0.0, speech_rate=1.0, duration_noise_level=0.0)
    assert pcm.dtype == np.int16 and pcm.size > 0 and pcm.size % 256 == 0
    ids = np.array([synth.g2p_noembed(text)], np.int64)
    want, _ = model.onnx._model.synthesize_pcm16(ids, [ids.shape[1]], [0.0, 1.0, 0.0], [2])
    assert np.array_equal(pcm, want.reshape(-1))
