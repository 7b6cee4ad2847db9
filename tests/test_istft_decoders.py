"""The multi-stream (dec_type 2, Multistream_iSTFT_Generator, models.py:1066-1163) and single-band (dec_type 3,
iSTFT_Generator, models.py:901-971) iSTFT decoders on the CPU side: ONNX import, tensor inventory, hparams checks and the
ragged-batch limits (host arithmetic).  The GPU side is tests/test_istft_decoders_gpu.py."""
import numpy as np
import pytest


def _stride_nodes(strides_ups, stft_hop):
    nodes = [(f"/dec/ups.{i}/ConvTranspose", "ConvTranspose", ["x"], ["y"], {"strides": [u]}) for i, u in enumerate(strides_ups)]
    nodes.append(("/dec/stft/ConvTranspose", "ConvTranspose", ["x"], ["y"], {"strides": [stft_hop]}))
    return nodes


def test_multistream_graph_imports_as_dec_type_2(tmp_path):
    """A multi-stream voice's graph has the multi-band decoder's subband_conv_post shape; it must not import as the
    multi-band decoder (which would drop the post-conv bias and the learned synthesis filter and play PQMF audio)."""
    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W

    rng = np.random.default_rng(5)
    t = W.make_synthetic_weights(W.tiny_hparams(), 3)
    bias = rng.standard_normal(72).astype(np.float32)
    filt = rng.standard_normal((1, 4, 63)).astype(np.float32)
    t["dec.subband_conv_post.bias"] = bias
    t["dec.multistream_conv_post.weight"] = filt
    hp, tens = oi.import_onnx(oi.write_minimal_onnx(str(tmp_path / "ms.onnx"), t))
    assert hp.dec_type == 2
    assert (hp.subbands, hp.istft_n_fft, hp.istft_hop, hp.pqmf_taps, hp.hop_length) == (4, 16, 4, 62, 256)
    assert np.array_equal(tens["dec.subband_conv_post.bias"], bias)
    assert np.array_equal(tens["dec.multistream_conv_post.weight"], filt)
    assert set(tens) == {n for n, *_ in W.tensor_specs(hp)}
    hp2, tens2 = W.unpack_blob(W.pack_blob(hp, tens))
    assert hp2.dec_type == 2 and np.array_equal(tens2["dec.multistream_conv_post.weight"], filt)


def test_istft_graph_imports_as_dec_type_3(tmp_path):
    """conv_post with n_fft + 2 rows: the single-band decoder.  The iSTFT hop comes from the STFT ConvTranspose stride,
    hop_length = prod(upsample_rates) * hop; a training config's "subbands" does not apply; a contradicting hop_length raises."""
    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W

    t = W.make_synthetic_weights(W.tiny_istft_hparams(), 3)
    assert "dec.conv_post.weight" in t and t["dec.conv_post.weight"].shape == (18, 32, 7)
    assert not any(k.startswith("dec.cond.") or k == "dec.conv_post.bias" for k in t)
    path = oi.write_minimal_onnx(str(tmp_path / "i.onnx"), t, nodes=_stride_nodes([8, 8], 4))
    hp, tens = oi.import_onnx(path)
    assert hp.dec_type == 3
    assert (hp.istft_n_fft, hp.istft_hop, hp.subbands, hp.hop_length) == (16, 4, 1, 256)
    assert [hp.up_rates[i] for i in range(hp.n_ups)] == [8, 8]
    assert np.array_equal(tens["dec.conv_post.weight"], t["dec.conv_post.weight"])
    # the graph decides the hop: stride 2 -> 128 samples per frame
    hp2, _ = oi.import_onnx(oi.write_minimal_onnx(str(tmp_path / "i2.onnx"), t, nodes=_stride_nodes([8, 8], 2)))
    assert (hp2.istft_hop, hp2.hop_length) == (2, 128)
    # config values: the reference's training config carries subbands 4 even for istft_vits
    hp3, _ = oi.import_onnx(path, {"subbands": 4, "gen_istft_hop_size": 4, "upsample_rates": [8, 8], "hop_length": 256})
    assert (hp3.subbands, hp3.hop_length) == (1, 256)
    with pytest.raises(ValueError, match="hop_length"):
        oi.import_onnx(path, {"hop_length": 300})


def test_resblock2_and_deterministic_duration_predictor_are_named():
    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W

    t = W.make_synthetic_weights(W.tiny_hparams(), 3)
    r2 = {k: v for k, v in t.items() if not k.startswith("dec.resblocks.")}
    r2["dec.resblocks.0.convs.0.weight"] = np.zeros((64, 64, 3), np.float32)
    r2["dec.resblocks.0.convs.1.weight"] = np.zeros((64, 64, 3), np.float32)
    with pytest.raises(NotImplementedError, match="ResBlock2"):
        oi.import_onnx(_bytes(r2))
    dp = {k: v for k, v in t.items() if not k.startswith("dp.flows.")}
    dp["dp.conv_1.weight"] = np.zeros((256, 64, 3), np.float32)
    dp["dp.norm_1.gamma"] = np.ones(256, np.float32)
    with pytest.raises(NotImplementedError, match="DurationPredictor"):
        oi.import_onnx(_bytes(dp))


def _bytes(tensors):
    import os
    import tempfile

    from vosk_tts_amd import onnx_import as oi

    with tempfile.TemporaryDirectory() as d:
        p = oi.write_minimal_onnx(os.path.join(d, "m.onnx"), tensors)
        return open(p, "rb").read()


def test_hparams_checks_for_the_new_decoder_types():
    from vosk_tts_amd import weights as W

    for hp in (W.multistream_hparams(), W.tiny_multistream_hparams(), W.istft_hparams(), W.tiny_istft_hparams()):
        W.validate_hparams(hp)
        assert hp.hop_length == 256
        W.unpack_blob(W.synthetic_blob(hp, 7))
    hp = W.tiny_hparams()
    hp.dec_type = 4
    with pytest.raises(ValueError, match="dec_type 4"):
        W.pack_blob(hp, W.make_synthetic_weights(W.tiny_hparams(), 1))
    hp = W.tiny_multistream_hparams()
    hp.pqmf_taps = 61
    with pytest.raises(ValueError, match="odd"):
        W.validate_hparams(hp)
    hp = W.tiny_istft_hparams()
    hp.subbands = 4
    with pytest.raises(ValueError, match="subbands"):
        W.validate_hparams(hp)
    hp = W.tiny_istft_hparams()
    hp.up_rates[1] = 4  # 8 * 4 * 4 = 128 samples per frame, hop_length says 256
    with pytest.raises(ValueError, match="hop_length"):
        W.validate_hparams(hp)
    specs = {n: s for n, s, *_ in W.tensor_specs(W.multistream_hparams())}
    assert specs["dec.subband_conv_post.bias"] == (72,) and specs["dec.multistream_conv_post.weight"] == (1, 4, 63)


def test_ragged_limits_of_the_new_tails():
    """decoder_needs: the multi-stream tail has the multi-band tail's reach (same filter geometry), the single-band tail
    only the iSTFT's (ceil(n_fft / hop) + 2 columns); types outside 0..3 are refused."""
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.capi import VitsError, VitsLib

    lib = VitsLib()
    n0, n2 = lib.decoder_needs(W.default_hparams()), lib.decoder_needs(W.multistream_hparams())
    assert n0 == n2
    n3 = lib.decoder_needs(W.istft_hparams())
    assert n3["tail_cols"] == 16 // 4 + 2 and n3["post_out"] == n3["tail_cols"] + 1
    assert n3["tail_cols"] < n0["tail_cols"]
    hp = W.default_hparams()
    hp.dec_type = 5
    with pytest.raises(VitsError):
        lib.decoder_needs(hp)
