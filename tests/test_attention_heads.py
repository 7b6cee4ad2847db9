"""Voices whose n_heads is not 2: only the text encoder takes the config's n_heads (models.py:307-314); the pre_conv2 flow's
pre-transformer is attentions.Encoder(hidden, hidden, n_heads=2, ...) (models.py:352-360).  The CPU oracle and the synthetic weight
inventory are pinned to fixtures computed by the reference's own SynthesizerTrn (tools/gen_golden_heads.py).  CPU-only."""
import numpy as np
import pytest

from conftest import assert_close, golden

TOL = 2e-5  # as tests/test_oracle_golden.py: fp32 restatement vs PyTorch-CPU fp32
VARIANTS = ("heads3", "heads4")


def _hp(v):
    from vosk_tts_amd import weights as W

    return {"heads3": W.heads3_hparams, "heads4": W.heads4_hparams}[v]()


@pytest.fixture(scope="module")
def oracles(oracle_lib):
    from vosk_tts_amd import weights as W

    ms = {v: oracle_lib.create(W.synthetic_blob(_hp(v), 1234)) for v in VARIANTS}
    yield ms
    for m in ms.values():
        m.close()


@pytest.mark.parametrize("v", VARIANTS)
def test_oracle_stages_match_the_reference(oracles, v):
    """text encoder -> logw -> regulated z_p -> flow z of a ragged B=2 batch"""
    g = golden(f"{v}_b2")
    m = oracles[v]
    ids, lengths, sid, scales = g["ids"], g["lengths"], g["sid"], g["scales"]
    x, m_p, logs_p = m.text_encoder(ids, lengths, sid)
    assert_close("x", g["x"], x, TOL)
    assert_close("m_p", g["m_p_tok"], m_p, TOL)
    assert_close("logs_p", g["logs_p_tok"], logs_p, TOL)
    logw = m.duration(g["x"], lengths, sid, g["noise_dp"], float(scales[2]))
    assert_close("logw", g["logw"], logw, 5 * TOL)
    Ty = int(g["y_lengths"].max())
    _, ylen, z_p = m.regulate(None, g["forced_durations"], lengths, float(scales[1]), g["m_p_tok"], g["logs_p_tok"], g["noise_prior"],
                              float(scales[0]), Ty)
    assert np.array_equal(ylen, g["y_lengths"])
    assert_close("z_p", g["z_p"], z_p, TOL)
    z = m.flow(g["z_p"], g["y_lengths"], sid)
    for b, n in enumerate(g["y_lengths"]):
        assert_close(f"z[{b}]", g["z"][b, :, :n], z[b, :, :n], TOL)


@pytest.mark.parametrize("T", [1, 5, 17])
@pytest.mark.parametrize("v", VARIANTS)
def test_oracle_text_encoder_matches_the_reference(oracles, v, T):
    g = golden(f"{v}_enc_T{T}")
    x, m_p, logs_p = oracles[v].text_encoder(g["ids"], g["lengths"], g["sid"])
    assert_close("x", g["x"], x, TOL)
    assert_close("m_p", g["m_p_tok"], m_p, TOL)
    assert_close("logs_p", g["logs_p_tok"], logs_p, TOL)


@pytest.mark.parametrize("v", VARIANTS)
def test_synthetic_tables_have_the_reference_shapes(v):
    from vosk_tts_amd import weights as W

    hp = _hp(v)
    g = golden(f"{v}_b2")
    tens = W.make_synthetic_weights(hp, 1)
    names = [str(n) for n in g["attn_names"]]
    assert {k for k in tens if k.endswith((".emb_rel_k", ".emb_rel_v"))} == set(names)
    for n, shape in zip(names, g["attn_shapes"]):
        assert tens[n].shape == tuple(int(d) for d in shape), n
    # the text encoder at n_heads, every flow pre-transformer at 2 heads, both at the same window
    nw = 2 * hp.window_size + 1
    assert tens["enc_p.encoder.attn_layers.0.emb_rel_k"].shape == (1, nw, hp.hidden_channels // hp.n_heads)
    assert tens["flow.flows.6.pre_transformer.attn_layers.0.emb_rel_v"].shape == (1, nw, hp.hidden_channels // 2)


def test_importer_keeps_the_flow_at_two_heads(tmp_path):
    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W

    hp = W.heads3_hparams()
    tens = W.make_synthetic_weights(hp, 7)
    path = oi.write_minimal_onnx(str(tmp_path / "m.onnx"), tens)
    got_hp, got = oi.import_onnx(path)
    assert got_hp.n_heads == 3 and got_hp.window_size == hp.window_size and got_hp.flow_type == 0
    assert set(got) == set(tens) and all(np.array_equal(got[k], tens[k]) for k in tens)
    assert got["flow.flows.2.pre_transformer.attn_layers.0.emb_rel_k"].shape == (1, 9, 96)
    blob = str(tmp_path / "m.vitsw")
    oi.convert(path, blob)
    hp2, t2 = W.unpack_blob(open(blob, "rb").read())
    assert hp2.n_heads == 3 and t2["flow.flows.0.pre_transformer.attn_layers.0.emb_rel_v"].shape == (1, 9, 96)
    # a flow table laid out for n_heads (what the reference never writes) is refused, naming the tensor
    bad = dict(tens)
    name = "flow.flows.4.pre_transformer.attn_layers.0.emb_rel_k"
    bad[name] = np.zeros((1, 9, 64), np.float32)
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        oi.import_onnx(oi.write_minimal_onnx(str(tmp_path / "bad.onnx"), bad))


def test_oracle_refuses_a_flow_table_laid_out_for_n_heads(oracle_lib):
    from vosk_tts_amd import weights as W

    hp = W.heads3_hparams()
    tens = W.make_synthetic_weights(hp, 7)
    for k in list(tens):
        if k.startswith("flow.") and k.endswith((".emb_rel_k", ".emb_rel_v")):
            tens[k] = np.zeros((1, 9, 64), np.float32)
    m = oracle_lib.create(W.pack_blob(hp, tens))
    z_p = np.zeros((1, hp.inter_channels, 4), np.float32)
    with pytest.raises(Exception, match="emb_rel"):
        m.flow(z_p, [4], [0])
