#!/usr/bin/env python3
"""The ONNX importer (vosk_tts_amd/onnx_import.py) against REAL exports: the reference's own export procedures
(oracle/onnx_export_ref.py) run on build-owned synthetic weights, and the importers must give back byte-identical blobs.
TEST INFRASTRUCTURE, container-only (needs the reference):   python oracle/check_onnx_exports.py
tests/test_onnx_import.py checks the same renamings on files written by the minimal writer, which runs anywhere."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def check_vits_export():
    """The REAL exporter output, not a synthetic file: the reference SynthesizerTrn (tiny widths, synthetic weights) goes through
    training/vits2/onnx_export.py's procedure (oracle/onnx_export_ref.py), and the importer must give back the byte-identical
    VITSW001 blob.  What the exporter does to names (observed): spk_emb_linear.weight is folded into a transposed anonymous
    MatMul constant, dp.flows.0.logs into an anonymous -logs feeding Exp, and byte-identical tensors are de-duplicated behind
    Identity nodes - the second model below has untrained-style repeated tensors to exercise exactly that."""
    import gen_golden as G
    import onnx_export_ref as X

    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W

    hp = W.tiny_hparams()
    cfgm = {"upsample_rates": list(hp.up_rates)[:hp.n_ups], "resblock_dilation_sizes": [list(x)[:hp.n_resd] for x in hp.res_dilations][:hp.n_resk]}
    tens = W.make_synthetic_weights(hp, 77)
    dup = dict(tens)  # de-duplication: every LayerNorm gamma / beta identical, zero `post` convs, m == logs == 0
    for k in dup:
        if k.endswith(".gamma"):
            dup[k] = np.ones_like(dup[k])
        elif k.endswith(".beta") or ".post." in k or k in ("dp.flows.0.m", "dp.flows.0.logs"):
            dup[k] = np.zeros_like(dup[k])
    for case, t in (("distinct", tens), ("deduplicated", dup)):
        data = X.export_vits(G.ref_for(hp, t))
        g = oi.OnnxGraph(data)
        assert "enc_p.encoder.spk_emb_linear.weight" not in g.inits, "exporter behaviour changed: update the notes in OnnxGraph"
        if case == "deduplicated":
            assert len(g.alias) > 20
        hp2, got = oi.import_onnx(data, cfgm)
        assert W.pack_blob(hp2, got) == W.pack_blob(hp, t), case


def check_stts_and_bert_exports():
    """matcha/onnx/export.py's MatchaWithVocoder (reference MatchaTTS + in-tree HiFi-GAN V1, synthetic weights) and
    bert-export.py's BertModel -> real torch.onnx exports -> importers -> byte-identical STTSW001 / VITSW001 / BERTW001 blobs,
    every hyper-parameter (incl. n_timesteps, guidance scale, mel statistics read off the traced graph) recovered."""
    import torch

    import onnx_export_ref as X

    BertConfig, BertModel = X.transformers_bert()
    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W
    from vosk_tts_amd import weights_bert as BW
    from vosk_tts_amd import weights_stts as S

    hp = BW.small_hparams(120, 128, 4)
    cfg = BertConfig(vocab_size=hp.vocab_size, hidden_size=hp.hidden, num_hidden_layers=hp.n_layers, num_attention_heads=hp.n_heads,
                     intermediate_size=hp.intermediate, max_position_embeddings=hp.max_position, type_vocab_size=hp.type_vocab,
                     layer_norm_eps=hp.ln_eps, hidden_act="gelu", attn_implementation="eager")
    net = BertModel(cfg).eval()
    tens = BW.make_synthetic_weights(hp, 31)
    sd = net.state_dict()
    with torch.no_grad():
        for k, v in tens.items():
            sd[k].copy_(torch.from_numpy(v))
    hp2, got = oi.import_bert_onnx(X.export_bert(net), {"n_heads": hp.n_heads})
    assert BW.pack_blob(hp2, got) == BW.pack_blob(hp, tens)

    import gen_golden_stts as G

    shp, snet, voc = G.build()  # reference MatchaTTS + HiFi-GAN V1 carrying the synthetic blobs' tensors
    voc.decode = voc.forward   # export.py:30 calls vocoder.decode(): Vocos' method; the in-tree generator is called directly (cli.py)
    data = X.export_stts(snet, voc, n_timesteps=3)
    hp3, t3, v3 = oi.import_stts_onnx(data)
    shp.n_timesteps = 3
    assert S.pack_blob(hp3, t3) == S.pack_blob(shp, S.make_synthetic_weights(shp, G.SEED))
    vhp = W.hifigan_v1_vocoder_hparams()
    assert W.pack_blob(*v3) == W.pack_blob(vhp, W.make_synthetic_weights(vhp, G.SEED))
    # a foreign embedded vocoder is reported, not guessed
    g = oi.OnnxGraph(data)
    foreign = {("vocoder.backbone." + k[len("vocoder."):] if k.startswith("vocoder.") else k): v for k, v in g.inits.items() if v.dtype == np.float32 and v.size > 1}
    with pytest.raises(NotImplementedError, match="Vocos"):
        oi.import_stts_onnx(oi.write_minimal_onnx(os.path.join(os.environ.get("TMPDIR", "/tmp"), "foreign_voc.onnx"), foreign))


if __name__ == "__main__":
    check_vits_export()
    check_stts_and_bert_exports()
    print("ONNX exports import bit-exactly")
