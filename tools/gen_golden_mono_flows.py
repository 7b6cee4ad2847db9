#!/usr/bin/env python3
"""Golden fixtures for the two mono_layer_* flows (flow_type 4 = mono_layer_inter_residual, 5 = mono_layer_post_residual:
[ResidualCouplingLayer, Flip, MonoTransformerFlowLayer] per flow, models.py:696-734, 545-627), computed by the REFERENCE's own
SynthesizerTrn on build-owned synthetic weights.  Needs the reference tree (imported through oracle/refimport.py, which is used
read-only), so it runs only where the reference exists:

    python tools/gen_golden_mono_flows.py    # writes tests/golden/flow_mono{inter,post}_{tiny_b3,default_b2,e2e_b3}.npz

Weights are regenerated from (hparams, seed 1234) by vosk_tts_amd.weights on any machine; the files hold inputs and outputs only,
with the contents and shapes of tools/gen_golden_flow_types.py's flow_{preconv,plain}_* files:
  flow_<kind>_tiny_b3     flow reverse (models.py:750-757) alone, tiny size, ragged B=3: z_p, y_lengths, sid, z
  flow_<kind>_default_b2  the same at the default size (mono layer: head dim 48), ragged B=2
  flow_<kind>_e2e_b3      SynthesizerTrn.infer stage by stage: ragged B=3, forced durations, injected noise
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

import refimport  # noqa: E402
import gen_golden_flow_types as base  # noqa: E402  (flow_case / e2e_case: the same cases, shapes and file contents)
from vosk_tts_amd import weights as W  # noqa: E402

SEED = 1234
# mono_layer_inter_residual is built only with transformer flows on; mono_layer_post_residual is the OUTER elif (models.py:715), taken
# with them off -- the reference's own defaults (models.py:1560-1561)
CONFIG = {4: dict(use_transformer_flows=True, transformer_flow_type="mono_layer_inter_residual"),
          5: dict(use_transformer_flows=False, transformer_flow_type="mono_layer_post_residual")}
NAME = {4: "monointer", 5: "monopost"}
# The e2e files are mostly audio, 256 samples per drawn frame.  Seeds whose forced durations sum to 35 frames over the three items (the
# flow_preconv_e2e_b3 case drew 38) keep each file below its flow_preconv_* counterpart; nothing else about them was looked at.
E2E_SEED = {4: 4017, 5: 4028}


def reference_model(hp):
    """SynthesizerTrn with the mono_layer_* flow of hp.flow_type and the build-owned synthetic weights loaded (a nonzero `post` in
    the mono layers, unlike the reference's zero init).  ResidualCouplingTransformersBlock.remove_weight_norm (models.py:759-762)
    walks flows[::2], which on these lists of three hits Flips and mono layers and fails: the weight norm is removed from the decoder
    and from each coupling layer's WN (flows[::3].enc) directly."""
    tens = W.make_synthetic_weights(hp, SEED)
    cfg = refimport.ref_config()
    cfg["model"].update(hidden_channels=hp.hidden_channels, inter_channels=hp.inter_channels, filter_channels=hp.filter_channels,
                        n_layers=hp.n_layers, gin_channels=hp.gin_channels, upsample_initial_channel=hp.dec_initial_channel,
                        **CONFIG[hp.flow_type])
    cfg["data"]["n_speakers"] = hp.n_speakers
    models = refimport.ref_modules()["models"]
    with contextlib.redirect_stdout(io.StringIO()):
        net = models.SynthesizerTrn(hp.n_vocab, 80, cfg["train"]["segment_size"] // cfg["data"]["hop_length"],
                                    n_speakers=cfg["data"]["n_speakers"], is_onnx=True, **cfg["model"])
        net.eval()
        with torch.no_grad():
            net.dec.remove_weight_norm()
            for layer in net.flow.flows[::3]:
                layer.enc.remove_weight_norm()
    assert len(net.flow.flows) == 3 * hp.flow_n_flows
    refimport.load_into_reference(net, tens)
    return net


def main():
    if not refimport.have_reference():
        sys.exit("the reference tree is not present on this machine")
    os.makedirs(base.OUT, exist_ok=True)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    rng = np.random.default_rng(2026)
    base.reference_model = reference_model  # flow_case / e2e_case build their model through the module's name
    for ft, tiny, default in ((4, W.tiny_mono_inter_hparams, W.mono_inter_hparams), (5, W.tiny_mono_post_hparams, W.mono_post_hparams)):
        base.flow_case(f"flow_{NAME[ft]}_tiny_b3", tiny(), rng, [70, 1, 33], [1, 4, 2])
        base.flow_case(f"flow_{NAME[ft]}_default_b2", default(), rng, [36, 17], [5, 190])
        base.e2e_case(f"flow_{NAME[ft]}_e2e_b3", tiny(), np.random.default_rng(E2E_SEED[ft]))


if __name__ == "__main__":
    main()
