#!/usr/bin/env python3
"""Golden fixtures for the `pre_conv` (flow_type 1, ResidualCouplingTransformersLayer, models.py:399-483) and plain
(flow_type 2, modules.ResidualCouplingLayer, modules.py:298-345) flows, computed by the REFERENCE's own SynthesizerTrn on
build-owned synthetic weights.  Needs the reference tree (imported through oracle/refimport.py, which is used read-only), so it
runs only where the reference exists:

    python tools/gen_golden_flow_types.py        # writes tests/golden/flow_{preconv,plain}_{tiny_b3,default_b2,e2e_b3}.npz

Weights are regenerated from (hparams, seed 1234) by vosk_tts_amd.weights on any machine; the files hold inputs and outputs only.
  flow_<kind>_tiny_b3     flow reverse (models.py:750-757) alone, tiny size, ragged B=3: z_p, y_lengths, sid, z
  flow_<kind>_default_b2  the same at the default size (pre_conv: head dim 48), ragged B=2
  flow_<kind>_e2e_b3      SynthesizerTrn.infer stage by stage: ragged B=3, forced durations, injected noise
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)

import refimport  # noqa: E402
from vosk_tts_amd import weights as W  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SEED = 1234
CONFIG = {1: dict(use_transformer_flows=True, transformer_flow_type="pre_conv"),
          2: dict(use_transformer_flows=False, transformer_flow_type="plain")}  # (any type but mono_layer_post_residual, models.py:731)
NAME = {1: "preconv", 2: "plain"}


def save(name, **arrs):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrs)
    print(f"  {name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")


def reference_model(hp):
    """SynthesizerTrn with the flow of hp.flow_type and the build-owned synthetic weights loaded."""
    tens = W.make_synthetic_weights(hp, SEED)
    cfg = refimport.ref_config()
    mc = cfg["model"]
    mc.update(hidden_channels=hp.hidden_channels, inter_channels=hp.inter_channels, filter_channels=hp.filter_channels,
              n_layers=hp.n_layers, gin_channels=hp.gin_channels, upsample_initial_channel=hp.dec_initial_channel, **CONFIG[hp.flow_type])
    cfg["data"]["n_speakers"] = hp.n_speakers
    if hp.flow_type == 2:
        # modules.ResidualCouplingLayer has no remove_weight_norm (ResidualCouplingTransformersBlock.remove_weight_norm, models.py:759-762,
        # calls it and fails, so onnx_export.py cannot export this flow unmodified): build as build_reference_model does, removing the
        # weight norm from each layer's WN directly, as an export of such a voice has to
        import contextlib
        import io

        models = refimport.ref_modules()["models"]
        with contextlib.redirect_stdout(io.StringIO()):
            net = models.SynthesizerTrn(hp.n_vocab, 80, cfg["train"]["segment_size"] // cfg["data"]["hop_length"],
                                        n_speakers=cfg["data"]["n_speakers"], is_onnx=True, **cfg["model"])
            net.eval()
            with torch.no_grad():
                net.dec.remove_weight_norm()
                for layer in net.flow.flows[::2]:
                    layer.enc.remove_weight_norm()
    else:
        net = refimport.build_reference_model(n_vocab=hp.n_vocab, cfg=cfg)
    feed = dict(tens)
    sd = net.state_dict()
    # pre_conv's post_transformer (models.py:436-444) is never executed and not in the blob: load_into_reference only checks coverage
    for k in sd:
        if ".post_transformer." in k:
            feed[k] = sd[k].numpy().copy()
    refimport.load_into_reference(net, feed)
    return net


def flow_case(name, hp, rng, lengths, sid):
    net = reference_model(hp)
    B, Ty = len(lengths), int(max(lengths))
    z_p = rng.standard_normal((B, hp.inter_channels, Ty)).astype(np.float32)
    with torch.no_grad():
        mask = (torch.arange(Ty)[None, :] < torch.as_tensor(lengths)[:, None]).float().unsqueeze(1)
        g = net.emb_g(torch.as_tensor(sid)).unsqueeze(-1)
        z = net.flow(torch.from_numpy(z_p), mask, g=g, reverse=True).numpy()
    save(name, z_p=z_p, y_lengths=np.asarray(lengths, np.int64), sid=np.asarray(sid, np.int64), z=z)


def e2e_case(name, hp, rng):
    net = reference_model(hp)
    B, Tx = 3, 14
    ids = rng.integers(1, hp.n_vocab, size=(B, Tx))
    lengths = np.array([14, 5, 9])
    sid = np.array([0, 3, 1])
    dur = rng.integers(0, 4, size=(B, Tx))
    dur[1, 0] = 0
    scales = [0.667, 1.0, 0.8]
    nd = rng.standard_normal((B, 2, Tx)).astype(np.float32)
    r = refimport.run_reference_stages(net, ids, lengths, sid, scales, nd,
                                       lambda s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)), forced_durations=dur)
    save(name, ids=ids.astype(np.int64), lengths=lengths.astype(np.int64), sid=sid.astype(np.int64), scales=np.asarray(scales, np.float32),
         noise_dp=nd, noise_prior=r["noise_prior"], forced_durations=dur.astype(np.int32), y_lengths=r["y_lengths"].astype(np.int64),
         z=r["z"], audio=r["audio"][:, 0])


def main():
    if not refimport.have_reference():
        sys.exit("the reference tree is not present on this machine")
    os.makedirs(OUT, exist_ok=True)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    rng = np.random.default_rng(2025)
    for ft, tiny, default in ((1, W.tiny_pre_conv_hparams, W.pre_conv_hparams), (2, W.tiny_plain_flow_hparams, W.plain_flow_hparams)):
        flow_case(f"flow_{NAME[ft]}_tiny_b3", tiny(), rng, [70, 1, 33], [1, 4, 2])
        flow_case(f"flow_{NAME[ft]}_default_b2", default(), rng, [36, 17], [5, 190])
        e2e_case(f"flow_{NAME[ft]}_e2e_b3", tiny(), rng)


if __name__ == "__main__":
    main()
