#!/usr/bin/env python3
"""Golden fixtures for voices whose n_heads is not 2, computed by the REFERENCE's own SynthesizerTrn on build-owned synthetic
weights.  Only the text encoder takes the config's n_heads (models.py:307-314); the pre_conv2 flow's pre-transformer is
attentions.Encoder(hidden, hidden, n_heads=2, ...) (models.py:352-360), so the two encoders run different head counts.  Needs the
reference tree (imported through oracle/refimport.py, which is used read-only), so it runs only where the reference exists:

    python tools/gen_golden_heads.py        # writes tests/golden/heads{3,4}_{b2,enc_T1,enc_T5,enc_T17}.npz

Weights are regenerated from (hparams, seed 1234) by vosk_tts_amd.weights on any machine; the files hold inputs and outputs only.
  heads<n>_b2        SynthesizerTrn.infer stage by stage up to the flow: ragged B=2, forced durations, injected noise
                     (text encoder -> logw -> regulated z_p -> flow z; the decoder does not depend on the heads)
  heads<n>_enc_T<T>  the text encoder alone at T = 1, 5, 17
Each file also records the names and shapes of the reference's relative-position tables (attn_names, attn_shapes).
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
VARIANTS = {"heads3": W.heads3_hparams, "heads4": W.heads4_hparams}


def save(name, **arrs):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrs)
    print(f"  {name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")


def reference_model(hp):
    """SynthesizerTrn with cfg["model"]["n_heads"] = hp.n_heads and the build-owned synthetic weights loaded (load_into_reference
    refuses any tensor whose shape differs from the reference's)."""
    cfg = refimport.ref_config()
    cfg["model"].update(hidden_channels=hp.hidden_channels, inter_channels=hp.inter_channels, filter_channels=hp.filter_channels,
                        n_heads=hp.n_heads, n_layers=hp.n_layers, gin_channels=hp.gin_channels,
                        upsample_initial_channel=hp.dec_initial_channel)
    cfg["data"]["n_speakers"] = hp.n_speakers
    net = refimport.build_reference_model(n_vocab=hp.n_vocab, cfg=cfg)
    refimport.load_into_reference(net, W.make_synthetic_weights(hp, SEED))
    return net


def attention_tables(net):
    """(names, shapes) of the reference's emb_rel_k / emb_rel_v tensors, in state_dict order"""
    sd = net.state_dict()
    names = [k for k in sd if k.endswith((".emb_rel_k", ".emb_rel_v"))]
    return np.array(names), np.array([tuple(sd[k].shape) for k in names], np.int64)


def b2_case(name, net, hp, rng):
    names, shapes = attention_tables(net)
    B, Tx = 2, 16
    ids = rng.integers(1, hp.n_vocab, size=(B, Tx))
    lengths = np.array([16, 7])
    sid = np.array([4, 151])
    dur = rng.integers(0, 4, size=(B, Tx))
    dur[1, 0] = 0
    scales = [0.667, 1.0, 0.8]
    nd = rng.standard_normal((B, 2, Tx)).astype(np.float32)
    r = refimport.run_reference_stages(net, ids, lengths, sid, scales, nd,
                                       lambda s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)), forced_durations=dur)
    save(name, ids=ids.astype(np.int64), lengths=lengths.astype(np.int64), sid=sid.astype(np.int64), scales=np.asarray(scales, np.float32),
         noise_dp=nd, noise_prior=r["noise_prior"], forced_durations=dur.astype(np.int32), x=r["x"], m_p_tok=r["m_p_tok"],
         logs_p_tok=r["logs_p_tok"], logw=r["logw"][:, 0], y_lengths=r["y_lengths"].astype(np.int64), z_p=r["z_p"], z=r["z"],
         attn_names=names, attn_shapes=shapes)


def enc_case(name, net, hp, rng, T):
    names, shapes = attention_tables(net)
    ids = rng.integers(1, hp.n_vocab, size=(1, T))
    with torch.no_grad():
        g = net.emb_g(torch.tensor([3])).unsqueeze(-1)
        x, m_p, logs_p, _ = net.enc_p(torch.from_numpy(ids), torch.tensor([T]), g=g)
    save(name, ids=ids.astype(np.int64), lengths=np.array([T], np.int64), sid=np.array([3], np.int64), x=x.numpy(),
         m_p_tok=m_p.numpy(), logs_p_tok=logs_p.numpy(), attn_names=names, attn_shapes=shapes)


def main():
    if not refimport.have_reference():
        sys.exit("the reference tree is not present on this machine")
    os.makedirs(OUT, exist_ok=True)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    rng = np.random.default_rng(2026)
    for v, fn in VARIANTS.items():
        hp = fn()
        net = reference_model(hp)
        b2_case(f"{v}_b2", net, hp, rng)
        for T in (1, 5, 17):
            enc_case(f"{v}_enc_T{T}", net, hp, rng, T)


if __name__ == "__main__":
    main()
