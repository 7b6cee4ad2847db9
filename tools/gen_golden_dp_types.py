#!/usr/bin/env python3
"""Golden fixtures for the deterministic duration predictor (use_sdp false: DurationPredictor, models.py:104-139), computed by the
REFERENCE's own SynthesizerTrn(use_sdp=False) on build-owned synthetic weights.  Needs the reference tree (imported through
oracle/refimport.py, which is used read-only), so it runs only where the reference exists:

    python tools/gen_golden_dp_types.py        # writes tests/golden/dp_det_{tiny_b3,default_b2,e2e_b3}.npz

Weights are regenerated from (hparams, seed 1234) by vosk_tts_amd.weights on any machine; the files hold inputs and outputs only.
  dp_det_tiny_b3     DurationPredictor.forward alone, tiny size, ragged B=3: x, lengths, sid, logw
  dp_det_default_b2  the same at the default size, ragged B=2
  dp_det_e2e_b3      SynthesizerTrn.infer stage by stage, ragged B=3: forced durations with injected prior noise (audio), and
                     free-running (logw, the durations w_ceil and y_lengths)
Every free-running w * length_scale on a valid token is at least 1e-3 from an integer (asserted; the seed is stepped until it holds),
so an fp32 ceil on the device cannot land on the other side.
"""
import contextlib
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)

import refimport  # noqa: E402
from vosk_tts_amd import weights as W  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SEED = 1234
CONFIG = dict(use_sdp=False)
CEIL_MARGIN = 1e-3


def save(name, **arrs):
    """np.savez_compressed with a fixed member timestamp: a rerun writes the same bytes"""
    path = os.path.join(OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrs[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(f"  {name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")


def reference_model(hp):
    """SynthesizerTrn(use_sdp=False) as the exporter builds it, with the build-owned synthetic weights loaded."""
    assert hp.dp_n_flows == 0
    tens = W.make_synthetic_weights(hp, SEED)
    cfg = refimport.ref_config()
    mc = cfg["model"]
    mc.update(hidden_channels=hp.hidden_channels, inter_channels=hp.inter_channels, filter_channels=hp.filter_channels,
              n_layers=hp.n_layers, gin_channels=hp.gin_channels, upsample_initial_channel=hp.dec_initial_channel, **CONFIG)
    cfg["data"]["n_speakers"] = hp.n_speakers
    with contextlib.redirect_stdout(io.StringIO()):
        net = refimport.build_reference_model(n_vocab=hp.n_vocab, cfg=cfg)
    refimport.load_into_reference(net, tens)
    return net


class _DpShim(torch.nn.Module):
    """run_reference_stages calls net.dp(x, x_mask, g=g, reverse=True, noise_scale=...) (the stochastic signature); the deterministic
    predictor takes (x, x_mask, g) and draws no noise (models.py:1685-1688)"""

    def __init__(self, dp):
        super().__init__()
        self.dp = dp

    def forward(self, x, x_mask, g=None, reverse=True, noise_scale=1.0):
        return self.dp(x, x_mask, g=g)


def dp_case(name, hp, rng, lengths, sid):
    net = reference_model(hp)
    B, Tx = len(lengths), int(max(lengths))
    x = rng.standard_normal((B, hp.hidden_channels, Tx)).astype(np.float32)
    with torch.no_grad():
        mask = (torch.arange(Tx)[None, :] < torch.as_tensor(lengths)[:, None]).float().unsqueeze(1)
        g = net.emb_g(torch.as_tensor(sid)).unsqueeze(-1)
        logw = net.dp(torch.from_numpy(x), mask, g=g)[:, 0].numpy()
    save(name, x=x, lengths=np.asarray(lengths, np.int64), sid=np.asarray(sid, np.int64), logw=logw)


def _margin(w, lengths):
    return min(float(np.min(np.abs(w[b, :n] - np.round(w[b, :n])))) for b, n in enumerate(lengths))


def e2e_case(name, hp, seed):
    net = reference_model(hp)
    net.dp = _DpShim(net.dp)
    B, Tx = 3, 14
    lengths = np.array([14, 5, 9])
    sid = np.array([0, 3, 1])
    scales = [0.667, 1.0, 0.8]
    nd = np.zeros((B, 2, Tx), np.float32)  # (not read by the deterministic predictor)
    for s in range(seed, seed + 1000):
        rng = np.random.default_rng(s)
        ids = rng.integers(1, hp.n_vocab, size=(B, Tx))
        free = refimport.run_reference_stages(net, ids, lengths, sid, scales, nd,
                                              lambda sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32)))
        w = np.exp(free["logw"][:, 0]) * scales[1]
        if _margin(w, lengths) >= CEIL_MARGIN:
            break
    else:
        raise RuntimeError("no seed with every w * length_scale away from an integer")
    print(f"  {name}: seed {s}, ceil margin {_margin(w, lengths):.2e}, free-running durations {free['durations'].min()}.."
          f"{free['durations'].max()}, y_lengths {free['y_lengths'].tolist()}")
    dur = rng.integers(0, 4, size=(B, Tx))
    dur[1, 0] = 0
    r = refimport.run_reference_stages(net, ids, lengths, sid, scales, nd,
                                       lambda sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32)), forced_durations=dur)
    save(name, ids=ids.astype(np.int64), lengths=lengths.astype(np.int64), sid=sid.astype(np.int64), scales=np.asarray(scales, np.float32),
         noise_prior=r["noise_prior"], forced_durations=dur.astype(np.int32), y_lengths=r["y_lengths"].astype(np.int64), audio=r["audio"][:, 0],
         logw=free["logw"][:, 0], durations_free=free["durations"].astype(np.int32), y_lengths_free=free["y_lengths"].astype(np.int64))


def main():
    if not refimport.have_reference():
        sys.exit("the reference tree is not present on this machine")
    os.makedirs(OUT, exist_ok=True)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    rng = np.random.default_rng(2026)
    dp_case("dp_det_tiny_b3", W.tiny_deterministic_dp_hparams(), rng, [70, 1, 33], [1, 4, 2])
    dp_case("dp_det_default_b2", W.deterministic_dp_hparams(), rng, [36, 17], [5, 190])
    e2e_case("dp_det_e2e_b3", W.tiny_deterministic_dp_hparams(), 7)


if __name__ == "__main__":
    main()
