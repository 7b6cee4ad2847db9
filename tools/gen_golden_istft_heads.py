#!/usr/bin/env python3
"""Golden fixtures for the multi-stream (dec_type 2) and single-band (dec_type 3) iSTFT decoders, computed by the
REFERENCE's own PyTorch modules on build-owned synthetic weights.  Needs the reference tree (imported through
oracle/refimport.py, which is used read-only), so it runs only where the reference exists:

    python tools/gen_golden_istft_heads.py        # writes tests/golden/{ms,istft}_{dec_b2,e2e_b3}.npz

Cases (tiny sizes, weights regenerated from (hparams, seed 1234) by vosk_tts_amd.weights on any machine)
  ms_dec_b2     Multistream_iSTFT_Generator alone (models.py:1066-1163), B=2: z, audio, y_mb_hat (the zero-stuffed
                sub-band signal [B, S, T_m * S]: S times the engine's audio_mb on every S-th sample, 0 elsewhere)
  istft_dec_b2  iSTFT_Generator alone (models.py:901-971), ups [8,8], n_fft 16, hop 4, B=2: z, audio
  ms_e2e_b3     SynthesizerTrn with ms_istft_vits set: ragged B=3, forced durations, injected noise
  istft_e2e_b3  SynthesizerTrn with istft_vits set, the same kind of batch
"""
import contextlib
import io
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


def save(name, **arrs):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrs)
    print(f"  {name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")


def decoder_module(hp):
    models = refimport.ref_modules()["models"]
    ups = [hp.up_rates[i] for i in range(hp.n_ups)]
    kers = [hp.up_kernels[i] for i in range(hp.n_ups)]
    rk = [hp.res_kernels[j] for j in range(hp.n_resk)]
    rd = [[hp.res_dilations[j][d] for d in range(hp.n_resd)] for j in range(hp.n_resk)]
    with contextlib.redirect_stdout(io.StringIO()):
        if hp.dec_type == 2:
            dec = models.Multistream_iSTFT_Generator(hp.inter_channels, "1", rk, rd, ups, hp.dec_initial_channel, kers, hp.istft_n_fft,
                                                     hp.istft_hop, hp.subbands, gin_channels=hp.gin_channels, is_onnx=True)
        else:
            dec = models.iSTFT_Generator(hp.inter_channels, "1", rk, rd, ups, hp.dec_initial_channel, kers, hp.istft_n_fft,
                                         hp.istft_hop, gin_channels=hp.gin_channels, is_onnx=True)
        dec.eval()
        dec.remove_weight_norm()
    return dec


def load_decoder(dec, tens):
    sd = dec.state_dict()
    ours = {k[4:]: v for k, v in tens.items() if k.startswith("dec.")}
    # buffers of the module that are not weights: the STFT bases and the multi-stream zero-stuffing filter
    left = sorted(k for k in sd if k not in ours and not k.startswith("stft.") and k != "updown_filter")
    assert not left, left
    with torch.no_grad():
        for k, v in ours.items():
            assert tuple(sd[k].shape) == v.shape, (k, sd[k].shape, v.shape)
            sd[k].copy_(torch.from_numpy(v))


def decoder_case(name, hp, rng):
    tens = W.make_synthetic_weights(hp, SEED)
    dec = decoder_module(hp)
    load_decoder(dec, tens)
    z = rng.standard_normal((2, hp.inter_channels, 12)).astype(np.float32)
    with torch.no_grad():
        o, o_mb = dec(torch.from_numpy(z))
    arrs = dict(z=z, audio=o.numpy()[:, 0])
    if o_mb is not None:
        S = hp.subbands
        ymb = o_mb.numpy()
        arrs["y_mb_hat"] = ymb
        assert np.all(ymb.reshape(ymb.shape[0], S, -1, S)[..., 1:] == 0)  # zero-stuffed: only every S-th sample is set
    save(name, **arrs)


def e2e_case(name, hp, rng):
    tens = W.make_synthetic_weights(hp, SEED)
    cfg = refimport.ref_config()
    mc = cfg["model"]
    mc.update(hidden_channels=hp.hidden_channels, inter_channels=hp.inter_channels, filter_channels=hp.filter_channels,
              n_layers=hp.n_layers, gin_channels=hp.gin_channels, upsample_initial_channel=hp.dec_initial_channel,
              upsample_rates=[hp.up_rates[i] for i in range(hp.n_ups)], upsample_kernel_sizes=[hp.up_kernels[i] for i in range(hp.n_ups)],
              gen_istft_n_fft=hp.istft_n_fft, gen_istft_hop_size=hp.istft_hop, subbands=hp.subbands,
              mb_istft_vits=False, ms_istft_vits=hp.dec_type == 2, istft_vits=hp.dec_type == 3)
    cfg["data"]["n_speakers"] = hp.n_speakers
    net = refimport.build_reference_model(n_vocab=hp.n_vocab, cfg=cfg)
    feed = dict(tens)
    if hp.dec_type == 2:  # a constant buffer of the module, not a weight: load_into_reference only checks it is covered
        feed["dec.updown_filter"] = net.state_dict()["dec.updown_filter"].numpy().copy()
    refimport.load_into_reference(net, feed)
    if hp.dec_type == 3:  # iSTFT_Generator returns (audio, None); run_reference_stages reads the second output as an array
        fwd = net.dec.forward
        net.dec.forward = lambda x, g=None: (fwd(x, g)[0], torch.zeros(0))
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
    rng = np.random.default_rng(2024)
    decoder_case("ms_dec_b2", W.tiny_multistream_hparams(), rng)
    decoder_case("istft_dec_b2", W.tiny_istft_hparams(), rng)
    e2e_case("ms_e2e_b3", W.tiny_multistream_hparams(), rng)
    e2e_case("istft_e2e_b3", W.tiny_istft_hparams(), rng)


if __name__ == "__main__":
    main()
