#!/usr/bin/env python3
"""Decoder-stage kernels of one decoder type at T_y = 150, B = 1 and B = 32 (default sizes, synthetic weights), for a
kernel-trace profiler run per type:

    rocprofv3 --kernel-trace --stats -d OUT -o dec0 -- python tools/decoder_tail_profile.py 0      # 0, 2 or 3

Each batch size runs `--iters` decoder stages after two warm-up calls; the profiler's per-kernel stats then give the
per-call kernel times (divide by the call count printed here)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (one HIP runtime per process: torch's, loaded before the product library)

from vosk_tts_amd import weights as W  # noqa: E402
from vosk_tts_amd.capi import VitsLib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dec_type", type=int, choices=(0, 2, 3))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--ty", type=int, default=150)
    a = ap.parse_args()
    hp = {0: W.default_hparams, 2: W.multistream_hparams, 3: W.istft_hparams}[a.dec_type]()
    model = VitsLib().create(W.synthetic_blob(hp, 1234), 0)
    rng = np.random.default_rng(0)
    for B in (1, 32):
        z = rng.standard_normal((B, hp.inter_channels, a.ty)).astype(np.float32)
        for _ in range(2):
            model.decoder(z, want_mb=False)
        for _ in range(a.iters):
            audio, _ = model.decoder(z, want_mb=False)
        assert np.isfinite(audio).all()
        print(f"dec_type {a.dec_type}: B={B} T_y={a.ty}: {a.iters + 2} decoder calls")
    model.close()


if __name__ == "__main__":
    main()
