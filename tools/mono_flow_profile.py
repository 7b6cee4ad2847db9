#!/usr/bin/env python3
"""Flow-stage and whole-forward time of the mono_layer_* flows (flow_type 4, 5) next to types 1 (pre_conv) and 2 (plain), default
size, through vits_stage_flow and vits_synthesize:

    python tools/mono_flow_profile.py [--types 1 2 4 5] [--reps 30]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/mono_flow_profile.py --types 4 5 --reps 10    # kernel times

Shapes: c2 = one utterance of 50 tokens x 3 frames = T_y 150 (the c2 workload's frame count); b32 = 32 ragged items of 20..200
tokens x 3 frames (T_y 60..600, seeded).  Durations are forced, noise comes from a seed.  Prints one line per (type, shape):
median wall time of the flow-stage call (it includes the host copies of z_p in and z out: 2 * B * 192 * T_y * 4 bytes) and of the
whole forward (ids in, audio out)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vosk_tts_amd import weights as W  # noqa: E402
from vosk_tts_amd.capi import VitsLib  # noqa: E402

HP = {0: W.default_hparams, 1: W.pre_conv_hparams, 2: W.plain_flow_hparams, 4: W.mono_inter_hparams, 5: W.mono_post_hparams}
FRAMES_PER_TOKEN = 3


def tokens(name):
    if name == "c2":
        return np.array([50], np.int64)
    return np.random.default_rng(7).integers(20, 201, size=32).astype(np.int64)


def median_ms(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * np.median(ts), 1e3 * min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", type=int, nargs="+", default=[1, 2, 4, 5])
    ap.add_argument("--shapes", nargs="+", default=["c2", "b32"])
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    lib = VitsLib()
    for ft in args.types:
        hp = HP[ft]()
        m = lib.create(W.synthetic_blob(hp, 1234), 0)
        try:
            for sh in args.shapes:
                lx = tokens(sh)
                B, Tx = len(lx), int(lx.max())
                ly = lx * FRAMES_PER_TOKEN
                Ty = int(ly.max())
                rng = np.random.default_rng(1)
                z_p = rng.standard_normal((B, hp.inter_channels, Ty)).astype(np.float32)
                ids = rng.integers(1, hp.n_vocab, size=(B, Tx)).astype(np.int64)
                dur = np.full((B, Tx), FRAMES_PER_TOKEN, np.int32)
                sid = (np.arange(B) % hp.n_speakers).astype(np.int64)
                fl, fl_min = median_ms(lambda: m.flow(z_p, ly, sid), args.reps)
                fw, fw_min = median_ms(lambda: m.synthesize(ids, lx, [0.667, 1.0, 0.8], sid, forced_durations=dur, seed=3), args.reps)
                print(f"flow_type {ft} shape {sh:3s} B {B:2d} T_y max {Ty:4d} sum {int(ly.sum()):6d}: flow stage median {fl:7.3f} ms "
                      f"(min {fl_min:7.3f})  whole forward median {fw:7.3f} ms (min {fw_min:7.3f})  {args.reps} calls each", flush=True)
        finally:
            m.close()


if __name__ == "__main__":
    main()
