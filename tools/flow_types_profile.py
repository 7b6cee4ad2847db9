#!/usr/bin/env python3
"""Flow-stage time of each flow type (0 pre_conv2, 1 pre_conv, 2 plain) at the default size, through vits_stage_flow:

    python tools/flow_types_profile.py --types 0 1 2 --shapes c2 c3 long [--reps 20]

Shapes: c2 = one utterance of T_y 150 (the c2 workload's frame count), c3 = 32 ragged items (T_y 60..600, seeded),
long = one utterance of T_y 6000.  Prints one line per (type, shape): median wall time of the stage call (it includes the host
copies of z_p in and z out: 2 * B * 192 * T_y * 4 bytes), and the attention FLOPs on valid frames (4 * C * len^2 per layer) that a
kernel-trace run (rocprofv3 --kernel-trace --stats -- python tools/flow_types_profile.py ...) turns into a rate."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vosk_tts_amd import weights as W  # noqa: E402
from vosk_tts_amd.capi import VitsLib  # noqa: E402

HP = {0: W.default_hparams, 1: W.pre_conv_hparams, 2: W.plain_flow_hparams}


def shape(name):
    rng = np.random.default_rng(7)
    if name == "c2":
        return np.array([150], np.int64)
    if name == "c3":
        return rng.integers(60, 601, size=32).astype(np.int64)
    return np.array([6000], np.int64)


def attention_flops(hp, lengths):
    """4 * C * len^2 per attention layer on valid frames: pre_conv2 1 layer at H, pre_conv 2 layers at I/2, plain none"""
    n2 = float(np.sum(lengths.astype(np.float64) ** 2))
    if hp.flow_type == 0:
        return hp.flow_n_flows * 4.0 * hp.hidden_channels * n2
    if hp.flow_type == 1:
        return hp.flow_n_flows * 2 * 4.0 * (hp.inter_channels // 2) * n2
    return 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--shapes", nargs="+", default=["c2", "c3", "long"])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    lib = VitsLib()
    for ft in args.types:
        hp = HP[ft]()
        m = lib.create(W.synthetic_blob(hp, 1234), 0)
        try:
            for sh in args.shapes:
                lengths = shape(sh)
                B, T = len(lengths), int(lengths.max())
                z_p = np.random.default_rng(1).standard_normal((B, hp.inter_channels, T)).astype(np.float32)
                sid = (np.arange(B) % hp.n_speakers).astype(np.int64)
                for _ in range(3):
                    m.flow(z_p, lengths, sid)
                reps = max(3, args.reps // (10 if sh == "long" else 1))
                ts = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    m.flow(z_p, lengths, sid)
                    ts.append(time.perf_counter() - t0)
                print(f"flow_type {ft} shape {sh:4s} B {B:2d} T_y max {T:5d} sum {int(lengths.sum()):6d}: stage call median "
                      f"{1e3 * np.median(ts):8.3f} ms (min {1e3 * min(ts):8.3f}, {reps} calls)  attention GFLOP on valid frames "
                      f"{attention_flops(hp, lengths) / 1e9:8.3f} per call", flush=True)
        finally:
            m.close()


if __name__ == "__main__":
    main()
