#!/usr/bin/env python3
"""Duration-predictor time, stochastic (dp_n_flows 4) against deterministic (dp_n_flows 0, use_sdp false), at the default size:

    python tools/dp_types_profile.py [--shapes c2 c3 long] [--reps 20] [--forward-steps 200]

Stage: vits_stage_duration, median wall time of the call (it includes the host copies of x in and logw out: B * 192 * T_x * 4 and
B * T_x * 4 bytes).  c2 = one utterance of T_x 50, c3 = 32 ragged items (T_x 20..200, bench.py's c3 lengths), long = one utterance
of T_x 2000.  At B=1, T_x <= 256 the stochastic predictor runs as its persistent program (when no other process holds the device's
programs), the deterministic one on launches.
Forward: the c2 workload exactly as bench.py times it -- a device session with hipGraph replay, durations pinned to bench.py's c2
durations and the duration predictor executed anyway (set_sdp_always) -- median per-forward time over blocks of --forward-steps.
For the kernel list of one deterministic c2 forward: rocprofv3 --kernel-trace --stats -- python tools/dp_types_profile.py --shapes
--only det --forward-steps 50."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (one HIP runtime per process: torch first, as bench.py)

from vosk_tts_amd import weights as W  # noqa: E402
from vosk_tts_amd.capi import VitsDeviceSession, VitsLib  # noqa: E402

HP = {"sdp": W.default_hparams, "det": W.deterministic_dp_hparams}


def lengths_of(name):
    if name == "c2":
        return np.array([50], np.int64)
    if name == "c3":
        return np.random.default_rng(1234).integers(20, 201, size=32).astype(np.int64)
    return np.array([2000], np.int64)


def stage(m, hp, name, reps):
    lengths = lengths_of(name)
    B, T = len(lengths), int(lengths.max())
    rng = np.random.default_rng(1)
    x = rng.standard_normal((B, hp.hidden_channels, T)).astype(np.float32)
    noise = rng.standard_normal((B, 2, T)).astype(np.float32)
    sid = (np.arange(B) % hp.n_speakers).astype(np.int64)
    for _ in range(3):
        m.duration(x, lengths, sid, noise, 0.8)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        m.duration(x, lengths, sid, noise, 0.8)
        ts.append(time.perf_counter() - t0)
    return B, T, np.median(ts), min(ts)


def forward_c2(m, steps, blocks=5):
    sys.path.insert(0, ROOT)
    import bench

    ids, lengths, dur = bench.make_workload("c2", np.random.default_rng(1234))
    B, Tx = ids.shape
    Ty = int(dur.sum(1).max())
    S = Ty * m.hp.hop_length
    scales = np.array([0.8, 1.0, 0.8], np.float32)
    dev = torch.device("cuda", 0)
    d_ids, d_len, d_dur = (torch.from_numpy(a).to(dev) for a in (ids, lengths, dur))
    d_sid = torch.full((B,), 2, dtype=torch.int64, device=dev)
    d_audio = torch.zeros((B, S), dtype=torch.float32, device=dev)
    sess = VitsDeviceSession(m, B, Tx, Ty)
    try:
        sess.set_options(use_graph=True, profile=False)
        sess.set_sdp_always(True)

        def step():
            sess.synthesize_device(d_ids.data_ptr(), d_len.data_ptr(), B, Tx, scales, d_sid.data_ptr(), d_dur.data_ptr(), Ty, 7,
                                   d_audio.data_ptr(), S)

        for _ in range(20):
            step()
        sess.sync()
        out = []
        for _ in range(blocks):
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            sess.sync()
            out.append((time.perf_counter() - t0) / steps)
        return Tx, Ty, np.median(out), min(out)
    finally:
        sess.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["c2", "c3", "long"])
    ap.add_argument("--only", choices=["sdp", "det"], default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--forward-steps", type=int, default=200)
    args = ap.parse_args()
    lib = VitsLib()
    kinds = [args.only] if args.only else ["sdp", "det"]
    for kind in kinds:
        hp = HP[kind]()
        m = lib.create(W.synthetic_blob(hp, 1234), 0)
        try:
            for sh in args.shapes:
                B, T, med, mn = stage(m, hp, sh, max(3, args.reps // (4 if sh == "long" else 1)))
                print(f"duration stage  {kind}  {sh:4s} B {B:2d} T_x max {T:5d}: median {1e3 * med:8.3f} ms (min {1e3 * mn:8.3f})", flush=True)
            if args.forward_steps > 0:
                Tx, Ty, med, mn = forward_c2(m, args.forward_steps)
                print(f"c2 forward      {kind}  T_x {Tx} T_y {Ty}: median {1e3 * med:8.4f} ms per forward (min {1e3 * mn:8.4f})", flush=True)
        finally:
            m.close()


if __name__ == "__main__":
    main()
