#!/usr/bin/env python3
"""What the vocoder-bias denoiser costs per request (include/vits_denoise.h): host wall time of stts_synthesize for the c2-sized
multistream request (50 symbols, 3 frames each) and of stts_synthesize_batch for 32 ragged utterances (20..200 symbols), without
the denoiser and with it at filter lengths 1024 and 256, synthetic default-size weights, bundled HiFi-GAN V1.  Every call ends in
the engine's own stream synchronise and the copy to the host, so the clock brackets finished work.  The variants are timed in
alternation (`--rounds` times `--calls` calls each) so that drift of the machine hits them alike; the figure is the median over
rounds of the mean call.

    python tools/denoise_bench.py --out profiles/denoise_bench.txt

A helper, not a gate: nothing asserts on these numbers.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALES = np.array([0.8, 1.0, 0.8], np.float32)
STRENGTH = 0.00025  # the StableTTS script's default (the cost does not depend on it)
VARIANTS = (("plain", None), ("n 1024", 1024), ("n 256", 256))


def workloads():
    rng = np.random.default_rng(0)
    one = dict(ids=rng.integers(1, 40, size=(5, 50)).astype(np.int64), pde=np.full(50, 3.0, np.float32))
    lens = np.linspace(20, 200, 32).astype(np.int64)
    ids = np.zeros((32, 5, 200), np.int64)
    for b, n in enumerate(lens):
        ids[b, :, :n] = rng.integers(1, 40, size=(5, n))
    batch = dict(ids=ids, lens=lens, pde=np.full((32, 200), 3.0, np.float32), sid=np.arange(32, dtype=np.int64) % 7)
    return {"c2 (1 x 50 symbols)": one, "batch (32 x 20..200 symbols)": batch}


def call(model, w, n):
    kw = {} if n is None else {"denoiser_strength": STRENGTH, "denoiser_filter_length": n}
    if "lens" in w:
        return model.synthesize_batch(w["ids"], w["lens"], SCALES, w["sid"], None, w["pde"], seed=1, **kw)[0]
    return model.synthesize(w["ids"], SCALES, 2, None, w["pde"], seed=1, want_mel=False, **kw)[0]


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown (not a git checkout)"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="calls per variant per round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="", help="a word for the header (e.g. which tree this is)")
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()

    from vosk_tts_amd import weights as W
    from vosk_tts_amd import weights_stts as S
    from vosk_tts_amd.capi import VitsLib
    from vosk_tts_amd.capi_stts import SttsModel

    lib = VitsLib()
    if not lib.is_device or lib.device_count() < 1:
        sys.exit("denoise_bench: no GPU: a timing needs one")
    voc = lib.create(W.synthetic_blob(W.hifigan_v1_vocoder_hparams(), 1234), 0)
    model = SttsModel(lib, S.synthetic_blob(S.default_hparams(40, 7), 1234), voc)
    variants = VARIANTS if lib.has_denoise else VARIANTS[:1]
    path = os.path.relpath(lib.path, ROOT) if os.path.abspath(lib.path).startswith(ROOT + os.sep) else lib.path
    lines = [f"denoise_bench  commit {commit()}  library {path}  {args.label}".rstrip(),
             f"host wall time per call (ms): median over {args.rounds} rounds of the mean of {args.calls} calls, variants alternated"]
    for name, w in workloads().items():
        for _, n in variants:
            for _ in range(args.warmup):
                audio = call(model, w, n)
        per = {v: [] for v, _ in variants}
        for _ in range(args.rounds):
            for v, n in variants:
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    audio = call(model, w, n)
                per[v].append((time.perf_counter() - t0) / args.calls * 1e3)
        base = statistics.median(per["plain"])
        for v, _ in variants:
            med = statistics.median(per[v])
            lines.append(f"  {name}  {v:>7}  {med:8.4f} ms  (min {min(per[v]):.4f}, max {max(per[v]):.4f})  {med - base:+.4f} ms vs plain  "
                         f"{audio.size} samples to the host")
    model.close()
    report = "\n".join(lines)
    print(report)
    if args.out:
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
