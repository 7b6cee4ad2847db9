#!/usr/bin/env python3
"""What an output sample rate costs per request (include/vits_resample.h): host wall time of synthesize_pcm16 at the voice's own
rate and at 8000 / 16000 / 48000 Hz, for the c2 request (B = 1, 50 tokens, 150 frames) and the c3 batch (B = 32, 20..200 tokens,
3 frames per token), durations pinned, synthetic default-size weights.  Every call ends in the engine's own stream synchronise and
the copy to the host, so the clock brackets finished work.  The variants are timed in alternation (round-robin over the rates,
`--rounds` times `--calls` calls each) so that drift of the machine hits them alike; the figure is the median over rounds of the
mean call.

    python tools/resample_bench.py --out profiles/resample_bench.txt
    VITS_MI355_LIB=/path/to/another/libvits_mi355.so python tools/resample_bench.py     # a library without the resampler: native only
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/resample_bench.py --trace-run  # few calls, for the kernel's own time

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

RATES = (8000, 16000, 48000)
SCALES = [0.667, 1.0, 0.8]


def workloads():
    rng = np.random.default_rng(0)
    c2 = dict(ids=rng.integers(1, 62, size=(1, 50)).astype(np.int64), lens=np.array([50], np.int64))
    lens = np.linspace(20, 200, 32).astype(np.int64)
    ids = np.zeros((32, 200), np.int64)
    for b, n in enumerate(lens):
        ids[b, :n] = rng.integers(1, 62, size=n)
    c3 = dict(ids=ids, lens=lens)
    for w in (c2, c3):
        dur = np.zeros(w["ids"].shape, np.int32)
        for b, n in enumerate(w["lens"]):
            dur[b, :n] = 3
        w["dur"] = dur
        w["sid"] = np.arange(w["ids"].shape[0], dtype=np.int64) % 4
    return {"c2": c2, "c3": c3}


def call(model, w, rate):
    kw = {"sample_rate": rate} if rate else {}
    return model.synthesize_pcm16(w["ids"], w["lens"], SCALES, w["sid"], forced_durations=w["dur"], seed=1, **kw)


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown (not a git checkout)"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=40, help="calls per variant per round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace-run", action="store_true", help="warm up, then 20 calls per variant: the run to put under a kernel trace")
    ap.add_argument("--label", default="", help="a word for the header (e.g. which library this is)")
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()

    from vosk_tts_amd import weights as W
    from vosk_tts_amd.capi import VitsLib

    lib = VitsLib()
    if not lib.is_device or lib.device_count() < 1:
        sys.exit("resample_bench: no GPU: a timing needs one")
    model = lib.create(W.synthetic_blob(W.default_hparams(), 1234), 0)
    rates = (None,) + (RATES if getattr(lib, "has_resample", False) else ())
    lines = [f"resample_bench  commit {commit()}  library {lib.path}  {args.label}".rstrip(),
             f"synthesize_pcm16, host wall time per call (ms): median over {args.rounds} rounds of the mean of {args.calls} calls, variants alternated"]
    for name, w in workloads().items():
        for r in rates:
            for _ in range(args.warmup):
                pcm, ol = call(model, w, r)
        if args.trace_run:
            for r in rates:
                for _ in range(20):
                    call(model, w, r)
            continue
        per = {r: [] for r in rates}
        size = {}
        for _ in range(args.rounds):
            for r in rates:
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    pcm, ol = call(model, w, r)
                per[r].append((time.perf_counter() - t0) / args.calls * 1e3)
                size[r] = pcm.nbytes
        base = statistics.median(per[None])
        for r in rates:
            med = statistics.median(per[r])
            lines.append(f"  {name}  {'native' if r is None else r:>6}  {med:8.4f} ms  (min {min(per[r]):.4f}, max {max(per[r]):.4f})  "
                         f"{med - base:+.4f} ms vs native  {size[r]:>9} bytes to the host")
    model.close()
    if args.trace_run:
        print("trace run done")
        return
    report = "\n".join(lines)
    print(report)
    if args.out:
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
