#!/usr/bin/env python3
"""What the peak limiter costs per request (include/vits_limit.h): host wall time of vits_synthesize_pcm16 for the c2 request
(1 x 50 tokens), the c3 batch (32 ragged utterances of 20..200 tokens, independent items) and a 2000-token utterance at the voice's
own rate, with the flags off, with a loudness target alone (-19 LUFS), and with the target plus the limiter in sample-peak and in
true-peak mode (two passes), synthetic default-size weights.  Every call ends in the engine's own stream synchronise and the copy to
the host, so the clock brackets finished work.  The legs are timed in alternation (`--rounds` times `--calls` calls each) so that drift
of the machine hits them alike, and the flags-off leg runs twice per round: the difference of its two medians is the spread the other
differences have to be read against.  The figure is the median over rounds of the mean call.

    python tools/limit_bench.py --out profiles/limit_bench.txt
    VITS_MI355_LIB=/path/to/the/parent/libvits_mi355.so python tools/limit_bench.py --plain-only --commit <its hash> --out ...

The second form times the flags-off and the loudness-only calls on another build of the library (the parent commit's) in the same
visit: those legs of this tree have to sit inside that build's own run-to-run spread.

A helper, not a gate: nothing asserts on these numbers.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from loudness_bench import SCALES, commit, workloads  # noqa: E402


def call(model, w, kw):
    B = w["ids"].shape[0]
    return model.synthesize_pcm16(w["ids"], w["lens"], SCALES, np.arange(B, dtype=np.int64) % 7, seed=1, solo=w["solo"], **kw)[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="calls per leg per round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true", help="only the legs without the limiter (a library without it: the parent commit's)")
    ap.add_argument("--only", default="", help="time only the workloads whose name starts with this (c2, c3, long)")
    ap.add_argument("--label", default="", help="a word for the header (e.g. which build this is)")
    ap.add_argument("--commit", default=None, help="the commit the library under test was built from (default: this checkout's HEAD)")
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()

    from vosk_tts_amd import weights as W
    from vosk_tts_amd.capi import VitsLib, loudness_spec

    lib = VitsLib()
    if not lib.is_device or lib.device_count() < 1:
        sys.exit("limit_bench: no GPU: a timing needs one")
    hp = W.default_hparams()
    model = lib.create(W.synthetic_blob(hp, 1234), 0)
    legs = [("off", {}), ("off again", {}), ("loudness", {"loudness": loudness_spec(loudness=-19.0)})]
    if not args.plain_only and getattr(lib, "has_limit", False):
        from vosk_tts_amd.capi import limit_spec

        free = loudness_spec(loudness=-19.0, peak_ceiling=0.0)
        legs += [("+ sample", {"loudness": free, "limit": limit_spec("sample", 0.5)}), ("+ true", {"loudness": free, "limit": limit_spec("true", 0.5)})]
    lines = [f"limit_bench  commit {args.commit or commit()}  {args.label}".rstrip(),
             f"host wall time per call (ms): median over {args.rounds} rounds of the mean of the calls of a leg, legs alternated"]
    for name, w in workloads(hp.n_vocab).items():
        if not name.startswith(args.only):
            continue
        calls = max(args.calls // 4, 2) if w["ids"].shape[1] >= 1000 or w["ids"].shape[0] > 1 else args.calls
        for _, kw in legs:
            for _ in range(args.warmup):
                pcm = call(model, w, kw)
        per = {v: [] for v, _ in legs}
        for _ in range(args.rounds):
            for v, kw in legs:
                t0 = time.perf_counter()
                for _ in range(calls):
                    pcm = call(model, w, kw)
                per[v].append((time.perf_counter() - t0) / calls * 1e3)
        base = statistics.median(per["off"])
        for v, _ in legs:
            med = statistics.median(per[v])
            lines.append(f"  {name}  {v:>9}  {med:8.4f} ms  (min {min(per[v]):.4f}, max {max(per[v]):.4f})  {med - base:+.4f} ms vs off  "
                         f"{calls} calls per leg  {pcm.size} samples to the host")
    model.close()
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
