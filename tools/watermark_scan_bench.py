#!/usr/bin/env python3
"""What the watermark scan costs next to the detector on the same audio (include/vits_watermark_scan.h): host wall time of
vits_op_watermark_scan on 3 s, 12.5 s and 60 s of the marked test signal at spans 1, 4 and 8, and of vits_op_watermark_detect on the
same buffers in the same visit.  Both doors upload the audio, allocate, launch, synchronise and download, so the clock brackets
finished work and the figures include the copies (the scan downloads [128, W] doubles where the detector downloads 128): an upper
bound for the kernels.  The legs are timed in alternation (`--rounds` times `--calls` calls each) so that drift of the machine hits
them alike, and the detector runs twice per round: the difference of its two medians is the spread every ratio has to be read against.
The figure is the median over rounds of the mean call.

    python tools/watermark_scan_bench.py --out profiles/watermark_scan_bench.txt

A helper, not a gate: nothing asserts on these numbers, and no target was fixed in advance.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

KEY = 0x5EED1234
SPANS = (1, 4, 8)


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown (not a git checkout)"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10, help="calls per leg per round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="", help="a word for the header")
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()

    import watermark_ref as R

    from vosk_tts_amd.capi import VitsLib
    from vosk_tts_amd.watermark_scan import segments

    lib = VitsLib()
    if not lib.is_device or lib.device_count() < 1:
        sys.exit("watermark_scan_bench: no GPU: a timing needs one")
    if not getattr(lib, "has_watermark_scan", False):
        sys.exit("watermark_scan_bench: this library has no vits_op_watermark_scan")
    path = os.path.relpath(lib.path, ROOT) if os.path.abspath(lib.path).startswith(ROOT + os.sep) else lib.path
    lines = [f"watermark_scan_bench  commit {commit()}  library {path}  {args.label}".rstrip(),
             f"host wall time per call (ms): median over {args.rounds} rounds of the mean of {args.calls} calls, legs alternated, doors with their copies"]
    x3 = R.embed(R.voiced_signal(3.0), KEY).astype(np.float32)
    tiled = np.tile(x3[:65536], 21)  # (whole pattern periods, so the tiling keeps the mark)
    for name, x in (("3 s", x3), ("12.5 s", tiled[:275625]), ("60 s", tiled[:60 * 22050])):
        n = [x.shape[0]]
        legs = {"detect": lambda: lib.op_watermark_detect(x[None], n, KEY), "detect again": lambda: lib.op_watermark_detect(x[None], n, KEY)}
        for span in SPANS:
            legs[f"scan span {span}"] = lambda span=span: lib.op_watermark_scan(x[None], n, KEY, span=span)
        for fn in legs.values():
            for _ in range(args.warmup):
                fn()
        per = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                per[k].append((time.perf_counter() - t0) / args.calls * 1e3)
        base = statistics.median(per["detect"])
        for k in legs:
            med = statistics.median(per[k])
            what = ""
            if k.startswith("scan"):
                span = int(k.split()[-1])
                z, first, wins = lib.op_watermark_scan(x[None], n, KEY, span=span)
                what = f"  {int(wins.max())} windows x 128 offsets, best {z.max():.2f}, {len(segments(z[0], first[0], wins[0], span, n[0]))} segment(s)"
            elif k == "detect":
                what = f"  z {lib.op_watermark_detect(x[None], n, KEY)[0][0]:.2f}"
            lines.append(f"  {name:>6} ({n[0]:>7} samples)  {k:>12}  {med:8.4f} ms  (min {min(per[k]):.4f}, max {max(per[k]):.4f})  x{med / base:.2f} of detect{what}")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
