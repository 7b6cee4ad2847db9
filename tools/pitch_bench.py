#!/usr/bin/env python3
"""What a pitch shift costs per request (include/vits_pitch.h): host wall time of vits_synthesize_pcm16 for the c2 request
(1 x 50 tokens), the c3 batch (32 ragged utterances of 20..200 tokens, independent items) and a 2000-token utterance at the voice's own
rate, with VITS_FLAG_PITCH off and on at +3 and -12 semitones (the stretch ratios 1.189 and 0.5: more and fewer steps than analysis
frames), and at +3 semitones with VITS_FLAG_PITCH_FORMANT (the envelope correction: its cost is the difference to the +3 leg of the same
run), synthetic default-size weights.  Every call ends in the engine's own stream synchronise and the copy to the host, so the clock
brackets finished work.  The legs are timed in alternation (`--rounds` times `--calls` calls each) so that drift of the machine hits
them alike, and the flag-off leg runs twice per round: the difference of its two medians is the spread a flag-on difference has to be
read against.  The figure is the median over rounds of the mean call.

    python tools/pitch_bench.py --out profiles/pitch_bench.txt
    VITS_MI355_LIB=/path/to/the/parent/libvits_mi355.so python tools/pitch_bench.py --plain-only --label parent --out ...
    rocprofv3 --kernel-trace --stats -- python tools/pitch_bench.py --profile 3 --only long
    rocprofv3 --kernel-trace --stats -- python tools/pitch_bench.py --profile 3 --formants --only c2

The second form times the same plain calls on another build of the library (the parent commit's) in the same visit: "flag off" of this
tree has to sit inside that build's own run-to-run spread.  The third is a run of its own for the per-kernel times of the flagged
calls: `--profile S` makes a few calls at S semitones and nothing else, so the pitch_* rows of the kernel statistics are theirs
(`--formants`: with the envelope correction, for pitch_formant_kernel's row).

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

SCALES = np.array([0.667, 1.0, 0.8], np.float32)
SHIFTS = (3.0, -12.0)


def workloads(n_vocab):
    rng = np.random.default_rng(0)
    lens = np.linspace(20, 200, 32).astype(np.int64)
    ids = np.zeros((32, 200), np.int64)
    for b, n in enumerate(lens):
        ids[b, :n] = rng.integers(1, n_vocab, size=n)
    return {
        "c2 (1 x 50 tokens)": dict(ids=rng.integers(1, n_vocab, size=(1, 50)).astype(np.int64), lens=np.array([50], np.int64), solo=False),
        "c3 (32 x 20..200 tokens)": dict(ids=ids, lens=lens, solo=True),
        "long (1 x 2000 tokens)": dict(ids=rng.integers(1, n_vocab, size=(1, 2000)).astype(np.int64), lens=np.array([2000], np.int64), solo=False),
    }


def call(model, w, pitch, formants=False):
    B = w["ids"].shape[0]
    kw = {} if pitch is None else ({"pitch": pitch, "preserve_formants": True} if formants else {"pitch": pitch})
    return model.synthesize_pcm16(w["ids"], w["lens"], SCALES, np.arange(B, dtype=np.int64) % 7, seed=1, solo=w["solo"], **kw)[0]


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown (not a git checkout)"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="calls per leg per round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true", help="only the flag-off legs (a library without the flag: the parent commit's)")
    ap.add_argument("--only", default="", help="time only the workloads whose name starts with this (c2, c3, long)")
    ap.add_argument("--profile", type=float, default=None, metavar="S", help="no timing: 1 + 4 flagged calls at S semitones, for a kernel trace")
    ap.add_argument("--formants", action="store_true", help="with --profile: the flagged calls keep the formants (VITS_FLAG_PITCH_FORMANT)")
    ap.add_argument("--label", default="", help="a word for the header (e.g. which build this is)")
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()

    from vosk_tts_amd import weights as W
    from vosk_tts_amd.capi import VitsLib

    lib = VitsLib()
    if not lib.is_device or lib.device_count() < 1:
        sys.exit("pitch_bench: no GPU: a timing needs one")
    hp = W.default_hparams()
    model = lib.create(W.synthetic_blob(hp, 1234), 0)
    if args.profile is not None:
        for name, w in workloads(hp.n_vocab).items():
            if name.startswith(args.only):
                for _ in range(5):
                    pcm = call(model, w, args.profile, args.formants)
                print(f"profile: 5 calls of {name} at {args.profile:+g} semitones{', formants kept' if args.formants else ''}, {pcm.size} samples each")
        model.close()
        return
    on = [] if args.plain_only or not getattr(lib, "has_pitch", False) else [(f"{s:+g} st", s, False) for s in SHIFTS]
    if on and getattr(lib, "has_pitch_formant", False):
        on.append((f"{SHIFTS[0]:+g} st, formants kept", SHIFTS[0], True))
    legs = [("off", None, False), ("off again", None, False)] + on
    path = os.path.relpath(lib.path, ROOT) if os.path.abspath(lib.path).startswith(ROOT + os.sep) else lib.path
    lines = [f"pitch_bench  commit {commit()}  library {path}  {args.label}".rstrip(),
             f"host wall time per call (ms): median over {args.rounds} rounds of the mean of {args.calls} calls, legs alternated"]
    for name, w in workloads(hp.n_vocab).items():
        if not name.startswith(args.only):
            continue
        calls = max(args.calls // 4, 2) if w["ids"].shape[1] >= 1000 or w["ids"].shape[0] > 1 else args.calls
        for _, s, fm in legs:
            for _ in range(args.warmup):
                pcm = call(model, w, s, fm)
        per = {v: [] for v, _, _ in legs}
        for _ in range(args.rounds):
            for v, s, fm in legs:
                t0 = time.perf_counter()
                for _ in range(calls):
                    pcm = call(model, w, s, fm)
                per[v].append((time.perf_counter() - t0) / calls * 1e3)
        base = statistics.median(per["off"])
        for v, _, _ in legs:
            med = statistics.median(per[v])
            lines.append(f"  {name}  {v:>22}  {med:8.4f} ms  (min {min(per[v]):.4f}, max {max(per[v]):.4f})  "
                         f"{med - base:+.4f} ms vs off  {pcm.size} samples to the host")
    model.close()
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
