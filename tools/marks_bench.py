#!/usr/bin/env python3
"""What a speech-marks request costs (include/vits_marks.h): host wall time of the c2-shaped request (B = 1, 50 tokens, 150 frames,
durations pinned, synthetic default-size weights) with marks off and on

  * through the C ABI (synthesize_pcm16), on the persistent programs and on the launch path (vits_debug_persist 7 / 0);
  * through Synth.synth_audio on a toy voice directory of the same size (front end, session, coalescer included).

Every call ends in the engine's own stream synchronise and the copy to the host, so the clock brackets finished work.  The legs are
timed in alternation -- off, on, off again -- `--rounds` times `--calls` calls each, so that drift of the machine hits them alike; the
figure is the median over rounds of the mean call.  The marks-off leg runs TWICE: the distance between its two medians is the
run-to-run spread a difference has to be read against, and it is written next to the difference.

    python tools/marks_bench.py --out profiles/marks_bench.txt
    VITS_MI355_LIB=/path/to/the/parent/libvits_mi355.so python tools/marks_bench.py --label parent   # no marks symbols: off legs only

A helper, not a gate: nothing asserts on these numbers.
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALES = [0.667, 1.0, 0.8]


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown (not a git checkout)"


def measure(legs, rounds, calls, warmup):
    """legs: [(name, callable)] -> {name: [ms per call, one per round]}, the legs alternated inside every round"""
    for _, fn in legs:
        for _ in range(warmup):
            fn()
    per = {name: [] for name, _ in legs}
    for _ in range(rounds):
        for name, fn in legs:
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            per[name].append((time.perf_counter() - t0) / calls * 1e3)
    return per


def report(title, per, lines):
    med = {k: statistics.median(v) for k, v in per.items()}
    for k, v in per.items():
        lines.append(f"  {title:<28} {k:<8} {med[k]:8.4f} ms  (min {min(v):.4f}, max {max(v):.4f})")
    spread = abs(med["off"] - med["off_2"])
    lines.append(f"  {title:<28} spread of the doubled marks-off leg: {spread:.4f} ms")
    if "on" in med:
        off = (med["off"] + med["off_2"]) / 2
        lines.append(f"  {title:<28} marks on - off: {med['on'] - off:+.4f} ms ({(med['on'] - off) / off * 100:+.2f} %)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=100, help="calls per leg per round")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--label", default="", help="a word for the header (e.g. which library this is)")
    ap.add_argument("--commit", default=None, help="the commit id for the header where the tree is not a git checkout")
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()

    from vosk_tts_amd import Model, Synth
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.capi import VitsLib
    from vosk_tts_amd.toymodel import PHONEMES, write_toy_model

    lib = VitsLib()
    if not lib.is_device or lib.device_count() < 1:
        sys.exit("marks_bench: no GPU: a timing needs one")
    has = getattr(lib, "has_marks", False)
    lines = [f"marks_bench  commit {args.commit or commit()}  library {lib.path}  {args.label}".rstrip(),
             f"c2 request (B = 1, 50 tokens, 150 frames), host wall time per call (ms): median over {args.rounds} rounds of the mean of "
             f"{args.calls} calls, legs alternated" + ("" if has else "; this library has no speech marks: marks-off legs only")]

    # ---- the C ABI
    rng = np.random.default_rng(0)
    ids = rng.integers(1, 62, size=(1, 50)).astype(np.int64)
    lens = np.array([50], np.int64)
    dur = np.full((1, 50), 3, np.int32)
    sid = np.array([1], np.int64)
    model = lib.create(W.synthetic_blob(W.default_hparams(), 1234), 0)

    def abi(marks):
        kw = {"marks": True} if marks else {}
        return lambda: model.synthesize_pcm16(ids, lens, SCALES, sid, forced_durations=dur, seed=1, **kw)

    for name, mask in (("C ABI, persistent programs", 7), ("C ABI, launch path", 0)):
        lib.lib.vits_debug_persist(mask)
        legs = [("off", abi(False))] + ([("on", abi(True))] if has else []) + [("off_2", abi(False))]
        report(name, measure(legs, args.rounds, args.calls, args.warmup), lines)
    lib.lib.vits_debug_persist(7)
    model.close()

    # ---- Synth.synth_audio: a text whose front end gives about 50 tokens
    with tempfile.TemporaryDirectory() as d:
        write_toy_model(d, W.default_hparams(n_vocab=len(PHONEMES)))
        voice = Model(model_path=d, device=0)
        synth = Synth(voice)
        text = "прив+ет, м+ир! прив+ет м+ир."
        n_tok = len(synth.g2p_noembed(synth.normalize(text)))

        def door(marks):
            kw = {"marks": True} if marks else {}
            return lambda: synth.synth_audio(text, speaker_id=1, duration_noise_level=0.0, **kw)

        for name, mask in ((f"synth_audio ({n_tok} tok), persistent", 7), (f"synth_audio ({n_tok} tok), launch", 0)):
            lib.lib.vits_debug_persist(mask)
            legs = [("off", door(False))] + ([("on", door(True))] if has else []) + [("off_2", door(False))]
            report(name, measure(legs, args.rounds, args.calls, args.warmup), lines)
        lib.lib.vits_debug_persist(7)
        voice.onnx.close()

    out = "\n".join(lines)
    print(out)
    if args.out:
        with open(args.out, "a") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
