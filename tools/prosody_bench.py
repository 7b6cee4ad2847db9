#!/usr/bin/env python3
"""What the prosody controls cost and what they buy (include/vits_prosody.h), as host wall time on synthetic default-size weights:

  1. one 50-token request through the C ABI (synthesize_pcm16, free-running durations, fixed seed) with the flag off, and with a pause, a
     per-token rate and a fit to a frame count: the controlled call runs the text side as launches, the uncontrolled one the
     single-utterance program;
  2. a solo batch of 32 such requests (durations pinned, so both legs do the same work) with one set of scales, and with 32 different ones
     as item_scales;
  3. the serving leg -- 16 threads on ONE Synth of a toy voice directory (server/tts_server.py's shape), every client asking for its own
     speech_rate: requests/s and the mean batch the coalescer formed, next to the same traffic at one common rate.

Legs 1 and 2 alternate off, on, off again; the distance between the two off medians is the spread a difference is read against.  Leg 3
also runs on a tree without the controls (copy this file into it): there, requests at different rates never share a batch.

    python tools/prosody_bench.py --out profiles/prosody_bench.txt

A helper, not a gate: nothing asserts on these numbers.
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import threading
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
        lines.append(f"  {title:<34} {k:<6} {med[k]:8.4f} ms  (min {min(v):.4f}, max {max(v):.4f})")
    off = (med["off"] + med["off_2"]) / 2
    lines.append(f"  {title:<34} spread of the doubled off leg: {abs(med['off'] - med['off_2']):.4f} ms;  on - off: "
                 f"{med['on'] - off:+.4f} ms ({(med['on'] - off) / off * 100:+.2f} %)")


def serving(synth, sess, text, rates, seconds):
    """len(rates) threads, thread k calling synth_audio(text, speech_rate=rates[k]) for `seconds` -> (requests/s, mean batch, largest)"""
    n = len(rates)
    for k in range(min(n, 4)):
        synth.synth_audio(text, speaker_id=2, speech_rate=rates[k])
    wstop = time.perf_counter() + 0.5  # the same traffic untimed first: every batch size / bucket it produces gets its workspace and graphs

    def warm(k):
        while time.perf_counter() < wstop:
            synth.synth_audio(text, speaker_id=2, speech_rate=rates[k])

    wt = [threading.Thread(target=warm, args=(k,)) for k in range(n)]
    [t.start() for t in wt]
    [t.join() for t in wt]
    co = sess.coalescer
    c0 = (co.calls, co.requests)
    co.largest = 0
    done = [0] * n
    stop = time.perf_counter() + seconds

    def worker(k):
        while time.perf_counter() < stop:
            synth.synth_audio(text, speaker_id=2, speech_rate=rates[k])
            done[k] += 1

    t0 = time.perf_counter()
    th = [threading.Thread(target=worker, args=(k,)) for k in range(n)]
    [t.start() for t in th]
    [t.join() for t in th]
    el = time.perf_counter() - t0
    calls, reqs = co.calls - c0[0], co.requests - c0[1]
    return sum(done) / el, reqs / max(calls, 1), co.largest


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=60, help="calls per leg per round")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=2.0, help="length of each serving leg")
    ap.add_argument("--serving-legs", type=int, default=3, help="repeats of each serving leg (their spread is printed)")
    ap.add_argument("--serving-only", action="store_true")
    ap.add_argument("--label", default="", help="a word for the header (e.g. which tree this is)")
    ap.add_argument("--commit", default=None, help="the commit id for the header where the tree is not a git checkout")
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()

    from vosk_tts_amd import Model, Synth
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.capi import VitsLib
    from vosk_tts_amd.toymodel import PHONEMES, write_toy_model

    lib = VitsLib()
    if not lib.is_device or lib.device_count() < 1:
        sys.exit("prosody_bench: no GPU: a timing needs one")
    has = getattr(lib, "has_prosody", False)
    lines = [f"prosody_bench  commit {args.commit or commit()}  library {lib.path}  {args.label}".rstrip(),
             f"host wall time per call (ms): median over {args.rounds} rounds of the mean of {args.calls} calls, legs alternated"
             + ("" if has else "; this library has no prosody controls: the serving leg only")]

    if has and not args.serving_only:
        rng = np.random.default_rng(0)
        model = lib.create(W.synthetic_blob(W.default_hparams(), 1234), 0)
        # ---- 1. one request
        ids = rng.integers(1, 62, size=(1, 50)).astype(np.int64)
        lens, sid = np.array([50], np.int64), np.array([1], np.int64)
        _, ol = model.synthesize_pcm16(ids, lens, SCALES, sid, seed=1)
        tls = np.ones((1, 50), np.float32)
        tls[0, 10:20] = 1.5
        pause = np.zeros((1, 50), np.int32)
        pause[0, 25] = 20
        fit = np.array([int(ol[0]) // 256 + 30], np.int32)
        plain = lambda: model.synthesize_pcm16(ids, lens, SCALES, sid, seed=1)
        ctl = lambda: model.synthesize_pcm16(ids, lens, SCALES, sid, seed=1, token_length_scale=tls, token_pause=pause, fit_frames=fit)
        for name, mask in (("1 request, persistent programs", 7), ("1 request, launch path", 0)):
            lib.lib.vits_debug_persist(mask)
            report(name, measure([("off", plain), ("on", ctl), ("off_2", plain)], args.rounds, args.calls, args.warmup), lines)
        lib.lib.vits_debug_persist(7)
        # ---- 2. a solo batch of 32
        ids = rng.integers(1, 62, size=(32, 50)).astype(np.int64)
        lens, sid = np.full(32, 50, np.int64), np.arange(32, dtype=np.int64) % 4
        dur = np.full((32, 50), 3, np.int32)
        isc = np.stack([0.5 + 0.01 * np.arange(32), 0.8 + 0.0125 * np.arange(32), 0.6 + 0.01 * np.arange(32)], axis=1).astype(np.float32)
        plain = lambda: model.synthesize_pcm16(ids, lens, SCALES, sid, seed=1, solo=True, forced_durations=dur)
        ctl = lambda: model.synthesize_pcm16(ids, lens, SCALES, sid, seed=1, solo=True, forced_durations=dur, item_scales=isc)
        report("batch of 32, one scale set / 32", measure([("off", plain), ("on", ctl), ("off_2", plain)], args.rounds, max(args.calls // 4, 5), 4), lines)
        model.close()

    # ---- 3. serving: 16 threads, one Synth
    with tempfile.TemporaryDirectory() as d:
        write_toy_model(d, W.default_hparams(n_vocab=len(PHONEMES)))
        voice = Model(model_path=d, device=0)
        synth = Synth(voice)
        text = "привет мир привет мир."
        n_tok = len(synth.g2p_noembed(synth.normalize(text)))
        own = [round(0.8 + 0.03 * k, 2) for k in range(16)]
        lines.append(f"  serving: 16 threads x synth_audio ({n_tok} tokens) on one Synth, {args.seconds:g} s per leg, {args.serving_legs} legs each, alternated")
        res = {"one common speech_rate": [], "every client its own speech_rate": []}
        for _ in range(args.serving_legs):
            res["one common speech_rate"].append(serving(synth, voice.onnx, text, [1.0] * 16, args.seconds))
            res["every client its own speech_rate"].append(serving(synth, voice.onnx, text, own, args.seconds))
        for name, rows in res.items():
            rps = [r[0] for r in rows]
            lines.append(f"  serving, {name:<34} {statistics.median(rps):8.1f} requests/s (min {min(rps):.1f}, max {max(rps):.1f}), mean batch "
                         f"{statistics.median(r[1] for r in rows):.2f}, largest {max(r[2] for r in rows)}")
        voice.onnx.close()

    out = "\n".join(lines)
    print(out)
    if args.out:
        with open(args.out, "a") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
