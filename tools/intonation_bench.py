#!/usr/bin/env python3
"""What an intonation range costs per request (include/vits_intonation.h), and that a call without the flag is the call it was: host
wall time of vits_synthesize_pcm16 for the c2 request (1 x 50 tokens) and the c3 batch (32 ragged utterances, independent items) plain,
with pitch=+3 (the pitch stage), with a three-word contour (the contour stage), with pitch_range=0.5, and with both; and the tracker
alone through vits_op_f0_track on the requests' own audio.  Synthetic default-size weights: their audio has no voiced frame, so the
range alone is the exact case of include/vits_intonation.h (the tracker, the per-item kernel, the read-back and the gain kernel, no
vocoder), and what the stage costs a voiced utterance is the "contour + range" leg against the "contour" leg.
Every call ends in the engine's own stream synchronise and the copy to the host, so the clock brackets finished work.  The legs are
timed in alternation (`--rounds` times `--calls` calls each) so that drift of the machine hits them alike, and the plain leg runs
twice per round: the difference of its two medians is the spread every other difference has to be read against.  The figure is the
median over rounds of the mean call.  The door's figure includes its upload, its allocation and its download: an upper bound for the
kernel.

    python tools/intonation_bench.py --out profiles/intonation_bench.txt
    VITS_MI355_LIB=/path/to/the/parent/libvits_mi355.so python tools/intonation_bench.py --label parent --out profiles/intonation_bench.txt
    python tools/intonation_bench.py --identity --out profiles/intonation_identity.txt

The second form times the legs the other build has (the parent commit's has no intonation) in the same visit.  The third prints SHA-256
digests of the paths that carry no intonation flag -- vits_op_pitch_shift, vits_op_contour, a plain, a shifted and a contoured toy-voice
request -- on fixed seeded inputs: run on both builds they must be equal, since contour_run now takes the frame table as an argument.

A helper, not a gate: nothing asserts on these numbers.
"""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALES = np.array([0.667, 1.0, 0.8], np.float32)


def workloads(n_vocab):
    rng = np.random.default_rng(0)
    lens = np.linspace(20, 200, 32).astype(np.int64)
    ids = np.zeros((32, 200), np.int64)
    for b, n in enumerate(lens):
        ids[b, :n] = rng.integers(1, n_vocab, size=n)
    return {"c2 (1 x 50 tokens)": dict(ids=rng.integers(1, n_vocab, size=(1, 50)).astype(np.int64), lens=np.array([50], np.int64), solo=False),
            "c3 (32 x 20..200 tokens)": dict(ids=ids, lens=lens, solo=True)}


def three_words(B, Tx):
    st, db = np.zeros((B, Tx), np.float32), np.zeros((B, Tx), np.float32)
    st[:, 2:7], st[:, 9:14], st[:, 15:20] = 3.0, -4.0, 2.0
    db[:, 2:7], db[:, 15:20] = 6.0, -6.0
    return st, db


def call(model, w, leg):
    B, Tx = w["ids"].shape
    kw = {}
    if leg == "pitch":
        kw = {"pitch": 3.0}
    elif leg == "contour":
        kw = dict(zip(("token_pitch", "token_gain_db"), three_words(B, Tx)))
    elif leg == "range":
        kw = {"pitch_range": 0.5}
    elif leg == "contour + range":
        kw = dict(zip(("token_pitch", "token_gain_db"), three_words(B, Tx)), pitch_range=0.5)
    return model.synthesize_pcm16(w["ids"], w["lens"], SCALES, np.arange(B, dtype=np.int64) % 7, seed=1, solo=w["solo"], **kw)[0]


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown (not a git checkout)"


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def identity(lib, W):
    rng = np.random.default_rng(20)
    x = (0.2 * rng.standard_normal((2, 6000))).astype(np.float32)
    lens = np.array([6000, 4173], np.int64)
    lines = [f"  op_pitch_shift {s:+g} st  {sha(lib.op_pitch_shift(x, lens, s))}" for s in (3.0, -12.0)]
    cum = np.array([[8, 16, 24], [5, 11, 17]], np.int32)
    st = np.array([[3.0, -4.0, 0.0], [12.0, 0.0, -12.0]], np.float32)
    db = np.array([[0.0, 6.0, -6.0], [0.0, 0.0, 3.0]], np.float32)
    lines.append(f"  op_contour            {sha(lib.op_contour(x, lens, cum, [3, 3], 256, st, db))}")
    hp = W.tiny_hparams()
    model = lib.create(W.synthetic_blob(hp, 1234), 0)
    ids = np.random.default_rng(21).integers(1, 20, size=(1, 24)).astype(np.int64)
    tp = np.zeros((1, 24), np.float32)
    tp[0, 3:9], tp[0, 12:20] = 4.0, -3.0
    lines.append(f"  plain request, float  {sha(model.synthesize(ids, [24], SCALES, [1], seed=3)[0])}")
    lines.append(f"  plain request, int16  {sha(model.synthesize_pcm16(ids, [24], SCALES, [1], seed=3)[0])}")
    lines.append(f"  pitch=+3 request      {sha(model.synthesize(ids, [24], SCALES, [1], seed=3, pitch=3.0)[0])}")
    lines.append(f"  contoured request     {sha(model.synthesize(ids, [24], SCALES, [1], seed=3, token_pitch=tp)[0])}")
    lines.append(f"  contoured, int16      {sha(model.synthesize_pcm16(ids, [24], SCALES, [1], seed=3, token_pitch=tp)[0])}")
    model.close()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="calls per leg per round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--identity", action="store_true", help="no timing: the digests of the unflagged paths")
    ap.add_argument("--label", default="", help="a word for the header (e.g. which build this is)")
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()

    from vosk_tts_amd import weights as W
    from vosk_tts_amd.capi import VitsLib

    lib = VitsLib()
    if not lib.is_device or lib.device_count() < 1:
        sys.exit("intonation_bench: no GPU: a timing needs one")
    path = os.path.relpath(lib.path, ROOT) if os.path.abspath(lib.path).startswith(ROOT + os.sep) else lib.path
    head = f"commit {commit()}  library {path}  {args.label}".rstrip()
    if args.identity:
        lines = [f"intonation_identity  {head}"] + identity(lib, W)
    else:
        hp = W.default_hparams()
        model = lib.create(W.synthetic_blob(hp, 1234), 0)
        has = getattr(lib, "has_intonation", False)
        legs = ["plain", "plain again", "pitch"] + (["contour"] if getattr(lib, "has_contour", False) else []) + (["range", "contour + range"] if has else [])
        lines = [f"intonation_bench  {head}",
                 f"host wall time per call (ms): median over {args.rounds} rounds of the mean of {args.calls} calls, legs alternated"]
        for name, w in workloads(hp.n_vocab).items():
            calls = max(args.calls // 4, 2) if w["ids"].shape[0] > 1 else args.calls
            for leg in legs:
                for _ in range(args.warmup):
                    call(model, w, leg)
            per = {leg: [] for leg in legs}
            for _ in range(args.rounds):
                for leg in legs:
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        call(model, w, leg)
                    per[leg].append((time.perf_counter() - t0) / calls * 1e3)
            base = statistics.median(per["plain"])
            for leg in legs:
                med = statistics.median(per[leg])
                lines.append(f"  {name}  {leg:>15}  {med:8.4f} ms  (min {min(per[leg]):.4f}, max {max(per[leg]):.4f})  {med - base:+.4f} ms vs plain")
        if has:  # the tracker alone, on the audio of the c2 request and of the c3 batch
            for name, w in workloads(hp.n_vocab).items():
                B = w["ids"].shape[0]
                audio, ol = model.synthesize(w["ids"], w["lens"], SCALES, np.arange(B, dtype=np.int64) % 7, seed=1, solo=w["solo"])
                for _ in range(args.warmup):
                    cents = lib.op_f0_track(audio, ol, hp.sampling_rate)
                per = []
                for _ in range(args.rounds):
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        lib.op_f0_track(audio, ol, hp.sampling_rate)
                    per.append((time.perf_counter() - t0) / args.calls * 1e3)
                rows = int((1 + ol // 256).sum())
                lines.append(f"  {name}  op_f0_track  {statistics.median(per):8.4f} ms  (min {min(per):.4f}, max {max(per):.4f})  {rows} rows, "
                             f"{int((cents > 0).sum())} voiced, door with its copies")
        model.close()
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
