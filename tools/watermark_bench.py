#!/usr/bin/env python3
"""What the audio watermark costs per request (include/vits_watermark.h), and that a call without the flag is the call it was: host
wall time of vits_synthesize_pcm16 for the c2 request (1 x 50 tokens) and the c3 batch (32 ragged utterances, independent items) plain
and with watermark=KEY, alone and next to a loudness target (where the stage is no longer the last one); and the detector alone through
vits_op_watermark_detect on 3 s and 60 s of audio.  Where the build has the payload (include/vits_watermark_payload.h): the marked request
and batch with a payload (the batch: one per item) next to the plain mark, and the reader (vits_op_watermark_read) next to the detector on
the same 3 s and 60 s.  Synthetic default-size weights.
Every call ends in the engine's own stream synchronise and the copy to the host, so the clock brackets finished work.  The legs are
timed in alternation (`--rounds` times `--calls` calls each) so that drift of the machine hits them alike, and the plain leg runs
twice per round: the difference of its two medians is the spread every other difference has to be read against.  The figure is the
median over rounds of the mean call.  The door's figure includes its upload, its allocation and its download: an upper bound for the
kernels.

    python tools/watermark_bench.py --out profiles/watermark_bench.txt
    VITS_MI355_LIB=/path/to/the/parent/libvits_mi355.so python tools/watermark_bench.py --label parent --out profiles/watermark_bench.txt
    python tools/watermark_bench.py --identity --out profiles/watermark_identity.txt

The second form times the legs the other build has (the parent commit's has no watermark) in the same visit.  The third prints SHA-256
digests of the paths that carry no watermark flag -- vits_op_denoise, whose device functions and tables the stage shares, a plain, a
resampled, a normalised, a shifted and a contoured toy-voice request, float and int16, and a document -- on fixed seeded inputs: run on
both builds they must be equal, since tail_run now has a stage between the resampler and the normalisation.

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
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCALES = np.array([0.667, 1.0, 0.8], np.float32)
KEY = 0x5EED1234
LOUD = (1, -23.0, 0.0)  # capi.loudness_spec(loudness=-23, peak_ceiling=0)


def workloads(n_vocab):
    rng = np.random.default_rng(0)
    lens = np.linspace(20, 200, 32).astype(np.int64)
    ids = np.zeros((32, 200), np.int64)
    for b, n in enumerate(lens):
        ids[b, :n] = rng.integers(1, n_vocab, size=n)
    return {"c2 (1 x 50 tokens)": dict(ids=rng.integers(1, n_vocab, size=(1, 50)).astype(np.int64), lens=np.array([50], np.int64), solo=False),
            "c3 (32 x 20..200 tokens)": dict(ids=ids, lens=lens, solo=True)}


def call(model, w, leg):
    B = w["ids"].shape[0]
    kw = {}
    if "watermark" in leg:
        kw["watermark"] = KEY
    if "payload" in leg:  # (one per item: the array of a coalesced batch)
        kw["watermark_payload"] = 0xBEEF if B == 1 else [(0xBEEF + 257 * b) & 0xFFFF for b in range(B)]
    if "loudness" in leg:
        kw["loudness"] = LOUD
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
    bias = rng.uniform(0.5, 1.5, 513).astype(np.float32)
    lines = [f"  op_denoise n = 1024       {sha(lib.op_denoise(x, lens, bias, 2.0, 1024))}"]
    hp = W.tiny_hparams()
    model = lib.create(W.synthetic_blob(hp, 1234), 0)
    ids = np.random.default_rng(21).integers(1, 20, size=(3, 24)).astype(np.int64)
    ln = np.array([24, 15, 5], np.int64)
    sid = np.array([1, 2, 0], np.int64)
    tp = np.zeros((3, 24), np.float32)
    tp[:, 3:9] = 4.0
    for name, B in (("one utterance", 1), ("solo batch of 3", 3)):
        a = (ids[:B], ln[:B], SCALES, sid[:B])
        kw = dict(seed=3, solo=B > 1)
        lines.append(f"  {name}: plain, float       {sha(model.synthesize(*a, **kw)[0])}")
        lines.append(f"  {name}: plain, int16       {sha(model.synthesize_pcm16(*a, **kw)[0])}")
        lines.append(f"  {name}: 8000 Hz, float     {sha(model.synthesize(*a, sample_rate=8000, **kw)[0])}")
        lines.append(f"  {name}: 8000 Hz, int16     {sha(model.synthesize_pcm16(*a, sample_rate=8000, **kw)[0])}")
        lines.append(f"  {name}: -23 LUFS, float    {sha(model.synthesize(*a, loudness=LOUD, **kw)[0])}")
        lines.append(f"  {name}: -23 LUFS at 8000   {sha(model.synthesize_pcm16(*a, loudness=LOUD, sample_rate=8000, **kw)[0])}")
        lines.append(f"  {name}: pitch=+3, int16    {sha(model.synthesize_pcm16(*a, pitch=3.0, **kw)[0])}")
        lines.append(f"  {name}: contoured, int16   {sha(model.synthesize_pcm16(*a, token_pitch=tp[:B], **kw)[0])}")
    doc = (ids, ln, SCALES, sid)
    lines.append(f"  document, float                {sha(model.synthesize_document(*doc, seed=3, gap_frames=[2, 0, 1], fade_samples=9)[0])}")
    lines.append(f"  document, int16 at 8000        {sha(model.synthesize_document(*doc, seed=3, gap_frames=[2, 0, 1], pcm=True, sample_rate=8000)[0])}")
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
        sys.exit("watermark_bench: no GPU: a timing needs one")
    path = os.path.relpath(lib.path, ROOT) if os.path.abspath(lib.path).startswith(ROOT + os.sep) else lib.path
    head = f"commit {commit()}  library {path}  {args.label}".rstrip()
    if args.identity:
        lines = [f"watermark_identity  {head}"] + identity(lib, W)
    else:
        hp = W.default_hparams()
        model = lib.create(W.synthetic_blob(hp, 1234), 0)
        has = getattr(lib, "has_watermark", False)
        has_payload = getattr(lib, "has_watermark_payload", False)
        legs = (["plain", "plain again"] + (["watermark"] if has else []) + (["watermark + payload"] if has_payload else []) + ["loudness"] +
                (["loudness + watermark"] if has else []))
        lines = [f"watermark_bench  {head}",
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
                lines.append(f"  {name}  {leg:>20}  {med:8.4f} ms  (min {min(per[leg]):.4f}, max {max(per[leg]):.4f})  {med - base:+.4f} ms vs plain")
        if has:  # the detector alone, on 3 s and 60 s of the marked test signal
            import watermark_ref as R

            x3 = R.embed(R.voiced_signal(3.0), KEY).astype(np.float32)
            for name, x in (("3 s", x3), ("60 s", np.tile(x3[:65536], 21)[:60 * 22050])):  # (whole pattern periods, so the tiling keeps the mark)
                for _ in range(args.warmup):
                    z, off, rows, _ = lib.op_watermark_detect(x[None], [x.shape[0]], KEY)
                per = []
                for _ in range(args.rounds):
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        lib.op_watermark_detect(x[None], [x.shape[0]], KEY)
                    per.append((time.perf_counter() - t0) / args.calls * 1e3)
                lines.append(f"  op_watermark_detect {name:>5}  {statistics.median(per):8.4f} ms  (min {min(per):.4f}, max {max(per):.4f})  "
                             f"z {z[0]:.2f} offset {off[0]} rows {rows[0]}, door with its copies")
        if has_payload:  # the reader next to the detector, on 3 s and 60 s of the test signal marked with a payload at 2 dB, rounds alternated
            import watermark_payload_ref as P

            x3 = P.embed(R.voiced_signal(3.0), KEY, 0xBEEF, 2.0).astype(np.float32)
            for name, x in (("3 s", x3), ("60 s", np.tile(x3[:65536], 21)[:60 * 22050])):
                doors = {"op_watermark_read": lib.op_watermark_read, "op_watermark_detect": lib.op_watermark_detect}
                for fn in doors.values():
                    for _ in range(args.warmup):
                        fn(x[None], [x.shape[0]], KEY)
                per = {k: [] for k in doors}
                for _ in range(args.rounds):
                    for k, fn in doors.items():
                        t0 = time.perf_counter()
                        for _ in range(args.calls):
                            fn(x[None], [x.shape[0]], KEY)
                        per[k].append((time.perf_counter() - t0) / args.calls * 1e3)
                z, off, rows, payload, valid, _, bit_z = lib.op_watermark_read(x[None], [x.shape[0]], KEY)
                zd = lib.op_watermark_detect(x[None], [x.shape[0]], KEY)[0]
                for k in doors:
                    what = (f"z {z[0]:.2f} offset {off[0]} rows {rows[0]} payload {int(payload[0]):#06x} valid {valid[0]} min |z_i| {np.abs(bit_z[0]).min():.2f}"
                            if k == "op_watermark_read" else f"z {zd[0]:.2f} on the payload mark")
                    lines.append(f"  {k:>19} {name:>5}  {statistics.median(per[k]):8.4f} ms  (min {min(per[k]):.4f}, max {max(per[k]):.4f})  {what}, door with its copies")
        model.close()
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
