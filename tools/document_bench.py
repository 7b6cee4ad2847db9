#!/usr/bin/env python3
"""What a document costs (include/vits_document.h) against what a caller does without it, and that the calls which are no document are
the calls they were.  Toy voice (synthetic default-size weights), 8 and 32 sentences of 20 - 200 tokens, every leg timed in alternation
in one process (`--rounds` times `--calls` calls each; the figure is the median over rounds of the mean call; "batch again" is the same
leg as "batch + host join" and shows the spread the differences have to be read against):

    document        vits_synthesize_document_pcm16: one call, one int16 row back (sentence pause 17 frames, 2 ms fades)
    batch + host    what a caller does today on this same commit: vits_synthesize_pcm16 of the same batch (SOLO), then the rows cut at
                    their lengths and concatenated with the same silences by NumPy on the host; with it the bytes each form copies
                    back (the batch returns B padded rows) and the eager launches of each form behind the decoder
    one utterance   the whole text as one utterance (the same tokens in one row; refused or not, the report says which)
    single / batch  the plain single request (1 x 50 tokens) and the plain batch: the legs another build has too

    python tools/document_bench.py --out profiles/document_bench.txt
    VITS_MI355_LIB=/path/to/the/parent/libvits_mi355.so python tools/document_bench.py --label parent --out profiles/document_bench.txt
    python tools/document_bench.py --identity --out profiles/document_identity.txt
    python tools/document_bench.py --no-document --label "document leg left out" --out profiles/document_bench.txt

The second form times the legs the other build has (the parent commit's has no document) in the same visit; the fourth times this
build's legs in a process that never makes a document call, for the same comparison.  The third prints SHA-256
digests of the paths that are no document -- plain and SOLO batches at float and int16, another rate, a loudness target with a limiter,
a pitch shift, a contour -- on fixed seeded inputs: run on both builds they must be equal, since tail_run and both synthesize paths now
carry the join.

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
GAP, FADE = 17, 44  # 0.2 s of frames and 2 ms of samples at 22050 Hz / hop 256


def sentences(B, n_vocab):
    rng = np.random.default_rng(B)
    lens = np.linspace(20, 200, B).astype(np.int64)
    ids = np.zeros((B, 200), np.int64)
    for b, n in enumerate(lens):
        ids[b, :n] = rng.integers(1, n_vocab, size=n)
    return ids, lens, np.arange(B, dtype=np.int64) % 7


def host_join(pcm, ol, hop):
    gap = np.zeros(GAP * hop, np.int16)
    return np.concatenate([p for b in range(pcm.shape[0]) for p in (pcm[b, :int(ol[b])], gap)])


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return ""


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def identity(lib, W):
    from vosk_tts_amd.capi import limit_spec, loudness_spec

    hp = W.tiny_hparams()
    model = lib.create(W.synthetic_blob(hp, 1234), 0)
    rng = np.random.default_rng(21)
    ids = rng.integers(1, 20, size=(3, 24)).astype(np.int64)
    lens, sid = np.array([24, 15, 5], np.int64), np.array([0, 1, 0], np.int64)
    tp = np.zeros((3, 24), np.float32)
    tp[1, 3:9] = 4.0
    spec, lim = loudness_spec(loudness=-19.0, peak_ceiling=0.0), limit_spec("true", 0.9)
    lines = []
    for fast in (1, 0):
        lib.lib.vits_debug_fast_path(fast)
        tag = "fast " if fast else "eager"
        lines += [f"  {tag} single request, float     {sha(model.synthesize(ids[:1], lens[:1], SCALES, sid[:1], seed=3)[0])}",
                  f"  {tag} single request, int16     {sha(model.synthesize_pcm16(ids[:1], lens[:1], SCALES, sid[:1], seed=3)[0])}",
                  f"  {tag} padded batch, float       {sha(model.synthesize(ids, lens, SCALES, sid, seed=3)[0])}",
                  f"  {tag} SOLO batch, float         {sha(model.synthesize(ids, lens, SCALES, sid, seed=3, solo=True)[0])}",
                  f"  {tag} SOLO batch, int16         {sha(model.synthesize_pcm16(ids, lens, SCALES, sid, seed=3, solo=True)[0])}",
                  f"  {tag} SOLO batch, 8000 Hz int16 {sha(model.synthesize_pcm16(ids, lens, SCALES, sid, seed=3, solo=True, sample_rate=8000)[0])}",
                  f"  {tag} SOLO batch, LUFS + limit  {sha(model.synthesize(ids, lens, SCALES, sid, seed=3, solo=True, loudness=spec, limit=lim)[0])}",
                  f"  {tag} SOLO batch, pitch=+2      {sha(model.synthesize(ids, lens, SCALES, sid, seed=3, solo=True, pitch=2.0)[0])}",
                  f"  {tag} SOLO batch, contour int16 {sha(model.synthesize_pcm16(ids, lens, SCALES, sid, seed=3, solo=True, token_pitch=tp)[0])}",
                  f"  {tag} SOLO batch, marks         {sha(model.synthesize(ids, lens, SCALES, sid, seed=3, solo=True, marks=True, sample_rate=8000)[2])}"]
    lib.lib.vits_debug_fast_path(1)
    model.close()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=6, help="calls per leg per round")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--one-utterance-max-tokens", type=int, default=1200, help="the whole text as one utterance is timed up to this length")
    ap.add_argument("--sizes", type=int, nargs="+", default=[8, 32], help="sentences per document")
    ap.add_argument("--no-document", action="store_true", help="leave the document leg out (what the other legs cost in a process without it)")
    ap.add_argument("--identity", action="store_true", help="no timing: the digests of the paths that are no document")
    ap.add_argument("--label", default="", help="a word for the header (e.g. which build this is)")
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()

    from vosk_tts_amd import weights as W
    from vosk_tts_amd.capi import VitsError, VitsLib

    lib = VitsLib()
    if not lib.is_device or lib.device_count() < 1:
        sys.exit("document_bench: no GPU: a timing needs one")
    path = os.path.relpath(lib.path, ROOT) if os.path.abspath(lib.path).startswith(ROOT + os.sep) else lib.path
    if os.environ.get("VITS_MI355_LIB"):
        path = "(VITS_MI355_LIB) " + os.path.basename(lib.path)
    head = "  ".join(v for v in (f"commit {commit()}" if commit() else "", f"library {path}", args.label) if v)
    if args.identity:
        lines = [f"document_identity  {head}"] + identity(lib, W)
    else:
        hp = W.default_hparams()
        hop = hp.hop_length
        model = lib.create(W.synthetic_blob(hp, 1234), 0)
        has = getattr(lib, "has_document", False) and not args.no_document
        lines = [f"document_bench  {head}",
                 f"host wall time per call (ms): median over {args.rounds} rounds of the mean of {args.calls} calls, legs alternated"]
        one = sentences(1, hp.n_vocab)
        one = (one[0][:, :50], np.array([50], np.int64), one[2])
        for B in args.sizes:
            ids, lens, sid = sentences(B, hp.n_vocab)
            whole = np.concatenate([ids[b, :lens[b]] for b in range(B)])[None]
            legs = {"single (1 x 50)": lambda: model.synthesize_pcm16(one[0], one[1], SCALES, one[2], seed=1),
                    "batch": lambda: model.synthesize_pcm16(ids, lens, SCALES, sid, seed=1, solo=True),
                    "batch + host join": lambda: host_join(*model.synthesize_pcm16(ids, lens, SCALES, sid, seed=1, solo=True), hop),
                    "batch again": lambda: host_join(*model.synthesize_pcm16(ids, lens, SCALES, sid, seed=1, solo=True), hop)}
            if has:
                legs["document"] = lambda: model.synthesize_document(ids, lens, SCALES, sid, pcm=True, seed=1, gap_frames=GAP, fade_samples=FADE)
            if whole.shape[1] > args.one_utterance_max_tokens:
                lines.append(f"  {B:2d} sentences  one utterance of {whole.shape[1]} tokens: not measured (above --one-utterance-max-tokens "
                             f"{args.one_utterance_max_tokens})")
            else:
                try:  # the whole text as one utterance
                    model.synthesize_pcm16(whole, [whole.shape[1]], SCALES, sid[:1], seed=1)
                    legs["one utterance"] = lambda: model.synthesize_pcm16(whole, [whole.shape[1]], SCALES, sid[:1], seed=1)
                except VitsError as e:
                    lines.append(f"  {B:2d} sentences  one utterance of {whole.shape[1]} tokens: refused ({e})")
            for fn in legs.values():
                for _ in range(args.warmup):
                    fn()
            per = {leg: [] for leg in legs}
            for _ in range(args.rounds):
                for leg, fn in legs.items():
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        fn()
                    per[leg].append((time.perf_counter() - t0) / args.calls * 1e3)
            base = statistics.median(per["batch + host join"])
            pcm, ol = model.synthesize_pcm16(ids, lens, SCALES, sid, seed=1, solo=True)
            sec = float(ol.sum() + B * GAP * hop) / hp.sampling_rate
            for leg in legs:
                med = statistics.median(per[leg])
                note = f"  {sec / (med / 1e3):8.0f} x real time" if leg in ("document", "batch + host join") else ""
                lines.append(f"  {B:2d} sentences  {leg:>18}  {med:9.4f} ms  (min {min(per[leg]):.4f}, max {max(per[leg]):.4f})  "
                             f"{med - base:+.4f} ms vs batch + host join{note}")
            lines.append(f"  {B:2d} sentences  bytes copied back: batch {pcm.nbytes} (B padded int16 rows)" +
                         (f", document {model.synthesize_document(ids, lens, SCALES, sid, pcm=True, seed=1, gap_frames=GAP, fade_samples=FADE)[0].nbytes}"
                          " (one int16 row)" if has else ""))
            if has:  # the eager launches of each form (the fast path replays its graphs, which the log does not count one by one)
                lib.lib.vits_debug_fast_path(0)
                counts = {}
                for leg in ("batch", "document"):
                    lib.launch_log(1)
                    legs[leg]()
                    lib.launch_log(0)
                    counts[leg] = sum(lib.launch_dump().values())
                lib.lib.vits_debug_fast_path(1)
                lines.append(f"  {B:2d} sentences  eager launches: batch {counts['batch']}, document {counts['document']}")
        model.close()
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
