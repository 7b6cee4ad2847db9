#!/usr/bin/env python3
"""The BERT front end of a batch of requests, serial against batched (rubert-base geometry, synthetic weights, 32 sentences of 8 - 40
tokens from fixed seeds), for the first B = 1, 2, 4, 8, 16, 32 sentences:

  solo    B stts_bert_encode calls, one per sentence, as the per-request front end makes them (graph replay included)  -- the baseline
  batch   one stts_bert_encode_batch
  host    the whole per-request pipeline of the batch door: encode, keep the word rows, fan out to the phonemes (a Python list of
          768-vectors), np.transpose(np.array(...)), pad into [B, 768, T]
  feed    one stts_bert_feed_batch for the same rows -> [B, 768, T]

All four in one process on one model, alternating inside every repetition; every call ends in a device synchronise, so a host clock
around it times the call.  Medians, with the 10th / 90th percentile to show the spread.  Results are compared before they are timed.
    python tools/bert_batch_bench.py [--reps 60] [--out profiles/bert_batch_bench.txt] [--head <git head>]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (one HIP runtime per process: before the product library, as tests/conftest.py does)

from vosk_tts_amd import weights_bert as BW  # noqa: E402
from vosk_tts_amd.capi import VitsLib  # noqa: E402
from vosk_tts_amd.capi_stts import BertEncoder  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bert_batch_bench.txt"))
ap.add_argument("--head", default=None)
args = ap.parse_args()

head = args.head
if head is None:
    try:
        head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:  # noqa: BLE001
        head = "unknown (not a git checkout)"

hp = BW.base_hparams(1000)
enc = BertEncoder(VitsLib(), BW.synthetic_blob(hp, 7))
rng = np.random.default_rng(20)
lens = rng.integers(8, 41, size=32)
sent = [rng.integers(0, hp.vocab_size, size=int(L)).astype(np.int64) for L in lens]
# a front end's row map: [CLS], words of 1 - 3 word pieces (the first piece stands for the word), [SEP]; 1 - 6 phonemes per word with the
# interspersed blank of g2p (every phoneme twice), '^' on row 0 and '$' on the last row
word_rows, rows = [], []
for L in lens:
    first = [0]
    t = 1
    while t < L - 1:
        first.append(t)
        t += int(rng.integers(1, 4))
    first.append(int(L) - 1)
    wr = np.array(first, np.int32)
    words = [0] + [w for w in range(1, len(wr) - 1) for _ in range(2 * int(rng.integers(1, 7)))] + [len(wr) - 1] * 2
    word_rows.append(wr)
    rows.append(np.array(words, np.int64))


def solo(B):
    return [enc.encode(sent[b]) for b in range(B)]


def batch(B):
    return enc.encode_batch(sent[:B])


def host(B):
    fronts = []
    for b in range(B):
        bert = enc.encode(sent[b])[word_rows[b]]
        emb = [bert[w] for w in rows[b]]
        fronts.append(np.transpose(np.array(emb, np.float32)))
    T = max(f.shape[1] for f in fronts)
    out = np.zeros((B, hp.hidden, T), np.float32)
    for b, f in enumerate(fronts):
        out[b, :, :f.shape[1]] = f
    return out


def feed(B):
    return enc.feed_batch(sent[:B], [word_rows[b][rows[b]] for b in range(B)])


lines = [f"bert_batch_bench: git head {head}; {torch.cuda.get_device_name(0) if torch.cuda.is_available() else 'no GPU'}",
         f"rubert-base geometry ({hp.out_layers} of {hp.n_layers} layers run), 32 sentences of {lens.min()}-{lens.max()} tokens "
         f"(sum {lens.sum()}), feeds of {min(len(r) for r in rows)}-{max(len(r) for r in rows)} phonemes; {args.reps} repetitions, "
         "the four forms alternating; ms per batch: median [p10 .. p90]",
         f"{'B':>3} {'tokens':>6} | {'solo (baseline)':>24} | {'batch':>24} | solo/batch | {'host pipeline':>24} | {'feed':>24} | host/feed | max rel diff"]
for B in (1, 2, 4, 8, 16, 32):
    s, bt, h, f = solo(B), batch(B), host(B), feed(B)  # (also the warm-up of every shape: graphs captured, workspaces laid out)
    scale = max(np.abs(a).max() for a in s)
    diff = max(max(np.abs(a - c).max() for a, c in zip(s, bt)), np.abs(h - f).max()) / scale
    for _ in range(5):
        solo(B), batch(B), host(B), feed(B)
    times = {k: [] for k in ("solo", "batch", "host", "feed")}
    for _ in range(args.reps):
        for k, fn in (("solo", solo), ("batch", batch), ("host", host), ("feed", feed)):
            t0 = time.perf_counter()
            fn(B)
            times[k].append((time.perf_counter() - t0) * 1e3)

    def fmt(k):
        a = np.array(times[k])
        return f"{np.median(a):7.3f} [{np.percentile(a, 10):6.3f} .. {np.percentile(a, 90):6.3f}]"

    med = {k: float(np.median(times[k])) for k in times}
    lines.append(f"{B:>3} {int(lens[:B].sum()):>6} | {fmt('solo'):>24} | {fmt('batch'):>24} | {med['solo'] / med['batch']:>9.2f}x | {fmt('host'):>24} | "
                 f"{fmt('feed'):>24} | {med['host'] / med['feed']:>8.2f}x | {diff:.2e}")
    print(lines[-1], flush=True)
enc.close()
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write(text)
