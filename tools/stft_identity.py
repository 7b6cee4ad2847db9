#!/usr/bin/env python3
"""That a build computes the output tail (the frame transform of csrc/stft.hip.h and every stage that takes the batch descriptor of
csrc/ragged.hip.h) bit for bit as another does: one SHA-256 per line over fixed seeded inputs, for every door of a tail stage and for the
tail end to end.

    python tools/stft_identity.py --out profiles/stft_frames_identity.txt
    VITS_MI355_LIB=/path/to/the/other/libvits_mi355.so python tools/stft_identity.py --label parent --out profiles/stft_frames_identity.txt

Doors: vits_op_denoise at the five filter lengths; the pitch doors (shift, stretch, their formant forms, the formant gain) at +3 and -12
semitones; vits_op_contour / _stretch; vits_op_intonation / _stretch; vits_op_watermark / _detect / _payload / _read; vits_op_resample down and
up; vits_op_loudness / _normalize; vits_op_true_peak; vits_op_limit in both modes; vits_op_loudness_limit.  One padded batch of four items of
400 samples (no frame), 513 (F_s of 2 or 3 at -12), 5000 and 22050; the denoiser's door refuses an item below n/2 + 1 samples, so its
first item is that long.  The pitch and contour doors once more on six items of up to 2,000,000 samples, which their runners must split
into groups (the group counts, from the scratch formulas of csrc/pitch.hip.h and csrc/contour.hip.h, are on the line).  End to end, on
the tiny voice as float and as int16: plain, 8000 Hz, -23 LUFS, the limiter, pitch, a contour, the watermark, every stage at once, a
two-item document; and on the toy multistream voice a denoised utterance in one call and streamed.

A helper, not a gate: it prints, the reader compares the two listings.
"""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALES = np.array([0.667, 1.0, 0.8], np.float32)
KEY = 0x5EED1234
PAYLOADS = (0xBEEF, 0x0000, 0xFFFF, 0x1234)  # one per item of the doors' batch
LOUD = (1, -23.0, 0.0)  # capi.loudness_spec(loudness=-23, peak_ceiling=0)
LENGTHS = np.array([400, 513, 5000, 22050], np.int64)
RATE = 22050


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown (not a git checkout)"


def signal():
    """four voiced items (harmonics of 110 .. 170 Hz with a slow glide, so that the F0 tracker has a track) plus noise, zero beyond each length"""
    rng = np.random.default_rng(31)
    N = int(LENGTHS.max())
    t = np.arange(N) / RATE
    x = np.zeros((len(LENGTHS), N), np.float32)
    for b, n in enumerate(LENGTHS):
        f0 = (110.0 + 20.0 * b) * (1.0 + 0.2 * np.sin(2 * np.pi * 1.5 * t))
        ph = 2 * np.pi * np.cumsum(f0) / RATE
        v = sum(np.sin(h * ph) / h for h in range(1, 9))
        x[b, :n] = (0.1 * v + 0.01 * rng.standard_normal(N))[:n].astype(np.float32)
    return x


def pv_groups(lengths, item_bytes, limit=512 << 20):
    """the groups of consecutive items pv_run (csrc/pitch.hip.h) forms: how many"""
    n, b0 = 0, 0
    while b0 < len(lengths):
        mx, c = 0, 0
        while b0 + c < len(lengths) and item_bytes(max(mx, int(lengths[b0 + c]))) * (c + 1) <= limit:
            mx, c = max(mx, int(lengths[b0 + c])), c + 1
        assert c, "an item fits no group"
        n, b0 = n + 1, b0 + c
    return n


def pitch_item_bytes(n, P, Q):
    fa = 1 + n // 256 if n >= 513 else 0
    fs = ((fa + 1) * P + Q - 1) // Q if fa else 0
    return (fa + 2) * 513 * 8 + fs * 513 * 4 + fs * 1024 * 4 + (fs - 1) * 256 * 4 + 8 + 64 if fa else 8


def contour_item_bytes(n):
    fa, f = (1 + n // 256 if n >= 513 else 0), 1 + n // 256
    cap = 2 * (fa + 1)
    return (f + 1) * 12 + (cap + 2) * 8 + 64 + ((fa + 2) * 513 * 8 + cap * 513 * 4 + cap * 1024 * 4 + (cap - 1) * 256 * 4 if fa else 0)


def grouped(lib):
    """the pitch and contour doors on a batch their runners split: six items of up to 2,000,000 samples"""
    ln = np.array([2_000_000, 1_999_000, 1_500_000, 2_000_000, 1_800_001, 1_234_567], np.int64)
    rng = np.random.default_rng(33)
    N = int(ln.max())
    t = np.arange(N, dtype=np.float64) / RATE
    x = np.zeros((len(ln), N), np.float32)
    for b, n in enumerate(ln):
        x[b, :n] = (0.2 * np.sin(2 * np.pi * (120.0 + 15.0 * b) * t) + 0.02 * rng.standard_normal(N))[:n].astype(np.float32)
    P, Q = lib.pitch_plan(3.0)
    gp, gc = pv_groups(ln, lambda n: pitch_item_bytes(n, P, Q)), pv_groups(ln, contour_item_bytes)
    Tx = 8
    cum = np.stack([np.maximum(1, (np.arange(1, Tx + 1) * f) // Tx) for f in (ln + 255) // 256]).astype(np.int32)
    tl = np.full(len(ln), Tx, np.int64)
    semi = np.tile(np.array([0, 2, 4, 7, 0, -3, -12, 0], np.float32), (len(ln), 1))
    gain = np.tile(np.array([0, 0, 3, 3, -6, -6, 0, 0], np.float32), (len(ln), 1))
    return [f"  op_pitch_shift +3, 6 x 2e6 samples, {gp} groups        {sha(lib.op_pitch_shift(x, ln, 3.0))}",
            f"  op_contour, 6 x 2e6 samples, {gc} groups              {sha(lib.op_contour(x, ln, cum, tl, 256, semi, gain))}"]


def doors(lib):
    x = signal()
    B, N = x.shape
    rng = np.random.default_rng(32)
    lines = []
    for n in (64, 128, 256, 512, 1024):
        ln = np.maximum(LENGTHS, n // 2 + 1)
        xd = (0.2 * rng.standard_normal((B, N))).astype(np.float32)
        bias = rng.uniform(0.5, 1.5, n // 2 + 1).astype(np.float32)
        strength = float(np.float32(0.83 * 0.2 * np.sqrt(3 * n / 8)))  # about half of the bins under the threshold
        lines.append(f"  op_denoise n = {n:<4}                                {sha(lib.op_denoise(xd, ln, bias, strength, n))}")
    for st in (3.0, -12.0):
        lines.append(f"  op_pitch_shift {st:+.0f}                                 {sha(lib.op_pitch_shift(x, LENGTHS, st))}")
        lines.append(f"  op_pitch_stretch {st:+.0f}                               {sha(lib.op_pitch_stretch(x, LENGTHS, st))}")
        lines.append(f"  op_pitch_shift_formant {st:+.0f}                         {sha(lib.op_pitch_shift_formant(x, LENGTHS, st))}")
        lines.append(f"  op_pitch_stretch_formant {st:+.0f}                       {sha(lib.op_pitch_stretch_formant(x, LENGTHS, st))}")
        lines.append(f"  op_pitch_formant_gain {st:+.0f}                          {sha(lib.op_pitch_formant_gain(x, LENGTHS, st))}")
    # eight tokens per item, their frames (hop 256) spread over the item; a rise, a fall and a gain step
    Tx = 8
    frames = (LENGTHS + 255) // 256
    cum = np.stack([np.maximum(1, (np.arange(1, Tx + 1) * f) // Tx) for f in frames]).astype(np.int32)
    tl = np.full(B, Tx, np.int64)
    semi = np.tile(np.array([0, 2, 4, 7, 0, -3, -12, 0], np.float32), (B, 1))
    gain = np.tile(np.array([0, 0, 3, 3, -6, -6, 0, 0], np.float32), (B, 1))
    lines.append(f"  op_contour                                        {sha(lib.op_contour(x, LENGTHS, cum, tl, 256, semi, gain))}")
    lines.append(f"  op_contour_stretch                                {sha(*lib.op_contour_stretch(x, LENGTHS, cum, tl, 256, semi, gain))}")
    lines.append(f"  op_intonation r = 1.8                             {sha(lib.op_intonation(x, LENGTHS, RATE, 1.8))}")
    lines.append(f"  op_intonation r = 0.5 with tokens                 {sha(lib.op_intonation(x, LENGTHS, RATE, 0.5, cum, tl, 256, semi, gain))}")
    lines.append(f"  op_intonation_stretch r = 1.8                     {sha(*lib.op_intonation_stretch(x, LENGTHS, RATE, 1.8))}")
    y = lib.op_watermark(x, LENGTHS, KEY)
    lines.append(f"  op_watermark                                      {sha(y)}")
    lines.append(f"  op_watermark 2 dB                                 {sha(lib.op_watermark(x, LENGTHS, KEY, 2.0))}")
    lines.append(f"  op_watermark_detect                               {sha(*lib.op_watermark_detect(y, LENGTHS, KEY))}")
    if getattr(lib, "has_watermark_payload", False):  # (include/vits_watermark_payload.h; a build from before it lists the doors above only)
        yp = lib.op_watermark_payload(x, LENGTHS, KEY, PAYLOADS)
        lines.append(f"  op_watermark_payload                              {sha(yp)}")
        lines.append(f"  op_watermark_read                                 {sha(*lib.op_watermark_read(yp, LENGTHS, KEY))}")
    for ro in (8000, 48000):
        lines.append(f"  op_resample {RATE} -> {ro:<5}                        {sha(lib.op_resample(x, LENGTHS, RATE, ro))}")
    lines.append(f"  op_loudness                                       {sha(*lib.op_loudness(x, LENGTHS, RATE))}")
    lines.append(f"  op_loudness_normalize -23 LUFS                    {sha(*lib.op_loudness_normalize(x, LENGTHS, RATE, 1, -23.0))}")
    lines.append(f"  op_true_peak                                      {sha(lib.op_true_peak(x, LENGTHS, RATE))}")
    for mode, name in ((1, "sample"), (2, "true")):
        lines.append(f"  op_limit {name:<6} ceiling 0.05                       {sha(*lib.op_limit(x, LENGTHS, RATE, mode, 0.05))}")
    lines.append(f"  op_loudness_limit -23 LUFS, true, 0.05            {sha(*lib.op_loudness_limit(x, LENGTHS, RATE, -23.0, 2, 0.05))}")
    return lines + grouped(lib)


def tail(lib, W):
    from vosk_tts_amd.capi import limit_spec

    model = lib.create(W.synthetic_blob(W.tiny_hparams(), 1234), 0)
    ids = np.random.default_rng(21).integers(1, 20, size=(2, 24)).astype(np.int64)
    ln = np.array([24, 15], np.int64)
    sid = np.array([1, 2], np.int64)
    tp = np.zeros((2, 24), np.float32)
    tp[:, 3:9] = 4.0
    legs = (("plain", {}), ("8000 Hz", dict(sample_rate=8000)), ("-23 LUFS", dict(loudness=LOUD)),
            ("limiter", dict(loudness=LOUD, limit=limit_spec("true", 0.05))), ("pitch +3", dict(pitch=3.0)), ("pitch -5 formant", dict(pitch=-5.0, preserve_formants=True)),
            ("contour", dict(token_pitch=tp)), ("watermark", dict(watermark=KEY)), ("watermark -23 LUFS 8000 Hz", dict(watermark=KEY, loudness=LOUD, sample_rate=8000)))
    lines = []
    for name, kw in legs:
        a = (ids, ln, SCALES, sid)
        lines.append(f"  tiny voice, {name + ', float':<38}{sha(model.synthesize(*a, seed=3, solo=True, **kw)[0])}")
        lines.append(f"  tiny voice, {name + ', int16':<38}{sha(model.synthesize_pcm16(*a, seed=3, solo=True, **kw)[0])}")
    doc = (ids, ln, SCALES, sid)
    every = dict(sample_rate=8000, token_pitch=tp, watermark=KEY, loudness=LOUD, limit=limit_spec("true", 0.05))
    lines.append(f"  tiny voice, {'every stage at once, int16':<38}{sha(model.synthesize_pcm16(ids, ln, SCALES, sid, seed=3, solo=True, **every)[0])}")
    lines.append(f"  tiny voice, document, float                       {sha(model.synthesize_document(*doc, seed=3, gap_frames=[2, 1], fade_samples=9)[0])}")
    lines.append(f"  tiny voice, document, watermark, int16            {sha(model.synthesize_document(*doc, seed=3, gap_frames=[2, 1], pcm=True, watermark=KEY)[0])}")
    model.close()
    return lines


def stream():
    from vosk_tts_amd import Model
    from vosk_tts_amd.toymodel import write_toy_multistream_model

    with tempfile.TemporaryDirectory() as d:
        write_toy_multistream_model(d)
        voice = Model(model_path=d, device=0)
        try:
            m = voice.onnx._model
            ids = np.random.default_rng(21).integers(1, 40, size=(5, 53)).astype(np.int64)
            pde = np.ones(53, np.float32)
            lines = []
            for n in (256, 1024):
                one = m.synthesize(ids, SCALES, 2, None, pde, seed=9, denoiser_strength=1.5, denoiser_filter_length=n)[0]
                parts = list(m.stream(ids, SCALES, 2, None, pde, seed=9, chunk_frames=8, denoiser_strength=1.5, denoiser_filter_length=n))
                lines.append(f"  multistream voice, denoised n = {n:<4}, one call  {sha(one)}")
                lines.append(f"  multistream voice, denoised n = {n:<4}, streamed  {sha(np.concatenate(parts))}")
            return lines
        finally:
            voice.onnx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--label", default="", help="a word for the header (e.g. which build this is)")
    ap.add_argument("--out", default=None, help="append the listing to this file")
    args = ap.parse_args()

    from vosk_tts_amd import weights as W
    from vosk_tts_amd.capi import VitsLib

    lib = VitsLib()
    if not lib.is_device or lib.device_count() < 1:
        sys.exit("stft_identity: no GPU")
    path = os.path.relpath(lib.path, ROOT) if os.path.abspath(lib.path).startswith(ROOT + os.sep) else lib.path
    lines = [f"stft_identity  commit {commit()}  library {path}  {args.label}".rstrip()] + doors(lib) + tail(lib, W) + stream()
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
