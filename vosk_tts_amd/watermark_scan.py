"""Watermark localisation (include/vits_watermark_scan.h): from the windowed detector scores of VitsLib.op_watermark_scan to the marked
segments of a recording.  The scores come from the device; what is here is host work on a [128, W] array per item: the derived
threshold, the nominal sample range of a window, and the grouping of the windows over the threshold into segments.  Checked against
tests/watermark_scan_ref.py."""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from .capi import WATERMARK_OFFSETS, WATERMARK_PERIOD_SAMPLES, WATERMARK_SCAN_DEFAULT_SPAN, WATERMARK_SCAN_MAX_SPAN

DETECT_HOP = 128  # VITS_WATERMARK_DETECT_HOP: samples per offset index


@dataclass
class WatermarkSegment:
    """One marked stretch of a recording: samples [start, end) (the union of the nominal ranges of its windows, so each end is good to
    about a span of periods), z of its best window, offset_samples = 128 o of that window (how far into the 16384-sample pattern the
    recording starts, as detect_watermark reports it).  payload / bit_z: filled by Synth.locate_watermark(payload=True)."""

    start: int
    end: int
    z: float
    offset_samples: int
    payload: Optional[int] = None
    bit_z: Optional[np.ndarray] = None


def span_arg(span):
    """span -> 1 .. 8 (0 or None = the default 4); anything else is a ValueError naming the value"""
    if span is None:
        span = 0
    if isinstance(span, bool) or not isinstance(span, (int, np.integer)) or not 0 <= int(span) <= WATERMARK_SCAN_MAX_SPAN:
        raise ValueError(f"watermark span {span!r} outside [1, {WATERMARK_SCAN_MAX_SPAN}] (0 = the default, {WATERMARK_SCAN_DEFAULT_SPAN})")
    return int(span) or WATERMARK_SCAN_DEFAULT_SPAN


def threshold(wmax):
    """t(Wmax) = sqrt(36 + 2 ln(max(1, Wmax))).  Hoeffding bounds a window's false alarm by exp(-t^2 / 2); over at most 128 Wmax
    (offset, window) pairs that is 128 Wmax e^(-t^2 / 2) = 128 e^(-18) = 1.9e-6 per item, the detector's figure; t(1) = 6."""
    return math.sqrt(36.0 + 2.0 * math.log(max(1, int(wmax))))


def window_range(o, p0, w, span, length):
    """the nominal range [start, end) in samples of window w of `span` periods at offset index o whose first complete period is p0,
    clipped to [0, length): pattern frame p (hop 256) is centred on sample 256 p - 128 o"""
    a = WATERMARK_PERIOD_SAMPLES * (int(p0) + int(w)) - DETECT_HOP * int(o)
    return min(max(a, 0), int(length)), min(max(a + WATERMARK_PERIOD_SAMPLES * int(span), 0), int(length))


def segments(z_scan, first_period, windows, span, length):
    """z_scan [128, W], first_period [128], windows [128] of ONE item (op_watermark_scan's outputs at [b]) -> [WatermarkSegment],
    sorted by start.
      1. every (o, w < windows[o]) with z >= threshold(max(windows)) is a candidate, the highest z first
      2. the best one, (o*, w*), grows over the candidates at offset indices o* - 1 .. o* + 1 whose first period p0 + w continues
         its own in steps of one period, on either side
      3. the segment is the union of their nominal ranges, with the best window's z and 128 o*
      4. every candidate left whose nominal range overlaps the segment is dropped; the best of the rest is next"""
    S = span_arg(span)
    z_scan = np.asarray(z_scan, np.float64)
    first_period, windows = np.asarray(first_period).reshape(-1), np.asarray(windows).reshape(-1)
    if z_scan.ndim != 2 or z_scan.shape[0] != WATERMARK_OFFSETS or first_period.shape != (WATERMARK_OFFSETS,) or windows.shape != first_period.shape:
        raise ValueError("segments: z_scan [128, W], first_period [128] and windows [128] of one item")
    t = threshold(int(windows.max()))
    live = np.arange(z_scan.shape[1])[None, :] < windows[:, None]
    cand = [(float(z_scan[o, w]), int(o), int(w)) for o, w in zip(*np.nonzero(live & (z_scan >= t)))]
    cand.sort(key=lambda c: (-c[0], c[1], c[2]))
    out = []
    while cand:
        z, o, w = cand[0]
        near = {}  # first period -> the candidates of the three offsets that start there
        for c in cand:
            if abs(c[1] - o) <= 1:
                near.setdefault(int(first_period[c[1]]) + c[2], []).append(c)
        lo = hi = int(first_period[o]) + w
        while lo - 1 in near:
            lo -= 1
        while hi + 1 in near:
            hi += 1
        ranges = [window_range(c[1], first_period[c[1]], c[2], S, length) for p in range(lo, hi + 1) for c in near[p]]
        seg = WatermarkSegment(min(r[0] for r in ranges), max(r[1] for r in ranges), z, DETECT_HOP * o)
        out.append(seg)
        rest = []
        for c in cand[1:]:
            a, b = window_range(c[1], first_period[c[1]], c[2], S, length)
            if b <= seg.start or a >= seg.end:
                rest.append(c)
        cand = rest
    return sorted(out, key=lambda s: s.start)
