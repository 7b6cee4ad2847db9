"""The watermark payload on the CPU (include/vits_watermark_payload.h): the code and the positions against the header's figures, the
conditions the float64 restatement (tests/watermark_payload_ref.py) has to meet on the test signal -- which are also the decision
margins of every input of tests/test_watermark_payload_gpu.py -- and the plumbing from Synth, the sessions and the command line down to
the C ABI, against the call recorder of tools/tail_calls.py.  The device is checked in tests/test_watermark_payload_gpu.py.

Figures of the float64 restatement on voiced_signal(4.0) at 2 dB (printed by the test), over the five payloads and the five forms
(marked, int16, scaled by 1e-3, cropped at 5000 and at 12345): pilot z 15.7 to 17.2, every word read without a wrong bit,
min |z_i| >= 1.89, the best offset ahead of every other by >= 0.0047 (payload 0xFFFF cropped at 12345; 0x0000 uncropped: 0.0053, where the
best index is 127, the cyclic neighbour of 0).  A plain 2 dB mark reads z = 16.1, word 0x000000, not valid; unmarked audio scores at
most 0.92 and three other keys at most 2.72.  The plain detector on payload-marked audio scores by the weight of the word: 16.6 for
payload 0x0000 (word 0x0000D7), 14.3 for 0x1234, 8.4 for 0xA5A5, 4.8 for 0xBEEF, 1.3 for 0xFFFF."""
import ctypes
import hashlib
import importlib
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import watermark_payload_ref as P
import watermark_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = 0x5EED1234
OTHER_KEYS = (KEY + 1, 1, 0xDEADBEEF)
PAYLOADS = (0xBEEF, 0x0000, 0xFFFF, 0x1234, 0xA5A5)
BIT_COUNTS = (31, 31, 36, 27, 23, 37, 31, 24, 28, 37, 28, 27, 32, 37, 29, 30, 31, 34, 37, 30, 41, 29, 37, 25)


# ---- the code and the positions -----------------------------------------------------------------------------------------------------
def test_crc_and_words():
    assert P.word(0) == 0x0000D7 and P.word(0xBEEF) == 0xBEEFCD and P.crc8(0xFFFF) == 0xF3
    assert [int(b) for b in P.word_bits(0xBEEFCD)] == [int(c) for c in f"{0xBEEFCD:024b}"]  # bit i = (W >> (23 - i)) & 1
    assert P.crc8(0, init=0) == 0  # the linear part
    for bad in (-1, 65536, 1.0, True, "7"):
        with pytest.raises(ValueError, match="outside"):
            P.word(bad)
    with pytest.raises(ValueError, match="65536"):
        P.word(65536)


def test_minimum_distance_is_four():
    """The linear part (initial value 0) over all 65535 non-zero payloads: the lowest weight is 4, so up to three wrong bits never read
    as another payload; the affine code (initial value 0xFF) has the same distances and does not hold the all-zero word."""
    crc_byte = [P.crc8(b, init=0) for b in range(256)]  # of payloads 0x00bb; the code is linear: crc(hi:lo) = crc(hi:00) ^ crc(00:lo)
    crc_hi = [P.crc8(b << 8, init=0) for b in range(256)]
    pop = [bin(v).count("1") for v in range(256)]
    weights = [pop[p >> 8] + pop[p & 255] + pop[crc_hi[p >> 8] ^ crc_byte[p & 255]] for p in range(1, 65536)]
    for p in (1, 0x8000, 0xBEEF, 0xFFFF, 0x0107):  # the shortcut above against the definition
        assert crc_hi[p >> 8] ^ crc_byte[p & 255] == P.crc8(p, init=0)
    assert min(weights) == 4
    const = P.crc8(0)  # crc8(p) = crc8_0(p) ^ const: the words are the linear code shifted by one fixed word
    assert all(P.crc8(p) == P.crc8(p, init=0) ^ const for p in (1, 0x8000, 0xBEEF, 0xFFFF))
    assert const == 0xD7 and all(P.word(p) != 0 for p in (0, 1, 0xFFFF))
    assert 0 not in {P.crc8(p) | (p << 8) for p in range(65536)}  # the all-zero word is not a codeword


def test_positions_of_the_test_key():
    pil, bi = P.pilots(), P.bit_index(KEY)
    assert pil.shape == (16, 96) and bi.shape == (16, 96) and bi.min() >= 0 and bi.max() <= 23
    assert pil[0, 1] and not pil[0, 0] and not pil[1, 1] and pil.sum() == 768
    assert int(pil[:, 1:-1].sum()) == 752  # the scored pilot chips, j in 1 .. 94
    assert tuple(int((~pil & (bi == i))[:, 1:-1].sum()) for i in range(24)) == BIT_COUNTS
    # i(q, j) from the definition's words, element by element
    mk = int(R.mix(KEY))
    for q, j in ((0, 0), (3, 5), (15, 95)):
        assert int(bi[q, j]) == int(R.mix(mk ^ (0x80000000 | (96 * q + j + 1)))) % 24
    c, cp = R.chips(KEY), P.payload_chips(KEY, 0xBEEF)
    bits = P.word_bits(P.word(0xBEEF))
    assert np.array_equal(cp[pil], c[pil])  # pilots carry the plain chip
    assert np.array_equal(cp[~pil], (c * (1 - 2 * bits[bi]))[~pil])
    assert np.array_equal(P.payload_chips(KEY, 0xBEEF) != c, ~pil & (bits[bi] == 1))


# ---- the conditions on the restatement ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def signal():
    x = R.voiced_signal(4.0)
    x.setflags(write=False)
    return x


def _forms(y):
    """the five forms of a marked item, as float32 like the device's input: (name, audio, the offset index of the crop)"""
    y = y.astype(np.float32)
    return (("marked", y, 0), ("int16", np.round(y * 32767.0).astype(np.int16).astype(np.float32) / np.float32(32767.0), 0),
            ("x 1e-3", y * np.float32(1e-3), 0), ("crop 5000", y[5000:], 39), ("crop 12345", y[12345:], 96))


def _lead(d):
    za = d["z_all"].copy()
    za[d["offset"] // 128] = -np.inf
    return d["z"] - za.max()


def test_restatement_reads_every_payload_back(signal):
    x = signal
    for p in PAYLOADS:
        y = P.embed(x, KEY, p, 2.0)
        assert y.shape == x.shape and 0.01 < np.abs(y - x).max() / np.abs(x).max() < 0.4  # a ripple of about 2 dB, not a rewrite
        for name, a, o in _forms(y):
            d = P.read(a, KEY)
            errs = bin(d["word"] ^ P.word(p)).count("1")
            got = d["offset"] // 128
            print(f"{p:#06x} {name}: z {d['z']:.3f} at index {got} rows {d['rows']} errs {errs} min |z_i| {np.abs(d['bit_z']).min():.3f} lead {_lead(d):.4f}")
            assert d["valid"] and d["detected"] and errs == 0 and d["payload"] == p, (p, name)
            assert min((got - o) % 128, (o - got) % 128) <= 1, (p, name, got)
            # the two input conditions that make the device comparison of integers meaningful
            assert np.abs(d["bit_z"]).min() >= 1.0, (p, name)
            assert _lead(d) >= 1e-3, (p, name)
            assert d["z"] - R.THRESHOLD >= 2.0


def test_plain_marks_other_keys_and_unmarked_audio(signal):
    x = signal
    plain = R.embed(x, KEY, 2.0).astype(np.float32)
    d = P.read(plain, KEY)
    print(f"plain mark: z {d['z']:.3f} word {d['word']:#08x} min z_i {d['bit_z'].min():.3f} lead {_lead(d):.4f}; the detector: {R.detect(plain, KEY)['z']:.3f}")
    assert d["detected"] and not d["valid"] and d["word"] == 0 and d["payload"] == 0
    assert d["bit_z"].min() >= 1.0 and _lead(d) >= 1e-3  # (an input of the GPU test: its margins too)
    assert d["z"] < R.detect(plain, KEY)["z"]  # on half the chips: lower than the detector's score
    d = P.read(x, KEY)
    print(f"unmarked: max z = {d['z_all'].max():.3f}")
    assert d["z_all"].max() < 4.0 and not d["detected"] and not d["valid"]
    y = P.embed(x, KEY, 0xBEEF, 2.0)
    for key in OTHER_KEYS:
        d = P.read(y, key)
        print(f"key {key:#x}: max z = {d['z_all'].max():.3f}")
        assert d["z_all"].max() < 4.0 and not d["detected"] and not d["valid"]
    # what the plain detector makes of payload marks goes with the weight of the word: it is not their detector
    zs = {p: R.detect(P.embed(x, KEY, p, 2.0), KEY)["z"] for p in (0x0000, 0xFFFF)}
    print("the detector on payload marks:", {hex(p): round(z, 2) for p, z in zs.items()})
    assert zs[0xFFFF] < R.THRESHOLD < zs[0x0000]


def test_embed_edges_and_the_untouched_plain_restatement(signal):
    x = signal
    for n in (400, 512):  # below n/2 + 1: as it went in
        assert np.array_equal(P.embed(x[:n], KEY, 7), x[:n].astype(np.float64))
    y = P.embed(x[:5000], KEY, 7)
    assert np.array_equal(y[256 * (5000 // 256):], x[256 * (5000 // 256):5000].astype(np.float64))
    assert np.array_equal(P.embed(x[:5000], KEY, 7, 0.0), P.embed(x[:5000], KEY, 7, 2.0))  # 0 = the payload default, 2 dB
    assert not np.array_equal(P.embed(x[:5000], KEY, 7, 1.0), P.embed(x[:5000], KEY, 7, 2.0))
    for bad, match in ((-0.5, "-0.5"), (2.5, "2.5"), (float("nan"), "nan")):
        with pytest.raises(ValueError, match=match):
            P.embed(x[:5000], KEY, 7, bad)
    with pytest.raises(ValueError, match="65536"):
        P.embed(x[:5000], KEY, 65536)
    d = P.read(x[:600], KEY)  # frames, but no complete row
    assert (d["z"], d["offset"], d["rows"], d["valid"], d["payload"]) == (0.0, 0, 0, False, 0) and not d["z_all"].any()
    y64, y32 = P.embed(x[:22050], KEY, 0xBEEF), P.embed(x[:22050], KEY, 0xBEEF, dtype=np.float32)
    assert y32.dtype == np.float32 and 0 < np.abs(y32 - y64).max() < 2e-6  # the yardstick of the GPU test
    # watermark_ref is as it was: a figure of tests/test_watermark.py (3 s, 1 dB: z_all[0] = 10.05) and the module's own words
    x3 = R.voiced_signal(3.0)
    assert abs(R.detect(R.embed(x3, KEY), KEY)["z_all"][0] - 10.05) < 0.01
    assert (R.DEFAULT_DEPTH_DB, P.DEFAULT_DEPTH_DB, R.MAX_DEPTH_DB) == (1.0, 2.0, 2.0)
    out = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "tests/watermark_ref.py"], capture_output=True, text=True)
    assert out.returncode != 0 or out.stdout.strip() == ""  # (outside a checkout there is nothing to compare with)


# ---- the header against its mirrors ---------------------------------------------------------------------------------------------------
def test_header_layout_flags_and_export(tmp_path, hip_lib):
    from vosk_tts_amd import capi, capi_stts

    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "vits_watermark_payload.h"', 'int main(void) {',
             '  printf("%d %d %d %d %u %g\\n", VITS_FLAG_WATERMARK_PAYLOAD, STTS_FLAG_WATERMARK_PAYLOAD, VITS_WATERMARK_PAYLOAD_BITS, '
             'VITS_WATERMARK_CODED_BITS, VITS_WATERMARK_PAYLOAD_MAX, (double)VITS_WATERMARK_PAYLOAD_DEFAULT_DEPTH_DB);']
    for fam in ("vits", "stts"):
        t = f"{fam}_synth_opts_watermark_payload"
        lines.append(f'  printf("%zu %zu %zu %zu %zu\\n", sizeof({t}), offsetof({t}, base), offsetof({t}, watermark_payload), '
                     f'offsetof({t}, watermark_payloads), sizeof({fam}_synth_opts_watermark));')
    lines += ['  return 0;', '}']
    src = tmp_path / "c.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "c"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert [float(v) for v in out[0]] == [capi.FLAG_WATERMARK_PAYLOAD, capi_stts.STTS_FLAG_WATERMARK_PAYLOAD, 16, capi.WATERMARK_CODED_BITS,
                                         capi.WATERMARK_PAYLOAD_MAX, P.DEFAULT_DEPTH_DB]
    assert (capi.FLAG_WATERMARK_PAYLOAD, capi_stts.STTS_FLAG_WATERMARK_PAYLOAD, P.CODED_BITS, P.PAYLOAD_MAX) == (512, 512, 24, 65535)
    for row, C, W in ((out[1], capi.SynthWatermarkPayloadOpts, capi.SynthWatermarkOpts), (out[2], capi_stts.SttsWatermarkPayloadOpts, capi_stts.SttsWatermarkOpts)):
        assert [int(v) for v in row] == [ctypes.sizeof(C), 0, C.watermark_payload.offset, C.watermark_payloads.offset, ctypes.sizeof(W)]
        assert issubclass(C, W)
    # the bit is free in both families, and the library exports the doors with the binding's argument lists
    assert capi.FLAG_WATERMARK_PAYLOAD not in (1, capi.FLAG_LOUDNESS, capi.FLAG_PITCH, capi.FLAG_PITCH_FORMANT, capi.FLAG_LIMIT, capi.FLAG_PROSODY,
                                               capi.FLAG_CONTOUR, capi.FLAG_INTONATION, capi.FLAG_WATERMARK)
    assert capi_stts.STTS_FLAG_WATERMARK_PAYLOAD not in (capi_stts.STTS_FLAG_ITEM_SEEDS, capi_stts.STTS_FLAG_DENOISE, capi_stts.STTS_FLAG_LOUDNESS,
                                                         capi_stts.STTS_FLAG_PITCH, capi_stts.STTS_FLAG_PITCH_FORMANT, capi_stts.STTS_FLAG_LIMIT,
                                                         capi_stts.STTS_FLAG_CONTOUR, capi_stts.STTS_FLAG_INTONATION, capi_stts.STTS_FLAG_WATERMARK)
    assert hip_lib.has_watermark_payload
    assert [len(hip_lib._fn(n).argtypes) for n in ("op_watermark_payload", "op_watermark_read")] == [9, 13]


# ---- plumbing against the call recorder -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rec():
    """tools/tail_calls.py: a Recorder where the CDLL stands, and sessions made around it"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        T = importlib.import_module("tail_calls")
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    Pk = type("P", (), {n: importlib.import_module("vosk_tts_amd." + n)
                        for n in ("capi", "capi_stts", "session", "session_stts", "batching", "weights", "weights_stts")})
    return T, Pk


def _sha_u32(values):
    return hashlib.sha256(np.array(values, np.uint32).tobytes()).hexdigest()[:16]


def test_payload_spec_and_refusals_before_any_device_work(rec):
    from vosk_tts_amd import capi
    from vosk_tts_amd.synth import Synth

    assert capi.payload_spec(None) is None and capi.payload_spec(0) == 0 and capi.payload_spec(np.uint16(65535)) == 65535
    assert capi.payload_spec([1, 2]) == (1, 2) and capi.payload_spec(np.array([3, 4])) == (3, 4)
    for bad in (-1, 65536, 1.5, True, "7", [1, 65536]):
        with pytest.raises(ValueError, match="watermark_payload"):
            capi.payload_spec(bad)
    assert capi.watermark_spec(KEY) == (KEY, 0.0) and capi.watermark_spec(KEY, 1.5, 7) == (KEY, 1.5, 7)  # without a payload: the spec of before
    with pytest.raises(ValueError, match="watermark_payload needs watermark"):
        capi.watermark_spec(None, None, 7)
    T, Pk = rec
    sess = T.vits_session(Pk)
    for fn in (sess.run_pcm16, lambda f: sess.run(None, f), lambda f: sess.run_document(dict(f, **{"vits.doc_gap_frames": [1]}))):
        for ext, match in (({"vits.watermark_payload": 5}, "watermark_payload without watermark"),
                           ({"vits.watermark_key": KEY, "vits.watermark_payload": 65536}, "65536"),
                           ({"vits.watermark_key": KEY, "vits.watermark_payload": -1}, "-1")):
            with pytest.raises(ValueError, match=match):
                fn(T.vits_feed(1, 5, **ext))
    with pytest.raises(ValueError, match="VITS_FLAG_WATERMARK_PAYLOAD"):
        sess.run_stream(None, T.vits_feed(1, 5, **{"vits.watermark_key": KEY, "vits.watermark_payload": 5}))
    st = T.stts_session(Pk)
    with pytest.raises(ValueError, match="STTS_FLAG_WATERMARK_PAYLOAD"):
        st.run_stream(None, T.stts_feed(1, 5, False, **{"vits.watermark_key": KEY, "vits.watermark_payload": 5}))
    assert sess._lib.lib.records == [] and st._lib.lib.records == []  # nothing reached the C ABI
    # Synth: the three refusals, by name, before the model is touched (the stub has none)
    s = Synth.__new__(Synth)
    s.model = type("M", (), {"config": {"inference": {}}})()
    with pytest.raises(ValueError, match="watermark_payload needs watermark"):
        s._watermark({}, None, None, 5)
    with pytest.raises(ValueError, match="65536"):
        s._watermark({}, KEY, None, 65536)
    with pytest.raises(ValueError, match="VITS_FLAG_WATERMARK_PAYLOAD"):
        next(iter(s.synth_stream("a", watermark=KEY, watermark_payload=5)))
    args = {}
    assert s._watermark(args, KEY, None, 0xBEEF) and args == {"vits.watermark_key": KEY, "vits.watermark_payload": 0xBEEF}
    args = {}
    assert s._watermark(args, KEY) and args == {"vits.watermark_key": KEY}  # the feed of before


def test_keywords_exist_where_watermark_does():
    from vosk_tts_amd import capi, capi_stts
    from vosk_tts_amd.batching import MultiDeviceSynth
    from vosk_tts_amd.synth import Synth

    for fn in (Synth.synth_audio, Synth.synth, Synth.synth_document, Synth.synth_stream, MultiDeviceSynth.synth_batch, capi.VitsModel.synthesize,
               capi.VitsModel.synthesize_pcm16, capi.VitsModel.synthesize_document, capi.VitsModel.stream, capi_stts.SttsModel.synthesize,
               capi_stts.SttsModel.synthesize_batch, capi_stts.SttsModel.synthesize_document, capi_stts.SttsModel.stream):
        assert inspect.signature(fn).parameters["watermark_payload"].default is None, fn
    assert hasattr(Synth, "read_watermark") and hasattr(capi.VitsLib, "op_watermark_read") and hasattr(capi.VitsLib, "op_watermark_payload")
    from vosk_tts_amd import session, session_stts
    from vosk_tts_amd.outopts import TAIL_FEEDS

    assert all("vits.watermark_payload" in t for t in (session._EXT, session_stts._EXT, TAIL_FEEDS))


def test_the_payload_rides_with_the_request_and_a_batch_gets_the_array(rec):
    """Two feeds of one key with different payloads share a coalescer key and reach the C ABI as ONE solo batch call whose struct
    carries watermark_payloads [B]; a lone request carries the scalar; a request without a payload passes the struct of before."""
    T, Pk = rec
    from vosk_tts_amd.session import RequestExtra

    sess = T.vits_session(Pk)
    keys, extras = [], []
    submit = sess.coalescer.submit
    sess.coalescer.submit = lambda key, ids, sid, seed, extra=None: (keys.append(key), extras.append(extra), submit(key, ids, sid, seed, extra))[2]
    wm = {"vits.watermark_key": KEY}
    sess.run_pcm16(T.vits_feed(1, 5, **wm, **{"vits.watermark_payload": 0x1234}), 1.0)
    sess.run_pcm16(T.vits_feed(1, 5, **wm, **{"vits.watermark_payload": 0xBEEF}), 1.0)
    sess.run_pcm16(T.vits_feed(1, 5, **wm), 1.0)
    sess.run_pcm16(T.vits_feed(1, 5, **wm, **{"vits.watermark_payload": 7, "vits.watermark_depth_db": 1.0}), 1.0)
    assert keys[0] == keys[1] and [e.payload for e in extras] == [0x1234, 0xBEEF, None, 7]
    assert len({keys[0], keys[2], keys[3]}) == 3  # a plain mark, and another depth, are other batches
    assert tuple(extras[0]) == (np.float32(0.8), 1.0, np.float32(0.8)) or len(extras[0]) == 3  # the scales ride as they did
    r = sess._lib.lib.records
    both = Pk.capi.FLAG_WATERMARK | Pk.capi.FLAG_WATERMARK_PAYLOAD
    assert len(r) == 4 and all(x.startswith("vits_synthesize_pcm16(") for x in r)
    size = ctypes.sizeof(Pk.capi.SynthWatermarkPayloadOpts)
    assert f"{{SynthWatermarkPayloadOpts/{size} " in r[0] and f"flags={both} " in r[0] and f"watermark_payload={0x1234}" in r[0] and "watermark_payloads" not in r[0]
    assert f"watermark_payload={0xBEEF}" in r[1]
    assert f"{{SynthWatermarkOpts/{ctypes.sizeof(Pk.capi.SynthWatermarkOpts)} " in r[2] and f"flags={Pk.capi.FLAG_WATERMARK} " in r[2] and "payload" not in r[2]
    assert "watermark_payload=7" in r[3] and "watermark_depth_db=1.0" in r[3]
    # the merged call of a busy server: one call, B = 2, the array
    del r[:]
    reqs = [(np.ones((1, 4), np.int64), 0, 1, RequestExtra.of((0.8, 1.0, 0.8), 0x1234)), (np.full((1, 3), 2, np.int64), 1, 2, RequestExtra.of((0.8, 1.0, 0.8), 0xBEEF))]
    out = sess._run_solo_batch(keys[0], reqs)
    assert len(out) == 2 and len(r) == 1 and r[0].startswith("vits_synthesize_pcm16(h, ") and ", 2, 4, " in r[0]
    assert f"flags={1 | both} " in r[0] and f"watermark_payloads=&{_sha_u32([0x1234, 0xBEEF])}" in r[0] and f"watermark_key={KEY}" in r[0]
    # three requests: padded to four with a one-token dummy, whose payload is 0
    del r[:]
    sess._run_solo_batch(keys[0], reqs + [(np.ones((1, 2), np.int64), 0, 3, RequestExtra.of((0.8, 1.0, 0.8), 9))])
    assert len(r) == 1 and f"watermark_payloads=&{_sha_u32([0x1234, 0xBEEF, 9, 0])}" in r[0]
    # a feed that is not coalesced (a batch of its own) takes one value, or one per item, in the call itself
    del r[:]
    sess.run_pcm16(T.vits_feed(2, 4, **wm, **{"vits.watermark_payload": [5, 6]}), 1.0)
    sess.run_pcm16(T.vits_feed(2, 4, **wm, **{"vits.watermark_payload": 5}), 1.0)
    assert f"watermark_payloads=&{_sha_u32([5, 6])}" in r[0] and "watermark_payload=5" in r[1] and "watermark_payloads" not in r[1]
    with pytest.raises(ValueError, match="3 values for a batch of 2"):
        sess.run_pcm16(T.vits_feed(2, 4, **wm, **{"vits.watermark_payload": [5, 6, 7]}), 1.0)
    # a document takes the scalar
    del r[:]
    sess.run_document(T.vits_feed(2, 4, **wm, **{"vits.watermark_payload": 5, "vits.doc_gap_frames": [1, 0]}))
    assert r[0].startswith("vits_synthesize_document") and "watermark_payload=5" in r[0] and "SynthWatermarkPayloadOpts" in r[0]
    with pytest.raises(ValueError, match="one value"):
        sess.run_document(T.vits_feed(2, 4, **wm, **{"vits.watermark_payload": [5, 6], "vits.doc_gap_frames": [1, 0]}))


def test_multistream_session_and_the_shard_runners(rec):
    T, Pk = rec
    st = T.stts_session(Pk)
    r = st._lib.lib.records
    wm = {"vits.watermark_key": KEY, "vits.watermark_payload": 0xA5A5}
    both = Pk.capi_stts.STTS_FLAG_WATERMARK | Pk.capi_stts.STTS_FLAG_WATERMARK_PAYLOAD
    st.run(None, T.stts_feed(1, 5, False, **wm))
    assert r[0].startswith("stts_synthesize(") and "SttsWatermarkPayloadOpts" in r[0] and f"flags={both} " in r[0] and f"watermark_payload={0xA5A5}" in r[0]
    del r[:]
    st.run(None, T.stts_feed(1, 5, False, **wm, **{"vits.sample_rate": T.RATE}))  # at another rate the session marks on the host, behind its resampler
    names = [x.split("(")[0] for x in r]
    assert names.index("vits_op_resample") < names.index("vits_op_watermark_payload") and "payload" not in r[0]
    del r[:]
    st.run_batch(T.stts_feed(2, 4, True, **{"vits.watermark_key": KEY, "vits.watermark_payload": [5, 6]}))
    assert r[0].startswith("stts_synthesize_batch(") and f"watermark_payloads=&{_sha_u32([5, 6])}" in r[0]
    # MultiDeviceSynth: one int per request is cut to every part of a shard
    from vosk_tts_amd.batching import tail_part

    frag = {"vits.watermark_key": KEY, "vits.watermark_payload": (10, 11, 12)}
    assert tail_part(frag, [2, 0]) == {"vits.watermark_key": KEY, "vits.watermark_payload": [12, 10]} and frag["vits.watermark_payload"] == (10, 11, 12)
    assert tail_part({"vits.watermark_key": KEY, "vits.watermark_payload": 4}, [1]) == {"vits.watermark_key": KEY, "vits.watermark_payload": 4}
    assert tail_part(None, [0]) == {}
    sess = T.vits_session(Pk)
    del sess._lib.lib.records[:]
    T.multi_device(Pk, sess, "vits", lambda mds: mds.synth_tokens([[1, 2, 3, 4], [5, 6, 7]], [0, 1], None, None, None, None, [7, 8], None, False, frag))
    rv = sess._lib.lib.records
    assert len(rv) == 1 and f"watermark_payloads=&{_sha_u32([10, 11])}" in rv[0]


def test_command_line_flags(tmp_path, capsys):
    import json
    import wave

    from vosk_tts_amd import cli

    p = cli.build_parser()
    o = p.parse_args(["-i", "x", "--watermark", "0x5EED1234", "--watermark-payload", "48879"])
    assert (o.watermark, o.watermark_payload, o.read_watermark) == (KEY, 48879, None)
    o = p.parse_args(["--read-watermark", "a.wav", "--watermark", "5"])
    assert (o.read_watermark, o.watermark, o.input, o.watermark_payload) == ("a.wav", 5, None, None)
    assert p.parse_args(["-i", "x"]).watermark_payload is None
    path = str(tmp_path / "a.wav")
    with wave.open(path, "w") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(22050)
        f.writeframes(np.arange(1000, dtype=np.int16).tobytes())
    seen = []

    class S:
        def read_watermark(self, audio, key):
            seen.append((audio.dtype, audio.shape, key))
            return True, 16.25, 640, 0xBEEF, np.linspace(-3.0, 3.0, 24) + 0.5

    assert cli.read_watermark(S(), path, 5) == 0
    assert seen == [(np.dtype(np.int16), (1000,), 5)]
    assert json.loads(capsys.readouterr().out) == {"detected": True, "z": 16.25, "offset_samples": 640, "payload": 0xBEEF, "min_abs_bit_z": 0.109}
