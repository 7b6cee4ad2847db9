"""Documents on the device (include/vits_document.h): the join's kernels against the NumPy restatement (tests/document_ref.py) through
the parity door, bit for bit, and the document entry points against the same restatement applied to the rows of the batch call.

Bounds: none of its own.  The join copies samples or multiplies them once in fp32 by a host-made table, so every comparison of the
join is with tobytes().  The stages behind the join are compared with their float64 restatements under the bounds of their own GPU
tests (named where they are used)."""
import ctypes
import itertools

import numpy as np
import pytest

import document_ref as D

pytestmark = pytest.mark.gpu

SCALES = [0.667, 1.0, 0.8]
NATIVE = 22050
SEED = 6
TRIM_DB = -20.0


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert hip_lib.has_document, "libvits_mi355.so exports no vits_op_document_join"
    return hip_lib


# ---- 1. the door against the restatement ---------------------------------------------------------------------------------------------
SHAPES = {"3": [5, 1, 9], "1": [4], "33": [1 + b % 4 for b in range(16)] + [40] + [1 + b % 4 for b in range(16)]}


def _items(lens, hop, seed, quiet):
    """x float32 [B, N], NaN beyond every item.  quiet: heads and tails of frames below the trim threshold (one of their samples exactly
    at it), item 1 quiet altogether."""
    rng = np.random.default_rng(seed)
    B, N = len(lens), max(lens) * hop + 12
    thr = D.threshold(TRIM_DB)
    x = np.full((B, N), np.nan, np.float32)
    for b, n in enumerate(lens):
        v = rng.uniform(0.2, 0.9, n * hop).astype(np.float32) * rng.choice(np.array([-1.0, 1.0], np.float32), n * hop)
        if quiet:
            q = (0.5 * thr * rng.uniform(-1, 1, n * hop)).astype(np.float32)
            head, tail = ((b + 1) % 3, 1 - b % 2) if (b != 1 and n > 3) else (n, 0) if b == 1 else (0, 0)
            if B == 1:
                head, tail = 1, 1
            v[:head * hop] = q[:head * hop]
            if tail:
                v[-tail * hop:] = q[-tail * hop:]
            if head:
                v[hop // 2] = -thr  # |x| == thr exactly: not loud
        x[b, :n * hop] = v
    return x


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("hop", (256, 64))
def test_door_equals_the_restatement(lib, hop, shape):
    lens = SHAPES[shape]
    B = len(lens)
    n_cases = 0
    for quiet, (trim_db, keep) in ((False, (None, 0)), (True, (TRIM_DB, 0)), (True, (TRIM_DB, 2))):
        x = _items(lens, hop, 11 + B, quiet)
        for fade, gap, lead in itertools.product((0, 7, hop // 2), (0, 3), (0, 2)):
            gaps = [gap if (b % 2 == 0 or gap == 0) else gap + b % 5 for b in range(B)]
            want = D.join(x, lens, hop, lead, gaps, fade, trim_db, keep)
            if quiet:  # the case is what it claims to be
                assert B == 1 or (want["n"][1] == 0 and want["F"] > 0)
                b = 3 if B > 4 else 0  # (an item with a quiet head, whose frame 0 holds the sample at the threshold)
                assert abs(x[b, hop // 2]) == D.threshold(TRIM_DB)
                if keep == 0:
                    assert want["lo"][b] >= 1 and any(0 < h < n for h, n in zip(want["hi"], lens))
                else:  # keep reaches past both ends of an item
                    assert want["lo"][b] == 0 and want["hi"][b] == lens[b]
            else:
                assert want["n"] == lens
            cap = (lead + sum(lens) + sum(gaps)) * hop + 100
            y0 = np.full(cap, 7.5, np.float32)
            y, F, start, trim = lib.op_document_join(x, lens, hop, y=y0, lead_frames=lead, gap_frames=gaps, fade_samples=fade, trim_db=trim_db,
                                                     trim_keep_frames=keep)
            tag = (hop, shape, quiet, keep, fade, gap, lead)
            assert F == want["F"], tag
            assert start.tolist() == want["start"] and trim[:, 0].tolist() == want["lo"] and trim[:, 1].tolist() == want["hi"], tag
            assert y[:F * hop].tobytes() == want["y"].tobytes(), tag
            assert y[F * hop:].tobytes() == y0[F * hop:].tobytes(), tag
            n_cases += 1
    assert n_cases == 36


def test_door_searches_long_tables_in_global_memory(lib):
    """more segments than the tables kept in LDS hold (DOC_LDS_SEG = 1024), with a hop that is no multiple of 4 (the scalar form)"""
    for hop, B in ((64, 1030), (6, 1030), (6, 5)):
        lens = [1 + b % 2 for b in range(B)]
        x = _items(lens, hop, 3, False)
        gaps = [b % 3 for b in range(B)]
        want = D.join(x, lens, hop, 1, gaps, hop // 2)
        y, F, start, _ = lib.op_document_join(x, lens, hop, lead_frames=1, gap_frames=gaps, fade_samples=hop // 2)
        assert F == want["F"] and start.tolist() == want["start"]
        assert y[:F * hop].tobytes() == want["y"].tobytes()


def test_door_an_empty_document_is_ok(lib):
    """every frame at or below the threshold, no lead, no gap: F = 0 and nothing is written"""
    hop = 64
    x = np.full((2, 3 * hop), D.threshold(TRIM_DB), np.float32)
    y0 = np.full(5 * hop, 7.5, np.float32)
    y, F, start, trim = lib.op_document_join(x, [3, 2], hop, y=y0, trim_db=TRIM_DB, trim_keep_frames=2, fade_samples=5)
    assert F == 0 and start.tolist() == [0, 0] and not trim.any() and y.tobytes() == y0.tobytes()
    assert D.join(x, [3, 2], hop, trim_db=TRIM_DB, keep=2, fade=5)["F"] == 0


# ---- the entry points ------------------------------------------------------------------------------------------------------------------
class _Path:
    """one host path: the fast one as it is, the eager one with vits_debug_fast_path(0) around every call"""

    def __init__(self, lib, fast):
        self.lib, self.fast = lib, fast

    def call(self, fn, *a, **kw):
        self.lib.lib.vits_debug_fast_path(1 if self.fast else 0)
        try:
            return fn(*a, **kw)
        finally:
            self.lib.lib.vits_debug_fast_path(1)


@pytest.fixture(scope="module")
def feed():
    rng = np.random.default_rng(47)
    Tx = 24
    lens = np.array([Tx, Tx - 9, 5], np.int64)
    ids = rng.integers(1, 20, size=(3, Tx)).astype(np.int64)
    sid = np.array([0, 1, 0], np.int64)  # two speakers
    return ids, lens, sid


@pytest.fixture(scope="module")
def batch(lib, hip_tiny, feed):
    """per path: the rows of the SOLO batch call (float), their frame counts and the cumulative frame counts of their tokens.  Computed
    once, never written to."""
    ids, lens, sid = feed
    hop = hip_tiny.hp.hop_length
    out = {}
    for fast in (True, False):
        rows, ol, ends = _Path(lib, fast).call(hip_tiny.synthesize, ids, lens, SCALES, sid, seed=SEED, solo=True, marks=True)
        assert ol.min() > 0 and not (ol % hop).any() and not (ends % hop).any()
        frames, cum = ol // hop, ends // hop
        for a in (rows, frames, cum):
            a.setflags(write=False)
        out[fast] = dict(rows=rows, frames=frames, cum=cum)
    return out


GAPS = [3, 0, 2]


@pytest.mark.parametrize("fast", (True, False), ids=("fast", "eager"))
def test_document_equals_the_joined_batch(lib, hip_tiny, feed, batch, fast):
    ids, lens, sid = feed
    hop = hip_tiny.hp.hop_length
    ref, path = batch[fast], _Path(lib, fast)
    for fade in (0, 9):
        want = D.join(ref["rows"], ref["frames"], hop, 2, GAPS, fade)
        got, info = path.call(hip_tiny.synthesize_document, ids, lens, SCALES, sid, seed=SEED, lead_frames=2, gap_frames=GAPS, fade_samples=fade)
        assert got.dtype == np.float32 and got.shape == (want["F"] * hop,)
        assert got.tobytes() == want["y"].tobytes(), fade
        assert info["trim"][:, 0].tolist() == want["lo"] and info["trim"][:, 1].tolist() == want["hi"]
    assert not np.array_equal(D.join(ref["rows"], ref["frames"], hop, 2, GAPS, 9)["y"], D.join(ref["rows"], ref["frames"], hop, 2, GAPS, 0)["y"])
    # one segment without lead, gap, fade or trim is the plain call
    plain, ol = path.call(hip_tiny.synthesize, ids[:1], lens[:1], SCALES, sid[:1], seed=SEED)
    one, info = path.call(hip_tiny.synthesize_document, ids[:1], lens[:1], SCALES, sid[:1], seed=SEED)
    assert one.tobytes() == plain[0, :ol[0]].tobytes() and info["seg_end"].tolist() == [int(ol[0])]


@pytest.mark.parametrize("fast", (True, False), ids=("fast", "eager"))
def test_document_trims_on_the_device(lib, hip_tiny, feed, batch, fast):
    ids, lens, sid = feed
    hop = hip_tiny.hp.hop_length
    ref = batch[fast]
    # a threshold just above the quietest first or last frame of any row: that frame goes, the loudest frame stays
    edge = min(min(float(D.frame_peaks(r, n, hop)[0]), float(D.frame_peaks(r, n, hop)[-1])) for r, n in zip(ref["rows"], ref["frames"]))
    assert 0 < edge * 1.05 < 1  # (a negative dBFS value)
    trim_db = 20.0 * np.log10(edge * 1.05)
    for keep in (0, 1):
        want = D.join(ref["rows"], ref["frames"], hop, 0, GAPS, 5, trim_db, keep)
        if keep == 0:
            assert sum(want["n"]) < int(ref["frames"].sum()), "no frame is trimmed"
        assert sum(want["n"]) > 0, "no frame is kept"
        got, info = _Path(lib, fast).call(hip_tiny.synthesize_document, ids, lens, SCALES, sid, seed=SEED, gap_frames=GAPS, fade_samples=5,
                                          trim_db=trim_db, trim_keep_frames=keep)
        print(f"trim_db {trim_db:.2f} keep {keep}: lo {want['lo']} hi {want['hi']} of {ref['frames'].tolist()}")
        assert info["trim"][:, 0].tolist() == want["lo"] and info["trim"][:, 1].tolist() == want["hi"]
        assert got.tobytes() == want["y"].tobytes()


@pytest.mark.parametrize("fast", (True, False), ids=("fast", "eager"))
def test_document_int16(lib, hip_tiny, feed, batch, fast):
    ids, lens, sid = feed
    hop = hip_tiny.hp.hop_length
    ref, path = batch[fast], _Path(lib, fast)
    rows16, ol = path.call(hip_tiny.synthesize_pcm16, ids, lens, SCALES, sid, pcm_scale=0.9, seed=SEED, solo=True)
    assert (ol // hop).tolist() == ref["frames"].tolist()
    want = D.join(rows16.astype(np.float32), ref["frames"], hop, 2, GAPS, 0)["y"]  # (int16 values are exact in fp32)
    got, _ = path.call(hip_tiny.synthesize_document, ids, lens, SCALES, sid, seed=SEED, pcm=True, pcm_scale=0.9, lead_frames=2, gap_frames=GAPS)
    assert got.dtype == np.int16 and got.tobytes() == want.astype(np.int16).tobytes()
    # with a fade: the float document through the conversion's rule
    want = D.pcm16(D.join(ref["rows"], ref["frames"], hop, 2, GAPS, 9)["y"], 0.9)
    got, _ = path.call(hip_tiny.synthesize_document, ids, lens, SCALES, sid, seed=SEED, pcm=True, pcm_scale=0.9, lead_frames=2, gap_frames=GAPS,
                       fade_samples=9)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("rate", (None, 8000), ids=("native", "8000"))
@pytest.mark.parametrize("fast", (True, False), ids=("fast", "eager"))
def test_document_marks(lib, hip_tiny, feed, batch, fast, rate):
    ids, lens, sid = feed
    hop = hip_tiny.hp.hop_length
    ref = batch[fast]
    edge = min(float(D.frame_peaks(r, n, hop)[0]) for r, n in zip(ref["rows"], ref["frames"]))
    for trim_db in (None, 20.0 * np.log10(edge * 1.05)):
        lay = D.join(ref["rows"], ref["frames"], hop, 2, GAPS, 0, trim_db, 0)
        s0, s1, ends, total = D.marks(lay, ref["cum"], lens, hop, NATIVE, rate)
        got, info = _Path(lib, fast).call(hip_tiny.synthesize_document, ids, lens, SCALES, sid, seed=SEED, lead_frames=2, gap_frames=GAPS,
                                          trim_db=trim_db, marks=True, sample_rate=rate)
        assert got.shape == (total,)
        assert info["seg_start"].tolist() == s0 and info["seg_end"].tolist() == s1
        assert info["token_ends"].tolist() == ends.tolist()
        flat = [int(info["token_ends"][b, t]) for b in range(3) for t in range(int(lens[b]))]
        assert flat == sorted(flat) and flat[-1] <= total
        assert all(s0[b] <= info["token_ends"][b, 0] and info["token_ends"][b, lens[b] - 1] <= s1[b] for b in range(3))


@pytest.mark.parametrize("fast", (True, False), ids=("fast", "eager"))
def test_per_item_stages_stay_per_item(lib, hip_tiny, feed, fast):
    """pitch=+2 for the call and a contour on segment 1: the join of the flagged batch call's rows"""
    ids, lens, sid = feed
    hop = hip_tiny.hp.hop_length
    tp = np.zeros(ids.shape, np.float32)
    tp[1, :int(lens[1])] = np.linspace(-3.0, 4.0, int(lens[1]))
    kw = dict(seed=SEED, pitch=2.0, token_pitch=tp)
    path = _Path(lib, fast)
    rows, ol = path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, solo=True, **kw)
    plain, _ = path.call(hip_tiny.synthesize, ids, lens, SCALES, sid, solo=True, seed=SEED)
    assert not np.array_equal(rows, plain)
    want = D.join(rows, ol // hop, hop, 1, GAPS, 9)
    got, _ = path.call(hip_tiny.synthesize_document, ids, lens, SCALES, sid, lead_frames=1, gap_frames=GAPS, fade_samples=9, **kw)
    assert got.tobytes() == want["y"].tobytes()


def test_refusals_leave_the_model_usable(lib, hip_tiny, feed, batch):
    from vosk_tts_amd.capi import VitsError, c_f32p, c_i64p, _p

    ids, lens, sid = feed
    hop = hip_tiny.hp.hop_length

    def refused(what, **kw):
        with pytest.raises(VitsError) as e:
            hip_tiny.synthesize_document(ids, lens, SCALES, sid, seed=SEED, **kw)
        assert e.value.code == 1 and what in str(e.value), (what, str(e.value))  # VITS_ERR_ARG

    refused("gap_frames -1 of segment 1", gap_frames=[0, -1, 0])
    refused(f"fade_samples {hop // 2 + 1}", fade_samples=hop // 2 + 1)
    refused("trim_db 3", trim_db=3.0)
    refused("trim_db nan", trim_db=float("nan"))
    refused("trim_db -inf", trim_db=float("-inf"))
    refused("trim_keep_frames -1", trim_keep_frames=-1)
    refused("lead_frames -2", lead_frames=-2)
    refused("2^31", gap_frames=[0, 2 ** 31 // hop, 0])
    refused("2^31", gap_frames=[2 ** 30 // hop, 2 ** 30 // hop - 4, 0])  # (only with the frames themselves: refused behind phase 1)
    out, ns = c_f32p(), ctypes.c_int64()
    sc = np.asarray(SCALES, np.float32)
    rc = lib._fn("synthesize_document")(hip_tiny._h, _p(ids, c_i64p), _p(lens, c_i64p), 3, ids.shape[1], _p(sc, c_f32p), _p(sid, c_i64p), None, None,
                                        0, ctypes.byref(out), ctypes.byref(ns), None)
    assert rc == 1 and b"NULL" in lib._fn("last_error")()
    rows, ol = hip_tiny.synthesize(ids, lens, SCALES, sid, seed=SEED, solo=True)
    assert rows.tobytes() == batch[True]["rows"].tobytes()
    got, _ = hip_tiny.synthesize_document(ids, lens, SCALES, sid, seed=SEED, gap_frames=GAPS)
    assert got.tobytes() == D.join(rows, ol // hop, hop, 0, GAPS)["y"].tobytes()


# ---- 5. the stages behind the join see one item --------------------------------------------------------------------------------------
def test_the_resampler_sees_one_item(lib, hip_tiny, feed, batch):
    """Bound, as tests/test_resample_gpu.py: resample_ref.fp32_bound, the worst-case error of an fp32 sum of `taps` products, at the
    joined signal's max |x|, against the float64 restatement applied to the reference join."""
    import resample_ref

    ids, lens, sid = feed
    hop = hip_tiny.hp.hop_length
    x = D.join(batch[True]["rows"], batch[True]["frames"], hop, 2, GAPS, 9)["y"]
    got, info = hip_tiny.synthesize_document(ids, lens, SCALES, sid, seed=SEED, lead_frames=2, gap_frames=GAPS, fade_samples=9, sample_rate=8000)
    P = resample_ref.plan(NATIVE, 8000)
    want = resample_ref.resample(x, NATIVE, 8000)
    bound = resample_ref.fp32_bound(lib.resample_table(NATIVE, 8000), np.abs(x).max())
    assert got.shape == want.shape == (resample_ref.n_out(x.shape[0], P["L"], P["M"]),)
    err = float(np.abs(got - want).max())
    print(f"document at 8000 Hz: err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    # across a gap the joined signal is resampled as one: an item resampled alone would end in its own filter tail
    via_op = lib.op_resample(x[None], [x.shape[0]], NATIVE, 8000)[0]
    assert np.abs(got - via_op).max() <= bound


def test_loudness_and_limiter_see_one_item(lib, hip_tiny, feed, batch):
    """Bounds, as tests/test_limit_gpu.py's two-pass form: the measured loudness within 0.01 LU of the float64 restatement's, the returned
    gain within 10^(0.02/20) - 1 of its g_1, and the audio the one-pass limiter at the returned gain, bit for bit."""
    import limit_ref
    import loudness_ref
    from vosk_tts_amd.capi import limit_spec, loudness_spec

    ids, lens, sid = feed
    hop = hip_tiny.hp.hop_length
    x = D.join(batch[True]["rows"], batch[True]["frames"], hop, 2, GAPS, 9)["y"]
    L0, pk = loudness_ref.integrated(x, NATIVE), float(np.abs(x).max())
    target = min(0.0, L0 + 6.0)
    c = min(1.0, 1.2 * pk)
    ref = limit_ref.loudness_limit(x, NATIVE, target, limit_ref.TRUE, c, 5.0, 50.0)
    out = {}
    got, info = hip_tiny.synthesize_document(ids, lens, SCALES, sid, seed=SEED, lead_frames=2, gap_frames=GAPS, fade_samples=9,
                                             loudness=loudness_spec(loudness=target, peak_ceiling=0.0), limit=limit_spec("true", c), loudness_out=out)
    assert sorted(out) == ["gain", "loudness", "reduction"] and all(v.shape == (1,) for v in out.values())
    rel = abs(float(out["gain"][0]) / ref["g1"] - 1.0)
    print(f"document: L {out['loudness'][0]:.3f} vs {ref['L']:.3f}, gain {out['gain'][0]:.6f} vs g_1 {ref['g1']:.6f} (rel {rel:.2e}), "
          f"reduction {out['reduction'][0]:.4f} vs {ref['reduction']:.4f}")
    assert abs(float(out["loudness"][0]) - ref["L"]) <= 0.01
    assert rel <= 10.0 ** (0.02 / 20.0) - 1.0
    one, red = lib.op_limit(x[None], [x.shape[0]], NATIVE, limit_ref.TRUE, c, gain=float(out["gain"][0]))
    assert got.tobytes() == one[0].tobytes() and red[0] == out["reduction"][0] and red[0] < 1
    # the batch call measures every sentence on its own: other numbers
    per = {}
    hip_tiny.synthesize(ids, lens, SCALES, sid, seed=SEED, solo=True, loudness=loudness_spec(loudness=target, peak_ceiling=0.0), loudness_out=per)
    print(f"per sentence: {per['loudness'].tolist()}")
    assert per["loudness"].shape == (3,) and all(abs(float(v) - float(out["loudness"][0])) > 0.01 for v in per["loudness"])


# ---- 8. the multistream family ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def voice(tmp_path_factory):
    from vosk_tts_amd import Model
    from vosk_tts_amd.toymodel import write_toy_multistream_model

    d = str(tmp_path_factory.mktemp("ms"))
    write_toy_multistream_model(d)
    model = Model(model_path=d, device=0)
    yield model
    model.onnx.close()


def test_stts_document_equals_the_joined_batch(lib, voice):
    sess = voice.onnx
    hop, native = sess._vocoder.hp.hop_length, sess._vocoder.hp.sampling_rate
    B, T = 3, 14
    lens = np.array([T, 9, 4], np.int64)
    ids = np.stack([np.random.default_rng(10 + b).integers(1, 40, size=(5, T)).astype(np.int64) for b in range(B)])
    pde = np.full((B, T), 3.0, np.float32)
    sc = np.array([0.8, 1.0, 0.8], np.float32)
    kw = dict(seed=0, n_timesteps=2, item_seeds=[5, 6, 7], pitch=2.0)
    for rate in (None, 8000):
        rows, ol, ends = sess._model.synthesize_batch(ids, lens, sc, [0, 1, 2], None, pde, marks=True, **kw)
        assert not (ol % hop).any()
        frames, cum = ol // hop, ends // hop
        want = D.join(rows, frames, hop, 1, GAPS, 9)
        s0, s1, tok, total = D.marks(want, cum, lens, hop, native, rate)
        got, info = sess._model.synthesize_document(ids, lens, sc, [0, 1, 2], None, pde, marks=True, sample_rate=rate, lead_frames=1,
                                                    gap_frames=GAPS, fade_samples=9, **kw)
        assert got.shape == (total,) and info["seg_start"].tolist() == s0 and info["seg_end"].tolist() == s1
        assert info["token_ends"].tolist() == tok.tolist()
        if rate is None:
            assert got.tobytes() == want["y"].tobytes()
        else:  # the joined signal through the resampler's own door, as that family's tail crosses the host
            assert got.tobytes() == lib.op_resample(want["y"][None], [want["y"].shape[0]], native, rate)[0].tobytes()
    from vosk_tts_amd.capi import VitsError

    with pytest.raises(VitsError, match="gap_frames -2 of segment 0"):
        sess._model.synthesize_document(ids, lens, sc, [0, 1, 2], None, pde, gap_frames=[-2, 0, 0], **kw)
    with pytest.raises(ValueError, match="a stream cannot take a document"):
        sess.run_stream(None, {"input": ids[:1], "input_lengths": lens[:1], "scales": sc, "vits.doc_lead_frames": 1})


# ---- 9. through Synth, both families -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from vosk_tts_amd import Model, Synth
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.toymodel import PHONEMES, write_toy_model

    d = write_toy_model(str(tmp_path_factory.mktemp("vits") / "m"), W.default_hparams(n_vocab=len(PHONEMES)))
    model = Model(model_path=d, device=0)
    yield Synth(model)
    model.onnx.close()


SSML = ('<speak><s>прив+ет, м+ир!</s><voice name="1"><s>м+ир прив+ет?</s></voice><s>прив+ет.</s></speak>')


def _check_document(synth, family):
    from vosk_tts_amd import ssml as S

    rate, hop = synth.native_rate(), synth.hop_length()
    audio, sm = synth.synth_document_ssml(SSML, marks=True, seed=21, speaker_id=0, fade_ms=0.0, scale=1.0)
    assert audio.dtype == np.int16 and audio.ndim == 1
    # the length: the end of the last segment plus the trailing gap (the end of the document ends a paragraph: 0.6 s)
    assert audio.shape[0] == sm.segments[-1][1] + D.frames(0.6, rate, hop) * hop
    assert [b - a for a, b in sm.segments] and all(a < b for a, b in sm.segments) and sm.segments[1][0] == sm.segments[0][1] + D.frames(0.2, rate, hop) * hop
    # the words of the document are the words of its segments
    plan = S.parse_document(SSML)
    per = [synth.synth_audio(s.text, speaker_id=s.speaker_id or 0, marks=True)[1] for s in plan.segments]
    assert len(sm.words) == sum(len(p.words) for p in per) == 5 and [w[0] for w in sm.words] == [w[0] for p in per for w in p.words]
    assert sm.word_segment == [0, 0, 1, 1, 2]
    # the <voice name="1"> segment is, in the document, that sentence's row of the same batch under speaker 1
    a, b = sm.segments[1]
    feed, scale = synth._document_feed(plan.segments, 0, None, None, None, 1.0)
    assert feed["sid"].tolist() == [0, 1, 0]
    feed["vits.seed"] = 21
    sess = synth.model.onnx
    if family == "vits":
        rows, ol = sess.run_pcm16(dict(feed, **{"vits.solo": True}), scale, return_lengths=True)
        other, _ = sess.run_pcm16(dict(feed, sid=np.zeros(3, np.int64), **{"vits.solo": True}), scale, return_lengths=True)
    else:
        rows, ol = sess.run_batch(feed)
        other, _ = sess.run_batch(dict(feed, sid=np.zeros(3, np.int64)))
        rows, other = synth.audio_float_to_int16(rows * scale), synth.audio_float_to_int16(other * scale)
    assert audio[a:b].tobytes() == rows[1, :int(ol[1])].tobytes() and not np.array_equal(rows[1], other[1])
    assert audio[sm.segments[0][0]:sm.segments[0][1]].tobytes() == rows[0, :int(ol[0])].tobytes()
    with pytest.raises(ValueError, match="synth_stream cannot take document="):
        next(synth.synth_stream("м+ир", document="м+ир. м+ир."))


def test_synth_document_vits_session(toy):
    _check_document(toy, "vits")
    # plain text: the splitter, one call; a whole-output loudness target is met by the document, not by every sentence
    text = "прив+ет, м+ир! м+ир прив+ет?\n\nприв+ет."
    plain = toy.synth_document(text, seed=3, scale=1.0)
    l0, _ = toy.measure_loudness(plain)
    target = float(max(round(l0 - 6.0), -60))
    got = toy.synth_document(text, seed=3, scale=1.0, loudness=target)
    lufs, pk = toy.measure_loudness(got)
    print(f"document {l0:.2f} LUFS; target {target}: {lufs:.3f} LUFS peak {pk:.3f}")
    assert got.shape == plain.shape and pk < 0.99 and abs(lufs - target) <= 0.05  # (the bound of tests/test_loudness_gpu.py's Synth test)


def test_synth_document_multistream_session(voice):
    from vosk_tts_amd import Synth

    _check_document(Synth(voice), "multistream")
