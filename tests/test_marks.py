"""Speech marks (include/vits_marks.h) without a GPU: the integer restatement's own properties, the token -> phoneme -> word mapping
rules of vosk_tts_amd/marks.py against the restatement (tests/marks_ref.py), and the Python surface around the engine."""
import ctypes
import os
import re
import threading
import time

import numpy as np
import pytest

import marks_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 256
RATES = (None, 8000, 48000)


# ---- the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_restatement_properties(rate):
    rng = np.random.default_rng(5)
    L, M = R.ratio(22050, rate)
    for _ in range(20):
        B, T = int(rng.integers(1, 5)), int(rng.integers(1, 40))
        dur = rng.integers(0, 7, size=(B, T)) * (rng.random((B, T)) < 0.7)  # zeros inside
        lens = rng.integers(0, T + 1, size=B)
        lens[0] = T
        if B > 1:
            lens[1] = 0
        ends = R.token_ends(dur, lens, HOP, 22050, rate)
        assert ends.dtype == np.int64 and ends.shape == (B, T)
        assert (np.diff(ends, axis=1) >= 0).all() and (ends >= 0).all()
        for b in range(B):
            n = int(lens[b])
            if n == 0:
                assert not ends[b].any()
                continue
            total = int(dur[b, :n].sum())
            assert ends[b, n - 1] == R.n_out(total * HOP, L, M)
            assert (ends[b, n:] == ends[b, n - 1]).all()  # the padding rule
            if total:
                assert ends[b, n - 1] == R.out_lengths(dur, lens, HOP, 22050, rate)[b]
            else:  # the clamp exception: one frame of audio that belongs to no token
                assert R.out_lengths(dur, lens, HOP, 22050, rate)[b] == R.n_out(HOP, L, M) and not ends[b].any()
            for t in range(n):
                if dur[b, t] == 0:  # a token of zero frames has an empty span
                    assert ends[b, t] == (ends[b, t - 1] if t else 0)


def test_n_out_is_the_resamplers_rule():
    from vosk_tts_amd import marks as M

    for rate in (8000, 16000, 44100, 48000, 22050, None):
        L, Mm = R.ratio(22050, rate)
        assert (L, Mm) == M.rate_ratio(22050, rate)
        for x in (0, 1, 255, 256, 12345, 2 ** 33 + 7):
            assert M.n_out(x, L, Mm) == R.n_out(x, L, Mm) == (x * L + Mm - 1) // Mm


# ---- mapping rules ------------------------------------------------------------------------------------------------------------
DIC = {"привет": "p rj i0 vj e1 t", "мир": "mj i1 r"}
TEXT = 'Прив+ет, "м+ир" - да!'


class _Model:
    def __init__(self, id_map, model_type="vits", tokenizer=None, no_blank=0):
        self.dic = dict(DIC)
        self.tokenizer = tokenizer
        self.onnx = None
        self.config = {"phoneme_id_map": id_map, "inference": {}, "model_type": model_type, "no_blank": no_blank}


def _phonemes_of_word(w):
    from vosk_tts_amd.g2p import convert

    return (DIC[w] if w in DIC else convert(w)).split()


def _ends_for(n_tokens, seed, rate=None):
    rng = np.random.default_rng(seed)
    dur = rng.integers(0, 5, size=(1, n_tokens))
    dur[0, rng.integers(0, n_tokens)] = 0
    return R.token_ends(dur, [n_tokens], HOP, 22050, rate)[0]


def _check_tiling(marks, ends):
    assert marks.phonemes[0][1] == 0 and marks.phonemes[-1][2] == int(ends[-1])
    for (_, _, e0), (_, s1, _) in zip(marks.phonemes, marks.phonemes[1:]):
        assert e0 == s1, "phoneme spans must tile the utterance without gaps"
    assert all(s <= e for _, s, e in marks.phonemes)
    starts = [s for _, s, _ in marks.words]
    assert starts == sorted(starts)


@pytest.mark.parametrize("front", ["g2p", "g2p_noblank", "g2p_noembed", "g2p_noembed_lists"])
@pytest.mark.parametrize("text", [TEXT, "м+ир", "!"])
def test_vits_mapping_rules(front, text):
    from vosk_tts_amd.synth import Synth
    from vosk_tts_amd.toymodel import phoneme_id_map

    id_map = phoneme_id_map()
    if front == "g2p_noembed_lists":  # list-valued id map (synth.py:241-246): every second phoneme gets two ids
        id_map = {p: ([i, i] if i % 2 else [i]) for p, i in id_map.items()}
    tok = object() if front in ("g2p", "g2p_noblank") else None
    s = Synth(_Model(id_map, tokenizer=tok, no_blank=1 if front == "g2p_noblank" else 0))
    norm = s.normalize(text)
    symbols, owner, words = R.vits_words(norm, _phonemes_of_word)
    assert symbols == s.phonemize(norm)
    if front == "g2p":
        ids, _ = s.g2p(norm, np.arange(64))
    elif front == "g2p_noblank":
        ids, _ = s.g2p_noblank(norm, np.arange(64))
    else:
        ids = s.g2p_noembed(norm)
    for rate in RATES:
        ends = _ends_for(len(ids), len(ids) + (rate or 0), rate)
        got = s._marks(text, ends, rate or 22050)
        if front == "g2p_noblank":
            want_ph = R.phonemes_plain(ends, symbols)
        else:
            per = [len(id_map[p]) if isinstance(id_map[p], list) else 1 for p in symbols]
            want_ph = R.phonemes_blank(ends, symbols, per)
            if front != "g2p_noembed_lists":  # phoneme 0 is token 0, phoneme k the blank 2k-1 plus token 2k
                assert want_ph[0][1:] == (0, int(ends[0])) and all(p[2] == int(ends[2 * k]) for k, p in enumerate(want_ph))
        assert got.phonemes == want_ph
        assert got.words == R.words_from(want_ph, owner, words)
        assert got.rate == (rate or 22050) and np.array_equal(got.token_ends, ends)
        _check_tiling(got, ends)
        sec = got.seconds()
        assert sec["phonemes"][-1][2] == pytest.approx(int(ends[-1]) / got.rate)
    if text == TEXT:
        assert [w[0] for w in got.words] == ["прив+ет", "м+ир", "да"]
    if text == "!":
        assert got.words == [] and [p[0] for p in got.phonemes] == ["^", "!", "$"]


@pytest.mark.parametrize("model_type,text", [("multistream_v2", 'Прив+ет, "м+ир" да... нет!'), ("multistream_v2", "!"),
                                             ("multistream_v3", 'Прив+ет, "м+ир" _ да... нет!'), ("multistream_v3", "!")])
def test_multistream_mapping_rules(model_type, text):  # (the '_' pause mark is a token of v3 only)
    from vosk_tts_amd.multistream import g2p_multistream
    from vosk_tts_amd.synth import Synth
    from vosk_tts_amd.toymodel import multistream_phoneme_id_map

    id_map = multistream_phoneme_id_map()
    v3 = model_type == "multistream_v3"
    s = Synth(_Model(id_map, model_type, tokenizer=object() if v3 else None))
    norm = s.normalize(text)
    plain = g2p_multistream(norm, s.model.dic, id_map, None, word_pos=not v3, pause_marks=v3)
    res = g2p_multistream(norm, s.model.dic, id_map, None, word_pos=not v3, pause_marks=v3, return_words=True)
    assert res[:-1] == plain, "existing callers must be unaffected by the optional return"
    symbols, widx, wtexts = res[-1]
    assert len(symbols) == len(plain[0]) and symbols[0] == "^" and symbols[-1] == "$"
    if v3 and text != "!":
        assert 20.0 in plain[2] and "_" not in wtexts.values()  # the '_' pause is a mark on a boundary, not a word
    ends = _ends_for(len(symbols), 99)
    got = s._marks(text, ends, 22050)
    want_ph = R.phonemes_plain(ends, symbols)
    assert got.phonemes == want_ph
    assert got.words == R.multistream_words(want_ph, widx, wtexts)
    _check_tiling(got, ends)
    if text == "!":
        assert got.words == []
    else:
        assert [w[0] for w in got.words] == ["прив+ет", "м+ир", "да", "нет"]
        for _, a, b in got.words:  # no word contains a space symbol's span it does not own: words lie between boundaries
            inside = [p for p in got.phonemes if a <= p[1] and p[2] <= b and p[1] < p[2]]
            assert all(p[0] not in ("^", "$") for p in inside)


def test_layout_mismatch_is_an_error():
    from vosk_tts_amd import marks as M

    with pytest.raises(ValueError, match="layout"):
        M.phoneme_spans([10, 20, 30], [1, 1, 1], blank=True)  # three phonemes with blanks need five tokens


# ---- bindings ------------------------------------------------------------------------------------------------------------------
def _prototypes():
    """{name: [argument types as written]} of include/vits_marks.h"""
    hdr = open(os.path.join(ROOT, "include", "vits_marks.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+((?:vits|stts)_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr):
        out[name] = [re.sub(r"\s*\b[A-Za-z_][A-Za-z0-9_]*$", "", a.strip()).replace(" ", "") for a in args.split(",")]
    return out


_C = {"vits_model*": ctypes.c_void_p, "stts_model*": ctypes.c_void_p, "vits_stream*": ctypes.c_void_p,
      "constint64_t*": ctypes.POINTER(ctypes.c_int64), "int64_t*": ctypes.POINTER(ctypes.c_int64), "int32_t": ctypes.c_int32,
      "int64_t": ctypes.c_int64, "float": ctypes.c_float, "constfloat*": ctypes.POINTER(ctypes.c_float),
      "int32_t*": ctypes.POINTER(ctypes.c_int32), "float**": ctypes.POINTER(ctypes.POINTER(ctypes.c_float)),
      "int16_t**": ctypes.POINTER(ctypes.POINTER(ctypes.c_int16))}


def test_header_prototypes_match_the_ctypes_declarations(hip_lib, oracle_lib):
    from vosk_tts_amd import capi

    protos = _prototypes()
    assert sorted(protos) == ["stts_synthesize_batch_marks", "stts_synthesize_marks", "vits_stream_marks", "vits_synthesize_marks",
                              "vits_synthesize_pcm16_marks"]
    for name, args in protos.items():
        assert hasattr(hip_lib.lib, name), f"libvits_mi355.so lacks {name}"
        if name.startswith("stts_"):  # (declared when an SttsModel is made, which needs a device: checked from the source below)
            continue
        fn = getattr(hip_lib.lib, name)
        got = fn.argtypes
        assert got is not None and len(got) == len(args), (name, args)
        for i, (a, g) in enumerate(zip(args, got)):
            want = ctypes.POINTER(capi.SynthOpts) if a == "constvits_synth_opts*" else _C[a]
            assert g == want or (want is ctypes.c_void_p and g is ctypes.c_void_p), (name, i, a, g)
    # declared only where the symbols exist
    assert hip_lib.has_marks and not oracle_lib.has_marks
    assert not any(hasattr(oracle_lib.lib, "vitsref_" + n[5:]) or hasattr(oracle_lib.lib, "sttsref_" + n[5:]) for n in protos)


def test_stts_prototypes_match_their_ctypes_declarations():
    """the multistream pair: the argtypes lists in capi_stts.py, read from its source (an SttsModel needs a device to exist)"""
    from vosk_tts_amd import capi_stts

    protos = _prototypes()
    src = open(capi_stts.__file__).read()
    for short in ("synthesize_marks", "synthesize_batch_marks"):
        m = re.search(r'f\("' + short + r'"\)\.argtypes = \[(.*?)\]\n', src, flags=re.S)
        assert m, short
        decl = [a.strip() for a in re.sub(r"\s+", " ", m.group(1)).split(", ")]
        args = protos["stts_" + short]
        assert len(decl) == len(args), (short, decl, args)
        names = {"vp": ("vits_model*", "stts_model*"), "c_i64p": ("constint64_t*", "int64_t*"), "ctypes.c_int32": ("int32_t",),
                 "ctypes.c_int64": ("int64_t",), "c_f32p": ("constfloat*",), "ctypes.POINTER(SttsOpts)": ("conststts_synth_opts*",),
                 "ctypes.POINTER(c_f32p)": ("float**",)}
        for d, a in zip(decl, args):
            assert a in names[d], (short, d, a)


def test_oracle_backend_refuses_marks_and_says_why(oracle_tiny):
    from vosk_tts_amd.capi import VitsError
    from vosk_tts_amd.session import VitsSession

    ids = np.ones((1, 5), np.int64)
    with pytest.raises(VitsError, match="no speech marks") as e:
        oracle_tiny.synthesize(ids, [5], [0.6, 1.0, 0.8], [0], marks=True)
    assert e.value.code == 4 and "oracle" in str(e.value)
    sess = VitsSession.__new__(VitsSession)
    sess._lib = oracle_tiny.lib
    with pytest.raises(VitsError, match="no speech marks"):
        sess._marks({"vits.marks": True})
    assert sess._marks({}) is False


def test_cli_has_a_marks_flag():
    from vosk_tts_amd import cli

    ap = cli.build_parser()
    assert ap.parse_args([]).marks is None
    assert ap.parse_args(["--marks", "m.json"]).marks == "m.json"


def test_marks_json_carries_samples_and_seconds():
    import json

    from vosk_tts_amd.marks import SpeechMarks

    m = SpeechMarks(8000, [4000, 8000], [("^", 0, 4000), ("$", 4000, 8000)], [("да", 0, 8000)])
    d = json.loads(m.to_json())
    assert d["rate"] == 8000 and d["words"] == [{"text": "да", "start_sample": 0, "end_sample": 8000, "start": 0.0, "end": 1.0}]
    assert d["phonemes"][1] == {"symbol": "$", "start_sample": 4000, "end_sample": 8000, "start": 0.5, "end": 1.0}
    assert m.seconds()["words"] == [("да", 0.0, 1.0)]


# ---- the coalescer ---------------------------------------------------------------------------------------------------------------
class _Hp:
    sampling_rate, hop_length, bert_dim, n_speakers = 22050, 256, 0, 4


class _EngineStub:
    """stands where capi.VitsModel stands; the first call waits for `gate`, so that the others queue up behind it"""

    def __init__(self):
        self.hp = _Hp()
        self.calls = []
        self.gate = threading.Event()
        self.entered = threading.Event()
        self._lock = threading.Lock()

    def synthesize_pcm16(self, ids, lens, scales, sid, pcm_scale=1.0, seed=0, solo=False, item_seeds=None, sample_rate=None, marks=False, **kw):
        with self._lock:
            first = not self.calls
            self.calls.append((ids.shape[0], bool(marks)))
        if first:
            self.entered.set()
            assert self.gate.wait(30)
        B, T = ids.shape
        out = (np.zeros((B, 8), np.int16), np.full(B, 8, np.int64))
        return out + (np.tile(np.arange(1, T + 1, dtype=np.int64) * 3, (B, 1)),) if marks else out

    def close(self):
        pass


class _LibStub:
    is_device = True
    has_marks = True

    def __init__(self):
        self.model = _EngineStub()

    def create(self, blob, device):
        return self.model

    def _need_marks(self):
        pass


def test_coalescer_never_hands_a_non_marks_caller_a_tuple():
    from vosk_tts_amd.session import VitsSession

    lib = _LibStub()
    sess = VitsSession(b"", lib=lib, max_inflight=1)
    eng = lib.model
    want_marks = [False, True, False, True, True, False, False, True]
    lens = [5, 3, 4, 5, 2, 5, 1, 4]
    results = [None] * len(want_marks)

    def worker(i):
        feed = {"input": np.ones((1, 5), np.int64), "input_lengths": np.array([lens[i]]), "scales": np.array([0.8, 1.0, 0.8], np.float32),
                "sid": np.array([1])}
        if want_marks[i]:
            feed["vits.marks"] = True
        results[i] = sess.run_pcm16(feed, 1.0)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(len(want_marks))]
    threads[0].start()
    assert eng.entered.wait(30)
    for t in threads[1:]:
        t.start()
    deadline = time.monotonic() + 30
    while len(sess.coalescer._queue) < len(want_marks) - 1 and time.monotonic() < deadline:
        time.sleep(0.001)
    assert len(sess.coalescer._queue) == len(want_marks) - 1
    eng.gate.set()
    for t in threads:
        t.join(30)
    for i, (m, out) in enumerate(zip(want_marks, results)):
        if not m:
            assert isinstance(out, np.ndarray) and out.dtype == np.int16, (i, type(out))
        else:
            pcm, ends = out
            assert isinstance(pcm, np.ndarray) and pcm.dtype == np.int16 and ends.dtype == np.int64 and ends.shape == (1, 5)
            n = lens[i]  # its own tokens' ends, then the padding rule
            assert ends[0, :n].tolist() == [3 * (t + 1) for t in range(n)] and (ends[0, n:] == 3 * n).all()
    # no engine call served both kinds, and the queued requests of one kind did share calls
    assert sess.coalescer.calls < len(want_marks) and max(c[0] for c in eng.calls) > 1
    assert sum(c[0] for c in eng.calls if c[1]) == 4 and {c[1] for c in eng.calls} == {False, True}


# ---- Synth ---------------------------------------------------------------------------------------------------------------------
class _SessionStub:
    def __init__(self):
        self.feeds = []

    def run(self, names, feed):
        self.feeds.append(feed)
        T = feed["input"].shape[1]
        out = [np.zeros((1, 1, 1, 256 * T), np.float32)]
        if feed.get("vits.marks"):
            out.append((np.arange(1, T + 1, dtype=np.int64) * 256)[None])
        return out

    def run_stream(self, names, feed, chunk_frames=64, on_marks=None):
        T = feed["input"].shape[1]
        if on_marks is not None:
            on_marks(np.arange(1, T + 1, dtype=np.int64) * 256)
        for _ in range(3):
            yield np.zeros(100, np.float32)


def test_synth_audio_default_is_a_bare_array_and_marks_is_a_pair():
    from vosk_tts_amd.synth import Synth
    from vosk_tts_amd.toymodel import phoneme_id_map

    m = _Model(phoneme_id_map())
    m.onnx = _SessionStub()
    s = Synth(m)
    a = s.synth_audio("м+ир, да")
    assert isinstance(a, np.ndarray) and "vits.marks" not in m.onnx.feeds[-1]
    a2, marks = s.synth_audio("м+ир, да", marks=True)
    assert m.onnx.feeds[-1]["vits.marks"] is True and np.array_equal(a, a2)
    assert marks.rate == 22050 and marks.phonemes[-1][2] == len(a2) and [w[0] for w in marks.words] == ["м+ир", "да"]
    calls = []
    chunks = []
    for c in s.synth_stream("м+ир, да", on_marks=lambda mk: calls.append((mk, len(chunks)))):
        chunks.append(c)
    assert len(calls) == 1 and calls[0][1] == 0 and calls[0][0] == marks and len(chunks) == 3
    assert len(list(s.synth_stream("м+ир, да"))) == 3  # without the callback the session is called as before
