"""Every call that reaches the C ABI for a matrix of output-tail requests, as stable text (tests/test_tail_calls.py compares it line for
line with tests/golden/tail_calls.txt, which is this tool's output for the commit BEFORE the Python tail was refactored).

A `Recorder` stands where the CDLL stands: every vits_* / stts_* symbol appends a record (symbol, scalar arguments, and for each struct
passed by reference its class, sizeof, flags and fields) and returns 0.  No library is loaded and no device is touched; the models and
sessions are made with __new__ around it.  The matrix goes through names that exist on both sides of such a refactor only: the sessions'
run* methods, _run_solo_batch with a key captured from coalescer.submit, and MultiDeviceSynth's shard runners.

    python tools/tail_calls.py [--package-root DIR] [--out FILE]      # DIR: the tree whose vosk_tts_amd is recorded (default: this one)

Reading a record: `symbol(arg, ...)`; `h` a handle, `NULL` / `&` a pointer, `&<16 hex>` an input array with the head of the sha256 of
its contents (only where the shape follows from B and T_x), `out` a result the recorder filled, `{Class/sizeof field=value ...}` a struct
(fields that are 0 / NULL are left out; `flags` is always there).  Every call returns N_OUT samples per item from a zeroed buffer, so the
host chains behind a call (resample -> mark -> normalise) run and show up in call order.
"""
import argparse
import ctypes
import hashlib
import itertools
import os
import sys
import threading

import numpy as np

N_OUT = 4           # samples (or frames) every synthesize call "returns"
PLAN = (2, 3, 16, 8)  # vits_resample_plan's answer: L, M, taps, half
KEY = 0x5EED1234
RATE = 16000


def _sha(ptr, n):
    size = n * ctypes.sizeof(ptr._type_)
    return hashlib.sha256(ctypes.string_at(ctypes.cast(ptr, ctypes.c_void_p).value, size)).hexdigest()[:16] if size else "empty"


# symbol (without prefix and _rate / _marks / _pcm16 endings) -> argument position -> element count from (B, T, bert_dim)
def _layout(name):
    if name.startswith("vits_synthesize"):
        return (3, 4), {1: lambda B, T, D: B * T, 2: lambda B, T, D: B, 5: lambda B, T, D: 3, 6: lambda B, T, D: B}
    if name.startswith("vits_stream_open") and "latent" not in name:
        return (None, 2), {1: lambda B, T, D: T, 3: lambda B, T, D: 3}
    if name.startswith(("stts_synthesize_batch", "stts_synthesize_document")):
        return (3, 4), {1: lambda B, T, D: B * 5 * T, 2: lambda B, T, D: B, 5: lambda B, T, D: 3, 6: lambda B, T, D: B,
                        7: lambda B, T, D: B * D * T, 8: lambda B, T, D: B * T}
    if name.startswith(("stts_synthesize", "stts_stream_open")):
        return (None, 2), {1: lambda B, T, D: 5 * T, 3: lambda B, T, D: 3, 5: lambda B, T, D: D * T, 6: lambda B, T, D: T}
    return None, {}


# pointer fields of the structs that are inputs of a known shape
_FIELD_COUNT = {"item_seeds": lambda B, T, D: B, "forced_durations": lambda B, T, D: B * T, "bert": lambda B, T, D: B * D * T,
                "item_scales": lambda B, T, D: B * 3, "token_length_scale": lambda B, T, D: B * T, "token_pause": lambda B, T, D: B * T,
                "fit_frames": lambda B, T, D: B, "token_semitones": lambda B, T, D: B * T, "token_gain_db": lambda B, T, D: B * T,
                "gap_frames": lambda B, T, D: B, "watermark_payloads": lambda B, T, D: B}


def _all_fields(cls):
    out = []
    for c in reversed(cls.__mro__):
        out += list(c.__dict__.get("_fields_", []))
    return out


class _Symbol:
    def __init__(self, rec, name):
        self._rec, self._name = rec, name

    def __call__(self, *args):
        return self._rec.call(self._name, args)


class Recorder:
    def __init__(self, bert_dim=0):
        self.records = []
        self._syms = {}
        self._buf = (ctypes.c_char * (1 << 16))()
        self.bert_dim = bert_dim

    def __getattr__(self, name):
        if not name.startswith(("vits_", "stts_")):
            raise AttributeError(name)
        return self._syms.setdefault(name, _Symbol(self, name))

    def _struct(self, s, dims):
        parts = [f"{type(s).__name__}/{ctypes.sizeof(s)}"]
        for name, typ in _all_fields(type(s)):
            v = getattr(s, name)
            if isinstance(v, ctypes._Pointer):
                if not v:
                    continue
                if issubclass(typ._type_, ctypes.Structure):
                    parts.append(f"{name}=&{self._struct(v.contents, dims)}")
                elif name in _FIELD_COUNT and dims is not None:
                    parts.append(f"{name}=&{_sha(v, _FIELD_COUNT[name](*dims))}")
                else:
                    parts.append(f"{name}=&")
            elif isinstance(v, ctypes.Array):
                parts.append(f"{name}={list(v)}")
            elif v or name == "flags":
                parts.append(f"{name}={v!r}")
        return "{" + " ".join(parts) + "}"

    def call(self, name, args):
        if name.endswith(("_free_output", "_free_pcm16", "_destroy", "_stream_close")):
            return None
        bt, hashed = _layout(name)
        dims = None
        if bt is not None:
            dims = (1 if bt[0] is None else int(args[bt[0]]), int(args[bt[1]]), self.bert_dim)
        plan = iter(PLAN)
        out = []
        for i, a in enumerate(args):
            if a is None:
                out.append("NULL")
            elif isinstance(a, (bool, int, float)):
                out.append(repr(a))
            elif isinstance(a, ctypes.c_void_p):
                out.append("h")
            elif isinstance(a, ctypes._Pointer):
                out.append("NULL" if not a else "&" + (_sha(a, hashed[i](*dims)) if i in hashed else ""))
            elif hasattr(a, "_obj"):  # byref(...)
                o = a._obj
                if isinstance(o, ctypes.Structure):
                    out.append(self._struct(o, dims))
                elif isinstance(o, ctypes._Pointer):  # a result buffer: N_OUT zero samples per item
                    o.contents = o._type_.from_buffer(self._buf)
                    out.append("out")
                elif isinstance(o, ctypes.c_void_p):
                    o.value = 16
                    out.append("out")
                else:
                    o.value = next(plan) if name.endswith("_resample_plan") else N_OUT if isinstance(o, ctypes.c_int64) else 0
                    out.append("out")
            else:
                out.append(type(a).__name__)
        self.records.append(f"{name}({', '.join(out)})")
        return 0


# ---- the objects around the recorder --------------------------------------------------------------------------------------------------
def _lib(P, bert_dim=0):
    lib = P.capi.VitsLib.__new__(P.capi.VitsLib)
    lib.lib = Recorder(bert_dim)
    lib.prefix, lib.path, lib.is_device = "vits_", "<recorder>", True
    for k in ("resample", "denoise", "marks", "loudness", "pitch", "pitch_formant", "limit", "prosody", "contour", "document", "intonation",
              "watermark", "watermark_payload"):
        setattr(lib, "has_" + k, True)
    return lib


def _vits_model(P, lib, **hp):
    m = P.capi.VitsModel.__new__(P.capi.VitsModel)
    m.lib, m._h, m.device = lib, ctypes.c_void_p(), 0
    m.hp = P.weights.HParams()
    for k, v in dict({"sampling_rate": 22050, "hop_length": 256, "bert_dim": 0, "n_speakers": 4, "inter_channels": 4}, **hp).items():
        setattr(m.hp, k, v)
    return m


def vits_session(P):
    lib = _lib(P)
    s = P.session.VitsSession.__new__(P.session.VitsSession)
    s._lib, s._model = lib, _vits_model(P, lib)
    s.hp = s._model.hp
    s._seed, s._seed_lock, s._ps_timeouts = itertools.count(1), threading.Lock(), 0
    s.coalescer = P.session.RequestCoalescer(s._run_solo_batch, 32, 8, 0)
    return s


BERT, FEATS = 8, 4


def stts_session(P):
    lib = _lib(P, BERT)
    s = P.session_stts.SttsSession.__new__(P.session_stts.SttsSession)
    s._lib = lib
    s._vocoder = _vits_model(P, lib, inter_channels=FEATS)
    m = P.capi_stts.SttsModel.__new__(P.capi_stts.SttsModel)
    m.vlib, m.prefix, m._vocoder, m._h = lib, "stts_", s._vocoder, ctypes.c_void_p()
    m.has_marks = m.has_document = True
    m.hp = P.weights_stts.SttsHParams()
    m.hp.n_feats, m.hp.bert_dim, m.hp.hop_length, m.hp.sampling_rate = FEATS, BERT, 256, 22050
    s._model, s.hp = m, m.hp
    s._seed, s._seed_lock = itertools.count(1), threading.Lock()
    return s


class _Synth:
    """stands where Synth stands for the shard runners: the per-request front end of a multistream voice, and the voice's config"""

    def __init__(self, sess):
        self.model = type("M", (), {"config": {"inference": {}}, "onnx": sess, "tokenizer": None})()

    @staticmethod
    def _feed(text, sid, *_):
        T = len(text)
        return {"input": np.arange(5 * T, dtype=np.int64).reshape(1, 5, T) % 7, "bert": np.full((1, BERT, T), 0.25, np.float32),
                "phone_duration_extra": None}, None

    @staticmethod
    def audio_float_to_int16(a):
        return np.zeros(a.shape, np.int16)


def multi_device(P, sess, family, run):
    """run(a MultiDeviceSynth of one stub replica around `sess`)"""
    from concurrent.futures import ThreadPoolExecutor

    M = P.batching.MultiDeviceSynth
    m = M.__new__(M)
    m.devices, m.max_batch, m.batched_front, m.family = [0], 32, False, family
    m.synths = [_Synth(sess)]
    m.models = [m.synths[0].model]
    m._replica_locks, m._lock, m._seed = [threading.Lock()], threading.Lock(), 0
    m._pool = ThreadPoolExecutor(max_workers=1)
    try:
        return run(m)
    finally:
        m._pool.shutdown(wait=True)


# ---- the matrix -----------------------------------------------------------------------------------------------------------------------
def _contour(B, T, neutral=False):
    a = np.zeros((B, T), np.float32)
    if not neutral:
        a[:, 1] = 2.0
    return {"vits.token_pitch": a, "vits.token_gain_db": a * (-1.5)}


EVERYTHING = {"vits.loudness": -16.0, "vits.limit": "true", "vits.peak_ceiling": 0.89, "vits.limit_lookahead_ms": 2.0, "vits.limit_release_ms": 80.0,
              "vits.pitch": -5, "vits.pitch_formants": True, "vits.pitch_range": 0.5, "vits.watermark_key": KEY, "vits.watermark_depth_db": 1.5}

# name -> (B, T) -> the extension feeds; "arrays": such a request is not coalesced and is no fragment of MultiDeviceSynth's
SETTINGS = [
    ("none", lambda B, T: {}),
    ("lufs", lambda B, T: {"vits.loudness": -16.0}),
    ("peak", lambda B, T: {"vits.peak": 0.5, "vits.peak_ceiling": 0.9}),
    ("limit", lambda B, T: {"vits.limit": "true", "vits.peak_ceiling": 0.89}),
    ("lufs+limit", lambda B, T: {"vits.loudness": -16.0, "vits.limit": "sample", "vits.limit_release_ms": 80.0}),
    ("pitch", lambda B, T: {"vits.pitch": -5}),
    ("pitch+formants", lambda B, T: {"vits.pitch": 3.0, "vits.pitch_formants": True}),
    ("formants", lambda B, T: {"vits.pitch_formants": True}),
    ("pitch0", lambda B, T: {"vits.pitch": 0.0}),
    ("range", lambda B, T: {"vits.pitch_range": 0.5}),
    ("range1.0004", lambda B, T: {"vits.pitch_range": 1.0004}),
    ("wm", lambda B, T: {"vits.watermark_key": KEY}),
    ("wm+depth", lambda B, T: {"vits.watermark_key": 5, "vits.watermark_depth_db": 0.5}),
    ("contour", _contour),
    ("contour0", lambda B, T: _contour(B, T, True)),
    ("item_scales", lambda B, T: {"vits.item_scales": np.tile(np.array([[0.5, 1.25, 0.25]], np.float32), (B, 1))}),
    ("all", lambda B, T: dict(EVERYTHING, **_contour(B, T))),
]
ARRAYS = ("contour", "contour0", "item_scales", "all")
FAULTS = [("wm-1", {"vits.watermark_key": -1}), ("depth3", {"vits.watermark_key": KEY, "vits.watermark_depth_db": 3.0}),
          ("depth-no-key", {"vits.watermark_depth_db": 1.0}), ("peak+limit", {"vits.limit": "sample", "vits.peak": 0.5}),
          ("limit-bogus", {"vits.limit": "bogus"}), ("pitch12.5", {"vits.pitch": 12.5})]
DOC = {"vits.doc_gap_frames": [3, 0], "vits.doc_lead_frames": 2, "vits.doc_fade_samples": 64, "vits.doc_trim_db": -40.0, "vits.doc_trim_keep": 1}


def vits_feed(B, T, **ext):
    return dict({"input": (np.arange(B * T, dtype=np.int64).reshape(B, T) % 7) + 1, "input_lengths": np.full(B, T, np.int64),
                 "scales": np.array([0.8, 1.0, 0.8], np.float32), "sid": np.arange(B, dtype=np.int64) % 4}, **ext)


def stts_feed(B, T, batch, **ext):
    ids = (np.arange(B * 5 * T, dtype=np.int64).reshape(B, 5, T) % 7) + 1
    bert = np.full((B, BERT, T), 0.5, np.float32)
    f = {"input": ids, "input_lengths": np.full(B, T, np.int64), "scales": np.array([0.6, 1.0, 0.7], np.float32),
         "sid": np.arange(B, dtype=np.int64), "bert": bert}
    if batch:
        f["vits.item_seeds"] = np.arange(B, dtype=np.uint64) + 11
    return dict(f, **ext)


def _rm(rate, marks):
    return dict({"vits.sample_rate": RATE} if rate else {}, **({"vits.marks": True} if marks else {}))


def cases(P):
    """-> (label, make_session, run(session)) for every request of the matrix"""
    for name, ext in SETTINGS:
        for rate, marks in itertools.product((False, True), (False, True)):
            tag = f"{name} rate={int(rate)} marks={int(marks)}"
            rm = _rm(rate, marks)
            yield f"vits.run B=1 {tag}", vits_session, lambda s, e=ext, rm=rm: s.run(None, vits_feed(1, 5, **e(1, 5), **rm))
            yield f"vits.run_pcm16 B=1 {tag}", vits_session, lambda s, e=ext, rm=rm: s.run_pcm16(vits_feed(1, 5, **e(1, 5), **rm), 0.5)
            yield (f"vits.run_pcm16 B=2 {tag}", vits_session,
                   lambda s, e=ext, rm=rm: s.run_pcm16(vits_feed(2, 4, **e(2, 4), **rm), 1.0, return_lengths=True))
            if name not in ARRAYS:
                yield f"vits._run_solo_batch 2 requests {tag}", vits_session, lambda s, e=ext, rm=rm: _solo_batch(s, e(1, 5), rm)
            yield f"stts.run {tag}", stts_session, lambda s, e=ext, rm=rm: s.run(None, stts_feed(1, 5, False, **e(1, 5), **rm))
            yield f"stts.run_batch {tag}", stts_session, lambda s, e=ext, rm=rm: s.run_batch(stts_feed(2, 4, True, **e(2, 4), **rm))
            if name not in ARRAYS or name == "all":
                frag = {k: v for k, v in ext(1, 5).items() if not isinstance(v, np.ndarray)}  # (what Synth hands MultiDeviceSynth)
                yield (f"mds.synth_tokens {tag}", vits_session,
                       lambda s, f=frag, r=rate, m=marks: multi_device(P, s, "vits", lambda mds: mds.synth_tokens(
                           [[1, 2, 3, 4], [5, 6, 7]], [0, 1], None, None, None, None, [7, 8], RATE if r else None, m, f)))
                yield (f"mds._run_shard_multistream {tag}", stts_session,
                       lambda s, f=frag, r=rate, m=marks: multi_device(P, s, "multistream", lambda mds: mds._run_shard_multistream(
                           0, ["abcd", "efg"], [0, 1], [0, 1], np.array([0.6, 1.0, 0.7], np.float32), 1.0, [7, 8], True, RATE if r else None, 0.01, m, f)))
        for rate in (False, True):
            rm = _rm(rate, False)
            yield f"vits.run_stream {name} rate={int(rate)}", vits_session, lambda s, e=ext, rm=rm: s.run_stream(None, vits_feed(1, 5, **e(1, 5), **rm))
            yield f"stts.run_stream {name} rate={int(rate)}", stts_session, lambda s, e=ext, rm=rm: s.run_stream(None, stts_feed(1, 5, False, **e(1, 5), **rm))
    for rate, marks in itertools.product((False, True), (False, True)):
        tag = f"all rate={int(rate)} marks={int(marks)}"
        rm = _rm(rate, marks)
        for pcm in (False, True):
            yield (f"vits.run_document pcm16={int(pcm)} {tag}", vits_session,
                   lambda s, rm=rm, pcm=pcm: s.run_document(vits_feed(2, 4, **EVERYTHING, **_contour(2, 4), **DOC, **rm), 0.5, pcm))
        yield f"vits.run (document) {tag}", vits_session, lambda s, rm=rm: s.run(None, vits_feed(2, 4, **EVERYTHING, **DOC, **rm))
        yield (f"stts.run_document {tag}", stts_session,
               lambda s, rm=rm: s.run_document(stts_feed(2, 4, True, **EVERYTHING, **_contour(2, 4), **DOC, **rm)))
    yield "vits.run_document none", vits_session, lambda s: s.run_document(vits_feed(2, 4, **DOC))
    yield "stts.run_document none", stts_session, lambda s: s.run_document(stts_feed(2, 4, True, **DOC))
    yield "vits.run_stream document", vits_session, lambda s: s.run_stream(None, vits_feed(1, 5, **DOC))
    yield "stts.run_stream document", stts_session, lambda s: s.run_stream(None, stts_feed(1, 5, False, **DOC))
    for name, ext in FAULTS:
        yield f"vits.run_pcm16 fault {name}", vits_session, lambda s, e=ext: s.run_pcm16(vits_feed(1, 5, **e), 1.0)
        yield f"vits.run_document fault {name}", vits_session, lambda s, e=ext: s.run_document(vits_feed(2, 4, **e, **DOC))
        yield f"stts.run fault {name}", stts_session, lambda s, e=ext: s.run(None, stts_feed(1, 5, False, **e))
        yield f"stts.run_batch fault {name}", stts_session, lambda s, e=ext: s.run_batch(stts_feed(2, 4, True, **e))
        if name == "peak+limit":  # (on a stream that feed breaks two rules, and which of them is named is not pinned)
            continue
        yield f"vits.run_stream fault {name}", vits_session, lambda s, e=ext: s.run_stream(None, vits_feed(1, 5, **e))
        yield f"stts.run_stream fault {name}", stts_session, lambda s, e=ext: s.run_stream(None, stts_feed(1, 5, False, **e))


def _solo_batch(sess, ext, rm):
    """two requests under the key that run_pcm16 hands the coalescer for this feed (the merged call of a busy server)"""
    keys = []
    submit = sess.coalescer.submit
    sess.coalescer.submit = lambda key, *a: (keys.append(key), submit(key, *a))[1]
    sess.run_pcm16(vits_feed(1, 5, **ext, **rm), 1.0)
    del sess._lib.lib.records[:]  # (the lone call is the run_pcm16 case's; what is recorded here is the batch)
    sess._run_solo_batch(keys[0], [(np.ones((1, 4), np.int64), 0, 1, (0.8, 1.0, 0.8)), (np.full((1, 3), 2, np.int64), 1, 2, (0.8, 1.25, 0.8))])


def dump(package_root=None):
    """the records of the whole matrix as text: one `== label` line per request, then its calls in order and, where the request was
    refused, the exception's type and message"""
    if package_root:
        sys.path.insert(0, os.path.abspath(package_root))
    import importlib

    P = type("P", (), {n: importlib.import_module("vosk_tts_amd." + n)
                       for n in ("capi", "capi_stts", "session", "session_stts", "batching", "weights", "weights_stts")})
    lines = []
    for label, make, run in cases(P):
        sess = make(P)
        lines.append("== " + label)
        err = None
        try:
            run(sess)
        except Exception as e:  # a refusal is part of the record
            err = f"!! {type(e).__name__}: {e}"
        lines += sess._lib.lib.records
        if err:
            lines.append(err)
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--package-root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("--out")
    a = ap.parse_args()
    text = dump(a.package_root)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(f"{text.count(chr(10))} lines, {len(text)} bytes, sha256 {hashlib.sha256(text.encode()).hexdigest()}")
