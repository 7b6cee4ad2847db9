"""Synth.front_batch against Synth._feed, text by text, on toy voices with a stub BERT session (no GPU): the stub hands both sides the
same floats, so an exact comparison of the `bert` feed tests the row maps front_batch composes from the existing front ends.  Plus the
ABI of include/stts_bert_batch.h: exported by the product library, bound with the header's argument kinds."""
import ctypes
import json
import os
import re
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TEXTS = ["м+ир",                              # one word
         "прив+ет, м+ир!",
         "... прив+ет ?! , м+ир .",            # punctuation-only neighbours
         "прив+еты м+иру, да",                # words of several word pieces
         "да-нет — прив+ет - м+ир",            # hyphens (and the dash normalize() rewrites)
         "\"прив+ет\" (м+ир): нет; да?"]
TEXTS_V3 = [t.replace(" м+ир", " _ м+ир") for t in TEXTS]  # forced pauses -> phone_duration_extra


class _StubBert:
    """`encode`: a fixed random [T, 768] per token list; `feed_batch`: the gather of those rows, in numpy"""
    has_batch = True

    def __init__(self):
        self.solo_calls = self.batch_calls = 0

    def _hidden(self, ids):
        ids = np.asarray(ids, np.int64).reshape(-1)
        return np.random.default_rng(zlib.crc32(ids.tobytes())).standard_normal((ids.shape[0], 768)).astype(np.float32)

    def encode(self, input_ids, token_type_ids=None):
        self.solo_calls += 1
        return self._hidden(input_ids)

    def run(self, output_names, feed):
        assert np.all(np.asarray(feed["attention_mask"]) == 1) and len(feed["token_type_ids"][0]) == len(feed["input_ids"][0])
        return [self.encode(feed["input_ids"][0])]

    def feed_batch(self, id_lists, row_lists, T_x=None, token_type_ids=None):
        self.batch_calls += 1
        assert token_type_ids is None or [len(t) for t in token_type_ids] == [len(i) for i in id_lists]
        T_x = max(len(r) for r in row_lists) if T_x is None else T_x
        out = np.zeros((len(id_lists), 768, T_x), np.float32)
        for b, (ids, rows) in enumerate(zip(id_lists, row_lists)):
            h = self._hidden(ids)
            for t, r in enumerate(rows):
                assert r < len(ids)
                if r >= 0:
                    out[b, :, t] = h[r]
        return out


class _DirModel:
    """what Model reads from a voice directory for the front end (dictionary, config, tokenizer), with the stub in place of the sessions"""

    def __init__(self, path):
        self.dic, probs = {}, {}
        with open(os.path.join(path, "dictionary"), encoding="utf-8") as f:
            for line in f:
                items = line.split(maxsplit=2)
                if len(items) == 3 and probs.get(items[0], 0) < float(items[1]):
                    self.dic[items[0]], probs[items[0]] = items[2], float(items[1])
        with open(os.path.join(path, "config.json")) as f:
            self.config = json.load(f)
        self.tokenizer, self.bert_onnx = None, _StubBert()
        vocab = os.path.join(path, "bert", "vocab.txt")
        if os.path.exists(vocab):
            from tokenizers import BertWordPieceTokenizer

            self.tokenizer = BertWordPieceTokenizer(vocab=vocab, unk_token="[UNK]", lowercase=True)


@pytest.fixture(scope="module")
def voices(tmp_path_factory):
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.toymodel import PHONEMES, write_toy_model, write_toy_multistream_model

    root = tmp_path_factory.mktemp("front_batch")
    v = {}
    for nb in (0, 1):
        v["g2p_noblank" if nb else "g2p"] = write_toy_model(str(root / f"vits{nb}"), W.tiny_hparams(n_vocab=len(PHONEMES)), bert=True, no_blank=nb)
    for mt in ("multistream_v1", "multistream_v2", "multistream_v3"):
        v[mt] = write_toy_multistream_model(str(root / mt), model_type=mt, with_bert=True)
    v["multistream_v2_notok"] = write_toy_multistream_model(str(root / "v2_notok"), model_type="multistream_v2", with_bert=False)
    return v


@pytest.mark.parametrize("voice", ["g2p", "g2p_noblank", "multistream_v1", "multistream_v2", "multistream_v3"])
def test_front_batch_equals_feed_item_by_item(voices, voice):
    from vosk_tts_amd.synth import Synth

    model = _DirModel(voices[voice])
    assert model.tokenizer is not None
    synth = Synth(model)
    texts = TEXTS_V3 if voice == "multistream_v3" else TEXTS
    sids = [3, 0, 1, 4, 2, None]
    fb = synth.front_batch(texts, sids)
    assert model.bert_onnx.batch_calls == 1 and model.bert_onnx.solo_calls == 0
    B, T = len(texts), int(fb["input_lengths"].max())
    assert fb["bert"].shape == (B, 768, T) and fb["bert"].dtype == np.float32 and fb["input"].shape[0] == B and fb["input"].shape[-1] == T
    assert fb["input_lengths"].dtype == np.int64 and fb["sid"].tolist() == [3, 0, 1, 4, 2, 0]
    pieces = [len(model.tokenizer.encode(t.replace("+", "").replace("_", "")).tokens) for t in texts]
    assert len(set(fb["input_lengths"].tolist())) > 2 and max(pieces) > 12  # ragged, and word pieces really occur
    assert any(tok.startswith("##") for tok in model.tokenizer.encode(texts[3].replace("+", "")).tokens)
    for b, text in enumerate(texts):
        args, _ = synth._feed(text, sids[b], None, None, None, None)
        L = int(args["input_lengths"][0])
        assert fb["input_lengths"][b] == L
        assert np.array_equal(fb["input"][b, ..., :L], args["input"][0]) and not fb["input"][b, ..., L:].any()
        assert np.array_equal(fb["bert"][b, :, :L], args["bert"][0]), (voice, text)
        assert np.abs(args["bert"][0]).max() > 0 and not fb["bert"][b, :, L:].any()
        assert fb["sid"][b] == args["sid"][0]
        if voice == "multistream_v3":
            assert np.array_equal(fb["phone_duration_extra"][b, :L], args["phone_duration_extra"][0]) and not fb["phone_duration_extra"][b, L:].any()
        else:
            assert args["phone_duration_extra"] is None
    if voice == "multistream_v3":
        assert fb["phone_duration_extra"].max() == 20.0
    else:
        assert fb["phone_duration_extra"] is None
    assert np.array_equal(synth.front_batch(texts[1:2], 2)["bert"], fb["bert"][1:2, :, :int(fb["input_lengths"][1])])  # a batch of one, scalar sid


def test_front_batch_tokenizerless_v2_is_a_zero_feed_without_a_bert_call(voices):
    from vosk_tts_amd.synth import Synth

    model = _DirModel(voices["multistream_v2_notok"])
    assert model.tokenizer is None
    synth = Synth(model)
    fb = synth.front_batch(TEXTS, 1)
    assert model.bert_onnx.batch_calls == 0 and model.bert_onnx.solo_calls == 0
    assert fb["bert"].shape == (len(TEXTS), 768, int(fb["input_lengths"].max())) and not fb["bert"].any() and fb["phone_duration_extra"] is None
    for b, text in enumerate(TEXTS):
        args, _ = synth._feed(text, 1, None, None, None, None)
        L = int(args["input_lengths"][0])
        assert fb["input_lengths"][b] == L and np.array_equal(fb["input"][b, :, :L], args["input"][0]) and not args["bert"].any()
    # the branches _feed refuses are refused here too
    model.config["model_type"] = "multistream_v1"
    with pytest.raises(NotImplementedError):
        synth.front_batch(TEXTS[:1])


def _batch_header_prototypes():
    """name -> argument kinds ('p' pointer, 'f' floating point, 'i' integer) of the functions include/stts_bert_batch.h declares"""
    text = open(os.path.join(ROOT, "include", "stts_bert_batch.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = {}
    for m in re.finditer(r"\bint\s+(stts_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        args = [a.strip() for a in m.group(2).split(",")]
        protos[m.group(1)] = ["p" if "*" in a else ("f" if re.match(r"(const\s+)?(float|double)\b", a) else "i") for a in args]
    return protos


def _ctypes_kind(t):
    if t in (ctypes.c_float, ctypes.c_double):
        return "f"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or hasattr(t, "contents") or issubclass(t, ctypes._Pointer):
        return "p"
    return "i"


def test_batch_header_is_exported_and_bound_with_its_argument_kinds(hip_lib, oracle_lib):
    from vosk_tts_amd import weights_bert as BW
    from vosk_tts_amd.capi import VitsError
    from vosk_tts_amd.capi_stts import BertEncoder

    protos = _batch_header_prototypes()
    assert sorted(protos) == ["stts_bert_encode_batch", "stts_bert_feed_batch"]
    assert '#include "stts_mi355.h"' in open(os.path.join(ROOT, "include", "stts_bert_batch.h")).read()
    assert "stts_bert_encode_batch" not in open(os.path.join(ROOT, "include", "stts_mi355.h")).read()  # (the oracle mirrors that header)
    for name in protos:
        assert hasattr(hip_lib.lib, name), f"libvits_mi355.so lacks {name}"
    blob = BW.synthetic_blob(BW.small_hparams(120, 64, 2), 1234)
    try:  # the bindings are declared before the model is created: without a GPU the constructor stops at stts_bert_create
        BertEncoder(hip_lib, blob).close()
    except VitsError as e:
        assert "no HIP device" in str(e)
    for name, kinds in protos.items():
        fn = getattr(hip_lib.lib, name)
        assert fn.argtypes is not None and [_ctypes_kind(t) for t in fn.argtypes] == kinds, name
    ref = BertEncoder(oracle_lib, blob)  # the oracle stays a single-sentence encoder: nothing is bound, the methods say so
    assert not ref.has_batch
    with pytest.raises(NotImplementedError):
        ref.encode_batch([[1, 2, 3]])
    with pytest.raises(NotImplementedError):
        ref.feed_batch([[1, 2, 3]], [[0]])
    ref.close()
