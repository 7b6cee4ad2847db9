"""Synth.front_batch on the HIP library (one stts_bert_feed_batch call per batch) against the per-request front end, and
MultiDeviceSynth with the batched front end on (the default) and off."""
import numpy as np
import pytest

from conftest import assert_close

pytestmark = pytest.mark.gpu

STAGE_TOL = 1e-4

TEXTS = ["прив+ет, м+ир!", "м+ир", "прив+еты м+иру, да-нет.", "м+ир прив+ет?", "... прив+ет ?!"]
SIDS, SEEDS = [2, 0, 4, 1, 3], [101, 7, 33, 58, 4]


def _write(tmp_path, voice):
    from vosk_tts_amd.toymodel import write_toy_model, write_toy_multistream_model

    if voice in ("g2p", "g2p_noblank"):
        return write_toy_model(str(tmp_path / "m"), bert=True, no_blank=int(voice == "g2p_noblank"))
    return write_toy_multistream_model(str(tmp_path / "ms"), model_type=voice, with_bert=True)


def _texts(voice):
    return [t.replace(" м+ир", " _ м+ир") for t in TEXTS] if voice == "multistream_v3" else TEXTS


@pytest.mark.parametrize("voice", ["g2p", "g2p_noblank", "multistream_v1", "multistream_v2", "multistream_v3"])
def test_front_batch_feed_vs_per_request_feed(tmp_path, voice):
    from vosk_tts_amd import Model, Synth

    model = Model(model_path=_write(tmp_path, voice), device=0)
    try:
        assert model.bert_onnx.has_batch
        synth = Synth(model)
        texts = _texts(voice)
        fb = synth.front_batch(texts, SIDS)
        for b, text in enumerate(texts):
            args, _ = synth._feed(text, SIDS[b], None, None, None, None)
            L = int(args["input_lengths"][0])
            assert fb["input_lengths"][b] == L and np.array_equal(fb["input"][b, ..., :L], args["input"][0])
            rel = assert_close(f"{voice}: bert feed of {text!r}", args["bert"][0], fb["bert"][b, :, :L], 2 * STAGE_TOL)
            print(f"{voice} item {b}: rel err {rel:.3e}")
            assert not fb["bert"][b, :, L:].any()
    finally:
        model.bert_onnx.close()
        model.onnx.close()


@pytest.mark.parametrize("voice,lsb", [("g2p", 1), ("multistream_v3", 2)])
def test_multi_device_synth_with_the_batched_front_end_on_and_off(tmp_path, voice, lsb):
    """Off: bit for bit what the per-request code gives (it is the per-request code).  On (the default): every request has the length
    of its solo call and lies within the bound the existing batch tests of its family use (tests/test_host_api.py: 1 LSB for the
    BERT-conditioned VITS voices, 2 for multistream)."""
    from vosk_tts_amd import Model, Synth
    from vosk_tts_amd.batching import BATCHED_FRONT_MIN, MultiDeviceSynth, plan_shards

    d = _write(tmp_path, voice)
    texts = _texts(voice)
    on = MultiDeviceSynth(d, devices=[0], max_batch=2)  # five requests: two parts of two through front_batch, the part of one per request
    off = MultiDeviceSynth(d, devices=[0], max_batch=2, batched_front=False)
    model = Model(model_path=d, device=0)
    try:
        assert on.batched_front and not off.batched_front and on._front_is_batched(0, 2) and not off._front_is_batched(0, 2)
        assert not on._front_is_batched(0, BATCHED_FRONT_MIN - 1)  # (profiles/bert_batch_bench.txt: one sentence is a tie)
        got_off = off.synth_batch(texts, speaker_ids=SIDS, seeds=SEEDS)
        # the per-request code itself, on the same plan
        s0 = off.synths[0]
        norm = [s0.normalize(t) for t in texts]
        scales, scale, sids, seeds = off._call_params(len(texts), SIDS, None, None, None, None, SEEDS)
        idx = plan_shards([len(s0.phonemize(t.replace("_", " "))) for t in norm], 1)[0]
        run = off._run_shard_bert if off.family == "vits_bert" else off._run_shard_multistream
        direct = run(0, norm, idx, sids, scales, scale, seeds, per_request=True)
        for i, pcm in zip(idx, direct):
            assert got_off[i].dtype == np.int16 and np.array_equal(got_off[i], pcm), i
        got_on = on.synth_batch(texts, speaker_ids=SIDS, seeds=SEEDS)
        synth = Synth(model)
        for i, t in enumerate(texts):
            f, sc = synth._feed(t, SIDS[i], None, None, None, None)
            if off.family == "vits_bert":
                want = model.onnx.run_pcm16(dict(f, **{"vits.seed": SEEDS[i]}), 1.0)[0]
            else:
                want = synth.audio_float_to_int16(model.onnx.run(None, dict(f, **{"vits.seed": SEEDS[i]}))[0][0] * sc)
            assert got_on[i].dtype == np.int16 and got_on[i].shape == want.shape == got_off[i].shape, (i, got_on[i].shape, want.shape)
            diff = np.abs(got_on[i].astype(np.int32) - want.astype(np.int32)).max()
            print(f"{voice} request {i}: max |batched front - solo| = {diff} LSB")
            assert diff <= lsb, i
    finally:
        on.close()
        off.close()
        model.onnx.close()
