"""stts_bert_encode_batch / stts_bert_feed_batch (include/stts_bert_batch.h): a padded batch of sentences in one forward, and the
acoustic models' phoneme feed gathered from it on the device.  The CPU oracle encodes one sentence per call; every item of a batch is
compared with the oracle's result for that sentence alone, at the bound test_bert_base_geometry_vs_oracle uses for this encoder."""
import numpy as np
import pytest

from conftest import assert_close

pytestmark = pytest.mark.gpu

STAGE_TOL = 1e-4
TOL = 2 * STAGE_TOL
VITS_ERR_ARG = 1

SMALL_LENS = [1, 7, 8, 9, 33]  # the shortest sentence; both sides of the 8-column bucket and of a 16-key tile; past one 32-query tile
BASE8_LENS = [70, 3, 64, 65, 17, 33, 1, 48]
BASE2_LENS = [70, 2]


def _sentences(rng, lens, vocab):
    return [rng.integers(0, vocab, size=L).astype(np.int64) for L in lens], [rng.integers(0, 2, size=L).astype(np.int64) for L in lens]


def _padded(seqs, T, garbage):
    """[B, T] with the sentences in front and `garbage` (two values that are an error wherever they are read) behind them"""
    a = np.empty((len(seqs), T), np.int64)
    a[:, 0::2], a[:, 1::2] = garbage[0], garbage[1]
    for b, s in enumerate(seqs):
        a[b, :len(s)] = s
    return a


@pytest.fixture(scope="module")
def small(hip_lib, oracle_lib):
    from vosk_tts_amd import weights_bert as BW
    from vosk_tts_amd.capi_stts import BertEncoder

    hp = BW.small_hparams(120, 128, 4)
    blob = BW.synthetic_blob(hp, 1234)
    hip, ref = BertEncoder(hip_lib, blob), BertEncoder(oracle_lib, blob)
    assert hip.has_batch and not ref.has_batch
    ids, types = _sentences(np.random.default_rng(41), SMALL_LENS, hp.vocab_size)
    want = [ref.encode(i, t) for i, t in zip(ids, types)]
    yield {"hip": hip, "ref": ref, "hp": hp, "ids": ids, "types": types, "want": want, "garbage": (hp.vocab_size + 5, -3)}
    hip.close()
    ref.close()


@pytest.fixture(scope="module")
def base(hip_lib, oracle_lib):
    """rubert-base geometry; the eight sentences of the B = 8 case and their oracle rows (the B = 2 case reuses sentence 0)"""
    from vosk_tts_amd import weights_bert as BW
    from vosk_tts_amd.capi_stts import BertEncoder

    hp = BW.base_hparams(300)
    blob = BW.synthetic_blob(hp, 7)
    hip, ref = BertEncoder(hip_lib, blob), BertEncoder(oracle_lib, blob)
    rng = np.random.default_rng(43)
    ids, _ = _sentences(rng, BASE8_LENS, hp.vocab_size)
    short = rng.integers(0, hp.vocab_size, size=2).astype(np.int64)
    want = [ref.encode(i) for i in ids]
    yield {"hip": hip, "hp": hp, "ids": ids, "want": want, "short": short, "want_short": ref.encode(short)}
    hip.close()
    ref.close()


def _small_call(s, ids=None, garbage=None):
    ids = s["ids"] if ids is None else ids
    g = s["garbage"] if garbage is None else garbage
    T = max(SMALL_LENS)
    return s["hip"].encode_batch_padded(_padded(ids, T, g), _padded(s["types"], T, g), SMALL_LENS)


def test_small_geometry_one_call_vs_oracle_per_item(small):
    out = _small_call(small)
    assert out.shape == (5, 33, 128)
    for b, L in enumerate(SMALL_LENS):
        rel = assert_close(f"item {b} (length {L})", small["want"][b], out[b, :L], TOL)
        print(f"item {b} length {L}: rel err {rel:.3e}")
        assert not out[b, L:].any(), f"item {b}: rows beyond its length are not zero"
    # the list form pads for the caller and hands back the valid rows
    got = small["hip"].encode_batch(small["ids"], small["types"])
    assert [g.shape for g in got] == [(L, 128) for L in SMALL_LENS]
    for b, L in enumerate(SMALL_LENS):
        assert np.array_equal(got[b], out[b, :L])


def test_padding_and_neighbours_do_not_leak(small):
    first = _small_call(small)
    rng = np.random.default_rng(42)
    others, _ = _sentences(rng, SMALL_LENS[:4], small["hp"].vocab_size)
    second = _small_call(small, others + [small["ids"][4]], (-(1 << 40), small["hp"].vocab_size))
    assert np.array_equal(first[4], second[4])
    assert not np.array_equal(first[3, :9], second[3, :9])  # (the neighbours did change)


@pytest.mark.parametrize("case", ["mfma32_B8", "q16_8wave_B2"])
def test_the_other_two_attention_kernels(hip_lib, base, case):
    hp, T = base["hp"], 70
    if case == "mfma32_B8":
        lens, ids, want, kernel = BASE8_LENS, base["ids"], base["want"], "relpos_attention_mfma_kernel"
    else:  # T > 64: the 16-query kernel runs 8 waves per workgroup (launch_relpos_attention_on)
        lens, ids, want, kernel = BASE2_LENS, [base["ids"][0], base["short"]], [base["want"][0], base["want_short"]], "relpos_attention16_kernel"
    padded = _padded(ids, T, (hp.vocab_size + 5, -3))
    hip_lib.launch_log(1)
    try:
        out = base["hip"].encode_batch_padded(padded, None, lens)
    finally:
        hip_lib.launch_log(0)
    n_att = hip_lib.launch_count("attention", "")
    assert n_att == hp.out_layers and hip_lib.launch_count("attention", kernel) == n_att, hip_lib.launch_dump()
    for b, L in enumerate(lens):
        rel = assert_close(f"{case} item {b} (length {L})", want[b], out[b, :L], TOL)
        print(f"{case} item {b} length {L}: rel err {rel:.3e}")
        assert not out[b, L:].any()


def test_feed_batch_is_exactly_a_gather_of_encode_batch(small):
    hip = small["hip"]
    enc = hip.encode_batch(small["ids"], small["types"])
    rows = [np.array([0, 0, -1, 0], np.int32),                       # repeats of the only row
            np.arange(6, -1, -1, dtype=np.int32),                    # reversed
            np.array([-1, 7, 7, 3, -1, -1, 0, 7, 2], np.int32),      # gaps
            np.array([8], np.int32),                                 # one column, the last row
            np.concatenate([np.arange(33), np.arange(32, -1, -1), [-1, 16, 16, 16]]).astype(np.int32)]  # T_x > T: 70 columns, two blocks
    T_x = 71  # ragged: every list is padded with -1
    out = hip.feed_batch(small["ids"], rows, T_x=T_x, token_type_ids=small["types"])
    assert out.shape == (5, 128, T_x)
    for b, r in enumerate(rows):
        for t in range(T_x):
            if t < len(r) and r[t] >= 0:
                assert np.array_equal(out[b, :, t], enc[b][r[t]]), (b, t)
            else:
                assert not out[b, :, t].any(), (b, t)
    assert np.array_equal(hip.feed_batch(small["ids"], rows, token_type_ids=small["types"]), out[:, :, :70])  # T_x defaults to the longest list


def test_refusals_name_the_value_and_leave_the_model_usable(small):
    from vosk_tts_amd.capi import VitsError

    hip, ids, types = small["hip"], small["ids"], small["types"]
    T = 33
    pid, pty = _padded(ids, T, (0, 0)), _padded(types, T, (0, 0))
    lens = np.array(SMALL_LENS, np.int32)
    rows = np.zeros((5, 4), np.int32)

    def good():
        out = hip.encode_batch_padded(pid, pty, lens)
        for b, L in enumerate(SMALL_LENS):
            assert_close(f"after a refusal, item {b}", small["want"][b], out[b, :L], TOL)

    def refused(match, fn):
        with pytest.raises(VitsError, match=match) as e:
            fn()
        assert e.value.code == VITS_ERR_ARG, e.value
        good()

    bad_rows = rows.copy(); bad_rows[2, 3] = 8  # == lengths[2]
    refused(r"rows\[2, 3\] = 8", lambda: hip.feed_batch_padded(pid, pty, lens, bad_rows))
    zero = lens.copy(); zero[1] = 0
    refused(r"lengths\[1\] = 0", lambda: hip.encode_batch_padded(pid, pty, zero))
    long = lens.copy(); long[3] = 34
    refused(r"lengths\[3\] = 34", lambda: hip.feed_batch_padded(pid, pty, long, rows))
    big = small["hp"].max_position + 1
    refused(rf"{big} tokens exceed max_position {small['hp'].max_position}",
            lambda: hip.encode_batch_padded(np.zeros((1, big), np.int64), None, np.array([big], np.int32)))
    # an id out of range in a valid column: what the single-sentence call answers
    with pytest.raises(VitsError, match="token id") as solo:
        hip.encode(np.array([1, 2, 9999]))
    bad = pid.copy(); bad[4, 32] = 9999
    with pytest.raises(VitsError, match="token id") as e:
        hip.encode_batch_padded(bad, pty, lens)
    assert e.value.code == solo.value.code
    good()


def test_the_solo_path_is_untouched_by_batched_calls(hip_lib, small, base):
    """enc.encode before and after batched calls on the same model, bit for bit: a bucket length and a length inside a bucket on the
    graph path, the same on the eager path, and T = 70 (the 8-wave attention, no K-sliced FFN)"""
    rng = np.random.default_rng(44)
    for s, B in ((small, 5), (base, 2)):
        hip, vocab = s["hip"], s["hp"].vocab_size
        sent = [rng.integers(0, vocab, size=T).astype(np.int64) for T in (8, 13, 70)]

        def solo():
            graph = [hip.encode(i) for i in sent]
            hip_lib.lib.vits_debug_fast_path(0)
            try:
                eager = [hip.encode(i) for i in sent]
            finally:
                hip_lib.lib.vits_debug_fast_path(1)
            return graph + eager

        before = solo()
        batch = [s["ids"][0], s["short"]] if B == 2 else s["ids"]
        hip.encode_batch(batch)
        hip.feed_batch(batch, [np.array([0, -1, 0], np.int32)] * B)
        after = solo()
        assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_a_call_beyond_the_workspace_cap_runs_as_sub_batches(base):
    """18 items of 512 columns need more than the 256 MiB a call lays out at once (17 MB an item at this geometry): the library runs
    them as consecutive sub-batches inside the one call.  Items on both sides of every possible cut equal their own one-item calls
    (the bound of the other tests: a batch takes other tiles than one item), rows beyond the length are zero, and the feed is the
    gather of those rows."""
    hip, hp = base["hip"], base["hp"]
    B, T, Tx = 18, 512, 8
    rng = np.random.default_rng(45)
    lens = rng.integers(1, T + 1, size=B).astype(np.int32)
    lens[0], lens[B - 1] = T, 5
    ids = rng.integers(0, hp.vocab_size, size=(B, T)).astype(np.int64)
    rows = np.stack([rng.integers(-1, L, size=Tx) for L in lens]).astype(np.int32)
    whole = hip.encode_batch_padded(ids, None, lens)
    feed = hip.feed_batch_padded(ids, None, lens, rows)
    for b in (0, 13, 14, 15, 16, 17):
        L = int(lens[b])
        alone = hip.encode_batch_padded(ids[b:b + 1], None, lens[b:b + 1])[0]
        assert_close(f"item {b} (length {L}) of the split call", alone[:L], whole[b, :L], TOL)
        assert not whole[b, L:].any()
        want = np.where(rows[b][None, :] >= 0, alone[np.maximum(rows[b], 0)].T, 0.0)
        assert_close(f"feed of item {b}", want, feed[b], TOL)
        assert not feed[b][:, rows[b] < 0].any()
