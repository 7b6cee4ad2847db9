"""The decoder at every geometry the loader accepts (tests/decoder_grid.py: 43 rows over ResBlock chains / kernels / dilations,
upsampling (rate, kernel) pairs from (1,3) to (8,24), 1-4 stages from 64-512 channels, 11 multi-band / multi-stream tails, 6
single-band iSTFT tails, the plain Generator with and without cond(g)) against the float64 restatement of the reference's modules
(tests/decoder_ref.py, pinned on the CPU by tests/test_decoder_geometry.py).  Per row: dense decodes at T_y 1 / mid / 70 by the
default dispatch and with every conv kernel and the separate tail kernels forced; for chosen rows a batch sized from the dispatch
threshold so that the polyphase upsampler itself takes the 128 x 128 tile (rates 3, 5, 6, 7, 8; asserted from the launch log, not assumed),
ragged batches through vits_synthesize on a poisoned workspace with lengths inside and outside the measured reach, latent streaming
with chunks below and above the reach, the split-bf16 convs (ResBlocks and the polyphase launch, again asserted from the launch log), and
the graph-replayed fast path against the eager one.  A second table lists geometries vits_create must refuse, by error code and message.

Tolerance: STAGE_TOL = 1e-4 on the assert_close scale for every row (fp32 kernels against float64); an indexing error shows up at 1e-1.
Observed on the MI355X (printed per row with -s): WORST below.
"""
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, assert_close
from decoder_grid import GRID, N_GRID, N_REFUSED, REFUSED, measured_field, refused_hparams, row_hparams, row_id
from decoder_ref import decoder_ref

pytestmark = pytest.mark.gpu

STAGE_TOL = 1e-4   # the project's per-stage bound (tests/test_hip_parity.py)
STREAM_TOL = 2e-5  # streaming chunks against the one-shot decode (test_streaming_chunks_equal_one_shot)
BF3_TOL = 5e-5     # split-bf16 against the fp32 kernels (test_bf16x3_decoder_variant)
ROWS = {r[0]: r for r in GRID}
# worst observed error per dec_type, dense legs, every kernel (max abs error / max abs reference):
WORST = {0: "1.54e-06 (mb_default)", 1: "1.37e-06 (hg_v1)", 2: "1.30e-06 (ms_4stage)", 3: "1.40e-06 (is_4stage)"}
# 128 x 128 polyphase legs 1.1e-06 .. 1.5e-06; ragged legs 3.8e-07 .. 5.8e-07; streaming chunks vs one-shot 0 .. 3.0e-07; split-bf16 vs
# float64 2.3e-06 .. 9.2e-06 (ms_u6_u5).  No row came near the cap, and no engine bug was found at any geometry of the grid.

assert len(GRID) == N_GRID == 43 and len(REFUSED) == N_REFUSED == 9
# recorded from the library before the decoder's shape moved into DecGeom (tools/gen_golden_decoder_geom.py --device): per row
# vits_algorithmic_flops(1, 1, 0) / (1, 0, 1), per refused geometry vits_create's code and message
RECORDED = json.load(open(os.path.join(GOLDEN, "decoder_geom.json")))
assert sorted(RECORDED["flops"]) == sorted(ROWS) and sorted(RECORDED["refusals"]) == sorted(e[0] for e in REFUSED)

# (hook, value, restore): every conv kernel the decoder can be forced onto, and the separately written tail kernels
FORCED = [("force_tile", 1, 0), ("force_tile", 2, 0), ("force_tile", 3, 0), ("conv_sp", 2, -1), ("conv_wp", 2, 0), ("tail_impl", 1, 0)]
T_YS = {0: (1, 7, 70), 1: (1, 33, 70), 2: (2, 7, 70)}  # by row index % 3: T_y 1 (or 2), one mid, one that spans several tail blocks


@functools.lru_cache(maxsize=None)
def _weights(name, voice=None, conv_precision=0):
    from vosk_tts_amd import weights as W

    hp = row_hparams(ROWS[name], conv_precision=conv_precision, voice=voice)
    tens = W.make_synthetic_weights(hp, 1234)
    return hp, tens, W.pack_blob(hp, tens)


def _create(hip_lib, name, **kw):
    """vits_create has to accept every row: a VitsError here (any code but VITS_OK) fails the test"""
    return _weights(name, **kw)[:2] + (hip_lib.create(_weights(name, **kw)[2], 0),)


def _not_vacuous(name, a):
    assert np.abs(a).max() > 1e-3 and np.ptp(a) > 1e-3, f"{name}: the reference waveform is (nearly) constant"


def _compare(name, ref, got, tol=STAGE_TOL):
    a, mb = ref
    e = assert_close(f"{name}: audio", a, got[0], tol)
    if mb is not None:
        e = max(e, assert_close(f"{name}: audio_mb", mb, got[1], tol))
    return e


@pytest.mark.parametrize("row", GRID, ids=row_id)
def test_dense_on_every_kernel(hip_lib, row):
    """legs 1 and 2: B = 2, three T_y, default dispatch and every forced kernel, audio and audio_mb against float64"""
    name = row[0]
    hp, tens, model = _create(hip_lib, name)
    rng = np.random.default_rng(100 + GRID.index(row))
    sid = np.array([1, 3], np.int64) if row[8] else None
    worst = 0.0
    try:
        assert [model.algorithmic_flops(1, 1, 0), model.algorithmic_flops(1, 0, 1)] == RECORDED["flops"][name]  # exact: integer-valued doubles
        for Ty in T_YS[GRID.index(row) % 3]:
            z = rng.standard_normal((2, hp.inter_channels, Ty)).astype(np.float32)
            ref = decoder_ref(hp, tens, z, sid=sid)
            assert ref[0].shape == (2, Ty * hp.hop_length)
            if Ty > 2:  # (one or two frames of a long-hop row can be nearly flat; every row also runs the longer lengths, guarded)
                _not_vacuous(name, ref[0])
            e = _compare(f"{name} T_y={Ty} default", ref, model.decoder(z, sid=sid))
            print(f"{name} T_y={Ty} default dispatch: {e:.2e}")
            worst = max(worst, e)
            for hook, val, restore in FORCED:
                fn = getattr(hip_lib.lib, "vits_debug_" + hook)
                try:
                    fn(val)
                    e = _compare(f"{name} T_y={Ty} {hook}({val})", ref, model.decoder(z, sid=sid))
                finally:
                    fn(restore)
                worst = max(worst, e)
        print(f"{name}: worst over kernels and lengths {worst:.2e}")
    finally:
        model.close()


BIG_TILE = "conv_mfma_kernel<2,2,2,2"  # the 128 x 128 fp32 tile (plan_conv, engine_convplan.hip.h)
# (row, B, T_y, upsampler launches that must take the 128 x 128 tile).  A polyphase launch has M = u * C_out rows and T input positions as
# columns; the dispatch takes the big tile when C_out % 128 == 0 and cdiv(M, 128) * cdiv(T, 128) * B >= 512.  Sized from that rule so that
# the "tile inside one phase" indexing (tap_base = ups_shift[m0 / C_out]) runs at rates 5, 6, 3, 7 and 8, several taps and one tap per phase:
#   is_u5_u6        (5,5) 1280 rows x 400, (6,6) 768 x 2000      ms_u6_u5  (6,6) 1536 x 400, (5,5) 640 x 2400
#   mb_8x16_3x9_s1  (8,16) 2048 x 400, (3,9) 384 x 3200          mb_default (4,16) 1024 x 400, (4,16) 512 x 1600
#   ms_u7_2x8       (7,7) 896 x 400 at B = 24 (its second stage has 64 output channels: never the big tile)
BIG_ROWS = (("is_u5_u6", 16, 400, 2), ("ms_u6_u5", 16, 400, 2), ("mb_8x16_3x9_s1", 16, 400, 2), ("mb_default", 16, 400, 2),
            ("ms_u7_2x8", 24, 400, 1))


@pytest.mark.parametrize("name,B,Ty,n_big", BIG_ROWS, ids=[r[0] for r in BIG_ROWS])
def test_polyphase_upsamplers_on_the_128_row_tile(hip_lib, name, B, Ty, n_big):
    """the 128 x 128 tile and its "tile inside one polyphase phase" rule are only reached at size; which kernel each upsampler launch
    took is read from the launch log, so a change of the dispatch that leaves this path untested fails here instead of passing"""
    hp, tens, model = _create(hip_lib, name)
    try:
        z = np.random.default_rng(7).standard_normal((B, hp.inter_channels, Ty)).astype(np.float32)
        ref = decoder_ref(hp, tens, z)
        _not_vacuous(name, ref[0])
        hip_lib.launch_log(1)
        try:
            got = model.decoder(z)
        finally:
            hip_lib.launch_log(0)
        ups, big = hip_lib.launch_count("dec.ups", ""), hip_lib.launch_count("dec.ups", BIG_TILE)
        res_big = hip_lib.launch_count("dec.res_c1", BIG_TILE)
        e = _compare(f"{name} {B}x{Ty}", ref, got)
        print(f"{name} B={B} T_y={Ty}: {e:.2e}; {big} of {ups} upsampler launches and {res_big} ResBlock c1 launches on the 128 x 128 tile")
        assert ups == hp.n_ups and big == n_big, f"{name}: {big} of {ups} upsampler launches took {BIG_TILE}, expected {n_big}"
    finally:
        model.close()


# ------------------------------------------------------------------------------------------------ ragged batches, fast path
RAGGED_ROWS = ("mb_u5_u2", "mb_2x8_3x9", "ms_u7_2x8", "ms_3stage_s2", "is_u7_3x9", "is_4x16_u7_perchain", "hg_cond_4x12_u3", "hg_cond_2x8_6x18")


def _voice_batch(model, hp, lens, rng):
    """a ragged batch with one frame per token (T_x = T_y): ids, lengths, sid, durations, injected noise and the library's own z"""
    B, T = len(lens), int(max(lens))
    lengths = np.asarray(lens, np.int64)
    ids = rng.integers(1, hp.n_vocab, size=(B, T)).astype(np.int64)
    sid = rng.integers(0, hp.n_speakers, size=B).astype(np.int64)
    dur = np.ones((B, T), np.int32)
    noise = rng.standard_normal((B, hp.inter_channels, T)).astype(np.float32)
    scales = np.array([0.667, 1.0, 0.8], np.float32)
    _, m_p, logs_p = model.text_encoder(ids, lengths, sid)
    d, ylen, z_p = model.regulate(None, dur, lengths, 1.0, m_p, logs_p, noise, float(scales[0]), T)
    assert np.array_equal(ylen, lengths)
    z = model.flow(z_p, ylen, sid)
    mask = (np.arange(T)[None, :] < lengths[:, None])[:, None, :]
    return ids, lengths, sid, dur, noise, scales, z * mask


@pytest.mark.parametrize("name", RAGGED_ROWS)
def test_ragged_batch_on_a_poisoned_workspace(hip_lib, name):
    """leg 3: a tiny voice around the row's decoder; items whose lengths differ from the longest by less and by more than the measured
    reach; a fresh model on NaN-filled workspaces.  Every valid sample equals the float64 decode of the DENSE padded z * y_mask of the
    same batch (z from the library's own flow stage), everything is finite, and beyond the tail's limit the output is defined zeros."""
    left, right = measured_field(name)
    rng = np.random.default_rng(55)
    hip_lib.lib.vits_debug_poison_workspace(1)
    try:
        hp, tens, model = _create(hip_lib, name, voice=True)
        needs = hip_lib.decoder_needs(hp)
        try:
            L = right + 40
            lens = [L, L - max(right - 2, 1), L - (right + 3), 2]
            ids, lengths, sid, dur, noise, scales, zm = _voice_batch(model, hp, lens, rng)
            audio, olen = model.synthesize(ids, lengths, scales, sid, noise_prior=noise, forced_durations=dur)
            assert np.array_equal(olen, lengths * hp.hop_length) and np.isfinite(audio).all()
            ref, _ = decoder_ref(hp, tens, zm, sid=sid)
            _not_vacuous(name, ref)
            worst = 0.0
            for b in range(len(lens)):
                n = int(olen[b])
                worst = max(worst, assert_close(f"{name} ragged item {b} (len {lens[b]}, reach {right})", ref[b, :n], audio[b, :n], STAGE_TOL))
                per_col = hp.hop_length // hp.total_upsample()  # samples per column of the last conv
                end = (lens[b] * hp.total_upsample() + needs["tail_cols"] + 1) * per_col
                assert np.all(audio[b, end:] == 0.0), f"{name} item {b}: samples beyond the tail's limit are not zero"
            print(f"{name} ragged, reach {right}, lens {lens}: {worst:.2e}")
        finally:
            model.close()
    finally:
        hip_lib.lib.vits_debug_poison_workspace(0)


@pytest.mark.parametrize("name", ("mb_2x8_3x9", "is_u7_3x9", "hg_cond_4x12_u3"))
def test_fast_path_equals_eager_path(hip_lib, name):
    """graph replay over bucketed shapes against the exact-size eager path (test_fast_path_equals_eager_path_over_shapes' bound).  Like
    that test it compares the two settings of vits_debug_fast_path; the library has no query for whether a call was served by a graph."""
    hp, tens, model = _create(hip_lib, name, voice=True)
    rng = np.random.default_rng(9)
    try:
        for B, Tx in ((1, 9), (3, 21)):
            lengths = rng.integers(max(1, Tx // 2), Tx + 1, size=B).astype(np.int64)
            lengths[0] = Tx
            ids = rng.integers(1, hp.n_vocab, size=(B, Tx)).astype(np.int64)
            sid = rng.integers(0, hp.n_speakers, size=B).astype(np.int64)
            dur = rng.integers(0, 4, size=(B, Tx)).astype(np.int32)
            out = []
            try:
                for on in (1, 0):
                    hip_lib.lib.vits_debug_fast_path(on)
                    out.append(model.synthesize(ids, lengths, [0.667, 1.0, 0.8], sid, forced_durations=dur, seed=5))
            finally:
                hip_lib.lib.vits_debug_fast_path(1)
            (a_f, l_f), (a_e, l_e) = out
            assert np.array_equal(l_f, l_e) and a_f.shape == a_e.shape
            m = np.arange(a_e.shape[1])[None, :] < l_e[:, None]
            assert_close(f"{name} fast vs eager B={B} Tx={Tx}", a_e * m, a_f * m, 2e-5)
    finally:
        model.close()


# ------------------------------------------------------------------------------------------------ streaming
STREAM_ROWS = ("mb_u1_3stage_d4", "ms_4stage", "mb_2x8_3x9", "is_3stage_d4", "ms_4x12_u1_s8", "is_u1_4x12_n64h4")


@pytest.mark.parametrize("name", STREAM_ROWS)
def test_streaming_chunks_below_and_above_the_reach(hip_lib, name):
    """leg 4, the rows with the widest fields (4 dilations, rates 1-2; reach 33-94 frames, beyond the 32-frame default halo): latent
    streaming in chunks smaller and larger than the reach equals the one-shot decode, which equals float64"""
    left, right = measured_field(name)
    assert max(left, right) > 32
    hp, tens, model = _create(hip_lib, name)
    try:
        Ty = 2 * max(left, right) + 37
        z = np.random.default_rng(3).standard_normal((1, hp.inter_channels, Ty)).astype(np.float32)
        one, _ = model.decoder(z, want_mb=False)
        ref, _ = decoder_ref(hp, tens, z)
        _not_vacuous(name, ref)
        assert_close(f"{name} one-shot", ref, one, STAGE_TOL)
        for chunk in (max(min(left, right) // 3, 2), max(left, right) + 5):
            got = np.concatenate(list(model.stream_latent(z[0], chunk_frames=chunk)))[None]
            assert got.shape == one.shape
            e = assert_close(f"{name} stream chunk {chunk} (reach {left}/{right}) vs one-shot", one, got, STREAM_TOL)
            print(f"{name} stream chunk {chunk}, reach {left}/{right}: {e:.2e}")
    finally:
        model.close()


# ------------------------------------------------------------------------------------------------ split-bf16 ResBlock convs
# (row, B, T_y, polyphase launches that must take the split-bf16 kernel).  The kernel is taken by tile count as well as by channels
# (engine_convplan.hip.h: 512 tiles of 128 x 128, or 256 of 64 x 128 for other multiples of 64 rows), and a polyphase launch only when
# C_out % 128 == 0 and its input is one tensor (stage 0, or a later stage of a one-chain decoder), so sizes follow the rows:
# rates 4, 6, 5, 7, 8, 2 at the first stage; is_3stage_d4's (2,2) first stage is too small at this size (ResBlocks only).
BF3_ROWS = (("mb_default", 16, 400, 1), ("ms_u6_u5", 16, 400, 1), ("is_u5_u6", 16, 400, 1), ("ms_u7_2x8", 24, 400, 1), ("hg_v1", 8, 120, 1),
            ("mb_2x8_3x9", 16, 400, 1), ("is_3stage_d4", 8, 120, 0))


@pytest.mark.parametrize("name,B,Ty,n_ups_bf3", BF3_ROWS, ids=[r[0] for r in BF3_ROWS])
def test_split_bf16_convs(hip_lib, name, B, Ty, n_ups_bf3):
    """leg 5: conv_precision = 1 where the stage channels (C % 64 == 0) make the split-bf16 kernel eligible, at batch size; the launch
    log says which launches took it (ResBlock convs on every row, the polyphase upsampler where listed)"""
    hp, tens, model = _create(hip_lib, name, conv_precision=1)
    try:
        z = np.random.default_rng(31).standard_normal((B, hp.inter_channels, Ty)).astype(np.float32)
        hip_lib.launch_log(1)
        try:
            a_bf, _ = model.decoder(z, want_mb=False)
        finally:
            hip_lib.launch_log(0)
        ups_bf3 = hip_lib.launch_count("dec.ups", "conv_bf3_kernel")
        res_bf3 = hip_lib.launch_count("dec.res_c1", "conv_bf3_kernel") + hip_lib.launch_count("dec.res_c2", "conv_bf3_kernel")
        try:
            hip_lib.lib.vits_debug_no_bf16x3(1)
            a_fp, _ = model.decoder(z, want_mb=False)
        finally:
            hip_lib.lib.vits_debug_no_bf16x3(0)
        assert not np.array_equal(a_bf, a_fp), "the split-bf16 variant did not run"
        e = assert_close(f"{name}: bf16x3 vs fp32 kernels", a_fp, a_bf, BF3_TOL)
        ref, _ = decoder_ref(hp, tens, z[:2])
        e2 = assert_close(f"{name}: bf16x3 vs float64", ref, a_bf[:2], BF3_TOL)
        print(f"{name} bf16x3: vs fp32 {e:.2e}, vs float64 {e2:.2e}; split-bf16 launches: {ups_bf3} polyphase, {res_bf3} ResBlock")
        assert res_bf3 > 0 and ups_bf3 == n_ups_bf3, f"{name}: {ups_bf3} polyphase launches took conv_bf3_kernel, expected {n_ups_bf3}"
    finally:
        model.close()


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("entry", REFUSED, ids=row_id)
def test_loader_refuses(hip_lib, entry):
    """a refusal is a correct answer: the error code and a message that names the offending value"""
    import re

    from vosk_tts_amd import weights as W
    from vosk_tts_amd.capi import VitsError

    codes = {"BLOB": 2, "UNSUPPORTED": 4}  # VITS_ERR_BLOB / VITS_ERR_UNSUPPORTED (include/vits_mi355.h)
    hp = refused_hparams(entry)
    blob = W.pack_blob(hp, W.make_synthetic_weights(hp, 1234), validate=False)
    with pytest.raises(VitsError) as ei:
        hip_lib.create(blob, 0)
    assert ei.value.code == codes[entry[3]], str(ei.value)
    assert re.search(entry[4], str(ei.value)), str(ei.value)
    assert {"code": ei.value.code, "message": str(ei.value)} == RECORDED["refusals"][entry[0]]
