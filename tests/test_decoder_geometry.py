"""The float64 restatement of the four decoders (tests/decoder_ref.py) pinned on the CPU, and the geometry grid (tests/decoder_grid.py)
checked for what it claims: no GPU here.

  * restatement == the reference modules' own outputs: the committed fixtures at the geometries that existed (full_c1, full_b2,
    tiny_b3, plain_b2, hifigan_v1, ms_dec_b2, istft_dec_b2, consts) and the new per-row fixtures tests/golden/geom_<row>.npz
    (tools/gen_golden_decoder_geometry.py; 3-4 rows of each dec_type);
  * restatement == the C oracle at every dec_type 0 / 1 row of the grid (the oracle is general over geometry for those two);
  * the restatement's measured one-sided reach (perturb one frame of z, see how far the waveform moves) against the engine's
    host arithmetic: decoder_needs has to read at least that many frames of z beyond an item's end, and the ragged / streaming
    halo (vits_debug_rag_halo) has to cover both sides;
  * mutations of the REFERENCE side (one phase's taps shifted, mean / 3 whatever n_resk is, dilations reversed, reflection column
    dropped, PQMF pad off by one) are each caught by the oracle comparison at the tolerance used.

Tolerance: 2e-5 on the assert_close scale (max abs error over max abs reference), the figure the project pins its oracle to the
fixtures with.  No row needed more: worst restatement-vs-fixture 1.15e-6 (hifigan_v1; 1.02e-6 among the new ones, geom_hg_v1),
worst restatement-vs-oracle 1.46e-6 (hg_5x15_8x24); every mutation shows up at 0.27 or more.  Figures are printed (-s).

Rows the reference cannot construct (n_resd != 3: ResBlock1 has exactly three dilations; PQMF other than 4 bands / 62 taps; a
multi-stream filter other than 63 taps) have no fixture: for dec_type 0 / 1 they rest on the restatement and the oracle agreeing,
for dec_type 2 / 3 with n_resd != 3 or other taps on the restatement alone (the same code paths the fixtures pin at n_resd = 3).
"""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, assert_close, golden
from decoder_grid import (AXES, GRID, N_GRID, N_REFUSED, REFUSED, axis_values, chains, measured_field, refused_hparams, row_hparams, row_id,
                          row_weights)
from decoder_ref import MUTATIONS, decoder_ref, istft_inverse_basis, pqmf_synthesis_filter

TOL = 2e-5
ROWS = {r[0]: r for r in GRID}
FIXTURE_ROWS = sorted(f[5:-4] for f in os.listdir(GOLDEN) if f.startswith("geom_") and f.endswith(".npz"))


# ------------------------------------------------------------------------------------------------ the table itself
def test_grid_counts_and_axes():
    assert len(GRID) == N_GRID == 43 and len(REFUSED) == N_REFUSED == 9
    assert len({r[0] for r in GRID}) == len(GRID) and len({r[0] for r in REFUSED}) == len(REFUSED)
    seen = {a: {} for a in AXES}
    for row in GRID:
        for axis, vals in axis_values(row).items():
            for v in vals:
                seen[axis].setdefault(v, []).append(row)
    for axis, values in AXES.items():
        for v in values:
            rows = seen[axis].get(v, [])
            assert len(rows) >= 2, f"{axis} value {v} occurs in {len(rows)} rows"
            # ... with different partners: the rows that carry it are not all the same in every other axis
            others = {tuple(sorted((a, tuple(sorted(map(str, s)))) for a, s in axis_values(r).items() if a != axis)) for r in rows}
            assert len(others) >= 2, f"{axis} value {v} always has the same partners"
        assert set(seen[axis]) >= set(values)
    assert {r[1] for r in GRID} == {0, 1, 2, 3}
    assert {len(chains(r)[0]) for r in GRID} == {1, 2, 3, 4} and {len(r[3]) for r in GRID} == {1, 2, 3}
    assert any(len(set(chains(r))) > 1 for r in GRID)  # per-chain lists that differ


@pytest.mark.parametrize("row", GRID, ids=row_id)
def test_rows_validate_and_tensor_specs_follow_the_geometry(row):
    """every row passes validate_hparams with hop_length the product of its rates, and tensor_specs enumerates exactly the tensors the
    geometry implies (n_ups upsamplers, n_ups * n_resk ResBlocks of n_resd conv pairs, the kernels and channel counts of the row)"""
    from vosk_tts_amd import weights as W

    name, dt, ups, rk, _, tail, C0, I, voice = row
    hp = row_hparams(row)
    W.validate_hparams(hp)
    rate = int(np.prod([u for u, _ in ups]))
    if dt in (0, 2):
        rate *= tail[0] * tail[2]
    elif dt == 3:
        rate *= tail[1]
    assert hp.hop_length == rate and hp.total_upsample() * (hp.hop_length // hp.total_upsample()) == rate
    specs = {n: s for n, s, *_ in W.tensor_specs(hp) if n.startswith("dec.")}
    want = {"dec.conv_pre.weight": (C0, I, 7), "dec.conv_pre.bias": (C0,)}
    ch, nd = C0, len(chains(row)[0])
    for i, (u, Ku) in enumerate(ups):
        want[f"dec.ups.{i}.weight"] = (ch, ch // 2, Ku)
        want[f"dec.ups.{i}.bias"] = (ch // 2,)
        ch //= 2
        for j, k in enumerate(rk):
            for d in range(nd):
                for c in ("convs1", "convs2"):
                    want[f"dec.resblocks.{i * len(rk) + j}.{c}.{d}.weight"] = (ch, ch, k)
                    want[f"dec.resblocks.{i * len(rk) + j}.{c}.{d}.bias"] = (ch,)
    if dt in (0, 2):
        S, N, _, taps = tail
        want["dec.subband_conv_post.weight"] = (S * (N + 2), ch, 7)
        if dt == 2:
            want["dec.subband_conv_post.bias"] = (S * (N + 2),)
            want["dec.multistream_conv_post.weight"] = (1, S, taps + 1)
    elif dt == 3:
        want["dec.conv_post.weight"] = (tail[0] + 2, ch, 7)
    else:
        want["dec.conv_post.weight"] = (1, ch, 7)
        if voice:
            want["dec.cond.weight"], want["dec.cond.bias"] = (C0, hp.gin_channels, 1), (C0,)
        else:
            want["dec.conv_post.bias"] = (1,)
    assert specs == want
    hp2, tens = W.unpack_blob(W.synthetic_blob(hp, 3))
    assert bytes(hp2) == bytes(hp) and {n: t.shape for n, t in tens.items() if n.startswith("dec.")} == want


@pytest.mark.parametrize("entry", REFUSED, ids=row_id)
def test_validate_hparams_refuses_what_the_loader_refuses(entry):
    from vosk_tts_amd import weights as W

    hp = refused_hparams(entry)
    with pytest.raises(ValueError, match=entry[4]):
        W.validate_hparams(hp)
    with pytest.raises(ValueError, match=entry[4]):
        W.pack_blob(hp, W.make_synthetic_weights(hp, 1))
    assert W.unpack_blob(W.pack_blob(hp, W.make_synthetic_weights(hp, 1), validate=False))[0].hop_length == hp.hop_length


# ------------------------------------------------------------------------------------------------ restatement vs reference modules
def _check(name, hp, tens, z, audio, mb=None, sid=None):
    a, m = decoder_ref(hp, tens, z, sid=sid)
    e = assert_close(f"{name}: audio", a, audio, TOL)  # (the float64 side is the `ref` of assert_close's scale)
    e2 = 0.0
    if mb is not None:
        e2 = assert_close(f"{name}: audio_mb", m, mb, TOL)
    print(f"restatement vs fixture {name}: audio {e:.2e} audio_mb {e2:.2e}")
    return max(e, e2)


@pytest.mark.parametrize("fixture,which", [("full_c1", "default"), ("full_b2", "default"), ("tiny_b3", "tiny")])
def test_restatement_equals_the_multiband_fixtures(fixture, which):
    from vosk_tts_amd import weights as W

    hp = W.default_hparams() if which == "default" else W.tiny_hparams()
    g = golden(fixture)
    Ty = g["z"].shape[2]
    mask = (np.arange(Ty)[None, :] < g["y_lengths"][:, None])[:, None, :]
    _check(fixture, hp, W.make_synthetic_weights(hp, 1234), g["z"] * mask, g["audio"], g["audio_mb"])


def test_restatement_equals_the_other_decoder_fixtures():
    from vosk_tts_amd import weights as W

    g = golden("plain_b2")
    hp = W.plain_hparams()
    _check("plain_b2", hp, W.make_synthetic_weights(hp, 1234), g["z"], g["audio"], sid=g["sid"])
    g = golden("hifigan_v1")
    hp = W.hifigan_v1_vocoder_hparams()
    _check("hifigan_v1", hp, W.make_synthetic_weights(hp, 1234), g["mel"], g["audio"])
    g = golden("ms_dec_b2")
    hp = W.tiny_multistream_hparams()
    S = hp.subbands
    _check("ms_dec_b2", hp, W.make_synthetic_weights(hp, 1234), g["z"], g["audio"], g["y_mb_hat"][:, :, ::S] / S)
    g = golden("istft_dec_b2")
    hp = W.tiny_istft_hparams()
    _check("istft_dec_b2", hp, W.make_synthetic_weights(hp, 1234), g["z"], g["audio"])


def test_restatement_constants_equal_the_reference_buffers():
    g = golden("consts")
    assert_close("inverse basis", istft_inverse_basis(16, 4), g["istft_inverse_basis"], 1e-6)
    assert_close("PQMF synthesis filter", pqmf_synthesis_filter(4, 62, 0.15, 9.0), g["pqmf_synthesis_filter"], 1e-6)
    with pytest.raises(ValueError, match="even"):
        pqmf_synthesis_filter(4, 61, 0.15, 9.0)  # (an odd `taps` is not defined by the reference's design: no such grid row)


def test_fixture_rows_cover_every_decoder_type():
    assert len(FIXTURE_ROWS) == 13 and set(FIXTURE_ROWS) <= set(ROWS)
    per_type = {dt: sum(1 for n in FIXTURE_ROWS if ROWS[n][1] == dt) for dt in range(4)}
    assert min(per_type.values()) >= 3, per_type
    for n in FIXTURE_ROWS:
        assert os.path.getsize(os.path.join(GOLDEN, f"geom_{n}.npz")) < 48 * 1024


@pytest.mark.parametrize("name", FIXTURE_ROWS)
def test_restatement_equals_the_reference_modules_at_grid_rows(name):
    g = golden("geom_" + name)
    hp, tens = row_weights(name)
    _check(name, hp, tens, g["z"], g["audio"], g.get("audio_mb"), sid=g.get("sid"))


# ------------------------------------------------------------------------------------------------ restatement vs the C oracle
ORACLE_ROWS = [r for r in GRID if r[1] in (0, 1)]


def _oracle_vs_ref(oracle_lib, name, Ty=9, mutate=None, seed=21):
    from vosk_tts_amd import weights as W

    hp, tens = row_weights(name)
    model = oracle_lib.create(W.pack_blob(hp, tens))
    try:
        rng = np.random.default_rng(seed)
        z = rng.standard_normal((2, hp.inter_channels, Ty)).astype(np.float32)
        sid = np.array([1, 3], np.int64) if ROWS[name][8] else None
        got, got_mb = model.decoder(z, sid=sid)
        a, mb = decoder_ref(hp, tens, z, sid=sid, mutate=mutate)
        assert np.abs(a).max() > 1e-3 and np.ptp(a) > 1e-3
        e = assert_close(f"{name}: audio (oracle vs float64)", a, got, TOL)
        if mb is not None:
            e = max(e, assert_close(f"{name}: audio_mb (oracle vs float64)", mb, got_mb, TOL))
        return e
    finally:
        model.close()


@pytest.mark.parametrize("row", ORACLE_ROWS, ids=row_id)
def test_restatement_equals_the_oracle_at_every_type_0_and_1_row(oracle_lib, row):
    assert len(ORACLE_ROWS) == 20
    e = _oracle_vs_ref(oracle_lib, row[0])
    print(f"restatement vs oracle {row[0]}: {e:.2e}")


MUTATION_ROWS = ("mb_u3_nooverlap", "mb_u6_u4_s2", "hg_u6_d4", "hg_4x16", "hg_u5_u4")


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_mutations_are_detected(oracle_lib, mutation):
    """the grid is sensitive: each deliberately wrong restatement fails the oracle comparison on at least one (small) grid row, at the
    tolerance every row is held to.  (The unmutated restatement passes on these rows: the test above.)"""
    caught = []
    for name in MUTATION_ROWS:
        try:
            _oracle_vs_ref(oracle_lib, name, mutate=mutation)
        except AssertionError as e:
            m = re.search(r"rel ([0-9.e+-]+) >", str(e))
            if m is None:  # not assert_close's comparison (e.g. the vacuity guard): that is not a detection
                raise
            caught.append((name, float(m.group(1))))
    print(f"mutation {mutation}: caught at {caught}")
    assert caught, f"mutation {mutation} passes on every row of {MUTATION_ROWS}"


# ------------------------------------------------------------------------------------------------ reach
@pytest.mark.parametrize("row", GRID, ids=row_id)
def test_ragged_limit_covers_the_measured_reach(row):
    """An item's valid samples depend on z up to `right` frames beyond its end (measured on the restatement, exact: a sample either
    changes or it does not).  The engine's ragged batches read decoder_needs()['z_frames'] frames of the padded continuation: fewer than
    the reach would make a valid sample wrong.  (Host arithmetic only; the per-layer limits themselves are proven on the GPU by the
    ragged, poisoned-workspace leg of tests/test_decoder_geometry_gpu.py.)"""
    from vosk_tts_amd.capi import VitsLib

    left, right = measured_field(row[0])
    needs = VitsLib().decoder_needs(row_hparams(row))
    print(f"{row[0]}: reach left {left} right {right} frames, decoder_needs z_frames {needs['z_frames']}")
    assert 3 <= left <= 200 and 3 <= right <= 200
    assert needs["z_frames"] >= right
    # the halo of streaming windows and of the uniform ragged form (load_decoder's own formula, a separate one) covers both sides
    halo = VitsLib().rag_halo(row_hparams(row))
    print(f"{row[0]}: rag_halo {halo}")
    assert halo >= max(left, right)


# ------------------------------------------------------------------------------------------------ the recorded host arithmetic
def _recorded():
    import json

    from vosk_tts_amd import weights as W

    doc = json.load(open(os.path.join(GOLDEN, "decoder_geom.json")))
    hps = {r[0]: row_hparams(r) for r in GRID}
    hps.update(default=W.default_hparams(), multistream=W.multistream_hparams(), istft=W.istft_hparams(), plain=W.plain_hparams())
    return doc, hps, {e[0]: refused_hparams(e) for e in REFUSED}


def _hooks(lib, hp):
    from vosk_tts_amd.capi import VitsError

    out = {}
    for key, fn in (("rag_halo", lib.rag_halo), ("needs", lib.decoder_needs)):
        try:
            out[key] = fn(hp)
        except VitsError as e:
            out[key] = {"error": e.code}
    return out


def test_host_arithmetic_equals_the_recording():
    """rag_halo and the whole decoder_needs vector of all 43 grid rows, the default / multistream / single-band / plain-Generator
    hparams and the nine refused geometries equal tests/golden/decoder_geom.json, recorded (tools/gen_golden_decoder_geom.py) from
    the library as it stood before the decoder's shape moved into DecGeom.  Equality, no tolerance: these are integers."""
    from vosk_tts_amd.capi import VitsLib

    doc, hps, refused = _recorded()
    lib = VitsLib()
    assert sorted(doc["rows"]) == sorted(hps) and len(hps) == N_GRID + 4
    assert sorted(doc["refused"]) == sorted(refused) and len(refused) == N_REFUSED
    for name, hp in hps.items():
        assert _hooks(lib, hp) == doc["rows"][name], name
    for name, hp in refused.items():
        assert _hooks(lib, hp) == doc["refused"][name], name
