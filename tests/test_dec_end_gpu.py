"""The end of the single utterance's decoder: column-pair workgroups in the chunk split of the 16-wave K-split conv kernel
(ks_chunk_body NT = 2, csrc/conv_mfma.hip.h; who takes them: ks_pair_takes, csrc/engine_launch.hip.h; switch: VITS_KS_PAIR=0|1|2, read
once per process, 2 = wherever the chunk split runs on two or more column tiles) and the fused decoder tail at compile-time geometry
(tail_body, csrc/kernels_misc.hip.h; who takes it: tail_fixed_geometry, csrc/engine_stages.hip.h; switch: VITS_TAIL_GENERIC=0|1).

Pairs, in two child processes, VITS_KS_PAIR=0 and 2:
  * single convs through vits_op_conv1d on the K-split kernel with 16 waves (force_tile 2, ks_waves 16) against the float64 conv_ref of
    tests/test_ks_chunk_gpu.py at its CONV_TOL: C_in 128 / 512 (half-chunk and whole-chunk units), C_out 32 / 64, 4 and 7 taps, T 33 (a
    pair whose second tile holds one column), 63, 64 (a full pair), 65 (a lone last tile behind a pair), 97 and 129 (even and odd tile
    counts), and T 1 and 3 (rows shorter than a vector load: the tap split).  The pair form is built for 4 taps -- the polyphase
    upsamplers, the shape the rule exists for; with 7 taps two accumulators beside a seven-slot weight ring do not fit the 128 registers
    of a 16-wave workgroup, so those cases run single tiles under either setting;
  * the decoder rows mb_default, ms_4stage, hg_v1 and hg_cond_4x12_u3 at T_y 2 / 5 / 17 / 33 with every conv forced onto the 16-wave
    K-split kernel, against tests/decoder_ref.py at STAGE_TOL.  What of the staging this puts into the PAIR body is what these rows'
    4-tap upsamplers read -- ups[0] of mb_default (4, 16) and of ms_4stage (2, 8): one input; ups[1] of mb_default: the three-input
    mean with its scale; hg_v1 and hg_cond_4x12_u3 have no 4-tap launch and run single tiles throughout -- with edge tiles on both
    sides, odd and even tile counts and a lone last tile.  The reflection column and cond(g) belong to conv_post and
    conv_pre, which have 7 taps and therefore run single tiles here; an absent x3 does not occur in these rows' upsamplers (three
    chains each).  Those three cases are covered for the single-tile chunk split by tests/test_ks_chunk_gpu.py and are NOT covered
    for pairs: the pair body shares the staging code (stage() of ks_chunk_body, one template), but no test drives it there;
  * a length limit inside a tile, and whole tiles beyond it: one utterance of the default voice on the fast path (padded to its
    bucket), against the CPU oracle at E2E_TOL of tests/test_hip_parity.py;
  * the two children are bit-identical everywhere: the pair form keeps each accumulator's sequence of MFMAs and the order of the
    cross-wave sum.  Identity is the design, so no difference can show that pairs ran: the fixture first evaluates the rule the
    engine calls (csrc/dec_end_rules.h, through the host program of tests/test_dec_end_rules.py) under each child's environment and
    asserts that it takes these shapes under 2 and none under 0.
  The grid of a launch is not visible from Python (the launch log records names, and the ABI test pins the debug hooks): that the
  default rule gives ups[1] of the c2 shape 160 workgroups and leaves conv_pre, ups[0] and conv_post alone is asserted on the host
  function in tests/test_dec_end_rules.py (and seen in the kernel trace of profiles/dec_end_bench.txt).

The tail:

  * every row of tests/decoder_grid.py with an iSTFT tail (dec_type 0 / 2 / 3) at T_y 1 / 2 / 5 / 33: the fused tail (tail_impl 0)
    against the separately written istft_kernel (+ pqmf_synthesis_kernel) (tail_impl 1).  The rows with the geometry (4, 16, 4, 62) --
    mb_default, mb_4stage, ms_4stage -- and the single-band N 16 / hop 4 -- is_default, is_u5_u6 -- run the compile-time body, whose
    multi-band blocks own 32 sub-band samples (mb_4stage has 48 per frame: a short last block at odd T_y; the others 64: 2 to 66
    blocks; is_u5_u6 has 120 output samples per frame: one short 256-sample block at T_y 1 / 2, a short last one at 5 and 33); every
    other row runs the run-time body on 64; T_y 5 and 33 run as a batch of two;
  * mb_default and is_default in two child processes, VITS_TAIL_GENERIC=0 and 1, at the same T_y and at 70 (140 and 70 blocks): audio
    and sub-band signal bit-identical -- both bodies keep every element's sequence of operations;
  * a ragged batch of two items (5 and 3 frames) on a NaN-filled fresh workspace through synthesize(solo=True): every valid sample is the
    item's own single-utterance call's, every sample beyond an item's end is zero.

Tolerances.  Fused against separate: 1e-5 on the assert_close scale (max abs error over max abs reference), the bound
tests/test_istft_decoders_gpu.py holds the same pair to (the fused form re-uses the rounded products mag cos / mag sin of a frame
in every overlapping sample; the separate kernel recomputes them -- identical values, other contraction of the sum).  Solo batch
against the single calls: 2e-5, the bound of tests/test_hip_parity.py for the same comparison (the convs' kernel choice differs with
the batch size, so not bit for bit); the tail itself is checked for identity by the child processes.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_close

HERE = os.path.dirname(os.path.abspath(__file__))
TAIL_TOL = 1e-5
SOLO_TOL = 2e-5
TYS = (1, 2, 5, 33)
CHILD_ROWS = ("mb_default", "is_default")
CHILD_TYS = TYS + (70,)
FIXED_ROWS = {"mb_default", "mb_4stage", "ms_4stage", "is_default", "is_u5_u6"}


def tail_rows():
    from decoder_grid import GRID

    return [r[0] for r in GRID if r[1] in (0, 2, 3)]


def fixed_geometry(row):
    """the rule of tail_fixed_geometry, restated on a grid row"""
    dt, tail = row[1], row[5]
    return tail == (4, 16, 4, 62) if dt in (0, 2) else tail == (16, 4)


def row_z(name, Ty, B=1):
    from decoder_grid import row_weights

    hp, _ = row_weights(name)
    return np.random.default_rng([tail_rows().index(name), Ty]).standard_normal((B, hp.inter_channels, Ty)).astype(np.float32)


def test_the_rows_that_take_the_compile_time_body():
    from decoder_grid import GRID

    assert {r[0] for r in GRID if r[1] in (0, 2, 3) and fixed_geometry(r)} == FIXED_ROWS


@pytest.mark.gpu
@pytest.mark.parametrize("name", tail_rows())
def test_fused_tail_equals_separate_kernels(hip_lib, name):
    from decoder_grid import row_weights
    from vosk_tts_amd import weights as W

    hp, tens = row_weights(name)
    model = hip_lib.create(W.pack_blob(hp, tens), 0)
    try:
        for Ty in TYS:
            z = row_z(name, Ty, B=1 + Ty % 2 if Ty > 1 else 1)
            out = {}
            try:
                for impl in (1, 0):
                    hip_lib.lib.vits_debug_tail_impl(impl)
                    out[impl] = model.decoder(z)
            finally:
                hip_lib.lib.vits_debug_tail_impl(0)
            assert np.isfinite(out[0][0]).all()
            e = assert_close(f"{name} T_y={Ty}: audio, fused vs separate", out[1][0], out[0][0], TAIL_TOL)
            if out[1][1] is not None:
                e = max(e, assert_close(f"{name} T_y={Ty}: audio_mb, fused vs separate", out[1][1], out[0][1], TAIL_TOL))
            print(f"{name} T_y={Ty}: {e:.2e}")
    finally:
        model.close()


# ------------------------------------------------------------------------------------------------ pairs: two child processes
PAIR_CONVS = [(Cin, Cout, K, T, 0.1) for Cin in (128, 512) for Cout in (32, 64) for K in (4, 7) for T in (1, 3, 33, 63, 64, 65, 97, 129)]
PAIR_DEC_ROWS = ("mb_default", "ms_4stage", "hg_v1", "hg_cond_4x12_u3")
PAIR_DEC = [(name, Ty) for name in PAIR_DEC_ROWS for Ty in (2, 5, 17, 33)]


def pair_child_main(out_path):
    import conftest  # noqa: F401  (torch before the library, as the suite)
    from test_ks_chunk_gpu import KS16, conv_case, dec_case, hooks
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.capi import VitsLib, op_conv1d

    lib = VitsLib()
    out = {}
    with hooks(lib, KS16):
        for i, c in enumerate(PAIR_CONVS):
            x, w, bias = conv_case(*c)
            out[f"conv{i}"] = op_conv1d(lib, x, w, bias, 1, c[4])
    for name in PAIR_DEC_ROWS:
        hp, tens, _, _ = dec_case(name, 1)
        model = lib.create(W.pack_blob(hp, tens), 0)
        for n2, Ty in PAIR_DEC:
            if n2 == name:
                _, _, z, sid = dec_case(name, Ty)
                with hooks(lib, KS16):
                    out[f"dec_{name}_{Ty}"] = model.decoder(z, sid=sid, want_mb=False)[0]
        model.close()
    # a single utterance on the fast path is padded to its bucket: ups[0] and ups[1] (default dispatch: the 16-wave chunk split) carry a
    # length limit inside a column tile, and whole tiles beyond it
    default = lib.create(W.synthetic_blob(W.default_hparams(), 1234), 0)
    ids, dur = bucketed_case()
    out["bucketed"], out["bucketed_len"] = default.synthesize(ids, [ids.shape[1]], [0.667, 1.0, 0.8], [2], forced_durations=dur, seed=5)
    default.close()
    np.savez(out_path, **out)


def bucketed_case():
    rng = np.random.default_rng(77)
    return rng.integers(1, 62, size=(1, 21)).astype(np.int64), rng.integers(1, 4, size=(1, 21)).astype(np.int32)


def run_children(tmp_path_factory, var, mode):
    """{setting: npz of the child's outputs}: both children run at the same time"""
    d = tmp_path_factory.mktemp("dec_end_" + mode)
    procs = {}
    for v in (("0", "2") if mode == "pair" else ("0", "1")):
        env = dict(os.environ, **{var: v})
        procs[v] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", mode, str(d / f"out{v}.npz")], env=env, cwd=HERE,
                                    stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    res = {}
    for v, p in procs.items():
        log, _ = p.communicate()
        assert p.returncode == 0, f"child {var}={v} ended with {p.returncode}:\n{log[-2000:]}"
        res[v] = dict(np.load(d / f"out{v}.npz"))
    return res


@pytest.fixture(scope="module")
def rules_exe(tmp_path_factory):
    from test_dec_end_rules import build_rules_program

    return build_rules_program(tmp_path_factory.mktemp("dec_end_rules"))


@pytest.fixture(scope="module")
def pair_children(tmp_path_factory, rules_exe):
    """the children's outputs; first, the rule the engine calls (csrc/dec_end_rules.h) evaluated under each child's environment: with
    VITS_KS_PAIR=2 it takes these shapes' 4-tap launches and with 0 none, so identical outputs are not the same code run twice"""
    from test_dec_end_rules import run_rules_program

    on, off = (run_rules_program(rules_exe, VITS_KS_PAIR=v) for v in ("2", "0"))
    assert on["mode"] == 2 and off["mode"] == 0
    assert on["launches"]["conv_t64"][1] == 1 and on["launches"]["conv_t33_b2"][1] == 1 and on["launches"]["ups1"][1] == 1
    assert not any(v[1] for v in off["launches"].values())
    return run_children(tmp_path_factory, "VITS_KS_PAIR", "pair")


@pytest.mark.gpu
def test_pairs_single_convs_against_float64_and_bit_identical_to_single_tiles(pair_children):
    from test_ks_chunk_gpu import CONV_TOL, conv_case, conv_ref

    worst = 0.0
    for i, c in enumerate(PAIR_CONVS):
        x, w, bias = conv_case(*c)
        ref = conv_ref(x, w, bias, 1, c[4])
        for v in ("0", "2"):
            worst = max(worst, assert_close(f"VITS_KS_PAIR={v} conv {c}", ref, pair_children[v][f"conv{i}"], CONV_TOL))
        assert pair_children["0"][f"conv{i}"].tobytes() == pair_children["2"][f"conv{i}"].tobytes(), f"conv {c}: pairs differ from single tiles"
    print(f"single convs, single tiles and pairs: worst {worst:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("row", PAIR_DEC_ROWS)
def test_pairs_decoder_against_float64_and_bit_identical_to_single_tiles(pair_children, row):
    from decoder_ref import decoder_ref
    from test_decoder_geometry_gpu import STAGE_TOL
    from test_ks_chunk_gpu import dec_case

    for name, Ty in PAIR_DEC:
        if name != row:
            continue
        hp, tens, z, sid = dec_case(name, Ty)
        ref = decoder_ref(hp, tens, z, sid=sid)[0]
        for v in ("0", "2"):
            e = assert_close(f"VITS_KS_PAIR={v} decoder {name} T_y={Ty}", ref, pair_children[v][f"dec_{name}_{Ty}"], STAGE_TOL)
        assert pair_children["0"][f"dec_{name}_{Ty}"].tobytes() == pair_children["2"][f"dec_{name}_{Ty}"].tobytes(), \
            f"decoder {name} T_y={Ty}: pairs differ from single tiles"
        print(f"{name} T_y={Ty}: {e:.2e}")


@pytest.mark.gpu
def test_pairs_bucketed_single_utterance_length_limit_inside_a_tile(pair_children, oracle_default):
    from test_hip_parity import E2E_TOL

    ids, dur = bucketed_case()
    want, wl = oracle_default.synthesize(ids, [ids.shape[1]], [0.667, 1.0, 0.8], [2], forced_durations=dur, seed=5)
    n = int(wl[0])
    for v in ("0", "2"):
        assert np.array_equal(pair_children[v]["bucketed_len"], wl)
        assert_close(f"VITS_KS_PAIR={v} bucketed single utterance", want[0, :n], pair_children[v]["bucketed"][0, :n], E2E_TOL)
    assert pair_children["0"]["bucketed"].tobytes() == pair_children["2"]["bucketed"].tobytes(), "pairs differ from single tiles"


# ------------------------------------------------------------------------------------------------ the tail: two child processes
def child_main(out_path):
    import conftest  # noqa: F401  (torch before the library, as the suite)
    from decoder_grid import row_weights
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.capi import VitsLib

    lib = VitsLib()
    out = {}
    for name in CHILD_ROWS:
        hp, tens = row_weights(name)
        model = lib.create(W.pack_blob(hp, tens), 0)
        for Ty in CHILD_TYS:
            audio, mb = model.decoder(row_z(name, Ty))
            out[f"{name}_{Ty}_audio"] = audio
            if mb is not None:
                out[f"{name}_{Ty}_mb"] = mb
        model.close()
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def children(tmp_path_factory, rules_exe):
    """as pair_children: the host predicate takes both rows' geometries under VITS_TAIL_GENERIC=0 and neither under 1"""
    from test_dec_end_rules import run_rules_program

    on, off = (run_rules_program(rules_exe, VITS_TAIL_GENERIC=v) for v in ("0", "1"))
    assert on["tails"]["mb_4_16_4_62"] == 1 and on["tails"]["is_16_4"] == 1 and not any(off["tails"].values())
    return run_children(tmp_path_factory, "VITS_TAIL_GENERIC", "tail")


@pytest.mark.gpu
def test_compile_time_and_run_time_bodies_are_bit_identical(children):
    keys = sorted(children["0"])
    assert keys == sorted(children["1"]) and len(keys) == len(CHILD_TYS) * 3  # audio of both rows, audio_mb of the multi-band one
    for k in keys:
        a, b = children["0"][k], children["1"][k]
        assert np.isfinite(a).all() and np.abs(a).max() > 0, k
        assert a.tobytes() == b.tobytes(), f"{k}: largest difference {np.abs(a - b).max():.3e} of max {np.abs(b).max():.3e}"


# ------------------------------------------------------------------------------------------------ a ragged batch
@pytest.mark.gpu
def test_ragged_batch_of_5_and_3_frames_on_a_poisoned_workspace(hip_lib, default_blob):
    """default hparams: the (4, 16, 4, 62) tail.  Item 0 ends inside the tail's third 32-sample block, item 1 inside its second; the
    batch buffer is 5 frames long, so item 1's last 2 frames are padding the tail has to write as zeros"""
    ids = np.array([[5, 9, 0], [7, 3, 11]], np.int64)
    lengths = np.array([2, 3], np.int64)
    dur = np.array([[2, 3, 0], [1, 1, 1]], np.int32)
    sid = np.array([2, 5], np.int64)
    scales = [0.667, 1.0, 0.8]
    hip_lib.lib.vits_debug_poison_workspace(1)
    try:
        fresh = hip_lib.create(default_blob, 0)
        try:
            got, glen = fresh.synthesize(ids, lengths, scales, sid, forced_durations=dur, seed=9, solo=True)
        finally:
            fresh.close()
    finally:
        hip_lib.lib.vits_debug_poison_workspace(0)
    assert glen.tolist() == [5 * 256, 3 * 256] and got.shape == (2, 5 * 256)
    assert np.isfinite(got).all()
    model = hip_lib.create(default_blob, 0)
    try:
        for b in range(2):
            L, n = int(lengths[b]), int(glen[b])
            one, ol = model.synthesize(ids[b:b + 1, :L], [L], scales, sid[b:b + 1], forced_durations=dur[b:b + 1, :L], seed=9 + b)
            assert int(ol[0]) == n
            assert_close(f"item {b}: valid samples against its solo run", one[0, :n], got[b, :n], SOLO_TOL)
            assert not got[b, n:].any(), f"item {b}: samples beyond its end are not zeros"
    finally:
        model.close()


if __name__ == "__main__" and "--child" in sys.argv:
    mode, path = sys.argv[sys.argv.index("--child") + 1:][:2]
    (pair_child_main if mode == "pair" else child_main)(path)
