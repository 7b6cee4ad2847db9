"""The chunk-owned contraction of the 16-wave K-split conv kernel (ks_chunk_body, csrc/conv_mfma.hip.h; who takes it: ks_chunk_takes,
csrc/engine_launch.hip.h; A/B switch: VITS_KS_CHUNK=0|1, read once per process).

  * single convs through vits_op_conv1d on the K-split kernel with 16 waves (force_tile 2, ks_waves 16) against a float64 numpy conv:
    C_in 128 / 192 / 512 (8 and 12 chunks: half-chunk units; 32: whole chunks, two per wave), C_out 32 / 64, 4 and 7 taps (the two
    unrolled tap counts), T 1 / 3 (rows shorter than a vector load: the launch keeps the tap split) / 31 / 32 / 33 / 65 (edge tiles on
    both sides, one and several column tiles), leaky-relu slopes 0.1 and 0.01.  vits_op_conv1d has no mask, no second or third input and
    no reflection column, and the ABI is pinned (tests/test_abi_cpu.py): those staging cases run through the decoder below, where
    ups[i > 0] and conv_post read the three-input MRF mean (in_scale 1/3), conv_post the reflection column (dec_type 0 / 2) or none
    (dec_type 1), conv_pre adds cond(g) (hg_cond_4x12_u3), and a bucketed single utterance puts the length limit inside a tile;
  * the decoder (tests/decoder_ref.py, float64) at T_y 1 / 2 / 5 / 33 for mb_default, ms_4stage, hg_v1 and hg_cond_4x12_u3, by the
    default dispatch and with every conv forced onto the 16-wave K-split kernel: both polyphase shapes that share a window (4 taps per
    phase: (4,16) and (2,8)), the ones that do not (1 - 3 taps per phase stay on the tap split), conv_pre and conv_post;
  * the same inputs in two child processes, VITS_KS_CHUNK=0 and 1: both meet the float64 bounds, they differ (the switch does
    something: the summation order changes), and their largest difference is printed (-s);
  * the launch log of the recorded decoder scenario (tests/golden/conv_selection.json, "stage/decoder": the c2-shaped single
    utterance and a batch) is the recorded one under both settings.

Tolerances.  Decoder: STAGE_TOL of tests/test_decoder_geometry_gpu.py, imported.  Single convs: CONV_TOL = 2e-5 on the assert_close
scale (max abs error over max abs reference), the bound the project's other K-split tests hold against the fp32 oracle
(tests/test_hip_parity.py).  From the formats: n = C_in K <= 3584 fp32 products of unit-variance inputs and weights of variance 1 / n
are summed in chains of at most n / 16 + 16 terms; with u = 2^-24 a random walk of rounding errors over n terms of rms 1 / sqrt(n)
gives about sqrt(n) u / sqrt(n) = 6e-8 per output against max |y| of about 4: 2e-5 leaves two orders of magnitude for the worst
element of 10^4 outputs and still sits four orders below an indexing error (1e-1).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_close

CONV_TOL = 2e-5
HERE = os.path.dirname(os.path.abspath(__file__))
CINS, COUTS, TAPS, TS, SLOPES = (128, 192, 512), (32, 64), (4, 7), (1, 3, 31, 32, 33, 65), (0.1, 0.01)
DEC_ROWS = ("mb_default", "ms_4stage", "hg_v1", "hg_cond_4x12_u3")
DEC_TYS = (1, 2, 5, 33)
KS16 = (("force_tile", 2, 0), ("ks_waves", 16, 0))


def conv_ref(x, w, bias, dil, slope):
    """float64 'same'-padded conv of leaky_relu(x), pad_l = (K - 1) dil // 2 as vits_op_conv1d"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, Cin, T = x.shape
    K = w.shape[2]
    pad_l = (K - 1) * dil // 2
    xa = np.zeros((B, Cin, T + (K - 1) * dil))
    xa[:, :, pad_l:pad_l + T] = np.where(x >= 0, x, x * slope)
    y = np.zeros((B, w.shape[0], T))
    for k in range(K):
        y += np.einsum("oc,bct->bot", w[:, :, k], xa[:, :, k * dil:k * dil + T])
    return y + np.asarray(bias, np.float64)[None, :, None]


def conv_case(Cin, Cout, K, T, slope):
    """seeded inputs of one case: B = 2 for odd T (the batch index enters the addresses)"""
    rng = np.random.default_rng([Cin, Cout, K, T, int(slope * 100)])
    x = rng.standard_normal((1 + T % 2, Cin, T)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, K)) / np.sqrt(Cin * K)).astype(np.float32)
    return x, w, rng.standard_normal(Cout).astype(np.float32)


class hooks:
    def __init__(self, lib, rows):
        self.lib, self.rows = lib, rows

    def __enter__(self):
        for h, v, _ in self.rows:
            getattr(self.lib.lib, "vits_debug_" + h)(v)

    def __exit__(self, *a):
        for h, _, r in self.rows:
            getattr(self.lib.lib, "vits_debug_" + h)(r)


def dec_case(name, Ty):
    from decoder_grid import GRID, row_hparams
    from vosk_tts_amd import weights as W

    row = {r[0]: r for r in GRID}[name]
    hp = row_hparams(row)
    tens = W.make_synthetic_weights(hp, 1234)
    z = np.random.default_rng([DEC_ROWS.index(name), Ty]).standard_normal((1, hp.inter_channels, Ty)).astype(np.float32)
    return hp, tens, z, (np.array([3], np.int64) if row[8] else None)


# ------------------------------------------------------------------------------------------------ in this process
@pytest.mark.gpu
@pytest.mark.parametrize("K", TAPS)
@pytest.mark.parametrize("Cin", CINS)
def test_single_convs_against_float64(hip_lib, Cin, K):
    from vosk_tts_amd.capi import op_conv1d

    worst = 0.0
    with hooks(hip_lib, KS16):
        for Cout in COUTS:
            for T in TS:
                for slope in SLOPES:
                    x, w, bias = conv_case(Cin, Cout, K, T, slope)
                    e = assert_close(f"conv1d Cin={Cin} Cout={Cout} K={K} T={T} slope={slope}", conv_ref(x, w, bias, 1, slope),
                                     op_conv1d(hip_lib, x, w, bias, 1, slope), CONV_TOL)
                    worst = max(worst, e)
    print(f"K-split 16 waves, Cin={Cin} K={K}: worst {worst:.2e}")


@pytest.fixture(scope="module")
def dec_refs():
    from decoder_ref import decoder_ref

    out = {}
    for name in DEC_ROWS:
        for Ty in DEC_TYS:
            hp, tens, z, sid = dec_case(name, Ty)
            out[name, Ty] = decoder_ref(hp, tens, z, sid=sid)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", DEC_ROWS)
def test_decoder_against_float64(hip_lib, dec_refs, name):
    from test_decoder_geometry_gpu import STAGE_TOL
    from vosk_tts_amd import weights as W

    hp, tens, _, _ = dec_case(name, 1)
    model = hip_lib.create(W.pack_blob(hp, tens), 0)
    try:
        for Ty in DEC_TYS:
            _, _, z, sid = dec_case(name, Ty)
            a, mb = dec_refs[name, Ty]
            for label, rows in (("default", ()), ("K-split 16 waves", KS16)):
                with hooks(hip_lib, rows):
                    got = model.decoder(z, sid=sid)
                e = assert_close(f"{name} T_y={Ty} {label}: audio", a, got[0], STAGE_TOL)
                if mb is not None:
                    e = max(e, assert_close(f"{name} T_y={Ty} {label}: audio_mb", mb, got[1], STAGE_TOL))
                print(f"{name} T_y={Ty} {label}: {e:.2e}")
    finally:
        model.close()


@pytest.mark.gpu
def test_bucketed_single_utterance_length_limit_inside_a_tile(hip_lib, hip_default, oracle_default):
    """the fast path pads a single utterance to its bucket: the decoder's launches then carry a length limit that falls inside a
    column tile of conv_pre and of the upsamplers (graph replay against the exact-size eager path, and against the CPU oracle)"""
    from test_hip_parity import E2E_TOL

    rng = np.random.default_rng(77)
    Tx = 21
    ids = rng.integers(1, 62, size=(1, Tx)).astype(np.int64)
    dur = rng.integers(1, 4, size=(1, Tx)).astype(np.int32)
    want, wl = oracle_default.synthesize(ids, [Tx], [0.667, 1.0, 0.8], [2], forced_durations=dur, seed=5)
    try:
        for on in (1, 0):
            hip_lib.lib.vits_debug_fast_path(on)
            got, gl = hip_default.synthesize(ids, [Tx], [0.667, 1.0, 0.8], [2], forced_durations=dur, seed=5)
            assert np.array_equal(gl, wl)
            n = int(wl[0])
            assert_close(f"single utterance, fast path {on}", want[0, :n], got[0, :n], E2E_TOL)
    finally:
        hip_lib.lib.vits_debug_fast_path(1)


# ------------------------------------------------------------------------------------------------ two child processes
CHILD_CONVS = [(Cin, 64, K, T, 0.1) for Cin in CINS for K in TAPS for T in (33, 65)]
CHILD_DEC = [(name, Ty) for name in DEC_ROWS for Ty in (5, 33)]


def child_main(out_path):
    import conftest  # noqa: F401  (torch before the library, as the suite)
    from test_conv_selection_gpu import stage_scenario
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.capi import VitsLib, op_conv1d

    lib = VitsLib()
    out = {}
    with hooks(lib, KS16):
        for i, c in enumerate(CHILD_CONVS):
            x, w, bias = conv_case(*c)
            out[f"conv{i}"] = op_conv1d(lib, x, w, bias, 1, c[4])
    for name in DEC_ROWS:
        hp, tens, _, _ = dec_case(name, 1)
        model = lib.create(W.pack_blob(hp, tens), 0)
        for n2, Ty in CHILD_DEC:
            if n2 == name:
                _, _, z, sid = dec_case(name, Ty)
                with hooks(lib, KS16):
                    out[f"dec_{name}_{Ty}"] = model.decoder(z, sid=sid, want_mb=False)[0]
        model.close()
    default = lib.create(W.synthetic_blob(W.default_hparams(), 1234), 0)
    out["log"] = np.array(json.dumps(stage_scenario(lib, {"default": default}, "decoder"), sort_keys=True))
    default.close()
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """{setting: npz of the child's outputs}: both children run at the same time"""
    d = tmp_path_factory.mktemp("ks_chunk")
    procs = {}
    for v in ("0", "1"):
        env = dict(os.environ, VITS_KS_CHUNK=v)
        procs[v] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", str(d / f"out{v}.npz")], env=env, cwd=HERE,
                                    stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    res = {}
    for v, p in procs.items():
        log, _ = p.communicate()
        assert p.returncode == 0, f"child VITS_KS_CHUNK={v} ended with {p.returncode}:\n{log[-2000:]}"
        res[v] = dict(np.load(d / f"out{v}.npz"))
    return res


@pytest.mark.gpu
def test_tap_split_and_chunk_split_both_meet_the_bounds(children, dec_refs):
    from test_decoder_geometry_gpu import STAGE_TOL

    diff = {"conv": 0.0, "dec": 0.0}
    for i, c in enumerate(CHILD_CONVS):
        x, w, bias = conv_case(*c)
        ref = conv_ref(x, w, bias, 1, c[4])
        for v in ("0", "1"):
            assert_close(f"VITS_KS_CHUNK={v} conv {c}", ref, children[v][f"conv{i}"], CONV_TOL)
        diff["conv"] = max(diff["conv"], np.abs(children["0"][f"conv{i}"] - children["1"][f"conv{i}"]).max() / np.abs(ref).max())
    for name, Ty in CHILD_DEC:
        ref = dec_refs[name, Ty][0]
        for v in ("0", "1"):
            assert_close(f"VITS_KS_CHUNK={v} decoder {name} T_y={Ty}", ref, children[v][f"dec_{name}_{Ty}"], STAGE_TOL)
        diff["dec"] = max(diff["dec"], np.abs(children["0"][f"dec_{name}_{Ty}"] - children["1"][f"dec_{name}_{Ty}"]).max() / np.abs(ref).max())
    print(f"tap split vs chunk split, largest difference over max |ref|: single convs {diff['conv']:.2e}, decoder audio {diff['dec']:.2e}")
    assert diff["conv"] > 0 and diff["dec"] > 0, "VITS_KS_CHUNK changed nothing: the chunk split did not run"


@pytest.mark.gpu
def test_launch_log_is_the_recorded_one_under_both_settings(children):
    from test_conv_selection_gpu import load_fixture

    want = json.dumps({"stage/decoder": load_fixture()["stage/decoder"]}, sort_keys=True)
    for v in ("0", "1"):
        assert str(children[v]["log"]) == want, f"VITS_KS_CHUNK={v}: launches differ from the recorded selection"


if __name__ == "__main__" and "--child" in sys.argv:
    child_main(sys.argv[sys.argv.index("--child") + 1])
