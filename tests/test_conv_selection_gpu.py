"""Which conv kernel every launch takes (plan_conv, csrc/engine_convplan.hip.h), pinned by a recorded fixture.

tests/golden/conv_selection.json maps scenario -> {"op|kernel": launches}: the launch log (vits_debug_launch_log / _dump) of the scenarios
below, recorded before kernel selection was split from the launch.  The GPU tests replay every scenario and require the same map: missing
keys, extra keys and counts all fail.  The scenarios are the smallest that reach each leaf of the decision tree: single convs through
vits_op_conv1d under every forcing hook, and stage calls of the session-scoped models.  A change that moves a threshold on purpose records
the fixture again:  python tests/test_conv_selection_gpu.py --record
"""
import contextlib
import json
import os
import sys

import numpy as np
import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_selection.json")

# (B, C_in, C_out, T, K) and the leaf each takes with no hook set
CONV_SHAPES = (
    (1, 192, 192, 50, 3),     # conv16_kernel<STORE,...>
    (1, 256, 256, 600, 7),    # conv_wp_kernel<8>
    (1, 64, 64, 1000, 3),     # conv_mfma_ks_kernel<1,1,STORE,1,...>
    (8, 64, 32, 2048, 3),     # conv_mfma_kernel<1,4,1,1,STORE>
    (32, 64, 64, 2048, 3),    # conv_mfma_kernel<2,2,1,2,STORE>
    (32, 128, 128, 2048, 3),  # conv_mfma_kernel<2,2,2,2,STORE>
    (8, 192, 192, 1408, 3),   # conv_sp_kernel<STORE>
    (32, 192, 192, 1408, 3),  # conv_mfma_kernel<2,2,1,1,STORE>
)
DEFAULT_LEAVES = ("conv16_kernel<STORE,", "conv_wp_kernel<8>", "conv_mfma_ks_kernel<1,1,STORE,1,", "conv_mfma_kernel<1,4,1,1,STORE>",
                  "conv_mfma_kernel<2,2,1,2,STORE>", "conv_mfma_kernel<2,2,2,2,STORE>", "conv_sp_kernel<STORE>", "conv_mfma_kernel<2,2,1,1,STORE>")
# (hook, value, value that restores the default)
HOOKS = ((None, 0, 0), ("force_tile", 1, 0), ("force_tile", 2, 0), ("force_tile", 3, 0), ("conv_wp", 1, 0), ("conv_wp", 2, 0),
         ("conv_sp", 0, -1), ("conv_sp", 2, -1), ("ks_waves", 4, 0), ("ks_waves", 8, 0), ("ks_waves", 16, 0))
HOOK_IDS = ["default" if h is None else f"{h}{v}" for h, v, _ in HOOKS]
# every kernel-name family the scenarios are there to reach (prefixes of the names in the fixture)
FAMILIES = DEFAULT_LEAVES + (
    "conv_mfma_ks_kernel<1,2,STORE,", "conv16_kernel<STORE,ln,", "conv16_kernel<STORE,dds>", "conv16_kernel<GATE,", "conv16_kernel<COUPLE,",
    "conv16_kernel<RESSKIP,", "conv_mfma_kernel<2,2,2,1,GATE>", "conv_mfma_kernel<2,1,2,1,GATE>", "conv_mfma_kernel<2,2,1,1,RESSKIP>",
    "conv_mfma_kernel<2,2,1,1,COUPLE>", "conv_sp_kernel<RESSKIP>", "conv_sp_kernel<COUPLE>", "conv_mfma_ks_kernel<2,1,GATE,1,",
    "conv_mfma_ks_kernel<1,1,RESSKIP,1,", "conv_mfma_ks_kernel<1,1,COUPLE,1,", "conv_mfma_ks_kernel<1,1,STORE,2,", "conv_mfma_ks_kernel<1,1,STORE,3,",
    "conv_bf3_kernel<2>", "conv_bf3_kernel<1>", "conv_bf3_kernel<2,GATE>")


def _shape_id(shape):
    return "x".join(str(v) for v in shape)


@contextlib.contextmanager
def _hooks(lib, *rows):
    """sets every (hook, value, restore) of rows, and restores them all afterwards"""
    rows = [r for r in rows if r[0]]
    try:
        for hook, value, _ in rows:
            getattr(lib.lib, "vits_debug_" + hook)(value)
        yield
    finally:
        for hook, _, restore in rows:
            getattr(lib.lib, "vits_debug_" + hook)(restore)


def _logged(lib, run):
    lib.launch_log(1)
    try:
        run()
    finally:
        lib.launch_log(0)
    return lib.launch_dump()


def conv1d_scenarios(lib, hook_row):
    """{scenario: launch map} of every shape of CONV_SHAPES under one hook setting"""
    from vosk_tts_amd.capi import op_conv1d

    out = {}
    with _hooks(lib, hook_row):
        for shape in CONV_SHAPES:
            B, Cin, Cout, T, K = shape
            x, w = np.zeros((B, Cin, T), np.float32), np.zeros((Cout, Cin, K), np.float32)
            out[f"conv1d/{HOOK_IDS[HOOKS.index(hook_row)]}/{_shape_id(shape)}"] = _logged(lib, lambda: op_conv1d(lib, x, w, None))
    return out


def _text_dp(models):
    for m in (models["default"], models["tiny"]):
        hp = m.hp
        ids, lens, sid = np.ones((1, 50), np.int64), np.array([50], np.int64), np.array([1], np.int64)
        m.text_encoder(ids, lens, sid)
        m.duration(np.zeros((1, hp.hidden_channels, 50), np.float32), lens, sid, np.zeros((1, 2, 50), np.float32), 0.8)


def _flow_at(m, B, Ty):
    m.flow(np.zeros((B, m.hp.inter_channels, Ty), np.float32), np.full(B, Ty, np.int64), np.ones(B, np.int64))


def _flow(models):
    for B, Ty in ((1, 150), (8, 704), (16, 704)):
        _flow_at(models["default"], B, Ty)
    _flow_at(models["tiny"], 1, 150)


def _flow_small(models):
    _flow_at(models["default"], 1, 150)


def _flow_batch(models):
    _flow_at(models["default"], 8, 704)


def _decoder(models):
    m = models["default"]
    for B, Ty in ((1, 150), (8, 400)):
        m.decoder(np.zeros((B, m.hp.inter_channels, Ty), np.float32), want_mb=False)


def _bf16x3(models):
    m = models["bf16x3"]
    m.flow(np.zeros((16, m.hp.inter_channels, 704), np.float32), np.full(16, 704, np.int64), np.ones(16, np.int64))
    m.decoder(np.zeros((8, m.hp.inter_channels, 400), np.float32), want_mb=False)


def _stts_estimator(models):
    m = models["stts"]
    T = 304
    m.estimator(np.zeros((1, 80, T), np.float32), np.zeros((1, 256, T), np.float32), [T], 0.37, np.zeros((1, 128), np.float32))


# scenario -> (hooks, stage calls).  The forced ones are the only way to the leaves that no default-size stage reaches at test size: the
# 64 x 64 RESSKIP / COUPLE tiles (grids beyond 2048 workgroups otherwise), the K-split gate conv, conv_sp_kernel<COUPLE>, and the K-split
# kernel on the StableTTS estimator's channel-split pair
STAGE_TABLE = {
    "text_dp": ((), _text_dp),
    "text_dp_ln_stats0": ((("ln_stats", 0, 1),), _text_dp),
    "flow": ((), _flow),
    "flow_wn_fold0": ((("wn_fold", 0, 1),), _flow),
    "flow_batch_wn_fold0_force_tile1": ((("wn_fold", 0, 1), ("force_tile", 1, 0)), _flow_batch),
    "flow_batch_conv_sp2": ((("conv_sp", 2, -1),), _flow_batch),
    "flow_small_force_tile2": ((("force_tile", 2, 0),), _flow_small),
    "decoder": ((), _decoder),
    "bf16x3": ((), _bf16x3),
    "stts_estimator": ((), _stts_estimator),
    "stts_estimator_conv_wp1": ((("conv_wp", 1, 0),), _stts_estimator),
}
STAGES = tuple(STAGE_TABLE)


def stage_scenario(lib, models, name):
    """{scenario: launch map} of one stage scenario, on launches (the persistent programs off)"""
    hooks, run = STAGE_TABLE[name]
    lib.lib.vits_debug_persist(0)
    try:
        with _hooks(lib, *hooks):
            return {f"stage/{name}": _logged(lib, lambda: run(models))}
    finally:
        lib.lib.vits_debug_persist(7)


def create_extra_models(lib):
    """the two models the session fixtures do not have: a conv_precision = 1 default-size voice and a StableTTS voice"""
    from vosk_tts_amd import weights as W
    from vosk_tts_amd import weights_stts as S
    from vosk_tts_amd.capi_stts import SttsModel

    hp = W.default_hparams()
    hp.conv_precision = 1
    bf = lib.create(W.synthetic_blob(hp, 1234), 0)
    stts = SttsModel(lib, S.synthetic_blob(S.default_hparams(40, 7), 1234), lib.create(W.synthetic_blob(W.hifigan_v1_vocoder_hparams(), 1234), 0))
    return bf, stts


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------ CPU: the fixture itself
def test_fixture_names_every_kernel_family():
    """keeps the GPU tests from going vacuous: every scenario is in the fixture, and every leaf they are there to reach is named"""
    fx = load_fixture()
    want = {f"conv1d/{h}/{_shape_id(s)}" for h in HOOK_IDS for s in CONV_SHAPES} | {f"stage/{n}" for n in STAGES}
    assert set(fx) == want
    kernels = {key.split("|", 1)[1] for m in fx.values() for key in m}
    missing = [f for f in FAMILIES if not any(k.startswith(f) for k in kernels)]
    assert not missing, f"no scenario reaches {missing}"
    for shape, leaf in zip(CONV_SHAPES, DEFAULT_LEAVES):
        (key, n), = fx[f"conv1d/default/{_shape_id(shape)}"].items()
        assert key.startswith("op.conv1d|" + leaf) and n == 1, (shape, key, n)
    forced_ks = {key for name, m in fx.items() if name.startswith("conv1d/force_tile2/") for key in m}
    assert any(k.startswith("op.conv1d|conv_mfma_ks_kernel<1,2,STORE,1,") for k in forced_ks), forced_ks  # (the only way to the 32 x 64 K-split tile)


# ------------------------------------------------------------------------------------------------ GPU: replay
@pytest.fixture(scope="module")
def models(hip_lib, hip_default, hip_tiny):
    bf, stts = create_extra_models(hip_lib)
    yield {"default": hip_default, "tiny": hip_tiny, "bf16x3": bf, "stts": stts}
    bf.close()
    stts.close()


def _assert_same(got):
    fx = load_fixture()
    for name, m in got.items():
        assert m == fx[name], f"{name}: launches differ from the recorded selection\n  recorded {fx[name]}\n  now      {m}"


@pytest.mark.gpu
@pytest.mark.parametrize("hook_row", HOOKS, ids=HOOK_IDS)
def test_conv1d_selection(hip_lib, hook_row):
    _assert_same(conv1d_scenarios(hip_lib, hook_row))


@pytest.mark.gpu
@pytest.mark.parametrize("name", STAGES)
def test_stage_selection(hip_lib, models, name):
    _assert_same(stage_scenario(hip_lib, models, name))


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from vosk_tts_amd import weights as W
    from vosk_tts_amd.capi import VitsLib

    lib = VitsLib()
    bf, stts = create_extra_models(lib)
    all_models = {"default": lib.create(W.synthetic_blob(W.default_hparams(), 1234), 0), "tiny": lib.create(W.synthetic_blob(W.tiny_hparams(), 1234), 0),
                  "bf16x3": bf, "stts": stts}
    rec = {}
    for row in HOOKS:
        rec.update(conv1d_scenarios(lib, row))
    for stage in STAGES:
        rec.update(stage_scenario(lib, all_models, stage))
    out = sys.argv[sys.argv.index("--record") + 1] if len(sys.argv) > sys.argv.index("--record") + 1 else FIXTURE
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec)} scenarios to {out}")
