"""The mono_layer_* flows (flow_type 4 = mono_layer_inter_residual, 5 = mono_layer_post_residual: [ResidualCouplingLayer, Flip,
MonoTransformerFlowLayer] per flow, models.py:696-734, 545-627) on the CPU side: the blob field, the tensor inventory, ONNX import
(synthetic and, where the reference tree exists, a real torch.onnx.export), the config that tells the two kinds apart, and the float64
restatement tests/flow_ref.py against fixtures computed by the reference's own SynthesizerTrn (tools/gen_golden_mono_flows.py).
The GPU side is tests/test_mono_flows_gpu.py."""
import os
import sys

import numpy as np
import pytest

from conftest import assert_close, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"monointer": 4, "monopost": 5}
CONFIG = {"monointer": {"use_transformer_flows": True, "transformer_flow_type": "mono_layer_inter_residual"},
          "monopost": {"use_transformer_flows": False, "transformer_flow_type": "mono_layer_post_residual"}}
ORACLE_PIN_TOL = 2e-5  # the bound the C oracle is pinned to the reference's fixtures with (tests/test_oracle_golden.py)


def _hp(kind, default=False):
    from vosk_tts_amd import weights as W

    if kind == "monointer":
        return W.mono_inter_hparams() if default else W.tiny_mono_inter_hparams()
    return W.mono_post_hparams() if default else W.tiny_mono_post_hparams()


@pytest.mark.parametrize("kind", KINDS)
def test_head_dims_are_validated_and_type_3_stays_refused(kind):
    from vosk_tts_amd import weights as W

    hp = _hp(kind)
    assert hp.flow_type == KINDS[kind]
    for I, ok in ((64, True), (128, True), (192, True), (320, True), (384, True), (96, False), (448, False)):
        hp.inter_channels = I
        if ok:
            W.validate_hparams(hp)
        else:
            with pytest.raises(ValueError, match=f"head dim inter_channels/4 = {I // 4} "):
                W.validate_hparams(hp)
    hp.inter_channels = 64
    for bad in (3, 6, -1):
        hp.flow_type = bad
        with pytest.raises(ValueError, match="flow_type"):
            W.validate_hparams(hp)
        with pytest.raises(ValueError, match="flow_type"):
            W.pack_blob(hp, {})


@pytest.mark.parametrize("kind", KINDS)
def test_inventory(kind):
    """The plain coupling layer's tensors at 3f, the mono layer's at 3f + 2, nothing at 3f + 1; everything else as the tiny voice."""
    from vosk_tts_amd import weights as W

    hp = _hp(kind)
    specs = dict((n, s) for n, s, *_ in W.tensor_specs(hp))
    plain = dict((n, s) for n, s, *_ in W.tensor_specs(W.tiny_plain_flow_hparams()))
    assert {n: s for n, s in specs.items() if not n.startswith("flow.")} == {n: s for n, s in plain.items() if not n.startswith("flow.")}
    half = hp.inter_channels // 2
    want = {}
    for f in range(hp.flow_n_flows):
        for n, s in plain.items():
            if n.startswith(f"flow.flows.{2 * f}."):
                want[n.replace(f"flow.flows.{2 * f}.", f"flow.flows.{3 * f}.", 1)] = s
        p = f"flow.flows.{3 * f + 2}"
        for i in range(2):
            for c in ("conv_q", "conv_k", "conv_v", "conv_o"):
                want[f"{p}.pre_transformer.attn_layers.{i}.{c}.weight"] = (half, half, 1)
                want[f"{p}.pre_transformer.attn_layers.{i}.{c}.bias"] = (half,)
            for c in ("conv_1", "conv_2"):
                want[f"{p}.pre_transformer.ffn_layers.{i}.{c}.weight"] = (half, half, 3)
                want[f"{p}.pre_transformer.ffn_layers.{i}.{c}.bias"] = (half,)
            for n in ("norm_layers_1", "norm_layers_2"):
                want[f"{p}.pre_transformer.{n}.{i}.gamma"] = (half,)
                want[f"{p}.pre_transformer.{n}.{i}.beta"] = (half,)
        want[p + ".post.weight"] = (half, half, 1)
        want[p + ".post.bias"] = (half,)
    assert {n: s for n, s in specs.items() if n.startswith("flow.")} == want
    t = W.make_synthetic_weights(hp, 1234)
    for f in range(hp.flow_n_flows):  # a zero post (the reference's init) would make the mono layer the identity on x1
        assert np.abs(t[f"flow.flows.{3 * f + 2}.post.weight"]).min() > 0 and np.abs(t[f"flow.flows.{3 * f + 2}.post.bias"]).max() > 0
    # the two kinds share their tensors, seed for seed
    other = W.make_synthetic_weights(_hp("monopost" if kind == "monointer" else "monointer"), 1234)
    assert set(other) == set(t) and all(np.array_equal(other[n], t[n]) for n in t)


@pytest.mark.parametrize("kind", KINDS)
def test_synthetic_graph_imports_with_its_config_and_round_trips(tmp_path, kind):
    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W

    hp = _hp(kind)
    t = W.make_synthetic_weights(hp, 3)
    path = oi.write_minimal_onnx(str(tmp_path / "m.onnx"), t)
    hp2, tens = oi.import_onnx(path, CONFIG[kind])
    assert hp2.flow_type == KINDS[kind] and hp2.flow_n_flows == hp.flow_n_flows == 4
    assert set(tens) == {n for n, *_ in W.tensor_specs(hp2)}
    assert all(np.array_equal(tens[n], t[n]) for n in tens)
    blob = W.pack_blob(hp2, tens)
    assert blob == W.pack_blob(hp, t)
    hp3, tens3 = W.unpack_blob(blob)
    assert hp3.flow_type == KINDS[kind] and bytes(hp3) == bytes(hp2)
    assert W.pack_blob(hp3, tens3) == blob


def test_the_config_decides_between_the_two_kinds(tmp_path):
    """Absent keys select mono_layer_post_residual, as SynthesizerTrn's defaults do (models.py:1560-1561); no config at all cannot
    decide; a config that selects another family contradicts the tensors."""
    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W

    path = oi.write_minimal_onnx(str(tmp_path / "m.onnx"), W.make_synthetic_weights(W.tiny_mono_post_hparams(), 3))
    assert oi.import_onnx(path, {})[0].flow_type == 5
    assert oi.import_onnx(path, {"sampling_rate": 22050})[0].flow_type == 5
    assert oi.import_onnx(path, {"use_transformer_flows": False})[0].flow_type == 5
    assert oi.import_onnx(path, CONFIG["monointer"])[0].flow_type == 4
    with pytest.raises(ValueError, match="use_transformer_flows.*transformer_flow_type"):
        oi.import_onnx(path)
    for cfg in ({"use_transformer_flows": True, "transformer_flow_type": "pre_conv"},
                {"use_transformer_flows": True, "transformer_flow_type": "pre_conv2"},
                {"use_transformer_flows": True, "transformer_flow_type": "fft"},
                {"use_transformer_flows": True},  # builds no flow at all
                {"use_transformer_flows": False, "transformer_flow_type": "mono_layer_inter_residual"}):  # the outer elif: plain
        with pytest.raises(ValueError, match="flow"):
            oi.import_onnx(path, cfg)
    # and the other way round: a mono config on graphs of the other families
    for other in (W.tiny_hparams(), W.tiny_pre_conv_hparams(), W.tiny_plain_flow_hparams()):
        p = oi.write_minimal_onnx(str(tmp_path / "o.onnx"), W.make_synthetic_weights(other, 3))
        for kind in KINDS:
            with pytest.raises(ValueError, match="flow"):
                oi.import_onnx(p, CONFIG[kind])


def test_incomplete_or_misplaced_mono_layers_are_named(tmp_path):
    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W

    t = W.make_synthetic_weights(W.tiny_mono_inter_hparams(), 3)
    cut = {k: v for k, v in t.items() if k != "flow.flows.8.pre_transformer.norm_layers_2.1.beta"}
    with pytest.raises(NotImplementedError, match=r"mono_layer.*flow\.flows\.8\.pre_transformer\.norm_layers_2\.1\.beta"):
        oi.import_onnx(oi.write_minimal_onnx(str(tmp_path / "a.onnx"), cut), CONFIG["monointer"])
    wide = dict(t)
    wide["flow.flows.5.post.weight"] = np.zeros((64, 64, 1), np.float32)
    with pytest.raises(NotImplementedError, match=r"mono_layer.*flow\.flows\.5\.post\.weight"):
        oi.import_onnx(oi.write_minimal_onnx(str(tmp_path / "b.onnx"), wide), CONFIG["monointer"])
    fft = dict(t)
    fft["flow.flows.0.enc.self_attn_layers.0.conv_q.weight"] = np.zeros((64, 64, 1), np.float32)
    with pytest.raises(NotImplementedError, match="fft"):
        oi.import_onnx(oi.write_minimal_onnx(str(tmp_path / "f.onnx"), fft), CONFIG["monointer"])


@pytest.mark.parametrize("kind", KINDS)
def test_real_export_imports_to_the_modules_blob(kind):
    """torch.onnx.export of the reference's SynthesizerTrn with the mono flow its config selects (tools/gen_golden_mono_flows.py
    builds it; oracle/onnx_export_ref.export_vits is onnx_export.py's procedure) imports to the blob built from the module's
    state_dict."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import refimport

    if not refimport.have_reference():
        pytest.skip("reference tree not present")
    pytest.importorskip("torch")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_golden_mono_flows as gen
    from onnx_export_ref import export_vits

    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W

    hp = _hp(kind)
    net = gen.reference_model(hp)
    sd = {k: v.numpy() for k, v in net.state_dict().items()}
    hp2, tens = oi.import_onnx(export_vits(net), dict(gen.CONFIG[hp.flow_type]))
    assert hp2.flow_type == KINDS[kind] and hp2.flow_n_flows == 4
    want = {n: sd[n] for n, *_ in W.tensor_specs(hp2)}
    assert W.pack_blob(hp2, tens) == W.pack_blob(hp2, want)


@pytest.mark.parametrize("case", ["tiny_b3", "default_b2"])
@pytest.mark.parametrize("kind", KINDS)
def test_flow_ref_reproduces_the_reference(kind, case):
    """tests/flow_ref.py (float64, written from the formulas) against the reference's own float32 SynthesizerTrn, valid frames."""
    pytest.importorskip("torch")
    import flow_ref

    from vosk_tts_amd import weights as W

    hp = _hp(kind, default=case == "default_b2")
    g = golden(f"flow_{kind}_{case}")
    z = flow_ref.flow_reverse(hp, W.make_synthetic_weights(hp, 1234), g["z_p"], g["y_lengths"], g["sid"])
    for b, n in enumerate(g["y_lengths"]):
        assert_close(f"{kind} {case} z[{b}]", g["z"][b, :, :n], z[b, :, :n], ORACLE_PIN_TOL)


def test_flow_ref_tells_the_kinds_and_the_flip_parity_apart():
    """The restatement is only worth something if the errors the GPU tests are after move it: the other kind, and a Flip on the
    wrong side of the mono layer, each miss the fixture by far more than any tolerance in use."""
    pytest.importorskip("torch")
    import flow_ref
    import torch

    from vosk_tts_amd import weights as W

    hp = _hp("monointer")
    g = golden("flow_monointer_tiny_b3")
    t = W.make_synthetic_weights(hp, 1234)
    n = int(g["y_lengths"][0])
    scale = np.abs(g["z"][0, :, :n]).max()
    other = flow_ref.flow_reverse(_hp("monopost"), t, g["z_p"], g["y_lengths"], g["sid"])
    assert np.abs(other[0, :, :n] - g["z"][0, :, :n]).max() > 1e-2 * scale
    orig = flow_ref.mono_reverse
    try:
        flow_ref.mono_reverse = lambda z, T, p, post: torch.flip(orig(torch.flip(z, [1]), T, p, post), [1])
        wrong = flow_ref.flow_reverse(hp, t, g["z_p"], g["y_lengths"], g["sid"])
    finally:
        flow_ref.mono_reverse = orig
    assert np.abs(wrong[0, :, :n] - g["z"][0, :, :n]).max() > 1e-2 * scale
