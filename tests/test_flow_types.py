"""The `pre_conv` (flow_type 1, ResidualCouplingTransformersLayer, models.py:399-483) and plain (flow_type 2,
modules.ResidualCouplingLayer, modules.py:298-345) flows on the CPU side: blob field, tensor inventory, ONNX import (synthetic and,
where the reference tree exists, a real torch.onnx.export), the config selection of models.py:653-747, the flows that stay
unsupported, and the ISA of the attention kernels without relative positions.  The GPU side is tests/test_flow_types_gpu.py."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KINDS = {"pre_conv": 1, "plain": 2}


def _tiny(kind):
    from vosk_tts_amd import weights as W

    return W.tiny_pre_conv_hparams() if kind == "pre_conv" else W.tiny_plain_flow_hparams()


def test_flow_type_takes_a_reserved_word_and_defaults_to_pre_conv2():
    from vosk_tts_amd import weights as W

    assert ctypes.sizeof(W.HParams) == 284
    assert W.HParams.flow_type.offset == W.HParams.reserved.offset - 4 and len(W.HParams().reserved) == 5
    hp = W.default_hparams()
    assert hp.flow_type == 0
    # a blob written before the field existed (the word was reserved and zero) packs byte-identically
    raw = bytearray(bytes(hp))
    assert raw[W.HParams.flow_type.offset:W.HParams.flow_type.offset + 4] == b"\0\0\0\0"
    t = W.make_synthetic_weights(hp, 7)
    assert W.pack_blob(hp, t) == W.pack_blob(W.HParams.from_buffer_copy(bytes(raw)), t)


@pytest.mark.parametrize("kind", KINDS)
def test_inventories(kind):
    from vosk_tts_amd import weights as W

    hp = _tiny(kind)
    names = [n for n, *_ in W.tensor_specs(hp)]
    base = {n for n, *_ in W.tensor_specs(W.tiny_hparams())}
    assert not any(".post_transformer." in n for n in names)
    assert not any("emb_rel" in n and n.startswith("flow.") for n in names)
    flow = {n for n in names if n.startswith("flow.")}
    assert {n for n in names if not n.startswith("flow.")} == {n for n in base if not n.startswith("flow.")}
    if kind == "plain":
        assert not any(".pre_transformer." in n for n in flow)
        assert flow == {n for n in base if n.startswith("flow.") and ".pre_transformer." not in n}
    else:
        I = hp.inter_channels
        specs = dict((n, s) for n, s, *_ in W.tensor_specs(hp))
        assert specs["flow.flows.0.pre_transformer.attn_layers.1.conv_q.weight"] == (I // 2, I // 2, 1)
        assert specs["flow.flows.0.pre_transformer.ffn_layers.1.conv_1.weight"] == (I // 2, I // 2, 3)
        assert "flow.flows.0.pre_transformer.attn_layers.2.conv_q.weight" not in specs
        assert specs["flow.flows.6.pre.weight"] == (hp.hidden_channels, I // 2, 1)


@pytest.mark.parametrize("kind", KINDS)
def test_synthetic_graph_imports_with_its_flow_type_and_round_trips(tmp_path, kind):
    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W

    hp = _tiny(kind)
    t = W.make_synthetic_weights(hp, 3)
    hp2, tens = oi.import_onnx(oi.write_minimal_onnx(str(tmp_path / "f.onnx"), t))
    assert hp2.flow_type == KINDS[kind]
    assert set(tens) == {n for n, *_ in W.tensor_specs(hp2)}
    assert all(np.array_equal(tens[n], t[n]) for n in tens)
    blob = W.pack_blob(hp2, tens)
    hp3, tens3 = W.unpack_blob(blob)
    assert hp3.flow_type == KINDS[kind] and bytes(hp3) == bytes(hp2)
    assert W.pack_blob(hp3, tens3) == blob


def test_pre_conv_head_dims_are_validated():
    from vosk_tts_amd import weights as W

    hp = W.tiny_pre_conv_hparams()
    for I, ok in ((64, True), (128, True), (192, True), (320, True), (384, True), (96, False), (448, False)):
        hp.inter_channels = I
        if ok:
            W.validate_hparams(hp)
        else:
            with pytest.raises(ValueError, match="head dim"):
                W.validate_hparams(hp)
    hp.inter_channels = 64
    hp.flow_type = 3
    with pytest.raises(ValueError, match="flow_type"):
        W.validate_hparams(hp)


def test_config_selection_follows_the_reference():
    """models.py:653-747 with SynthesizerTrn's defaults (:1560-1561): mono_layer_post_residual is an OUTER elif."""
    from vosk_tts_amd.onnx_import import flow_kind_from_config as kind

    assert kind({}) == "mono_layer_post_residual"
    assert kind({"use_transformer_flows": True, "transformer_flow_type": "pre_conv2"}) == "pre_conv2"
    assert kind({"use_transformer_flows": True, "transformer_flow_type": "pre_conv"}) == "pre_conv"
    assert kind({"use_transformer_flows": True}) == "none"  # no type given: the default mono_layer_post_residual builds nothing here
    assert kind({"use_transformer_flows": True, "transformer_flow_type": "fft"}) == "fft"
    assert kind({"use_transformer_flows": True, "transformer_flow_type": "mono_layer_inter_residual"}) == "mono_layer_inter_residual"
    assert kind({"use_transformer_flows": False, "transformer_flow_type": "mono_layer_post_residual"}) == "mono_layer_post_residual"
    for t in ("pre_conv", "pre_conv2", "fft", "mono_layer_inter_residual", "anything"):
        assert kind({"use_transformer_flows": False, "transformer_flow_type": t}) == "plain"


def test_config_must_agree_with_the_tensors(tmp_path):
    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W

    path = oi.write_minimal_onnx(str(tmp_path / "p.onnx"), W.make_synthetic_weights(W.tiny_pre_conv_hparams(), 3))
    hp, _ = oi.import_onnx(path, {"use_transformer_flows": True, "transformer_flow_type": "pre_conv"})
    assert hp.flow_type == 1
    for cfg in ({"use_transformer_flows": True, "transformer_flow_type": "pre_conv2"},
                {"use_transformer_flows": False, "transformer_flow_type": "pre_conv"},  # the outer elif: plain
                {"use_transformer_flows": False}):  # mono_layer_post_residual
        with pytest.raises(ValueError, match="flow"):
            oi.import_onnx(path, cfg)
    path0 = oi.write_minimal_onnx(str(tmp_path / "z.onnx"), W.make_synthetic_weights(W.tiny_hparams(), 3))
    assert oi.import_onnx(path0, {"use_transformer_flows": True, "transformer_flow_type": "pre_conv2"})[0].flow_type == 0
    with pytest.raises(ValueError, match="flow"):
        oi.import_onnx(path0, {"use_transformer_flows": True, "transformer_flow_type": "pre_conv"})


def test_unsupported_flows_are_named(tmp_path):
    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W

    t = W.make_synthetic_weights(W.tiny_plain_flow_hparams(), 3)
    # mono_layer_*: coupling layers at 0, 3, 6, 9 and MonoTransformerFlowLayer (pre_transformer + post, no pre) at 2, 5, ...
    mono = {k: v for k, v in t.items() if not k.startswith("flow.")}
    src = {k: v for k, v in t.items() if k.startswith("flow.flows.0.")}
    for f in range(4):
        mono.update({k.replace("flow.flows.0.", f"flow.flows.{3 * f}."): v for k, v in src.items()})
        mono[f"flow.flows.{3 * f + 2}.pre_transformer.attn_layers.0.conv_q.weight"] = np.zeros((32, 32, 1), np.float32)
        mono[f"flow.flows.{3 * f + 2}.post.weight"] = np.zeros((32, 32, 1), np.float32)
    with pytest.raises(NotImplementedError, match="mono_layer"):
        oi.import_onnx(oi.write_minimal_onnx(str(tmp_path / "m.onnx"), mono))
    fft = dict(t)
    fft["flow.flows.0.enc.self_attn_layers.0.conv_q.weight"] = np.zeros((64, 64, 1), np.float32)
    with pytest.raises(NotImplementedError, match="fft"):
        oi.import_onnx(oi.write_minimal_onnx(str(tmp_path / "f.onnx"), fft))


@pytest.mark.parametrize("kind", KINDS)
def test_real_export_imports_to_the_modules_blob(kind):
    """torch.onnx.export of the reference's SynthesizerTrn with the flow the config selects (tools/gen_golden_flow_types.py builds
    it; oracle/onnx_export_ref.export_vits is onnx_export.py's procedure) imports to the blob built from the module's state_dict."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import refimport

    if not refimport.have_reference():
        pytest.skip("reference tree not present")
    pytest.importorskip("torch")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_golden_flow_types as gen
    from onnx_export_ref import export_vits

    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W

    hp = _tiny(kind)
    net = gen.reference_model(hp)
    sd = {k: v.numpy() for k, v in net.state_dict().items()}
    hp2, tens = oi.import_onnx(export_vits(net), dict(gen.CONFIG[hp.flow_type]))
    assert hp2.flow_type == KINDS[kind]
    want = {n: sd[n] for n, *_ in W.tensor_specs(hp2)}
    assert W.pack_blob(hp2, tens) == W.pack_blob(hp2, want)


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC) or not shutil.which("c++filt"):
        pytest.skip("hipcc / c++filt not available")
    out = tmp_path_factory.mktemp("isa") / "engine.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-w", "-S", "-o", str(out), "engine.hip"],
                          cwd=os.path.join(ROOT, "vosk_tts_amd", "csrc"))
    text = out.read_text()
    mangled = re.findall(r"^(_Z[0-9A-Za-z_]+):\s+; @", text, flags=re.M)
    names = subprocess.run(["c++filt"] + mangled, capture_output=True, text=True, check=True).stdout.splitlines()
    kernels = {}
    for m, d in zip(mangled, names):
        if "plain_attention" not in d:
            continue
        i = text.index("\n" + m + ":")
        j = text.index(".Lfunc_end", i)
        meta = text[j:j + 6000]
        kernels[d.split("(")[0].replace("void ", "")] = dict(
            body=text[i:j], scratch=int(re.search(r"; ScratchSize: (\d+)", meta).group(1)),
            occupancy=int(re.search(r"; Occupancy: (\d+)", meta).group(1)))
    return kernels


def test_plain_attention_kernels_are_fp32_mfma_without_spills(isa):
    """Every instantiation runs on the fp32 matrix cores (no bf16 / xf32 forms), keeps no scratch, and keeps its occupancy: the
    32-query kernel two 256-thread workgroups per CU (__launch_bounds__(256, 2)), four up to head dim 48; the 16-query kernel three."""
    for dk in (16, 32, 48, 64, 80, 96):
        k = isa[f"plain_attention_kernel<{dk}>"]
        assert "v_mfma_f32_32x32x2_f32" in k["body"] and k["scratch"] == 0, (dk, k["scratch"])
        assert not re.search(r"v_mfma_\w*(bf16|xf32)", k["body"])
        assert k["occupancy"] >= (4 if dk <= 48 else 2), (dk, k["occupancy"])
        for nw in (4, 8):
            k = isa[f"plain_attention16_kernel<{dk}, {nw}>"]
            assert "v_mfma_f32_16x16x4_f32" in k["body"] and k["scratch"] == 0, (dk, nw, k["scratch"])
            assert not re.search(r"v_mfma_\w*(bf16|xf32)", k["body"])
            assert k["occupancy"] >= 3, (dk, nw, k["occupancy"])
