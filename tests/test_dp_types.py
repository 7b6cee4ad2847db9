"""The deterministic duration predictor (use_sdp false: DurationPredictor, models.py:104-139; hparams.dp_n_flows == 0) on the CPU
side: tensor inventory, ONNX import (synthetic and, where the reference tree exists, a real torch.onnx.export), the "use_sdp" config
check, the hparams refusals, the graphs that stay refused, and the ISA of the tail kernel.  The GPU side is tests/test_dp_types_gpu.py."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
DET = ("dp.conv_1.weight", "dp.conv_1.bias", "dp.norm_1.gamma", "dp.norm_1.beta", "dp.conv_2.weight", "dp.conv_2.bias",
       "dp.norm_2.gamma", "dp.norm_2.beta", "dp.proj.weight", "dp.proj.bias")


def test_hparams_of_the_deterministic_predictor():
    from vosk_tts_amd import weights as W

    for hp in (W.deterministic_dp_hparams(), W.tiny_deterministic_dp_hparams()):
        assert (hp.dp_n_flows, hp.dp_num_bins, hp.dp_dds_layers, hp.dp_filter_channels, hp.dp_kernel_size) == (0, 0, 0, 256, 3)
        W.validate_hparams(hp)
    assert W.tiny_deterministic_dp_hparams().gin_channels > 0 and W.tiny_deterministic_dp_hparams().n_speakers > 1
    # the stochastic voices keep their fields
    assert W.default_hparams().dp_n_flows == 4 and W.tiny_hparams().dp_n_flows == 4


@pytest.mark.parametrize("tiny", [True, False])
def test_inventory(tiny):
    from vosk_tts_amd import weights as W

    hp = W.tiny_deterministic_dp_hparams() if tiny else W.deterministic_dp_hparams()
    base = W.tiny_hparams() if tiny else W.default_hparams()
    H, D, G = hp.hidden_channels, hp.dp_filter_channels, hp.gin_channels
    specs = {n: s for n, s, *_ in W.tensor_specs(hp)}
    dp = {n: s for n, s in specs.items() if n.startswith("dp.")}
    assert dp == {"dp.conv_1.weight": (D, H, 3), "dp.conv_1.bias": (D,), "dp.norm_1.gamma": (D,), "dp.norm_1.beta": (D,),
                  "dp.conv_2.weight": (D, D, 3), "dp.conv_2.bias": (D,), "dp.norm_2.gamma": (D,), "dp.norm_2.beta": (D,),
                  "dp.proj.weight": (1, D, 1), "dp.proj.bias": (1,), "dp.cond.weight": (H, G, 1), "dp.cond.bias": (H,)}
    others = {n: s for n, s in specs.items() if not n.startswith("dp.")}
    assert others == {n: s for n, s, *_ in W.tensor_specs(base) if not n.startswith("dp.")}
    hp.gin_channels, hp.n_speakers = 0, 0
    assert not any(n.startswith(("dp.cond.", "emb_g.")) for n, *_ in W.tensor_specs(hp))


def test_synthetic_durations_are_speech_like():
    """dp.proj.bias of the synthetic weights centres exp(logw) at a few frames per token (the stochastic voices are unchanged)."""
    from vosk_tts_amd import weights as W

    b = W.make_synthetic_weights(W.tiny_deterministic_dp_hparams(), 1234)["dp.proj.bias"]
    assert b.shape == (1,) and 2.0 < np.exp(b[0]) < 6.0
    t = W.make_synthetic_weights(W.tiny_hparams(), 1234)
    assert abs(t["dp.proj.bias"]).max() <= 0.05


@pytest.mark.parametrize("tiny", [True, False])
def test_synthetic_graph_imports_and_round_trips(tmp_path, tiny):
    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W

    hp = W.tiny_deterministic_dp_hparams() if tiny else W.deterministic_dp_hparams()
    t = W.make_synthetic_weights(hp, 3)
    hp2, tens = oi.import_onnx(oi.write_minimal_onnx(str(tmp_path / "d.onnx"), t))
    assert bytes(hp2) == bytes(hp)
    assert set(tens) == set(t) and all(np.array_equal(tens[n], t[n]) for n in t)
    blob = W.pack_blob(hp2, tens)
    hp3, tens3 = W.unpack_blob(blob)
    assert hp3.dp_n_flows == 0 and bytes(hp3) == bytes(hp2)
    assert W.pack_blob(hp3, tens3) == blob


def test_use_sdp_must_agree_with_the_tensors(tmp_path):
    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W

    det = oi.write_minimal_onnx(str(tmp_path / "d.onnx"), W.make_synthetic_weights(W.tiny_deterministic_dp_hparams(), 3))
    sdp = oi.write_minimal_onnx(str(tmp_path / "s.onnx"), W.make_synthetic_weights(W.tiny_hparams(), 3))
    assert oi.import_onnx(det, {"use_sdp": False})[0].dp_n_flows == 0
    assert oi.import_onnx(sdp, {"use_sdp": True})[0].dp_n_flows == 4
    with pytest.raises(ValueError, match="use_sdp"):
        oi.import_onnx(det, {"use_sdp": True})
    with pytest.raises(ValueError, match="use_sdp"):
        oi.import_onnx(sdp, {"use_sdp": False})


def test_mixed_and_incomplete_predictors_are_named(tmp_path):
    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W

    t = W.make_synthetic_weights(W.tiny_deterministic_dp_hparams(), 3)
    for name in DET:
        part = {k: v for k, v in t.items() if k != name}
        with pytest.raises(NotImplementedError, match=re.escape(name)) as e:
            oi.import_onnx(oi.write_minimal_onnx(str(tmp_path / "p.onnx"), part))
        assert "DurationPredictor" in str(e.value)
    s = W.make_synthetic_weights(W.tiny_hparams(), 3)
    mixed = dict(t, **{k: v for k, v in s.items() if k.startswith("dp.flows.")})
    with pytest.raises(NotImplementedError, match="DurationPredictor"):
        oi.import_onnx(oi.write_minimal_onnx(str(tmp_path / "m.onnx"), mixed))


def test_hparams_refusals():
    from vosk_tts_amd import weights as W

    t = W.make_synthetic_weights(W.tiny_deterministic_dp_hparams(), 1)
    for field, value, what in (("dp_dds_layers", 3, "dp_dds_layers"), ("dp_num_bins", 10, "dp_num_bins"), ("dp_kernel_size", 4, "odd"),
                               ("dp_kernel_size", 0, "odd"), ("dp_filter_channels", 48, "filter channels"),
                               ("dp_filter_channels", 416, "filter channels")):
        hp = W.tiny_deterministic_dp_hparams()
        setattr(hp, field, value)
        with pytest.raises(ValueError, match=what):
            W.pack_blob(hp, t)


def test_real_export_imports_to_the_modules_blob():
    """torch.onnx.export of the reference's SynthesizerTrn(use_sdp=False) (tools/gen_golden_dp_types.py builds it;
    oracle/onnx_export_ref.export_vits is onnx_export.py's procedure) imports to the blob built from the module's state_dict."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import refimport

    if not refimport.have_reference():
        pytest.skip("reference tree not present")
    pytest.importorskip("torch")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_golden_dp_types as gen
    from onnx_export_ref import export_vits

    from vosk_tts_amd import onnx_import as oi
    from vosk_tts_amd import weights as W

    hp = W.tiny_deterministic_dp_hparams()
    net = gen.reference_model(hp)
    sd = {k: v.numpy() for k, v in net.state_dict().items()}
    hp2, tens = oi.import_onnx(export_vits(net), {"use_sdp": False})
    assert hp2.dp_n_flows == 0 and (hp2.dp_filter_channels, hp2.dp_kernel_size) == (256, 3)
    want = {n: sd[n] for n, *_ in W.tensor_specs(hp2)}
    assert W.pack_blob(hp2, tens) == W.pack_blob(hp2, want)


def test_tail_kernel_isa_has_no_scratch():
    """dp_det_tail_kernel keeps its D/8 channel values in registers: no scratch, and at least two 256-thread workgroups per SIMD set
    (occupancy >= 4 waves per SIMD)."""
    if not os.path.exists(HIPCC) or not shutil.which("c++filt"):
        pytest.skip("hipcc / c++filt not available")
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "engine.s")
        subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-w", "-S", "-o", out, "engine.hip"],
                              cwd=os.path.join(ROOT, "vosk_tts_amd", "csrc"))
        text = open(out).read()
    m = re.search(r"^(_Z\w*dp_det_tail_kernel\w*):\s+; @", text, flags=re.M)
    assert m, "dp_det_tail_kernel not in the device code"
    i = text.index("\n" + m.group(1) + ":")
    j = text.index(".Lfunc_end", i)
    meta = text[j:j + 6000]
    scratch = int(re.search(r"; ScratchSize: (\d+)", meta).group(1))
    occ = int(re.search(r"; Occupancy: (\d+)", meta).group(1))
    vgpr = int(re.search(r"; NumVgprs: (\d+)", meta).group(1))
    print(f"dp_det_tail_kernel: {vgpr} VGPRs, occupancy {occ}, scratch {scratch}")
    assert scratch == 0 and "scratch_" not in text[i:j]
    assert occ >= 4, occ
