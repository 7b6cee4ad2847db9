"""The vocoder-bias denoiser (include/vits_denoise.h) without a device: the float64 restatement the GPU tests use as their reference
(tests/denoise_ref.py) against torch.stft / torch.istft, and the Python surface (feed keys, Synth, CLI, config default)."""
import json
import os

import numpy as np
import pytest

import denoise_ref as R

FILTERS = (64, 1024)
STRENGTHS = (2.5e-4, 0.5, 50.0)


def _lengths(n):
    return (n // 2 + 1, 3 * n + 17, 40 * (n // 4))


def _torch_denoise(x, bias, strength, n, dtype):
    """the reference's route in torch (magnitude and angle of torch.stft, the clamped subtraction, cos / sin back, torch.istft)"""
    import torch

    hop = n // 4
    w = torch.hann_window(n, dtype=dtype)
    spec = torch.stft(torch.as_tensor(x, dtype=dtype)[None], n_fft=n, hop_length=hop, win_length=n, window=w, return_complex=True)
    mag, ang = spec.abs(), torch.atan2(spec.imag, spec.real)
    mag = torch.clamp(mag - torch.as_tensor(bias, dtype=dtype)[None, :, None] * strength, 0.0)
    out = torch.istft(torch.complex(mag * torch.cos(ang), mag * torch.sin(ang)), n_fft=n, hop_length=hop, win_length=n, window=w)
    return out[0].numpy()


@pytest.mark.parametrize("n", FILTERS)
def test_restatement_agrees_with_torch_stft_istft_in_float64(n):
    import torch

    rng = np.random.default_rng(n)
    bias = rng.uniform(0.5, 1.5, n // 2 + 1) * 0.1 * np.sqrt(n)
    for length in _lengths(n):
        x = rng.uniform(-0.3, 0.3, length)
        for s in STRENGTHS:
            want = _torch_denoise(x, bias, s, n, torch.float64)
            got = R.denoise(x, bias, s, n)
            assert got.shape == want.shape == (R.out_length(length, n),)
            err = np.abs(got - want).max()
            assert err <= 1e-12 * np.abs(x).max(), (n, length, s, err)
    # the bias: frame 0 of torch.stft
    audio = rng.standard_normal(88 * 256)
    spec = torch.stft(torch.as_tensor(audio)[None], n_fft=n, hop_length=n // 4, win_length=n, window=torch.hann_window(n, dtype=torch.float64),
                      return_complex=True)
    want = spec.abs()[0, :, 0].numpy()
    assert np.abs(R.bias_of(audio, n) - want).max() <= 1e-12 * want.max()


def test_restatement_edges():
    rng = np.random.default_rng(3)
    n = 64
    x = rng.uniform(-0.3, 0.3, 5 * n)
    bias = np.ones(n // 2 + 1)
    # strength 0 is the identity on the samples the transform returns; a huge strength silences everything
    assert np.abs(R.denoise(x, bias, 0.0, n) - x[:R.out_length(len(x), n)]).max() < 1e-15
    y, clamped = R.denoise(x, bias, 1e6, n, return_clamped=True)
    assert clamped == 1.0 and not y.any()
    # continuity at the threshold: the gain has no jump where |X| crosses strength * bias
    X = np.array([[1.0 + 0j, 1e-9 + 1.0j]])
    lo, _ = R.gain(X, [1.0, 1.0], 1.0 - 1e-9)
    hi, _ = R.gain(X, [1.0, 1.0], 1.0 + 1e-9)
    assert np.abs(lo - hi).max() < 1e-8
    with pytest.raises(ValueError, match="33"):
        R.denoise(x[:n // 2], bias, 0.1, n)
    for bad in (100, 32, 2048):
        with pytest.raises(ValueError, match=str(bad)):
            R.denoise(x, bias, 0.1, bad)
    with pytest.raises(ValueError, match="-0.5"):
        R.denoise(x, bias, -0.5, n)


# ---- the Python surface ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy_dir(tmp_path_factory):
    from vosk_tts_amd.toymodel import write_toy_multistream_model

    return write_toy_multistream_model(str(tmp_path_factory.mktemp("ms")), inference={"noise_level": 0.8, "speech_rate": 1.0, "duration_noise_level": 0.8,
                                                                                      "scale": 1.0, "denoiser_strength": 0.00025})


def _feed(T=6, **ext):
    feed = {"input": np.ones((1, 5, T), np.int64), "input_lengths": np.array([T], np.int64), "scales": np.array([0.8, 1.0, 0.8], np.float32),
            "sid": np.array([0], np.int64)}
    feed.update(ext)
    return feed


def test_session_validates_the_denoiser_feeds_before_the_engine(toy_dir, oracle_lib):
    """SttsSession on the CPU oracle: the two feed keys are known names, bad values are refused by name before any work, and a backend
    without the denoiser says so instead of ignoring the flag"""
    from vosk_tts_amd.capi import VitsError
    from vosk_tts_amd.capi_stts import STTS_FLAG_DENOISE, SttsOpts
    from vosk_tts_amd.session_stts import SttsSession

    assert STTS_FLAG_DENOISE == 2 and [f[0] for f in SttsOpts._fields_][-2:] == ["denoiser_strength", "denoiser_filter_length"]
    sess = SttsSession(open(os.path.join(toy_dir, "model.sttsw"), "rb").read(), open(os.path.join(toy_dir, "vocoder.vitsw"), "rb").read(), lib=oracle_lib)
    try:
        calls = []
        real = sess._model.synthesize
        sess._model.synthesize = lambda *a, **kw: calls.append(kw) or real(*a, **kw)
        with pytest.raises(ValueError, match="Invalid input name: vits.denoiser"):
            sess.run(None, _feed(**{"vits.denoiser": 0.1}))
        with pytest.raises(ValueError, match="-0.25"):
            sess.run(None, _feed(**{"vits.denoiser_strength": -0.25}))
        for bad in (100, 2048, 32):
            with pytest.raises(ValueError, match=str(bad)):
                sess.run(None, _feed(**{"vits.denoiser_strength": 0.1, "vits.denoiser_filter_length": bad}))
        with pytest.raises(ValueError, match="needs vits.denoiser_strength"):
            sess.run(None, _feed(**{"vits.denoiser_filter_length": 256}))
        with pytest.raises(ValueError, match="-1"):
            list(sess.run_stream(None, _feed(**{"vits.denoiser_strength": -1.0})))
        with pytest.raises(ValueError, match="2048"):
            sess.run_batch(_feed(**{"vits.denoiser_strength": 0.1, "vits.denoiser_filter_length": 2048}))
        with pytest.raises(VitsError, match="8000"):  # a stream with a denoiser at another rate
            sess.run_stream(None, _feed(**{"vits.denoiser_strength": 0.1, "vits.sample_rate": 8000}))
        assert calls == []  # nothing above reached the model
        # valid values are handed on as the model call's keywords; the CPU oracle has no denoiser and refuses rather than ignore them
        with pytest.raises(VitsError, match="no denoiser"):
            sess.run(None, _feed(**{"vits.denoiser_strength": 0.5, "vits.denoiser_filter_length": 256, "vits.seed": 1}))
        assert calls[-1]["denoiser_strength"] == 0.5 and calls[-1]["denoiser_filter_length"] == 256
        with pytest.raises(VitsError, match="no denoiser"):
            sess.run_batch(_feed(**{"vits.denoiser_strength": 0.5}))
        # without the keys the call is the one of before
        wav, n = sess.run(None, _feed(**{"vits.seed": 1}))
        assert "denoiser_strength" not in calls[-1] and wav.shape == (1, int(n[0]))
        assert not oracle_lib.has_denoise
        with pytest.raises(VitsError, match="no denoiser"):
            oracle_lib.op_denoise(np.zeros((1, 64), np.float32), [64], np.ones(33), 0.1, 64)
    finally:
        sess.close()


class _Session:
    def __init__(self):
        self.feeds = []

    def run(self, names, feed):
        self.feeds.append(feed)
        return [np.zeros((1, 512), np.float32)]

    def run_stream(self, names, feed, chunk_frames=64):
        self.feeds.append(feed)
        yield np.zeros(100, np.float32)


class _Model:
    def __init__(self, config):
        self.onnx = _Session()
        self.dic = {}
        self.tokenizer = None
        self.config = config


def test_synth_takes_the_strength_from_the_argument_or_the_config(toy_dir):
    from vosk_tts_amd.synth import Synth

    cfg = json.load(open(os.path.join(toy_dir, "config.json")))
    assert cfg["model_type"].startswith("multistream") and cfg["inference"]["denoiser_strength"] == 0.00025
    m = _Model(cfg)
    s = Synth(m)
    s.synth_audio("м+ир")  # the config key is the default
    assert m.onnx.feeds[-1]["vits.denoiser_strength"] == 0.00025
    s.synth_audio("м+ир", denoiser_strength=0.5)
    assert m.onnx.feeds[-1]["vits.denoiser_strength"] == 0.5
    list(s.synth_stream("м+ир", denoiser_strength=0.25))
    assert m.onnx.feeds[-1]["vits.denoiser_strength"] == 0.25
    del cfg["inference"]["denoiser_strength"]  # absent = off: the feed of before
    s.synth_audio("м+ир")
    assert set(m.onnx.feeds[-1]) == {"input", "input_lengths", "scales", "sid", "bert", "phone_duration_extra"}


def test_a_vits_voice_refuses_a_strength(tmp_path):
    from vosk_tts_amd.synth import Synth
    from vosk_tts_amd.toymodel import phoneme_id_map

    m = _Model({"phoneme_id_map": phoneme_id_map(), "inference": {}, "model_type": "vits"})
    s = Synth(m)
    s.synth_audio("м+ир")
    with pytest.raises(ValueError, match="0.5.*VITS-family"):
        s.synth_audio("м+ир", denoiser_strength=0.5)
    with pytest.raises(ValueError, match="VITS-family"):
        s.synth("м+ир", str(tmp_path / "x.wav"), denoiser_strength=0.1)
    with pytest.raises(ValueError, match="VITS-family"):
        list(s.synth_stream("м+ир", denoiser_strength=0.1))
    assert len(m.onnx.feeds) == 1


def test_cli_has_a_denoiser_strength_flag():
    from vosk_tts_amd import cli

    ap = cli.build_parser()
    assert ap.parse_args([]).denoiser_strength is None
    assert ap.parse_args(["--denoiser-strength", "0.00025"]).denoiser_strength == 0.00025


def test_header_and_bindings_agree(hip_lib):
    """the three entry points exist in the product library with the argument kinds of include/vits_denoise.h"""
    import ctypes
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(root, "include", "vits_denoise.h")).read(), flags=re.S)
    protos = {m.group(1): [a.strip() for a in m.group(2).split(",")] for m in re.finditer(r"\bint\s+(vits_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)}
    assert set(protos) == {"vits_denoise_bias", "vits_op_denoise", "vits_stream_open_latent_denoise"}
    assert hip_lib.has_denoise
    for name, args in protos.items():
        kinds = ["p" if "*" in a else ("f" if re.match(r"(const\s+)?(float|double)\b", a) else "i") for a in args]
        got = []
        for t in getattr(hip_lib.lib, name).argtypes:
            got.append("f" if t in (ctypes.c_float, ctypes.c_double) else ("p" if t is ctypes.c_void_p or hasattr(t, "contents") else "i"))
        assert got == kinds, (name, got, kinds)
