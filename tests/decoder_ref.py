"""A float64 statement of the four VITS2 decoders, the way the reference's modules execute them (models.py: Generator :845-891,
iSTFT_Generator :901-962, Multiband_iSTFT_Generator :974-1054, Multistream_iSTFT_Generator :1066-1159; modules.ResBlock1
:187-223; stft.OnnxSTFT :181-262; pqmf.PQMF :15-116): conv1d / conv_transpose1d(stride=u, padding=(Ku-u)//2), one ResBlock1 loop
per chain and an explicit sum divided by the number of chains, ReflectionPad1d((1, 0)), the inverse STFT as a transposed conv
with the pseudo-inverse basis, PQMF synthesis as zero-stuffing, a gain of S and a padded conv.  Nothing here knows about
phases, bands, tiles or folded means: it is the independent side of tests/test_decoder_geometry*.py.

Where the reference hard-codes a value the hyper-parameters leave open, the obvious generalisation is taken and noted:
  * ResBlock1 has exactly 3 (convs1, convs2) pairs; here one pair per entry of the chain's dilation list (n_resd 1..4);
  * PQMF() is always built with subbands 4 / taps 62 / cutoff 0.15 / beta 9; here from hp.subbands / pqmf_taps / pqmf_cutoff /
    pqmf_beta (the prototype is only defined for an even `taps`: an odd one raises);
  * the multi-stream synthesis filter is always 63 taps with padding 31; here taps + 1 with padding taps // 2.

`mutate` switches on ONE deliberate error (tests/test_decoder_geometry.py::test_mutations_are_detected proves that the
grid would notice each of them); it never touches the code under test.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

LRELU_SLOPE = 0.1  # modules.py:17
MUTATIONS = ("phase_shift", "mean3", "dil_reversed", "no_reflect", "pqmf_pad")
F64 = torch.float64


def _kaiser(L, beta):
    n = np.arange(L, dtype=np.float64)
    a = (L - 1) / 2.0
    return np.i0(beta * np.sqrt(np.clip(1.0 - ((n - a) / a) ** 2, 0.0, 1.0))) / np.i0(beta)


def pqmf_synthesis_filter(S, taps, cutoff, beta):
    """[S, taps + 1] float64 (pqmf.py:15-43, 64-75)"""
    if taps % 2:
        raise ValueError("the PQMF prototype filter is defined for an even number of taps")
    n = np.arange(taps + 1, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        h = np.sin(np.pi * cutoff * (n - 0.5 * taps)) / (np.pi * (n - 0.5 * taps))
    h[taps // 2] = cutoff
    h = h * _kaiser(taps + 1, beta)
    return np.stack([2 * h * np.cos((2 * k + 1) * (np.pi / (2 * S)) * (n - (taps - 1) / 2) - (-1) ** k * np.pi / 4) for k in range(S)])


def istft_inverse_basis(N, hop):
    """[N + 2, N] float64: pinv(scale * [Re F; Im F]).T times the periodic Hann window (stft.py:191-211)"""
    fb = np.fft.fft(np.eye(N))
    cut = N // 2 + 1
    fb = np.vstack([fb[:cut].real, fb[:cut].imag])
    inv = np.linalg.pinv((N / hop) * fb).T
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)  # scipy get_window('hann', N, fftbins=True)
    return inv * win[None, :]


def istft_inverse(spec, phase, N, hop):
    """OnnxSTFT.inverse (stft.py:246-262): [B, N/2+1, T] x2 -> [B, 1, (T - 1) * hop]"""
    rec = torch.cat([spec * torch.cos(phase), spec * torch.sin(phase)], dim=1)
    basis = torch.from_numpy(istft_inverse_basis(N, hop))[:, None, :]
    y = F.conv_transpose1d(rec, basis, stride=hop, padding=0) * (float(N) / hop)
    y = y[:, :, N // 2:]
    return y[:, :, :-(N // 2)]


def _resblock1(x, T, idx, K, dils):
    for d, dil in enumerate(dils):
        xt = F.leaky_relu(x, LRELU_SLOPE)
        xt = F.conv1d(xt, T(f"dec.resblocks.{idx}.convs1.{d}.weight"), T(f"dec.resblocks.{idx}.convs1.{d}.bias"), dilation=dil,
                      padding=(K * dil - dil) // 2)
        xt = F.leaky_relu(xt, LRELU_SLOPE)
        xt = F.conv1d(xt, T(f"dec.resblocks.{idx}.convs2.{d}.weight"), T(f"dec.resblocks.{idx}.convs2.{d}.bias"), padding=(K - 1) // 2)
        x = xt + x
    return x


def decoder_ref(hp, tensors, z, sid=None, mutate=None):
    """(audio [B, T_y * hop_length], audio_mb [B, S, T_y * hop_length / S] or None) in float64.  z: [B, inter_channels, T_y]."""
    assert mutate is None or mutate in MUTATIONS

    def T(name):
        return torch.from_numpy(np.asarray(tensors[name])).to(F64)

    x = torch.from_numpy(np.asarray(z)).to(F64)
    B = x.shape[0]
    x = F.conv1d(x, T("dec.conv_pre.weight"), T("dec.conv_pre.bias"), padding=3)
    if hp.dec_type == 1 and "dec.cond.weight" in tensors:
        g = T("emb_g.weight")[torch.as_tensor(np.asarray(sid), dtype=torch.long)].unsqueeze(-1)  # [B, G, 1]
        x = x + F.conv1d(g, T("dec.cond.weight"), T("dec.cond.bias"))
    for i in range(hp.n_ups):
        u, Ku = hp.up_rates[i], hp.up_kernels[i]
        x = F.leaky_relu(x, LRELU_SLOPE)
        w = T(f"dec.ups.{i}.weight")
        if mutate == "phase_shift" and i == 0:  # the taps of output phase (u - 1) moved by one input sample
            w = w.clone()
            p = (Ku - u) // 2
            ks = [k for k in range(Ku) if (k - p) % u == u - 1]
            w[:, :, ks] = torch.roll(w[:, :, ks], 1, dims=2)
        x = F.conv_transpose1d(x, w, T(f"dec.ups.{i}.bias"), stride=u, padding=(Ku - u) // 2)
        xs = None
        for j in range(hp.n_resk):
            dils = [hp.res_dilations[j][d] for d in range(hp.n_resd)]
            if mutate == "dil_reversed":
                dils = dils[::-1]
            r = _resblock1(x, T, i * hp.n_resk + j, hp.res_kernels[j], dils)
            xs = r if xs is None else xs + r
        x = xs / (3 if mutate == "mean3" else hp.n_resk)
    x = F.leaky_relu(x)  # default slope 0.01
    if hp.dec_type == 1:
        b = T("dec.conv_post.bias") if "dec.conv_post.bias" in tensors else None
        return torch.tanh(F.conv1d(x, T("dec.conv_post.weight"), b, padding=3))[:, 0].numpy(), None

    if x.shape[-1] < 2:
        raise ValueError("ReflectionPad1d((1, 0)) needs at least two columns")
    if mutate != "no_reflect":
        x = torch.cat([x[:, :, 1:2], x], dim=2)  # ReflectionPad1d((1, 0))
    else:
        x = torch.cat([torch.zeros_like(x[:, :, :1]), x], dim=2)
    N, hop, S = hp.istft_n_fft, hp.istft_hop, hp.subbands
    cut = N // 2 + 1
    if hp.dec_type == 3:
        x = F.conv1d(x, T("dec.conv_post.weight"), None, padding=3)
        y = istft_inverse(torch.exp(x[:, :cut]), math.pi * torch.sin(x[:, cut:]), N, hop)
        return y[:, 0].numpy(), None
    b = T("dec.subband_conv_post.bias") if hp.dec_type == 2 else None
    x = F.conv1d(x, T("dec.subband_conv_post.weight"), b, padding=3)
    x = x.reshape(B, S, x.shape[1] // S, x.shape[-1])
    spec = torch.exp(x[:, :, :cut, :])
    phase = math.pi * torch.sin(x[:, :, cut:, :])
    mb = istft_inverse(spec.reshape(B * S, cut, -1), phase.reshape(B * S, cut, -1), N, hop).reshape(B, S, -1)
    updown = torch.zeros((S, S, S), dtype=F64)
    for k in range(S):
        updown[k, k, 0] = 1.0
    y = F.conv_transpose1d(mb, updown * S, stride=S)
    taps = hp.pqmf_taps
    if hp.dec_type == 0:
        filt = torch.from_numpy(pqmf_synthesis_filter(S, taps, float(hp.pqmf_cutoff), float(hp.pqmf_beta)))[None]
    else:
        filt = T("dec.multistream_conv_post.weight")
    pad = taps // 2
    if mutate == "pqmf_pad":
        y = F.pad(y, (pad + 1, pad - 1))
    else:
        y = F.pad(y, (pad, pad))
    return F.conv1d(y, filt)[:, 0].numpy(), mb.numpy()


def receptive_field(hp, tensors, T_y=None, thresh=0.0, seed=5):
    """The decoder's true one-sided reach in latent frames, measured on the restatement: perturb one frame of z in the middle of a
    dense input and see how far (left, right) the waveform changes by more than `thresh` of its scale -> (left, right) frames,
    rounded up.  thresh 0 (default) gives the structural field (every tap counts; the synthetic weights have no zero taps): float64
    samples outside it are bit-identical in the two runs."""
    rng = np.random.default_rng(seed)
    hop = hp.hop_length
    T_y = T_y or 161
    c = T_y // 2
    z = rng.standard_normal((1, hp.inter_channels, T_y))
    z2 = z.copy()
    z2[:, :, c] += 1.0
    sid = [0] if "dec.cond.weight" in tensors else None
    a, _ = decoder_ref(hp, tensors, z, sid=sid)
    b, _ = decoder_ref(hp, tensors, z2, sid=sid)
    d = np.abs(a - b)[0] > thresh * np.abs(a).max()
    idx = np.nonzero(d)[0]
    assert idx.size, "the perturbation did not reach the waveform"
    left = -(-(c * hop - int(idx[0])) // hop)
    right = -(-(int(idx[-1]) + 1 - (c + 1) * hop) // hop)
    assert 0 < idx[0] // hop and idx[-1] // hop < T_y - 1, "the field reaches the edge of the probe: use a longer T_y"
    return max(left, 0), max(right, 0)
