"""Weight container ("VITSW001" blob), hyper-parameters and the build-owned
deterministic synthetic weight generator.

The real vosk-model-tts-ru-0.9-multi weights are not available offline
(SURVEY.md §0.3), so parity and benchmarks run on seeded synthetic weights with
the exact tensor names/shapes of the reference's state_dict after
remove_weight_norm (training/vits2/onnx_export.py:77-80; names enumerated from
SynthesizerTrn, training/vits2/models.py:1503-1630).  The same numpy generator
runs in the build container (where the values are also pushed into the imported
reference via load_state_dict to produce tests/golden/) and on the GPU box.

Blob layout: see include/vits_mi355.h.
"""
import ctypes
import struct
import zlib

import numpy as np

VITS_ABI_VERSION = 1
MAX_UPS = 4
MAX_RESK = 4
MAX_RESD = 4
MAGIC = b"VITSW001"


class HParams(ctypes.Structure):
    """ctypes mirror of `struct vits_hparams` (include/vits_mi355.h)."""

    _fields_ = [
        ("abi_version", ctypes.c_int32),
        ("n_vocab", ctypes.c_int32),
        ("hidden_channels", ctypes.c_int32),
        ("inter_channels", ctypes.c_int32),
        ("filter_channels", ctypes.c_int32),
        ("n_heads", ctypes.c_int32),
        ("n_layers", ctypes.c_int32),
        ("kernel_size", ctypes.c_int32),
        ("window_size", ctypes.c_int32),
        ("gin_channels", ctypes.c_int32),
        ("n_speakers", ctypes.c_int32),
        ("enc_cond_layer", ctypes.c_int32),
        ("dp_filter_channels", ctypes.c_int32),
        ("dp_kernel_size", ctypes.c_int32),
        ("dp_n_flows", ctypes.c_int32),  # 0: the deterministic DurationPredictor (use_sdp false, include/vits_mi355.h)
        ("dp_num_bins", ctypes.c_int32),
        ("dp_dds_layers", ctypes.c_int32),
        ("flow_n_flows", ctypes.c_int32),
        ("flow_wn_layers", ctypes.c_int32),
        ("flow_kernel_size", ctypes.c_int32),
        ("flow_dilation_rate", ctypes.c_int32),
        ("dec_type", ctypes.c_int32),
        ("dec_initial_channel", ctypes.c_int32),
        ("n_ups", ctypes.c_int32),
        ("up_rates", ctypes.c_int32 * MAX_UPS),
        ("up_kernels", ctypes.c_int32 * MAX_UPS),
        ("n_resk", ctypes.c_int32),
        ("res_kernels", ctypes.c_int32 * MAX_RESK),
        ("n_resd", ctypes.c_int32),
        ("res_dilations", (ctypes.c_int32 * MAX_RESD) * MAX_RESK),
        ("subbands", ctypes.c_int32),
        ("istft_n_fft", ctypes.c_int32),
        ("istft_hop", ctypes.c_int32),
        ("pqmf_taps", ctypes.c_int32),
        ("pqmf_cutoff", ctypes.c_float),
        ("pqmf_beta", ctypes.c_float),
        ("dp_tail_bound", ctypes.c_float),
        ("sampling_rate", ctypes.c_int32),
        ("hop_length", ctypes.c_int32),
        ("bert_dim", ctypes.c_int32),
        ("conv_precision", ctypes.c_int32),  # 0 fp32 (default), 1 split-bf16 decoder ResBlock convs at batch size ("bf16x3")
        # 0 pre_conv2 (default), 1 pre_conv, 2 plain ResidualCouplingLayer, 3 reserved (fft, refused), 4 mono_layer_inter_residual,
        # 5 mono_layer_post_residual (include/vits_mi355.h)
        ("flow_type", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 5),
    ]

    def total_upsample(self):
        u = 1
        for i in range(self.n_ups):
            u *= self.up_rates[i]
        return u


class BlobEntry(ctypes.Structure):
    _fields_ = [
        ("name", ctypes.c_char * 96),
        ("ndim", ctypes.c_uint32),
        ("dims", ctypes.c_uint32 * 4),
        ("pad_", ctypes.c_uint32),
        ("offset", ctypes.c_uint64),
        ("nelem", ctypes.c_uint64),
    ]


def default_hparams(n_vocab=62):
    """The in-repo MB-iSTFT-VITS2 config
    (training/vits2/configs/mb_istft_vits2_multi.json:29-72)."""
    hp = HParams()
    hp.abi_version = VITS_ABI_VERSION
    hp.n_vocab = n_vocab
    hp.hidden_channels = 192
    hp.inter_channels = 192
    hp.filter_channels = 768
    hp.n_heads = 2
    hp.n_layers = 6
    hp.kernel_size = 3
    hp.window_size = 4
    hp.gin_channels = 256
    hp.n_speakers = 200
    hp.enc_cond_layer = 2
    hp.dp_filter_channels = 256
    hp.dp_kernel_size = 3
    hp.dp_n_flows = 4
    hp.dp_num_bins = 10
    hp.dp_dds_layers = 3
    hp.flow_n_flows = 4
    hp.flow_wn_layers = 4
    hp.flow_kernel_size = 5
    hp.flow_dilation_rate = 1
    hp.dec_type = 0
    hp.dec_initial_channel = 512
    hp.n_ups = 2
    hp.up_rates[0], hp.up_rates[1] = 4, 4
    hp.up_kernels[0], hp.up_kernels[1] = 16, 16
    hp.n_resk = 3
    for i, k in enumerate((3, 7, 11)):
        hp.res_kernels[i] = k
    hp.n_resd = 3
    for i in range(3):
        for j, d in enumerate((1, 3, 5)):
            hp.res_dilations[i][j] = d
    hp.subbands = 4
    hp.istft_n_fft = 16
    hp.istft_hop = 4
    hp.pqmf_taps = 62
    hp.pqmf_cutoff = 0.15
    hp.pqmf_beta = 9.0
    hp.dp_tail_bound = 5.0
    hp.sampling_rate = 22050
    hp.hop_length = 256
    return hp


def tiny_hparams(n_vocab=20):
    """A scaled-down graph of the same family for fast CPU tests
    (channels stay multiples of 32 so every MFMA tile path is exercised)."""
    hp = default_hparams(n_vocab)
    hp.hidden_channels = 64
    hp.inter_channels = 64
    hp.filter_channels = 128
    hp.n_layers = 3
    hp.gin_channels = 32
    hp.n_speakers = 5
    # dp filter (256), flow depth (4x4) and flow kernel (5) are hard-coded in the
    # reference's SynthesizerTrn (models.py:1609-1625), so the tiny graph keeps them
    # and stays constructible by the reference for golden generation.
    hp.dec_initial_channel = 128
    return hp


def plain_hparams(n_vocab=20):
    """Tiny graph with the plain HiFi-GAN `Generator` decoder (models.py:845-898) and the classic V1
    upsampling [8,8,2,2] / kernels [16,16,4,4] — SURVEY.md §8a row a21."""
    hp = tiny_hparams(n_vocab)
    hp.dec_type = 1
    hp.dec_initial_channel = 512
    hp.n_ups = 4
    for i, (u, k) in enumerate(((8, 16), (8, 16), (2, 4), (2, 4))):
        hp.up_rates[i], hp.up_kernels[i] = u, k
    return hp


def multistream_hparams(n_vocab=62):
    """Default-size graph with the `Multistream_iSTFT_Generator` decoder (models.py:1066-1163, config flag ms_istft_vits):
    the multi-band trunk and geometry, a biased subband_conv_post and a learned 63-tap synthesis filter
    (multistream_conv_post) in place of the fixed PQMF filter."""
    hp = default_hparams(n_vocab)
    hp.dec_type = 2
    return hp


def tiny_multistream_hparams(n_vocab=20):
    hp = tiny_hparams(n_vocab)
    hp.dec_type = 2
    return hp


def istft_hparams(n_vocab=62):
    """Default-size graph with the single-band `iSTFT_Generator` decoder (models.py:901-971, config flag istft_vits):
    conv_post into n_fft + 2 rows, one iSTFT, no sub-bands.  Upsampling [8,8] with n_fft 16 / hop 4 is the original
    iSTFT-VITS geometry that gives 256 samples per frame."""
    hp = default_hparams(n_vocab)
    hp.dec_type = 3
    hp.up_rates[0], hp.up_rates[1] = 8, 8
    hp.subbands = 1
    return hp


def tiny_istft_hparams(n_vocab=20):
    hp = istft_hparams(n_vocab)
    t = tiny_hparams(n_vocab)
    for f in ("hidden_channels", "inter_channels", "filter_channels", "n_layers", "gin_channels", "n_speakers", "dec_initial_channel"):
        setattr(hp, f, getattr(t, f))
    return hp


# The pre_conv2 flow's pre-transformer is attentions.Encoder(hidden, hidden, n_heads=2, ...) whatever the config's n_heads is
# (models.py:352-360; only the text encoder takes n_heads, models.py:307-314); both use the Encoder's default window.
FLOW_N_HEADS = 2


def heads3_hparams(n_vocab=62):
    """Default-size graph with 3 attention heads: the text encoder runs at head dim 64, the pre_conv2 flow keeps 2 heads of 96."""
    hp = default_hparams(n_vocab)
    hp.n_heads = 3
    return hp


def heads4_hparams(n_vocab=62):
    """hidden 128 with 4 attention heads (the most the persistent programs take): the text encoder runs 4 heads of 32, the pre_conv2
    flow 2 heads of 64."""
    hp = default_hparams(n_vocab)
    hp.hidden_channels = 128
    hp.inter_channels = 128
    hp.filter_channels = 512
    hp.n_heads = 4
    return hp


PRE_CONV_HEAD_DIMS = (16, 32, 48, 64, 80, 96)  # head dims the plain (no relative position) attention kernels are built for


def pre_conv_hparams(n_vocab=62):
    """Default-size graph with the `pre_conv` flow (flow_type 1, ResidualCouplingTransformersLayer, models.py:399-483): the
    upstream VITS2 default.  Its pre-transformer runs at inter_channels/2 = 96 channels, 2 heads of 48."""
    hp = default_hparams(n_vocab)
    hp.flow_type = 1
    return hp


def tiny_pre_conv_hparams(n_vocab=20):
    hp = tiny_hparams(n_vocab)
    hp.flow_type = 1
    return hp


def plain_flow_hparams(n_vocab=62):
    """Default-size graph with the VITS-1 coupling layers (flow_type 2, modules.ResidualCouplingLayer, modules.py:298-345)."""
    hp = default_hparams(n_vocab)
    hp.flow_type = 2
    return hp


def tiny_plain_flow_hparams(n_vocab=20):
    hp = tiny_hparams(n_vocab)
    hp.flow_type = 2
    return hp


MONO_FLOW_TYPES = (4, 5)  # mono_layer_inter_residual, mono_layer_post_residual (3 is reserved for the fft flow)


def mono_inter_hparams(n_vocab=62):
    """Default-size graph with the `mono_layer_inter_residual` flow (flow_type 4, models.py:696-714): per flow a plain
    ResidualCouplingLayer at flow.flows.{3f}, a Flip, and a MonoTransformerFlowLayer (models.py:545-627) at flow.flows.{3f+2} whose
    2-layer, 2-head pre-transformer runs on the inter_channels/2 = 96 channels of x0 (head dim 48) and adds x0 back before `post`."""
    hp = default_hparams(n_vocab)
    hp.flow_type = 4
    return hp


def tiny_mono_inter_hparams(n_vocab=20):
    hp = tiny_hparams(n_vocab)
    hp.flow_type = 4
    return hp


def mono_post_hparams(n_vocab=62):
    """Default-size graph with the `mono_layer_post_residual` flow (flow_type 5, models.py:715-734): what SynthesizerTrn builds
    when a config says nothing about flows.  The tensors of flow_type 4; the mono layer halves both halves of z instead of adding
    x0 to the pre-transformer's output (residual_connection=True, models.py:595-608)."""
    hp = default_hparams(n_vocab)
    hp.flow_type = 5
    return hp


def tiny_mono_post_hparams(n_vocab=20):
    hp = tiny_hparams(n_vocab)
    hp.flow_type = 5
    return hp


def deterministic_dp_hparams(n_vocab=62):
    """Default-size graph with the deterministic `DurationPredictor` (use_sdp false, models.py:104-139, 1624-1627):
    conv_1 / norm_1 / conv_2 / norm_2 / proj at dp_filter_channels 256, kernel 3.  dp_n_flows == 0 selects it: the reference
    hard-codes 4 flows for the stochastic predictor (models.py:1625), so a stochastic voice never has 0."""
    hp = default_hparams(n_vocab)
    hp.dp_n_flows = 0
    hp.dp_num_bins = 0
    hp.dp_dds_layers = 0
    return hp


def tiny_deterministic_dp_hparams(n_vocab=20):
    """The tiny graph (with speaker conditioning: dp.cond) with the deterministic duration predictor."""
    hp = tiny_hparams(n_vocab)
    hp.dp_n_flows = 0
    hp.dp_num_bins = 0
    hp.dp_dds_layers = 0
    return hp


def hifigan_v1_vocoder_hparams():
    """Vocoder-only blob (n_vocab = 0): the HiFi-GAN V1 generator bundled with StableTTS
    (training/stabletts/matcha/hifigan/models.py:148-199, config.py v1) that the multistream export wraps as
    `vocoder.decode(mel)` (matcha/onnx/export.py:28-32): 80 mel channels in, ups [8,8,2,2], conv_post WITH bias,
    no speaker conditioning.  Only the decoder stage is available on such a model."""
    hp = default_hparams(0)
    hp.n_vocab = 0
    hp.n_speakers = 0
    hp.gin_channels = 0
    hp.inter_channels = 80
    hp.dec_type = 1
    hp.dec_initial_channel = 512
    hp.n_ups = 4
    for i, (u, k) in enumerate(((8, 16), (8, 16), (2, 4), (2, 4))):
        hp.up_rates[i], hp.up_kernels[i] = u, k
    return hp


def decoder_hparams(dec_type, ups, res_kernels, res_dilations, tail=None, dec_initial_channel=128, inter_channels=64, n_vocab=0,
                    gin_channels=0, n_speakers=0, conv_precision=0):
    """One decoder geometry as an hparams struct.  ups: ((u, Ku), ...); res_kernels: (k, ...); res_dilations: one list for every
    chain, (d, ...), or one list per chain, ((d, ...), ...); tail: (subbands, n_fft, hop, taps) for dec_type 0 / 2, (n_fft, hop) for
    dec_type 3, None for the plain Generator.  hop_length is set to the product.  n_vocab 0 (default): a vocoder-only blob (decoder
    tensors only, no speaker conditioning); n_vocab > 0: the tiny voice (tiny_hparams) around this decoder, gin_channels /
    n_speakers as given (0 keeps the tiny voice's)."""
    hp = tiny_hparams(n_vocab) if n_vocab > 0 else default_hparams(0)
    if n_vocab > 0:
        if gin_channels:
            hp.gin_channels = gin_channels
        if n_speakers:
            hp.n_speakers = n_speakers
    else:
        hp.n_vocab, hp.n_speakers, hp.gin_channels = 0, 0, 0
    hp.inter_channels = inter_channels
    if n_vocab > 0:
        hp.hidden_channels = inter_channels  # the tiny voice keeps hidden == inter
    hp.dec_type = dec_type
    hp.dec_initial_channel = dec_initial_channel
    hp.conv_precision = conv_precision
    hp.n_ups = len(ups)
    for i in range(MAX_UPS):
        hp.up_rates[i], hp.up_kernels[i] = ups[i] if i < len(ups) else (0, 0)
    per_chain = res_dilations if isinstance(res_dilations[0], (tuple, list)) else [res_dilations] * len(res_kernels)
    if len(per_chain) != len(res_kernels) or len({len(d) for d in per_chain}) != 1:
        raise ValueError("res_dilations: one list per ResBlock chain, all of one length")
    hp.n_resk, hp.n_resd = len(res_kernels), len(per_chain[0])
    for j in range(MAX_RESK):
        hp.res_kernels[j] = res_kernels[j] if j < hp.n_resk else 0
        for d in range(MAX_RESD):
            hp.res_dilations[j][d] = per_chain[j][d] if j < hp.n_resk and d < hp.n_resd else 0
    rate = 1
    for u, _ in ups:
        rate *= u
    if dec_type in (0, 2):
        hp.subbands, hp.istft_n_fft, hp.istft_hop, hp.pqmf_taps = tail
        rate *= hp.istft_hop * hp.subbands
    elif dec_type == 3:
        hp.istft_n_fft, hp.istft_hop = tail
        hp.subbands = 1
        rate *= hp.istft_hop
    hp.hop_length = rate
    return hp


# --------------------------------------------------------------------------- #
# tensor inventory
# --------------------------------------------------------------------------- #

def tensor_specs(hp):
    """Ordered [(name, shape, kind, fan_in)] for every tensor on the inference
    path.  kind selects the synthetic init."""
    H, I, F = hp.hidden_channels, hp.inter_channels, hp.filter_channels
    G = hp.gin_channels
    W = 2 * hp.window_size + 1
    specs = []

    def conv(name, co, ci, k, bias=True, gain=1.0):
        specs.append((name + ".weight", (co, ci, k), "w", ci * k, gain))
        if bias:
            specs.append((name + ".bias", (co,), "b", 0, 1.0))

    def ln(name, c):
        specs.append((name + ".gamma", (c,), "gamma", 0, 1.0))
        specs.append((name + ".beta", (c,), "beta", 0, 1.0))

    def encoder(prefix, n_layers, filt, k, C=H, rel=True, nh=hp.n_heads):
        dk = C // nh
        for i in range(n_layers):
            a = f"{prefix}.attn_layers.{i}"
            if rel:
                specs.append((a + ".emb_rel_k", (1, W, dk), "rel", dk, 1.0))
                specs.append((a + ".emb_rel_v", (1, W, dk), "rel", dk, 1.0))
            for n in ("conv_q", "conv_k", "conv_v", "conv_o"):
                conv(f"{a}.{n}", C, C, 1)
        for i in range(n_layers):
            ln(f"{prefix}.norm_layers_1.{i}", C)
        for i in range(n_layers):
            conv(f"{prefix}.ffn_layers.{i}.conv_1", filt, C, k)
            conv(f"{prefix}.ffn_layers.{i}.conv_2", C, filt, k)
        for i in range(n_layers):
            ln(f"{prefix}.norm_layers_2.{i}", C)

    def ddsconv(prefix, c, k, n):
        for i in range(n):
            specs.append((f"{prefix}.convs_sep.{i}.weight", (c, 1, k), "w", k, 1.0))
            specs.append((f"{prefix}.convs_sep.{i}.bias", (c,), "b", 0, 1.0))
        for i in range(n):
            conv(f"{prefix}.convs_1x1.{i}", c, c, 1)
        for i in range(n):
            ln(f"{prefix}.norms_1.{i}", c)
        for i in range(n):
            ln(f"{prefix}.norms_2.{i}", c)

    acoustic = hp.n_vocab > 0  # n_vocab == 0: vocoder-only blob, decoder tensors only
    if acoustic:
        # text encoder (models.py:283-326)
        specs.append(("enc_p.emb.weight", (hp.n_vocab, H), "emb", H, 1.0))
        encoder("enc_p.encoder", hp.n_layers, F, hp.kernel_size)
        if hp.enc_cond_layer >= 0 and G > 0:
            specs.append(("enc_p.encoder.spk_emb_linear.weight", (H, G), "w", G, 1.0))
            specs.append(("enc_p.encoder.spk_emb_linear.bias", (H,), "b", 0, 1.0))
        conv("enc_p.proj", 2 * I, H, 1, gain=0.5)
        if hp.bert_dim > 0:  # BERT-conditioned flavour (vosk_tts/synth.py:88-99): 1x1 projection of the "bert" feed
            conv("enc_p.bert_proj", H, hp.bert_dim, 1, gain=0.5)

    # decoder (models.py:974-1014 / 845-871)
    C0 = hp.dec_initial_channel
    conv("dec.conv_pre", C0, I, 7)
    ch = C0
    for i in range(hp.n_ups):
        # ConvTranspose1d weight is [C_in, C_out, K] (models.py:986-990)
        specs.append((f"dec.ups.{i}.weight", (ch, ch // 2, hp.up_kernels[i]), "w", ch * hp.up_kernels[i] // hp.up_rates[i], 1.0))
        specs.append((f"dec.ups.{i}.bias", (ch // 2,), "b", 0, 1.0))
        ch //= 2
        for j in range(hp.n_resk):
            k = hp.res_kernels[j]
            rb = f"dec.resblocks.{i * hp.n_resk + j}"
            for d in range(hp.n_resd):
                conv(f"{rb}.convs1.{d}", ch, ch, k, gain=0.7)
            for d in range(hp.n_resd):
                conv(f"{rb}.convs2.{d}", ch, ch, k, gain=0.7)
    if hp.dec_type == 0:
        conv("dec.subband_conv_post", hp.subbands * (hp.istft_n_fft + 2), ch, 7, bias=False, gain=0.5)
    elif hp.dec_type == 2:
        # Multistream_iSTFT_Generator: the post conv has a bias (models.py:1095), the synthesis filter is learned (:1107)
        conv("dec.subband_conv_post", hp.subbands * (hp.istft_n_fft + 2), ch, 7, bias=True, gain=0.5)
        specs.append(("dec.multistream_conv_post.weight", (1, hp.subbands, hp.pqmf_taps + 1), "w", hp.pqmf_taps + 1, 1.0))
    elif hp.dec_type == 3:
        conv("dec.conv_post", hp.istft_n_fft + 2, ch, 7, bias=False, gain=0.5)  # iSTFT_Generator (models.py:932), no cond
    else:
        # VITS' Generator: no conv_post bias (models.py:866); StableTTS' HiFi-GAN: bias (hifigan/models.py:176)
        conv("dec.conv_post", 1, ch, 7, bias=not acoustic, gain=0.5)
        if G > 0 and hp.n_speakers > 1:
            conv("dec.cond", C0, G, 1)  # Generator.cond (models.py:869-870)
    if not acoustic:
        return specs

    # flow (models.py:329-483, 630-762, modules.py:298-345); only even indices carry weights.  flow_type 1 (pre_conv): the
    # pre-transformer is a 2-layer, 2-head Encoder on the I/2 channels of x0 with FFN kernel 3 and no relative positions
    # (models.py:417-425); its post_transformer (:436-444) is never run and not part of the export.  flow_type 2: no transformer.
    # flow_type 4 / 5 (mono_layer_*, models.py:696-734): [ResidualCouplingLayer, Flip, MonoTransformerFlowLayer] per flow, so the plain
    # coupling layer sits at index 3f and the mono layer (models.py:545-627: the pre_conv Encoder geometry, then post = Conv1d(I/2, I/2, 1),
    # mean_only, no speaker conditioning) at 3f + 2.  The reference zero-initialises that post; the synthetic one is not zero.
    mono = hp.flow_type in MONO_FLOW_TYPES
    for f in range(hp.flow_n_flows):
        p = f"flow.flows.{(3 if mono else 2) * f}"
        if hp.flow_type == 1:
            encoder(p + ".pre_transformer", 2, I // 2, 3, C=I // 2, rel=False)
        conv(p + ".pre", H, I // 2, 1)
        if hp.flow_type == 0:  # pre_conv2 (models.py:352-360): 2 heads whatever n_heads is, the Encoder's default window
            encoder(p + ".pre_transformer", 1, H, hp.flow_kernel_size, nh=FLOW_N_HEADS)
        for i in range(hp.flow_wn_layers):
            conv(f"{p}.enc.in_layers.{i}", 2 * H, H, hp.flow_kernel_size)
        for i in range(hp.flow_wn_layers):
            rs = 2 * H if i < hp.flow_wn_layers - 1 else H
            conv(f"{p}.enc.res_skip_layers.{i}", rs, H, 1, gain=0.7)
        if G > 0:
            conv(p + ".enc.cond_layer", 2 * H * hp.flow_wn_layers, G, 1)
        conv(p + ".post", I // 2, H, 1, gain=0.5)
        if mono:
            p = f"flow.flows.{3 * f + 2}"
            encoder(p + ".pre_transformer", 2, I // 2, 3, C=I // 2, rel=False, nh=2)
            conv(p + ".post", I // 2, I // 2, 1, gain=0.5)

    D = hp.dp_filter_channels
    if hp.dp_n_flows == 0:
        # deterministic DurationPredictor (models.py:104-139): dp.proj and dp.cond share their names with stochastic-predictor tensors
        # of other shapes.  proj's gain keeps the synthetic logw spread small; its bias is set in synthetic_from_specs.
        conv("dp.conv_1", D, H, hp.dp_kernel_size)
        ln("dp.norm_1", D)
        conv("dp.conv_2", D, D, hp.dp_kernel_size)
        ln("dp.norm_2", D)
        conv("dp.proj", 1, D, 1, gain=0.3)
        if G > 0:
            conv("dp.cond", H, G, 1)
        if hp.n_speakers > 1:
            specs.append(("emb_g.weight", (hp.n_speakers, G), "emb1", G, 1.0))
        return specs
    # stochastic duration predictor, reverse path only (models.py:23-63,93-101):
    # flows[0] ElementwiseAffine, flows[2k+1] ConvFlow for k>=1 (flows[1] is skipped, :94-95)
    specs.append(("dp.flows.0.m", (2, 1), "small", 0, 1.0))
    specs.append(("dp.flows.0.logs", (2, 1), "small", 0, 1.0))
    for k in range(1, hp.dp_n_flows):
        p = f"dp.flows.{2 * k + 1}"
        conv(p + ".pre", D, 1, 1)
        ddsconv(p + ".convs", D, hp.dp_kernel_size, hp.dp_dds_layers)
        conv(p + ".proj", 3 * hp.dp_num_bins - 1, D, 1, gain=4.0)
    conv("dp.pre", D, H, 1)
    conv("dp.proj", D, D, 1)
    ddsconv("dp.convs", D, hp.dp_kernel_size, hp.dp_dds_layers)
    if G > 0:
        conv("dp.cond", D, G, 1)
    if hp.n_speakers > 1:
        specs.append(("emb_g.weight", (hp.n_speakers, G), "emb1", G, 1.0))
    return specs


def _rng(name, seed):
    key = np.array([zlib.crc32(name.encode()), seed & 0xFFFFFFFF], dtype=np.uint64)
    return np.random.Generator(np.random.Philox(key=key))


def make_synthetic_weights(hp, seed=1234, heavy_sigma=0.0):
    """name -> float32 ndarray.  Fan-in scaled uniform so activations stay O(1).

    heavy_sigma > 0: the "heavy-tailed" variant for dynamic-range tests -- every weight matrix gets per-row (first-axis) scales that
    are log-normal with that sigma, normalised to unit mean square (so the average gain of a layer is unchanged while individual
    channels differ by an order of magnitude, as weight-normed trained layers do; tests/golden/full_heavy.npz)."""
    return synthetic_from_specs(tensor_specs(hp), seed, heavy_sigma)


def synthetic_from_specs(specs, seed=1234, heavy_sigma=0.0):
    out = {}
    for name, shape, kind, fan_in, gain in specs:
        r = _rng(name, seed)
        u = r.random(size=shape, dtype=np.float64) * 2.0 - 1.0  # U(-1,1)
        if kind == "w":
            a = gain * np.sqrt(3.0 / max(fan_in, 1))
            t = u * a
            if heavy_sigma > 0 and len(shape) >= 2 and shape[0] > 1:
                g = np.exp(heavy_sigma * _rng(name + ":heavy", seed).standard_normal(shape[0]))
                g /= np.sqrt(np.mean(g * g))
                t = t * g.reshape((-1,) + (1,) * (len(shape) - 1))
        elif kind == "b":
            t = u * 0.05
            if name == "dp.proj.bias" and shape == (1,):
                t = t + 0.9  # deterministic predictor: logw about 0.9 - 1.4 +- 0.3 on encoder outputs, i.e. 2 - 6 frames per token
        elif kind == "gamma":
            t = 1.0 + 0.1 * u
        elif kind == "beta":
            t = 0.05 * u
        elif kind == "rel":
            t = u * np.sqrt(3.0) * fan_in ** -0.5
        elif kind == "emb":
            t = u * np.sqrt(3.0) * fan_in ** -0.5  # std = H^-0.5 as nn.init.normal_ at models.py:304
        elif kind == "emb1":
            t = u * np.sqrt(3.0)
        elif kind == "small":
            t = u * 0.2
            if name == "dp.flows.0.m":
                t = t - 1.0  # logw = (z - m) * exp(-logs): centres free-running durations near e ~ 3 frames/token
        else:
            raise ValueError(kind)
        out[name] = np.ascontiguousarray(t.astype(np.float32))
    return out


# --------------------------------------------------------------------------- #
# blob I/O
# --------------------------------------------------------------------------- #

CONV_MAX_HALO = 64  # (kernel - 1) * dilation of a ResBlock conv (csrc/conv_mfma.hip.h)


def tail_lds_bytes(synth, S, N, hop, taps):
    """LDS of the fused decoder tail for one geometry: the mirror of tail_lds_bytes in csrc/kernels_misc.hip.h"""
    HM = (taps // 2 + S - 1) // S + 1 if synth else 0
    nsub = (64 if synth else 256) + 2 * HM
    FR = (nsub + N) // hop + 2
    return 4 * (2 * S * (N // 2 + 1) * FR + (S * nsub if synth else 0) + (N + 2) * N + (S * (taps + 1) if synth else 0))


def validate_hparams(hp):
    """The checks vits_create makes before it divides by a rate or sizes a buffer from hop_length (engine.hip load_decoder):
    the decoder writes T_y * prod(up_rates) [* istft_hop * subbands] samples per item into buffers of T_y * hop_length."""
    if not isinstance(hp, HParams):
        return
    rate = 1
    if not 1 <= hp.n_ups <= MAX_UPS or not 1 <= hp.n_resk <= 3 or not 1 <= hp.n_resd <= MAX_RESD:
        raise ValueError(f"decoder with n_ups {hp.n_ups} / n_resk {hp.n_resk} / n_resd {hp.n_resd}: 1-{MAX_UPS} upsampling stages, 1-3 ResBlock "
                         f"chains and 1-{MAX_RESD} dilations are served")
    ch = hp.dec_initial_channel
    for i in range(hp.n_ups):
        u, k = hp.up_rates[i], hp.up_kernels[i]
        if u <= 0 or k < u:
            raise ValueError(f"decoder stage {i}: upsample rate {u} / kernel {k} invalid")
        if u > 8 or k % u or (k - u) % 2:
            raise ValueError(f"decoder stage {i}: upsample rate {u} / kernel {k} unsupported (rate <= 8, kernel a multiple of the rate, "
                             "kernel - rate even)")
        if ch <= 0 or ch % 64:
            raise ValueError(f"decoder stage {i}: {ch} input channels (must be a multiple of 64)")
        ch //= 2
        rate *= u
    for j in range(hp.n_resk):
        k = hp.res_kernels[j]
        if k <= 0 or k % 2 == 0:
            raise ValueError(f"resblock kernel {k} invalid (must be odd)")
        for d in range(hp.n_resd):
            if hp.res_dilations[j][d] <= 0 or (k - 1) * hp.res_dilations[j][d] > CONV_MAX_HALO:
                raise ValueError(f"resblock kernel {k} with dilation {hp.res_dilations[j][d]}: a halo of {(k - 1) * hp.res_dilations[j][d]} "
                                 f"columns (1 .. {CONV_MAX_HALO} are served)")
    if hp.dec_type not in (0, 1, 2, 3):
        raise ValueError(f"dec_type {hp.dec_type}: 0 = multi-band iSTFT, 1 = HiFi-GAN Generator, 2 = multi-stream iSTFT, "
                         "3 = single-band iSTFT")
    if hp.dec_type in (0, 2, 3):
        if hp.subbands <= 0 or hp.istft_hop <= 0 or hp.istft_n_fft <= 0 or hp.istft_n_fft % hp.istft_hop:
            raise ValueError("iSTFT / PQMF parameters invalid")
        if hp.dec_type == 2 and (hp.pqmf_taps <= 0 or hp.pqmf_taps % 2):
            raise ValueError(f"multi-stream synthesis filter of {hp.pqmf_taps + 1} taps: the length must be odd")
        if hp.dec_type == 3 and hp.subbands != 1:
            raise ValueError(f"single-band iSTFT decoder with subbands {hp.subbands}: must be 1")
        lds = tail_lds_bytes(hp.dec_type != 3, hp.subbands, hp.istft_n_fft, hp.istft_hop, hp.pqmf_taps)
        if lds > 65536:
            raise ValueError(f"decoder tail geometry (subbands {hp.subbands}, n_fft {hp.istft_n_fft}, hop {hp.istft_hop}, taps {hp.pqmf_taps}) "
                             f"needs {lds} bytes of LDS > 65536")
        rate *= hp.istft_hop * hp.subbands
    if hp.flow_type not in (0, 1, 2) + MONO_FLOW_TYPES:
        raise ValueError(f"flow_type {hp.flow_type}: 0 = pre_conv2, 1 = pre_conv, 2 = plain ResidualCouplingLayer, "
                         "4 = mono_layer_inter_residual, 5 = mono_layer_post_residual (3 is reserved for the fft flow, which is not served)")
    if hp.flow_type == 1 and hp.n_vocab > 0 and not (hp.inter_channels % 4 == 0 and (hp.inter_channels // 4) in PRE_CONV_HEAD_DIMS):
        raise ValueError(f"pre_conv flow with inter_channels {hp.inter_channels}: head dim inter_channels/4 must be one of {PRE_CONV_HEAD_DIMS}")
    if hp.flow_type in MONO_FLOW_TYPES and hp.n_vocab > 0 and not (hp.inter_channels % 4 == 0 and (hp.inter_channels // 4) in PRE_CONV_HEAD_DIMS):
        raise ValueError(f"mono_layer flow with inter_channels {hp.inter_channels}: head dim inter_channels/4 = {hp.inter_channels / 4:g} "
                         f"must be one of {PRE_CONV_HEAD_DIMS}")
    if hp.n_vocab > 0 and hp.dp_n_flows == 0:  # deterministic duration predictor (use_sdp false)
        if hp.dp_dds_layers or hp.dp_num_bins:
            raise ValueError(f"deterministic duration predictor (dp_n_flows 0) with dp_dds_layers {hp.dp_dds_layers} / dp_num_bins "
                             f"{hp.dp_num_bins}: both must be 0")
        if hp.dp_kernel_size <= 0 or hp.dp_kernel_size % 2 == 0:
            raise ValueError(f"deterministic duration predictor kernel {hp.dp_kernel_size}: must be odd")
        if hp.dp_filter_channels <= 0 or hp.dp_filter_channels % 32 or hp.dp_filter_channels > 384:
            raise ValueError(f"deterministic duration predictor of {hp.dp_filter_channels} filter channels: the conv kernels take a "
                             "multiple of 32 up to 384")
    if hp.conv_precision not in (0, 1):
        raise ValueError(f"conv_precision {hp.conv_precision}: 0 = fp32, 1 = split-bf16 decoder ResBlock convs")
    if rate != hp.hop_length:
        raise ValueError(f"decoder produces {rate} samples per frame but hop_length is {hp.hop_length}: upsample_rates / "
                         "gen_istft_hop_size / subbands / hop_length are inconsistent")


def pack_blob(hp, tensors, magic=MAGIC, validate=True):
    """validate=False: pack whatever the struct says (tests hand the library hparams it has to refuse itself)"""
    if validate:
        validate_hparams(hp)
    names = list(tensors.keys())
    n = len(names)
    head = magic + struct.pack("<I", ctypes.sizeof(type(hp))) + bytes(hp) + struct.pack("<I", n)
    table_bytes = n * ctypes.sizeof(BlobEntry)
    off = len(head) + table_bytes
    off = (off + 63) // 64 * 64
    entries = []
    chunks = []
    cur = off
    for nm in names:
        a = np.ascontiguousarray(tensors[nm], dtype=np.float32)
        e = BlobEntry()
        e.name = nm.encode()
        e.ndim = a.ndim
        for i, d in enumerate(a.shape):
            e.dims[i] = d
        e.offset = cur
        e.nelem = a.size
        entries.append(bytes(e))
        b = a.tobytes()
        pad = (-len(b)) % 64
        chunks.append(b + b"\0" * pad)
        cur += len(b) + pad
    table = b"".join(entries)
    pre = head + table
    pre += b"\0" * (off - len(pre))
    return pre + b"".join(chunks)


def unpack_blob(blob):
    return unpack_blob_generic(blob, HParams, MAGIC)


def unpack_blob_generic(blob, hp_type, magic):
    """(hparams struct, {name: ndarray}) of any blob of this container family (VITSW001 / STTSW001 / BERTW001)"""
    if blob[:8] != magic:
        raise ValueError(f"not a {magic.decode()} blob")
    (hb,) = struct.unpack_from("<I", blob, 8)
    if hb != ctypes.sizeof(hp_type):
        raise ValueError("hparams size mismatch")
    hp = hp_type.from_buffer_copy(blob[12:12 + hb])
    (n,) = struct.unpack_from("<I", blob, 12 + hb)
    pos = 16 + hb
    tensors = {}
    es = ctypes.sizeof(BlobEntry)
    for i in range(n):
        e = BlobEntry.from_buffer_copy(blob[pos + i * es: pos + (i + 1) * es])
        shape = tuple(e.dims[j] for j in range(e.ndim))
        a = np.frombuffer(blob, dtype=np.float32, count=e.nelem, offset=e.offset).reshape(shape)
        tensors[e.name.decode()] = a
    return hp, tensors


def synthetic_blob(hp=None, seed=1234, heavy_sigma=0.0):
    hp = hp or default_hparams()
    return pack_blob(hp, make_synthetic_weights(hp, seed, heavy_sigma))


def save_blob(path, hp, tensors):
    with open(path, "wb") as f:
        f.write(pack_blob(hp, tensors))


def load_blob(path):
    with open(path, "rb") as f:
        return f.read()
