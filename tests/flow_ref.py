"""A float64 statement of the flow reverse of the two mono_layer_* flows (flow_type 4 = mono_layer_inter_residual,
5 = mono_layer_post_residual), the way the reference's modules execute them (models.py: ResidualCouplingTransformersBlock
:696-757, MonoTransformerFlowLayer :545-627; modules.py: ResidualCouplingLayer :298-345, WN :148-176, Flip :270-277;
attentions.py: Encoder :48-65, MultiHeadAttention with window_size=None :165-196, FFN :308-317; commons.py
fused_add_tanh_sigmoid_multiply :100-107), on the synthetic tensor dict of vosk_tts_amd.weights.  The block's list is
[ResidualCouplingLayer_f, Flip, MonoTransformerFlowLayer_f] for each flow f, and reverse walks it backwards: Mono_f, Flip, RCL_f
for f = n_flows-1 .. 0.  Every layer is written on z in the reference's own channel order with an explicit torch.flip: nothing
here knows about folded Flips, reversed reads, stacked gate outputs or a folded WN tail.  It is the independent side of
tests/test_mono_flows*.py.

Each item is computed alone at its own length.  On the frames below an item's length that equals the reference's padded batch:
every conv with a kernel wider than 1 reads a masked input (zeros beyond the length, as the 'same' padding gives an item alone),
attention gives masked keys no weight, and everything else acts on one frame at a time.
"""
import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
MONO_HEADS = 2  # MonoTransformerFlowLayer.pre_transformer: n_heads=2, n_layers=2, kernel_size=3, window_size=None (models.py:562-570)
MONO_LAYERS = 2


def _layer_norm(x, gamma, beta):
    """modules.LayerNorm (modules.py:20-32): over the channels of [1, C, T], eps 1e-5"""
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    return (x - mean) / torch.sqrt(var + 1e-5) * gamma[None, :, None] + beta[None, :, None]


def _attention(x, T, p, n_heads):
    C, n = x.shape[1], x.shape[2]
    dk = C // n_heads
    q = F.conv1d(x, T(p + ".conv_q.weight"), T(p + ".conv_q.bias")).view(n_heads, dk, n)
    k = F.conv1d(x, T(p + ".conv_k.weight"), T(p + ".conv_k.bias")).view(n_heads, dk, n)
    v = F.conv1d(x, T(p + ".conv_v.weight"), T(p + ".conv_v.bias")).view(n_heads, dk, n)
    scores = torch.einsum("hdi,hdj->hij", q / np.sqrt(dk), k)
    out = torch.einsum("hij,hdj->hdi", torch.softmax(scores, dim=-1), v).reshape(1, C, n)
    return F.conv1d(out, T(p + ".conv_o.weight"), T(p + ".conv_o.bias"))


def encoder(x, T, p, n_layers=MONO_LAYERS, n_heads=MONO_HEADS, kernel=3):
    """attentions.Encoder.forward on one item of full length (its mask is all ones)"""
    pad = (kernel - 1) // 2
    for i in range(n_layers):
        y = _attention(x, T, f"{p}.attn_layers.{i}", n_heads)
        x = _layer_norm(x + y, T(f"{p}.norm_layers_1.{i}.gamma"), T(f"{p}.norm_layers_1.{i}.beta"))
        y = F.conv1d(x, T(f"{p}.ffn_layers.{i}.conv_1.weight"), T(f"{p}.ffn_layers.{i}.conv_1.bias"), padding=pad)
        y = F.conv1d(torch.relu(y), T(f"{p}.ffn_layers.{i}.conv_2.weight"), T(f"{p}.ffn_layers.{i}.conv_2.bias"), padding=pad)
        x = _layer_norm(x + y, T(f"{p}.norm_layers_2.{i}.gamma"), T(f"{p}.norm_layers_2.{i}.beta"))
    return x


def wn(x, g, T, p, n_layers, kernel):
    """modules.WN.forward, dilation_rate 1"""
    H = x.shape[1]
    out = torch.zeros_like(x)
    if g is not None:
        g = F.conv1d(g, T(p + ".cond_layer.weight"), T(p + ".cond_layer.bias"))
    for i in range(n_layers):
        a = F.conv1d(x, T(f"{p}.in_layers.{i}.weight"), T(f"{p}.in_layers.{i}.bias"), padding=(kernel - 1) // 2)
        if g is not None:
            a = a + g[:, i * 2 * H:(i + 1) * 2 * H, :]
        acts = torch.tanh(a[:, :H]) * torch.sigmoid(a[:, H:])
        rs = F.conv1d(acts, T(f"{p}.res_skip_layers.{i}.weight"), T(f"{p}.res_skip_layers.{i}.bias"))
        if i < n_layers - 1:
            x = x + rs[:, :H]
            out = out + rs[:, H:]
        else:
            out = out + rs
    return out


def coupling_reverse(z, g, T, p, hp):
    """modules.ResidualCouplingLayer.forward(reverse=True), mean_only"""
    half = z.shape[1] // 2
    x0, x1 = z[:, :half], z[:, half:]
    h = F.conv1d(x0, T(p + ".pre.weight"), T(p + ".pre.bias"))
    h = wn(h, g, T, p + ".enc", hp.flow_wn_layers, hp.flow_kernel_size)
    m = F.conv1d(h, T(p + ".post.weight"), T(p + ".post.bias"))
    return torch.cat([x0, x1 - m], 1)


def mono_reverse(z, T, p, post_residual):
    """MonoTransformerFlowLayer.forward(reverse=True), mean_only (logs = 0)"""
    half = z.shape[1] // 2
    x0, x1 = z[:, :half], z[:, half:]
    if post_residual:  # residual_connection=True (models.py:595-608)
        x0 = x0 / 2
        m = F.conv1d(encoder(x0, T, p + ".pre_transformer"), T(p + ".post.weight"), T(p + ".post.bias"))
        return torch.cat([x0, (x1 - m) / (1 + np.exp(-0.0))], 1)
    h = encoder(x0, T, p + ".pre_transformer") + x0  # (models.py:610-627)
    m = F.conv1d(h, T(p + ".post.weight"), T(p + ".post.bias"))
    return torch.cat([x0, x1 - m], 1)


def flow_reverse(hp, tensors, z_p, y_lengths, sid):
    """z [B, I, Ty] float64 of ResidualCouplingTransformersBlock.forward(reverse=True) for hp.flow_type 4 / 5; frames at or beyond
    an item's length are left 0 (the callers compare valid frames only)."""
    if hp.flow_type not in (4, 5):
        raise ValueError("flow_ref states the mono_layer_* flows (flow_type 4 / 5) only")
    cache = {}

    def T(name):
        if name not in cache:
            cache[name] = torch.from_numpy(np.asarray(tensors[name], np.float64))
        return cache[name]

    z_p = np.asarray(z_p)
    out = np.zeros(z_p.shape, np.float64)
    with torch.no_grad():
        for b, n in enumerate(int(v) for v in y_lengths):
            z = torch.from_numpy(z_p[b:b + 1, :, :n].astype(np.float64))
            g = T("emb_g.weight")[int(sid[b])].view(1, -1, 1) if hp.gin_channels > 0 and hp.n_speakers > 1 else None
            for f in range(hp.flow_n_flows - 1, -1, -1):  # reversed([RCL_0, Flip, Mono_0, RCL_1, Flip, Mono_1, ...])
                z = mono_reverse(z, T, f"flow.flows.{3 * f + 2}", hp.flow_type == 5)
                z = torch.flip(z, [1])
                z = coupling_reverse(z, g, T, f"flow.flows.{3 * f}", hp)
            out[b, :, :n] = z[0].numpy()
    return out
