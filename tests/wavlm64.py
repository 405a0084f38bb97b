"""float64 numpy restatement of WavLM (transformers.models.wavlm.modeling_wavlm in eval mode: feat_extract_norm "group", post-LN encoder, no conv
bias, exact GELU) and of the reference's WavLMLoss mean (train/losses.py:408-426), from a state_dict of WavLMModel's keys.  What is WavLM's own -
the relative-position bucket, the gate, the biased attention and the L1 mean over all hidden states - is written out; the shared front end
(feature extractor, projection, positional conv) is the plain definition of each layer.  One utterance at a time: [samples] -> states.
tests/test_wavlm_cpu.py holds it against the float64 run of the reference (tests/golden/gen_golden_wavlm.py); the engine is csrc/wavlm.hip.h."""
import math

import numpy as np

_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def layer_norm(x, g, b, eps):
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + eps) * g + b


def conv1d(x, w, stride):
    """x [T, cin], w [cout, cin, k] -> [T', cout], no padding, no bias."""
    k = w.shape[2]
    n = (x.shape[0] - k) // stride + 1
    win = np.stack([x[j : j + stride * (n - 1) + 1 : stride] for j in range(k)], axis=2)  # [n, cin, k]
    return np.einsum("nck,ock->no", win, w)


def bucket(d, num_buckets=320, max_distance=800):
    """_relative_positions_bucket of d = key - query."""
    d = np.asarray(d, np.int64)
    nb = num_buckets // 2
    me = nb // 2
    a = np.abs(d)
    large = me + np.log(np.maximum(a, 1).astype(np.float64) / me) / math.log(max_distance / me) * (nb - me)
    large = np.minimum(large.astype(np.int64), nb - 1)
    return (d > 0) * nb + np.where(a < me, a, large)


def gate(x, w, b, const, heads):
    """x [T, heads * 64] -> gate [T, heads]: Linear(64, 8) per head, summed in two groups of four, sigmoid, a * (b * const - 1) + 2."""
    T = x.shape[0]
    g = x.reshape(T, heads, -1) @ w.T + b  # [T, heads, 8]
    s = 1.0 / (1.0 + np.exp(-g.reshape(T, heads, 2, 4).sum(-1)))
    return s[..., 0] * (s[..., 1] * const.reshape(1, heads) - 1.0) + 2.0


def position_bias(T, embed, num_buckets, max_distance):
    """[heads, T, T]: rel_attn_embed[bucket(j - q)][h]."""
    q = np.arange(T)
    return embed[bucket(q[None, :] - q[:, None], num_buckets, max_distance)].transpose(2, 0, 1)


def biased_attention(q, k, v, gated_bias, heads):
    """softmax(q . k / sqrt(head) + gated_bias[h]) v per head; q, k, v [T, heads * hd], gated_bias [heads, T, T]."""
    T = q.shape[0]
    hd = q.shape[1] // heads
    out = np.empty_like(q)
    for h in range(heads):
        sl = slice(h * hd, (h + 1) * hd)
        s = q[:, sl] @ k[:, sl].T / math.sqrt(hd) + gated_bias[h]
        s = np.exp(s - s.max(-1, keepdims=True))
        out[:, sl] = (s / s.sum(-1, keepdims=True)) @ v[:, sl]
    return out


def forward(sd, arch, wave):
    """wave [samples] -> dict(states=[layers + 1 arrays [T, hidden]], gate0 [T, heads], bias0 [heads, T, T] the gated bias of layer 0)."""
    w = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    eps = arch["layer_norm_eps"]
    heads = arch["num_attention_heads"]
    x = np.asarray(wave, np.float64)[:, None]
    for i, s in enumerate(arch["conv_stride"]):
        p = f"feature_extractor.conv_layers.{i}."
        x = conv1d(x, w[p + "conv.weight"], s)
        if i == 0:  # GroupNorm(groups = channels): per channel over time, biased variance
            m, v = x.mean(0, keepdims=True), x.var(0, keepdims=True)
            x = (x - m) / np.sqrt(v + 1e-5) * w[p + "layer_norm.weight"] + w[p + "layer_norm.bias"]
        x = gelu(x)
    x = layer_norm(x, w["feature_projection.layer_norm.weight"], w["feature_projection.layer_norm.bias"], eps)
    x = x @ w["feature_projection.projection.weight"].T + w["feature_projection.projection.bias"]
    # positional conv: weight norm over dim 2, groups, padding k / 2, the extra last frame of an even kernel dropped
    p = "encoder.pos_conv_embed.conv."
    g, v = w[p + "parametrizations.weight.original0"], w[p + "parametrizations.weight.original1"]
    pw = v * (g / np.sqrt((v * v).sum(axis=(0, 1), keepdims=True)))
    H, ci, K = pw.shape
    G = H // ci
    T = x.shape[0]
    xp = np.concatenate([np.zeros((K // 2, H)), x, np.zeros((K // 2, H))])
    pos = np.empty((T, H))
    for gi in range(G):
        win = np.stack([xp[j : j + T, gi * ci : (gi + 1) * ci] for j in range(K)], axis=2)  # [T, ci, K]
        pos[:, gi * ci : (gi + 1) * ci] = np.einsum("tck,ock->to", win, pw[gi * ci : (gi + 1) * ci])
    x = x + gelu(pos + w[p + "bias"])
    x = layer_norm(x, w["encoder.layer_norm.weight"], w["encoder.layer_norm.bias"], eps)
    states = [x]
    bias = position_bias(T, w["encoder.layers.0.attention.rel_attn_embed.weight"], arch["num_buckets"], arch["max_bucket_distance"])
    out = {}
    for l in range(arch["num_hidden_layers"]):
        p = f"encoder.layers.{l}."
        a = p + "attention."
        gt = gate(x, w[a + "gru_rel_pos_linear.weight"], w[a + "gru_rel_pos_linear.bias"], w[a + "gru_rel_pos_const"], heads)
        gb = gt.T[:, :, None] * bias
        if l == 0:
            out["gate0"], out["bias0"] = gt, gb
        lin = lambda n, t: t @ w[a + n + ".weight"].T + w[a + n + ".bias"]  # noqa: E731
        att = biased_attention(lin("q_proj", x), lin("k_proj", x), lin("v_proj", x), gb, heads)
        x = layer_norm(x + lin("out_proj", att), w[p + "layer_norm.weight"], w[p + "layer_norm.bias"], eps)
        f = gelu(x @ w[p + "feed_forward.intermediate_dense.weight"].T + w[p + "feed_forward.intermediate_dense.bias"])
        f = f @ w[p + "feed_forward.output_dense.weight"].T + w[p + "feed_forward.output_dense.bias"]
        x = layer_norm(x + f, w[p + "final_layer_norm.weight"], w[p + "final_layer_norm.bias"], eps)
        states.append(x)
    out["states"] = states
    return out


def l1_mean(states_x, states_y):
    """F.l1_loss(torch.stack(x states), torch.stack(y states)): the mean absolute difference over states, frames and channels."""
    tot = math.fsum(float(np.abs(a - b).sum()) for a, b in zip(states_x, states_y))
    return tot / sum(a.size for a in states_x)
