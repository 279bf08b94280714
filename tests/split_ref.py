"""Host-side yardsticks of the fp32 rollout forward on split-fp16 products (csrc/g2048_f32split.hip, fused_policy.FusedPolicyF32).

- ``forward``: the PPOAgent forward written out from its state dict in numpy, in float64 or float32, with a pluggable product for
  every Linear (``product(x, w, name) -> x @ w.T``);
- ``split_linear``: the model of a split product (operands taken as f32 values, split terms exact, the sum rounded once to f32);
- ``kernel_products``: the products of the kernels at the scales ``fused_policy.f32_split_scales`` chooses (heads: plain f32);
- ``accept`` / ``gemm_bound``: the acceptance bounds of tests/test_gpu_f32_rollout.py.
"""
import numpy as np

ENC = ("self_attn.in_proj", "self_attn.out_proj", "linear1", "linear2")


def _round_bf16(v):
    """f32 -> nearest-even bfloat16, returned as f32."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def round_fmt(v, fmt, flush=False):
    """f32 values rounded to ``fmt`` ("fp16" | "bf16"), returned as float64; ``flush``: fp16 subnormals become zero."""
    v = np.asarray(v, np.float32)
    if fmt == "bf16":
        return _round_bf16(v).astype(np.float64)
    with np.errstate(over="ignore"):
        r = v.astype(np.float16).astype(np.float64)
    if flush:
        r = np.where(np.abs(r) < 2.0 ** -14, 0.0, r)
    return r


def split_linear(x, w, fmt="fp16", sx=1.0, sw=1.0, flush=False, terms=3):
    """x [T, K] @ w [N, K]^T as a two-way split product: hi = fmt(s v), lo = fmt(s v - hi); hi hi + hi lo + lo hi (+ lo lo for
    ``terms`` = 4) summed exactly, rounded once to f32, unscaled in f32."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    xs, ws = (x * np.float32(sx)).astype(np.float32), (w * np.float32(sw)).astype(np.float32)
    xh = round_fmt(xs, fmt, flush)
    wh = round_fmt(ws, fmt, flush)
    with np.errstate(invalid="ignore"):
        xl = round_fmt((xs - xh).astype(np.float32), fmt, flush)
        wl = round_fmt((ws - wh).astype(np.float32), fmt, flush)
        acc = xh @ wh.T + xh @ wl.T + xl @ wh.T
        if terms == 4:
            acc = acc + xl @ wl.T
    return acc.astype(np.float32) * np.float32(1.0 / (sx * sw))


def layer_norm(x, g, b, eps=1e-5):
    m = x.mean(-1, keepdims=True)
    d = x - m
    v = (d * d).mean(-1, keepdims=True)
    return d / np.sqrt(v + x.dtype.type(eps)) * g + b


def forward(sd, boards, reduction, product=None, dtype=np.float64, nhead=8):
    """-> (features [B, D], logits [B, 4], values [B]) of the PPOAgent whose state dict (name -> ndarray) is ``sd``, every operation
    in ``dtype``; ``product(x2d, w, name)`` computes the Linears (default: ``x @ w.T`` in ``dtype``)."""
    c = lambda k: np.asarray(sd[k]).astype(dtype)
    if product is None:
        product = lambda x, w, name: x @ w.T
    lin = lambda x, name, bias=True: (product(x.reshape(-1, x.shape[-1]), c(name + ("_weight" if name.endswith("in_proj") else ".weight")), name)
                                      .astype(dtype).reshape(*x.shape[:-1], -1) + (c(name + ("_bias" if name.endswith("in_proj") else ".bias")) if bias else 0))
    boards = np.asarray(boards).astype(np.int64)
    B = boards.shape[0]
    emb = c("input_embedding.weight").T
    D = emb.shape[1]
    pe = c("transformer.positional_encoding.pe").reshape(-1, D)
    x = emb[boards] + pe[None]
    x = np.concatenate([np.broadcast_to(c("transformer.cls_token").reshape(1, 1, D), (B, 1, D)), x], axis=1)
    S, hd = x.shape[1], D // nhead
    n_layers = 1 + max(int(k.split(".")[3]) for k in sd if k.startswith("transformer.encoder.layers."))
    for i in range(n_layers):
        p = f"transformer.encoder.layers.{i}."
        h = layer_norm(x, c(p + "norm1.weight"), c(p + "norm1.bias"))
        qkv = lin(h, p + "self_attn.in_proj").reshape(B, S, 3, nhead, hd)
        q, k, v = (qkv[:, :, j].transpose(0, 2, 1, 3) for j in range(3))
        s = (q @ k.transpose(0, 1, 3, 2)) * dtype(1.0 / np.sqrt(hd))
        s = np.exp(s - s.max(-1, keepdims=True))
        a = ((s / s.sum(-1, keepdims=True)) @ v).transpose(0, 2, 1, 3).reshape(B, S, D)
        x = x + lin(a, p + "self_attn.out_proj")
        h = layer_norm(x, c(p + "norm2.weight"), c(p + "norm2.bias"))
        x = x + lin(np.maximum(lin(h, p + "linear1"), 0), p + "linear2")
    feats = x[:, 0] if reduction == "cls" else x[:, 1:].mean(1)
    outs = []
    for head in ("actor", "critic"):
        y = np.maximum(lin(feats, head + ".0"), 0)
        y = np.maximum(lin(y, head + ".2"), 0)
        outs.append(lin(y, head + ".4", bias=False))
    return feats, outs[0], outs[1].reshape(-1)


def state_dict_numpy(agent):
    return {k: v.detach().cpu().numpy() for k, v in agent.state_dict().items()}


def kernel_products(agent, fmt="fp16", flush=False):
    """The product of every Linear as FusedPolicyF32 computes it: the encoder's four per layer as split products at the scales of
    ``fused_policy.f32_split_scales`` (``flush``: the pessimistic reading of the matrix core, fp16 subnormals flushed), the heads
    as plain f32 products."""
    from src.ppo.fused_policy import f32_split_scales

    scales = f32_split_scales(agent)
    keys = {"self_attn.in_proj": ("h1", "wqkv"), "self_attn.out_proj": ("a", "wo"), "linear1": ("h2", "w1"), "linear2": ("f", "w2")}

    def product(x, w, name):
        if not name.startswith("transformer.encoder.layers."):
            return np.asarray(x, np.float32) @ np.asarray(w, np.float32).T
        parts = name.split(".")
        s = scales[int(parts[3])]
        kx, kw = keys[".".join(parts[4:])]
        return split_linear(x, w, fmt, s[kx], s[kw], flush)

    return product


def uniform_products(fmt, sx=1.0, sw=1.0, flush=False):
    """Every Linear (heads included) as the same split product: the rows of the issue's model table."""
    return lambda x, w, name: split_linear(x, w, fmt, sx, sw, flush)


def gemm_bound(x, w):
    """Elementwise bound of the split GEMM against the float64 product: 2^-20 sum_k |x_k w_k| (split residuals and the dropped
    lo lo term <= 3 * 2^-24 per product, f32 accumulation of <= 3072 terms ~ 5 * 2^-24, together 2^-21, margin 2)."""
    return 2.0 ** -20 * (np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(w, np.float64)).T)


def accept(err_native: float, err_f32: float) -> bool:
    """Whole-forward acceptance against float64: at most twice the error of the module's own fp32 forward on the same inputs
    + 2e-6 (the f32 forward's own worst case in the model table)."""
    return err_native <= 2.0 * err_f32 + 2e-6


def rescale_hidden(agent, k: int):
    """Multiply linear1 (weight, bias) of every encoder layer and the first Linear of both heads by 2^k and divide the Linear behind
    each by 2^k: ReLU is positively homogeneous, so the function is unchanged in exact arithmetic while the hidden activations
    move by 2^k.  In place; returns the agent."""
    import torch

    with torch.no_grad():
        f = 2.0 ** k
        for l in agent.transformer.encoder.layers:
            l.linear1.weight.mul_(f)
            l.linear1.bias.mul_(f)
            l.linear2.weight.div_(f)
        for head in (agent.actor, agent.critic):
            head[0].weight.mul_(f)
            head[0].bias.mul_(f)
            head[2].weight.div_(f)
    return agent
