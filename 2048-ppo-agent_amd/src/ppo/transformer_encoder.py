"""Transformer trunk of the policy (state-dict compatible with the reference src/ppo/transformer_encoder.py).

Parameter/buffer names are the reference's (``positional_encoding.{inv_freq,pe}``, ``cls_token``,
``encoder.layers.N.*`` of ``nn.TransformerEncoder``) so checkpoints interchange; the forward is written
out explicitly (pre-norm layers over fused QKV) so that the update path can run through the HIP kernels bound in
``hip_ops.py`` (attention, add + dropout + LayerNorm, Linear blocks, token embedding) and be captured in a hipGraph;
without a HIP device, gradients or bf16 autocast every step falls back to the PyTorch operator it mirrors.
"""
import math
import os
from typing import NamedTuple, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..env_definitions import BOARD_DIM
from .hip_ops import (Bf16Shadow, ClsLink, FFNLink, HLink, LNPre, _AddLayerNorm, _ClsRows, _AttnCls, _AttnPacked, _EmbedBoards, _ExpandRows, _InProjCls,  # noqa: F401
                      _LinearAddCast, _LinearAddLayerNorm, _LinearReluDropout, _LinearSplitK, _add_norm, _fused_attention_ok, _fused_norm_ok,
                      _linear, _train_bf16, graph_seed_state)

LINEARS = ("in_proj", "out_proj", "linear1", "linear2")  # the four Linears of an encoder layer, in the order of its parameters


def encoder_shadow_spec(num_layers: int, d_model: int):
    """What the update path asks of the encoder's ``Bf16Shadow`` besides the bf16 views: per layer {Linear name: the set of copies of
    its weight}, a copy being one of the shadow's three requests ("transposed", "packed", "packed_t").
    - row-major transposes: linear2 of every layer (the masked input-gradient GEMM) and out_proj of the layers in front of the last
      (out_proj's input gradient through g2048_linear_bf16);
    - the last layer: out_proj, linear1 and linear2 packed both ways (the fused CLS tail, g2048_cls_tail_fwd / _bwd);
    - at d_model 256, the layers in front of the last: packed out_proj and linear2 (the forward operands of g2048_linear_add_ln_fwd)
      and packed transposes of in_proj and linear1 (the input-gradient GEMM fused with the LayerNorm backward,
      g2048_linear_add_ln_bwd) - and, when there is such a layer, the packed transpose of the last layer's in_proj too (the CLS-only
      K/V input gradient runs in the backward of the layer before it)."""
    last = num_layers - 1
    spec = []
    for i in range(num_layers):
        row = {name: set() for name in LINEARS}
        row["linear2"].add("transposed")
        if i < last:
            row["out_proj"].add("transposed")
        else:
            for name in ("out_proj", "linear1", "linear2"):
                row[name] |= {"packed", "packed_t"}
        if d_model == 256 and i < last:
            row["out_proj"].add("packed"), row["linear2"].add("packed")
            row["in_proj"].add("packed_t"), row["linear1"].add("packed_t")
        if d_model == 256 and i == last and last >= 1:
            row["in_proj"].add("packed_t")
        spec.append(row)
    return spec


class LayerWeights(NamedTuple):
    """What one encoder layer reads on the update path (all None elsewhere): the bf16 views of its eight Linear parameters, and
    the derived copies of the weights - ``_t`` a row-major transpose, ``_p`` fragment-packed, ``_pt`` the fragment-packed transpose.
    ``out_p`` / ``l2_p`` / ``l1_pt`` are None in the last layer, whose packed copies belong to the fused CLS tail (``tail_dense`` /
    ``tail_transposed``: {wo, w1, w2}, None in every other layer)."""
    in_w: Optional[torch.Tensor] = None
    in_b: Optional[torch.Tensor] = None
    out_w: Optional[torch.Tensor] = None
    out_b: Optional[torch.Tensor] = None
    l1_w: Optional[torch.Tensor] = None
    l1_b: Optional[torch.Tensor] = None
    l2_w: Optional[torch.Tensor] = None
    l2_b: Optional[torch.Tensor] = None
    l2_t: Optional[torch.Tensor] = None
    out_t: Optional[torch.Tensor] = None
    out_p: Optional[torch.Tensor] = None
    l2_p: Optional[torch.Tensor] = None
    in_pt: Optional[torch.Tensor] = None
    l1_pt: Optional[torch.Tensor] = None
    tail_dense: Optional[dict] = None
    tail_transposed: Optional[dict] = None


class LayerLinks(NamedTuple):
    """The hand-overs between the autograd nodes of neighbouring layers (hip_ops.HLink / ClsLink), seen from one layer: ``h_in`` joins
    the producer of its normalised input with its in_proj, ``h_out`` the same for the next layer; ``cls_in`` / ``cls_out``: the
    CLS-only last layer takes / the layer before it hands over the CLS rows of the residual stream."""
    h_in: Optional[HLink] = None
    h_out: Optional[HLink] = None
    cls_in: Optional[ClsLink] = None
    cls_out: Optional[ClsLink] = None


def get_emb(sin_inp: torch.Tensor) -> torch.Tensor:
    """Interleave sin and cos of ``sin_inp`` along the last axis: [..., n] -> [..., 2n]."""
    return torch.stack((sin_inp.sin(), sin_inp.cos()), dim=-1).flatten(-2, -1)


class PositionalEncoding2D(nn.Module):
    """Fixed 2-D sinusoidal code: the first half of the channels encodes the row, the second the column.

    Buffers: ``inv_freq`` [channels/2] and ``pe`` [1, x, y, 2*channels] with channels = 2*ceil(C/4).
    """

    def __init__(self, x_size, y_size, channels, dropout=0.1, dtype_override=None):
        super().__init__()
        self.org_channels = channels
        self.dtype_override = dtype_override
        self.channels = int(math.ceil(channels / 4) * 2)
        inv_freq = 1.0 / (10000 ** (torch.arange(0, self.channels, 2).float() / self.channels))
        self.register_buffer("inv_freq", inv_freq)
        self.dropout = nn.Dropout(p=dropout)
        ex = get_emb(torch.outer(torch.arange(x_size, dtype=inv_freq.dtype), inv_freq))  # [x, channels]
        ey = get_emb(torch.outer(torch.arange(y_size, dtype=inv_freq.dtype), inv_freq))  # [y, channels]
        pe = torch.zeros((x_size, y_size, 2 * self.channels), dtype=torch.float)
        pe[:, :, : self.channels] = ex[:, None, :]
        pe[:, :, self.channels:] = ey[None, :, :]
        self.register_buffer("pe", pe.unsqueeze(0))

    def flat_table(self) -> torch.Tensor:
        """[x*y, C] table in row-major cell order."""
        return self.pe.reshape(-1, self.org_channels)

    def forward(self, tensor):  # [B, x, y, C]
        return self.dropout(tensor + self.pe[:, : tensor.shape[1], : tensor.shape[2]])

    def forward_flat(self, tensor: torch.Tensor) -> torch.Tensor:  # [B, x*y, C]
        return self.dropout(tensor + self.flat_table().unsqueeze(0))

    def forward_with_inds(self, x: torch.Tensor, inds: torch.Tensor) -> torch.Tensor:  # [B, S, C], [B, S]
        return self.dropout(x + self.flat_table()[inds])


class TransformerEncoder(nn.Module):
    """CLS token + 16 board tokens through ``num_layers`` pre-norm encoder layers; reduce to [B, d_model]."""

    def __init__(self, d_model: int, nhead: int, num_layers: int, dim_feedforward: int, dropout: float = 0.1):
        super().__init__()
        self.d_model, self.nhead, self.num_layers = d_model, nhead, num_layers
        self.dim_feedforward, self.dropout = dim_feedforward, dropout
        self.positional_encoding = PositionalEncoding2D(BOARD_DIM[0], BOARD_DIM[1], channels=d_model, dropout=dropout)
        self.cls_token = nn.Parameter(torch.randn(1, 1, d_model))
        self._shadow = None  # Bf16Shadow of the layers' Linear parameters, built on first use by the update path
        # parameter container with the reference's names; its own forward is not used
        self.encoder = nn.TransformerEncoder(
            nn.TransformerEncoderLayer(d_model=d_model, nhead=nhead, dim_feedforward=dim_feedforward, dropout=dropout,
                                       norm_first=True, batch_first=True),
            num_layers=num_layers, enable_nested_tensor=False)

    def _bf16_weights(self, like: torch.Tensor):
        """Per layer the ``LayerWeights`` of the update path (bf16 shadows of the Linear parameters and the derived copies the fused
        kernels read, ``Bf16Shadow``); everywhere else every field is None (``_linear`` then uses the masters directly)."""
        layers = self.encoder.layers
        if not _train_bf16(like, layers[0].linear1.weight):
            return [LayerWeights()] * len(layers)
        ps, at = [], {}  # the shadow's parameter list; (layer, Linear) -> the positions of its weight and bias in it
        for i, l in enumerate(layers):
            sa = l.self_attn
            for name, w, b in zip(LINEARS, (sa.in_proj_weight, sa.out_proj.weight, l.linear1.weight, l.linear2.weight),
                                  (sa.in_proj_bias, sa.out_proj.bias, l.linear1.bias, l.linear2.bias)):
                at[i, name] = (len(ps), len(ps) + 1)
                ps += [w, b]
        if self._shadow is None:
            spec = encoder_shadow_spec(len(layers), self.d_model)
            self._shadow = Bf16Shadow(ps, **{copy: [at[i, name][0] for i, row in enumerate(spec) for name in LINEARS if copy in row[name]]
                                             for copy in ("transposed", "packed", "packed_t")})
        v, sh = self._shadow(), self._shadow
        out = []
        for i in range(len(layers)):
            (in_w, in_b), (out_w, out_b), (l1_w, l1_b), (l2_w, l2_b) = (at[i, name] for name in LINEARS)
            rec = LayerWeights(v[in_w], v[in_b], v[out_w], v[out_b], v[l1_w], v[l1_b], v[l2_w], v[l2_b],
                               l2_t=sh.tviews[l2_w], out_t=sh.tviews.get(out_w), in_pt=sh.ptviews.get(in_w))
            if i < len(layers) - 1:
                rec = rec._replace(out_p=sh.pviews.get(out_w), l2_p=sh.pviews.get(l2_w), l1_pt=sh.ptviews.get(l1_w))
            else:  # the last layer's packed copies belong to the fused CLS tail (and in_pt to the CLS-only K/V input gradient)
                tail = dict(wo=out_w, w1=l1_w, w2=l2_w)
                rec = rec._replace(tail_dense={k: sh.pviews[j] for k, j in tail.items()},
                                   tail_transposed={k: sh.ptviews[j] for k, j in tail.items()})
            out.append(rec)
        return out

    def _layer(self, layer: nn.TransformerEncoderLayer, x: torch.Tensor, h: torch.Tensor, next_norm, cls_only: bool = False,
               w=LayerWeights(), links=LayerLinks()):
        """One pre-norm encoder layer.  ``h`` = norm1(x), already computed (by the previous layer's tail); returns
        (x_out, next_norm(x_out)) so that every residual add + dropout + LayerNorm is one fused kernel
        (``_add_norm``); ``next_norm`` None: (x_out, None).  With ``cls_only`` only the CLS row of the output is
        produced (keys and values still come from every token): that is all the "cls" reduction reads from the LAST
        layer, and it skips 16/17 of that layer's query/out-projection/FFN work."""
        a, x = self._attention(layer, x, h, cls_only, w, links)
        return self._sublayers(layer, a, x, next_norm, w, links)

    def _attention(self, layer, x, h, cls_only, w, links):
        """in_proj and the attention of one layer on ``h`` = norm1(x) -> (attention output, residual stream); with ``cls_only``
        both hold the CLS row only."""
        B, S, D = x.shape
        H = self.nhead
        p = self.dropout if self.training else 0.0
        attn = layer.self_attn
        if cls_only:
            wq, b = attn.in_proj_weight, attn.in_proj_bias
            if w.in_w is not None and h.dtype == torch.bfloat16:
                q, kv = _InProjCls.apply(h, wq, b, w.in_w, w.in_b, links.h_in, w.in_pt)
            else:
                q = _linear(h[:, :1], wq[:D], b[:D])
                kv = _linear(h, wq[D:], b[D:])
            x = _ClsRows.apply(x, links.cls_in) if links.cls_in is not None else x[:, :1]
            if _fused_attention_ok(kv, S, D // H):
                a = _AttnCls.apply(q, kv, H, p)
            else:
                k, v = kv.view(B, S, 2, H, D // H).unbind(dim=2)
                a = F.scaled_dot_product_attention(q.view(B, 1, H, D // H).transpose(1, 2), k.transpose(1, 2),
                                                   v.transpose(1, 2), dropout_p=p).transpose(1, 2).reshape(B, 1, D)
        else:
            # (links.h_in: the node that produced h runs this Linear's input-gradient GEMM inside its own LayerNorm backward)
            qkv = _linear(h, attn.in_proj_weight, attn.in_proj_bias, w.in_w, w.in_b, h_link=links.h_in, wt_packed=w.in_pt)
            if _fused_attention_ok(qkv, S, D // H):
                a = _AttnPacked.apply(qkv, H, p)
            else:
                q, k, v = qkv.view(B, S, 3, H, D // H).unbind(dim=2)
                a = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
                                                   dropout_p=p).transpose(1, 2).reshape(B, S, D)
        return a, x

    def _cls_tail(self, layer, a, x, w, tail_heads):
        """Update path, CLS-only last layer: everything from out_proj to the heads' outputs as ONE node (g2048_cls_tail_fwd/bwd) when
        its shapes apply; the agent's closure ``tail_heads`` adds the heads' parameters and returns (logits, values).  Else None."""
        if not (w.in_w is not None and a.dtype == torch.bfloat16 and _fused_norm_ok(x, None)
                and layer.linear1.out_features == 1024 and x.shape[-1] == 256):
            return None
        attn, n2 = layer.self_attn, layer.norm2
        return tail_heads(a, x, dict(wo=attn.out_proj.weight, bo=attn.out_proj.bias, ln_g=n2.weight, ln_b=n2.bias,
                                     w1=layer.linear1.weight, b1=layer.linear1.bias, w2=layer.linear2.weight, b2=layer.linear2.bias),
                          w.tail_dense, w.tail_transposed, n2.eps, self.dropout if self.training else 0.0)

    def _sublayers(self, layer, a, x, next_norm, w, links):
        """out_proj, the residual add and the feed-forward block of one layer on the attention output ``a`` -> (x_out,
        next_norm(x_out)); ``next_norm`` None: (x_out, None)."""
        p = self.dropout if self.training else 0.0
        attn = layer.self_attn
        if w.in_w is not None and a.dtype == torch.bfloat16 and _fused_norm_ok(x, None) \
                and layer.linear1.out_features % 8 == 0 and layer.linear1.out_features <= 2048:
            # update path: out_proj + add + LayerNorm, linear1 + ReLU + dropout, linear2 + add + LayerNorm as three ops
            n2 = layer.norm2
            mid = HLink() if w.l1_pt is not None else None  # out_proj's add + LayerNorm <-> linear1's input gradient
            x, h = _LinearAddLayerNorm.apply(a, attn.out_proj.weight, attn.out_proj.bias, w.out_w, w.out_b, x, n2.weight,
                                             n2.bias, n2.eps, p, w.out_t, None, None, mid, w.out_p)
            link = FFNLink(p) if next_norm is not None else None
            f = _LinearReluDropout.apply(h, layer.linear1.weight, layer.linear1.bias, w.l1_w, w.l1_b, p, link, mid, w.l1_pt)
            if next_norm is None:
                if w.l2_w is not None and layer.linear2.bias is not None:
                    # the encoder's output: residual add + dropout + bf16 cast in one launch (the heads read bf16 anyway)
                    return _LinearAddCast.apply(f, layer.linear2.weight, layer.linear2.bias, w.l2_w, w.l2_b, x, p), None
                f = _linear(f, layer.linear2.weight, layer.linear2.bias, w.l2_w, w.l2_b)
                return x + F.dropout(f, p, self.training), None
            return _LinearAddLayerNorm.apply(f, layer.linear2.weight, layer.linear2.bias, w.l2_w, w.l2_b, x, next_norm.weight,
                                             next_norm.bias, next_norm.eps, p, w.l2_t, link, links.cls_out, links.h_out, w.l2_p)
        a = _linear(a, attn.out_proj.weight, attn.out_proj.bias, w.out_w, w.out_b)
        x, h = _add_norm(x, a, layer.norm2, p, self.training)
        f = F.dropout(F.relu(_linear(h, layer.linear1.weight, layer.linear1.bias, w.l1_w, w.l1_b)), p, self.training)
        f = _linear(f, layer.linear2.weight, layer.linear2.bias, w.l2_w, w.l2_b)
        if next_norm is None:
            return x + F.dropout(f, p, self.training), None
        return _add_norm(x, f, next_norm, p, self.training)

    def forward(self, src: torch.Tensor, reduction: str = "mean") -> torch.Tensor:
        """``src`` [B, 16, d_model] token embeddings (no positions yet) -> [B, d_model]."""
        if reduction not in ["mean", "cls"]:
            raise ValueError(f"reduction must be 'mean' or 'cls', got {reduction}")
        x = self.positional_encoding.forward_flat(src)
        x = torch.cat([_ExpandRows.apply(self.cls_token.to(x.dtype), x.shape[0]), x], dim=1)
        return self.encode(x, reduction)[0]

    def embed_boards_ok(self, boards: torch.Tensor, emb_weight: torch.Tensor) -> bool:
        """The update path with packed boards at the reference shape: ``_EmbedBoards`` applies."""
        return (boards.dtype == torch.uint8 and boards.dim() == 2 and boards.shape[1] == 16 and self.d_model == 256
                and tuple(emb_weight.shape) == (256, 31) and _train_bf16(boards, emb_weight))

    def forward_boards(self, boards: torch.Tensor, emb_weight: torch.Tensor, reduction: str = "mean", tail_heads=None):
        """Packed boards u8 [B, 16] through embedding, positions, CLS and the encoder layers -> what ``encode`` returns."""
        pe = self.positional_encoding.flat_table().float().contiguous()
        p = self.positional_encoding.dropout.p if self.training else 0.0
        # (the embedding kernel also normalises its rows for layers[0].norm1: LNPre)
        pre = LNPre(self.encoder.layers[0].norm1) if os.environ.get("G2048_EMBED_LN", "1") != "0" else None
        return self.encode(_EmbedBoards.apply(boards, emb_weight, pe, self.cls_token, p, pre), reduction, tail_heads, pre=pre)

    def encode(self, x: torch.Tensor, reduction: str = "mean", tail_heads=None, pre=None):
        """[B, 17, d_model] tokens (CLS first, positions added) through the encoder layers -> (features [B, d_model], None).
        ``tail_heads(o, x_cls, params, dense, transposed, eps, p) -> (logits, values)``: offered by an agent whose heads can run
        inside the fused CLS tail; when the update path takes it, the result is (None, (logits, values))."""
        if reduction not in ["mean", "cls"]:
            raise ValueError(f"reduction must be 'mean' or 'cls', got {reduction}")
        layers = self.encoder.layers
        last = len(layers) - 1
        ws = self._bf16_weights(x)
        # h_links[i]: joins the node that produces layer i's normalised input with that layer's in_proj (where the fragment-packed
        # transpose of its weight exists): see hip_ops.HLink
        h_links = [HLink() if w.in_pt is not None else None for w in ws] + [None]
        x, h = _add_norm(x, None, layers[0].norm1, 0.0, self.training, h_link=h_links[0], pre=pre)
        # update path with a CLS-only last layer: its CLS-row gradient goes straight into the backward kernel of the layer
        # before it (ClsLink) instead of through a zero-filled [B, 17, 256] tensor
        cls_link = ClsLink() if (reduction == "cls" and last >= 1 and ws[0].in_w is not None) else None
        for i, layer in enumerate(layers):
            cls_only = reduction == "cls" and i == last
            links = LayerLinks(h_in=h_links[i], h_out=h_links[i + 1], cls_in=cls_link if i == last else None,
                               cls_out=cls_link if i == last - 1 else None)
            a, x = self._attention(layer, x, h, cls_only, ws[i], links)
            if cls_only and tail_heads is not None and self.encoder.norm is None:
                heads_out = self._cls_tail(layer, a, x, ws[i], tail_heads)
                if heads_out is not None:
                    return None, heads_out
            x, h = self._sublayers(layer, a, x, layers[i + 1].norm1 if i < last else None, ws[i], links)
        if self.encoder.norm is not None:
            x = self.encoder.norm(x)
        if reduction == "cls":
            # a CLS-only last layer leaves [B, 1, D]: a view (its backward is free) instead of a select (zero-fill + copy)
            return (x.reshape(x.shape[0], x.shape[2]) if x.shape[1] == 1 else x[:, 0, :]), None
        return x[:, 1:, :].mean(dim=1), None
