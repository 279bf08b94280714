"""The two-kernel form of g2048_policy_encoder with the CLS row's attention inside k_encoder_main (the default) against the
form that parks the last layer's K / V in the workspace and attends in k_encoder_tail (G2048_ENCODER_KV_WS=1, read by the
library per call): the same operations in the same order, so the features must be equal bit for bit.

Cases: B = 1, 6, 7, 8 (a partial 7-board tile, a full one, one board into the next), 13 (a CLS lane in every wave of the first tile and
none in the last wave of the second), 127, 128, 129, 300 (partial, full and several 128-board tail workgroups); 1, 2 and 4 layers
(1: the last-layer phase starts from the embedding and the prologue's weight fetches); weights from two seeds and a "hot" set whose
last-layer query / key projections are scaled until a score of the CLS query reaches 75 in f32 (checked below), where the max
subtraction decides the result; boards with random exponents 0..15 and boards whose 16 cells are equal.
"""
import math

import pytest
import torch

from src.g2048 import native
from src.ppo import PPOAgent
from src.ppo.fused_policy import FusedPolicy

pytestmark = pytest.mark.gpu

SWITCH = "G2048_ENCODER_KV_WS"
BOARD_COUNTS = (1, 6, 7, 8, 13, 127, 128, 129, 300)
LAYERS = (1, 2, 4)
WEIGHTS = ("seed0", "seed1", "hot")
HOT_SCORE = 75.0


def _boards(B, dev):
    g = torch.Generator(device="cpu").manual_seed(1000 + B)
    rnd = torch.randint(0, 16, (B, 16), dtype=torch.uint8, generator=g)
    same = (torch.arange(B, dtype=torch.uint8) % 16)[:, None].expand(B, 16).contiguous()
    return {"random": rnd.to(dev), "equal": same.to(dev)}


def _cls_scores(agent, boards):
    """max |score| of the CLS query over its board's keys in the last layer, from the f32 modules"""
    t = agent.transformer
    layer = t.encoder.layers[-1]
    with torch.no_grad():
        emb = agent.input_embedding.weight.t().float()                      # [31][256]
        pe = t.positional_encoding.flat_table().float()                     # [16][256]
        cells = boards.long().clamp(max=30)
        x = emb[cells] + pe[None]
        x = torch.cat([t.cls_token.float().reshape(1, 1, 256).expand(x.shape[0], 1, 256), x], dim=1)
        for l in t.encoder.layers[:-1]:
            x = l(x)
        xn = layer.norm1(x)
        w, b = layer.self_attn.in_proj_weight.float(), layer.self_attn.in_proj_bias.float()
        q = (xn[:, :1] @ w[:256].t() + b[:256]).reshape(-1, 1, 8, 32)
        k = (xn @ w[256:512].t() + b[256:512]).reshape(xn.shape[0], -1, 8, 32)
        return (torch.einsum("bqhd,bkhd->bhqk", q, k) / math.sqrt(32.0)).abs().max().item()


_packed = {}


def _policy(layers, kind, dev):
    """one packed agent per (layers, weights), shared by the tests and never changed after packing"""
    key = (layers, kind)
    if key not in _packed:
        torch.manual_seed({"seed0": 0, "seed1": 1, "hot": 2}[kind])
        agent = PPOAgent(hidden_dim=512, d_model=256, nhead=8, num_layers=layers, dim_feedforward=1024, reduction="cls").to(dev).eval()
        with torch.no_grad():
            for p in agent.parameters():
                if p.dim() == 1:
                    p.add_(torch.randn_like(p) * 0.05)  # non-trivial biases / LayerNorm affine
            if kind == "hot":
                probe = _boards(300, dev)["random"]
                attn = agent.transformer.encoder.layers[-1].self_attn
                s = math.sqrt(HOT_SCORE / _cls_scores(agent, probe))  # the layer's input does not depend on s: scores scale by s * s
                attn.in_proj_weight[:512] *= s
                attn.in_proj_bias[:512] *= s
                assert _cls_scores(agent, probe) >= 60.0
        _packed[key] = FusedPolicy(agent)
    return _packed[key]


def _run(fp, boards, ws, poison):
    B = boards.shape[0]
    out = torch.empty((B, 256), dtype=torch.float32, device=boards.device)
    if poison:
        ws.view(torch.float32).fill_(float("nan"))
        out.fill_(float("nan"))
    native.policy_encoder(boards, fp.table, fp.cls, fp.weights, fp.params, fp.n_layers, out, ws)
    return out


def _workspace(B, dev):
    return torch.zeros(native.policy_encoder_workspace_bytes(B), dtype=torch.uint8, device=dev)


def _both(fp, boards, ws, monkeypatch, poison):
    monkeypatch.delenv(SWITCH, raising=False)
    new = _run(fp, boards, ws, poison)
    monkeypatch.setenv(SWITCH, "1")
    old = _run(fp, boards, ws, poison)
    monkeypatch.delenv(SWITCH, raising=False)
    return new, old


@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("layers", LAYERS)
def test_bit_equal_to_kv_workspace_form(dev, monkeypatch, layers, kind):
    fp = _policy(layers, kind, dev)
    for B in BOARD_COUNTS:
        ws = _workspace(B, dev)
        for name, boards in _boards(B, dev).items():
            new, old = _both(fp, boards, ws, monkeypatch, poison=False)
            assert torch.isfinite(new).all(), (layers, kind, B, name)
            assert torch.equal(new, old), (layers, kind, B, name, (new - old).abs().max().item())


@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("layers", LAYERS)
def test_poisoned_workspace_and_features(dev, monkeypatch, layers, kind):
    """NaN in every workspace byte and every output row before each call: a read of the region that is no longer written, or a row
    that is never written, shows as a NaN or as a difference between the forms"""
    fp = _policy(layers, kind, dev)
    for B in BOARD_COUNTS:
        ws = _workspace(B, dev)
        for name, boards in _boards(B, dev).items():
            new, old = _both(fp, boards, ws, monkeypatch, poison=True)
            assert torch.isfinite(new).all() and torch.isfinite(old).all(), (layers, kind, B, name)
            assert torch.equal(new, old), (layers, kind, B, name)


@pytest.mark.parametrize("kind", ("seed0", "seed1"))
@pytest.mark.parametrize("layers", LAYERS)
def test_single_kernel_form_within_its_bound(dev, monkeypatch, layers, kind):
    """against workspace=None (every token through every layer in one kernel): the bound test_fused_encoder_matches_autocast_forward
    holds the two forms to, at that test's scale of weights (the bound was set for those; the hot set belongs to the bit comparisons)"""
    monkeypatch.delenv(SWITCH, raising=False)
    fp = _policy(layers, kind, dev)
    for B in BOARD_COUNTS:
        ws = _workspace(B, dev)
        for name, boards in _boards(B, dev).items():
            two, one = _run(fp, boards, ws, False), _run(fp, boards, None, False)
            assert (one - two).abs().max().item() < 0.02 * max(1.0, one.abs().max().item()), (layers, kind, B, name)


@pytest.mark.parametrize("layers", LAYERS)
def test_two_calls_give_equal_bits(dev, monkeypatch, layers):
    monkeypatch.delenv(SWITCH, raising=False)
    fp = _policy(layers, "seed0", dev)
    for B in BOARD_COUNTS:
        ws = _workspace(B, dev)
        boards = _boards(B, dev)["random"]
        first = _run(fp, boards, ws, True)
        assert torch.equal(first, _run(fp, boards, ws, True)), (layers, B)
