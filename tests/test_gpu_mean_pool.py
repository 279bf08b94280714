"""The "mean" reduction on the fused rollout encoder (g2048_policy_encoder_mean, k_encoder_main<MODE_MEAN>): parity with a
plain-PyTorch forward of the same weights, determinism, the heads, path selection and a PPO iteration end to end."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from src.ppo import PPOAgent, PPOTrainer, RolloutBuffer, TorchActionFunction
from src.ppo.fused_policy import FusedPolicy, supports, supports_mean
from src.runs import BatchRunner

pytestmark = pytest.mark.gpu
OPTIM = dict(opt_name="adamw", max_lr=4e-4, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, warmup_steps_ratio=0.025,
             scheduler_names=["constant", "constant"], blacklist_weight_modules=["norm", "embedding"])


def _mean_agent(dev, layers, dropout=0.0):
    return PPOAgent(hidden_dim=512, d_model=256, nhead=8, num_layers=layers, dim_feedforward=1024, dropout=dropout,
                    reduction="mean").to(dev).eval()


@torch.no_grad()
def _torch_features(agent, boards):
    """Mean-pooled features out of plain PyTorch modules only (one-hot Linear, positions, CLS, nn.TransformerEncoder), in
    whatever precision the caller's autocast context gives."""
    t = agent.transformer
    x = agent.input_embedding(F.one_hot(boards.long(), 31).float())
    x = x + t.positional_encoding.flat_table().unsqueeze(0).to(x.dtype)
    x = torch.cat([t.cls_token.expand(x.shape[0], -1, -1).to(x.dtype), x], dim=1)
    return t.encoder(x)[:, 1:].mean(dim=1).float()  # over the 16 board tokens


def _check_parity(fp, agent, boards, what):
    ref32 = _torch_features(agent, boards)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ref16 = _torch_features(agent, boards)
    got = fp.features(boards)
    assert got.shape == ref32.shape and torch.isfinite(got).all(), what
    err, base = (got - ref16).abs().mean().item(), (ref16 - ref32).abs().mean().item()
    assert err < 1.5 * base + 1e-4, (what, err, base)
    assert (got - ref32).abs().max().item() < 0.05 * max(1.0, ref32.abs().max().item()), what
    return got


@pytest.mark.parametrize("layers", [1, 2, 4])
def test_mean_encoder_matches_torch_forward(dev, layers):
    """Kernel parity at partial workgroups (B < 7, B = 13), the pad tokens, a ragged last block (300, 4099)."""
    torch.manual_seed(layers)
    agent = _mean_agent(dev, layers)
    with torch.no_grad():
        for p in agent.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.05)  # non-trivial biases / LayerNorm affine
    fp = FusedPolicy(agent)
    assert fp.mean
    for B in (1, 6, 7, 8, 13, 300, 4099):
        boards = torch.randint(0, 16, (B, 16), dtype=torch.uint8, device=dev)
        _check_parity(fp, agent, boards, (layers, B))


def test_mean_encoder_is_deterministic_and_has_no_split_form(dev):
    torch.manual_seed(0)
    fp = FusedPolicy(_mean_agent(dev, 2))
    boards = torch.randint(0, 16, (4099, 16), dtype=torch.uint8, device=dev)
    one, two = fp.features(boards), fp.features(boards)
    assert torch.equal(one, two)
    assert torch.equal(fp.features(boards, split=False), one)
    with pytest.raises(ValueError):
        fp.features(boards, split=True)


def test_mean_policy_heads_match_autocast_forward(dev):
    torch.manual_seed(1)
    agent = _mean_agent(dev, 2)
    fp = FusedPolicy(agent)
    for B in (5, 300):
        boards = torch.randint(0, 14, (B, 16), dtype=torch.uint8, device=dev)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            l16, v16 = agent(boards)
        l16, v16 = l16.float(), v16.float().flatten()
        logits, values = fp(boards)
        assert logits.shape == (B, 4) and values.shape == (B,)
        assert (logits - l16).abs().max().item() < 0.05 and (values - v16).abs().max().item() < 0.05
        # the heads on g2048_gemm_jobs / g2048_mlp_out_fwd (G2048_OWN_HEADS_MAX, opt-in)
        assert fp.own is not None
        fp.OWN_HEADS_MAX_BOARDS = 16384
        try:
            l_own, v_own = fp(boards)
        finally:
            del fp.OWN_HEADS_MAX_BOARDS  # (back to the class attribute)
        assert (l_own - l16).abs().max().item() < 0.05 and (v_own - v16).abs().max().item() < 0.05


def test_mean_agent_selects_fused_encoder(dev):
    agent = PPOAgent().to(dev)  # the reference's defaults: 4 layers, "mean"
    assert agent.reduction == "mean"
    assert supports_mean(agent)
    assert not supports(agent)  # supports() keeps meaning "cls"
    assert not supports_mean(PPOAgent(reduction="cls").to(dev))
    assert not supports_mean(PPOAgent(d_model=128, nhead=8, num_layers=1, dim_feedforward=256, reduction="mean").to(dev))
    act = TorchActionFunction(agent, device=dev, amp_dtype=torch.bfloat16)
    assert act._fused is not None and act._fused.mean
    assert TorchActionFunction(agent, device=dev, amp_dtype=torch.bfloat16, use_fused=False)._fused is None
    assert TorchActionFunction(agent, device=dev, amp_dtype=None)._fused is None


def test_bf16_rollout_of_mean_agent_uses_fused_encoder_and_trains(dev, tmp_path, monkeypatch):
    """Rollout on the mean kernel, update on the HIP update path: the two compute the same policy (|kl| small), and after the
    optimiser step the rollout's features follow the new weights."""
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    agent = PPOAgent(hidden_dim=512, d_model=256, nhead=8, num_layers=2, dim_feedforward=1024, reduction="mean")
    tr = PPOTrainer(agent, BatchRunner(init_seed=0), RolloutBuffer(31, 16, 4), OPTIM, max_steps=1000, gamma=0.99,
                    lambda_gae=0.95, clip_epsilon=0.2, value_loss_coef=0.5, entropy_coef=0.01, max_grad_norm=0.5,
                    target_kl=0.25, use_action_mask=True, device=dev, mixed_precision="bfloat16", max_samples_per_epoch=2000,
                    shuffle_on_reset=True, rollout_amp=True)
    tr.collect_rollouts(64, 1)
    fp = tr.batch_runner.act_fn._fused
    assert fp is not None and fp.mean
    m = tr.update_policy(batch_size=256, n_epochs=1)
    assert np.isfinite(m["total_loss"]) and abs(m["kl_divergence"]) < 0.05  # rollout and update policies agree
    agent.eval()
    boards = torch.randint(0, 14, (300, 16), dtype=torch.uint8, device=dev)
    fp(boards)  # the rollout's entry: re-packs the updated weights (refresh_if_stale)
    _check_parity(fp, agent, boards, "after update")
