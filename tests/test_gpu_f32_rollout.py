"""The fp32 rollout forward on split-fp16 products (csrc/g2048_f32split.hip, fused_policy.FusedPolicyF32) on the MI355X: the GEMM
alone against float64, the whole forward against the reference's vectors and against float64 at size, the range of the scales,
staleness after an optimiser step, and one lock-step of the rollout engine with the switch on and off."""
import copy
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import split_ref as sr
from src.g2048 import native as nv
from src.ppo import PPOAgent, TorchActionFunction
from src.ppo.fused_policy import FusedPolicyF32, pow2_scale
from src.runs import BatchRunner
from test_host_logic import default_shape_agent

pytestmark = pytest.mark.gpu
REF = np.load(os.path.join(os.path.dirname(__file__), "golden", "torch_reference.npz"))
BITS = [1, 2, 4, 8]
PAD = 64  # guard rows behind every output


def _t(key, dev):
    return torch.from_numpy(REF[key]).to(dev)


# (K, N, epilogue, activation scale): every GEMM of the forward; the activation scales are those of the default-shape agent
GEMMS = [(256, 768, nv.F32SPLIT_BIAS, 2.0 ** 10), (256, 256, nv.F32SPLIT_ADD_LN, 2.0 ** 11), (256, 1024, nv.F32SPLIT_BIAS_RELU, 2.0 ** 10),
         (1024, 256, nv.F32SPLIT_ADD_LN, 2.0 ** 11), (1024, 256, nv.F32SPLIT_ADD, 2.0 ** 11)]


@pytest.mark.parametrize("T", [17, 119, 2048 * 17, 34816 + 5])
@pytest.mark.parametrize("K,N,epi,sx", GEMMS)
def test_split_gemm_against_float64(dev, K, N, epi, sx, T):
    """|y - y64| <= 2^-20 sum_k |x_k w_k| + the f32 roundings of the epilogue's adds (2^-24 relative each, margin 2); the
    LayerNorm output against float64 LayerNorm of the kernel's own pre-norm row, within the worst-case f32 error of a 256-term
    mean and variance (2^-16 relative each).  Rows past T and columns past N keep their NaN guard."""
    g = torch.Generator(device="cpu").manual_seed(1000 * K + N + epi + T)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    x = rnd(T, K)
    if K == 1024:
        x = torch.relu(x)  # linear2 reads ReLU outputs
    w, bias, resid = rnd(N, K) / math.sqrt(K), 0.1 * rnd(N), rnd(T, 256)
    gamma, beta = 1.0 + 0.1 * rnd(256), 0.1 * rnd(256)
    x, w, bias, resid, gamma, beta = (v.to(dev) for v in (x, w, bias, resid, gamma, beta))
    sw = pow2_scale(float(w.abs().max()))
    packed = torch.empty(2 * N * K, dtype=torch.float16, device=dev)
    nv.f32split_pack(w, sw, packed)
    row = epi in (nv.F32SPLIT_ADD_LN, nv.F32SPLIT_ADD)
    ldy = N + 8
    y = torch.full((T + PAD, ldy), float("nan"), device=dev)
    h = torch.full((T + PAD, 256), float("nan"), device=dev) if epi == nv.F32SPLIT_ADD_LN else None
    nv.f32split_gemm(x, packed, bias, y, K, N, epi, sx, sw, resid=resid if row else None, gamma=gamma if h is not None else None,
                     beta=beta if h is not None else None, h=h, eps=1e-5, T=T)
    torch.cuda.synchronize()
    assert torch.isnan(y[T:]).all() and torch.isnan(y[:, N:]).all() and not torch.isnan(y[:T, :N]).any()
    x64, w64 = x.double(), w.double()
    acc64 = x64 @ w64.T
    bound = 2.0 ** -20 * (x64.abs() @ w64.abs().T)
    pre = acc64 + bias.double()
    if epi == nv.F32SPLIT_BIAS_RELU:
        want = torch.relu(pre)
        tol = bound + 2.0 ** -23 * pre.abs()
    elif row:
        want = resid.double() + pre
        tol = bound + 2.0 ** -23 * (pre.abs() + want.abs())
    else:
        want, tol = pre, bound + 2.0 ** -23 * pre.abs()
    err = (y[:T, :N].double() - want).abs()
    lin = F.linear(x, w, bias)
    lin = torch.relu(lin) if epi == nv.F32SPLIT_BIAS_RELU else (resid + lin if row else lin)
    err_lin = (lin.double() - want).abs()
    print(f"K {K} N {N} epilogue {epi} T {T}: worst err / bound split {float((err / tol).max()):.3f}  torch f32 F.linear {float((err_lin / tol).max()):.3f}"
          f"  (max err {float(err.max()):.3e} / {float(err_lin.max()):.3e})")
    assert (err <= tol).all(), float((err / tol).max())
    if h is not None:
        assert torch.isnan(h[T:]).all() and not torch.isnan(h[:T]).any()
        v = y[:T, :256].double()
        mean = v.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((v - mean) ** 2).mean(1, keepdim=True) + 1e-5)
        z = (v - mean) * rstd
        h64 = z * gamma.double() + beta.double()
        tol_h = gamma.double().abs() * 2.0 ** -16 * (v.abs().mean(1, keepdim=True) * rstd + z.abs()) + 2.0 ** -22 * (h64.abs() + beta.double().abs())
        err_h = (h[:T].double() - h64).abs()
        print(f"    LayerNorm epilogue: worst err / bound {float((err_h / tol_h).max()):.3f} (max err {float(err_h.max()):.3e})")
        assert (err_h <= tol_h).all()


def test_whole_forward_on_the_reference_vectors(dev):
    """default/boards through FusedPolicyF32: the tolerances the eager fp32 path is held to (test_default_shape_agent_on_every_device_path)."""
    agent = default_shape_agent(dropout=0.0).to(dev).eval()
    boards, actions, bits = _t("default/boards", dev), _t("default/actions", dev), _t("default/mask_bits", dev)
    masks = (bits.unsqueeze(-1) & torch.tensor(BITS, dtype=torch.uint8, device=dev)) != 0
    fp = FusedPolicyF32(agent)
    feats = fp.features(boards)
    logits, values = fp(boards)
    lp = torch.log_softmax(logits - 1e8 * (1 - masks.float()), dim=-1).gather(1, actions.long().reshape(-1, 1)).reshape(-1)
    for got, key, atol in ((feats, "features", 3e-5), (logits, "logits", 1e-5), (values, "values", 1e-5), (lp, "eval_logp", 1e-5)):
        want = REF[f"default/{key}"].reshape(got.shape)
        print(key, "max |err|", float(np.abs(got.cpu().numpy() - want).max()))
        np.testing.assert_allclose(got.cpu().numpy(), want, atol=atol, rtol=1e-5, err_msg=key)


def _game_boards(dev, n):
    """n boards of random-policy games of the engine, evenly spread from the first move to the last."""
    from src.actions import act_randomly

    traj = BatchRunner(init_seed=3, act_fn=act_randomly, rng_mode="partitionable", device=dev).collect(256)
    valid = torch.arange(traj.T, device=dev)[:, None] < traj.ep_len[None, :].to(dev)
    frames = traj.boards[valid]  # step-major: early game first
    idx = torch.linspace(0, frames.shape[0] - 1, n, device=dev).long()
    return frames[idx].contiguous()


def _against_float64(agent, boards, label):
    """(native, module) worst |logits - f64|, |values - f64| on ``boards``; asserts the whole-forward acceptance."""
    sd = sr.state_dict_numpy(agent)
    b = boards.cpu().numpy()
    f64 = [np.concatenate(p) for p in zip(*[sr.forward(sd, b[i:i + 512], agent.reduction) for i in range(0, len(b), 512)])]
    with torch.no_grad():
        ml, mv = agent(boards, None)
    nl, nvl = FusedPolicyF32(agent)(boards)
    e = lambda got, want: float(np.abs(got.double().cpu().numpy().reshape(want.shape) - want).max())
    out = {}
    for name, n, m, want in (("logits", nl, ml, f64[1]), ("values", nvl, mv, f64[2])):
        en, em = e(n, want), e(m, want)
        out[name] = (en, em)
        print(f"{label} {name}: native {en:.3e}  module fp32 {em:.3e}  ratio {en / max(em, 1e-30):.2f}")
    for name, (en, em) in out.items():
        assert sr.accept(en, em), (label, name, en, em)
    return out


@pytest.mark.parametrize("layers", [1, 4])
@pytest.mark.parametrize("reduction", ["cls", "mean"])
def test_whole_forward_against_float64_at_size(dev, reduction, layers):
    """4 096 game boards: max |logits - f64| and max |values - f64| <= 2 x the module's own fp32 forward's + 2e-6."""
    torch.manual_seed(5)
    agent = PPOAgent(hidden_dim=512, d_model=256, nhead=8, num_layers=layers, dim_feedforward=1024, dropout=0.0, reduction=reduction).to(dev).eval()
    _against_float64(agent, _game_boards(dev, 4096), f"{reduction} x {layers} layers")


@pytest.mark.parametrize("k", [-12, -6, 6, 12])
def test_range_of_the_hidden_activations(dev, k):
    """linear1 * 2^k, linear2 / 2^k (and the heads' first two layers): the scales come from bounds on the weights and follow them,
    so the rescaled agent passes the same acceptance against ITS float64 forward; there is no fallback to count."""
    torch.manual_seed(6)
    agent = PPOAgent(hidden_dim=512, d_model=256, nhead=8, num_layers=4, dim_feedforward=1024, dropout=0.0, reduction="cls").to(dev).eval()
    _against_float64(sr.rescale_hidden(agent, k), _game_boards(dev, 1024), f"k = {k}")


def test_cached_planes_refresh_after_a_flat_optimiser_step(dev, tmp_path, monkeypatch):
    from test_gpu_optim import _trainer

    monkeypatch.chdir(tmp_path)
    torch.manual_seed(9)
    agent = PPOAgent(hidden_dim=512, d_model=256, nhead=8, num_layers=2, dim_feedforward=1024, dropout=0.0, reduction="cls")
    tr = _trainer(dev, agent, tmp_path / "v", use_hip_graph=False, rollout_amp=False, fp32_native=True)
    assert tr._flat_step is not None
    act = TorchActionFunction(agent, use_mask=True, device=dev, fp32_native=True)
    assert isinstance(act._fused, FusedPolicyF32)
    boards = torch.randint(0, 6, (64, 16), dtype=torch.uint8, device=dev)
    masks = torch.full((64,), 15, dtype=torch.uint8, device=dev)
    before, _ = act.policy_fn(boards, masks)
    before = before.clone()
    tr.collect_rollouts(batch_size=64, num_batches=1)
    assert isinstance(tr.batch_runner.act_fn._fused, FusedPolicyF32)  # the trainer passed the switch through
    tr.update_policy(batch_size=256, n_epochs=1)
    after, _ = act.policy_fn(boards, masks)  # the SAME act_fn object: must have re-packed
    fresh, _ = TorchActionFunction(agent, use_mask=True, device=dev, fp32_native=True).policy_fn(boards, masks)
    assert torch.equal(after, fresh) and not torch.equal(after, before)
    with torch.no_grad():
        want, _ = agent(boards, None)
    assert (after - want).abs().max().item() < 1e-5


def test_one_lock_step_of_the_engine_with_and_without_the_switch(dev):
    """2 048 boards, one lock-step, same seed.  Both runs draw with the same Gumbel noise g, so where the actions differ (a with the
    module's logits l, a' with the native logits l') 0 <= (l_a + g_a) - (l_a' + g_a') <= (l_a - l_a') - (l'_a - l'_a') =: D:
    the fp32 Gumbel-top-2 margin is at most D.  "Identical wherever that margin exceeds 1e-4" is therefore D <= 1e-4 on every
    differing board.  Log-probs within 1e-5 where the actions agree."""
    torch.manual_seed(4)
    agent = PPOAgent(hidden_dim=512, d_model=256, nhead=8, num_layers=4, dim_feedforward=1024, dropout=0.0, reduction="cls").to(dev).eval()
    runs = {}
    for native in (False, True):
        fn = TorchActionFunction(agent, use_mask=True, device=dev, fp32_native=native)
        assert (fn._fused is not None) == native
        traj, _ = BatchRunner(init_seed=11, act_fn=fn, rng_mode="partitionable", device=dev).collect_fixed(2048, 1, restart=True)
        logits, _ = fn.policy_fn(traj.boards[0].contiguous(), None)
        runs[native] = (traj.boards[0].clone(), traj.actions[0].long().clone(), traj.log_probs[0].clone(), logits.clone())
    (b0, a0, lp0, l0), (b1, a1, lp1, l1) = runs[False], runs[True]
    assert torch.equal(b0, b1)
    same = a0 == a1
    print("boards with differing actions:", int((~same).sum()), "of", same.numel(), " max |log-prob diff| where equal:",
          float((lp0 - lp1)[same].abs().max()))
    assert (lp0 - lp1)[same].abs().max().item() <= 1e-5
    if (~same).any():
        i = (~same).nonzero().reshape(-1)
        d = (l0[i, a0[i]] - l0[i, a1[i]]) - (l1[i, a0[i]] - l1[i, a1[i]])
        assert (d <= 1e-4).all(), d
