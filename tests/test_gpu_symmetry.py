"""Canonical frame on the GPU: the two kernels bit-exact against the numpy restatement (tests/symmetry_ref.py), the wrapped policy
exactly equivariant, the env untouched, and PPO on-policy at the rollout and through the real update."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import symmetry_ref as R  # noqa: E402
from oracle import g2048_oracle as npo  # noqa: E402
from src.g2048 import native as nv  # noqa: E402
from src.ppo import LookaheadActionFunction, PPOAgent, PPOTrainer, RolloutBuffer, TorchActionFunction  # noqa: E402
from src.runs import BatchRunner  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 257, 4099)  # partial waves, one wave, partial workgroups, more than one workgroup
GUARD = 0xA5
OPTIM = dict(opt_name="adamw", max_lr=4e-4, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, warmup_steps_ratio=0.025,
             scheduler_names=["constant", "constant"], blacklist_weight_modules=["norm", "embedding"])


@pytest.fixture(scope="module")
def ref():
    """The reference, computed once for the longest input and shared: rows cycle through test_boards()."""
    tb = R.test_boards()
    boards = tb[np.arange(max(SIZES)) % len(tb)]
    rng = np.random.default_rng(11)
    actions = rng.integers(0, 256, len(boards)).astype(np.uint8)  # (the kernel reads the low two bits)
    masks = rng.integers(0, 256, len(boards)).astype(np.uint8)    # (and the low four of the mask)
    canon, frame = R.canon(boards)
    out = dict(boards=boards, actions=actions, masks=masks, canon=canon, frame=frame, canon_actions=R.perm_actions(actions, frame),
               canon_masks=R.perm_mask(masks & 15, frame))
    for v in out.values():
        v.setflags(write=False)
    return out


def _guarded(n, width, dev):
    """A tensor of n rows in front of 64 guard rows; the kernel gets the first n."""
    shape = (n + 64, width) if width else (n + 64,)
    return torch.full(shape, GUARD, dtype=torch.uint8, device=dev)


@pytest.mark.parametrize("B", SIZES)
def test_sym_canon_is_bit_exact(dev, ref, B):
    t = lambda k: torch.from_numpy(ref[k][:B].copy()).to(dev)
    boards, actions, masks = t("boards"), t("actions"), t("masks")
    for with_actions in (False, True):
        for with_masks in (False, True):
            for with_frame in (False, True):
                ob, oa, om, fr = _guarded(B, 16, dev), _guarded(B, 0, dev), _guarded(B, 0, dev), _guarded(B, 0, dev)
                nv.sym_canon(boards, ob[:B], actions=actions if with_actions else None, masks=masks if with_masks else None,
                             frame=fr[:B] if with_frame else None, out_actions=oa[:B] if with_actions else None,
                             out_masks=om[:B] if with_masks else None)
                assert np.array_equal(ob[:B].cpu().numpy(), ref["canon"][:B])
                for used, got, key in ((with_actions, oa, "canon_actions"), (with_masks, om, "canon_masks"), (with_frame, fr, "frame")):
                    if used:
                        assert np.array_equal(got[:B].cpu().numpy(), ref[key][:B]), key
                    else:
                        assert (got == GUARD).all(), key  # an output that was not asked for is not written
                for g in (ob, oa, om, fr):
                    assert (g[B:] == GUARD).all()  # rows at or past B are not touched
                # in place equals out of place
                ib, ia, im = boards.clone(), actions.clone(), masks.clone()
                nv.sym_canon(ib, actions=ia if with_actions else None, masks=im if with_masks else None)
                assert torch.equal(ib, ob[:B])
                assert torch.equal(ia, oa[:B] if with_actions else actions) and torch.equal(im, om[:B] if with_masks else masks)
    assert np.array_equal(boards.cpu().numpy(), ref["boards"][:B])  # the out-of-place input is read only


@pytest.mark.parametrize("B", SIZES)
def test_sym_logits_moves_bit_patterns(dev, B):
    rng = np.random.default_rng(B)
    bits = rng.integers(0, 1 << 32, (B, 4), dtype=np.uint64).astype(np.uint32)  # random patterns: NaN payloads, denormals
    special = np.array([0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x7FC00001, 0xFFFFFFFF, 0x00000001, 0x3F800000], np.uint32)
    flat = bits.reshape(-1)
    flat[: min(len(special), len(flat))] = special[: len(flat)]  # +-inf, -0, +0, NaNs, a denormal, 1.0
    frame = rng.integers(0, 256, B).astype(np.uint8)  # (the kernel reads the low three bits)
    want = R.logits_back(bits, frame & 7).view(np.int32)
    logits = torch.from_numpy(bits.view(np.int32)).to(dev).view(torch.float32)
    fr = torch.from_numpy(frame).to(dev)
    out = torch.full((B + 16, 4), -1.0, dtype=torch.float32, device=dev)
    nv.sym_logits(logits, fr, out[:B])
    assert np.array_equal(out[:B].view(torch.int32).cpu().numpy(), want)
    assert (out[B:] == -1.0).all()
    assert np.array_equal(logits.view(torch.int32).cpu().numpy(), bits.view(np.int32))
    nv.sym_logits(logits, fr)  # in place
    assert torch.equal(logits.view(torch.int32), out[:B].view(torch.int32))


# ---------------------------------------------------------------------------------------------- the wrapped policy
def _distinct_boards(n, seed):
    """Boards whose eight views are pairwise distinct, by rejection: every input of the equivariance check counts."""
    cand = R.random_boards(4 * n, seed=seed)
    cand = cand[R.stabiliser_is_trivial(cand)]
    assert len(cand) >= n
    return cand[:n]


def _perturb(agent):
    with torch.no_grad():
        for p in agent.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.05)  # non-trivial biases / LayerNorm affine
    return agent


def _check_equivariance(fn, dev, n=96):
    S = _distinct_boards(n, seed=7)
    base_l, base_v = (x.clone() for x in fn.policy_fn(torch.from_numpy(S).to(dev), None))
    assert torch.isfinite(base_l).all() and base_l.shape == (n, 4) and base_v.shape == (n,)
    assert (base_l.max(dim=1).values > base_l.min(dim=1).values).all()  # four different logits: a wrong permutation shows
    for h in range(8):
        l, v = fn.policy_fn(torch.from_numpy(R.view(S, h)).to(dev), None)  # row b is still board b: its slot does not move
        idx = torch.from_numpy(R.sigma(h, np.arange(4))).to(dev)
        assert torch.equal(l[:, idx].view(torch.int32), base_l.view(torch.int32)), h  # l[:, sigma_h(a)] == base[:, a], bit for bit
        assert torch.equal(v.view(torch.int32), base_v.view(torch.int32)), h
    return S, base_l


@pytest.mark.parametrize("reduction", ["cls", "mean"])
def test_fused_policy_is_exactly_equivariant(dev, reduction):
    torch.manual_seed(0)
    agent = _perturb(PPOAgent(hidden_dim=512, d_model=256, nhead=8, num_layers=2, dim_feedforward=1024, reduction=reduction))
    fn = TorchActionFunction(agent, use_mask=True, device=dev, amp_dtype=torch.bfloat16, symmetry="canonical")
    assert fn._fused is not None
    S, base = _check_equivariance(fn, dev)
    # what the wrapper is made of: the unchanged forward on the canonical boards, turned back
    canon, frame = R.canon(S)
    inner, _ = fn._policy(torch.from_numpy(canon).to(dev))
    assert np.array_equal(base.cpu().numpy(), R.logits_back(inner.cpu().numpy(), frame))
    # and the network itself is not equivariant: without the mode the same check fails
    plain = TorchActionFunction(agent, use_mask=True, device=dev, amp_dtype=torch.bfloat16, symmetry="none")
    l0, _ = plain.policy_fn(torch.from_numpy(S).to(dev), None)
    l1, _ = plain.policy_fn(torch.from_numpy(R.view(S, 1)).to(dev), None)
    assert not torch.equal(l1[:, torch.from_numpy(R.sigma(1, np.arange(4))).to(dev)], l0)


def test_module_forward_is_exactly_equivariant_and_values_invariant(dev):
    torch.manual_seed(0)
    agent = _perturb(PPOAgent(hidden_dim=32, d_model=32, nhead=4, num_layers=1, dim_feedforward=64, dropout=0.0))
    fn = TorchActionFunction(agent, use_mask=True, device=dev, use_fused=False, symmetry="canonical")
    assert fn._fused is None
    _check_equivariance(fn, dev)
    # the lookahead's value forward: invariant on ALL boards, symmetric ones included (nothing is mapped back)
    la = LookaheadActionFunction(agent, device=dev, use_fused=False, symmetry="canonical")
    tb = R.test_boards()
    n = len(tb) // 8
    rows = tb[:n][:128]  # the hand-made symmetric boards come first
    base = la._values(torch.from_numpy(rows).to(dev)).clone()
    for h in range(8):
        got = la._values(torch.from_numpy(R.view(rows, h)).to(dev))
        assert torch.equal(got.view(torch.int32), base.view(torch.int32)), h
    # q is in the env's frame because the expansion is: it turns with the board on boards without symmetry of their own
    S = torch.from_numpy(_distinct_boards(64, seed=9)).to(dev)
    q0, v0 = la.policy_fn(S)
    q1, v1 = la.policy_fn(torch.from_numpy(R.view(S.cpu().numpy(), 5)).to(dev))
    idx = torch.from_numpy(R.sigma(5, np.arange(4))).to(dev)
    assert torch.allclose(q1[:, idx], q0, rtol=1e-5, atol=1e-5) and torch.allclose(v1, v0, rtol=1e-5, atol=1e-5)


def test_unbatched_call_goes_down_policy_fn(dev):
    torch.manual_seed(0)
    agent = _perturb(PPOAgent(hidden_dim=32, d_model=32, nhead=4, num_layers=1, dim_feedforward=64, dropout=0.0))
    fn = TorchActionFunction(agent, use_mask=True, sample_actions=False, device=dev, symmetry="canonical")
    S = _distinct_boards(8, seed=3)
    legal = npo.legal_mask(S)
    key = np.tile(npo.key(5), (8, 1))
    a0, lp0, v0 = fn(key, npo.observation(S), legal)
    for h in (1, 6):
        Sh = R.view(S, h)
        a, lp, v = fn(key, npo.observation(Sh), npo.legal_mask(Sh))
        assert np.array_equal(a, R.sigma(h, a0)) and np.array_equal(v, v0)  # the greedy move turns with the board
        np.testing.assert_allclose(lp, lp0, rtol=0, atol=1e-6)


# ---------------------------------------------------------------------------------------------- rollout, buffer, update
def _bits(legal):
    return (legal.astype(np.uint8) * np.array([1, 2, 4, 8], np.uint8)).sum(axis=1).astype(np.uint8)


def _small_agent():
    torch.manual_seed(0)
    return _perturb(PPOAgent(hidden_dim=32, d_model=32, nhead=4, num_layers=1, dim_feedforward=64, dropout=0.0))


@pytest.fixture(scope="module")
def rollouts(dev):
    """One 64-env rollout per mode with the same agent, seed and sizes, sampling on; + the buffers made of them."""
    out = {}
    for mode in ("canonical", "none"):
        fn = TorchActionFunction(_small_agent(), use_mask=True, sample_actions=True, device=dev, symmetry=mode)
        traj = BatchRunner(init_seed=3, act_fn=fn, device=dev).collect(64)
        buf = RolloutBuffer(31, 16, 4)
        buf.store_trajectory(traj, 0.99, 0.95, canonical=mode == "canonical")
        out[mode] = (fn, traj, buf.device_data(dev))
    return out


def _env_major(traj, x):
    """[T, B, ...] -> the kept steps env-major, as the compaction orders them (numpy)."""
    x = np.swapaxes(x.cpu().numpy(), 0, 1)
    keep = np.arange(traj.T)[None, :] < traj.ep_len.cpu().numpy()[:, None]
    return x[keep]


def test_env_is_untouched_and_buffer_holds_what_the_network_saw(dev, rollouts):
    fn, traj, data = rollouts["canonical"]
    boards, actions = _env_major(traj, traj.boards), _env_major(traj, traj.actions)
    masks, rewards = _env_major(traj, traj.masks), _env_major(traj, traj.rewards)
    assert len(boards) == int(traj.ep_len.sum()) > 64
    # the env-frame trajectory still obeys the oracle
    assert np.array_equal(masks, _bits(npo.legal_mask(boards)))
    assert ((masks >> actions) & 1).all()
    _, score = npo.move(boards, actions.astype(np.int32))
    assert np.array_equal(rewards, score)
    assert len(np.unique(R.canon(boards)[1])) >= 4  # the boards of a game lie in many frames: the maps below are not the identity
    # the buffer: the reference applied to the env-frame rows, bit for bit; everything else as without the mode
    canon, frame = R.canon(boards)
    assert np.array_equal(data["boards"].cpu().numpy(), canon)
    assert np.array_equal(data["actions"].cpu().numpy(), R.perm_actions(actions, frame))
    assert np.array_equal(data["masks"].cpu().numpy(), R.perm_mask(masks, frame))
    plain = RolloutBuffer(31, 16, 4)
    plain.store_trajectory(traj, 0.99, 0.95)
    pdata = plain.device_data(dev)
    assert set(pdata) == set(data)
    assert np.array_equal(pdata["boards"].cpu().numpy(), boards) and np.array_equal(pdata["actions"].cpu().numpy(), actions)
    for k in data:
        if k not in ("boards", "actions", "masks"):
            assert torch.equal(pdata[k].view(torch.int32) if pdata[k].dtype == torch.float32 else pdata[k],
                               data[k].view(torch.int32) if data[k].dtype == torch.float32 else data[k]), k


def _recomputed_gap(forward, data, actions=None):
    """max |stored log-prob - log-prob of the stored (board, action, mask) under ``forward``| (masked log-softmax in f32, as the
    reference's tail computes it)."""
    logits, _ = forward(data["boards"])
    legal = ((data["masks"][:, None].to(torch.int32) >> torch.arange(4, device=logits.device)) & 1).bool()
    logp = torch.where(legal, logits.float(), torch.full_like(logits, torch.finfo(torch.float32).min)).log_softmax(dim=1)
    a = (data["actions"] if actions is None else actions).to(torch.int64)
    return float((data["log_probs"] - logp.gather(1, a[:, None]).squeeze(1)).abs().max().item())


def test_on_policy_at_the_rollout(dev, rollouts):
    """max |stored - recomputed log-prob| over the buffer.  Measured on an MI355X (64 envs, seed 3, the small fp32 agent):
    d_on = 3.6e-7, d_off = 2.4e-7, and f32-min (3.4e38: an illegal action) when the actions stay in the env's frame."""
    fn_on, traj_on, on = rollouts["canonical"]
    fn_off, _, off = rollouts["none"]
    d_on = _recomputed_gap(fn_on._policy, on)                        # the network's own frame: what the update will compute
    d_off = _recomputed_gap(lambda b: fn_off.policy_fn(b, None), off)  # the same statistic without the mode
    # sensitivity: canonical boards and masks, but the env-frame actions
    env_actions = torch.from_numpy(_env_major(traj_on, traj_on.actions)).to(dev)
    d_wrong = _recomputed_gap(fn_on._policy, on, actions=env_actions)
    print(f"\non-policy at the rollout: d_on = {d_on:.3e}  d_off = {d_off:.3e}  d_without_action_map = {d_wrong:.3e}")
    assert np.isfinite([d_on, d_off, d_wrong]).all()
    assert d_on <= 2 * d_off + 1e-6
    assert d_wrong > 100 * d_off


def _update_once(dev, tmp_path, mode):
    torch.manual_seed(0)
    agent = PPOAgent(hidden_dim=512, d_model=256, nhead=8, num_layers=2, dim_feedforward=1024, dropout=0.0, reduction="cls")
    tr = PPOTrainer(agent, BatchRunner(init_seed=0, device=dev), RolloutBuffer(31, 16, 4), dict(OPTIM), max_steps=1000, device=dev,
                    gamma=0.99, lambda_gae=0.95, use_action_mask=True, mixed_precision="bfloat16", rollout_amp=True,
                    target_kl=0.25, max_samples_per_epoch=2000, log_dir=str(tmp_path / mode), rollout_mode="fixed_horizon",
                    rollout_horizon=16, symmetry=mode)
    assert tr.use_hip_graph and tr.symmetry == mode
    tr.collect_rollouts(16, 1)  # 16 lanes x 16 steps: exactly one minibatch of 256, the captured update's smallest size in test_gpu_ppo
    assert tr.rollout_buffer.buffer_size == 256 and tr.batch_runner.act_fn.symmetry == mode
    m = tr.update_policy(batch_size=256, n_epochs=1)
    assert m["n_updates"] == 1 and m["hip_graph"] and m["symmetry"] == mode
    assert np.isfinite([m["policy_loss"], m["value_loss"], m["entropy_loss"], m["total_loss"], m["kl_divergence"]]).all()
    return tr, m


def test_on_policy_through_the_real_update(dev, tmp_path, caplog):
    tr_on, m_on = _update_once(dev, tmp_path, "canonical")
    tr_off, m_off = _update_once(dev, tmp_path, "none")
    kl_on, kl_off = abs(m_on["kl_divergence"]), abs(m_off["kl_divergence"])
    print(f"\non-policy through the update: |mean(old - new log-prob)| = {kl_on:.3e} (canonical)  {kl_off:.3e} (none)")
    assert kl_on <= 2 * kl_off + 1e-4
    # the stored rows are canonical: canon is idempotent on them
    boards = tr_on.rollout_buffer.device_data(dev)["boards"].cpu().numpy()
    assert np.array_equal(R.canon(boards)[0], boards)
    # a checkpoint keeps the mode; loading it into a trainer of the other mode warns
    path = str(tmp_path / "ck.pt")
    tr_on.save_checkpoint(path)
    assert torch.load(path, weights_only=False)["symmetry"] == "canonical"
    with caplog.at_level(logging.WARNING, logger="src.ppo.ppo_trainer"):
        caplog.clear()
        tr_on.load_checkpoint(path)
        assert not [r for r in caplog.records if "symmetry" in r.getMessage()]
        tr_off.load_checkpoint(path)
        assert [r for r in caplog.records if "symmetry" in r.getMessage() and r.levelno == logging.WARNING]
