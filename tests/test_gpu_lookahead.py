"""One-ply expectimax on the device: the three lookahead kernels against the numpy restatement (tests/lookahead_ref.py),
LookaheadActionFunction against the agent's own value forward, action choice through the engine, and "off means off"."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

import lookahead_ref as R  # noqa: E402
from oracle import g2048_oracle as npo  # noqa: E402
from src.g2048 import native as nv  # noqa: E402
from src.ppo import LookaheadActionFunction, PPOAgent, TorchActionFunction  # noqa: E402
from src.ppo.fused_policy import FusedPolicy  # noqa: E402
from src.runs import BatchRunner, evaluate_agent  # noqa: E402
from src.runs.evaluate import evaluate_max_tile  # noqa: E402
from weights_recipe import fill_state_dict, sample_boards  # noqa: E402

pytestmark = pytest.mark.gpu
GAMMA = 0.99


@pytest.fixture(scope="module")
def case():
    """>= 20 000 boards (oracle rollouts, uniform tiles, hand-made edges) and their numpy expansion."""
    boards = R.kernel_test_boards()
    assert len(boards) >= 20000
    after, reward, nchild = R.expand(boards)
    children, terminal, offset = R.children(after, nchild)
    return dict(boards=boards, after=after, reward=reward, nchild=nchild, children=children, terminal=terminal, offset=offset)


def _dev_expand(boards_np, dev):
    B = len(boards_np)
    boards = torch.from_numpy(boards_np).to(dev)
    after = torch.full((B, 4, 16), 0xEE, dtype=torch.uint8, device=dev)
    reward = torch.full((B, 4), -7.0, dtype=torch.float32, device=dev)
    nchild = torch.full((B, 4), -7, dtype=torch.int32, device=dev)
    nv.lookahead_expand(boards, after, reward, nchild)
    return after, reward, nchild


def test_expand_equals_numpy_bit_for_bit(dev, case):
    after, reward, nchild = _dev_expand(case["boards"], dev)
    assert np.array_equal(nchild.cpu().numpy(), case["nchild"])
    assert np.array_equal(after.cpu().numpy(), case["after"])
    assert np.array_equal(reward.cpu().numpy().view(np.uint32), case["reward"].view(np.uint32))  # integers in f32
    # a legal move leaves an empty cell, so nchild > 0 is exactly the engine's legal mask
    assert np.array_equal(case["nchild"] > 0, npo.legal_mask(case["boards"]))


def test_children_equal_numpy_enumeration_and_leave_the_slack_alone(dev, case):
    N = len(case["children"])
    assert N == int(case["nchild"].sum()) and case["nchild"].max() <= 30
    to = lambda k: torch.from_numpy(case[k]).to(dev)
    after, nchild = to("after"), to("nchild")
    incl = torch.cumsum(nchild.view(-1), 0, dtype=torch.int32)
    offset = (incl - nchild.view(-1)).view(-1, 4)
    assert int(incl[-1].item()) == N and np.array_equal(offset.cpu().numpy(), case["offset"])
    slack = 4099
    children = torch.full((N + slack, 16), 0xA5, dtype=torch.uint8, device=dev)
    terminal = torch.full((N + slack,), 0xA5, dtype=torch.uint8, device=dev)
    nv.lookahead_children(after, nchild, offset, N, children, terminal)
    assert np.array_equal(children[:N].cpu().numpy(), case["children"])
    assert np.array_equal(terminal[:N].cpu().numpy(), case["terminal"])
    assert (children[N:] == 0xA5).all() and (terminal[N:] == 0xA5).all()
    assert 0 < case["terminal"].sum() < N  # both kinds occur in the inputs
    # N = 0 (nothing but terminal boards) launches nothing and fails nothing
    z = torch.zeros((3, 4), dtype=torch.int32, device=dev)
    nv.lookahead_children(after[:3].contiguous(), z, z, 0, children[:0], terminal[:0])
    assert (children[:1] == torch.from_numpy(case["children"][:1]).to(dev)).all()


def _dev_reduce(case, values_np, dev, gamma=GAMMA):
    to = lambda k: torch.from_numpy(case[k]).to(dev)
    q = torch.full(case["nchild"].shape, 123.0, dtype=torch.float32, device=dev)
    nv.lookahead_reduce(to("reward"), to("nchild"), to("offset"), torch.from_numpy(values_np).to(dev), to("terminal"), gamma,
                        len(values_np), q)
    return q.cpu().numpy()


@pytest.mark.parametrize("scale", [1.0, 100.0])
def test_reduce_within_the_derived_bound(dev, case, scale):
    """|q - q64| <= 64 * 2^-24 * S per output (63 rounded f32 operations on partial results no larger than S, the sum of
    magnitudes); exactly 0 where nchild == 0; terminal children contribute exactly nothing."""
    N = len(case["children"])
    values = np.random.default_rng(int(scale)).normal(0.0, scale, N).astype(np.float32)
    args = (case["reward"], case["nchild"], case["offset"], values, case["terminal"], GAMMA)
    q = _dev_reduce(case, values, dev)
    q64, bound = R.q_values(*args, dtype=np.float64), R.q_bound(*args)
    err = np.abs(q.astype(np.float64) - q64)
    print(f"scale {scale}: max |q - q64| = {err.max():.3e}, max err / bound = {(err / np.maximum(bound, 1e-300)).max():.4f}, "
          f"median |q64| = {np.median(np.abs(q64[case['nchild'] > 0])):.3e}")
    assert (err <= bound).all()
    assert (q[case["nchild"] == 0].view(np.uint32) == 0).all()
    poisoned = np.where(case["terminal"] != 0, np.float32(1e30), values).astype(np.float32)
    assert np.array_equal(_dev_reduce(case, poisoned, dev).view(np.uint32),
                          _dev_reduce(case, np.where(case["terminal"] != 0, np.float32(0), values).astype(np.float32), dev).view(np.uint32))
    assert np.array_equal(_dev_reduce(case, poisoned, dev).view(np.uint32), q.view(np.uint32))


# ----------------------------------------------------------------------------------------------- composition with a real agent
def _recipe_agent(dev, reduction):
    agent = PPOAgent(observation_dim=31, action_dim=4, hidden_dim=512, d_model=256, nhead=8, num_layers=4, dim_feedforward=1024,
                     dropout=0.1, reduction=reduction).eval()
    sd = agent.state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in fill_state_dict({k: tuple(v.shape) for k, v in sd.items()}).items()})
    agent.load_state_dict(sd)
    return agent.to(dev).eval()


def _check_composition(fn, boards_np, value_rows, dev, what):
    """fn.policy_fn(boards) against reduce_numpy(value_rows(children_numpy)), bound 3; v = max of q over the legal actions.
    ``value_rows`` is handed the same row ranges the function forwards (rows [k * max_children, (k + 1) * max_children)):
    GEMM libraries choose kernels by row count, so only equal calls give equal bits."""
    after, reward, nchild = R.expand(boards_np)
    children, terminal, offset = R.children(after, nchild)
    N = len(children)
    rows = torch.from_numpy(children).to(dev)
    with torch.no_grad():
        values = torch.cat([value_rows(rows[c0:c0 + fn.max_children]).float().reshape(-1)
                            for c0 in range(0, N, fn.max_children)]).cpu().numpy()
    q, v = fn.policy_fn(torch.from_numpy(boards_np).to(dev), None)
    assert fn.last_children == N
    q, v = q.cpu().numpy(), v.cpu().numpy()
    args = (reward, nchild, offset, values, terminal, fn.gamma)
    q64, bound = R.q_values(*args, dtype=np.float64), R.q_bound(*args)
    err = np.abs(q.astype(np.float64) - q64)
    print(f"{what}: N = {N}, calls = {-(-N // fn.max_children)}, max err / bound = {(err / np.maximum(bound, 1e-300)).max():.4f}")
    assert (err <= bound).all(), what
    legal = nchild > 0
    vmax = np.where(legal.any(axis=1), np.where(legal, q, -np.inf).max(axis=1), 0.0).astype(np.float32)
    assert np.array_equal(v, vmax), what
    return N


@pytest.mark.parametrize("reduction", ["cls", "mean"])
def test_composition_fused_bf16(dev, reduction):
    agent = _recipe_agent(dev, reduction)
    boards = sample_boards(2048)
    fp = FusedPolicy(agent)
    whole = LookaheadActionFunction(agent, gamma=GAMMA, device=dev, amp_dtype=torch.bfloat16)
    assert whole._fused is not None and whole.use_mask and not whole.sample_actions
    N = _check_composition(whole, boards, lambda r: fp(r)[1], dev, f"fused {reduction}, one call")
    assert N <= whole.max_children
    # several forward calls, a boundary inside one board's children (1001 is odd: it even splits a cell's pair of tiles)
    chunked = LookaheadActionFunction(agent, gamma=GAMMA, device=dev, amp_dtype=torch.bfloat16, max_children=1001)
    _check_composition(chunked, boards, lambda r: fp(r)[1], dev, f"fused {reduction}, chunks of 1001")


def test_composition_module_forward_fp32(dev):
    agent = _recipe_agent(dev, "cls")
    boards = sample_boards(512)
    module = lambda r: agent(r, None)[1]
    whole = LookaheadActionFunction(agent, gamma=GAMMA, device=dev, use_fused=False)
    assert whole._fused is None
    _check_composition(whole, boards, module, dev, "fp32 module, one call")
    _check_composition(LookaheadActionFunction(agent, gamma=GAMMA, device=dev, use_fused=False, max_children=777), boards, module,
                       dev, "fp32 module, chunks of 777")


def test_lookahead_sees_new_weights(dev):
    """refresh_if_stale carries over: a function kept across an in-place parameter update uses the new critic."""
    agent = _recipe_agent(dev, "cls")
    boards = torch.from_numpy(sample_boards(64)).to(dev)
    fn = LookaheadActionFunction(agent, device=dev, amp_dtype=torch.bfloat16)
    q0, _ = fn.policy_fn(boards, None)
    with torch.no_grad():
        for p in agent.parameters():
            p.mul_(1.05)
    q1, _ = fn.policy_fn(boards, None)
    fresh, _ = LookaheadActionFunction(agent, device=dev, amp_dtype=torch.bfloat16).policy_fn(boards, None)
    assert torch.equal(q1, fresh) and not torch.equal(q0, q1)


# ----------------------------------------------------------------------------------------------- action choice through the engine
class TableCritic(torch.nn.Module):
    """V(s) = sum_cell T[cell, tile], T f32 normal: summed in float64 and rounded once, so the value of a board does not depend
    on the batch it sits in and numpy float64 reproduces it up to that one rounding.  The logits are never read."""

    def __init__(self, seed=5):
        super().__init__()
        self.table = torch.nn.Parameter(torch.from_numpy(np.random.default_rng(seed).normal(0.0, 1.0, (16, 32)).astype(np.float32)))

    def forward(self, boards, mask=None):
        cells = torch.arange(16, device=boards.device)
        v = self.table.double()[cells[None, :], boards.long()].sum(dim=1)
        return torch.zeros((boards.shape[0], 4), device=boards.device), v.float()

    def numpy_values(self, boards_np):
        T = self.table.detach().cpu().numpy().astype(np.float64)
        return T[np.arange(16)[None, :], boards_np.astype(np.int64)].sum(axis=1)


@pytest.mark.parametrize("mode", ["legacy", "partitionable"])
def test_engine_plays_the_expectimax_argmax(dev, mode):
    """BatchRunner.collect(256) with the lookahead function: (a) an oracle replay of the recorded actions reproduces boards,
    rewards and episode lengths bit for bit; (b) every recorded action is the float64 expectimax argmax, except where the float64
    gap between the two best legal Q is below twice bound 3 - at most 1 % of the steps (checked on the CPU for this table and
    seed, float32 against float64 numpy on the trajectory the float32 player visits: 9 such steps of 49 333 with the legacy
    stream, 3 of 49 917 with the partitionable one, and no other disagreement)."""
    B, seed = 256, 11
    critic = TableCritic()
    fn = LookaheadActionFunction(critic, gamma=GAMMA, device=dev)
    tr = BatchRunner(init_seed=seed, act_fn=fn, rng_mode=mode, device=dev).collect(B)
    actions = tr.actions.cpu().numpy().astype(np.int32)  # [T, B]
    ep_len = tr.ep_len.cpu().numpy()
    valid = np.arange(tr.T)[:, None] < ep_len[None, :]
    step = iter(range(tr.T))
    replay = npo.Runner(seed, 0 if mode == "legacy" else 1).run(
        B, "callable", policy_fn=lambda k, b, m: (actions[next(step)], np.zeros(B, np.float32), np.zeros(B, np.float32)))
    rb, rr, rt = (np.swapaxes(replay[k], 0, 1) for k in ("boards", "rewards", "terms"))
    To = rb.shape[0]  # the engine polls for the end every sync_every lock-steps: tr.T is To rounded up
    assert To == ep_len.max() and To <= tr.T < To + fn.sync_every
    valid, actions = valid[:To], actions[:To]
    assert np.array_equal(tr.boards.cpu().numpy()[:To][valid], rb[valid])
    assert np.array_equal(tr.rewards.cpu().numpy()[:To][valid].view(np.uint32), rr[valid].view(np.uint32))
    assert np.array_equal(ep_len, rt.argmax(axis=0) + 1) and rt[-1].all()
    assert np.array_equal(tr.final_boards.cpu().numpy(), replay["final_boards"])
    # (b)
    boards = rb[valid]
    after, reward, nchild = R.expand(boards)
    children, terminal, offset = R.children(after, nchild)
    values = critic.numpy_values(children)
    args = (reward, nchild, offset, values, terminal, GAMMA)
    q64, bound = R.q_values(*args, dtype=np.float64), R.q_bound(*args)
    legal = nchild > 0
    assert legal.any(axis=1).all()  # a board the engine still steps has a move
    qm = np.where(legal, q64, -np.inf)
    order = np.argsort(-qm, axis=1, kind="stable")
    best, second = np.take_along_axis(qm, order[:, :1], 1)[:, 0], np.take_along_axis(qm, order[:, 1:2], 1)[:, 0]
    slack = 2.0 * np.take_along_axis(bound, order[:, :2], 1).max(axis=1)
    near_tie = (best - second) < slack
    print(f"{mode}: {len(boards)} steps, T = {tr.T}, near ties skipped = {int(near_tie.sum())}, mean children per board = "
          f"{nchild.sum() / len(boards):.1f}")
    assert near_tie.mean() <= 0.01
    assert np.array_equal(actions[valid][~near_tie], order[:, 0][~near_tie])
    # the recorded value is max_a q, the log-prob the log-softmax of q at the chosen action (not a policy probability)
    got_v = tr.values.cpu().numpy()[:To][valid]
    assert (np.abs(got_v - best) <= bound.max(axis=1) + 2.0 ** -23 * np.abs(best)).all()
    lp = tr.log_probs.cpu().numpy()[:To][valid]
    ref_lp = -np.log(np.exp(qm - best[:, None]).sum(axis=1))
    assert (np.abs(lp - ref_lp)[~near_tie] <= 1e-3 + 1e-6 * np.abs(best[~near_tie])).all()  # f32 q - logsumexp(q) at |q| up to 1e3


# ----------------------------------------------------------------------------------------------- off means off
def test_off_means_off(dev, monkeypatch):
    torch.manual_seed(3)
    agent = PPOAgent(hidden_dim=64, d_model=64, nhead=4, num_layers=2, dim_feedforward=128, reduction="cls")
    direct = TorchActionFunction(agent, use_mask=True, sample_actions=False, device=dev)
    ref = evaluate_max_tile(direct, 24, seed=5, batch_size=100, device=dev)
    tr_ref = BatchRunner(init_seed=9, act_fn=direct, device=dev).collect(32, fill_frozen=True)

    def boom(*a, **k):
        raise AssertionError("lookahead=0 must not build a LookaheadActionFunction")

    with monkeypatch.context() as m:
        m.setattr(LookaheadActionFunction, "__init__", boom)
        assert evaluate_agent(agent, dev, 24, seed=5) == ref
        assert evaluate_agent(agent, dev, 24, seed=5, lookahead=0, gamma=0.5) == ref
    tr = BatchRunner(init_seed=9, act_fn=TorchActionFunction(agent, use_mask=True, sample_actions=False, device=dev), device=dev).collect(32, fill_frozen=True)
    for k in ("boards", "meta", "rewards", "log_probs", "values", "ep_len", "final_boards"):
        assert torch.equal(getattr(tr, k), getattr(tr_ref, k)), k
    with pytest.raises(ValueError):
        LookaheadActionFunction(agent, depth=2, device=dev)
    with pytest.raises(ValueError):
        evaluate_agent(agent, dev, 4, lookahead=2)
    # lookahead=1 runs the same protocol on the same seeds and plays something else
    la = evaluate_agent(agent, dev, 24, seed=5, lookahead=1)
    assert la["episodes"] == 24 and la != ref


def test_unbatched_call_equals_batched_path(dev):
    critic = TableCritic(seed=8)
    fn = LookaheadActionFunction(critic, gamma=GAMMA, device=dev)
    boards = sample_boards(80, seed=3)
    boards = boards[npo.legal_mask(boards).any(axis=1)][:64]
    assert len(boards) == 64
    masks = npo.legal_mask(boards)
    obs = npo.observation(boards)
    q, v = fn.policy_fn(torch.from_numpy(boards).to(dev), None)
    want = torch.where(torch.from_numpy(masks).to(dev), q, torch.full_like(q, float("-inf"))).argmax(dim=1).cpu().numpy()
    keys = np.stack([npo.key(i) for i in range(len(boards))])
    for i in range(len(boards)):
        a, lp, val = fn(keys[i], obs[i], masks[i])
        assert int(a) == int(want[i]) and np.float32(val) == v[i].item() and np.isfinite(lp)
    a, lp, val = fn(keys, obs, masks)  # leading batch dimension
    assert np.array_equal(a, want) and np.array_equal(val, v.cpu().numpy())
