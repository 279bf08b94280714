"""Two-ply expectimax on the device: g2048_lookahead_dedup / _backup against the numpy restatement (tests/lookahead2_ref.py),
ExpectimaxActionFunction against the float64 pipeline and against the agent's own value forward, action choice through the
engine's argmax, and the public evaluation path."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

import lookahead2_ref as R2  # noqa: E402
import lookahead_ref as R  # noqa: E402
from oracle import g2048_oracle as npo  # noqa: E402
from src.g2048 import native as nv  # noqa: E402
from src.ppo import ExpectimaxActionFunction, LookaheadActionFunction, PPOAgent  # noqa: E402
from src.ppo.fused_policy import FusedPolicy  # noqa: E402
from src.runs import evaluate_agent  # noqa: E402
from weights_recipe import fill_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu
GAMMA = 0.99
TABLE_SEED = 5


class TableCritic(torch.nn.Module):
    """V(s) = sum_cell T[cell, tile], summed in float64 and rounded once: the value of a board does not depend on the batch it
    sits in, and numpy float64 reproduces it up to that one rounding.  The logits are never read."""

    def __init__(self, seed=TABLE_SEED):
        super().__init__()
        self.table = torch.nn.Parameter(torch.from_numpy(R2.table(seed)))

    def forward(self, boards, mask=None):
        cells = torch.arange(16, device=boards.device)
        v = self.table.double()[cells[None, :], boards.long()].sum(dim=1)
        return torch.zeros((boards.shape[0], 4), device=boards.device), v.float()


@pytest.fixture(scope="module")
def case():
    """The test boards and their float64 two-ply pipeline under the table critic, computed once and left unchanged."""
    boards = R2.test_boards()
    T = R2.table(TABLE_SEED)
    p = R2.pipeline(boards, lambda rows: R2.table_values(T, rows), GAMMA, np.float64, True)
    sizes = np.diff(p["group_start"])
    assert sizes.max() == R2.MAX_GROUP and sizes.min() == 0 and 200 <= len(boards) <= 600
    return dict(boards=boards, table=T, p=p, bound=R2.q2_bound(p, GAMMA))


def test_dedup_equals_numpy_bit_for_bit_and_leaves_the_slack_alone(dev, case):
    p = case["p"]
    P = p["nchild2"].size
    slack = 1031
    rep = torch.full((P + slack,), -77, dtype=torch.int32, device=dev)
    nuniq = torch.full((P + slack,), -77, dtype=torch.int32, device=dev)
    nv.lookahead_dedup(torch.from_numpy(p["after2"]).to(dev), torch.from_numpy(p["nchild2"]).to(dev),
                       torch.from_numpy(p["group_start"]).to(dev), rep, nuniq)
    assert np.array_equal(rep[:P].cpu().numpy(), p["rep"].reshape(-1))
    assert np.array_equal(nuniq[:P].cpu().numpy(), p["nuniq"].reshape(-1))
    assert (rep[P:] == -77).all() and (nuniq[P:] == -77).all()
    assert 0 < p["nuniq"].sum() < p["nchild2"].sum()
    # one group alone, the largest (480 pairs, every lane of the block's four passes in use), gives the same answer
    g = int(np.diff(p["group_start"]).argmax())
    s, e = int(p["group_start"][g]), int(p["group_start"][g + 1])
    rep1 = torch.full((e - s,), -77, dtype=torch.int32, device=dev)
    nuniq1 = torch.full((e - s,), -77, dtype=torch.int32, device=dev)
    nv.lookahead_dedup(torch.from_numpy(p["after2"].reshape(-1, 16)[s:e].copy()).to(dev),
                       torch.from_numpy(p["nchild2"].reshape(-1)[s:e].copy()).to(dev),
                       torch.tensor([0, e - s], dtype=torch.int32, device=dev), rep1, nuniq1)
    assert np.array_equal(rep1.cpu().numpy() + s, p["rep"].reshape(-1)[s:e])
    assert np.array_equal(nuniq1.cpu().numpy(), p["nuniq"].reshape(-1)[s:e])
    # a group of more than 480 pairs (the host cannot see it: P <= 480 G) is left without duplicates and without children, its
    # neighbour is served as usual, and nothing outside [0, P) is written
    n = 488
    keys, cnt = p["after2"].reshape(-1, 16)[:n].copy(), p["nchild2"].reshape(-1)[:n].copy()
    rep2 = torch.full((n + 8,), -77, dtype=torch.int32, device=dev)
    nuniq2 = torch.full((n + 8,), -77, dtype=torch.int32, device=dev)
    nv.lookahead_dedup(torch.from_numpy(keys).to(dev), torch.from_numpy(cnt).to(dev),
                       torch.tensor([0, 484, n], dtype=torch.int32, device=dev), rep2[:n], nuniq2[:n])
    want_rep, want_n = R2.dedup(keys.reshape(-1, 4, 16)[121:], cnt.reshape(-1, 4)[121:], np.array([0, 4], np.int32))
    assert np.array_equal(rep2[:484].cpu().numpy(), np.arange(484)) and (nuniq2[:484] == 0).all()
    assert np.array_equal(rep2[484:n].cpu().numpy(), want_rep.reshape(-1) + 484)
    assert np.array_equal(nuniq2[484:n].cpu().numpy(), want_n.reshape(-1))
    assert (rep2[n:] == -77).all() and (nuniq2[n:] == -77).all()


def test_backup_equals_numpy_f32_bit_for_bit(dev, case):
    """Individually rounded adds and an exact max: numpy float32 gives the same bits."""
    p = case["p"]
    N1 = len(p["children1"])
    rng = np.random.default_rng(7)
    e = rng.normal(0.0, 100.0, (N1, 4)).astype(np.float32)
    e[rng.random((N1, 4)) < 0.05] = 0.0
    assert (~(p["nchild2"] > 0).any(axis=1)).any()                                  # rows with no legal action
    assert (p["rep"][p["nchild2"] > 0] // 4 != np.nonzero(p["nchild2"] > 0)[0]).any()  # reps that point into another child
    v1 = torch.full((N1 + 9,), 123.0, dtype=torch.float32, device=dev)
    nv.lookahead_backup(torch.from_numpy(p["reward2"]).to(dev), torch.from_numpy(p["nchild2"]).to(dev),
                        torch.from_numpy(p["rep"]).to(dev), torch.from_numpy(e).to(dev), v1)
    want = R2.backup(p["reward2"], p["nchild2"], p["rep"], e, np.float32)
    assert np.array_equal(v1[:N1].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert (v1[N1:] == 123.0).all()
    assert (want[~(p["nchild2"] > 0).any(axis=1)].view(np.uint32) == 0).all()


@pytest.fixture(scope="module")
def table_q2(dev, case):
    """policy_fn of the table critic on the test boards: dedup on, dedup off, and slices / chunks of 120."""
    critic = TableCritic().to(dev)
    boards = torch.from_numpy(case["boards"]).to(dev)
    out = {}
    for name, kw in (("dedup", dict(dedup=True)), ("full", dict(dedup=False)), ("sliced", dict(dedup=True, max_children=120))):
        fn = ExpectimaxActionFunction(critic, gamma=GAMMA, device=dev, **kw)
        assert fn.use_mask and not fn.sample_actions and fn._fused is None
        q, v = fn.policy_fn(boards, None)
        out[name] = dict(q=q.cpu().numpy(), v=v.cpu().numpy(), rows=fn.last_children, rows_full=fn.last_children_full, q_dev=q)
    return out


def test_composition_table_critic(case, table_q2):
    p, bound = case["p"], case["bound"]
    d, f, s = table_q2["dedup"], table_q2["full"], table_q2["sliced"]
    assert np.array_equal(d["q"].view(np.uint32), f["q"].view(np.uint32))  # dedup changes no bit
    assert np.array_equal(d["q"].view(np.uint32), s["q"].view(np.uint32))  # nor do several root slices and forward chunks
    assert np.array_equal(d["v"].view(np.uint32), f["v"].view(np.uint32)) and np.array_equal(d["v"].view(np.uint32), s["v"].view(np.uint32))
    err = np.abs(d["q"].astype(np.float64) - p["q2"])
    print(f"{len(case['boards'])} boards, rows {d['rows']} of {d['rows_full']}, max |q2 - q64| = {err.max():.3e}, "
          f"max err / bound = {(err / np.maximum(bound, 1e-300)).max():.4f}")
    assert (err <= bound).all()
    assert (d["q"][p["nchild1"] == 0].view(np.uint32) == 0).all()
    n_uniq, n_full = int(p["nuniq"].sum()), int(p["nchild2"].sum())
    assert (d["rows"], d["rows_full"]) == (n_uniq, n_full) and (s["rows"], s["rows_full"]) == (n_uniq, n_full)
    assert (f["rows"], f["rows_full"]) == (n_full, n_full)
    assert len(p["children1"]) > 120 * 50  # max_children=120 cut the roots into many slices
    legal = p["nchild1"] > 0
    vmax = np.where(legal.any(axis=1), np.where(legal, d["q"], -np.inf).max(axis=1), 0.0).astype(np.float32)
    assert np.array_equal(d["v"], vmax)


def test_one_ply_delegates(dev, case):
    critic = TableCritic().to(dev)
    boards = torch.from_numpy(case["boards"]).to(dev)
    one = ExpectimaxActionFunction(critic, plies=1, gamma=GAMMA, device=dev)
    ref = LookaheadActionFunction(critic, gamma=GAMMA, device=dev)
    (q, v), (qr, vr) = one.policy_fn(boards, None), ref.policy_fn(boards, None)
    assert torch.equal(q, qr) and torch.equal(v, vr) and one.last_children == ref.last_children == one.last_children_full


# ----------------------------------------------------------------------------------------------- composition with real agents
def _recipe_agent(dev, reduction):
    agent = PPOAgent(observation_dim=31, action_dim=4, hidden_dim=512, d_model=256, nhead=8, num_layers=4, dim_feedforward=1024,
                     dropout=0.1, reduction=reduction).eval()
    sd = agent.state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in fill_state_dict({k: tuple(v.shape) for k, v in sd.items()}).items()})
    agent.load_state_dict(sd)
    return agent.to(dev).eval()


def _boards24(case):
    """24 boards: the largest group, a full board without a move, one merge, one legal move, double merges, big tiles, and 18 of
    the rollout boards."""
    hand = len(R.hand_made_boards())
    rest = np.linspace(hand, len(case["boards"]) - 1, 18).astype(int)
    return case["boards"][np.concatenate([[3, 10, 14, 15, 21, 22], rest])]


def _check_real_agent(fn, value_rows, boards_np, dev, what):
    """fn.policy_fn against the float64 numpy pipeline fed with the device's own values of the same rows, read back (one call on
    the same row range the function forwards: GEMM libraries choose kernels by row count)."""

    def values_of(rows_np):
        assert len(rows_np) <= fn.max_children
        with torch.no_grad():
            return value_rows(torch.from_numpy(rows_np).to(dev)).float().reshape(-1).cpu().numpy()

    p = R2.pipeline(boards_np, values_of, fn.gamma, np.float64, fn.dedup)
    bound = R2.q2_bound(p, fn.gamma, value_rounding=False)
    q, _ = fn.policy_fn(torch.from_numpy(boards_np).to(dev), None)
    err = np.abs(q.cpu().numpy().astype(np.float64) - p["q2"])
    print(f"{what}: rows {fn.last_children} of {fn.last_children_full}, max err / bound = {(err / np.maximum(bound, 1e-300)).max():.4f}")
    assert fn.last_children == len(p["children2"]) and fn.last_children_full == int(p["nchild2"].sum())
    assert (err <= bound).all(), what


@pytest.mark.parametrize("reduction", ["cls", "mean"])
def test_composition_fused_bf16(dev, case, reduction):
    agent = _recipe_agent(dev, reduction)
    fp = FusedPolicy(agent)
    fn = ExpectimaxActionFunction(agent, gamma=GAMMA, device=dev, amp_dtype=torch.bfloat16)
    assert fn._fused is not None
    _check_real_agent(fn, lambda r: fp(r)[1], _boards24(case), dev, f"fused {reduction}")


def test_composition_module_forward_fp32(dev, case):
    torch.manual_seed(3)
    agent = PPOAgent(hidden_dim=64, d_model=64, nhead=4, num_layers=2, dim_feedforward=128, reduction="cls").to(dev).eval()
    fn = ExpectimaxActionFunction(agent, gamma=GAMMA, device=dev, use_fused=False)
    assert fn._fused is None
    _check_real_agent(fn, lambda r: agent(r, None)[1], _boards24(case), dev, "fp32 module")


# ----------------------------------------------------------------------------------------------- action choice through the engine
def test_engine_argmax_is_the_float64_argmax(dev, case, table_q2):
    """g2048_act_logits on the device's q2 (the un-batched plug-in protocol with a leading batch dimension): every action of a
    board with a move equals the float64 argmax, except where the float64 gap between the two best legal Q2 is below twice the
    bound; such near ties may be at most 1 % of those boards.  Counted on the CPU for table seed 5 before any device run, float32
    against float64 numpy: 2 near ties of 281 boards with a move (0.7 %), and no disagreement at all between the two."""
    p, bound = case["p"], case["bound"]
    legal = p["nchild1"] > 0
    live = legal.any(axis=1)
    boards = case["boards"][live]
    assert np.array_equal(legal, npo.legal_mask(case["boards"]))
    fn = ExpectimaxActionFunction(TableCritic().to(dev), gamma=GAMMA, device=dev)
    keys = np.stack([npo.key(i) for i in range(len(boards))])
    actions, logp, values = fn(keys, npo.observation(boards), legal[live])
    assert np.array_equal(values.view(np.uint32), table_q2["dedup"]["v"][live].view(np.uint32)) and np.isfinite(logp).all()
    qm = np.where(legal, p["q2"], -np.inf)[live]
    order = np.argsort(-qm, axis=1, kind="stable")
    best, second = np.take_along_axis(qm, order[:, :1], 1)[:, 0], np.take_along_axis(qm, order[:, 1:2], 1)[:, 0]
    near_tie = (best - second) < 2.0 * np.take_along_axis(bound[live], order[:, :2], 1).max(axis=1)
    print(f"{len(boards)} boards with a move, near ties skipped = {int(near_tie.sum())}")
    assert near_tie.mean() <= 0.01
    assert np.array_equal(np.asarray(actions)[~near_tie], order[:, 0][~near_tie])


# ----------------------------------------------------------------------------------------------- the public path
def test_evaluate_agent_expectimax(dev):
    torch.manual_seed(3)
    agent = PPOAgent(hidden_dim=64, d_model=64, nhead=4, num_layers=2, dim_feedforward=128, reduction="cls")
    greedy = evaluate_agent(agent, dev, 8, seed=5)
    assert evaluate_agent(agent, dev, 8, seed=5, expectimax=0) == greedy  # off means off
    one = evaluate_agent(agent, dev, 8, seed=5, lookahead=1)
    two = evaluate_agent(agent, dev, 8, seed=5, expectimax=2)
    assert two["episodes"] == 8 and two != one and two != greedy
    with pytest.raises(ValueError):
        evaluate_agent(agent, dev, 8, seed=5, expectimax=1)  # one ply has one public spelling: lookahead=1
    with pytest.raises(ValueError):
        evaluate_agent(agent, dev, 8, lookahead=2)
    with pytest.raises(ValueError):
        evaluate_agent(agent, dev, 8, lookahead=1, expectimax=2)
