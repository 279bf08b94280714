"""Multi-stage n-tuple network on the GPU: values, scores, expectimax, the TD(0) and TC steps and whole training runs with promotions,
bit-exact against the numpy restatement (tests/ntuple_stage_ref.py); promotion invariance on the device; the player, evaluation and
distillation on a staged network; and the unstaged path unchanged."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import ntuple_ref as N  # noqa: E402
import ntuple_stage_ref as G  # noqa: E402
from oracle import g2048_oracle as npo  # noqa: E402
from src.g2048 import native as nv  # noqa: E402
from src.ppo import DistillTrainer, NTupleActionFunction, NTupleNetwork, NTupleTrainer, PPOAgent  # noqa: E402
from src.runs import BatchRunner, evaluate_ntuple  # noqa: E402

pytestmark = pytest.mark.gpu
SLACK = 259
GUARD = 0xA5A5A5A5
GUARD_F32 = float(np.array([GUARD], np.uint32).view(np.float32)[0])
SIZES = (1, 5, 63, 257, 1000)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _dev(a, dev):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(dev)  # a copy: the shared cases are read-only arrays


def _f32(a, dev):
    return _dev(np.asarray(a, np.float32).view(np.int32), dev).view(torch.float32)


def _network(name, dev, weights=None):
    """The fixture network ``name`` on the device with every stage active and the restatement's per-stage random weights."""
    tuples, tiles, F = G.NETWORKS[name]
    net = NTupleNetwork(tuples, F, dev, tiles)
    net.weights.copy_(_dev(G.staged_weights(name) if weights is None else weights, dev))
    net.active_stages = net.stages
    return net


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("name", list(G.NETWORKS))
def test_values_and_scores_are_bit_exact(dev, name, B):
    """Through the entry points, inside guard words; the restatement asserts on the CPU that every stage is looked up and that some
    afterstate's stage is not its board's."""
    tuples, tiles, F = G.NETWORKS[name]
    c = G.values_case(name)
    cells, w = N.cells_array(tuples), _dev(G.staged_weights(name), dev)
    boards = _dev(c["boards"][:B], dev)
    v = torch.full((B + SLACK,), GUARD_F32, device=dev)
    nv.ntuple_values(boards, w, cells, F, v[:B], np.array(tiles, np.uint8))
    assert np.array_equal(_bits(v[:B]), c["v"][:B].view(np.uint32)) and (_bits(v[B:]) == GUARD).all()
    q = torch.full((B + SLACK, 4), GUARD_F32, device=dev)
    qv = torch.full((B + SLACK,), GUARD_F32, device=dev)
    nv.ntuple_scores(boards, w, cells, F, q[:B], qv[:B], tiles)
    assert np.array_equal(_bits(q[:B]), c["q"][:B].view(np.uint32)) and np.array_equal(_bits(qv[:B]), c["qv"][:B].view(np.uint32))
    assert (_bits(q[B:]) == GUARD).all() and (_bits(qv[B:]) == GUARD).all()


@pytest.mark.parametrize("plies", [1, 2])
@pytest.mark.parametrize("name", list(G.NETWORKS))
def test_expectimax_is_bit_exact(dev, name, plies):
    """B = 37, both gammas, through NTupleNetwork.expectimax; for two plies the restatement asserts that a leaf's stage differs from
    its root's."""
    c = G.search_case(name, plies)
    net = _network(name, dev)
    boards = _dev(c["boards"], dev)
    assert len(c["boards"]) == 37
    for gamma in G.GAMMAS:
        q, v = net.expectimax(boards, plies, gamma)
        assert np.array_equal(_bits(q), c["q"][gamma].view(np.uint32)), gamma
        assert np.array_equal(_bits(v), c["v"][gamma].view(np.uint32)), gamma


class Tables:
    """Device weights, coherence tables and accumulators of one staged network."""

    def __init__(self, dev, w0, tuples, tiles):
        self.dev, self.cells, self.tiles = dev, N.cells_array(tuples), np.array(tiles, np.uint8)
        self.w = _dev(w0, dev)
        self.coh_e, self.coh_a = torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.acc = torch.zeros(self.w.shape, dtype=torch.int64, device=dev)
        self.abs_acc, self.cnt = torch.zeros_like(self.acc), torch.zeros_like(self.w)

    def step(self, learner, prev, flag, target, F, alpha):
        """accumulate + apply -> td_error bits; the accumulators must be all-zero afterwards."""
        B, dev = len(flag), self.dev
        err = torch.full((B + SLACK,), GUARD_F32, device=dev)
        t_prev, t_flag, t_target = _dev(prev, dev), _dev(flag, dev), _f32(target, dev)
        if learner == "tc":
            nv.ntuple_tc_accumulate(t_prev, t_flag, t_target, self.w, self.cells, F, alpha, self.acc, self.abs_acc, self.cnt, err[:B],
                                    self.tiles)
            hits = int(self.cnt.sum().item())
            nv.ntuple_tc_apply(t_prev, t_flag, self.cells, self.w, self.acc, self.abs_acc, self.cnt, self.coh_e, self.coh_a, self.tiles)
        else:
            nv.ntuple_td_accumulate(t_prev, t_flag, t_target, self.w, self.cells, F, alpha, self.acc, self.cnt, err[:B], self.tiles)
            hits = int(self.cnt.sum().item())
            nv.ntuple_td_apply(t_prev, t_flag, self.cells, self.w, self.acc, self.cnt, self.tiles)
        assert hits == 8 * self.cells.shape[0] * int((flag != 0).sum())
        assert not self.acc.any() and not self.abs_acc.any() and not self.cnt.any()
        assert (_bits(err[B:]) == GUARD).all()
        return _bits(err[:B])

    def equal(self, w, coh_e=None, coh_a=None):
        same = np.array_equal(self.w.cpu().numpy(), w)
        if coh_e is not None:
            same = same and np.array_equal(self.coh_e.cpu().numpy(), coh_e) and np.array_equal(self.coh_a.cpu().numpy(), coh_a)
        return same


def test_td_and_tc_step_under_collision_in_two_orders(dev):
    """1000 envs, 300 of them identical, over at least three stages (asserted by the restatement), flags 0 / 1 / 2, in two env orders:
    the atomics' sums are order-free, and the top stage, which no env is in, keeps its tables."""
    c = G.collision_case()
    tuples, tiles, F = G.NETWORKS["small5"]
    w0 = G.staged_weights("small5")
    assert len(c["stages_hit"]) >= 3 and np.unique(c["prev"], axis=0, return_counts=True)[1].max() >= 300
    perm = np.random.default_rng(1).permutation(1000)
    for order in (np.arange(1000), perm):
        prev, flag, target = c["prev"][order], c["flag"][order], c["target"][order]
        td = Tables(dev, w0, tuples, tiles)
        err = td.step("td0", prev, flag, target, F, 0.1)
        assert td.equal(c["td_w"]) and np.array_equal(err, c["td_e"][order].view(np.uint32))
        tc = Tables(dev, w0, tuples, tiles)
        err = tc.step("tc", prev, flag, target, F, 0.1)
        assert tc.equal(c["tc_w"], c["tc_ce"], c["tc_ca"]) and np.array_equal(err, c["tc_e"][order].view(np.uint32))
        assert np.array_equal(tc.w[4].cpu().numpy(), w0[4]) and not tc.coh_a[4].any()


def test_six_steps_with_saturation_and_the_clamp_in_two_stages(dev):
    """The saturation and clamp sequence of the unstaged tests with its envs in two stages: weights preset near +-2^31, alpha 1000
    and targets of 1e9, six TC steps; the weights saturate, delta sits on the clamp, A is halved (asserted on the restatement)."""
    c = G.sequence_case(1000.0, 1e9, True)
    assert c["stats"]["saturated"] > 0 and c["stats"]["clamped"] > 0 and c["stats"]["halved"] > 0 and c["stats"]["slowed"] > 0
    tb = Tables(dev, c["w0"], c["tuples"], c["tiles"])
    for t, want in enumerate(c["after"]):
        err = tb.step("tc", c["prev"], c["flag"], c["targets"][t], c["F"], 1000.0)
        assert tb.equal(want["weights"], want["coh_e"], want["coh_a"]), t
        assert np.array_equal(err, want["td_error"].view(np.uint32)), t
    assert tb.coh_a[0].any() and tb.coh_a[1].any()


@pytest.mark.parametrize("learner,alpha", [("td0", 0.1), ("tc", 1.0)])
def test_trainer_replay_with_promotions(dev, learner, alpha):
    """NTupleTrainer(net, 64, promote_every=8).train(48, record=True) on SMALL with stage_tiles (3, 4, 5) from zero weights: the
    restatement, fed the recorded boards and meta rows, reproduces scores, targets, the final weights (and coherence tables), the
    ``promotions`` list and ``active_stages == 4``.  ``train(20); train(28)`` from the same seed gives the same bits."""
    tiles = (3, 4, 5)

    def fresh():
        net = NTupleNetwork(N.SMALL, 12, dev, tiles)
        return net, NTupleTrainer(net, 64, alpha=alpha, seed=0, rng_mode=npo.MODE_PARTITIONABLE, device=dev, learner=learner,
                                  promote_every=8)

    net, trainer = fresh()
    out = trainer.train(48, record=True)
    boards, meta = out["boards"].cpu().numpy(), out["meta"].cpu().numpy()
    ref = G.Net(np.zeros((4, 3, 256), np.int32), N.SMALL, tiles, 12)
    ce, ca = np.zeros(ref.w.shape, np.int32), np.zeros(ref.w.shape, np.int32)
    want_q, want_v, promotions = G.replay_training(ref, boards, meta, alpha, learner, 8, ce, ca)
    assert ref.active == 4 and net.active_stages == 4
    assert trainer.promotions == promotions and [p[1] for p in promotions] == [2, 3, 4]
    assert np.array_equal(_bits(out["scores"]), want_q.view(np.uint32))
    assert np.array_equal(_bits(out["targets"]), want_v.view(np.uint32))
    assert np.array_equal(net.weights.cpu().numpy(), ref.w) and all(ref.w[s].any() for s in range(4))
    if learner == "tc":
        assert np.array_equal(trainer.coh_e.cpu().numpy(), ce) and np.array_equal(trainer.coh_a.cpu().numpy(), ca)
        assert not trainer.abs_acc.any()
    assert not trainer.acc.any() and not trainer.cnt.any() and trainer.lock_steps == 48
    assert np.array_equal(net.stage_of(out["boards"][-1]).cpu().numpy(), G.stage(boards[-1], tiles).astype(np.uint8))
    net2, split = fresh()
    split.train(20)
    split.train(28)
    assert torch.equal(net2.weights, net.weights) and split.promotions == trainer.promotions and net2.active_stages == 4
    if learner == "tc":
        assert torch.equal(split.coh_e, trainer.coh_e) and torch.equal(split.coh_a, trainer.coh_a)


def test_promotion_changes_no_result_on_the_device(dev):
    """Values, scores and two-ply results of 257 boards before and after every ``promote()``: equal, bit for bit."""
    tuples, tiles, F = G.NETWORKS["small5"]
    net = NTupleNetwork(tuples, F, dev, tiles)
    net.weights[0].copy_(_dev(N.small_weights(), dev))
    boards = _dev(G.boards_for("small5", 257), dev)

    def results():
        q, v = net.scores(boards)
        q2, v2 = net.expectimax(boards, 2, 0.99)
        return [_bits(x) for x in (net.values(boards), q, v, q2, v2)]

    before = results()
    for p in range(2, 6):
        assert net.promote() == p
        after = results()
        assert all(np.array_equal(a, b) for a, b in zip(after, before)), p
        # ... and once the new stage's table differs, the boards of that stage (and only they) change
        net.weights[p - 1] += 1
        moved = _bits(net.values(boards)) != before[0]
        assert np.array_equal(moved, G.stage(G.boards_for("small5", 257), tiles[:p - 1]) == p - 1), p  # over the active prefix
        net.weights[p - 1] -= 1
    with pytest.raises(ValueError):
        net.promote()


def test_player_through_the_engine(dev):
    """NTupleActionFunction over a staged network with per-stage random weights plays a small BatchRunner batch: every recorded action
    is the restatement's masked argmax on the recorded board, step by step."""
    tuples, tiles, F = G.NETWORKS["small5"]
    net = _network("small5", dev)
    B = 16
    tr = BatchRunner(init_seed=5, act_fn=NTupleActionFunction(net, device=dev), rng_mode="partitionable", device=dev).collect(B)
    actions, ep_len = tr.actions.cpu().numpy().astype(np.int32), tr.ep_len.cpu().numpy()
    recorded = tr.boards.cpu().numpy()
    stages = set()
    for t in range(int(ep_len.max())):
        live = t < ep_len
        q, v, legal = G.scores(recorded[t][live], G.staged_weights("small5"), tuples, F, tiles)
        assert np.array_equal(actions[t][live], N.masked_argmax(q, legal)), t
        assert np.array_equal(tr.values.cpu().numpy()[t][live].view(np.uint32), v.view(np.uint32)), t
        stages |= set(G.stage(recorded[t][live], tiles).tolist())
    assert len(stages) >= 3  # the games crossed thresholds


def test_evaluation_and_distillation_on_a_staged_teacher(dev):
    """``evaluate_ntuple`` (greedy and one ply) and one ``DistillTrainer`` step go through the network's own methods: they run on a
    staged teacher as they are, and the ring holds the staged scores."""
    net = _network("small5", dev)
    a = evaluate_ntuple(net, dev, num_episodes=16, seed=42)
    b = evaluate_ntuple(net, dev, num_episodes=16, seed=42)
    assert a["mean_max_tile"] == b["mean_max_tile"] > 0
    assert evaluate_ntuple(net, dev, num_episodes=8, seed=42, plies=1)["mean_max_tile"] > 0
    torch.manual_seed(0)
    agent = PPOAgent(observation_dim=31, action_dim=4, hidden_dim=64, d_model=64, nhead=2, num_layers=2, dim_feedforward=128, dropout=0.0,
                     reduction="cls")
    tr = DistillTrainer(agent, net, num_envs=64, capacity=128, batch_size=64, seed=3, beta=1.0, device=dev)
    assert tr.collect(2) == 128
    q, _ = net.scores(tr.ring["boards"][:64])
    assert torch.equal(tr.ring["q"][:64], q)
    sums = tr.update(1)
    torch.cuda.synchronize()
    assert tr.updates == 1 and bool(torch.isfinite(sums).all())


def test_the_unstaged_path_is_unchanged(dev):
    """``stage_tiles=None``: [m, 16^L] weights and the bits of ``ntuple_values`` / ``ntuple_scores`` called directly, which are the
    restatement's; a one-stage call of the staged symbol gives them too."""
    net = NTupleNetwork(N.SMALL, device=dev)
    assert tuple(net.weights.shape) == (3, 256) and net.stage_tiles is None and net.active_tiles is None
    net.weights.copy_(_dev(N.small_weights(), dev))
    boards_h = N.boards_for(257)
    boards, cells = _dev(boards_h, dev), N.cells_array(N.SMALL)
    v = torch.empty(257, device=dev)
    nv.ntuple_values(boards, net.weights, cells, 12, v)
    q, qv = torch.empty((257, 4), device=dev), torch.empty(257, device=dev)
    nv.ntuple_scores(boards, net.weights, cells, 12, q, qv)
    got_q, got_v = net.scores(boards)
    assert torch.equal(net.values(boards), v) and torch.equal(got_q, q) and torch.equal(got_v, qv)
    want_q, want_v, _ = N.scores(boards_h, N.small_weights(), N.SMALL, 12)
    assert np.array_equal(_bits(v), N.values(boards_h, N.small_weights(), N.SMALL, 12).view(np.uint32))
    assert np.array_equal(_bits(q), want_q.view(np.uint32)) and np.array_equal(_bits(qv), want_v.view(np.uint32))
    v1 = torch.empty(257, device=dev)
    nv.ntuple_values(boards, net.weights, cells, 12, v1, ())  # no thresholds: n_stages = 1 of the staged symbol
    assert torch.equal(v1, v)
