"""N-tuple searched episodes on the GPU: the persistent kernel bit-exact against the numpy restatement
(tests/ntuple_search_episodes_ref.py), against the engine batch by batch, on the illegal-move edge case, through
``evaluate_ntuple_episodes``, and from one launch to the next."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import ntuple_ref as N  # noqa: E402
import ntuple_search_episodes_ref as S  # noqa: E402
from src.g2048 import native as nv  # noqa: E402
from src.ppo import NTupleActionFunction, NTupleNetwork, NTupleTrainer  # noqa: E402
from src.runs import BatchRunner, evaluate_ntuple, evaluate_ntuple_episodes  # noqa: E402

pytestmark = pytest.mark.gpu
SLACK = 259
GUARD = 0xA5
SIZES = S.SIZES + ((2, 2), (5, 5))  # one workgroup per game: N = 1, 2 and 5 are the grid's small ends
STEPS = (1, 7, 4096)
STATE = ("boards", "masks", "ep_len", "score", "chain")


def _dev(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # a copy: the shared references are read-only


@pytest.fixture(scope="module")
def tables(dev):
    """name -> (cells, device weights, frac_bits, stage thresholds or None), uploaded once."""
    out = {}
    for name in S.NETWORKS + ("floor",):
        tuples, w, F, tiles = S.network(name)
        out[name] = (N.cells_array(tuples), _dev(w, dev), F, None if tiles is None else np.array(tiles, np.uint8))
    return out


class Games:
    """The kernel's state arrays with SLACK guard rows past N; ``view`` is what the entry point is given."""

    def __init__(self, dev, n, bs):
        self.n, rows = n, n + SLACK
        self.full = dict(chain=torch.full((rows, 2), GUARD, dtype=nv.KEY_DTYPE, device=dev),
                         boards=torch.full((rows, 16), GUARD, dtype=torch.uint8, device=dev),
                         masks=torch.full((rows,), GUARD, dtype=torch.uint8, device=dev),
                         done=torch.full((rows,), GUARD, dtype=torch.uint8, device=dev),
                         ep_len=torch.full((rows,), GUARD, dtype=torch.int32, device=dev),
                         score=torch.full((rows,), GUARD, dtype=torch.int64, device=dev))
        self.full["chain"][:n] = nv.keys_from_numpy(S.chain_heads(n, bs), dev)
        self.view = {k: v[:n] for k, v in self.full.items()}
        self.live = torch.zeros(1, dtype=torch.int32, device=dev)

    def launch(self, table, bs, mode, gamma, start, n_steps):
        cells, w, F, tiles = table
        v = self.view
        self.live.zero_()
        nv.ntuple_search_episodes(start, n_steps, bs, w, cells, F, 1, gamma, v["chain"], v["boards"], v["masks"], v["done"], v["ep_len"],
                                  v["score"], mode, self.live, tiles)
        return int(self.live.item())

    def play(self, table, bs, mode, gamma, n_steps, max_launches=1 << 12):
        live, launches = self.launch(table, bs, mode, gamma, True, n_steps), 1
        while live and launches < max_launches:
            live, launches = self.launch(table, bs, mode, gamma, False, n_steps), launches + 1
        assert live == 0
        return launches

    def host(self):
        out = {k: v.cpu().numpy() for k, v in self.view.items()}
        out["chain"] = out["chain"].view(np.uint32)
        return out

    def guards_kept(self):
        return all(bool((v[self.n:] == GUARD).all()) for v in self.full.values())


def _same(got, ref):
    return all(np.array_equal(got[k], ref[k]) for k in STATE) and (got["done"] == 1).all()


@pytest.mark.parametrize("gamma", S.GAMMAS)
@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("name", S.NETWORKS)
def test_kernel_equals_the_restatement(dev, tables, name, mode, gamma):
    """Every size at 1, 7 and 4 096 steps per launch, guard rows past N on all six state arrays, the weights compared before and after."""
    w_before = tables[name][1].clone()
    for n, bs in SIZES:
        ref = S.case(name, mode, gamma, n, bs)
        for n_steps in STEPS:
            g = Games(dev, n, bs)
            launches = g.play(tables[name], bs, mode, gamma, n_steps)
            assert _same(g.host(), ref), (n, bs, n_steps)
            assert g.guards_kept(), (n, bs, n_steps)
            assert launches == -(-int(ref["ep_len"].max()) // n_steps)
    assert torch.equal(tables[name][1], w_before)


def _network(dev, tables, name):
    tuples, _, F, tiles = S.network(name)
    net = NTupleNetwork(tuples, frac_bits=F, device=dev, stage_tiles=tiles)
    net.weights.copy_(tables[name][1].view(net.weights.shape))
    net.active_stages = net.stages
    return net


def _engine(dev, net, mode, gamma, n, bs, seed=S.SEED):
    """The evaluation protocol batch by batch through the engine -> final boards, lengths, int64 sums of the live steps' rewards."""
    fn = NTupleActionFunction(net, device=dev, rng_mode=mode, plies=1, gamma=gamma)
    boards, lens, scores = [], [], []
    for first in range(0, n, bs):
        tr = BatchRunner(seed + first, fn, rng_mode=mode, device=dev).collect(min(bs, n - first))
        boards.append(tr.final_boards.cpu().numpy())
        lens.append(tr.ep_len.cpu().numpy())
        scores.append((tr.rewards.to(torch.int64) * tr.valid()).sum(dim=0).cpu().numpy())
    return np.concatenate(boards), np.concatenate(lens), np.concatenate(scores)


@pytest.mark.parametrize("gamma", S.GAMMAS)
@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("name", S.NETWORKS)
def test_kernel_equals_the_engine(dev, tables, name, mode, gamma):
    n, bs = 23, 10
    net = _network(dev, tables, name)
    boards, ep_len, score = net.play_search_episodes(n, S.SEED, bs, mode, plies=1, gamma=gamma)
    want = _engine(dev, net, mode, gamma, n, bs)
    assert np.array_equal(boards.cpu().numpy(), want[0])
    assert np.array_equal(ep_len.cpu().numpy(), want[1]) and ep_len.dtype == torch.int32
    assert np.array_equal(score.cpu().numpy(), want[2]) and score.dtype == torch.int64


@pytest.mark.parametrize("mode", S.MODES)
def test_scores_below_the_mask_penalty_play_the_engines_illegal_move(dev, tables, mode):
    """The edge case of tests/test_ntuple_search_episodes_abi.py (frac_bits 0, every weight INT32_MIN) against the engine and the
    restatement: every game ends by an illegal move, reward -1, with the spawn env_step still applies."""
    n, bs, gamma = 30, 10, 1.0
    ref = S.case("floor", mode, gamma, n, bs)
    assert ref["illegal"].all() and (ref["ep_len"] == 1).any() and (ref["ep_len"] > 1).any()
    net = _network(dev, tables, "floor")
    for steps in (1, None):
        boards, ep_len, score = net.play_search_episodes(n, S.SEED, bs, mode, steps_per_launch=steps, plies=1, gamma=gamma)
        assert np.array_equal(boards.cpu().numpy(), ref["boards"]) and np.array_equal(ep_len.cpu().numpy(), ref["ep_len"])
        assert np.array_equal(score.cpu().numpy(), ref["score"])
    want = _engine(dev, net, mode, gamma, n, bs)
    assert np.array_equal(want[0], ref["boards"]) and np.array_equal(want[1], ref["ep_len"]) and np.array_equal(want[2], ref["score"])


@pytest.mark.parametrize("staged", (False, True), ids=("unstaged", "staged"))
def test_fused_evaluation_equals_the_lock_step_evaluation(dev, staged):
    """The default tuples after 300 lock-steps of NTupleTrainer at 1 024 envs (games of a few hundred moves); the staged network has
    split its second stage off by then."""
    net = NTupleNetwork(device=dev, stage_tiles=(6,) if staged else None)
    trainer = NTupleTrainer(net, num_envs=1024, alpha=0.1, seed=0, device=dev)
    trainer.train(300)
    del trainer
    if staged:
        assert net.active_stages == 2
    w = net.weights.clone()
    plain = evaluate_ntuple(net, dev, 230, plies=1)
    fused = evaluate_ntuple_episodes(net, 230, plies=1)
    assert set(fused) == set(plain) | {"mean_score"}
    for k in plain:
        assert fused[k] == plain[k], k
    assert fused["mean_episode_length"] > 100 and fused["mean_score"] > 0
    assert evaluate_ntuple_episodes(net, 230, plies=1) == fused
    assert fused != evaluate_ntuple_episodes(net, 230)  # the greedy games are other games
    assert torch.equal(net.weights, w)
    if staged:
        assert max(fused["counts"]) >= 64  # games reach the threshold: both stages are looked up


@pytest.mark.parametrize("mode", S.MODES)
def test_start_and_continue(dev, tables, mode):
    """50 launches of one step, 10 of seven (some games end inside those, some after them), then launches of 4 096, equal the one-shot
    result; a launch on the finished state changes nothing and leaves live_count at 0."""
    n, bs, name, gamma = 23, 10, "small", 0.99
    ref = S.case(name, mode, gamma, n, bs)
    assert ref["ep_len"].min() < 120 < ref["ep_len"].max()
    one = Games(dev, n, bs)
    assert one.play(tables[name], bs, mode, gamma, 4096) == 1
    g = Games(dev, n, bs)
    live = g.launch(tables[name], bs, mode, gamma, True, 1)
    for _ in range(49):
        live = g.launch(tables[name], bs, mode, gamma, False, 1)
    assert live == int((ref["ep_len"] > 50).sum())
    for _ in range(10):
        live = g.launch(tables[name], bs, mode, gamma, False, 7)
    assert live == int((ref["ep_len"] > 120).sum())
    while live:
        live = g.launch(tables[name], bs, mode, gamma, False, 4096)
    a, b = g.host(), one.host()
    assert all(np.array_equal(a[k], b[k]) for k in a) and _same(a, ref)
    assert g.launch(tables[name], bs, mode, gamma, False, 4096) == 0
    c = g.host()
    assert all(np.array_equal(a[k], c[k]) for k in a) and g.guards_kept()


def test_no_plies_are_the_greedy_episodes(dev, tables):
    net = _network(dev, tables, "small")
    a = net.play_episodes(23, S.SEED, 10)
    b = net.play_search_episodes(23, S.SEED, 10, plies=0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert evaluate_ntuple_episodes(net, 23) == evaluate_ntuple(net, dev, 23, fused=True)
