"""N-tuple budgeted search on the GPU: scores, values, depth_used and entries bit-exact against the numpy reference
(tests/ntuple_budget_ref.py) on its recorded cases, whatever the workspace holds and with guard rows behind every output; against the
fixed-depth device paths at sizes the numpy reference does not reach; byte-identical across calls; across workspace chunks; through
the engine; and reproducible in evaluation."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import ntuple_budget_ref as BR  # noqa: E402
import ntuple_ref as N  # noqa: E402
import ntuple_search_ref as X  # noqa: E402
from src.g2048 import native as nv  # noqa: E402
from src.ppo import NTupleBudgetSearchActionFunction, NTupleNetwork, NTupleTrainer  # noqa: E402
from src.ppo import ntuple as M  # noqa: E402
from src.runs import BatchRunner, evaluate_ntuple, evaluate_ntuple_budget  # noqa: E402

pytestmark = pytest.mark.gpu
SLACK = 259
GUARD = 0xA5A5A5A5
GUARD_F32 = float(np.array([GUARD], np.uint32).view(np.float32)[0])
FILLS = ("nan", 0, 0xFF)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _dev(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # a copy: the shared references are read-only


@pytest.fixture(scope="module")
def tables(dev):
    """network -> (cells, device weights, host tiles or None), uploaded once."""
    out = {}
    for name in BR.NETWORKS:
        tuples, w, _, tiles, _ = BR.network(name)
        out[name] = (N.cells_array(tuples), _dev(w, dev), None if tiles is None else np.array(tiles, np.uint8))
    return out


def _run(dev, boards, cells, w, frac_bits, tiles, max_depth, budget, gamma, fill, outputs=True):
    """One guarded call -> (q bits [B,4], v bits [B], depth_used [B], entries [B,6]); the rows past B of all four outputs and the
    bytes past the workspace's documented size must keep their guard, and the weights their bytes."""
    B = len(boards)
    need = nv.ntuple_budget_search_workspace_bytes(B, max_depth, budget)
    q = torch.full((B + SLACK, 4), GUARD_F32, device=dev)
    v = torch.full((B + SLACK,), GUARD_F32, device=dev)
    used = torch.full((B + SLACK,), 0xEE, dtype=torch.uint8, device=dev)
    entries = torch.full((B + SLACK, 6), -7, dtype=torch.int32, device=dev)
    if fill == "nan":
        ws = torch.full(((need + SLACK + 3) // 4,), float("nan"), device=dev).view(torch.uint8)[:need + SLACK]
    else:
        ws = torch.full((need + SLACK,), fill, dtype=torch.uint8, device=dev)
    ws[need:] = 0x5A
    before = w.clone()
    nv.ntuple_budget_search(_dev(boards, dev), w, cells, frac_bits, max_depth, budget, gamma, ws, q[:B], v[:B],
                            used[:B] if outputs else None, entries[:B] if outputs else None, tiles)
    assert (_bits(q[B:]) == GUARD).all() and (_bits(v[B:]) == GUARD).all()
    assert bool((used[B if outputs else 0:] == 0xEE).all()) and bool((entries[B if outputs else 0:] == -7).all())
    assert bool((ws[need:] == 0x5A).all()) and torch.equal(w, before)
    return _bits(q[:B]), _bits(v[:B]), used[:B].cpu().numpy(), entries[:B].cpu().numpy()


def _check(c, got, gamma, rows=slice(None)):
    q, v, used, entries = got
    legal = c["legal"][rows]
    assert np.array_equal(used, c["depth"][rows]) and np.array_equal(entries, c["entries"][rows]), (used, c["depth"][rows])
    assert np.array_equal(q, c["q"][gamma][rows].view(np.uint32)) and np.array_equal(v, c["v"][gamma][rows].view(np.uint32)), gamma
    assert (q[~legal] == 0).all() and (v[~legal.any(axis=1)] == 0).all()  # +0


@pytest.mark.parametrize("budget", BR.BUDGETS)
@pytest.mark.parametrize("name", BR.NETWORKS)
def test_search_is_bit_exact_whatever_the_workspace_holds(dev, tables, name, budget):
    c = BR.case(name, 4, budget)
    cells, w, tiles = tables[name]
    for gamma, fill in zip(X.GAMMAS + X.GAMMAS[-1:], FILLS):
        _check(c, _run(dev, c["boards"], cells, w, c["frac_bits"], tiles, 4, budget, gamma, fill), gamma)
    # one root alone, and without the two optional outputs
    for i in (0, len(c["boards"]) - 1):
        _check(c, _run(dev, c["boards"][i:i + 1], cells, w, c["frac_bits"], tiles, 4, budget, 0.99, 0xFF), 0.99, slice(i, i + 1))
    q, v, _, _ = _run(dev, c["boards"], cells, w, c["frac_bits"], tiles, 4, budget, 0.99, 0xFF, outputs=False)
    assert np.array_equal(q, c["q"][0.99].view(np.uint32)) and np.array_equal(v, c["v"][0.99].view(np.uint32))


def test_depth_five(dev, tables):
    deep = BR.DEEP
    c = BR.case("small", deep["max_depth"], deep["budget"], deep["boards"])
    assert tuple(c["depth"]) == deep["depth"]
    cells, w, tiles = tables["small"]
    for gamma, fill in zip(X.GAMMAS, FILLS):
        _check(c, _run(dev, c["boards"], cells, w, c["frac_bits"], tiles, deep["max_depth"], deep["budget"], gamma, fill), gamma)


@pytest.fixture(scope="module")
def small_net(dev, tables):
    net = NTupleNetwork(X.network("small")[0], device=dev)
    net.weights.copy_(tables["small"][1])
    return net


@pytest.fixture(scope="module")
def rollout_boards(dev):
    return _dev(N.boards_for(4097, seed=7), dev)


def test_max_depth_three_equals_the_frontier_search_where_the_budget_admits_it(dev, small_net, rollout_boards):
    """4 097 rollout boards, more than the numpy reference covers, at the largest budget: a root searched to depth 3 equals
    search(depth=3) bit for bit; a root that stopped at 2 has more than the budget at level 3 by the reference's count."""
    budget = 24576
    q, v, used, entries = small_net.search_budget(rollout_boards, 3, budget, 0.99, return_depths=True)
    want_q, want_v = small_net.search(rollout_boards, 3, 0.99)
    used_h, entries_h = used.cpu().numpy(), entries.cpu().numpy()
    at3 = used_h == 3
    assert at3.sum() > 4000 and set(np.unique(used_h)) <= {2, 3}
    assert np.array_equal(_bits(q)[at3], _bits(want_q)[at3]) and np.array_equal(_bits(v)[at3], _bits(want_v)[at3])
    assert (entries_h[:, 3:] == 0).all() and (entries_h[at3, :3] <= budget).all() and (entries_h[~at3, 2] == 0).all()
    stopped = np.flatnonzero(~at3)[:8]
    if len(stopped):
        boards = rollout_boards[torch.from_numpy(stopped).to(dev)].cpu().numpy()
        d, e, over = BR.depths(boards, 3, budget, with_over=True)
        assert (d == 2).all() and (over > budget).all() and np.array_equal(e, entries_h[stopped])
        want2 = small_net.expectimax(rollout_boards, 2, 0.99)[0]
        assert np.array_equal(_bits(q)[stopped], _bits(want2)[stopped])
    # two calls give the same bytes in all four outputs
    again = small_net.search_budget(rollout_boards, 3, budget, 0.99, return_depths=True)
    for a, b in zip((q, v, used, entries), again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("max_depth", (1, 2))
def test_max_depth_one_and_two_equal_the_fused_expectimax(dev, small_net, rollout_boards, max_depth):
    want_q, want_v = small_net.expectimax(rollout_boards, max_depth, 0.99)
    q, v, used, entries = small_net.search_budget(rollout_boards, max_depth, 24576, 0.99, return_depths=True)
    assert np.array_equal(_bits(q), _bits(want_q)) and np.array_equal(_bits(v), _bits(want_v))
    assert bool((used == max_depth).all()) and bool((entries[:, max_depth:] == 0).all())  # levels 1 and 2 fit any budget from 480 up
    assert bool((entries[:, 0] <= 4).all()) and bool((entries[:, 1] <= 480).all()) and int(entries[:, 0].max()) == 4


def test_past_one_workspace_chunk(dev, small_net, monkeypatch):
    """The workspace bound set to three roots' worth: 35 roots go through the cached workspace in twelve calls, the last one short, and
    B = chunk + 1 in two."""
    c = BR.case("small", 4, 600)
    monkeypatch.setattr(M, "BUDGET_WORKSPACE_BYTES", nv.ntuple_budget_search_workspace_bytes(3, 4, 600))
    assert M.budget_chunk(4, 600) == 3
    small_net._budget_ws = None
    for B in (len(c["boards"]), 4, 1):
        q, v, used, entries = small_net.search_budget(_dev(c["boards"][:B], dev), 4, 600, 0.99, return_depths=True)
        assert small_net._budget_ws.numel() == nv.ntuple_budget_search_workspace_bytes(3, 4, 600)
        _check(c, (_bits(q), _bits(v), used.cpu().numpy(), entries.cpu().numpy()), 0.99, slice(0, B))
    q, v = small_net.search_budget(_dev(c["boards"], dev), 4, 600, 0.99)
    assert np.array_equal(_bits(q), c["q"][0.99].view(np.uint32))
    empty = small_net.search_budget(_dev(c["boards"][:0], dev), 4, 600, return_depths=True)
    assert [tuple(t.shape) for t in empty] == [(0, 4), (0,), (0,), (0, 6)]
    small_net._budget_ws = None


def test_player_through_the_engine(dev, small_net):
    """BatchRunner with NTupleBudgetSearchActionFunction(max_depth=4, budget=600) on 4 boards to the end of their episodes; on 24
    evenly spaced recorded boards policy_fn equals the reference, the recorded action is its masked argmax (bit-exact scores: no
    near-tie exclusion) and the recorded value its v."""
    tuples, w_host = X.network("small")
    fn = NTupleBudgetSearchActionFunction(small_net, device=dev, max_depth=4, budget=600)
    tr = BatchRunner(init_seed=5, act_fn=fn, rng_mode="partitionable", device=dev).collect(4)
    ep_len = tr.ep_len.cpu().numpy()
    valid = np.arange(tr.T)[:, None] < ep_len[None, :]
    boards = tr.boards.cpu().numpy()[valid]
    actions = tr.actions.cpu().numpy().astype(np.int32)[valid]
    values = tr.values.cpu().numpy()[valid]
    assert len(boards) == ep_len.sum() and len(boards) >= 24
    pick = np.arange(len(boards))[:: len(boards) // 24][:24]
    sel = np.ascontiguousarray(boards[pick])
    q, v, d, _ = BR.search(sel, tuples, w_host, 4, 600, 1.0)
    legal = BR.R.expand(sel)[2] > 0
    assert legal.any(axis=1).all() and len(set(d.tolist())) >= 2
    got_q, got_v = fn.policy_fn(_dev(sel, dev), None)
    assert np.array_equal(_bits(got_q), q.view(np.uint32)) and np.array_equal(_bits(got_v), v.view(np.uint32))
    assert np.array_equal(actions[pick], N.masked_argmax(q, legal))
    assert np.array_equal(values[pick].view(np.uint32), v.view(np.uint32))


def test_evaluation_is_reproducible(dev):
    """The network of test_gpu_ntuple_frontier.py's evaluation test (1 024 envs, 2 400 lock-steps), 32 evaluation episodes (seed 42)
    twice at the defaults: the same histogram and the same mean episode length.  The mean max tile next to depth 3's is printed, not
    asserted."""
    net = NTupleNetwork(device=dev)
    NTupleTrainer(net, num_envs=1024, alpha=0.1, seed=0, device=dev).train(2400)
    a = evaluate_ntuple_budget(net, dev, num_episodes=32, seed=42)
    b = evaluate_ntuple_budget(net, dev, num_episodes=32, seed=42)
    assert a["counts"] == b["counts"] and a["mean_episode_length"] == b["mean_episode_length"]
    three = evaluate_ntuple(net, dev, num_episodes=32, seed=42, depth=3)
    print(f"mean max tile over 32 episodes after 2400 lock-steps of 1024 envs: budget {M.BUDGET_DEFAULT} to depth "
          f"{M.BUDGET_DEFAULT_DEPTH}: {a['mean_max_tile']:.1f}, depth 3: {three['mean_max_tile']:.1f}")
