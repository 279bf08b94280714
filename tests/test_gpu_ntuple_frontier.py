"""N-tuple frontier search on the GPU: depths 1, 2 and 3 bit-exact against the numpy composition (tests/ntuple_frontier_ref.py) with
its level counts, against the fused and the composed device paths at sizes the numpy reference does not reach, on a multi-stage
network, across workspace chunks, through the engine, and reproducible in evaluation."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import ntuple_frontier_ref as FR  # noqa: E402
import ntuple_ref as N  # noqa: E402
import ntuple_search_ref as X  # noqa: E402
import ntuple_stage_ref as ST  # noqa: E402
from src.g2048 import native as nv  # noqa: E402
from src.ppo import NTupleNetwork, NTupleSearchActionFunction, NTupleTrainer  # noqa: E402
from src.ppo.lookahead import expand_level, spawn_children  # noqa: E402
from src.runs import BatchRunner, evaluate_ntuple  # noqa: E402

pytestmark = pytest.mark.gpu
SLACK = 259
GUARD = 0xA5A5A5A5
GUARD_F32 = float(np.array([GUARD], np.uint32).view(np.float32)[0])
SHAPES = ("small", "wide", "eight")


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _dev(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # a copy: the shared references are read-only


@pytest.fixture(scope="module")
def tables(dev):
    """shape -> (cells, device weights), uploaded once."""
    return {s: (N.cells_array(X.network(s)[0]), _dev(X.network(s)[1], dev)) for s in SHAPES}


def _run(dev, boards, cells, w, depth, gamma, dedup, fill, stage_tiles=None, frac_bits=X.FRAC_BITS):
    """One guarded call -> (q bits [B,4], v bits [B], counts [3]); the rows past B of both outputs and the bytes past the workspace's
    documented size must keep their guard."""
    B = len(boards)
    need = nv.ntuple_search_workspace_bytes(B, depth)
    q = torch.full((B + SLACK, 4), GUARD_F32, device=dev)
    v = torch.full((B + SLACK,), GUARD_F32, device=dev)
    ws = torch.full((need + SLACK,), fill, dtype=torch.uint8, device=dev)
    ws[need:] = 0x5A
    counts = torch.full((3 + SLACK,), -7, dtype=torch.int32, device=dev)
    nv.ntuple_search(_dev(boards, dev), w, cells, frac_bits, depth, gamma, dedup, ws, q[:B], v[:B], counts[:3], stage_tiles)
    assert (_bits(q[B:]) == GUARD).all() and (_bits(v[B:]) == GUARD).all()
    assert bool((ws[need:] == 0x5A).all()) and bool((counts[3:] == -7).all())
    return _bits(q[:B]), _bits(v[:B]), counts[:3].cpu().numpy()


def _want_counts(c, boards, depth, dedup, tuples):
    """The reference's counts of the first rows of a case: the case's own for all rows, else computed for the prefix."""
    if len(boards) == len(c["boards"]):
        return c["counts"][dedup]
    if not dedup:
        return FR.plain_counts(boards, depth)
    return FR.search(boards, tuples, c["weights"], depth, 1.0, True)[2]


@pytest.mark.parametrize("dedup", (True, False))
@pytest.mark.parametrize("B", (1, 2, None))
@pytest.mark.parametrize("depth", FR.DEPTHS)
@pytest.mark.parametrize("shape", SHAPES)
def test_search_is_bit_exact_whatever_the_workspace_holds(dev, tables, shape, depth, B, dedup):
    c = FR.case(shape, depth)
    X.check_inputs(c["boards"], c["legal"], c["nchild"])
    B = len(c["boards"]) if B is None else B
    boards, legal = c["boards"][:B], c["legal"][:B]
    cells, w = tables[shape]
    want = _want_counts(c, boards, depth, dedup, c["tuples"])
    for gamma in X.GAMMAS:
        q, v, counts = _run(dev, boards, cells, w, depth, gamma, dedup, 0xFF)  # every f32 a NaN, every index -1
        assert np.array_equal(q, c["q"][gamma][:B].view(np.uint32)), gamma
        assert np.array_equal(v, c["v"][gamma][:B].view(np.uint32)), gamma
        assert (q[~legal] == 0).all() and (v[~legal.any(axis=1)] == 0).all()  # +0
        assert np.array_equal(counts, want), (counts, want)
    q0, v0, counts0 = _run(dev, boards, cells, w, depth, X.GAMMAS[-1], dedup, 0)
    assert np.array_equal(q0, q) and np.array_equal(v0, v) and np.array_equal(counts0, want)


@pytest.mark.parametrize("dedup", (True, False))
@pytest.mark.parametrize("depth", (1, 2))
def test_depth_one_and_two_equal_the_fused_expectimax(dev, tables, depth, dedup):
    """4 097 rollout boards, more than the numpy reference covers: the frontier search against g2048_ntuple_expectimax."""
    cells, w = tables["small"]
    B = 4097
    boards = _dev(N.boards_for(B, seed=7), dev)
    want_q, want_v = torch.empty((B, 4), device=dev), torch.empty(B, device=dev)
    ws = torch.empty(max(1, nv.ntuple_expectimax_workspace_floats(B, depth)), device=dev)
    nv.ntuple_expectimax(boards, w, cells, X.FRAC_BITS, depth, 0.99, ws, want_q, want_v)
    q, v, counts = _run(dev, boards.cpu().numpy(), cells, w, depth, 0.99, dedup, 0xFF)
    assert np.array_equal(q, _bits(want_q)) and np.array_equal(v, _bits(want_v))
    assert counts[depth - 1] > 0 and (counts[depth:] == 0).all()


def test_depth_three_equals_the_composed_device_path(dev, tables):
    """64 rollout boards: expand -> spawn children -> two fused plies on every child -> g2048_lookahead_reduce."""
    tuples, _ = X.network("small")
    cells, w = tables["small"]
    net = NTupleNetwork(tuples, device=dev)
    net.weights.copy_(w)
    boards = _dev(N.boards_for(64, seed=9), dev)
    after, reward, nchild, offset, incl = expand_level(boards)
    n = int(incl[-1].item())
    children, terminal = spawn_children(after, nchild, offset, n)
    v2 = net.expectimax(children, 2, 0.99)[1]
    want = torch.empty_like(reward)
    nv.lookahead_reduce(reward, nchild, offset, v2, terminal, 0.99, n, want)
    for dedup in (True, False):
        q, v, counts = net.search(boards, 3, 0.99, dedup, return_counts=True)
        assert np.array_equal(_bits(q), _bits(want)), dedup
        assert np.array_equal(_bits(v), _bits(net.search(boards, 3, 0.99, not dedup)[1]))
        assert (counts > 0).all()


@pytest.mark.parametrize("depth", (2, 3))
@pytest.mark.parametrize("active", (2, 5))
def test_multi_stage_network(dev, depth, active):
    """"small5" (thresholds 2, 5, 9, 12) with one and with all thresholds active, on the threshold boards: every leaf in its stage."""
    tuples, tiles, F = ST.NETWORKS["small5"]
    w = ST.staged_weights("small5")
    net = NTupleNetwork(tuples, frac_bits=F, device=dev, stage_tiles=tiles)
    net.weights.copy_(_dev(w, dev))
    net.active_stages = active
    boards = np.ascontiguousarray(ST.threshold_boards(tiles))
    seen = set()
    ST.scores(boards, w, tuples, F, tiles[:active - 1], seen)
    assert len(seen) >= 2
    want_q, want_v, want_counts = FR.search(boards, tuples, w, depth, 0.99, True, tiles=tiles[:active - 1], frac_bits=F)
    q, v, counts = net.search(_dev(boards, dev), depth, 0.99, True, return_counts=True)
    assert np.array_equal(_bits(q), want_q.view(np.uint32)) and np.array_equal(_bits(v), want_v.view(np.uint32))
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    unstaged = FR.search(boards, tuples, w[0], depth, 0.99, True, frac_bits=F)[0]
    assert (unstaged.view(np.uint32) != want_q.view(np.uint32)).any()  # the stages reach the result


def test_depth_three_past_one_workspace_chunk(dev, tables):
    """One root more than a depth-3 chunk goes through the cached workspace in two calls: row i equals the reference of the board it
    repeats, and the counts are those of the rows."""
    from src.ppo.ntuple import FRONTIER_CHUNK

    c = FR.case("small", 3)
    net = NTupleNetwork(c["tuples"], device=dev)
    net.weights.copy_(tables["small"][1])
    n, B = len(c["boards"]), FRONTIER_CHUNK[3] + 1
    rows = np.arange(B) % n
    q, v, counts = net.search(_dev(c["boards"][rows], dev), 3, 0.99, return_counts=True)
    assert net._frontier_ws.numel() == nv.ntuple_search_workspace_bytes(FRONTIER_CHUNK[3], 3)
    assert np.array_equal(_bits(q), c["q"][0.99][rows].view(np.uint32)) and np.array_equal(_bits(v), c["v"][0.99][rows].view(np.uint32))
    full, rest = divmod(B, n)
    per_root = [FR.search(c["boards"][i:i + 1], c["tuples"], c["weights"], 3, 1.0, True)[2] for i in range(rest)]
    assert np.array_equal(counts.cpu().numpy(), full * c["counts"][True] + sum(per_root))
    empty = net.search(_dev(c["boards"][:0], dev), 3, return_counts=True)
    assert empty[0].shape == (0, 4) and empty[1].shape == (0,) and empty[2].tolist() == [0, 0, 0]


def test_player_through_the_engine(dev, tables):
    """BatchRunner with NTupleSearchActionFunction(depth=3) on 4 boards to the end of their episodes; on 24 evenly spaced recorded
    boards policy_fn equals the reference, the recorded action is its masked argmax (bit-exact scores: no near-tie exclusion) and the
    recorded value its v."""
    tuples, w_host = X.network("small")
    net = NTupleNetwork(tuples, device=dev)
    net.weights.copy_(tables["small"][1])
    fn = NTupleSearchActionFunction(net, device=dev, depth=3)
    tr = BatchRunner(init_seed=5, act_fn=fn, rng_mode="partitionable", device=dev).collect(4)
    ep_len = tr.ep_len.cpu().numpy()
    valid = np.arange(tr.T)[:, None] < ep_len[None, :]
    boards = tr.boards.cpu().numpy()[valid]
    actions = tr.actions.cpu().numpy().astype(np.int32)[valid]
    values = tr.values.cpu().numpy()[valid]
    assert len(boards) == ep_len.sum() and len(boards) >= 24
    pick = np.arange(len(boards))[:: len(boards) // 24][:24]
    sel = np.ascontiguousarray(boards[pick])
    q, v, _ = FR.search(sel, tuples, w_host, 3, 1.0, True)
    legal = FR.R.expand(sel)[2] > 0
    assert legal.any(axis=1).all()
    got_q, got_v = fn.policy_fn(_dev(sel, dev), None)
    assert np.array_equal(_bits(got_q), q.view(np.uint32)) and np.array_equal(_bits(got_v), v.view(np.uint32))
    assert np.array_equal(actions[pick], N.masked_argmax(q, legal))
    assert np.array_equal(values[pick].view(np.uint32), v.view(np.uint32))


def test_evaluation_is_reproducible_at_depth_three(dev):
    """The network of test_evaluation_is_reproducible_at_every_depth (1 024 envs, 2 400 lock-steps), 32 evaluation episodes (seed 42)
    twice at depth 3: the same histogram and the same mean episode length.  The mean max tile at depth 3 and at plies 2 is printed,
    not asserted."""
    net = NTupleNetwork(device=dev)
    NTupleTrainer(net, num_envs=1024, alpha=0.1, seed=0, device=dev).train(2400)
    a = evaluate_ntuple(net, dev, num_episodes=32, seed=42, depth=3)
    b = evaluate_ntuple(net, dev, num_episodes=32, seed=42, depth=3)
    assert a["counts"] == b["counts"] and a["mean_episode_length"] == b["mean_episode_length"]
    two = evaluate_ntuple(net, dev, num_episodes=32, seed=42, plies=2)
    print(f"mean max tile over 32 episodes after 2400 lock-steps of 1024 envs: depth 3: {a['mean_max_tile']:.1f}, plies 2: {two['mean_max_tile']:.1f}")
