"""N-tuple network on the GPU: values, scores, one TD step, the link and a whole training run bit-exact against the numpy
restatement (tests/ntuple_ref.py); the player through the engine; and that TD(0) learns."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import ntuple_ref as N  # noqa: E402
from oracle import g2048_oracle as npo  # noqa: E402
from src.g2048 import native as nv  # noqa: E402
from src.ppo import NTupleActionFunction, NTupleNetwork, NTupleTrainer  # noqa: E402
from src.runs import BatchRunner, evaluate_ntuple  # noqa: E402

pytestmark = pytest.mark.gpu
SLACK = 259
GUARD = 0xA5A5A5A5
GUARD_F32 = float(np.array([GUARD], np.uint32).view(np.float32)[0])
SIZES = (1, 63, 64, 65, 257)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _f32(a, dev):
    return _dev(np.asarray(a, np.float32).view(np.int32), dev).view(torch.float32)


@pytest.fixture(scope="module")
def tables(dev):
    """(tuples, cells, device weights, host weights) of the two shapes the kernel tests use."""
    return {name: (tuples, N.cells_array(tuples), _dev(w, dev), w)
            for name, tuples, w in (("small", N.SMALL, N.small_weights()), ("wide", N.WIDE, N.wide_weights()))}


@pytest.fixture(scope="module")
def expected():
    """The restatement on the 257 test boards, computed once per shape; a run on B boards is checked against its first B rows."""
    boards = N.boards_for(max(SIZES), seed=3)
    out = {"boards": boards}
    for name, tuples, w in (("small", N.SMALL, N.small_weights()), ("wide", N.WIDE, N.wide_weights())):
        q, v, legal = N.scores(boards, w, tuples, 12)
        out[name] = dict(q=q, v=v, legal=legal, val=N.values(boards, w, tuples, 12))
    return out


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("shape", ["small", "wide"])
def test_values_and_scores_are_bit_exact(dev, tables, expected, shape, B):
    tuples, cells, w, _ = tables[shape]
    want = expected[shape]
    boards = _dev(expected["boards"][:B], dev)
    val = torch.full((B + SLACK,), GUARD_F32, device=dev)
    q = torch.full((B + SLACK, 4), GUARD_F32, device=dev)
    v = torch.full((B + SLACK,), GUARD_F32, device=dev)
    nv.ntuple_values(boards, w, cells, 12, val[:B])
    nv.ntuple_scores(boards, w, cells, 12, q[:B], v[:B])
    assert np.array_equal(_bits(val[:B]), want["val"][:B].view(np.uint32))
    assert np.array_equal(_bits(q[:B]), want["q"][:B].view(np.uint32))
    assert np.array_equal(_bits(v[:B]), want["v"][:B].view(np.uint32))
    assert (_bits(val[B:]) == GUARD).all() and (_bits(q[B:]) == GUARD).all() and (_bits(v[B:]) == GUARD).all()
    legal = want["legal"][:B]
    assert (_bits(q[:B])[~legal] == 0).all()  # +0 at illegal moves
    if B >= 9:
        assert expected["boards"][:B].max() == 17 and (~legal.any(axis=1)).any() and (_bits(v[:B])[~legal.any(axis=1)] == 0).all()


def _td_step(dev, prev, flag, target, w, cells, F, alpha):
    """accumulate + apply on fresh acc / cnt, in place on the device weights w -> (td_error bits, acc, cnt)."""
    B = len(flag)
    acc, cnt = torch.zeros(w.shape, dtype=torch.int64, device=dev), torch.zeros(w.shape, dtype=torch.int32, device=dev)
    err = torch.full((B + SLACK,), GUARD_F32, device=dev)
    t_prev, t_flag, t_target = _dev(prev, dev), _dev(flag, dev), _f32(target, dev)
    nv.ntuple_td_accumulate(t_prev, t_flag, t_target, w, cells, F, alpha, acc, cnt, err[:B])
    hits = int(cnt.sum().item())
    nv.ntuple_td_apply(t_prev, t_flag, cells, w, acc, cnt)
    assert hits == 8 * cells.shape[0] * int((flag != 0).sum())
    assert (_bits(err[B:]) == GUARD).all()
    return _bits(err[:B]), acc, cnt


def test_td_step_under_heavy_collision(dev):
    c = N.collision_case()
    cells = N.cells_array(N.SMALL)
    assert len(c["flag"]) == 1000 and set(c["flag"].tolist()) == {0, 1, 2}
    assert np.unique(c["prev"], axis=0, return_counts=True)[1].max() >= 300  # 300 of the boards are identical
    w = _dev(N.small_weights(), dev)
    err, acc, cnt = _td_step(dev, c["prev"], c["flag"], c["target"], w, cells, 12, 0.1)
    assert np.array_equal(w.cpu().numpy(), c["weights_after"])
    assert np.array_equal(err, c["td_error"].view(np.uint32))
    assert not acc.any() and not cnt.any()
    # the same boards in another order: the sums are order-free
    perm = np.random.default_rng(1).permutation(1000)
    w2 = _dev(N.small_weights(), dev)
    err2, acc2, cnt2 = _td_step(dev, c["prev"][perm], c["flag"][perm], c["target"][perm], w2, cells, 12, 0.1)
    assert torch.equal(w2, w) and np.array_equal(err2, err[perm]) and not acc2.any() and not cnt2.any()
    # accumulate without td_error
    w3 = _dev(N.small_weights(), dev)
    acc3, cnt3 = torch.zeros(w3.shape, dtype=torch.int64, device=dev), torch.zeros(w3.shape, dtype=torch.int32, device=dev)
    t_prev, t_flag = _dev(c["prev"], dev), _dev(c["flag"], dev)
    nv.ntuple_td_accumulate(t_prev, t_flag, _f32(c["target"], dev), w3, cells, 12, 0.1, acc3, cnt3, None)
    assert torch.equal(w3, _dev(N.small_weights(), dev))  # weights are only read in this launch
    nv.ntuple_td_apply(t_prev, t_flag, cells, w3, acc3, cnt3)
    assert torch.equal(w3, w)


def test_td_step_on_wide_tables(dev, tables):
    _, cells, w_shared, w_host = tables["wide"]
    rng = np.random.default_rng(11)
    prev = N.boards_for(65, seed=12)
    flag = rng.integers(0, 3, 65).astype(np.uint8)
    flag[:9] = [1, 2, 1, 2, 1, 2, 1, 2, 1]  # the special boards take part
    target = (rng.standard_normal(65) * 800).astype(np.float32)
    want = w_host.copy()
    want_err = N.td_step(prev, flag, target, want, N.WIDE, 12, 0.1)
    w = w_shared.clone()
    err, acc, cnt = _td_step(dev, prev, flag, target, w, cells, 12, 0.1)
    assert torch.equal(w, _dev(want, dev)) and np.array_equal(err, want_err.view(np.uint32))
    assert not acc.any() and not cnt.any()
    assert not torch.equal(w, w_shared)


def test_td_step_saturates_and_clamps(dev):
    """Weights near +-2^31 saturate; targets of 1e9 with alpha = 1000 put delta on the +-2^30 clamp."""
    cells, rng = N.cells_array(N.SMALL), np.random.default_rng(3)
    prev = N.boards_for(200, seed=4)
    flag = rng.integers(0, 3, 200).astype(np.uint8)
    target = (rng.standard_normal(200) * 1e9).astype(np.float32)
    w0 = N.random_weights(N.SMALL, seed=8)
    w0[:, ::3] = 2 ** 31 - 1 - rng.integers(0, 50, w0[:, ::3].shape)
    w0[:, 1::3] = -2 ** 31 + rng.integers(0, 50, w0[:, 1::3].shape)
    delta, _ = N.td_deltas(prev, flag, target, w0, N.SMALL, 12, 1000.0)
    assert (np.abs(delta) == 2 ** 30).any()
    want = w0.copy()
    want_err = N.td_step(prev, flag, target, want, N.SMALL, 12, 1000.0)
    assert (want == 2 ** 31 - 1).any() and (want == -2 ** 31).any()
    w = _dev(w0, dev)
    err, acc, cnt = _td_step(dev, prev, flag, target, w, cells, 12, 1000.0)
    assert np.array_equal(w.cpu().numpy(), want) and np.array_equal(err, want_err.view(np.uint32)) and not acc.any() and not cnt.any()


def test_link(dev):
    """Every action, the done bit set and cleared, rows where the move merges; rows past B untouched."""
    merge = np.array([[1, 1, 2, 2], [3, 0, 3, 0], [0, 0, 0, 0], [4, 4, 4, 4]], np.uint8).reshape(-1)
    base = np.concatenate([merge[None], N.boards_for(40, seed=2)])
    boards = np.repeat(base, 8, axis=0)  # every board under every (action, done) pair
    meta = np.tile(np.arange(8, dtype=np.uint8), len(base))
    meta = ((meta & 3) | (0xB << 2) | ((meta >> 2) << 6)).astype(np.uint8)
    B = len(boards)
    prev = torch.full((B + SLACK, 16), 0xA5, dtype=torch.uint8, device=dev)
    flag = torch.full((B + SLACK,), 0xA5, dtype=torch.uint8, device=dev)
    nv.ntuple_link(_dev(boards, dev), _dev(meta, dev), prev[:B], flag[:B])
    want_prev, want_flag = N.link(boards, meta)
    assert np.array_equal(prev[:B].cpu().numpy(), want_prev) and np.array_equal(flag[:B].cpu().numpy(), want_flag)
    assert (prev[B:] == 0xA5).all() and (flag[B:] == 0xA5).all()
    assert want_prev[0].reshape(4, 4)[0].tolist() == [2, 3, 0, 0] and want_prev[2].reshape(4, 4)[3].tolist() == [0, 0, 5, 5]
    assert want_flag[:8].tolist() == [1, 1, 1, 1, 2, 2, 2, 2]


REPLAY_TUPLES = ((0, 1, 2), (4, 5, 6))


def test_trainer_replay(dev):
    """NTupleTrainer(num_envs=192, m=2 L=3, alpha=0.1).train(48, record=True): the restatement, fed the recorded boards and meta
    rows, reproduces the scores and targets of every step and the final weights bit for bit.  The network starts from
    ``crowding_weights`` so that episodes end inside 48 lock-steps: on the CPU (``ntuple_ref.engine_training``, the C oracle's env
    on the engine's key chain) seed 0 ends 22 episodes, seeds 1 and 2 end 24 and 20; an all-zero start ends none."""
    net = NTupleNetwork(REPLAY_TUPLES, device=dev)
    start = N.crowding_weights(REPLAY_TUPLES)
    net.weights.copy_(_dev(start, dev))
    trainer = NTupleTrainer(net, num_envs=192, alpha=0.1, seed=0, rng_mode=npo.MODE_PARTITIONABLE, device=dev)
    out = trainer.train(48, record=True)
    boards, meta = out["boards"].cpu().numpy(), out["meta"].cpu().numpy()
    ends = int(((meta >> 6) & 1).sum())
    assert ends >= 1 and int(out["episodes"].item()) == ends
    w = start.copy()
    want_q, want_v = N.replay_training(w, REPLAY_TUPLES, boards, meta, alpha=0.1, frac_bits=12)
    assert np.array_equal(_bits(out["scores"]), want_q.view(np.uint32))
    assert np.array_equal(_bits(out["targets"]), want_v.view(np.uint32))
    assert np.array_equal(net.weights.cpu().numpy(), w) and (w != start).any()
    assert not trainer.acc.any() and not trainer.cnt.any()
    # every recorded action is the masked argmax of the recorded scores, and the env is the oracle's on the engine's key chain
    legal = ((meta[..., None] >> (2 + np.arange(4))) & 1).astype(bool)
    for t in range(48):
        assert np.array_equal(meta[t] & 3, N.masked_argmax(want_q[t], legal[t])), t
    ref_w = start.copy()
    ref = N.engine_training(ref_w, REPLAY_TUPLES, 192, 48, alpha=0.1, frac_bits=12, seed=0)
    assert np.array_equal(ref["boards"], boards) and np.array_equal(ref["meta"], meta) and np.array_equal(ref_w, w)
    assert float(out["td_sq_sum"].item()) > 0


def test_player_through_the_engine(dev, tables):
    """BatchRunner.collect(64) with a random-weights network: every recorded action is the masked argmax of the restatement's scores
    on the recorded board, and an oracle replay of the recorded actions reproduces boards, rewards and episode lengths."""
    tuples, _, w, w_host = tables["small"]
    net = NTupleNetwork(tuples, device=dev)
    net.weights.copy_(w)
    fn = NTupleActionFunction(net, device=dev)
    B, seed = 64, 5
    tr = BatchRunner(init_seed=seed, act_fn=fn, rng_mode="partitionable", device=dev).collect(B)
    actions = tr.actions.cpu().numpy().astype(np.int32)
    ep_len = tr.ep_len.cpu().numpy()
    step = iter(range(tr.T))
    replay = npo.Runner(seed, 1).run(B, "callable", policy_fn=lambda k, b, m: (actions[next(step)], np.zeros(B, np.float32),
                                                                               np.zeros(B, np.float32)))
    rb, rr, rt = (np.swapaxes(replay[k], 0, 1) for k in ("boards", "rewards", "terms"))
    To = rb.shape[0]
    assert To == ep_len.max() and To <= tr.T < To + 8
    valid = (np.arange(tr.T)[:, None] < ep_len[None, :])[:To]
    assert np.array_equal(tr.boards.cpu().numpy()[:To][valid], rb[valid])
    assert np.array_equal(tr.rewards.cpu().numpy()[:To][valid].view(np.uint32), rr[valid].view(np.uint32))
    assert np.array_equal(ep_len, rt.argmax(axis=0) + 1) and np.array_equal(tr.final_boards.cpu().numpy(), replay["final_boards"])
    boards = rb[valid]
    q, v, legal = N.scores(boards, w_host, tuples, 12)
    assert legal.any(axis=1).all()
    assert np.array_equal(actions[:To][valid], N.masked_argmax(q, legal))
    assert np.array_equal(tr.values.cpu().numpy()[:To][valid].view(np.uint32), v.view(np.uint32))


def test_it_learns(dev):
    """The default network, 1 024 envs, 2 400 lock-steps of TD(0), then 100 evaluation episodes (seed 42) against an all-zero network
    on the same seeds (greedy on the immediate merge reward): trained mean max tile >= 2 x the zero network's.
    The restatement's own loop on the CPU at this size (``ntuple_ref.simulate_training`` / ``simulate_evaluation``, numpy's RNG for
    the spawns, 100 evaluation episodes): zero network 226.6; after 800 lock-steps 619.5, a ratio of 2.73, below the 3 that the
    factor 2 wants as a margin, hence the longer run; after 2 400 lock-steps 852.5, a ratio of 3.76."""
    net = NTupleNetwork(device=dev)
    zero = evaluate_ntuple(net, dev, num_episodes=100, seed=42)
    out = NTupleTrainer(net, num_envs=1024, alpha=0.1, seed=0, device=dev).train(2400)
    trained = evaluate_ntuple(net, dev, num_episodes=100, seed=42)
    print(f"mean max tile over 100 episodes: zero network {zero['mean_max_tile']:.1f}, after 2400 lock-steps of 1024 envs "
          f"{trained['mean_max_tile']:.1f} ({int(out['episodes'].item())} training episodes, max |w| "
          f"{int(net.weights.abs().max().item())})")
    assert trained["mean_max_tile"] >= 2 * zero["mean_max_tile"]
