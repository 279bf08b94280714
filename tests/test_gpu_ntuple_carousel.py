"""Carousel shaping for the n-tuple trainer on the GPU: one record and one restart step through the entry points, inside guard
words, and whole training runs, all bit-exact against the numpy restatement (tests/ntuple_carousel_ref.py); thresholds nothing
reaches leave a run as it is without the carousel; and the trainer still learns."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import ntuple_carousel_ref as K  # noqa: E402
import ntuple_ref as N  # noqa: E402
from oracle import g2048_oracle as npo  # noqa: E402
from src.g2048 import native as nv  # noqa: E402
from src.g2048.engine import seed_key  # noqa: E402
from src.ppo import NTupleNetwork, NTupleTrainer  # noqa: E402
from src.runs import evaluate_ntuple  # noqa: E402

pytestmark = pytest.mark.gpu
SLACK = 259
GUARD = 0xA5


class Guarded:
    """A device array of exactly ``shape`` at the front of a buffer whose SLACK elements behind it hold guard words."""

    def __init__(self, a, dev):
        a = np.ascontiguousarray(a)
        self.n = a.size
        host = np.full(self.n + SLACK, GUARD, a.dtype) if a.dtype == np.uint8 else np.full(self.n + SLACK, -0x5A5A5A5B, a.dtype)
        host[:self.n] = a.reshape(-1)
        self.guard = host[self.n:].copy()
        self.buf = torch.from_numpy(host).to(dev)
        self.t = self.buf[:self.n].view(a.shape)

    def get(self):
        assert np.array_equal(self.buf[self.n:].cpu().numpy(), self.guard), "a guard word was overwritten"
        return self.t.cpu().numpy()


def _i32(u32):
    return np.ascontiguousarray(u32, np.uint32).view(np.int32)


class DeviceState:
    def __init__(self, st, dev):
        self.pool_boards, self.pool_masks = Guarded(st.pool_boards, dev), Guarded(st.pool_masks, dev)
        self.reached, self.turn, self.starts = Guarded(st.reached, dev), Guarded(_i32(st.turn), dev), Guarded(st.starts, dev)

    def equal(self, st):
        return (np.array_equal(self.pool_boards.get(), st.pool_boards) and np.array_equal(self.pool_masks.get(), st.pool_masks)
                and np.array_equal(self.reached.get(), st.reached) and np.array_equal(self.turn.get().view(np.uint32), st.turn)
                and np.array_equal(self.starts.get(), st.starts))


def device_restart(dev, st0, sub, flag, boards0, masks0, mode, want_start=True):
    """-> (DeviceState, boards, masks, start_stage or None) after one restart launch, every guard checked."""
    d = DeviceState(st0, dev)
    boards, masks, fl = Guarded(boards0, dev), Guarded(masks0, dev), Guarded(flag, dev)
    start = Guarded(np.full(len(flag), 0x77, np.uint8), dev) if want_start else None
    nv.ntuple_carousel_restart(sub, fl.t, d.pool_boards.t, d.pool_masks.t, boards.t, masks.t, d.reached.t, d.turn.t, d.starts.t, mode,
                               None if start is None else start.t)
    assert np.array_equal(fl.get(), flag)
    return d, boards.get(), masks.get(), None if start is None else start.get()


@pytest.mark.parametrize("B", K.SIZES)
def test_record_is_bit_exact(dev, B):
    """The shared case (its contents are asserted on the CPU): flags mixed, tiles 16 and 17 against threshold 17, jumps of two and
    three stages, reached at or above the stage, a recorded mask of 0."""
    c = K.record_case(B)
    d = DeviceState(c["st0"], dev)
    boards, masks, flag = Guarded(c["boards"], dev), Guarded(c["masks"], dev), Guarded(c["flag"], dev)
    nv.ntuple_carousel_record(boards.t, masks.t, flag.t, K.TILES, d.reached.t, d.pool_boards.t, d.pool_masks.t)
    assert d.equal(c["st"]) and not c["st"].equal(c["st0"])
    assert np.array_equal(boards.get(), c["boards"]) and np.array_equal(masks.get(), c["masks"]) and np.array_equal(flag.get(), c["flag"])


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("B", K.SIZES)
def test_restart_is_bit_exact(dev, B, mode):
    """The shared case: pools part empty, a pool start and a fallback at every stage (B >= 63), turn 0xFFFFFFFF, starts not zero
    before; B = 1 is its own donor.  With and without start_stage."""
    c = K.restart_case(B, mode)
    for want_start in (True, False):
        d, boards, masks, start = device_restart(dev, c["st0"], c["sub"], c["flag"], c["boards0"], c["masks0"], mode, want_start)
        assert d.equal(c["st"]) and np.array_equal(boards, c["boards"]) and np.array_equal(masks, c["masks"])
        assert start is None or np.array_equal(start, c["start_stage"])


@pytest.mark.parametrize("mode", K.MODES)
def test_restart_in_a_permuted_env_order(dev, mode):
    """The envs in another lane order (``permuted_case``): the permuted boards, masks and start stages, identical starts."""
    c = K.permuted_case()
    p, got = c["p"], {}
    for which in ("a", "b"):
        st = c["pools"].copy()
        st.turn = c[which]["turn"].copy()
        want = K.run_permuted(c, which, mode)
        d, boards, masks, start = device_restart(dev, st, c["sub"], c[which]["flag"], c[which]["boards0"], c[which]["masks0"], mode)
        assert np.array_equal(boards, want[0]) and np.array_equal(masks, want[1]) and np.array_equal(start, want[2])
        assert np.array_equal(d.starts.get(), want[3]) and np.array_equal(d.reached.get(), want[4])
        got[which] = (boards, start, d.starts.get())
    assert np.array_equal(got["b"][0][p], got["a"][0]) and np.array_equal(got["b"][1][p], got["a"][1])
    assert np.array_equal(got["a"][2], got["b"][2]) and got["a"][2][1] > 0 and got["a"][2][3] > 0 and got["a"][2][2] == 0


def test_wrappers_check_shapes(dev):
    B, n, u8 = 4, 2, torch.uint8
    z = lambda *s, dtype=u8: torch.zeros(s, dtype=dtype, device=dev)  # noqa: E731
    boards, masks, flag, reached, pb, pm = z(B, 16), z(B), z(B), z(B), z(n, B, 16), z(n, B)
    turn, starts, sub = z(B, dtype=torch.int32), z(n + 1, dtype=torch.int64), np.array([1, 2], np.uint32)
    calls = [lambda: nv.ntuple_carousel_record(boards, masks, flag, (3, 5, 7), reached, pb, pm),  # pools of another threshold count
             lambda: nv.ntuple_carousel_record(boards, masks, flag, (3, 5), reached, pb.reshape(n, B * 16), pm),
             lambda: nv.ntuple_carousel_record(boards, masks, flag, (3, 5), reached.to(torch.int32), pb, pm),
             lambda: nv.ntuple_carousel_record(boards, masks, flag, (5, 3), reached, pb, pm),  # the entry point's own refusal
             lambda: nv.ntuple_carousel_restart(sub, flag, pb, pm, boards, masks, reached, turn, starts[:n], 1),
             lambda: nv.ntuple_carousel_restart(sub, flag, pb, z(n, B + 1)[:, :B], boards, masks, reached, turn, starts, 1),
             lambda: nv.ntuple_carousel_restart(sub, flag, pb, pm, boards, masks, reached, turn.to(torch.int64), starts, 1),
             lambda: nv.ntuple_carousel_restart(sub, flag, pb, pm, boards, masks, reached, turn, starts, 1, z(B + 1)),
             lambda: nv.ntuple_carousel_restart(sub, flag, pb, pm, boards, masks, reached, turn, starts, 7)]
    for i, call in enumerate(calls):
        with pytest.raises(nv.NativeError):
            call()
    nv.ntuple_carousel_record(boards, masks, flag, (3, 5), reached, pb, pm)
    nv.ntuple_carousel_restart(sub, flag, pb, pm, boards, masks, reached, turn, starts, 1)
    assert not pm.any() and not starts.any()


# ---------------------------------------------------------------------------------------------- whole runs
RUN = dict(num_envs=65, alpha=0.1, seed=0, rng_mode=npo.MODE_PARTITIONABLE)
RUN_TILES = (4, 6, 8)


def _run_subs(seed, T, mode):
    """The sub-keys of the first T lock-steps of a trainer: the init split, then two per lock-step."""
    key, _ = nv.chain_keys(seed_key(seed), 1, mode)
    return nv.chain_keys(key, 2 * T, mode)[1]


def _carousel_state(tr):
    return [x.cpu().numpy() for x in (tr.pool_boards, tr.pool_masks, tr.reached, tr.turn, tr.starts, tr.boards, tr.masks,
                                      tr.network.weights, tr.prev_after, tr.flag)]


def test_whole_run_replays_through_the_restatement(dev):
    """65 envs, SMALL, TD(0), thresholds (4, 6, 8), 600 lock-steps with record=True.  The restatement, fed the recorded boards, meta
    rows and start stages, reproduces every start stage, every restarted board and mask (the next row's) and the final pools,
    reached, turn and starts; the run holds a pool start at each of the three stages and a fallback; train(250) + train(350) gives
    the same bits; and the whole loop on the C oracle's env (``ntuple_carousel_ref.engine_training``, 38 / 31 / 29 / 26 starts at
    stages 0 .. 3 on this seed) ends in the same state."""
    T = 600
    tr = NTupleTrainer(NTupleNetwork(N.SMALL, device=dev), carousel_tiles=RUN_TILES, device=dev, **RUN)
    out = tr.train(T, record=True)
    boards, meta, start = (out[k].cpu().numpy() for k in ("boards", "meta", "start_stage"))
    st, counts = K.replay(boards, meta, start, tr.boards.cpu().numpy(), tr.masks.cpu().numpy(), _run_subs(0, T, RUN["rng_mode"]),
                          RUN_TILES, RUN["rng_mode"])
    print(f"starts per stage {st.starts.tolist()}, fallbacks {counts['fallback']}, fresh by turn {counts['fresh']}, "
          f"episodes {int(out['episodes'].item())}")
    assert np.array_equal(tr.pool_boards.cpu().numpy(), st.pool_boards) and np.array_equal(tr.pool_masks.cpu().numpy(), st.pool_masks)
    assert np.array_equal(tr.reached.cpu().numpy(), st.reached) and np.array_equal(tr.turn.cpu().numpy().view(np.uint32), st.turn)
    assert np.array_equal(tr.starts.cpu().numpy(), st.starts) and int(st.starts.sum()) == int(out["episodes"].item())
    assert (counts["pool"] > 0).all() and counts["fallback"] >= 1
    # the same run in two calls
    tr2 = NTupleTrainer(NTupleNetwork(N.SMALL, device=dev), carousel_tiles=RUN_TILES, device=dev, **RUN)
    tr2.train(250), tr2.train(350)
    assert all(np.array_equal(a, b) for a, b in zip(_carousel_state(tr), _carousel_state(tr2)))
    # the restatement's own loop, env included
    w = N.zero_weights(N.SMALL)
    ref, ref_start, _ = K.engine_training(w, N.SMALL, 65, T, RUN_TILES, alpha=0.1, seed=0, mode=RUN["rng_mode"])
    assert ref.equal(st) and np.array_equal(ref_start, start) and np.array_equal(tr.network.weights.cpu().numpy(), w)


def test_unreachable_thresholds_leave_the_run_as_it_is(dev):
    """carousel_tiles=(17,) against no carousel, same seed, 300 lock-steps: identical weights, boards and recorded rows (every
    restart falls back or is at stage 0, and the key chain does not move), starts[1] == 0."""
    runs = []
    for tiles in ((17,), None):
        tr = NTupleTrainer(NTupleNetwork(N.SMALL, device=dev), carousel_tiles=tiles, device=dev, **RUN)
        out = tr.train(300, record=True)
        runs.append((tr, out))
    (on, a), (off, b) = runs
    assert set(a) == set(b) | {"start_stage"} and int(a["episodes"].item()) > 0
    for k in b:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(on.network.weights, off.network.weights) and torch.equal(on.boards, off.boards) and torch.equal(on.masks, off.masks)
    assert torch.equal(on.prev_after, off.prev_after) and np.array_equal(on.key, off.key)
    assert int(on.starts[1].item()) == 0 and int(on.starts[0].item()) == int(a["episodes"].item()) and not on.pool_masks.any()
    assert set(np.unique(a["start_stage"].cpu().numpy()).tolist()) == {0, K.NO_START}


def test_it_still_learns(dev):
    """The protocol of ``test_gpu_ntuple_tc.test_it_learns`` (default tuples, 1 024 envs, 2 400 lock-steps of TC at alpha 1.0, 100
    evaluation episodes on seed 42) on a network with stage_tiles=(9, 10) and carousel_tiles="stages": mean max tile >= 2 x the
    all-zero network's, and every carousel stage has had episode starts."""
    net = NTupleNetwork(device=dev, stage_tiles=(9, 10))
    zero = evaluate_ntuple(net, dev, num_episodes=100, seed=42)
    trainer = NTupleTrainer(net, num_envs=1024, alpha=1.0, seed=0, device=dev, learner="tc", carousel_tiles="stages")
    out = trainer.train(2400)
    got = evaluate_ntuple(net, dev, num_episodes=100, seed=42)
    starts = trainer.starts.cpu().tolist()
    print(f"mean max tile over 100 episodes: zero network {zero['mean_max_tile']:.1f}; after 2400 lock-steps of 1024 envs, TC alpha 1.0, "
          f"stage_tiles (9, 10), carousel on: {got['mean_max_tile']:.1f} ({int(out['episodes'].item())} training episodes, starts per "
          f"stage {starts}, active stages {net.active_stages})")
    assert got["mean_max_tile"] >= 2 * zero["mean_max_tile"]
    assert all(s > 0 for s in starts) and sum(starts) == int(out["episodes"].item())
