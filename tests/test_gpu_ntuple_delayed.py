"""Delayed TD(lambda) / TC(lambda) on the GPU: one step at every ring position, a collision case in two lane orders and a six-step
sequence through the entry points inside guard words, and whole training runs (staged with promotions, split, with the carousel),
all bit-exact against the numpy restatement (tests/ntuple_delayed_ref.py); horizon 1 equal to the TD(0) and TC kernels; the
trainer's state; and that TC(0.5) learns."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import ntuple_delayed_ref as D  # noqa: E402
import ntuple_ref as N  # noqa: E402
import ntuple_tc_ref as T  # noqa: E402
from oracle import g2048_oracle as npo  # noqa: E402
from src.g2048 import native as nv  # noqa: E402
from src.ppo import NTupleNetwork, NTupleTrainer  # noqa: E402
from src.runs import evaluate_ntuple  # noqa: E402

pytestmark = pytest.mark.gpu
SLACK = 259
LEARNERS = [("td0", 0.1), ("tc", 1.0)]


class Guarded:
    """A device array of exactly ``a``'s shape between two runs of SLACK guard elements: the kernels must write neither side."""

    def __init__(self, a, dev):
        a = np.ascontiguousarray(a)
        self.n, self.dtype = a.size, a.dtype
        raw = a.reshape(-1).view(np.uint8)
        pad = SLACK * a.itemsize + (-SLACK * a.itemsize) % 16  # the front run keeps the array 16-byte aligned
        host = np.full(pad + raw.size + SLACK * a.itemsize, 0xA5, np.uint8)
        host[pad:pad + raw.size] = raw
        self.pad, self.size, self.guard = pad, raw.size, host.copy()
        self.buf = torch.from_numpy(host).to(dev)
        self.t = self.buf[pad:pad + raw.size].view(_TORCH[a.dtype.type]).view(a.shape)
        assert self.t.data_ptr() % 16 == 0

    def get(self):
        host = self.buf.cpu().numpy()
        assert np.array_equal(host[:self.pad], self.guard[:self.pad]), "a guard word in front was overwritten"
        assert np.array_equal(host[self.pad + self.size:], self.guard[self.pad + self.size:]), "a guard word behind was overwritten"
        return host[self.pad:self.pad + self.size].view(self.dtype).reshape(self.t.shape).copy()


_TORCH = {np.uint8: torch.uint8, np.int32: torch.int32, np.int64: torch.int64, np.float32: torch.float32}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Device:
    """Ring, flag, tables and td_error of one case on the device, every array guarded on both sides."""

    def __init__(self, dev, ring, flag, w0, tuples, tiles, learner, coh=None):
        self.cells, self.tiles, self.learner = N.cells_array(tuples), (np.array(tiles, np.uint8) if len(tiles) else None), learner
        self.h, self.B = ring.h, ring.B
        self.hist, self.herr, self.hlen = Guarded(ring.hist, dev), Guarded(ring.err, dev), Guarded(ring.len, dev)
        self.flag, self.w = Guarded(flag, dev), Guarded(w0, dev)
        self.acc, self.cnt = Guarded(np.zeros(w0.shape, np.int64), dev), Guarded(np.zeros(w0.shape, np.int32), dev)
        self.err = Guarded(np.full(ring.B, -7, np.float32), dev)
        self.prev = Guarded(np.zeros((ring.B, 16), np.uint8), dev)
        self.abs_acc = self.coh_e = self.coh_a = None
        if learner == "tc":
            ce, ca = T.zero_coherence(w0) if coh is None else coh
            self.abs_acc, self.coh_e, self.coh_a = Guarded(np.zeros(w0.shape, np.int64), dev), Guarded(ce, dev), Guarded(ca, dev)

    def _t(self, g):
        return None if g is None else g.t

    def step(self, target, head, lam, F, alpha):
        """accumulate + apply -> td_error; the accumulators must be all-zero afterwards."""
        tgt = Guarded(np.asarray(target, np.float32), self.w.buf.device)
        nv.ntuple_delayed_accumulate(self.hist.t, self.herr.t, self.hlen.t, self.flag.t, tgt.t, head, lam, self.w.t, self.cells, F, alpha,
                                     self.acc.t, self._t(self.abs_acc), self.cnt.t, self.err.t, self.tiles)
        hits = int(self.cnt.t.sum().item())
        assert hits % (8 * self.cells.shape[0]) == 0
        nv.ntuple_delayed_apply(self.hist.t, self.hlen.t, self.flag.t, head, self.cells, self.w.t, self.acc.t, self._t(self.abs_acc),
                                self.cnt.t, self._t(self.coh_e), self._t(self.coh_a), self.tiles)
        assert not self.acc.get().any() and not self.cnt.get().any() and (self.abs_acc is None or not self.abs_acc.get().any())
        assert np.array_equal(_bits(tgt.get()), _bits(target))
        return self.err.get(), hits // (8 * self.cells.shape[0])

    def link(self, row, meta, slot):
        r, m = Guarded(row, self.w.buf.device), Guarded(meta, self.w.buf.device)
        nv.ntuple_delayed_link(r.t, m.t, slot, self.prev.t, self.flag.t, self.hist.t, self.hlen.t)
        assert np.array_equal(r.get(), row) and np.array_equal(m.get(), meta)

    def equal(self, ring, w, coh_e=None, coh_a=None):
        same = (np.array_equal(self.hist.get(), ring.hist) and np.array_equal(_bits(self.herr.get()), _bits(ring.err))
                and np.array_equal(self.hlen.get(), ring.len) and np.array_equal(self.w.get(), w))
        if self.learner == "tc":
            same = same and np.array_equal(self.coh_e.get(), coh_e) and np.array_equal(self.coh_a.get(), coh_a)
        return same


def _one_step(dev, case, head, lam, tuples, F, alpha, tiles, learner):
    stats = {}
    want_ring, want = case["ring"].copy(), case["w0"].copy()
    want_e, want_a = np.full(want.shape, 1000, np.int32), np.full(want.shape, 4000, np.int32)  # a rate of 1 / 4 wherever TC reads one
    want_err = D.step(want_ring, case["flag"], case["target"], head, lam, want, tuples, F, alpha, tiles, learner, want_e, want_a, stats)
    d = Device(dev, case["ring"], case["flag"], case["w0"], tuples, tiles, learner,
               (np.full(want.shape, 1000, np.int32), np.full(want.shape, 4000, np.int32)))
    err, due = d.step(case["target"], head, lam, F, alpha)
    assert d.equal(want_ring, want, want_e, want_a) and np.array_equal(_bits(err), _bits(want_err)) and due == stats["due"]
    assert np.array_equal(d.flag.get(), case["flag"])
    stats["moved"] = bool((want != case["w0"]).any())
    return stats


@pytest.mark.parametrize("learner,alpha", LEARNERS)
@pytest.mark.parametrize("lam", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("h", [1, 2, 3, 8])
@pytest.mark.parametrize("B", [1, 257])
def test_one_step_at_every_ring_position_is_bit_exact(dev, B, h, lam, learner, alpha):
    """The CPU test's cases on SMALL through the entry points: every head, hist_len 0 .. h under flags 0, 1 and 2, the due-at-h
    state, flushes shorter than h, one env with the same board at every ring position; guard words on both sides of every array."""
    case = D.ring_case(N.SMALL, 12, h, B)
    total = {}
    for head in range(h):
        for k, v in _one_step(dev, case, head, lam, N.SMALL, 12, alpha, (), learner).items():
            total[k] = total.get(k, 0) + v
    if B == 257:
        assert total["moved"] == h and total["due"] > 0 and (h == 1 or total["flushed_short"] > 0)


@pytest.mark.parametrize("learner,alpha", LEARNERS)
@pytest.mark.parametrize("tuples,F", D.SHAPES)
def test_every_table_shape_is_bit_exact(dev, tuples, F, learner, alpha):
    """(m, L) in (1, 2), (3, 2), (8, 2), (2, 6) at h = 3, lam = 0.5; the wide tables at one head."""
    wide = len(tuples[0]) == 6
    case = D.ring_case(tuples, F, 3, 65 if wide else 257)
    for head in ((1,) if wide else range(3)):
        assert _one_step(dev, case, head, 0.5, tuples, F, alpha, (), learner)["moved"]


@pytest.mark.parametrize("learner,alpha", LEARNERS)
@pytest.mark.parametrize("h", [2, 8])
def test_staged_network_and_the_clamp(dev, h, learner, alpha):
    """Three stages with a top-stage board between stage-0 neighbours in env 0's ring; then errors of 1e9 at alpha 1000 (delta on
    the +-2^30 clamp, asserted on the restatement)."""
    case = D.ring_case(N.SMALL, 12, h, 257, tiles=D.STAGE_TILES)
    for head in (0, h - 1):
        _one_step(dev, case, head, 0.5, N.SMALL, 12, alpha, D.STAGE_TILES, learner)
    big = D.ring_case(N.SMALL, 12, h, 257, scale=1e9)
    assert _one_step(dev, big, 1, 1.0, N.SMALL, 12, 1000.0, (), learner)["clamped"] > 0


@pytest.mark.parametrize("learner,alpha", LEARNERS)
def test_collision_case_in_two_lane_orders(dev, learner, alpha):
    """200 of 600 envs hold identical rings: the same envs in another order give the same tables, equal to the restatement's."""
    c = D.collision_case()
    perm = np.random.default_rng(1).permutation(600)
    got = []
    for case in (c, D.permuted(c, perm)):
        want_ring, want = case["ring"].copy(), N.small_weights().copy()
        want_e, want_a = T.zero_coherence(want)
        want_err = D.step(want_ring, case["flag"], case["target"], 2, 0.5, want, N.SMALL, 12, alpha, (), learner, want_e, want_a)
        d = Device(dev, case["ring"], case["flag"], N.small_weights(), N.SMALL, (), learner)
        err, _ = d.step(case["target"], 2, 0.5, 12, alpha)
        assert d.equal(want_ring, want, want_e, want_a) and np.array_equal(_bits(err), _bits(want_err))
        got.append((d.w.get(), err))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(_bits(got[0][1][perm]), _bits(got[1][1]))
    assert (got[0][0] != N.small_weights()).any()


@pytest.mark.parametrize("learner", ["td0", "tc"])
def test_six_lock_steps_from_a_fixed_ring(dev, learner):
    """accumulate -> apply -> link six times: tables, ring, prev_after and flag after every step."""
    c = D.sequence_case(learner)
    d = Device(dev, c["ring0"], c["flag0"], c["w0"], N.SMALL, (), learner)
    for t, ((row, meta, target, head, slot), want) in enumerate(zip(c["rows"], c["after"])):
        err, _ = d.step(target, head, c["lam"], 12, c["alpha"])
        d.link(row, meta, slot)
        assert d.equal(want["ring"], want["weights"], want["coh_e"], want["coh_a"]), t
        assert np.array_equal(_bits(err), _bits(want["td_error"])), t
        assert np.array_equal(d.prev.get(), want["prev"]) and np.array_equal(d.flag.get(), want["flag"]), t


@pytest.mark.parametrize("lam", [0.0, 0.7])
def test_horizon_one_equals_the_td0_and_tc_kernels(dev, lam):
    """h = 1 against ntuple_td_accumulate / ntuple_td_apply / ntuple_link and the TC pair on the same inputs, two lock-steps (the
    second reads rates below 1): weights, coherence tables, td_error, prev_after and flag bit for bit."""
    c = N.collision_case()
    B, cells = 1000, N.cells_array(N.SMALL)
    rng = np.random.default_rng(2)
    rows = [N.boards_for(B, seed=31 + t) for t in range(2)]
    metas = [(rng.integers(0, 4, B) | (0xF << 2) | ((rng.random(B) < 0.2).astype(np.int64) << 6)).astype(np.uint8) for t in range(2)]
    targets = [c["target"], (rng.standard_normal(B) * 500).astype(np.float32)]
    up = lambda a: torch.from_numpy(np.array(a, copy=True)).to(dev)  # noqa: E731
    for learner, alpha in LEARNERS:
        w, prev, flag = up(N.small_weights()), up(c["prev"]), up(c["flag"])
        acc, cnt = torch.zeros(w.shape, dtype=torch.int64, device=dev), torch.zeros_like(w)
        abs_acc, ce, ca = torch.zeros_like(acc), torch.zeros_like(w), torch.zeros_like(w)
        err = torch.empty(B, device=dev)
        ring = D.Ring(1, B)
        ring.hist[0], ring.len[:] = c["prev"], 1
        d = Device(dev, ring, c["flag"], N.small_weights(), N.SMALL, (), learner)
        d.prev.t.copy_(prev)
        for t in range(2):
            tgt = up(targets[t])
            if learner == "tc":
                nv.ntuple_tc_accumulate(prev, flag, tgt, w, cells, 12, alpha, acc, abs_acc, cnt, err)
                nv.ntuple_tc_apply(prev, flag, cells, w, acc, abs_acc, cnt, ce, ca)
            else:
                nv.ntuple_td_accumulate(prev, flag, tgt, w, cells, 12, alpha, acc, cnt, err)
                nv.ntuple_td_apply(prev, flag, cells, w, acc, cnt)
            live = int((flag != 0).sum().item())
            nv.ntuple_link(up(rows[t]), up(metas[t]), prev, flag)
            got_err, due = d.step(targets[t], 0, lam, 12, alpha)
            d.link(rows[t], metas[t], 0)
            assert due == live  # every env with a predecessor updates its one state
            assert np.array_equal(d.w.get(), w.cpu().numpy()) and np.array_equal(_bits(got_err), _bits(err.cpu().numpy())), (learner, t)
            assert np.array_equal(d.prev.get(), prev.cpu().numpy()) and np.array_equal(d.flag.get(), flag.cpu().numpy())
            assert np.array_equal(d.hist.get()[0], prev.cpu().numpy()) and (d.hlen.get() == 1).all()
            if learner == "tc":
                assert np.array_equal(d.coh_e.get(), ce.cpu().numpy()) and np.array_equal(d.coh_a.get(), ca.cpu().numpy())
        assert not torch.equal(w, up(N.small_weights()))


# ---------------------------------------------------------------------------------------------- whole runs
RUN_TILES = (3, 5)


def _trainer(dev, learner, alpha, staged, **kw):
    net = NTupleNetwork(N.SMALL, 12, dev, RUN_TILES if staged else None)
    start = N.crowding_weights(N.SMALL)  # a greedy player on them fills the board: episodes end inside 48 lock-steps
    (net.weights[0] if staged else net.weights).copy_(torch.from_numpy(start.copy()).to(dev))
    return net, NTupleTrainer(net, 64, alpha=alpha, seed=0, rng_mode=npo.MODE_PARTITIONABLE, device=dev, learner=learner, promote_every=8,
                              lam=0.5, **kw)


def _start_weights(staged):
    w = np.zeros((len(RUN_TILES) + 1, 3, 256) if staged else (3, 256), np.int32)
    (w[0] if staged else w)[...] = N.crowding_weights(N.SMALL)
    return w


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("learner,alpha", LEARNERS)
def test_trainer_run_replays_through_the_restatement(dev, learner, alpha, staged):
    """NTupleTrainer(64 envs, SMALL, lam=0.5: horizon 4).train(48, record=True) from ``crowding_weights``, unstaged and with
    stage_tiles (3, 5) at promote_every=8: the restatement, fed the recorded boards and meta rows, reproduces scores, targets, the
    final weights, coherence tables, ring, promotions; it shows at least one episode end with a flush and (staged) a promotion inside
    the run, so the case is not vacuous; the whole loop on the C oracle's env gives the same record; train(20) + train(28) gives
    the same bits."""
    net, trainer = _trainer(dev, learner, alpha, staged)
    assert trainer.horizon == 4
    out = trainer.train(48, record=True)
    boards, meta = out["boards"].cpu().numpy(), out["meta"].cpu().numpy()
    w = _start_weights(staged)
    ce, ca = T.zero_coherence(w)
    want_q, want_v, lr = D.replay_training(w, N.SMALL, boards, meta, alpha, 12, learner, 0.5, None, RUN_TILES if staged else None, 8, ce, ca)
    assert lr.stats["episode_ends"] >= 1 and lr.stats["flushed"] >= 1 and lr.stats["due"] > 64
    assert int(out["episodes"].item()) == lr.stats["episode_ends"]
    if staged:
        assert len(lr.promotions) >= 1 and 0 < lr.promotions[0][0] < 48 and trainer.promotions == lr.promotions
        assert net.active_stages == lr.net.active
    assert np.array_equal(_bits(out["scores"].cpu().numpy()), _bits(want_q)) and np.array_equal(_bits(out["targets"].cpu().numpy()), _bits(want_v))
    assert np.array_equal(net.weights.cpu().numpy(), w) and (w != _start_weights(staged)).any()
    if learner == "tc":
        assert np.array_equal(trainer.coh_e.cpu().numpy(), ce) and np.array_equal(trainer.coh_a.cpu().numpy(), ca)
        assert not trainer.abs_acc.any()
    assert not trainer.acc.any() and not trainer.cnt.any() and trainer.lock_steps == 48
    assert np.array_equal(trainer.hist.cpu().numpy(), lr.ring.hist) and np.array_equal(trainer.hist_len.cpu().numpy(), lr.ring.len)
    assert np.array_equal(_bits(trainer.hist_err.cpu().numpy()), _bits(lr.ring.err))
    assert np.array_equal(trainer.prev_after.cpu().numpy(), lr.prev) and np.array_equal(trainer.flag.cpu().numpy(), lr.flag)
    w2 = _start_weights(staged)
    ref = D.engine_training(w2, N.SMALL, 64, 48, alpha=alpha, seed=0, learner=learner, lam=0.5, stage_tiles=RUN_TILES if staged else None,
                            promote_every=8)
    assert np.array_equal(ref["boards"], boards) and np.array_equal(ref["meta"], meta) and np.array_equal(w2, w)
    net2, split = _trainer(dev, learner, alpha, staged)
    split.train(20)
    split.train(28)
    assert torch.equal(net2.weights, net.weights) and split.promotions == trainer.promotions
    assert torch.equal(split.hist, trainer.hist) and torch.equal(split.hist_len, trainer.hist_len)
    assert torch.equal(split.hist_err.view(torch.int32), trainer.hist_err.view(torch.int32))
    if learner == "tc":
        assert torch.equal(split.coh_e, trainer.coh_e) and torch.equal(split.coh_a, trainer.coh_a)


def test_trainer_run_with_the_carousel_on(dev):
    """The staged TC run with carousel_tiles=(3,): every ended episode restarts through the carousel, prev_after stays the newest
    ring slot, and the restatement still reproduces the run from the recorded boards and meta rows."""
    net, trainer = _trainer(dev, "tc", 1.0, True, carousel_tiles=(3,))
    out = trainer.train(48, record=True)
    boards, meta = out["boards"].cpu().numpy(), out["meta"].cpu().numpy()
    print(f"carousel starts per stage {trainer.starts.cpu().tolist()}")
    assert int(trainer.starts.sum().item()) == int(out["episodes"].item()) >= 1 and bool(trainer.pool_masks.any())
    assert int(trainer.starts[1].item()) >= 1  # an episode started on a pool board: its first link restarts the ring there
    w = _start_weights(True)
    ce, ca = T.zero_coherence(w)
    want_q, want_v, lr = D.replay_training(w, N.SMALL, boards, meta, 1.0, 12, "tc", 0.5, None, RUN_TILES, 8, ce, ca)
    assert lr.stats["flushed"] >= 1 and trainer.promotions == lr.promotions and len(lr.promotions) >= 1
    assert np.array_equal(_bits(out["scores"].cpu().numpy()), _bits(want_q)) and np.array_equal(net.weights.cpu().numpy(), w)
    assert np.array_equal(trainer.coh_e.cpu().numpy(), ce) and np.array_equal(trainer.coh_a.cpu().numpy(), ca)
    assert torch.equal(trainer.prev_after, trainer.hist[47 % 4]) and np.array_equal(trainer.hist.cpu().numpy(), lr.ring.hist)


def test_lam_off_allocates_nothing_and_state_round_trips(dev):
    net = NTupleNetwork(N.SMALL, device=dev)
    off = NTupleTrainer(net, 64, device=dev)
    assert off.hist is None and off.hist_err is None and off.hist_len is None and "lam" not in off.state_dict()
    on = NTupleTrainer(net, 64, alpha=1.0, device=dev, learner="tc", lam=0.5)
    on.train(10)
    state = on.state_dict()
    assert state["lam"] == 0.5 and state["horizon"] == 4 and state["lock_steps"] == 10 and not state["coh_e"].is_cuda
    fresh = NTupleTrainer(net, 32, alpha=0.5, seed=1, device=dev, learner="tc", lam=0.5)
    fresh.load_state_dict(state)
    assert torch.equal(fresh.coh_e, on.coh_e) and fresh.lock_steps == 10 and fresh.alpha == 1.0
    assert not fresh.hist_len.any() and not fresh.flag.any()  # the ring starts afresh
    fresh.train(7)  # resumes at ring position 10 mod 4 with an empty ring
    assert int(fresh.hist_len.max().item()) == 4 and fresh.lock_steps == 17
    for other in (NTupleTrainer(net, 8, device=dev, learner="tc"), NTupleTrainer(net, 8, device=dev, learner="tc", lam=0.5, horizon=3),
                  NTupleTrainer(net, 8, device=dev, learner="tc", lam=0.4, horizon=4)):
        with pytest.raises(ValueError):
            other.load_state_dict(state)
        assert other.lock_steps == 0 and not other.coh_a.any()
    with pytest.raises(ValueError):
        on.load_state_dict(NTupleTrainer(net, 8, device=dev, learner="tc").state_dict())


def test_it_learns(dev):
    """The protocol of ``test_gpu_ntuple_tc.test_it_learns`` with lam=0.5 (horizon 4): the default network, 1 024 envs, 2 400
    lock-steps of TC at alpha 1.0, then 100 evaluation episodes (seed 42) against the all-zero network on the same seeds: trained
    mean max tile >= 2 x the zero network's.  Nothing is asserted about lambda against lambda-off.
    The restatement's own loop on the CPU (``ntuple_delayed_ref.simulate_training`` / ``ntuple_ref.simulate_evaluation``, numpy's
    RNG for the spawns, 100 evaluation episodes on seed 42), zero network 226.6: at this size, training seed 0, 1 781.8 after 1 726 training episodes, a ratio of 7.9 where the factor 2 wants 3 as a margin;
    on the small network of the TC section (m = 2, L = 3, 64 envs, 300 lock-steps) the ratio is 2.11 / 2.44 / 2.14 on seeds 0 / 1 / 2
    and 1.94 after 600 lock-steps on seed 0 (plain TC: 2.4 / 2.2 / 2.4 and 3.1), so that network, not this one, sits near the bound."""
    net = NTupleNetwork(device=dev)
    zero = evaluate_ntuple(net, dev, num_episodes=100, seed=42)
    trainer = NTupleTrainer(net, num_envs=1024, alpha=1.0, seed=0, device=dev, learner="tc", lam=0.5)
    out = trainer.train(2400)
    got = evaluate_ntuple(net, dev, num_episodes=100, seed=42)
    coh = trainer.coherence()
    print(f"mean max tile over 100 episodes: zero network {zero['mean_max_tile']:.1f}; after 2400 lock-steps of 1024 envs, TC(0.5) "
          f"horizon {trainer.horizon} at alpha 1.0: {got['mean_max_tile']:.1f} ({int(out['episodes'].item())} training episodes, max |w| "
          f"{int(net.weights.abs().max().item())}, mean rate {float(coh['mean_rate'].item()):.3f})")
    assert got["mean_max_tile"] >= 2 * zero["mean_max_tile"]
