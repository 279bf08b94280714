"""N-tuple TC learning on the GPU: one step, step sequences (rates below 1, saturation, the clamp, the halving) and a whole training
run bit-exact against the numpy restatement (tests/ntuple_tc_ref.py); the first step equal to the TD(0) kernels'; the trainer's
state; and that TC learns."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import ntuple_ref as N  # noqa: E402
import ntuple_tc_ref as T  # noqa: E402
from oracle import g2048_oracle as npo  # noqa: E402
from src.g2048 import native as nv  # noqa: E402
from src.ppo import NTupleNetwork, NTupleTrainer  # noqa: E402
from src.runs import evaluate_ntuple  # noqa: E402

pytestmark = pytest.mark.gpu
SLACK = 259
GUARD = 0xA5A5A5A5
GUARD_F32 = float(np.array([GUARD], np.uint32).view(np.float32)[0])
SIZES = (1, 63, 64, 65, 257)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _dev(a, dev):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(dev)  # a copy: the shared cases are read-only arrays


def _f32(a, dev):
    return _dev(np.asarray(a, np.float32).view(np.int32), dev).view(torch.float32)


class Tables:
    """Device weights, coherence tables and accumulators of one network."""

    def __init__(self, dev, w0, tuples):
        self.dev, self.cells = dev, N.cells_array(tuples)
        self.w = _dev(w0, dev)
        self.coh_e, self.coh_a = torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.acc = torch.zeros(self.w.shape, dtype=torch.int64, device=dev)
        self.abs_acc, self.cnt = torch.zeros_like(self.acc), torch.zeros_like(self.w)

    def step(self, prev, flag, target, F, alpha, with_error=True):
        """accumulate + apply -> td_error bits (None without td_error); the accumulators must be all-zero afterwards."""
        B, dev = len(flag), self.dev
        err = torch.full((B + SLACK,), GUARD_F32, device=dev)
        t_prev, t_flag, t_target = _dev(prev, dev), _dev(flag, dev), _f32(target, dev)
        nv.ntuple_tc_accumulate(t_prev, t_flag, t_target, self.w, self.cells, F, alpha, self.acc, self.abs_acc, self.cnt,
                                err[:B] if with_error else None)
        hits = int(self.cnt.sum().item())
        assert bool((self.abs_acc >= self.acc.abs()).all())
        nv.ntuple_tc_apply(t_prev, t_flag, self.cells, self.w, self.acc, self.abs_acc, self.cnt, self.coh_e, self.coh_a)
        assert hits == 8 * self.cells.shape[0] * int((flag != 0).sum())
        assert not self.acc.any() and not self.abs_acc.any() and not self.cnt.any()
        assert (_bits(err[B:]) == GUARD).all()
        if not with_error:
            assert (_bits(err) == GUARD).all()
            return None
        return _bits(err[:B])

    def equal(self, w, coh_e, coh_a):
        return (np.array_equal(self.w.cpu().numpy(), w) and np.array_equal(self.coh_e.cpu().numpy(), coh_e)
                and np.array_equal(self.coh_a.cpu().numpy(), coh_a))


@pytest.fixture(scope="module")
def one_step():
    """The inputs of the one-step test on SMALL (257 boards, the special ones first, flags mixed); a run on B boards uses the first B."""
    prev, flag, target, w0 = T.one_step_inputs(N.SMALL, 12, n=max(SIZES))
    return prev, flag, target, w0


@pytest.mark.parametrize("with_error", [True, False])
@pytest.mark.parametrize("B", SIZES)
def test_one_step_is_bit_exact(dev, one_step, B, with_error):
    prev, flag, target, w0 = (x[:B] if i < 3 else x for i, x in enumerate(one_step))
    want, (want_e, want_a) = w0.copy(), T.zero_coherence(w0)
    want_err = T.tc_step(prev, flag, target, want, want_e, want_a, N.SMALL, 12, 0.1)
    tb = Tables(dev, w0, N.SMALL)
    err = tb.step(prev, flag, target, 12, 0.1, with_error)
    assert tb.equal(want, want_e, want_a)
    if with_error:
        assert np.array_equal(err, want_err.view(np.uint32)) and (err[flag == 0] == 0).all()
    if B >= 9:
        assert set(flag.tolist()) == {0, 1, 2} and prev.max() == 17 and (want != w0).any()


def test_collision_case_in_two_orders(dev):
    c = N.collision_case()
    assert np.unique(c["prev"], axis=0, return_counts=True)[1].max() >= 300  # 300 of the boards are identical
    want, (want_e, want_a) = N.small_weights().copy(), T.zero_coherence(N.small_weights())
    want_err = T.tc_step(c["prev"], c["flag"], c["target"], want, want_e, want_a, N.SMALL, 12, 0.1)
    tb = Tables(dev, N.small_weights(), N.SMALL)
    err = tb.step(c["prev"], c["flag"], c["target"], 12, 0.1)
    assert tb.equal(want, want_e, want_a) and np.array_equal(err, want_err.view(np.uint32))
    assert np.array_equal(want, c["weights_after"])  # rate 1 everywhere: TD(0)'s weights
    perm = np.random.default_rng(1).permutation(1000)  # the same boards in another order: the sums are order-free
    tb2 = Tables(dev, N.small_weights(), N.SMALL)
    err2 = tb2.step(c["prev"][perm], c["flag"][perm], c["target"][perm], 12, 0.1)
    assert torch.equal(tb2.w, tb.w) and torch.equal(tb2.coh_e, tb.coh_e) and torch.equal(tb2.coh_a, tb.coh_a)
    assert np.array_equal(err2, err[perm])


@pytest.mark.parametrize("alpha,scale,extreme", [(0.1, 500.0, False), (1000.0, 1e9, True)])
def test_six_steps_are_bit_exact(dev, alpha, scale, extreme):
    """The two sequences of the CPU tests: rates below 1 are read; in the second the weights saturate, delta sits on the clamp and A
    is halved (asserted on the restatement there and here)."""
    c = T.sequence_case(alpha, scale, extreme)
    assert c["stats"]["slowed"] > 0
    if extreme:
        assert c["stats"]["saturated"] > 0 and c["stats"]["clamped"] > 0 and c["stats"]["halved"] > 0
    tb = Tables(dev, c["w0"], N.SMALL)
    for t, want in enumerate(c["after"]):
        err = tb.step(c["prev"], c["flag"], c["targets"][t], 12, alpha)
        assert tb.equal(want["weights"], want["coh_e"], want["coh_a"]), t
        assert np.array_equal(err, want["td_error"].view(np.uint32)), t


def test_one_step_on_wide_tables(dev):
    rng = np.random.default_rng(11)
    prev = N.boards_for(65, seed=12)
    flag = rng.integers(0, 3, 65).astype(np.uint8)
    flag[:9] = [1, 2, 1, 2, 1, 2, 1, 2, 1]  # the special boards take part
    target = (rng.standard_normal(65) * 800).astype(np.float32)
    want, (want_e, want_a) = N.wide_weights().copy(), T.zero_coherence(N.wide_weights())
    want_err = T.tc_step(prev, flag, target, want, want_e, want_a, N.WIDE, 12, 0.1)
    tb = Tables(dev, N.wide_weights(), N.WIDE)
    err = tb.step(prev, flag, target, 12, 0.1)
    assert torch.equal(tb.w, _dev(want, dev)) and torch.equal(tb.coh_e, _dev(want_e, dev)) and torch.equal(tb.coh_a, _dev(want_a, dev))
    assert np.array_equal(err, want_err.view(np.uint32)) and (want != N.wide_weights()).any()


def test_the_first_step_equals_the_td0_kernels(dev):
    """From zero coherence: the same weights and td_error as ntuple_td_accumulate + ntuple_td_apply on the same inputs."""
    c = N.collision_case()
    cells = N.cells_array(N.SMALL)
    t_prev, t_flag, t_target = _dev(c["prev"], dev), _dev(c["flag"], dev), _f32(c["target"], dev)
    w = _dev(N.small_weights(), dev)
    acc, cnt = torch.zeros(w.shape, dtype=torch.int64, device=dev), torch.zeros_like(w)
    err = torch.empty(1000, device=dev)
    nv.ntuple_td_accumulate(t_prev, t_flag, t_target, w, cells, 12, 0.1, acc, cnt, err)
    nv.ntuple_td_apply(t_prev, t_flag, cells, w, acc, cnt)
    tb = Tables(dev, N.small_weights(), N.SMALL)
    tc_err = tb.step(c["prev"], c["flag"], c["target"], 12, 0.1)
    assert torch.equal(tb.w, w) and np.array_equal(tc_err, _bits(err)) and not torch.equal(w, _dev(N.small_weights(), dev))


REPLAY_TUPLES = ((0, 1, 2), (4, 5, 6))


def test_trainer_replay_and_state(dev):
    """NTupleTrainer(num_envs=192, m=2 L=3, alpha=1.0, learner="tc").train(48, record=True) from ``crowding_weights``: the restatement,
    fed the recorded boards and meta rows, reproduces scores, targets, final weights and both coherence tables bit for bit, and
    ``engine_training(learner="tc")`` reproduces the boards and meta rows on the C oracle.  On the CPU that ``engine_training`` ends
    8 episodes inside the 48 lock-steps at alpha = 1.0 with seed 0 (9 and 13 with seeds 1 and 2; checked first, below): no longer
    run is needed.  Then state_dict -> a fresh trainer -> load_state_dict gives equal tables."""
    start = N.crowding_weights(REPLAY_TUPLES)
    ref_w = start.copy()
    ref_e, ref_a = T.zero_coherence(ref_w)
    ref = T.engine_training(ref_w, REPLAY_TUPLES, 192, 48, alpha=1.0, frac_bits=12, seed=0, learner="tc", coh_e=ref_e, coh_a=ref_a)
    assert ref["episodes"] >= 1
    net = NTupleNetwork(REPLAY_TUPLES, device=dev)
    net.weights.copy_(_dev(start, dev))
    trainer = NTupleTrainer(net, num_envs=192, alpha=1.0, seed=0, rng_mode=npo.MODE_PARTITIONABLE, device=dev, learner="tc")
    out = trainer.train(48, record=True)
    boards, meta = out["boards"].cpu().numpy(), out["meta"].cpu().numpy()
    assert int(out["episodes"].item()) == int(((meta >> 6) & 1).sum()) == ref["episodes"]
    w = start.copy()
    ce, ca = T.zero_coherence(w)
    want_q, want_v = T.replay_training(w, REPLAY_TUPLES, boards, meta, alpha=1.0, frac_bits=12, learner="tc", coh_e=ce, coh_a=ca)
    assert np.array_equal(_bits(out["scores"]), want_q.view(np.uint32))
    assert np.array_equal(_bits(out["targets"]), want_v.view(np.uint32))
    assert np.array_equal(net.weights.cpu().numpy(), w) and (w != start).any()
    assert np.array_equal(trainer.coh_e.cpu().numpy(), ce) and np.array_equal(trainer.coh_a.cpu().numpy(), ca)
    assert (np.abs(ce) < ca).any()  # rates below 1 were in use
    assert not trainer.acc.any() and not trainer.abs_acc.any() and not trainer.cnt.any()
    assert np.array_equal(ref["boards"], boards) and np.array_equal(ref["meta"], meta)
    assert np.array_equal(ref_w, w) and np.array_equal(ref_e, ce) and np.array_equal(ref_a, ca)
    coh = trainer.coherence()
    n, rate = T.coherence(ce, ca)
    assert int(coh["entries"].item()) == n and abs(float(coh["mean_rate"].item()) - rate) < 1e-12
    state = trainer.state_dict()
    assert not state["coh_e"].is_cuda and state["lock_steps"] == 48 and state["alpha"] == 1.0 and state["learner"] == "tc"
    fresh = NTupleTrainer(net, num_envs=64, alpha=0.1, seed=1, device=dev, learner="tc")
    fresh.load_state_dict(state)
    assert torch.equal(fresh.coh_e, trainer.coh_e) and torch.equal(fresh.coh_a, trainer.coh_a)
    assert fresh.alpha == 1.0 and fresh.lock_steps == 48


def test_it_learns(dev):
    """The default network, 1 024 envs, 2 400 lock-steps of TC at alpha = 1.0, then 100 evaluation episodes (seed 42) against an all-zero
    network on the same seeds: trained mean max tile >= 2 x the zero network's, the property of ``test_gpu_ntuple.test_it_learns``.
    A second default network trains TD(0) at alpha = 0.1 for the same 2 400 lock-steps; both means are printed and TC's must not be
    below TD(0)'s.
    The restatement's own loop on the CPU at this size (``ntuple_tc_ref.simulate_training`` / ``ntuple_ref.simulate_evaluation``,
    numpy's RNG for the spawns, 100 evaluation episodes on seed 42), training seeds 0 / 1 / 2: zero network 226.6; TC at alpha 1.0
    1702.4 / 1634.6 / 1689.6, a ratio to the zero network of 7.5 on seed 0, above the 3 that the factor 2 wants as a margin; TD(0) at
    alpha 0.1 846.1 / 926.7 / 891.5, so TC / TD(0) is 2.01 / 1.76 / 1.90, at least 1.25 on each seed: the comparison is asserted.
    Mean rate over the 1.3 M entries touched: 0.64."""
    net = NTupleNetwork(device=dev)
    zero = evaluate_ntuple(net, dev, num_episodes=100, seed=42)
    trainer = NTupleTrainer(net, num_envs=1024, alpha=1.0, seed=0, device=dev, learner="tc")
    out = trainer.train(2400)
    tc = evaluate_ntuple(net, dev, num_episodes=100, seed=42)
    coh = trainer.coherence()
    max_w = int(net.weights.abs().max().item())
    del trainer, net
    net0 = NTupleNetwork(device=dev)
    out0 = NTupleTrainer(net0, num_envs=1024, alpha=0.1, seed=0, device=dev).train(2400)
    td0 = evaluate_ntuple(net0, dev, num_episodes=100, seed=42)
    print(f"mean max tile over 100 episodes: zero network {zero['mean_max_tile']:.1f}; after 2400 lock-steps of 1024 envs: TC alpha 1.0 "
          f"{tc['mean_max_tile']:.1f} ({int(out['episodes'].item())} training episodes, max |w| {max_w}, {int(coh['entries'].item())} "
          f"entries with a rate, mean rate {float(coh['mean_rate'].item()):.3f}), TD(0) alpha 0.1 {td0['mean_max_tile']:.1f} "
          f"({int(out0['episodes'].item())} training episodes)")
    assert tc["mean_max_tile"] >= 2 * zero["mean_max_tile"]
    assert tc["mean_max_tile"] >= td0["mean_max_tile"]
