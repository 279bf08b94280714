"""Imitation learning on the device: g2048_distill_loss and g2048_distill_gather against tests/distill_ref.py inside guard buffers,
DistillTrainer's collect / ring / update mechanics against a teacher-only replay of the same keys, and a short distillation run."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import distill_ref as D  # noqa: E402
import ntuple_ref as N  # noqa: E402
from src.g2048 import native as nv  # noqa: E402
from src.g2048.engine import seed_key  # noqa: E402
from src.ppo import DistillTrainer, NTupleNetwork, NTupleTrainer, PPOAgent  # noqa: E402
from src.runs import evaluate_agent  # noqa: E402

pytestmark = pytest.mark.gpu
SLACK = 259


def _guarded(n, dtype, dev):
    """-> (whole, view): ``view`` = n + SLACK elements that start SLACK elements into ``whole``, every byte 0xA5."""
    size = torch.empty((), dtype=dtype).element_size()
    whole = torch.full(((2 * SLACK + n) * size,), 0xA5, dtype=torch.uint8, device=dev).view(dtype)
    return whole, whole[SLACK:]


def _intact(whole, n):
    """Every byte before the view and past its first n elements still holds the guard pattern."""
    raw = whole.view(torch.uint8)
    size = whole.element_size()
    return bool((raw[:SLACK * size] == 0xA5).all()) and bool((raw[(SLACK + n) * size:] == 0xA5).all())


def _to(d, dev):
    return {k: None if v is None else v.to(dev) for k, v in d.items()}


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("M", D.MS)
def test_loss_against_the_float64_reference(dev, M, bf16):
    """M in {1, 63, 255, 256, 257, 2055} x {f32, bf16} x {mask bits, NULL} x {values, NULL} x (tau, grad_scale) in {0, 1, 100} x {None,
    1024, 1000}: the planted rows first, every output inside guard bytes, two launches bit-identical, ``running`` accumulated,
    everything within the bounds of distill_ref (worst error / bound printed per stage)."""
    dt = torch.bfloat16 if bf16 else torch.float32
    n_ws = nv.distill_loss_workspace_floats(M)
    for masks in (True, False):
        for with_v in (True, False):
            d = D.inputs(M, bf16=bf16, masks=masks, values=with_v)
            g = _to(d, dev)
            for tau in D.TAUS:
                for scale in D.SCALES:
                    ref = D.distill_ref(d["logits"], d["values"], d["mask_bits"], d["teacher_q"], d["value_target"], tau, D.C_VALUE,
                                        D.C_ENTROPY, scale)
                    D.planted_expectations(ref, d, tau)
                    sc = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=dev)
                    running = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0], dtype=torch.float64, device=dev)
                    runs = []
                    for _ in range(2):
                        bufs = dict(new_logp=_guarded(M, torch.float32, dev), sums=_guarded(5, torch.float32, dev),
                                    dlogits=_guarded(4 * M, dt, dev), ws=_guarded(n_ws, torch.float32, dev))
                        if with_v:
                            bufs["dvalues"] = _guarded(M, dt, dev)
                        out = (bufs["new_logp"][1], bufs["sums"][1], bufs["dlogits"][1], bufs["dvalues"][1] if with_v else None)
                        got = nv.distill_loss(g["logits"], g["values"], g["mask_bits"], g["teacher_q"], g["value_target"], tau, D.C_VALUE,
                                              D.C_ENTROPY, grad_scale=sc, running=running, workspace=bufs["ws"][1], out=out)
                        torch.cuda.synchronize()
                        assert got[3] is None if not with_v else got[3] is out[3]
                        for k, n in (("new_logp", M), ("sums", 5), ("dlogits", 4 * M), ("ws", n_ws), ("dvalues", M)):
                            if k in bufs:
                                assert _intact(bufs[k][0], n), (k, masks, with_v, tau, scale)
                        runs.append((got[0][:M].clone(), got[1][:5].clone(), got[2][:4 * M].clone(),
                                     got[3][:M].clone() if with_v else None))
                    a, b = runs
                    for x, y in zip(a, b):
                        if x is not None:
                            assert torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32),
                                               y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32))
                    want_running = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0], dtype=torch.float64) + 2 * a[1].double().cpu()
                    assert torch.equal(running.cpu(), want_running)
                    bad = D.distill_check(ref, a[0].cpu(), a[1].cpu(), a[2].cpu(), None if a[3] is None else a[3].cpu(), planted=D.N_PLANTED,
                                          show=f"gpu M={M} bf16={bf16} masks={masks} v={with_v} tau={tau} scale={scale}")
                    assert not bad, bad
                    assert not torch.isnan(a[0]).any() and not torch.isnan(a[2].float()).any() and not torch.isnan(a[1]).any()
                    if not with_v:
                        assert float(a[1][1]) == 0.0
                    if masks and M > 4:
                        assert not a[2][16:20].float().any() and float(a[0][4]) == 0.0  # no legal action: all zeros
                    if masks and M > 3:
                        assert not a[2][12:16].float().any() and float(a[0][3]) == 0.0  # a single legal action: log-probability 0


@pytest.mark.parametrize("with_vt", [True, False], ids=["vt", "no_vt"])
@pytest.mark.parametrize("M", [1, 255, 257])
def test_gather_equals_index_select(dev, M, with_vt):
    Nr = 1000
    g = torch.Generator().manual_seed(5 + M)
    boards = torch.randint(0, 256, (Nr, 16), generator=g, dtype=torch.uint8).to(dev)
    masks = torch.randint(0, 16, (Nr,), generator=g).to(torch.uint8).to(dev)
    q = torch.randn(Nr, 4, generator=g).to(dev)
    vt = torch.randn(Nr, generator=g).to(dev) if with_vt else None
    special = [0, Nr - 1, -5, Nr + 5]
    idx_sets = [[s] for s in special] if M == 1 else [special + torch.randint(0, Nr, (M - 4,), generator=g).tolist()]
    for ids in idx_sets:
        idx = torch.tensor(ids, dtype=torch.int64, device=dev)
        bufs = dict(obs=_guarded(16 * M, torch.uint8, dev), masks=_guarded(M, torch.uint8, dev), q=_guarded(4 * M, torch.float32, dev))
        if with_vt:
            bufs["vt"] = _guarded(M, torch.float32, dev)
        # the views start SLACK elements into an allocation: boards and q need 16-byte alignment, so step to the next multiple
        out = {}
        for k, (whole, view) in bufs.items():
            skip = (-view.data_ptr()) % 16 // view.element_size()
            out[k] = view[skip:]
        out.setdefault("vt", None)
        n_of = dict(obs=16 * M, masks=M, q=4 * M, vt=M)
        nv.distill_gather(idx, boards, masks, q, vt, out=out)
        torch.cuda.synchronize()
        c = idx.clamp(0, Nr - 1)
        assert torch.equal(out["obs"][:16 * M].reshape(M, 16), boards.index_select(0, c))
        assert torch.equal(out["masks"][:M], masks.index_select(0, c))
        assert torch.equal(out["q"][:4 * M].view(torch.int32).reshape(M, 4), q.index_select(0, c).view(torch.int32))
        if with_vt:
            assert torch.equal(out["vt"][:M].view(torch.int32), vt.index_select(0, c).view(torch.int32))
        for k, (whole, view) in bufs.items():
            raw, size = whole.view(torch.uint8), whole.element_size()
            start = out[k].data_ptr() - whole.data_ptr()
            assert bool((raw[:start] == 0xA5).all()) and bool((raw[start + n_of[k] * size:] == 0xA5).all()), k


# ------------------------------------------------------------------------------------------------------------- trainer mechanics
def _small_agent(seed=0):
    torch.manual_seed(seed)
    return PPOAgent(observation_dim=31, action_dim=4, hidden_dim=64, d_model=64, nhead=2, num_layers=2, dim_feedforward=128, dropout=0.0,
                    reduction="cls")


def _small_teacher(dev):
    net = NTupleNetwork(N.SMALL, device=dev)
    net.weights.copy_(torch.from_numpy(N.small_weights().copy()).to(dev))
    return net


def _teacher_only_replay(net, num_envs, lock_steps, seed, dev, rng_mode):
    """What NTupleTrainer.train drives, without a learner: chain_keys, reset_fused, scores, policy_step_autoreset on the masked argmax.
    -> per-step (boards before the step, mask nibble, q, v)."""
    B = num_envs
    u8, f32 = torch.uint8, torch.float32
    boards, masks = torch.empty((B, 16), dtype=u8, device=dev), torch.empty(B, dtype=u8, device=dev)
    done, ep_len = torch.empty(B, dtype=u8, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    tr = [torch.empty((1, B, 16), dtype=u8, device=dev), torch.empty((1, B), dtype=u8, device=dev)] + \
         [torch.empty((1, B), dtype=f32, device=dev) for _ in range(3)]
    key, sub = nv.chain_keys(seed_key(seed), 1, rng_mode)
    nv.reset_fused(sub[0], boards, masks, done, ep_len, B, 0, rng_mode)
    key, subs = nv.chain_keys(key, 2 * lock_steps, rng_mode)
    rows = []
    for t in range(lock_steps):
        q, v = net.scores(boards)
        before = boards.clone()
        nv.policy_step_autoreset(subs[2 * t], subs[2 * t + 1], q, v, True, False, 0, boards, masks, ep_len, *tr, B, 0, rng_mode)
        assert torch.equal(tr[0][0], before)
        rows.append((before, (tr[1][0] >> 2) & 15, q, v))
    return rows


def test_trainer_collect_ring_and_update(dev):
    """DistillTrainer(num_envs=64, capacity=512, batch_size=128) on a small agent and an N.SMALL teacher: two trainers with the same
    seed fill identical rings; with beta=1 the ring equals a teacher-only replay of the same keys, and wraps at ``capacity``; after
    update(4) every parameter with a gradient path has changed and, with value_coef=0, no critic-head parameter has."""
    net = _small_teacher(dev)
    kw = dict(num_envs=64, capacity=512, batch_size=128, seed=3, device=dev)
    a, b = DistillTrainer(_small_agent(), net, **kw), DistillTrainer(_small_agent(), net, **kw)
    assert a.collect(8) == 512 and b.collect(8) == 512 and a.filled == 512 and a.pos == 0
    for k in a.ring:
        assert torch.equal(a.ring[k], b.ring[k]), k
    assert int(a.ring["masks"].max()) <= 15 and int(a.ring["masks"].min()) >= 1 and int(a.student_top) >= 1

    bc = DistillTrainer(_small_agent(), net, beta=1.0, value_scale=0.5, **kw)
    assert bc.n_teacher == 64
    bc.collect(8)
    rows = _teacher_only_replay(net, 64, 10, 3, dev, bc.rng_mode)
    for t in range(8):
        s = slice(64 * t, 64 * (t + 1))
        boards, mask, q, v = rows[t]
        assert torch.equal(bc.ring["boards"][s], boards) and torch.equal(bc.ring["masks"][s], mask)
        assert torch.equal(bc.ring["q"][s], q) and torch.equal(bc.ring["vt"][s], v * 0.5)
    # the first 32 envs of the mixed trainer play the teacher too, but the boards differ as soon as the others' moves do not: only
    # the first lock-step (the reset boards) is common
    assert torch.equal(a.ring["boards"][:64], bc.ring["boards"][:64])
    old = {k: v.clone() for k, v in bc.ring.items()}
    bc.collect(2)  # wraps: rows 0 .. 127 are lock-steps 8 and 9, the rest stays
    assert bc.pos == 128 and bc.filled == 512 and bc.rows == 640 and bc.lock_steps == 10
    for t in (8, 9):
        s = slice(64 * (t - 8), 64 * (t - 7))
        assert torch.equal(bc.ring["boards"][s], rows[t][0]) and torch.equal(bc.ring["q"][s], rows[t][2])
    for k in old:
        assert torch.equal(bc.ring[k][128:], old[k][128:]), k

    before = {n: p.detach().clone() for n, p in a.agent.named_parameters()}
    sums = a.update(4)
    torch.cuda.synchronize()
    assert a.updates == 4 and bool(torch.isfinite(sums).all()) and float(sums[1]) == 0.0
    for n, p in a.agent.named_parameters():
        if n.startswith("critic."):
            assert torch.equal(p.detach(), before[n]), n
        else:
            assert not torch.equal(p.detach(), before[n]), n
    # value_coef > 0: the critic is regressed too
    c = DistillTrainer(_small_agent(), net, value_coef=0.5, value_scale=1e-3, **kw)
    c.collect(8)
    before = {n: p.detach().clone() for n, p in c.agent.named_parameters() if n.startswith("critic.")}
    sums = c.update(2)
    assert float(sums[1]) > 0.0 and all(not torch.equal(p.detach(), before[n]) for n, p in c.agent.named_parameters() if n in before)
    out = a.train(2, 2, 2)
    assert int(out["rows"]) == 256 and 0.0 <= float(out["agreement"]) <= 1.0 and float(out["ce"]) > 0.0
    sc = a.score(bc)
    assert 0.0 <= float(sc["agreement"]) <= 1.0 and float(sc["ce"]) > 0.0


# ------------------------------------------------------------------------------------------------------------- it learns
MODEL = dict(observation_dim=31, action_dim=4, hidden_dim=512, d_model=256, nhead=8, num_layers=4, dim_feedforward=1024, dropout=0.1,
             reduction="cls")  # run/train_to_2048.py's
LEARN = dict(num_envs=1024, capacity=16384, batch_size=1024)
ITERATIONS, COLLECT_STEPS, MINIBATCHES = 12, 8, 8
HELD_STEPS = ITERATIONS * COLLECT_STEPS  # the held-out envs run as long as the training envs: the same mix of early and later boards
# the CPU loop at this size, training seeds 0 / 1 / 2 (docstring of test_it_learns)
CPU_AGREEMENT_GAIN = (0.1556, 0.1340, 0.2081)
CPU_TILE_RATIO = (254.72 / 194.24, 207.36 / 113.44, 225.28 / 77.92)
MIN_AGREEMENT_GAIN = 0.5 * min(CPU_AGREEMENT_GAIN)
MIN_TILE_RATIO = 2.0 if min(CPU_TILE_RATIO) >= 3.0 else min(CPU_TILE_RATIO) / 1.5


def test_it_learns(dev):
    """Teacher: the default n-tuple network after 2 400 TC lock-steps at 1 024 envs (as ``test_gpu_ntuple_tc.test_it_learns`` trains it).
    Student: the run/train_to_2048.py model, ``torch.manual_seed(0)``.  ``DistillTrainer`` at 1 024 envs, batch 1 024, ``tau=0``,
    ``beta=0.5``, 12 iterations of 8 lock-steps and 8 minibatches (96 optimiser steps, 98 304 rows).  Held out: the ring of a second trainer
    on seed 1 that runs its envs for the same 96 lock-steps before training starts (98 304 rows; the student's half of it is the untrained
    student's states), so that it holds the mix of early and later boards the training ring holds.  (A held-out ring of the first 8
    lock-steps only holds openings, on which a barely trained network answers with one move for every board: its agreement then jumps
    between the shares of the teacher's four moves, 0.41 / 0.34 / 0.20, from one iteration to the next and measures nothing.)
    Asserted: the greedy agreement with the teacher's move on the held-out ring rises by at least MIN_AGREEMENT_GAIN, and the greedy mean
    max tile over 100 episodes (seed 42) is at least MIN_TILE_RATIO times the untrained agent's on the same seeds.
    Both thresholds come from the same loop on the CPU at this size (torch CPU student in f32, ``ntuple_ref.scores`` teacher trained by
    ``ntuple_tc_ref.simulate_training``, numpy's RNG for the spawns as ``simulate_training``, held-out loop on seed 1000 + s), training
    seeds s = 0 / 1 / 2:
        held-out agreement  0.3263 -> 0.4819   0.2891 -> 0.4232   0.2645 -> 0.4726     gains 0.1556 / 0.1340 / 0.2081
        mean max tile       194.2 -> 254.7     113.4 -> 207.4     77.9 -> 225.3        ratios 1.31 / 1.83 / 2.89
    Agreement: half the smallest gain, 0.0670.  Tile: the three seeds do NOT all show 3 x, so "trained >= 2 x untrained" is not asserted;
    what all three support with a 1.5 x margin is 1.31 / 1.5 = 0.87 x, and that is what is asserted: at 96 optimiser steps the tile
    assertion only says that distillation does not make the play much worse, the agreement assertion carries the test.  (The untrained
    agents differ a lot, 78 to 194, which is most of the spread of the ratios.)  What longer runs give is measured, not asserted:
    DESIGN.md, "Distillation", Strength.  On the MI355X: agreement 0.3318 -> 0.4519 (gain 0.1202), tile 188.2 -> 204.5 (1.09 x)."""
    net = NTupleNetwork(device=dev)
    teacher = NTupleTrainer(net, num_envs=1024, alpha=1.0, seed=0, device=dev, learner="tc")
    teacher.train(2400)
    del teacher
    torch.manual_seed(0)
    agent = PPOAgent(**MODEL)
    held = DistillTrainer(agent, net, num_envs=1024, capacity=1024 * HELD_STEPS, batch_size=1024, tau=0.0, beta=0.5, seed=1, device=dev)
    held.collect(HELD_STEPS)
    tr = DistillTrainer(agent, net, tau=0.0, beta=0.5, seed=0, device=dev, **LEARN)
    before = float(tr.score(held)["agreement"])
    tile0 = evaluate_agent(agent, dev, 100, seed=42)["mean_max_tile"]
    out = tr.train(ITERATIONS, COLLECT_STEPS, MINIBATCHES)
    after = float(tr.score(held)["agreement"])
    tile1 = evaluate_agent(agent, dev, 100, seed=42)["mean_max_tile"]
    print(f"held-out agreement {before:.4f} -> {after:.4f} (gain {after - before:.4f}, asserted >= {MIN_AGREEMENT_GAIN:.4f}); greedy mean max "
          f"tile over 100 episodes {tile0:.1f} -> {tile1:.1f} (ratio {tile1 / tile0:.2f}, asserted >= {MIN_TILE_RATIO:.2f}); training ce "
          f"{float(out['ce']):.4f}, agreement {float(out['agreement']):.4f}, {int(out['rows'])} rows, {tr.updates} updates")
    assert int(out["rows"]) == 1024 * ITERATIONS * COLLECT_STEPS and tr.updates == ITERATIONS * MINIBATCHES
    assert after - before >= MIN_AGREEMENT_GAIN
    assert tile1 >= MIN_TILE_RATIO * tile0
