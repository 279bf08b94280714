"""Numpy restatement of temporal-coherence (TC) learning on the n-tuple network (include/g2048.h, "n-tuple TC learning").  TEST
INFRASTRUCTURE ONLY.

Written from the definition, on top of ``ntuple_ref``: e, delta and c are TD(0)'s (``td_deltas``); per lock-step

  accumulate : acc += delta, abs_acc += |delta|, cnt += 1 at every (g, t) entry of every env with flag != 0
  apply      : where n = cnt > 0:  d = rdiv(acc, n), a = rdiv(abs_acc, n)            (a >= |d|)
               step = d if A == 0 else rdiv(d |E|, A);  weights = sat(weights + step)  (the rate |E| / A is read before the update)
               E += d, A += a;  if A >= 2^31: E = sign(E) (|E| / 2), A >>= 1           (|E| <= A < 2^31)
               acc = abs_acc = cnt = 0

``a >= |d|`` and ``|E| <= A < 2^31`` are asserted on every call.
"""
from __future__ import annotations

import functools

import numpy as np

import ntuple_ref as N
from oracle import g2048_oracle as npo

F32 = np.float32
LIMIT = 2 ** 31


def zero_coherence(weights):
    return np.zeros(weights.shape, np.int32), np.zeros(weights.shape, np.int32)


def hit_entries(prev_after, flag, tuples) -> np.ndarray:
    """-> int64 [live, 8 m]: the flat positions t 16^L + idx(view_g, t) of every env with flag != 0 (repeats included)."""
    live = np.nonzero(np.asarray(flag) != 0)[0]
    e = N.entries(np.asarray(prev_after)[live], tuples)
    size = 16 ** N.cells_array(tuples).shape[1]
    return (e + size * np.arange(e.shape[2], dtype=np.int64)).reshape(len(live), 8 * e.shape[2])


def tc_accumulate(prev_after, flag, delta, tuples, acc, abs_acc, cnt):
    N.accumulate(prev_after, flag, delta, tuples, acc, cnt)
    live = np.nonzero(np.asarray(flag) != 0)[0]
    flat = hit_entries(prev_after, flag, tuples)
    np.add.at(abs_acc.reshape(-1), flat.reshape(-1), np.repeat(np.abs(delta[live].astype(np.int64)), flat.shape[1]))
    hit = np.unique(flat)
    assert int(cnt.reshape(-1)[hit].sum(dtype=np.int64)) == flat.size  # cnt was all-zero before: nothing else is pending
    return hit


def tc_apply(weights, acc, abs_acc, cnt, coh_e, coh_a, hit, stats=None):
    """The entries ``hit`` (flat positions, each once; all of those with cnt > 0).  In place on everything."""
    w, s, sa, c, ce, ca = (x.reshape(-1) for x in (weights, acc, abs_acc, cnt, coh_e, coh_a))
    n = c[hit].astype(np.int64)
    assert (n > 0).all()
    d, a = N.rdiv(s[hit], n), N.rdiv(sa[hit], n)
    assert (a >= np.abs(d)).all() and (np.abs(d) <= 2 ** 30).all()
    E, A = ce[hit].astype(np.int64), ca[hit].astype(np.int64)
    assert (np.abs(E) <= A).all() and (A < LIMIT).all() and (A >= 0).all()
    step = np.where(A == 0, d, N.rdiv(d * np.abs(E), np.maximum(A, 1)))
    moved = w[hit].astype(np.int64) + step
    w[hit] = np.clip(moved, -LIMIT, LIMIT - 1).astype(np.int32)
    E, A = E + d, A + a
    big = A >= LIMIT
    E = np.where(big, np.sign(E) * (np.abs(E) // 2), E)
    A = np.where(big, A >> 1, A)
    assert (np.abs(E) <= A).all() and (A < LIMIT).all()
    ce[hit], ca[hit] = E.astype(np.int32), A.astype(np.int32)
    s[hit], sa[hit], c[hit] = 0, 0, 0
    if stats is not None:
        stats["halved"] = stats.get("halved", 0) + int(big.sum())
        stats["saturated"] = stats.get("saturated", 0) + int(((moved < -LIMIT) | (moved > LIMIT - 1)).sum())
        stats["slowed"] = stats.get("slowed", 0) + int(((A > 0) & (step != d)).sum())


def tc_step(prev_after, flag, target, weights, coh_e, coh_a, tuples, frac_bits: int, alpha: float, acc=None, abs_acc=None,
            cnt=None, stats=None):
    """accumulate + apply, in place on weights, coh_e, coh_a -> td_error f32 [B]."""
    acc = np.zeros(weights.shape, np.int64) if acc is None else acc
    abs_acc = np.zeros(weights.shape, np.int64) if abs_acc is None else abs_acc
    cnt = np.zeros(weights.shape, np.int32) if cnt is None else cnt
    delta, e = N.td_deltas(prev_after, flag, target, weights, tuples, frac_bits, alpha)
    if stats is not None:
        stats["clamped"] = stats.get("clamped", 0) + int((np.abs(delta.astype(np.int64)) == 2 ** 30).sum())
    hit = tc_accumulate(prev_after, flag, delta, tuples, acc, abs_acc, cnt)
    tc_apply(weights, acc, abs_acc, cnt, coh_e, coh_a, hit, stats)
    return e


def coherence(coh_e, coh_a):
    """-> (entries with A > 0, mean of |E| / A over them as float64; 0.0 if there is none)."""
    on = coh_a.reshape(-1) > 0
    n = int(on.sum())
    rate = np.abs(coh_e.reshape(-1)[on].astype(np.float64)) / coh_a.reshape(-1)[on].astype(np.float64)
    return n, float(rate.mean()) if n else 0.0


class _Learner:
    """One learner's step with its tables: ``step(prev, flag, target)`` in place on weights."""

    def __init__(self, learner, weights, tuples, frac_bits, alpha, coh_e=None, coh_a=None):
        if learner not in ("td0", "tc"):
            raise ValueError(learner)
        self.learner, self.w, self.tuples, self.F, self.alpha = learner, weights, tuples, frac_bits, alpha
        self.acc, self.cnt = np.zeros(weights.shape, np.int64), np.zeros(weights.shape, np.int32)
        if learner == "tc":
            self.abs_acc = np.zeros(weights.shape, np.int64)
            self.coh_e = np.zeros(weights.shape, np.int32) if coh_e is None else coh_e
            self.coh_a = np.zeros(weights.shape, np.int32) if coh_a is None else coh_a

    def step(self, prev, flag, target):
        if self.learner == "td0":
            return N.td_step(prev, flag, target, self.w, self.tuples, self.F, self.alpha, self.acc, self.cnt)
        return tc_step(prev, flag, target, self.w, self.coh_e, self.coh_a, self.tuples, self.F, self.alpha, self.acc, self.abs_acc,
                       self.cnt)


def replay_training(weights, tuples, boards, meta, alpha: float = 1.0, frac_bits: int = 12, learner: str = "tc", coh_e=None,
                    coh_a=None):
    """``ntuple_ref.replay_training`` with the learner chosen: -> (scores [T,B,4], targets [T,B]); in place on weights and, for
    "tc", on coh_e / coh_a (zero tables are used if none are given)."""
    B = boards.shape[1]
    lr = _Learner(learner, weights, tuples, frac_bits, alpha, coh_e, coh_a)
    prev, flag = np.zeros((B, 16), np.uint8), np.zeros(B, np.uint8)
    qs, vs = [], []
    for t in range(len(boards)):
        q, v, _ = N.scores(boards[t], weights, tuples, frac_bits)
        lr.step(prev, flag, v)
        prev, flag = N.link(boards[t], meta[t])
        qs.append(q)
        vs.append(v)
    return np.stack(qs), np.stack(vs)


def engine_training(weights, tuples, num_envs: int, lock_steps: int, alpha: float = 1.0, frac_bits: int = 12, seed: int = 0,
                    mode: int = npo.MODE_PARTITIONABLE, learner: str = "tc", coh_e=None, coh_a=None):
    """``ntuple_ref.engine_training`` (the C oracle's env on the engine's key chain) with the learner chosen."""
    from oracle import c_oracle as orc

    B = num_envs
    lr = _Learner(learner, weights, tuples, frac_bits, alpha, coh_e, coh_a)
    _, subs = orc.chain(npo.key(seed), 1 + 2 * lock_steps, mode)
    b, m, _ = orc.init(orc.split(subs[0], B, mode), mode)
    prev, flag = np.zeros((B, 16), np.uint8), np.zeros(B, np.uint8)
    rec = dict(boards=[], meta=[], scores=[], targets=[])
    episodes = 0
    for t in range(lock_steps):
        q, v, legal = N.scores(b, weights, tuples, frac_bits)
        lr.step(prev, flag, v)
        a = N.masked_argmax(q, legal)
        nb, nm, nd, _ = orc.step(b, m, np.zeros(B, np.uint8), a, orc.split(subs[2 + 2 * t], B, mode), mode)
        meta = (a.astype(np.uint8) | (m.astype(np.uint8) << 2) | (nd.astype(np.uint8) << 6)).astype(np.uint8)
        for k, x in zip(("boards", "meta", "scores", "targets"), (b, meta, q, v)):
            rec[k].append(np.array(x))
        prev, flag = N.link(b, meta)
        if nd.any():
            fb, fm, _ = orc.init(orc.split(npo.fold_in(subs[2 + 2 * t], 0xFFFFFFFF), B, mode), mode)
            nb, nm = np.where(nd[:, None] != 0, fb, nb), np.where(nd != 0, fm, nm)
            episodes += int(nd.sum())
        b, m = nb, nm
    out = {k: np.stack(x) for k, x in rec.items()}
    out["episodes"] = episodes
    return out


def simulate_training(weights, tuples, num_envs: int, lock_steps: int, alpha: float = 1.0, frac_bits: int = 12, seed: int = 0,
                      learner: str = "tc", coh_e=None, coh_a=None):
    """``ntuple_ref.simulate_training`` (numpy's RNG for the spawns) with the learner chosen.  In place -> episodes finished."""
    rng = np.random.default_rng(seed)
    lr = _Learner(learner, weights, tuples, frac_bits, alpha, coh_e, coh_a)
    boards = N._fresh(num_envs, rng)
    prev, flag = np.zeros((num_envs, 16), np.uint8), np.zeros(num_envs, np.uint8)
    episodes = 0
    for _ in range(lock_steps):
        a, v, _ = N._greedy(boards, weights, tuples, frac_bits)
        lr.step(prev, flag, v)
        after, _ = npo.move(boards, a.astype(np.int32))
        nxt = N._spawn(after, rng)
        done = ~npo.legal_mask(nxt).any(axis=1)
        prev, flag = after, np.where(done, 2, 1).astype(np.uint8)
        nxt[done] = N._fresh(int(done.sum()), rng)
        episodes += int(done.sum())
        boards = nxt
    return episodes


# ---------------------------------------------------------------------------------------------- shared cases
# the four shapes of test_ntuple_abi.py's CASES
CASES = [(N.SMALL, 12), (((0, 1, 2, 3), (4, 5, 6, 7), (0, 4, 8, 12), (5, 6, 9, 10), (15, 0, 3, 12)), 0), (((7,),), 20),
         (tuple((i, i + 1, i + 4) for i in range(8)), 7)]


def one_step_inputs(tuples, F, n=400):
    """n boards (the special ones first), flags 0 / 1 / 2 mixed, targets of scale 500, random weights."""
    rng = np.random.default_rng(100 + F)
    prev = N.boards_for(n, seed=len(tuples))
    flag = rng.integers(0, 3, n).astype(np.uint8)
    flag[:9] = [1, 2, 1, 2, 1, 2, 1, 0, 1][:min(n, 9)]  # the special boards take part
    target = (rng.standard_normal(n) * 500).astype(F32)
    return prev, flag, target, N.random_weights(tuples, seed=F)


@functools.lru_cache(maxsize=None)
def sequence_case(alpha: float, scale: float, extreme: bool, steps: int = 6):
    """``steps`` consecutive TC steps on SMALL (F = 12) on the same 200 boards and flags with fresh random targets of ``scale`` at
    each step, from zero coherence.  ``extreme``: a third of the weights start within 50 of 2^31 - 1 and a third within 50 of -2^31.
    -> dict with the inputs, the restatement's tables and td_error after every step and its ``stats``."""
    rng = np.random.default_rng(3)
    prev = N.boards_for(200, seed=4)
    flag = rng.integers(0, 3, len(prev)).astype(np.uint8)
    targets = (rng.standard_normal((steps, len(prev))) * scale).astype(F32)
    w0 = N.random_weights(N.SMALL, seed=8)
    if extreme:
        w0[:, ::3] = 2 ** 31 - 1 - rng.integers(0, 50, w0[:, ::3].shape)
        w0[:, 1::3] = -2 ** 31 + rng.integers(0, 50, w0[:, 1::3].shape)
    w = w0.copy()
    ce, ca = zero_coherence(w)
    stats, after = {}, []
    for t in range(steps):
        e = tc_step(prev, flag, targets[t], w, ce, ca, N.SMALL, 12, alpha, stats=stats)
        after.append(dict(weights=w.copy(), coh_e=ce.copy(), coh_a=ca.copy(), td_error=e))
    out = dict(prev=prev, flag=flag, targets=targets, w0=w0, after=after, stats=stats, alpha=alpha)
    for v in (prev, flag, targets, w0):
        v.setflags(write=False)
    return out
