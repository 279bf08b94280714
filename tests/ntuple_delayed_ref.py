"""Numpy restatement of delayed TD(lambda) / TC(lambda) on the n-tuple network (include/g2048.h, "n-tuple delayed TD(lambda)").  TEST
INFRASTRUCTURE ONLY.

Written from the definition, one env at a time, on top of ``ntuple_ref`` / ``ntuple_tc_ref`` / ``ntuple_stage_ref`` (``entries`` through
``accumulate`` and ``hit_entries``, ``apply``, ``tc_apply``, ``rdiv`` inside them, ``stage``).  Ring: hist u8 [h, B, 16], hist_err f32
[h, B], hist_len u8 [B]; the newest afterstate is in slot ``head``, the state j steps back in slot (head - j + 1) mod h.

  accumulate : e = f32(target if flag == 1 else 0) - V(hist[head])  -> td_error, hist_err[head]
               x_1 = e, x_{j+1} = f32(hist_err[(head - j) mod h] + f32(lam * x_j)) for j + 1 <= hist_len     (np.float32 scalars)
               state j is due if flag == 2, or if flag == 1 and j == h;  delta_j = int32(rint(clip(f32(x_j * c), +-2^30)))
               acc += delta_j, cnt += 1 (TC: abs_acc += |delta_j|) at the 8 m entries of the due board, in the board's own stage
  apply      : every entry with cnt > 0: ``ntuple_ref.apply`` / ``ntuple_tc_ref.tc_apply``
  link       : prev_after = hist[slot] = the afterstate, hist_len = min((0 if the old flag == 2 else hist_len) + 1, h)

All tables are [S, m, 16^L]; an unstaged network is S = 1 with no thresholds (``as_staged`` makes the view).
"""
from __future__ import annotations

import functools

import numpy as np

import ntuple_ref as N
import ntuple_stage_ref as G
import ntuple_tc_ref as T
from oracle import g2048_oracle as npo

F32 = np.float32
MAX_HORIZON = 8


def default_horizon(lam: float) -> int:
    h = 1
    while h < MAX_HORIZON and lam ** h > 0.1:
        h += 1
    return h


def as_staged(a):
    """[m, 16^L] -> a [1, m, 16^L] view; [S, m, 16^L] as it is."""
    return a.reshape((1,) + a.shape) if a.ndim == 2 else a


class Ring:
    def __init__(self, h: int, B: int):
        self.h, self.B = h, B
        self.hist = np.zeros((h, B, 16), np.uint8)
        self.err = np.zeros((h, B), F32)
        self.len = np.zeros(B, np.uint8)

    def copy(self):
        r = Ring(self.h, self.B)
        r.hist, r.err, r.len = self.hist.copy(), self.err.copy(), self.len.copy()
        return r


def lambda_sums(errs, lam) -> list:
    """errs: the TD errors from the newest back -> [x_1, x_2, ...], every operation a rounded np.float32 one."""
    lam = F32(lam)
    xs = [F32(errs[0])]
    for e in errs[1:]:
        xs.append(F32(F32(e) + F32(lam * xs[-1])))
    return xs


def due_states(ring: Ring, flag, target, head: int, lam, weights, tuples, frac_bits: int, alpha: float, tiles):
    """The accumulate half up to the tables, env by env: writes hist_err[head] -> (td_error f32 [B], due boards u8 [n, 16], their
    deltas int32 [n], the env of each)."""
    h, B = ring.h, ring.B
    w = as_staged(weights)
    c = N.step_constant(alpha, frac_bits, len(tuples))
    td_error = np.zeros(B, F32)
    boards, deltas, envs = [], [], []
    values = G.values(ring.hist[head], w, tuples, frac_bits, tiles)  # V of every env's newest afterstate, in its own stage
    for b in range(B):
        f = int(flag[b])
        if f == 0:
            continue
        e = F32(F32(target[b] if f == 1 else 0.0) - values[b])
        td_error[b] = ring.err[head, b] = e
        n = min(int(ring.len[b]), h)
        if n == 0:
            continue
        xs = lambda_sums([ring.err[(head - j + 1) % h, b] for j in range(1, n + 1)], lam)
        for j in range(1, n + 1):
            if f == 2 or j == h:
                d = F32(xs[j - 1] * c)
                boards.append(ring.hist[(head - j + 1) % h, b].copy())
                deltas.append(np.int32(np.rint(np.clip(d, -N.CLAMP, N.CLAMP))))
                envs.append(b)
    boards = np.array(boards, np.uint8).reshape(-1, 16)
    return td_error, boards, np.array(deltas, np.int32), np.array(envs, np.int64)


def step(ring: Ring, flag, target, head: int, lam, weights, tuples, frac_bits: int, alpha: float, tiles=(), learner="td0", coh_e=None,
         coh_a=None, stats=None, tables=None):
    """accumulate + apply, in place on ring.err, weights and (TC) coh_e / coh_a -> td_error f32 [B].  ``tables``: all-zero (acc,
    abs_acc, cnt) of the weights' shape to use instead of fresh ones (they are all-zero again afterwards)."""
    assert learner in ("td0", "tc") and 0 <= head < ring.h
    w = as_staged(weights)
    td_error, boards, deltas, envs = due_states(ring, flag, target, head, lam, weights, tuples, frac_bits, alpha, tiles)
    if stats is not None:
        stats["due"] = stats.get("due", 0) + len(boards)
        stats["clamped"] = stats.get("clamped", 0) + int((np.abs(deltas.astype(np.int64)) == 2 ** 30).sum())
        stats["flushed"] = stats.get("flushed", 0) + len(set(envs[np.asarray(flag)[envs] == 2].tolist()))  # envs, not states
        stats["flushed_short"] = stats.get("flushed_short", 0) + int(((np.asarray(flag)[envs] == 2) & (ring.len[envs] < ring.h)).sum())
    if not len(boards):
        return td_error
    if tables is None:
        tables = np.zeros(w.shape, np.int64), np.zeros(w.shape, np.int64), np.zeros(w.shape, np.int32)
    acc, abs_acc, cnt = (as_staged(t) for t in tables)
    live = np.ones(len(boards), np.uint8)
    for s, sel in G._groups(boards, tiles):
        if learner == "td0":
            N.accumulate(boards[sel], live[sel], deltas[sel], tuples, acc[s], cnt[s])
            N.apply(w[s], acc[s], cnt[s])
        else:
            hit = T.tc_accumulate(boards[sel], live[sel], deltas[sel], tuples, acc[s], abs_acc[s], cnt[s])
            T.tc_apply(w[s], acc[s], abs_acc[s], cnt[s], as_staged(coh_e)[s], as_staged(coh_a)[s], hit, stats)
    for s, _ in G._groups(boards, tiles):
        assert not acc[s].any() and not cnt[s].any() and not abs_acc[s].any()
    return td_error


def link(ring: Ring, boards_row, meta_row, slot: int, old_flag):
    """-> (prev_after u8 [B,16], flag u8 [B]); in place on the ring."""
    prev, flag = N.link(boards_row, meta_row)
    ring.hist[slot] = prev
    ring.len = np.minimum(np.where(np.asarray(old_flag) == 2, 0, ring.len.astype(np.int64)) + 1, ring.h).astype(np.uint8)
    return prev, flag


class Learner:
    """The trainer's learner state with ``lam`` on: tables, ring, the global lock-step count and (staged) the promotion rule."""

    def __init__(self, learner, weights, tuples, frac_bits, alpha, lam, horizon, num_envs, stage_tiles=None, promote_every=64,
                 coh_e=None, coh_a=None):
        self.learner, self.tuples, self.F, self.alpha, self.lam = learner, tuples, frac_bits, alpha, lam
        self.h = default_horizon(lam) if horizon is None else horizon
        self.net = None if stage_tiles is None else G.Net(weights, tuples, stage_tiles, frac_bits)
        self.w, self.every, self.promotions = weights, int(promote_every), []
        self.coh_e = np.zeros(weights.shape, np.int32) if coh_e is None else coh_e
        self.coh_a = np.zeros(weights.shape, np.int32) if coh_a is None else coh_a
        self.ring = Ring(self.h, num_envs)
        self.prev, self.flag = np.zeros((num_envs, 16), np.uint8), np.zeros(num_envs, np.uint8)
        self.count = 0
        self.stats = {}
        self.tables = np.zeros(weights.shape, np.int64), np.zeros(weights.shape, np.int64), np.zeros(weights.shape, np.int32)

    @property
    def tiles(self):
        return () if self.net is None else self.net.tiles

    def check_promotion(self):
        net = self.net
        if net is None or not self.every or self.count == 0 or self.count % self.every:
            return
        top = int(self.prev.max())
        while net.active < net.S and top >= net.stage_tiles[net.active - 1]:
            self.promotions.append((self.count, net.promote()))

    def scores(self, boards):
        if self.net is None:
            return N.scores(boards, self.w, self.tuples, self.F)
        return G.scores(boards, self.w, self.tuples, self.F, self.tiles)

    def learn(self, target):
        return step(self.ring, self.flag, target, (self.count - 1) % self.h, self.lam, self.w, self.tuples, self.F, self.alpha, self.tiles,
                    self.learner, self.coh_e, self.coh_a, self.stats, self.tables)

    def link(self, boards_row, meta_row):
        self.stats["episode_ends"] = self.stats.get("episode_ends", 0) + int(((np.asarray(meta_row) >> 6) & 1).sum())
        self.prev, self.flag = link(self.ring, boards_row, meta_row, self.count % self.h, self.flag)
        self.count += 1


def replay_training(weights, tuples, boards, meta, alpha: float, frac_bits: int = 12, learner: str = "td0", lam=0.5, horizon=None,
                    stage_tiles=None, promote_every: int = 64, coh_e=None, coh_a=None):
    """The learner's half of a recorded run of ``NTupleTrainer(lam=...).train(record=True)`` from lock-step 0 -> (scores [T,B,4],
    targets [T,B], the Learner: promotions, stats).  In place on weights and coh_e / coh_a."""
    lr = Learner(learner, weights, tuples, frac_bits, alpha, lam, horizon, boards.shape[1], stage_tiles, promote_every, coh_e, coh_a)
    qs, vs = [], []
    for t in range(len(boards)):
        lr.check_promotion()
        q, v, _ = lr.scores(boards[t])
        lr.learn(v)
        lr.link(boards[t], meta[t])
        qs.append(q)
        vs.append(v)
    return np.stack(qs), np.stack(vs), lr


def simulate_training(weights, tuples, num_envs: int, lock_steps: int, alpha: float = 1.0, frac_bits: int = 12, seed: int = 0,
                      learner: str = "tc", lam=0.5, horizon=None, coh_e=None, coh_a=None):
    """``ntuple_tc_ref.simulate_training`` (numpy's RNG for the spawns) with ``lam`` on.  In place -> (episodes finished, Learner)."""
    rng = np.random.default_rng(seed)
    lr = Learner(learner, weights, tuples, frac_bits, alpha, lam, horizon, num_envs, coh_e=coh_e, coh_a=coh_a)
    boards = N._fresh(num_envs, rng)
    episodes = 0
    for _ in range(lock_steps):
        a, v, _ = N._greedy(boards, weights, tuples, frac_bits)
        lr.learn(v)
        after, _ = npo.move(boards, a.astype(np.int32))
        nxt = N._spawn(after, rng)
        done = ~npo.legal_mask(nxt).any(axis=1)
        meta = (a.astype(np.uint8) | (done.astype(np.uint8) << 6)).astype(np.uint8)  # link reads the action and the done bit
        lr.link(boards, meta)
        assert np.array_equal(lr.prev, after)
        nxt[done] = N._fresh(int(done.sum()), rng)
        episodes += int(done.sum())
        boards = nxt
    return episodes, lr


def engine_training(weights, tuples, num_envs: int, lock_steps: int, alpha: float = 1.0, frac_bits: int = 12, seed: int = 0,
                    mode: int = npo.MODE_PARTITIONABLE, learner: str = "tc", lam=0.5, horizon=None, stage_tiles=None,
                    promote_every: int = 64, coh_e=None, coh_a=None):
    """``ntuple_tc_ref.engine_training`` (the trainer's whole loop on the C oracle's env and the engine's key chain) with ``lam`` on
    -> the record of ``train(record=True)`` as numpy arrays plus "episodes" and "learner"."""
    from oracle import c_oracle as orc

    B = num_envs
    lr = Learner(learner, weights, tuples, frac_bits, alpha, lam, horizon, B, stage_tiles, promote_every, coh_e, coh_a)
    _, subs = orc.chain(npo.key(seed), 1 + 2 * lock_steps, mode)
    b, m, _ = orc.init(orc.split(subs[0], B, mode), mode)
    rec = dict(boards=[], meta=[], scores=[], targets=[])
    episodes = 0
    for t in range(lock_steps):
        lr.check_promotion()
        q, v, legal = lr.scores(b)
        lr.learn(v)
        a = N.masked_argmax(q, legal)
        nb, nm, nd, _ = orc.step(b, m, np.zeros(B, np.uint8), a, orc.split(subs[2 + 2 * t], B, mode), mode)
        meta = (a.astype(np.uint8) | (m.astype(np.uint8) << 2) | (nd.astype(np.uint8) << 6)).astype(np.uint8)
        for k, x in zip(("boards", "meta", "scores", "targets"), (b, meta, q, v)):
            rec[k].append(np.array(x))
        lr.link(b, meta)
        if nd.any():
            fb, fm, _ = orc.init(orc.split(npo.fold_in(subs[2 + 2 * t], 0xFFFFFFFF), B, mode), mode)
            nb, nm = np.where(nd[:, None] != 0, fb, nb), np.where(nd != 0, fm, nm)
            episodes += int(nd.sum())
        b, m = nb, nm
    out = {k: np.stack(x) for k, x in rec.items()}
    out.update(episodes=episodes, learner=lr)
    return out


# ---------------------------------------------------------------------------------------------- shared cases
SHAPES = [(((0, 1),), 12), (N.SMALL, 12), (tuple((i, i + 4) for i in range(8)), 7), (N.WIDE, 12)]  # (m, L) = (1,2) (3,2) (8,2) (2,6)
STAGE_TILES = (3, 6)


def ring_case(tuples, F, h: int, B: int, tiles=(), seed: int = 0, scale: float = 500.0):
    """A ring of B envs over horizon h in which hist_len takes every value 0 .. h under each of flag 0, 1 and 2 (as far as B
    allows), boards from ``ntuple_ref.boards_for`` (tiles up to 17); with ``tiles`` env 0 holds a board in a higher stage than its
    newer neighbours; env 1 (if there is one) holds the SAME board at every ring position; errors of ``scale`` in hist_err.
    -> dict(ring, flag, target, w0)."""
    rng = np.random.default_rng(1000 * h + B + seed)
    ring = Ring(h, B)
    pool = N.boards_for(h * B + 9, seed=seed + 3)
    ring.hist[:] = pool[rng.permutation(len(pool))[:h * B]].reshape(h, B, 16)
    ring.err[:] = (rng.standard_normal((h, B)) * scale).astype(F32)
    combos = [(f, n) for n in range(h + 1) for f in (1, 2, 0)]
    flag = np.array([combos[b % len(combos)][0] for b in range(B)], np.uint8)
    ring.len[:] = [combos[b % len(combos)][1] for b in range(B)]
    if B > 1:
        ring.hist[:, 1] = pool[4]
        flag[1], ring.len[1] = 2, h
    if tiles:
        hi = np.zeros(16, np.uint8)
        hi[0], hi[5] = 1, max(tiles)
        ring.hist[:, 0] = np.array([1, 2, 1, 0] * 4, np.uint8)                 # stage 0 everywhere ...
        ring.hist[h // 2, 0] = hi                                              # ... but one slot in the top stage
        flag[0], ring.len[0] = 2, h
    target = (rng.standard_normal(B) * scale).astype(F32)
    if tiles:
        w0 = np.stack([N.random_weights(tuples, seed=40 + s) for s in range(len(tiles) + 1)])
    elif tuples == N.WIDE:
        w0 = N.wide_weights()  # 128 MB: the shared read-only table
    else:
        w0 = N.random_weights(tuples, seed=F + len(tuples))
    return dict(ring=ring, flag=flag, target=target, w0=w0)


@functools.lru_cache(maxsize=None)
def collision_case(h: int = 3, B: int = 600, same: int = 200, seed: int = 5):
    """One step under heavy collision on SMALL: ``same`` envs hold identical rings (so every due state collides), flags mixed.
    -> dict(ring, flag, target) (read-only inputs)."""
    c = ring_case(N.SMALL, 12, h, B, seed=seed)
    ring, flag = c["ring"], c["flag"]
    ring.hist[:, :same] = ring.hist[:, :1]
    ring.len[:same] = h
    flag[:same] = np.where(np.arange(same) % 3 == 0, 2, 1)
    perm = np.random.default_rng(seed).permutation(B)
    ring.hist, ring.err, ring.len = ring.hist[:, perm].copy(), ring.err[:, perm].copy(), ring.len[perm].copy()
    return dict(ring=ring, flag=flag[perm].copy(), target=c["target"][perm].copy())


def permuted(c, perm):
    r = Ring(c["ring"].h, c["ring"].B)
    r.hist, r.err, r.len = c["ring"].hist[:, perm].copy(), c["ring"].err[:, perm].copy(), c["ring"].len[perm].copy()
    return dict(ring=r, flag=c["flag"][perm].copy(), target=c["target"][perm].copy())


@functools.lru_cache(maxsize=None)
def sequence_case(learner: str, lam: float = 0.5, h: int = 3, B: int = 67, steps: int = 6, seed: int = 9):
    """Six consecutive lock-steps on SMALL from a fixed ring: the learner half and ``link`` with made-up trajectory rows (random
    boards, random actions, an episode end with probability 1 / 4), fresh random targets at every step.
    -> dict(ring0, flag0, rows=[(boards_row, meta_row, target)], w0, after=[dict(weights, coh_e, coh_a, td_error, ring, prev, flag)])."""
    rng = np.random.default_rng(seed)
    c = ring_case(N.SMALL, 12, h, B, seed=seed)
    ring, flag = c["ring"].copy(), c["flag"].copy()
    w = N.random_weights(N.SMALL, seed=8)
    w0 = w.copy()
    ce, ca = T.zero_coherence(w)
    rows, after = [], []
    for t in range(steps):
        n = 5 + t  # any start of the global count
        boards_row = N.boards_for(B, seed=seed + 20 + t)
        meta_row = (rng.integers(0, 4, B) | (0xF << 2) | ((rng.random(B) < 0.25).astype(np.int64) << 6)).astype(np.uint8)
        target = (rng.standard_normal(B) * 500).astype(F32)
        rows.append((boards_row, meta_row, target, (n - 1) % h, n % h))
        err = step(ring, flag, target, (n - 1) % h, lam, w, N.SMALL, 12, 1.0 if learner == "tc" else 0.1, (), learner, ce, ca)
        prev, flag = link(ring, boards_row, meta_row, n % h, flag)
        after.append(dict(weights=w.copy(), coh_e=ce.copy(), coh_a=ca.copy(), td_error=err, ring=ring.copy(), prev=prev, flag=flag.copy()))
    return dict(ring0=c["ring"], flag0=c["flag"], rows=rows, w0=w0, after=after, lam=lam, h=h, alpha=1.0 if learner == "tc" else 0.1)
