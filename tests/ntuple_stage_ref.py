"""Numpy restatement of the multi-stage n-tuple network (include/g2048.h, "multi-stage n-tuple network").  TEST INFRASTRUCTURE ONLY.

Written from the definition on top of ``ntuple_ref``, ``ntuple_tc_ref`` and the lookahead restatements ``ntuple_search_ref`` composes:

  stage(x)     = #{ i : max over the 16 cells of x[c] >= k_i }          (the unclamped log2 tile)
  off(x, g, t) = ((stage(x) * m + t) << 4 L) + idx(view_g(x), t)

Nothing of the single-stage arithmetic is restated: the boards are grouped by their stage and every group goes through the
single-stage function on its stage's [m, 16^L] slice of the [S, m, 16^L] arrays (views, so the learners work in place).  ``tiles``
is always what the kernels are given: the ACTIVE thresholds (the first ``active_stages - 1``); promotion lives in ``Net`` and in
the training loops only.
"""
from __future__ import annotations

import functools

import numpy as np

import lookahead2_ref as R2
import lookahead_ref as R
import ntuple_ref as N
import ntuple_search_ref as NS
import ntuple_tc_ref as T
import symmetry_ref as S
from oracle import g2048_oracle as npo

F32 = np.float32
GAMMAS = NS.GAMMAS


def stage(boards, tiles) -> np.ndarray:
    """boards u8 [n,16] -> int64 [n]: the number of thresholds at or below the board's largest (unclamped) log2 tile."""
    mx = np.asarray(boards, np.uint8).reshape(-1, 16).max(axis=1).astype(np.int64)
    return sum((mx >= int(k)).astype(np.int64) for k in tiles) + np.zeros(len(mx), np.int64)


def _groups(boards, tiles):
    st = stage(boards, tiles)
    return [(int(s), np.nonzero(st == s)[0]) for s in np.unique(st)]


def values(boards, weights, tuples, frac_bits: int, tiles, seen=None) -> np.ndarray:
    """weights i32 [S, m, 16^L] -> V f32 [n].  ``seen``: a set that collects the stages looked up."""
    boards = np.asarray(boards, np.uint8).reshape(-1, 16)
    out = np.zeros(len(boards), F32)
    for s, sel in _groups(boards, tiles):
        out[sel] = N.values(boards[sel], weights[s], tuples, frac_bits)
        if seen is not None:
            seen.add(s)
    return out


def scores(boards, weights, tuples, frac_bits: int, tiles, seen=None):
    """``ntuple_ref.scores`` with every afterstate valued by its OWN stage -> (q f32 [B,4], v f32 [B], legal bool [B,4])."""
    boards = np.asarray(boards, np.uint8).reshape(-1, 16)
    B = len(boards)
    q, legal = np.zeros((B, 4), F32), np.zeros((B, 4), bool)
    for a in range(4):
        after, r = npo.move(boards, np.full(B, a, np.int32))
        legal[:, a] = (after != boards).any(axis=1)
        ok = np.nonzero(legal[:, a])[0]  # only the afterstates of legal moves are looked up
        qa = np.zeros(B, F32)
        qa[ok] = (r[ok].astype(F32) + values(after[ok], weights, tuples, frac_bits, tiles, seen)).astype(F32)
        q[:, a] = qa
    v = np.where(legal, q, -np.inf).max(axis=1)
    return q, np.where(legal.any(axis=1), v, 0).astype(F32), legal


def expectimax(boards, weights, tuples, frac_bits: int, tiles, plies: int, gammas=GAMMAS, seen=None):
    """-> ({gamma: (q f32 [B,4], v f32 [B])}, legal): ``ntuple_search_ref.one_ply`` / ``two_plies`` with the staged ``scores`` as
    the leaf."""
    boards = np.ascontiguousarray(boards, np.uint8).reshape(-1, 16)
    out = {}
    if plies == 1:
        after, reward, nchild = R.expand(boards)
        children, terminal, offset = R.children(after, nchild)
        v0 = scores(children, weights, tuples, frac_bits, tiles, seen)[1]
        legal = nchild > 0
        for g in gammas:
            q = R.q_values(reward, nchild, offset, v0, terminal, g, F32).astype(F32)
            out[g] = (q, NS._best(q, legal))
        return out, legal
    memo = {}

    def value_fn(children):
        key = (children.shape, hash(children.tobytes()))
        if key not in memo:
            memo[key] = scores(children, weights, tuples, frac_bits, tiles, seen)[1]
        return memo[key]

    legal = None
    for g in gammas:
        p = R2.pipeline(boards, value_fn, g, F32, dedup_pairs=False)
        legal = p["nchild1"] > 0
        q = p["q2"].astype(F32)
        out[g] = (q, NS._best(q, legal))
    return out, legal


# ---------------------------------------------------------------------------------------------- learners
def td_deltas(prev_after, flag, target, weights, tuples, frac_bits: int, alpha: float, tiles):
    """``ntuple_ref.td_deltas`` with V(prev_after) from prev_after's stage -> (delta int32 [B], e f32 [B]); 0 where flag == 0."""
    flag = np.asarray(flag, np.uint8)
    tgt = np.where(flag == 1, np.asarray(target, F32), F32(0)).astype(F32)
    e = (tgt - values(prev_after, weights, tuples, frac_bits, tiles)).astype(F32)
    d = (e * N.step_constant(alpha, frac_bits, len(tuples))).astype(F32)
    delta = np.rint(np.clip(d, -N.CLAMP, N.CLAMP)).astype(np.int32)
    live = flag != 0
    return np.where(live, delta, 0).astype(np.int32), np.where(live, e, F32(0)).astype(F32)


def td_step(prev_after, flag, target, weights, tuples, frac_bits: int, alpha: float, tiles, acc=None, cnt=None):
    """accumulate + apply, in place on weights [S, m, 16^L] -> td_error f32 [B]."""
    acc = np.zeros(weights.shape, np.int64) if acc is None else acc
    cnt = np.zeros(weights.shape, np.int32) if cnt is None else cnt
    prev_after, flag = np.asarray(prev_after, np.uint8), np.asarray(flag, np.uint8)
    delta, e = td_deltas(prev_after, flag, target, weights, tuples, frac_bits, alpha, tiles)
    for s, sel in _groups(prev_after, tiles):
        N.accumulate(prev_after[sel], flag[sel], delta[sel], tuples, acc[s], cnt[s])
        N.apply(weights[s], acc[s], cnt[s])
    return e


def tc_step(prev_after, flag, target, weights, coh_e, coh_a, tuples, frac_bits: int, alpha: float, tiles, acc=None, abs_acc=None,
            cnt=None, stats=None):
    """accumulate + apply of TC, in place on weights, coh_e, coh_a (all [S, m, 16^L]) -> td_error f32 [B]."""
    acc = np.zeros(weights.shape, np.int64) if acc is None else acc
    abs_acc = np.zeros(weights.shape, np.int64) if abs_acc is None else abs_acc
    cnt = np.zeros(weights.shape, np.int32) if cnt is None else cnt
    prev_after, flag = np.asarray(prev_after, np.uint8), np.asarray(flag, np.uint8)
    delta, e = td_deltas(prev_after, flag, target, weights, tuples, frac_bits, alpha, tiles)
    if stats is not None:
        stats["clamped"] = stats.get("clamped", 0) + int((np.abs(delta.astype(np.int64)) == 2 ** 30).sum())
    for s, sel in _groups(prev_after, tiles):
        if not (flag[sel] != 0).any():
            continue
        hit = T.tc_accumulate(prev_after[sel], flag[sel], delta[sel], tuples, acc[s], abs_acc[s], cnt[s])
        T.tc_apply(weights[s], acc[s], abs_acc[s], cnt[s], coh_e[s], coh_a[s], hit, stats)
    return e


class Net:
    """The promotion state of a restated network: ``w`` i32 [S, m, 16^L], ``active`` = the stages split off so far."""

    def __init__(self, weights, tuples, stage_tiles, frac_bits: int = 12, active: int = 1):
        self.w, self.tuples, self.stage_tiles, self.F, self.active = weights, tuples, tuple(stage_tiles), frac_bits, active
        self.S = len(self.stage_tiles) + 1
        assert weights.shape[0] == self.S and 1 <= active <= self.S

    @property
    def tiles(self):
        return self.stage_tiles[:self.active - 1]

    def promote(self) -> int:
        assert self.active < self.S
        self.w[self.active] = self.w[self.active - 1]
        self.active += 1
        return self.active


class Learner:
    """One learner's step on a ``Net`` with its tables, and the trainer's promotion rule."""

    def __init__(self, learner, net: Net, alpha, promote_every, coh_e=None, coh_a=None):
        assert learner in ("td0", "tc")
        self.learner, self.net, self.alpha, self.every = learner, net, alpha, int(promote_every)
        w = net.w
        self.acc, self.cnt = np.zeros(w.shape, np.int64), np.zeros(w.shape, np.int32)
        if learner == "tc":
            self.abs_acc = np.zeros(w.shape, np.int64)
            self.coh_e = np.zeros(w.shape, np.int32) if coh_e is None else coh_e
            self.coh_a = np.zeros(w.shape, np.int32) if coh_a is None else coh_a
        self.promotions = []

    def check_promotion(self, count: int, prev_after):
        """In front of lock-step ``count``: at a positive multiple of ``promote_every``, promote while the largest tile among the
        previous afterstates has reached the next threshold."""
        net = self.net
        if not self.every or count == 0 or count % self.every:
            return
        top = int(np.asarray(prev_after).max())
        while net.active < net.S and top >= net.stage_tiles[net.active - 1]:
            self.promotions.append((count, net.promote()))

    def step(self, prev, flag, target):
        net = self.net
        if self.learner == "td0":
            return td_step(prev, flag, target, net.w, net.tuples, net.F, self.alpha, net.tiles, self.acc, self.cnt)
        return tc_step(prev, flag, target, net.w, self.coh_e, self.coh_a, net.tuples, net.F, self.alpha, net.tiles, self.acc,
                       self.abs_acc, self.cnt)


def replay_training(net: Net, boards, meta, alpha: float, learner: str, promote_every: int, coh_e=None, coh_a=None):
    """The learner's half of a recorded run of ``NTupleTrainer.train(record=True)`` from lock-step 0: boards u8 [T,B,16] before each
    step and the engine's meta rows u8 [T,B] -> (scores [T,B,4], targets [T,B], promotions).  In place on net (weights, active)
    and on coh_e / coh_a."""
    B = boards.shape[1]
    lr = Learner(learner, net, alpha, promote_every, coh_e, coh_a)
    prev, flag = np.zeros((B, 16), np.uint8), np.zeros(B, np.uint8)
    qs, vs = [], []
    for t in range(len(boards)):
        lr.check_promotion(t, prev)
        q, v, _ = scores(boards[t], net.w, net.tuples, net.F, net.tiles)
        lr.step(prev, flag, v)
        prev, flag = N.link(boards[t], meta[t])
        qs.append(q)
        vs.append(v)
    return np.stack(qs), np.stack(vs), lr.promotions


def simulate_training(net: Net, num_envs: int, lock_steps: int, alpha: float = 0.1, seed: int = 0, learner: str = "td0",
                      promote_every: int = 64):
    """``ntuple_ref.simulate_training`` (numpy's RNG for the spawns) on a staged network with the trainer's promotion rule.  In
    place on net -> (episodes finished, promotions)."""
    rng = np.random.default_rng(seed)
    lr = Learner(learner, net, alpha, promote_every)
    boards = N._fresh(num_envs, rng)
    prev, flag = np.zeros((num_envs, 16), np.uint8), np.zeros(num_envs, np.uint8)
    episodes = 0
    for t in range(lock_steps):
        lr.check_promotion(t, prev)
        q, v, legal = scores(boards, net.w, net.tuples, net.F, net.tiles)
        a = np.where(legal, q, -np.inf).argmax(axis=1)
        lr.step(prev, flag, v)
        after, _ = npo.move(boards, a.astype(np.int32))
        nxt = N._spawn(after, rng)
        done = ~npo.legal_mask(nxt).any(axis=1)
        prev, flag = after, np.where(done, 2, 1).astype(np.uint8)
        nxt[done] = N._fresh(int(done.sum()), rng)
        episodes += int(done.sum())
        boards = nxt
    return episodes, lr.promotions


# ---------------------------------------------------------------------------------------------- shared fixtures
# name -> (tuples, stage_tiles, frac_bits): SMALL with two and five stages, EIGHT with all eight (the widest register arrays with
# the most stages; its last threshold, 17, is only reached by the unclamped tile); frac_bits 0 and 20 among them
NETWORKS = {
    "small2": (N.SMALL, (3,), 0),
    "small5": (N.SMALL, (2, 5, 9, 12), 12),
    "eight8": (NS.EIGHT, (2, 4, 6, 9, 12, 15, 17), 20),
}


@functools.lru_cache(maxsize=None)
def staged_weights(name: str) -> np.ndarray:
    """i32 [S, m, 16^L], random and seeded PER STAGE: a lookup in the wrong stage gives wrong bits.  Read-only."""
    tuples, tiles, _ = NETWORKS[name]
    w = np.stack([N.random_weights(tuples, seed=100 + 7 * s) for s in range(len(tiles) + 1)])
    assert all((w[s] != w[s + 1]).any() for s in range(len(tiles)))
    w.setflags(write=False)
    return w


def threshold_boards(tiles) -> np.ndarray:
    """For every threshold k: a board whose largest tile is k, one whose largest tile is k - 1, and one with two adjacent k - 1
    tiles whose merge (left or right) creates k."""
    out = []
    for k in tiles:
        for cells in ({5: k}, {5: k - 1}, {5: k - 1, 6: k - 1}):
            b = np.zeros(16, np.uint8)
            b[0], b[15] = 1, min(1, k - 1)
            for c, v in cells.items():
                b[c] = v
            out.append(b)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def boards_for(name: str, n: int) -> np.ndarray:
    """n boards: the threshold boards first (as many as fit), then ``ntuple_ref.boards_for`` (which holds a 17 tile).  Read-only."""
    b = np.ascontiguousarray(np.concatenate([threshold_boards(NETWORKS[name][1]), N.boards_for(n, seed=11)])[:n], np.uint8)
    b.setflags(write=False)
    return b


def check_inputs(name: str, boards):
    """What the fixtures promise, on the CPU: every stage is looked up by values and by scores, and some (board, action) has an
    afterstate whose stage is not the board's."""
    tuples, tiles, F = NETWORKS[name]
    S_ = len(tiles) + 1
    assert set(stage(boards, tiles).tolist()) == set(range(S_))
    seen = set()
    _, _, legal = scores(boards, staged_weights(name), tuples, F, tiles, seen)
    assert seen == set(range(S_))
    differs = False
    for a in range(4):
        after, _ = npo.move(boards, np.full(len(boards), a, np.int32))
        differs |= bool((legal[:, a] & (stage(after, tiles) != stage(boards, tiles))).any())
    assert differs
    assert boards.max() == 17


@functools.lru_cache(maxsize=None)
def values_case(name: str, n: int = 1000):
    """-> dict(boards, v, q, qv, legal) of the restatement on ``boards_for(name, n)``; a run on B boards uses the first B rows."""
    tuples, tiles, F = NETWORKS[name]
    boards = boards_for(name, n)
    check_inputs(name, boards[:257])
    v = values(boards, staged_weights(name), tuples, F, tiles)
    q, qv, legal = scores(boards, staged_weights(name), tuples, F, tiles)
    out = dict(boards=boards, v=v, q=q, qv=qv, legal=legal)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def search_case(name: str, plies: int, n: int = 37):
    """-> dict(boards, q={gamma: ...}, v={gamma: ...}) of 1- or 2-ply expectimax on the first n fixture boards.  For two plies the
    restatement also shows that some leaf's stage differs from its root's."""
    tuples, tiles, F = NETWORKS[name]
    boards = boards_for(name, n)
    seen = set()
    res, legal = expectimax(boards, staged_weights(name), tuples, F, tiles, plies, seen=seen)
    assert len(seen) >= 2
    if plies == 2:
        root = boards[2:3]  # two adjacent k_1 - 1 tiles: the root is in stage 0, the leaves after the merge are not
        leaf = set()
        expectimax(root, staged_weights(name), tuples, F, tiles, 2, gammas=(1.0,), seen=leaf)
        assert leaf - set(stage(root, tiles).tolist())
    out = dict(boards=boards, legal=legal, q={g: r[0] for g, r in res.items()}, v={g: r[1] for g, r in res.items()})
    for a in [*out["q"].values(), *out["v"].values()]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def collision_case(B: int = 1000, same: int = 300, seed: int = 5):
    """One TD and one TC step under heavy collision on "small5": ``same`` identical boards, flags 0 / 1 / 2 mixed, the envs spread
    over at least three stages, no env in the top stage (its tables must stay as they are) -> dict with the inputs and the
    restatement's tables / td_error after each learner's step."""
    tuples, tiles, F = NETWORKS["small5"]
    rng = np.random.default_rng(seed)
    prev = S.random_boards(B, seed=seed)  # tiles 0 .. 11: below the last threshold
    prev[:same] = prev[0]
    tb = threshold_boards(tiles[:-1])
    prev[same:same + len(tb)] = tb
    prev = prev[rng.permutation(B)]
    flag = rng.integers(0, 3, B).astype(np.uint8)
    target = (rng.standard_normal(B) * 500).astype(F32)
    st = stage(prev[flag != 0], tiles)
    assert len(set(st.tolist())) >= 3 and len(tiles) not in set(st.tolist()) and set(flag.tolist()) == {0, 1, 2}
    w0 = staged_weights("small5")
    td_w = w0.copy()
    td_e = td_step(prev, flag, target, td_w, tuples, F, 0.1, tiles)
    tc_w, tc_ce, tc_ca = w0.copy(), np.zeros(w0.shape, np.int32), np.zeros(w0.shape, np.int32)
    tc_e = tc_step(prev, flag, target, tc_w, tc_ce, tc_ca, tuples, F, 0.1, tiles)
    hit = sorted(set(st.tolist()))
    assert all((td_w[s] != w0[s]).any() for s in hit) and np.array_equal(td_w[-1], w0[-1])
    out = dict(prev=prev, flag=flag, target=target, td_w=td_w, td_e=td_e, tc_w=tc_w, tc_ce=tc_ce, tc_ca=tc_ca, tc_e=tc_e)
    for v in out.values():
        v.setflags(write=False)
    out["stages_hit"] = hit
    return out


@functools.lru_cache(maxsize=None)
def sequence_case(alpha: float, scale: float, extreme: bool, steps: int = 6):
    """``ntuple_tc_ref.sequence_case`` on "small2" (F = 12 here), the 200 boards in both of its stages: ``steps`` consecutive TC
    steps on the same boards and flags with fresh targets of ``scale``.  ``extreme``: weights near +-2^31, so that with alpha = 1000
    and targets of 1e9 the weights saturate, delta sits on the clamp and A is halved, in both stages."""
    tuples, tiles, F = N.SMALL, (3,), 12
    rng = np.random.default_rng(3)
    prev = np.concatenate([threshold_boards(tiles), N.boards_for(197, seed=4)])
    flag = rng.integers(0, 3, len(prev)).astype(np.uint8)
    flag[:3] = 1
    assert set(stage(prev[flag != 0], tiles).tolist()) == {0, 1}
    targets = (rng.standard_normal((steps, len(prev))) * scale).astype(F32)
    w0 = np.stack([N.random_weights(tuples, seed=8), N.random_weights(tuples, seed=9)])
    if extreme:
        w0[:, :, ::3] = 2 ** 31 - 1 - rng.integers(0, 50, w0[:, :, ::3].shape)
        w0[:, :, 1::3] = -2 ** 31 + rng.integers(0, 50, w0[:, :, 1::3].shape)
    w = w0.copy()
    ce, ca = np.zeros(w.shape, np.int32), np.zeros(w.shape, np.int32)
    stats, after = {}, []
    for t in range(steps):
        e = tc_step(prev, flag, targets[t], w, ce, ca, tuples, F, alpha, tiles, stats=stats)
        after.append(dict(weights=w.copy(), coh_e=ce.copy(), coh_a=ca.copy(), td_error=e))
    out = dict(prev=prev, flag=flag, targets=targets, w0=w0, after=after, stats=stats, alpha=alpha, tuples=tuples, tiles=tiles, F=F)
    for v in (prev, flag, targets, w0):
        v.setflags(write=False)
    return out
