"""Numpy restatement of the n-tuple afterstate value network (include/g2048.h, "n-tuple network").  TEST INFRASTRUCTURE ONLY.

Written from the definitions with the oracle's ``move`` and the view definition of ``symmetry_ref``:

  idx(x, t) = sum_j min(x[c_tj], 15) << 4 j
  S(board)  = sum over g < 8, t < m of weights[t][idx(view_g(board), t)]   (int64),   V = f32(S) * 2^-F
  q[a]      = f32(r_a) + V(after_a) where the move is legal, +0 where not;  v = max over the legal a, 0 if none
  TD(0)     : e = target - V(prev_after), delta = int32(rint(clip(e * c, +-2^30))), c = f32(alpha 2^F / (8 m));
              acc += delta, cnt += 1 at every (g, t) entry of prev_after; weights = sat(weights + rdiv(acc, cnt)) where cnt > 0
"""
from __future__ import annotations

import functools

import numpy as np

import symmetry_ref as S
from oracle import g2048_oracle as npo

F32 = np.float32
DEFAULT_TUPLES = ((0, 1, 2, 3, 4, 5), (4, 5, 6, 7, 8, 9), (0, 1, 2, 4, 5, 6), (4, 5, 6, 8, 9, 10))
CLAMP = F32(2.0 ** 30)


def cells_array(tuples) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(tuples, np.uint8).reshape(len(tuples), -1))


def zero_weights(tuples) -> np.ndarray:
    c = cells_array(tuples)
    return np.zeros((c.shape[0], 16 ** c.shape[1]), np.int32)


def index(boards: np.ndarray, cells) -> np.ndarray:
    """boards u8 [N,16], cells [L] -> int64 [N]."""
    x = np.minimum(np.asarray(boards, np.uint8)[:, np.asarray(cells, np.int64)], 15).astype(np.int64)
    return (x << (4 * np.arange(x.shape[1], dtype=np.int64))).sum(axis=1)


def entries(boards: np.ndarray, tuples) -> np.ndarray:
    """-> int64 [N, 8, m]: idx(view_g(board), t)."""
    boards = np.asarray(boards, np.uint8).reshape(-1, 16)
    c = cells_array(tuples)
    out = np.empty((len(boards), 8, len(c)), np.int64)
    for g in range(8):
        v = S.view(boards, g)
        for t in range(len(c)):
            out[:, g, t] = index(v, c[t])
    return out


def table_sum(boards, weights, tuples) -> np.ndarray:
    e = entries(boards, tuples)
    s = np.zeros(len(e), np.int64)
    for t in range(e.shape[2]):
        s += weights[t][e[:, :, t]].astype(np.int64).sum(axis=1)
    return s


def values(boards, weights, tuples, frac_bits: int) -> np.ndarray:
    return (table_sum(boards, weights, tuples).astype(F32) * F32(2.0 ** -frac_bits)).astype(F32)


def scores(boards, weights, tuples, frac_bits: int):
    """-> (q f32 [B,4], v f32 [B], legal bool [B,4])."""
    boards = np.asarray(boards, np.uint8).reshape(-1, 16)
    B = len(boards)
    q, legal = np.zeros((B, 4), F32), np.zeros((B, 4), bool)
    for a in range(4):
        after, r = npo.move(boards, np.full(B, a, np.int32))
        legal[:, a] = (after != boards).any(axis=1)
        qa = (r.astype(F32) + values(after, weights, tuples, frac_bits)).astype(F32)
        q[:, a] = np.where(legal[:, a], qa, F32(0))
    v = np.where(legal, q, -np.inf).max(axis=1)
    return q, np.where(legal.any(axis=1), v, 0).astype(F32), legal


def step_constant(alpha: float, frac_bits: int, m: int) -> np.float32:
    return F32(float(alpha) * float(2 ** frac_bits) / (8.0 * m))  # the double product, rounded once


def td_deltas(prev_after, flag, target, weights, tuples, frac_bits: int, alpha: float):
    """-> (delta int32 [B], e f32 [B]); both 0 where flag == 0."""
    flag = np.asarray(flag, np.uint8)
    tgt = np.where(flag == 1, np.asarray(target, F32), F32(0)).astype(F32)
    e = (tgt - values(prev_after, weights, tuples, frac_bits)).astype(F32)
    d = (e * step_constant(alpha, frac_bits, len(tuples))).astype(F32)
    delta = np.rint(np.clip(d, -CLAMP, CLAMP)).astype(np.int32)
    live = flag != 0
    return np.where(live, delta, 0).astype(np.int32), np.where(live, e, F32(0)).astype(F32)


def accumulate(prev_after, flag, delta, tuples, acc, cnt):
    live = np.nonzero(np.asarray(flag) != 0)[0]
    e = entries(np.asarray(prev_after)[live], tuples)
    for t in range(e.shape[2]):
        np.add.at(acc[t], e[:, :, t].reshape(-1), np.repeat(delta[live].astype(np.int64), 8))
        np.add.at(cnt[t], e[:, :, t].reshape(-1), 1)


def rdiv(a: np.ndarray, c: np.ndarray) -> np.ndarray:
    a, c = a.astype(np.int64), c.astype(np.int64)
    return np.sign(a) * ((2 * np.abs(a) + c) // (2 * c))


def apply(weights, acc, cnt):
    hit = np.flatnonzero(cnt)  # (only the entries that were hit are rewritten: the tables are large)
    w, a, c = weights.reshape(-1), acc.reshape(-1), cnt.reshape(-1)
    assert (c[hit] > 0).all()
    w[hit] = np.clip(w[hit].astype(np.int64) + rdiv(a[hit], c[hit]), -2 ** 31, 2 ** 31 - 1).astype(np.int32)
    a[hit] = 0
    c[hit] = 0


def td_step(prev_after, flag, target, weights, tuples, frac_bits: int, alpha: float, acc=None, cnt=None):
    """accumulate + apply, in place on weights -> td_error f32 [B]."""
    acc = np.zeros(weights.shape, np.int64) if acc is None else acc
    cnt = np.zeros(weights.shape, np.int32) if cnt is None else cnt
    delta, e = td_deltas(prev_after, flag, target, weights, tuples, frac_bits, alpha)
    accumulate(prev_after, flag, delta, tuples, acc, cnt)
    apply(weights, acc, cnt)
    return e


def link(boards_row, meta_row):
    """-> (prev_after u8 [B,16], flag u8 [B]) from the trajectory row the engine wrote."""
    meta = np.asarray(meta_row, np.uint8)
    after, _ = npo.move(np.asarray(boards_row, np.uint8).reshape(-1, 16), (meta & 3).astype(np.int32))
    return after, np.where((meta >> 6) & 1, 2, 1).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- test boards
def special_boards() -> np.ndarray:
    """Tiles 16 and 17 (the clamp), boards equal to one of their own views (repeated hits), full boards without a legal move, the
    empty board."""
    b = [np.zeros(16, np.uint8), np.full(16, 3, np.uint8)]
    b.append(np.array([[16, 17, 1, 2], [3, 16, 0, 0], [15, 14, 17, 1], [0, 0, 2, 16]], np.uint8).reshape(-1))
    b.append(np.array([[17, 16, 15, 14], [1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]], np.uint8).reshape(-1))
    b.append(np.array([[5, 1, 2, 0], [1, 4, 3, 0], [2, 3, 0, 1], [0, 0, 1, 2]], np.uint8).reshape(-1))  # transpose-symmetric
    b.append(np.array([[1, 2, 3, 4], [5, 6, 7, 0], [0, 7, 6, 5], [4, 3, 2, 1]], np.uint8).reshape(-1))  # 180-degree-symmetric
    b.append(np.array([[1, 2, 1, 2], [2, 1, 2, 1], [1, 2, 1, 2], [2, 1, 2, 1]], np.uint8).reshape(-1))  # full, no move, symmetric
    b.append(np.array([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12], [13, 14, 15, 16]], np.uint8).reshape(-1))  # full, no move
    b.append(np.array([[2, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12], [13, 14, 15, 1]], np.uint8).reshape(-1))  # full, one merge
    return np.stack(b)


def boards_for(n: int, seed: int = 0) -> np.ndarray:
    """n boards: the special ones first (as many as fit), then random ones of mixed fill."""
    sp = special_boards()
    rnd = S.random_boards(max(n, 1), seed=seed + 77)
    return np.ascontiguousarray(np.concatenate([sp, rnd])[:n], np.uint8)


def random_weights(tuples, seed: int = 0, bits: int = 20) -> np.ndarray:
    c = cells_array(tuples)
    rng = np.random.default_rng(seed)
    return rng.integers(-(1 << bits), (1 << bits) + 1, size=(c.shape[0], 16 ** c.shape[1]), dtype=np.int64).astype(np.int32)


# ---------------------------------------------------------------------------------------------- a CPU training loop
def _spawn(boards: np.ndarray, rng) -> np.ndarray:
    """A 2 (p = .9) or 4 on a uniformly chosen empty cell, numpy's RNG (not the engine's key stream)."""
    out = boards.copy()
    empty = out == 0
    pick = (rng.random(len(out))[:, None] * empty.sum(axis=1, keepdims=True)).astype(np.int64)
    pos = (np.cumsum(empty, axis=1) > pick).argmax(axis=1)
    has = empty.any(axis=1)
    out[np.nonzero(has)[0], pos[has]] = np.where(rng.random(int(has.sum())) < 0.9, 1, 2)
    return out


def _fresh(n: int, rng) -> np.ndarray:
    return _spawn(_spawn(np.zeros((n, 16), np.uint8), rng), rng)


def _greedy(boards, weights, tuples, frac_bits):
    q, v, legal = scores(boards, weights, tuples, frac_bits)
    return np.where(legal, q, -np.inf).argmax(axis=1), v, legal


def simulate_training(weights, tuples, num_envs: int, lock_steps: int, alpha: float = 0.1, frac_bits: int = 12, seed: int = 0):
    """The trainer's lock-step (scores -> accumulate -> apply -> step with auto-reset -> link) with numpy's RNG for the spawns.
    In place on weights -> episodes finished."""
    rng = np.random.default_rng(seed)
    boards = _fresh(num_envs, rng)
    prev, flag = np.zeros((num_envs, 16), np.uint8), np.zeros(num_envs, np.uint8)
    acc, cnt = np.zeros(weights.shape, np.int64), np.zeros(weights.shape, np.int32)
    episodes = 0
    for _ in range(lock_steps):
        a, v, _ = _greedy(boards, weights, tuples, frac_bits)
        td_step(prev, flag, v, weights, tuples, frac_bits, alpha, acc, cnt)
        after, _ = npo.move(boards, a.astype(np.int32))
        nxt = _spawn(after, rng)
        done = ~npo.legal_mask(nxt).any(axis=1)
        prev, flag = after, np.where(done, 2, 1).astype(np.uint8)
        nxt[done] = _fresh(int(done.sum()), rng)
        episodes += int(done.sum())
        boards = nxt
    return episodes


def simulate_evaluation(weights, tuples, episodes: int, frac_bits: int = 12, seed: int = 42, max_steps: int = 100000) -> float:
    """Mean max tile of ``episodes`` greedy games, numpy's RNG for the spawns."""
    rng = np.random.default_rng(seed)
    boards = _fresh(episodes, rng)
    live = np.ones(episodes, bool)
    for _ in range(max_steps):
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            break
        a, _, legal = _greedy(boards[idx], weights, tuples, frac_bits)
        ok = legal.any(axis=1)
        live[idx[~ok]] = False
        idx, a = idx[ok], a[ok]
        after, _ = npo.move(boards[idx], a.astype(np.int32))
        boards[idx] = _spawn(after, rng)
    return float((1 << boards.max(axis=1).astype(np.int64)).mean())


def masked_argmax(q, legal):
    """The engine's greedy choice (use_mask=1, sample=0): q - 1e8 where illegal, the first maximum."""
    return (q - np.where(legal, F32(0), F32(1e8))).astype(F32).argmax(axis=1).astype(np.int32)


def engine_training(weights, tuples, num_envs: int, lock_steps: int, alpha: float = 0.1, frac_bits: int = 12, seed: int = 0,
                    mode: int = npo.MODE_PARTITIONABLE):
    """NTupleTrainer.train on the C oracle's env and the engine's key chain (init split, then act / step sub-keys per lock-step, a
    finished env re-initialised from split(fold_in(step_sub, 0xFFFFFFFF), B)[env]).  In place on weights -> the record of
    ``train(record=True)`` as numpy arrays plus "episodes"."""
    from oracle import c_oracle as orc

    B = num_envs
    _, subs = orc.chain(npo.key(seed), 1 + 2 * lock_steps, mode)
    b, m, _ = orc.init(orc.split(subs[0], B, mode), mode)
    prev, flag = np.zeros((B, 16), np.uint8), np.zeros(B, np.uint8)
    rec = dict(boards=[], meta=[], scores=[], targets=[])
    episodes = 0
    for t in range(lock_steps):
        q, v, legal = scores(b, weights, tuples, frac_bits)
        td_step(prev, flag, v, weights, tuples, frac_bits, alpha)
        a = masked_argmax(q, legal)
        nb, nm, nd, _ = orc.step(b, m, np.zeros(B, np.uint8), a, orc.split(subs[2 + 2 * t], B, mode), mode)
        meta = (a.astype(np.uint8) | (m.astype(np.uint8) << 2) | (nd.astype(np.uint8) << 6)).astype(np.uint8)
        for k, x in zip(("boards", "meta", "scores", "targets"), (b, meta, q, v)):
            rec[k].append(np.array(x))
        prev, flag = link(b, meta)
        if nd.any():
            fb, fm, _ = orc.init(orc.split(npo.fold_in(subs[2 + 2 * t], 0xFFFFFFFF), B, mode), mode)
            nb, nm = np.where(nd[:, None] != 0, fb, nb), np.where(nd != 0, fm, nm)
            episodes += int(nd.sum())
        b, m = nb, nm
    out = {k: np.stack(x) for k, x in rec.items()}
    out["episodes"] = episodes
    return out


def replay_training(weights, tuples, boards, meta, alpha: float = 0.1, frac_bits: int = 12):
    """The learner's half of a recorded run: boards u8 [T,B,16] before each step and the engine's meta rows u8 [T,B] -> scores,
    targets per step (scores -> targets -> accumulate -> apply -> link).  In place on weights."""
    B = boards.shape[1]
    prev, flag = np.zeros((B, 16), np.uint8), np.zeros(B, np.uint8)
    qs, vs = [], []
    for t in range(len(boards)):
        q, v, _ = scores(boards[t], weights, tuples, frac_bits)
        td_step(prev, flag, v, weights, tuples, frac_bits, alpha)
        prev, flag = link(boards[t], meta[t])
        qs.append(q)
        vs.append(v)
    return np.stack(qs), np.stack(vs)


def crowding_weights(tuples, per_tile: int = 1 << 14) -> np.ndarray:
    """Initial weights that value every occupied cell of a pattern: a greedy player on them avoids merges, fills the board and ends
    its episodes within a few dozen moves (the replay test wants episode ends inside a short run)."""
    c = cells_array(tuples)
    idx = np.arange(16 ** c.shape[1], dtype=np.int64)
    occupied = sum(((idx >> (4 * j)) & 15) != 0 for j in range(c.shape[1]))
    return np.ascontiguousarray(np.broadcast_to((occupied * per_tile).astype(np.int32), (c.shape[0], len(idx))))


# ---------------------------------------------------------------------------------------------- shared cases
SMALL = ((0, 1), (5, 6), (3, 15))                        # m = 3, L = 2
WIDE = ((0, 1, 2, 3, 4, 5), (4, 5, 6, 8, 9, 10))         # m = 2, L = 6 (128 MB of weights)


@functools.lru_cache(maxsize=None)
def small_weights() -> np.ndarray:
    w = random_weights(SMALL, seed=1)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def wide_weights() -> np.ndarray:
    w = random_weights(WIDE, seed=2)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def collision_case(B: int = 1000, same: int = 300, seed: int = 5):
    """One TD step under heavy collision on SMALL: ``same`` identical boards, flags 0 / 1 / 2 mixed -> dict with the inputs and the
    restatement's weights_after / td_error."""
    rng = np.random.default_rng(seed)
    prev = S.random_boards(B, seed=seed)
    prev[:same] = prev[0]
    prev[same:same + len(special_boards())] = special_boards()
    prev = prev[rng.permutation(B)]
    flag = rng.integers(0, 3, B).astype(np.uint8)
    target = (rng.standard_normal(B) * 500).astype(F32)
    w = small_weights().copy()
    e = td_step(prev, flag, target, w, SMALL, 12, 0.1)
    out = dict(prev=prev, flag=flag, target=target, weights_after=w, td_error=e)
    for v in out.values():
        v.setflags(write=False)
    return out
