"""Numpy restatement of the Monte-Carlo playout player (include/g2048.h, "Monte-Carlo playouts").  TEST INFRASTRUCTURE ONLY.

Written with the oracle's own ``split``, ``act_randomly``, ``act_drul``, ``env_step`` and ``legal_mask`` and ``np.float32`` arithmetic
in the order the header gives: lane j = (4 b + a) R + r, key index g = lane0 + j of n_total, step 0 plays the root action, later
steps the playout policy, ``ret = ret + disc * r`` then ``disc = disc * f32(gamma)`` with every operation rounded on its own, the
pair's R lanes summed in ascending r from +0 and divided once by f32(R).
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import g2048_oracle as npo

F32 = np.float32
POLICY_DRUL, POLICY_RANDOM = 0, 1
MAX_LAUNCH = 128
BITS = np.array([1, 2, 4, 8], np.uint8)


def mask_bits(m: np.ndarray) -> np.ndarray:
    return (m.astype(np.uint8) * BITS).sum(axis=1).astype(np.uint8)


def bits_mask(b: np.ndarray) -> np.ndarray:
    return (b[:, None] & BITS) != 0


def chain_keys(key: np.ndarray, n: int, mode: int):
    """n times ``key, sub = jax.random.split(key)`` -> (key, subs u32 [n, 2])  (g2048_chain_keys)."""
    subs = np.empty((n, 2), np.uint32)
    for i in range(n):
        ks = npo.split(key, 2, mode)
        key, subs[i] = ks[0], ks[1]
    return key, subs


def seed_state(roots: np.ndarray, R: int) -> dict:
    """Lane state at global step 0.  ``score``: exact int64 sum of the merge scores (a property the tests check, not ABI)."""
    B = len(roots)
    b = np.repeat(np.arange(B), 4 * R)
    a = np.tile(np.repeat(np.arange(4), R), B)
    boards = roots[b].copy()
    legal = npo.legal_mask(roots)[b]
    return dict(boards=boards, masks=mask_bits(legal), done=(~legal[np.arange(len(b)), a]).astype(np.uint8),
                ret=np.zeros(len(b), F32), disc=np.ones(len(b), F32), score=np.zeros(len(b), np.int64), a_root=a.astype(np.int32))


def playout(step_subs, t0: int, roots, R: int, lane0: int, n_total: int, policy: int, gamma: float, mode: int, state=None) -> dict:
    """g2048_mc_playout: ``len(step_subs)`` steps from global step t0; t0 == 0 seeds from roots, else continues ``state``."""
    subs = np.asarray(step_subs, np.uint32).reshape(-1, 4)
    st = seed_state(np.asarray(roots, np.uint8), R) if t0 == 0 else {k: v.copy() for k, v in state.items()}
    n = len(st["done"])
    assert lane0 + n <= n_total
    g32 = F32(gamma)
    for s in range(len(subs)):
        live = np.nonzero(st["done"] == 0)[0]
        if live.size == 0:
            break
        masks = bits_mask(st["masks"][live])
        if t0 + s == 0:
            a = st["a_root"][live]
        elif policy == POLICY_RANDOM:
            act_keys = npo.split(subs[s, 0:2], n_total, mode)[lane0 + live]
            a, _ = npo.act_randomly(act_keys, masks, mode)
        else:
            a = npo.act_drul(masks)
        step_keys = npo.split(subs[s, 2:4], n_total, mode)[lane0 + live]
        nb, r, nm, nd = npo.env_step(st["boards"][live], masks, np.zeros(live.size, bool), a, step_keys, mode)
        assert (r >= 0).all()  # a live lane never plays an illegal move
        st["boards"][live] = nb
        st["masks"][live] = mask_bits(nm)
        st["done"][live] = nd.astype(np.uint8)
        st["ret"][live] = (st["ret"][live] + (st["disc"][live] * r.astype(F32)).astype(F32)).astype(F32)
        st["disc"][live] = (st["disc"][live] * g32).astype(F32)
        st["score"][live] += r.astype(np.int64)
    return st


def reduce(ret, disc, done, values, R: int) -> np.ndarray:
    """g2048_mc_reduce -> q f32 [pairs]: the sequential f32 sum over each pair's R lanes, one division."""
    ret, disc, done = (np.asarray(x).reshape(-1, R) for x in (ret, disc, done))
    acc = np.zeros(ret.shape[0], F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(R):
            x = ret[:, r]
            if values is not None:
                v = np.asarray(values, F32).reshape(-1, R)[:, r]
                x = np.where(done[:, r] != 0, x, (x + (disc[:, r] * v).astype(F32)).astype(F32))
            acc = (acc + x).astype(F32)
        return (acc / F32(R)).astype(F32)


class Player:
    """MonteCarloActionFunction: the key chain of its own (seeded by ``seed``, two sub-keys per playout step, drawn per launch of
    at most 128 steps) and ``policy_fn``."""

    def __init__(self, seed: int, mode: int, playouts: int, depth=None, policy: int = POLICY_RANDOM, gamma: float = 1.0,
                 max_steps: int = 4096):
        self.key = np.array([(seed >> 32) & 0xFFFFFFFF, seed & 0xFFFFFFFF], np.uint32)
        self.mode, self.R, self.depth, self.policy, self.gamma, self.max_steps = mode, playouts, depth, policy, gamma, max_steps
        self.last_steps = 0

    def playout(self, boards: np.ndarray) -> dict:
        n_total = 4 * len(boards) * self.R
        limit = self.max_steps if self.depth is None else self.depth
        t, st = 0, None
        while t < limit:
            n_steps = min(MAX_LAUNCH, limit - t)
            self.key, subs = chain_keys(self.key, 2 * n_steps, self.mode)
            st = playout(subs.reshape(n_steps, 4), t, boards, self.R, 0, n_total, self.policy, self.gamma, self.mode, st)
            t += n_steps
            if self.depth is None and not (st["done"] == 0).any():
                break
        else:
            if self.depth is None:
                raise RuntimeError("max_steps exceeded")
        self.last_steps = t
        return st

    def policy_fn(self, boards: np.ndarray, critic=None):
        """-> (q f32 [B, 4], v f32 [B], lane state).  ``critic``: boards u8 [n, 16] -> f32 [n], the leaf values."""
        st = self.playout(boards)
        values = None if critic is None else np.asarray(critic(st["boards"]), F32)
        q = reduce(st["ret"], st["disc"], st["done"], values, self.R).reshape(-1, 4)
        legal = npo.legal_mask(boards)
        v = np.where(legal, q, -np.inf).max(axis=1)
        return q, np.where(legal.any(axis=1), v, 0).astype(F32), st


@functools.lru_cache(maxsize=None)
def root_pool():
    """Boards of lookahead_ref.kernel_test_boards() by kind: terminal, exactly one legal move, full but not terminal, opening
    (two tiles), the rest."""
    import lookahead_ref

    boards = np.unique(lookahead_ref.kernel_test_boards(n_random=6000), axis=0)
    boards = boards[boards.max(axis=1) <= 15]
    legal = npo.legal_mask(boards)
    n_legal, n_tiles = legal.sum(axis=1), (boards != 0).sum(axis=1)
    kinds = dict(terminal=(n_legal == 0) & (n_tiles == 16), one_move=n_legal == 1, full_live=(n_tiles == 16) & (n_legal > 0),
                 opening=(n_tiles == 2) & (boards.max(axis=1) <= 2))
    rest = ~np.logical_or.reduce(list(kinds.values())) & (n_legal > 0)
    out = {k: boards[v] for k, v in kinds.items()}
    out["rest"] = boards[rest]
    for k, v in out.items():
        assert len(v) > 0, k
        v.setflags(write=False)
    return out


def root_boards(n: int, seed: int = 0) -> np.ndarray:
    """n roots that cycle through the kinds of ``root_pool`` (so even n = 5 holds a terminal board, a one-move board, a full live
    board and an opening), each kind walked in a seeded order."""
    pool = root_pool()
    rng = np.random.default_rng(seed)
    order = {k: rng.permutation(len(v)) for k, v in pool.items()}
    kinds = ["terminal", "one_move", "full_live", "opening", "rest"]
    rows = [pool[kinds[i % 5]][order[kinds[i % 5]][(i // 5) % len(order[kinds[i % 5]])]] for i in range(n)]
    return np.ascontiguousarray(np.stack(rows), np.uint8)


# ---------------------------------------------------------------------------------------------- the shared test matrix
SHAPES = ((1, 1), (5, 3), (37, 3), (8, 64), (3, 130))  # one lane per pair .. several workgroups, R past a wave and past 128
GAMMAS = (1.0, 0.99)
STEPS, CUT = 12, 5
EXTRA_ROOTS, EXTRA_TAIL = 2, 5  # the lane0 case: two more boards in front, five unused key indices behind


@functools.lru_cache(maxsize=None)
def matrix_case(policy: int, mode: int, gamma: float, B: int, R: int) -> dict:
    """One case of the matrix, computed once and shared: 12 steps in one go (``full``), the state after the first 5 (``first``),
    and the same roots as rows 8 R .. of a run with two more boards in front inside a larger n_total (``ext``)."""
    roots = root_boards(B + EXTRA_ROOTS, seed=B * 1000 + R)
    _, subs = chain_keys(npo.key(7 + 13 * B + R), 2 * STEPS, mode)
    subs = subs.reshape(STEPS, 4)
    n = 4 * B * R
    own = roots[EXTRA_ROOTS:]
    first = playout(subs[:CUT], 0, own, R, 0, n, policy, gamma, mode)
    full = playout(subs[CUT:], CUT, None, R, 0, n, policy, gamma, mode, first)
    lane0 = 4 * EXTRA_ROOTS * R
    n_ext = lane0 + n + EXTRA_TAIL
    ext = playout(subs, 0, roots, R, 0, n_ext, policy, gamma, mode)
    out = dict(roots=own, all_roots=roots, subs=subs, first=first, full=full, ext=ext, lane0=lane0, n_ext=n_ext, n=n)
    for d in (first, full, ext):
        for v in d.values():
            v.setflags(write=False)
    return out


def matrix():
    return [(p, m, g, B, R) for p in (POLICY_DRUL, POLICY_RANDOM) for m in (npo.MODE_LEGACY, npo.MODE_PARTITIONABLE) for g in GAMMAS
            for (B, R) in SHAPES]
