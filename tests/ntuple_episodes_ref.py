"""Numpy restatement of the n-tuple episode player (include/g2048.h, "n-tuple episodes").  TEST INFRASTRUCTURE ONLY (not a test module).

Nothing is restated here: per batch it composes the C oracle's ``chain`` / ``split`` / ``init`` / ``step`` (as
``ntuple_ref.engine_training`` does) with ``ntuple_ref.scores`` (``ntuple_stage_ref.scores`` for a staged network) and
``ntuple_ref.masked_argmax``.  The argmax is masked by the STEP's mask, the env's, not by the ``legal`` of the scores.

    batch j = games j bs .. min(N, (j + 1) bs) - 1, key chain from key(seed + j bs), B_total = the games it holds
    init sub-key = chain step 1; lock-step t: act sub-key = chain step 2 + 2 t (unused), step sub-key = chain step 3 + 2 t

``play`` returns what the kernel leaves in its state arrays, the chain heads included (a finished game keeps the head it had after
its terminal step).  ``case`` holds one evaluation per (network, mode, N, bs), computed once per process and read-only.
"""
import functools

import numpy as np

import ntuple_ref as N
import ntuple_search_ref as X
import ntuple_stage_ref as SR
from oracle import c_oracle as orc
from oracle import g2048_oracle as npo

SEED = 42
STAGED = "small5"
NETWORKS = ("small", "wide", "eight", STAGED)
SIZES = ((1, 1), (17, 7), (100, 100), (230, 100))  # (N, bs): one game, a short last batch, one full batch, the protocol's shape
MODES = (npo.MODE_LEGACY, npo.MODE_PARTITIONABLE)
INT32_MIN = -2 ** 31


@functools.lru_cache(maxsize=None)
def network(name: str):
    """-> (tuples, weights i32 [m, 16^L] or [S, m, 16^L] (read-only), frac_bits, tiles or None)."""
    if name == STAGED:
        tuples, tiles, F = SR.NETWORKS[name]
        return tuples, SR.staged_weights(name), F, tiles
    if name == "floor":  # the edge case: every legal score is about -5.2e10 (24 entries of -2^31), below the -1e8 of a masked move
        w = np.full(N.zero_weights(N.SMALL).shape, INT32_MIN, np.int32)
        w.setflags(write=False)
        return N.SMALL, w, 0, None
    tuples, w = X.network(name)
    return tuples, w, X.FRAC_BITS, None


def mask_bool(masks) -> np.ndarray:
    return ((np.asarray(masks, np.uint8)[:, None] >> np.arange(4, dtype=np.uint8)) & 1).astype(bool)


def chain_heads(n: int, bs: int, seed: int = SEED) -> np.ndarray:
    """u32 [n, 2]: what the caller seeds the games with, the key of the game's batch."""
    return np.stack([npo.key(seed + (i // bs) * bs) for i in range(n)]).astype(np.uint32)


def play(weights, tuples, frac_bits: int, n: int, bs: int, mode: int, tiles=None, seed: int = SEED, max_steps: int = 1 << 16):
    """-> dict(boards u8 [n,16], masks u8 [n], ep_len i32 [n], score i64 [n], chain u32 [n,2], illegal bool [n]: the game ended by
    a move its mask forbids)."""
    firsts = list(range(0, n, bs))
    keys, state = [], []
    for first in firsts:  # (the batches are independent: they go through the lock-steps together, so the scores are one numpy call)
        b = min(bs, n - first)
        key, subs = orc.chain(npo.key(seed + first), 1, mode)
        keys.append(key)
        state.append(list(orc.init(orc.split(subs[0], b, mode), mode)))
    ep_len, score, illegal = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, bool)
    heads = np.concatenate([np.tile(k, (len(st[0]), 1)) for k, st in zip(keys, state)]).astype(np.uint32)
    for _ in range(max_steps):
        boards, masks, done = (np.concatenate([st[k] for st in state]) for k in range(3))
        live = np.nonzero(done == 0)[0]
        if live.size == 0:
            break
        if tiles is None:
            q, _, _ = N.scores(boards[live], weights, tuples, frac_bits)
        else:
            q, _, _ = SR.scores(boards[live], weights, tuples, frac_bits, tiles)
        a = np.zeros(n, np.int32)
        a[live] = N.masked_argmax(q, mask_bool(masks[live]))  # the env's mask
        illegal[live] = ((masks[live] >> a[live]) & 1) == 0
        for j, first in enumerate(firsts):
            bd, mk, dn = state[j]
            if (dn != 0).all():
                continue  # a finished batch: its chain stops with its last game
            b = len(bd)
            keys[j], subs = orc.chain(keys[j], 2, mode)
            was_live = first + np.nonzero(dn == 0)[0]
            bd, mk, dn, r = orc.step(bd, mk, dn, a[first:first + b], orc.split(subs[1], b, mode), mode)
            assert (r == np.rint(r)).all()
            state[j] = [bd, mk, dn]
            ep_len[was_live] += 1
            score[was_live] += r[was_live - first].astype(np.int64)
            heads[was_live] = keys[j]
    boards, masks, done = (np.concatenate([st[k] for st in state]) for k in range(3))
    assert (done != 0).all(), "max_steps reached"
    return dict(boards=boards, masks=masks, ep_len=ep_len, score=score, chain=heads, illegal=illegal)


@functools.lru_cache(maxsize=None)
def case(name: str, mode: int, n: int, bs: int):
    tuples, w, F, tiles = network(name)
    out = play(w, tuples, F, n, bs, mode, tiles)
    for v in out.values():
        v.setflags(write=False)
    return out
