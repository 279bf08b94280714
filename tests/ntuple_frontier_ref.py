"""The numpy restatements of tests/ composed into the reference of the n-tuple frontier search (not a test module).

    search(boards, tuples, w, depth, gamma, dedup, tiles=None) -> q f32 [B,4], v f32 [B], counts int64 [3]

Level by level: ``lookahead_ref.expand`` gives the afterstates of the positions of a level, ``lookahead_ref.children`` their spawn
children, which are the positions of the next level; the last level's children are valued by ``ntuple_ref.scores`` (the staged case by
``ntuple_stage_ref.scores``) and ``lookahead_ref.q_values`` folds every level back.  Nothing is restated here: the enumeration, the
reduction and the n-tuple scores are the modules' own.  With ``dedup`` the (root, afterstate) rows of a level are made unique with
``np.unique`` before they are expanded, and ``q_values`` is pointed at the children of the unique row through its ``offset``
argument.  Equal leaf boards are valued once either way.  ``counts`` = the unique (root, afterstate) rows per level with ``dedup``,
the plain number without; 0 beyond ``depth``.
"""
import functools

import numpy as np

import lookahead2_ref as R2
import lookahead_ref as R
import ntuple_ref as N
import ntuple_search_ref as X
import ntuple_stage_ref as ST

F32 = np.float32
FRAC_BITS = X.FRAC_BITS
GAMMAS = X.GAMMAS
DEPTHS = (1, 2, 3)
N_HAND_MADE = 25


def _leaf_values(boards, tuples, w, frac_bits, tiles, memo):
    """V_0 of the boards, every distinct board valued once."""
    if not len(boards):
        return np.zeros(0, F32)
    key = (boards.shape, hash(boards.tobytes()))
    if memo is not None and key in memo:
        return memo[key]
    rows = np.ascontiguousarray(boards).view(np.dtype((np.void, 16))).reshape(-1)
    uniq, inv = np.unique(rows, return_inverse=True)
    ub = uniq.view(np.uint8).reshape(-1, 16)
    v = (N.scores(ub, w, tuples, frac_bits) if tiles is None else ST.scores(ub, w, tuples, frac_bits, tiles))[1]
    out = np.asarray(v, F32)[inv.reshape(-1)]
    if memo is not None:
        memo[key] = out
    return out


def _level(pos, root, k, gamma, dedup, leaf, counts):
    """Q_k and V_k of the positions ``pos`` (u8 [n,16]) that descend from the roots ``root`` (u32 [n])."""
    n = len(pos)
    after, reward, nchild = R.expand(pos)
    legal = nchild > 0
    flat = legal.reshape(-1)
    rows = np.concatenate([np.repeat(root, 4)[flat].astype("<u4").view(np.uint8).reshape(-1, 4), after.reshape(-1, 16)[flat]], axis=1)
    rows = np.ascontiguousarray(rows)
    if dedup and len(rows):
        uniq, inv = np.unique(rows.view(np.dtype((np.void, 20))).reshape(-1), return_inverse=True)
        uniq, inv = uniq.view(np.uint8).reshape(-1, 20), inv.reshape(-1)
    else:
        uniq, inv = rows, np.arange(len(rows))
    counts[len(counts) - k] += len(uniq)
    u_after = np.ascontiguousarray(uniq[:, 4:])
    u_root = np.ascontiguousarray(uniq[:, :4]).view("<u4").reshape(-1)
    u_nchild = (2 * (u_after == 0).sum(axis=1)).astype(np.int32)
    ch, term, u_off = R.children(u_after[:, None, :], u_nchild[:, None])
    v_ch = leaf(ch) if k == 1 else _level(ch, np.repeat(u_root, u_nchild), k - 1, gamma, dedup, leaf, counts)[1]
    offset = np.zeros(4 * n, np.int32)
    offset[flat] = u_off.reshape(-1)[inv]  # every (position, action) reads the children of its unique afterstate
    q = R.q_values(reward, nchild, offset.reshape(n, 4), v_ch, term, gamma, F32).astype(F32)
    return q, X._best(q, legal)


def search(boards, tuples, w, depth, gamma, dedup, tiles=None, frac_bits=FRAC_BITS, memo=None):
    boards = np.ascontiguousarray(boards, np.uint8).reshape(-1, 16)
    counts = [0] * depth
    q, v = _level(boards, np.arange(len(boards), dtype=np.uint32), depth, gamma, dedup,
                  lambda b: _leaf_values(b, tuples, w, frac_bits, tiles, memo), counts)
    return q, v, np.array(counts + [0] * (3 - depth), np.int64)


@functools.lru_cache(maxsize=None)
def boards_for(shape: str) -> np.ndarray:
    """"small": all 25 hand-made boards and 10 rollout boards; the wide shapes: 4 hand-made boards with the edge cases and 8 rollout
    boards (the numpy reference stays at seconds)."""
    hand, roll = R.hand_made_boards(), R2.test_boards()[N_HAND_MADE:]
    assert len(hand) == N_HAND_MADE
    if shape == "small":
        b = np.concatenate([hand, roll[:: len(roll) // 10][:10]])
    else:
        b = np.concatenate([hand[[4, 10, 15, 22]], roll[:: len(roll) // 8][:8]])  # 120 children, no move, one move, tiles above 15
    b = np.ascontiguousarray(b, np.uint8)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def case(shape: str, depth: int):
    """-> dict(boards, tuples, weights, legal, nchild, q={gamma: f32 [B,4]}, v={gamma: f32 [B]}, counts={dedup: int64 [3]}), computed
    once per process with dedup on, arrays read-only.  The counts without dedup come from the enumeration alone."""
    tuples, w = X.network(shape)
    boards = boards_for(shape)
    memo, q, v, counts = {}, {}, {}, {}
    for g in GAMMAS:
        q[g], v[g], counts[True] = search(boards, tuples, w, depth, g, True, memo=memo)
    counts[False] = plain_counts(boards, depth)
    _, _, nchild = R.expand(boards)
    out = dict(boards=boards, tuples=tuples, weights=w, legal=nchild > 0, nchild=nchild.sum(axis=1), q=q, v=v, counts=counts)
    for a in [out["legal"], out["nchild"], *q.values(), *v.values(), *counts.values()]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _plain_counts(key, depth):
    boards = np.frombuffer(key, np.uint8).reshape(-1, 16)
    counts, pos = [], boards
    for level in range(depth):
        after, _, nchild = R.expand(pos)
        counts.append(int((nchild > 0).sum()))
        if level + 1 < depth:
            pos = R.children(after, nchild)[0]
    return np.array(counts + [0] * (3 - depth), np.int64)


def plain_counts(boards, depth):
    """|A_1|, |A_2|, |A_3| without merging: the legal (position, action) pairs of every level of the plain enumeration."""
    return _plain_counts(np.ascontiguousarray(boards, np.uint8).tobytes(), depth)
