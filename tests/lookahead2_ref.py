"""Numpy restatement of two-ply expectimax with per-root afterstate dedup, for the expectimax tests (not a test module).

Built on ``lookahead_ref`` (one ply), which is built on the pinned scalar rules of ``oracle.g2048_oracle``; nothing here is read
by the product.

    group_starts(offset1, N1)                     -> i32 [B+1]: root b owns the level-2 pairs [4 offset1[b,0], 4 end_b)
    dedup(after2, nchild2, group_start)           -> rep i32 [N1,4], nuniq i32 [N1,4], first occurrence per group
    backup(reward2, nchild2, rep, e, dtype)       -> v1 [N1] = max over nchild2 > 0 of reward2 + e[rep], 0 if none
    pipeline(boards, value_fn, gamma, dtype, dedup) -> dict of every intermediate and ``q2``
    q2_values(...)                                -> q2 [B,4] in ``dtype``
    q2_bound(pipe64, gamma, value_rounding)       -> the f32 error bound of q2 per output, in float64
"""
import numpy as np

import lookahead_ref as R

EPS = 2.0 ** -24
MAX_GROUP = 480


def group_starts(offset1: np.ndarray, N1: int) -> np.ndarray:
    return np.concatenate([4 * offset1[:, 0].astype(np.int64), [4 * N1]]).astype(np.int32)


def dedup(after2: np.ndarray, nchild2: np.ndarray, group_start: np.ndarray):
    keys = after2.reshape(-1, 16)
    n = nchild2.reshape(-1)
    rep = np.arange(len(n), dtype=np.int32)
    for g in range(len(group_start) - 1):
        first = {}
        for p in range(int(group_start[g]), int(group_start[g + 1])):
            if n[p] > 0:
                rep[p] = first.setdefault(keys[p].tobytes(), p)
    nuniq = np.where(rep == np.arange(len(n)), n, 0).astype(np.int32)
    return rep.reshape(nchild2.shape), nuniq.reshape(nchild2.shape)


def backup(reward2, nchild2, rep, e, dtype=np.float64):
    x = (reward2.astype(dtype) + e.reshape(-1).astype(dtype)[rep]).astype(dtype)
    legal = nchild2 > 0
    best = np.where(legal, x, -np.inf).max(axis=1) if len(x) else np.zeros(0)
    return np.where(legal.any(axis=1), best, 0).astype(dtype)


def pipeline(boards, value_fn, gamma, dtype=np.float64, dedup_pairs=True):
    """``value_fn(children u8 [n,16]) -> values [n]`` is called once on all level-2 children (cast to ``dtype``)."""
    after1, reward1, nchild1 = R.expand(boards)
    children1, terminal1, offset1 = R.children(after1, nchild1)
    N1 = len(children1)
    after2, reward2, nchild2 = R.expand(children1) if N1 else (np.zeros((0, 4, 16), np.uint8), np.zeros((0, 4), np.float32),
                                                                np.zeros((0, 4), np.int32))
    gs = group_starts(offset1, N1)
    if dedup_pairs:
        rep, nuniq = dedup(after2, nchild2, gs)
    else:
        rep, nuniq = np.arange(4 * N1, dtype=np.int32).reshape(N1, 4), nchild2
    children2, terminal2, offset2 = R.children(after2, nuniq)
    values = np.asarray(value_fn(children2)).astype(dtype) if len(children2) else np.zeros(0, dtype)
    e = R.q_values(np.zeros_like(reward2), nuniq, offset2, values, terminal2, gamma, dtype)
    v1 = backup(reward2, nchild2, rep, e, dtype)
    q2 = R.q_values(reward1, nchild1, offset1, v1, terminal1, gamma, dtype)
    return dict(after1=after1, reward1=reward1, nchild1=nchild1, children1=children1, terminal1=terminal1, offset1=offset1,
                after2=after2, reward2=reward2, nchild2=nchild2, group_start=gs, rep=rep, nuniq=nuniq, children2=children2,
                terminal2=terminal2, offset2=offset2, values=values, e=e, v1=v1, q2=q2)


def q2_values(boards, value_fn, gamma, dtype=np.float64, dedup=True):
    return pipeline(boards, value_fn, gamma, dtype, dedup)["q2"]


def q2_bound(p, gamma, value_rounding=True):
    """|q2_f32 - q2_f64| per output, from a float64 ``pipeline`` result ``p``.  Three terms:

    err2[c] = max over a' of the one-ply bound of level 2, 64 * 2^-24 * (|reward2| + S_e[rep]) with S_e = gamma * sum_j (0.9 |v_2j|
              + 0.1 |v_2j+1|) (``R.q_bound`` with a zero reward on the pair that was valued), plus, for a critic whose f32 value is
              the float64 value rounded once, 2^-24 * S_e[rep] (each |v| is off by at most 2^-24 |v|, and the mean is no larger than
              the sum).  The error of a max is at most the max of the errors.
    level 1: ``R.q_bound`` of the level-1 reduce on |V1| + err2 (the f32 reduce runs on the perturbed values),
    and the perturbation itself carried through the exact expectation: gamma * (0.9 / 0.1-weighted mean of err2)."""
    S_e = R.q_bound(np.zeros_like(p["reward2"]), p["nuniq"], p["offset2"], p["values"], p["terminal2"], gamma) / (64.0 * EPS)
    S_at = S_e.reshape(-1)[p["rep"]]
    b2 = 64.0 * EPS * (np.abs(p["reward2"].astype(np.float64)) + S_at) + (EPS * S_at if value_rounding else 0.0)
    err2 = np.where(p["nchild2"] > 0, b2, 0.0).max(axis=1) if len(b2) else np.zeros(0)
    level1 = R.q_bound(p["reward1"], p["nchild1"], p["offset1"], np.abs(p["v1"].astype(np.float64)) + err2, p["terminal1"], gamma)
    terms, ne = R._cell_terms(p["nchild1"], p["offset1"], err2, p["terminal1"], np.float64)
    carried = np.float64(np.float32(gamma)) * terms.sum(axis=1) / np.maximum(ne, 1)
    return level1 + carried.reshape(p["nchild1"].shape)


def test_boards() -> np.ndarray:
    """The hand-made edge cases (among them the one-tile board at cell 5: 4 moves x 15 empties x 2 = 120 children = 480 pairs,
    the largest group; full boards without a move: an empty group; boards with one legal move) and every fourth lock-step of two
    4-board oracle rollouts, random and DRUL (consecutive steps differ by one move; a few hundred boards, about 6e5 level-2
    children, keep the numpy reference at seconds)."""
    from oracle import g2048_oracle as npo

    parts = [R.hand_made_boards()]
    for policy in ("random", "drul"):
        parts.append(npo.Runner(seed=5, mode=npo.MODE_LEGACY).run(4, policy)["boards"][:, ::4].reshape(-1, 16))
    return np.ascontiguousarray(np.concatenate(parts), np.uint8)


test_boards.__test__ = False  # a helper, whatever its name


def table(seed: int) -> np.ndarray:
    """T f32 [16,32] of the table critic: V(s) = sum_cell T[cell, tile]."""
    return np.random.default_rng(seed).normal(0.0, 1.0, (16, 32)).astype(np.float32)


def table_values(T: np.ndarray, boards: np.ndarray) -> np.ndarray:
    """float64 sum (exact to ~1e-16 relative); the device critic rounds this once to f32."""
    return T.astype(np.float64)[np.arange(16)[None, :], boards.astype(np.int64)].sum(axis=1)
