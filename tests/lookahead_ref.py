"""Numpy restatement of the one-ply expectimax enumeration and of Q, for the lookahead tests (not a test module).

Built on the pinned scalar rules of ``oracle.g2048_oracle`` (``move``, ``legal_mask``); nothing here is read by the product.

    expand(boards)                      -> after u8 [B,4,16], reward f32 [B,4], nchild i32 [B,4]
    children(after, nchild)             -> children u8 [N,16], terminal u8 [N], offset i32 [B,4]
    q_values(reward, nchild, offset, values, terminal, gamma, dtype)  -> q [B,4] in ``dtype``
    q_bound(...)                        -> 64 * 2^-24 * S per output (the derived f32 error bound of the reduce kernel)

Order of the children of (b, a): empty cells of the afterstate in ascending cell index, within a cell tile 2 (log2 = 1)
first, tile 4 (log2 = 2) second.  Spawn law (``oracle.g2048_oracle.spawn``): uniform over the empty cells, 2 with p = 0.9.
"""
import numpy as np

from oracle import g2048_oracle as npo

P2 = np.float32(0.9)  # the constants both sides use, as f32 values
P4 = np.float32(0.1)
MAX_CELLS = 15  # a legal move leaves at most 15 empty cells


def expand(boards: np.ndarray):
    boards = np.ascontiguousarray(boards, np.uint8)
    B = boards.shape[0]
    after = np.empty((B, 4, 16), np.uint8)
    reward = np.zeros((B, 4), np.float32)
    nchild = np.zeros((B, 4), np.int32)
    for a in range(4):
        moved, score = npo.move(boards, np.full(B, a, np.int32))
        legal = (moved != boards).any(axis=1)
        after[:, a] = np.where(legal[:, None], moved, boards)
        reward[:, a] = np.where(legal, score, np.float32(0.0))
        nchild[:, a] = np.where(legal, 2 * (moved == 0).sum(axis=1), 0)
    return after, reward, nchild


def exclusive_offsets(nchild: np.ndarray) -> np.ndarray:
    flat = nchild.reshape(-1).astype(np.int64)
    return (np.cumsum(flat) - flat).astype(np.int32).reshape(nchild.shape)


def children(after: np.ndarray, nchild: np.ndarray):
    pairs = after.reshape(-1, 16)
    has = (nchild.reshape(-1) > 0)
    pair_idx, cell_idx = np.nonzero((pairs == 0) & has[:, None])  # row-major: by pair, then ascending cell
    pair_idx, cell_idx = np.repeat(pair_idx, 2), np.repeat(cell_idx, 2)
    tile = np.tile(np.array([1, 2], np.uint8), len(pair_idx) // 2)
    out = pairs[pair_idx].copy()
    out[np.arange(len(out)), cell_idx] = tile
    terminal = (~npo.legal_mask(out).any(axis=1)).astype(np.uint8) if len(out) else np.zeros(0, np.uint8)
    return out, terminal, exclusive_offsets(nchild)


def spawn_probabilities(nchild: np.ndarray) -> np.ndarray:
    """Probability of every child, in enumeration order (float64): (0.9 | 0.1) / empty cells of its afterstate."""
    n = nchild.reshape(-1).astype(np.int64)
    per_pair = np.repeat(n // 2, n)
    return np.tile(np.array([0.9, 0.1]), int(n.sum()) // 2) / per_pair


def _cell_terms(nchild, offset, values, terminal, dtype, magnitude=False):
    """[P, 15] terms 0.9 v[2j] + 0.1 v[2j+1] (0 past the pair's cells), terminal children zeroed, in ``dtype``."""
    n = nchild.reshape(-1).astype(np.int64)
    o = offset.reshape(-1).astype(np.int64)
    v = np.where(np.asarray(terminal) != 0, 0, np.asarray(values)).astype(dtype)
    if magnitude:
        v = np.abs(v)
    v = np.concatenate([v, np.zeros(2 * MAX_CELLS, dtype)])  # padding for the gathers past a pair's range
    j = np.arange(MAX_CELLS)
    idx = o[:, None] + 2 * j[None, :]
    live = j[None, :] < (n // 2)[:, None]
    idx = np.where(live, idx, len(v) - 2)
    t = (dtype(P2) * v[idx]).astype(dtype) + (dtype(P4) * v[idx + 1]).astype(dtype)
    return np.where(live, t, dtype(0)).astype(dtype), n // 2


def q_values(reward, nchild, offset, values, terminal, gamma, dtype=np.float64):
    """reward + (float)gamma * (sum_j (0.9f v[2j] + 0.1f v[2j+1]) / n_e), summed in ascending j in ``dtype``; 0 where nchild == 0."""
    terms, ne = _cell_terms(nchild, offset, values, terminal, dtype)
    acc = np.zeros(len(ne), dtype)
    for j in range(MAX_CELLS):
        acc = (acc + terms[:, j]).astype(dtype)
    mean = (acc / np.maximum(ne, 1).astype(dtype)).astype(dtype)
    q = (reward.reshape(-1).astype(dtype) + (dtype(np.float32(gamma)) * mean).astype(dtype)).astype(dtype)
    return np.where(ne > 0, q, dtype(0)).reshape(nchild.shape)


def q_bound(reward, nchild, offset, values, terminal, gamma):
    """64 * 2^-24 * S, S = |reward| + gamma * sum_j (0.9 |v_2j| + 0.1 |v_2j+1|) in float64: at most 63 rounded f32 operations per
    output, each with relative error <= 2^-24 on a partial result no larger than S."""
    terms, _ = _cell_terms(nchild, offset, values, terminal, np.float64, magnitude=True)
    S = np.abs(reward.reshape(-1).astype(np.float64)) + np.float64(np.float32(gamma)) * terms.sum(axis=1)
    return (64.0 * 2.0 ** -24 * S).reshape(nchild.shape)


def hand_made_boards() -> np.ndarray:
    """The edge cases of the issue: one tile, full boards with / without a move, exactly one legal move, 2 2 2 2, big tiles."""
    rows = []
    for cell in (0, 5, 15):
        for t in (1, 2, 11):
            b = np.zeros(16, np.uint8)
            b[cell] = t
            rows.append(b)
    rows.append(np.zeros(16, np.uint8))                                                       # empty: nothing is legal
    rows.append(np.array([1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1], np.uint8))         # full, no move
    rows.append(np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16], np.uint8))  # full, no move, big tiles
    rows.append(np.array([1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4], np.uint8))         # full, horizontal merges only
    rows.append(np.array([1, 2, 3, 4, 1, 2, 3, 4, 5, 6, 7, 8, 5, 6, 7, 8], np.uint8))         # full, vertical merges only
    rows.append(np.array([3, 3, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1], np.uint8))         # full, one merge
    rows.append(np.array([1, 2, 3, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.uint8))         # only "down" is legal
    rows.append(np.array([1, 0, 0, 0, 2, 0, 0, 0, 3, 0, 0, 0, 4, 0, 0, 0], np.uint8))         # only "right" is legal
    rows.append(np.array([0, 0, 0, 1, 0, 0, 0, 2, 0, 0, 0, 3, 0, 0, 0, 4], np.uint8))         # only "left" is legal
    rows.append(np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 3, 2, 1], np.uint8))         # only "up" is legal
    rows.append(np.array([1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.uint8))         # 2 2 2 2
    rows.append(np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], np.uint8))         # 2 2 2 2 everywhere
    rows.append(np.array([2, 2, 1, 1, 3, 3, 3, 0, 4, 4, 0, 4, 5, 0, 5, 5], np.uint8))         # double merges, gaps
    rows.append(np.array([15, 15, 0, 0, 16, 16, 16, 16, 17, 0, 17, 0, 18, 18, 1, 1], np.uint8))  # log2 15 and above
    rows.append(np.array([29, 29, 0, 0, 28, 28, 28, 28, 0, 0, 0, 0, 30, 1, 30, 1], np.uint8))
    rows.append(np.array([15, 16, 17, 18, 18, 17, 16, 15, 15, 16, 17, 18, 20, 19, 16, 15], np.uint8))  # full, big, vertical merge
    return np.stack(rows)


def kernel_test_boards(n_random: int = 16000, seed: int = 20481) -> np.ndarray:
    """>= 20 000 boards: oracle rollouts (random and DRUL policy, both RNG modes), uniform tiles 0..11 with 0..16 empties, edges."""
    parts = [hand_made_boards()]
    for mode in (npo.MODE_LEGACY, npo.MODE_PARTITIONABLE):
        for policy, B in (("random", 24), ("drul", 12)):
            tr = npo.Runner(seed=3 + mode, mode=mode).run(B, policy)
            parts.append(tr["boards"].reshape(-1, 16))
            parts.append(tr["final_boards"].reshape(-1, 16))
    rng = np.random.default_rng(seed)
    rnd = rng.integers(1, 12, size=(n_random, 16)).astype(np.uint8)
    n_empty = rng.integers(0, 17, size=n_random)
    order = rng.random((n_random, 16)).argsort(axis=1)
    rnd[order < n_empty[:, None]] = 0  # exactly n_empty cells, uniformly placed
    parts.append(rnd)
    return np.ascontiguousarray(np.concatenate(parts), np.uint8)
