"""The reference of the n-tuple budgeted search, composed from the restatements of tests/ (not a test module).

    depths(boards, max_depth, budget) -> d u8 [B], entries i32 [B, 6]
    search(boards, tuples, w, max_depth, budget, gamma, tiles=None, only=None) -> q f32 [B,4], v f32 [B], d u8 [B], entries i32 [B,6]

No arithmetic is added.  ``U_j`` of a root is the number of ``np.unique`` rows among the afterstates ``lookahead_ref.expand`` gives
for the positions of level j, which are ``lookahead_ref.children`` of the unique afterstates of level j - 1; the enumeration of a root
stops at the first level with more than ``budget`` rows (that level is counted, never expanded), which gives ``d(s)``.  The scores
of the roots with ``d(s) = k`` are ``ntuple_frontier_ref.search(those roots, depth=k, dedup=True)``: the reference never builds a level
the rule rejects.  ``only`` (a boolean mask) limits the value computation to those roots; the others' q and v rows are NaN.
"""
import functools

import numpy as np

import lookahead_ref as R
import ntuple_frontier_ref as FR
import ntuple_search_ref as X
import ntuple_stage_ref as ST

F32 = np.float32
MAX_DEPTH, MIN_BUDGET, MAX_BUDGET = 6, 4, 24576
BUDGETS = (8, 70, 600, 2100)  # at max_depth 4: every depth occurs at each of them on the 35 "small" boards
HISTOGRAMS = {  # budget -> the roots with d = 1, 2, 3, 4 at max_depth 4
    "small": {8: (29, 1, 0, 5), 70: (9, 19, 2, 5), 600: (0, 13, 16, 6), 2100: (0, 0, 21, 14)},
    "other": {8: (11, 0, 0, 1), 70: (8, 3, 0, 1), 600: (0, 9, 2, 1), 2100: (0, 0, 10, 2)},
}
DEEP = dict(max_depth=5, budget=24576, boards=(14, 28, 32, 27),  # of the "small" boards: three reach depth 5, board 27 stops at 4
            entries=((2, 8, 68, 892, 12787), (4, 40, 304, 2025, 14463), (2, 17, 65, 327, 2011)), depth=(5, 5, 5, 4), u5_of_27=65734)


def _unique(rows):
    rows = np.ascontiguousarray(rows)
    if not len(rows):
        return rows
    return np.unique(rows.view(np.dtype((np.void, 16))).reshape(-1)).view(np.uint8).reshape(-1, 16)


def root_levels(board, max_depth, budget):
    """-> [U_1, ..] of one root: every level that was enumerated, the last one past the budget if the rule stopped there."""
    counts, pos = [], np.ascontiguousarray(board, np.uint8).reshape(1, 16)
    for _ in range(max_depth):
        after, _, nchild = R.expand(pos)
        uniq = _unique(after.reshape(-1, 16)[(nchild > 0).reshape(-1)])
        counts.append(len(uniq))
        if len(uniq) > budget or len(counts) == max_depth:
            break
        n = (2 * (uniq == 0).sum(axis=1)).astype(np.int32)
        pos = R.children(uniq[:, None, :], n[:, None])[0] if len(uniq) else np.zeros((0, 16), np.uint8)
    return counts


@functools.lru_cache(maxsize=None)
def _depths(key, max_depth, budget):
    boards = np.frombuffer(key, np.uint8).reshape(-1, 16)
    d, entries = np.zeros(len(boards), np.uint8), np.zeros((len(boards), 6), np.int32)
    over = np.zeros(len(boards), np.int64)  # the count of the level that stopped the root, 0 if none did
    for i, b in enumerate(boards):
        u = root_levels(b, max_depth, budget)
        if u[-1] > budget:
            over[i] = u.pop()
        d[i] = len(u)
        entries[i, :len(u)] = u
    for a in (d, entries, over):
        a.setflags(write=False)
    return d, entries, over


def depths(boards, max_depth, budget, with_over=False):
    out = _depths(np.ascontiguousarray(boards, np.uint8).tobytes(), int(max_depth), int(budget))
    return out if with_over else out[:2]


def search(boards, tuples, w, max_depth, budget, gamma, tiles=None, frac_bits=X.FRAC_BITS, only=None, memo=None):
    boards = np.ascontiguousarray(boards, np.uint8).reshape(-1, 16)
    d, entries = depths(boards, max_depth, budget)
    q, v = np.full((len(boards), 4), np.nan, F32), np.full(len(boards), np.nan, F32)
    want = np.ones(len(boards), bool) if only is None else np.asarray(only, bool)
    for k in range(1, max_depth + 1):
        rows = np.flatnonzero((d == k) & want)
        if len(rows):
            q[rows], v[rows], counts = FR.search(boards[rows], tuples, w, k, gamma, True, tiles=tiles, frac_bits=frac_bits, memo=memo)
            assert np.array_equal(counts[:k], entries[rows, :k].sum(axis=0))  # the two enumerations agree
    return q, v, d, entries


# ---- the cases of the CPU and the GPU tests, computed once per process -----------------------------------------------------------
NETWORKS = ("small", "wide", "eight", "small5")  # m = 3 L = 2 on the 35 boards; m = 2 L = 6, m = 8 L = 2 and five stages on the 12


def network(name):
    """-> (tuples, weights, frac_bits, stage tiles or None, boards)"""
    if name == "small5":
        tuples, tiles, F = ST.NETWORKS["small5"]
        return tuples, ST.staged_weights("small5"), F, tuple(tiles), FR.boards_for("other")
    tuples, w = X.network(name)
    return tuples, w, X.FRAC_BITS, None, FR.boards_for(name)


@functools.lru_cache(maxsize=None)
def case(name, max_depth, budget, rows=None):
    """-> dict(boards, tuples, weights, frac_bits, tiles, legal, q={gamma: ..}, v={gamma: ..}, depth, entries), arrays read-only.
    ``rows`` (a tuple of indices) takes those boards of the network's set."""
    tuples, w, F, tiles, boards = network(name)
    if rows is not None:
        boards = np.ascontiguousarray(boards[list(rows)])
    memo, q, v = {}, {}, {}
    for g in X.GAMMAS:
        q[g], v[g], d, entries = search(boards, tuples, w, max_depth, budget, g, tiles=tiles, frac_bits=F, memo=memo)
    out = dict(boards=boards, tuples=tuples, weights=w, frac_bits=F, tiles=tiles, legal=R.expand(boards)[2] > 0, q=q, v=v, depth=d,
               entries=entries)
    for a in [out["legal"], *q.values(), *v.values()]:
        a.setflags(write=False)
    return out
