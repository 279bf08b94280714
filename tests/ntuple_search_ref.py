"""The numpy restatements of tests/ composed into the reference of n-tuple expectimax (not a test module).

    one ply : ``lookahead_ref.q_values(..., dtype=np.float32)`` over ``ntuple_ref.scores(children)[1]``
    two plies: ``lookahead2_ref.pipeline(boards, value_fn, gamma, np.float32, dedup_pairs=False)`` with the same ``value_fn``

Nothing is restated here: the enumeration, the reduction and the n-tuple scores are the modules' own.  ``case(shape, plies)`` holds
the boards and the expected ``q`` / ``v`` / ``legal`` per gamma of one network shape, computed once per process and read-only.
"""
import functools

import numpy as np

import lookahead2_ref as R2
import lookahead_ref as R
import ntuple_ref as N

F32 = np.float32
FRAC_BITS = 12
GAMMAS = (1.0, 0.99)
EIGHT = ((0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (8, 9), (10, 11), (14, 15))  # m = 8, L = 2: the widest register arrays


@functools.lru_cache(maxsize=None)
def network(shape: str):
    """-> (tuples, weights i32 [m, 16^L], read-only)."""
    if shape == "small":
        return N.SMALL, N.small_weights()
    if shape == "wide":
        return N.WIDE, N.wide_weights()
    w = N.random_weights(EIGHT, seed=3)
    w.setflags(write=False)
    return EIGHT, w


@functools.lru_cache(maxsize=None)
def boards_for(shape: str, plies: int) -> np.ndarray:
    if plies == 1:
        b = np.concatenate([R.hand_made_boards(), N.boards_for(257, seed=3)])
    else:
        b = np.concatenate([R.hand_made_boards(), R2.test_boards()[::3]])
        if shape != "small":
            b = b[:48]  # the wide shapes: the numpy reference stays at seconds
    b = np.ascontiguousarray(b, np.uint8)
    b.setflags(write=False)
    return b


def _best(q, legal):
    v = np.where(legal, q, -np.inf).max(axis=1)
    return np.where(legal.any(axis=1), v, 0).astype(F32)


def one_ply(boards, tuples, w, gammas=GAMMAS, frac_bits=FRAC_BITS):
    """-> {gamma: (q f32 [B,4], v f32 [B])}, legal bool [B,4], children per board."""
    after, reward, nchild = R.expand(boards)
    children, terminal, offset = R.children(after, nchild)
    v0 = N.scores(children, w, tuples, frac_bits)[1]
    legal = nchild > 0
    out = {}
    for g in gammas:
        q = R.q_values(reward, nchild, offset, v0, terminal, g, F32).astype(F32)
        out[g] = (q, _best(q, legal))
    return out, legal, nchild.sum(axis=1)


def two_plies(boards, tuples, w, gammas=GAMMAS, frac_bits=FRAC_BITS):
    memo = {}

    def value_fn(children):  # the level-2 children do not depend on gamma: valued once
        key = (children.shape, hash(children.tobytes()))
        if key not in memo:
            memo[key] = N.scores(children, w, tuples, frac_bits)[1]
        return memo[key]

    out, legal, n1 = {}, None, None
    for g in gammas:
        p = R2.pipeline(boards, value_fn, g, F32, dedup_pairs=False)
        legal, n1 = p["nchild1"] > 0, p["nchild1"].sum(axis=1)
        q = p["q2"].astype(F32)
        out[g] = (q, _best(q, legal))
    return out, legal, n1


@functools.lru_cache(maxsize=None)
def case(shape: str, plies: int):
    """-> dict(boards, tuples, weights, legal, nchild, q={gamma: f32 [B,4]}, v={gamma: f32 [B]}), arrays read-only."""
    tuples, w = network(shape)
    boards = boards_for(shape, plies)
    res, legal, nchild = (one_ply if plies == 1 else two_plies)(boards, tuples, w)
    out = dict(boards=boards, tuples=tuples, weights=w, legal=legal, nchild=nchild, q={g: r[0] for g, r in res.items()},
               v={g: r[1] for g, r in res.items()})
    for a in [legal, nchild, *out["q"].values(), *out["v"].values()]:
        a.setflags(write=False)
    return out


def check_inputs(boards, legal, nchild):
    """The edge cases the issue wants among the inputs."""
    assert (nchild == 120).any()              # the one-tile board off the edge: 4 moves x 15 empty cells x 2 tiles
    assert (~legal.any(axis=1)).any()         # no legal move
    assert (legal.sum(axis=1) == 1).any()     # exactly one
    assert boards.max() > 15                  # the index clamp
