"""Numpy restatement of the searched n-tuple episode player (include/g2048.h, "n-tuple searched episodes").  TEST INFRASTRUCTURE ONLY
(not a test module).

Nothing is restated here: per batch it composes the C oracle's ``chain`` / ``split`` / ``init`` / ``step`` (as
``ntuple_episodes_ref.play`` does) with the one-ply ``q`` of ``ntuple_search_ref.one_ply`` (``ntuple_stage_ref.expectimax`` for a
staged network) and ``ntuple_ref.masked_argmax``.  The argmax is masked by the STEP's mask, the env's, not by the ``legal`` of the search.

    batch j = games j bs .. min(N, (j + 1) bs) - 1, key chain from key(seed + j bs), B_total = the games it holds
    init sub-key = chain step 1; lock-step t: act sub-key = chain step 2 + 2 t (unused), step sub-key = chain step 3 + 2 t

The batches of an evaluation are independent of each other, and so are the evaluations: ``games(name, mode, gamma)`` plays every
batch of all ``SIZES`` (a batch that two sizes share is played once) through the lock-steps together, so that the search over their
boards is one numpy call per lock-step.  ``case`` concatenates the batches of one
evaluation into what the kernel leaves in its state arrays, the chain heads included (a finished game keeps the head it had after its
terminal step); all arrays are read-only.
"""
import functools

import numpy as np

import ntuple_episodes_ref as E
import ntuple_ref as N
import ntuple_search_ref as X
import ntuple_stage_ref as SR
from oracle import c_oracle as orc
from oracle import g2048_oracle as npo

SEED = E.SEED
STAGED = E.STAGED
NETWORKS = E.NETWORKS  # m = 3 L = 2, m = 2 L = 6, m = 8 L = 2 and the five-stage network
SIZES = ((1, 1), (17, 7), (30, 10), (23, 10))  # (N, bs): one game, a short last batch, full batches, full batches and a short one
MODES = E.MODES
GAMMAS = X.GAMMAS
network = E.network
chain_heads = E.chain_heads
mask_bool = E.mask_bool


def one_ply_q(boards, weights, tuples, frac_bits: int, gamma: float, tiles=None) -> np.ndarray:
    """q f32 [B, 4] of one ply of expectimax: the search modules' own."""
    if tiles is None:
        return X.one_ply(boards, tuples, weights, (gamma,), frac_bits)[0][gamma][0]
    return SR.expectimax(boards, weights, tuples, frac_bits, tiles, 1, (gamma,))[0][gamma][0]


def batches_of(n: int, bs: int, seed: int = SEED):
    """-> [(the seed of the batch's chain, its size)]"""
    return [(seed + first, min(bs, n - first)) for first in range(0, n, bs)]


class _Batch:
    def __init__(self, seed, b, mode):
        self.b, self.mode = b, mode
        self.key, subs = orc.chain(npo.key(seed), 1, mode)
        self.bd, self.mk, self.dn = orc.init(orc.split(subs[0], b, mode), mode)
        self.ep_len, self.score, self.illegal = np.zeros(b, np.int32), np.zeros(b, np.int64), np.zeros(b, bool)
        self.heads = np.tile(self.key, (b, 1)).astype(np.uint32)

    def step(self, live, a_live):
        a = np.zeros(self.b, np.int32)
        a[live] = a_live
        self.illegal[live] = ((self.mk[live] >> a_live) & 1) == 0
        self.key, subs = orc.chain(self.key, 2, self.mode)
        self.bd, self.mk, self.dn, r = orc.step(self.bd, self.mk, self.dn, a, orc.split(subs[1], self.b, self.mode), self.mode)
        assert (r == np.rint(r)).all()
        self.ep_len[live] += 1
        self.score[live] += r[live].astype(np.int64)
        self.heads[live] = self.key

    def result(self):
        out = dict(boards=self.bd, masks=self.mk, ep_len=self.ep_len, score=self.score, chain=self.heads, illegal=self.illegal)
        for v in out.values():
            v.setflags(write=False)
        return out


def play(name: str, wanted, max_steps: int = 1 << 16):
    """wanted: (mode, gamma, seed, b) per batch -> {that tuple: dict(boards, masks, ep_len, score, chain, illegal)}."""
    tuples, weights, frac_bits, tiles = network(name)
    state = {w: _Batch(w[2], w[3], w[0]) for w in wanted}
    for _ in range(max_steps):
        running = [(w, s, np.nonzero(s.dn == 0)[0]) for w, s in state.items()]
        running = [x for x in running if x[2].size]  # a finished batch: its chain stops with its last game
        if not running:
            break
        for gamma in sorted({w[1] for w, _, _ in running}):
            group = [x for x in running if x[0][1] == gamma]
            q = one_ply_q(np.concatenate([s.bd[live] for _, s, live in group]), weights, tuples, frac_bits, gamma, tiles)
            first = 0
            for _, s, live in group:
                s.step(live, N.masked_argmax(q[first:first + live.size], mask_bool(s.mk[live])))  # the env's mask
                first += live.size
    assert all((s.dn != 0).all() for s in state.values()), "max_steps reached"
    return {w: s.result() for w, s in state.items()}


@functools.lru_cache(maxsize=None)
def games(name: str, mode: int, gamma: float):
    return play(name, sorted({(mode, gamma, seed, b) for n, bs in SIZES for seed, b in batches_of(n, bs)}))


@functools.lru_cache(maxsize=None)
def case(name: str, mode: int, gamma: float, n: int, bs: int):
    if (n, bs) in SIZES and gamma in GAMMAS:
        parts = [games(name, mode, gamma)[(mode, gamma, seed, b)] for seed, b in batches_of(n, bs)]
    else:
        got = play(name, [(mode, gamma, seed, b) for seed, b in batches_of(n, bs)])
        parts = [got[(mode, gamma, seed, b)] for seed, b in batches_of(n, bs)]
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    for v in out.values():
        v.setflags(write=False)
    return out
