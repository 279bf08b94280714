"""N-tuple afterstate value network: table-lookup play and on-device TD(0) learning (no reference counterpart).

    V(s) = 2^-F * sum over the eight views g of s and the tuples t of weights[t][idx(view_g(s), t)]

The 2048 literature's standard learner: no matrix engine, one evaluation is ``8 m`` gathers, one update ``8 m`` integer atomics.
The player scores every legal move by ``reward + V(afterstate)`` (``g2048_ntuple_scores``) and the engine takes the masked argmax;
the trainer learns V by temporal differences between consecutive afterstates of always-live boards, batch-synchronously: all envs
of a lock-step accumulate into integer tables (``g2048_ntuple_td_accumulate``), every entry that was hit moves by the mean of its
deltas (``g2048_ntuple_td_apply``).  All accumulation is integer arithmetic, so a run is reproducible bit for bit.  How the scores
become moves outside the trainer (the un-batched ``__call__``, the rng mode) is ``QPlayer``'s (``q_player.py``).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..actions import _common as C
from ..g2048 import native as nv
from ..g2048.engine import seed_key
from .q_player import QPlayer

DEFAULT_TUPLES = ((0, 1, 2, 3, 4, 5), (4, 5, 6, 7, 8, 9), (0, 1, 2, 4, 5, 6), (4, 5, 6, 8, 9, 10))
MAX_TUPLES, MAX_CELLS, MAX_FRAC_BITS = 8, 6, 20
MAX_STAGES, MAX_STAGE_TILE = 8, 17
MAX_HORIZON = 8
SEARCH_CHUNK = 1 << 16  # roots per two-ply call: 128 workspace floats each
SEARCH_EPISODE_STEPS = 256  # steps per launch of the searched episode kernel (play_search_episodes has the reason)


def _check_search(plies, gamma):
    """-> (plies, gamma) as (int, float); ``ValueError`` for plies outside {0, 1, 2} or a gamma that is negative or not finite."""
    if isinstance(plies, bool) or plies not in (0, 1, 2):
        raise ValueError(f"plies must be 0, 1 or 2, got {plies!r}")
    try:
        g = float(gamma)
    except (TypeError, ValueError):
        raise ValueError(f"gamma must be a finite non-negative number, got {gamma!r}") from None
    if not (np.isfinite(g) and g >= 0.0):
        raise ValueError(f"gamma must be a finite non-negative number, got {gamma!r}")
    return int(plies), g


FRONTIER_CHUNK = {1: 1 << 16, 2: 1 << 13, 3: 1 << 8}  # roots per frontier-search call: about 6 MB, 100 MB and 0.36 GB of workspace


def _check_depth(depth, gamma):
    """-> (depth, gamma) as (int, float); ``ValueError`` for a depth that is a bool, not an integer or outside 1 .. 3, and for a gamma
    that is negative or not finite."""
    if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or not 1 <= int(depth) <= 3:
        raise ValueError(f"depth must be 1, 2 or 3, got {depth!r}")
    return int(depth), _check_search(0, gamma)[1]


BUDGET_MAX_DEPTH, BUDGET_MIN, BUDGET_MAX = 6, 4, 24576
BUDGET_WORKSPACE_BYTES = 4 << 30  # the most workspace ``search_budget`` keeps: a chunk is the roots that fit, at least one
# what ``search_budget`` searches by default ("N-tuple budgeted search", has the measurements behind them)
BUDGET_DEFAULT_DEPTH, BUDGET_DEFAULT = 4, 8192


def _check_budget(max_depth, budget, gamma):
    """-> (max_depth, budget, gamma) as (int, int, float); ``ValueError`` for a ``max_depth`` or ``budget`` that is a bool, not an
    integer or outside 1 .. 6 / 4 .. 24 576, and for a gamma that is negative or not finite."""
    for name, x, lo, hi in (("max_depth", max_depth, 1, BUDGET_MAX_DEPTH), ("budget", budget, BUDGET_MIN, BUDGET_MAX)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not lo <= int(x) <= hi:
            raise ValueError(f"{name} must be an integer in {lo} .. {hi}, got {x!r}")
    return int(max_depth), int(budget), _check_search(0, gamma)[1]


def budget_chunk(max_depth: int, budget: int) -> int:
    """The roots per call of ``search_budget``: the most whose workspace stays at or below ``BUDGET_WORKSPACE_BYTES`` (the size is
    linear in the roots but for 16-byte rounding), at least 1 and at most the entry point's own limit."""
    size = nv.load().g2048_ntuple_budget_search_workspace_bytes  # -1 past the entry point's limit
    lo, hi = 1, max(1, BUDGET_WORKSPACE_BYTES // nv.ntuple_budget_search_workspace_bytes(1, max_depth, budget))
    while lo < hi:  # the largest n that has a size within the bound: both conditions hold up to some n and fail above it
        mid = (lo + hi + 1) // 2
        if 0 < size(mid, max_depth, budget) <= BUDGET_WORKSPACE_BYTES:
            lo = mid
        else:
            hi = mid - 1
    return lo


def _check_tuples(tuples) -> np.ndarray:
    try:
        rows = [tuple(int(c) for c in t) for t in tuples]
    except TypeError:
        raise ValueError(f"tuples must be a sequence of sequences of cell indices, got {tuples!r}") from None
    if not 1 <= len(rows) <= MAX_TUPLES:
        raise ValueError(f"the number of tuples must be in 1 .. {MAX_TUPLES}, got {len(rows)}")
    L = len(rows[0])
    if not 1 <= L <= MAX_CELLS:
        raise ValueError(f"a tuple has 1 .. {MAX_CELLS} cells, got {L}")
    for t in rows:
        if len(t) != L:
            raise ValueError(f"all tuples must have the same number of cells, got {rows!r}")
        if any(not 0 <= c <= 15 for c in t):
            raise ValueError(f"cell indices are 0 .. 15 (row-major), got {t!r}")
        if len(set(t)) != L:
            raise ValueError(f"a tuple's cells must be distinct, got {t!r}")
    return np.ascontiguousarray(np.array(rows, np.uint8).reshape(len(rows), L))


def _check_stage_tiles(stage_tiles):
    """-> None (unstaged) or the thresholds as a tuple of ints: 1 .. 7 log2 tile values in 1 .. 17, strictly ascending."""
    if stage_tiles is None:
        return None
    try:
        tiles = tuple(stage_tiles)
    except TypeError:
        raise ValueError(f"stage_tiles must be a sequence of log2 tile values, got {stage_tiles!r}") from None
    if not 1 <= len(tiles) <= MAX_STAGES - 1:
        raise ValueError(f"stage_tiles holds 1 .. {MAX_STAGES - 1} thresholds, got {len(tiles)}")
    for k in tiles:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_STAGE_TILE:
            raise ValueError(f"a stage threshold is an integer log2 tile value in 1 .. {MAX_STAGE_TILE}, got {k!r}")
    tiles = tuple(int(k) for k in tiles)
    if any(a >= b for a, b in zip(tiles, tiles[1:])):
        raise ValueError(f"stage_tiles must be strictly ascending, got {tiles!r}")
    return tiles


def _check_carousel_tiles(carousel_tiles, network):
    """-> None (no carousel) or the carousel's thresholds as a tuple of ints: ``"stages"`` is the network's ``stage_tiles``,
    anything else goes through the rules of ``stage_tiles``."""
    if carousel_tiles is None:
        return None
    if isinstance(carousel_tiles, str):
        if carousel_tiles != "stages":
            raise ValueError(f"carousel_tiles must be None, 'stages' or a sequence of log2 tile values, got {carousel_tiles!r}")
        if network.stage_tiles is None:
            raise ValueError("carousel_tiles='stages' needs a multi-stage network; give an unstaged one thresholds of its own")
        return network.stage_tiles
    try:
        return _check_stage_tiles(carousel_tiles)
    except ValueError as e:
        raise ValueError(str(e).replace("stage_tiles", "carousel_tiles")) from None


def default_horizon(lam: float) -> int:
    """The smallest h >= 1 with lam^h <= 0.1, capped at ``MAX_HORIZON``: 1 for lam = 0, 4 for lam = 0.5, 8 from lam = 0.75 up."""
    h = 1
    while h < MAX_HORIZON and lam ** h > 0.1:
        h += 1
    return h


def _check_lambda(lam, horizon):
    """-> (None, None) (off) or (lam as a float in [0, 1], horizon as an int in 1 .. 8); ``ValueError`` for anything else, also for a
    horizon without lam."""
    if lam is None:
        if horizon is not None:
            raise ValueError(f"horizon={horizon!r} needs lam: the delayed learner is on only when lam is given")
        return None, None
    if isinstance(lam, bool) or not isinstance(lam, (int, float, np.integer, np.floating)):
        raise ValueError(f"lam must be None or a number in [0, 1], got {lam!r}")
    lam = float(lam)
    if not (np.isfinite(lam) and 0.0 <= lam <= 1.0):
        raise ValueError(f"lam must be None or a number in [0, 1], got {lam!r}")
    if horizon is None:
        return lam, default_horizon(lam)
    if isinstance(horizon, bool) or not isinstance(horizon, (int, np.integer)) or not 1 <= int(horizon) <= MAX_HORIZON:
        raise ValueError(f"horizon must be None or an integer in 1 .. {MAX_HORIZON}, got {horizon!r}")
    return lam, int(horizon)


def _device(device) -> torch.device:
    return C.device() if device is None else torch.device(device)


class NTupleNetwork:
    """``weights`` i32 [m, 16^L] (zeros) over ``tuples``: m tuples (1 .. 8) of L distinct cells each (1 .. 6), fixed point with
    ``frac_bits`` fractional bits (0 .. 20; the default 12 resolves 2.4e-4 and holds +-524 288 per entry).  The default network,
    four 6-tuples, is 256 MB.  Bad settings raise ``ValueError`` before any device is touched.

    ``stage_tiles=(k_1 < ... < k_n)`` (log2 tile values in 1 .. 17, n in 1 .. 7) makes it a MULTI-STAGE network of ``stages`` = n + 1
    sets of tables, ``weights`` i32 [S, m, 16^L]: a board is looked up in stage #{i : its largest tile >= k_i} (the afterstate's own
    stage in ``scores``, each leaf's in ``expectimax``).  Stages are split off in order: ``active_stages`` = p (1 at the start) means
    that the kernels see the first p - 1 thresholds only, so boards at or above k_p are served, and learned, by stage p - 1's tables
    until ``promote()`` copies them into stage p (``weights[p] = weights[p - 1]``, ``active_stages = p + 1``): right after it every
    value, score and search result is what it was before, bit for bit.  Memory is S times the unstaged network's: the default
    tuples with ``stage_tiles=(11, 12, 13, 14)`` hold 1.34 GB of weights.  ``stage_tiles=None`` is the unstaged network, unchanged."""

    def __init__(self, tuples=DEFAULT_TUPLES, frac_bits: int = 12, device=None, stage_tiles=None):
        self.cells = _check_tuples(tuples)
        self.stage_tiles = _check_stage_tiles(stage_tiles)
        self.stages = 1 if self.stage_tiles is None else len(self.stage_tiles) + 1
        self._active = 1
        if not 0 <= int(frac_bits) <= MAX_FRAC_BITS:
            raise ValueError(f"frac_bits must be in 0 .. {MAX_FRAC_BITS}, got {frac_bits!r}")
        self.frac_bits = int(frac_bits)
        self.tuples = tuple(tuple(int(c) for c in t) for t in self.cells)
        self.m, self.L = self.cells.shape
        self.device = _device(device)
        shape = (self.m, 16 ** self.L) if self.stage_tiles is None else (self.stages, self.m, 16 ** self.L)
        self.weights = torch.zeros(shape, dtype=torch.int32, device=self.device)
        self._search_ws = None  # the two-ply workspace, allocated at the first two-ply call
        self._frontier_ws = None  # the frontier search's workspace, allocated at the first ``search`` call
        self._budget_ws = None  # the budgeted search's workspace, allocated at the first ``search_budget`` call

    @property
    def active_stages(self) -> int:
        """p in 1 .. ``stages``: the stages split off so far (always 1 for the unstaged network)."""
        return self._active

    @active_stages.setter
    def active_stages(self, p) -> None:
        if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not 1 <= int(p) <= self.stages:
            raise ValueError(f"active_stages must be an integer in 1 .. {self.stages}, got {p!r}")
        self._active = int(p)

    @property
    def active_tiles(self):
        """What the kernels are given: None for the unstaged network, else the first ``active_stages - 1`` thresholds (u8, host)."""
        if self.stage_tiles is None:
            return None
        return np.array(self.stage_tiles[:self._active - 1], np.uint8)

    def promote(self) -> int:
        """Split the next stage off: ``weights[p] = weights[p - 1]``, ``active_stages = p + 1`` -> the new ``active_stages``.
        ``ValueError`` at the top stage (and for the unstaged network, whose one stage is its top)."""
        p = self._active
        if p >= self.stages:
            raise ValueError(f"all {self.stages} stages are active: nothing to promote")
        self.weights[p].copy_(self.weights[p - 1])
        self._active = p + 1
        return self._active

    def stage_of(self, boards: torch.Tensor) -> torch.Tensor:
        """boards u8 [n, 16] -> u8 [n]: the stage whose tables a board is looked up in now (over the ACTIVE thresholds; plain torch,
        for logging)."""
        mx = boards.reshape(-1, 16).max(dim=1).values
        tiles = [] if self.stage_tiles is None else self.stage_tiles[:self._active - 1]
        out = torch.zeros(mx.shape, dtype=torch.uint8, device=boards.device)
        for k in tiles:
            out += (mx >= k).to(torch.uint8)
        return out

    def values(self, boards: torch.Tensor) -> torch.Tensor:
        """boards u8 [n, 16] -> V f32 [n]."""
        boards = boards.contiguous()
        out = torch.empty(boards.shape[0], dtype=torch.float32, device=boards.device)
        if out.numel():
            nv.ntuple_values(boards, self.weights, self.cells, self.frac_bits, out, self.active_tiles)
        return out

    def scores(self, boards: torch.Tensor):
        """boards u8 [B, 16] -> (q f32 [B, 4], v f32 [B]): q[a] = reward + V(afterstate) of a legal move and +0 of an illegal one,
        v = the max over the legal moves (0 if there is none)."""
        boards = boards.contiguous()
        B = boards.shape[0]
        q = torch.empty((B, 4), dtype=torch.float32, device=boards.device)
        v = torch.empty(B, dtype=torch.float32, device=boards.device)
        if B:
            nv.ntuple_scores(boards, self.weights, self.cells, self.frac_bits, q, v, self.active_tiles)
        return q, v

    def expectimax(self, boards: torch.Tensor, plies: int, gamma: float = 1.0):
        """boards u8 [B, 16] -> (q f32 [B, 4], v f32 [B]) of ``plies``-ply expectimax whose leaf is ``scores``' v (the network's
        greedy value), searched inside the kernel (``g2048_ntuple_expectimax``): one launch for one ply, two for two, nothing
        read back.  ``plies=0`` is ``scores``.  Two plies go in chunks of at most 2^16 roots through one cached 32 MB workspace."""
        plies, gamma = _check_search(plies, gamma)
        if plies == 0:
            return self.scores(boards)
        boards = boards.contiguous()
        B = boards.shape[0]
        q = torch.empty((B, 4), dtype=torch.float32, device=boards.device)
        v = torch.empty(B, dtype=torch.float32, device=boards.device)
        ws = None
        if plies == 2 and B:
            ws = self._search_ws
            if ws is None or ws.device != boards.device:
                ws = self._search_ws = torch.empty(SEARCH_CHUNK * 128, dtype=torch.float32, device=boards.device)
        step = SEARCH_CHUNK if plies == 2 else 1 << 24  # the entry point's own limit for one ply
        for s in range(0, B, step):
            e = min(B, s + step)
            nv.ntuple_expectimax(boards[s:e], self.weights, self.cells, self.frac_bits, plies, gamma, ws, q[s:e], v[s:e],
                                 self.active_tiles)
        return q, v

    def search(self, boards: torch.Tensor, depth: int, gamma: float = 1.0, dedup: bool = True, return_counts: bool = False):
        """boards u8 [B, 16] -> (q f32 [B, 4], v f32 [B]) of ``depth``-ply (1, 2 or 3) expectimax whose leaf is ``scores``' v, searched
        on packed lists of afterstates (``g2048_ntuple_search``); ``dedup`` merges the equal afterstates of one root at every level,
        which changes no output bit.  At depth 1 and 2 the outputs equal ``expectimax``'s bit for bit.  ``return_counts`` adds an int64
        [3] tensor: the entries of the three levels, summed over the chunks.  The roots go in chunks (``FRONTIER_CHUNK``: 256 at depth
        3) through one cached workspace sized for a chunk's worst case, 0.36 GB at depth 3; nothing is read back."""
        depth, gamma = _check_depth(depth, gamma)
        boards = boards.contiguous()
        B = boards.shape[0]
        q = torch.empty((B, 4), dtype=torch.float32, device=boards.device)
        v = torch.empty(B, dtype=torch.float32, device=boards.device)
        total = torch.zeros(3, dtype=torch.int64, device=boards.device) if return_counts else None
        step = FRONTIER_CHUNK[depth]
        if B:
            need = nv.ntuple_search_workspace_bytes(min(B, step), depth)
            ws = self._frontier_ws
            if ws is None or ws.device != boards.device or ws.numel() < need:
                ws = self._frontier_ws = None  # release the smaller one first
                ws = self._frontier_ws = torch.empty(nv.ntuple_search_workspace_bytes(step, depth), dtype=torch.uint8, device=boards.device)
            counts = torch.empty(3, dtype=torch.int32, device=boards.device) if return_counts else None
            for s in range(0, B, step):
                e = min(B, s + step)
                nv.ntuple_search(boards[s:e], self.weights, self.cells, self.frac_bits, depth, gamma, dedup, ws, q[s:e], v[s:e], counts,
                                 self.active_tiles)
                if return_counts:
                    total += counts
        return (q, v, total) if return_counts else (q, v)

    def search_budget(self, boards: torch.Tensor, max_depth: int = BUDGET_DEFAULT_DEPTH, budget: int = BUDGET_DEFAULT, gamma: float = 1.0,
                      return_depths: bool = False):
        """boards u8 [B, 16] -> (q f32 [B, 4], v f32 [B]) of expectimax whose leaf is ``scores``' v, every root searched as deep as its
        frontier fits (``g2048_ntuple_budget_search``): to d = the largest depth in 1 .. ``max_depth`` (at most 6) up to which every
        level of the root holds at most ``budget`` (4 .. 24 576) distinct afterstates.  A root's row equals ``search(root, depth=d)``
        bit for bit wherever that exists (d <= 3).  ``return_depths`` adds ``depth_used`` u8 [B] = d and ``entries`` i32 [B, 6] = the
        distinct afterstates of the levels 1 .. d, 0 beyond.  The roots go in chunks (``budget_chunk``) through one cached workspace
        of at most ``BUDGET_WORKSPACE_BYTES``; nothing is read back."""
        max_depth, budget, gamma = _check_budget(max_depth, budget, gamma)
        boards = boards.contiguous()
        B, dev = boards.shape[0], boards.device
        q = torch.empty((B, 4), dtype=torch.float32, device=dev)
        v = torch.empty(B, dtype=torch.float32, device=dev)
        used = torch.empty(B, dtype=torch.uint8, device=dev) if return_depths else None
        entries = torch.empty((B, 6), dtype=torch.int32, device=dev) if return_depths else None
        if B:
            step = budget_chunk(max_depth, budget)
            need = nv.ntuple_budget_search_workspace_bytes(min(B, step), max_depth, budget)
            ws = self._budget_ws
            if ws is None or ws.device != dev or ws.numel() < need:
                ws = self._budget_ws = None  # release the smaller one first
                ws = self._budget_ws = torch.empty(need, dtype=torch.uint8, device=dev)
            for s in range(0, B, step):
                e = min(B, s + step)
                nv.ntuple_budget_search(boards[s:e], self.weights, self.cells, self.frac_bits, max_depth, budget, gamma, ws, q[s:e], v[s:e],
                                        None if used is None else used[s:e], None if entries is None else entries[s:e], self.active_tiles)
        return (q, v, used, entries) if return_depths else (q, v)

    def play_episodes(self, num_episodes: int, seed: int = 42, batch_size: int = 100, rng_mode=None, steps_per_launch: int = 2048,
                      max_steps: int = 1 << 20):
        """``num_episodes`` greedy games, each to its end, inside the persistent kernel (``g2048_ntuple_episodes``) ->
        (final_boards u8 [N, 16], ep_len i32 [N], score i64 [N]) as device tensors.  The games are those of the evaluation protocol:
        batch j holds games ``j * batch_size ..``, is as large as the games it holds and starts its key chain at
        ``seed_key(seed + j * batch_size)``, so game g of batch j is env g of ``BatchRunner(seed + j * batch_size,
        NTupleActionFunction(self)).collect(B_j)``, bit for bit.  All batches play at once; a launch plays ``steps_per_launch`` steps
        (at most 65 536) and the host reads four bytes back per launch.  ``RuntimeError`` past ``max_steps``; ``ValueError`` for a
        non-positive episode count, batch size or ``steps_per_launch``, before a device is touched."""
        return self._episodes(num_episodes, seed, batch_size, rng_mode, steps_per_launch, max_steps, 0, 1.0)

    def play_search_episodes(self, num_episodes: int, seed: int = 42, batch_size: int = 100, rng_mode=None, steps_per_launch=None,
                             max_steps: int = 1 << 20, *, plies: int = 0, gamma: float = 1.0):
        """``play_episodes`` with the search depth as an argument: ``plies=0`` is ``play_episodes`` itself (its launches, its default of
        2 048 steps per launch); ``plies=1`` plays every move by one ply of expectimax at discount ``gamma``
        (``g2048_ntuple_search_episodes``, one wavefront per game), so game g of batch j is env g of ``BatchRunner(seed + j *
        batch_size, NTupleActionFunction(self, plies=1, gamma=gamma)).collect(B_j)``, bit for bit.  ``ValueError`` before a device is
        touched for any other ``plies`` (``True`` and 2 included: two plies stay on the lock-step path) and for a gamma that is
        negative or not finite.  ``steps_per_launch=None`` takes the depth's default, ``SEARCH_EPISODE_STEPS`` for one ply."""
        plies, gamma = _check_search(plies, gamma)
        if plies == 2:
            raise ValueError("play_search_episodes: plies must be 0 or 1, got 2 (two plies play on the lock-step path)")
        if steps_per_launch is None:
            steps_per_launch = SEARCH_EPISODE_STEPS if plies else 2048
        return self._episodes(num_episodes, seed, batch_size, rng_mode, steps_per_launch, max_steps, plies, gamma)

    def _episodes(self, num_episodes, seed, batch_size, rng_mode, steps_per_launch, max_steps, plies: int, gamma: float):
        """``play_episodes`` (``plies == 0``) and ``play_search_episodes`` (``plies == 1``): the same checks, state and launch loop."""
        for name, x in (("num_episodes", num_episodes), ("batch_size", batch_size), ("steps_per_launch", steps_per_launch)):
            if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or int(x) <= 0:
                raise ValueError(f"{name} must be a positive integer, got {x!r}")
        N, bs, n_steps = int(num_episodes), int(batch_size), min(int(steps_per_launch), 65536)
        mode = C.resolve_rng_mode(rng_mode)
        dev = self.weights.device
        heads = np.stack([seed_key(int(seed) + first) for first in range(0, N, bs)])  # one key per batch ...
        chain = nv.keys_from_numpy(np.repeat(heads, bs, axis=0)[:N], dev)             # ... expanded to the games
        boards = torch.empty((N, 16), dtype=torch.uint8, device=dev)
        masks, done = torch.empty(N, dtype=torch.uint8, device=dev), torch.empty(N, dtype=torch.uint8, device=dev)
        ep_len = torch.empty(N, dtype=torch.int32, device=dev)
        score = torch.empty(N, dtype=torch.int64, device=dev)
        live = torch.zeros(1, dtype=torch.int32, device=dev)
        t = 0
        while True:
            live.zero_()
            if plies:
                nv.ntuple_search_episodes(t == 0, n_steps, bs, self.weights, self.cells, self.frac_bits, plies, gamma, chain, boards,
                                          masks, done, ep_len, score, mode, live, self.active_tiles)
            else:
                nv.ntuple_episodes(t == 0, n_steps, bs, self.weights, self.cells, self.frac_bits, chain, boards, masks, done, ep_len,
                                   score, mode, live, self.active_tiles)
            t += n_steps
            if int(live.item()) == 0:
                break
            if t >= max_steps:
                raise RuntimeError("play_episodes exceeded max_steps")
        return boards, ep_len, score

    def save(self, path: str) -> None:
        torch.save({"weights": self.weights.cpu(), "tuples": self.tuples, "frac_bits": self.frac_bits,
                    "stage_tiles": self.stage_tiles, "active_stages": self._active}, path)

    @classmethod
    def load(cls, path: str, device=None) -> "NTupleNetwork":
        """A file written before the network had stages (no ``stage_tiles`` key) loads as an unstaged network."""
        d = torch.load(path, map_location="cpu")
        net = cls(d["tuples"], d["frac_bits"], device=device, stage_tiles=d.get("stage_tiles"))
        if tuple(d["weights"].shape) != tuple(net.weights.shape) or d["weights"].dtype != torch.int32:
            raise ValueError(f"{path}: weights of shape {tuple(d['weights'].shape)} do not fit tuples {net.tuples} "
                             f"and stage_tiles {net.stage_tiles}")
        net.active_stages = d.get("active_stages", 1)
        net.weights.copy_(d["weights"])
        return net


class NTupleActionFunction(QPlayer):
    """``act_fn`` plug-in for ``BatchRunner`` whose "logits" are the n-tuple network's afterstate scores.

    ``policy_fn(boards, masks)`` returns ``(q f32 [B, 4], v f32 [B])`` of ``NTupleNetwork.scores``.  ``use_mask=True,
    sample_actions=False`` are forced (``QPlayer``), so the engine (``g2048_policy_step``) takes the masked argmax of ``q``; the env,
    its key stream and the trajectory format are untouched.  The recorded ``log_prob`` is the log-softmax of scores at the chosen action:
    NOT a policy probability (``q`` is in score units), so such trajectories are for evaluation only, not for a PPO update.
    ``rng_mode``: anything ``resolve_rng_mode`` takes; an unknown spelling raises ``ValueError`` (it used to mean "partitionable").
    ``plies`` (0, 1 or 2) puts that many plies of expectimax over every spawn in front of the greedy value
    (``NTupleNetwork.expectimax``; 0, the default, is ``scores`` itself), discounted by ``gamma`` per ply (1.0: the TD(0) learner is
    undiscounted); anything else raises ``ValueError`` before a device is touched.
    """

    compact = True

    def __init__(self, network: NTupleNetwork, device=None, rng_mode=None, *, plies: int = 0, gamma: float = 1.0):
        if not isinstance(network, NTupleNetwork):
            raise ValueError(f"network must be an NTupleNetwork, got {type(network).__name__}")
        self.plies, self.gamma = _check_search(plies, gamma)
        self.network = network
        self.device = device
        self.rng_mode = rng_mode

    @torch.no_grad()
    def policy_fn(self, boards: torch.Tensor, masks: torch.Tensor = None):
        """boards u8 [B, 16], masks unused (legality is ``afterstate != board``) -> (q f32 [B, 4], v f32 [B])."""
        return self.network.expectimax(boards, self.plies, self.gamma)

    policy_fn.needs_masks = False


class NTupleSearchActionFunction(QPlayer):
    """``act_fn`` plug-in for ``BatchRunner`` whose "logits" are ``NTupleNetwork.search``'s: ``depth`` plies (1, 2 or 3) of
    expectimax over the n-tuple network on packed, deduplicated lists of afterstates, discounted by ``gamma`` per ply.  Everything
    else is ``NTupleActionFunction``'s: the engine takes the masked argmax, the recorded ``log_prob`` is no policy probability.  A
    depth that is a bool, not an integer or outside 1 .. 3, or a bad gamma, raises ``ValueError`` before a device is touched."""

    compact = True

    def __init__(self, network: NTupleNetwork, device=None, rng_mode=None, *, depth: int = 1, gamma: float = 1.0, dedup: bool = True):
        if not isinstance(network, NTupleNetwork):
            raise ValueError(f"network must be an NTupleNetwork, got {type(network).__name__}")
        self.depth, self.gamma = _check_depth(depth, gamma)
        self.dedup = bool(dedup)
        self.network = network
        self.device = device
        self.rng_mode = rng_mode

    @torch.no_grad()
    def policy_fn(self, boards: torch.Tensor, masks: torch.Tensor = None):
        """boards u8 [B, 16], masks unused (legality is ``afterstate != board``) -> (q f32 [B, 4], v f32 [B])."""
        return self.network.search(boards, self.depth, self.gamma, self.dedup)

    policy_fn.needs_masks = False


class NTupleBudgetSearchActionFunction(QPlayer):
    """``act_fn`` plug-in for ``BatchRunner`` whose "logits" are ``NTupleNetwork.search_budget``'s: expectimax over the n-tuple network
    on packed, deduplicated lists of afterstates, every board searched as deep (1 .. ``max_depth``) as its levels stay within
    ``budget`` distinct afterstates, discounted by ``gamma`` per ply.  Everything else is ``NTupleActionFunction``'s: the engine takes
    the masked argmax, the recorded ``log_prob`` is no policy probability.  A ``max_depth`` or ``budget`` that is a bool, not an
    integer or out of range (1 .. 6, 4 .. 24 576), or a bad gamma, raises ``ValueError`` before a device is touched."""

    compact = True

    def __init__(self, network: NTupleNetwork, device=None, rng_mode=None, *, max_depth: int = BUDGET_DEFAULT_DEPTH,
                 budget: int = BUDGET_DEFAULT, gamma: float = 1.0):
        if not isinstance(network, NTupleNetwork):
            raise ValueError(f"network must be an NTupleNetwork, got {type(network).__name__}")
        self.max_depth, self.budget, self.gamma = _check_budget(max_depth, budget, gamma)
        self.network = network
        self.device = device
        self.rng_mode = rng_mode

    @torch.no_grad()
    def policy_fn(self, boards: torch.Tensor, masks: torch.Tensor = None):
        """boards u8 [B, 16], masks unused (legality is ``afterstate != board``) -> (q f32 [B, 4], v f32 [B])."""
        return self.network.search_budget(boards, self.max_depth, self.budget, self.gamma)

    policy_fn.needs_masks = False


class NTupleTrainer:
    """TD(0) on afterstates over ``num_envs`` always-live boards, greedy in the network being learned.

    One lock-step is five launches on the ambient stream: scores of the current boards (their max is the TD target of the
    previous afterstate) -> ``td_accumulate`` -> ``td_apply`` -> the engine's auto-reset step on the masked argmax of the scores
    (``use_mask=1, sample=0``, a one-row trajectory) -> ``link``, which replays the recorded move to get the new afterstate and
    reads the done bit.  The key chain advances as in ``RolloutEngine.rollout_policy_fixed``: the init split at the first call,
    then two sub-keys per lock-step.  Nothing is read back inside the loop; env state and learner state persist across calls.

    ``learner="tc"`` replaces the middle pair by ``tc_accumulate`` -> ``tc_apply`` (temporal-coherence learning): every table entry
    moves by its mean delta times its own rate ``|coh_e| / coh_a``, the sum of its past updates over the sum of their magnitudes
    (rate 1 while ``coh_a == 0``), all in integer arithmetic, so a run stays reproducible bit for bit.  ``alpha`` keeps its default
    of 0.1, but TC is meant to run at ``alpha=1.0``: the rates take the step size down where updates disagree.  It adds ``abs_acc``
    (i64), ``coh_e`` and ``coh_a`` (i32) to ``acc`` and ``cnt``: at the default network the trainer then holds about 2.3 GB of tables
    (weights 0.27, acc and abs_acc 0.54 each, cnt, coh_e and coh_a 0.27 each) where ``"td0"`` holds 1.07 GB.  Anything but ``"td0"``
    or ``"tc"`` raises ``ValueError`` before a device is touched.

    On a multi-stage network every learner table takes the weights' shape [S, m, 16^L], so the table memory is S times the figures
    above, per stage 1.07 GB for ``"td0"`` and 2.3 GB for ``"tc"`` at the default tuples: about 11.5 GB for TC at S = 5.  The
    kernels get the network's active thresholds, and the trainer promotes: before a lock-step whose global count (``lock_steps``)
    is a positive multiple of ``promote_every`` it reads ``prev_after.max()`` (one torch reduction and one host read, the only one
    the loop has, and only while a stage is left to split off) and calls ``network.promote()`` while that maximum is at or above
    the next threshold, several times at one check if need be.  ``promote_every=0`` never promotes.  A new stage's ``coh_e`` /
    ``coh_a`` stay zero (rate 1).  ``promotions`` lists ``(lock_steps, new active_stages)``.  The count is global, so
    ``train(48)`` and ``train(20); train(28)`` give the same bits.

    ``carousel_tiles`` turns carousel shaping on (Jaskowski 2017): episodes no longer all start from an empty board but go round
    the stages of the game, so tables for late boards get as many episode starts as those for early ones.  ``None`` (the default)
    is off: nothing is allocated and the launches are the five above.  ``"stages"`` takes the network's ``stage_tiles`` (a
    ``ValueError`` on an unstaged network); a sequence gives the carousel thresholds of its own, under the rules of
    ``stage_tiles``, on any network.  All of them are always in use, whatever ``active_stages`` is.  With n thresholds a lock-step
    gets two more launches after ``link``: ``carousel_record`` puts the board of an env whose episode has entered carousel stage
    s (the number of thresholds at or below its largest tile) into the env's slot of ``pool_boards`` u8 [n, B, 16] /
    ``pool_masks`` u8 [n, B] (a slot is empty while its mask is 0; ``reached`` u8 [B] is the highest stage recorded in the
    running episode), and ``carousel_restart`` sends an env whose episode has just ended to stage c = (b + ``turn[b]``) mod
    (n + 1) (``turn`` i32 [B], the bits of a u32 count of the env's restarts): c = 0 keeps the engine's fresh board, c >= 1 takes
    the board in slot (c - 1, j) of a donor env j drawn from the lock-step's act sub-key (which the greedy step does not use),
    and falls back to the fresh board if that slot is empty.  ``starts`` i64 [n + 1] counts the episode starts per stage, the
    fallbacks under 0.  The learner is untouched: an ended episode's last update has target 0, and the first ``link`` after a
    restart takes the afterstate of the move played on the pool board.  The key chain advances as without the carousel.  The
    pools, ``reached``, ``turn`` and ``starts`` are env state: they are not in ``state_dict()`` and start afresh on resume.

    ``lam`` turns delayed TD(lambda) / TC(lambda) on (Jaskowski 2017), for either learner: multi-step credit assignment without
    eligibility traces.  ``None`` (the default) is off: nothing is allocated and the launches and every bit of a run stay as they
    are.  With ``lam`` in [0, 1] every env keeps a ring of its last ``horizon`` = h afterstates and of their TD errors (``hist`` u8
    [h, B, 16], ``hist_err`` f32 [h, B], ``hist_len`` u8 [B]; 1 .. 8, by default the smallest h with lam^h <= 0.1 capped at 8: 1 for
    lam = 0, 4 for lam = 0.5), and the middle pair and ``link`` become ``delayed_accumulate`` -> ``delayed_apply`` and
    ``delayed_link``, the same number of launches.  An afterstate is still updated exactly once, h - 1 lock-steps after it was
    reached, by e_0 + lam e_1 + ... + lam^(h-1) e_(h-1), the errors of the h transitions since (a Horner sum of individually
    rounded f32 operations; everything after it is the integer arithmetic of the learner), so the atomic volume per lock-step is
    TD(0)'s and a run stays reproducible bit for bit.  At an episode's end the states still in the ring are flushed with the
    shorter sums they have.  ``horizon=1`` is the plain learner bit for bit for any ``lam``; ``lam=0`` with h > 1 is TD(0) applied
    h - 1 steps late.  The ring position is ``lock_steps`` mod h, a global count, so ``train(48)`` equals ``train(20); train(28)``.
    ``prev_after`` stays valid (promotion and the carousel read it), and both work unchanged on top.  ``horizon`` without ``lam``,
    values out of range and bools raise ``ValueError`` before a device is touched.  The ring is env state: it is not in
    ``state_dict()`` (which carries ``lam`` and ``horizon``) and starts afresh on resume.
    """

    LEARNERS = ("td0", "tc")

    def __init__(self, network: NTupleNetwork, num_envs: int, alpha: float = 0.1, seed: int = 0, rng_mode=None, device=None,
                 learner: str = "td0", promote_every: int = 64, carousel_tiles=None, lam=None, horizon=None):
        if learner not in self.LEARNERS:
            raise ValueError(f"learner must be one of {self.LEARNERS}, got {learner!r}")
        self.lam, self.horizon = _check_lambda(lam, horizon)
        if isinstance(promote_every, bool) or not isinstance(promote_every, (int, np.integer)) or promote_every < 0:
            raise ValueError(f"promote_every must be a non-negative integer (0: never promote), got {promote_every!r}")
        if not isinstance(network, NTupleNetwork):
            raise ValueError(f"network must be an NTupleNetwork, got {type(network).__name__}")
        if int(num_envs) < 1:
            raise ValueError(f"num_envs must be positive, got {num_envs!r}")
        if not (float(alpha) > 0.0 and np.isfinite(float(alpha))):
            raise ValueError(f"alpha must be a finite positive number, got {alpha!r}")
        self.carousel_tiles = _check_carousel_tiles(carousel_tiles, network)
        self.network = network
        self.num_envs = B = int(num_envs)
        self.alpha = float(alpha)
        self.rng_mode = C.resolve_rng_mode(rng_mode)
        self.device = dev = network.device if device is None else torch.device(device)
        if dev != network.weights.device:
            raise ValueError(f"the trainer's device {dev} is not the network's {network.weights.device}")
        self.key = seed_key(int(seed))
        u8, f32 = torch.uint8, torch.float32
        self.acc = torch.zeros(network.weights.shape, dtype=torch.int64, device=dev)
        self.cnt = torch.zeros(network.weights.shape, dtype=torch.int32, device=dev)
        self.learner = learner
        self.abs_acc = self.coh_e = self.coh_a = None
        if learner == "tc":
            self.abs_acc = torch.zeros(network.weights.shape, dtype=torch.int64, device=dev)
            self.coh_e = torch.zeros(network.weights.shape, dtype=torch.int32, device=dev)
            self.coh_a = torch.zeros(network.weights.shape, dtype=torch.int32, device=dev)
        self.prev_after = torch.zeros((B, 16), dtype=u8, device=dev)
        self.flag = torch.zeros(B, dtype=u8, device=dev)
        self.boards = torch.empty((B, 16), dtype=u8, device=dev)
        self.masks = torch.empty(B, dtype=u8, device=dev)
        self.ep_len = torch.empty(B, dtype=torch.int32, device=dev)
        self._done = torch.empty(B, dtype=u8, device=dev)
        self.scores = torch.empty((B, 4), dtype=f32, device=dev)
        self.targets = torch.empty(B, dtype=f32, device=dev)
        self.td_error = torch.empty(B, dtype=f32, device=dev)
        self._tr = dict(boards=torch.empty((1, B, 16), dtype=u8, device=dev), meta=torch.empty((1, B), dtype=u8, device=dev),
                        rewards=torch.empty((1, B), dtype=f32, device=dev), logp=torch.empty((1, B), dtype=f32, device=dev),
                        values=torch.empty((1, B), dtype=f32, device=dev))
        self._started = False
        self.lock_steps = 0
        self.promote_every = int(promote_every)
        self.promotions = []
        self.pool_boards = self.pool_masks = self.reached = self.turn = self.starts = None
        if self.carousel_tiles is not None:
            n = len(self.carousel_tiles)
            self._carousel = np.array(self.carousel_tiles, np.uint8)
            self.pool_boards = torch.zeros((n, B, 16), dtype=u8, device=dev)
            self.pool_masks = torch.zeros((n, B), dtype=u8, device=dev)
            self.reached = torch.zeros(B, dtype=u8, device=dev)
            self.turn = torch.zeros(B, dtype=nv.KEY_DTYPE, device=dev)  # u32 counts, carried as i32 like the keys
            self.starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        self.hist = self.hist_err = self.hist_len = None
        if self.lam is not None:
            self.hist = torch.zeros((self.horizon, B, 16), dtype=u8, device=dev)
            self.hist_err = torch.zeros((self.horizon, B), dtype=f32, device=dev)
            self.hist_len = torch.zeros(B, dtype=u8, device=dev)

    def _learn_delayed(self, count: int, st) -> None:
        """The middle pair of lock-step ``count`` with ``lam`` on: the newest afterstate is in ring slot (count - 1) mod h."""
        net, head = self.network, (count - 1) % self.horizon
        nv.ntuple_delayed_accumulate(self.hist, self.hist_err, self.hist_len, self.flag, self.targets, head, self.lam, net.weights,
                                     net.cells, net.frac_bits, self.alpha, self.acc, self.abs_acc, self.cnt, self.td_error, st)
        nv.ntuple_delayed_apply(self.hist, self.hist_len, self.flag, head, net.cells, net.weights, self.acc, self.abs_acc, self.cnt,
                                self.coh_e, self.coh_a, st)

    def _promote_if_reached(self, count: int) -> None:
        """The promotion check in front of lock-step ``count`` (see the class docstring)."""
        net = self.network
        if not self.promote_every or count == 0 or count % self.promote_every or net.active_stages >= net.stages:
            return
        top = int(self.prev_after.max().item())
        while net.active_stages < net.stages and top >= net.stage_tiles[net.active_stages - 1]:
            self.promotions.append((count, net.promote()))

    @torch.no_grad()
    def train(self, lock_steps: int, record: bool = False):
        """``lock_steps`` lock-steps -> {"episodes": i64 [], "td_sq_sum": f64 []} (device tensors: episodes finished, sum of
        td_error^2).  ``record=True`` adds per-step copies "boards" u8 [T, B, 16] (before the step), "meta" u8 [T, B], "scores"
        f32 [T, B, 4] and "targets" f32 [T, B]: for replaying a run in a test, not for training.  With the carousel on it also adds
        "start_stage" u8 [T, B]: the stage at which an env restarted after the step (0: a fresh board), 0xFF where it did not."""
        T, B, net, tr = int(lock_steps), self.num_envs, self.network, self._tr
        if T < 1:
            raise ValueError(f"lock_steps must be positive, got {lock_steps!r}")
        if not self._started:
            self.key, sub = nv.chain_keys(self.key, 1, self.rng_mode)
            nv.reset_fused(sub[0], self.boards, self.masks, self._done, self.ep_len, B, 0, self.rng_mode)
            self._started = True
        self.key, subs = nv.chain_keys(self.key, 2 * T, self.rng_mode)
        episodes = torch.zeros((), dtype=torch.int64, device=self.device)
        td_sq = torch.zeros((), dtype=torch.float64, device=self.device)
        rec = None
        if record:
            rec = dict(boards=torch.empty((T, B, 16), dtype=torch.uint8, device=self.device),
                       meta=torch.empty((T, B), dtype=torch.uint8, device=self.device),
                       scores=torch.empty((T, B, 4), dtype=torch.float32, device=self.device),
                       targets=torch.empty((T, B), dtype=torch.float32, device=self.device))
            if self.carousel_tiles is not None:
                rec["start_stage"] = torch.empty((T, B), dtype=torch.uint8, device=self.device)
        for t in range(T):
            self._promote_if_reached(self.lock_steps + t)
            st = net.active_tiles
            nv.ntuple_scores(self.boards, net.weights, net.cells, net.frac_bits, self.scores, self.targets, st)
            if self.lam is not None:
                self._learn_delayed(self.lock_steps + t, st)
            elif self.learner == "tc":
                nv.ntuple_tc_accumulate(self.prev_after, self.flag, self.targets, net.weights, net.cells, net.frac_bits, self.alpha,
                                        self.acc, self.abs_acc, self.cnt, self.td_error, st)
                nv.ntuple_tc_apply(self.prev_after, self.flag, net.cells, net.weights, self.acc, self.abs_acc, self.cnt, self.coh_e,
                                   self.coh_a, st)
            else:
                nv.ntuple_td_accumulate(self.prev_after, self.flag, self.targets, net.weights, net.cells, net.frac_bits, self.alpha,
                                        self.acc, self.cnt, self.td_error, st)
                nv.ntuple_td_apply(self.prev_after, self.flag, net.cells, net.weights, self.acc, self.cnt, st)
            nv.policy_step_autoreset(subs[2 * t], subs[2 * t + 1], self.scores, self.targets, True, False, 0, self.boards, self.masks,
                                     self.ep_len, tr["boards"], tr["meta"], tr["rewards"], tr["logp"], tr["values"], B, 0,
                                     self.rng_mode)
            if self.lam is not None:
                nv.ntuple_delayed_link(tr["boards"][0], tr["meta"][0], (self.lock_steps + t) % self.horizon, self.prev_after, self.flag,
                                       self.hist, self.hist_len)
            else:
                nv.ntuple_link(tr["boards"][0], tr["meta"][0], self.prev_after, self.flag)
            if self.carousel_tiles is not None:
                nv.ntuple_carousel_record(self.boards, self.masks, self.flag, self._carousel, self.reached, self.pool_boards,
                                          self.pool_masks)
                nv.ntuple_carousel_restart(subs[2 * t], self.flag, self.pool_boards, self.pool_masks, self.boards, self.masks,
                                           self.reached, self.turn, self.starts, self.rng_mode,
                                           None if rec is None else rec["start_stage"][t])
            episodes += (self.flag == 2).sum()
            td_sq += self.td_error.double().square().sum()
            if rec is not None:
                rec["boards"][t].copy_(tr["boards"][0])
                rec["meta"][t].copy_(tr["meta"][0])
                rec["scores"][t].copy_(self.scores)
                rec["targets"][t].copy_(self.targets)
        self.lock_steps += T
        out = {"episodes": episodes, "td_sq_sum": td_sq}
        if rec is not None:
            out.update(rec)
        return out

    def state_dict(self) -> dict:
        """The learner's own state (host tensors): ``learner``, ``alpha``, ``lock_steps`` and, for ``"tc"``, ``coh_e`` / ``coh_a``, so
        that a resumed run keeps its rates.  The weights are the network's (``NTupleNetwork.save``); the envs start afresh.  On a
        multi-stage network also ``stages`` and ``promotions``; with the carousel on also ``carousel_tiles`` (the thresholds only:
        the pools are env state and start afresh on resume); with the delayed learner on also ``lam`` and ``horizon`` (the ring is
        env state too)."""
        out = {"learner": self.learner, "alpha": self.alpha, "lock_steps": self.lock_steps}
        if self.network.stage_tiles is not None:
            out.update(stages=self.network.stages, promotions=list(self.promotions))
        if self.carousel_tiles is not None:
            out.update(carousel_tiles=tuple(self.carousel_tiles))
        if self.lam is not None:
            out.update(lam=self.lam, horizon=self.horizon)
        if self.learner == "tc":
            out.update(coh_e=self.coh_e.cpu().clone(), coh_a=self.coh_a.cpu().clone())
        return out

    def load_state_dict(self, state: dict) -> None:
        """``ValueError`` for another learner's state, another stage count's, other carousel thresholds (none counts as other), another
        ``lam`` / ``horizon`` (none counts as other), or tables of another shape or dtype; nothing is changed then."""
        if state.get("learner") != self.learner:
            raise ValueError(f"the state is of learner {state.get('learner')!r}, the trainer's is {self.learner!r}")
        theirs = state.get("carousel_tiles")
        if (None if theirs is None else tuple(int(k) for k in theirs)) != self.carousel_tiles:
            raise ValueError(f"the state is of carousel thresholds {theirs!r}, the trainer's are {self.carousel_tiles!r}")
        if (state.get("lam"), state.get("horizon")) != (self.lam, self.horizon):
            raise ValueError(f"the state is of lam {state.get('lam')!r} and horizon {state.get('horizon')!r}, the trainer's are "
                             f"{self.lam!r} and {self.horizon!r}")
        if state.get("stages", 1) != self.network.stages:
            raise ValueError(f"the state is of a network of {state.get('stages', 1)} stages, the trainer's has {self.network.stages}")
        tables = {}
        if self.learner == "tc":
            for k in ("coh_e", "coh_a"):
                t = state.get(k)
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(self.coh_e.shape) or t.dtype != torch.int32:
                    raise ValueError(f"{k} of shape {None if t is None else tuple(t.shape)} does not fit tuples {self.network.tuples}")
                tables[k] = t
        alpha = float(state["alpha"])
        if not (alpha > 0.0 and np.isfinite(alpha)):
            raise ValueError(f"alpha must be a finite positive number, got {state['alpha']!r}")
        self.alpha, self.lock_steps = alpha, int(state["lock_steps"])
        self.promotions = [(int(a), int(b)) for a, b in state.get("promotions", [])]
        for k, t in tables.items():
            getattr(self, k).copy_(t)

    @torch.no_grad()
    def coherence(self) -> dict:
        """``learner="tc"`` -> {"entries": i64 [] entries with coh_a > 0, "mean_rate": f64 [] mean of |coh_e| / coh_a over them (0 if
        there is none)} as device tensors.  Torch reductions over the whole tables: for logging between chunks, not inside the loop."""
        if self.learner != "tc":
            raise ValueError(f"coherence() is of learner 'tc', the trainer's is {self.learner!r}")
        entries = (self.coh_a > 0).sum()
        rate = self.coh_e.abs().double() / self.coh_a.clamp(min=1).double()  # |coh_e| <= coh_a: 0 where coh_a == 0
        return {"entries": entries, "mean_rate": rate.sum() / entries.clamp(min=1).double()}
