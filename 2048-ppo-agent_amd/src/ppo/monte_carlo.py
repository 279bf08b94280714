"""Monte-Carlo playout play on the rollout engine, with an optional critic bootstrap (no reference counterpart).

    Q(s, a) = mean over R playouts of [ sum_t gamma^t r_t  (+ gamma^d V(leaf) where the playout was cut off alive) ]

For every root board and every legal move, R playouts of a cheap policy (uniformly random legal moves, or DRUL) start from the
afterstate; the move with the best mean return is played.  The playouts run in ``g2048_mc_playout``: one lane per playout, lane
``(4 b + a) R + r``, the board in registers across a launch of up to 128 steps, no trajectory written; ``g2048_mc_reduce`` sums
each pair's R lanes in ascending order.  Without an agent no network is touched; with one, the playouts are cut off after
``depth`` steps and the agent's critic values the leaves (``4 R`` value-forward rows per board).  How the scores become moves
(the un-batched ``__call__``, the rng mode, the masked max) is ``QPlayer``'s (``q_player.py``).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..g2048 import native as nv
from ..g2048.engine import seed_key
from .q_player import QPlayer
from .torch_action_wrapper import resolve_symmetry

PLAYOUT_POLICIES = {"random": "POLICY_RANDOM", "drul": "POLICY_DRUL"}


class MonteCarloActionFunction(QPlayer):
    """``act_fn`` plug-in for ``BatchRunner`` whose "logits" are Monte-Carlo estimates ``Q(s, .)`` of the playout returns.

    ``policy_fn(boards, masks)`` returns ``(q f32 [B, 4], v f32 [B])`` with ``v = max over the legal actions of q`` (0 where
    there is none; ``q`` of an illegal action is +0).  ``use_mask=True, sample_actions=False`` are forced (``QPlayer``), so the
    engine (``g2048_policy_step``) takes the masked argmax of ``q``; the env, its key stream and the trajectory format are untouched.
    The recorded ``log_prob`` is therefore the log-softmax of scores at the chosen action: NOT a policy probability (``q`` is in
    score units), so such trajectories are for evaluation only, not for a PPO update.

    ``playouts``: R per (board, action) pair, 1 .. 1024.  ``playout_policy``: "random" (act_randomly) or "drul".  ``depth``: steps
    per playout, the root move included; ``None`` plays until every lane has terminated (launches of at most 128 steps, the live
    counter read once per launch; more than ``max_steps`` steps raise ``RuntimeError``); ``depth=d`` runs ``ceil(d / 128)`` launches
    and reads nothing back.  ``gamma``: discount, default 0.99 with an agent and 1.0 without.  ``agent``: its critic values the leaf
    boards (the value forward of ``LookaheadActionFunction.values``, in chunks of ``max_children`` rows, ``symmetry`` and
    ``amp_dtype`` as there); ``None``: plain playout returns.  ``rng_mode``: anything ``resolve_rng_mode`` takes; an unknown
    spelling raises ``ValueError`` at the first call (it used to mean "partitionable").
    The playout keys are a chain of their own, seeded by ``seed`` and advanced by two sub-keys per playout step
    (``g2048_chain_keys``): independent of the env's stream, deterministic in ``seed`` and the sequence of calls.  The roots of a
    call are cut into slices of whole boards with ``4 R B_slice <= max_lanes``; every slice draws the keys of the uncut call, so
    ``q`` does not depend on ``max_lanes``.  ``last_steps`` / ``last_lanes``: playout steps launched (per lane) and lanes of the
    latest call.
    """

    compact = True

    def __init__(self, agent=None, playouts: int = 32, depth: Optional[int] = None, playout_policy: str = "random",
                 gamma: Optional[float] = None, seed: int = 0, max_lanes: int = 1 << 22, device=None, rng_mode=None,
                 sync_every: int = 8, symmetry: Optional[str] = None, max_steps: int = 4096, amp_dtype: Optional[torch.dtype] = None,
                 use_fused: Optional[bool] = None, max_children: int = 1 << 18):
        if not 1 <= int(playouts) <= 1024:
            raise ValueError(f"playouts must be in 1 .. 1024, got {playouts!r}")
        if playout_policy not in PLAYOUT_POLICIES:
            raise ValueError(f"playout_policy must be one of {tuple(PLAYOUT_POLICIES)}, got {playout_policy!r}")
        if depth is not None and int(depth) < 1:
            raise ValueError(f"depth must be a positive number of steps or None (play to the end), got {depth!r}")
        if gamma is None:
            gamma = 0.99 if agent is not None else 1.0
        if not 0.0 < float(gamma) <= 1.0:
            raise ValueError(f"gamma must be in (0, 1], got {gamma!r}")
        if int(max_lanes) < 4 * int(playouts):
            raise ValueError(f"max_lanes must hold the 4 * playouts = {4 * int(playouts)} lanes of one board, got {max_lanes!r}")
        if int(max_steps) < 1:
            raise ValueError("max_steps must be positive")
        self.symmetry = resolve_symmetry(symmetry)
        self.playouts = int(playouts)
        self.depth = None if depth is None else int(depth)
        self.playout_policy = playout_policy
        self.gamma = float(gamma)
        self.seed = int(seed)
        self.max_lanes = int(max_lanes)
        self.max_steps = int(max_steps)
        self.device = device
        self.rng_mode = rng_mode
        self.sync_every = sync_every
        self.agent = agent
        self._critic = None
        if agent is not None:
            from .lookahead import LookaheadActionFunction

            self._critic = LookaheadActionFunction(agent, gamma=self.gamma, max_children=max_children,
                                                   device=torch.device("cpu") if device is None else device, amp_dtype=amp_dtype,
                                                   rng_mode=rng_mode, use_fused=use_fused, symmetry=self.symmetry)
        self._key = seed_key(self.seed)  # head of the playout key chain
        self.last_steps = 0
        self.last_lanes = 0

    # ------------------------------------------------------------------ playouts
    def _launch_subs(self, cache: list, k: int, n_steps: int) -> np.ndarray:
        """Sub-keys [n_steps, 4] of launch k of this call; drawn from the chain the first time a slice asks for them."""
        while len(cache) <= k:
            self._key, subs = nv.chain_keys(self._key, 2 * n_steps, self._rng_mode())
            cache.append(subs.reshape(n_steps, 4))
        return cache[k]

    def _playout_slice(self, roots: torch.Tensor, lane0: int, n_total: int, cache: list):
        """All playouts of one slice of roots -> (lane_boards, lane_masks, lane_done, lane_ret, lane_disc), steps launched."""
        Bs, R, dev = roots.shape[0], self.playouts, roots.device
        n = 4 * Bs * R
        state = (torch.empty((n, 16), dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev),
                 torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
                 torch.empty(n, dtype=torch.float32, device=dev))
        policy = getattr(nv, PLAYOUT_POLICIES[self.playout_policy])
        live = torch.zeros(1, dtype=torch.int32, device=dev) if self.depth is None else None
        limit = self.max_steps if self.depth is None else self.depth
        t = k = 0
        while t < limit:
            n_steps = min(nv.MAX_FUSED_STEPS, limit - t)
            subs = self._launch_subs(cache, k, n_steps)
            if live is not None:
                live.zero_()
            nv.mc_playout(subs, t, roots, Bs, R, lane0, n_total, policy, self.gamma, *state, self._rng_mode(), live)
            t += n_steps
            k += 1
            if live is not None and int(live.item()) == 0:  # the one host read of the launch
                return state, t
        if live is not None:
            raise RuntimeError(f"Monte-Carlo playouts exceeded max_steps={self.max_steps}")
        return state, t

    def playout(self, boards: torch.Tensor):
        """The playouts of one call, slice by slice -> list of (b0, b1, lane state of roots b0 .. b1 - 1).  Advances the key
        chain; ``policy_fn`` is this plus the reduction."""
        boards = boards.contiguous()
        B, R = boards.shape[0], self.playouts
        per_slice = max(1, self.max_lanes // (4 * R))
        cache, out, steps = [], [], 0
        for b0 in range(0, B, per_slice):
            b1 = min(B, b0 + per_slice)
            state, t = self._playout_slice(boards[b0:b1], 4 * b0 * R, 4 * B * R, cache)
            steps = max(steps, t)
            out.append((b0, b1, state))
        self.last_steps, self.last_lanes = steps, 4 * B * R
        return out

    @torch.no_grad()
    def policy_fn(self, boards: torch.Tensor, masks: torch.Tensor = None):
        """boards u8 [B, 16], masks unused (legality comes out of the seeding) -> (q f32 [B, 4], v f32 [B])."""
        boards = boards.contiguous()
        B, R, dev = boards.shape[0], self.playouts, boards.device
        q = torch.empty((B, 4), dtype=torch.float32, device=dev)
        legal = torch.empty((B, 4), dtype=torch.bool, device=dev)
        if B == 0:
            return q, torch.empty(0, dtype=torch.float32, device=dev)
        for b0, b1, (lb, lm, ld, lret, ldisc) in self.playout(boards):
            values = None if self._critic is None else self._critic.values(lb)
            nv.mc_reduce(lret, ldisc, ld, values, R, q[b0:b1])
            # a legal root move changes the board (and a tile is spawned); the lane of an illegal one still holds the root
            legal[b0:b1] = (lb.view(b1 - b0, 4, R, 16)[:, :, 0] != boards[b0:b1, None]).any(dim=-1)
        return q, self.best_legal(q, legal)

    policy_fn.needs_masks = False
