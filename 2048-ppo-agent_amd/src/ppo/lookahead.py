"""One-ply expectimax play: the critic looked up behind every possible spawn, on the device (no reference counterpart).

    Q(s, a) = r(s, a) + gamma * E_{s' ~ spawn(after(s, a))} [ V(s') ],     V(terminal s') = 0

The env model is the engine's own (``board_move`` / ``board_legal``), the spawn law is the env's (uniform over the empty
cells of the afterstate, tile 2 with p = 0.9, tile 4 with p = 0.1), so the expectation is exact; only V is learned.  Per
lock-step: ``g2048_lookahead_expand`` (four afterstates per board) -> ``torch.cumsum`` over the 4 B child counts, whose total
is read back once (the children have to be sized for the forward) -> ``g2048_lookahead_children`` -> the agent's value
forward on the children, in chunks of ``max_children`` rows -> ``g2048_lookahead_reduce``.

The steps are functions of this module, shared with the two-ply player (``expectimax.py``) and the probes: ``expand_level`` (expand and
scan, no host read), ``spawn_children``, and ``LookaheadActionFunction.values``, the chunked critic forward that the Monte-Carlo
player bootstraps from as well.  The un-batched ``__call__`` and the masked max are ``QPlayer``'s (``q_player.py``).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from ..g2048 import native as nv
from .q_player import QPlayer
from .torch_action_wrapper import TorchActionFunction


class Level(NamedTuple):
    """One expansion level of n boards: the four afterstates, their merge scores, the spawn children behind each move (0 where it
    is illegal), where a move's children start in the packed child rows, and the inclusive scan (its last entry is their number)."""
    after: torch.Tensor  # u8 [n, 4, 16]
    reward: torch.Tensor  # f32 [n, 4]
    nchild: torch.Tensor  # i32 [n, 4]
    offset: torch.Tensor  # i32 [n, 4]
    incl: torch.Tensor  # i32 [4 n]


def expand(boards: torch.Tensor):
    """boards u8 [n, 16] (contiguous) -> (after, reward, nchild) of ``g2048_lookahead_expand``, newly allocated."""
    n, dev = boards.shape[0], boards.device
    after = torch.empty((n, 4, 16), dtype=torch.uint8, device=dev)
    reward = torch.empty((n, 4), dtype=torch.float32, device=dev)
    nchild = torch.empty((n, 4), dtype=torch.int32, device=dev)
    nv.lookahead_expand(boards, after, reward, nchild)
    return after, reward, nchild


def scan(counts: torch.Tensor):
    """counts i32 [n, 4] -> (offset i32 [n, 4], incl i32 [4 n]): the exclusive and the inclusive prefix sum, on the device."""
    incl = torch.cumsum(counts.view(-1), 0, dtype=torch.int32)
    return (incl - counts.view(-1)).view(-1, 4), incl


def expand_level(boards: torch.Tensor) -> Level:
    """``expand`` and the ``scan`` of its child counts; no host read (the caller reads ``incl`` to size the children)."""
    after, reward, nchild = expand(boards)
    return Level(after, reward, nchild, *scan(nchild))


def spawn_children(after: torch.Tensor, counts: torch.Tensor, offset: torch.Tensor, N: int):
    """Every spawn child of every afterstate, packed at ``offset`` -> (children u8 [N, 16], terminal u8 [N])."""
    dev = after.device
    children = torch.empty((N, 16), dtype=torch.uint8, device=dev)
    terminal = torch.empty(N, dtype=torch.uint8, device=dev)
    nv.lookahead_children(after, counts, offset, N, children, terminal)
    return children, terminal


class LookaheadActionFunction(QPlayer, TorchActionFunction):
    """``TorchActionFunction`` whose "logits" are the one-ply expectimax values ``Q(s, .)`` of the agent's critic, played as a
    ``QPlayer`` (its un-batched ``__call__``; ``rng_mode`` may be a string, an unknown one raises ``ValueError`` when it is used).

    ``policy_fn(boards, masks)`` returns ``(q f32 [B, 4], v f32 [B])`` with ``v = max over the legal actions of q`` (0 where
    there is none).  ``use_mask=True, sample_actions=False`` are forced, so the engine (``g2048_policy_step``) takes the
    masked argmax of ``q`` exactly as it does for actor logits; the env, its key stream and the trajectory format are
    untouched.  The recorded ``log_prob`` is therefore the log-softmax of ``q`` at the chosen action: NOT a policy
    probability (``q`` is in score units), so such trajectories are for evaluation, not for a PPO update.

    ``gamma``: discount on the children's values (default: the trainer's 0.99).  ``depth``: only 1.  ``max_children``: rows per
    value-forward call (the forward of a 65 536-board batch would otherwise allocate activations for millions of rows).
    The value forward is the agent's existing one: ``FusedPolicy.__call__`` for a bf16 default-shape PPOAgent of either
    reduction, ``TorchActionFunction._forward`` otherwise; the children's logits are discarded.  A function kept across
    optimiser steps sees the new weights (the fused pack is refreshed when stale, the module forward reads the parameters).
    ``symmetry``: as in ``TorchActionFunction``; use the mode the critic was trained in, or "ensemble" with any critic: the value
    of a child is then the mean over its eight views, ``max_children`` still bounds the forward rows per call (a chunk holds
    ``max(1, max_children // 8)`` boards) and ``last_children`` still counts boards.
    """

    def __init__(self, agent, gamma: float = 0.99, depth: int = 1, max_children: int = 1 << 18,
                 device: torch.device = torch.device("cpu"), amp_dtype: Optional[torch.dtype] = None, sync_every: int = 8,
                 rng_mode=None, use_fused: Optional[bool] = None, symmetry: Optional[str] = None):
        if depth != 1:
            raise ValueError(f"LookaheadActionFunction: only depth=1 is implemented, got depth={depth!r}")
        if int(max_children) <= 0:
            raise ValueError("max_children must be a positive number of rows")
        super().__init__(agent, use_mask=True, sample_actions=False, device=device, amp_dtype=amp_dtype,
                         sync_every=sync_every, rng_mode=rng_mode, use_fused=use_fused, symmetry=symmetry)
        self.gamma = float(gamma)
        self.depth = 1
        self.max_children = int(max_children)
        self.last_children = 0  # N of the latest policy_fn call (probes and tests read it; no extra synchronisation)

    def _values(self, rows: torch.Tensor) -> torch.Tensor:
        """The agent's critic on packed boards u8 [n, 16] -> f32 [n].  With ``symmetry="canonical"`` the rows are turned into their
        canonical views first; nothing is mapped back (values are invariant, and ``q`` is in the env's frame because the
        expansion is).  With ``symmetry="ensemble"`` the value forward runs on the eight views of every row and the values are
        folded (``g2048_sym_fold``, values only): f32 [n] again, invariant under the symmetries of each row."""
        if self.symmetry == "ensemble":  # (_policy is the forward below: this class never holds a graph cache)
            return self._ensemble(rows, want_logits=False)[1]
        if self.symmetry == "canonical":
            rows = self._canonical(rows, with_frame=False)[0]
        agent_dev = next(self.agent.parameters()).device
        if self._fused is not None and rows.device == agent_dev:
            return self._fused(rows)[1]
        return self._forward(rows, agent_dev)[1]

    @property
    def _chunk(self) -> int:
        """Boards per ``_values`` call: ``max_children`` counts forward rows, and the ensemble makes eight of a board."""
        return max(1, self.max_children // 8) if self.symmetry == "ensemble" else self.max_children

    def values(self, rows: torch.Tensor) -> torch.Tensor:
        """The critic on any number of packed boards u8 [n, 16] -> f32 [n], ``_chunk`` boards per ``_values`` call."""
        n = rows.shape[0]
        out = torch.empty(n, dtype=torch.float32, device=rows.device)
        for c0 in range(0, n, self._chunk):
            c1 = min(n, c0 + self._chunk)
            out[c0:c1] = self._values(rows[c0:c1]).to(torch.float32).reshape(-1)
        return out

    @torch.no_grad()
    def policy_fn(self, boards: torch.Tensor, masks: torch.Tensor = None):
        """boards u8 [B, 16], masks unused (legality comes out of the expansion) -> (q f32 [B, 4], v f32 [B])."""
        after, reward, nchild, offset, incl = expand_level(boards.contiguous())
        N = self.last_children = int(incl[-1].item())  # the one host read of the lock-step
        children, terminal = spawn_children(after, nchild, offset, N)
        q = torch.empty_like(reward)
        nv.lookahead_reduce(reward, nchild, offset, self.values(children), terminal, self.gamma, N, q)
        return q, self.best_legal(q, nchild > 0)

    policy_fn.needs_masks = False
