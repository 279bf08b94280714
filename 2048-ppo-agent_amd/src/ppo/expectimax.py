"""Two-ply expectimax play over the critic, with the duplicate afterstates of one root removed (no reference counterpart).

    V1(s') = 0 if s' is terminal, else max over the legal a' of [ r(s', a') + gamma * E_spawn V(s'') ],   V(terminal s'') = 0
    Q2(s, a) = r(s, a) + gamma * E_spawn V1(s')

Env model, spawn law, child order and per-operation f32 rounding are those of the one-ply kernels (``lookahead.py``), which
run on both levels: a level-1 child is just a board, so both levels are built from that module's ``expand_level`` (= ``expand`` +
``scan``; level 2 scans after the dedup), ``spawn_children`` and the parent's ``values``.  Per lock-step and slice of roots:

    expand(boards) -> cumsum, host read 1 -> children                           children1 [N1,16], terminal1, offset1
    expand(children1)                                                           after2 [N1,4,16], reward2, nchild2
    g2048_lookahead_dedup, one workgroup per root                               rep, nuniq
    cumsum(nuniq), host read 2 -> children(after2, nuniq) -> value forward      values [N2]
    reduce(reward = 0, nuniq, values)                                           e [4 N1] = gamma * mean at representatives
    g2048_lookahead_backup                                                      V1 [N1] = max_a' reward2 + e[rep]
    reduce(reward1, nchild1, offset1, values = V1, terminal1)                   q2 [B,4]

Spawns in the same line along the next move's direction slide into the same afterstate, so about half of one root's legal
(child, action) pairs repeat an earlier one; equal afterstates have equal spawn children and hence equal expectations, which
are therefore computed once.  ``0 + x`` is exact in f32, so ``reward2 + e[rep]`` rounds exactly as the undeduplicated
``reward2 + gamma * mean`` does: with a value function that does not depend on the batch a row sits in, ``dedup=True`` and
``dedup=False`` return the same bits.
"""
from __future__ import annotations

from typing import Optional

import torch

from ..g2048 import native as nv
from .lookahead import LookaheadActionFunction, expand, expand_level, scan, spawn_children

MAX_CHILDREN_PER_BOARD = 120  # one tile: 4 legal moves x 15 empty cells x 2 tiles
MAX_SLICE_CHILDREN = 1 << 24  # the entry points take at most 2^24 boards, and a level-1 child is a board


class ExpectimaxActionFunction(LookaheadActionFunction):
    """``LookaheadActionFunction`` whose "logits" are the two-ply expectimax values ``Q2(s, .)`` of the agent's critic.

    ``plies=1`` is the parent (same outputs); ``plies=2`` the pipeline above; anything else raises ``ValueError``.
    ``policy_fn(boards, masks) -> (q2 f32 [B,4], v f32 [B])`` with the parent's shapes and masking, ``use_mask=True,
    sample_actions=False`` forced, ``QPlayer``'s un-batched ``__call__``.  ``dedup=False`` skips the dedup launch and values every
    afterstate's children.  ``max_children``: rows per value-forward call AND level-1 children per slice of roots (whole boards;
    a board has at most 120, hence ``max_children >= 120``): the largest input stays bounded in memory and inside the int32
    offsets.  ``last_children`` is the number of value-forward rows of the latest call, ``last_children_full`` that number without
    dedup (both from sums the lock-step reads back anyway).  ``symmetry``: as in the parent (the value forward sees canonical
    boards, or under "ensemble" all eight views of every child, in chunks of ``max_children // 8`` boards; the dedup still compares
    afterstates as they lie, and ``last_children`` counts boards)."""

    def __init__(self, agent, plies: int = 2, gamma: float = 0.99, dedup: bool = True, max_children: int = 1 << 18,
                 device: torch.device = torch.device("cpu"), amp_dtype: Optional[torch.dtype] = None, sync_every: int = 8,
                 rng_mode=None, use_fused: Optional[bool] = None, symmetry: Optional[str] = None):
        if plies not in (1, 2):
            raise ValueError(f"ExpectimaxActionFunction: plies must be 1 or 2, got plies={plies!r}")
        if plies == 2 and int(max_children) < MAX_CHILDREN_PER_BOARD:
            raise ValueError(f"max_children must hold one board's level-1 children (>= {MAX_CHILDREN_PER_BOARD})")
        super().__init__(agent, gamma=gamma, depth=1, max_children=max_children, device=device, amp_dtype=amp_dtype,
                         sync_every=sync_every, rng_mode=rng_mode, use_fused=use_fused, symmetry=symmetry)
        self.plies = int(plies)
        self.dedup = bool(dedup)
        self.last_children_full = 0

    def _slices(self, per_board_incl):
        """Whole boards, at most ``max_children`` level-1 children each: [(b0, b1)] from the inclusive per-board counts."""
        cap = min(self.max_children, MAX_SLICE_CHILDREN)
        out, b0, base = [], 0, 0
        B = len(per_board_incl)
        if per_board_incl[-1] <= cap:
            return [(0, B)]
        for b in range(B):
            if per_board_incl[b] - base > cap:  # board b does not fit any more: close the slice before it
                out.append((b0, b))
                b0, base = b, per_board_incl[b - 1]
        out.append((b0, B))
        return out

    @torch.no_grad()
    def policy_fn(self, boards: torch.Tensor, masks: torch.Tensor = None):
        """boards u8 [B, 16], masks unused (legality comes out of the expansion) -> (q2 f32 [B, 4], v f32 [B])."""
        if self.plies == 1:
            out = super().policy_fn(boards, masks)
            self.last_children_full = self.last_children
            return out
        after1, reward1, nchild1, offset1, incl1 = expand_level(boards.contiguous())
        per_board = incl1[3::4].tolist()  # host read 1: the level-1 totals, per board so that the slices can be cut
        q2 = torch.empty_like(reward1)
        rows = rows_full = 0
        for b0, b1 in self._slices(per_board):
            base = per_board[b0 - 1] if b0 else 0
            n2, n2_full = self._slice(after1[b0:b1], reward1[b0:b1], nchild1[b0:b1], offset1[b0:b1] - base,
                                      per_board[b1 - 1] - base, q2[b0:b1])
            rows += n2
            rows_full += n2_full
        self.last_children, self.last_children_full = rows, rows_full
        return q2, self.best_legal(q2, nchild1 > 0)

    policy_fn.needs_masks = False

    def _slice(self, after1, reward1, nchild1, offset1, N1: int, q2):
        """One slice of roots (views of whole boards; ``offset1`` relative to the slice) -> q2 in place; (rows, rows_full)."""
        G, dev = nchild1.shape[0], nchild1.device
        if N1 == 0:  # nothing but terminal boards
            q2.zero_()
            return 0, 0
        children1, terminal1 = spawn_children(after1, nchild1, offset1, N1)
        after2, reward2, nchild2 = expand(children1)  # (scanned below: the dedup decides which counts)
        if self.dedup:
            group_start = torch.empty(G + 1, dtype=torch.int32, device=dev)
            group_start[:G] = offset1[:, 0] * 4
            group_start[G] = 4 * N1
            rep = torch.empty((N1, 4), dtype=torch.int32, device=dev)
            nuniq = torch.empty((N1, 4), dtype=torch.int32, device=dev)
            nv.lookahead_dedup(after2, nchild2, group_start, rep, nuniq)
        else:
            rep = torch.arange(4 * N1, dtype=torch.int32, device=dev).view(N1, 4)
            nuniq = nchild2
        offset2, incl2 = scan(nuniq)
        if self.dedup:
            N2, N2_full = torch.stack((incl2[-1], nchild2.sum(dtype=torch.int32))).tolist()  # host read 2
        else:
            N2 = N2_full = int(incl2[-1].item())
        children2, terminal2 = spawn_children(after2, nuniq, offset2, N2)
        values = self.values(children2)
        e = torch.empty((N1, 4), dtype=torch.float32, device=dev)
        nv.lookahead_reduce(torch.zeros_like(reward2), nuniq, offset2, values, terminal2, self.gamma, N2, e)
        v1 = torch.empty(N1, dtype=torch.float32, device=dev)
        nv.lookahead_backup(reward2, nchild2, rep, e, v1)
        nv.lookahead_reduce(reward1, nchild1, offset1, v1, terminal1, self.gamma, N1, q2)
        return int(N2), int(N2_full)
