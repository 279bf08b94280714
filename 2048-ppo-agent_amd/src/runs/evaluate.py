"""Max-tile evaluation protocol of the reference's visualisation scripts, without the plotting.

run/viz_naive_strategies.py:123-200 and run/viz_ppo_agent.py:238-300 both do: ``num_episodes`` episodes in batches
of 100, batch *i* from ``BatchRunner(init_seed=seed + 100 * i)``, metric = the largest tile on the FINAL board of
each episode; the PPO agent is evaluated greedily with the legal-action mask
(``TorchActionFunction(agent, use_mask=True, sample_actions=False)``).  The README histograms are this protocol
with seed 42 (random policy: mean max tile 109.17, DRUL: 189.44, the reference's trained PPO agent: about 383).
Only the 16-byte final boards leave the device.
"""
from __future__ import annotations

from collections import Counter
from typing import Callable, Dict

import numpy as np
import torch

from .batch_runner import BatchRunner


def evaluate_max_tile(act_fn: Callable, num_episodes: int = 1000, seed: int = 42, batch_size: int = 100,
                      rng_mode=None, device=None) -> Dict:
    """-> {"mean_max_tile", "percent": {tile: % of episodes}, "counts": {tile: n}, "mean_episode_length", "episodes"}"""
    batch_size = min(batch_size, num_episodes)
    tiles, lengths = [], []
    done, i = 0, 0
    while done < num_episodes:
        b = min(batch_size, num_episodes - done)
        runner = BatchRunner(init_seed=seed + i * batch_size, act_fn=act_fn, rng_mode=rng_mode, device=device)
        tr = runner.collect(b)
        tiles.append((1 << tr.final_boards.max(dim=1).values.cpu().numpy().astype(np.int64)))  # exact powers of two
        lengths.append(tr.ep_len.cpu().numpy())
        done += b
        i += 1
    tiles = np.concatenate(tiles).astype(np.int64)
    counts = Counter(tiles.tolist())
    return {
        "episodes": int(len(tiles)), "mean_max_tile": float(tiles.mean()),
        "counts": {int(k): int(v) for k, v in sorted(counts.items())},
        "percent": {int(k): round(100.0 * v / len(tiles), 1) for k, v in sorted(counts.items())},
        "mean_episode_length": float(np.concatenate(lengths).mean()),
    }


def evaluate_agent(agent, device, num_episodes: int = 1000, seed: int = 42, rng_mode=None, lookahead: int = 0,
                   gamma: float = 0.99, expectimax: int = 0, symmetry=None) -> Dict:
    """Greedy, masked evaluation of a PPO agent (run/viz_ppo_agent.py:267-300).  ``lookahead=1``: the same protocol (same
    seeds, same env and key stream) played by one-ply expectimax over the agent's critic with discount ``gamma``
    (``LookaheadActionFunction``) instead of the actor's argmax; ``lookahead=0`` is the reference's evaluation.  ``expectimax=2``: the same
    protocol played by two-ply expectimax (``ExpectimaxActionFunction``); it excludes ``lookahead``, whose only depth stays 1, and takes
    no other value than 0 and 2 (one ply is spelled ``lookahead=1``).  ``symmetry``: "none" / "canonical" / "ensemble" / None (ask
    G2048_SYMMETRY), handed to whichever action function is built; evaluate an agent in the mode it was trained in, or any agent
    trained without the canonical frame under "ensemble" (the mean over the eight views of every board, no retraining)."""
    from ..ppo.torch_action_wrapper import TorchActionFunction, resolve_symmetry

    symmetry = resolve_symmetry(symmetry)

    if lookahead and expectimax:
        raise ValueError("evaluate_agent: lookahead and expectimax are mutually exclusive")
    if expectimax not in (0, 2):
        raise ValueError(f"evaluate_agent: expectimax is 0 (off) or 2 plies, got {expectimax!r}; one ply is lookahead=1")
    was_training = agent.training
    if expectimax:
        from ..ppo.expectimax import ExpectimaxActionFunction

        fn = ExpectimaxActionFunction(agent, plies=expectimax, gamma=gamma, device=device, symmetry=symmetry)
    elif lookahead:
        from ..ppo.lookahead import LookaheadActionFunction

        fn = LookaheadActionFunction(agent, gamma=gamma, depth=lookahead, device=device, symmetry=symmetry)
    else:
        fn = TorchActionFunction(agent, use_mask=True, sample_actions=False, device=device, symmetry=symmetry)
    try:
        return evaluate_max_tile(fn, num_episodes, seed, rng_mode=rng_mode, device=device)
    finally:
        agent.train(was_training)


def evaluate_monte_carlo(device, num_episodes: int = 1000, seed: int = 42, agent=None, rng_mode=None, **mc_kwargs) -> Dict:
    """The same protocol (same seeds, same env and key stream) played by ``MonteCarloActionFunction(agent, **mc_kwargs)``: for
    every legal move ``playouts`` playouts of a cheap policy, the move with the best mean return wins.  ``agent=None``: plain
    playout returns, no network; with an agent its critic values the leaves the playouts were cut off at (``depth``)."""
    from ..ppo.monte_carlo import MonteCarloActionFunction

    was_training = agent.training if agent is not None else False
    fn = MonteCarloActionFunction(agent, device=device, rng_mode=rng_mode, **mc_kwargs)
    try:
        return evaluate_max_tile(fn, num_episodes, seed, rng_mode=rng_mode, device=device)
    finally:
        if agent is not None:
            agent.train(was_training)


def _max_tile_summary(tiles: np.ndarray, lengths: np.ndarray) -> Dict:
    """``evaluate_max_tile``'s dict from the max tile and the length of every episode (for an evaluation that plays no ``BatchRunner``)."""
    tiles = tiles.astype(np.int64)
    counts = Counter(tiles.tolist())
    return {
        "episodes": int(len(tiles)), "mean_max_tile": float(tiles.mean()),
        "counts": {int(k): int(v) for k, v in sorted(counts.items())},
        "percent": {int(k): round(100.0 * v / len(tiles), 1) for k, v in sorted(counts.items())},
        "mean_episode_length": float(lengths.mean()),
    }


def evaluate_ntuple(network, device, num_episodes: int = 1000, seed: int = 42, rng_mode=None, plies: int = 0, gamma: float = 1.0,
                    depth: int = 0, dedup: bool = True, fused: bool = False) -> Dict:
    """The same protocol (same seeds, same env and key stream) played by ``NTupleActionFunction(network)``: the legal move with the
    best ``reward + V(afterstate)`` under the n-tuple network, no other network involved; ``plies`` (1 or 2) searches that many
    plies of expectimax over that value first.  ``depth`` (1, 2 or 3; 0, the default, is off) plays the frontier search instead
    (``NTupleSearchActionFunction``, ``dedup`` as there); it excludes a non-zero ``plies``.  ``fused=True`` plays the greedy
    evaluation (``plies == 0`` and ``depth == 0`` only, anything else raises ``ValueError``) inside the persistent kernel
    (``NTupleNetwork.play_episodes``): all batches at once, the same games bit for bit, the same dict plus ``"mean_score"``."""
    from ..ppo.ntuple import NTupleActionFunction, NTupleSearchActionFunction

    if fused:
        if isinstance(plies, bool) or isinstance(depth, bool) or plies != 0 or depth != 0:
            raise ValueError(f"evaluate_ntuple: fused=True plays the greedy evaluation only, got plies={plies!r}, depth={depth!r}")
        if isinstance(num_episodes, bool) or not isinstance(num_episodes, (int, np.integer)) or num_episodes <= 0:
            raise ValueError(f"evaluate_ntuple: num_episodes must be a positive integer, got {num_episodes!r}")
        boards, ep_len, score = network.play_episodes(num_episodes, seed, min(100, num_episodes), rng_mode)
        out = _max_tile_summary(1 << boards.max(dim=1).values.cpu().numpy().astype(np.int64), ep_len.cpu().numpy())
        out["mean_score"] = float(score.cpu().numpy().mean())
        return out
    if isinstance(depth, bool) or depth != 0:
        if plies != 0:
            raise ValueError(f"evaluate_ntuple: depth={depth!r} and plies={plies!r} are mutually exclusive")
        fn = NTupleSearchActionFunction(network, device=device, rng_mode=rng_mode, depth=depth, gamma=gamma, dedup=dedup)
        return evaluate_max_tile(fn, num_episodes, seed, rng_mode=rng_mode, device=device)
    fn = NTupleActionFunction(network, device=device, rng_mode=rng_mode, plies=plies, gamma=gamma)
    return evaluate_max_tile(fn, num_episodes, seed, rng_mode=rng_mode, device=device)


def evaluate_ntuple_budget(network, device, num_episodes: int = 1000, seed: int = 42, rng_mode=None, max_depth: int = 4,
                           budget: int = 8192, gamma: float = 1.0) -> Dict:
    """The same protocol (same seeds, same env and key stream) played by ``NTupleBudgetSearchActionFunction(network, max_depth=...,
    budget=..., gamma=...)``: every board searched as deep, up to ``max_depth``, as its levels stay within ``budget`` distinct
    afterstates (the defaults are ``NTupleNetwork.search_budget``'s).  A bad ``max_depth``, ``budget`` or gamma raises ``ValueError``
    before a device is touched."""
    from ..ppo.ntuple import NTupleBudgetSearchActionFunction

    fn = NTupleBudgetSearchActionFunction(network, device=device, rng_mode=rng_mode, max_depth=max_depth, budget=budget, gamma=gamma)
    return evaluate_max_tile(fn, num_episodes, seed, rng_mode=rng_mode, device=device)


def evaluate_ntuple_episodes(network, num_episodes: int = 1000, seed: int = 42, rng_mode=None, plies: int = 0, gamma: float = 1.0) -> Dict:
    """``evaluate_ntuple(network, network's device, num_episodes, seed, rng_mode, plies, gamma)`` played inside the persistent kernels
    (``NTupleNetwork.play_search_episodes``): all batches at once, the same games bit for bit, the same dict key for key plus
    ``"mean_score"``.  ``plies`` is 0 (greedy) or 1 (one ply of expectimax at discount ``gamma``); anything else raises
    ``ValueError`` before a device is touched, as a non-positive ``num_episodes`` does."""
    if isinstance(num_episodes, bool) or not isinstance(num_episodes, (int, np.integer)) or num_episodes <= 0:
        raise ValueError(f"evaluate_ntuple_episodes: num_episodes must be a positive integer, got {num_episodes!r}")
    boards, ep_len, score = network.play_search_episodes(num_episodes, seed, min(100, num_episodes), rng_mode, plies=plies, gamma=gamma)
    out = _max_tile_summary(1 << boards.max(dim=1).values.cpu().numpy().astype(np.int64), ep_len.cpu().numpy())
    out["mean_score"] = float(score.cpu().numpy().mean())
    return out
