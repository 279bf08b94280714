#!/usr/bin/env python3
"""N-tuple expectimax on one GPU: the player's lock-step fused against the enumerated pipeline, the work per root, and strength.

    python tools/probe_ntuple_search.py [--out profiles/ntuple_search_probe.json]

Timing: HIP events around one call, 3 warm-up calls, median of ``--repeats`` with min and max, one process (the method of
tools/probe_ntuple.py).  The default network after ``--train-steps`` lock-steps at 4 096 envs; boards ``--board-steps`` lock-steps
into a random rollout.
  (a) lock-step: ``NTupleActionFunction(plies=p).policy_fn`` at ``--player-boards`` boards for p = 0, 1, 2 ("fused"), and for p = 1, 2
      the same Q from the entry points that existed before the fused kernels ("composed": expand -> scan -> children ->
      g2048_ntuple_scores -> reduce, two plies as ``ExpectimaxActionFunction._slice`` with the dedup on and off, host reads
      included).  Fused and composed calls alternate inside one process; their outputs are compared bit for bit first.
  (b) work: live slots per root, Q1 blocks launched and the share that exits at once, gathers per root for each depth, computed
      from the same boards with the expansion kernels.
  (c) strength: mean max tile and the share of episodes reaching 2048 over ``--episodes`` episodes of the README protocol at plies
      0, 1, 2 for each of ``--eval-seeds``, on that network and on one trained for ``--train-seconds`` of wall-clock at 4 096 envs.
``--frontier`` probes the frontier search instead (``NTupleNetwork.search``, writes profiles/ntuple_frontier_probe.json): ms per call
of ``search`` at depth 1, 2 and 3 with the dedup on and off, of the unchanged fused ``expectimax(plies=1 | 2)`` and of the composed
two-ply pipeline with dedup, alternating in one process on the same boards, the entries per root of every level, and the strength of
depth 3 against plies 2 on the two networks of (c).
``--budget`` probes the budgeted search (``NTupleNetwork.search_budget``, writes profiles/ntuple_budget_probe.json): ms per call of
``search(depth=3)`` against ``search_budget(max_depth=5)`` at budgets 1 024 / 8 192 / 24 576 and ``search_budget(max_depth=3)`` at
the largest budget, alternating in one process, on rollout boards and on boards three quarters into the games the network plays
itself; the histogram of ``depth_used`` and the leaf-level entries per root; and the strength of depth 3 against budgets 8 192 and
24 576 at ``max_depth=5`` on the two networks of (c).  The file is rewritten after every finished part.
Prints one JSON line.  ``--trace-calls N`` times nothing: it makes N calls of every variant at the largest board count, for
``rocprofv3 --kernel-trace --stats -d DIR -- python tools/probe_ntuple_search.py --trace-calls 10`` (per-kernel times of both paths).
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "2048-ppo-agent_amd"))

import torch  # noqa: E402

from src.g2048 import native as nv  # noqa: E402
from src.ppo import NTupleActionFunction, NTupleNetwork, NTupleTrainer  # noqa: E402
from src.ppo.lookahead import expand, expand_level, scan, spawn_children  # noqa: E402
from src.ppo.q_player import QPlayer  # noqa: E402
from src.runs import BatchRunner, evaluate_ntuple, evaluate_ntuple_budget  # noqa: E402


def _stat(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def timed_alternating(fns: dict, repeats, warmup=3):
    """One call of every function per round, in turn: drift of the machine falls on all of them alike."""
    ms = {k: [] for k in fns}
    for i in range(warmup + repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warmup:
                ms[k].append(a.elapsed_time(b))
    return {k: _stat(v) for k, v in ms.items()}


def leaf_values(net, rows):
    n = rows.shape[0]
    v = torch.empty(n, dtype=torch.float32, device=rows.device)
    if n:
        nv.ntuple_scores(rows, net.weights, net.cells, net.frac_bits, torch.empty((n, 4), dtype=torch.float32, device=rows.device), v)
    return v


def composed_one_ply(net, boards, gamma):
    """``LookaheadActionFunction.policy_fn`` with the n-tuple greedy value as the leaf."""
    after, reward, nchild, offset, incl = expand_level(boards)
    N = int(incl[-1].item())  # the host read of the lock-step
    children, terminal = spawn_children(after, nchild, offset, N)
    q = torch.empty_like(reward)
    nv.lookahead_reduce(reward, nchild, offset, leaf_values(net, children), terminal, gamma, N, q)
    return q, QPlayer.best_legal(q, nchild > 0)


def composed_two_plies(net, boards, gamma, dedup):
    """``ExpectimaxActionFunction.policy_fn`` / ``_slice`` (one slice) with the n-tuple greedy value as the leaf."""
    dev = boards.device
    after1, reward1, nchild1, offset1, incl1 = expand_level(boards)
    N1 = int(incl1[-1].item())  # host read 1
    q2 = torch.empty_like(reward1)
    if N1 == 0:
        return q2.zero_(), torch.zeros(boards.shape[0], device=dev)
    G = nchild1.shape[0]
    children1, terminal1 = spawn_children(after1, nchild1, offset1, N1)
    after2, reward2, nchild2 = expand(children1)
    if dedup:
        group_start = torch.empty(G + 1, dtype=torch.int32, device=dev)
        group_start[:G] = offset1[:, 0] * 4
        group_start[G] = 4 * N1
        rep = torch.empty((N1, 4), dtype=torch.int32, device=dev)
        nuniq = torch.empty((N1, 4), dtype=torch.int32, device=dev)
        nv.lookahead_dedup(after2, nchild2, group_start, rep, nuniq)
    else:
        rep, nuniq = torch.arange(4 * N1, dtype=torch.int32, device=dev).view(N1, 4), nchild2
    offset2, incl2 = scan(nuniq)
    N2 = int(incl2[-1].item())  # host read 2
    children2, terminal2 = spawn_children(after2, nuniq, offset2, N2)
    e = torch.empty((N1, 4), dtype=torch.float32, device=dev)
    nv.lookahead_reduce(torch.zeros_like(reward2), nuniq, offset2, leaf_values(net, children2), terminal2, gamma, N2, e)
    v1 = torch.empty(N1, dtype=torch.float32, device=dev)
    nv.lookahead_backup(reward2, nchild2, rep, e, v1)
    nv.lookahead_reduce(reward1, nchild1, offset1, v1, terminal1, gamma, N1, q2)
    return q2, QPlayer.best_legal(q2, nchild1 > 0)


def play_boards(B, dev, board_steps):
    traj = BatchRunner(init_seed=7, device=dev)._engine.rollout_fused(B, nv.POLICY_RANDOM, fill_frozen=True)
    return traj.boards[min(board_steps, traj.T - 1)].contiguous().clone()


def same_bits(x, y):
    return bool(torch.equal(x[0].view(torch.int32), y[0].view(torch.int32)) and torch.equal(x[1].view(torch.int32), y[1].view(torch.int32)))


def lockstep_probe(net, B, dev, repeats, board_steps, gamma):
    boards = play_boards(B, dev, board_steps)
    fused = {p: NTupleActionFunction(net, device=dev, plies=p, gamma=gamma) for p in (0, 1, 2)}
    fns = {"fused_plies0": lambda: fused[0].policy_fn(boards, None),
           "fused_plies1": lambda: fused[1].policy_fn(boards, None),
           "composed_plies1": lambda: composed_one_ply(net, boards, gamma),
           "fused_plies2": lambda: fused[2].policy_fn(boards, None),
           "composed_plies2_dedup": lambda: composed_two_plies(net, boards, gamma, True),
           "composed_plies2_no_dedup": lambda: composed_two_plies(net, boards, gamma, False)}
    agree = {"plies1": same_bits(fns["fused_plies1"](), fns["composed_plies1"]()),
             "plies2_dedup": same_bits(fns["fused_plies2"](), fns["composed_plies2_dedup"]()),
             "plies2_no_dedup": same_bits(fns["fused_plies2"](), fns["composed_plies2_no_dedup"]())}
    return {"boards": B, "board_steps": board_steps, "gamma": gamma, "fused_equals_composed_bit_for_bit": agree,
            **timed_alternating(fns, repeats), "work": work(net, boards)}


def work(net, boards):
    """What the fused kernels do on these boards, counted with the expansion kernels (a legal (board, action) lane gathers 8 m)."""
    B, g = boards.shape[0], 8 * net.m
    after1, _, nchild1, offset1, incl1 = expand_level(boards)
    N1 = int(incl1[-1].item())
    children1, _ = spawn_children(after1, nchild1, offset1, N1)
    after2, _, nchild2 = expand(children1)
    legal2 = int((nchild2 > 0).sum().item())
    offset2, incl2 = scan(nchild2)
    N2 = int(incl2[-1].item())
    children2, _ = spawn_children(after2, nchild2, offset2, N2)
    _, _, nchild3 = expand(children2)
    legal3 = int((nchild3 > 0).sum().item())
    return {"live_slots_per_root": round(N1 / B, 2), "plies1": {"blocks": B, "gathers_per_root": round(g * legal2 / B, 1)},
            "plies2": {"q1_blocks_launched": 128 * B, "q1_blocks_live": N1, "share_exiting_at_once": round(1 - N1 / (128 * B), 4),
                       "level2_children_per_root": round(N2 / B, 1), "gathers_per_root": round(g * legal3 / B, 1)},
            "plies0": {"gathers_per_root": round(g * int((nchild1 > 0).sum().item()) / B, 1)}}


def strength(net, dev, episodes, seeds, gamma):
    out = []
    for plies in (0, 1, 2):
        per_seed = []
        for s in seeds:
            t0 = time.perf_counter()
            ev = evaluate_ntuple(net, dev, num_episodes=episodes, seed=s, plies=plies, gamma=gamma)
            per_seed.append({"seed": s, "mean_max_tile": ev["mean_max_tile"],
                             "percent_2048": round(sum(v for k, v in ev["percent"].items() if int(k) >= 2048), 1),
                             "mean_episode_length": ev["mean_episode_length"], "seconds": round(time.perf_counter() - t0, 1)})
        means = [r["mean_max_tile"] for r in per_seed]
        out.append({"plies": plies, "episodes": episodes, "per_seed": per_seed, "mean_max_tile": round(statistics.mean(means), 1),
                    "min": min(means), "max": max(means), "percent_2048": round(statistics.mean(r["percent_2048"] for r in per_seed), 1)})
        print(json.dumps(out[-1]), flush=True)
    return out


def frontier_probe(net, B, dev, repeats, board_steps, gamma):
    """``NTupleNetwork.search`` at depth 1, 2, 3 with the dedup on and off against the unchanged fused path and the composed two-ply
    pipeline with dedup, alternating in one process on the same boards; the entries per root of every level."""
    boards = play_boards(B, dev, board_steps)
    fns = {"expectimax_plies1": lambda: net.expectimax(boards, 1, gamma),
           "expectimax_plies2": lambda: net.expectimax(boards, 2, gamma),
           "composed_plies2_dedup": lambda: composed_two_plies(net, boards, gamma, True)}
    for depth in (1, 2, 3):
        for dedup in (True, False):
            fns[f"search_depth{depth}_{'dedup' if dedup else 'no_dedup'}"] = lambda depth=depth, dedup=dedup: net.search(boards, depth, gamma, dedup)
    agree = {"depth1": same_bits(fns["search_depth1_dedup"](), fns["expectimax_plies1"]()),
             "depth2": same_bits(fns["search_depth2_dedup"](), fns["expectimax_plies2"]()),
             "depth2_no_dedup": same_bits(fns["search_depth2_no_dedup"](), fns["expectimax_plies2"]()),
             "depth3_dedup_equals_no_dedup": same_bits(fns["search_depth3_dedup"](), fns["search_depth3_no_dedup"]())}
    counts = {}
    for dedup in (True, False):
        c = net.search(boards, 3, gamma, dedup, return_counts=True)[2].cpu().tolist()
        counts["dedup" if dedup else "no_dedup"] = [round(x / B, 2) for x in c]
    return {"boards": B, "board_steps": board_steps, "gamma": gamma, "search_equals_expectimax_bit_for_bit": agree,
            "entries_per_root": counts, **timed_alternating(fns, repeats)}


def frontier_strength(net, dev, episodes, seeds, gamma):
    """Depth 3 of the frontier search against plies 2 of the fused path: the same episodes, seconds per evaluation."""
    out = []
    for key, n in (("plies", 2), ("depth", 3)):
        per_seed = []
        for s in seeds:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev = evaluate_ntuple(net, dev, num_episodes=episodes, seed=s, gamma=gamma, **{key: n})
            per_seed.append({"seed": s, "mean_max_tile": ev["mean_max_tile"],
                             "percent_2048": round(sum(v for k, v in ev["percent"].items() if int(k) >= 2048), 1),
                             "mean_episode_length": ev["mean_episode_length"], "seconds": round(time.perf_counter() - t0, 1)})
        means = [r["mean_max_tile"] for r in per_seed]
        out.append({key: n, "episodes": episodes, "per_seed": per_seed, "mean_max_tile": round(statistics.mean(means), 1),
                    "min": min(means), "max": max(means)})
        print(json.dumps(out[-1]), flush=True)
    return out


def frontier_main(a, dev):
    res = {"command": "python tools/probe_ntuple_search.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(dev),
           "network": "4 x 6-tuples (default), frac_bits 12, alpha 0.1", "repeats": a.repeats,
           "timer": "HIP events around one call, 3 warm-up calls, median [min, max], the variants alternating", "lock_step": [],
           "strength": []}
    net = NTupleNetwork(device=dev)
    trainer = NTupleTrainer(net, 4096, device=dev)
    trainer.train(a.train_steps)
    for B in a.player_boards:
        res["lock_step"].append(frontier_probe(net, B, dev, a.repeats, a.board_steps, a.gamma))
        print(json.dumps(res["lock_step"][-1]), flush=True)
    if a.episodes > 0:
        res["strength"].append({"network": f"{trainer.lock_steps} lock-steps at 4096 envs",
                                "by_search": frontier_strength(net, dev, a.episodes, a.eval_seeds, a.gamma)})
        if a.train_seconds > 0:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < a.train_seconds:
                trainer.train(50)
                trainer.boards.max().item()
            res["strength"].append({"network": f"{a.train_seconds:.0f} s more of training at 4096 envs ({trainer.lock_steps} lock-steps in all)",
                                    "by_search": frontier_strength(net, dev, a.episodes, a.eval_seeds, a.gamma)})
    print(json.dumps(res))
    out = a.out or os.path.join(HERE, "..", "profiles", "ntuple_frontier_probe.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)


def late_boards(net, B, dev):
    """Board b = the board three quarters into the greedy game env b plays under ``net``."""
    tr = BatchRunner(init_seed=11, act_fn=NTupleActionFunction(net, device=dev), device=dev).collect(B)
    t = (tr.ep_len.to(torch.int64) * 3 // 4).clamp(max=tr.T - 1)
    return tr.boards[t, torch.arange(B, device=dev)].contiguous().clone()


BUDGET_VARIANTS = ((5, 1024), (5, 8192), (5, 24576), (3, 24576))  # (max_depth, budget)


def budget_probe(net, boards, kind, repeats, gamma):
    """``search(depth=3)`` against ``search_budget`` at the variants above, alternating in one process on the same boards."""
    B = boards.shape[0]
    fns = {"search_depth3": lambda: net.search(boards, 3, gamma)}
    for D, K in BUDGET_VARIANTS:
        fns[f"budget{K}_max_depth{D}"] = lambda D=D, K=K: net.search_budget(boards, D, K, gamma)
    out = {"boards": B, "kind": kind, "gamma": gamma, "variants": {}}
    want = fns["search_depth3"]()
    for D, K in BUDGET_VARIANTS:
        q, v, used, entries = net.search_budget(boards, D, K, gamma, return_depths=True)
        at3 = used == 3
        leaf = entries.gather(1, (used.to(torch.int64) - 1)[:, None])[:, 0]
        out["variants"][f"budget{K}_max_depth{D}"] = {
            "depth_used_histogram": {d: int((used == d).sum().item()) for d in range(1, D + 1)},
            "mean_leaf_level_entries_per_root": round(float(leaf.double().mean().item()), 1),
            "mean_entries_per_root_by_level": [round(x, 1) for x in entries.double().mean(dim=0).cpu().tolist()],
            "roots_at_depth3_equal_search_depth3_bit_for_bit": bool(torch.equal(q[at3].view(torch.int32), want[0][at3].view(torch.int32)))}
    out.update(timed_alternating(fns, repeats))
    return out


def budget_strength(net, dev, episodes, seeds, gamma, save, large_seeds=None):
    """Depth 3 of the frontier search against the budgeted search: the same episodes, seconds per evaluation.  ``large_seeds``: the
    seeds the largest budget is evaluated at (the others are NOT MEASURED for it)."""
    out = []
    for name, kw in (("depth=3", None), ("budget=8192, max_depth=5", dict(max_depth=5, budget=8192)),
                     ("budget=24576, max_depth=5", dict(max_depth=5, budget=24576))):
        per_seed = []
        out.append({"search": name, "episodes": episodes, "per_seed": per_seed})
        for s in (large_seeds or seeds) if kw and kw["budget"] == 24576 else seeds:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kw is None:
                ev = evaluate_ntuple(net, dev, num_episodes=episodes, seed=s, gamma=gamma, depth=3)
            else:
                ev = evaluate_ntuple_budget(net, dev, num_episodes=episodes, seed=s, gamma=gamma, **kw)
            per_seed.append({"seed": s, "mean_max_tile": ev["mean_max_tile"],
                             "percent_2048": round(sum(v for k, v in ev["percent"].items() if int(k) >= 2048), 1),
                             "mean_episode_length": ev["mean_episode_length"], "seconds": round(time.perf_counter() - t0, 1)})
            means = [r["mean_max_tile"] for r in per_seed]
            out[-1].update(mean_max_tile=round(statistics.mean(means), 1), min=min(means), max=max(means))
            print(json.dumps({"search": name, **per_seed[-1]}), flush=True)
            save(out)
    return out


def budget_main(a, dev):
    res = {"command": "python tools/probe_ntuple_search.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(dev),
           "network": "4 x 6-tuples (default), frac_bits 12, alpha 0.1", "repeats": a.repeats,
           "timer": "HIP events around one call, 3 warm-up calls, median [min, max], the variants alternating", "lock_step": [],
           "strength": []}
    out = a.out or os.path.join(HERE, "..", "profiles", "ntuple_budget_probe.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)) or ".", exist_ok=True)

    def save(partial=None):
        json.dump(res if partial is None else {**res, "strength_in_progress": partial}, open(out, "w"), indent=1)

    net = NTupleNetwork(device=dev)
    trainer = NTupleTrainer(net, 4096, device=dev)
    trainer.train(a.train_steps)
    for B in a.player_boards:
        for kind, boards in (("48 lock-steps into a random rollout", play_boards(B, dev, a.board_steps)),
                             ("three quarters into the network's own greedy games", late_boards(net, B, dev))):
            res["lock_step"].append(budget_probe(net, boards, kind, a.repeats, a.gamma))
            print(json.dumps(res["lock_step"][-1]), flush=True)
            save()
    if a.episodes > 0:
        res["strength"].append({"network": f"{trainer.lock_steps} lock-steps at 4096 envs",
                                "by_search": budget_strength(net, dev, a.episodes, a.eval_seeds, a.gamma, save, a.large_budget_seeds)})
        save()
        if a.train_seconds > 0:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < a.train_seconds:
                trainer.train(50)
                trainer.boards.max().item()
            network = f"{a.train_seconds:.0f} s more of training at 4096 envs ({trainer.lock_steps} lock-steps in all)"
            res["strength"].append({"network": network, "by_search": []})
            res["strength"][-1]["by_search"] = budget_strength(net, dev, a.episodes, a.eval_seeds, a.gamma, save, a.large_budget_seeds)
            save()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--budget", action="store_true", help="probe the budgeted search (NTupleNetwork.search_budget) against search(depth=3) "
                    "instead; writes profiles/ntuple_budget_probe.json unless --out is given")
    ap.add_argument("--frontier", action="store_true", help="probe the frontier search (NTupleNetwork.search) against the fused and the "
                    "composed paths instead; writes profiles/ntuple_frontier_probe.json unless --out is given")
    ap.add_argument("--large-budget-seeds", type=int, nargs="+", default=None, help="with --budget: evaluate budget 24576 at these seeds only "
                    "(it costs some twenty times depth 3); default: every one of --eval-seeds")
    ap.add_argument("--player-boards", type=int, nargs="+", default=[100, 1024, 4096])
    ap.add_argument("--train-steps", type=int, default=2000)
    ap.add_argument("--train-seconds", type=float, default=120.0)
    ap.add_argument("--episodes", type=int, default=200)
    ap.add_argument("--eval-seeds", type=int, nargs="+", default=[42, 1042, 2042])
    ap.add_argument("--board-steps", type=int, default=48)
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--trace-calls", type=int, default=0, help="no timing: this many calls of every variant at the largest of "
                    "--player-boards, for a kernel trace taken from outside")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_ntuple_search.py measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.frontier:
        return frontier_main(a, dev)
    if a.budget:
        return budget_main(a, dev)
    res = {"command": "python tools/probe_ntuple_search.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(dev),
           "network": "4 x 6-tuples (default), frac_bits 12, alpha 0.1", "repeats": a.repeats,
           "timer": "HIP events around one call, 3 warm-up calls, median [min, max], the variants alternating", "lock_step": [],
           "strength": []}
    net = NTupleNetwork(device=dev)
    trainer = NTupleTrainer(net, 4096, device=dev)
    trainer.train(a.train_steps)
    if a.trace_calls > 0:  # for `rocprofv3 --kernel-trace --stats -- python tools/probe_ntuple_search.py --trace-calls 10`
        boards = play_boards(a.player_boards[-1], dev, a.board_steps)
        fused = {p: NTupleActionFunction(net, device=dev, plies=p, gamma=a.gamma) for p in (1, 2)}
        for _ in range(a.trace_calls):
            fused[1].policy_fn(boards, None), fused[2].policy_fn(boards, None)
            composed_one_ply(net, boards, a.gamma)
            composed_two_plies(net, boards, a.gamma, True), composed_two_plies(net, boards, a.gamma, False)
        torch.cuda.synchronize()
        return
    for B in a.player_boards:
        res["lock_step"].append(lockstep_probe(net, B, dev, a.repeats, a.board_steps, a.gamma))
        print(json.dumps(res["lock_step"][-1]), flush=True)
    if a.episodes > 0:
        res["strength"].append({"network": f"{trainer.lock_steps} lock-steps at 4096 envs",
                                "by_plies": strength(net, dev, a.episodes, a.eval_seeds, a.gamma)})
        if a.train_seconds > 0:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < a.train_seconds:
                trainer.train(50)
                trainer.boards.max().item()  # the chunk's host read, as run/train_ntuple.py does
            res["strength"].append({"network": f"{a.train_seconds:.0f} s more of training at 4096 envs ({trainer.lock_steps} lock-steps in all)",
                                    "by_plies": strength(net, dev, a.episodes, a.eval_seeds, a.gamma)})
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
