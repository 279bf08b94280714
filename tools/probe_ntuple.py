#!/usr/bin/env python3
"""N-tuple network on one GPU: time per launch of its five kernels, the training lock-step, the player's lock-step, learning speed.

    python tools/probe_ntuple.py [--out profiles/ntuple_probe.json]

Timing: HIP events around one call, 3 warm-up calls, median of ``--repeats`` with min and max, one process (the style of
tools/probe_mc.py).
  (a) every kernel at 4 096 and 65 536 boards of the default network in two board states: "reset" (every board freshly reset, one
      lock-step played so that each env has a predecessor) and "trained" (``--train-steps`` lock-steps into training at that env
      count).  td_accumulate is timed on zeroed acc / cnt and td_apply after an untimed accumulate (both restored outside the
      events); next to the times: gathers and atomics per launch, the number of distinct entries hit and the largest number of
      same-address atomics of the launch (the max of cnt).
  (b) the whole training lock-step (``NTupleTrainer.train``, per lock-step) at 1 024, 4 096 and 65 536 envs.
  (c) the player's lock-step (``NTupleActionFunction.policy_fn``) at 100 and 4 096 boards after ``--board-steps`` lock-steps of
      random play, next to the greedy-agent and one-ply lock-steps of a fresh-weights PPOAgent on the same boards.
  (d) learning speed: mean max tile over ``--episodes`` evaluation episodes (seed 42) after ``--learn-steps`` lock-steps at 1 024,
      4 096 and 65 536 envs, from zero weights, one seed each.
``--tc`` adds the TC learner (``NTupleTrainer(learner="tc")``, alpha 1.0) under the key "tc": its two launches tc_accumulate and
tc_apply timed as td_accumulate and td_apply are in (a), in the same two board states of a TC trainer, and its training lock-step as
in (b).  Without it the output is unchanged.
``--stage-tiles 11 12 13 14`` adds (a) and (b) on a multi-stage network with those thresholds, every stage active, under the key
"staged", in the same process: the cost of the stage (the max tile of every board looked up, S times the tables).
``--only-kernels`` leaves (c) and (d) out.
``--carousel`` measures carousel shaping instead of all of the above and writes ``profiles/ntuple_carousel_probe.json`` unless
``--out`` says otherwise: at every ``--boards`` env count two TD(0) trainers of the default network, one with
``carousel_tiles=--carousel-tiles`` and one without, each ``--train-steps`` lock-steps into training; the two launches
carousel_record and carousel_restart on the first one's state, and the whole training lock-step of both, alternating on, off, on,
off in the same process.
``--delayed`` measures the delayed TC(lambda) learner instead of all of the above and writes ``profiles/ntuple_delayed_probe.json``
unless ``--out`` says otherwise: at every ``--boards`` env count two TC trainers of the default network at alpha 1.0, one with
``lam=--lam`` (0.5: horizon 4) and one without, each ``--train-steps`` lock-steps into training; the three launches
delayed_accumulate, delayed_apply and delayed_link on the first one's state next to tc_accumulate, tc_apply and link on the second's,
and the whole training lock-step of both, alternating on, off, on, off in the same process.
``--episodes`` (the flag alone, without a count) measures the persistent episode kernel instead of all of the above and writes
``profiles/ntuple_episodes_probe.json`` unless ``--out`` says otherwise: one default network trained by TC at alpha 1.0 on 4 096 envs
for ``--episode-train-steps`` lock-steps; 1 000 evaluation episodes (seed 42) through ``evaluate_ntuple(fused=False)`` and
``fused=True``, alternating, three runs each after one warm-up of each, host wall time around a device synchronise, the two dicts
compared; ``fused=True`` alone at 10 000 and 100 000 episodes; the kernel time per step of one launch in which every game stays live,
at 1 000 and 100 000 games.
``--episodes --episodes-plies 1`` measures the searched episode kernel the same way and writes
``profiles/ntuple_search_episodes_probe.json``: ``evaluate_ntuple(plies=1)`` against ``evaluate_ntuple_episodes(plies=1)``, the scale
rows through ``play_search_episodes(plies=1)``, the per-step launch through ``g2048_ntuple_search_episodes``.
Prints one JSON line.
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
from src.ppo import (LookaheadActionFunction, NTupleActionFunction, NTupleNetwork, NTupleTrainer, PPOAgent,  # noqa: E402
                     TorchActionFunction)
from src.runs import BatchRunner, evaluate_ntuple, evaluate_ntuple_episodes  # noqa: E402

MODEL = dict(observation_dim=31, action_dim=4, hidden_dim=512, d_model=256, nhead=8, num_layers=4, dim_feedforward=1024,
             dropout=0.1, reduction="cls")


def timed(fn, repeats, warmup=3, setup=None):
    ms = []
    for i in range(warmup + repeats):
        if setup is not None:
            setup()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def kernel_state(trainer, label, repeats):
    """The five kernels on the trainer's current boards / prev_after / flag."""
    net, B = trainer.network, trainer.num_envs
    w, cells, F, st = net.weights, net.cells, net.frac_bits, net.active_tiles
    m = net.m
    saved = w.clone()
    values = torch.empty(B, dtype=torch.float32, device=w.device)
    prev, flag = trainer.prev_after.clone(), trainer.flag.clone()
    tr = trainer._tr

    def zero():
        trainer.acc.zero_(), trainer.cnt.zero_()

    def accumulate():
        nv.ntuple_td_accumulate(trainer.prev_after, trainer.flag, trainer.targets, w, cells, F, trainer.alpha, trainer.acc, trainer.cnt,
                                trainer.td_error, st)

    def prepare_apply():
        zero(), accumulate()

    nv.ntuple_scores(trainer.boards, w, cells, F, trainer.scores, trainer.targets, st)
    zero(), accumulate()
    live = int((trainer.flag != 0).sum().item())
    res = {"state": label, "boards": B, "envs_with_predecessor": live,
           "distinct_entries_hit": int((trainer.cnt > 0).sum().item()), "max_same_address_atomics": int(trainer.cnt.max().item()),
           "per_launch": {"values": f"{8 * m * B} gathers", "scores": f"<= {4 * 8 * m * B} gathers (legal moves only)",
                          "td_accumulate": f"{8 * m * live} gathers, {8 * m * live} 64-bit + {8 * m * live} 32-bit atomic adds",
                          "td_apply": f"{8 * m * live} atomic exchanges, one read-modify-write of weights and acc per distinct entry",
                          "link": f"{B} boards, 17 B in, 17 B out"}}
    res["values"] = timed(lambda: nv.ntuple_values(trainer.boards, w, cells, F, values, st), repeats)
    res["scores"] = timed(lambda: nv.ntuple_scores(trainer.boards, w, cells, F, trainer.scores, trainer.targets, st), repeats)
    res["td_accumulate"] = timed(accumulate, repeats, setup=zero)
    res["td_apply"] = timed(lambda: nv.ntuple_td_apply(trainer.prev_after, trainer.flag, cells, w, trainer.acc, trainer.cnt, st), repeats,
                            setup=prepare_apply)
    res["link"] = timed(lambda: nv.ntuple_link(tr["boards"][0], tr["meta"][0], prev, flag), repeats)
    w.copy_(saved)  # the timed applies moved the weights
    zero()
    return res


def tc_kernel_state(trainer, label, repeats):
    """The two TC kernels on the trainer's current boards / prev_after / flag, timed as td_accumulate / td_apply are."""
    net = trainer.network
    w, cells, F, m = net.weights, net.cells, net.frac_bits, net.m
    saved = w.clone(), trainer.coh_e.clone(), trainer.coh_a.clone()

    def zero():
        trainer.acc.zero_(), trainer.abs_acc.zero_(), trainer.cnt.zero_()

    def accumulate():
        nv.ntuple_tc_accumulate(trainer.prev_after, trainer.flag, trainer.targets, w, cells, F, trainer.alpha, trainer.acc, trainer.abs_acc,
                                trainer.cnt, trainer.td_error)

    def prepare_apply():
        zero(), accumulate()

    nv.ntuple_scores(trainer.boards, w, cells, F, trainer.scores, trainer.targets)
    zero(), accumulate()
    live = int((trainer.flag != 0).sum().item())
    distinct = int((trainer.cnt > 0).sum().item())
    res = {"state": label, "boards": trainer.num_envs, "envs_with_predecessor": live, "distinct_entries_hit": distinct,
           "max_same_address_atomics": int(trainer.cnt.max().item()),
           "per_launch": {"tc_accumulate": f"{8 * m * live} gathers, {16 * m * live} 64-bit + {8 * m * live} 32-bit atomic adds",
                          "tc_apply": f"{8 * m * live} atomic exchanges, one read-modify-write of weights, acc, abs_acc, coh_e and coh_a "
                                      f"per distinct entry ({distinct})"}}
    res["tc_accumulate"] = timed(accumulate, repeats, setup=zero)
    res["tc_apply"] = timed(lambda: nv.ntuple_tc_apply(trainer.prev_after, trainer.flag, cells, w, trainer.acc, trainer.abs_acc,
                                                       trainer.cnt, trainer.coh_e, trainer.coh_a), repeats, setup=prepare_apply)
    w.copy_(saved[0]), trainer.coh_e.copy_(saved[1]), trainer.coh_a.copy_(saved[2])  # the timed applies moved them
    zero()
    return res


def tc_probe(boards, envs, dev, repeats, train_steps, chunk=50):
    out = {"learner": "tc, alpha 1.0", "kernels": [], "training_lock_step": []}
    for B in boards:
        trainer = NTupleTrainer(NTupleNetwork(device=dev), B, alpha=1.0, device=dev, learner="tc")
        trainer.train(1)
        out["kernels"].append(tc_kernel_state(trainer, "reset: one lock-step after a reset of all boards", repeats))
        trainer.train(train_steps - 1)
        out["kernels"].append(tc_kernel_state(trainer, f"trained: {train_steps} lock-steps into training", repeats))
        print(json.dumps(out["kernels"][-2:]), flush=True)
        del trainer
    for B in envs:
        trainer = NTupleTrainer(NTupleNetwork(device=dev), B, alpha=1.0, device=dev, learner="tc")
        t = timed(lambda: trainer.train(chunk), repeats)
        out["training_lock_step"].append({"envs": B, "lock_steps_per_call": chunk,
                                          **{k.replace("_ms", "_ms_per_lock_step"): round(v / chunk, 4) for k, v in t.items()}})
        print(json.dumps(out["training_lock_step"][-1]), flush=True)
        del trainer
    return out


def carousel_probe(boards, dev, repeats, train_steps, tiles, chunk=50):
    out = {"carousel_tiles": list(tiles), "learner": "td0, alpha 0.1", "train_steps": train_steps, "kernels": [], "training_lock_step": []}
    for B in boards:
        on = NTupleTrainer(NTupleNetwork(device=dev), B, device=dev, carousel_tiles=tiles)
        off = NTupleTrainer(NTupleNetwork(device=dev), B, device=dev)
        on.train(train_steps), off.train(train_steps)
        saved = [t.clone() for t in (on.boards, on.masks, on.reached, on.turn, on.starts)]
        sub = (0x12345678, 0x9ABCDEF0)
        flag2 = int((on.flag == 2).sum().item())
        res = {"boards": B, "envs_restarting": flag2, "pool_slots_filled": on.pool_masks.ne(0).sum(dim=1).cpu().tolist(),
               "starts_so_far": on.starts.cpu().tolist(),
               "per_launch": {"carousel_record": f"{B} flags, 17 B in per env whose episode goes on, 17 B out per env that records",
                              "carousel_restart": f"{B} flags; per restarting env ({flag2}) two threefry blocks, <= 17 B in, <= 22 B out, "
                                                  "one 64-bit atomic add"}}
        res["carousel_record"] = timed(lambda: nv.ntuple_carousel_record(on.boards, on.masks, on.flag, on.carousel_tiles, on.reached,
                                                                         on.pool_boards, on.pool_masks), repeats)
        res["carousel_restart"] = timed(lambda: nv.ntuple_carousel_restart(sub, on.flag, on.pool_boards, on.pool_masks, on.boards, on.masks,
                                                                           on.reached, on.turn, on.starts, on.rng_mode), repeats)
        for t, s in zip((on.boards, on.masks, on.reached, on.turn, on.starts), saved):  # the timed restarts moved them
            t.copy_(s)
        out["kernels"].append(res)
        print(json.dumps(res), flush=True)
        for run in (1, 2):
            for name, trainer in (("on", on), ("off", off)):
                t = timed(lambda: trainer.train(chunk), repeats)
                out["training_lock_step"].append({"envs": B, "carousel": name, "run": run, "lock_steps_per_call": chunk,
                                                  **{k.replace("_ms", "_ms_per_lock_step"): round(v / chunk, 4) for k, v in t.items()}})
                print(json.dumps(out["training_lock_step"][-1]), flush=True)
        del on, off
    return out


def delayed_probe(boards, dev, repeats, train_steps, lam, chunk=50):
    out = {"lam": lam, "learner": "tc, alpha 1.0", "train_steps": train_steps, "kernels": [], "training_lock_step": []}
    for B in boards:
        on = NTupleTrainer(NTupleNetwork(device=dev), B, alpha=1.0, device=dev, learner="tc", lam=lam)
        off = NTupleTrainer(NTupleNetwork(device=dev), B, alpha=1.0, device=dev, learner="tc")
        on.train(train_steps), off.train(train_steps)
        out["horizon"] = h = on.horizon
        net, head, slot = on.network, (on.lock_steps - 1) % on.horizon, on.lock_steps % on.horizon
        w, cells, F, m = net.weights, net.cells, net.frac_bits, net.m
        saved = [t.clone() for t in (w, on.coh_e, on.coh_a, on.hist, on.hist_err, on.hist_len, on.prev_after, on.flag)]

        def zero():
            on.acc.zero_(), on.abs_acc.zero_(), on.cnt.zero_()

        def accumulate():
            nv.ntuple_delayed_accumulate(on.hist, on.hist_err, on.hist_len, on.flag, on.targets, head, lam, w, cells, F, on.alpha, on.acc,
                                         on.abs_acc, on.cnt, on.td_error)

        def prepare_apply():
            zero(), accumulate()

        nv.ntuple_scores(on.boards, w, cells, F, on.scores, on.targets)
        zero(), accumulate()
        live, ended = int((on.flag != 0).sum().item()), int((on.flag == 2).sum().item())
        due = int(on.cnt.sum().item()) // (8 * m)
        res = {"boards": B, "envs_with_predecessor": live, "envs_flushing": ended, "due_states": due,
               "distinct_entries_hit": int((on.cnt > 0).sum().item()), "max_same_address_atomics": int(on.cnt.max().item()),
               "per_launch": {"delayed_accumulate": f"{8 * m * live} gathers, {(h - 1) * live} f32 ring reads, {due} board loads, "
                                                    f"{16 * m * due} 64-bit + {8 * m * due} 32-bit atomic adds",
                              "delayed_apply": f"{due} board loads, {8 * m * due} atomic exchanges",
                              "delayed_link": f"{B} boards, 19 B in, 34 B out"}}
        res["delayed_accumulate"] = timed(accumulate, repeats, setup=zero)
        res["delayed_apply"] = timed(lambda: nv.ntuple_delayed_apply(on.hist, on.hist_len, on.flag, head, cells, w, on.acc, on.abs_acc, on.cnt,
                                                                     on.coh_e, on.coh_a), repeats, setup=prepare_apply)
        tr = on._tr
        res["delayed_link"] = timed(lambda: nv.ntuple_delayed_link(tr["boards"][0], tr["meta"][0], slot, on.prev_after, on.flag, on.hist,
                                                                   on.hist_len), repeats)
        zero()
        for t, s0 in zip((w, on.coh_e, on.coh_a, on.hist, on.hist_err, on.hist_len, on.prev_after, on.flag), saved):
            t.copy_(s0)  # the timed launches moved them
        plain = tc_kernel_state(off, f"lam off, {train_steps} lock-steps into training", repeats)
        res.update(tc_accumulate=plain["tc_accumulate"], tc_apply=plain["tc_apply"])
        pa, fl = off.prev_after.clone(), off.flag.clone()
        res["link"] = timed(lambda: nv.ntuple_link(off._tr["boards"][0], off._tr["meta"][0], pa, fl), repeats)
        out["kernels"].append(res)
        print(json.dumps(res), flush=True)
        for run in (1, 2):
            for name, trainer in (("on", on), ("off", off)):
                t = timed(lambda: trainer.train(chunk), repeats)
                out["training_lock_step"].append({"envs": B, "lam": name, "run": run, "lock_steps_per_call": chunk,
                                                  **{k.replace("_ms", "_ms_per_lock_step"): round(v / chunk, 4) for k, v in t.items()}})
                print(json.dumps(out["training_lock_step"][-1]), flush=True)
        del on, off
    return out


def staged_network(dev, stage_tiles):
    """The default network, unstaged or with ``stage_tiles`` and every stage active from the start (promotion is not what is timed)."""
    net = NTupleNetwork(device=dev, stage_tiles=stage_tiles)
    net.active_stages = net.stages
    return net


def kernel_probe(B, dev, repeats, train_steps, stage_tiles=None):
    net = staged_network(dev, stage_tiles)
    trainer = NTupleTrainer(net, B, device=dev)
    trainer.train(1)
    out = [kernel_state(trainer, "reset: one lock-step after a reset of all boards", repeats)]
    trainer.train(train_steps - 1)
    out.append(kernel_state(trainer, f"trained: {train_steps} lock-steps into training", repeats))
    return out


def train_probe(B, dev, repeats, chunk=50, stage_tiles=None):
    trainer = NTupleTrainer(staged_network(dev, stage_tiles), B, device=dev)
    t = timed(lambda: trainer.train(chunk), repeats)
    return {"envs": B, "lock_steps_per_call": chunk, **{k.replace("_ms", "_ms_per_lock_step"): round(v / chunk, 4) for k, v in t.items()}}


def play_boards(B, dev, board_steps):
    traj = BatchRunner(init_seed=7, device=dev)._engine.rollout_fused(B, nv.POLICY_RANDOM, fill_frozen=True)
    t = min(board_steps, traj.T - 1)
    return traj.boards[t].contiguous().clone()


def lockstep_probe(net, agent, B, dev, repeats, board_steps):
    boards = play_boards(B, dev, board_steps)
    player = NTupleActionFunction(net, device=dev)
    greedy = TorchActionFunction(agent, use_mask=True, sample_actions=False, device=dev, amp_dtype=torch.bfloat16)
    look = LookaheadActionFunction(agent, device=dev, amp_dtype=torch.bfloat16)
    return {"boards": B, "board_steps": board_steps, "ntuple": timed(lambda: player.policy_fn(boards, None), repeats),
            "greedy_agent": timed(lambda: greedy.policy_fn(boards, None), repeats),
            "one_ply_lookahead": timed(lambda: look.policy_fn(boards, None), repeats)}


def learning_probe(B, dev, steps, episodes):
    net = NTupleNetwork(device=dev)
    out = NTupleTrainer(net, B, device=dev).train(steps)
    ev = evaluate_ntuple(net, dev, num_episodes=episodes, seed=42)
    return {"envs": B, "lock_steps": steps, "training_episodes": int(out["episodes"].item()), "eval_episodes": episodes,
            "mean_max_tile": ev["mean_max_tile"], "percent": ev["percent"], "max_abs_weight": int(net.weights.abs().max().item())}


def episodes_probe(dev, train_steps, latency_steps, plies=0, chunk=1000):
    import numpy as np

    from src.actions._common import resolve_rng_mode
    from src.g2048.engine import seed_key
    from src.ppo.ntuple import SEARCH_EPISODE_STEPS

    per_launch = SEARCH_EPISODE_STEPS if plies else 2048

    net = NTupleNetwork(device=dev)
    trainer = NTupleTrainer(net, 4096, alpha=1.0, device=dev, learner="tc")
    for _ in range(train_steps // chunk):
        trainer.train(chunk)
    del trainer
    torch.cuda.empty_cache()
    out = {"network": f"4 x 6-tuples (default), frac_bits 12, TC at alpha 1.0, 4096 envs, {train_steps} lock-steps",
           "steps_per_launch": per_launch, "plies": plies}

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t

    def spread(x):
        return {"median_s": round(statistics.median(x), 4), "min_s": round(min(x), 4), "max_s": round(max(x), 4)}

    paths = {"lock_step": lambda: evaluate_ntuple(net, dev, num_episodes=1000, seed=42, plies=plies),
             "fused": lambda: evaluate_ntuple_episodes(net, num_episodes=1000, seed=42, plies=plies)}
    times, dicts = {k: [] for k in paths}, {}
    for k, fn in paths.items():
        dicts[k], _ = wall(fn)  # the warm-up
    for _ in range(3):
        for k, fn in paths.items():
            d, dt = wall(fn)
            times[k].append(dt)
            assert d == dicts[k], k
    common = [k for k in dicts["lock_step"]]
    out["episodes_1000"] = {"lock_step": spread(times["lock_step"]), "fused": spread(times["fused"]),
                            "dicts_equal_on_every_common_key": all(dicts["fused"][k] == dicts["lock_step"][k] for k in common),
                            "result": dicts["fused"]}
    print(json.dumps(out["episodes_1000"]), flush=True)
    out["fused_only"] = []
    for N in (10000, 100000):
        (boards, ep_len, score), dt = wall(lambda: net.play_search_episodes(N, 42, plies=plies))
        tiles = (1 << boards.max(dim=1).values.cpu().numpy().astype(np.int64)).astype(np.float64)
        ln = ep_len.cpu().numpy()
        out["fused_only"].append({"episodes": N, "wall_s": round(dt, 4), "launches": int(-(-int(ln.max()) // per_launch)),
                                  "mean_episode_length": float(ln.mean()), "longest_episode": int(ln.max()),
                                  "mean_max_tile": float(tiles.mean()), "mean_max_tile_standard_error": float(tiles.std(ddof=1) / np.sqrt(N)),
                                  "mean_score": float(score.cpu().numpy().mean())})
        print(json.dumps(out["fused_only"][-1]), flush=True)
    out["per_step"] = []
    mode = resolve_rng_mode(None)
    for N in (1000, 100000):
        heads = np.stack([seed_key(42 + first) for first in range(0, N, 100)])
        chain0 = nv.keys_from_numpy(np.repeat(heads, 100, axis=0)[:N], dev)
        boards = torch.empty((N, 16), dtype=torch.uint8, device=dev)
        masks, done = torch.empty(N, dtype=torch.uint8, device=dev), torch.empty(N, dtype=torch.uint8, device=dev)
        ep_len, score = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int64, device=dev)
        live = torch.zeros(1, dtype=torch.int32, device=dev)
        chain = chain0.clone()
        steps = latency_steps
        while True:  # the longest launch, halving from --episode-latency-steps, that no game ends in

            def launch():
                if plies:
                    nv.ntuple_search_episodes(True, steps, 100, net.weights, net.cells, net.frac_bits, plies, 1.0, chain, boards, masks, done,
                                              ep_len, score, mode, live)
                else:
                    nv.ntuple_episodes(True, steps, 100, net.weights, net.cells, net.frac_bits, chain, boards, masks, done, ep_len, score,
                                       mode, live)

            t = timed(launch, 5, setup=lambda: (chain.copy_(chain0), live.zero_()))
            if int(live.item()) == N or steps == 1:
                break
            steps //= 2
        out["per_step"].append({"games": N, "n_steps": steps, "games_live_afterwards": int(live.item()),
                                "launch": t, "us_per_step": round(1000.0 * t["median_ms"] / steps, 3),
                                "default_launch_ms": round(t["median_ms"] * per_launch / steps, 2)})
        print(json.dumps(out["per_step"][-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--envs", type=int, nargs="+", default=[1024, 4096, 65536])
    ap.add_argument("--player-boards", type=int, nargs="+", default=[100, 4096])
    ap.add_argument("--train-steps", type=int, default=2000)
    ap.add_argument("--learn-steps", type=int, default=800)
    ap.add_argument("--episodes", type=int, nargs="?", default=200, const=-1,
                    help="with a count: the evaluation episodes of (d); alone: measure the persistent episode kernel only (see above)")
    ap.add_argument("--episodes-plies", type=int, default=0, choices=(0, 1), help="with --episodes alone: 0 the greedy kernel, 1 the searched one")
    ap.add_argument("--episode-train-steps", type=int, default=100000, help="TC lock-steps at 4 096 envs before --episodes measures")
    ap.add_argument("--episode-latency-steps", type=int, default=256, help="steps of the launch --episodes times per step, halved until no game ends in it")
    ap.add_argument("--board-steps", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--tc", action="store_true", help="also time the TC learner's two launches and its training lock-step")
    ap.add_argument("--stage-tiles", type=int, nargs="+", default=None, metavar="K",
                    help="also time the kernels and the training lock-step on a multi-stage network with these thresholds")
    ap.add_argument("--carousel", action="store_true", help="measure carousel shaping only (see above)")
    ap.add_argument("--carousel-tiles", type=int, nargs="+", default=[7, 8, 9, 10], metavar="K",
                    help="the carousel's thresholds for --carousel (low enough that the pools fill within --train-steps)")
    ap.add_argument("--delayed", action="store_true", help="measure the delayed TC(lambda) learner only (see above)")
    ap.add_argument("--lam", type=float, default=0.5, help="lambda for --delayed")
    ap.add_argument("--only-kernels", action="store_true", help="(a) and (b) only: no player lock-step, no learning speed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_ntuple.py measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.episodes == -1:
        res = {"command": "python tools/probe_ntuple.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(dev),
               "timer": "evaluations: host wall time around a device synchronise, one warm-up of each path, then 3 runs each, alternating, "
                        "median [min, max]; per step: HIP events around one launch, 3 warm-up launches, median of 5 [min, max]",
               "episodes": episodes_probe(dev, a.episode_train_steps, a.episode_latency_steps, a.episodes_plies)}
        print(json.dumps(res))
        out = a.out or os.path.join(HERE, "..", "profiles", "ntuple_search_episodes_probe.json" if a.episodes_plies else "ntuple_episodes_probe.json")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(res, open(out, "w"), indent=1)
        return
    if a.carousel:
        res = {"command": "python tools/probe_ntuple.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(dev),
               "network": "4 x 6-tuples (default), frac_bits 12, alpha 0.1", "repeats": a.repeats,
               "timer": "HIP events around one call, 3 warm-up calls, median [min, max]",
               "carousel": carousel_probe(a.boards, dev, a.repeats, a.train_steps, a.carousel_tiles)}
        print(json.dumps(res))
        out = a.out or os.path.join(HERE, "..", "profiles", "ntuple_carousel_probe.json")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(res, open(out, "w"), indent=1)
        return
    if a.delayed:
        res = {"command": "python tools/probe_ntuple.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(dev),
               "network": "4 x 6-tuples (default), frac_bits 12, TC at alpha 1.0", "repeats": a.repeats,
               "timer": "HIP events around one call, 3 warm-up calls, median [min, max]",
               "delayed": delayed_probe(a.boards, dev, a.repeats, a.train_steps, a.lam)}
        print(json.dumps(res))
        out = a.out or os.path.join(HERE, "..", "profiles", "ntuple_delayed_probe.json")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(res, open(out, "w"), indent=1)
        return
    torch.manual_seed(0)
    agent = PPOAgent(**MODEL).to(dev).eval()
    res = {"command": "python tools/probe_ntuple.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(dev),
           "network": "4 x 6-tuples (default), frac_bits 12, alpha 0.1", "repeats": a.repeats,
           "timer": "HIP events around one call, 3 warm-up calls, median [min, max]", "kernels": [], "training_lock_step": [],
           "player_lock_step": [], "learning": []}
    for B in a.boards:
        res["kernels"] += kernel_probe(B, dev, a.repeats, a.train_steps)
        print(json.dumps(res["kernels"][-2:]), flush=True)
    for B in a.envs:
        res["training_lock_step"].append(train_probe(B, dev, a.repeats))
        print(json.dumps(res["training_lock_step"][-1]), flush=True)
    if a.stage_tiles:
        res["staged"] = {"stage_tiles": a.stage_tiles, "stages": len(a.stage_tiles) + 1, "active_stages": len(a.stage_tiles) + 1,
                         "kernels": [], "training_lock_step": []}
        for B in a.boards:
            res["staged"]["kernels"] += kernel_probe(B, dev, a.repeats, a.train_steps, a.stage_tiles)
            print(json.dumps(res["staged"]["kernels"][-2:]), flush=True)
        for B in a.envs:
            res["staged"]["training_lock_step"].append(train_probe(B, dev, a.repeats, stage_tiles=a.stage_tiles))
            print(json.dumps(res["staged"]["training_lock_step"][-1]), flush=True)
    net = NTupleNetwork(device=dev)
    for B in ([] if a.only_kernels else a.player_boards):
        res["player_lock_step"].append(lockstep_probe(net, agent, B, dev, a.repeats, a.board_steps))
        print(json.dumps(res["player_lock_step"][-1]), flush=True)
    del net
    for B in ([] if a.only_kernels else a.envs):
        res["learning"].append(learning_probe(B, dev, a.learn_steps, a.episodes))
        print(json.dumps(res["learning"][-1]), flush=True)
    if a.tc:
        res["tc"] = tc_probe(a.boards, a.envs, dev, a.repeats, a.train_steps)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
