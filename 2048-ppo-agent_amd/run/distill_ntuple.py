#!/usr/bin/env python3
"""Distil an n-tuple network into the Transformer policy and report the student's strength on the README protocol.

    python 2048-ppo-agent_amd/run/distill_ntuple.py --teacher net.pt --envs 4096 --minutes 3 --evals 3 --out result.json
    python 2048-ppo-agent_amd/run/distill_ntuple.py --teacher-minutes 2 --teacher-plies 1 --beta 0.5 --minutes 10

The teacher is an ``NTupleNetwork``: loaded from ``--teacher`` (what run/train_ntuple.py ``--save`` writes) or trained here by TC at
alpha 1.0 for ``--teacher-minutes`` on the same number of envs.  It labels at ``--teacher-plies`` plies of expectimax (0: its greedy
scores).  Training = ``DistillTrainer`` on ``--envs`` always-live boards (the model of run/train_to_2048.py, its optimiser settings):
iterations of ``--collect-steps`` lock-steps and ``--minibatches`` optimiser steps; after every iteration one byte is read back, the
largest tile on a board the STUDENT played.  "First 2048" is the training wall-clock of the first iteration after which that byte
says 2048, as run/train_to_2048.py defines it for its rollouts.  Evaluation = ``evaluate_agent`` (greedy, legal-action mask,
``--eval-episodes`` episodes, seed 42) at ``--evals`` points spread evenly over the budget plus the untrained student, each with the
mean cross-entropy and agreement of the iterations since the last point; the teacher is evaluated once (``evaluate_ntuple`` at the
same plies).  Evaluation time is excluded from the training clock.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

from src.ppo import DistillTrainer, NTupleActionFunction, NTupleNetwork, NTupleSearchActionFunction, NTupleTrainer, PPOAgent  # noqa: E402
from src.runs import evaluate_agent, evaluate_ntuple  # noqa: E402

MODEL = dict(observation_dim=31, action_dim=4, hidden_dim=512, d_model=256, nhead=8, num_layers=4, dim_feedforward=1024,
             dropout=0.1, reduction="cls")  # run/train_to_2048.py's


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--teacher", default=None, help="an NTupleNetwork saved by run/train_ntuple.py --save (default: train one here)")
    ap.add_argument("--teacher-minutes", type=float, default=2.0, help="without --teacher: minutes of TC training at alpha 1.0")
    ap.add_argument("--teacher-plies", type=int, default=0, choices=(0, 1, 2), help="expectimax depth the teacher labels (and is evaluated) at")
    ap.add_argument("--teacher-depth", type=int, default=0, choices=(0, 1, 2, 3), metavar="D",
                    help="1 2 3: the teacher labels (and is evaluated) with the frontier search at this depth; excludes --teacher-plies")
    ap.add_argument("--envs", type=int, default=4096, help="parallel boards")
    ap.add_argument("--minutes", type=float, default=3.0, help="distillation budget (wall-clock, evaluation excluded)")
    ap.add_argument("--tau", type=float, default=0.0, help="0: the teacher's move; > 0: softmax(q / tau) over the legal moves")
    ap.add_argument("--beta", type=float, default=0.5, help="share of the envs the teacher plays; the student plays the others")
    ap.add_argument("--batch", type=int, default=4096, help="minibatch rows")
    ap.add_argument("--capacity", type=int, default=1 << 19, help="rows of the ring")
    ap.add_argument("--collect-steps", type=int, default=16, help="lock-steps per iteration")
    ap.add_argument("--minibatches", type=int, default=16, help="optimiser steps per iteration")
    ap.add_argument("--evals", type=int, default=3, help="evaluation points, evenly spread, the last at the end of the budget")
    ap.add_argument("--eval-episodes", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0, help="seed of the weights, the environments and the minibatch draws")
    ap.add_argument("--out", default=None, help="write the JSON result here")
    ap.add_argument("--save-agent", default=None, help="write the final agent's state_dict here")
    a = ap.parse_args(argv)
    if a.teacher_depth and a.teacher_plies:
        ap.error("--teacher-depth and a non-zero --teacher-plies are mutually exclusive")
    return a


def main():
    a = parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.teacher:
        net = NTupleNetwork.load(a.teacher, device=dev)
        teacher_info = dict(path=a.teacher)
    else:
        net = NTupleNetwork(device=dev)
        nt = NTupleTrainer(net, a.envs, alpha=1.0, seed=a.seed, device=dev, learner="tc")
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < a.teacher_minutes * 60.0:
            nt.train(50)
            torch.cuda.synchronize()
        teacher_info = dict(trained_minutes=round((time.perf_counter() - t0) / 60, 2), lock_steps=nt.lock_steps, learner="tc", alpha=1.0)
        del nt  # (its accumulators are 2 GB)
        torch.cuda.empty_cache()
    tev = evaluate_ntuple(net, dev, num_episodes=a.eval_episodes, seed=42, plies=a.teacher_plies, depth=a.teacher_depth)
    teacher_info.update(plies=a.teacher_plies, depth=a.teacher_depth, mean_max_tile=tev["mean_max_tile"], percent=tev["percent"])
    print(f"teacher at {a.teacher_depth or a.teacher_plies} plies: mean max tile {tev['mean_max_tile']:.1f}  {tev['percent']}", flush=True)

    torch.manual_seed(a.seed)
    agent = PPOAgent(**MODEL)
    teacher = (NTupleSearchActionFunction(net, device=dev, depth=a.teacher_depth) if a.teacher_depth
               else NTupleActionFunction(net, device=dev, plies=a.teacher_plies))
    tr = DistillTrainer(agent, teacher, a.envs, max(a.capacity, a.batch, a.envs),
                        batch_size=a.batch, tau=a.tau, beta=a.beta, seed=a.seed, device=dev)

    def evaluate(minutes, ce, agreement):
        ev = evaluate_agent(agent, dev, a.eval_episodes)
        ev.update(train_minutes=round(minutes, 2), rows=tr.rows, updates=tr.updates, ce=ce, agreement=agreement)
        print(f"eval @ {minutes:.2f} min / {tr.updates} updates: mean max tile {ev['mean_max_tile']:.1f}  {ev['percent']}  "
              f"ce {ce}  agreement {agreement}", flush=True)
        return ev

    evals = [evaluate(0.0, None, None)]
    train_s, it, first_2048, log = 0.0, 0, None, []
    points = [a.minutes * 60.0 * (k + 1) / max(a.evals, 1) for k in range(max(a.evals, 1))]
    ce_sum = ag_sum = 0.0
    n_since = 0
    while points:
        it += 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = tr.train(1, a.collect_steps, a.minibatches)
        top = int(tr.student_top.item())  # the one host read of an iteration (it also ends the iteration's clock)
        train_s += time.perf_counter() - t0
        ce, ag = float(out["ce"]), float(out["agreement"])
        ce_sum, ag_sum, n_since = ce_sum + ce, ag_sum + ag, n_since + 1
        log.append({"iteration": it, "train_minutes": round(train_s / 60, 3), "rows": tr.rows, "updates": tr.updates,
                    "max_tile_student_envs": 1 << top, "ce": round(ce, 5), "agreement": round(ag, 4)})
        if it % 10 == 0:
            print(json.dumps(log[-1]), flush=True)
        if top >= 11 and first_2048 is None:
            first_2048 = {"train_minutes": round(train_s / 60, 3), "iteration": it, "rows": tr.rows}
            print("FIRST 2048 TILE on a student-driven board:", first_2048, flush=True)
        if train_s >= points[0]:
            points.pop(0)
            evals.append(evaluate(train_s / 60, round(ce_sum / n_since, 5), round(ag_sum / n_since, 4)))
            ce_sum = ag_sum = 0.0
            n_since = 0
    if a.save_agent:
        os.makedirs(os.path.dirname(os.path.abspath(a.save_agent)) or ".", exist_ok=True)
        torch.save(agent.state_dict(), a.save_agent)
    res = {"config": "distillation of an n-tuple teacher into the run/train_to_2048.py model", "envs": a.envs, "n_gpus": 1,
           "tau": a.tau, "beta": a.beta, "batch": a.batch, "capacity": tr.capacity, "collect_steps": a.collect_steps,
           "minibatches": a.minibatches, "seed": a.seed, "train_minutes": round(train_s / 60, 2), "rows": tr.rows, "updates": tr.updates,
           "rows_per_sec_training": round(tr.rows / max(train_s, 1e-9), 1), "first_2048_tile": first_2048, "teacher": teacher_info,
           "evals": evals, "iterations": log,
           "baselines_mean_max_tile": {"random": 109.17, "drul": 189.44, "reference_ppo_readme": 383, "ppo_10_minutes": 462}}
    print(json.dumps({k: v for k, v in res.items() if k != "iterations"}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
