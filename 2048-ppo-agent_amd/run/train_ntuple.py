#!/usr/bin/env python3
"""Train the n-tuple afterstate value network by TD(0) or TC and report its strength on the README protocol.

    python 2048-ppo-agent_amd/run/train_ntuple.py --envs 4096 --minutes 10 --evals 3 --out result.json
    python 2048-ppo-agent_amd/run/train_ntuple.py --learner tc --alpha 1.0 --envs 4096 --minutes 10 --evals 3

Training = ``NTupleTrainer`` on ``--envs`` always-live boards, greedy in the network being learned, in chunks of lock-steps; after
every chunk one byte per env is read back (the largest tile on a training board).  "First 2048" is the training wall-clock and
the lock-step count at the end of the first chunk after which a training board holds a 2048 tile.  Evaluation = the histogram
protocol of ``evaluate_max_tile`` (``--eval-episodes`` episodes, seed 42, batches of 100, largest tile of the final board), at
``--evals`` points spread evenly over the budget, the last one at its end; evaluation time is excluded from the training clock.
``--eval-plies 0 1 2`` plays every evaluation point once per listed expectimax depth over the network (0: greedy, the default).
``--learner tc`` learns by temporal coherence (a step size per table entry, ``NTupleTrainer``); it is meant to run at ``--alpha 1.0``
and records the coherence numbers (entries with a rate, their mean rate) at every evaluation point.
``--stage-tiles 11 12 13 14`` trains a multi-stage network (one set of tables per max-tile stage, ``NTupleNetwork``); the trainer
splits a stage off at the first check, every ``--promote-every`` lock-steps, at which a training board has reached its threshold.
The result records ``stage_tiles``, every promotion (lock-step, training seconds at the end of its chunk) and ``active_stages`` at
every evaluation point.
``--carousel`` turns carousel shaping on with the network's stage thresholds (``NTupleTrainer(carousel_tiles="stages")``: episodes
start in turn at every stage, from pools of boards at which games entered it), ``--carousel-tiles K ...`` with thresholds of its own
(on any network).  The result records ``carousel_tiles`` and, at every evaluation point, ``carousel_starts``: the episode starts per
stage so far (index 0: fresh boards, fallbacks included).
``--lam 0.5`` turns delayed TD(lambda) / TC(lambda) on for either learner (``NTupleTrainer(lam=...)``: an afterstate is updated once,
``--horizon`` - 1 lock-steps late, by the lambda-sum of the errors since; the default horizon is the smallest h with lam^h <= 0.1,
capped at 8).  The result records ``lam`` and ``horizon``.
``--eval-fused`` plays the greedy and the one-ply evaluation (``--eval-plies 0 1``) inside the persistent episode kernels
(``evaluate_ntuple(fused=True)`` and ``evaluate_ntuple_episodes(plies=1)``: the same games bit for bit, all batches at once); two
plies and ``--eval-depth`` stay on the lock-step path.  Every evaluation records ``mean_score`` where the path reports it and
``eval_seconds``.
``--eval-budget K`` adds the budgeted search (``evaluate_ntuple_budget``: every board as deep, up to ``--eval-max-depth``, as its
levels stay within K distinct afterstates) to every evaluation point, recorded under the key ``"budget"`` with its ``max_depth``.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

from src.ppo import NTupleNetwork, NTupleTrainer  # noqa: E402
from src.ppo.ntuple import BUDGET_DEFAULT_DEPTH  # noqa: E402
from src.runs import evaluate_ntuple, evaluate_ntuple_budget, evaluate_ntuple_episodes  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096, help="parallel boards")
    ap.add_argument("--minutes", type=float, default=10.0, help="training budget (wall-clock, evaluation excluded)")
    ap.add_argument("--alpha", type=float, default=0.1, help="learning rate of the whole network (split over its 8 m lookups)")
    ap.add_argument("--learner", choices=NTupleTrainer.LEARNERS, default="td0", help="td0: one alpha for every entry; tc: a rate per entry")
    ap.add_argument("--evals", type=int, default=3, help="evaluation points, evenly spread, the last at the end of the budget")
    ap.add_argument("--eval-at", type=float, nargs="*", default=None, help="evaluation points in minutes instead of --evals")
    ap.add_argument("--eval-episodes", type=int, default=1000)
    ap.add_argument("--eval-plies", type=int, nargs="+", default=[0], choices=(0, 1, 2),
                    help="expectimax depths to evaluate at: every evaluation point plays the same seeds once per depth")
    ap.add_argument("--eval-depth", type=int, nargs="+", default=[], choices=(1, 2, 3), metavar="D",
                    help="frontier-search depths (1 2 3) to evaluate at as well, one strength line per depth")
    ap.add_argument("--eval-budget", type=int, default=None, choices=range(4, 24577), metavar="K",
                    help="evaluate the budgeted search as well: at most K (4 .. 24576) distinct afterstates per level of a board")
    ap.add_argument("--eval-max-depth", type=int, default=None, choices=range(1, 7), metavar="D",
                    help="its depth ceiling, 1 .. 6 (default: the search's own); needs --eval-budget")
    ap.add_argument("--eval-fused", action="store_true", help="play the greedy and the one-ply evaluation (--eval-plies 0 1) inside the persistent episode kernels")
    ap.add_argument("--stage-tiles", type=int, nargs="+", default=None, metavar="K",
                    help="log2 tile thresholds of a multi-stage network, ascending (11 12 13 14: a stage from 2048, 4096, 8192, 16384)")
    ap.add_argument("--promote-every", type=int, default=64, metavar="N", help="lock-steps between two promotion checks (0: never)")
    ap.add_argument("--carousel", action="store_true", help="carousel shaping over the network's --stage-tiles")
    ap.add_argument("--carousel-tiles", type=int, nargs="+", default=None, metavar="K",
                    help="carousel shaping over these log2 tile thresholds, ascending (instead of --carousel)")
    ap.add_argument("--lam", type=float, default=None, help="delayed TD(lambda) / TC(lambda) with this lambda in [0, 1] (default: off)")
    ap.add_argument("--horizon", type=int, default=None, metavar="H", help="its horizon, 1 .. 8 (default: the smallest h with lam^h <= 0.1)")
    ap.add_argument("--chunk", type=int, default=50, help="lock-steps between two looks at the clock")
    ap.add_argument("--seed", type=int, default=0, help="seed of the training environments")
    ap.add_argument("--out", default=None, help="write the JSON result here")
    ap.add_argument("--save", default=None, help="save the trained network here")
    args = ap.parse_args(argv)
    if args.eval_max_depth is not None and args.eval_budget is None:
        ap.error("--eval-max-depth is the depth ceiling of --eval-budget: give that too")
    if args.carousel and args.carousel_tiles:
        ap.error("--carousel takes the network's thresholds, --carousel-tiles its own: give one of them")
    return args


def main():
    args = parse_args()

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    net = NTupleNetwork(device=dev, stage_tiles=args.stage_tiles)
    trainer = NTupleTrainer(net, args.envs, alpha=args.alpha, seed=args.seed, device=dev, learner=args.learner,
                            promote_every=args.promote_every, carousel_tiles="stages" if args.carousel else args.carousel_tiles,
                            lam=args.lam, horizon=args.horizon)
    budget = args.minutes * 60.0
    points = sorted(60.0 * m for m in args.eval_at) if args.eval_at else [budget * (k + 1) / args.evals for k in range(max(args.evals, 1))]
    result = dict(envs=args.envs, learner=args.learner, alpha=args.alpha, seed=args.seed, tuples=[list(t) for t in net.tuples],
                  frac_bits=net.frac_bits, minutes=args.minutes, first_2048=None, evaluations=[],
                  stage_tiles=None if net.stage_tiles is None else list(net.stage_tiles), promote_every=args.promote_every, promotions=[],
                  carousel_tiles=None if trainer.carousel_tiles is None else list(trainer.carousel_tiles),
                  lam=trainer.lam, horizon=trainer.horizon)
    trained = 0.0
    episodes = 0
    while points:
        t0 = time.perf_counter()
        out = trainer.train(args.chunk)
        top = int(trainer.boards.max().item())  # the one host read of a chunk (it also ends the chunk's clock)
        trained += time.perf_counter() - t0
        episodes += int(out["episodes"].item())
        for lock_step, active in trainer.promotions[len(result["promotions"]):]:  # those of this chunk, timed at its end
            result["promotions"].append(dict(lock_step=lock_step, active_stages=active, train_seconds=round(trained, 2)))
            print(f"stage {active - 1} split off at lock-step {lock_step} ({trained:.1f} s of training)", flush=True)
        if result["first_2048"] is None and top >= 11:
            result["first_2048"] = dict(seconds=round(trained, 2), lock_steps=trainer.lock_steps)
            print(f"first 2048 tile on a training board after {trained:.1f} s, {trainer.lock_steps} lock-steps", flush=True)
        if trained >= points[0]:
            points.pop(0)
            coherence = None
            if args.learner == "tc":
                c = trainer.coherence()
                coherence = dict(entries=int(c["entries"].item()), mean_rate=round(float(c["mean_rate"].item()), 4))
                print(f"{trained / 60:.2f} min: {coherence['entries']} entries with a rate, mean rate {coherence['mean_rate']}", flush=True)
            budgeted = [] if args.eval_budget is None else [("budget", args.eval_budget)]
            for key, n in [("plies", p) for p in args.eval_plies] + [("depth", d) for d in args.eval_depth] + budgeted:
                t_eval = time.perf_counter()
                if key == "budget":
                    depth_kw = {} if args.eval_max_depth is None else {"max_depth": args.eval_max_depth}
                    ev = evaluate_ntuple_budget(net, dev, num_episodes=args.eval_episodes, seed=42, budget=n, **depth_kw)
                    ev.update(max_depth=depth_kw.get("max_depth", BUDGET_DEFAULT_DEPTH))
                elif args.eval_fused and key == "plies" and n == 1:
                    ev = evaluate_ntuple_episodes(net, num_episodes=args.eval_episodes, seed=42, plies=1)
                else:
                    fused = args.eval_fused and key == "plies" and n == 0
                    ev = evaluate_ntuple(net, dev, num_episodes=args.eval_episodes, seed=42, **({"fused": True} if fused else {key: n}))
                ev.update({key: n}, eval_seconds=round(time.perf_counter() - t_eval, 2), train_seconds=round(trained, 2), lock_steps=trainer.lock_steps, episodes_trained=episodes,
                          max_abs_weight=int(net.weights.abs().max().item()), active_stages=net.active_stages)
                if coherence is not None:
                    ev.update(coherence=coherence)
                if trainer.starts is not None:
                    ev.update(carousel_starts=trainer.starts.cpu().tolist())
                result["evaluations"].append(ev)
                print(f"{trained / 60:.2f} min, {trainer.lock_steps} lock-steps, {key} {n}: mean max tile "
                      f"{ev['mean_max_tile']:.1f}, percent {ev['percent']}", flush=True)
    result["lock_steps"] = trainer.lock_steps
    result["lock_steps_per_s"] = round(trainer.lock_steps / trained, 1)
    result["env_steps_per_s"] = round(trainer.lock_steps * args.envs / trained, 1)
    if args.save:
        net.save(args.save)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
