"""Cost of the canonical frame: the two kernels (g2048_sym_canon / g2048_sym_logits) at 65 536 and 2^22 boards (HIP events around
``launches`` back-to-back launches, best of 3), and the collect phase of 65 536 boards with and without the mode (same weights,
same seed, wall time of whole collect_rollouts calls).  Prints one JSON line.
usage: python tools/probe_symmetry.py [boards for the collect, default 65536] [--no-collect]

``--ensemble [--agent state_dict.pt] [--out result.json]`` measures the eight-view ensemble instead, by the protocol of
tools/probe_lookahead.py (HIP events around one call, 3 warm-up calls, median of 7 with min and max): g2048_sym_views and
g2048_sym_fold at 100, 65 536 and 2^20 boards next to g2048_sym_canon, and the greedy and one-ply lock-steps at 100 and 4 096
boards with symmetry "none" and "ensemble" on the same weights and boards."""
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "2048-ppo-agent_amd"))
sys.path.insert(0, ROOT)
import torch

import bench
from src.g2048 import native as nv
from src.ppo import PPOAgent, PPOTrainer, RolloutBuffer
from src.runs import BatchRunner

dev = torch.device("cuda:0")
B_COLLECT = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 65536


def time_us(fn, launches=20):
    best = None
    for _ in range(3):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / launches
        best = us if best is None else min(best, us)
    return round(best, 2)




def ensemble_probe():
    import probe_lookahead as pl
    from src.ppo import LookaheadActionFunction, PPOAgent as Agent, TorchActionFunction

    arg = lambda name: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None
    torch.manual_seed(0)
    agent = Agent(**pl.MODEL)
    if arg("--agent"):
        agent.load_state_dict(torch.load(arg("--agent"), map_location="cpu"))
    agent = agent.to(dev).eval()
    res = {"agent": os.path.basename(arg("--agent")) if arg("--agent") else "fresh weights", "precision": "bfloat16",
           "timer": "HIP events around one call, 3 warm-up calls, median [min, max] of 7", "kernels": {}, "lockstep": {}}
    for B in (100, 65536, 1 << 20):
        boards = torch.randint(0, 12, (B, 16), dtype=torch.uint8, device=dev)
        canon, frame = torch.empty_like(boards), torch.empty(B, dtype=torch.uint8, device=dev)
        views = torch.empty((B, 8, 16), dtype=torch.uint8, device=dev)
        logits, values = torch.randn((8 * B, 4), device=dev), torch.randn(8 * B, device=dev)
        ol, ov = torch.empty((B, 4), device=dev), torch.empty(B, device=dev)
        k = {"sym_canon_boards_frame": pl.timed(lambda: nv.sym_canon(boards, canon, frame=frame), 7),      # 33 B per board
             "sym_views": pl.timed(lambda: nv.sym_views(boards, views), 7),                                # 16 r + 128 w
             "sym_fold": pl.timed(lambda: nv.sym_fold(logits, values, ol, ov), 7),                          # 160 r + 20 w
             "sym_fold_values_only": pl.timed(lambda: nv.sym_fold(None, values, None, ov), 7)}              # 32 r + 4 w
        for name, nbytes in (("sym_canon_boards_frame", 33), ("sym_views", 144), ("sym_fold", 180), ("sym_fold_values_only", 36)):
            k[name]["GBps"] = round(B * nbytes / k[name]["median_ms"] / 1e6, 1)
        res["kernels"][str(B)] = k
    for B in (100, 4096):
        boards = pl.mid_game_boards(agent, B, dev)
        row = {}
        for mode in ("none", "ensemble"):
            greedy = TorchActionFunction(agent, use_mask=True, sample_actions=False, device=dev, amp_dtype=torch.bfloat16, symmetry=mode)
            look = LookaheadActionFunction(agent, device=dev, amp_dtype=torch.bfloat16, symmetry=mode)
            row[mode] = {"greedy": pl.timed(lambda: greedy.policy_fn(boards, None), 7), "greedy_forward_rows": B * (8 if mode == "ensemble" else 1),
                         "one_ply": pl.timed(lambda: look.policy_fn(boards, None), 7)}
            row[mode]["one_ply_forward_rows"] = look.last_children * (8 if mode == "ensemble" else 1)
        for player in ("greedy", "one_ply"):
            row[player + "_ensemble_over_none"] = round(row["ensemble"][player]["median_ms"] / row["none"][player]["median_ms"], 2)
        res["lockstep"][str(B)] = row
    print(json.dumps(res))
    if arg("--out"):
        os.makedirs(os.path.dirname(os.path.abspath(arg("--out"))) or ".", exist_ok=True)
        json.dump(res, open(arg("--out"), "w"), indent=1)


if "--ensemble" in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    ensemble_probe()
    sys.exit(0)

out = {"kernels": {}, "collect": {}}
for B in (65536, 1 << 22):
    boards = torch.randint(0, 12, (B, 16), dtype=torch.uint8, device=dev)
    actions = torch.randint(0, 4, (B,), dtype=torch.uint8, device=dev)
    masks = torch.randint(0, 16, (B,), dtype=torch.uint8, device=dev)
    canon, frame = torch.empty_like(boards), torch.empty(B, dtype=torch.uint8, device=dev)
    logits = torch.randn((B, 4), device=dev)
    back = torch.empty_like(logits)
    rollout_us = time_us(lambda: nv.sym_canon(boards, canon, frame=frame))                   # what a lock-step launches
    buffer_us = time_us(lambda: nv.sym_canon(canon, actions=actions, masks=masks))           # the in-place pass over a buffer
    logits_us = time_us(lambda: nv.sym_logits(logits, frame, back))
    out["kernels"][str(B)] = {
        "sym_canon_boards_frame_us": rollout_us, "GBps": round(B * 33 / rollout_us / 1e3, 1),
        "sym_canon_in_place_boards_actions_masks_us": buffer_us, "in_place_GBps": round(B * 36 / buffer_us / 1e3, 1),
        "sym_logits_us": logits_us, "logits_GBps": round(B * 33 / logits_us / 1e3, 1)}

if "--no-collect" not in sys.argv:
    for mode in ("none", "canonical"):
        torch.manual_seed(0)
        agent = PPOAgent(**bench.MODEL_CFG)
        tr = PPOTrainer(agent, BatchRunner(0, device=dev), RolloutBuffer(31, 16, 4), bench.OPTIM_CFG, max_steps=500000, device=dev,
                        rollout_amp=True, log_dir="/tmp/lg", symmetry=mode, **bench.TRAINER_CFG)
        tr.collect_rollouts(B_COLLECT, 1)  # warm-up
        secs = []
        for _ in range(3):
            tr.rollout_buffer.reset()
            torch.cuda.synchronize()
            t = time.perf_counter()
            tr.collect_rollouts(B_COLLECT, 1)
            torch.cuda.synchronize()
            secs.append(round(time.perf_counter() - t, 4))
        st = tr.last_rollout_stats
        out["collect"][mode] = {"boards": B_COLLECT, "seconds": secs, "best_seconds": min(secs), "steps_in_buffer": tr.rollout_buffer.buffer_size,
                                "mean_episode_length": round(st["mean_episode_length"], 1)}
print(json.dumps(out))
