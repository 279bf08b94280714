"""Cost of the canonical frame: the two kernels (g2048_sym_canon / g2048_sym_logits) at 65 536 and 2^22 boards (HIP events around
``launches`` back-to-back launches, best of 3), and the collect phase of 65 536 boards with and without the mode (same weights,
same seed, wall time of whole collect_rollouts calls).  Prints one JSON line.
usage: python tools/probe_symmetry.py [boards for the collect, default 65536] [--no-collect]"""
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
