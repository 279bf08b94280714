"""Kernel breakdown of the collect phase (policy-in-the-loop rollout of 65536 boards with the bf16 Transformer).
usage: python tools/probe_collect.py [boards] [--fp32] [--fp32-native] [--reduction {cls,mean}] [--unfused] [--no-profile]
  --fp32: the reference's rollout precision, the PyTorch fp32 module forward
  --fp32-native: fp32 rollout through the split-fp16 kernels (FusedPolicyF32); implies --fp32
  --reduction: the agent's reduction (default cls, bench.py's model); "mean" is the reference PPOAgent's default
  --unfused: bf16 rollout without the fused encoder kernels (the layer kernels forward-only + library-GEMM heads)
  --no-profile: the collect wall time only"""
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "2048-ppo-agent_amd"))
sys.path.insert(0, ROOT)
import torch

import bench
from src.ppo import PPOAgent, PPOTrainer, RolloutBuffer
from src.runs import BatchRunner

B = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 65536
NATIVE = "--fp32-native" in sys.argv
FP32 = "--fp32" in sys.argv or NATIVE
RED = sys.argv[sys.argv.index("--reduction") + 1] if "--reduction" in sys.argv else "cls"
assert RED in ("cls", "mean"), RED
if "--unfused" in sys.argv:
    from src.ppo import fused_policy

    fused_policy.supports = fused_policy.supports_mean = lambda agent: False
dev = torch.device("cuda:0")
torch.manual_seed(0)
agent = PPOAgent(**dict(bench.MODEL_CFG, reduction=RED))
tr = PPOTrainer(agent, BatchRunner(0, device=dev), RolloutBuffer(31, 16, 4), bench.OPTIM_CFG, max_steps=500000, device=dev,
                rollout_amp=not FP32, log_dir="/tmp/lg", **bench.TRAINER_CFG, **(dict(fp32_native=True) if NATIVE else {}))
tr.collect_rollouts(B, 1)
tr.rollout_buffer.reset()
torch.cuda.synchronize()
t = time.time()
tr.collect_rollouts(B, 1)
torch.cuda.synchronize()
print(f"reduction {RED} fused {tr.batch_runner.act_fn._fused is not None} collect wall s", round(time.time() - t, 3),
      tr.last_rollout_stats)
if "--no-profile" in sys.argv:
    sys.exit(0)
tr.rollout_buffer.reset()
from torch.profiler import ProfilerActivity, profile

with profile(activities=[ProfilerActivity.CUDA]) as prof:
    tr.collect_rollouts(B, 1)
    torch.cuda.synchronize()
ka = prof.key_averages()
tot = sum(k.self_device_time_total for k in ka)
print(f"GPU busy {tot / 1e6:.3f} s in {sum(k.count for k in ka)} kernels")
for k in sorted(ka, key=lambda k: -k.self_device_time_total)[:25]:
    print(f"{k.self_device_time_total / 1e3:9.1f} ms {k.count:7d} x {k.self_device_time_total / max(k.count, 1):8.1f} us  {k.key[:110]}")
