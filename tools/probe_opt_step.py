#!/usr/bin/env python3
"""Cost of the optimiser step of the PPO update, alone and inside a trainer's minibatch, on one GPU.

    python tools/probe_opt_step.py --opt adamw|lamb --flat 0|1 [--repeats 7] [--out result.json]

On the default agent (4 layers, d_model 256, "cls", 3.96 M parameters) at minibatch 2048, bf16 update:
  step        one optimiser step alone on gradients that are already there: the flat step's kernels where the trainer holds one,
              else the PyTorch calls of the reference's loop (scaler.unscale_, clip_grad_norm_, scaler.step, scaler.update).
              HIP events, 3 warm-up calls, median of ``--repeats`` with min and max.
  update      ``ms_per_minibatch`` of ``PPOTrainer.update_policy`` (forward + loss + backward + optimiser step per minibatch,
              hipGraph replay where the trainer captures one), wall clock over whole calls after one warm-up call.
``--flat 0`` sets G2048_FLAT_OPT=0 (the PyTorch calls for every optimiser).  Only names that the trainer has had since the flat AdamW
step exist are used, so the same file measures an older checkout.  Prints one JSON object.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "2048-ppo-agent_amd"))

MODEL = dict(observation_dim=31, action_dim=4, hidden_dim=512, d_model=256, nhead=8, num_layers=4, dim_feedforward=1024,
             dropout=0.1, reduction="cls")
TRAINER = dict(gamma=0.99, lambda_gae=0.95, clip_epsilon=0.2, value_loss_coef=0.5, entropy_coef=0.01, max_grad_norm=0.5,
               target_kl=1e9, use_action_mask=True, mixed_precision="bfloat16", shuffle_on_reset=True, rollout_amp=True)
OPTIM = dict(max_lr=4e-4, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, warmup_steps_ratio=0.025,
             scheduler_names=["constant", "constant"], blacklist_weight_modules=["norm", "embedding"])


def timed(fn, repeats, warmup=3):
    """-> {"median_ms", "min_ms", "max_ms"} of ``repeats`` event-timed calls after ``warmup`` untimed ones."""
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--opt", choices=["adamw", "lamb"], default="lamb")
    ap.add_argument("--flat", type=int, choices=[0, 1], default=1)
    ap.add_argument("--minibatch", type=int, default=2048)
    ap.add_argument("--minibatches", type=int, default=24, help="minibatches per timed update_policy call")
    ap.add_argument("--boards", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["G2048_FLAT_OPT"] = str(a.flat)

    import torch

    from src.ppo import PPOAgent, PPOTrainer, RolloutBuffer
    from src.runs import BatchRunner

    if not torch.cuda.is_available():
        raise SystemExit("probe_opt_step.py measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(a.seed)
    agent = PPOAgent(**MODEL)
    tr = PPOTrainer(agent, BatchRunner(init_seed=a.seed), RolloutBuffer(31, 16, 4), dict(OPTIM, opt_name=a.opt), max_steps=100000,
                    device=dev, max_samples_per_epoch=a.minibatch * a.minibatches, log_dir=tempfile.mkdtemp(prefix="probe_opt_"),
                    **TRAINER)
    flat = getattr(tr, "_flat_step", None)
    res = {"opt": a.opt, "flat_requested": a.flat, "flat_step": type(flat).__name__ if flat is not None else None,
           "parameters": sum(p.numel() for p in agent.parameters()), "minibatch": a.minibatch, "repeats": a.repeats,
           "timer": "step: HIP events around one call, 3 warm-up calls, median [min, max]; update: wall clock of update_policy / minibatches"}

    # ---- the update as the trainer runs it
    tr.collect_rollouts(a.boards, 1)
    m = tr.update_policy(batch_size=a.minibatch, n_epochs=1)  # warm-up: captures the graph
    per_call = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = tr.update_policy(batch_size=a.minibatch, n_epochs=1)
        torch.cuda.synchronize()
        per_call.append((time.perf_counter() - t0) / max(m["n_updates"], 1) * 1e3)
    res["update"] = {"ms_per_minibatch": round(statistics.median(per_call), 4), "min_ms": round(min(per_call), 4),
                     "max_ms": round(max(per_call), 4), "minibatches_per_call": m["n_updates"], "hip_graph": bool(m.get("hip_graph"))}

    # ---- one optimiser step alone, on the gradients the last minibatch left behind
    scaler = tr.scaler if tr.use_amp else None
    if flat is not None:
        skip = tuple(getattr(tr, "_no_grad", ()))
        res["step"] = timed(lambda: flat.step(tr.max_grad_norm, scaler, skip=skip), a.repeats)
    else:
        params = [p for p in agent.parameters() if p.requires_grad]
        for p in params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)

        def torch_calls():
            if scaler is not None:
                scaler.unscale_(tr.optimizer)
                torch.nn.utils.clip_grad_norm_(agent.parameters(), tr.max_grad_norm)
                scaler.step(tr.optimizer)
                scaler.update()
            else:
                torch.nn.utils.clip_grad_norm_(agent.parameters(), tr.max_grad_norm)
                tr.optimizer.step()

        res["step"] = timed(torch_calls, a.repeats)
        res["step"]["note"] = "gradients are clipped in place and shrink from call to call; the launches do not depend on the values"
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
