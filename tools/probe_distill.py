#!/usr/bin/env python3
"""The imitation update on one GPU: the fused loss against the same loss composed from eager torch ops, and the trainer's two phases.

    python tools/probe_distill.py [--out profiles/distill_probe.json]

Timing: HIP events around one call, 3 warm-up calls, median of ``--repeats`` with min and max, the variants alternating inside one
process (the method of tools/probe_ntuple_search.py).
  (a) loss: ``_FusedDistillLoss`` forward + backward (g2048_distill_loss: two launches, the backward hands the gradients on) against
      ``composed_loss`` (masking, log-softmax, the teacher's masked argmax / softmax, cross-entropy, entropy, the five means) forward
      + ``backward()``, on bf16 logits [M, 4] and values [M] that require grad, at ``--sizes``, tau 0 and tau 1.  The two are compared
      first (means within 1e-3 relative, gradients within bf16 resolution).
  (b) trainer: one ``collect`` lock-step and one ``update`` minibatch of ``DistillTrainer`` at ``--envs`` envs, batch ``--envs``, the
      run/train_to_2048.py model, an n-tuple teacher after ``--train-steps`` lock-steps of TC, at teacher plies 0 and ``--plies``.
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "2048-ppo-agent_amd"))

import torch  # noqa: E402

from src.ppo import DistillTrainer, NTupleActionFunction, NTupleNetwork, NTupleTrainer, PPOAgent  # noqa: E402
from src.ppo.distill import _FusedDistillLoss  # noqa: E402

MODEL = dict(observation_dim=31, action_dim=4, hidden_dim=512, d_model=256, nhead=8, num_layers=4, dim_feedforward=1024,
             dropout=0.1, reduction="cls")


def _stat(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def timed_alternating(fns: dict, repeats, warmup=3):
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


def composed_loss(logits, values, mask_bits, q, vt, tau, c_value, c_entropy):
    """The definition of g2048_distill_loss from eager torch ops -> (sums f32 [5], total)."""
    bits = torch.tensor([1, 2, 4, 8], dtype=torch.uint8, device=q.device)
    legal = (mask_bits.unsqueeze(-1) & bits) != 0
    z = torch.where(legal, logits.float(), logits.float() - 1e8)
    lp = torch.log_softmax(z, 1)
    p = lp.exp()
    ent = -(lp * p).sum(1)
    qm = torch.where(legal, q, q - 1e8)
    a = qm.argmax(1, keepdim=True)
    if tau > 0:
        pstar = torch.where(legal, ((q - q.gather(1, a)) / tau).exp(), torch.zeros_like(q))
        pstar = pstar / pstar.sum(1, keepdim=True)
    else:
        pstar = torch.zeros_like(q).scatter_(1, a, 1.0)
    ce = -torch.where(legal, pstar * lp, torch.zeros_like(lp)).sum(1)
    vl = (values.float() - vt) ** 2
    tot = ce + c_value * vl - c_entropy * ent
    agree = (z.argmax(1, keepdim=True) == a).float().reshape(-1)
    sums = torch.stack([ce.mean(), vl.mean(), (-ent).mean(), tot.mean(), agree.mean()])
    return sums, sums[3]


def loss_probe(M, tau, dev, repeats):
    g = torch.Generator(device=dev).manual_seed(M)
    logits = (2 * torch.randn(M, 4, generator=g, device=dev)).to(torch.bfloat16).requires_grad_(True)
    values = torch.randn(M, generator=g, device=dev).to(torch.bfloat16).requires_grad_(True)
    q = 100 * torch.randn(M, 4, generator=g, device=dev)
    vt = torch.randn(M, generator=g, device=dev)
    mask = torch.randint(1, 16, (M,), generator=g, device=dev).to(torch.uint8)
    sel = torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0], device=dev)

    def fused():
        logits.grad = values.grad = None
        sums, _ = _FusedDistillLoss.apply(logits, values, mask, q, vt, tau, 0.5, 0.01)
        sums.backward(sel)
        return sums.detach(), logits.grad, values.grad

    def composed():
        logits.grad = values.grad = None
        sums, tot = composed_loss(logits, values, mask, q, vt, tau, 0.5, 0.01)
        tot.backward()
        return sums.detach(), logits.grad, values.grad

    f, c = [[t.float().clone() for t in fn()] for fn in (fused, composed)]
    same = {"means_rel": float(((f[0] - c[0]).abs() / c[0].abs().clamp_min(1e-6)).max()),
            "dlogits_abs": float((f[1] - c[1]).abs().max()), "dlogits_scale": float(c[1].abs().max()),
            "dvalues_abs": float((f[2] - c[2]).abs().max())}
    return {"M": M, "tau": tau, "fused_vs_composed": same, **timed_alternating({"fused": fused, "composed": composed}, repeats)}


def trainer_probe(net, envs, plies, dev, repeats):
    torch.manual_seed(0)
    tr = DistillTrainer(PPOAgent(**MODEL), NTupleActionFunction(net, device=dev, plies=plies), envs, 16 * envs, batch_size=envs, device=dev)
    tr.collect(16)
    tr.update(2)
    out = timed_alternating({"collect_lock_step": lambda: tr.collect(1), "update_minibatch": lambda: tr.update(1)}, repeats)
    return {"envs": envs, "batch": envs, "teacher_plies": plies, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096, 16384])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--plies", type=int, default=1)
    ap.add_argument("--train-steps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_distill.py measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"command": "python tools/probe_distill.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(dev),
           "repeats": a.repeats, "timer": "HIP events around one call, 3 warm-up calls, median [min, max], the variants alternating",
           "loss": [], "trainer": []}
    for M in a.sizes:
        for tau in (0.0, 1.0):
            res["loss"].append(loss_probe(M, tau, dev, a.repeats))
            print(json.dumps(res["loss"][-1]), flush=True)
    net = NTupleNetwork(device=dev)
    nt = NTupleTrainer(net, 4096, alpha=1.0, device=dev, learner="tc")
    nt.train(a.train_steps)
    del nt
    torch.cuda.empty_cache()
    for plies in sorted({0, a.plies}):
        res["trainer"].append(trainer_probe(net, a.envs, plies, dev, a.repeats))
        print(json.dumps(res["trainer"][-1]), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
