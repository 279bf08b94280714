#!/usr/bin/env python3
"""Cost of one lock-step of one-ply expectimax play next to a greedy lock-step, on one GPU.

    python tools/probe_lookahead.py [--agent state_dict.pt] [--boards 100 65536] [--repeats 7] [--out result.json]
    python tools/probe_lookahead.py --plies 2 [--no-dedup] [--boards 100 4096] ...

For each batch size: boards that the agent's own greedy play visits (half an episode's worth of lock-steps into a rollout, so the
fill of the boards is that of real play), then, with HIP events after a warm-up, the time of
  greedy     TorchActionFunction.policy_fn (bf16, the fused encoder for a default-shape agent)
  lookahead  LookaheadActionFunction.policy_fn on the same boards (same precision, same encoder on every child)
and of the parts of the lookahead lock-step: the three new kernels, the prefix sum with its host read, the value forward.
``--plies 2`` times the two-ply lock-step (ExpectimaxActionFunction, one slice of roots) and each of its parts instead: both
expands, the dedup kernel, both prefix sums with their host reads, both children launches, the value forward, both reduces and
the backup, with ``rows`` (value-forward rows) and ``rows_full`` (the rows without dedup); ``--no-dedup`` skips the dedup launch.
``--symmetry ensemble`` (or ``canonical``) puts the timed action functions into that mode (the boards are still those of plain
greedy play): under "ensemble" every forward runs on eight views of its rows, ``children`` / ``rows`` keep counting boards.
Every figure is the median of ``--repeats`` timed repeats with the min and max next to it.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "2048-ppo-agent_amd"))

import torch  # noqa: E402

from src.g2048 import native as nv  # noqa: E402
from src.ppo import ExpectimaxActionFunction, LookaheadActionFunction, PPOAgent, TorchActionFunction  # noqa: E402
from src.ppo.lookahead import expand, expand_level, scan, spawn_children  # noqa: E402
from src.runs import BatchRunner  # noqa: E402

MODEL = dict(observation_dim=31, action_dim=4, hidden_dim=512, d_model=256, nhead=8, num_layers=4, dim_feedforward=1024,
             dropout=0.1, reduction="cls")


def timed(fn, repeats, warmup=3):
    """-> {"median_ms", "min_ms", "max_ms"} of ``repeats`` event-timed calls after ``warmup`` untimed ones."""
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


def mid_game_boards(agent, B, dev, steps=96):
    """The boards after ``steps`` greedy lock-steps of a fresh batch (boards that ended earlier stay in, as they do in a rollout)."""
    fn = TorchActionFunction(agent, use_mask=True, sample_actions=False, device=dev, amp_dtype=torch.bfloat16)
    eng = BatchRunner(init_seed=7, act_fn=fn, device=dev)._engine
    traj = eng.rollout_policy_fixed(B, steps, fn.policy_fn, use_mask=True, sample=False)
    return traj.boards[steps - 1].contiguous()


def probe(agent, B, dev, repeats, symmetry="none"):
    boards = mid_game_boards(agent, B, dev)
    greedy = TorchActionFunction(agent, use_mask=True, sample_actions=False, device=dev, amp_dtype=torch.bfloat16, symmetry=symmetry)
    look = LookaheadActionFunction(agent, device=dev, amp_dtype=torch.bfloat16, symmetry=symmetry)
    res = {"boards": B, "symmetry": symmetry, "fused_encoder": look._fused is not None,
           "greedy": timed(lambda: greedy.policy_fn(boards, None), repeats),
           "lookahead": timed(lambda: look.policy_fn(boards, None), repeats)}
    N = look.last_children
    res["children"] = N
    res["children_per_board"] = round(N / B, 2)
    # the parts, on the tensors of one expansion
    after, reward, nchild, offset, _ = expand_level(boards)
    children, terminal = spawn_children(after, nchild, offset, N)
    values = look.values(children)
    q = torch.empty_like(reward)
    parts = {"expand": timed(lambda: nv.lookahead_expand(boards, after, reward, nchild), repeats),
             "scan_and_host_read": timed(lambda: int(scan(nchild)[1][-1].item()), repeats),
             "children": timed(lambda: nv.lookahead_children(after, nchild, offset, N, children, terminal), repeats),
             "value_forward": timed(lambda: look.values(children), repeats),
             "reduce": timed(lambda: nv.lookahead_reduce(reward, nchild, offset, values, terminal, look.gamma, N, q), repeats)}
    res["parts"] = parts
    kernels = sum(parts[k]["median_ms"] for k in ("expand", "children", "reduce"))
    res["new_kernels_ms"] = round(kernels, 4)
    res["new_kernels_share_of_lockstep"] = round(kernels / res["lookahead"]["median_ms"], 4)
    res["lookahead_over_greedy"] = round(res["lookahead"]["median_ms"] / res["greedy"]["median_ms"], 2)
    # expand 16 r + 96 w; children 64 + 32 r + 17 w per child; reduce 48 r + 5 r per child + 16 w
    res["bytes_per_board_new_kernels"] = round(272 + 22 * N / B, 1)
    return res


def probe2(agent, B, dev, repeats, dedup, symmetry="none"):
    """The two-ply lock-step and its parts on the tensors of one expansion (a single slice of roots)."""
    boards = mid_game_boards(agent, B, dev)
    fn = ExpectimaxActionFunction(agent, plies=2, dedup=dedup, device=dev, amp_dtype=torch.bfloat16, symmetry=symmetry)
    res = {"boards": B, "symmetry": symmetry, "dedup": dedup, "fused_encoder": fn._fused is not None,
           "lockstep": timed(lambda: fn.policy_fn(boards, None), repeats)}
    res["rows"], res["rows_full"] = fn.last_children, fn.last_children_full
    res["rows_over_rows_full"] = round(fn.last_children / max(fn.last_children_full, 1), 4)
    i32, f32 = torch.int32, torch.float32
    after1, reward1, nchild1, offset1, incl1 = expand_level(boards)
    N1 = int(incl1[-1].item())
    if N1 > fn.max_children:
        raise SystemExit(f"{B} boards have {N1} level-1 children: more than one slice of {fn.max_children}; probe a smaller batch")
    res["level1_children"] = N1
    children1, terminal1 = spawn_children(after1, nchild1, offset1, N1)
    after2, reward2, nchild2 = expand(children1)
    group_start = torch.cat([offset1[:, 0] * 4, torch.tensor([4 * N1], dtype=i32, device=dev)]).to(i32)
    rep = torch.arange(4 * N1, dtype=i32, device=dev).view(N1, 4)
    nuniq = nchild2.clone()
    if dedup:
        nv.lookahead_dedup(after2, nchild2, group_start, rep, nuniq)
    offset2, incl2 = scan(nuniq)
    N2 = int(incl2[-1].item())
    assert N2 == fn.last_children
    children2, terminal2 = spawn_children(after2, nuniq, offset2, N2)
    values = fn.values(children2)
    zero2 = torch.zeros_like(reward2)
    e = torch.empty((N1, 4), dtype=f32, device=dev)
    v1 = torch.empty(N1, dtype=f32, device=dev)
    q2 = torch.empty((B, 4), dtype=f32, device=dev)

    def scan2():
        c = scan(nuniq)[1]
        return torch.stack((c[-1], nchild2.sum(dtype=i32))).tolist() if dedup else int(c[-1].item())

    parts = {"expand1": timed(lambda: nv.lookahead_expand(boards, after1, reward1, nchild1), repeats),
             "scan1_and_host_read": timed(lambda: scan(nchild1)[1][3::4].tolist(), repeats),
             "children1": timed(lambda: nv.lookahead_children(after1, nchild1, offset1, N1, children1, terminal1), repeats),
             "expand2": timed(lambda: nv.lookahead_expand(children1, after2, reward2, nchild2), repeats)}
    if dedup:
        parts["dedup"] = timed(lambda: nv.lookahead_dedup(after2, nchild2, group_start, rep, nuniq), repeats)
    parts.update({
        "scan2_and_host_read": timed(scan2, repeats),
        "children2": timed(lambda: nv.lookahead_children(after2, nuniq, offset2, N2, children2, terminal2), repeats),
        "value_forward": timed(lambda: fn.values(children2), repeats),
        "reduce2": timed(lambda: nv.lookahead_reduce(zero2, nuniq, offset2, values, terminal2, fn.gamma, N2, e), repeats),
        "backup": timed(lambda: nv.lookahead_backup(reward2, nchild2, rep, e, v1), repeats),
        "reduce1": timed(lambda: nv.lookahead_reduce(reward1, nchild1, offset1, v1, terminal1, fn.gamma, N1, q2), repeats)})
    res["parts"] = parts
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agent", default=None, help="state_dict of a default-shape PPOAgent (run/train_to_2048.py --save-agent); default: fresh weights")
    ap.add_argument("--boards", type=int, nargs="+", default=[100, 65536])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--plies", type=int, default=1, choices=[1, 2], help="2: the two-ply lock-step and its parts")
    ap.add_argument("--no-dedup", action="store_true", help="with --plies 2: value every afterstate's children")
    ap.add_argument("--symmetry", default="none", choices=["none", "canonical", "ensemble"], help="mode of the timed action functions")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_lookahead.py measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(a.seed)
    agent = PPOAgent(**MODEL)
    if a.agent:
        agent.load_state_dict(torch.load(a.agent, map_location="cpu"))
    agent = agent.to(dev).eval()
    res = {"agent": os.path.basename(a.agent) if a.agent else "fresh weights", "precision": "bfloat16", "repeats": a.repeats,
           "timer": "HIP events around one policy_fn call, 3 warm-up calls, median [min, max]",
           "plies": a.plies,
           "runs": [probe(agent, B, dev, a.repeats, a.symmetry) if a.plies == 1 else probe2(agent, B, dev, a.repeats, not a.no_dedup, a.symmetry)
                    for B in a.boards]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
