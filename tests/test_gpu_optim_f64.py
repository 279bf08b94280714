"""g2048_opt_step, g2048_lamb_step (csrc/g2048_optim.hip) and g2048_reduce_jobs (csrc/g2048_reduce.hip) against the stage references of
tests/optim_ref.py: the norm partials and their total within derived summation bounds (exact on integer gradients), the per-group
constants within one f32 rounding, every element of the parameters, both moments and all four shadow layouts bit for bit against the
f32 restatement of the kernels' arithmetic, the trust ratio per tensor from the kernel's own sums, the scaler's bookkeeping, and every
word that no stage owns untouched.  The kernels are driven through nv.opt_chunk_table / nv.opt_step / nv.lamb_step / nv.reduce_jobs with
hand-built parameter sets: every parameter, shadow, flat buffer, the workspace and the scalars are slices of two NaN-patterned arenas
(optim_ref.Layout), so a store outside its tensor, into a padding element or on a skipped step fails U1.  No trainer, no agent.
tests/test_optim_ref.py holds the same rules to an f32 emulation and to planted defects, at the same cases.

Cases (optim_ref.CASES, three steps each unless the case says otherwise, AdamW and LAMB): the parameter set SMALL ([64][256], [32][512],
[32][1024] with all four shadows, tiled at R = 8, 4, 2; [4][512]; [1][512]; [64][128] R = 16; [32][2048] R = 1; [12][256] rows % 8 != 0 plus a
ragged chunk; [41][300]; [7][3]; 1-D 1, 41, 2050, 2051; [16][512] with a dense shadow at 4-byte and a transposed one at 8-byte alignment:
one 8-byte aligned shadow cannot fail both conditions, the dense address of a float4 is always a multiple of 8 bytes from its base) in
four interleaved groups, at scales 1024, none, 2^60, 2^-10 and 1000 (not a power of two: the order of unscale and clip shows), trainer clip
0.5 / 4 / off and LAMB's clip 1 / off with norms on both sides, integer gradients, a table that skips two tensors, all-zero gradients,
t = 5000, one group, the set plus a 1-D tensor of 260 chunks (350 chunks: the strided sum of the partials takes a second pass), and single
tensors of 1, 255, 256 and 257 chunks.  Then the scaler sequence and the NaN step of optim_ref, and g2048_reduce_jobs over 150 jobs.

Measured on the MI355X (42 tests, 6 s in all, the slowest 0.4 s): every exact stage (the cast fields of D1, A1, L1, L3, L4, S1, U1, K1 and
the integer tier of N1, N2, R1) is bit-equal, f32 division and sqrtf included; worst error / bound of the bounded stages: N1 0.20, N2 0.009,
L2 pn 0.14, un 0.21, R1 0.23.

Every test records the largest error / bound of its bounded stages (N1, N2, L2, R1; must stay <= 1, the bounds are derived in
tests/optim_ref.py) and dumps them as JSON when G2048_OPTIM_F64_OUT names a file; profiles/optim_f64_figures.json holds one such run.
"""
import json
import os

import numpy as np
import pytest
import torch

import optim_ref as orf

pytestmark = pytest.mark.gpu
_FIG = {}


def _record(test, fig):
    _FIG[test] = {k: round(v, 4) for k, v in sorted(fig.items())}
    print("OPTFIG " + json.dumps({test: _FIG[test]}))
    assert all(v <= 1.0 for v in fig.values()), fig
    out = os.environ.get("G2048_OPTIM_F64_OUT")
    if out:
        with open(out, "w") as fh:
            json.dump(_FIG, fh, indent=1, sort_keys=True)


def _upload(mem, dev):
    F = torch.from_numpy(mem.f.view(np.int32).copy()).to(dev)
    H = torch.from_numpy(mem.h.view(np.int16).copy()).to(dev)
    return F, H


def _download(mem, F, H):
    torch.cuda.synchronize()
    mem.f[:] = F.cpu().numpy().view(np.uint32)
    mem.h[:] = H.cpu().numpy().view(np.uint16)


def gpu_step(L, mem, hp, dev=None):
    """One g2048_opt_step / g2048_lamb_step on the arenas of ``mem``."""
    from src.g2048 import native as nv

    F, H = _upload(mem, dev)
    Ff, Hb = F.view(torch.float32), H.view(torch.bfloat16)
    assert F.data_ptr() % 256 == 0 and H.data_ptr() % 256 == 0
    params, offsets, groups, shadows = [], [], [], {}
    for p in L.params:
        if p.skip:
            continue
        t = Ff[p.off:p.off + p.n].view(p.shape)
        shapes = (p.shape, p.shape[::-1], (p.n,), (p.n,))
        sh = tuple(None if o is None else Hb[o:o + p.n].view(s) for o, s in zip(p.sh, shapes))
        params.append(t)
        offsets.append(p.flat)
        groups.append(p.group)
        shadows[id(t)] = sh
    table = nv.opt_chunk_table(params, offsets, groups, dev, shadows)
    assert table.numel() == L.nc * nv.OPT_CHUNK_BYTES
    flat = lambda off: Ff[off:off + L.flat_len]
    sc = hp.get("scaler")
    scale, tracker = (Ff[L.scale:L.scale + 1], F[L.tracker:L.tracker + 1]) if sc else (None, None)
    growth, backoff, interval = (sc["growth"], sc["backoff"], sc["interval"]) if sc else (2.0, 0.5, 2000)
    ws, steps, info = Ff[L.ws:L.ws + L.ws_len], Ff[L.steps:L.steps + L.n_steps], Ff[L.info:L.info + 2]
    if L.lamb:
        assert L.ws_len == nv.load().g2048_lamb_workspace_floats(L.nc)
        nv.lamb_step(table, L.nc, flat(L.grads), flat(L.m), flat(L.v), hp["groups"], hp["max_norm"], hp["lamb_max"], steps, scale, tracker,
                     growth, backoff, interval, ws, info)
    else:
        assert L.ws_len == nv.load().g2048_opt_workspace_floats(L.nc)
        nv.opt_step(table, L.nc, flat(L.grads), flat(L.m), flat(L.v), hp["groups"], hp["max_norm"], steps, scale, tracker, growth, backoff,
                    interval, ws, info)
    _download(mem, F, H)


@pytest.mark.parametrize("lamb", (False, True), ids=("adamw", "lamb"))
@pytest.mark.parametrize("c", orf.CASES, ids=lambda c: c["id"])
def test_every_stage(dev, c, lamb):
    fig, state = {}, {}
    failures = orf.run_case(c, lamb, gpu_step, fig, state=state, dev=dev)
    if c["zero"] and not lamb:
        failures += orf.zero_gradient_check(state, orf.ADAMW_GROUPS)
    assert not failures, failures
    _record(f"{'lamb' if lamb else 'adamw'}:{c['id']}", fig)


@pytest.mark.parametrize("lamb", (False, True), ids=("adamw", "lamb"))
def test_scaler_sequence(dev, lamb):
    """K1: growth after the third clean step, backoff on inf, on a NaN in the scalar tail of the last chunk and on finite gradients whose
    squares overflow the f32 sum; a skipped step leaves p, m, v, the shadows and steps as they were (U1)."""
    fig = {}
    failures = orf.run_scaler_sequence(lamb, gpu_step, fig, dev=dev)
    assert not failures, failures
    _record(f"{'lamb' if lamb else 'adamw'}:scaler_sequence", fig)


@pytest.mark.parametrize("lamb", (False, True), ids=("adamw", "lamb"))
def test_nan_gradient_without_a_scaler_steps(dev, lamb):
    failures = orf.run_nan_without_scaler(lamb, gpu_step, dev=dev)
    assert not failures, failures


@pytest.mark.parametrize("lamb", (False, True), ids=("adamw", "lamb"))
def test_two_runs_give_identical_bits(dev, lamb):
    c = orf.CASES[0]
    runs = []
    for _ in range(2):
        L = orf.Layout(c["specs"], lamb)
        mem, hp = L.mem(), orf.hyper(c, lamb)
        orf.init_state(L, mem, c)
        for s in range(2):
            orf.set_grads(L, mem, c, s)
            gpu_step(L, mem, hp, dev)
        runs.append(mem)
    assert (runs[0].f == runs[1].f).all() and (runs[0].h == runs[1].h).all()


@pytest.mark.parametrize("tier_a", (True, False), ids=("tierA", "tierB"))
def test_reduce_jobs(dev, tier_a):
    """R1 over every (parts, n) of optim_ref.R_PARTS x R_NS and the named jobs, more than two launches' worth of jobs in one call; canaried
    destinations and sources; a second call gives identical bits."""
    from src.g2048 import native as nv

    mem, jobs = orf.reduce_jobs_problem(tier_a)
    assert len(jobs) > 2 * nv.CONSTANTS["G2048_REDUCE_MAX_JOBS"]
    F, H = _upload(mem, dev)
    Ff, Hb = F.view(torch.float32), H.view(torch.bfloat16)
    recs = []
    for J in jobs:
        size = (J["parts"] - 1) * J["stride"] + J["n"]
        src = (Hb if J["kind"] == "bf16" else Ff)[J["src"]:J["src"] + size]
        recs.append((src, Ff[J["dst"]:J["dst"] + J["n"]], J["stride"], J["n"], J["parts"], J["tr"]))
    nv.reduce_jobs(recs)
    after = mem.copy()
    _download(after, F, H)
    fig = {}
    failures = orf.reduce_check(mem, after, jobs, tier_a, fig)
    assert not failures, failures
    nv.reduce_jobs(recs)
    again = mem.copy()
    _download(again, F, H)
    assert (again.f == after.f).all() and (again.h == after.h).all()
    _record(f"reduce_jobs:{'tierA' if tier_a else 'tierB'}", fig)
