"""The block shapes of the grouped weight-gradient launch (k_dweight_jobs, csrc/g2048_dweight.hip) against the float64 references of
tests/gemm_ref.py: [256 x 256] blocks (wave tile 64 x 128, 32-token stages), [128 x 128] blocks (wave tile 32 x 64, 64-token stages) and
every way the two share a job.

One launch holds each (N, K) of NK twice: bf16 partials with column sums, then f32 partials (column sums on every other one).  A job
whose N and K are multiples of 256 is cut into [256 x 256] cells; ``big_cells`` deals that many cells, in job order, to the
[256 x 256] shape and leaves the rest to [128 x 128] blocks.  The jobs have 1, 3, 4, 4, 1, 3, 4, 4 cells, so PLANS gives:

    0     every block [128 x 128]
    6     jobs 0, 1 whole; job 2 (1024 x 256, bf16) 2 of 4 cells: rows 512.. and their column sums come from [128 x 128] blocks
    10    job 3 (256 x 1024, bf16) 2 of 4 cells: the column sums come from the [256 x 256] block of column block 0 alone
    14    job 5 (768 x 256, f32) 1 of 3 cells
    19    job 6 (1024 x 256, f32) 3 of 4 cells
    23    job 7 (256 x 1024, f32) 3 of 4 cells
    1000  every block [256 x 256] (the f32 partials leave in two passes of 128 rows)
    -1    the entry point's own choice for the device

T = 8 slices x {64, 128, 320} tokens.  T = 512 is the smallest the entry point takes: one 64-token stage per slice for the [128 x 128]
blocks (prologue only), two 32-token stages for the [256 x 256] blocks.  T = 1024: 2 and 4 stages (4 is the first count at which a
[256 x 256] block fetches inside its loop and waits with two younger stages in flight).  T = 2560: 5 and 10 stages, every wait of both
shapes and buffers reused.

Tier A (small-integer operands, every partial sum exact in f32): every partial and every per-slice column sum of every plan is BIT
EQUAL to the rounded float64 result, so the plans are bit-identical to each other.  Tier B (realistic ranges): the per-element bound of
gemm_ref.bound that tests/test_gpu_gemm.py::test_dweight_tier_b holds the kernel to (half a bf16 unit plus the any-order f32 summation
bound over the slice's tokens; the summation term alone for f32 outputs), and the whole-tensor 4e-3.  Outputs and operands live in the
NaN-patterned guard buffers of tests/test_gpu_gemm.py: a write outside an output or a read outside an operand fails the case.
"""
import pytest
import torch

import gemm_ref as gr
from test_gpu_gemm import BF16, F32, Guarded, _operand

pytestmark = pytest.mark.gpu
S = 8
NK = ((256, 256), (768, 256), (1024, 256), (256, 1024))
# (N, K, f32 partials, column sums)
JOBS = tuple((N, K, False, True) for N, K in NK) + tuple((N, K, True, i % 2 == 0) for i, (N, K) in enumerate(NK))
PLANS = (0, 6, 10, 14, 19, 23, 1000, -1)
T_LIST = (512, 1024, 2560)
_cache = {}


def _case(dev, T, tier):
    """Operands (device views into guard buffers) and float64 references per (N, K), computed once per (T, tier)."""
    key = (T, tier)
    if key not in _cache:
        case = {}
        for N, K in NK:
            dy, x = (t.to(dev) for t in (gr.tier_a_dweight(T, N, K, S, tag=7) if tier == "a" else gr.tier_b_dweight(T, N, K, tag=7)))
            parts, cs = gr.dweight(dy, x, S)
            mag, cmag = gr.dweight(dy.abs(), x.abs(), S)
            if tier == "a":
                gr.assert_exact(mag)
                gr.assert_exact(cmag)
                gr.assert_exercises_rounding(parts)
            case[(N, K)] = dict(dy=_operand(dev, dy), x=_operand(dev, x, g=2, col0=16), parts=parts, cs=cs, mag=mag, cmag=cmag)
        _cache[key] = case
    return _cache[key]


def _launch(dev, case, plan):
    from src.g2048 import native as nv

    bufs, jobs = [], []
    for N, K, f32_parts, colsums in JOBS:
        pg, cg = Guarded(dev, S * N, K, F32 if f32_parts else BF16), Guarded(dev, S, N, F32) if colsums else None
        c = case[(N, K)]
        jobs.append((c["dy"], c["x"], pg.view.view(S, N, K), None if cg is None else cg.view))
        bufs.append((pg, cg))
    nv.dweight_jobs(jobs, big_cells=plan)
    return [(pg.take(f"plan {plan} job {i}: parts").view(S, JOBS[i][0], JOBS[i][1]),
             None if cg is None else cg.take(f"plan {plan} job {i}: column sums")) for i, (pg, cg) in enumerate(bufs)]


def test_plans_cover_every_shape_and_mix():
    """PLANS does what the docstring says (host arithmetic, no launch)."""
    from src.g2048 import native as nv

    shapes = [(N, K, S) for N, K, _, _ in JOBS]
    cells = [1, 3, 4, 4, 1, 3, 4, 4]
    assert nv.dweight_jobs_plan(shapes, 0) == [0] * 8 and nv.dweight_jobs_plan(shapes, 1000) == cells
    mixed = set()
    for plan in PLANS[1:6]:
        n_big = nv.dweight_jobs_plan(shapes, plan)
        assert sum(n_big) == plan
        mixed |= {i for i, (b, c) in enumerate(zip(n_big, cells)) if 0 < b < c}
    assert mixed == {2, 3, 5, 6, 7}


@pytest.mark.parametrize("T", T_LIST)
def test_tier_a_every_plan_bit_equal(dev, T):
    case = _case(dev, T, "a")
    failures = []
    for plan in PLANS:
        for i, (got, cs) in enumerate(_launch(dev, case, plan)):
            N, K, f32_parts, _ = JOBS[i]
            c = case[(N, K)]
            what = f"plan {plan} job {i} {JOBS[i]}"
            failures += gr.accept_exact(got, c["parts"] if f32_parts else gr.bf16_rne(c["parts"]), what + ": parts")
            if cs is not None:
                failures += gr.accept_exact(cs, c["cs"], what + ": column sums")
    assert not failures, failures


@pytest.mark.parametrize("T", T_LIST)
def test_tier_b_every_plan_within_the_bound(dev, T):
    case = _case(dev, T, "b")
    L = T // S
    failures, first = [], None
    for plan in PLANS:
        outs, fig = _launch(dev, case, plan), {}
        for i, (got, cs) in enumerate(outs):
            N, K, f32_parts, _ = JOBS[i]
            c = case[(N, K)]
            what = f"plan {plan} job {i} {JOBS[i]}"
            failures += gr.accept_bound(got, c["parts"], gr.bound(c["parts"], c["mag"], L, half_ulp=not f32_parts), what + ": parts", fig)
            if cs is not None:
                failures += gr.accept_bound(cs, c["cs"], gr.bound(c["cs"], c["cmag"], L, half_ulp=False), what + ": column sums", fig)
            whole = gr.rel(got.double().sum(0), c["parts"].sum(0))
            if not whole < gr.REL_LIMIT:
                failures.append(f"{what}: sum of the parts, whole-tensor error {whole:.3e}")
        print("DWRETILE", dict(T=T, plan=plan, worst_error_over_bound=max(v["ratio"] for v in fig.values())))
        # the same tokens in the same 16-token steps whatever the block shape: the plans agree bit for bit on any operands
        if first is None:
            first = outs
        else:
            for i, ((g0, c0), (g1, c1)) in enumerate(zip(first, outs)):
                if not torch.equal(g0, g1) or (c0 is not None and not torch.equal(c0, c1)):
                    failures.append(f"plan {plan} job {i} {JOBS[i]}: differs from plan {PLANS[0]}")
    assert not failures, failures
