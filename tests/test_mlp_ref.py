"""tests/mlp_ref.py held to itself on the CPU: every tier-A generator meets its preconditions at every cell that
tests/test_gpu_mlp_f64.py runs (the cell lists are mlp_ref's), a straightforward f32 emulation of each kernel of csrc/g2048_mlp.hip is
bit-equal in tier A and within the tier-B bound, and every planted defect - the slips a kernel of this kind makes - is rejected by the
acceptance rule of the GPU test, in tier A, at the smallest cell that can show it.

Worst error / bound of the emulations in tier B (printed by the tests below as MLPFIG lines; a report, no threshold):
    embed y            0.991   (M 2051; the f32 sum in the kernel's order IS the emulation: mlp_ref.embed_f32_ordered)
    gemm job y         0.988   (M 2051, K 64, N 512, bias + ReLU; 64-wide K chunks, 280 cells over the seven epilogues)
    out_fwd logits     0.0015  values 0.0012   (M 2051; the summation term alone, n = 512)
    out_bwd dh2        0.992   (actor half, n = 4, M 2051)   0.985 (critic half, n = 1, M 300)
    out_bwd partial    0.190   (M 2051; the summation term alone, n = 8)
The bf16 outputs sit where the GEMM suite's do (0.95-0.98: the half unit in the last place dominates), the f32 outputs far below 1.
"""
import json

import pytest
import torch

import gemm_ref as gr
import mlp_ref as mr

BF16, F32, F64 = gr.BF16, gr.F32, gr.F64
D = mr.D


def _fig(kernel, **kw):
    print("MLPFIG " + json.dumps(dict(kernel=kernel, **kw)))


# ---------------------------------------------------------------------------------------------------------- emulations
def emu_embed(boards, wt, bias, clamp=True, onehot_ones=True):
    """-> (y bf16, one-hot matrix bf16) as k_mlp_embed_fwd computes them.  ``clamp`` False: an exponent above 30 indexes past its
    cell's 31 rows (the next cell's rows; past the table: zeros here, whatever lies there on the GPU)."""
    if clamp:
        y, idx = mr.embed_f32_ordered(boards, wt, bias), mr._classes(boards)
    else:
        idx = boards.long() + mr.CLASSES * torch.arange(mr.CELLS)
        w32 = torch.cat([wt.to(F32), torch.zeros(256, D)])
        acc = bias.to(F32).expand(boards.shape[0], D).clone()
        for c in range(mr.CELLS):
            acc = acc + w32[idx[:, c]]
        y = torch.clamp_min(acc, 0.0).to(BF16)
    oh = torch.zeros(boards.shape[0], 1024)
    oh.scatter_(1, idx, 1.0)
    oh = oh[:, :D]
    if onehot_ones:
        oh[:, mr.ONES_COL] = 1.0
    return y, oh.to(BF16)


def emu_gemm(segs, bias=None, relu=False, act=None, drop_chunk=None, cross_weights=False, bias_after_relu=False, bf16_between=False,
             minus_zero_active=False):
    """f32 emulation of one job of k_gemm_jobs: the accumulator starts at the bias, takes the K chunks of 64 of segment 0, then of
    segment 1; ReLU; mask; one rounding.  Defects: ``drop_chunk`` (that chunk number is never multiplied), ``cross_weights`` (segment 1
    meets segment 0's weights), ``bias_after_relu``, ``bf16_between`` (the accumulator rounded to bf16 between the segments, or
    before the bias when there is one segment), ``minus_zero_active`` (the mask tests the 16 bits, not the low 15)."""
    M, N = segs[0][0].shape[0], segs[0][1].shape[0]
    late_bias = bias is not None and (bias_after_relu or (bf16_between and len(segs) == 1))
    acc = torch.zeros(M, N) if bias is None or late_bias else bias.to(F32).expand(M, N).clone()
    c = 0
    for s, (x, w) in enumerate(segs):
        if s == 1 and cross_weights:
            w = segs[0][1][:, :x.shape[1]]
        if s == 1 and bf16_between:
            acc = acc.to(BF16).float()
        for k0 in range(0, x.shape[1], 64):
            if c != drop_chunk:
                acc = acc + x[:, k0:k0 + 64].float() @ w[:, k0:k0 + 64].float().t()
            c += 1
    if late_bias and not bias_after_relu:
        acc = acc.to(BF16).float() + bias
    if relu:
        acc = torch.clamp_min(acc, 0.0)
    if late_bias and bias_after_relu:
        acc = acc + bias
    if act is not None:
        on = act.view(torch.int16) != 0 if minus_zero_active else mr.active(act)
        acc = torch.where(on, acc, torch.zeros(()))
    return acc.to(BF16)


def emu_out_fwd(h2, w3, value_from_actor=False):
    """k_mlp_out_fwd: lane part p of a row's 16 takes elements p + 16 i, i = 0..31, as one chain of fused multiply-adds (bf16 x bf16
    is exact in f32: an add of the product rounds the same), then the xor tree over the 16 parts."""
    M = h2.shape[0]
    a, c = h2[:, :D].float().view(M, 32, 16), h2[:, (0 if value_from_actor else D):][:, :D].float().view(M, 32, 16)
    w = w3.float().view(5, 32, 16)
    s = torch.zeros(M, 5, 16)
    for i in range(32):
        for o in range(5):
            s[:, o] = s[:, o] + (a if o < 4 else c)[:, i] * w[o, i]
    lanes = torch.arange(16)
    for m in (8, 4, 2, 1):
        s = s + s[:, :, lanes ^ m]
    return s[:, :4, 0].contiguous(), s[:, 4, 0].contiguous()


def emu_out_bwd(dlogits, dvalues, h2, w3, round_d=True, leak_row=False, skip_masked=False):
    """k_mlp_out_bwd: the gradients rounded to bf16, four chained multiply-adds per actor element and one product per critic element
    (all products exact in f32), one rounding, zero where h2 is +-0; partial sums over ascending rows of 8-row blocks.  Defects:
    ``round_d`` False, ``leak_row`` (the last block also adds the row the clamped index re-reads: row M - 1 again), ``skip_masked``
    (masked elements keep what the buffer held: a NaN)."""
    M = h2.shape[0]
    d = torch.cat([dlogits, dvalues.view(M, 1)], 1)
    if round_d:
        d = d.to(BF16).float()
    h, w = h2.float(), w3.float()
    ga = torch.zeros(M, D)
    for o in range(4):
        ga = ga + d[:, o:o + 1] * w[o]
    dh2 = torch.cat([ga, d[:, 4:] * w[4]], 1).to(BF16)
    dh2 = torch.where(mr.active(h2), dh2, torch.full((), float("nan") if skip_masked else 0.0, dtype=BF16))
    blocks = (M + 7) // 8
    partial = torch.zeros(blocks, 5, 2 * D)
    for r in range(M + (1 if leak_row and M % 8 else 0)):
        rr = min(r, M - 1)
        partial[r // 8] = partial[r // 8] + d[rr].view(5, 1) * h[rr]
    return dh2, torch.cat([partial[:, :4, :D], partial[:, 4:, D:]], 1)


# ---------------------------------------------------------------------------------------------------------- preconditions at every GPU cell
@pytest.mark.parametrize("M", mr.EMBED_M)
def test_embed_generator_and_emulation(M):
    boards, wt, bias = mr.tier_a_embed(M)
    assert boards.max() == 255 and (M < 2 or set(range(18, 31)) <= set(boards.flatten().tolist()))
    assert M < 7 or all(bool((boards[:, 15] == v).any()) for v in (31, 32, 255))
    want, want_oh = mr.expect_a_embed(boards, wt, bias)
    y, oh = emu_embed(boards, wt, bias)
    assert not gr.accept_exact(y, want, "y") and not gr.accept_exact(oh, want_oh, "onehot")
    assert oh.float().sum(1).eq(17).all() and oh[:, 497:].float().abs().sum() == 0
    boards, wt, bias = mr.tier_b_embed(M)
    assert abs(wt.float().mean().item()) > 0.015
    pre, ref, _ = mr.embed(boards, wt, bias)
    fig = {}
    assert not gr.accept_bound(emu_embed(boards, wt, bias)[0], ref, gr.bound(pre, mr.embed_mag(boards, wt, bias), 17), "y", fig)
    _fig("embed", M=M, fig=fig)


@pytest.mark.parametrize("m", range(len(mr.GEMM_M)))
@pytest.mark.parametrize("e", range(len(mr.EPILOGUES)))
def test_gemm_generator_and_emulation(e, m):
    bias, relu, act = mr.EPILOGUES[e]
    for M, ks, N in mr.gemm_cells(e, m):
        segs, b, a, want = mr.tier_a_gemm_case(M, ks, N, bias, relu, act)
        assert not gr.accept_exact(emu_gemm(segs, b, relu, a), want, f"y {M, ks, N}")
        segs, b, a = mr.tier_b_gemm(M, ks, N, bias, act)
        pre, ref = mr.gemm_job(segs, b, relu, a)
        fig = {}
        assert not gr.accept_bound(emu_gemm(segs, b, relu, a), ref, gr.bound(pre, mr.gemm_mag(segs, b), sum(ks)), "y", fig)
        _fig("gemm_jobs", M=M, K=ks, N=N, epilogue=mr.EPILOGUES[e], fig=fig)


@pytest.mark.parametrize("M", mr.LAUNCH_M)
def test_launch_form_generators(M):
    case = mr.tier_a_launch_forms(M)
    fwd, bwd, two, cls = mr.expect_a_launch_forms(case)
    x, wa, ba, wc, bc = case["fwd"]
    assert not gr.accept_exact(torch.cat([emu_gemm([(x, wa)], ba, True), emu_gemm([(x, wc)], bc, True)], 1), fwd, "fwd")
    xa, wa, aa, xc, wc, ac = case["bwd"]
    assert not gr.accept_exact(emu_gemm([(xa, wa), (xc, wc)], act=aa), two, "two segments")
    assert gr.accept_exact(emu_gemm([(xa, wa), (xc, wc)], act=ac), two, "two segments")  # the neighbouring job's mask


@pytest.mark.parametrize("M", mr.EIGHT_JOBS_M)
def test_eight_job_generators(M):
    assert len(mr.EIGHT_JOBS) == 8 and len({(ks, N) for ks, N, _ in mr.EIGHT_JOBS}) == 8
    for ks, N, e in mr.EIGHT_JOBS:
        bias, relu, act = mr.EPILOGUES[e]
        segs, b, a, want = mr.tier_a_gemm_case(M, ks, N, bias, relu, act)
        assert not gr.accept_exact(emu_gemm(segs, b, relu, a), want, f"y {ks, N, e}")


def test_gemm_cells_cover_every_value_with_every_epilogue():
    pairs = set()
    for e in range(len(mr.EPILOGUES)):
        cells = [c for m in range(len(mr.GEMM_M)) for c in mr.gemm_cells(e, m)]
        assert {c[0] for c in cells} == set(mr.GEMM_M) and {c[1] for c in cells} == set(mr.GEMM_K) and {c[2] for c in cells} == set(mr.GEMM_N)
        assert {(c[0], c[2]) for c in cells} == {(M, N) for M in mr.GEMM_M for N in mr.GEMM_N}
        pairs |= {(c[0], c[1]) for c in cells}
    assert len(pairs) == len(mr.GEMM_M) * len(mr.GEMM_K)


@pytest.mark.parametrize("M", mr.OUT_FWD_M)
def test_out_fwd_generator_and_emulation(M):
    h2, w3 = mr.tier_a_out_fwd(M)
    logits, values = mr.expect_a_out_fwd(h2, w3)
    lo, va = emu_out_fwd(h2, w3)
    assert not gr.accept_exact(lo, logits, "logits") and not gr.accept_exact(va, values, "values")
    h2, w3, _, _ = mr.tier_b_out(M)
    (logits, values), (ml, mv) = mr.out_fwd(h2, w3), mr.out_fwd(h2.abs(), w3.abs())
    lo, va = emu_out_fwd(h2, w3)
    fig = {}
    assert not gr.accept_bound(lo, logits, gr.bound(logits, ml, D, half_ulp=False), "logits", fig)
    assert not gr.accept_bound(va, values, gr.bound(values, mv, D, half_ulp=False), "values", fig)
    _fig("out_fwd", M=M, fig=fig)


@pytest.mark.parametrize("M", mr.OUT_BWD_M)
def test_out_bwd_generator_and_emulation(M):
    for large in (False, True):
        dl, dv, h2, w3 = mr.tier_a_out_bwd(M, large)
        want, want_p = mr.expect_a_out_bwd(dl, dv, h2, w3, large)
        dh2, partial = emu_out_bwd(dl, dv, h2, w3)
        assert partial.shape == want_p.shape == ((M + 7) // 8, 5, D)
        assert not gr.accept_exact(dh2, want, "dh2") and not gr.accept_exact(partial, want_p, "partial")
    h2, w3, dl, dv = mr.tier_b_out(M)
    d16, ref, ref_p = mr.out_bwd(dl, dv, h2, w3)
    assert (d16.float() != torch.cat([dl, dv.view(-1, 1)], 1)).float().mean() > 0.9
    b, bp = mr.bound_out_bwd(d16, ref, ref_p, h2, w3)
    dh2, partial = emu_out_bwd(dl, dv, h2, w3)
    fig = {}
    assert not gr.accept_bound(dh2[:, :D], ref[:, :D], b[:, :D], "dh2 actor", fig)
    assert not gr.accept_bound(dh2[:, D:], ref[:, D:], b[:, D:], "dh2 critic", fig)
    assert not gr.accept_bound(partial, ref_p, bp, "partial", fig)
    _fig("out_bwd", M=M, fig=fig)


# ---------------------------------------------------------------------------------------------------------- planted defects
def _rejected(got, want, name):
    assert gr.accept_exact(got, want, name), f"tier A accepted: {name}"


def test_planted_defects_of_the_gemm_job_are_rejected():
    # one K chunk dropped: the smallest cell with two chunks; every chunk of a two-segment job
    for M, ks in ((1, (128,)), (1, (64, 64)), (33, (192, 64))):
        segs, b, _ = mr.tier_a_gemm(M, ks, 64, 1, 0, 0)
        want = mr.expect_a_gemm(segs, b, 0, None) if M > 1 else gr.bf16_rne(mr.gemm_job(segs, b)[1])
        assert not gr.accept_exact(emu_gemm(segs, b), want, "y")
        for c in range(sum(ks) // 64):
            _rejected(emu_gemm(segs, b, drop_chunk=c), want, f"K chunk {c} of {ks} dropped")
    # segment 1 multiplied by segment 0's weights: the smallest two-segment cell
    segs, b, _ = mr.tier_a_gemm(1, (64, 64), 64, 0, 0, 0)
    want = gr.bf16_rne(mr.gemm_job(segs)[1])
    assert not gr.accept_exact(emu_gemm(segs), want, "y")
    _rejected(emu_gemm(segs, cross_weights=True), want, "segment 1 on segment 0's weights")
    # a bias added after the ReLU; a bf16 intermediate (with a bias: the product rounded before the bias; two segments: between them)
    segs, b, _ = mr.tier_a_gemm(31, (64,), 64, 1, 1, 0)
    want = mr.expect_a_gemm(segs, b, 1, None)
    assert not gr.accept_exact(emu_gemm(segs, b, relu=True), want, "y")
    _rejected(emu_gemm(segs, b, relu=True, bias_after_relu=True), want, "bias after the ReLU")
    segs, b, _ = mr.tier_a_gemm(31, (256,), 64, 1, 0, 0)
    want = mr.expect_a_gemm(segs, b, 0, None)
    _rejected(emu_gemm(segs, b, bf16_between=True), want, "the product rounded to bf16 before the bias")
    segs, _, _ = mr.tier_a_gemm(31, (128, 64), 64, 0, 0, 0)
    want = mr.expect_a_gemm(segs, None, 0, None)
    _rejected(emu_gemm(segs, bf16_between=True), want, "the accumulator rounded to bf16 between the segments")
    # two tile rows swapped (what a wrong piece of the swizzle does to rows r and r + 2 of a tile): the smallest M that has both
    segs, b, _ = mr.tier_a_gemm(3, (64,), 64, 1, 0, 0)
    want = gr.bf16_rne(mr.gemm_job(segs, b)[1])
    y = emu_gemm(segs, b)
    assert not gr.accept_exact(y, want, "y")
    bad = y.clone()
    bad[0, 8:16], bad[2, 8:16] = y[2, 8:16], y[0, 8:16]
    _rejected(bad, want, "a 16-byte piece of tile rows 0 and 2 swapped")
    # the mask: -0 treated as active; the neighbouring job's activation
    segs, b, a = mr.tier_a_gemm(31, (64,), 64, 1, 0, 1)
    want = mr.expect_a_gemm(segs, b, 0, a)
    assert not gr.accept_exact(emu_gemm(segs, b, act=a), want, "y")
    assert ((a.view(torch.int16) == -32768) & (mr.gemm_job(segs, b)[0] != 0)).any()
    _rejected(emu_gemm(segs, b, act=a, minus_zero_active=True), want, "-0 activation treated as active")
    _, _, other = mr.tier_a_gemm(31, (64,), 64, 1, 0, 1, tag=1)
    _rejected(emu_gemm(segs, b, act=other), want, "the mask of the neighbouring job's activation")
    wide = torch.cat([a, other], 1)  # ldact != ldy: an activation read at the output's leading dimension takes the wrong rows
    _rejected(emu_gemm(segs, b, act=wide.view(-1)[:2 * 31 * 64].view(62, 64)[:31]), want, "the mask read at another leading dimension")


def test_planted_defects_of_the_output_layers_are_rejected():
    h2, w3 = mr.tier_a_out_fwd(1)
    logits, values = mr.expect_a_out_fwd(h2, w3)
    lo, va = emu_out_fwd(h2, w3)
    assert not gr.accept_exact(va, values, "values")
    _rejected(emu_out_fwd(h2, w3, value_from_actor=True)[1], values, "the value head fed the actor's half")
    lanes = torch.arange(16)  # a lost shuffle step: the tree without its m = 2 step
    s = (h2[:, :D].float().view(1, 32, 16) * w3[0].float().view(32, 16)).sum(1)
    for m in (8, 4, 1):
        s = s + s[:, lanes ^ m]
    _rejected(torch.cat([s[:, :1], lo[:, 1:]], 1), logits, "a lost shuffle step")
    # dlogits not rounded to bf16: the cell whose gradients are no bf16 numbers
    dl, dv, h2, w3 = mr.tier_a_out_bwd(1, True)
    want, want_p = mr.expect_a_out_bwd(dl, dv, h2, w3, True)
    dh2, partial = emu_out_bwd(dl, dv, h2, w3, round_d=False)
    _rejected(dh2, want, "dlogits not rounded to bf16 (dh2)")
    _rejected(partial, want_p, "dlogits not rounded to bf16 (partial)")
    # a row past M in the last block's sums: the smallest M with a ragged block; masked elements left unwritten
    for M in (1, 9):
        dl, dv, h2, w3 = mr.tier_a_out_bwd(M, False)
        want, want_p = mr.expect_a_out_bwd(dl, dv, h2, w3, False)
        _rejected(emu_out_bwd(dl, dv, h2, w3, leak_row=True)[1], want_p, f"a row past M = {M} added to the last partial block")
    _rejected(emu_out_bwd(dl, dv, h2, w3, skip_masked=True)[0], want, "masked elements of dh2 left unwritten")


def test_planted_defects_of_the_embed_are_rejected():
    boards, wt, bias = mr.tier_a_embed(1)
    want, want_oh = mr.expect_a_embed(boards, wt, bias)
    assert int(boards[0, 7]) > 30
    y, oh = emu_embed(boards, wt, bias, clamp=False)
    _rejected(y, want, "class clamp missing (y)")
    _rejected(oh, want_oh, "class clamp missing (one-hot matrix)")
    _rejected(emu_embed(boards, wt, bias, onehot_ones=False)[1], want_oh, "one-hot column 496 missing")
    # the last workgroup's missing rows: M = 5 is one row into the second workgroup of four
    boards, wt, bias = mr.tier_a_embed(5)
    want, _ = mr.expect_a_embed(boards, wt, bias)
    bad = emu_embed(boards, wt, bias)[0]
    bad[4] = bad[3]
    _rejected(bad, want, "row 4 computed from row 3")
