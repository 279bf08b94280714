"""tests/gemm_ref.py held to itself on the CPU: an f32 emulation of every GEMM of the update passes both tiers, the generators meet their
own preconditions at the edges of the GPU grid, and every planted defect - the slips a kernel of this kind makes - is rejected."""
import numpy as np
import pytest
import torch

import gemm_ref as gr

BF16, F32 = gr.BF16, gr.F32


# ---------------------------------------------------------------------------------------------------------- emulations
def _truncate_bf16(v32):
    return (v32.contiguous().view(torch.int32) & -65536).view(F32).to(BF16)


def emu_linear(x, w, b, drop=None, truncate=False, bias_after=False):
    """f32 emulation of y = bf16(x w^T + b).  ``drop`` = (row, k0): that row misses the k-step k0 .. k0 + 15; ``truncate``: the
    accumulator is cut, not rounded, to bf16; ``bias_after``: the bias is added to the bf16-rounded product and rounded again."""
    acc = x.float() @ w.float().t()
    if drop is not None:
        r, k0 = drop
        acc[r] -= x[r, k0:k0 + 16].float() @ w[:, k0:k0 + 16].float().t()
    if b is not None:
        acc = (acc.to(BF16).float() + b) if bias_after else acc + b
    return _truncate_bf16(acc) if truncate else acc.to(BF16)


def emu_masked_bwd(dy, w2t, bit, p):
    """-> (dz bf16, db f32): the masked backward and the column sums of the bf16 dz, accumulated in f32."""
    g = (dy.float() @ w2t.float().t()) * torch.tensor(gr.inv_keep_f32(p))
    dz = torch.where(bit, g, torch.zeros(())).to(BF16)
    return dz, dz.float().sum(0)


def emu_dweight(dy, x, slices, f32_parts=False):
    T = dy.shape[0]
    d, xx = dy.float().reshape(slices, T // slices, -1), x.float().reshape(slices, T // slices, -1)
    parts = d.transpose(1, 2) @ xx
    return (parts if f32_parts else parts.to(BF16)), d.sum(1)


def _linear_case(tier, T, K, N, bias=True):
    x, w, b = gr.tier_a_linear(T, K, N, bias) if tier == "A" else gr.tier_b_linear(T, K, N)
    ref = gr.linear(x, w, b)
    mag = gr.linear(x.abs(), w.abs(), None if b is None else b.abs())
    return x, w, b, ref, mag


def _judge(tier, y, ref, mag, K, what="y"):
    return gr.accept_exact(y, gr.bf16_rne(ref), what) if tier == "A" else gr.accept_bound(y, ref, gr.bound(ref, mag, K), what)


# ---------------------------------------------------------------------------------------------------------- the yardstick itself
def test_bf16_rne_is_round_to_nearest_even():
    """Against the integer form of the rounding, on values that include ties in both directions."""
    v = torch.cat([torch.arange(-5000, 5000).float(), torch.randn(4096) * 300])
    u = v.numpy().view(np.uint32).astype(np.uint64)
    want = (((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)).view(np.float32)
    assert np.array_equal(gr.bf16_rne(v.double()).float().numpy(), want)
    with pytest.raises(AssertionError):
        gr.bf16_rne(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))
    assert gr.rounding_shares(torch.tensor([255.0, 256.0, 257.0, 258.0, 514.0, 513.0, 0.0, 1.5])) == (3 / 8, 2 / 8)


def test_scaling_constants_match_the_entry_points():
    assert gr.thr16(0.0) == 0 and gr.thr16(0.5) == 32768 and gr.thr16(0.1) == 6554
    assert gr.inv_keep_f32(0.5) == np.float32(2.0) and gr.inv_keep_f32(0.0) == np.float32(1.0)
    assert gr.inv_keep_f32(0.1) == np.float32(1.0) / np.float32(0.9) and gr.inv_keep_f32(0.1).dtype == np.float32


@pytest.mark.parametrize("T", [1, 33, 129])
@pytest.mark.parametrize("K,N", [(128, 128), (256, 384), (384, 128), (640, 256), (1024, 256)])
@pytest.mark.parametrize("bias", [True, False])
def test_tier_a_linear_meets_its_preconditions_and_the_emulation_is_exact(T, K, N, bias):
    x, w, b, ref, mag = _linear_case("A", T, K, N, bias)
    assert x.abs().max() <= 8 and w.abs().max() <= 8 and (b is None or (b.abs().max() <= 4096 and torch.equal(b, b.round())))
    gr.assert_exact(mag)
    gr.assert_exercises_rounding(ref)
    assert not _judge("A", emu_linear(x, w, b), ref, mag, K)
    # any order: the k-steps summed backwards, in bf16-sized blocks of 16
    acc = torch.zeros(T, N) if b is None else b.expand(T, N).clone()
    for k0 in reversed(range(0, K, 16)):
        acc = acc + x[:, k0:k0 + 16].float() @ w[:, k0:k0 + 16].float().t()
    assert not gr.accept_exact(acc.to(BF16), gr.bf16_rne(ref), "y")


def test_preconditions_refuse_cases_that_do_not_hold_them():
    x, w, _ = gr.tier_a_linear(64, 256, 128, True)
    with pytest.raises(AssertionError, match="need rounding"):
        gr.assert_exercises_rounding(gr.linear(x, w))  # |x|, |w| <= 4 at K = 256 without a bias: about 1 % need rounding
    with pytest.raises(AssertionError, match="2\\^24"):
        gr.assert_exact(torch.tensor([2.0 ** 24]))


@pytest.mark.parametrize("T,K,N", [(200, 256, 1024), (200, 1024, 256), (129, 384, 128)])
def test_tier_b_emulation_passes_and_the_bound_is_tight(T, K, N):
    x, w, b, ref, mag = _linear_case("B", T, K, N)
    assert abs(x.float().mean().item()) > 0.2 and abs(w.float().mean().item()) > 0.015
    fig = {}
    assert not gr.accept_bound(emu_linear(x, w, b), ref, gr.bound(ref, mag, K), "y", fig)
    assert 0.85 < fig["y"]["ratio"] <= 1.0, fig


# ---------------------------------------------------------------------------------------------------------- planted defects
@pytest.mark.parametrize("tier", ["A", "B"])
def test_planted_defects_of_the_forward_are_rejected(tier):
    T, K, N = 77, 256, 256
    x, w, b, ref, mag = _linear_case(tier, T, K, N)
    good = emu_linear(x, w, b)
    assert not _judge(tier, good, ref, mag, K)

    def rejected(y, name):
        assert _judge(tier, y, ref, mag, K), f"tier {tier} accepted: {name}"

    y = good.clone()
    if tier == "A":  # one unit in the last place
        y.view(torch.int16)[40, 100] += 1
    else:            # the value of another row
        y[40, 100] = good[41, 100] + 1
    rejected(y, "one wrong element")
    y = good.clone()
    y[32:64, 130], y[32:64, 131] = good[32:64, 131], good[32:64, 130]
    rejected(y, "two swapped neighbouring columns in one 32-row tile")
    rejected(emu_linear(x, w, b, drop=(50, 112)), "one k-step of 16 dropped for one row")
    rejected(emu_linear(x, w, b, truncate=True), "truncation instead of round-to-nearest-even")
    rejected(emu_linear(x, w, b, bias_after=True), "the bias added after the bf16 rounding")
    y = good.clone()
    y[T - 1] = emu_linear(x[T - 2:T - 1], w, b)[0]
    rejected(y, "a last partial tile computed from row T - 2")


def test_masked_backward_emulation_and_its_planted_defects():
    T, K, N = 65, 128, 128
    xf, wf, bf = gr.tier_a_linear(T, K, N, True)
    dy, w2t = gr.tier_a_grad(T, K, N)
    for p in (0.0, 0.5):
        inv = gr.inv_keep_f32(p)
        bit = gr.relu(gr.linear(xf, wf, bf)) > 0
        want = gr.masked_bwd(dy, w2t, bit, float(inv))
        gr.assert_exact(gr.linear(dy.abs(), w2t.abs()) * float(inv))
        want16 = gr.bf16_rne(want)
        gr.assert_exact(want16.double().abs().sum(0))
        dz, db = emu_masked_bwd(dy, w2t, bit, p)
        assert not gr.accept_exact(dz, want16, "dz") and not gr.accept_exact(db, gr.colsum(want16), "db")
        # one column sum that includes a row >= T: the clamped tile re-reads row T - 1
        col = int((want16[T - 1] != 0).nonzero()[0])
        bad = db.clone()
        bad[col] += dz[T - 1, col].float()
        assert gr.accept_exact(bad, gr.colsum(want16), "db")
        # a gradient that passes where the forward output was zero
        leak = dz.clone()
        r, c = (~bit & (gr.linear(dy, w2t) != 0)).nonzero()[0].tolist()
        leak[r, c] = gr.linear(dy, w2t)[r, c].to(BF16)
        assert gr.accept_exact(leak, want16, "dz")
    # p = 0.1: one f32 multiply, then one rounding - nearly every non-zero result needs rounding
    bit = gr.relu(gr.linear(xf, wf, bf)) > 0
    e32 = torch.where(bit, gr.scaled_f32(gr.linear(dy, w2t), gr.inv_keep_f32(0.1)), torch.zeros(()))
    assert gr.rounding_shares(e32)[0] >= 0.25
    assert not gr.accept_exact(emu_masked_bwd(dy, w2t, bit, 0.1)[0], e32.to(BF16), "dz")


def test_dropout_acceptance():
    T, K, N = 129, 128, 256
    x, w, b = gr.tier_a_linear(T, K, N, True)
    act = gr.relu(gr.linear(x, w, b))
    gr.assert_exercises_rounding(act)
    for p in (0.5, 0.1):
        expected = gr.scaled_f32(act, gr.inv_keep_f32(p)).to(BF16)
        keep = torch.rand(T, N, generator=torch.Generator().manual_seed(3)) >= gr.thr16(p) / 65536.0
        y = torch.where(keep, expected, torch.zeros((), dtype=BF16))
        assert not gr.accept_dropout(y, expected, act > 0, p, "y")
        assert gr.accept_dropout(expected, expected, act > 0, p, "y")  # nothing dropped: the keep rate is off
        bad = y.clone()
        r, c = (act == 0).nonzero()[0].tolist()
        bad[r, c] = 1.0
        assert gr.accept_dropout(bad, expected, act > 0, p, "y")       # alive where relu(ref) is 0
        if p == 0.1:  # scaled by the float64 1 / 0.9 and rounded: another value on some elements
            other = torch.where(keep, (act / 0.9).to(F32).to(BF16), torch.zeros((), dtype=BF16))
            assert gr.accept_dropout(other, expected, act > 0, p, "y") or torch.equal(other, y)


@pytest.mark.parametrize("stages,S", [(1, 1), (2, 8), (3, 8), (5, 1), (9, 8), (17, 1), (34, 1)])
def test_tier_a_dweight(stages, S):
    T, N, K = 64 * S * stages, 128, 128
    dy, x = gr.tier_a_dweight(T, N, K, S)
    parts, cs = gr.dweight(dy, x, S)
    gr.assert_exact(gr.dweight(dy.abs(), x.abs(), S)[0])
    gr.assert_exact(gr.dweight(dy.abs(), x.abs(), S)[1])
    gr.assert_exercises_rounding(parts)
    p16, c32 = emu_dweight(dy, x, S)
    p32, _ = emu_dweight(dy, x, S, f32_parts=True)
    assert not gr.accept_exact(p16, gr.bf16_rne(parts), "parts") and not gr.accept_exact(p32, parts, "parts f32")
    assert not gr.accept_exact(c32, cs, "colsum")
    if S > 1:  # a partial that took one token stage of its neighbour's slice
        L = T // S
        shifted = torch.cat([dy[:L], dy[L + 64:2 * L + 64]]), torch.cat([x[:L], x[L + 64:2 * L + 64]])
        bad = p16.clone()
        bad[1] = emu_dweight(*shifted, 2)[0][1]
        assert gr.accept_exact(bad, gr.bf16_rne(parts), "parts")
    if stages > 1:  # the last token stage of every slice never multiplied
        L = T // S
        keep = (torch.arange(T) % L) < L - 64
        short = emu_dweight(dy[keep], x[keep], S)[0]
        assert gr.accept_exact(short, gr.bf16_rne(parts), "parts")


def test_tier_b_dweight():
    T, N, K, S = 1024, 256, 128, 8
    dy, x = gr.tier_b_dweight(T, N, K)
    parts, cs = gr.dweight(dy, x, S)
    mag, cmag = gr.dweight(dy.abs(), x.abs(), S)
    p16, c32 = emu_dweight(dy, x, S)
    p32, _ = emu_dweight(dy, x, S, f32_parts=True)
    L = T // S
    assert not gr.accept_bound(p16, parts, gr.bound(parts, mag, L), "parts")
    assert not gr.accept_bound(p32, parts, gr.bound(parts, mag, L, half_ulp=False), "parts f32")
    assert not gr.accept_bound(c32, cs, gr.bound(cs, cmag, L, half_ulp=False), "colsum")
    assert gr.accept_bound(p16, parts, gr.bound(parts, mag, L, half_ulp=False), "parts")  # bf16 partials do not pass for f32 ones
    bad = p16.clone()
    bad[3] = p16[4]
    assert gr.accept_bound(bad, parts, gr.bound(parts, mag, L), "parts")
