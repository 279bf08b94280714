"""Float64 references, operand generators, bounds and the cell lists for the four kernels of csrc/g2048_mlp.hip (the MLP policy, the
own-kernel heads of FusedPolicy, the CLS query projection): tests/test_gpu_mlp_f64.py runs the kernels against them, per element;
tests/test_mlp_ref.py holds them to f32 emulations and to planted defects on the CPU.  The tiers, the acceptance rules and the NaN
patterns are those of tests/gemm_ref.py; this file adds what is specific to these kernels.  Everything is a plain torch float64
operation and runs on any device.

    embed        y = bf16(relu(bias + sum over the 16 cells c of wt[31 c + min(v_c, 30)])), and the one-hot matrix [M, 512]
    gemm job     y = bf16(mask(relu(sum over the K-segments s of x_s w_s^T + bias))), relu and mask optional
    out_fwd      logits = h2[:, :512] w3[:4]^T, values = h2[:, 512:] . w3[4]   (f32)
    out_bwd      d = bf16([dlogits | dvalues]); dh2 = bf16([d[:, :4] w3[:4] | d[:, 4:] w3[4]]) where h2 != 0; partial[b][o] = the sum over
                 the rows of block b (8 rows) of d[row][o] h2[row][half(o)][:]   (f32)

Tier A operands: bf16 holds every integer up to 256, so the short reductions (16 table rows, 4 logits, 1 value) take operands in
[-256, 256] and the embed an integer f32 bias in [-4096, 4096]; their results then sit between 2^8 and 2^14, where integers need
rounding to bf16 and ties occur.  The GEMM jobs take gemm_ref's ranges; a ReLU without a bias multiplies the rows of x and of w by
signs, so that the results keep their magnitudes and half of them are negative.

Tier B bounds (gemm_ref.bound; n the reduction length, half_ulp for bf16 outputs; derived, none measured):
    embed 17 (the bias and 16 rows; mag = |bias| + sum |wt rows|) half_ulp | gemm job k[0] + k[1] half_ulp | out_fwd 512 |
    dh2 actor half 4, critic half 1, half_ulp | partials 8.
The bound of a ReLU output is that of its argument (ReLU is 1-Lipschitz); a masked element is exactly zero on both sides.
"""
import torch

import gemm_ref as gr

BF16, F32, F64 = gr.BF16, gr.F32, gr.F64
D, CELLS, CLASSES, ONES_COL = 512, 16, 31, 496
OUT_BWD_ROWS = 8

# ------------------------------------------------------------------------------------------------------------ the GPU cells
EMBED_M = (1, 2, 3, 4, 5, 63, 65, 2051)
GEMM_M = (1, 31, 33, 63, 64, 65, 129, 2051)
GEMM_K = ((64,), (128,), (192,), (256,), (512,), (64, 64), (64, 128), (128, 64), (192, 64), (512, 512))
GEMM_N = (64, 128, 512, 1024)
# (bias, relu, act)
EPILOGUES = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1))
OUT_FWD_M = (1, 15, 16, 17, 300, 2051)
OUT_BWD_M = (1, 7, 8, 9, 300, 2051)


def gemm_cells(e, m):
    """The (M, K plan, N) cells of epilogue number ``e`` at row count number ``m``: a diagonal through the product GEMM_M x GEMM_K x
    GEMM_N.  Per epilogue every M meets every N and five K plans, every K plan appears four times; over the epilogues every (M, K plan)
    pair appears (an odd ``e`` takes the pairs whose indices differ in parity)."""
    out = []
    for i in range(m, 40, 8):
        out.append((GEMM_M[m], GEMM_K[(i + e) % 10], GEMM_N[(i + i // 8 + e) % 4]))
    return out


# ------------------------------------------------------------------------------------------------------------ references
def _classes(boards):
    """boards u8 [M, 16] -> the table rows 31 c + min(v_c, 30), int64 [M, 16]."""
    v = boards.long().clamp_max(CLASSES - 1)
    return v + CLASSES * torch.arange(CELLS, device=boards.device)


def embed(boards, wt, bias):
    """-> (bias + the 16 table rows before the ReLU, the same after it, the one-hot matrix [M, 512]) in float64."""
    idx = _classes(boards)
    pre = gr.f64(bias) + gr.f64(wt)[idx].sum(1)
    onehot = torch.zeros(boards.shape[0], D, dtype=F64, device=boards.device)
    onehot.scatter_(1, idx, 1.0)
    onehot[:, ONES_COL] = 1.0
    return pre, gr.relu(pre), onehot


def embed_mag(boards, wt, bias):
    return gr.f64(bias).abs() + gr.f64(wt).abs()[_classes(boards)].sum(1)


def embed_f32_ordered(boards, wt, bias):
    """The same sum in f32 in the kernel's order: the bias first, then the cells 0..15 ascending; -> bf16(relu(.))."""
    idx = _classes(boards)
    w32 = wt.to(F32)
    acc = bias.to(F32).expand(boards.shape[0], D).clone()
    for c in range(CELLS):
        acc = acc + w32[idx[:, c]]
    return torch.clamp_min(acc, 0.0).to(BF16)


def active(act):
    """The mask of a saved activation: bf16 bits & 0x7FFF non-zero (-0 is masked, a subnormal is active)."""
    return (act.contiguous().view(torch.int16) & 0x7FFF) != 0


def gemm_job(segs, bias=None, relu=False, act=None):
    """-> (the sum over the segments (x, w) of x w^T (+ bias) before the epilogue, the result after ReLU and mask) in float64."""
    pre = sum(gr.linear(x, w) for x, w in segs)
    if bias is not None:
        pre = pre + gr.f64(bias)
    y = gr.relu(pre) if relu else pre
    if act is not None:
        y = torch.where(active(act), y, torch.zeros((), dtype=F64, device=y.device))
    return pre, y


def gemm_mag(segs, bias=None):
    return gemm_job([(x.abs(), w.abs()) for x, w in segs], None if bias is None else bias.abs())[0]


def out_fwd(h2, w3):
    """-> (logits [M, 4], values [M]) in float64."""
    return gr.linear(h2[:, :D], w3[:4]), gr.f64(h2[:, D:]) @ gr.f64(w3[4])


def out_bwd(dlogits, dvalues, h2, w3):
    """-> (d [M, 5] bf16: the rounded gradients, dh2 [M, 1024], partial [ceil(M / 8), 5, 512]) in float64."""
    M = h2.shape[0]
    d16 = gr.bf16_rne(torch.cat([dlogits, dvalues.view(M, 1)], 1))
    d, h, w = gr.f64(d16), gr.f64(h2), gr.f64(w3)
    dh2 = torch.cat([d[:, :4] @ w[:4], d[:, 4:] * w[4]], 1)
    dh2 = torch.where(h != 0, dh2, torch.zeros((), dtype=F64, device=h.device))  # (-0 == 0: masked)
    blocks = (M + OUT_BWD_ROWS - 1) // OUT_BWD_ROWS
    pad = blocks * OUT_BWD_ROWS - M
    dp = torch.cat([d, d.new_zeros(pad, 5)]).view(blocks, OUT_BWD_ROWS, 5)
    hp = torch.cat([h, h.new_zeros(pad, 2 * D)]).view(blocks, OUT_BWD_ROWS, 2 * D)
    partial = torch.cat([dp[:, :, :4].transpose(1, 2) @ hp[:, :, :D], dp[:, :, 4:].transpose(1, 2) @ hp[:, :, D:]], 1)
    return d16, dh2, partial


def out_bwd_mag(d16, h2, w3):
    """-> the references of ``out_bwd`` on absolute values: (actor half of dh2, critic half, partial).  (A masked element is zero
    here too, and so is its error.)"""
    _, dh2, partial = out_bwd(d16[:, :4].abs().float(), d16[:, 4].abs().float(), h2.abs(), w3.abs())
    return dh2[:, :D], dh2[:, D:], partial


# ------------------------------------------------------------------------------------------------------------ tier A
def big_ints(shape, lo, hi, gen):
    """Integers in [lo, hi] as bf16 (|value| <= 256: exact)."""
    assert -256 <= lo <= hi <= 256
    return torch.randint(lo, hi + 1, shape, generator=gen).to(BF16)


def assert_relu_split(pre, need=0.25):
    pos, zero = (pre > 0).double().mean().item(), (pre <= 0).double().mean().item()
    assert pos >= need and zero >= need, f"tier A precondition: {pos:.3f} of the ReLU outputs positive, {zero:.3f} zero"


def boards_for(M, gen):
    """u8 [M, 16]: exponents 0..17; rows 1, 5, 9, .. hold 18..30 in thirteen of their cells; rows 0, 3, 6, .. hold 31, 32 and 255 (class
    30, like every exponent above it) in cells 15, 7 and 0, each value in each of those cells over three such rows."""
    b = torch.randint(0, 18, (M, CELLS), generator=gen)
    for r in range(1, M, 4):
        b[r, (r + torch.arange(13)) % CELLS] = torch.arange(18, 31)
    for r in range(0, M, 3):
        for j, cell in enumerate((15, 7, 0)):  # (cell 15: an unclamped class would read past the table)
            b[r, cell] = (31, 32, 255)[(j + r // 3) % 3]
    return b.to(torch.uint8)


def tier_a_embed(M, tag=0):
    """boards u8 [M, 16], wt [496, 512] bf16 integers in [-256, 256], bias f32 integers in [-4096, 4096]."""
    g = gr._gen(M, tag, 11)
    return boards_for(M, g), big_ints((CELLS * CLASSES, D), -256, 256, g), torch.randint(-4096, 4097, (D,), generator=g).to(F32)


def expect_a_embed(boards, wt, bias):
    """Asserts the preconditions; -> (y bf16, one-hot matrix bf16)."""
    pre, y, onehot = embed(boards, wt, bias)
    gr.assert_exact(embed_mag(boards, wt, bias))
    gr.assert_exercises_rounding(y)
    assert_relu_split(pre)
    return gr.bf16_rne(y), onehot.to(BF16)


def act_for(M, N, gen):
    """A saved activation bf16 [M, N]: 15 % +0, 15 % -0 (0x8000), 5 % the smallest subnormal (0x0001, active), else ordinary
    positives."""
    u = torch.rand(M, N, generator=gen)
    bits = (torch.rand(M, N, generator=gen) * 4 + 0.125).to(BF16).view(torch.int16).clone()
    bits[u < 0.35] = 1
    bits[u < 0.30] = -32768
    bits[u < 0.15] = 0
    return bits.view(BF16)


def tier_a_gemm(M, ks, N, bias, relu, act, tag=0):
    """-> (segs [(x [M, k] , w [N, k]) ...] bf16 integers, bias f32 integers or None, act bf16 or None) on the CPU.  With a bias
    |x|, |w| <= 4 and the bias in [-4096, 4096] spreads the results around zero; without one ``int_range`` of the whole reduction
    length, and under a ReLU a sign per row of x and per row of w (every segment the same), so that half of the results are negative."""
    g = gr._gen(M, sum(ks), len(ks), ks[0], N, 4 * bias + 2 * relu + act, tag, 12)
    lo, hi = (-4, 4) if bias else gr.int_range(sum(ks))
    sx = torch.randint(0, 2, (M, 1), generator=g) * 2 - 1
    sw = torch.randint(0, 2, (N, 1), generator=g) * 2 - 1
    segs = []
    for k in ks:
        x, w = gr.ints((M, k), lo, hi, g), gr.ints((N, k), lo, hi, g)
        if relu and not bias:
            x, w = (x * sx).to(BF16), (w * sw).to(BF16)
        segs.append((x, w))
    b = torch.randint(-4096, 4097, (N,), generator=g) if bias else None
    if bias and relu and act:  # 35 % of the outputs survive both: magnitudes from 1024 on, so that nearly all of those need rounding
        b = torch.randint(1024, 4097, (N,), generator=g) * (torch.randint(0, 2, (N,), generator=g) * 2 - 1)
    return segs, None if b is None else b.to(F32), act_for(M, N, g) if act else None


def expect_a_gemm(segs, bias, relu, act):
    """Asserts the preconditions; -> y bf16."""
    pre, y = gemm_job(segs, bias, relu, act)
    gr.assert_exact(gemm_mag(segs, bias))
    gr.assert_exercises_rounding(y)
    if relu:
        assert_relu_split(pre)
    if act is not None:
        hit = (~active(act) & (pre > 0 if relu else pre != 0)).double().mean().item()
        assert hit >= 0.1, f"tier A precondition: the mask zeroes {hit:.3f} of the outputs"
    return gr.bf16_rne(y)


def tier_a_gemm_case(M, ks, N, bias, relu, act, dev="cpu"):
    """-> (segs, bias, act, y bf16) on ``dev``, preconditions asserted.  A cell of fewer than 4096 outputs has shares that a handful of
    values decide (one tie among 64 is 1.6 %): there the generator draws again, tags 0, 1, .., at most 16 times, until they hold."""
    for tag in range(16 if M * N < 4096 else 1):
        segs, b, a = tier_a_gemm(M, ks, N, bias, relu, act, tag)
        segs = [(x.to(dev), w.to(dev)) for x, w in segs]
        b, a = (None if t is None else t.to(dev) for t in (b, a))
        try:
            return segs, b, a, expect_a_gemm(segs, b, relu, a)
        except AssertionError as err:
            last = err
    raise last


LAUNCH_M = (1, 65, 2051)
# (K plan, N, epilogue number): eight jobs of one launch, every one another shape
EIGHT_JOBS = (((64,), 64, 0), ((512, 512), 128, 6), ((128,), 1024, 3), ((64, 128), 512, 4), ((192,), 128, 1), ((128, 64), 64, 5),
              ((256,), 512, 2), ((192, 64), 1024, 6))
EIGHT_JOBS_M = (33, 129)


def tier_a_launch_forms(M):
    """The operands of the launches that the code makes (tests/test_gpu_mlp_f64.py: test_gemm_jobs_launch_forms), CPU tensors:
    fwd = (x, wa, ba, wc, bc): two 512 -> 512 jobs with bias + ReLU on ONE input; bwd = (xa, wa, aa, xc, wc, ac): two 512 -> 512 jobs
    with masks, also the two segments of one job under the mask aa; cls = (x, w, b): 256 -> 256 with a bias."""
    (sa, ba, _), (sc, bc, _) = tier_a_gemm(M, (512,), 512, 1, 1, 0, tag=31), tier_a_gemm(M, (512,), 512, 1, 1, 0, tag=32)
    fwd = (sa[0][0], sa[0][1], ba, sc[0][1], bc)
    (sa, _, aa), (sc, _, ac) = tier_a_gemm(M, (512,), 512, 0, 0, 1, tag=33), tier_a_gemm(M, (512,), 512, 0, 0, 1, tag=34)
    bwd = (sa[0][0], sa[0][1], aa, sc[0][0], sc[0][1], ac)
    segs, b, _ = tier_a_gemm(M, (256,), 256, 1, 0, 0, tag=35)
    return dict(fwd=fwd, bwd=bwd, cls=(segs[0][0], segs[0][1], b))


def expect_a_launch_forms(case):
    """Asserts every job's preconditions; -> y bf16 of (fwd [M, 1024], bwd [M, 1024], the two-segment job [M, 512], cls [M, 256])."""
    x, wa, ba, wc, bc = case["fwd"]
    fwd = torch.cat([expect_a_gemm([(x, wa)], ba, 1, None), expect_a_gemm([(x, wc)], bc, 1, None)], 1)
    xa, wa, aa, xc, wc, ac = case["bwd"]
    bwd = torch.cat([expect_a_gemm([(xa, wa)], None, 0, aa), expect_a_gemm([(xc, wc)], None, 0, ac)], 1)
    two = expect_a_gemm([(xa, wa), (xc, wc)], None, 0, aa)
    x, w, b = case["cls"]
    return fwd, bwd, two, expect_a_gemm([(x, w)], b, 0, None)


W3_RANGES = ((-8, 8), (-6, 8), (-8, 6), (-4, 8), (-8, 4))


def tier_a_out_fwd(M, tag=0):
    """h2 [M, 1024]: the actor's half integers in [0, 8], the critic's in [0, 5]; w3 [5, 512]: every row its own range."""
    g = gr._gen(M, tag, 13)
    h2 = torch.cat([gr.ints((M, D), 0, 8, g), gr.ints((M, D), 0, 5, g)], 1)
    w3 = torch.cat([gr.ints((1, D), lo, hi, g) for lo, hi in W3_RANGES])
    return h2, w3


def expect_a_out_fwd(h2, w3):
    logits, values = out_fwd(h2, w3)
    ml, mv = out_fwd(h2.abs(), w3.abs())
    gr.assert_exact(ml)
    gr.assert_exact(mv)
    return logits, values


def h2_with_zeros(M, gen, values):
    """bf16 [M, 1024]: ``values`` with 15 % +0 and 15 % -0 in their place."""
    u = torch.rand(M, 2 * D, generator=gen)
    bits = values.to(BF16).view(torch.int16).clone()
    bits[u < 0.30] = -32768
    bits[u < 0.15] = 0
    return bits.view(BF16)


def tier_a_out_bwd(M, large, tag=0):
    """dlogits f32 [M, 4], dvalues f32 [M], h2 bf16 [M, 1024] integers in [1, 8] with +0 and -0, w3 bf16 [5, 512] integers in
    [-128, 128].  ``large`` False: gradients in [-16, 16], bf16 numbers.  True: odd integers of magnitude 257..4095, none of them a
    bf16 number, and w3 in [-8, 8]."""
    g = gr._gen(M, int(large), tag, 14)
    h2 = h2_with_zeros(M, g, torch.randint(1, 9, (M, 2 * D), generator=g))
    if large:
        d = (2 * torch.randint(128, 2048, (M, 5), generator=g) + 1) * (torch.randint(0, 2, (M, 5), generator=g) * 2 - 1)
        w3 = gr.ints((5, D), -8, 8, g)
    else:
        d = torch.randint(-16, 17, (M, 5), generator=g)
        w3 = big_ints((5, D), -128, 128, g)
    d = d.to(F32)
    return d[:, :4].contiguous(), d[:, 4].contiguous(), h2, w3


def expect_a_out_bwd(dlogits, dvalues, h2, w3, large):
    """Asserts the preconditions; -> (dh2 bf16, partial float64)."""
    d16, dh2, partial = out_bwd(dlogits, dvalues, h2, w3)
    ma, mc, mp = out_bwd_mag(d16, h2, w3)
    for m in (ma, mc, mp):
        gr.assert_exact(m)
    raw = torch.cat([dlogits, dvalues.view(-1, 1)], 1)
    changed = (gr.f64(d16) != gr.f64(raw)).double().mean().item()
    assert (changed >= 0.25) if large else (changed == 0.0), \
        f"tier A precondition: {changed:.3f} of the gradients change when rounded to bf16"
    zeros = (gr.f64(h2) == 0).double().mean().item()
    assert zeros >= 0.25, f"tier A precondition: {zeros:.3f} of h2 is zero"
    gr.assert_exercises_rounding(dh2)
    return gr.bf16_rne(dh2), partial


# ------------------------------------------------------------------------------------------------------------ tier B
def tier_b_embed(M, tag=0):
    """Weights at the trained scale (randn / 4) with a non-zero mean, an f32 randn bias."""
    g = gr._gen(M, tag, 21)
    wt = (torch.randn(CELLS * CLASSES, D, generator=g) / 4 + 0.02).to(BF16)
    return boards_for(M, g), wt, torch.randn(D, generator=g) * 0.1


def tier_b_gemm(M, ks, N, bias, act, tag=0):
    g = gr._gen(M, sum(ks), len(ks), ks[0], N, 2 * bias + act, tag, 22)
    K = sum(ks)
    segs = [(gr.tier_b_rows(M, k, g, 0.3), (torch.randn(N, k, generator=g) / K ** 0.5 + 0.02).to(BF16)) for k in ks]
    return segs, torch.randn(N, generator=g) if bias else None, act_for(M, N, g) if act else None


def tier_b_out(M, tag=0):
    """h2 = relu of rows at scales 2^[-6, 3] with +0 and -0, w3 at the trained scale with a non-zero mean, f32 randn gradients at row
    scales 2^[-6, 3] (no bf16 numbers)."""
    g = gr._gen(M, tag, 23)
    h2 = h2_with_zeros(M, g, gr.tier_b_rows(M, 2 * D, g, 0.3).abs())
    w3 = (torch.randn(5, D, generator=g) / D ** 0.5 + 0.02).to(BF16)
    d = torch.randn(M, 5, generator=g) * torch.exp2(torch.randint(-6, 4, (M, 1), generator=g).float())
    return h2, w3, d[:, :4].contiguous(), d[:, 4].contiguous()


def bound_out_bwd(d16, dh2, partial, h2, w3):
    """-> the bounds of (dh2 [M, 1024], partial)."""
    ma, mc, mp = out_bwd_mag(d16, h2, w3)
    b = torch.cat([gr.bound(dh2[:, :D], ma, 4), gr.bound(dh2[:, D:], mc, 1)], 1)
    return b, gr.bound(partial, mp, OUT_BWD_ROWS, half_ulp=False)
