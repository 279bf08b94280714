"""The GEMM kernels of the update against the float64 references of tests/gemm_ref.py, per element:

    g2048_linear_bf16               k_linear_ws (K <= 256; 4 or 8 waves, K = 128 or 256), k_linear (K > 256; 3, 4, 5, 6, 8 chunks of K)
    g2048_linear_relu_dropout_bf16  k_linear_ws with the ReLU + dropout epilogue
    g2048_linear_mask_bwd_bf16      k_linear_ws with the mask + column-sum epilogue, k_colsum_final
    g2048_dweight_bf16              k_dweight, 128- and 256-row blocks
    g2048_dweight_jobs              k_dweight_jobs, bf16 and f32 partials

Tier A (gemm_ref: small-integer operands, every partial sum exact in f32) asserts BIT EQUALITY with the rounded float64 result, after
asserting the generator's preconditions from the reference (exactness; >= 25 % of the results need rounding to bf16, >= 1 % are ties).
Tier B (non-zero means, row scales 2^[-6, 3]) asserts the derived per-element bound of gemm_ref.bound next to the whole-tensor 4e-3.

Cells:
    * linear, tier A:   T in T_LIST x (K, N) in LINEAR_KN, with and without bias, ldy = N + 8 g for g in {0, 1, 5}
      (T_LIST puts the clamped last tile first and later in a workgroup's sequence; 34 821 = 544 full tiles + 5 rows)
    * linear, tier B:   T in {129, 2048, 34 821} x LINEAR_KN
    * ReLU + dropout:   T_LIST x FFN_KN; p = 0: y bit-equal to bf16(relu(ref)); p = 0.5 and 0.1: every element 0 or exactly the kept
      value (one f32 multiply by the f32 1 / (1 - p), one rounding), 0 wherever relu(ref) is 0, keep rate within 5 sigma, same seed same
      bits, the mask output changes nothing
    * masked backward:  T_LIST x FFN_KN with the mask of a forward launch on the same T, N.  p = 0 and 0.5 (operands in [-2, 2]): dz bit-equal
      to where(y != 0, bf16(ref / keep), 0), db bit-equal to the float64 column sums of that dz, the partial rows of final=False sum
      to the same.  These products stay below 256, so dz needs no rounding there; p = 0.1 makes nearly every non-zero dz round (bit-equal
      all the same) and its db, no longer exact in f32, is held to the summation bound.
    * tier B of both epilogues at p = 0 (T in {129, 2048, 34 821})
    * dweight, tier A:  stages per slice in {1, 2, 3, 4, 5, 6, 9, 17, 34} x slices in {1, 8, 16, 32} (T = 64 slices stages <= 34 816) x
      (N, K) in DW_NK x block_rows in {0, 128, 256}; the cells above half the full size keep (1024, 256) only.  Every partial and every
      per-slice column sum bit-equal to its own slice's reference; operands are column slices of wider buffers.
    * dweight jobs:     a mixed table of bf16 and f32 partials with and without column sums, each against its own reference (tier A), and
      tier B at (34 816, 16 slices) and (1024, 8 slices) through both entry points.

Footprint: every output (y, dz, mask words, column-sum workspace, db, partials, per-slice column sums) is a view into a buffer filled with
a NaN pattern, >= 64 guard rows on either side and padding behind every row; after the launch the inside is finite and every byte outside
still holds the pattern.  Every operand is a view into such a buffer too (ldx > K, NaN rows around it), so a read outside the operand
shows up as a non-finite or inexact output.

Measured on the MI355X (511 cells, all passing; the file takes 15 s).  Worst tier-B error / bound over all cells (must stay <= 1; the
f32 emulation of tests/test_gemm_ref.py sits at 0.95-0.98) and worst whole-tensor error (must stay < 4e-3):
    kernel                 output                    error / bound                     whole-tensor
    linear                 y, bias                   0.986  (T 34 821, K 128, N 128)   1.69e-3
                           y, no bias                0.985  (T 34 821, K 128, N 128)   1.78e-3
    linear_relu_dropout    y                         0.985  (T 34 821, K 128, N 128)   1.67e-3
    linear_mask_bwd        dz                        0.982  (T 34 821, K 128, N 128)   1.69e-3
                           db (summation bound)      0.003
    dweight                bf16 partials             0.987  (T 1024, 8 slices, 1024 x 256)  1.66e-3; sum of the partials 1.64e-3
                           column sums               0.003                             4.2e-8
    dweight_jobs           bf16 partials             0.987  (bit-identical to the single launch's)
                           f32 partials              0.023  (summation term alone)     3.0e-7
                           column sums               0.003                             4.2e-8
Every tier-A cell is bit-equal: no kernel or host check had to change.
"""
import json

import pytest
import torch

import gemm_ref as gr

pytestmark = pytest.mark.gpu
BF16, F32, U8 = gr.BF16, gr.F32, torch.uint8
GUARD = 64
G_LIST = (0, 1, 5)
T_LIST = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 2048, 34816, 34821)
T_B = (129, 2048, 34821)
LINEAR_KN = ((128, 128), (128, 256), (256, 256), (256, 384), (256, 768), (256, 1024), (384, 128), (512, 384), (640, 256), (768, 256),
             (1024, 256))
FFN_KN = ((256, 1024), (256, 512), (256, 384), (128, 128))
DW_NK = ((1024, 256), (256, 1024), (768, 256), (256, 256), (128, 128), (384, 128))
DW_STAGES, DW_SLICES = (1, 2, 3, 4, 5, 6, 9, 17, 34), (1, 8, 16, 32)
FULL = 34816 * 1024 * 256
_PATTERN = {BF16: (torch.int16, gr.BF16_NAN), F32: (torch.int32, gr.F32_NAN), U8: (torch.uint8, gr.U8_PAT)}


class Guarded:
    """A [rows, cols] view into a pattern-filled buffer: GUARD rows before and after, ``col0`` elements in front of and 8 ``g`` behind
    every row."""

    def __init__(self, dev, rows, cols, dtype, g=0, col0=0):
        self.rows, self.cols, self.col0, self.ld, self.dtype = rows, cols, col0, col0 + cols + 8 * g, dtype
        self.idt, self.pat = _PATTERN[dtype]
        self.raw = torch.full((rows + 2 * GUARD, self.ld), self.pat, dtype=self.idt, device=dev)
        self.view = self.raw.view(dtype)[GUARD:GUARD + rows, col0:col0 + cols]

    def fill(self, t):
        self.view.copy_(t.to(self.view.device))
        return self.view

    def take(self, what, finite_rows=None):
        """The inside after a launch (a copy); asserts that it is finite (its first ``finite_rows`` rows) and that every byte outside
        still holds the pattern.  Leaves the buffer ready for the next launch."""
        torch.cuda.synchronize()
        out = self.view.clone()
        if self.dtype != U8:
            assert torch.isfinite(out[:finite_rows]).all(), f"{what}: elements left unwritten"
        self.raw[GUARD:GUARD + self.rows, self.col0:self.col0 + self.cols] = self.pat
        assert (self.raw == self.pat).all(), f"{what}: the launch wrote outside its [{self.rows} x {self.cols}] output (ld {self.ld})"
        return out


def _operand(dev, t, g=1, col0=8):
    """``t`` on the device as a column slice of a wider NaN-filled buffer."""
    return Guarded(dev, t.shape[0], t.shape[1], t.dtype, g, col0).fill(t)


def _vector(dev, t):
    return None if t is None else Guarded(dev, 1, t.numel(), t.dtype).fill(t.view(1, -1)).view(-1)


def _fig(kernel, **kw):
    print("GEMMFIG " + json.dumps(dict(kernel=kernel, **kw)))


def _abs(t):
    return None if t is None else t.abs()


# ------------------------------------------------------------------------------------------------------------------- linear
@pytest.mark.parametrize("K,N", LINEAR_KN)
@pytest.mark.parametrize("T", T_LIST)
def test_linear_tier_a(dev, T, K, N):
    from src.g2048 import native as nv

    failures = []
    for bias in (True, False):
        x, w, b = (None if t is None else t.to(dev) for t in gr.tier_a_linear(T, K, N, bias))
        ref = gr.linear(x, w, b)
        gr.assert_exact(gr.linear(x.abs(), w.abs(), _abs(b)))
        gr.assert_exercises_rounding(ref)
        want = gr.bf16_rne(ref)
        xv, wv, bv = _operand(dev, x), _operand(dev, w, g=2, col0=0), _vector(dev, b)
        for g in G_LIST:
            out = Guarded(dev, T, N, BF16, g)
            nv.linear_bf16(xv, wv, bv, out=out.view)
            failures += gr.accept_exact(out.take(f"y (bias {bias}, g {g})"), want, f"y (bias {bias}, g {g})")
    assert not failures, failures


@pytest.mark.parametrize("K,N", LINEAR_KN)
@pytest.mark.parametrize("T", T_B)
def test_linear_tier_b(dev, T, K, N):
    from src.g2048 import native as nv

    failures, fig = [], {}
    x, w, b = (t.to(dev) for t in gr.tier_b_linear(T, K, N))
    xv, wv = _operand(dev, x), _operand(dev, w, g=2, col0=0)
    for name, bias in (("bias", b), ("no bias", None)):
        ref = gr.linear(x, w, bias)
        bnd = gr.bound(ref, gr.linear(x.abs(), w.abs(), _abs(bias)), K)
        out = Guarded(dev, T, N, BF16, 1)
        nv.linear_bf16(xv, wv, _vector(dev, bias), out=out.view)
        failures += gr.accept_bound(out.take(name), ref, bnd, name, fig)
    _fig("linear", T=T, K=K, N=N, fig=fig)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------- feed-forward epilogues
def _mask_buffer(dev, nv, T, N):
    nbytes = nv.load().g2048_ffn_mask_bytes(T, N)
    assert nbytes % 2048 == 0
    return Guarded(dev, nbytes // 2048, 2048, U8)


@pytest.mark.parametrize("K,N", FFN_KN)
@pytest.mark.parametrize("T", T_LIST)
def test_linear_relu_dropout_tier_a(dev, T, K, N):
    from src.g2048 import native as nv

    failures = []
    x, w, b = (t.to(dev) for t in gr.tier_a_linear(T, K, N, True))
    ref = gr.linear(x, w, b)
    gr.assert_exact(gr.linear(x.abs(), w.abs(), b.abs()))
    act = gr.relu(ref)
    gr.assert_exercises_rounding(act)
    xv, wv, bv = _operand(dev, x), _operand(dev, w, g=2, col0=0), _vector(dev, b)
    want = gr.bf16_rne(act)
    for g in G_LIST:
        out = Guarded(dev, T, N, BF16, g)
        nv.linear_relu_dropout(xv, wv, bv, 0.0, out=out.view)
        failures += gr.accept_exact(out.take(f"y (p 0, g {g})"), want, f"y (p 0, g {g})")  # the zero set is identical as well
    for p, g in ((0.5, 1), (0.1, 5)):
        expected = gr.scaled_f32(act, gr.inv_keep_f32(p)).to(BF16)
        out, mask = Guarded(dev, T, N, BF16, g), _mask_buffer(dev, nv, T, N)
        seed = 0x9E3779B97F4A7C15 ^ (T * 1000003 + N)
        nv.linear_relu_dropout(xv, wv, bv, p, seed=seed, out=out.view)
        y = out.take(f"y (p {p})")
        failures += gr.accept_dropout(y, expected, act > 0, p, f"y (p {p})")
        nv.linear_relu_dropout(xv, wv, bv, p, seed=seed, out=out.view, mask=mask.view.view(-1))
        y2 = out.take(f"y (p {p}, with mask)")
        mask.take("mask words")
        failures += gr.accept_exact(y2, y, f"y (p {p}) of the same seed, with the mask output")
        if T * N >= 4096:
            nv.linear_relu_dropout(xv, wv, bv, p, seed=seed + 1, out=out.view)
            assert not torch.equal(out.take("y"), y), "another seed, the same mask"
    assert not failures, failures


@pytest.mark.parametrize("K,N", FFN_KN)
@pytest.mark.parametrize("T", T_LIST)
def test_linear_mask_bwd_tier_a(dev, T, K, N):
    from src.g2048 import native as nv

    failures = []
    xf, wf, bf = (t.to(dev) for t in gr.tier_a_linear(T, K, N, True, tag=7))
    dy, w2t = (t.to(dev) for t in gr.tier_a_grad(T, K, N))
    prod = gr.linear(dy, w2t)
    gr.assert_exact(gr.linear(dy.abs(), w2t.abs()) * 2.0)
    xv, wv, bv = _operand(dev, xf), _operand(dev, wf, g=2, col0=0), _vector(dev, bf)
    dyv, w2v = _operand(dev, dy), _operand(dev, w2t, g=2, col0=0)
    ws_floats, rows = nv.load().g2048_linear_mask_bwd_workspace_floats(T, N), nv.load().g2048_linear_mask_bwd_partial_rows(T, N)
    assert ws_floats == 512 * N and 1 <= rows <= 512
    for p in (0.0, 0.5, 0.1):
        mask, yb = _mask_buffer(dev, nv, T, N), Guarded(dev, T, N, BF16, 1)
        nv.linear_relu_dropout(xv, wv, bv, p, seed=11 + T, out=yb.view, mask=mask.view.view(-1))
        bit = yb.take("y") != 0
        bits = mask.take("mask words").view(-1)  # (a contiguous copy: the backward reads it from a plain tensor)
        e32 = torch.where(bit, gr.scaled_f32(prod, gr.inv_keep_f32(p)), torch.zeros((), device=dev))
        want = e32.to(BF16)
        want_db = gr.colsum(want)
        exact_db = p != 0.1
        if exact_db:
            gr.assert_exact(want.double().abs().sum(0))
        else:
            assert gr.rounding_shares(e32)[0] >= 0.25
        for g in G_LIST:
            tag = f"(p {p}, g {g})"
            dz, db, ws = Guarded(dev, T, N, BF16, g), Guarded(dev, 1, N, F32), Guarded(dev, 512, N, F32)
            nv.linear_mask_bwd(dyv, w2v, bits, p, out=dz.view, db=db.view.view(-1), workspace=ws.view.view(-1))
            failures += gr.accept_exact(dz.take("dz " + tag), want, "dz " + tag)
            got_db = db.take("db " + tag).view(-1)
            ws.take("workspace " + tag, finite_rows=rows)
            if exact_db:
                failures += gr.accept_exact(got_db, want_db, "db " + tag)
            else:
                failures += gr.accept_bound(got_db, want_db, gr.bound(want_db, want.double().abs().sum(0), T, half_ulp=False), "db " + tag)
        dz, ws = Guarded(dev, T, N, BF16, 1), Guarded(dev, 512, N, F32)
        _, part = nv.linear_mask_bwd(dyv, w2v, bits, p, final=False, out=dz.view, workspace=ws.view.view(-1))
        assert part.shape == (rows, N)
        failures += gr.accept_exact(dz.take("dz (partial rows)"), want, f"dz (p {p}, partial rows)")
        part = ws.take("workspace", finite_rows=rows)[:rows]
        if exact_db:
            failures += gr.accept_exact(part.double().sum(0).float(), want_db, f"sum of the partial rows (p {p})")
    assert not failures, failures


@pytest.mark.parametrize("K,N", FFN_KN)
@pytest.mark.parametrize("T", T_B)
def test_ffn_epilogues_tier_b(dev, T, K, N):
    """p = 0: y against relu(ref) (ReLU is 1-Lipschitz: the bound of the linear holds for it), dz = dy w2t^T where y != 0 and its column
    sums, under the per-element bounds."""
    from src.g2048 import native as nv

    failures, fig = [], {}
    x, w, b = (t.to(dev) for t in gr.tier_b_linear(T, K, N, tag=1))
    ref = gr.linear(x, w, b)
    out, mask = Guarded(dev, T, N, BF16, 1), _mask_buffer(dev, nv, T, N)
    nv.linear_relu_dropout(_operand(dev, x), _operand(dev, w, g=2, col0=0), _vector(dev, b), 0.0, out=out.view, mask=mask.view.view(-1))
    y = out.take("y")
    failures += gr.accept_bound(y, gr.relu(ref), gr.bound(ref, gr.linear(x.abs(), w.abs(), b.abs()), K), "y", fig)
    _fig("linear_relu_dropout", T=T, K=K, N=N, fig=fig)
    fig = {}
    dy, w2t, _ = (t.to(dev) for t in gr.tier_b_linear(T, K, N, tag=2))
    bit = y != 0
    want = gr.masked_bwd(dy, w2t, bit, 1.0)
    mag = gr.masked_bwd(dy.abs(), w2t.abs(), bit, 1.0)
    dz, db, ws = Guarded(dev, T, N, BF16, 5), Guarded(dev, 1, N, F32), Guarded(dev, 512, N, F32)
    nv.linear_mask_bwd(_operand(dev, dy), _operand(dev, w2t, g=2, col0=0), mask.take("mask words").view(-1), 0.0, out=dz.view,
                       db=db.view.view(-1), workspace=ws.view.view(-1))
    got = dz.take("dz")
    failures += gr.accept_bound(got, want, gr.bound(want, mag, K), "dz", fig)
    # the column sums are those of the kernel's own bf16 dz (held above), added in f32 in any order
    sums = gr.colsum(got)
    err = (db.take("db").view(-1).double() - sums).abs()
    bnd = gr.bound(sums, got.double().abs().sum(0), T, half_ulp=False)
    fig["db"] = dict(ratio=(err / bnd.clamp_min(1e-300)).max().item())
    if not (err <= bnd).all():
        failures.append(f"db: {fig['db']['ratio']:.3f} x the summation bound")
    ws.take("workspace", finite_rows=nv.load().g2048_linear_mask_bwd_partial_rows(T, N))
    _fig("linear_mask_bwd", T=T, K=K, N=N, fig=fig)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------- weight gradient
def _block_rows(N):
    return (0, 128, 256) if N % 256 == 0 else (0, 128)


DW_CELLS = [(st, S, N, K) for st in DW_STAGES for S in DW_SLICES for N, K in DW_NK
            if 64 * S * st <= 34816 and (64 * S * st * N * K <= FULL // 2 or (N, K) == (1024, 256))]


@pytest.mark.parametrize("stages,S,N,K", DW_CELLS)
def test_dweight_tier_a(dev, stages, S, N, K):
    from src.g2048 import native as nv

    T = 64 * S * stages
    dy, x = (t.to(dev) for t in gr.tier_a_dweight(T, N, K, S))
    parts, cs = gr.dweight(dy, x, S)
    mag = gr.dweight(dy.abs(), x.abs(), S)
    gr.assert_exact(mag[0])
    gr.assert_exact(mag[1])
    gr.assert_exercises_rounding(parts)
    want = gr.bf16_rne(parts)
    dyv, xv = _operand(dev, dy), _operand(dev, x, g=2, col0=16)
    failures = []
    for br in _block_rows(N):
        pg, cg = Guarded(dev, S * N, K, BF16), Guarded(dev, S, N, F32)
        nv.dweight_parts(dyv, xv, S, out=pg.view.view(S, N, K), block_rows=br, colsum_out=cg.view)
        failures += gr.accept_exact(pg.take(f"parts (block_rows {br})").view(S, N, K), want, f"parts (block_rows {br})")
        failures += gr.accept_exact(cg.take(f"column sums (block_rows {br})"), cs, f"column sums (block_rows {br})")
    pg = Guarded(dev, S * N, K, BF16)
    nv.dweight_parts(dyv, xv, S, out=pg.view.view(S, N, K))
    failures += gr.accept_exact(pg.take("parts (no column sums)").view(S, N, K), want, "parts (no column sums)")
    assert not failures, failures


# (stages, slices, N, K, f32 partials, column sums): slices a multiple of 8; every block shape of the table is [128 x 128]
DW_JOBS = ((3, 8, 256, 256, False, True), (4, 8, 384, 128, True, True), (5, 8, 128, 128, False, False), (2, 16, 768, 256, True, False),
           (34, 16, 1024, 256, False, True), (17, 32, 256, 1024, True, True), (1, 8, 256, 256, True, True), (6, 32, 128, 256, False, True),
           (9, 8, 128, 384, True, False), (4, 16, 256, 128, False, False))


def _dw_job_buffers(dev, S, N, K, f32_parts, colsums):
    pg = Guarded(dev, S * N, K, F32 if f32_parts else BF16)
    cg = Guarded(dev, S, N, F32) if colsums else None
    return pg, cg


def test_dweight_jobs_tier_a(dev):
    from src.g2048 import native as nv

    jobs, keep = [], []
    for i, (stages, S, N, K, f32_parts, colsums) in enumerate(DW_JOBS):
        T = 64 * S * stages
        dy, x = (t.to(dev) for t in gr.tier_a_dweight(T, N, K, S, tag=100 + i))
        parts, cs = gr.dweight(dy, x, S)
        mag = gr.dweight(dy.abs(), x.abs(), S)
        gr.assert_exact(mag[0])
        gr.assert_exact(mag[1])
        gr.assert_exercises_rounding(parts)
        pg, cg = _dw_job_buffers(dev, S, N, K, f32_parts, colsums)
        jobs.append((_operand(dev, dy), _operand(dev, x, g=2, col0=16), pg.view.view(S, N, K), None if cg is None else cg.view))
        keep.append((pg, cg, parts if f32_parts else gr.bf16_rne(parts), cs))
    nv.dweight_jobs(jobs)
    failures = []
    for i, (pg, cg, want, cs) in enumerate(keep):
        failures += gr.accept_exact(pg.take(f"job {i}: parts").view(want.shape), want, f"job {i} {DW_JOBS[i]}: parts")
        if cg is not None:
            failures += gr.accept_exact(cg.take(f"job {i}: column sums"), cs, f"job {i} {DW_JOBS[i]}: column sums")
    assert not failures, failures


@pytest.mark.parametrize("N,K", DW_NK)
@pytest.mark.parametrize("T,S", [(34816, 16), (1024, 8)])
def test_dweight_tier_b(dev, T, S, N, K):
    from src.g2048 import native as nv

    L = T // S
    dy, x = (t.to(dev) for t in gr.tier_b_dweight(T, N, K))
    parts, cs = gr.dweight(dy, x, S)
    mag, cmag = gr.dweight(dy.abs(), x.abs(), S)
    b16, b32, bcs = gr.bound(parts, mag, L), gr.bound(parts, mag, L, half_ulp=False), gr.bound(cs, cmag, L, half_ulp=False)
    dyv, xv = _operand(dev, dy), _operand(dev, x, g=2, col0=16)
    failures, fig = [], {}
    pg, cg = Guarded(dev, S * N, K, BF16), Guarded(dev, S, N, F32)
    nv.dweight_parts(dyv, xv, S, out=pg.view.view(S, N, K), colsum_out=cg.view)
    got = pg.take("parts").view(S, N, K)
    failures += gr.accept_bound(got, parts, b16, "parts", fig)
    failures += gr.accept_bound(cg.take("column sums"), cs, bcs, "column sums", fig)
    whole = gr.rel(got.double().sum(0), parts.sum(0))
    fig["sum of the parts"] = dict(rel=whole)
    if not whole < gr.REL_LIMIT:
        failures.append(f"sum of the parts: whole-tensor error {whole:.3e}")
    _fig("dweight", T=T, S=S, N=N, K=K, fig=fig)
    fig = {}
    (p32, c32), (p16, _) = _dw_job_buffers(dev, S, N, K, True, True), _dw_job_buffers(dev, S, N, K, False, False)
    nv.dweight_jobs([(dyv, xv, p32.view.view(S, N, K), c32.view), (dyv, xv, p16.view.view(S, N, K), None)])
    got32 = p32.take("job parts f32").view(S, N, K)
    failures += gr.accept_bound(got32, parts, b32, "job parts f32", fig)
    failures += gr.accept_bound(p16.take("job parts bf16").view(S, N, K), parts, b16, "job parts bf16", fig)
    failures += gr.accept_bound(c32.take("job column sums"), cs, bcs, "job column sums", fig)
    _fig("dweight_jobs", T=T, S=S, N=N, K=K, fig=fig)
    assert not failures, failures


def test_wrappers_refuse_buffers_that_do_not_fit(dev):
    """The keyword arguments that hand in output buffers: a wrong shape, dtype or size is refused before anything is launched, and an
    ``ldy`` below N or off the 8-element grid is refused by the entry point (G2048_EINVAL)."""
    from src.g2048 import native as nv

    T, K, N = 65, 128, 128
    x, w, b = (t.to(dev) for t in gr.tier_a_linear(T, K, N, True))
    wide = Guarded(dev, T, N, BF16, 1)
    with pytest.raises(nv.NativeError):
        nv.linear_bf16(x, w, b, out=wide.raw.view(BF16)[GUARD:GUARD + T, 4:4 + N])        # ldy fine, pointer off the 16-byte grid
    with pytest.raises(nv.NativeError):
        nv.linear_relu_dropout(x, w, b, 0.0, out=wide.view[:, :N - 8])                     # wrong shape
    with pytest.raises(nv.NativeError):
        nv.linear_relu_dropout(x, w, b, 0.0, mask=torch.zeros(8, dtype=U8, device=dev))    # wrong mask size
    odd = torch.full((T + 1, N + 4), 0, dtype=BF16, device=dev)
    with pytest.raises(nv.NativeError, match="invalid argument"):
        nv.linear_relu_dropout(x, w, b, 0.0, out=odd[:T, :N])                              # ldy = N + 4
    mask = torch.zeros(nv.load().g2048_ffn_mask_bytes(T, N), dtype=U8, device=dev)
    with pytest.raises(nv.NativeError):
        nv.linear_mask_bwd(x, w, mask, 0.0, workspace=torch.zeros(16, device=dev))         # workspace too small
    with pytest.raises(nv.NativeError):
        nv.linear_mask_bwd(x, w, mask, 0.0, db=torch.zeros(N - 1, device=dev))
    with pytest.raises(nv.NativeError):
        nv.dweight_parts(x[:64], x[:64], 1, colsum_out=torch.zeros(N - 1, device=dev))
    wide.take("y", finite_rows=0)  # nothing was written
