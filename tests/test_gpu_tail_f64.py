"""The fused CLS tail (g2048_cls_tail_fwd, g2048_cls_tail_bwd, g2048_dweight_t; csrc/g2048_tail.hip) against the float64 stage references of
tests/tail_ref.py: every saved tensor, every mask word and every gradient on its own, per element.  The kernels are driven directly
(explicit seeds, no autograd node); tests/test_tail_ref.py holds the same rules to an f32 / bf16 emulation and to planted defects.

Cells:
    * rows:            M in {1, 31, 32, 33, 95, 640, 2048} x p in {0, 0.1}; all stages F0..B8, MASK and ZERO in every cell (95: ld 96 and 2
                       slices; 640: 8 slices x 5 k-steps, one group + the remainder of k_dweight_t; 2048: 4 groups)
    * row stride:      x_row_stride in {256, 260, 17 * 256} at M = 33; the padding of the x rows holds NaNs
    * seeds:           a seed with bits above 32 and a device seed_state word at M = 33, p = 0.1; another word draws another mask
    * degenerate rows: M = 33, p = 0, bo = 0: every third row has o = 0 and x of standard deviation 1e-2 (eps is 10 % of the variance),
                       row 1 a constant x (variance 0, rstd = eps^-1/2)
    * larger buffers:  TailBuffers for M + 64 rows with buf.M lowered: ld > 32 ceil(M / 32); the extra rows keep their NaN patterns, the
                       extra columns stay zero
    * reuse:           EVERY cell starts from buffers filled with NaN patterns inside [rows, 32 blocks] (dlT rows 4..31 and dvT rows 1..31
                       excepted: they must stay zero) and ends without a NaN there; one cell also runs a second, different problem on the
                       buffers of the first
    * g2048_dweight_t alone, tier A (bit-equal per slice): k-steps per slice in {1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16} x slices in {1, 2, 8} x
                       (N, K) in {(32, 64), (64, 64), (96, 128), (256, 1024)}, with and without bias, m < ld with non-zero columns beyond m,
                       guarded NaN-pattern outputs; one launch of the product's nine jobs at ld = 64
    * refusals:        x_row_stride 258 and 252, p = 1, M = 0, ld < 32 blocks, ld = 40 (not a whole number of 16-row k-steps)

Measured on the MI355X (57 tests, all passing; the file takes 4 s).  Worst error / bound per stage over all cells (must stay <= 1), the
f32 / bf16 emulation of tests/test_tail_ref.py next to it, and the worst whole-tensor error (must stay < 4e-3):
    stage               error / bound                    emulation     whole-tensor
    F1 x_mid            0.956  (M 2048, p 0)             0.95          1.23e-3
    F2 mean             0.003  (M 2048, p 0)             0.002         1.8e-7
    F2 rstd             0.008  (degenerate rows)         0.007         4.8e-8
    F3 h2T              0.986  (M 640, p 0)              0.98          1.69e-3
    F4 uT               0.968  (M 33, p 0.1)             0.95          1.68e-3
    F5 featsT           0.988  (M 2048, p 0.1)           0.98          1.88e-3
    F6 a1T a2T c1T c2T  0.960  (M 640, p 0)              0.96          1.70e-3
    F7 logits, values   0.001                            0.001         8.3e-8
    B1 da2T dc2T        0.992  (M 2048, p 0)             0.99          1.82e-3
    B2 da1T dc1T        0.942  (M 2048, p 0.1)           0.92          1.82e-3
    B3 df2T             0.860  (M 2048, p 0)             0.83          2.41e-3  (p 0.1: two roundings)
    B4 dzT              0.969  (M 640, p 0)              0.95          1.68e-3
    B5 dx_cls           0.676  (M 2048, p 0)             0.61          1.71e-3
    B5 ln_partial       0.774  (M 33: one row in block)  0.67          1.74e-3
    B7 d_o              0.968  (M 2048, p 0)             0.95          1.84e-3
    B8 dw / db          0.070 / 0.015  (M 31, p 0.1)     0.07 / 0.014  8.8e-8
F0, B0, B6, MASK, ZERO and every g2048_dweight_t tier-A cell are bit-equal, every guard pattern is intact, every refusal holds: no kernel
arithmetic had to change.  The one product change is the host check of ld (a multiple of 16, as the layout the kernels write needs).
"""
import json

import pytest
import torch

import gemm_ref as gr
import tail_ref as tr

pytestmark = pytest.mark.gpu
BF16, F32 = gr.BF16, gr.F32
ROWS = (1, 31, 32, 33, 95, 640, 2048)
SEED = 0xF234_5678_9ABC_DEF1  # bits above 32 (and bit 63) set
DW_STEPS, DW_SLICES, DW_NK = (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16), (1, 2, 8), ((32, 64), (64, 64), (96, 128), (256, 1024))


class Net:
    """The parameters on the device, packed as the kernels read them."""

    def __init__(self, dev, P):
        from src.g2048 import native as nv

        self.P = {k: v.to(dev) for k, v in P.items()}
        w = [k for k, v in P.items() if v.dim() == 2]
        t = {k: (self.P[k].contiguous() if k in ("a3", "c3") else nv.pack_fragments(self.P[k])) for k in w}
        t.update({k: self.P[k] for k in P if k not in w})
        tt = {k + "T": nv.pack_fragments(self.P[k].t()) for k in w if k not in ("a3", "c3")}
        tt.update(a3=t["a3"], c3=t["c3"], ln_g=self.P["ln_g"])
        self.keep = (t, tt)
        self.W, self.WT = nv.tail_weights(t), nv.tail_weights_t(tt)


@pytest.fixture(scope="module")
def net(dev):
    return Net(dev, tr.make_params())


def _prefill(buf, cfg):
    """NaN patterns into everything a launch pair writes (inside [rows, 32 blocks]; all rows of the row-major outputs)."""
    from src.g2048 import native as nv

    dev, cols = buf.logits.device, 32 * cfg.blocks
    for name, n_rows in buf.rows.items():
        m = torch.zeros(n_rows, buf.ld, dtype=torch.int16, device=dev)
        m[:dict(dlT=4, dvT=1).get(name, n_rows), :cols] = gr.BF16_NAN
        (buf.saved if name in buf.saved else buf.grads)[name].copy_(nv.pack_fragments(m.view(BF16)))
    for t in (buf.saved["x_mid"], buf.saved["mean"], buf.saved["rstd"], buf.logits, buf.values, buf.dx_cls, buf.grads["ln_partial"],
              *buf.dw.values(), *buf.db.values()):
        t.view(torch.int32).fill_(gr.F32_NAN)
    buf.d_o.view(torch.int16).fill_(gr.BF16_NAN)
    buf.saved["masks"].fill_(gr.BF16_NAN)


def _launch(net, buf, inp, cfg, stride=256, state=None):
    """One forward, backward and weight-gradient launch -> the state tail_ref.check takes (device tensors)."""
    from src.g2048 import native as nv

    dev, M = buf.logits.device, cfg.M
    xs = torch.full((M, stride), float("nan"), device=dev)
    xs[:, :256] = inp["x"]
    sp = 0 if state is None else state.data_ptr()
    nv.cls_tail_fwd(inp["o"], xs.data_ptr(), stride, net.W, buf, cfg.eps, cfg.p, cfg.seed, sp)
    nv.cls_tail_bwd(inp["dlogits"], inp["dvalues"], net.WT, buf, cfg.p, cfg.seed, sp)
    jobs = [(buf.grads[dy], buf.saved[xt], buf.dw[k], buf.db[k] if has_b else None) for k, (dy, xt, _n, _k, has_b) in buf.dw_spec.items()]
    nv.dweight_t(jobs, buf.ld, buf.ld, buf.slices)
    torch.cuda.synchronize()
    T = {n: buf.unpacked(n) for n in buf.rows}
    T.update(x_mid=buf.saved["x_mid"][:M], mean=buf.saved["mean"][:M], rstd=buf.saved["rstd"][:M], masks=buf.saved["masks"][:cfg.blocks],
             logits=buf.logits[:M], values=buf.values[:M], d_o=buf.d_o[:M], dx_cls=buf.dx_cls[:M],
             ln_partial=buf.grads["ln_partial"][:cfg.blocks], dw=buf.dw, db=buf.db)
    return T


def _no_nan(T, cfg):
    cols = 32 * cfg.blocks
    bad = []
    for k, v in T.items():
        for kk, t in (v.items() if isinstance(v, dict) else [(k, v)]):
            if t.is_floating_point() and not bool(torch.isfinite(t[:, :cols] if k in tr.SAVED_ROWS or k in tr.GRAD_ROWS else t).all()):
                bad.append(f"{k} {kk}: a NaN is left (an element that is read is not rewritten)")
    return bad


def _cell(dev, net, M, p, tag, stride=256, state=None, degenerate=False, extra=0, seed=SEED, buf=None, prefill=True):
    from src.g2048 import native as nv

    if buf is None:
        buf = nv.TailBuffers(M + extra, dev)
        buf.M = M
    cfg = tr.Cfg(M, p, seed, seed_state=None if state is None else int(state.item()), ld=buf.ld, slices=buf.slices)
    inp = {k: v.to(dev) for k, v in tr.make_inputs(M, seed=len(tag), degenerate=degenerate).items()}
    if prefill:
        _prefill(buf, cfg)
    P = net.P
    if degenerate:
        net = Net(dev, dict({k: v.cpu() for k, v in P.items()}, bo=torch.zeros(256)))
        P = net.P
    T = _launch(net, buf, inp, cfg, stride, state)
    fig = {}
    failures = _no_nan(T, cfg) + tr.check(P, inp, T, cfg, fig)
    print("TAILFIG " + json.dumps(dict(cell=tag, M=M, p=p, ld=buf.ld, slices=buf.slices, ratio={k: round(v["ratio"], 3) for k, v in fig.items()},
                                       rel={k: float(f"{v['rel']:.2e}") for k, v in fig.items()})))
    return failures, T, buf, cfg, inp


@pytest.mark.parametrize("p", (0.0, 0.1))
@pytest.mark.parametrize("M", ROWS)
def test_rows(dev, net, M, p):
    failures, T, buf, cfg, _ = _cell(dev, net, M, p, "rows")
    assert not failures, failures
    if p:
        assert not torch.from_numpy(tr.keep_mask(cfg, 2, 1024)).all()  # (the hash dropped something)


@pytest.mark.parametrize("stride", (256, 260, 17 * 256))
def test_row_stride(dev, net, stride):
    failures, *_ = _cell(dev, net, 33, 0.1, "stride", stride=stride)
    assert not failures, failures


def test_seed_state_word(dev, net):
    """A device seed_state word enters the hash as tail_ref.keep_mask states; another word draws another mask, same seed."""
    words, masks = (0x1_0000_0003, 0x7654_3210_89AB_CDEF), []
    for wv in words:
        state = torch.tensor([wv], dtype=torch.int64, device=dev)
        failures, T, *_ = _cell(dev, net, 33, 0.1, "seed_state", state=state)
        assert not failures, (hex(wv), failures)
        masks.append(T["uT"][:, :33] != 0)
    failures, T, *_ = _cell(dev, net, 33, 0.1, "seed_state")  # (same inputs: the tag seeds them) no state word
    assert not failures, failures
    masks.append(T["uT"][:, :33] != 0)
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[0], masks[2]) and not torch.equal(masks[1], masks[2])
    failures, *_ = _cell(dev, net, 33, 0.1, "seed_lo", seed=7)  # and a seed without high bits
    assert not failures, failures


def test_degenerate_rows(dev, net):
    """eps is 10 % of the variance on every third row and all of it on row 1: F2, F3 and B5 hold there."""
    failures, T, _, cfg, _ = _cell(dev, net, 33, 0.0, "degenerate", degenerate=True)
    assert not failures, failures
    st = tr.ln_stats(T["x_mid"], cfg.eps)
    var = (st["d"] ** 2).mean(1)
    assert float(var[1]) == 0.0 and abs(float(T["rstd"][1]) - cfg.eps ** -0.5) <= float(st["Er"][1])
    rows = tr.eps_rows(33)
    assert bool((cfg.eps / var[rows] > 0.05).all())  # the precondition: eps matters on these rows
    assert bool(((cfg.eps + var[rows]).rsqrt() + st["Er"].reshape(-1)[rows] < var[rows].rsqrt()).all())  # eps = 0 would be rejected


@pytest.mark.parametrize("M,p", [(33, 0.1), (95, 0.0)])
def test_larger_buffers(dev, net, M, p):
    """ld > 32 ceil(M / 32): buffers for M + 64 rows.  Rows M.. of the row-major outputs keep their patterns, columns 32 blocks.. of the
    transposed buffers stay zero (ZERO covers every column from M on)."""
    failures, T, buf, cfg, _ = _cell(dev, net, M, p, "larger", extra=64)
    assert buf.ld == 32 * cfg.blocks + 64 and not failures, failures
    for name, t in (("x_mid", buf.saved["x_mid"]), ("mean", buf.saved["mean"]), ("rstd", buf.saved["rstd"]), ("logits", buf.logits),
                    ("values", buf.values), ("dx_cls", buf.dx_cls)):
        assert bool((t[M:].view(torch.int32) == gr.F32_NAN).all()), f"{name}: rows at or beyond M were written"
    assert bool((buf.d_o[M:].view(torch.int16) == gr.BF16_NAN).all()), "d_o: rows at or beyond M were written"
    assert bool((buf.saved["masks"][cfg.blocks:] == gr.BF16_NAN).all()) and bool(
        (buf.grads["ln_partial"][cfg.blocks:].view(torch.int32) == gr.F32_NAN).all()), "a block beyond the last was written"


def test_buffers_are_reused(dev, net):
    """A second, different problem on the buffers the first left behind (no refill): nothing of the first shows."""
    failures, _, buf, _, _ = _cell(dev, net, 95, 0.1, "reuse first")
    assert not failures, failures
    failures, *_ = _cell(dev, net, 95, 0.0, "reuse second problem", seed=11, buf=buf, prefill=False)
    assert not failures, failures
    buf.M = 70  # fewer rows in the same buffers: the columns 70..95 that the first two filled are zero again
    failures, *_ = _cell(dev, net, 70, 0.1, "reuse fewer rows", buf=buf, prefill=False)
    assert not failures, failures


# ----------------------------------------------------------------------------------------------------- g2048_dweight_t alone
def _dw_job(dev, N, K, ld, m, slices, bias, tag):
    """-> (job, Guarded dw, Guarded db or None, float64 parts, float64 sums): tier-A operands with non-zero integers beyond column m."""
    from src.g2048 import native as nv
    from test_gpu_gemm import Guarded

    g = gr._gen(N, K, ld, m, slices, int(bias), tag)
    lo, hi = gr.int_range(m // slices)
    dyT, xT = gr.ints((N, ld), lo, hi, g).to(dev), gr.ints((K, ld), lo, hi, g).to(dev)
    dyT[:, m:], xT[:, m:] = dyT[:, m:].abs() + 1, xT[:, m:].abs() + 1
    parts, sums = gr.dweight(dyT[:, :m].t(), xT[:, :m].t(), slices)
    for mag in gr.dweight(dyT[:, :m].t().abs(), xT[:, :m].t().abs(), slices):
        gr.assert_exact(mag)
    dw, db = Guarded(dev, slices * N, K, F32), Guarded(dev, 1, slices * N, F32) if bias else None
    job = (nv.pack_fragments(dyT), nv.pack_fragments(xT), dw.view.view(slices, N, K), None if db is None else db.view.view(slices, N))
    return job, dw, db, parts, sums


def _dw_accept(jobs, what):
    failures = []
    for i, (job, dw, db, parts, sums) in enumerate(jobs):
        s, N, K = parts.shape
        failures += gr.accept_exact(dw.take(f"{what} dw {i}").view(s, N, K), parts, f"{what} dw[{i}] {N} x {K}")
        if db is not None:
            failures += gr.accept_exact(db.take(f"{what} db {i}").view(s, N), sums, f"{what} db[{i}] {N}")
    return failures


@pytest.mark.parametrize("slices", DW_SLICES)
@pytest.mark.parametrize("steps", DW_STEPS)
def test_dweight_t_tier_a(dev, steps, slices):
    """Every slice's partial and bias partial bit-equal to its own slice's float64 result; 1..3 k-steps: the remainder loop alone, 4 / 8 /
    12 / 16: 1..4 groups (odd and even counts) of the double-buffered loop, 5 / 7 / 9 / 13: groups plus remainder.  N = 96: the last
    block has one row tile; N = 32: the only one has."""
    from src.g2048 import native as nv

    m = 16 * steps * slices
    ld = m + 32
    jobs = [_dw_job(dev, N, K, ld, m, slices, bias, 0) for N, K in DW_NK for bias in (True, False)]
    nv.dweight_t([j[0] for j in jobs], ld, m, slices)
    failures = _dw_accept(jobs, f"steps {steps} slices {slices}")
    assert not failures, failures


def test_dweight_t_product_jobs(dev):
    """One launch of the product's nine jobs (TailBuffers.dw_spec) at ld = 64."""
    from src.g2048 import native as nv

    buf = nv.TailBuffers(64, dev)
    assert (buf.ld, buf.slices) == (64, 4) and len(buf.dw_spec) == 9
    jobs = [_dw_job(dev, N, K, 64, 64, 4, has_b, i) for i, (_dy, _xt, N, K, has_b) in enumerate(buf.dw_spec.values())]
    nv.dweight_t([j[0] for j in jobs], 64, 64, 4)
    failures = _dw_accept(jobs, "product jobs")
    assert not failures, failures


# ----------------------------------------------------------------------------------------------------- refusals
def test_refusals(dev, net):
    """The host checks reject these before any launch."""
    from src.g2048 import native as nv

    buf = nv.TailBuffers(64, dev)
    buf.M = 33
    inp = {k: v.to(dev) for k, v in tr.make_inputs(33).items()}
    xs = torch.zeros(33, 512, device=dev)

    def fwd(stride=256, p=0.1):
        nv.cls_tail_fwd(inp["o"], xs.data_ptr(), stride, net.W, buf, 1e-5, p, 1)

    def bwd(p=0.1):
        nv.cls_tail_bwd(inp["dlogits"], inp["dvalues"], net.WT, buf, p, 1)

    for kw in (dict(stride=258), dict(stride=252), dict(p=1.0)):
        with pytest.raises(nv.NativeError, match="invalid argument"):
            fwd(**kw)
    with pytest.raises(nv.NativeError, match="invalid argument"):
        bwd(p=1.0)
    for ld in (32, 40):  # fewer columns than 32 blocks; enough columns (M = 1 below) but no whole number of 16-row k-steps
        buf.saved_c.ld = ld
        buf.M = 33 if ld == 32 else 1
        for f in (fwd, bwd):
            with pytest.raises(nv.NativeError, match="invalid argument"):
                f()
    buf.saved_c.ld, buf.M = 64, 0
    for f in (fwd, bwd):
        with pytest.raises(nv.NativeError, match="invalid argument"):
            f()
    buf.M = 33
    fwd()  # (and the same calls with valid arguments are accepted)
    bwd()
    torch.cuda.synchronize()
