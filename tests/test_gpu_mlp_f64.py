"""The kernels of csrc/g2048_mlp.hip against the float64 references of tests/mlp_ref.py, per element:

    g2048_mlp_embed_fwd   k_mlp_embed_fwd   trunk_in on packed boards, and the one-hot matrix
    g2048_gemm_jobs       k_gemm_jobs       the job table: K-segments, bias, ReLU, the mask of a saved activation
    g2048_mlp_out_fwd     k_mlp_out_fwd     both heads' output layers
    g2048_mlp_out_bwd     k_mlp_out_bwd     their input gradients and the first stage of their weight gradients

Tier A (integer operands, every partial sum exact in f32) asserts BIT EQUALITY with the rounded float64 result, after asserting the
generator's preconditions from the reference (exactness; >= 25 % of the bf16 results need rounding, >= 1 % are ties; >= 25 % of a ReLU's
outputs positive and >= 25 % zero).  Tier B (non-zero means, row scales 2^[-6, 3]) asserts the derived per-element bound of
gemm_ref.bound next to the whole-tensor 4e-3, and for the embed bit equality with the f32 sum in the kernel's documented order.  The
cell lists are mlp_ref's; tests/test_mlp_ref.py shows on the CPU that the preconditions hold at every one of them, that an f32 emulation
of each kernel passes and that the planted defects do not.

Cells:
    * embed:    M in EMBED_M (one to three rows of a workgroup of four; 2051 = 512 workgroups + 3 rows), with and without the one-hot
      output; exponents 0..17, rows with 18..30, rows with 31, 32 and 255 (class 30); the table lies in a NaN buffer that holds every
      row an unclamped exponent could index.
    * gemm job: for each of the seven epilogues the diagonal ``mlp_ref.gemm_cells`` through GEMM_M x GEMM_K x GEMM_N (40 cells: every M
      with every N, every K plan four times), both tiers; ldy = N + 8 g for g in {0, 1, 5}, ldact = N + 32.  Then the launches as the
      code makes them (two jobs into the column halves of one buffer; two jobs reading the halves of one buffer; the two-segment job
      over those halves; x rows at stride 17 * 256), one launch of 8 different jobs, and the refusals of the entry point.
    * out_fwd:  M in OUT_FWD_M (16 rows per workgroup), f32 outputs equal to the float64 result in tier A.
    * out_bwd:  M in OUT_BWD_M (8 rows per partial block), gradients that are bf16 numbers and gradients that are not; h2 with +0 and -0.

Footprint: every output is a view into a buffer filled with a NaN pattern, >= 64 guard rows on either side; after the launch the inside
is finite and every byte outside still holds the pattern.  The outputs of the job table also have padding behind every row (the other
three kernels write contiguous rows).  The operands of the job table are column slices of wider NaN-filled buffers, the contiguous
operands of the other kernels have NaN guard rows around them.

Measured on the MI355X (85 tests, 300 tier-B cells, all passing; this file and tests/test_gpu_mlp.py together take about 6 s, the slowest
test 1 s).  Worst tier-B error / bound over all cells (must stay <= 1) and worst whole-tensor error (must stay < 4e-3):
    kernel          output                 error / bound                                  whole-tensor
    mlp_embed_fwd   y                      0.991   (M 2051; bit-equal to the ordered f32 sum)   1.71e-3
    gemm_jobs       y                      0.988   (M 2051, K 64, N 512, bias + ReLU)     2.06e-3
    mlp_out_fwd     logits                 0.0015  (M 2051; summation term alone)         5.6e-8
                    values                 0.0012  (M 2051)                               4.6e-8
    mlp_out_bwd     dh2, actor half        0.992   (M 2051)                               1.67e-3
                    dh2, critic half       0.985   (M 300)                                1.75e-3
                    partial                0.190   (M 2051; summation term alone)         3.8e-8
These are the figures of the f32 emulations of tests/test_mlp_ref.py, digit for digit.  Every tier-A cell is bit-equal, every
footprint intact, every refusal returns G2048_EINVAL: no kernel, host check or wrapper had to change.
"""
import ctypes as C
import json

import pytest
import torch

import gemm_ref as gr
import mlp_ref as mr
from test_gpu_gemm import GUARD, Guarded, _operand, _vector

pytestmark = pytest.mark.gpu
BF16, F32, U8 = gr.BF16, gr.F32, torch.uint8
D = mr.D
G_LIST = (0, 1, 5)
EINVAL = -1


def _fig(kernel, **kw):
    print("MLPFIG " + json.dumps(dict(kernel=kernel, **kw)))


def _rows(dev, t):
    """``t`` [rows, cols] on the device, contiguous, with NaN guard rows around it."""
    return _operand(dev, t, g=0, col0=0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------------- embed
def _table(dev, wt):
    """The [496, 512] table inside a NaN buffer: GUARD rows in front, 256 behind (31 * 15 + 255 = 720 is the last row an unclamped
    exponent indexes)."""
    raw = torch.full((GUARD + 496 + 256, D), gr.BF16_NAN, dtype=torch.int16, device=dev)
    view = raw.view(BF16)[GUARD:GUARD + 496]
    view.copy_(wt)
    return view


@pytest.mark.parametrize("M", mr.EMBED_M)
def test_embed(dev, M):
    from src.g2048 import native as nv

    failures = []
    for tier, (boards, wt, bias) in (("A", mr.tier_a_embed(M)), ("B", mr.tier_b_embed(M))):
        boards, wt, bias = boards.to(dev), wt.to(dev), bias.to(dev)
        if tier == "A":
            want, want_oh = mr.expect_a_embed(boards, wt, bias)
        else:
            pre, ref, onehot = mr.embed(boards, wt, bias)
            want, want_oh = mr.embed_f32_ordered(boards, wt, bias), onehot.to(BF16)
            bnd = gr.bound(pre, mr.embed_mag(boards, wt, bias), 17)
        bv, wv, biasv = _rows(dev, boards), _table(dev, wt), _vector(dev, bias)
        y, oh = Guarded(dev, M, D, BF16), Guarded(dev, M, D, BF16)
        first = None
        for with_oh in (True, False, True):
            tag = f"tier {tier}, onehot {with_oh}"
            nv.mlp_embed_fwd(bv, wv, biasv, y.view, oh.view if with_oh else None)
            got = y.take("y, " + tag)
            failures += gr.accept_exact(got, want, "y, " + tag)
            got_oh = oh.take("onehot, " + tag, finite_rows=None if with_oh else 0)
            if with_oh:
                failures += gr.accept_exact(got_oh, want_oh, "onehot, " + tag)
                if first is not None:
                    failures += gr.accept_exact(got, first[0], "y of a second launch")
                    failures += gr.accept_exact(got_oh, first[1], "onehot of a second launch")
                first = (got, got_oh)
        if tier == "B":
            fig = {}
            failures += gr.accept_bound(first[0], ref, bnd, "y", fig)
            _fig("embed", M=M, fig=fig)
    assert not failures, failures


def test_embed_refusals(dev):
    from src.g2048 import native as nv

    boards, wt, bias = (t.to(dev) for t in mr.tier_a_embed(4))
    y = Guarded(dev, 4, D, BF16)
    lib = nv.load()

    def call(**kw):
        a = dict(boards=boards.data_ptr(), wt=wt.data_ptr(), bias=bias.data_ptr(), y=y.view.data_ptr(), onehot=None, M=4)
        a.update(kw)
        return lib.g2048_mlp_embed_fwd(a["boards"], a["wt"], a["bias"], a["y"], a["onehot"], a["M"], _stream())

    assert call(M=0) == EINVAL and call(M=-4) == EINVAL and call(wt=None) == EINVAL
    assert call(y=y.view.data_ptr() + 8) == EINVAL and call(onehot=y.view.data_ptr() + 2) == EINVAL
    y.take("y", finite_rows=0)  # nothing was written


# ------------------------------------------------------------------------------------------------------------------- the job table
def _job(dev, segs, bias, relu, act, out, g_act=3):
    """The wrapper's dict of one job: operands as column slices of NaN-filled buffers, ``out`` a Guarded or a view."""
    q = dict(segs=[(_operand(dev, x), _operand(dev, w, g=2, col0=0)) for x, w in segs], relu=bool(relu),
             y=out.view if isinstance(out, Guarded) else out)
    if bias is not None:
        q["bias"] = _vector(dev, bias)
    if act is not None:
        q["act"] = _operand(dev, act, g=g_act, col0=8)
    return q


@pytest.mark.parametrize("m", range(len(mr.GEMM_M)))
@pytest.mark.parametrize("e", range(len(mr.EPILOGUES)))
def test_gemm_jobs_cells(dev, e, m):
    from src.g2048 import native as nv

    bias, relu, act = mr.EPILOGUES[e]
    failures = []
    for i, (M, ks, N) in enumerate(mr.gemm_cells(e, m)):
        g = G_LIST[(i + e + m) % 3]
        tag = f"(M {M}, K {ks}, N {N}, epilogue {mr.EPILOGUES[e]}, g {g})"
        segs, b, a, want = mr.tier_a_gemm_case(M, ks, N, bias, relu, act, dev)
        out = Guarded(dev, M, N, BF16, g)
        q = _job(dev, segs, b, relu, a, out)
        assert a is None or q["act"].stride(0) != out.ld
        nv.gemm_jobs([q], M)
        failures += gr.accept_exact(out.take("y, tier A " + tag), want, "y, tier A " + tag)
        segs, b, a = mr.tier_b_gemm(M, ks, N, bias, act)
        segs, b, a = [(x.to(dev), w.to(dev)) for x, w in segs], None if b is None else b.to(dev), None if a is None else a.to(dev)
        pre, ref = mr.gemm_job(segs, b, relu, a)
        nv.gemm_jobs([_job(dev, segs, b, relu, a, out)], M)
        fig = {}
        failures += gr.accept_bound(out.take("y, tier B " + tag), ref, gr.bound(pre, mr.gemm_mag(segs, b), sum(ks)), "y", fig)
        _fig("gemm_jobs", M=M, K=ks, N=N, epilogue=mr.EPILOGUES[e], fig=fig)
    assert not failures, failures


@pytest.mark.parametrize("M", mr.LAUNCH_M)
def test_gemm_jobs_launch_forms(dev, M):
    """The launches of src/ppo/mlp_ops.py, src/ppo/fused_policy.py and src/ppo/hip_ops.py, each job against its own tier-A reference."""
    from src.g2048 import native as nv

    failures = []
    case = {k: tuple(t.to(dev) for t in v) for k, v in mr.tier_a_launch_forms(M).items()}
    want_fwd, want_bwd, want_two, want_cls = mr.expect_a_launch_forms(case)
    wide = lambda w: _operand(dev, w, g=2, col0=0)
    # forward: two jobs, ONE input, outputs = the column halves of one [M, 1024] buffer; bias + ReLU (mlp_ops.py:75, 146)
    x, wa, ba, wc, bc = case["fwd"]
    out, xv = Guarded(dev, M, 1024, BF16, 1), _operand(dev, x)
    nv.gemm_jobs([dict(segs=[(xv, wide(wa))], bias=_vector(dev, ba), relu=True, y=out.view[:, :512]),
                  dict(segs=[(xv, wide(wc))], bias=_vector(dev, bc), relu=True, y=out.view[:, 512:])], M)
    failures += gr.accept_exact(out.take("one input, two halves"), want_fwd, "one input, two halves")
    # two jobs reading the halves of one buffer, masks = the halves of one saved activation (mlp_ops.py:77, 97)
    xa, wa, aa, xc, wc, ac = case["bwd"]
    x2, a2 = _operand(dev, torch.cat([xa, xc], 1)), _operand(dev, torch.cat([aa, ac], 1), g=3)
    wav, wcv = wide(wa), wide(wc)
    nv.gemm_jobs([dict(segs=[(x2[:, :512], wav)], act=a2[:, :512], y=out.view[:, :512]),
                  dict(segs=[(x2[:, 512:], wcv)], act=a2[:, 512:], y=out.view[:, 512:])], M)
    failures += gr.accept_exact(out.take("two halves in, two halves out"), want_bwd, "two halves in, two halves out")
    # the two-segment job over the same halves (mlp_ops.py:99)
    one = Guarded(dev, M, 512, BF16, 5)
    nv.gemm_jobs([dict(segs=[(x2[:, :512], wav), (x2[:, 512:], wcv)], act=a2[:, :512], y=one.view)], M)
    failures += gr.accept_exact(one.take("two segments"), want_two, "two segments")
    # the CLS query projection: x rows at stride 17 * 256, K = N = 256, bias (hip_ops.py:498); the other 16 rows of every board are NaN
    x, w, b = case["cls"]
    h = torch.full((M, 17, 256), gr.BF16_NAN, dtype=torch.int16, device=dev).view(BF16)
    h[:, 0] = x
    q = Guarded(dev, M, 256, BF16)
    nv.gemm_jobs([dict(segs=[(h[:, 0], wide(w))], bias=_vector(dev, b), y=q.view)], M)
    failures += gr.accept_exact(q.take("x rows at stride 17 * 256"), want_cls, "x rows at stride 17 * 256")
    assert not failures, failures


@pytest.mark.parametrize("M", mr.EIGHT_JOBS_M)
def test_gemm_jobs_eight_jobs_in_one_launch(dev, M):
    from src.g2048 import native as nv

    jobs, keep = [], []
    for i, (ks, N, e) in enumerate(mr.EIGHT_JOBS):
        bias, relu, act = mr.EPILOGUES[e]
        segs, b, a, want = mr.tier_a_gemm_case(M, ks, N, bias, relu, act, dev)
        out = Guarded(dev, M, N, BF16, G_LIST[i % 3])
        jobs.append(_job(dev, segs, b, relu, a, out))
        keep.append((out, want))
    nv.gemm_jobs(jobs, M)
    failures = []
    for i, (out, want) in enumerate(keep):
        failures += gr.accept_exact(out.take(f"job {i}"), want, f"job {i} {mr.EIGHT_JOBS[i]}")
    with pytest.raises(nv.NativeError):
        nv.gemm_jobs(jobs + jobs[:1], M)  # 9 jobs
    for out, _ in keep:
        out.take("y of a refused launch", finite_rows=0)
    assert not failures, failures


def test_gemm_jobs_refusals(dev):
    """The host checks of g2048_gemm_jobs through the raw entry point: G2048_EINVAL, and the guarded output stays untouched."""
    from src.g2048 import native as nv

    M, K, N = 65, 128, 128
    x = torch.zeros(M, K + 64, dtype=BF16, device=dev)
    w = torch.zeros(N + 64, K + 64, dtype=BF16, device=dev)
    bias, act = torch.zeros(N + 64, device=dev), torch.ones(M, N + 64, dtype=BF16, device=dev)
    out = Guarded(dev, M, N, BF16, 8)  # ldy = N + 64
    lib = nv.load()
    assert nv.CONSTANTS["G2048_EINVAL"] == EINVAL
    base = dict(x0=x.data_ptr(), x1=0, ldx0=K + 64, ldx1=0, w0=w.data_ptr(), w1=0, ldw0=K + 64, ldw1=0, k0=K, k1=0, bias=bias.data_ptr(),
                act=act.data_ptr(), ldact=N + 64, y=out.view.data_ptr(), ldy=N + 64, N=N, relu=1)

    def call(n_jobs=1, M=M, **kw):
        f = dict(base, **kw)
        rec = nv.GemmJob((C.c_void_p * 2)(f["x0"], f["x1"]), (C.c_int64 * 2)(f["ldx0"], f["ldx1"]), (C.c_void_p * 2)(f["w0"], f["w1"]),
                         (C.c_int64 * 2)(f["ldw0"], f["ldw1"]), (C.c_int * 2)(f["k0"], f["k1"]), f["bias"], f["act"], f["ldact"], f["y"],
                         f["ldy"], f["N"], f["relu"])
        arr = (nv.GemmJob * max(n_jobs, 1))(*([rec] * max(n_jobs, 1)))
        return lib.g2048_gemm_jobs(C.cast(arr, C.c_void_p), n_jobs, M, _stream())

    two = dict(x1=x.data_ptr(), w1=w.data_ptr(), ldx1=K + 64, ldw1=K + 64, k1=64)
    refused = dict(
        k_not_64=dict(k0=96), k_zero=dict(k0=0), k1_not_64=dict(two, k1=32), n_not_64=dict(N=96), n_zero=dict(N=0),
        ldx_below_k=dict(ldx0=K - 8), ldw_below_k=dict(ldw0=K - 8), ldx1_below_k=dict(two, ldx1=56), ldy_below_n=dict(ldy=N - 8),
        ldact_below_n=dict(ldact=N - 4), ldy_off_8=dict(ldy=N + 4), ldact_off_4=dict(ldact=N + 2),
        k1_null_x=dict(two, x1=0), k1_null_w=dict(two, w1=0), null_y=dict(y=0), null_x=dict(x0=0),
        x_off_16=dict(x0=x.data_ptr() + 8), w_off_16=dict(w0=w.data_ptr() + 8), y_off_16=dict(y=out.view.data_ptr() + 8),
        bias_off_16=dict(bias=bias.data_ptr() + 4), act_off_8=dict(act=act.data_ptr() + 4), nine_jobs=dict(n_jobs=9), no_jobs=dict(n_jobs=0),
        no_rows=dict(M=0))
    accepted = [name for name, kw in refused.items() if call(**kw) != EINVAL]
    assert not accepted, accepted
    out.take("y", finite_rows=0)
    assert call(**two) == 0 and call() == 0  # the unmodified records are fine: zeros
    assert not out.take("y").float().abs().sum()


# ------------------------------------------------------------------------------------------------------------------- output layers
@pytest.mark.parametrize("M", mr.OUT_FWD_M)
def test_out_fwd(dev, M):
    from src.g2048 import native as nv

    failures = []
    logits, values = Guarded(dev, M, 4, F32), Guarded(dev, M, 1, F32)
    h2, w3 = (t.to(dev) for t in mr.tier_a_out_fwd(M))
    want_l, want_v = mr.expect_a_out_fwd(h2, w3)
    nv.mlp_out_fwd(_rows(dev, h2), _rows(dev, w3), logits.view, values.view.view(-1))
    failures += gr.accept_exact(logits.take("logits"), want_l, "logits, tier A")
    failures += gr.accept_exact(values.take("values").view(-1), want_v, "values, tier A")
    h2, w3 = (t.to(dev) for t in mr.tier_b_out(M)[:2])
    (ref_l, ref_v), (ml, mv) = mr.out_fwd(h2, w3), mr.out_fwd(h2.abs(), w3.abs())
    nv.mlp_out_fwd(_rows(dev, h2), _rows(dev, w3), logits.view, values.view.view(-1))
    fig = {}
    failures += gr.accept_bound(logits.take("logits"), ref_l, gr.bound(ref_l, ml, D, half_ulp=False), "logits", fig)
    failures += gr.accept_bound(values.take("values").view(-1), ref_v, gr.bound(ref_v, mv, D, half_ulp=False), "values", fig)
    _fig("out_fwd", M=M, fig=fig)
    assert not failures, failures


def test_out_fwd_refusals(dev):
    from src.g2048 import native as nv

    h2, w3 = (t.to(dev) for t in mr.tier_a_out_fwd(16))
    logits, values = Guarded(dev, 16, 4, F32), Guarded(dev, 16, 1, F32)
    lib, lp, vp = nv.load(), logits.view.data_ptr(), values.view.data_ptr()
    assert lib.g2048_mlp_out_fwd(h2.data_ptr(), w3.data_ptr(), lp, vp, 0, _stream()) == EINVAL
    assert lib.g2048_mlp_out_fwd(h2.data_ptr(), w3.data_ptr(), lp, vp, -16, _stream()) == EINVAL
    assert lib.g2048_mlp_out_fwd(h2.data_ptr(), w3.data_ptr(), lp + 4, vp, 15, _stream()) == EINVAL
    assert lib.g2048_mlp_out_fwd(h2.data_ptr(), None, lp, vp, 16, _stream()) == EINVAL
    logits.take("logits", finite_rows=0)
    values.take("values", finite_rows=0)


def _out_bwd(dev, nv, dl, dv, h2, w3, dh2, partial):
    """The raw entry point (the wrapper allocates the partial sums itself: no footprint to check)."""
    M = h2.shape[0]
    rc = nv.load().g2048_mlp_out_bwd(dl.data_ptr(), dv.data_ptr(), h2.data_ptr(), w3.data_ptr(), dh2.view.data_ptr(),
                                     partial.view.data_ptr(), M, _stream())
    assert rc == 0, rc
    return dh2.take("dh2"), partial.take("partial").view(-1, 5, D)


@pytest.mark.parametrize("M", mr.OUT_BWD_M)
def test_out_bwd(dev, M):
    from src.g2048 import native as nv

    failures = []
    rows = nv.load().g2048_mlp_out_bwd_partial_rows(M)
    assert rows == (M + 7) // 8
    dh2, partial = Guarded(dev, M, 2 * D, BF16), Guarded(dev, rows * 5, D, F32)
    for large in (False, True):
        dl, dv, h2, w3 = (t.to(dev) for t in mr.tier_a_out_bwd(M, large))
        want, want_p = mr.expect_a_out_bwd(dl, dv, h2, w3, large)
        got, got_p = _out_bwd(dev, nv, _rows(dev, dl), _rows(dev, dv.view(-1, 1)), _rows(dev, h2), _rows(dev, w3), dh2, partial)
        tag = f"(gradients {'beyond' if large else 'in'} bf16)"
        failures += gr.accept_exact(got, want, "dh2 " + tag) + gr.accept_exact(got_p, want_p, "partial " + tag)
        d = gr.bf16_rne(torch.cat([dl, dv.view(-1, 1)], 1)).double()
        full = torch.cat([d[:, :4].t() @ h2[:, :D].double(), d[:, 4:].t() @ h2[:, D:].double()])
        failures += gr.accept_exact(got_p.double().sum(0).float(), full, "sum of the partial blocks " + tag)
        ws = nv.mlp_out_bwd(dl, dv, h2, w3, torch.empty_like(got))
        assert ws.shape == (rows, 5, D) and torch.equal(ws, got_p), "the wrapper's partial sums"
    h2, w3, dl, dv = (t.to(dev) for t in mr.tier_b_out(M))
    d16, ref, ref_p = mr.out_bwd(dl, dv, h2, w3)
    b, bp = mr.bound_out_bwd(d16, ref, ref_p, h2, w3)
    got, got_p = _out_bwd(dev, nv, _rows(dev, dl), _rows(dev, dv.view(-1, 1)), _rows(dev, h2), _rows(dev, w3), dh2, partial)
    fig = {}
    failures += gr.accept_bound(got[:, :D], ref[:, :D], b[:, :D], "dh2 actor", fig)
    failures += gr.accept_bound(got[:, D:], ref[:, D:], b[:, D:], "dh2 critic", fig)
    failures += gr.accept_bound(got_p, ref_p, bp, "partial", fig)
    if not (got[~mr.active(h2)].view(torch.int16) == 0).all():
        failures.append("dh2: a masked element is not +0")
    _fig("out_bwd", M=M, fig=fig)
    assert not failures, failures


def test_out_bwd_refusals(dev):
    from src.g2048 import native as nv

    dl, dv, h2, w3 = (t.to(dev) for t in mr.tier_a_out_bwd(8, False))
    dh2, partial = Guarded(dev, 8, 2 * D, BF16), Guarded(dev, 5, D, F32)
    lib, ptrs = nv.load(), [dl.data_ptr(), dv.data_ptr(), h2.data_ptr(), w3.data_ptr(), dh2.view.data_ptr(), partial.view.data_ptr()]
    assert lib.g2048_mlp_out_bwd(*ptrs, 0, _stream()) == EINVAL and lib.g2048_mlp_out_bwd(*ptrs, -8, _stream()) == EINVAL
    assert lib.g2048_mlp_out_bwd(*ptrs[:4], ptrs[4] + 4, ptrs[5], 8, _stream()) == EINVAL
    assert lib.g2048_mlp_out_bwd(*ptrs[:5], ptrs[5] + 4, 8, _stream()) == EINVAL
    assert lib.g2048_mlp_out_bwd(None, *ptrs[1:], 8, _stream()) == EINVAL
    assert lib.g2048_mlp_out_bwd_partial_rows(0) == 0 and lib.g2048_mlp_out_bwd_partial_rows(-3) == 0
    dh2.take("dh2", finite_rows=0)
    partial.take("partial", finite_rows=0)
