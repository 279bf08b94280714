"""The row-wise kernels of the update (csrc/g2048_layernorm.hip: g2048_add_ln_fwd / _bwd, g2048_relu_dropout_fwd / _bwd, g2048_colsum,
g2048_embed_fwd / _ln_fwd / _bwd; csrc/g2048_ppo_loss.hip: g2048_ppo_loss) against the float64 stage references of tests/rowwise_ref.py:
every dropout mask bit for bit against the restated hash, every elementwise stage bit for bit, every statistic, LayerNorm output, sum
and loss within its derived per-element bound.  The kernels are driven through src.g2048.native with explicit seeds; every output lies
in a NaN-pattern guard buffer (``Guarded`` of tests/test_gpu_gemm.py), so an unwritten element or a store outside fails the test.
tests/test_rowwise_ref.py holds the same rules to an f32 / bf16 emulation and to planted defects.  Every test prints one ROWFIG line.

Cells (the smallest shapes that reach every branch):
    * add+LN forward   T in {1, 3, 4, 5, 4099} (4 rows per workgroup, 1024 workgroups at most: from 4097 on a wave walks a second row with
                       the prefetch live) x p in {0, 0.1, 0.5} x {a given, a absent (x_new keeps its pattern), gamma None with and without
                       x_new, x a [T, 1, 256] slice of a NaN-filled [T, 17, 256]}.  The seed puts element 545 exactly ON the 24-bit threshold of
                       p = 0.1 (kept when p 2^24 is truncated, dropped when rounded).  A device seed_state word moved between two launches.
    * add+LN backward  T in {1, 7, 8, 9, 33, 16383, 16384, 16417} and 17, 16405 with g_x of period 17 (8 rows per workgroup below 16384 rows,
                       32 from there on; ragged tails on both sides) x {all outputs, g_x None, da None, gamma None} x {dparams, workspace
                       partials per workgroup}; tier A (integers, bit-equal sums, the test's own mean = 0, rstd = 1) at p in {0, 0.5}, tier B
                       (mean / rstd of a forward launch) at p = 0.1; above 16 000 rows every variant and both kinds of sums once per tier
    * ReLU + dropout   (T, F) in {(1, 8), (5, 24), (37, 1024), (9, 2048), (16383, 8), (16385, 8)} x p in {0, 0.1, 0.5}: -0.0, negatives, products
                       that round; backward out of place and in place, dbias and partials, tier A and B; a moved seed_state word
    * colsum           N in {4, 12, 256, 768, 1024, 2048} x T in {1, 2, 4 step - 1, 4 step, 4 step + 1, two and three workgroups} x {bf16, f32}
                       x {contiguous, row stride 17 * 256}; the rows per pass are read off g2048_colsum_partial_rows
    * embedding        M in {1, 15, 16, 250} x the three table layouts x p in {0, 0.1, 0.5} x {with, without LN}; backward tier A and B,
                       dwt_dcls and partials
    * ppo_loss         M in {1, 63, 1023, 1024, 1025, 2055} x {f32, bf16} x {mask bits, none} x clip_eps in {0.2, 0} x grad_scale in {None,
                       1024, 1000}; planted ratio == 1 (old_logp from a first launch), ratios 0.1 % inside and outside both ends, zero
                       advantages, single legal actions; two launches bit-identical, ``running`` accumulates

Measured on the MI355X (92 tests, all passing; the slowest case takes 2.6 s).  Every exact stage (A1, A3 / A4 without LN, A5, R1, R2, E1, and
A6 / R3 / C1 / E3 on integers, partials included) is bit-equal.  Worst error / bound of the bounded stages (must stay <= 1):
    A2 mean 0.005, rstd 0.009   A3 h 0.986   A4 dx 0.113   A6 dgamma 0.320, dbeta 0.063, da sums 0.051   R3 0.021   C1 0.044
    E2 mean 0.002, rstd 0.009, h 0.988   E3 0.204   L1 new_logp 0.652   L2 means 0.177   L3 dlogits 0.991, L4 dvalues 0.983 (bf16 outputs)
No unplanted sample of any ppo_loss case is undecided.  NOTES.md ("Row-wise update kernels against float64") has the table.
"""
import functools
import json

import numpy as np
import pytest
import torch

import gemm_ref as gr
import rowwise_ref as rr

pytestmark = pytest.mark.gpu
BF16, F32 = gr.BF16, gr.F32
SEED = 0xF234_5678_F234_406F  # bits above 32 set; below 2^32 elements it draws the mask of seed 5655: element 545 ON the threshold of p = 0.1
STATE, STATE2 = 0x7654_3210_89AB_CDEF, 0x1_0000_0003
EPS = 1e-5
D = 256


def _G(dev, rows, cols, dtype):
    from test_gpu_gemm import Guarded

    return Guarded(dev, rows, cols, dtype)


def _untouched(g, what):
    torch.cuda.synchronize()
    assert bool((g.raw == g.pat).all()), f"{what}: written although the launch has no such output"


def _fig(kernel, fig, **kw):
    stages = {k: ({kk: (round(vv, 4) if kk == "ratio" else float(f"{vv:.2e}")) for kk, vv in v.items()} if "ratio" in v else v)
              for k, v in fig.items()}
    print("ROWFIG " + json.dumps(dict(kernel=kernel, **kw, stages=stages)))


def _merge(fig, part):
    """Worst figures over the variants of one test."""
    for k, v in part.items():
        old = fig.get(k)
        if old is None:
            fig[k] = dict(v)
        elif "ratio" in v:
            fig[k] = dict(ratio=max(old["ratio"], v["ratio"]), rel=max(old["rel"], v["rel"]))
        elif "exact" in v:
            fig[k] = dict(exact=old["exact"] and v["exact"])


def _state(dev, word):
    return torch.tensor([word], dtype=torch.int64, device=dev)


def _to(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


@functools.lru_cache(maxsize=2)
def _ln_inputs(T, dev):
    return _to(rr.ln_inputs(T), dev)


@functools.lru_cache(maxsize=2)
def _ln_tier_a(T, dev):
    return _to(rr.ln_bwd_tier_a(T), dev)


def _rows_per_group(T, G, choices):
    return next(r for r in choices if -(-T // r) == G)


# ------------------------------------------------------------------------------------------------------------------- add + LN forward
def _ln_fwd(dev, I, T, p, variant, seed=SEED, state=None):
    """One guarded launch -> (failures, fig)."""
    from src.g2048 import native as nv

    x = I["x"]
    if variant == "strided":
        full = torch.full((T, 17, D), float("nan"), device=dev)
        full[:, 0] = x
        ptr, rs = full.data_ptr(), 17 * D
    else:
        ptr, rs = x.data_ptr(), D
    a = None if variant == "no_a" else I["a"]
    norm = not variant.startswith("no_ln")
    gamma, beta = (I["gamma"], I["beta"]) if norm else (None, None)
    xg, hg, mg, rg = _G(dev, T, D, F32), _G(dev, T, D, BF16), _G(dev, 1, T, F32), _G(dev, 1, T, F32)
    pass_x = variant != "no_ln_nox"
    nv.add_ln_fwd(ptr, rs, a, gamma, beta, xg.view if pass_x else None, hg.view, mg.view[0] if norm else None, rg.view[0] if norm else None, T,
                  EPS, p, seed, 0 if state is None else state.data_ptr())
    h = hg.take(f"h {variant}")
    x_new = xg.take(f"x_new {variant}") if a is not None and pass_x else _untouched(xg, f"x_new {variant}")
    mean, rstd = (mg.take("mean")[0], rg.take("rstd")[0]) if norm else (_untouched(mg, "mean"), _untouched(rg, "rstd"))
    fig = {}
    word = None if state is None else int(state.item())
    return rr.add_ln_fwd_check(x, a, gamma, beta, EPS, p, seed, word, x_new, h, mean, rstd, fig), fig


@pytest.mark.parametrize("p", (0.0, 0.1, 0.5))
@pytest.mark.parametrize("T", (1, 3, 4, 5, 4099))
def test_add_ln_fwd(dev, T, p):
    I = _to(rr.ln_inputs(T, degenerate=T == 5), dev)
    failures, fig = [], {}
    for variant in ("full", "no_a", "no_ln", "no_ln_nox", "strided"):
        f, part = _ln_fwd(dev, I, T, p, variant)
        failures += [f"{variant}: {m}" for m in f]
        _merge(fig, part)
    _fig("add_ln_fwd", fig, T=T, p=p)
    assert not failures, failures
    if p == 0.1 and T >= 3:  # the precondition of the truncation check: the seed has an element on the threshold, and it is kept
        assert int(rr.hash32(np.array([545], dtype=np.uint64), *rr.seed_words(SEED))[0]) >> 8 == rr.thr24(0.1)


def test_add_ln_fwd_seed_state_word(dev):
    """The device word enters the hash as rowwise_ref states, is read at launch time (moved between two launches), and another word
    draws another mask."""
    I = _to(rr.ln_inputs(5), dev)
    state, fig = _state(dev, STATE), {}
    for word in (STATE, STATE2, 0):
        state.fill_(word)
        f, part = _ln_fwd(dev, I, 5, 0.5, "full", state=state)
        assert not f, (hex(word), f)
        _merge(fig, part)
    f, _ = _ln_fwd(dev, I, 5, 0.5, "full", seed=7)  # a seed without high bits, no word
    assert not f, f
    k = [rr.row_keep(SEED, w, 5, 0.5, "cpu") for w in (STATE, STATE2, None)]
    assert not torch.equal(k[0], k[1]) and not torch.equal(k[0], k[2]) and torch.equal(k[2], rr.row_keep(SEED, 0, 5, 0.5, "cpu"))
    _fig("add_ln_fwd seed_state", fig)


# ------------------------------------------------------------------------------------------------------------------- add + LN backward
def _ln_bwd(dev, T, p, variant, period, tier_a, partials, state):
    from src.g2048 import native as nv

    sp = state.data_ptr()
    if tier_a:
        I = _ln_tier_a(T, dev)
        xn, mean, rstd, gamma = I["xn"], I["mean"], I["rstd"], I["gamma"]
    else:  # the statistics of a forward launch on the device
        I = _ln_inputs(T, dev)
        gamma = I["gamma"]
        xn, mean, rstd = torch.empty(T, D, device=dev), torch.empty(T, device=dev), torch.empty(T, device=dev)
        nv.add_ln_fwd(I["x"].data_ptr(), D, I["a"], gamma, I["beta"], xn, torch.empty(T, D, dtype=BF16, device=dev), mean, rstd, T, EPS, p, SEED, sp)
    if variant == "no_ln":
        xn = mean = rstd = gamma = None
    g_x = None if variant == "no_gx" else I["g_x"][:T // period].contiguous()
    dxg, dag, dpg = _G(dev, T, D, F32), _G(dev, T, D, BF16), _G(dev, 3, D, F32)
    ws = nv.add_ln_bwd(0 if xn is None else xn.data_ptr(), D, g_x, I["g_h"], mean, rstd, gamma, dxg.view, None if variant == "no_da" else dag.view,
                       None if partials else dpg.view, T, p, SEED, sp, period)
    dx = dxg.take(f"dx {variant}")
    da = _untouched(dag, "da") if variant == "no_da" else dag.take(f"da {variant}")
    if partials:
        _untouched(dpg, "dparams")
        torch.cuda.synchronize()
        assert torch.isfinite(ws).all()
        sums, rows = ws, _rows_per_group(T, ws.shape[0], (8, 32))
    else:
        sums, rows = dpg.take("dparams"), None
    fig = {}
    return rr.add_ln_bwd_check(xn, g_x, period, I["g_h"], mean, rstd, gamma, p, SEED, int(state.item()), dx, da, sums, rows, fig, tier_a), fig


@pytest.mark.parametrize("T,period", [(1, 1), (7, 1), (8, 1), (9, 1), (33, 1), (16383, 1), (16384, 1), (16417, 1), (17, 17), (16405, 17)])
def test_add_ln_bwd(dev, T, period):
    state = _state(dev, STATE)
    failures, fig = [], {}
    cells = [(0.1, False, v, pt) for v in ("full", "no_gx", "no_da", "no_ln") for pt in (False, True)]
    cells += [(p, True, v, pt) for p in (0.0, 0.5) for v, pt in (("full", False), ("full", True), ("no_da", False), ("no_ln", True))]
    if T > 16000:  # 4 M elements per tensor: every variant and both kinds of sums once per tier (the small sizes take the full product)
        cells = [(0.1, False, "full", False), (0.1, False, "full", True), (0.1, False, "no_gx", True), (0.1, False, "no_da", False),
                 (0.1, False, "no_ln", True), (0.5, True, "full", False), (0.5, True, "full", True), (0.0, True, "no_da", True)]
    for p, tier_a, variant, partials in cells:
        f, part = _ln_bwd(dev, T, p, variant, period, tier_a, partials, state)
        failures += [f"p {p} {'A' if tier_a else 'B'} {variant} {'partials' if partials else 'dparams'}: {m}" for m in f]
        _merge(fig, {k + (" tier A" if tier_a and k.startswith("A6") else ""): v for k, v in part.items()})
    _fig("add_ln_bwd", fig, T=T, period=period)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------- ReLU + dropout
@pytest.mark.parametrize("p", (0.0, 0.1, 0.5))
@pytest.mark.parametrize("T,F", [(1, 8), (5, 24), (37, 1024), (9, 2048), (16383, 8), (16385, 8)])
def test_relu_dropout(dev, T, F, p):
    from src.g2048 import native as nv

    I = _to(rr.relu_inputs(T, F), dev)
    x, state, fig, failures = I["x"], _state(dev, STATE), {}, []
    assert bool((x.view(torch.int16) == -32768).any()) and bool((x.float() < 0).any())  # -0.0 and negatives are there
    yg = _G(dev, T, F, BF16)
    ys = []
    for word in (STATE, STATE2):  # the word is moved between the two launches
        state.fill_(word)
        nv.relu_dropout_fwd(x, yg.view, p, SEED, state.data_ptr())
        ys.append(yg.take("y"))
        failures += rr.relu_dropout_fwd_check(x, p, SEED, word, ys[-1], fig)
    y = ys[-1]
    assert p == 0.0 or T * F < 64 or not torch.equal(ys[0], ys[1])
    for tier_a in ((False, True) if p != 0.1 else (False,)):
        dy = I["dy_int"] if tier_a else I["dy"]
        part = {}
        for inplace, partials in ((False, False), (True, True), (True, False)):
            dxg, dbg = _G(dev, T, F, BF16), _G(dev, 1, F, F32)
            if inplace:
                dxg.fill(dy)
            ws = nv.relu_dropout_bwd(dxg.view if inplace else dy, y, dxg.view, None if partials else dbg.view[0], p)
            dx = dxg.take("dx")
            if partials:
                _untouched(dbg, "dbias")
                sums, rows = ws, _rows_per_group(T, ws.shape[0], (8, 64))
            else:
                sums, rows = dbg.take("dbias")[0], None
            failures += [f"tier {'A' if tier_a else 'B'} inplace {inplace}: {m}" for m in rr.relu_dropout_bwd_check(dy, y, p, dx, sums, rows, part, tier_a)]
            _merge(fig, {k + (" tier A" if tier_a and k.startswith("R3") else ""): v for k, v in part.items()})
    _fig("relu_dropout", fig, T=T, F=F, p=p)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------- colsum
def _colsum_rows(N):
    """-> (n, rows per pass) of the column tile that N is summed in, read off g2048_colsum_partial_rows: a workgroup is added for every
    16 passes, so the second one appears at 16 rows_per_pass + 1 rows."""
    from src.g2048 import native as nv

    lib = nv.load()
    n = N if lib.g2048_colsum_partial_rows(1, N) > 0 else N // 2
    assert lib.g2048_colsum_partial_rows(1, n) == 1
    first2 = next(t for t in range(1, 1 << 14) if lib.g2048_colsum_partial_rows(t, n) == 2)
    assert (first2 - 1) % 16 == 0
    return n, (first2 - 1) // 16


@pytest.mark.parametrize("dtype", (BF16, F32), ids=("bf16", "f32"))
@pytest.mark.parametrize("N", (4, 12, 256, 768, 1024, 2048))
def test_colsum(dev, N, dtype):
    from src.g2048 import native as nv

    n, rpp = _colsum_rows(N)
    lib = nv.load()
    step = lib.g2048_colsum_partial_rows(4 * rpp, n) * rpp  # (one workgroup at these sizes: step = rows per pass)
    assert step == rpp
    Ts = [1, 2, 4 * step - 1, 4 * step, 4 * step + 1, 16 * rpp + 1, 40 * rpp + 3]
    assert [lib.g2048_colsum_partial_rows(t, n) for t in Ts[-2:]] == [2, 3]
    fig, failures = {}, []
    for T in sorted(set(t for t in Ts if t >= 1)):
        g = gr._gen(T, N, 21)
        for tier_a in (True, False):
            x = (gr.ints((T, N), -8, 8, g) if tier_a else gr.tier_b_rows(T, N, g, 0.3)).to(dtype)
            if tier_a and dtype == F32:
                x = x * 129.0  # integers that bf16 could not hold
            for strided in (False, True):
                if strided:
                    full = torch.full((T, 17 * D), float("nan"), dtype=dtype, device=dev)
                    full[:, :N] = x.to(dev)
                    xd = full[:, :N]
                else:
                    xd = x.to(dev)
                og = _G(dev, 1, N, F32)
                nv.colsum(xd, og.view[0])
                part = {}
                failures += [f"T {T} strided {strided}: {m}" for m in
                             rr.colsum_check(x.to(dev), og.take("colsum")[0], part, tier_a, "C1 colsum tier A" if tier_a else "C1 colsum")]
                _merge(fig, part)
                if N == n:  # the first stage alone: the partials add up to the same column sums
                    ws = nv.colsum_partial(xd)
                    assert ws.shape[0] == lib.g2048_colsum_partial_rows(T, N)
                    failures += [f"T {T} partials: {m}" for m in rr.colsum_check(x.to(dev), ws.double().sum(0).float(), part, tier_a, "C1 partials tier A" if tier_a else "C1 partials")]
                    _merge(fig, part)
    _fig("colsum", fig, N=N, dtype=str(dtype), rows_per_pass=rpp, T=Ts)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("p", (0.0, 0.1, 0.5))
@pytest.mark.parametrize("M", (1, 15, 16, 250))
def test_embed(dev, M, p):
    from src.g2048 import native as nv

    I = _to(rr.embed_inputs(M), dev)
    boards, table = I["boards"], I["table"]
    if M >= 15:
        assert set(boards.view(-1).tolist()) >= set(range(32)) | {255}
    padded = torch.full((D, 32), float("nan"), device=dev)
    padded[:, :31] = table.t()
    layouts = dict(class_major=table, weight=table.t().contiguous(), padded=padded)
    state, fig, failures, x0s = _state(dev, STATE), {}, [], []
    R = M * 17
    for name, wt in layouts.items():
        for with_ln in (False, True):
            xg, hg, mg, rg = _G(dev, R, D, F32), _G(dev, R, D, BF16), _G(dev, 1, R, F32), _G(dev, 1, R, F32)
            ln = (I["gamma"], I["beta"], EPS, hg.view, mg.view[0], rg.view[0]) if with_ln else None
            nv.embed_fwd(boards, wt, I["pe"], I["cls"], xg.view, p, SEED, state.data_ptr(), ln)
            x0 = xg.take(f"x0 {name}")
            lnc = (I["gamma"], I["beta"], EPS, hg.take("h"), mg.take("mean")[0], rg.take("rstd")[0]) if with_ln else None
            if not with_ln:
                for g_ in (hg, mg, rg):
                    _untouched(g_, "LN outputs")
            part = {}
            failures += [f"{name} ln {with_ln}: {m}" for m in rr.embed_fwd_check(boards, table, I["pe"], I["cls"], p, SEED, STATE, x0, part, lnc)]
            _merge(fig, part)
            x0s.append(x0)
    assert all(torch.equal(x0s[0].view(torch.int32), t.view(torch.int32)) for t in x0s[1:])  # the same bits from every layout, with and without LN
    for tier_a in ((False, True) if p != 0.1 else (False,)):
        g = I["g_int"] if tier_a else I["g"]
        for partials in (False, True):
            og = _G(dev, 32, D, F32)
            ws = nv.embed_bwd(boards, g, None if partials else og.view, p, SEED, state.data_ptr())
            if partials:
                _untouched(og, "dwt_dcls")
                torch.cuda.synchronize()
                got, groups = ws, ws.shape[0]
            else:
                got, groups = og.take("dwt_dcls"), None
                empty = torch.bincount(rr.embed_classes(boards), minlength=32) == 0
                assert bool((got[empty] == 0).all())
            part = {}
            failures += [f"bwd tier {'A' if tier_a else 'B'} partials {partials}: {m}"
                         for m in rr.embed_bwd_check(boards, g, p, SEED, STATE, got, groups, part, tier_a)]
            _merge(fig, {k + (" tier A" if tier_a else ""): v for k, v in part.items()})
    _fig("embed", fig, M=M, p=p)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------- ppo_loss
CV, CE = 0.5, 0.01


def _ppo_launch(dev, I, clip_eps, scale, running=None):
    """One launch of g2048_ppo_loss itself with every output in a guard buffer."""
    from src.g2048 import native as nv

    M = I["actions"].numel()
    dt = I["logits"].dtype
    G = dict(nl=_G(dev, 1, M, F32), s=_G(dev, 1, 5, F32), dl=_G(dev, M, 4, dt), dv=_G(dev, 1, M, dt))
    sc = None if scale is None else torch.tensor([scale], dtype=F32, device=dev)
    rc = nv.load().g2048_ppo_loss(I["logits"].data_ptr(), int(dt == BF16), I["values"].data_ptr(), int(dt == BF16), I["actions"].data_ptr(),
                                  None if I["mask_bits"] is None else I["mask_bits"].data_ptr(), I["old_logp"].data_ptr(), I["adv"].data_ptr(),
                                  I["ret"].data_ptr(), M, float(clip_eps), CV, CE, G["nl"].view.data_ptr(), G["s"].view.data_ptr(),
                                  G["dl"].view.data_ptr(), G["dv"].view.data_ptr(), None if sc is None else sc.data_ptr(),
                                  None if running is None else running.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return dict(new_logp=G["nl"].take("new_logp")[0], sums=G["s"].take("sums")[0], dlogits=G["dl"].take("dlogits"), dvalues=G["dv"].take("dvalues")[0])


@pytest.mark.parametrize("scale", (None, 1024.0, 1000.0))
@pytest.mark.parametrize("clip_eps", (0.2, 0.0))
@pytest.mark.parametrize("masks", (True, False), ids=("masks", "nomask"))
@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
def test_ppo_loss(dev, bf16, masks, clip_eps, scale):
    fig, failures, undecided = {}, [], {}
    for M in (1, 63, 1023, 1024, 1025, 2055):
        I = rr.ppo_inputs(M, bf16, masks, clip_eps=clip_eps)
        Id = _to(I, dev)
        first = _ppo_launch(dev, Id, clip_eps, scale)
        planted = rr.ppo_plant(I, first["new_logp"].cpu(), clip_eps)
        Id = _to(I, dev)
        run = torch.full((5,), 2.0, dtype=torch.float64, device=dev)
        O = _ppo_launch(dev, Id, clip_eps, scale, run)
        O2 = _ppo_launch(dev, Id, clip_eps, scale, run)
        for k in O:  # two launches on the same inputs: the same bits
            assert torch.equal(O[k].view(torch.int16 if O[k].dtype == BF16 else torch.int32), O2[k].view(torch.int16 if O[k].dtype == BF16 else torch.int32)), (M, k)
        assert torch.equal(run, 2.0 + O["sums"].double() + O["sums"].double())
        assert torch.equal(O["new_logp"], first["new_logp"])  # (old_logp does not enter it)
        ratio = torch.exp(O["new_logp"] - Id["old_logp"])
        assert bool((ratio[0::16] == 1.0).all())  # the planted ties are ties on the device
        ref = rr.ppo_loss_ref(Id["logits"], Id["values"], Id["actions"], Id["mask_bits"], Id["old_logp"], Id["adv"], Id["ret"], clip_eps, CV, CE, scale)
        part = {}
        failures += [f"M {M}: {m}" for m in rr.ppo_loss_check(ref, O["new_logp"], O["sums"], O["dlogits"], O["dvalues"], part, planted.to(dev))]
        undecided[M] = part.pop("undecided")
        _merge(fig, part)
        if M >= 63:  # zero advantages and (with masks) single legal actions, new_logp = 0, are among the samples
            assert bool((Id["adv"] == 0).any()) and (not masks or bool((O["new_logp"] == 0).any()))
    _fig("ppo_loss", fig, bf16=bf16, masks=masks, clip_eps=clip_eps, scale=scale, undecided=undecided)
    assert not failures, failures
