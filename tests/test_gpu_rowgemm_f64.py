"""k_rowgemm (csrc/g2048_rowgemm.hip) behind g2048_linear_add_ln_fwd / _bwd against the float64 stage references of tests/rowgemm_ref.py:
every dropout mask bit for bit against the restated hash, the integer tier bit for bit through the GEMM, the dropout, the add, da and every
workgroup's partial sums, the realistic tier within derived per-element bounds.  The entry points are called directly (the partials too lie
in a guard buffer sized by g2048_linear_add_ln_bwd_partial_rows); every output is a ``Guarded`` NaN-pattern buffer of
tests/test_gpu_gemm.py, so an unwritten element or a store outside fails the test.  tests/test_rowgemm_ref.py holds the same rules to an
emulation and to planted defects.  Every test prints one ROWGEMMFIG line.

Shapes (rowgemm_ref.tile_plan says why these are the smallest that reach each branch) and the template bodies they launch, forward and
backward alike (body = 96- or 160-token tile x K / 128):
    T = 1, 7, 8, 9        one tile, 96-token body, waves without rows       T = 1 at every K: bodies (96, 2), (96, 4), (96, 6), (96, 8)
    T = 33                a second tile of one row                          every K, the same four bodies
    T = 413               13 tiles, the last of 29 rows                     every K
    T = 8193              tpw 33, last tile 9 rows                          K = 256, 1024
    T = 12288             tpw 48, 256 full tiles                            K = 256, 1024
    T = 12289             the first T of the 160-token body: tpw 49, last tile 39 rows    every K: bodies (160, 2), (160, 4), (160, 6), (160, 8)
    T = 34816, 34821      tpw 136 / 137, last tile 23 rows                  K = 256, 1024
    T = 40960, 40961      256 full tiles of 160 / 257 tiles: workgroup 0 walks a second tile of ONE row and adds it to its partial; 40961: every K
    T = 34816, 48700, 49153 under G2048_RG_TWO_TILES=1: the 96-token body at tpw 68 and 96 (the only policy under which its rows 48..95 are valid
                          rows) and the 160-token body at tpw 97, two tiles per workgroup      K = 256, 1024
    T = 17, 34, 425, 12291, 34816   the multiples of 17 for g_x / g_h_extra of period 17 (12291: the 160-token body)
Variants.  Forward: tier A and B x p in {0, 0.1, 0.5} x {bias, no bias, u a column slice of a wider NaN-filled matrix, x the [:, 0] slice of a
NaN-filled [T, 17, 256]}.  Backward: tier A at p in {0, 0.5}, tier B at p = 0.1 (statistics of a forward launch) x {g_x of period 1, g_x NULL,
da NULL, lddy > K, g_x of period 17, g_h_extra + g_x of period 17, the K = 512 window of a packed [256][768] with its tile stride}.  Up to
T = 12291 the full product, above it each direction once per tier with all outputs and one launch per remaining variant (the numpy hash of
12.6 M elements is the slow part).  A device seed_state word is passed to every launch and moved between two.

Measured on the MI355X (104 tests, all passing, 26.5 s; the slowest 0.94 s).  Bit-equal in every cell: A1 x_new of tier A, the dropped elements
of B1, A5 da, every workgroup's A6 partial of tier A; dx of tier A has error 0.  Worst error / bound of the bounded stages (must stay <= 1):
    B1 x_new 0.981   A2 mean 0.011, rstd 0.011   A3 h 0.988   A4 dx 0.797   A6 dgamma 0.826, dbeta 0.826, da sums 0.022
NOTES.md ("Fused Linear + add + LayerNorm against float64") has the table with the cells and the emulation's figures.
"""
import functools
import json

import numpy as np
import pytest
import torch

import gemm_ref as gr
import rowgemm_ref as rg
import rowwise_ref as rr

pytestmark = pytest.mark.gpu
BF16, F32 = gr.BF16, gr.F32
SEED = 0xF234_5678_F234_406F  # the seed of tests/test_gpu_rowwise.py: element 545 sits exactly ON the 24-bit threshold of p = 0.1
STATE, STATE2 = 0x7654_3210_89AB_CDEF, 0x1_0000_0003
EPS = 1e-5
D = 256
KS = (256, 512, 768, 1024)
ALL_K_T = (1, 33, 413, 12289, 40961)
FULL_PRODUCT_T = 12291  # up to here every variant at every p and tier
# (T, G2048_RG_TWO_TILES)
SHAPES = [(T, False) for T in (1, 7, 8, 9, 17, 33, 34, 413, 425, 8193, 12288, 12289, 12291, 34816, 34821, 40960, 40961)] + \
         [(34816, True), (48700, True), (49153, True)]
CELLS = [(T, two, K) for T, two in SHAPES for K in (KS if T in ALL_K_T and not two else (256, 1024))]


def _G(dev, rows, cols, dtype):
    from test_gpu_gemm import Guarded

    return Guarded(dev, rows, cols, dtype)


def _wide(dev, t):
    """``t`` as a column slice of a wider NaN-filled buffer (leading dimension K + 16)."""
    from test_gpu_gemm import _operand

    return _operand(dev, t)


def _untouched(g, what):
    torch.cuda.synchronize()
    assert bool((g.raw == g.pat).all()), f"{what}: written although the launch has no such output"


def _fig(kernel, fig, **kw):
    stages = {k: ({kk: (round(vv, 4) if kk == "ratio" else float(f"{vv:.2e}")) for kk, vv in v.items()} if "ratio" in v else v)
              for k, v in fig.items()}
    print("ROWGEMMFIG " + json.dumps(dict(kernel=kernel, **kw, stages=stages)))


def _merge(fig, part):
    for k, v in part.items():
        old = fig.get(k)
        if old is None:
            fig[k] = dict(v)
        elif "ratio" in v:
            fig[k] = dict(ratio=max(old["ratio"], v["ratio"]), rel=max(old["rel"], v["rel"]))
        else:
            fig[k] = dict(exact=old["exact"] and v["exact"])


def _to(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def _policy(monkeypatch, two):
    if two:
        monkeypatch.setenv("G2048_RG_TWO_TILES", "1")  # (the library reads it per call)
    else:
        monkeypatch.delenv("G2048_RG_TWO_TILES", raising=False)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=2)
def _ln(T, dev):
    return _to(rr.ln_inputs(T), dev)


@functools.lru_cache(maxsize=2)
def _ln_a(T, dev):
    return _to(rr.ln_bwd_tier_a(T), dev)


@functools.lru_cache(maxsize=4)
def _fwd_operands(T, K, tier_a, bias, dev):
    from src.g2048 import native as nv

    u, W, b = rg.fwd_tier_a(T, K, bias) if tier_a else rg.fwd_tier_b(T, K, bias)
    u, W, b = u.to(dev), W.to(dev), None if b is None else b.to(dev)
    return u, W, b, nv.pack_fragments(W)


@functools.lru_cache(maxsize=2)
def _bwd_operands(T, K, tier_a, wide, dev):
    """-> dy, the logical Wt [256, K], the packed weight the launch is pointed at, its tile stride, extra [T // 17, 256]."""
    from src.g2048 import native as nv

    I = _to(rg.bwd_tier_a(T, K, wide) if tier_a else rg.bwd_tier_b(T, K, wide), dev)
    packed, stride, Wt = nv.pack_fragments(I["Wt"]), 0, I["Wt"]
    if wide:  # the last K columns of the wide matrix: k-steps (wide - K) / 16 .. of every 32-row tile
        packed, stride, Wt = packed[((wide - K) // 16) * 512:], (wide // 16) * 512, I["Wt"][:, wide - K:].contiguous()
    return I["dy"], Wt, packed, stride, I["extra"][:T // 17].contiguous()


@functools.lru_cache(maxsize=2)
def _stats_b(T, dev, state_word):
    """xn, mean, rstd of a forward launch (g2048_add_ln_fwd at p = 0.1) on rr.ln_inputs."""
    from src.g2048 import native as nv

    I = _ln(T, dev)
    state = torch.tensor([state_word], dtype=torch.int64, device=dev)
    xn, mean, rstd = torch.empty(T, D, device=dev), torch.empty(T, device=dev), torch.empty(T, device=dev)
    nv.add_ln_fwd(I["x"].data_ptr(), D, I["a"], I["gamma"], I["beta"], xn, torch.empty(T, D, dtype=BF16, device=dev), mean, rstd, T, EPS, 0.1, SEED,
                  state.data_ptr())
    torch.cuda.synchronize()
    return xn, mean, rstd


# ------------------------------------------------------------------------------------------------------------------- forward
def _fwd_launch(dev, T, K, tier_a, p, variant, state, seed=SEED):
    """One guarded launch of g2048_linear_add_ln_fwd -> (inputs for the check, outputs)."""
    from src.g2048 import native as nv

    L = _ln(T, dev)
    u, W, b, Wp = _fwd_operands(T, K, tier_a, variant != "nobias" or not tier_a, dev)  # (tier A without a bias: operands of their own range)
    if variant == "nobias":
        b = None
    ud = _wide(dev, u) if variant == "wide_u" else u
    x = L["x"]
    if variant == "strided_x":
        full = torch.full((T, 17, D), float("nan"), device=dev)
        full[:, 0] = x
        xptr, xrs = full.data_ptr(), 17 * D
    else:
        xptr, xrs = x.data_ptr(), D
    xg, hg, mg, sg = _G(dev, T, D, F32), _G(dev, T, D, BF16), _G(dev, 1, T, F32), _G(dev, 1, T, F32)
    rc = nv.load().g2048_linear_add_ln_fwd(ud.data_ptr(), ud.stride(0), Wp.data_ptr(), _ptr(b), K, xptr, xrs, L["gamma"].data_ptr(), L["beta"].data_ptr(),
                                           xg.view.data_ptr(), hg.view.data_ptr(), mg.view.data_ptr(), sg.view.data_ptr(), T, EPS, float(p), seed,
                                           _ptr(state), _stream())
    assert rc == 0, rc
    O = dict(x_new=xg.take(f"x_new {variant}"), h=hg.take(f"h {variant}"), mean=mg.take("mean")[0], rstd=sg.take("rstd")[0])
    return (u, W, b, x, L["gamma"], L["beta"]), O


def _fwd(dev, T, K, tier_a, p, variant, state, seed=SEED):
    (u, W, b, x, gamma, beta), O = _fwd_launch(dev, T, K, tier_a, p, variant, state, seed)
    fig = {}
    word = None if state is None else int(state.item())
    return rg.fwd_check(u, W, b, x, gamma, beta, EPS, p, seed, word, O["x_new"], O["h"], O["mean"], O["rstd"], tier_a, fig), fig


@pytest.mark.parametrize("T,two,K", CELLS)
def test_linear_add_ln_fwd(dev, monkeypatch, T, two, K):
    _policy(monkeypatch, two)
    state = torch.tensor([STATE], dtype=torch.int64, device=dev)
    if T <= FULL_PRODUCT_T:
        cells = [(a, p, v) for a in (True, False) for p in (0.0, 0.1, 0.5) for v in ("full", "nobias", "wide_u", "strided_x")]
    else:
        cells = [(True, 0.5, "full"), (False, 0.1, "full"), (False, 0.1, "nobias"), (True, 0.0, "wide_u"), (False, 0.1, "strided_x")]
    failures, fig = [], {}
    for tier_a, p, variant in cells:
        f, part = _fwd(dev, T, K, tier_a, p, variant, state)
        failures += [f"tier {'A' if tier_a else 'B'} p {p} {variant}: {m}" for m in f]
        _merge(fig, {k + (" tier A" if tier_a and k[:2] in ("A2", "A3") else ""): v for k, v in part.items()})
    _fig("linear_add_ln_fwd", fig, T=T, K=K, two_tiles=two, plan=rg.tile_plan(T, two))
    assert not failures, failures
    if T >= 3:  # the precondition of the truncation check: element 545 is ON the threshold of p = 0.1, and kept
        assert int(rr.hash32(np.array([545], dtype=np.uint64), *rr.seed_words(SEED))[0]) >> 8 == rr.thr24(0.1)


def test_linear_add_ln_fwd_seed_state_word(dev, monkeypatch):
    """The device word enters the hash as rowwise_ref states, is read at launch time (moved between two launches); another word, no word
    and the word 0 draw the masks the restated hash gives, and they differ."""
    _policy(monkeypatch, False)
    T, K = 413, 512
    state, fig, xs = torch.tensor([STATE], dtype=torch.int64, device=dev), {}, []
    for tier_a in (True, False):
        for word in (STATE, STATE2, 0):
            state.fill_(word)
            f, part = _fwd(dev, T, K, tier_a, 0.5, "full", state)
            assert not f, (hex(word), f)
            _merge(fig, part)
        f, part = _fwd(dev, T, K, tier_a, 0.1, "full", None)  # no word: the threshold element of the seed itself
        assert not f, f
        f, part = _fwd(dev, T, K, tier_a, 0.5, "full", None, seed=7)  # a seed without high bits
        assert not f, f
    for word in (STATE, STATE2):
        state.fill_(word)
        xs.append(_fwd_launch(dev, T, K, True, 0.5, "full", state)[1]["x_new"])
    assert not torch.equal(xs[0], xs[1])
    k = [rr.row_keep(SEED, w, T, 0.5, "cpu") for w in (STATE, STATE2, None)]
    assert not torch.equal(k[0], k[1]) and not torch.equal(k[0], k[2]) and torch.equal(k[2], rr.row_keep(SEED, 0, T, 0.5, "cpu"))
    _fig("linear_add_ln_fwd seed_state", fig, T=T, K=K)


# ------------------------------------------------------------------------------------------------------------------- backward
BWD_VARIANTS = ("full", "no_gx", "no_da", "wide_dy")


def _bwd_launch(dev, T, K, tier_a, p, variant, state, two):
    from src.g2048 import native as nv

    lib = nv.load()
    dy, Wt, packed, stride, extra = _bwd_operands(T, K, tier_a, 768 if variant == "window" else None, dev)
    if tier_a:
        L = _ln_a(T, dev)
        xn, mean, rstd, gamma, gx_all = L["xn"], L["mean"], L["rstd"], L["gamma"], L["g_x"]
    else:
        xn, mean, rstd = _stats_b(T, dev, int(state.item()))
        gamma, gx_all = _ln(T, dev)["gamma"], _ln(T, dev)["g_x"]
    period = 17 if variant in ("gx17", "extra17") else 1
    g_x = None if variant == "no_gx" else gx_all[:T // period].contiguous()
    extra = extra if variant == "extra17" else None
    dyd = _wide(dev, dy) if variant == "wide_dy" else dy
    grid = int(lib.g2048_linear_add_ln_bwd_partial_rows(T))
    assert grid == rg.tile_plan(T, two)[3], (T, two, grid, rg.tile_plan(T, two))
    dxg, dag, pg = _G(dev, T, D, F32), _G(dev, T, D, BF16), _G(dev, grid, 3 * D, F32)
    rc = lib.g2048_linear_add_ln_bwd(dyd.data_ptr(), dyd.stride(0), packed.data_ptr(), stride, K, xn.data_ptr(), D, _ptr(g_x), period, _ptr(extra), 17,
                                     mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), dxg.view.data_ptr(),
                                     None if variant == "no_da" else dag.view.data_ptr(), pg.view.data_ptr(), T, float(p), SEED, state.data_ptr(), _stream())
    assert rc == 0, rc
    dx = dxg.take(f"dx {variant}")
    da = _untouched(dag, "da") if variant == "no_da" else dag.take(f"da {variant}")
    partial = pg.take(f"partial {variant}")
    return (dy, Wt, xn, g_x, period, extra, mean, rstd, gamma), dict(dx=dx, da=da, partial=partial), grid


def _bwd(dev, T, K, tier_a, p, variant, state, two):
    (dy, Wt, xn, g_x, period, extra, mean, rstd, gamma), O, grid = _bwd_launch(dev, T, K, tier_a, p, variant, state, two)
    fig = {}
    gid = rg.group_of_row(T, two, dev)
    f = rg.bwd_check(dy, Wt, xn, g_x, period, extra, 17, mean, rstd, gamma, p, SEED, int(state.item()), O["dx"], O["da"], O["partial"], gid, grid,
                     tier_a, fig)
    if variant == "no_da":
        assert not bool(O["partial"].reshape(grid, 3, D)[:, 2].any()), "da NULL: its column sums are exactly zero"
    return f, fig


@pytest.mark.parametrize("T,two,K", CELLS)
def test_linear_add_ln_bwd(dev, monkeypatch, T, two, K):
    _policy(monkeypatch, two)
    state = torch.tensor([STATE], dtype=torch.int64, device=dev)
    variants = BWD_VARIANTS + (("window",) if K == 512 else ()) + (("gx17", "extra17") if T % 17 == 0 else ())
    if T <= FULL_PRODUCT_T:
        cells = [(a, p, v) for a, p in ((True, 0.0), (True, 0.5), (False, 0.1)) for v in variants]
    else:
        cells = [(True, 0.5, "full"), (False, 0.1, "full"), (True, 0.0, "no_gx"), (False, 0.1, "no_da"), (True, 0.5, "wide_dy")]
        cells += [(a, p, "window") for a, p in ((True, 0.5), (False, 0.1)) if K == 512]
        cells += [(False, 0.1, "gx17"), (True, 0.5, "extra17"), (False, 0.1, "extra17")] if T % 17 == 0 else []
    failures, fig = [], {}
    for tier_a, p, variant in cells:
        f, part = _bwd(dev, T, K, tier_a, p, variant, state, two)
        failures += [f"tier {'A' if tier_a else 'B'} p {p} {variant}: {m}" for m in f]
        _merge(fig, {k + (" tier A" if tier_a and k[:2] in ("A4", "A6") else ""): v for k, v in part.items()})
    _fig("linear_add_ln_bwd", fig, T=T, K=K, two_tiles=two, plan=rg.tile_plan(T, two))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------- the rest
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


@pytest.mark.parametrize("T,K", [(413, 768), (40961, 1024)])
def test_two_launches_are_bit_identical(dev, monkeypatch, T, K):
    """The same inputs twice: every output the same bits (40961: workgroup 0's partial is the sum of two tiles, in a fixed order)."""
    _policy(monkeypatch, False)
    state = torch.tensor([STATE], dtype=torch.int64, device=dev)
    runs = [(_fwd_launch(dev, T, K, False, 0.1, "full", state)[1], _bwd_launch(dev, T, K, False, 0.1, "full", state, False)[1]) for _ in range(2)]
    for a, b in zip(runs[0], runs[1]):
        for k in a:
            assert torch.equal(_bits(a[k]), _bits(b[k])), (T, K, k)
    print("ROWGEMMFIG " + json.dumps(dict(kernel="two launches", T=T, K=K, identical=True)))


def test_a_period_that_does_not_divide_T_is_refused(dev, monkeypatch):
    """g_x is [T / g_x_period][256], g_h_extra [T / extra_period][256]: with T = 18 and period 17 the token row 17 would read the row behind
    them.  The same launches without that operand, and with T = 34, go through."""
    from src.g2048 import native as nv

    _policy(monkeypatch, False)
    K = 256
    for T, ok in ((18, False), (34, True)):
        I, L = _to(rg.bwd_tier_b(T, K), dev), _ln(T, dev)
        xn, mean, rstd = _stats_b(T, dev, STATE)
        Wp = nv.pack_fragments(I["Wt"])
        g17 = L["g_x"][:T // 17].contiguous()
        e17 = I["extra"][:T // 17].contiguous()
        dx, da = torch.empty(T, D, device=dev), torch.empty(T, D, dtype=BF16, device=dev)
        g_h = torch.zeros(T, D, dtype=BF16, device=dev)
        fused = lambda g_x, period, extra: nv.linear_add_ln_bwd(I["dy"], Wp, xn.data_ptr(), D, g_x, mean, rstd, L["gamma"], dx, da, 0.1, SEED,
                                                                g_x_period=period, g_h_extra=extra, extra_period=17)
        unfused = lambda g_x, period: nv.add_ln_bwd(xn.data_ptr(), D, g_x, g_h, mean, rstd, L["gamma"], dx, da, None, T, 0.1, SEED, g_x_period=period)
        calls = [lambda: fused(g17, 17, None), lambda: fused(None, 1, e17), lambda: fused(L["g_x"], 1, e17), lambda: unfused(g17, 17)]
        for call in calls:
            if ok:
                call()
            else:
                with pytest.raises(nv.NativeError):
                    call()
        fused(None, 17, None)  # without the operand the period is not looked at
        fused(L["g_x"], 1, None)
        unfused(None, 17)
        unfused(L["g_x"], 1)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(dx).all())
