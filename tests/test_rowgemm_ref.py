"""tests/rowgemm_ref.py held to itself on the CPU: an f32 / bf16 emulation of g2048_linear_add_ln_fwd / _bwd (the emulation of
tests/test_rowwise_ref.py behind an f32 matmul on the bf16 operands, the bias added in f32 before the ONE bf16 rounding, and the tile /
workgroup grouping of ``tile_plan``) must pass every rule of both tiers, with the whole-tensor error of every bounded output below
``gr.REL_LIMIT / 2``; every planted defect must be rejected by the stage that owns it; ``tile_plan`` must give the hand-written table.

Worst error / bound of the emulation per bounded stage (printed as ROWGEMMFIG lines; the exact stages are bit-equal, dx of tier A has error 0):
    B1 x_new 0.979   A2 mean 0.009, rstd 0.009   A3 h 0.987   A4 dx 0.707   A6 dgamma 0.846, dbeta 0.826, da sums 0.013
and the worst whole-tensor error 1.88e-3 (h of a single row), against REL_LIMIT / 2 = 2e-3: one bf16 rounding costs 1.65e-3 on average.
"""
import json

import numpy as np
import pytest
import torch

import gemm_ref as gr
import rowgemm_ref as rg
import rowwise_ref as rr
from test_rowwise_ref import _inv, _keep24_rounded, _owners, emu_add_ln_bwd, emu_add_ln_fwd

BF16, F32 = gr.BF16, gr.F32
SEED = 0xF234_5678_F234_406F  # the seed of tests/test_gpu_rowwise.py: element 545 sits exactly ON the 24-bit threshold of p = 0.1
STATE = 0x7654_3210_89AB_CDEF
EPS = 1e-5
D = 256
KS = (256, 512, 768, 1024)
HALF = gr.REL_LIMIT / 2


def _fig(kernel, fig, **kw):
    print("ROWGEMMFIG " + json.dumps(dict(kernel=kernel, **kw, stages={k: ({kk: (round(vv, 4) if kk == "ratio" else float(f"{vv:.2e}")) for kk, vv in v.items()}
                                                                       if "ratio" in v else v) for k, v in fig.items()})))


def _merge(fig, part):
    for k, v in part.items():
        old = fig.get(k)
        if old is None:
            fig[k] = dict(v)
        elif "ratio" in v:
            fig[k] = dict(ratio=max(old["ratio"], v["ratio"]), rel=max(old["rel"], v["rel"]))
        else:
            fig[k] = dict(exact=old["exact"] and v["exact"])


def _condition(fig, what):
    """Every exact stage bit-equal, every bounded one inside its bound, and its whole-tensor error below REL_LIMIT / 2."""
    for k, v in fig.items():
        assert v.get("exact", True) and v.get("ratio", 0) <= 1 and v.get("rel", 0) < HALF, (what, k, v)


# ------------------------------------------------------------------------------------------------------------------- emulation
def _window_without_stride(wt_full, K):
    """Defect 5.  The kernel is handed K = 512 columns (k-steps 16..47) of a packed [256][768]: 32-row tile w, k-step g of the window sits at
    the 512-element block 48 w + 16 + g.  With the dense stride (32 blocks per tile) it reads block 32 w + 16 + g instead: tile
    (32 w + 16 + g) // 48, k-step (32 w + 16 + g) % 48 of the wide matrix."""
    out = torch.empty(D, K, dtype=wt_full.dtype)
    for w in range(8):
        for g in range(K // 16):
            b = 32 * w + 16 + g
            out[32 * w:32 * w + 32, 16 * g:16 * g + 16] = wt_full[32 * (b // 48):32 * (b // 48) + 32, 16 * (b % 48):16 * (b % 48) + 16]
    return out


def emu_gemm(x, w, bias, defect=None):
    """-> the [T, 256] tile as the row pass reads it (bf16; f32 under the defects that leave it unrounded)."""
    xf, wf = x.to(F32), w.to(F32)
    if defect == "k_tail":
        xf, wf = xf[:, :-128], wf[:, :-128]
    acc = xf @ wf.t()
    if bias is None:
        return acc.to(BF16)
    if defect == "no_round":
        return acc + bias
    if defect == "bias_late":
        return (acc.to(BF16).to(F32) + bias).to(BF16)
    if defect == "bias_224":
        return (acc + torch.where(torch.arange(D) < 224, bias, torch.zeros(()))).to(BF16)
    return (acc + bias).to(BF16)


def emu_fwd(u, W, bias, x, gamma, beta, p, seed, state, tpw, defect=None):
    a = emu_gemm(u, W, bias, defect)
    T = x.shape[0]
    if defect == "local_row":  # the mask drawn on the row inside the tile: every tile is a launch of its own
        parts = [emu_add_ln_fwd(x[t:t + tpw], a[t:t + tpw], gamma, beta, EPS, p, seed, state) for t in range(0, T, tpw)]
        O = {k: torch.cat([q[k] for q in parts]) for k in parts[0]}
    else:
        O = emu_add_ln_fwd(x, a, gamma, beta, EPS, p, seed, state, defect if defect in ("thr_round", "no_state", "stride255") else None)
    if defect == "last_row":
        O["x_new"][T - 1] = float("nan")
    return O


def emu_bwd(I, L, g_x, period, extra, extra_period, p, seed, state, with_da, plan, defect=None):
    """I: dy, Wt; L: xn, mean, rstd, gamma; plan = (nb, tpw, tiles, grid) -> dx, da, partial [grid, 768]."""
    _, tpw, tiles, grid = plan
    wt = I["Wt"] if defect != "no_stride" else _window_without_stride(I["Wt_full"], I["dy"].shape[1])
    g_h = emu_gemm(I["dy"], wt, None, defect)
    T = g_h.shape[0]
    tok = torch.arange(T)
    local = tok % tpw
    if extra is not None:
        rows = tok[tok % extra_period == (1 if defect == "extra_row1" else 0)]
        s = g_h[rows].to(F32) + extra[:len(rows)].to(F32)
        if defect == "extra_unrounded":
            g_h = g_h.to(F32)
            g_h[rows] = s
        else:
            g_h[rows] = s.to(BF16)
    gx = torch.zeros(T, D)
    if g_x is not None:
        idx = local if defect == "gx_local" else tok
        rows = tok[idx % period == 0]
        gx[rows] = g_x[(idx[rows] // period).clamp_max(g_x.shape[0] - 1)]
    O = emu_add_ln_bwd(L["xn"], gx, 1, g_h, L["mean"], L["rstd"], L["gamma"], p, seed, state, False, T)
    dx = O["dx"]
    da, written = None, torch.zeros(T, D)
    if with_da:
        keep = rr.row_keep(seed, state, T, p, "cpu")
        if defect == "local_row":
            keep = keep[local]
        scaled = torch.where(keep, dx * _inv(p), torch.zeros(()))
        da = scaled.to(BF16)
        written = scaled if defect == "sums_f32" else da.to(F32)
    xh = (L["xn"] - L["mean"].reshape(T, 1)) * L["rstd"].reshape(T, 1)
    ghf = g_h.to(F32)
    terms = torch.stack([ghf * xh, ghf, written], 1).reshape(T, 3 * D)
    tile = tok // tpw
    if defect == "overwrite":  # only the last tile a workgroup walks is left in its partial row
        last = torch.zeros(grid, dtype=torch.long).scatter_reduce_(0, tile % grid, tile, "amax")
        terms = torch.where((tile == last[tile % grid])[:, None], terms, torch.zeros(()))
    partial = torch.zeros(grid, 3 * D).index_add_(0, tile % grid, terms)
    if defect == "duplicate" and T % tpw:  # the clamped copy of the partial tile's last row, counted once more
        partial[(tiles - 1) % grid] += terms[T - 1]
    if defect == "last_row":
        dx = dx.clone()
        dx[T - 1] = float("nan")
    return dict(dx=dx, da=da, partial=partial)


# ------------------------------------------------------------------------------------------------------------------- cases
def _fwd_case(T, K, tier_a, p, bias=True, state=STATE, defect=None, max_grid=rg.MAX_GRID):
    u, W, b = rg.fwd_tier_a(T, K, bias) if tier_a else rg.fwd_tier_b(T, K, bias)
    L = rr.ln_inputs(T)
    tpw = rg.tile_plan(T, False, max_grid)[1]
    O = emu_fwd(u, W, b, L["x"], L["gamma"], L["beta"], p, SEED, state, tpw, defect)
    fig = {}
    return rg.fwd_check(u, W, b, L["x"], L["gamma"], L["beta"], EPS, p, SEED, state, O["x_new"], O["h"], O["mean"], O["rstd"], tier_a, fig), fig


def _bwd_case(T, K, tier_a, p, variant="full", defect=None, max_grid=rg.MAX_GRID, state=STATE):
    """variant: full | no_gx | no_da | gx17 | extra17 | window (K = 512 columns of a [256, 768])."""
    wide = 768 if variant == "window" else None
    I = dict(rg.bwd_tier_a(T, K, wide) if tier_a else rg.bwd_tier_b(T, K, wide))
    if wide:
        I["Wt_full"], I["Wt"] = I["Wt"], I["Wt"][:, 256:].contiguous()
    if tier_a:
        L = rr.ln_bwd_tier_a(T)
    else:
        L = rr.ln_inputs(T)
        F = emu_add_ln_fwd(L["x"], L["a"], L["gamma"], L["beta"], EPS, p, SEED, state)
        L = dict(xn=F["x_new"], mean=F["mean"], rstd=F["rstd"], gamma=L["gamma"], g_x=L["g_x"])
    period = 17 if variant in ("gx17", "extra17") else 1
    g_x = None if variant == "no_gx" else L["g_x"][:T // period]
    extra = I["extra"][:T // 17] if variant == "extra17" else None
    plan = rg.tile_plan(T, False, max_grid)
    O = emu_bwd(I, L, g_x, period, extra, 17, p, SEED, state, variant != "no_da", plan, defect)
    fig = {}
    gid = rg.group_of_row(T, False, "cpu", max_grid)
    f = rg.bwd_check(I["dy"], I["Wt"], L["xn"], g_x, period, extra, 17, L["mean"], L["rstd"], L["gamma"], p, SEED, state, O["dx"], O["da"],
                     O["partial"], gid, plan[3], tier_a, fig)
    return f, fig


CASES = [(1, rg.MAX_GRID), (9, rg.MAX_GRID), (33, rg.MAX_GRID), (413, rg.MAX_GRID), (413, 5)]  # (413, 5): 13 tiles on 5 workgroups


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("T,max_grid", CASES)
def test_fwd_emulation(T, max_grid, K):
    fig = {}
    for tier_a in (True, False):
        for p in (0.0, 0.1, 0.5):
            for bias in (True, False):
                f, part = _fwd_case(T, K, tier_a, p, bias, max_grid=max_grid)
                assert not f, (tier_a, p, bias, f)
                _merge(fig, part)
    _fig("linear_add_ln_fwd emulation", fig, T=T, K=K)
    _condition(fig, (T, K))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("T,max_grid", CASES + [(34, rg.MAX_GRID), (425, 5)])
def test_bwd_emulation(T, max_grid, K):
    fig = {}
    variants = ["full", "no_gx", "no_da"] + (["window"] if K == 512 else []) + (["gx17", "extra17"] if T % 17 == 0 else [])
    for tier_a, p in ((True, 0.0), (True, 0.5), (False, 0.1)):
        for variant in variants:
            f, part = _bwd_case(T, K, tier_a, p, variant, max_grid=max_grid)
            assert not f, (tier_a, p, variant, f)
            _merge(fig, {k + (" tier A" if tier_a and k.startswith("A6") else ""): v for k, v in part.items()})
    _fig("linear_add_ln_bwd emulation", fig, T=T, K=K)
    _condition(fig, (T, K))


@pytest.mark.parametrize("K", KS)
def test_tier_a_preconditions(K):
    """What the issue states about the integer operands, at 320 rows (two 160-token tiles of one workgroup)."""
    I, L = rg.bwd_tier_a(320, K), rr.ln_bwd_tier_a(320)
    ref = gr.linear(I["dy"], I["Wt"])
    need, ties = gr.assert_exercises_rounding(ref)
    assert 0.75 <= need <= 0.97 and 0.04 <= ties <= 0.20, (need, ties)
    g_h = rg.gemm_a(I["dy"], I["Wt"])
    a = gr.f64(g_h) * gr.f64(L["gamma"])
    assert not bool(a.sum(1).any()) and not bool((a * gr.f64(L["xn"])).sum(1).any())  # c1 = c2 = 0
    assert float(gr.f64(g_h).abs().sum(0).max()) <= 1.5e6  # (1.47e6 at K = 1024: a ninth of 2^24)
    need, ties = gr.assert_exercises_rounding(gr.linear(*rg.fwd_tier_a(320, K, True)))
    assert need >= 0.7 and ties >= 0.1, (need, ties)
    ge = rg.add_extra_a(g_h[:34], I["extra"][:2], 17)
    assert torch.equal(ge[:, 4:8].float(), -ge[:, 0:4].float()) and not torch.equal(ge[0], g_h[0])


def test_the_seed_has_an_element_on_the_threshold():
    assert int(rr.hash32(np.array([545], dtype=np.uint64), *rr.seed_words(SEED))[0]) >> 8 == rr.thr24(0.1) == 1677721
    assert rr.keep24(SEED, None, np.array([545]), 0.1)[0] and not _keep24_rounded(SEED, None, 3, 0.1)[2, 33]


# ------------------------------------------------------------------------------------------------------------------- planted defects
def _exact_failed(fig, stage):
    return fig.get(stage, {}).get("exact") is False


@pytest.mark.parametrize("defect", ("no_round", "bias_late", "bias_224"))
def test_gemm_rounding_defects_are_rejected_by_a1(defect):
    """1, 2, 3: tier A, stage A1."""
    for K in KS:
        f, fig = _fwd_case(33, K, True, 0.5, defect=defect)
        assert "A1" in _owners(f) and _exact_failed(fig, "A1 x_new"), (defect, K, f)


@pytest.mark.parametrize("K", KS)
def test_short_k_is_rejected_by_both_tiers(K):
    """4: the last 128 columns of K left out."""
    f, fig = _fwd_case(33, K, True, 0.0, defect="k_tail")
    assert "A1" in _owners(f)
    f, fig = _fwd_case(33, K, False, 0.0, defect="k_tail")
    assert "B1" in _owners(f) and fig["B1 x_new"]["ratio"] > 10
    f, fig = _bwd_case(33, K, True, 0.5, defect="k_tail")
    assert {"A4", "A6"} <= _owners(f) and fig["A4 dx"]["ratio"] > 100
    f, fig = _bwd_case(33, K, False, 0.1, defect="k_tail")
    assert {"A4", "A6"} <= _owners(f) and fig["A4 dx"]["ratio"] > 10


def test_ignored_tile_stride_is_rejected_by_both_tiers():
    """5."""
    f, fig = _bwd_case(33, 512, True, 0.5, "window", "no_stride")
    assert {"A4", "A6"} <= _owners(f) and fig["A4 dx"]["ratio"] > 100
    f, fig = _bwd_case(33, 512, False, 0.1, "window", "no_stride")
    assert {"A4", "A6"} <= _owners(f) and fig["A4 dx"]["ratio"] > 10


@pytest.mark.parametrize("defect,p,state", [("local_row", 0.5, STATE), ("stride255", 0.5, STATE), ("no_state", 0.1, STATE), ("thr_round", 0.1, None)])
def test_mask_defects_are_rejected_by_the_exact_mask_stages(defect, p, state):
    """6, 7, 8, 9: A1 in tier A; in tier B the dropped elements are no longer bit-equal to x (or kept ones far outside their bound)."""
    f, fig = _fwd_case(413, 256, True, p, state=state, defect=defect)
    assert "A1" in _owners(f) and _exact_failed(fig, "A1 x_new"), (defect, f)
    f, fig = _fwd_case(413, 256, False, p, state=state, defect=defect)
    assert "B1" in _owners(f) and (_exact_failed(fig, "B1 x_new dropped") or fig["B1 x_new"]["ratio"] > 100), (defect, f)
    if defect == "local_row":  # and the backward's da
        for tier_a, pp in ((True, 0.5), (False, 0.1)):
            f, fig = _bwd_case(413, 256, tier_a, pp, defect=defect)
            assert "A5" in _owners(f) and _exact_failed(fig, "A5 da"), (tier_a, f)


@pytest.mark.parametrize("defect,T,max_grid", [("duplicate", 33, rg.MAX_GRID), ("duplicate", 413, 5), ("overwrite", 413, 5)])
def test_partial_defects_are_rejected_by_a6_tier_a(defect, T, max_grid):
    """10, 11."""
    f, fig = _bwd_case(T, 256, True, 0.5, defect=defect, max_grid=max_grid)
    assert _owners(f) == {"A6"} and all(_exact_failed(fig, f"A6 {k}") for k in ("dgamma", "dbeta", "da sums")), f
    # Tier B sees a lost tile, and a row counted twice into a group of one row (256 x its half-ulp bound); one row too many among the 96 of
    # a workgroup with three tiles is 2.7 x the bound of the group's rounding errors: the integer tier owns that one.
    f, fig = _bwd_case(T, 256, False, 0.1, defect=defect, max_grid=max_grid)
    assert _owners(f) == {"A6"} and (T == 413 and defect == "duplicate" or fig["A6 dbeta"]["ratio"] > 10), f


@pytest.mark.parametrize("defect,variant,tier_a", [("gx_local", "gx17", False), ("gx_local", "gx17", True), ("extra_unrounded", "extra17", True),
                                                   ("extra_row1", "extra17", False), ("extra_row1", "extra17", True)])
def test_row_indexing_defects_are_rejected_by_the_bounded_dx(defect, variant, tier_a):
    """12, 13, 14.  (13 is an integer-tier matter: one missing rounding of g_h is what the tier-B bound of the rounding allows.)"""
    f, fig = _bwd_case(425, 256, tier_a, 0.5 if tier_a else 0.1, variant, defect)
    assert "A4" in _owners(f) and fig["A4 dx"]["ratio"] > (100 if defect != "extra_unrounded" else 1), (defect, f)


@pytest.mark.parametrize("tier_a,p", [(True, 0.5), (False, 0.1)])
def test_sums_of_the_unrounded_da_are_rejected(tier_a, p):
    """15."""
    f, fig = _bwd_case(33, 256, tier_a, p, defect="sums_f32")
    assert _owners(f) == {"A6"} and [m.split(":")[0] for m in f] == ["A6 da sums"], f
    assert _exact_failed(fig, "A6 da sums") if tier_a else fig["A6 da sums"]["ratio"] > 100


def test_an_unstored_last_row_is_rejected_by_the_guard_pattern(monkeypatch):
    """16: the buffer of the GPU tests (``Guarded``) around the emulation's outputs: the row the launch did not store still holds the NaN
    pattern, and ``take`` says so.  (The stage rules reject it as well: a NaN is never bit-equal nor inside a bound.)"""
    from test_gpu_gemm import Guarded

    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    T = 33
    u, W, b = rg.fwd_tier_b(T, 256)
    L = rr.ln_inputs(T)
    for defect in (None, "last_row"):
        O = emu_fwd(u, W, b, L["x"], L["gamma"], L["beta"], 0.1, SEED, STATE, 32, defect)
        g = Guarded("cpu", T, D, F32)
        g.view[:T if defect is None else T - 1] = O["x_new"][:T if defect is None else T - 1]
        if defect is None:
            assert torch.equal(g.take("x_new"), O["x_new"])
        else:
            with pytest.raises(AssertionError, match="unwritten"):
                g.take("x_new")
    f, _ = _fwd_case(T, 256, False, 0.1, defect="last_row")
    assert "B1" in _owners(f)
    f, _ = _bwd_case(T, 256, True, 0.5, defect="last_row")
    assert "A4" in _owners(f)
    g = Guarded("cpu", T, D, F32)
    g.view.copy_(L["x"])
    g.raw[(g.raw.shape[0] - T) // 2 + T, 0] = 0  # and a store one row below the output
    with pytest.raises(AssertionError, match="outside"):
        g.take("dx")


# ------------------------------------------------------------------------------------------------------------------- tile plan
PLAN = {  # (T, two tiles) -> (nb, tpw, tiles, grid), by hand from rg_tpw / rg_launch
    (1, False): (3, 32, 1, 1), (7, False): (3, 32, 1, 1), (8, False): (3, 32, 1, 1), (9, False): (3, 32, 1, 1),
    (17, False): (3, 32, 1, 1), (33, False): (3, 32, 2, 2), (34, False): (3, 32, 2, 2),  # 33: a second tile of one row
    (413, False): (3, 32, 13, 13), (425, False): (3, 32, 14, 14),                           # 413 = 12 x 32 + 29, 425 = 13 x 32 + 9
    (8193, False): (3, 33, 249, 249),       # ceil(8193 / 256) = 33; 248 x 33 = 8184: a last tile of 9 rows
    (12288, False): (3, 48, 256, 256),      # 48 x 256, the last T of the 96-token body
    (12289, False): (5, 49, 251, 251),      # ceil = 49 > 48: the 160-token body; 250 x 49 = 12250: 39 rows
    (12291, False): (5, 49, 251, 251),      # 17 x 723: 41 rows
    (34816, False): (5, 136, 256, 256),
    (34821, False): (5, 137, 255, 255),     # 254 x 137 = 34798: 23 rows
    (40960, False): (5, 160, 256, 256),
    (40961, False): (5, 160, 257, 256),     # workgroup 0 walks tile 256, one row
    (34816, True): (3, 68, 512, 256),       # ceil(34816 / 512) = 68: two tiles per workgroup
    (48700, True): (3, 96, 508, 256),       # ceil(48700 / 512) = 96; 507 x 96 = 48672: 28 rows
    (49153, True): (5, 97, 507, 256),       # ceil = 97 > 96: the 160-token body; 506 x 97 = 49082: 71 rows
}


def test_tile_plan_table():
    for (T, two), want in PLAN.items():
        assert rg.tile_plan(T, two) == want, (T, two, rg.tile_plan(T, two))
    assert rg.tile_plan(413, False, 5) == (3, 32, 13, 5)


@pytest.mark.parametrize("T,two,max_grid", [(1, False, 256), (33, False, 256), (413, False, 5), (40961, False, 256), (48700, True, 256), (49153, True, 256)])
def test_group_of_row_covers_every_row_once(T, two, max_grid):
    nb, tpw, tiles, grid = rg.tile_plan(T, two, max_grid)
    gid = rg.group_of_row(T, two, "cpu", max_grid)
    assert gid.shape == (T,) and int(gid.min()) == 0 and int(gid.max()) == grid - 1
    seen = torch.zeros(T, dtype=torch.long)
    for b in range(grid):  # the kernel's own walk: tiles b, b + grid, ..
        for tile in range(b, tiles, grid):
            rows = torch.arange(tile * tpw, min(T, (tile + 1) * tpw))
            assert bool((gid[rows] == b).all())
            seen[rows] += 1
    assert bool((seen == 1).all()) and tpw <= 32 * nb
