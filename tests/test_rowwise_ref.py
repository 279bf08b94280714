"""tests/rowwise_ref.py held to itself on the CPU: an f32 / bf16 emulation of every row-wise kernel (torch CPU ops at the kernels' rounding
points; the wave reductions as the butterfly of ``wave_sum``, the column sums in any order) must pass every stage rule, every planted
defect must be rejected by the stage that owns it, and the mask restatements must agree with a scalar transcription of the C expressions,
also at element indices at and above 2^32 (which no device test of this size reaches).

Worst error / bound of the emulation per bounded stage (printed as ROWFIG lines; the exact stages are bit-equal):
    A2 mean 0.003, rstd 0.007   A3 h 0.98   A4 dx 0.11   A6 dgamma 0.27, dbeta 0.006, da sums 0.012   R3 0.000 (sums of <= 37 bf16 values are
    exact in f32)   C1 0.002   E2 mean 0.002, rstd 0.008, h 0.99   E3 0.14   L1 new_logp 0.65   L2 means 0.07   L3 dlogits, L4 dvalues 0.98 (bf16 outputs)
The f32 results are held to any-order summation and running-error bounds, which a particular order stays far inside (tests/test_tail_ref.py
says why that cannot be tightened); the planted defects are orders of magnitude outside (each test asserts its owner's rejection).
"""
import json

import numpy as np
import pytest
import torch

import gemm_ref as gr
import rowwise_ref as rr

BF16, F32 = gr.BF16, gr.F32
SEED = 0xF234_5678_F234_406F  # bits above 32 set; low ^ high word = 5655, so below 2^32 elements it draws the mask of THR_SEED
THR_SEED = 5655  # element 545 hashes to exactly uint32(f32(0.1) 2^24) = 1677721 under this seed: kept when truncated, dropped when rounded
STATE = 0x7654_3210_89AB_CDEF
D = 256


def _fig(kernel, fig, **kw):
    print("ROWFIG " + json.dumps(dict(kernel=kernel, **kw, stages={k: ({kk: (round(vv, 4) if kk == "ratio" else float(f"{vv:.2e}")) for kk, vv in v.items()}
                                                                    if "ratio" in v else v) for k, v in fig.items()})))


def _owners(failures):
    return {m.split(" ")[0] for m in failures}


def wave_sum(v):
    """[T, 64] f32: the butterfly of g2048_bits.h's wave_sum; every lane ends with the same bits."""
    lanes = torch.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ m]
    return v[:, :1]


def _lane4(t):
    """[T, 256] -> [T, 64]: ((x + y) + z) + w of every lane's four columns."""
    q = t.reshape(t.shape[0], 64, 4)
    return ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]


def _inv(p):
    return torch.tensor(np.float32(rr.inv_of(p)))


def _keep24_rounded(seed, state, T, p):
    """The planted defect: thr from p 2^24 ROUNDED to nearest."""
    idx = np.arange(T * D, dtype=np.uint64).reshape(T, D)
    thr = int(np.rint(np.float64(np.float32(p)) * 2.0 ** 24))
    return torch.from_numpy((rr.hash32(idx, *rr.seed_words(seed, state)) >> np.uint64(8)) >= np.uint64(thr))


# ------------------------------------------------------------------------------------------------------------------- emulations
def emu_ln(v, gamma, beta, eps, defect=None):
    s = _lane4(v)
    if defect == "lane":
        s[:, 17] = 0
    mean = wave_sum(s) * np.float32(1.0 / D)
    d = v - mean
    var = wave_sum(_lane4(d * d)) * np.float32(1.0 / (255 if defect == "div255" else D))
    e = torch.full_like(var, np.float32(eps))
    if defect == "eps0":
        e[rr.eps_rows(v.shape[0])] = 0
    rstd = torch.rsqrt(var + e)
    return (d * rstd * gamma + beta).to(BF16), mean.reshape(-1), rstd.reshape(-1)


def emu_add_ln_fwd(x, a, gamma, beta, eps, p, seed, state, defect=None):
    T = x.shape[0]
    v, x_new = x, None
    if a is not None:
        if defect == "thr_round":
            keep = _keep24_rounded(seed, state, T, p)
        else:
            keep = rr.row_keep(seed, None if defect == "no_state" else state, T, p, "cpu", 255 if defect == "stride255" else D)
        v = x_new = x + torch.where(keep, a.to(F32) * _inv(p), torch.zeros(()))
    if gamma is None:
        return dict(x_new=x_new, h=v.to(BF16), mean=None, rstd=None)
    h, mean, rstd = emu_ln(v, gamma, beta, eps, defect)
    return dict(x_new=x_new, h=h, mean=mean, rstd=rstd)


def emu_add_ln_bwd(xn, g_x, period, g_h, mean, rstd, gamma, p, seed, state, with_da=True, rows_per_group=8, defect=None):
    T = g_h.shape[0]
    gh = g_h.to(F32)
    gx = torch.zeros(T, D)
    if g_x is not None:
        rows = torch.arange(1 if defect == "gx_row1" else 0, T, period)[:g_x.shape[0]]
        gx[rows] = g_x[:len(rows)]
    if gamma is None:
        xh = torch.zeros(T, D)
        dx = gx + gh
    else:
        m, r = mean.reshape(T, 1), rstd.reshape(T, 1)
        xh = (xn - m) * r
        dxh = gh * gamma
        c1 = wave_sum(_lane4(dxh)) * np.float32(1.0 / D)
        q, x4 = dxh.reshape(T, 64, 4), xh.reshape(T, 64, 4)
        s2 = torch.zeros(T, 64)
        for k in range(4):
            s2 = s2 + q[..., k] * x4[..., k]
        c2 = wave_sum(s2) * np.float32(1.0 / D)
        if defect == "no_c2":
            c2 = c2 * 0
        dx = gx + r * (dxh - c1 - xh * c2)
    da, written = None, torch.zeros(T, D)
    if with_da:
        da = torch.where(rr.row_keep(seed, state, T, p, "cpu"), dx * _inv(p), torch.zeros(())).to(BF16)
        written = da.to(F32)
    terms = torch.stack([gh * xh, gh, written], 1).reshape(T, 3 * D)
    if defect == "last_row":
        terms[T - 1] = 0
    G = -(-T // rows_per_group)
    partial = torch.zeros(G, 3 * D).index_add_(0, torch.arange(T) // rows_per_group, terms)
    dparams = partial.sum(0) - (partial[1] if defect == "no_partial" else 0)
    return dict(dx=dx, da=da, partial=partial, dparams=dparams.reshape(3, D))


def emu_relu_fwd(x, p, seed, state, defect=None):
    k = rr.keep16_pairs(seed, None if defect == "no_state" else state, x.numel(), p)
    if defect == "swap_halves":
        k = k.reshape(-1, 2)[:, ::-1].reshape(-1).copy()
    keep = torch.from_numpy(k).reshape(x.shape) & (x.to(F32) > 0)
    return torch.where(keep, x.to(F32) * _inv(p), torch.zeros(())).to(BF16)


def emu_relu_bwd(dy, y, p, rows_per_group=8):
    T = y.shape[0]
    dx = torch.where(y.to(F32) != 0, dy.to(F32) * _inv(p), torch.zeros(())).to(BF16)
    partial = torch.zeros(-(-T // rows_per_group), y.shape[1]).index_add_(0, torch.arange(T) // rows_per_group, dx.to(F32))
    return dx, partial, partial.sum(0)


def emu_embed_fwd(I, table, p, seed, state, ln_eps=None, defect=None):
    boards = I["boards"]
    M = boards.shape[0]
    e = rr.embed_classes(boards)
    pos = torch.arange(M * 17) % 17
    v = table[e.clamp_max(30)] + I["pe"][(pos - 1).clamp_min(0)]
    v = torch.where((e == 31)[:, None], I["cls"].expand(M * 17, D), v)
    keep = rr.embed_keep(seed, state, M, p, "cpu", drop_cls=defect == "drop_cls")
    x0 = torch.where(keep, v * _inv(p), torch.zeros(())) if rr.thr24(p) else v
    x0 = torch.where((e == 31)[:, None] & (defect != "drop_cls"), v, x0)
    return x0, (None if ln_eps is None else emu_ln(x0, I["gamma"], I["beta"], ln_eps))


def emu_embed_bwd(boards, g, p, seed, state, groups=1, defect=None):
    M = boards.shape[0]
    R = M * 17
    e = rr.embed_classes(boards)
    keep = rr.embed_keep(seed, state, M, p, "cpu")
    t = torch.where((e == 31)[:, None], g, torch.where(keep, g * _inv(p), torch.zeros(())))
    if defect == "swap_30_31":
        e = torch.where(e == 30, 31, torch.where(e == 31, 30, e))
    gid = (torch.arange(R) // (-(-R // groups))) * 32 + e
    return torch.zeros(groups * 32, D).index_add_(0, gid, t).reshape(groups, 32 * D)


def emu_ppo(I, clip_eps, c_value, c_entropy, scale=None, defect=None):
    f = lambda v: torch.tensor(np.float32(v))
    M = I["actions"].numel()
    l = I["logits"].to(F32).reshape(M, 4)
    bits = torch.full((M,), 15) if I["mask_bits"] is None else I["mask_bits"].long()
    legal = ((bits[:, None] >> torch.arange(4)) & 1).bool()
    z = l if defect == "mask_ignored" else torch.where(legal, l, l - f(1e8))
    zmax = z.max(1, keepdim=True).values
    se = torch.zeros(M)
    for j in range(4):
        se = se + torch.exp(z[:, j] - zmax[:, 0])
    lse = zmax[:, 0] + torch.log(se)
    lp = z - lse[:, None]
    pj = torch.exp(lp)
    ent = torch.zeros(M)
    for j in range(4):
        ent = ent - lp[:, j] * pj[:, j]
    a = (I["actions"].long() & 3).reshape(M, 1)
    nlp, olp, A = lp.gather(1, a)[:, 0], I["old_logp"], I["adv"]
    ratio = torch.exp(nlp - olp)
    lo, hi = f(1.0) - f(clip_eps), f(1.0) + f(clip_eps)
    s1, s2 = ratio * A, torch.minimum(torch.maximum(ratio, lo), hi) * A
    pl = -torch.minimum(s1, s2)
    dv = I["values"].to(F32) - I["ret"]
    vl, el = dv * dv, -ent
    tot = pl + f(c_value) * vl + f(c_entropy) * el
    inv_m = f(1.0) / f(M)
    terms = torch.stack([pl, vl, el, tot, olp - nlp], 1)
    sums = terms.sum(0) * inv_m
    in_range = ((ratio > lo) & (ratio < hi)) if defect == "open_clamp" else ((ratio >= lo) & (ratio <= hi))
    w1 = torch.where(s1 < s2, 1.0, torch.where(s1 == s2, 0.5, 0.0))
    w2 = 1.0 - w1
    if defect == "tie_full":
        w1 = torch.where(s1 == s2, 1.0, w1)
        w2 = torch.where(s1 == s2, 1.0, w2)
    g_lp = -(w1 + w2 * in_range.float()) * A * ratio
    g_m = inv_m if scale is None or defect == "no_scale" else inv_m * f(scale)
    onehot = torch.zeros(M, 4).scatter_(1, a, 1.0)
    et = f(c_entropy) * pj * (lp + ent[:, None])
    dz = g_lp[:, None] * (onehot - pj) + (-et if defect == "ent_sign" else et)
    return dict(new_logp=nlp, sums=sums, dlogits=(dz * g_m).to(I["logits"].dtype), dvalues=(f(2.0) * f(c_value) * dv * g_m).to(I["values"].dtype))


# ------------------------------------------------------------------------------------------------------------------- masks
def _scalar_hash(idx, seed, state):
    s0, s1, m = seed & 0xFFFFFFFF, seed >> 32, 0xFFFFFFFF
    if state is not None:
        s0 ^= ((state & m) * 0x9E3779B1) & m
        s1 = (s1 + (state >> 32) * 0x85EBCA77 + (state & m)) & m
    x = (((idx & m) * 0x9E3779B1) & m) ^ s0
    x ^= ((idx >> 32) * 0x85EBCA77 + s1) & m
    x ^= x >> 16
    x = (x * 0x7FEB352D) & m
    x ^= x >> 15
    x = (x * 0x846CA68B) & m
    return x ^ (x >> 16)


@pytest.mark.parametrize("state", (None, STATE, 0x1_0000_0003))
@pytest.mark.parametrize("p", (0.1, 0.5, 2.0 ** -20))
def test_masks_agree_with_the_scalar_transcription(p, state):
    starts = (0, 2 ** 32 - 64, 2 ** 32, 5 * 2 ** 32 + 12346, 2 ** 40 + 2)
    idx = np.concatenate([np.arange(s, s + 128, dtype=np.uint64) for s in starts])
    for seed in (7, SEED, 2 ** 64 - 1):
        thr = int(np.float32(p) * np.float32(16777216.0))
        got = rr.keep24(seed, state, idx, p)
        assert got.tolist() == [(_scalar_hash(int(i), seed, state) >> 8) >= thr for i in idx]
        thr16 = int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))
        for s in starts:
            got = rr.keep16_pairs(seed, state, 128, p, start=s)
            want = []
            for e in range(s, s + 128):
                h = _scalar_hash(e >> 1, seed, state)
                want.append(((h >> 16) if e & 1 else (h & 0xFFFF)) >= thr16)
            assert got.tolist() == want
    assert rr.keep24(1, None, idx, 0.0).all() and rr.keep24(1, None, idx, 2.0 ** -25).all()  # thr == 0: nothing is dropped


def test_the_threshold_seed_has_an_element_on_the_threshold():
    """Precondition of the truncation test here and on the device: element 545 (row 2, column 33) hashes to thr exactly."""
    thr = rr.thr24(0.1)
    assert thr == 1677721 and np.float32(0.1) * np.float32(16777216.0) == np.float32(1677721.625)
    for seed in (THR_SEED, SEED):
        assert int(rr.hash32(np.array([545], dtype=np.uint64), *rr.seed_words(seed, None))[0]) >> 8 == thr
    assert rr.keep24(THR_SEED, None, np.array([545]), 0.1)[0] and not _keep24_rounded(THR_SEED, None, 5, 0.1)[2, 33]
    assert gr.thr16(0.1) == 6554 and rr.thr24(0.1) >> 8 == 6553  # the three conversions of p = 0.1 differ


# ------------------------------------------------------------------------------------------------------------------- add + LN
def _ln_fwd_case(T, p, variant, defect=None, degenerate=False, seed=SEED, state=None):
    I = rr.ln_inputs(T, degenerate=degenerate)
    a = None if variant == "no_a" else I["a"]
    gamma, beta = (None, None) if variant == "no_ln" else (I["gamma"], I["beta"])
    O = emu_add_ln_fwd(I["x"], a, gamma, beta, 1e-5, p, seed, state, defect)
    fig = {}
    return rr.add_ln_fwd_check(I["x"], a, gamma, beta, 1e-5, p, seed, state, O["x_new"], O["h"], O["mean"], O["rstd"], fig), fig


@pytest.mark.parametrize("variant", ("full", "no_a", "no_ln"))
@pytest.mark.parametrize("p", (0.0, 0.1, 0.5))
@pytest.mark.parametrize("T", (1, 5, 41))
def test_add_ln_fwd_emulation(T, p, variant):
    failures, fig = _ln_fwd_case(T, p, variant, state=STATE if T == 5 else None, degenerate=T == 41)
    _fig("add_ln_fwd emulation", fig, T=T, p=p, variant=variant)
    assert not failures, failures
    assert all(v.get("exact", True) and v.get("ratio", 0) < 0.995 for v in fig.values())


@pytest.mark.parametrize("defect,owner,p,degenerate", [("thr_round", "A1", 0.1, False), ("no_state", "A1", 0.1, False), ("stride255", "A1", 0.5, False),
                                                       ("eps0", "A2", 0.0, True), ("div255", "A2", 0.0, False), ("lane", "A2", 0.0, False)])
def test_add_ln_fwd_defect_is_rejected(defect, owner, p, degenerate):
    failures, fig = _ln_fwd_case(5 if not degenerate else 41, p, "full", defect, degenerate, state=STATE if defect == "no_state" else None)
    assert owner in _owners(failures), (defect, failures)
    if defect in ("eps0", "div255"):
        assert any(m.startswith("A2 rstd") for m in failures) and fig["A2 rstd"]["ratio"] > 10
    if defect == "lane":
        assert any(m.startswith("A2 mean") for m in failures) and fig["A2 mean"]["ratio"] > 10


def _ln_bwd_case(T, p, variant, period=1, defect=None, tier_a=False, partials=False):
    rpg = 8
    if tier_a:
        I = rr.ln_bwd_tier_a(T)
        xn, mean, rstd, gamma = I["xn"], I["mean"], I["rstd"], I["gamma"]
    else:
        I = rr.ln_inputs(T)
        F = emu_add_ln_fwd(I["x"], I["a"], I["gamma"], I["beta"], 1e-5, p, SEED, None)
        xn, mean, rstd, gamma = F["x_new"], F["mean"], F["rstd"], I["gamma"]
    if variant == "no_ln":
        xn = mean = rstd = gamma = None
    g_x = None if variant == "no_gx" else I["g_x"][:T // period]
    O = emu_add_ln_bwd(xn, g_x, period, I["g_h"], mean, rstd, gamma, p, SEED, STATE, variant != "no_da", rpg, defect)
    fig = {}
    sums, rows = (O["partial"], rpg) if partials else (O["dparams"], None)
    return rr.add_ln_bwd_check(xn, g_x, period, I["g_h"], mean, rstd, gamma, p, SEED, STATE, O["dx"], O["da"], sums, rows, fig, tier_a), fig


@pytest.mark.parametrize("variant", ("full", "no_gx", "no_da", "no_ln"))
@pytest.mark.parametrize("T,period,tier_a,p,partials", [(1, 1, False, 0.1, False), (9, 1, False, 0.1, True), (34, 17, False, 0.1, False),
                                                        (33, 1, True, 0.5, True), (34, 17, True, 0.0, False), (7, 1, True, 0.5, False)])
def test_add_ln_bwd_emulation(T, period, tier_a, p, partials, variant):
    failures, fig = _ln_bwd_case(T, p, variant, period, None, tier_a, partials)
    _fig("add_ln_bwd emulation", fig, T=T, p=p, variant=variant, period=period, tier_a=tier_a)
    assert not failures, failures
    assert all(v.get("exact", True) and v.get("ratio", 0) < 0.9 for v in fig.values())


@pytest.mark.parametrize("defect,owner,period,tier_a,partials", [("no_c2", "A4", 1, False, False), ("gx_row1", "A4", 17, False, False),
                                                                 ("last_row", "A6", 1, True, False), ("last_row", "A6", 1, False, True),
                                                                 ("no_partial", "A6", 1, True, False), ("no_partial", "A6", 1, False, False)])
def test_add_ln_bwd_defect_is_rejected(defect, owner, period, tier_a, partials):
    failures, fig = _ln_bwd_case(34, 0.5 if tier_a else 0.1, "full", period, defect, tier_a, partials)
    assert owner in _owners(failures), (defect, failures)
    if owner == "A4":
        assert fig["A4 dx"]["ratio"] > 100
    elif not tier_a:
        assert max(fig[k]["ratio"] for k in fig if k.startswith("A6")) > 100


# ------------------------------------------------------------------------------------------------------------------- ReLU + dropout
@pytest.mark.parametrize("p", (0.0, 0.1, 0.5))
@pytest.mark.parametrize("T,F", [(1, 8), (5, 24), (37, 1024)])
def test_relu_dropout_emulation(T, F, p):
    I, fig = rr.relu_inputs(T, F), {}
    y = emu_relu_fwd(I["x"], p, SEED, STATE)
    failures = rr.relu_dropout_fwd_check(I["x"], p, SEED, STATE, y, fig)
    assert bool((y.view(torch.int16)[I["x"].float() <= 0] == 0).all())  # -0 and negatives give +0
    for tier_a in (False, True) if p != 0.1 else (False,):
        dy = I["dy_int"] if tier_a else I["dy"]
        dx, partial, dbias = emu_relu_bwd(dy, y, p)
        failures += rr.relu_dropout_bwd_check(dy, y, p, dx, dbias, None, fig, tier_a)
        failures += rr.relu_dropout_bwd_check(dy, y, p, dx, partial, 8, fig, tier_a)
    _fig("relu_dropout emulation", fig, T=T, F=F, p=p)
    assert not failures, failures


@pytest.mark.parametrize("defect", ("swap_halves", "no_state"))
def test_relu_dropout_defect_is_rejected(defect):
    I = rr.relu_inputs(37, 1024)
    y = emu_relu_fwd(I["x"], 0.1, SEED, STATE, defect)
    assert "R1" in _owners(rr.relu_dropout_fwd_check(I["x"], 0.1, SEED, STATE, y))
    y = emu_relu_fwd(I["x"], 0.5, SEED, STATE)
    dx, partial, dbias = emu_relu_bwd(I["dy"], y, 0.5)
    bad = dx.clone()
    bad[36] = (I["dy"][36].float() * 2).to(BF16)  # the last row ignores y
    assert "R2" in _owners(rr.relu_dropout_bwd_check(I["dy"], y, 0.5, bad, dbias))
    fig = {}
    assert "R3" in _owners(rr.relu_dropout_bwd_check(I["dy"], y, 0.5, dx, dbias - dx[36].float(), None, fig)) and fig["R3 dbias"]["ratio"] > 100
    assert "R3" in _owners(rr.relu_dropout_bwd_check(I["dy"], y, 0.5, dx, dbias - partial[1], None, fig)) and fig["R3 dbias"]["ratio"] > 100


# ------------------------------------------------------------------------------------------------------------------- colsum
@pytest.mark.parametrize("dtype", (BF16, F32))
@pytest.mark.parametrize("T,N", [(1, 4), (2, 12), (129, 256), (1031, 2048)])
def test_colsum_emulation(T, N, dtype):
    g = gr._gen(T, N, 15)
    xa = gr.ints((T, N), -8, 8, g).to(dtype)
    xb = gr.tier_b_rows(T, N, g, 0.3).to(dtype)
    fig = {}
    failures = rr.colsum_check(xa, xa.float().sum(0), fig, True, "C1 colsum tier A") + rr.colsum_check(xb, xb.float().sum(0), fig, False)
    _fig("colsum emulation", fig, T=T, N=N)
    assert not failures, failures
    if T > 1:
        assert "C1" in _owners(rr.colsum_check(xa, xa[:-1].float().sum(0), None, True))  # the last row missing, tier A
        # (tier B: a missing row is 1 / T of the column against a bound of (T + 1) 2^-23 of it, 3 x at T = 1031: the integer tier owns the long sums)
        assert "C1" in _owners(rr.colsum_check(xb, xb[:-1].float().sum(0), fig, False)) and (T > 129 or fig["C1 colsum"]["ratio"] > 100)


# ------------------------------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("p", (0.0, 0.1, 0.5))
@pytest.mark.parametrize("M", (1, 15, 16))
def test_embed_emulation(M, p):
    I, fig = rr.embed_inputs(M), {}
    x0, ln = emu_embed_fwd(I, I["table"], p, SEED, STATE, 1e-5)
    failures = rr.embed_fwd_check(I["boards"], I["table"], I["pe"], I["cls"], p, SEED, STATE, x0, fig, (I["gamma"], I["beta"], 1e-5) + ln)
    for tier_a in (False, True) if p != 0.1 else (False,):
        g = I["g_int"] if tier_a else I["g"]
        for groups in (1, 256):
            got = emu_embed_bwd(I["boards"], g, p, SEED, STATE, groups)
            failures += rr.embed_bwd_check(I["boards"], g, p, SEED, STATE, got, None if groups == 1 else groups, fig, tier_a)
            if groups == 1:
                empty = torch.bincount(rr.embed_classes(I["boards"]), minlength=32) == 0
                assert bool((got.reshape(32, D)[empty] == 0).all())
    _fig("embed emulation", fig, M=M, p=p)
    assert not failures, failures


def test_embed_defects_are_rejected():
    I = rr.embed_inputs(15)
    x0, _ = emu_embed_fwd(I, I["table"], 0.5, SEED, STATE, None, "drop_cls")
    assert "E1" in _owners(rr.embed_fwd_check(I["boards"], I["table"], I["pe"], I["cls"], 0.5, SEED, STATE, x0))
    for g, tier_a in ((I["g"], False), (I["g_int"], True)):
        got, fig = emu_embed_bwd(I["boards"], g, 0.5, SEED, STATE, 1, "swap_30_31"), {}
        assert "E3" in _owners(rr.embed_bwd_check(I["boards"], g, 0.5, SEED, STATE, got, None, fig, tier_a))
        assert tier_a or fig["E3 dwt_dcls"]["ratio"] > 100


# ------------------------------------------------------------------------------------------------------------------- ppo_loss
CV, CE = 0.5, 0.01


def _ppo_case(M, bf16, masks, clip_eps, scale, defect=None):
    I = rr.ppo_inputs(M, bf16, masks, clip_eps=clip_eps)
    first = emu_ppo(I, clip_eps, CV, CE, scale)
    planted = rr.ppo_plant(I, first["new_logp"], clip_eps)
    O = emu_ppo(I, clip_eps, CV, CE, scale, defect)
    ref = rr.ppo_loss_ref(I["logits"], I["values"], I["actions"], I["mask_bits"], I["old_logp"], I["adv"], I["ret"], clip_eps, CV, CE, scale)
    fig = {}
    return rr.ppo_loss_check(ref, O["new_logp"], O["sums"], O["dlogits"], O["dvalues"], fig, planted), fig, I, O, ref, planted


@pytest.mark.parametrize("M,bf16,masks,clip_eps,scale", [(1, False, False, 0.2, None), (63, False, True, 0.2, 1024.0), (63, True, True, 0.0, 1000.0),
                                                         (1025, False, True, 0.0, None), (1025, True, False, 0.2, 1024.0),
                                                         (2055, False, True, 0.2, 1000.0)])
def test_ppo_loss_emulation(M, bf16, masks, clip_eps, scale):
    failures, fig, I, O, ref, planted = _ppo_case(M, bf16, masks, clip_eps, scale)
    _fig("ppo_loss emulation", fig, M=M, bf16=bf16, masks=masks, clip_eps=clip_eps, scale=scale)
    assert not failures, failures
    assert rr.undecided_share(ref, planted) <= rr.UNDECIDED_CAP
    ratio = torch.exp(O["new_logp"] - I["old_logp"])
    assert bool((ratio[0::16] == 1.0).all())  # the planted ties are ties
    if clip_eps == 0.0 and M > 16:
        assert int(ref["undecided"][planted].sum()) >= M // 16 // 2  # and, with lo = hi = 1, undecided by the float64 reference alone


@pytest.mark.parametrize("defect,owner,clip_eps", [("open_clamp", "L3", 0.0), ("tie_full", "L3", 0.2), ("no_scale", "L3", 0.2), ("ent_sign", "L3", 0.2),
                                                   ("mask_ignored", "L1", 0.2)])
def test_ppo_loss_defect_is_rejected(defect, owner, clip_eps):
    failures, fig, I, O, ref, planted = _ppo_case(1025, False, True, clip_eps, 1000.0, defect)
    assert owner in _owners(failures), (defect, failures)
    assert fig[[k for k in fig if k.startswith(owner)][0]]["ratio"] > 100
    if defect in ("open_clamp", "tie_full"):  # shown on the ratio == 1 samples
        good = emu_ppo(I, clip_eps, CV, CE, 1000.0)
        tie = torch.zeros(1025, dtype=torch.bool)
        tie[0::16] = True
        differs = (good["dlogits"] != O["dlogits"]).any(1)
        assert bool(differs[tie & (I["adv"] != 0) & (good["new_logp"] != 0)].all()) and (defect == "tie_full" or not bool(differs[~tie].any()))
    if defect == "no_scale":
        assert "L4" in _owners(failures)
