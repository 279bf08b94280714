"""tests/tail_ref.py held to itself on the CPU: an f32 / bf16 emulation of the fused CLS tail (plain torch, the kernel's rounding points:
bf16 GEMM inputs, f32 accumulation, Linear outputs rounded to bf16, f32 residual and LayerNorm, bf16 gradients between Linears) must pass
every stage rule, and every planted defect must be rejected by the stage that owns it.

Worst error / bound of the emulation per stage over M in {33, 95} x p in {0, 0.1} (printed as TAILFIG lines):
    F1 x_mid 0.95   F3 h2T 0.98   F4 uT 0.95   F5 featsT 0.98 (p = 0.1), 0.82 (p = 0)   F6 0.96   B1 0.99   B2 0.92   B3 df2T 0.83
    B4 dzT 0.95   B5 dx_cls 0.61, ln_partial 0.67   B7 d_o 0.95
    F2 mean 0.002, rstd 0.007   F7 0.001   B8 dw 0.07, db 0.014
The last line are the f32 results, held to ANY-ORDER summation bounds (n u sum|terms|, the worst case of adding one term after the
other): a fixed order reaches ~sqrt(n) u and a tree log2(n) u, and no tighter rule can be written without asserting the kernel's order of
additions (tests/gemm_ref.py records 0.003-0.023 for its f32 outputs for the same reason).  What these stages guard against is far
above the bound all the same: a term, lane or wave missing from a sum, a wrong divisor, eps left out (planted below).
The rest are bf16 results.  B3 and F5 at p = 0 carry a summation term over 1024 products that is as large as the half-ulp (mag ~ 30 |ref|),
F5 with dropout and B5 two half-ulps that are seldom both at their worst in one element; ln_partial's bound is the sum of up to 32
half-ulp terms, reached only if every rounding of d h2 in a column points the same way (0.67 with one row in the block, 0.23 with 32).
"""
import json

import numpy as np
import pytest
import torch

import gemm_ref as gr
import tail_ref as tr

BF16, F32 = gr.BF16, gr.F32


def _f(t):
    return t.to(F32)


def _bf(t):
    """Round to bf16, go on in f32."""
    return t.to(BF16).to(F32)


def _T(t, ld):
    """[M, features] -> the transposed buffer [features, ld] (bf16), columns at or beyond M zero."""
    out = torch.zeros(t.shape[1], ld, dtype=BF16)
    out[:, :t.shape[0]] = t.to(BF16).t()
    return out


def emulate(P, inp, cfg, defect=None):
    M, ld, B = cfg.M, cfg.ld, cfg.blocks
    inv, inv_b = torch.tensor(np.float32(cfg.scale)), torch.tensor(np.float32(cfg.inv))
    k1, k3 = (torch.from_numpy(tr.keep_mask(cfg, s, 256)) for s in (1, 3))
    k2 = torch.from_numpy(tr.keep_mask(cfg, 2, 1024, swap_halves=defect == "swap_halves"))
    zero = torch.zeros((), dtype=F32)
    W = {k: _f(v) for k, v in P.items()}
    o, x = _f(inp["o"]), inp["x"]
    x_mid = x + torch.where(k1, _bf(o @ W["wo"].t() + W["bo"]) * inv, zero)
    mean = x_mid.sum(1, keepdim=True) / 256
    d = x_mid - mean
    eps = torch.full((M, 1), np.float32(cfg.eps), dtype=F32)
    if defect == "eps0":
        eps[tr.eps_rows(M)] = 0
    rstd = torch.rsqrt((d * d).sum(1, keepdim=True) / (255 if defect == "div255" else 256) + eps)
    h2 = _bf(d * rstd * W["ln_g"] + W["ln_b"])
    b1 = W["b1"].clone()
    if defect == "no_bias_tile":
        b1[96:128] = 0
    u = _bf(torch.where(k2, torch.relu(h2 @ W["w1"].t() + b1) * inv, zero))
    feats = _bf(x_mid + torch.where(k3, _bf(u @ W["w2"].t() + W["b2"]) * inv, zero))
    a1 = _bf(torch.relu(feats @ W["a1"].t() + W["ab1"]))
    a2 = _bf(torch.relu(a1 @ W["a2"].t() + W["ab2"]))
    c1 = _bf(torch.relu(feats @ W["c1"].t() + W["cb1"]))
    c2 = _bf(torch.relu(c1 @ W["c2"].t() + W["cb2"]))
    T = dict(x_mid=x_mid, mean=mean.reshape(M), rstd=rstd.reshape(M), logits=a2 @ W["a3"].t(), values=(c2 @ W["c3"].t()).reshape(M))
    act = dict(oT=o, h2T=h2, uT=u, featsT=feats, a1T=a1, a2T=a2, c1T=c1, c2T=c2)
    T["masks"] = torch.zeros(B, tr.MASK_TILES, 64, dtype=torch.int16)
    for n in tr.MASK_BASE:
        tr.encode_masks(torch.cat([act[n] != 0, torch.zeros(32 * B - M, act[n].shape[1], dtype=torch.bool)]), n, T["masks"])
    # ---- backward
    dl, dv = _bf(inp["dlogits"]), _bf(inp["dvalues"]).reshape(M, 1)
    da2 = _bf(torch.where(a2 != 0, dl @ W["a3"], zero))
    dc2 = _bf(torch.where(c2 != 0, dv @ W["c3"], zero))
    da1 = _bf(torch.where(a1 != 0, da2 @ W["a2"], zero))
    dc1 = _bf(torch.where(c1 != 0, dc2 @ W["c2"], zero))
    g = _bf(da1 @ W["a1"] + dc1 @ W["c1"])
    df2 = _bf(torch.where(k3, g * inv, zero))
    dz = _bf(torch.where(u != 0, (df2 @ W["w2"]) * inv_b, zero))
    dh = _bf(dz @ W["w1"])
    xh = (x_mid - mean) * rstd
    a = dh * W["ln_g"]
    cc1, cc2 = a.sum(1, keepdim=True) / 256, (a * xh).sum(1, keepdim=True) / 256
    dx = g + rstd * (a - cc1 - xh * cc2)
    dao = _bf(torch.where(k1, dx * inv, zero))
    pad = torch.zeros(32 * B - M, 256)
    bs = lambda t: torch.cat([t, pad]).reshape(B, 32, 256).sum(1)
    dlT, dvT = torch.zeros(32, M), torch.zeros(32, M)
    dlT[:4], dvT[:1] = dl.t(), dv.t()
    act.update(daoT=dao, dzT=dz, df2T=df2, da1T=da1, da2T=da2, dlT=dlT.t(), dc1T=dc1, dc2T=dc2, dvT=dvT.t())
    T.update({n: _T(v, ld) for n, v in act.items()})
    T.update(dx_cls=dx, d_o=(dao @ W["wo"]).to(BF16), ln_partial=torch.cat([bs(dh * xh), bs(dh)], 1))
    T["dw"], T["db"] = {}, {}
    for k, (dy, xt, has_b) in tr.DW_SPEC.items():
        dyT, xT = _f(T[dy]).reshape(-1, cfg.slices, ld // cfg.slices), _f(T[xt]).reshape(-1, cfg.slices, ld // cfg.slices)
        T["dw"][k] = torch.einsum("nsm,ksm->snk", dyT, xT)
        if has_b:
            T["db"][k] = dyT.sum(2).t().contiguous()
    return T


@pytest.fixture(scope="module")
def P():
    return tr.make_params()


_CACHE = {}


def _case(P, M, p, degenerate=False, defect=None):
    key = (M, p, degenerate, defect)
    if key not in _CACHE:
        cfg = tr.Cfg(M, p, seed=0x1234_5678_9ABC_DEF1 + M)
        inp = tr.make_inputs(M, degenerate=degenerate)
        Pp = dict(P, bo=torch.zeros(256)) if degenerate else P
        _CACHE[key] = (Pp, inp, cfg, emulate(Pp, inp, cfg, defect))
    Pp, inp, cfg, T = _CACHE[key]
    T = {k: ({kk: vv.clone() for kk, vv in v.items()} if isinstance(v, dict) else v.clone()) for k, v in T.items()}
    return Pp, inp, cfg, T


@pytest.mark.parametrize("M,p,degenerate", [(33, 0.0, False), (33, 0.1, False), (95, 0.0, False), (95, 0.1, False), (33, 0.0, True)])
def test_emulation_passes_every_stage(P, M, p, degenerate):
    Pp, inp, cfg, T = _case(P, M, p, degenerate)
    fig = {}
    failures = tr.check(Pp, inp, T, cfg, fig)
    print("TAILFIG " + json.dumps(dict(cell="emulation", M=M, p=p, degenerate=degenerate, ratio={k: round(v["ratio"], 3) for k, v in fig.items()})))
    assert not failures, failures
    assert len(fig) >= 35  # every bounded stage reported


def _owners(failures):
    return {m.split(":")[0].split(" ")[0] for m in failures}


def _featsT_ulp(T, P_, inp, cfg):
    """One bf16 ulp, away from the reference, at the element whose bound is smallest in ulps (x_mid dominates the Linear's output)."""
    M = cfg.M
    f = gr.linear(T["uT"][:, :M].t(), P_["w2"], P_["b2"])
    k3 = torch.from_numpy(tr.keep_mask(cfg, 3, 256))
    ref = gr.f64(T["x_mid"]) + torch.where(k3, cfg.scale * f, torch.zeros((), dtype=gr.F64))
    m, c = divmod(int((f.abs() / ref.abs()).argmin()), 256)
    T["featsT"].view(torch.int16)[c, m] += 1 if abs(float(T["featsT"][c, m])) >= abs(float(ref[m, c])) else -1


def _mask_bit(T, P_, inp, cfg):
    T["masks"][1, tr.MASK_BASE["a2T"] + 3, 37] ^= 1 << 9


def _nonzero_past_M(T, P_, inp, cfg):
    T["dzT"][700, cfg.ld - 1] = 2.0 ** -20


def _dlT_row5(T, P_, inp, cfg):
    T["dlT"][5, 2] = 1.0


def _ln_partial_wave(T, P_, inp, cfg):
    """ln_partial of block 0 without the rows 8..15 (wave 1)."""
    M = cfg.M
    dh = _bf(_f(T["dzT"][:, :M].t()) @ _f(P_["w1"]))
    xh = (T["x_mid"] - T["mean"].reshape(M, 1)) * T["rstd"].reshape(M, 1)
    T["ln_partial"][0] -= torch.cat([(dh * xh)[8:16].sum(0), dh[8:16].sum(0)])


def _dao_unscaled(T, P_, inp, cfg):
    """bf16(dx) inv instead of bf16(dx inv)."""
    k1 = torch.from_numpy(tr.keep_mask(cfg, 1, 256))
    T["daoT"][:, :cfg.M] = (_bf(torch.where(k1, T["dx_cls"], torch.zeros(()))) * np.float32(cfg.inv)).to(BF16).t()


def _dw_shift(T, P_, inp, cfg):
    """Slice 1 of dw[a1] computed over columns shifted by one k-step (16 rows)."""
    n = cfg.ld // cfg.slices
    dyT, xT = _f(T["da1T"]), _f(T["featsT"])
    T["dw"]["a1"][1] = dyT[:, n - 16:2 * n - 16] @ xT[:, n - 16:2 * n - 16].t()


def _d_o_stale(T, P_, inp, cfg):
    """The last valid row keeps what an earlier launch left there."""
    T["d_o"][cfg.M - 1] = T["d_o"][cfg.M - 2]


PLANTED = [(_featsT_ulp, "F5", 0.0), (_mask_bit, "MASK", 0.0), (_nonzero_past_M, "ZERO", 0.0), (_dlT_row5, "B0", 0.0),
           (_ln_partial_wave, "B5", 0.1), (_dao_unscaled, "B6", 0.1), (_dw_shift, "B8", 0.1), (_d_o_stale, "B7", 0.0)]


@pytest.mark.parametrize("plant,owner,p", PLANTED, ids=[f.__name__[1:] for f, _, _ in PLANTED])
def test_planted_output_defect_is_rejected(P, plant, owner, p):
    Pp, inp, cfg, T = _case(P, 33, p)
    plant(T, Pp, inp, cfg)
    failures = tr.check(Pp, inp, T, cfg)
    assert owner in _owners(failures), (plant.__name__, failures)


@pytest.mark.parametrize("defect,owner,p,degenerate", [("swap_halves", "F4", 0.1, False), ("no_bias_tile", "F4", 0.0, False),
                                                       ("eps0", "F2", 0.0, True), ("div255", "F2", 0.0, False)])
def test_planted_arithmetic_defect_is_rejected(P, defect, owner, p, degenerate):
    Pp, inp, cfg, T = _case(P, 33, p, degenerate, defect)
    failures = tr.check(Pp, inp, T, cfg)
    assert owner in _owners(failures), (defect, failures)
    if defect == "eps0":
        assert any(m.startswith("F2 rstd") for m in failures)


def test_keep_mask_agrees_with_the_restatement_of_test_gpu_tail():
    import test_gpu_tail as old

    for seed in (0, 0x9E37_79B9_7F4A_7C15, 2 ** 64 - 1):
        for site, cols in ((1, 256), (2, 1024), (3, 256)):
            for p in (0.1, 0.5, 2.0 ** -20):
                cfg = tr.Cfg(37, p, seed)
                assert np.array_equal(tr.keep_mask(cfg, site, cols), old._keep(seed, site, 37, cols, p)), (seed, site, p)
    cfg, cfg2 = tr.Cfg(37, 0.1, 5), tr.Cfg(37, 0.1, 5, seed_state=0x1_0000_0003)
    k, k2 = tr.keep_mask(cfg, 2, 1024), tr.keep_mask(cfg2, 2, 1024)
    assert (k != k2).mean() > 0.1 and abs(k2.mean() - 0.9) < 0.01  # the state word draws another mask at the same rate
    assert abs(1 - (cfg.thr >> 8) / 65536 - 0.9) < 2e-5 and (cfg.thr >> 8) != gr.thr16(0.1)  # truncated twice, not rounded


def _packed_off(row, col, cols):
    return ((((row >> 5) * (cols >> 4) + (col >> 4)) * 2 + ((col >> 3) & 1)) * 32 + (row & 31)) * 8 + (col & 7)


def _rowof(i, h):
    return (i & 3) + 8 * (i >> 2) + 4 * h


def test_decoder_and_packing_agree_with_the_literal_layouts():
    from src.g2048 import native as nv

    g = torch.Generator().manual_seed(5)
    x = torch.randint(-100, 100, (64, 48), generator=g).to(BF16)
    flat = nv.pack_fragments(x)
    for r in range(64):
        for c in range(48):
            assert flat[_packed_off(r, c, 48)] == x[r, c]
    assert torch.equal(nv.unpack_fragments(flat, 64, 48), x)
    # word (block, tile, lane) bit i: accumulator register i of lane (r, h) = feature 32 tile + rowof(i, h), row 32 block + r
    blocks = 2
    act = {n: torch.rand(32 * blocks, rows_, generator=g) < 0.5 for n, rows_ in tr.SAVED_ROWS.items() if n in tr.MASK_BASE}
    words = torch.zeros(blocks, tr.MASK_TILES, 64, dtype=torch.int32)
    for n, a in act.items():
        a_l = a.tolist()
        for b in range(blocks):
            for t in range(a.shape[1] // 32):
                for lane in range(64):
                    r, h = lane & 31, lane >> 5
                    w = 0
                    for i in range(16):
                        w |= int(a_l[32 * b + r][32 * t + _rowof(i, h)]) << i
                    words[b, tr.MASK_BASE[n] + t, lane] = w
    words16 = torch.where(words >= 32768, words - 65536, words).to(torch.int16)
    enc = torch.zeros_like(words16)
    for n, a in act.items():
        assert torch.equal(tr.decode_masks(words16, n, blocks), a), n
        tr.encode_masks(a, n, enc)
    assert torch.equal(enc, words16)
