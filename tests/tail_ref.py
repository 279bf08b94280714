"""Float64 stage references and acceptance rules for the fused CLS tail of the update (g2048_cls_tail_fwd, g2048_cls_tail_bwd,
g2048_dweight_t in csrc/g2048_tail.hip): tests/test_gpu_tail_f64.py runs the kernels against them, tests/test_tail_ref.py holds them
to an f32 / bf16 emulation and to planted defects on the CPU.  Everything here is the textbook operation on torch tensors and runs on
any device.  The GEMM bound, the exact acceptance and the NaN patterns are those of tests/gemm_ref.py (``gr``).

The chain is verified STAGE BY STAGE, each stage from the kernel's own saved input of that stage, so every stage is one Linear or
one LayerNorm plus an epilogue whose rounding points are stated in the kernel: bf16 GEMM inputs, f32 accumulation, Linear outputs
rounded to bf16, f32 residual and LayerNorm.  ReLU is 1-Lipschitz (|relu(a) - relu(b)| <= |a - b|) and commutes with the rounding, so
the GEMM bound holds for the post-ReLU value unchanged and no element is left undecided.  ``check`` takes a *state*: every saved
tensor in plain form (transposed buffers [features, ld], the mask words int16 [blocks, 96, 64]) and returns the failures of all stages.

Notation: u = 2^-24 (f32 unit roundoff), s(n) = (n + 1) 2^-23 mag the any-order f32 summation term of ``gr.bound`` (mag: the same
operation on absolute values), and
    B(ref, e) = (1 + 2^-8) (2^-8 |ref| + e)
the bound of a value rounded to bf16 whose f32 predecessor is within e of ref (``gr.bound`` is B(ref, s(n))).  inv = the f32
1 / (1 - p); a product with it is ONE f32 multiply, relative error u.

Dropout (csrc/g2048_bits.h, Drop::site / Drop::apply4 / make_drop, restated in numpy by ``keep_mask``): one hash per PAIR of consecutive
elements, the low 16 bits decide the even element and the high 16 the odd one, against thr16 = ((uint32)(p 2^24)) >> 8.  This is NOT
``gr.thr16`` (which rounds p 2^16 to nearest, the convention of the stand-alone GEMM epilogues): the tail truncates twice.  With
(uint32)(p 2^24) == 0 nothing is dropped and nothing is scaled.  A non-null ``seed_state`` word s enters as s0 ^= lo(s) HASH_MUL,
s1 += hi(s) HASH_MUL_HI + lo(s) before the site offsets.

Mask words: word (block, tile, lane), bit 4g + q  <->  row 32 block + (lane & 31), feature 32 (tile - base) + 8g + 4 (lane >> 5) + q,
bases FFN 0, A1 32, A2 48, C1 64, C2 80 (the accumulator map rowof(i, h) = (i & 3) + 8 (i >> 2) + 4h with i = 4g + q).

Forward stages                                          rule
  F0 oT      = o^T                                      bit-equal
  F1 x_mid   = x + keep1 inv bf16(Wo o + bo)            inv B(z, s(256)) (1 + 2u) + u inv |z| + u |ref|: the rounded Linear, one
                                                        multiply, one f32 add
  F2 mean    = sum(v) / 256 from the saved x_mid        Em = 256 u mean|v|: any order of the 255 additions, exact scaling
     rstd    = (var + eps)^-1/2                         d^_i = fl(v_i - mean^) is within Ed_i = Em + u (|d_i| + Em) of d_i; the mean of
                                                        the 256 squares (each one rounding, any-order sum) is within
                                                        Ew = mean(2 |d| Ed + Ed^2) + 258 u (var + that) + u (var + eps) of var (the last
                                                        term: the addition of eps); rstd then lies in
                                                        [(w + Ew)^-1/2 (1 - rho), (w - Ew)^-1/2 (1 + rho)], w = var + eps,
                                                        rho = 2^-22: rsqrtf allowed 2 f32 ulp.  No accuracy statement for rsqrtf on gfx950
                                                        was at hand when this was written: the 2 ulp are an ASSUMPTION (1 ulp would
                                                        not change a verdict here: taking eps as 0 moves rstd by 5 % on the rows below).
                                                        The any-order bounds are ~30 x what a tree sum reaches, so the emulation sits at
                                                        a few per cent of Em / Er; they cannot be tightened without asserting the kernel's
                                                        summation order, and the defects they guard against (eps, divisor, a dropped
                                                        lane) are >= 1e-3 relative against a bound of ~3e-5.
  F3 h2T     = bf16(LN(x_mid) g + b)                    B(ref, |g| ((|d| + Ed) Er + rstd Ed) + 4u (|g d rstd| + |b|))
  F4 uT      = bf16(keep2 inv relu(W1 h2 + b1))         dropped: exactly 0; kept: B(ref, inv s(256) (1 + u) + u |ref|)
  F5 featsT  = bf16(x_mid + keep3 inv bf16(W2 u + b2))  B(ref, inv B(f, s(1024)) (1 + 2u) + u inv |f| + u |ref|): two half-ulps
  F6 a1T ..  = bf16(relu(Linear))                       gr.bound, n = 256 / 512
  F7 logits, values = a3 a2, c3 c2                      s(512), f32 outputs
Backward stages
  B0 dlT rows 0..3, dvT row 0 = bf16(dlogits / dvalues) bit-equal; rows up to 31 exactly zero
  B1 da2T    = mask sum_o w3[o, f] bf16(dl[o])          B(ref, n u mag), n = 4 (1): the products are exact in f32
  B2 da1T    = mask (W2^T da2)                          gr.bound, n = 512
  B3 df2T    = keep3 inv bf16(A1^T da1 + C1^T dc1)      p = 0: gr.bound, n = 1024; else B(ref, inv bg (1 + u) + u |ref|), bg that bound
  B4 dzT     = mask_u inv (W2^T df2)                    B(ref, inv s(256) (1 + u) + u |ref|)
  B5 dx_cls  = g + rstd (a - c1 - xh c2), a = dh gamma, c1 = mean(a), c2 = mean(a xh), xh = (v - mean) rstd, with the float64
               statistics of F2, g = A1^T da1 + C1^T dc1, dh = W1^T dz.  The kernel holds g and dh rounded to bf16 (within
               bg = gr.bound(g, n = 1024) and bh = gr.bound(dh, n = 1024)) and f32 statistics (within Em, Er).  With A = |gamma| bh,
               Exh = (|d| + Ed) Er + rstd Ed + 2u |xh|, dc1 = mean(A) + 257 u mean|a|, dc2 = mean(A |xh| + (|a| + A) Exh) + 258 u mean|a xh|:
                   |dx - ref| <= bg + Er |a - c1 - xh c2| + (rstd + Er) (A + dc1 + Exh (|c2| + dc2) + |xh| dc2)
                                 + 8u (|g| + rstd (|a| + |c1| + |xh c2|))
               (the LayerNorm backward is linear in dh: the interval of dh is carried through term by term).
     ln_partial[block] = sum over the block's rows of (dh xh | dh): sum of bh |xh| + (|dh| + bh) Exh (of bh) + 33 * 2^-23 sum|terms|
  B6 daoT    = bf16_rne(f32(dx_cls) f32(inv)) where keep1, else 0, from the kernel's saved dx_cls: bit-equal
  B7 d_o     = bf16(Wo^T dao)                           gr.bound, n = 256
  B8 dw, db  per slice = gr.dweight over that slice's columns of the saved transposed operands: s(ld / slices), f32 outputs
MASK  every word equals (saved activation != 0) bit for bit; rows at or beyond M are zero.
ZERO  every column at or beyond M of every transposed buffer is exactly zero.
Every bounded stage also holds the whole tensor to ``gr.REL_LIMIT``.
"""
import numpy as np
import torch

import gemm_ref as gr

BF16, F32, F64 = gr.BF16, gr.F32, gr.F64
D, FF, HID = 256, 1024, 512
U = 2.0 ** -24
RSQRT_REL = 2.0 ** -22  # 2 f32 ulp (assumption, see the module docstring)
SAVED_ROWS = dict(oT=256, h2T=256, uT=1024, featsT=256, a1T=512, a2T=512, c1T=512, c2T=512)
GRAD_ROWS = dict(daoT=256, dzT=1024, df2T=256, da1T=512, da2T=512, dlT=32, dc1T=512, dc2T=512, dvT=32)
MASK_BASE = dict(uT=0, a1T=32, a2T=48, c1T=64, c2T=80)
MASK_TILES = 96
DW_SPEC = dict(wo=("daoT", "oT", True), w1=("dzT", "h2T", True), w2=("df2T", "uT", True), a1=("da1T", "featsT", True),
               a2=("da2T", "a1T", True), a3=("dlT", "a2T", False), c1=("dc1T", "featsT", True), c2=("dc2T", "c1T", True),
               c3=("dvT", "c2T", False))
HASH_MUL, HASH_MUL_HI = 0x9E3779B1, 0x85EBCA77
_M32 = 0xFFFFFFFF


class Cfg:
    def __init__(self, M, p, seed, eps=1e-5, seed_state=None, ld=None, slices=None):
        self.M, self.p, self.seed, self.seed_state = int(M), float(p), int(seed), seed_state
        self.eps = float(np.float32(eps))
        self.blocks = (self.M + 31) // 32
        self.ld = 32 * self.blocks if ld is None else int(ld)
        self.slices = next(s for s in (8, 4, 2, 1) if self.ld % (16 * s) == 0) if slices is None else int(slices)
        self.inv = float(gr.inv_keep_f32(p))
        self.thr = int(np.float32(p) * np.float32(16777216.0))
        self.scale = self.inv if self.thr else 1.0  # (Drop::apply4 returns at once for thr == 0)


# ------------------------------------------------------------------------------------------------------------- dropout
def keep_mask(cfg, site, cols, swap_halves=False):
    """bool [M, cols] (numpy): the keep decision of site ``site`` for element row * cols + col.  ``swap_halves``: the planted defect."""
    if cfg.thr == 0:
        return np.ones((cfg.M, cols), bool)
    s0, s1 = cfg.seed & _M32, (cfg.seed >> 32) & _M32
    if cfg.seed_state is not None:
        s = int(cfg.seed_state)
        lo, hi = s & _M32, (s >> 32) & _M32
        s0 ^= (lo * HASH_MUL) & _M32
        s1 = (s1 + hi * HASH_MUL_HI + lo) & _M32
    s0 = (s0 + site * 0x632BE5AB) & _M32
    s1 ^= (site * 0x7F4A7C15) & _M32
    idx = np.arange(cfg.M * cols, dtype=np.uint64)
    pair, m = idx >> np.uint64(1), np.uint64(_M32)
    x = ((pair & m) * np.uint64(HASH_MUL) & m) ^ np.uint64(s0)
    x ^= ((pair >> np.uint64(32)) * np.uint64(HASH_MUL_HI) + np.uint64(s1)) & m
    x ^= x >> np.uint64(16)
    x = x * np.uint64(0x7FEB352D) & m
    x ^= x >> np.uint64(15)
    x = x * np.uint64(0x846CA68B) & m
    x ^= x >> np.uint64(16)
    even = (idx & np.uint64(1)) == 0
    if swap_halves:
        even = ~even
    half = np.where(even, x & np.uint64(0xFFFF), x >> np.uint64(16))
    return (half >= np.uint64(cfg.thr >> 8)).reshape(cfg.M, cols)


def _keep(cfg, site, cols, dev):
    return torch.from_numpy(keep_mask(cfg, site, cols)).to(dev)


# ------------------------------------------------------------------------------------------------------------- mask words
def decode_masks(words, name, blocks):
    """int16 [blocks, 96, 64] -> bool [32 blocks, features] of the activation ``name``."""
    nt = SAVED_ROWS[name] // 32
    w = words.reshape(blocks, MASK_TILES, 64)[:, MASK_BASE[name]:MASK_BASE[name] + nt].to(torch.int32) & 0xFFFF
    bits = (w.unsqueeze(-1) >> torch.arange(16, device=w.device, dtype=torch.int32)) & 1  # [B, nt, lane, bit]
    bits = bits.reshape(blocks, nt, 2, 32, 4, 4)  # [B, t, h, r, g, q]
    return bits.permute(0, 3, 1, 4, 2, 5).reshape(blocks * 32, nt * 32).bool()


def encode_masks(act, name, words):
    """The inverse: bool [32 blocks, features] into the tiles of ``name`` of ``words`` (int16 [blocks, 96, 64]), in place."""
    blocks, nt = words.shape[0], SAVED_ROWS[name] // 32
    b = act.reshape(blocks, 32, nt, 4, 2, 4).permute(0, 2, 4, 1, 3, 5).reshape(blocks, nt, 64, 16).to(torch.int32)
    w = (b << torch.arange(16, dtype=torch.int32, device=b.device)).sum(-1)
    words[:, MASK_BASE[name]:MASK_BASE[name] + nt] = torch.where(w >= 32768, w - 65536, w).to(torch.int16)


# ------------------------------------------------------------------------------------------------------------- pieces
def rows(T, name, M):
    """[M, features] of a transposed buffer [features, ld]."""
    return T[name][:, :M].t()


def lin(x, w, b=None):
    """-> (x w^T + b, the same on absolute values) in float64."""
    return gr.linear(x, w, b), gr.linear(x.abs(), w.abs(), None if b is None else b.abs())


def s_term(mag, n):
    return gr.bound(mag, mag, n, half_ulp=False)


def bf16_bound(ref, e32):
    return (1 + 2.0 ** -8) * (2.0 ** -8 * ref.abs() + e32)


def ln_stats(x_mid, eps):
    """Float64 statistics of the saved x_mid [M, 256] and the bounds of their f32 counterparts (module docstring, F2)."""
    v = gr.f64(x_mid)
    mean = v.mean(1, keepdim=True)
    d = v - mean
    var = (d * d).mean(1, keepdim=True)
    w = var + eps
    rstd = w.rsqrt()
    Em = D * U * v.abs().mean(1, keepdim=True)
    Ed = Em + U * (d.abs() + Em)
    dv = (2 * d.abs() * Ed + Ed * Ed).mean(1, keepdim=True)
    Ew = dv + (D + 2) * U * (var + dv) + U * w
    hi = (w - Ew).clamp_min(1e-300).rsqrt() * (1 + RSQRT_REL)
    lo = (w + Ew).rsqrt() * (1 - RSQRT_REL)
    Er = torch.maximum(hi - rstd, rstd - lo)
    return dict(mean=mean, rstd=rstd, d=d, Em=Em, Ed=Ed, Er=Er, xh=d * rstd)


def _exact(got, want, what):
    return gr.accept_exact(got.contiguous(), want.contiguous(), what)


def accept_stage(got, ref, bnd, what, fig=None):
    """One bounded stage: every element within its bound and the whole tensor within ``gr.REL_LIMIT``.  -> [] or messages; ``fig[what]``
    receives the worst error / bound and the whole-tensor error."""
    return gr.accept_bound(got, ref, bnd, what, fig)


def make_params(seed=0):
    """The tail's parameters from a fixed generator (CPU): bf16 weights ~ randn / sqrt(fan_in), f32 biases with NON-ZERO means, gamma
    around 1."""
    shapes = dict(wo=(256, 256), bo=(256,), ln_g=(256,), ln_b=(256,), w1=(1024, 256), b1=(1024,), w2=(256, 1024), b2=(256,),
                  a1=(512, 256), ab1=(512,), a2=(512, 512), ab2=(512,), a3=(4, 512), c1=(512, 256), cb1=(512,), c2=(512, 512),
                  cb2=(512,), c3=(1, 512))
    g = torch.Generator().manual_seed(1000 + seed)
    P = {}
    for k, shp in shapes.items():
        if k == "ln_g":
            P[k] = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif len(shp) == 1:
            P[k] = 0.05 + 0.1 * torch.randn(shp, generator=g)
        else:
            P[k] = (torch.randn(shp, generator=g) / shp[1] ** 0.5).to(BF16)
    return P


def make_inputs(M, seed=0, degenerate=False):
    """o bf16 [M, 256], x f32 [M, 256], dlogits f32 [M, 4], dvalues f32 [M] (CPU).  ``degenerate``: every third row has o = 0 and an x row
    of standard deviation 1e-2 (eps = 1e-5 is 10 % of its variance once bo = 0), row 1 has o = 0 and a constant x (variance 0)."""
    g = torch.Generator().manual_seed(2000 + 7 * M + seed)
    o = torch.randn(M, 256, generator=g).to(BF16)
    x = torch.randn(M, 256, generator=g) + 0.1
    if degenerate:
        o[0::3] = 0
        x[0::3] = 1e-2 * torch.randn(x[0::3].shape, generator=g)
        o[1], x[1] = 0, 0.75
    return dict(o=o, x=x, dlogits=torch.randn(M, 4, generator=g), dvalues=torch.randn(M, generator=g))


def eps_rows(M):
    return list(range(0, M, 3))


def _masked(ref, mag, mask):
    z = torch.zeros((), dtype=F64, device=ref.device)
    return torch.where(mask, ref, z), torch.where(mask, mag, z)


# ------------------------------------------------------------------------------------------------------------- the stages
def check(P, inp, T, cfg, fig=None):
    """P: parameters (bf16 weights [out, in], f32 biases and norm parameters); inp: o bf16 [M, 256], x f32 [M, 256], dlogits f32 [M, 4],
    dvalues f32 [M]; T: the state.  -> list of messages, each starting with its stage's name."""
    M, dev = cfg.M, inp["o"].device
    fig = {} if fig is None else fig
    out = []
    k1, k2, k3 = _keep(cfg, 1, D, dev), _keep(cfg, 2, FF, dev), _keep(cfg, 3, D, dev)
    sc, zero = cfg.scale, torch.zeros((), dtype=F64, device=dev)
    dec = {n: decode_masks(T["masks"], n, cfg.blocks) for n in MASK_BASE}

    def bounded(got, ref, bnd, what):
        out.extend(accept_stage(got, ref, bnd, what, fig))

    # ---- ZERO / MASK
    for n in list(SAVED_ROWS) + list(GRAD_ROWS):
        if bool((T[n][:, M:].contiguous().view(torch.int16) != 0).any()):
            out.append(f"ZERO {n}: non-zero in a column at or beyond M = {M}")
    for n in MASK_BASE:
        act = T[n][:, :32 * cfg.blocks].t() != 0
        if not torch.equal(dec[n], act):
            bad = (dec[n] != act).nonzero()
            out.append(f"MASK {n}: {bad.shape[0]} bits differ from (activation != 0); first (row, feature) {bad[0].tolist()}")
    mk = {n: dec[n][:M] for n in dec}

    # ---- F0 / F1
    out += _exact(rows(T, "oT", M), inp["o"], "F0 oT")
    o = rows(T, "oT", M)
    z, zm = lin(o, P["wo"], P["bo"])
    bz = gr.bound(z, zm, D)
    ref = gr.f64(inp["x"]) + torch.where(k1, sc * z, zero)
    bnd = torch.where(k1, sc * bz * (1 + 2 * U) + U * sc * z.abs(), zero) + U * ref.abs()
    bounded(T["x_mid"], ref, bnd, "F1 x_mid")

    # ---- F2 / F3
    st = ln_stats(T["x_mid"], cfg.eps)
    bounded(T["mean"].reshape(M, 1), st["mean"], st["Em"], "F2 mean")
    bounded(T["rstd"].reshape(M, 1), st["rstd"], st["Er"], "F2 rstd")
    g_, b_ = gr.f64(P["ln_g"]), gr.f64(P["ln_b"])
    ref = st["xh"] * g_ + b_
    e32 = g_.abs() * ((st["d"].abs() + st["Ed"]) * st["Er"] + st["rstd"] * st["Ed"]) + 4 * U * ((st["xh"] * g_).abs() + b_.abs())
    bounded(rows(T, "h2T", M), ref, bf16_bound(ref, e32), "F3 h2T")

    # ---- F4
    z, zm = lin(rows(T, "h2T", M), P["w1"], P["b1"])
    ref = torch.where(k2, sc * gr.relu(z), zero)
    bnd = torch.where(k2, bf16_bound(ref, sc * s_term(zm, D) * (1 + U) + U * ref.abs()), zero)
    bounded(rows(T, "uT", M), ref, bnd, "F4 uT")

    # ---- F5
    f, fm = lin(rows(T, "uT", M), P["w2"], P["b2"])
    bf = gr.bound(f, fm, FF)
    xm = gr.f64(T["x_mid"])
    ref = xm + torch.where(k3, sc * f, zero)
    e32 = torch.where(k3, sc * bf * (1 + 2 * U) + U * sc * f.abs(), zero) + U * ref.abs()
    bounded(rows(T, "featsT", M), ref, bf16_bound(ref, e32), "F5 featsT")

    # ---- F6 / F7
    for name, src, w, b, n in (("a1T", "featsT", "a1", "ab1", D), ("a2T", "a1T", "a2", "ab2", HID), ("c1T", "featsT", "c1", "cb1", D),
                               ("c2T", "c1T", "c2", "cb2", HID)):
        z, zm = lin(rows(T, src, M), P[w], P[b])
        bounded(rows(T, name, M), gr.relu(z), gr.bound(gr.relu(z), zm, n), f"F6 {name}")
    for name, src, w, got in (("logits", "a2T", "a3", T["logits"]), ("values", "c2T", "c3", T["values"].reshape(M, 1))):
        z, zm = lin(rows(T, src, M), P[w])
        bounded(got, z, s_term(zm, HID), f"F7 {name}")

    # ---- B0 / B1 / B2
    for name, d_in, n_out in (("dlT", inp["dlogits"].reshape(M, 4), 4), ("dvT", inp["dvalues"].reshape(M, 1), 1)):
        want = torch.zeros_like(T[name])
        want[:n_out, :M] = d_in.to(BF16).t()
        out += _exact(T[name], want, f"B0 {name}")
    for name, dname, w, n_out, act in (("da2T", "dlT", "a3", 4, "a2T"), ("dc2T", "dvT", "c3", 1, "c2T")):
        ref, mag = _masked(*lin(rows(T, dname, M)[:, :n_out], P[w].t()), mk[act])
        bounded(rows(T, name, M), ref, bf16_bound(ref, n_out * U * mag), f"B1 {name}")
    for name, src, w, act in (("da1T", "da2T", "a2", "a1T"), ("dc1T", "dc2T", "c2", "c1T")):
        ref, mag = _masked(*lin(rows(T, src, M), P[w].t()), mk[act])
        bounded(rows(T, name, M), ref, gr.bound(ref, mag, HID), f"B2 {name}")

    # ---- B3
    da1, dc1 = rows(T, "da1T", M), rows(T, "dc1T", M)
    g1, g1m = lin(da1, P["a1"].t())
    g2, g2m = lin(dc1, P["c1"].t())
    g, bg = g1 + g2, gr.bound(g1 + g2, g1m + g2m, 2 * HID)
    if cfg.thr == 0:
        ref, bnd = g, bg
    else:
        ref = torch.where(k3, sc * g, zero)
        bnd = torch.where(k3, bf16_bound(ref, sc * bg * (1 + U) + U * ref.abs()), zero)
    bounded(rows(T, "df2T", M), ref, bnd, "B3 df2T")

    # ---- B4 (the backward multiplies by inv_keep even for p = 0, where it is 1)
    du, dum = _masked(*lin(rows(T, "df2T", M), P["w2"].t()), mk["uT"])
    ref = cfg.inv * du
    bounded(rows(T, "dzT", M), ref, bf16_bound(ref, cfg.inv * s_term(dum, D) * (1 + U) + U * ref.abs()), "B4 dzT")

    # ---- B5
    dh, dhm = lin(rows(T, "dzT", M), P["w1"].t())
    bh = gr.bound(dh, dhm, FF)
    xh, rstd, Er = st["xh"], st["rstd"], st["Er"]
    a = dh * g_
    A = g_.abs() * bh
    Exh = (st["d"].abs() + st["Ed"]) * Er + rstd * st["Ed"] + 2 * U * xh.abs()
    mean = lambda t: t.mean(1, keepdim=True)
    c1, c2 = mean(a), mean(a * xh)
    dc1_ = mean(A) + (D + 1) * U * mean(a.abs())
    dc2_ = mean(A * xh.abs() + (a.abs() + A) * Exh) + (D + 2) * U * mean((a * xh).abs())
    core = a - c1 - xh * c2
    ref = g + rstd * core
    bnd = (bg + Er * core.abs() + (rstd + Er) * (A + dc1_ + Exh * (c2.abs() + dc2_) + xh.abs() * dc2_)
           + 8 * U * (g.abs() + rstd * (a.abs() + c1.abs() + (xh * c2).abs())))
    bounded(T["dx_cls"], ref, bnd, "B5 dx_cls")
    pad = 32 * cfg.blocks - M

    def block_sum(t):
        return torch.cat([t, t.new_zeros(pad, D)]).reshape(cfg.blocks, 32, D).sum(1)

    ref = torch.cat([block_sum(dh * xh), block_sum(dh)], 1)
    e_g = bh * xh.abs() + (dh.abs() + bh) * Exh
    bnd = torch.cat([block_sum(e_g) + 33 * 2.0 ** -23 * block_sum((dh * xh).abs()), block_sum(bh) + 33 * 2.0 ** -23 * block_sum(dh.abs())], 1)
    bounded(T["ln_partial"].reshape(cfg.blocks, 2 * D), ref, bnd, "B5 ln_partial")

    # ---- B6 / B7
    scaled = T["dx_cls"] * torch.tensor(np.float32(cfg.scale), dtype=F32, device=dev)
    want = torch.where(k1, scaled, torch.zeros((), dtype=F32, device=dev)).to(BF16)
    out += _exact(rows(T, "daoT", M), want, "B6 daoT")
    ref, mag = lin(rows(T, "daoT", M), P["wo"].t())
    bounded(T["d_o"], ref, gr.bound(ref, mag, D), "B7 d_o")

    # ---- B8
    n = cfg.ld // cfg.slices
    for k, (dy, xt, has_b) in DW_SPEC.items():
        parts, sums = gr.dweight(T[dy].t(), T[xt].t(), cfg.slices)
        pm, sm = gr.dweight(T[dy].t().abs(), T[xt].t().abs(), cfg.slices)
        bounded(T["dw"][k], parts, s_term(pm, n), f"B8 dw {k}")
        if has_b:
            bounded(T["db"][k], sums, s_term(sm, n), f"B8 db {k}")
    return out
