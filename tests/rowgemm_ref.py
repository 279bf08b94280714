"""Float64 stage references, the tile plan and the acceptance rules for the fused Linear + add + LayerNorm kernel of the update
(csrc/g2048_rowgemm.hip: k_rowgemm behind g2048_linear_add_ln_fwd / _bwd).  tests/test_gpu_rowgemm_f64.py runs the kernel against them,
tests/test_rowgemm_ref.py holds them to an f32 / bf16 emulation and to planted defects on the CPU.  Plain torch and numpy: runs on any
device.  Nothing is restated that the tree already has: the integer tier, ``bound`` and the acceptance come from tests/gemm_ref.py (``gr``),
the masks, the add + LayerNorm stages A1..A6 and their operands from tests/rowwise_ref.py (``rr``), the LayerNorm statistics from
tests/tail_ref.py (through ``rr``).  u = 2^-24, inv = the f32 1 / (1 - p), s(n) = (n + 1) 2^-23 sum|terms| as there.

Tile plan (``tile_plan``, a restatement of rg_tpw / rg_launch): t = ceil(T / 256) (ceil(T / 512) under G2048_RG_TWO_TILES=1); the 96-token
body (NB = 3) with tpw = max(32, t) when t <= 96 and (two tiles or t <= 48), else the 160-token body (NB = 5) with tpw = min(160, t);
tiles = ceil(T / tpw), grid = min(tiles, 256).  Workgroup b walks the tiles b, b + grid, ..: token row r is added into partial row
(r // tpw) % grid (``group_of_row``).

Stage G, the GEMM inside, is not observable (its bf16 tile lives in LDS) and never compared directly:
  tier A   integer operands: a = bf16_rne(float64 u W^T + bias) IS the kernel's tile (``gemm_a``, precondition asserted), likewise g_h; with
           g_h_extra on the rows tok % extra_period == 0 the kernel rounds a second time: bf16_rne(f64(g_h) + f64(extra)).
  tier B   |tile - ref| <= Ba = gr.bound(ref, mag, K + 1) (the bias enters through the accumulator: one more addend; Bg of the backward,
           whose accumulators start at zero, likewise); with g_h_extra, s = ref + extra, the kernel computes bf16(f32(tile + extra)):
           Bg' = Bg + (2^-8 + 2u) (|s| + Bg) (one f32 add, half a bf16 ulp of the sum).

Forward                                            rule
  tier A   rr.add_ln_fwd_check with the exact a    A1 x_new bit-equal (every dropped element exactly x), A2 / A3 from the kernel's x_new
  tier B   B1 x_new, mask from rr.row_keep         dropped: bit-equal to x.  Kept: ref = x + a64 inv, Ep = inv Ba (1 + u) + u |a64 inv| (one
                                                   f32 multiply of the tile's value), |x_new - ref| <= Ep (1 + u) + u |ref| (one f32 add)
           A2, A3                                  rr.ln_check on the kernel's x_new
Backward
  tier A   rr.add_ln_bwd_check(tier_a=True, gid=)  A4 bound, A5 da bit-equal from the kernel's dx, A6 every workgroup's partial bit-equal.
           Operands (``bwd_tier_a``): rr.ln_bwd_tier_a, dy integers in [-2, 6], Wt integers in [-2, 6] with row n + 4 = -row n for
           n % 8 < 4: g_h[:, n + 4] = -g_h[:, n] (the bf16 rounding is odd), so c1 = c2 = 0 (asserted) and dx = g_x + g_h gamma is an integer.
           The da sums are integers at p in {0, 0.5} only: tier A runs at those.
  tier B   A4 dx against the float64 g_h           rr's A4 bound with A = |a| + |gamma| Bg in place of |a| (|c1| <= mean A, |c2| <= mean A |xh|),
                                                   plus the propagation of Bg through the linear map dLayerNorm:
                                                   rstd (|gamma| Bg + mean(|gamma| Bg) + |xh| mean(|gamma| Bg |xh|))
           A5 da                                   exact from the kernel's dx
           A6 dbeta                                group sum of Bg + s(n) of |g_h| + Bg
              dgamma                               group sum of Bg |xh| + (|g_h| + Bg) Exh, + s(n) of the terms' magnitudes
              da sums                              s(n) of the written values (da NULL: exactly zero)
           n = rows of the group (all its tiles).
"""
import torch

import gemm_ref as gr
import rowwise_ref as rr

BF16, F32, F64 = gr.BF16, gr.F32, gr.F64
D, U = rr.D, rr.U
MAX_GRID = 256
HALF_BF16 = 2.0 ** -8


# ------------------------------------------------------------------------------------------------------------------- tile plan
def tile_plan(T, two_tiles=False, max_grid=MAX_GRID):
    """-> (nb, tpw, tiles, grid): 32-token blocks of the body, tokens per tile, tiles, workgroups.  ``max_grid``: 256 in the library; the
    host test passes a small one to make workgroups walk several tiles at a small T."""
    t = -(-T // (512 if two_tiles else 256))
    if t <= 96 and (two_tiles or t <= 48):
        nb, tpw = 3, max(32, t)
    else:
        nb, tpw = 5, min(160, t)
    tiles = -(-T // tpw)
    return nb, tpw, tiles, min(tiles, max_grid)


def group_of_row(T, two_tiles=False, dev="cpu", max_grid=MAX_GRID):
    """long [T]: the workgroup (= partial row) that adds token row r."""
    _, tpw, _, grid = tile_plan(T, two_tiles, max_grid)
    return (torch.arange(T, device=dev) // tpw) % grid


# ------------------------------------------------------------------------------------------------------------------- stage G
def _abs(t):
    return None if t is None else t.abs()


def gemm_a(x, w, bias=None):
    """Tier A: the bf16 tile of the kernel, exactly (precondition asserted)."""
    gr.assert_exact(gr.linear(x.abs(), w.abs(), _abs(bias)))
    return gr.bf16_rne(gr.linear(x, w, bias))


def gemm_b(x, w, bias=None, n_extra=0):
    """Tier B: (the float64 product, the bound of the kernel's bf16 tile around it)."""
    ref = gr.linear(x, w, bias)
    return ref, gr.bound(ref, gr.linear(x.abs(), w.abs(), _abs(bias)), x.shape[1] + n_extra)


def add_extra_a(g_h, extra, period):
    out = g_h.clone()
    out[0::period] = gr.bf16_rne(gr.f64(g_h[0::period]) + gr.f64(extra))
    return out


def add_extra_b(gh, Bg, extra, period):
    gh, Bg = gh.clone(), Bg.clone()
    s = gh[0::period] + gr.f64(extra)
    Bg[0::period] = Bg[0::period] + (HALF_BF16 + 2 * U) * (s.abs() + Bg[0::period])
    gh[0::period] = s
    return gh, Bg


# ------------------------------------------------------------------------------------------------------------------- forward
def fwd_check(u, W, bias, x, gamma, beta, eps, p, seed, seed_state, x_new, h, mean, rstd, tier_a, fig=None):
    """u bf16 [T, K], W bf16 [256, K], bias f32 [256] or None, x f32 [T, 256] (the logical rows); the outputs as the launch left them."""
    if tier_a:
        return rr.add_ln_fwd_check(x, gemm_a(u, W, bias), gamma, beta, eps, p, seed, seed_state, x_new, h, mean, rstd, fig)
    T, dev = x.shape[0], x.device
    a64, Ba = gemm_b(u, W, bias, 1)
    keep = rr.row_keep(seed, seed_state, T, p, dev)
    inv, x64, zero = rr.inv_of(p), gr.f64(x), torch.zeros((), dtype=F64, device=dev)
    out = rr.exact(torch.where(keep, x, x_new), x64, "B1 x_new dropped", fig)
    prod = a64 * inv
    Ep = inv * Ba * (1 + U) + U * prod.abs()
    ref = x64 + prod
    out += rr.bounded(x_new, torch.where(keep, ref, x64), torch.where(keep, Ep * (1 + U) + U * ref.abs(), zero), "B1 x_new", fig)
    return out + rr.ln_check(x_new, gamma, beta, eps, h, mean, rstd, "A2", "A3", fig)


# ------------------------------------------------------------------------------------------------------------------- backward
def _sums_b(got, terms, err, gid, G, n, what, fig):
    """Tier B sums: group sum of the terms' own error + s(n) of the magnitudes the kernel adds."""
    bnd = rr.group_sums(err, gid, G) + (n.to(F64).reshape(G, 1) + 1) * 2.0 ** -23 * rr.group_sums(terms.abs() + err, gid, G)
    return rr.bounded(got, rr.group_sums(terms, gid, G), bnd, what, fig)


def bwd_check(dy, Wt, xn, g_x, period, extra, extra_period, mean, rstd, gamma, p, seed, seed_state, dx, da, partial, gid, G, tier_a, fig=None):
    """dy bf16 [T, K], Wt bf16 [256, K] (the logical window), xn f32 [T, 256], g_x f32 [T / period, 256] or None, extra bf16
    [T / extra_period, 256] or None; dx, da (or None), partial [G, 768] as the launch left them; gid long [T] from ``group_of_row``."""
    T, dev = dy.shape[0], dy.device
    if tier_a:
        g_h = gemm_a(dy, Wt)
        gr.assert_exercises_rounding(gr.linear(dy, Wt))
        if extra is not None:
            g_h = add_extra_a(g_h, extra, extra_period)
        a = gr.f64(g_h) * gr.f64(gamma)
        xh = (gr.f64(xn) - gr.f64(mean).reshape(T, 1)) * gr.f64(rstd).reshape(T, 1)
        assert not bool(a.sum(1).any()) and not bool((a * xh).sum(1).any()), "tier A precondition: c1 = c2 = 0"
        return rr.add_ln_bwd_check(xn, g_x, period, g_h, mean, rstd, gamma, p, seed, seed_state, dx, da, partial, None, fig, True, (gid, G))
    gh, Bg = gemm_b(dy, Wt, None, 1)
    if extra is not None:
        gh, Bg = add_extra_b(gh, Bg, extra, extra_period)
    gx = torch.zeros(T, D, dtype=F64, device=dev)
    if g_x is not None:
        gx[0::period] = gr.f64(g_x)
    m, r, g_ = gr.f64(mean).reshape(T, 1), gr.f64(rstd).reshape(T, 1).abs(), gr.f64(gamma)
    d = gr.f64(xn) - m
    xh = d * gr.f64(rstd).reshape(T, 1)
    ax = xh.abs()
    Exh = r * U * d.abs() + 2 * U * ax
    a, Bga = gh * g_, g_.abs() * Bg
    A = a.abs() + Bga
    mn = lambda t: t.mean(1, keepdim=True)
    c1, c2, C1, C2 = mn(a), mn(a * xh), mn(A), mn(A * ax)
    dc1 = (D + 1) * U * C1
    dc2 = mn(A * Exh) + (D + 2) * U * C2
    ref = gx + gr.f64(rstd).reshape(T, 1) * (a - c1 - xh * c2)
    bnd = r * (dc1 + Exh * (C2 + dc2) + ax * dc2) + 8 * U * (gx.abs() + r * (A + C1 + ax * C2))
    bnd = bnd + r * (Bga + mn(Bga) + ax * mn(Bga * ax))
    out = rr.bounded(dx, ref, bnd, "A4 dx", fig)
    written = torch.zeros(T, D, dtype=F64, device=dev)
    if da is not None:
        out += rr.exact(da, rr.scaled_bf16(dx, rr.inv_of(p), rr.row_keep(seed, seed_state, T, p, dev)), "A5 da", fig)
        written = gr.f64(da)
    n = torch.bincount(gid, minlength=G)
    got = partial.reshape(G, 3, D)
    out += _sums_b(got[:, 0], gh * xh, Bg * ax + (gh.abs() + Bg) * Exh, gid, G, n, "A6 dgamma", fig)
    out += _sums_b(got[:, 1], gh, Bg, gid, G, n, "A6 dbeta", fig)
    return out + _sums_b(got[:, 2], written, torch.zeros_like(written), gid, G, n, "A6 da sums", fig)


# ------------------------------------------------------------------------------------------------------------------- operands
def _antisym(t):
    """[R, 256, ...] -> rows (of axis 1) n + 4 = -row n for n % 8 < 4."""
    v = t.reshape(t.shape[0], D // 8, 2, 4, *t.shape[2:])
    v[:, :, 1] = -v[:, :, 0]
    return v.reshape(t.shape)


def fwd_tier_a(T, K, bias=True):
    return gr.tier_a_linear(T, K, D, bias)


def fwd_tier_b(T, K, bias=True):
    u, w, b = gr.tier_b_linear(T, K, D)
    return u, w, (b if bias else None)


def bwd_tier_a(T, K, wide=None):
    """dy [T, K], Wt [256, wide or K] bf16 integers in [-2, 6], Wt antisymmetric in its rows (module docstring); extra [ceil(T / 17), 256]
    integers in [-8, 8] with the same antisymmetry in its columns."""
    g = gr._gen(T, K, wide or K, 31)
    dy = gr.ints((T, K), -2, 6, g)
    wt = _antisym(gr.ints((1, D, wide or K), -2, 6, g))[0]
    extra = _antisym(gr.ints((-(-T // 17), D), -8, 8, g))
    return dict(dy=dy, Wt=wt.contiguous(), extra=extra)


def bwd_tier_b(T, K, wide=None):
    """dy = gr.tier_b_rows / 8, Wt ZERO-mean randn / sqrt(K) (dLayerNorm projects the common mean of g_h out and its rounding error not:
    with gr's + 0.02 weight mean the bf16 rounding of a correct g_h alone costs 3.5e-3 of the whole tensor at K = 1024), extra 0.1 randn."""
    g = gr._gen(T, K, wide or K, 33)
    dy = (gr.tier_b_rows(T, K, g, 0.3) / 8).to(BF16)
    wt = (torch.randn(D, wide or K, generator=g) / K ** 0.5).to(BF16)
    return dict(dy=dy, Wt=wt, extra=(0.1 * torch.randn(-(-T // 17), D, generator=g)).to(BF16))
