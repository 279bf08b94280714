"""Float64 stage references, numpy restatements of the dropout masks and the acceptance rules for the row-wise kernels of the update
(csrc/g2048_layernorm.hip: add+LN forward / backward, ReLU + dropout, colsum, the token embedding; csrc/g2048_ppo_loss.hip: g2048_ppo_loss).
tests/test_gpu_rowwise.py runs the kernels against them, tests/test_rowwise_ref.py holds them to an f32 / bf16 emulation and to planted
defects on the CPU.  Plain torch and numpy: runs on any device.  The exact acceptance, the bounded acceptance (per element, and the whole
tensor under ``gr.REL_LIMIT``) and the integer tier are those of tests/gemm_ref.py (``gr``); the LayerNorm rules F2, F3, B5, B6 those of
tests/tail_ref.py (``ln_stats``, ``bf16_bound``, ``RSQRT_REL``), imported, not copied.

The library is built with -ffp-contract=off: every f32 add and multiply of these kernels is ONE IEEE rounding, so the elementwise stages are
held bit for bit.  Each stage is checked from the kernel's own saved input of that stage.  u = 2^-24; inv = the f32 1.0f / (1.0f - p); a
product with it is one f32 multiply.  s(n) = (n + 1) 2^-23 sum|terms|: the any-order f32 summation bound of ``gr.bound``.

Masks (restated here in uint64 numpy; csrc/g2048_bits.h)
  hash(i) = fin(lo(i) HASH_MUL ^ s0 ^ (hi(i) HASH_MUL_HI + s1)), (s0, s1) = the seed's words, a seed_state word w mixed in first as
  s0 ^= lo(w) HASH_MUL, s1 += hi(w) HASH_MUL_HI + lo(w).
  keep24: keep iff (hash(i) >> 8) >= thr, thr = uint32(f32(p) 2^24), TRUNCATED; thr == 0 drops nothing.  i = row 256 + col.  add+LN forward
          (only with ``a``) and backward (only with ``da``); the embedding with row = 17 m + c, rows c == 0 (CLS) never dropped.
  keep16_pairs: k_relu_dropout_fwd: one hash per pair e >> 1 of the flat index e, low 16 bits for the even element, high 16 for the odd
          one, against ``gr.thr16(p)`` = uint32(f32(p) 65536 + 0.5), ROUNDED.  (The CLS tail truncates twice: tail_ref.keep_mask.)

Stage                                              rule
  A1 x_new = x + keep (a inv)                      exact: f32(f64(x) + f64(f32(f64(a) f64(inv)))): the bf16 x f32 product rounded once, one f32
                                                   add (the float64 sum of two f32 numbers is exact for exponents within 29 of each other; the
                                                   generators stay there).  Dropped: x.  ``a`` absent: x_new is not written.
  A2 mean, rstd from the kernel's x_new (or x)     tail_ref F2 (Em, Er with RSQRT_REL, an ASSUMPTION stated there)
  A3 h = bf16(LN)                                  tail_ref F3; gamma None: exact, gr.bf16_rne of the f32 row
  A4 dx = g_x + rstd (a - c1 - xh c2)              tail_ref B5 with bg = bh = Em = Er = 0: mean, rstd (f32) and g_h (bf16) are INPUTS of this stage,
                                                   the reference takes them as they are; left are Ed = u |d|, Exh = rstd Ed + 2u |xh|,
                                                   dc1 = 257 u mean|a|, dc2 = mean(|a| Exh) + 258 u mean|a xh|:
                                                     rstd (dc1 + Exh (|c2| + dc2) + |xh| dc2) + 8u (|g_x| + rstd (|a| + |c1| + |xh c2|)).
                                                   gamma None: exact f32(g_x + g_h).  g_x of period 17: row r of it belongs to token row 17 r.
  A5 da from the kernel's dx                       exact: bf16_rne(f32(dx) inv) where kept, else +0 (tail_ref B6)
  A6 dgamma, dbeta, column sums of da              tier A (integer terms, sum|terms| < 2^24 asserted): exact.  Tier B: dgamma sum|gh| Exh + s(n)
     (dparams, or the partial of each workgroup    of gh xh; dbeta and the da sums s(n) alone (the da sums add the bf16 values the kernel wrote);
     against the sum over ITS rows)                n the number of rows added
  R1 y = dropout(relu(x))                          exact: bf16_rne(f32(x) inv) where x > 0 and kept, else +0 (-0 and negatives give +0)
  R2 dx from dy and the kernel's y                 exact: bf16_rne(f32(dy) inv) where y != +-0, else +0
  R3 dbias (or partials)                           tier A exact; tier B s(n) of the written values
  C1 colsum                                        tier A exact; tier B s(T), no half-ulp term (f32 output)
  E1 x0                                            exact: CLS rows = cls; others f32(f32(W[e] + pe[c]) inv) where kept, else +0, e = min(board, 30)
  E2 h, mean, rstd of embed_ln_fwd                 A2 and A3 from the kernel's x0
  E3 dwt_dcls [32, 256]                            class k < 31: sum over its rows of keep (g inv) (each term one multiply: u |term|), class 31:
                                                   sum of the CLS rows of g, never dropped.  Tier A exact.  Tier B sum|term| ((n_k + 1) 2^-23 + u),
                                                   n_k the rows of the class (in the workgroup, for partials).  Empty classes exactly 0.
  L1..L4 g2048_ppo_loss                            below

g2048_ppo_loss.  The float64 reference follows the kernel's statement per sample from its f32 / bf16 inputs: z_j = l_j or f32(l_j - 1e8)
(the kernel's one rounding point there), lse = zmax + log sum exp(z_j - zmax), lp_j = z_j - lse, p_j = exp(lp_j), ent = -sum lp_j p_j,
ratio = exp(lp_a - olp), s1 = ratio A, s2 = clamp(ratio, lo, hi) A with the f32 lo = 1 - eps, hi = 1 + eps, closed interval, pl = -min(s1, s2);
the gradient weight of d pl / d lp_a = -W A ratio is W = w1 + w2 [lo <= ratio <= hi], (w1, w2) = (1, 0) for s1 < s2, (0, 1) for s1 > s2 and
(0.5, 0.5) on a tie (torch.min splits ties evenly; every in-range sample IS a tie and has W = 1).
expf and logf are allowed rho = 2^-22 relative (2 f32 ulp).  No accuracy statement for them on gfx950 was at hand: an ASSUMPTION, like
RSQRT_REL.  The bounds are a running error analysis: every kernel operation carries (value, error) by
    add:  E(a + b) = Ea + Eb + u (|a + b| + Ea + Eb)              mul:  E(a b) = |a| Eb + |b| Ea + Ea Eb + u (|a| + Ea) (|b| + Eb)
    exp:  E = exp(a) (exp(Ea) (1 + rho) - 1)                      log:  E = dl + rho (|log a| + dl), dl = -log(1 - Ea / a)
  L1 new_logp: E_lp.  t_j = z_j - zmax is one rounding (|t_j| u); each expf carries that argument error and rho; se takes three f32 adds;
     logf gives rho |log se| + (error of se) / se; zmax + log se and z_a - lse are two more roundings.
  L2 the five means: mean of the per-term errors + (M + 1) 2^-23 mean(|term| + error) for the any-order sum + 2u |ref| (inv_m = f32(1 / M) and
     the product with it).
  L3 dlogits, L4 dvalues: the same propagation through g_lp (p_j - [j = a]) and c_e p_j (lp_j + ent), with
     E_ratio = ratio (exp(E_lp + u |lp_a - olp|) (1 + rho) - 1): the subtraction lp_a - olp is one rounding, u |lp_a - olp| (u |olp| would
     bound it only while |lp_a - olp| <= |olp|, which a single legal action, lp_a = 0, with ratio < 1 already breaks), times
     g_m = f32(inv_m scale), taken as the kernel computes it; bf16 outputs under bf16_bound(ref, e).
  Undecided samples: W is evaluated at ratio - E_ratio, ratio, ratio + E_ratio (that covers both the interval test and the sign of s1 - s2,
     which is (ratio - clamp) A).  A sample with A != 0 on which the three disagree may fall on either side: its gradient is accepted within
     the bound of the reference of ANY of these W.  At most 1 % of the samples of a case may be undecided, planted ones excluded: asserted.
"""
import functools

import numpy as np
import torch

import gemm_ref as gr
from tail_ref import RSQRT_REL, bf16_bound, ln_stats  # noqa: F401  (RSQRT_REL: the assumption the statistics rest on)

BF16, F32, F64 = gr.BF16, gr.F32, gr.F64
D, SEQ = 256, 17
U = 2.0 ** -24
RHO = 2.0 ** -22  # expf, logf: 2 f32 ulp (assumption, see the module docstring)
HASH_MUL, HASH_MUL_HI = 0x9E3779B1, 0x85EBCA77
_M32 = 0xFFFFFFFF
UNDECIDED_CAP = 0.01


# ------------------------------------------------------------------------------------------------------------------- masks
def seed_words(seed, seed_state=None):
    s0, s1 = int(seed) & _M32, (int(seed) >> 32) & _M32
    if seed_state is not None:
        lo, hi = int(seed_state) & _M32, (int(seed_state) >> 32) & _M32
        s0 ^= (lo * HASH_MUL) & _M32
        s1 = (s1 + hi * HASH_MUL_HI + lo) & _M32
    return s0, s1


def hash32(idx, s0, s1):
    """The 32 hash bits of every index of ``idx`` (numpy uint64)."""
    u, m = np.uint64, np.uint64(_M32)
    idx = np.asarray(idx, dtype=np.uint64)
    x = ((idx & m) * u(HASH_MUL) & m) ^ u(s0)
    x = x ^ (((idx >> u(32)) * u(HASH_MUL_HI) + u(s1)) & m)
    x = x ^ (x >> u(16))
    x = x * u(0x7FEB352D) & m
    x = x ^ (x >> u(15))
    x = x * u(0x846CA68B) & m
    return x ^ (x >> u(16))


def thr24(p):
    return int(np.float32(p) * np.float32(16777216.0))


def keep24(seed, seed_state, idx, p):
    """bool array like ``idx``: the keep decision of keep_elem for the element indices ``idx``."""
    idx = np.asarray(idx, dtype=np.uint64)
    thr = thr24(p)
    if thr == 0:
        return np.ones(idx.shape, bool)
    return (hash32(idx, *seed_words(seed, seed_state)) >> np.uint64(8)) >= np.uint64(thr)


def keep16_pairs(seed, seed_state, n, p, start=0):
    """bool [n]: the keep decision of k_relu_dropout_fwd for the flat elements start .. start + n - 1."""
    e = np.arange(n, dtype=np.uint64) + np.uint64(start)
    h = hash32(e >> np.uint64(1), *seed_words(seed, seed_state))
    half = np.where((e & np.uint64(1)) == 0, h & np.uint64(0xFFFF), h >> np.uint64(16))
    return half >= np.uint64(gr.thr16(p))


@functools.lru_cache(maxsize=8)
def _row_keep(seed, seed_state, T, p, row_stride):
    if thr24(p) == 0:
        return torch.ones(T, D, dtype=torch.bool)
    idx = np.arange(T, dtype=np.uint64)[:, None] * np.uint64(row_stride) + np.arange(D, dtype=np.uint64)[None, :]
    return torch.from_numpy(keep24(seed, seed_state, idx, p))


def row_keep(seed, seed_state, T, p, dev, row_stride=D):
    """keep24 of the [T, 256] elements row * 256 + col (``row_stride``: the planted defect).  A fresh tensor on ``dev``."""
    return _row_keep(int(seed), seed_state, int(T), float(p), int(row_stride)).clone().to(dev)


def embed_keep(seed, seed_state, M, p, dev, drop_cls=False):
    k = row_keep(seed, seed_state, M * SEQ, p, dev)
    if not drop_cls:
        k[0::SEQ] = True
    return k


# ------------------------------------------------------------------------------------------------------------------- pieces
def inv_of(p):
    return float(gr.inv_keep_f32(p))


def _t32(v, dev):
    return torch.tensor(np.float32(v), dtype=F32, device=dev)


def exact(got, want, what, fig=None):
    out = gr.accept_exact(got.contiguous(), want.contiguous(), what)
    if fig is not None:
        fig[what] = dict(exact=not out)
    return out


def bounded(got, ref, bnd, what, fig=None):
    return gr.accept_bound(got, ref, bnd, what, fig)


def rne32(v64):
    """float64 -> the nearest f32 (one rounding), returned as float64."""
    return v64.to(F32).to(F64)


def scaled_bf16(v32, inv, keep):
    """bf16_rne(f32(v) inv) where ``keep``, else +0 (rules A5, R1, R2)."""
    return torch.where(keep, v32.to(F32) * _t32(inv, v32.device), torch.zeros((), dtype=F32, device=v32.device)).to(BF16)


def group_sums(terms, gid, G):
    """[R, C] float64, group of every row -> [G, C]."""
    return torch.zeros(G, terms.shape[1], dtype=F64, device=terms.device).index_add_(0, gid, terms)


def sums_check(got, terms, extra, gid, G, counts, what, fig, tier_a):
    """``got`` [G, C] against the per-group sums of ``terms`` [R, C].  Tier A: exact, precondition asserted.  Tier B: bound
    group sum of ``extra`` + (n + 1) 2^-23 group sum of |terms|, n = ``counts`` [G] rows."""
    ref, mag = group_sums(terms, gid, G), group_sums(terms.abs(), gid, G)
    if tier_a:
        gr.assert_exact(mag)
        return exact(got, ref, what, fig)
    bnd = (counts.to(F64).reshape(G, 1) + 1) * 2.0 ** -23 * mag
    if extra is not None:
        bnd = bnd + group_sums(extra, gid, G)
    return bounded(got, ref, bnd, what, fig)


def _gid(T, rows_per_group, dev):
    """Group of every row and the rows per group: one group (dparams) or consecutive blocks of ``rows_per_group`` rows (partials)."""
    r = torch.arange(T, device=dev)
    gid = torch.zeros_like(r) if rows_per_group is None else r // rows_per_group
    G = int(gid[-1]) + 1
    return gid, G, torch.bincount(gid, minlength=G)


# ------------------------------------------------------------------------------------------------------------------- add + LN
def ln_check(v, gamma, beta, eps, h, mean, rstd, stats, out_h, fig):
    """Rules A2 and A3 (E2) from the saved f32 rows ``v`` [T, 256]; ``stats`` / ``out_h``: the stage names in the messages."""
    T = v.shape[0]
    st = ln_stats(v, float(np.float32(eps)))
    out = bounded(mean.reshape(T, 1), st["mean"], st["Em"], f"{stats} mean", fig)
    out += bounded(rstd.reshape(T, 1), st["rstd"], st["Er"], f"{stats} rstd", fig)
    g_, b_ = gr.f64(gamma), gr.f64(beta)
    ref = st["xh"] * g_ + b_
    e32 = g_.abs() * ((st["d"].abs() + st["Ed"]) * st["Er"] + st["rstd"] * st["Ed"]) + 4 * U * ((st["xh"] * g_).abs() + b_.abs())
    return out + bounded(h, ref, bf16_bound(ref, e32), f"{out_h} h", fig)


def add_ln_fwd_check(x, a, gamma, beta, eps, p, seed, seed_state, x_new, h, mean, rstd, fig=None):
    """x f32 [T, 256] (the logical rows), a bf16 [T, 256] or None; the outputs as the launch left them (x_new None: not passed)."""
    T, dev, out = x.shape[0], x.device, []
    v = x
    if a is not None:
        keep = row_keep(seed, seed_state, T, p, dev)
        prod = rne32(gr.f64(a) * inv_of(p))
        want = gr.f64(x) + torch.where(keep, prod, torch.zeros((), dtype=F64, device=dev))
        want = rne32(want)
        v = want.to(F32)
        if x_new is not None:
            out += exact(x_new, want, "A1 x_new", fig)
            v = x_new
    if gamma is None:
        return out + exact(h, gr.bf16_rne(v), "A3 h (no LN)", fig)
    return out + ln_check(v, gamma, beta, eps, h, mean, rstd, "A2", "A3", fig)


def add_ln_bwd_check(xn, g_x, period, g_h, mean, rstd, gamma, p, seed, seed_state, dx, da, sums, rows_per_group=None, fig=None, tier_a=False,
                     gid=None):
    """xn f32 [T, 256] (None without gamma); g_x f32 [T / period, 256] or None; sums: dparams [3, 256] (``rows_per_group`` None) or the
    workspace partials [groups, 768].  ``gid`` = (long [T]: the group of every row, the number of groups) replaces the consecutive
    blocks of ``rows_per_group`` rows (the fused kernel of tests/rowgemm_ref.py, whose workgroups walk tiles)."""
    T, dev, out = g_h.shape[0], g_h.device, []
    zero = torch.zeros((), dtype=F64, device=dev)
    gh = gr.f64(g_h)
    gx = torch.zeros(T, D, dtype=F64, device=dev)
    if g_x is not None:
        gx[0::period] = gr.f64(g_x)
    if gamma is None:
        xh = Exh = torch.zeros_like(gh)
        out += exact(dx, rne32(gx + gh), "A4 dx (no LN)", fig)
    else:
        m, r, g_ = gr.f64(mean).reshape(T, 1), gr.f64(rstd).reshape(T, 1), gr.f64(gamma)
        d = gr.f64(xn) - m
        xh = d * r
        Exh = r.abs() * U * d.abs() + 2 * U * xh.abs()
        a = gh * g_
        mn = lambda t: t.mean(1, keepdim=True)
        c1, c2 = mn(a), mn(a * xh)
        dc1 = (D + 1) * U * mn(a.abs())
        dc2 = mn(a.abs() * Exh) + (D + 2) * U * mn((a * xh).abs())
        ref = gx + r * (a - c1 - xh * c2)
        bnd = r.abs() * (dc1 + Exh * (c2.abs() + dc2) + xh.abs() * dc2) + 8 * U * (gx.abs() + r.abs() * (a.abs() + c1.abs() + (xh * c2).abs()))
        out += bounded(dx, ref, bnd, "A4 dx", fig)
    written = torch.zeros(T, D, dtype=F64, device=dev)
    if da is not None:
        out += exact(da, scaled_bf16(dx, inv_of(p), row_keep(seed, seed_state, T, p, dev)), "A5 da", fig)
        written = gr.f64(da)
    if gid is None:
        gid, G, n = _gid(T, rows_per_group, dev)
    else:
        gid, G = gid
        n = torch.bincount(gid, minlength=G)
    got = sums.reshape(G, 3, D)
    for k, (name, terms, extra) in enumerate((("dgamma", gh * xh, gh.abs() * Exh), ("dbeta", gh, None), ("da sums", written, None))):
        out += sums_check(got[:, k], terms, extra, gid, G, n, f"A6 {name}", fig, tier_a)
    return out


# ------------------------------------------------------------------------------------------------------------------- ReLU + dropout
def relu_dropout_fwd_check(x, p, seed, seed_state, y, fig=None):
    keep = torch.from_numpy(keep16_pairs(seed, seed_state, x.numel(), p)).to(x.device).reshape(x.shape)
    return exact(y, scaled_bf16(x, inv_of(p), keep & (x.to(F32) > 0)), "R1 y", fig)


def relu_dropout_bwd_check(dy, y, p, dx, sums, rows_per_group=None, fig=None, tier_a=False):
    """dy: as it was BEFORE the launch (the in-place variant overwrites it); sums: dbias [F] or the partials [groups, F]."""
    T, dev = y.shape[0], y.device
    out = exact(dx, scaled_bf16(dy, inv_of(p), (y.contiguous().view(torch.int16) & 0x7FFF) != 0), "R2 dx", fig)
    gid, G, n = _gid(T, rows_per_group, dev)
    return out + sums_check(sums.reshape(G, -1), gr.f64(dx), None, gid, G, n, "R3 dbias", fig, tier_a)


# ------------------------------------------------------------------------------------------------------------------- colsum
def colsum_check(x, got, fig=None, tier_a=False, what="C1 colsum"):
    T, dev = x.shape[0], x.device
    gid, G, n = _gid(T, None, dev)
    return sums_check(got.reshape(1, -1), gr.f64(x), None, gid, G, n, what, fig, tier_a)


# ------------------------------------------------------------------------------------------------------------------- embedding
def embed_classes(boards):
    """uint8 [M, 16] -> long [M * 17]: the table row of every token row, 31 for the CLS rows."""
    M = boards.shape[0]
    e = torch.full((M, SEQ), 31, dtype=torch.long, device=boards.device)
    e[:, 1:] = boards.long().clamp_max(30)
    return e.reshape(-1)


def embed_fwd_check(boards, table, pe, cls, p, seed, seed_state, x0, fig=None, ln=None):
    """table f32 [31, 256] class-major (the caller transposes the other layouts); ln = (gamma, beta, eps, h, mean, rstd) or None."""
    M, dev = boards.shape[0], boards.device
    e = embed_classes(boards)
    is_cls = e == 31
    keep = embed_keep(seed, seed_state, M, p, dev)
    pos = torch.arange(M * SEQ, device=dev) % SEQ
    s = rne32(gr.f64(table)[e.clamp_max(30)] + gr.f64(pe)[(pos - 1).clamp_min(0)])
    want = torch.where(keep, rne32(s * inv_of(p)), torch.zeros((), dtype=F64, device=dev))
    want = torch.where(is_cls[:, None], gr.f64(cls).expand(M * SEQ, D), want)
    out = exact(x0.reshape(M * SEQ, D), want, "E1 x0", fig)
    if ln is not None:
        gamma, beta, eps, h, mean, rstd = ln
        out += ln_check(x0.reshape(M * SEQ, D), gamma, beta, eps, h.reshape(M * SEQ, D), mean, rstd, "E2", "E2", fig)
    return out


def embed_bwd_check(boards, g, p, seed, seed_state, got, groups=None, fig=None, tier_a=False):
    """g f32 [M * 17, 256]; got: dwt_dcls [32, 256] (``groups`` None) or the partials [groups, 32 * 256], workgroup b of which adds the
    rows [b per, (b + 1) per), per = ceil(rows / groups)."""
    M, dev = boards.shape[0], boards.device
    R = M * SEQ
    e = embed_classes(boards)
    keep = embed_keep(seed, seed_state, M, p, dev)
    terms = torch.where(keep, rne32(gr.f64(g) * inv_of(p)), torch.zeros((), dtype=F64, device=dev))
    terms = torch.where((e == 31)[:, None], gr.f64(g), terms)
    G = 1 if groups is None else groups
    per = -(-R // G)
    gid = (torch.arange(R, device=dev) // per) * 32 + e
    n = torch.bincount(gid, minlength=G * 32)
    ref, mag = group_sums(terms, gid, G * 32), group_sums(terms.abs(), gid, G * 32)
    got = got.reshape(G * 32, D)
    if tier_a:
        gr.assert_exact(mag)
        return exact(got, ref, "E3 dwt_dcls", fig)
    return bounded(got, ref, mag * ((n.to(F64).reshape(-1, 1) + 1) * 2.0 ** -23 + U), "E3 dwt_dcls", fig)


# ------------------------------------------------------------------------------------------------------------------- ppo_loss
class V:
    """(value, error bound) in float64 under the running error analysis of the module docstring."""

    def __init__(self, v, e=None):
        self.v, self.e = v, torch.zeros_like(v) if e is None else e

    def __add__(self, o):
        s, e = self.v + o.v, self.e + o.e
        return V(s, e + U * (s.abs() + e))

    def __sub__(self, o):
        return self + V(-o.v, o.e)

    def __mul__(self, o):
        a, b = self.v.abs(), o.v.abs()
        return V(self.v * o.v, a * o.e + b * self.e + self.e * o.e + U * (a + self.e) * (b + o.e))

    def __neg__(self):
        return V(-self.v, self.e)

    def exp(self):
        v = self.v.exp()
        return V(v, v * (self.e.exp() * (1 + RHO) - 1))

    def log(self):
        dl = -torch.log1p(-(self.e / self.v).clamp_max(0.5))
        lg = self.v.log()
        return V(lg, dl + RHO * (lg.abs() + dl))

    def sel(self, idx):
        return V(self.v.gather(1, idx), self.e.gather(1, idx))


def _weight(ratio, A, lo, hi):
    """W of the module docstring at the float64 ``ratio``."""
    s1, s2 = ratio * A, ratio.clamp(lo, hi) * A
    w1 = torch.where(s1 < s2, 1.0, torch.where(s1 == s2, 0.5, 0.0)).to(F64)
    return w1 + (1 - w1) * ((ratio >= lo) & (ratio <= hi)).to(F64)


def ppo_loss_ref(logits, values, actions, mask_bits, old_logp, adv, ret, clip_eps, c_value, c_entropy, scale=None):
    """-> dict of V (new_logp [M], terms [M, 5], dlogits [n_w, M, 4] for the candidate weights, dvalues [M]), the weights W [n_w, M],
    ``undecided`` bool [M] and the f64 ratio."""
    M, dev = actions.numel(), logits.device
    lo, hi = float(np.float32(1.0) - np.float32(clip_eps)), float(np.float32(1.0) + np.float32(clip_eps))
    cv, ce = float(np.float32(c_value)), float(np.float32(c_entropy))
    inv_m = np.float32(1.0) / np.float32(M)
    g_m = float(inv_m if scale is None else np.float32(inv_m * np.float32(scale)))
    l32 = logits.to(F32).reshape(M, 4)
    bits = torch.full((M,), 15, dtype=torch.long, device=dev) if mask_bits is None else mask_bits.long()
    legal = ((bits[:, None] >> torch.arange(4, device=dev)) & 1).bool()
    z = V(gr.f64(torch.where(legal, l32, l32 - _t32(1e8, dev))))
    a_idx = (actions.long() & 3).reshape(M, 1)
    assert bool(legal.gather(1, a_idx).all()), "actions are always legal"
    zmax = V(z.v.max(1, keepdim=True).values)
    e = (z - zmax).exp()
    se = V(torch.zeros(M, 1, dtype=F64, device=dev))
    for j in range(4):
        se = se + V(e.v[:, j:j + 1], e.e[:, j:j + 1])
    lse = zmax + se.log()
    lp = z - V(lse.v.expand(M, 4), lse.e.expand(M, 4))
    pj = lp.exp()
    ent = V(torch.zeros(M, 1, dtype=F64, device=dev))
    for j in range(4):
        ent = ent - V(lp.v[:, j:j + 1], lp.e[:, j:j + 1]) * V(pj.v[:, j:j + 1], pj.e[:, j:j + 1])
    nlp, olp, A = lp.sel(a_idx), V(gr.f64(old_logp).reshape(M, 1)), V(gr.f64(adv).reshape(M, 1))
    d = nlp.v - olp.v
    ratio = (nlp - olp).exp()
    s1 = ratio * A
    s2 = V(ratio.v.clamp(lo, hi), ratio.e) * A
    pl = V(-torch.minimum(s1.v, s2.v), torch.maximum(s1.e, s2.e))
    dv = V(gr.f64(values.to(F32)).reshape(M, 1)) - V(gr.f64(ret).reshape(M, 1))
    vl, el = dv * dv, -ent
    tot = (pl + V(torch.full_like(d, cv)) * vl) + V(torch.full_like(d, ce)) * el
    kl = olp - nlp
    terms = V(torch.cat([t.v for t in (pl, vl, el, tot, kl)], 1), torch.cat([t.e for t in (pl, vl, el, tot, kl)], 1))
    # gradients, one reference per candidate weight
    Ws = torch.stack([_weight(r, A.v, lo, hi) for r in (ratio.v - ratio.e, ratio.v, ratio.v + ratio.e)])  # [3, M, 1]
    undecided = ((Ws != Ws[1]).any(0) & (A.v != 0)).reshape(M)
    onehot = V(torch.zeros(M, 4, dtype=F64, device=dev).scatter_(1, a_idx, 1.0))
    ex = lambda t: V(t.v.expand(M, 4), t.e.expand(M, 4))
    gm = V(torch.full((M, 4), g_m, dtype=F64, device=dev))
    ent_term = V(torch.full((M, 4), ce, dtype=F64, device=dev)) * pj * (lp + ex(ent))
    dl = []
    for W in Ws:
        g_lp = -(V(W * A.v) * ratio)
        dl.append((ex(g_lp) * (onehot - pj) + ent_term) * gm)
    dlog = V(torch.stack([t.v for t in dl]), torch.stack([t.e for t in dl]))
    dval = V(torch.full_like(d, 2.0 * cv)) * dv * V(torch.full_like(d, g_m))
    return dict(new_logp=V(nlp.v.reshape(M), nlp.e.reshape(M)), terms=terms, dlogits=dlog, dvalues=V(dval.v.reshape(M), dval.e.reshape(M)),
                W=Ws.reshape(3, M), undecided=undecided, ratio=ratio.v.reshape(M), M=M)


def undecided_share(ref, planted=None):
    u = ref["undecided"].clone()
    if planted is not None:
        u[planted] = False
    return float(u.double().mean())


def ppo_loss_check(ref, new_logp, sums, dlogits, dvalues, fig=None, planted=None):
    """The outputs of one launch against ``ppo_loss_ref``.  Also asserts the cap on undecided samples."""
    M = ref["M"]
    share = undecided_share(ref, planted)
    assert share <= UNDECIDED_CAP, f"{share:.4f} of the samples are undecided (cap {UNDECIDED_CAP})"
    out = bounded(new_logp, ref["new_logp"].v, ref["new_logp"].e, "L1 new_logp", fig)
    t = ref["terms"]
    mref = t.v.mean(0)
    mb = t.e.mean(0) + (M + 1) * 2.0 ** -23 * (t.v.abs() + t.e).mean(0) + 2 * U * mref.abs()
    out += bounded(sums, mref, mb, "L2 means", fig)
    g = ref["dlogits"]
    bf = dlogits.dtype == BF16
    bnd = bf16_bound(g.v, g.e) if bf else g.e
    err = (gr.f64(dlogits).reshape(1, M, 4) - g.v).abs()
    ok = (err <= bnd).all(2)  # [3, M]: the sample's four gradients within the bound of candidate w
    best = torch.where(ok.any(0), ok.double().argmax(0), torch.ones(M, dtype=torch.long, device=ok.device))  # decided: all three equal
    pick = best.reshape(1, M, 1).expand(1, M, 4)
    out += bounded(dlogits.reshape(M, 4), g.v.gather(0, pick)[0], bnd.gather(0, pick)[0], "L3 dlogits", fig)
    v = ref["dvalues"]
    out += bounded(dvalues.reshape(M), v.v, bf16_bound(v.v, v.e) if dvalues.dtype == BF16 else v.e, "L4 dvalues", fig)
    if fig is not None:
        fig["undecided"] = dict(share=share, planted=0 if planted is None else int(ref["undecided"][planted].sum()))
    return out


def ppo_inputs(M, bf16=False, masks=True, seed=0, clip_eps=0.2):
    """Inputs of one case (CPU): ratios spread over [0.78, 1.28] away from the interval's ends by more than 1e-4 (so that the float64
    reference alone leaves (almost) no sample undecided), every 7th advantage zero, every 5th mask with a single legal action.  old_logp
    is made from the float64 log-probabilities of these logits; the planted samples are set by ``ppo_plant``."""
    g = torch.Generator().manual_seed(7000 + 13 * M + seed)
    logits = 2.0 * torch.randn(M, 4, generator=g)
    values, ret, adv = torch.randn(M, generator=g), torch.randn(M, generator=g), torch.randn(M, generator=g)
    adv[3::7] = 0.0
    actions = torch.randint(0, 4, (M,), generator=g).to(torch.uint8)
    mask_bits = None
    if masks:
        mask_bits = torch.randint(0, 16, (M,), generator=g) | (1 << actions.long())
        mask_bits[2::5] = 1 << actions.long()[2::5]
        mask_bits = mask_bits.to(torch.uint8)
    if bf16:
        logits, values = logits.to(BF16), values.to(BF16)
    lr = 0.5 * torch.rand(M, generator=g, dtype=F64) - 0.25  # log ratio
    ref = ppo_loss_ref(logits, values, actions, mask_bits, torch.zeros(M), adv, ret, clip_eps, 0.5, 0.01)
    nlp = ref["new_logp"].v
    lo, hi = float(np.float32(1.0) - np.float32(clip_eps)), float(np.float32(1.0) + np.float32(clip_eps))
    for edge in (lo, hi):
        near = (lr.exp() - edge).abs() < 1e-4
        lr = torch.where(near, lr + 1e-3, lr)
    old = nlp - lr
    return dict(logits=logits, values=values, actions=actions, mask_bits=mask_bits, old_logp=old.to(F32), adv=adv, ret=ret)


def ppo_plant(inp, new_logp, clip_eps, stride=16):
    """Planted samples from a first launch's (or emulation's) ``new_logp``: of every ``stride`` samples the first gets ratio exactly 1
    (old = new), the next four ratios 0.1 % inside and outside both ends of the interval.  -> bool [M] of the planted samples."""
    M = new_logp.numel()
    old, nl = inp["old_logp"].clone(), new_logp.to(F32).to(inp["old_logp"].device)
    planted = torch.zeros(M, dtype=torch.bool)
    lo, hi = 1.0 - clip_eps, 1.0 + clip_eps
    for k, r in enumerate((1.0, lo * 1.001, lo * 0.999, hi * 0.999, hi * 1.001)):
        if k >= M:
            break
        idx = torch.arange(k, M, stride)
        old[idx] = nl[idx] if k == 0 else (nl[idx].double() - np.log(r)).to(F32)
        planted[idx] = True
    inp["old_logp"] = old
    return planted


# ------------------------------------------------------------------------------------------------------------------- operands
def ln_inputs(T, seed=0, degenerate=False):
    """Tier B operands of add+LN (CPU): x f32 rows at scales 2^[-3, 2] with mean 0.1, a and g_h bf16, g_x f32 [T, 256] (the period-17 cases
    take its first T / 17 rows), gamma around 1, beta with a non-zero mean.  ``degenerate``: every third row has a = 0 and x of standard
    deviation 1e-2 (eps = 1e-5 is 10 % of its variance), row 1 a = 0 and a constant x."""
    g = gr._gen(T, seed, 11)
    scale = torch.exp2(torch.randint(-3, 3, (T, 1), generator=g).float())
    x = torch.randn(T, D, generator=g) * scale + 0.1
    a = torch.randn(T, D, generator=g).to(BF16)
    if degenerate:
        a[0::3] = 0
        x[0::3] = 1e-2 * torch.randn(x[0::3].shape, generator=g)
        if T > 1:
            a[1], x[1] = 0, 0.75
    return dict(x=x, a=a, g_h=(torch.randn(T, D, generator=g) * scale / 16).to(BF16), g_x=torch.randn(T, D, generator=g),
                gamma=1.0 + 0.1 * torch.randn(D, generator=g), beta=0.05 + 0.1 * torch.randn(D, generator=g))


def eps_rows(T):
    return list(range(0, T, 3))


def ln_bwd_tier_a(T, seed=0):
    """Integer operands of the add+LN backward: xn = +-1 with sign (-1)^(row + col) (mean 0; pass mean = 0, rstd = 1, so xh = +-1), gamma
    in {1, 2} equal on the columns c and c + 4, g_h integers in [-4, 4] with g_h[c + 4] = -g_h[c] for c % 8 < 4 (so c1 = c2 = 0 and
    dx = g_x + g_h gamma, an integer), g_x integers in [-8, 8]."""
    g = gr._gen(T, seed, 12)
    c, r = torch.arange(D), torch.arange(T)
    xn = (1 - 2 * ((c[None] + r[:, None]) % 2)).float()
    gamma = torch.where((c // 2) % 2 == 0, 1.0, 2.0)
    gh = torch.randint(-4, 5, (T, D // 8, 2, 4), generator=g)
    gh[:, :, 1] = -gh[:, :, 0]
    return dict(xn=xn, gamma=gamma, g_h=gh.reshape(T, D).to(BF16), g_x=torch.randint(-8, 9, (T, D), generator=g).float(),
                mean=torch.zeros(T), rstd=torch.ones(T))


def relu_inputs(T, F, seed=0):
    """x bf16 [T, F] with -0.0, negatives and values whose product with inv needs rounding; dy bf16 tier B, dy_int tier A."""
    g = gr._gen(T, F, seed, 13)
    x = (torch.randn(T, F, generator=g) * 3).to(BF16)
    flat = x.view(-1)
    flat[0::7] = -0.0
    flat[3::11] = 0.0
    return dict(x=x, dy=torch.randn(T, F, generator=g).to(BF16), dy_int=gr.ints((T, F), -8, 8, g))


def embed_inputs(M, seed=0):
    """boards uint8 [M, 16] holding every value 0..31 and 255 (from M * 16 >= 33 on), table f32 [31, 256], pe [16, 256], cls [256], the
    upstream gradient g f32 [M * 17, 256] and its integer tier g_int."""
    g = gr._gen(M, seed, 14)
    boards = torch.randint(0, 18, (M, 16), generator=g).to(torch.uint8)
    vals = torch.tensor(list(range(32)) + [255], dtype=torch.uint8)
    n = min(33, M * 16)
    boards.view(-1)[torch.randperm(M * 16, generator=g)[:n]] = vals[torch.randperm(33, generator=g)[:n]] if n < 33 else vals
    return dict(boards=boards, table=torch.randn(31, D, generator=g), pe=torch.randn(16, D, generator=g), cls=torch.randn(D, generator=g),
                gamma=1.0 + 0.1 * torch.randn(D, generator=g), beta=0.05 + 0.1 * torch.randn(D, generator=g),
                g=torch.randn(M * SEQ, D, generator=g), g_int=torch.randint(-8, 9, (M * SEQ, D), generator=g).float())
