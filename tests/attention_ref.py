"""Float64 restatement of the update's attention (17 keys, head_dim 32), for the attention tests (not a test module).

Plain torch in float64, no kernel of this repository, no SDPA.  Operands are ``[B, H, Sq, 32]`` (q, dout) and
``[B, H, 17, 32]`` (k, v); bf16 values are promoted exactly.  ``keep`` is a boolean ``[B, H, Sq, 17]`` mask or None.

    attention_ref(q, k, v, dout, keep, p_drop, scale)            -> dict o, lse, dq, dk, dv (float64)
    attention_rounding_model(q, k, v, dout, keep, p_drop, scale) -> the same formulas with the roundings of a bf16 / f32
                                                                    implementation put in (see there): the yardstick
    pair_errors(got, want) / whole_error(got, want)              -> relative 2-norm errors per (sample, head) pair / whole
    accept(got, ref, model, floor=None)                          -> list of failures (empty: accepted)
    probe_operands / keep_from_forward_probe / keep_from_backward_probe: the dropout mask a kernel applied, read back
                                                                    from its outputs on one-hot operands
    xcd_block(n, blk)                                            -> the workgroup -> item map of the attention kernels

Formulas (P the softmax of the UNDROPPED scaled scores, keep/(1-p) applied afterwards, as nn.MultiheadAttention does):
    P = softmax(Q K^T scale)      Pd = P keep / (1-p)      O = Pd V           lse = logsumexp(Q K^T scale)
    dV = Pd^T dO                  dP = (dO V^T) keep / (1-p)
    dS = P o (dP - rowsum(P o dP)) scale                   dQ = dS K          dK = dS^T Q
"""
import torch

SK, HD = 17, 32
WHOLE_BOUND = 4e-3  # whole-tensor relative 2-norm error of o, dq, dk, dv (the bound test_small_attention_kernels_match_sdpa applies)
PAIR_FACTOR = 2.0   # worst per-pair error allowed, as a multiple of the rounding model's worst per-pair error
OUTPUTS = ("o", "dq", "dk", "dv")
LOG2E = 1.4426950408889634


def _f64(t):
    return t.detach().to("cpu").to(torch.float64)


def _bf16(t):  # round to nearest even (through f32, as a kernel that computes in f32 and stores bf16 does)
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _f32(t):
    return t.to(torch.float32).to(torch.float64)


def _ident(t):
    return t


def _attention(q, k, v, dout, keep, p_drop, scale, r16, r32):
    q, k, v, dout = _f64(q), _f64(k), _f64(v), _f64(dout)
    inv_keep = 1.0 / (1.0 - p_drop)
    w = torch.ones(q.shape[:3] + (SK,), dtype=torch.float64) if keep is None else keep.to("cpu").to(torch.float64)
    w = w * inv_keep
    # forward: scores from exact bf16 x bf16 products, softmax around the row maximum, lse = m + log(l) stored as f32
    s = torch.einsum("bhqd,bhkd->bhqk", q, k)  # unscaled, as the accumulator holds them
    m = s.max(dim=-1, keepdim=True).values
    e = r32(torch.exp(r32(r32(s - m) * scale)))
    l = r32(e.sum(dim=-1, keepdim=True))
    lse = r32(r32(m * scale) + r32(torch.log(l)))
    pd = r16(r32(e / l) * w)
    o = r16(torch.einsum("bhqk,bhkd->bhqd", pd, v))
    # backward: P recomputed from the scores and the STORED lse (in base 2: exp2(s * scale * log2e - lse * log2e))
    if r32 is _ident:
        p = torch.exp(s * scale - lse)
    else:
        p = r32(torch.exp2(r32(r32(s * r32(torch.tensor(scale * LOG2E))) - r32(lse * LOG2E))))
    pdb = r16(p * w)
    dv = r16(torch.einsum("bhqk,bhqd->bhkd", pdb, dout))
    dp = r32(r32(torch.einsum("bhqd,bhkd->bhqk", dout, v)) * w)
    delta = r32((p * dp).sum(dim=-1, keepdim=True))
    ds = r16(r32(p * r32(dp - delta)) * scale)
    dq = r16(torch.einsum("bhqk,bhkd->bhqd", ds, k))
    dk = r16(torch.einsum("bhqk,bhqd->bhkd", ds, q))
    return dict(o=o, lse=lse.squeeze(-1), dq=dq, dk=dk, dv=dv)


def attention_ref(q, k, v, dout, keep, p_drop, scale):
    """The float64 reference: no rounding anywhere."""
    return _attention(q, k, v, dout, keep, p_drop, scale, _ident, _ident)


def attention_rounding_model(q, k, v, dout, keep, p_drop, scale):
    """The reference's formulas with the roundings of an implementation that keeps its matrix operands in bf16 and everything
    else in f32: bf16 round-to-nearest-even on ``Pd`` and ``dS`` before they become matrix operands and on the five outputs
    (lse: f32); f32 on the softmax statistics, on the stored lse, on the recomputed P of the backward, on dP, on
    delta = rowsum(P o dP) and on dP - delta.  The f32 part matters where the softmax is (nearly) one-hot: there
    dP_j - delta cancels to the size of the f32 error of P_j (|score| 2^-24 relative, from exp(s - lse) with both arguments
    rounded), and a (sample, head) pair all of whose rows are one-hot has a dQ / dK made of little else.  Built from the
    reference above, not from any kernel; its distance to ``attention_ref`` is the yardstick for per-pair errors."""
    return _attention(q, k, v, dout, keep, p_drop, scale, _bf16, _f32)


def whole_error(got, want) -> float:
    got, want = _f64(got), _f64(want)
    den = want.norm().item()
    num = (got - want).norm().item()
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))


def pair_errors(got, want) -> torch.Tensor:
    """Relative 2-norm error per (sample, head) pair of ``[B, H, ...]`` tensors; a pair whose reference is exactly zero (every
    key dropped) counts 0 when the result is exactly zero too, inf otherwise."""
    got, want = _f64(got).flatten(2), _f64(want).flatten(2)
    num, den = (got - want).norm(dim=-1), want.norm(dim=-1)
    err = num / den.clamp_min(1e-300)
    return torch.where(den > 0, err, torch.where(num > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))


def model_pair_worst(ref: dict, model: dict) -> dict:
    return {n: pair_errors(model[n], ref[n]).max().item() for n in OUTPUTS}


def accept(got: dict, ref: dict, model: dict, floor: dict | None = None, figures: dict | None = None) -> list:
    """The acceptance of o, dq, dk, dv against the float64 reference: every value finite; whole-tensor relative 2-norm error
    below ``WHOLE_BOUND``; worst per-(sample, head)-pair error below ``PAIR_FACTOR`` x the rounding model's worst per-pair error
    on the same inputs (or ``floor[name]``, the model's worst over a large fixed draw, when that is larger: for cells with few
    pairs).  Returns the failures as strings; ``figures`` (optional dict) receives every measured number."""
    bad = []
    worst_model = model_pair_worst(ref, model)
    for n in OUTPUTS:
        g = _f64(got[n])
        if not torch.isfinite(g).all():
            bad.append(f"{n}: non-finite values")
            continue
        whole, pair = whole_error(g, ref[n]), pair_errors(g, ref[n]).max().item()
        yard = max(worst_model[n], floor[n] if floor else 0.0)
        if figures is not None:
            figures[n] = dict(whole=whole, pair=pair, model_pair=worst_model[n], yard=yard, ratio=pair / yard if yard > 0 else 0.0)
        if not whole < WHOLE_BOUND:
            bad.append(f"{n}: whole-tensor error {whole:.3e} >= {WHOLE_BOUND:.0e}")
        if not pair <= PAIR_FACTOR * yard:
            bad.append(f"{n}: worst per-pair error {pair:.3e} > {PAIR_FACTOR} x {yard:.3e}")
    return bad


# ---------------------------------------------------------------------------------------------------------- lse bound
# The kernels store lse = m * scale + logf(l) in f32, with m the row maximum of the scores, each score a 32-term dot product of
# exact bf16 x bf16 products accumulated in f32, and l = sum_j exp((s_j - m) * scale) in [1, 17].
#   * the dot product: 32 additions, each within 2^-24 relative of a partial sum bounded by A = sum_d |q_d k_d|: the score
#     carries at most 32 * 2^-24 * A, scaled by `scale`; A * scale <= A_max * scale, and A >= |s| - so with a = A * scale the
#     first term is 32 * 2^-24 * a.  (An MFMA accumulates in a tree, the scalar kernels in a chain: 32 covers both.)
#   * m * scale: one rounding, 2^-24 |m scale| <= 2^-24 a
#   * logf(l): l's own error (17 exps of <= 2 ulp each, their arguments (s_j - m) * scale rounded up to 3 times: |x| e^x <= 0.37 per
#     term; 17 additions; all relative: <= (34 + 19 + 17) 2^-24 = 70 * 2^-24 relative at the very most, which is the ABSOLUTE error it
#     puts on log l) + the fast logarithm's own (hardware log2 to 1 ulp of a value below 4.09, times ln 2, rounded: <= 6 * 2^-24 abs)
#   * the final addition: 2^-24 |lse| <= 2^-24 (a + 3)
# With a >= |lse| - log 17 this is  |err| <= 34 * 2^-24 * a + 80 * 2^-24, a = scale * sum_d |q_d k_d| of the row's maximal key,
# bounded here by the row's largest a over the keys (computed in float64 from the operands).
def lse_bound(q, k, scale) -> torch.Tensor:
    """The derived bound on |lse_kernel - lse_float64| per (b, h, query): 34 * 2^-24 * a + 80 * 2^-24 (see the comment above)."""
    a = torch.einsum("bhqd,bhkd->bhqk", _f64(q).abs(), _f64(k).abs()).max(dim=-1).values * abs(scale)
    return (34.0 * a + 80.0) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------- test operands
def make_operands(B: int, H: int, Sq: int, seed: int, qk_std: float = 1.5):
    """q [B, Sq, H, 32], k, v [B, 17, H, 32], dout [B, Sq, H, 32] as bf16 CPU tensors: Q, K = randn * qk_std (1.5: scores with sigma
    about 2, the usual range; 8: sigma about 64, row maxima beyond 88 where a bare f32 exp overflows), V = randn * 1.5, dO = randn."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, Sq, H, HD, generator=g) * qk_std).to(torch.bfloat16)
    k = (torch.randn(B, SK, H, HD, generator=g) * qk_std).to(torch.bfloat16)
    v = (torch.randn(B, SK, H, HD, generator=g) * 1.5).to(torch.bfloat16)
    dout = torch.randn(B, Sq, H, HD, generator=g).to(torch.bfloat16)
    return q, k, v, dout


def bhsd(t):
    """[B, S, H, 32] (the kernels' layout) <-> [B, H, S, 32] (the reference's)."""
    return t.transpose(1, 2)


_FLOOR = {}


def model_floor(Sq: int, p_drop: float, qk_std: float = 1.5) -> dict:
    """The rounding model's worst per-pair error over a fixed draw of 2048 pairs of the test distribution (Bernoulli(1 - p) mask):
    the yardstick for cells with fewer than 256 pairs, where the worst of a handful is noise.  Computed once per process."""
    key = (Sq, p_drop, qk_std)
    if key not in _FLOOR:
        q, k, v, dout = (bhsd(t) for t in make_operands(2048, 1, Sq, 4242, qk_std))
        g = torch.Generator().manual_seed(4243)
        keep = (torch.rand(2048, 1, Sq, SK, generator=g) >= p_drop) if p_drop > 0 else None
        scale = HD ** -0.5
        _FLOOR[key] = model_pair_worst(attention_ref(q, k, v, dout, keep, p_drop, scale),
                                       attention_rounding_model(q, k, v, dout, keep, p_drop, scale))
    return _FLOOR[key]


# ---------------------------------------------------------------------------------------------------------- mask probes
# The keep decision depends only on (seed, seed_state, pair, query, key), never on values.  So it can be read back from a
# launch on operands of the probe's own choosing: moderate Q, K (randn * 1.5: the smallest probability over 4096 x 17 x 17 draws
# is 5.6e-9, far above bf16's smallest normal, so no kept probability rounds to zero) and one-hot V or dO.
def probe_operands(B: int, H: int, Sq: int, seed: int = 1234):
    """q [B, Sq, H, 32], k, v [B, 17, H, 32], dout [B, Sq, H, 32] (bf16, CPU) with V[b, j, h, :] = e_j and dO[b, q, h, :] = e_q."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, Sq, H, HD, generator=g) * 1.5).to(torch.bfloat16)
    k = (torch.randn(B, SK, H, HD, generator=g) * 1.5).to(torch.bfloat16)
    eye = torch.eye(HD, dtype=torch.bfloat16)
    v = eye[:SK].view(1, SK, 1, HD).expand(B, SK, H, HD).contiguous()
    dout = eye[:Sq].view(1, Sq, 1, HD).expand(B, Sq, H, HD).contiguous()
    return q, k, v, dout


def keep_from_forward_probe(o) -> torch.Tensor:
    """o [B, Sq, H, 32] of a forward on probe operands: o[b, q, h, j] = Pd[q, j] -> keep [B, H, Sq, 17]."""
    return (o.detach().cpu().float()[..., :SK] != 0).permute(0, 2, 1, 3).contiguous()


def keep_from_backward_probe(dv, Sq: int) -> torch.Tensor:
    """dv [B, 17, H, 32] of a backward on probe operands: dv[b, j, h, q] = Pd[q, j] -> keep [B, H, Sq, 17] as the BACKWARD applied it."""
    return (dv.detach().cpu().float()[..., :Sq] != 0).permute(0, 2, 3, 1).contiguous()


def xcd_block(n: int, blk: int) -> int:
    """The kernels' workgroup -> item map as integer arithmetic: workgroup ``blk`` of a grid of ``n`` runs on XCD blk % 8 and takes
    item x * (n / 8) + min(x, n % 8) + blk / 8."""
    q, r, x = n // 8, n % 8, blk % 8
    return x * q + min(x, r) + blk // 8
