"""Float64 restatement of g2048_distill_loss (include/g2048.h, "imitation update: loss") with per-element error bounds.

The reference follows the definition per sample from the f32 / bf16 inputs:
    z_j = l_j or f32(l_j - 1e8) (one rounding point), lse = zmax + log sum exp(z_j - zmax), lp_j = z_j - lse, pi_j = exp(lp_j),
    ent = -sum lp_j pi_j;  a* = first maximum of q_j or f32(q_j - 1e8);  p*_j = one-hot at a* (tau == 0) or
    t_j / sum_legal t, t_j = exp((q_j - q_a*) / tau) (tau > 0);  ce = -sum_legal p*_j lp_j, vl = (V - vt)^2, el = -ent,
    tot = (ce + c_v vl) + c_e el;  dz_j = ((pi_j - p*_j) + (c_e pi_j) (lp_j + ent)) g_m,  dV = ((2 c_v) (V - vt)) g_m,
    g_m = f32(f32(1 / M) scale).  A row with mask_bits == 0 is all zeros.

Bounds: the running error analysis of tests/rowwise_ref.py (class ``V``: u = 2^-24 per f32 operation, rho = 2^-22 relative for expf
and logf - the same ASSUMPTION as there), carried through every operation of the kernel's statement (csrc/g2048_distill.h):
  D1 new_logp     E(lp_a*): one rounding for z_j - zmax, rho per expf, three adds for se, rho and E(se) / se for logf, two more adds.
  D2 the means    mean of the per-term errors + (M + 1) 2^-23 mean(|term| + error) for the sums (256 lanes by shuffles, four waves, then
                  ceil(M / 256) partials: any order is covered) + 2u |ref| (f32(1 / M) and the product).  Agreement is a mean of exact
                  0 / 1 terms: only the sum's share.
  D3 dlogits      through pi_j - p*_j and (c_e pi_j)(lp_j + ent), times g_m; for tau > 0 the division (q_j - q_a*) / tau is one rounding,
                  rho for expf, three adds for the sum, E(t / s) = (E_t + |t / s| E_s) / (s - E_s) + u |t / s|.  bf16 outputs: bf16_bound.
  D4 dvalues      two multiplies after the subtraction, times g_m.
Argmaxes.  Both a* and the student's first maximum compare f32 numbers that the definition fixes exactly (an input, or ONE IEEE
subtraction of 1e8 from it): the bound of a tie is 0, so only an exact tie is within it, and there the first-maximum rule decides.  A
sample counts as undecided where either top-two gap is below ``TIE_GAP`` without being a planted exact tie; the generated inputs keep all
gaps >= 1e-3, so no sample is undecided (asserted on the CPU, capped at 1 % like rowwise_ref's).
"""
import numpy as np
import torch

import gemm_ref as gr
from rowwise_ref import RHO, U, UNDECIDED_CAP, V, bf16_bound, bounded  # noqa: F401

BF16, F32, F64 = gr.BF16, gr.F32, gr.F64
TIE_GAP = 1e-3
N_PLANTED = 10
MS = (1, 63, 255, 256, 257, 2055)
TAUS = (0.0, 1.0, 100.0)
SCALES = (None, 1024.0, 1000.0)
C_VALUE, C_ENTROPY = 0.5, 0.01


def _t32(v, dev):
    return torch.tensor(np.float32(v), dtype=F32, device=dev)


def _legal(mask_bits, M, dev):
    bits = torch.full((M,), 15, dtype=torch.long, device=dev) if mask_bits is None else (mask_bits.long() & 15)
    return ((bits[:, None] >> torch.arange(4, device=dev)) & 1).bool()


def masked32(x32, legal):
    """x or f32(x - 1e8): the f32 numbers both argmaxes compare."""
    return torch.where(legal, x32, x32 - _t32(1e8, x32.device))


def first_max(x):
    """[M, 4] -> the first index of the row maximum (torch.argmax does not promise the first)."""
    eq = x == x.max(1, keepdim=True).values
    return torch.where(eq, torch.arange(4, device=x.device), 4).min(1).values


def top_gap(x):
    s = x.to(F64).sort(1, descending=True).values
    return s[:, 0] - s[:, 1]


def _col(t, j):
    return V(t.v[:, j:j + 1], t.e[:, j:j + 1])


def _div(a, b):
    """a / b for b > E_b > 0: one rounded division."""
    q = a.v / b.v
    return V(q, (a.e + q.abs() * b.e) / (b.v - b.e) + U * q.abs())


def _where(c, a, zero_like):
    z = torch.zeros_like(zero_like.v)
    return V(torch.where(c, a.v, z), torch.where(c, a.e, z))


def distill_ref(logits, values, mask_bits, teacher_q, value_target, tau, c_value, c_entropy, scale=None):
    """-> dict of V (new_logp [M], terms [M, 5], dlogits [M, 4], dvalues [M] or None), a_star, a_student, undecided, M."""
    M, dev = teacher_q.numel() // 4, logits.device
    tau32, cv, cen = float(np.float32(tau)), float(np.float32(c_value)), float(np.float32(c_entropy))
    inv_m = np.float32(1.0) / np.float32(M)
    g_m = float(inv_m if scale is None else np.float32(inv_m * np.float32(scale)))
    legal = _legal(mask_bits, M, dev)
    live = legal.any(1, keepdim=True)
    l32, q32 = logits.to(F32).reshape(M, 4), teacher_q.to(F32).reshape(M, 4)
    z32, qm32 = masked32(l32, legal), masked32(q32, legal)
    a_star, a_student = first_max(qm32), first_max(z32)
    z = V(gr.f64(z32))
    zmax = V(z.v.max(1, keepdim=True).values)
    e = (z - zmax).exp()
    se = V(torch.zeros(M, 1, dtype=F64, device=dev))
    for j in range(4):
        se = se + _col(e, j)
    lse = zmax + se.log()
    ex = lambda t: V(t.v.expand(M, 4), t.e.expand(M, 4))
    lp = z - ex(lse)
    pj = lp.exp()
    ent = V(torch.zeros(M, 1, dtype=F64, device=dev))
    for j in range(4):
        ent = ent - _col(lp, j) * _col(pj, j)
    a_idx = a_star.reshape(M, 1)
    onehot = torch.zeros(M, 4, dtype=F64, device=dev).scatter_(1, a_idx, 1.0)
    if tau32 > 0.0:
        q = V(gr.f64(q32))
        qa = q.sel(a_idx)
        d = q - ex(qa)
        arg = d.v / tau32
        t = V(arg, d.e / tau32 + U * arg.abs()).exp()
        t = _where(legal, t, t)
        ts = V(torch.zeros(M, 1, dtype=F64, device=dev))
        for j in range(4):
            ts = ts + _col(t, j)
        ts = V(torch.where(live, ts.v, torch.ones_like(ts.v)), ts.e)  # (rows without a legal action are zeroed below)
        pstar = _div(t, ex(ts))
    else:
        pstar = V(onehot)
    ce = V(torch.zeros(M, 1, dtype=F64, device=dev))
    for j in range(4):
        term = _col(pstar, j) * _col(lp, j)
        ce = ce - _where(legal[:, j:j + 1], term, term)
    nlp = lp.sel(a_idx)
    el = -ent
    has_v = values is not None
    if has_v:
        dv = V(gr.f64(values.to(F32)).reshape(M, 1)) - V(gr.f64(value_target).reshape(M, 1))
        vl = dv * dv
        dval = (V(torch.full_like(dv.v, 2.0 * cv)) * dv) * V(torch.full_like(dv.v, g_m))
    else:
        vl = V(torch.zeros(M, 1, dtype=F64, device=dev))
    full = lambda c: V(torch.full((M, 1), c, dtype=F64, device=dev))
    tot = (ce + full(cv) * vl) + full(cen) * el
    agree = V((a_student == a_star).to(F64).reshape(M, 1))
    cols = (ce, vl, el, tot, agree)
    terms = V(torch.cat([c.v for c in cols], 1), torch.cat([c.e for c in cols], 1))
    dz = ((pj - pstar) + (V(torch.full((M, 4), cen, dtype=F64, device=dev)) * pj) * (lp + ex(ent))) * V(torch.full((M, 4), g_m, dtype=F64, device=dev))
    zero = lambda t, shape: V(torch.where(live.expand(shape), t.v, torch.zeros_like(t.v)), torch.where(live.expand(shape), t.e, torch.zeros_like(t.e)))
    out = dict(new_logp=zero(nlp, (M, 1)), terms=zero(terms, (M, 5)), dlogits=zero(dz, (M, 4)), dvalues=zero(dval, (M, 1)) if has_v else None,
               a_star=a_star, a_student=a_student, M=M, legal=legal, pstar=pstar.v)
    for k in ("new_logp", "dvalues"):
        if out[k] is not None:
            out[k] = V(out[k].v.reshape(M), out[k].e.reshape(M))
    gap = torch.minimum(top_gap(z32), top_gap(qm32))
    out["undecided"] = (gap < TIE_GAP) & (gap > 0) & live.reshape(M)  # an exact tie (gap 0) is decided by the first-maximum rule
    return out


def undecided_share(ref, planted=0):
    u = ref["undecided"][planted:]
    return float(u.double().mean()) if u.numel() else 0.0


def distill_check(ref, new_logp, sums, dlogits, dvalues, fig=None, planted=0, show=None):
    """The outputs of one call against ``distill_ref`` -> [] or messages.  Asserts the cap on undecided samples; ``show``: a label under
    which the worst error / bound of every stage is printed."""
    M = ref["M"]
    share = undecided_share(ref, planted)
    assert share <= UNDECIDED_CAP, f"{share:.4f} of the unplanted samples are undecided (cap {UNDECIDED_CAP})"
    fig = {} if fig is None else fig
    dev = ref["terms"].v.device
    on = lambda t: t.to(dev)
    out = bounded(on(new_logp), ref["new_logp"].v, ref["new_logp"].e, "D1 new_logp", fig)
    t = ref["terms"]
    mref = t.v.mean(0)
    mb = t.e.mean(0) + (M + 1) * 2.0 ** -23 * (t.v.abs() + t.e).mean(0) + 2 * U * mref.abs()
    keep = ~ref["undecided"]
    if not bool(keep.all()):  # undecided samples leave the agreement comparison only: either answer is accepted for them
        mb[4] = mb[4] + float((~keep).sum()) / M
    out += bounded(on(sums), mref, mb, "D2 means", fig)
    g = ref["dlogits"]
    out += bounded(on(dlogits).reshape(M, 4), g.v, bf16_bound(g.v, g.e) if dlogits.dtype == BF16 else g.e, "D3 dlogits", fig)
    if ref["dvalues"] is not None:
        v = ref["dvalues"]
        out += bounded(on(dvalues).reshape(M), v.v, bf16_bound(v.v, v.e) if dvalues.dtype == BF16 else v.e, "D4 dvalues", fig)
    if show is not None:
        print(show, " ".join(f"{k.split()[0]} {v['ratio']:.3f}" for k, v in fig.items() if "ratio" in v), f"undecided {share:.4f}")
    return out


# ------------------------------------------------------------------------------------------------------------------- inputs
def inputs(M, bf16=False, masks=True, values=True, seed=0):
    """Inputs of one case (CPU tensors): per row four distinct logits on a 1/32 grid in [-4, 4] (bf16 numbers: the gaps survive the
    cast) and four distinct teacher scores on a 0.5 grid around a per-row base of score magnitude; every 5th mask a single legal
    action.  The first ``min(M, N_PLANTED)`` rows are then planted (``plant``)."""
    g = torch.Generator().manual_seed(9100 + 17 * M + seed)
    pick = lambda n: torch.rand(M, n, generator=g).argsort(1)[:, :4]
    logits = (pick(257) - 128).float() / 32.0
    q = pick(400).float() * 0.5 + torch.randint(0, 3000, (M, 1), generator=g).float()
    mask_bits = None
    if masks:
        mask_bits = torch.randint(1, 16, (M,), generator=g)
        mask_bits[2::5] = 1 << torch.randint(0, 4, (M,), generator=g)[2::5]
        mask_bits = mask_bits.to(torch.uint8)
    v = vt = None
    if values:
        v, vt = torch.randn(M, generator=g), torch.randn(M, generator=g)
    d = dict(logits=logits, values=v, mask_bits=mask_bits, teacher_q=q.contiguous(), value_target=vt)
    plant(d)
    if bf16:
        d["logits"] = d["logits"].to(BF16)
        if values:
            d["values"] = d["values"].to(BF16)
    return d


#        teacher_q                     logits            mask    what
PLANTED = [
    ((7.0, 3.0, 7.0, 1.0),            (0.5, 1.0, -1.0, 0.0), 15, "two-way tie of q among legal actions: a* = 0"),
    ((4.0, 4.0, 4.0, 4.0),            (0.0, 2.0, 1.0, -1.0), 15, "four-way tie, all-equal q: a* = 0, p* uniform for tau > 0"),
    ((5.0, 3.0, 3.0, 1.0),            (1.0, 0.0, 2.0, -2.0), 6, "an illegal maximum over a legal two-way tie: a* = 1"),
    ((1.0, 2.0, 3.0, 4.0),            (3.0, -1.0, 0.25, 1.0), 4, "a single legal action: ce == 0, dlogits is the entropy term (0)"),
    ((1.0, 2.0, 3.0, 4.0),            (1.0, 2.0, 3.0, 4.0), 0, "no legal action: all zeros"),
    ((1e5, -1e5, 3e4, 9.9e4),        (0.0, 1.0, 2.0, 3.0), 15, "scores of 1e5: one-hot by underflow at tau = 1, no NaN"),
    ((2.5, 2.5, 2.5, 2.5),            (1.0, 0.5, 0.0, 2.0), 10, "all-equal q under a mask: a* = 1"),
    ((9.0, 1.0, 2.0, 3.0),            (2.0, 1.0, 0.0, -1.0), 15, "V == value_target: vl = dvalues = 0"),
    ((9.0, 1.0, 2.0, 3.0),            (1.0, 1.0, 0.0, 0.0), 15, "the student's maximum is tied: first index 0 = a*, agreement 1"),
    ((1.0, 2.0, 9.0, 3.0),            (0.0, 1.0, 1.0, 0.0), 15, "the student's maximum is tied: first index 1 != a* = 2, agreement 0"),
]
assert len(PLANTED) == N_PLANTED


def plant(d):
    M = d["teacher_q"].shape[0]
    for i, (q, l, mb, _what) in enumerate(PLANTED[:M]):
        d["teacher_q"][i] = torch.tensor(q)
        d["logits"][i] = torch.tensor(l)
        if d["mask_bits"] is not None:
            d["mask_bits"][i] = mb
    if d["values"] is not None and M > 7:
        d["values"][7] = d["value_target"][7] = 0.75


def planted_expectations(ref, d, tau):
    """What the planted rows promise, asserted on the reference itself (so every consumer of the reference inherits them)."""
    M, masked = ref["M"], d["mask_bits"] is not None
    want_a = [0, 0, 1 if masked else 0, 2 if masked else 3, None, 0, 1 if masked else 0, 0, 0, 2]
    for i in range(min(M, N_PLANTED)):
        if i == 4 and masked:
            assert not ref["terms"].v[i].any() and not ref["dlogits"].v[i].any() and not ref["terms"].e[i].any()
            continue
        if want_a[i] is not None:
            assert int(ref["a_star"][i]) == want_a[i], (i, int(ref["a_star"][i]))
    if M > 3 and masked:
        assert float(ref["terms"].v[3, 0]) == 0.0 and not ref["dlogits"].v[3].any()
    if M > 5 and tau == 1.0:
        assert torch.equal(ref["pstar"][5], torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=F64)) and bool(torch.isfinite(ref["terms"].v[5]).all())
    if M > 1 and tau > 0:
        assert torch.equal(ref["pstar"][1], torch.full((4,), 0.25, dtype=F64))
    if M > 7 and d["values"] is not None:
        assert float(ref["terms"].v[7, 1]) == 0.0 and float(ref["dvalues"].v[7]) == 0.0
    if M > 9:
        assert float(ref["terms"].v[8, 4]) == 1.0 and float(ref["terms"].v[9, 4]) == 0.0


# ------------------------------------------------------------------------------------------------------------------- autograd
def torch_loss64(logits, values, mask_bits, teacher_q, value_target, tau, c_value, c_entropy):
    """The same loss composed from differentiable float64 torch ops -> the mean total loss (``logits`` / ``values`` f64 leaves)."""
    M = teacher_q.shape[0]
    legal = _legal(mask_bits, M, logits.device)
    live = legal.any(1)
    z = torch.where(legal, logits, logits - 1e8)
    lp = torch.log_softmax(z, 1)
    p = lp.exp()
    ent = -(lp * p).sum(1)
    q = teacher_q.to(F64)
    a = first_max(torch.where(legal, q, q - 1e8))
    if tau > 0:
        t = torch.where(legal, ((q - q.gather(1, a[:, None])) / tau).exp(), torch.zeros_like(q))
        pstar = t / t.sum(1, keepdim=True).clamp_min(1e-300)
    else:
        pstar = torch.zeros_like(q).scatter_(1, a[:, None], 1.0)
    ce = -(torch.where(legal, pstar * lp, torch.zeros_like(lp))).sum(1)
    tot = ce + c_entropy * -ent
    if values is not None:
        tot = tot + c_value * (values - value_target.to(F64)) ** 2
    return torch.where(live, tot, torch.zeros_like(tot)).sum() / M
