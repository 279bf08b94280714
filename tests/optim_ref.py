"""Float64 / exact-float32 stage references, case generators and acceptance rules for the optimiser kernels (csrc/g2048_optim.hip:
g2048_opt_step, g2048_lamb_step) and the second-stage gradient reduction (csrc/g2048_reduce.hip: g2048_reduce_jobs).
tests/test_gpu_optim_f64.py runs the kernels against them, tests/test_optim_ref.py holds them to an f32 emulation of the kernels as their
source states them and to planted defects on the CPU.  numpy + torch only; runs anywhere.

Every stage is checked from the kernel's OWN inputs of that stage: the kernels leave their intermediates in the workspace (layout above
g2048_opt_step / g2048_lamb_step in the .hip file; ``read_adamw_ws`` / ``read_lamb_ws`` are the one reader per layout), so a stage is
never held to the accumulated error of the stages before it.  u = 2^-24; s(n) = (n + 1) 2^-23 sum |terms| is ``gemm_ref.bound`` (any-order
summation, which also covers a truncating accumulator).

    N1  partial[b]      sum over chunk b of f32(g inv_scale)^2 against float64 of the same f32 products: s(n) + u |term| per square.
                        Tier A (integer gradients, power-of-two scale, sum < 2^24 by ``gemm_ref.assert_exact``): exact.
    N2  total, info[0]  the sum of the kernel's partials within s(n_chunks), tier A exact.  LAMB keeps the total in flags[0] and info[0] must
                        be its f32 sqrt bit for bit; AdamW keeps no total, so info[0] must be the f32 sqrt of SOME f32 within the bound.
                        info[1] / flags[1]: the non-finiteness of that total with a scaler, 0 without.
    D1  Derived         every field against float64 (here: 60-digit decimal) from the f64 hyper-parameters and t = steps[0] + 1, rounded
                        once: |d - ref| <= 2^-24 |ref| (1 + POW_REL).  Fields without a pow (casts, 1 - beta, lr wd, inv_scale =
                        f32(1 / f64(scale))) are computed exactly here and must be bit-equal.
    A1  AdamW element   bit for bit: clip = min(1, f32(max_norm / f32(norm + 1e-6f))) from info[0], then adamw1 in numpy float32 in its
                        order (decay, the lerp branch on w1 < 0.5, b2 v + (w2 g) g, sqrtf(v) inv_bc2_sqrt + eps, (step_size m) / denom).
    L1  LAMB moments    bit for bit: gfac = f32(f64(inv_scale) c1 / c2), c1, c2 in f64 from flags[0] as k_lamb_moments states them.
    L2  pn[b], un[b]    sum p^2, sum u^2 with u the exact f32 lamb_update of the kernel's new m, v and the old p: s(n) + u per square.
                        Chunks of a non-adapting group: the words are not written (U1).
    L3  trust ratio     per tensor from the kernel's pn / un added in ascending chunk order in f32 (the kernel's order: exact).  Owns a
                        chunk in which more than half of the moving elements disagree with L4's emulation (a wrong r moves every
                        element; anything less is L4's).
    L4  LAMB apply      bit for bit: p - f32(lr r) lamb_update(m, v, p) with the r of L3.
    S1  shadows         every shadow equals bf16_rne(the kernel's new p) bit for bit at its layout's offset: dense, [cols][rows],
                        nv.pack_fragments(p), nv.pack_fragments(p.t()).
    U1  untouched       every word of both arenas that no stage owns keeps its bits: guards around every tensor, the padding of the three
                        flat buffers, unowned workspace words, the gradient buffer, and on a skipped step p, m, v, shadows and steps.
    K1  bookkeeping     steps (every entry), scale, growth_tracker, info exactly as finish() states.
    R1  reduce_jobs     dst[c] = sum_p src[p stride + c] in float64 of the stored values; tier A (integers) exact, tier B s(parts) per
                        element against that column's own sum |terms|; transposed jobs at the transposed index; everything else untouched.

Memory model.  A case lives in two arenas (``Mem``: u32 words and u16 halves) pre-filled with the never-written patterns
gemm_ref.F32_NAN / BF16_NAN; every parameter, shadow, flat buffer, the workspace and the scalars are slices of them with guard words in
between, so U1 is ONE comparison of before and after outside the owned words.  The emulation and the GPU run mutate the same ``Mem``.

Assumptions, by name, and what would falsify each:
    POW_REL = 2^-20    the relative slack of D1 on top of the one f32 rounding, for the device's f64 pow (and the f64 divide and sqrt behind
                       it), whose accuracy nobody here has stated.  An error of k f64 ulp in pow(beta, t) is k 2^-53 / (1 - beta^t) relative
                       in a bias correction (k 2^-44 at beta = 0.999, t = 2, the worst of the cases) and moves the f32 result only if it
                       carries the value across a rounding boundary; 2^-24 2^-20 |ref| admits that for k of a few ulp and nothing coarser.
                       Falsified by a D1 failure on step_size / inv_bc2_sqrt / bc1 / bc2_sqrt alone, an ulp from the reference.
    IEEE_F32_DIV_SQRT  A1, L1..L4 rest on correctly rounded f32 division and sqrtf on the device (the file's comment claims "the IEEE
                       division and square-root sequences"; hipcc's default is correctly rounded).  L1's gfac also takes an f64 sqrt and
                       two f64 divisions as correctly rounded before its one rounding to f32 (IEEE_F64_DIV_SQRT, same standing).
                       Falsified by an exact rule failing only on elements one ulp off after a division or square root: then the ISA
                       decides between a build finding and a kernel bug.  No inexact fallback is in this module.
    NORMAL_RANGE       generators keep every intermediate of the emulations normal (``assert_normal``: min |nonzero| >= 2^-100, max <=
                       2^100); whether gfx950 keeps or flushes subnormal f32 intermediates is not decided here.  Cases that carry inf / NaN
                       on purpose (K1) are exempt.
Where the kernels and the reference optimisers differ on purpose the kernel is held to its own statement: LAMB's norm c1 in place of a
second pass over the clipped gradients, and an overflowing f32 sum of squares counting as found_inf although every gradient is finite.
"""
import decimal
import itertools

import numpy as np
import torch

import gemm_ref as gr

CHUNK, MAX_GROUPS = 2048, 4
U = 2.0 ** -24
POW_REL = 2.0 ** -20
F32_MAX = float(np.finfo(np.float32).max)
GUARD = 32
f4 = np.float32
ADAMW_FIELDS = ("step_size", "inv_bc2_sqrt", "lr_wd", "w1", "b2", "w2", "eps", "inv_scale")
LAMB_FIELDS = ("lr", "b1", "b3", "b2", "w2", "bc1", "bc2_sqrt", "eps", "wd", "inv_scale")


def _up(n, k):
    return (n + k - 1) // k * k


def s_bound(n, mag):
    """s(n) of the module docstring on numpy operands, through gemm_ref.bound."""
    return gr.bound(None, torch.as_tensor(np.asarray(mag, dtype=np.float64)), torch.as_tensor(np.asarray(n, dtype=np.float64)), half_ulp=False).numpy()


def _put(fig, key, ratio):
    if fig is not None:
        fig[key] = max(fig.get(key, 0.0), float(ratio))


# ------------------------------------------------------------------------------------------------------------------- memory
class Mem:
    def __init__(self, f_words, h_words):
        self.f = np.full(f_words, gr.F32_NAN, np.uint32)
        self.h = np.full(h_words, gr.BF16_NAN, np.uint16)

    @property
    def ff(self):
        return self.f.view(np.float32)

    def copy(self):
        m = Mem(0, 0)
        m.f, m.h = self.f.copy(), self.h.copy()
        return m


class Param:
    def __init__(self, shape, group):
        self.shape = tuple(shape)
        self.n = int(np.prod(shape))
        self.rows, self.cols = (shape[0], shape[1]) if len(shape) == 2 else (1, max(self.n, 1))
        self.group, self.skip = group, False
        self.off = self.flat = None
        self.sh = [None, None, None, None]  # dense, transposed, packed, packed transposed: offsets into Mem.h


class Layout:
    """specs: [(shape, kinds)]; kinds: d dense, t transposed, p packed, q packed transposed shadow at 16-byte alignment; D a dense shadow
    that is only 4-byte aligned (the uint2 store of refresh_shadow takes its element side), T a transposed one that is only 8-byte aligned
    (the tiled condition takes its scattered side).  Parameters are dealt round robin to ``n_groups`` groups; ``skip``: indices left
    out of the chunk table (a parameter without gradient)."""

    def __init__(self, specs, lamb, n_groups=MAX_GROUPS, skip=()):
        self.lamb, self.n_groups = lamb, n_groups
        self.params = [Param(s, i % n_groups) for i, (s, _) in enumerate(specs)]
        fc = hc = fl = 0

        def alloc_f(n):
            nonlocal fc
            off = fc + GUARD
            fc = off + _up(n, 4)
            return off

        for i, (p, (_, kinds)) in enumerate(zip(self.params, specs)):
            p.skip = i in skip
            p.off = alloc_f(p.n)
            p.flat = fl
            fl += _up(p.n, 4) + (4 if i % 2 else 0)  # padding elements between tensors, also after a multiple of 4
            for k in kinds:
                slot = "dtpq".index(k.lower())
                off = hc + GUARD + (2 if k == "D" else 4 if k == "T" else 0)
                hc = _up(off + p.n, 8)
                p.sh[slot] = off
        self.flat_len = fl
        self.grads, self.m, self.v = alloc_f(fl), alloc_f(fl), alloc_f(fl)
        self.chunks = [(i, c0, min(CHUNK, p.n - c0)) for i, p in enumerate(self.params) if not p.skip for c0 in range(0, p.n, CHUNK)]
        self.nc = len(self.chunks)
        self.nc4 = (self.nc + 3) & ~3
        self.ws_len = 3 * self.nc4 + 4 + MAX_GROUPS * 12 if lamb else self.nc4 + MAX_GROUPS * 8
        self.ws = alloc_f(self.ws_len)
        self.n_steps = len(self.params)
        self.steps, self.scale, self.tracker, self.info = alloc_f(self.n_steps), alloc_f(1), alloc_f(1), alloc_f(2)
        self.f_words, self.h_words = fc + GUARD, hc + GUARD
        # per element of the active parameters, in chunk order
        act = [p for p in self.params if not p.skip]
        self.idx_p = np.concatenate([p.off + np.arange(p.n) for p in act])
        self.idx_flat = np.concatenate([p.flat + np.arange(p.n) for p in act])
        self.gi = np.concatenate([np.full(p.n, p.group) for p in act])
        self.ci = np.concatenate([np.full(n, b) for b, (_, _, n) in enumerate(self.chunks)])
        self.chunk_group = np.array([self.params[i].group for i, _, _ in self.chunks])
        self.chunk_n = np.array([n for _, _, n in self.chunks])

    def mem(self):
        return Mem(self.f_words, self.h_words)


def read_adamw_ws(L, mem):
    """-> (partial [nc], {field: f32 [4]}) of g2048_opt_step's workspace: [nc4] partials, then Derived (8 f32) per group."""
    ws = mem.ff[L.ws:L.ws + L.ws_len]
    d = ws[L.nc4:L.nc4 + MAX_GROUPS * 8].reshape(MAX_GROUPS, 8)
    return ws[:L.nc].copy(), {k: d[:, j].copy() for j, k in enumerate(ADAMW_FIELDS)}


def read_lamb_ws(L, mem):
    """-> (partial, pn, un [nc], flags f32 [4], {field: [4]}) of g2048_lamb_step's workspace: [nc4] partials, [nc4] pn, [nc4] un, f32[4]
    flags, then LambDerived (48 bytes: 10 f32, adapt and trust_clip as int32) per group."""
    ws = mem.ff[L.ws:L.ws + L.ws_len]
    base = 3 * L.nc4 + 4
    d = ws[base:base + MAX_GROUPS * 12].reshape(MAX_GROUPS, 12)
    D = {k: d[:, j].copy() for j, k in enumerate(LAMB_FIELDS)}
    D["adapt"], D["trust_clip"] = d[:, 10].copy().view(np.int32), d[:, 11].copy().view(np.int32)
    return ws[:L.nc].copy(), ws[L.nc4:L.nc4 + L.nc].copy(), ws[2 * L.nc4:2 * L.nc4 + L.nc].copy(), ws[3 * L.nc4:3 * L.nc4 + 4].copy(), D


# ------------------------------------------------------------------------------------------------------------------- D1 references
def _bias_corrections(beta1, beta2, t):
    """(1 - beta1^t, 1 - beta2^t) at 60 digits from the exact f64 betas."""
    D = decimal.Decimal
    return 1 - D(float(beta1)) ** int(t), 1 - D(float(beta2)) ** int(t)


def adamw_derived_ref(group, t, scale):
    """{field: (float64 reference, exact?)} of Derived for group (lr, beta1, beta2, eps, wd) as f64, step t, f32 scale or None."""
    lr, b1, b2, eps, wd = (np.float64(x) for x in group)
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        bc1, bc2 = _bias_corrections(b1, b2, t)
        step_size = float(decimal.Decimal(float(lr)) / bc1) if bc1 != 0 else float("inf")
        inv_sqrt = float(1 / bc2.sqrt()) if bc2 != 0 else float("inf")
    inv_scale = f4(1.0) if scale is None else f4(np.float64(1.0) / np.float64(f4(scale)))
    return dict(step_size=(step_size, False), inv_bc2_sqrt=(inv_sqrt, False), lr_wd=(f4(lr * wd), True), w1=(f4(1.0 - b1), True), b2=(f4(b2), True),
                w2=(f4(1.0 - b2), True), eps=(f4(eps), True), inv_scale=(inv_scale, True))


def lamb_derived_ref(group, t, scale):
    lr, b1, b2, b3, eps, wd = (np.float64(x) for x in group[:6])
    bias_correction, adapt, trust_clip = (bool(x) for x in group[6:9])
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        bc1, bc2 = _bias_corrections(b1, b2, t)
        bc1, bc2s = float(bc1), float(bc2.sqrt())
    inv_scale = f4(1.0) if scale is None else f4(np.float64(1.0) / np.float64(f4(scale)))
    return dict(lr=(f4(lr), True), b1=(f4(b1), True), b3=(f4(b3), True), b2=(f4(b2), True), w2=(f4(1.0 - b2), True),
                bc1=(bc1, False) if bias_correction else (f4(1.0), True), bc2_sqrt=(bc2s, False) if bias_correction else (f4(1.0), True),
                eps=(f4(eps), True), wd=(f4(wd), True), inv_scale=(inv_scale, True), adapt=(int(adapt or wd != 0.0), True),
                trust_clip=(int(trust_clip), True))


def derived_check(D, refs):
    """D1.  D: {field: [4]} as read from the workspace; refs: one reference dict per group in use."""
    out = []
    for g, ref in enumerate(refs):
        for k, (want, exact) in ref.items():
            got = D[k][g]
            if exact:
                ok = got == want and np.signbit(got) == np.signbit(want)
            else:
                ok = abs(float(got) - want) <= U * abs(want) * (1 + POW_REL)
            if not ok:
                out.append(f"D1 {k} of group {g}: {got!r}, expected {want!r}" + ("" if exact else " within one f32 rounding (1 + POW_REL)"))
    return out


# ------------------------------------------------------------------------------------------------------------------- element arithmetic
def assert_normal(arrays):
    """NORMAL_RANGE of the module docstring on the emulation's intermediates."""
    for a in arrays:
        a = np.abs(np.asarray(a, dtype=np.float64)).reshape(-1)
        nz = a[a != 0]
        assert np.isfinite(a).all() and (nz.size == 0 or (nz.min() >= 2.0 ** -100 and nz.max() <= 2.0 ** 100)), \
            "generator precondition: an intermediate leaves the normal range [2^-100, 2^100]"


def clip_f32(norm, max_norm):
    """k_opt_adamw's clip factor from the f32 norm."""
    if not max_norm > 0:
        return f4(1.0)
    with np.errstate(all="ignore"):
        c = f4(max_norm) / (f4(norm) + f4(1e-6))
    return f4(1.0) if c > f4(1.0) else c


def adamw_elements(p, g, m, v, D, clip, keep=None):
    """adamw1 of the .hip file on f32 arrays, one IEEE rounding per operation; D: per-element f32 arrays of Derived."""
    one = f4(1.0)
    with np.errstate(all="ignore"):
        gp = (g * D["inv_scale"]) * clip
        dec = D["lr_wd"] * p
        p1 = p - dec
        d = gp - m
        a, b = D["w1"] * d, d * (one - D["w1"])
        m1 = np.where(D["w1"] < f4(0.5), m + a, gp - b)
        t1, t2 = D["b2"] * v, D["w2"] * gp
        t3 = t2 * gp
        v1 = t1 + t3
        sq = np.sqrt(v1)
        den0 = sq * D["inv_bc2_sqrt"]
        denom = den0 + D["eps"]
        num = D["step_size"] * m1
        q = num / denom
        p2 = p1 - q
    if keep is not None:
        keep += [gp, dec, p1, d, np.where(D["w1"] < f4(0.5), a, b), m1, t1, t2, t3, v1, sq, den0, denom, num, q, p2]
    return p2, m1, v1


def lamb_gfac(total, inv_scale, max_norm, lamb_max):
    """k_lamb_moments' one factor: f32(f64(inv_scale) c1 / c2) from the f32 total of the squares."""
    with np.errstate(all="ignore"):
        norm = np.sqrt(np.float64(total))
        c1 = c2 = np.float64(1.0)
        if max_norm > 0:
            c1 = min(np.float64(f4(max_norm)) / (norm + np.float64(1e-6)), np.float64(1.0)) if not np.isnan(norm) else np.float64("nan")
        if lamb_max > 0:
            c2 = (norm * c1) / np.float64(f4(lamb_max))
            if c2 < 1.0:
                c2 = np.float64(1.0)
        return f4(np.float64(inv_scale) * c1 / c2)


def lamb_moments_elements(g, m, v, D, gfac, keep=None):
    with np.errstate(all="ignore"):
        gp = g * gfac
        a, b = D["b1"] * m, D["b3"] * gp
        m1 = a + b
        t1, t2 = D["b2"] * v, D["w2"] * gp
        t3 = t2 * gp
        v1 = t1 + t3
    if keep is not None:
        keep += [gp, a, b, m1, t1, t2, t3, v1]
    return m1, v1


def lamb_update_elements(m, v, p, D, keep=None):
    with np.errstate(all="ignore"):
        sq = np.sqrt(v)
        d0 = sq / D["bc2_sqrt"]
        denom = d0 + D["eps"]
        q = m / denom
        u0 = q / D["bc1"]
        w = D["wd"] * p
        u = np.where(D["wd"] != 0, u0 + w, u0)
    if keep is not None:
        keep += [sq, d0, denom, q, u0, np.where(D["wd"] != 0, w, 0), u]
    return u


def bf16_bits(x):
    """f32 array -> bf16 bits, round to nearest even (NaN -> 0x7FC0)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    r[np.isnan(x)] = 0x7FC0
    return r


def _bf16_same(got, want):
    nan = lambda b: (b & 0x7FFF) > 0x7F80
    return (got == want) | (nan(got) & nan(want))


def _f32_same(got, want):
    """Bit equality of f32 arrays; a NaN matches any NaN."""
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


def _first(bad, got, want):
    i = np.flatnonzero(bad)
    return f"{i.size} of {bad.size} elements, first at {int(i[0])}: got {got.reshape(-1)[i[0]]!r}, want {want.reshape(-1)[i[0]]!r}"


# ------------------------------------------------------------------------------------------------------------------- shared stages
def _norm_stages(L, before, partial, inv_scale, total, info, has_scaler, fig, tier_a):
    """N1 and N2.  total: the kernel's f32 total (LAMB's flags[0]) or None (AdamW).  -> (failures, expected found_inf)."""
    out = []
    g = before.ff[L.grads + L.idx_flat]
    with np.errstate(all="ignore"):
        gs = g * f4(inv_scale)
        sq32 = gs * gs
        terms = gs.astype(np.float64) ** 2
    wild_el = ~np.isfinite(sq32)
    ref = np.bincount(L.ci, weights=np.where(wild_el, 0.0, terms), minlength=L.nc)
    wild = (np.bincount(L.ci, weights=wild_el, minlength=L.nc) > 0) | (ref > 0.99 * F32_MAX)
    bnd = s_bound(L.chunk_n, ref) + U * ref
    if tier_a:
        gr.assert_exact(torch.as_tensor(ref.sum()))
        assert not wild.any()
        bad = partial.astype(np.float64) != ref
        if bad.any():
            out.append("N1 partial (tier A): not exact in " + _first(bad, partial, ref))
    else:
        err = np.abs(partial.astype(np.float64) - ref)
        bad = ~wild & ~(err <= bnd)
        _put(fig, "N1 partial", np.max(np.where(~wild & (bnd > 0), err / np.maximum(bnd, 1e-300), 0.0)))
        if bad.any():
            out.append("N1 partial: beyond the bound in " + _first(bad, partial, ref))
    bad = wild & np.isfinite(partial)
    if bad.any():
        out.append("N1 partial: finite although the f32 squares of the chunk are not, in " + _first(bad, partial, ref))
    # N2 from the kernel's own partials
    pk = partial.astype(np.float64)
    finite = bool(np.isfinite(pk).all())
    tref = float(pk.sum()) if finite else float("nan")
    tb = float(s_bound(L.nc, np.abs(pk).sum())) if finite else 0.0
    must_overflow = (not finite) or tref - tb > F32_MAX
    may_overflow = must_overflow or tref + tb > F32_MAX
    info0 = f4(info[0])
    if total is not None:
        total = f4(total)
        with np.errstate(all="ignore"):
            want0 = np.sqrt(total)
        if not (_f32_same(np.array([info0]), np.array([want0]))[0]):
            out.append(f"N2 info[0]: {info0!r} is not sqrtf(flags[0]) = {want0!r}")
        cands = [total]
    else:
        with np.errstate(all="ignore"):
            c = info0 * info0
            cands = [c]
            for _ in range(4):
                cands = [np.nextafter(cands[0], f4(-np.inf))] + cands + [np.nextafter(cands[-1], f4(np.inf))]
            cands = [x for x in cands if _f32_same(np.array([np.sqrt(x)]), np.array([info0]))[0]]
    got_finite = bool(np.isfinite(info0))
    if must_overflow and got_finite:
        out.append(f"N2 total: finite ({info0!r}) although the partials are not finite or their sum overflows f32")
    elif not may_overflow:
        if not got_finite or not cands:
            out.append(f"N2 total: info[0] = {info0!r} for partials that sum to {tref!r}")
        elif tier_a:
            if not any(float(x) == tref for x in cands):
                out.append(f"N2 total (tier A): sqrt of {tref!r} expected, info[0] = {info0!r}")
        else:
            err = min(abs(float(x) - tref) for x in cands)
            _put(fig, "N2 total", err / tb if tb > 0 else 0.0)
            if not err <= tb:
                out.append(f"N2 total: {float(cands[0])!r} against {tref!r}, bound {tb!r}")
    found = has_scaler and not got_finite
    want1 = 1.0 if found else 0.0
    if float(info[1]) != want1:
        out.append(f"N2 info[1]: {info[1]!r}, expected {want1}")
    return out, found


def _shadow_stage(L, after):
    """S1: every shadow against bf16_rne of the kernel's own new parameter."""
    from src.g2048 import native as nv

    out = []
    for i, p in enumerate(L.params):
        if p.skip or not any(o is not None for o in p.sh):
            continue
        bits = bf16_bits(after.ff[p.off:p.off + p.n]).reshape(p.rows, p.cols)
        t = torch.from_numpy(bits.view(np.int16))
        want = (bits.reshape(-1), np.ascontiguousarray(bits.T).reshape(-1),
                nv.pack_fragments(t).numpy().view(np.uint16) if p.sh[2] is not None else None,
                nv.pack_fragments(t.t().contiguous()).numpy().view(np.uint16) if p.sh[3] is not None else None)
        for slot, name in enumerate(("dense", "transposed", "packed", "packed transposed")):
            if p.sh[slot] is None:
                continue
            got = after.h[p.sh[slot]:p.sh[slot] + p.n]
            bad = ~_bf16_same(got, want[slot])
            if bad.any():
                out.append(f"S1 {name} shadow of parameter {i} {p.shape}: " + _first(bad, got, want[slot]))
    return out


def _owned(L, taken, scaler, ws_words, lamb_pn_chunks=None):
    """-> (owned words of Mem.f, owned halves of Mem.h) of one step."""
    of, oh = np.zeros(L.f_words, bool), np.zeros(L.h_words, bool)
    of[L.ws + np.asarray(ws_words, dtype=np.int64)] = True
    of[L.info:L.info + 2] = True
    if scaler:
        of[L.scale] = of[L.tracker] = True
    if taken:
        of[L.steps:L.steps + L.n_steps] = True
        of[L.idx_p] = True
        of[L.m + L.idx_flat] = True
        of[L.v + L.idx_flat] = True
        for p in L.params:
            if not p.skip:
                for o in p.sh:
                    if o is not None:
                        oh[o:o + p.n] = True
    return of, oh


def _untouched_stage(before, after, of, oh):
    out = []
    bad = (before.f != after.f) & ~of
    if bad.any():
        out.append("U1 f32 arena: written outside the step's outputs: " + _first(bad, after.f, before.f))
    bad = (before.h != after.h) & ~oh
    if bad.any():
        out.append("U1 bf16 arena: written outside the step's outputs: " + _first(bad, after.h, before.h))
    return out


def _bookkeeping_stage(L, before, after, found, hp):
    """K1: finish() of the .hip file."""
    out = []
    want = before.ff[L.steps:L.steps + L.n_steps] + (f4(0.0) if found else f4(1.0))
    got = after.ff[L.steps:L.steps + L.n_steps]
    if not (got.view(np.uint32) == want.view(np.uint32)).all():
        out.append(f"K1 steps: {got.tolist()}, expected {want.tolist()}")
    sc = hp.get("scaler")
    if sc:
        s0, t0 = before.ff[L.scale], int(before.f.view(np.int32)[L.tracker])
        if found:
            s1, t1 = s0 * f4(sc["backoff"]), 0
        elif t0 + 1 == sc["interval"]:
            s1, t1 = s0 * f4(sc["growth"]), 0
        else:
            s1, t1 = s0, t0 + 1
        if after.ff[L.scale] != s1 or int(after.f.view(np.int32)[L.tracker]) != t1:
            out.append(f"K1 scaler: scale {after.ff[L.scale]!r} tracker {int(after.f.view(np.int32)[L.tracker])}, expected {s1!r} and {t1}")
    return out


def _per_element(D, gi, fields):
    return {k: D[k][gi] for k in fields}


# ------------------------------------------------------------------------------------------------------------------- AdamW
def adamw_check(L, before, after, hp, fig=None, tier_a=False, normal=True):
    """Every stage of one g2048_opt_step.  hp: dict(groups=[(lr, beta1, beta2, eps, wd)], max_norm, scaler=None or dict(growth, backoff,
    interval)).  -> list of messages, each starting with the stage that owns it."""
    out = []
    scaler = hp.get("scaler")
    partial, D = read_adamw_ws(L, after)
    info = after.ff[L.info:L.info + 2]
    scale = before.ff[L.scale] if scaler else None
    t = int(before.ff[L.steps]) + 1
    out += derived_check(D, [adamw_derived_ref(g, t, scale) for g in hp["groups"]])
    o, found = _norm_stages(L, before, partial, D["inv_scale"][0], None, info, bool(scaler), fig, tier_a)
    out += o
    ws_words = list(range(L.nc)) + list(range(L.nc4, L.nc4 + 8 * len(hp["groups"])))
    out += _untouched_stage(before, after, *_owned(L, not found, scaler, ws_words))
    out += _bookkeeping_stage(L, before, after, found, hp)
    if found:
        return out
    keep = [] if normal and not any(m.startswith("D1") for m in out) else None  # (a wrong Derived is D1's; its intermediates mean nothing)
    p2, m1, v1 = adamw_elements(before.ff[L.idx_p], before.ff[L.grads + L.idx_flat], before.ff[L.m + L.idx_flat], before.ff[L.v + L.idx_flat],
                                _per_element(D, L.gi, ADAMW_FIELDS), clip_f32(info[0], hp["max_norm"]), keep)
    if keep is not None:
        assert_normal(keep)
    for name, got, want in (("p", after.ff[L.idx_p], p2), ("exp_avg", after.ff[L.m + L.idx_flat], m1), ("exp_avg_sq", after.ff[L.v + L.idx_flat], v1)):
        bad = ~_f32_same(got, want)
        if bad.any():
            out.append(f"A1 {name}: not bit-equal to adamw1 in f32 in " + _first(bad, got, want))
    return out + _shadow_stage(L, after)


# ------------------------------------------------------------------------------------------------------------------- LAMB
def lamb_ratios(L, pn, un, D):
    """L3: the f32 trust ratio of every chunk's tensor from the kernel's own per-chunk sums, in ascending chunk order."""
    r = np.ones(L.nc, np.float32)
    b = 0
    for i, p in enumerate(L.params):
        if p.skip:
            continue
        count = (p.n + CHUNK - 1) // CHUNK
        if D["adapt"][p.group]:
            sp = su = f4(0.0)
            with np.errstate(all="ignore"):
                for k in range(b, b + count):
                    sp, su = sp + pn[k], su + un[k]
                wn, upd = np.sqrt(sp), np.sqrt(su)
                x = wn / upd if wn > 0 and upd > 0 else f4(1.0)
            if D["trust_clip"][p.group] and x > 1:
                x = f4(1.0)
            r[b:b + count] = x
        b += count
    return r


def lamb_check(L, before, after, hp, fig=None, tier_a=False, normal=True):
    """Every stage of one g2048_lamb_step.  hp: dict(groups=[(lr, b1, b2, b3, eps, wd, bias_correction, adapt, trust_clip)], max_norm,
    lamb_max, scaler)."""
    out = []
    scaler = hp.get("scaler")
    partial, pn, un, flags, D = read_lamb_ws(L, after)
    info = after.ff[L.info:L.info + 2]
    scale = before.ff[L.scale] if scaler else None
    t = int(before.ff[L.steps]) + 1
    out += derived_check(D, [lamb_derived_ref(g, t, scale) for g in hp["groups"]])
    o, found = _norm_stages(L, before, partial, D["inv_scale"][0], flags[0], info, bool(scaler), fig, tier_a)
    out += o
    if float(flags[1]) != (1.0 if found else 0.0):
        out.append(f"N2 flags[1]: {flags[1]!r}, expected {float(found)}")
    adapt_chunk = D["adapt"][L.chunk_group] != 0
    ng = len(hp["groups"])
    ws_words = list(range(L.nc)) + [3 * L.nc4, 3 * L.nc4 + 1] + list(range(3 * L.nc4 + 4, 3 * L.nc4 + 4 + 12 * ng))
    if not found:
        ws_words += (L.nc4 + np.flatnonzero(adapt_chunk)).tolist() + (2 * L.nc4 + np.flatnonzero(adapt_chunk)).tolist()
    out += _untouched_stage(before, after, *_owned(L, not found, scaler, ws_words))
    out += _bookkeeping_stage(L, before, after, found, hp)
    if found:
        return out
    De = _per_element(D, L.gi, LAMB_FIELDS)
    keep = [] if normal and not any(m.startswith("D1") for m in out) else None
    gfac = lamb_gfac(flags[0], D["inv_scale"][0], hp["max_norm"], hp.get("lamb_max") or 0.0)
    p0 = before.ff[L.idx_p]
    m1, v1 = lamb_moments_elements(before.ff[L.grads + L.idx_flat], before.ff[L.m + L.idx_flat], before.ff[L.v + L.idx_flat], De, gfac, keep)
    mk, vk = after.ff[L.m + L.idx_flat], after.ff[L.v + L.idx_flat]
    for name, got, want in (("exp_avg", mk, m1), ("exp_avg_sq", vk, v1)):
        bad = ~_f32_same(got, want)
        if bad.any():
            out.append(f"L1 {name}: not bit-equal to lamb_moments1 in f32 in " + _first(bad, got, want))
    u = lamb_update_elements(mk, vk, p0, De, keep)  # from the kernel's own moments
    if keep is not None:
        assert_normal(keep)
    for name, got, x in (("pn", pn, p0), ("un", un, u)):
        sq = x.astype(np.float64) ** 2
        ref = np.bincount(L.ci, weights=sq, minlength=L.nc)
        bnd = s_bound(L.chunk_n, ref) + U * ref
        err = np.where(adapt_chunk, np.abs(got.astype(np.float64) - ref), 0.0)
        ok = np.isfinite(ref)
        _put(fig, f"L2 {name}", np.max(np.where(ok & (bnd > 0), err / np.maximum(bnd, 1e-300), 0.0), initial=0.0))
        bad = adapt_chunk & ok & ~(err <= bnd)
        if bad.any():
            out.append(f"L2 {name}: beyond the bound in " + _first(bad, got, ref))
    r = lamb_ratios(L, pn, un, D)
    with np.errstate(all="ignore"):
        step = De["lr"] * r[L.ci]
        su = step * u
        p1 = p0 - su
    got = after.ff[L.idx_p]
    bad = ~_f32_same(got, p1)
    if bad.any():
        moving = su != 0
        share = np.bincount(L.ci, weights=bad & moving, minlength=L.nc) / np.maximum(np.bincount(L.ci, weights=moving, minlength=L.nc), 1)
        l3 = (share > 0.5) & adapt_chunk
        if l3.any():
            out.append(f"L3 trust ratio: chunks {np.flatnonzero(l3).tolist()[:8]} did not use r of their tensor's own pn / un ({r[l3][:4].tolist()})")
        rest = bad & ~l3[L.ci]
        if rest.any():
            out.append("L4 p: not bit-equal to p - f32(lr r) lamb_update in " + _first(rest, got, p1))
    return out + _shadow_stage(L, after)


# ------------------------------------------------------------------------------------------------------------------- cases
def _kinds(specs):
    return [(tuple(s), k) for s, k in specs]


SMALL = _kinds([((64, 256), "dtpq"), ((32, 512), "dtpq"), ((32, 1024), "dtpq"), ((4, 512), "dt"), ((1, 512), "dt"), ((64, 128), "dtp"),
                ((32, 2048), "dt"), ((12, 256), "dt"), ((41, 300), "dt"), ((7, 3), "d"), ((1,), "d"), ((41,), "d"), ((2050,), "d"),
                ((2051,), "d"), ((16, 512), "DT")])
BIG = SMALL + [((CHUNK * 260,), "")]
ADAMW_GROUPS = [(4e-4, 0.9, 0.999, 1e-6, 0.01), (1e-3, 0.3, 0.99, 1e-8, 0.0), (2e-4, 0.8, 0.95, 1e-7, 0.1), (3e-3, 0.95, 0.9995, 1e-5, 0.05)]
# (lr, beta1, beta2, beta3, eps, wd, bias_correction, adapt, trust_clip): adapting through the decay; not adapting, no grad averaging;
# adapting through the flag, no bias correction, trust clip; adapting with trust clip
LAMB_GROUPS = [(4e-4, 0.9, 0.999, 0.1, 1e-6, 0.01, 1, 0, 0), (1e-3, 0.3, 0.99, 1.0, 1e-8, 0.0, 1, 0, 0), (2e-4, 0.8, 0.95, 0.2, 1e-7, 0.0, 0, 1, 1),
               (3e-3, 0.95, 0.9995, 0.05, 1e-5, 0.05, 1, 0, 1)]
SCALER = dict(growth=2.0, backoff=0.5, interval=2000)


def case(id, specs=SMALL, tier="B", scale=1024.0, max_norm=0.5, lamb_max=1.0, norms=(0.3, 5.0, 0.7), skip=(), t0=0, n_groups=4, zero=False):
    return dict(id=id, specs=specs, tier=tier, scale=scale, max_norm=max_norm, lamb_max=lamb_max, norms=norms, skip=skip, t0=t0,
                n_groups=n_groups, zero=zero)


def _one(n):
    return [((n,), "")]


# three steps each: trainer clip not binding / binding / binding (0.5), off (0); LAMB's own clip binds when the trainer's is off or wide
CASES = [
    case("scale1024_clip0.5"),
    case("noscaler_clipoff", scale=None, max_norm=0.0, norms=(0.3, 5.0, 2.0)),
    case("scale2^60_clip4", scale=2.0 ** 60, max_norm=4.0, norms=(2.0, 9.0, 0.4)),
    case("scale2^-10_nolambclip", scale=2.0 ** -10, lamb_max=0.0),
    case("scale1000", scale=1000.0, norms=(5.0, 0.3, 5.0)),
    case("tierA_clipoff", tier="A", max_norm=0.0),
    case("tierA_clip0.5", tier="A", scale=1.0),
    case("skip_middle", skip=(2, 8)),
    case("zero_gradients", zero=True, norms=(0.0,)),
    case("t5000", t0=4999, norms=(0.3,)),
    case("one_group", n_groups=1, norms=(5.0, 0.3)),
    case("big_tierB", specs=BIG),
    case("big_tierA", specs=BIG, tier="A", norms=(0.0, 0.0)),
    case("chunks1", specs=_one(CHUNK), n_groups=1),
    case("chunks255", specs=_one(CHUNK * 254 + 5), n_groups=1, norms=(0.3, 5.0)),
    case("chunks256_tierA", specs=_one(CHUNK * 256), n_groups=1, tier="A", norms=(0.0, 0.0)),
    case("chunks257", specs=_one(CHUNK * 256 + 1), n_groups=1, norms=(5.0, 0.3)),
]


def hyper(c, lamb):
    groups = (LAMB_GROUPS if lamb else ADAMW_GROUPS)[:c["n_groups"]]
    return dict(groups=groups, max_norm=c["max_norm"], lamb_max=c["lamb_max"], scaler=dict(SCALER) if c["scale"] is not None else None)


def init_state(L, mem, c, seed=1):
    """Fresh state: parameters randn at 0.1 (every third tensor at 3: a trust ratio above 1), moments 0, steps t0, scaler scalars."""
    rng = np.random.default_rng(seed)
    for i, p in enumerate(L.params):
        mem.ff[p.off:p.off + p.n] = rng.standard_normal(p.n).astype(np.float32) * f4(3.0 if i % 3 == 2 else 0.1)
        if not p.skip:
            mem.ff[L.m + p.flat:L.m + p.flat + p.n] = 0
            mem.ff[L.v + p.flat:L.v + p.flat + p.n] = 0
    mem.ff[L.steps:L.steps + L.n_steps] = f4(c["t0"])
    if c["scale"] is not None:
        mem.ff[L.scale] = f4(c["scale"])
        mem.f.view(np.int32)[L.tracker] = 0


def set_grads(L, mem, c, step, seed=2):
    """The gradient buffer of step ``step``, loss-scaled.  Tier B: normal at the norm of c["norms"]; tier A: integers in [-3, 3] (norm
    ~ 2 sqrt(N)).  A skipped tensor's slice holds NaN."""
    rng = np.random.default_rng(seed * 1000 + step)
    n_act = len(L.idx_p)
    scale = f4(1.0 if c["scale"] is None else c["scale"])
    for p in L.params:
        sl = slice(L.grads + p.flat, L.grads + p.flat + p.n)
        if p.skip:
            mem.ff[sl] = np.nan
        elif c["zero"]:
            mem.ff[sl] = 0
        elif c["tier"] == "A":
            assert float(np.log2(scale)).is_integer()
            mem.ff[sl] = rng.integers(-3, 4, p.n).astype(np.float32) * scale
        else:
            norm = c["norms"][step % len(c["norms"])]
            mem.ff[sl] = (rng.standard_normal(p.n) * (norm / n_act ** 0.5)).astype(np.float32) * scale


def run_case(c, lamb, step_fn, fig=None, steps=None, state=None, **kw):
    """Build the case, run ``step_fn(L, mem, hp)`` (which mutates ``mem`` as one optimiser step does) for each step and check every stage
    of every step.  -> failures; ``state`` (a dict) receives the layout, the initial and the final memory."""
    L = Layout(c["specs"], lamb, c["n_groups"], c["skip"])
    mem, hp = L.mem(), hyper(c, lamb)
    init_state(L, mem, c)
    if state is not None:
        state.update(L=L, start=mem.copy(), end=mem)
    out = []
    for s in range(len(c["norms"]) if steps is None else steps):
        set_grads(L, mem, c, s)
        before = mem.copy()
        step_fn(L, mem, hp, **kw)
        assert (before.f[L.grads:L.grads + L.flat_len] == mem.f[L.grads:L.grads + L.flat_len]).all(), "U1 the gradient buffer was written"
        got = (lamb_check if lamb else adamw_check)(L, before, mem, hp, fig, c["tier"] == "A")
        out += [f"{m}  [step {s}]" for m in got]
    return out


def zero_gradient_check(state, groups):
    """The all-zero-gradient step on fresh state, stated without the emulation: AdamW leaves m = v = 0 and moves p by the decay only."""
    L, a, b = state["L"], state["start"], state["end"]
    out = []
    if b.ff[L.m + L.idx_flat].any() or b.ff[L.v + L.idx_flat].any():
        out.append("A1 moments: not zero after a zero gradient on fresh state")
    p0 = a.ff[L.idx_p]
    want = p0 - np.array([f4(np.float64(g[0]) * np.float64(g[4])) for g in groups], np.float32)[L.gi] * p0
    bad = b.ff[L.idx_p].view(np.uint32) != want.view(np.uint32)
    if bad.any():
        out.append("A1 p: moved by more than the decay on a zero gradient in " + _first(bad, b.ff[L.idx_p], want))
    return out


SEQ_SPECS = SMALL + [((7,), "d")]  # the last chunk has a scalar tail (elements 4..6)
SEQ_EVENTS = ("clean", "clean", "growth", "inf", "nan_tail", "overflow", "clean")
SEQ_SCALE = (1024.0, 1024.0, 2048.0, 1024.0, 512.0, 256.0, 256.0)  # after each event, growth_interval 3
SEQ_TRACKER = (1, 2, 0, 0, 0, 0, 1)


def run_scaler_sequence(lamb, step_fn, fig=None, events=SEQ_EVENTS, **kw):
    """K1: clean x (interval - 1), clean -> growth, inf -> backoff and tracker reset, NaN in the scalar tail of the last chunk, finite
    gradients whose squares overflow the f32 sum (a skipped step by this kernel's rule), clean.  Every step through every stage; the
    scaler's trace is asserted against SEQ_SCALE / SEQ_TRACKER as well.  -> failures."""
    c = case("k1", specs=SEQ_SPECS, norms=(0.3,))
    L = Layout(c["specs"], lamb)
    mem, hp = L.mem(), hyper(c, lamb)
    hp["scaler"]["interval"] = 3
    init_state(L, mem, c)
    out = []
    last = L.params[-1]
    for s, ev in enumerate(events):
        set_grads(L, mem, dict(c, scale=float(mem.ff[L.scale])), s)
        g = mem.ff[L.grads:L.grads + L.flat_len]
        if ev == "inf":
            g[L.params[2].flat + 4097] = np.inf
        elif ev == "nan_tail":
            g[last.flat + last.n - 1] = np.nan
        elif ev == "overflow":
            g[L.params[6].flat + 2048 * 3 + 8:L.params[6].flat + 2048 * 3 + 16] = f4(1.5e19) * mem.ff[L.scale]  # 8 squares of 2.25e38 in one chunk
        before = mem.copy()
        step_fn(L, mem, hp, **kw)
        wild = ev in ("inf", "nan_tail", "overflow")
        got = (lamb_check if lamb else adamw_check)(L, before, mem, hp, fig, False, normal=not wild)
        out += [f"{m}  [{ev}, step {s}]" for m in got]
        if float(mem.ff[L.info + 1]) != float(wild):
            out.append(f"K1 found_inf after {ev!r} (step {s}): info[1] = {mem.ff[L.info + 1]!r}")
        if float(mem.ff[L.scale]) != SEQ_SCALE[s] or int(mem.f.view(np.int32)[L.tracker]) != SEQ_TRACKER[s]:
            out.append(f"K1 scaler after {ev!r} (step {s}): scale {mem.ff[L.scale]!r}, tracker {int(mem.f.view(np.int32)[L.tracker])}")
    done = sum(e in ("clean", "growth") for e in events)
    if not (mem.ff[L.steps:L.steps + L.n_steps] == done).all():
        out.append(f"K1 steps: {mem.ff[L.steps:L.steps + L.n_steps].tolist()} after {done} steps taken")
    return out


def run_nan_without_scaler(lamb, step_fn, **kw):
    """No scaler and a NaN gradient: the step is taken (torch steps anyway), and the result is NaN where the emulation is NaN: with a
    clip every element (the factor is NaN), without one the element itself (AdamW) or every element (LAMB's gfac comes from the norm)."""
    out = []
    for max_norm in (0.5, 0.0):
        c = case("nan", scale=None, max_norm=max_norm, norms=(0.3,))
        L = Layout(c["specs"], lamb)
        mem, hp = L.mem(), hyper(c, lamb)
        init_state(L, mem, c)
        set_grads(L, mem, c, 0)
        mem.ff[L.grads + L.params[8].flat + 301] = np.nan
        before = mem.copy()
        step_fn(L, mem, hp, **kw)
        out += [f"{m}  [max_norm {max_norm}]" for m in (lamb_check if lamb else adamw_check)(L, before, mem, hp, None, False, normal=False)]
        nans = int(np.isnan(mem.ff[L.idx_p]).sum())
        want = len(L.idx_p) if (max_norm > 0 or lamb) else 1
        if nans != want or float(mem.ff[L.steps]) != 1.0 or float(mem.ff[L.info + 1]) != 0.0:
            out.append(f"K1 NaN without a scaler (max_norm {max_norm}): {nans} NaN parameters (expected {want}), steps {mem.ff[L.steps]!r}, info[1] {mem.ff[L.info + 1]!r}")
    return out


# ------------------------------------------------------------------------------------------------------------------- reduce_jobs
R_PARTS = (1, 3, 4, 5, 8, 9, 31, 32, 33, 100)
R_NS = (1, 3, 6, 8, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 2056)
R_WIDE_MAX_PARTS = 32


def reduce_jobs_problem(tier_a, seed=5):
    """-> (Mem, jobs): every (parts, n) of R_PARTS x R_NS once, cycling bf16 / f32 sources, contiguous sources and column blocks of a wider
    matrix (the gap keeps the NaN pattern), sources at 16-, 8-, 4- and 2-byte alignment (f32: 16, 8, 4), destinations at 16 and 4; then
    the named jobs: wide8's own shape over two workgroups, part_stride % 8 != 0 with n % 8 == 0, transposed (31, 256), (4, 8), (5, 7)
    with few and with many parts.  A job: dict(kind, src, dst, stride, n, parts, tr), offsets in elements of Mem.h / Mem.f."""
    rng = np.random.default_rng(seed)
    todo = []
    for k, (parts, n) in enumerate(itertools.product(R_PARTS, R_NS)):
        kind = "bf16" if k % 2 == 0 else "f32"
        pad = (0, 8, 0, 3, 0, 4, 0, 16)[(k // 2) % 8]
        al = (k // 4) % (4 if kind == "bf16" else 3)
        todo.append((kind, n, parts, n + pad, al, (k // 3) % 2, 0))
    todo += [("bf16", 4096 + 8, 16, 4096 + 8, 0, 0, 0), ("bf16", 2048, 8, 2052, 0, 0, 0), ("bf16", 2048, 8, 2050, 0, 0, 0), ("f32", 1024, 4, 1030, 0, 0, 0)]
    for R, cols in ((31, 256), (4, 8), (5, 7)):
        for parts, kind in ((4, "f32"), (32, "bf16"), (40, "f32"), (1, "bf16")):
            todo.append((kind, R * cols, parts, R * cols + (0 if parts % 2 else 4), 0, parts % 2, R))
    fc = hc = 0
    jobs = []
    for kind, n, parts, stride, al, dal, tr in todo:
        size = (parts - 1) * stride + n
        if kind == "bf16":
            src = _up(hc + GUARD, 8) + (0, 4, 2, 1)[al]
            hc = src + size
        else:
            src = _up(fc + GUARD, 4) + (0, 2, 1)[al]
            fc = src + size
        dst = _up(fc + GUARD, 4) + dal
        fc = dst + n
        jobs.append(dict(kind=kind, src=src, dst=dst, stride=stride, n=n, parts=parts, tr=tr))
    mem = Mem(fc + GUARD, hc + GUARD)
    for J in jobs:
        shape = (J["parts"], J["n"])
        if tier_a:
            vals = rng.integers(-8, 9, shape).astype(np.float32)
        else:
            vals = (rng.standard_normal(shape) * np.exp2(rng.integers(-6, 4, (J["parts"], 1))) + 0.3).astype(np.float32)
        idx = J["src"] + np.arange(J["parts"])[:, None] * J["stride"] + np.arange(J["n"])[None, :]
        if J["kind"] == "bf16":
            mem.h[idx] = bf16_bits(vals.reshape(-1)).reshape(shape)
        else:
            mem.ff[idx] = vals
    return mem, jobs


def job_source(mem, J):
    """[parts][n] float64 of the stored values."""
    idx = J["src"] + np.arange(J["parts"])[:, None] * J["stride"] + np.arange(J["n"])[None, :]
    if J["kind"] == "bf16":
        return (mem.h[idx].astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return mem.ff[idx].astype(np.float64)


def dst_index(J):
    c = np.arange(J["n"])
    if J["tr"]:
        cols = J["n"] // J["tr"]
        return (c % cols) * J["tr"] + c // cols
    return c


def reduce_check(before, after, jobs, tier_a, fig=None):
    """R1 and U1 of one g2048_reduce_jobs call."""
    out = []
    of = np.zeros(before.f.size, bool)
    worst = 0.0
    for j, J in enumerate(jobs):
        src = job_source(before, J)
        ref, mag = src.sum(0), np.abs(src).sum(0)
        got = after.ff[J["dst"] + dst_index(J)]
        of[J["dst"]:J["dst"] + J["n"]] = True
        what = f"job {j} ({J['kind']}, parts {J['parts']}, n {J['n']}, stride {J['stride']}, transpose_rows {J['tr']})"
        if tier_a:
            gr.assert_exact(torch.as_tensor(mag))
            bad = got.astype(np.float64) != ref
            if bad.any():
                out.append(f"R1 {what} (tier A): not exact in " + _first(bad, got, ref))
        else:
            bnd = s_bound(J["parts"], mag)
            err = np.abs(got.astype(np.float64) - ref)
            worst = max(worst, float(np.max(np.where(bnd > 0, err / np.maximum(bnd, 1e-300), 0.0))))
            bad = ~(err <= bnd)
            if bad.any():
                out.append(f"R1 {what}: beyond its column's bound in " + _first(bad, got, ref))
    if not tier_a:
        _put(fig, "R1 dst", worst)
    bad = (before.f != after.f) & ~of
    if bad.any():
        out.append("U1 f32 arena: written outside the destinations: " + _first(bad, after.f, before.f))
    if (before.h != after.h).any():
        out.append("U1 bf16 arena: a source was written")
    return out
