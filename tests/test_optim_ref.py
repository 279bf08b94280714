"""tests/optim_ref.py held to itself on the CPU: an f32 emulation of g2048_opt_step, g2048_lamb_step and g2048_reduce_jobs as their
source states them (the chunk walk, block_sum's order, the strided sum of the partials, the tiled and scattered shadow writes as index
arithmetic on the same memory model, the three reduce shapes) must pass every rule at every case of tests/test_gpu_optim_f64.py, and every
planted defect must be rejected by the stage that owns it.  The float64 statement itself is held to torch.optim.AdamW and src.optim.Lamb
run in float64 for three steps.
"""
import numpy as np
import pytest
import torch

import optim_ref as orf

f4 = np.float32
CHUNK = orf.CHUNK


def _owners(failures):
    return {m.split(" ")[0] for m in failures}


# ------------------------------------------------------------------------------------------------------------------- emulation
def block_sum(s):
    """[256] per-thread values -> the f32 every thread of block_sum ends with: __shfl_down tree per wave, then the four waves in order."""
    w = s.reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w[:, :o] + w[:, o:2 * o]
    t = f4(0.0)
    for i in range(4):
        t = t + w[i, 0]
    return t


def chunk_sum(sq):
    """Sum of a chunk's f32 squares: thread t takes elements 4t.. of every 1024-element pass, a whole float4 as s += ((x + y) + z) + w, the
    ragged tail element by element."""
    n = len(sq)
    pad = np.zeros(CHUNK, np.float32)
    pad[:n] = sq
    q = pad.reshape(CHUNK // 1024, 256, 4)
    s = np.zeros(256, np.float32)
    for k in range(q.shape[0]):
        full = k * 1024 + 4 * np.arange(256) + 4 <= n
        a = s + (((q[k, :, 0] + q[k, :, 1]) + q[k, :, 2]) + q[k, :, 3])
        b = (((s + q[k, :, 0]) + q[k, :, 1]) + q[k, :, 2]) + q[k, :, 3]
        s = np.where(full, a, b)
    return block_sum(s)


def strided_total(partial):
    pad = np.zeros(orf._up(len(partial), 256), np.float32)
    pad[:len(partial)] = partial
    s = np.zeros(256, np.float32)
    for row in pad.reshape(-1, 256):
        s = s + row
    return block_sum(s)


def packed_off(row, col, cols):
    return ((((row >> 5) * (cols >> 4) + (col >> 4)) * 2 + ((col >> 3) & 1)) * 32 + (row & 31)) * 8 + (col & 7)


def _inv_scale(L, mem, hp):
    return f4(np.float64(1.0) / np.float64(mem.ff[L.scale])) if hp.get("scaler") else f4(1.0)


def emu_sqnorm(L, mem, inv_scale):
    with np.errstate(all="ignore"):
        for b, (i, c0, n) in enumerate(L.chunks):
            g = mem.ff[L.grads + L.params[i].flat + c0:][:n] * inv_scale
            mem.ff[L.ws + b] = chunk_sum(g * g)
        return strided_total(mem.ff[L.ws:L.ws + L.nc])


def emu_finish(L, mem, hp, total, found, defect):
    if not found:
        mem.ff[L.steps:L.steps + L.n_steps] += f4(1.0)
    with np.errstate(all="ignore"):
        mem.ff[L.info] = np.sqrt(total)
    mem.ff[L.info + 1] = 1.0 if found else 0.0
    sc = hp.get("scaler")
    if sc:
        tr = mem.f.view(np.int32)
        if found:
            mem.ff[L.scale] *= f4(sc["backoff"])
            tr[L.tracker] = 0
        else:
            ok = tr[L.tracker] + 1
            if ok == sc["interval"] + (defect == "growth_late"):
                mem.ff[L.scale] *= f4(sc["growth"])
                tr[L.tracker] = 0
            else:
                tr[L.tracker] = ok


def emu_shadows(L, mem, p, c0, n, newp, defect, first_chunk):
    """refresh_shadow and the tiled write-out of one chunk, as index arithmetic on Mem.h (addresses: the arena is 256-byte aligned)."""
    bits = orf.bf16_bits(newp) if defect != "trunc" else (np.ascontiguousarray(newp).view(np.uint32) >> 16).astype(np.uint16)
    sh, sh_t, sh_p, sh_tp = p.sh
    rows, cols = p.rows, p.cols
    any_t = sh_t is not None or sh_tp is not None
    R = CHUNK // cols if any_t and cols > 0 else 0
    tiled = (any_t and n == CHUNK and CHUNK % cols == 0 and c0 % cols == 0 and R in (2, 4, 8) and rows % R == 0
             and not (((sh_t or 0) * 2 | (sh_tp or 0) * 2) & 15))
    e = c0 + np.arange(n)
    r, col = e // cols, e % cols
    if sh is not None:
        mem.h[sh + e] = bits  # (the uint2 store of an 8-byte aligned address and the element stores write the same halves)
    if sh_p is not None:
        mem.h[sh_p + packed_off(r, col, cols)] = bits
    if not tiled:
        if sh_t is not None:
            mem.h[sh_t + (e if defect == "t_rowcol" and first_chunk else col * rows + r)] = bits
        if sh_tp is not None:
            mem.h[sh_tp + (packed_off(col, r, cols) % p.n if defect == "tp_cols" else packed_off(col, r, rows))] = bits
        return
    stage = bits  # LDS
    r0 = c0 // cols + (defect == "tiled_r0")
    cc = np.arange(cols)
    for j in range(R):  # the run of R consecutive rows of one column
        if sh_t is not None:
            mem.h[sh_t + cc * rows + r0 + j] = stage[j * cols + cc]
        if sh_tp is not None:
            mem.h[sh_tp + (packed_off(cc, r0, cols) % p.n if defect == "tp_cols" else packed_off(cc, r0, rows)) + j] = stage[j * cols + cc]


def emu_adamw(L, mem, hp, defect=None):
    ff = mem.ff
    t = np.float64(ff[L.steps]) + (0.0 if defect == "bc_t" else 1.0)
    inv_scale = _inv_scale(L, mem, hp)
    D = []
    with np.errstate(all="ignore"):
        for g, G in enumerate(hp["groups"]):
            lr, b1, b2, eps, wd = (np.float64(x) for x in G)
            bc1, bc2 = 1.0 - np.power(b1, t), 1.0 - np.power(b2, t)
            d = [f4(lr / bc1), f4(1.0 / np.sqrt(bc2)), f4(lr * wd), f4(1.0 - b1), f4(b2), f4(1.0 - b2), f4(eps), inv_scale]
            D.append(d)
            ff[L.ws + L.nc4 + 8 * g:L.ws + L.nc4 + 8 * g + 8] = d
        total = emu_sqnorm(L, mem, inv_scale)
        norm = np.sqrt(total)
        clip = f4(1.0)
        if hp["max_norm"] > 0:
            clip = f4(hp["max_norm"]) / (norm if defect == "no_1e6" else norm + f4(1e-6))
            if clip > 1:
                clip = f4(1.0)
        found = bool(hp.get("scaler")) and not abs(total) <= orf.F32_MAX
        emu_finish(L, mem, hp, total, found, defect)
        if defect == "pad_write":
            ff[L.m + L.params[1].flat + orf._up(L.params[1].n, 4)] = 0.0
        if found and defect != "moments_on_skip":
            return
        for b, (i, c0, n) in enumerate(L.chunks):
            P = L.params[i]
            step_size, inv_bc2_sqrt, lr_wd, w1, b2, w2, eps, _ = D[P.group]
            ps, fs = slice(P.off + c0, P.off + c0 + n), P.flat + c0
            p, g, m, v = ff[ps], ff[L.grads + fs:][:n], ff[L.m + fs:][:n], ff[L.v + fs:][:n]
            g = (g * clip) * inv_scale if defect == "clip_first" else (g * inv_scale) * clip
            if defect != "decay_after":
                p = p - lr_wd * p
            d = g - m
            m = m + w1 * d if (w1 < 0.5 or defect == "lerp_first") else g - d * (f4(1.0) - w1)
            v = b2 * v + (w2 * g) * g
            if defect == "eps_in_sqrt":
                denom = np.sqrt(v + eps) * inv_bc2_sqrt
            elif defect == "no_bc2":
                denom = np.sqrt(v) + eps
            else:
                denom = np.sqrt(v) * inv_bc2_sqrt + eps
            p = p - (step_size * m) / denom
            if defect == "decay_after":
                p = p - lr_wd * p
            ff[L.m + fs:][:n], ff[L.v + fs:][:n] = m, v
            if found:  # (moments_on_skip)
                continue
            ff[ps] = p
            emu_shadows(L, mem, P, c0, n, p, defect, c0 == 0 and i == 8)


def emu_lamb(L, mem, hp, defect=None):
    ff = mem.ff
    t = np.float64(ff[L.steps]) + 1.0
    inv_scale = _inv_scale(L, mem, hp)
    base = L.ws + 3 * L.nc4 + 4
    D = []
    with np.errstate(all="ignore"):
        for g, G in enumerate(hp["groups"]):
            lr, b1, b2, b3, eps, wd = (np.float64(x) for x in G[:6])
            bc, adapt, trust = G[6:9]
            d = dict(lr=f4(lr), b1=f4(b1), b3=f4(b3), b2=f4(b2), w2=f4(1.0 - b2), bc1=f4(1.0 - np.power(b1, t)) if bc else f4(1.0),
                     bc2_sqrt=f4(np.sqrt(1.0 - np.power(b2, t))) if bc else f4(1.0), eps=f4(eps), wd=f4(wd), inv_scale=inv_scale)
            ff[base + 12 * g:base + 12 * g + 10] = [d[k] for k in orf.LAMB_FIELDS]
            d["adapt"], d["trust_clip"] = int(bool(adapt) or wd != 0.0), int(bool(trust))
            mem.f.view(np.int32)[base + 12 * g + 10:base + 12 * g + 12] = [d["adapt"], d["trust_clip"]]
            D.append(d)
        total = emu_sqnorm(L, mem, inv_scale)
        found = bool(hp.get("scaler")) and not abs(total) <= orf.F32_MAX
        ff[L.ws + 3 * L.nc4], ff[L.ws + 3 * L.nc4 + 1] = total, 1.0 if found else 0.0
        emu_finish(L, mem, hp, total, found, defect)
        if found:
            return
        gfac = orf.lamb_gfac(total, inv_scale, hp["max_norm"], hp.get("lamb_max") or 0.0)

        def update(m, v, p, d):
            denom = np.sqrt(v) / d["bc2_sqrt"] + d["eps"]
            u = (m / denom) / d["bc1"]
            return u + d["wd"] * p if d["wd"] != 0 else u

        for b, (i, c0, n) in enumerate(L.chunks):  # k_lamb_moments
            P, d = L.params[i], D[L.params[i].group]
            fs = P.flat + c0
            g = ff[L.grads + fs:][:n] * gfac
            m = d["b1"] * ff[L.m + fs:][:n] + d["b3"] * g
            v = d["b2"] * ff[L.v + fs:][:n] + (d["w2"] * g) * g
            ff[L.m + fs:][:n], ff[L.v + fs:][:n] = m, v
            if d["adapt"]:
                p = ff[P.off + c0:P.off + c0 + n]
                u = update(m, v, p, d)
                ff[L.ws + L.nc4 + b], ff[L.ws + 2 * L.nc4 + b] = chunk_sum(p * p), chunk_sum(u * u)
        pn, un = ff[L.ws + L.nc4:][:L.nc].copy(), ff[L.ws + 2 * L.nc4:][:L.nc].copy()
        for b, (i, c0, n) in enumerate(L.chunks):  # k_lamb_apply
            P, d = L.params[i], D[L.params[i].group]
            r = f4(1.0)
            if d["adapt"]:
                first = max(b - c0 // CHUNK, 0)
                count = (P.rows * P.cols + CHUNK - 1) // CHUNK
                if defect == "count_off":
                    count = P.rows * P.cols // CHUNK + 1
                if defect == "r_whole_table":
                    first, count = 0, L.nc
                count = min(count, L.nc - first)
                sp = su = f4(0.0)
                for k in range(first, first + count):
                    sp, su = sp + pn[k], su + un[k]
                wn, upd = np.sqrt(sp), np.sqrt(su)
                if wn > 0 and upd > 0:
                    r = wn / upd
                if d["trust_clip"] and r > 1:
                    r = f4(1.0)
            step = d["lr"] * r
            fs = P.flat + c0
            p = ff[P.off + c0:P.off + c0 + n]
            p = p - step * update(ff[L.m + fs:][:n], ff[L.v + fs:][:n], p, d)
            ff[P.off + c0:P.off + c0 + n] = p
            emu_shadows(L, mem, P, c0, n, p, defect, False)


def emu_step(L, mem, hp, defect=None):
    (emu_lamb if L.lamb else emu_adamw)(L, mem, hp, defect)


# ------------------------------------------------------------------------------------------------------------------- optimiser cases
@pytest.mark.parametrize("lamb", (False, True), ids=("adamw", "lamb"))
@pytest.mark.parametrize("c", orf.CASES, ids=lambda c: c["id"])
def test_emulation_passes_every_rule_at_every_gpu_case(c, lamb):
    fig, state = {}, {}
    failures = orf.run_case(c, lamb, emu_step, fig, state=state)
    if c["zero"] and not lamb:
        failures += orf.zero_gradient_check(state, orf.ADAMW_GROUPS)
    print("OPTFIG " + str(dict(case=c["id"], lamb=lamb, **{k: round(v, 4) for k, v in fig.items()})))
    assert not failures, failures
    assert all(v <= 1.0 for v in fig.values())


@pytest.mark.parametrize("lamb", (False, True), ids=("adamw", "lamb"))
def test_emulation_passes_the_scaler_sequence_and_the_nan_step(lamb):
    failures = orf.run_scaler_sequence(lamb, emu_step) + orf.run_nan_without_scaler(lamb, emu_step)
    assert not failures, failures


def test_cases_reach_every_branch():
    """Preconditions of the cases themselves: tiled chunks of R = 2, 4, 8, scattered ones for each reason, both lerp branches, a trust
    ratio above and below 1, LAMB's clip binding and not, more than 256 chunks."""
    L = orf.Layout(orf.SMALL, True)
    kinds = set()
    for i, c0, n in L.chunks:
        p = L.params[i]
        if p.sh[1] is None:
            continue
        R = CHUNK // p.cols
        if n != CHUNK:
            kinds.add("ragged")
        elif CHUNK % p.cols or c0 % p.cols:
            kinds.add("columns do not divide")
        elif R not in (2, 4, 8):
            kinds.add(f"R{R} scattered")
        elif p.rows % R:
            kinds.add("rows % R")
        elif (p.sh[1] * 2) & 15:
            kinds.add("misaligned")
        else:
            kinds.add(f"R{R} tiled")
    assert kinds >= {"ragged", "columns do not divide", "R1 scattered", "R16 scattered", "rows % R", "misaligned", "R2 tiled", "R4 tiled", "R8 tiled"}, kinds
    assert any(p.sh[0] is not None and (p.sh[0] * 2) & 7 for p in L.params)  # the uint2 condition's slow side
    assert any(f4(1.0 - g[1]) < 0.5 for g in orf.ADAMW_GROUPS) and any(f4(1.0 - g[1]) >= 0.5 for g in orf.ADAMW_GROUPS)
    assert any(g[4] == 0.0 for g in orf.ADAMW_GROUPS) and orf.Layout(orf.BIG, False).nc > 256
    c = orf.CASES[0]
    mem, hp = L.mem(), orf.hyper(c, True)
    orf.init_state(L, mem, c)
    orf.set_grads(L, mem, c, 0)
    emu_lamb(L, mem, hp)
    _, pn, un, flags, D = orf.read_lamb_ws(L, mem)
    ad = D["adapt"][L.chunk_group] != 0
    raw = np.sqrt(pn[ad] / un[ad])
    assert (raw > 1.5).any() and (raw < 0.7).any() and not ad.all()
    assert [[L.params[i].group for i, _, _ in L.chunks][k] != [L.params[i].group for i, _, _ in L.chunks][k + 1] for k in range(L.nc - 1)].count(True) >= 12


# ------------------------------------------------------------------------------------------------------------------- planted defects
def _defect(defect, lamb=False, c=None, steps=2, sequence=None):
    if sequence:
        return orf.run_scaler_sequence(lamb, emu_step, events=orf.SEQ_EVENTS[:sequence], defect=defect)
    return orf.run_case(c or orf.CASES[0], lamb, emu_step, None, steps, defect=defect)


@pytest.mark.parametrize("defect,owner,cid", [
    ("eps_in_sqrt", "A1", "scale1024_clip0.5"), ("no_bc2", "A1", "scale1024_clip0.5"), ("bc_t", "D1", "t5000"), ("bc_t", "D1", "scale1024_clip0.5"),
    ("lerp_first", "A1", "scale1024_clip0.5"), ("clip_first", "A1", "scale1000"), ("no_1e6", "A1", "scale1000"), ("decay_after", "A1", "scale1024_clip0.5"),
    ("trunc", "S1", "scale1024_clip0.5"), ("t_rowcol", "S1", "scale1024_clip0.5"), ("tp_cols", "S1", "scale1024_clip0.5"),
    ("tiled_r0", "S1", "scale1024_clip0.5"), ("pad_write", "U1", "scale1024_clip0.5")])
def test_adamw_defect_is_rejected_by_its_owner(defect, owner, cid):
    c = next(c for c in orf.CASES if c["id"] == cid)
    failures = _defect(defect, False, c)
    assert owner in _owners(failures), (defect, failures)
    if owner == "A1":
        assert _owners(failures) == {"A1"}, failures  # every other stage still passes from the kernel's own inputs


@pytest.mark.parametrize("defect,owner", [("r_whole_table", "L3"), ("count_off", "L3"), ("trunc", "S1"), ("tp_cols", "S1"), ("tiled_r0", "S1")])
def test_lamb_defect_is_rejected_by_its_owner(defect, owner):
    failures = _defect(defect, True)
    assert owner in _owners(failures), (defect, failures)
    if owner == "L3":
        assert _owners(failures) == {"L3"}, failures


def test_count_off_by_one_shows_on_whole_chunk_tensors_only():
    """The planted count = n / 2048 + 1 is right for every ragged tensor: only tensors of exactly k 2048 elements take a neighbour's sums."""
    c = orf.CASES[0]
    L = orf.Layout(c["specs"], True)
    failures = _defect("count_off", True, steps=1)
    msg = next(m for m in failures if m.startswith("L3"))
    chunks = [int(x) for x in msg.split("chunks [")[1].split("]")[0].split(",")]
    assert chunks and all(L.params[L.chunks[b][0]].n % CHUNK == 0 for b in chunks)


@pytest.mark.parametrize("lamb", (False, True), ids=("adamw", "lamb"))
def test_growth_one_step_late_is_rejected(lamb):
    assert "K1" in _owners(_defect("growth_late", lamb, sequence=7))


def test_moments_updated_on_a_skipped_step_are_rejected():
    failures = _defect("moments_on_skip", False, sequence=4)  # (through the inf step: the moments are NaN from there on)
    assert _owners(failures) == {"U1"} and all("[inf" in m for m in failures), failures


def test_derived_rule_rejects_one_ulp():
    ref = orf.adamw_derived_ref(orf.ADAMW_GROUPS[0], 3, 1024.0)
    D = {k: np.array([f4(v[0])] * 4) for k, v in ref.items()}
    assert not orf.derived_check(D, [ref])
    for k in ref:
        bad = {kk: vv.copy() for kk, vv in D.items()}
        for _ in range(1 if ref[k][1] else 2):  # one rounding of the reference admits the neighbour on one side, never two ulp
            bad[k][0] = np.nextafter(bad[k][0], f4(np.inf))
        assert "D1" in _owners(orf.derived_check(bad, [ref])), k
    assert ref["inv_scale"][0] == f4(1.0 / 1024.0) and orf.adamw_derived_ref(orf.ADAMW_GROUPS[0], 1, None)["inv_scale"][0] == 1.0


# ------------------------------------------------------------------------------------------------------------------- reference optimisers
def _f64_statement(lamb, hp, p, g, m, v, t):
    """The float64 statement of one step on one tensor, the order of the .hip file, hyper-parameters in f64 (not the f32 constants)."""
    G = hp["groups"][0]
    norm = np.sqrt((g ** 2).sum())
    c1 = min(hp["max_norm"] / (norm + 1e-6), 1.0) if hp["max_norm"] > 0 else 1.0
    if not lamb:
        lr, b1, b2, eps, wd = G
        g = g * c1
        p = p - lr * wd * p
        m = m + (1 - b1) * (g - m)
        v = b2 * v + (1 - b2) * g * g
        return p - (lr / (1 - b1 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps), m, v
    lr, b1, b2, b3, eps, wd, bc, adapt, trust = G
    c2 = max(norm * c1 / hp["lamb_max"], 1.0) if hp["lamb_max"] else 1.0
    g = g * (c1 / c2)
    m, v = b1 * m + b3 * g, b2 * v + (1 - b2) * g * g
    u = (m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)) / (1 - b1 ** t) + wd * p
    wn, un = np.sqrt((p ** 2).sum()), np.sqrt((u ** 2).sum())
    r = wn / un if wn > 0 and un > 0 else 1.0
    return p - lr * r * u, m, v


@pytest.mark.parametrize("lamb", (False, True), ids=("adamw", "lamb"))
def test_float64_statement_against_the_reference_optimisers(lamb):
    """Three steps in float64: the statement the kernels are held to against torch.optim.AdamW / src.optim.Lamb with clip_grad_norm_ in
    front.  They differ by rounding only (and LAMB by norm c1 standing for the norm of the clipped gradients): 1e-12 relative to the
    tensor's largest value, where the f32 constants of the kernels (2^-24 each) would show at 1e-7."""
    from src.optim import Lamb

    rng = np.random.default_rng(3)
    p0 = rng.standard_normal((41, 300)) * 0.1
    hp = dict(groups=[orf.LAMB_GROUPS[0] if lamb else orf.ADAMW_GROUPS[0]], max_norm=0.5, lamb_max=1.0)
    q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    G = hp["groups"][0]
    opt = Lamb([q], lr=G[0], betas=(G[1], G[2]), eps=G[4], weight_decay=G[5]) if lamb else \
        torch.optim.AdamW([q], lr=G[0], betas=(G[1], G[2]), eps=G[3], weight_decay=G[4])
    p, m, v = p0, np.zeros_like(p0), np.zeros_like(p0)
    for t, norm in enumerate((0.3, 5.0, 0.8), 1):  # trainer clip off / on / on with LAMB's own binding on none / none / none
        g = rng.standard_normal(p0.shape)
        g *= norm / np.sqrt((g ** 2).sum())
        q.grad = torch.from_numpy(g.copy())
        torch.nn.utils.clip_grad_norm_([q], 0.5)
        opt.step()
        p, m, v = _f64_statement(lamb, hp, p, g, m, v, t)
        st = opt.state[q]
        for name, got, want in (("p", p, q.detach().numpy()), ("m", m, st["exp_avg"].numpy()), ("v", v, st["exp_avg_sq"].numpy())):
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (t, name, np.abs(got - want).max())


# ------------------------------------------------------------------------------------------------------------------- reduce_jobs
def _addr(J):
    return (J["src"] * (2 if J["kind"] == "bf16" else 4), J["dst"] * 4)


def reduce_shape(J):
    src, dst = _addr(J)
    if (not J["tr"] and J["kind"] == "bf16" and J["parts"] <= orf.R_WIDE_MAX_PARTS and J["n"] % 8 == 0 and J["stride"] % 8 == 0
            and not src & 15 and not dst & 15):
        return "wide8"
    return "wide" if J["parts"] <= orf.R_WIDE_MAX_PARTS and not J["tr"] else "lds"


def emu_reduce(mem, jobs, defect=None):
    """k_reduce_jobs: every column's parts in the kernel's order (the vector and scalar loads read the same values)."""
    for J in jobs:
        src = orf.job_source(mem, J).astype(np.float32)
        parts, n = J["parts"], J["n"]
        shape = reduce_shape(J)
        if shape == "wide8":
            a = np.zeros(n, np.float32)
            for p in range(parts):
                a = a + src[p]
        else:
            step = 1 if shape == "wide" else 16
            lanes = []
            for ty in range(step):
                a = np.zeros(n, np.float32)
                p = ty
                while p + 3 * step < parts:
                    a = a + ((src[p] + src[p + step]) + (src[p + 2 * step] + src[p + 3 * step]))
                    p += 4 * step
                while p < parts and not (defect == "drop_part" and parts % 4 == 1):
                    a = a + src[p]
                    p += step
                lanes.append(a)
            if shape == "lds":
                a = np.zeros(n, np.float32)
                for k in range(16):
                    a = a + lanes[k]
        idx = orf.dst_index(J)
        if defect == "tr_swapped" and J["tr"]:
            c, R = np.arange(n), J["tr"]
            idx = (c % R) * (n // R) + c // R
        if defect == "last_column" and n % 4:
            idx, a = idx[:-1], a[:-1]
        mem.ff[J["dst"] + idx] = a


@pytest.mark.parametrize("tier_a", (True, False), ids=("tierA", "tierB"))
def test_reduce_emulation_and_defects(tier_a):
    mem, jobs = orf.reduce_jobs_problem(tier_a)
    assert len(jobs) > 64 and {reduce_shape(J) for J in jobs} == {"wide8", "wide", "lds"}
    assert all(reduce_shape(J) == "lds" for J in jobs if J["tr"]) and any(J["tr"] and J["parts"] <= 32 for J in jobs)
    assert any(J["n"] % 8 == 0 and J["stride"] % 8 and J["kind"] == "bf16" and J["parts"] <= 32 for J in jobs)
    assert {(_addr(J)[0] & 15) for J in jobs if J["kind"] == "bf16"} >= {0, 8, 4, 2} and {(_addr(J)[1] & 15) for J in jobs} >= {0, 4}
    fig = {}
    after = mem.copy()
    emu_reduce(after, jobs)
    failures = orf.reduce_check(mem, after, jobs, tier_a, fig)
    assert not failures, failures
    assert tier_a or 0 < fig["R1 dst"] <= 1.0
    for defect in ("drop_part", "tr_swapped", "last_column"):
        bad = mem.copy()
        emu_reduce(bad, jobs, defect)
        assert "R1" in _owners(orf.reduce_check(mem, bad, jobs, tier_a)), defect
    bad = after.copy()
    bad.f[jobs[5]["dst"] + jobs[5]["n"]] = 0  # one element beyond n
    assert "U1" in _owners(orf.reduce_check(mem, bad, jobs, tier_a))
