"""The ten attention kernels of csrc/g2048_attention.hip against the float64 reference of tests/attention_ref.py, with the
dropout mask each kernel actually applied (read back by probe launches, see attention_ref), at every head count.

Kernel families, selected per call through the environment (read per launch by the library):

    Sq = 17   mfma32  default                        k_attn_fwd17_mfma<true>  / k_attn_bwd17_mfma<true>
              mfma64  G2048_ATTN_WIDE_INDEX=1        k_attn_fwd17_mfma<false> / k_attn_bwd17_mfma<false>
              scalar  G2048_ATTN_SCALAR=1            k_attn_fwd17 / k_attn_bwd17
    Sq = 1    rows    default, H == 8 only           k_attn_fwd1_rows / k_attn_bwd1_rows
              lane    default for H != 8; G2048_ATTN_SCALAR=1 for H == 8      k_attn_fwd1 / k_attn_bwd1

Cells (every cell runs every family of its Sq):
    * GRID:    H in {1, 2, 3, 4, 6, 8, 12, 16} x B in {1, 5, 13, 683, 2048} x Sq in {17, 1} at p = 0.1          (80 cells)
               heads per forward MFMA wave 1, 1, 3, 2, 3, 1, 6, 2; grids that are and are not multiples of 8
    * P_SET:   p in {0, 0.5} at (H, B) in {(3, 13), (4, 683), (8, 2048), (12, 5), (16, 1)} x Sq in {17, 1}      (20 cells)
    * EXTREME: Q, K = randn * 8 at (H, B) in {(8, 2048), (3, 13), (6, 683)} x p in {0, 0.1} x Sq in {17, 1}     (12 cells)
    * STRIDES: three separate q, k, v with token stride H * 32 + 8 and a padded batch stride,
               (H, B) in {(3, 13), (8, 683)} x Sq in {17, 1} at p = 0.1                                        (4 cells)
GRID, P_SET and EXTREME use the layouts of the update (Sq = 17: packed qkv; Sq = 1: contiguous q + packed kv).
Every cell checks, per family: the forward-probe and backward-probe masks (bit-identical across families and between forward and
backward; keep rate within 5 binomial standard deviations of 1 - thr / 2^24), o / dq / dk / dv through ``attention_ref.accept``
(whole-tensor error < 4e-3, worst per-pair error < 2 x the rounding model's), lse within the derived ``attention_ref.lse_bound``,
and the footprint: outputs and gradients live in NaN-patterned buffers with a spare sample on either side and padding between the
rows; everything inside is finite afterwards, every byte outside is untouched.

At EXTREME most softmax rows are one-hot and a pair of 17 one-hot rows has a true dQ / dK far below f32 resolution (1e-78 occurs):
the rounding model's own worst per-pair error on dq / dk is then of order 1e2 and the per-pair test of those two tensors is vacuous
there; the whole-tensor bound and the per-pair test of o / dv still hold the kernels.

Measured on the MI355X (largest over all cells; per-pair ratio = kernel worst per-pair error / yardstick, must stay <= 2;
lse = worst |error| / derived bound, must stay <= 1):
    family   o     dq    dk    dv    (ratio, usual logits)   whole-tensor worst   lse worst |error|  (of bound)
    mfma32   1.00  1.00  1.00  1.00                          2.64e-3 (dq)         1.98e-6            0.060
    mfma64   bit-identical to mfma32 in every cell
    scalar   0.67  0.65  0.65  0.69                          1.81e-3              2.06e-6            0.065
    rows     0.58  0.57  0.57  0.60                          1.74e-3              1.17e-6            0.041
    lane     0.59  0.60  0.63  0.64                          1.87e-3              1.51e-6            0.055
    (mfma at 1.00: on the worst pair the kernels' error equals the model's - the model rounds where they round.)
    EXTREME: o / dv ratios <= 1.00 (mfma, rows, lane), <= 0.90 (scalar); dq / dk 1.52 / 1.73 on mfma in the vacuous regime described
    above (yardstick 3e2), <= 0.01 elsewhere; whole-tensor <= 2.39e-3; lse worst 6.0e-5 = 0.083 of the bound (scalar), 4.2e-5 = 0.060 (mfma).
"""
import json
import os

import numpy as np
import pytest
import torch

import attention_ref as ar

pytestmark = pytest.mark.gpu
S, HD = ar.SK, ar.HD
SCALE = HD ** -0.5
BF16_NAN, F32_NAN = 0x7FE5, 0x7FC12345  # the patterns unwritten memory holds
ENV = ("G2048_ATTN_SCALAR", "G2048_ATTN_WIDE_INDEX")


def _families(Sq, H):
    if Sq == S:
        return {"mfma32": ("0", "0"), "mfma64": ("0", "1"), "scalar": ("1", "0")}
    return {"rows": ("0", "0"), "lane": ("1", "0")} if H == 8 else {"lane": ("0", "0")}


def _layout(kind, B, H, Sq):
    """name -> (buffer, offset of sample 0, batch stride, token stride) in elements, and the buffers' sizes; one spare sample on
    either side of every buffer."""
    hw, G = H * HD, B + 2
    if kind == "packed":
        W = 3 * hw
        return {n: ("qkv", S * W + i * hw, S * W, W) for i, n in enumerate("qkv")}, {"qkv": G * S * W}
    if kind == "cls":
        W = 2 * hw
        return ({"q": ("q", Sq * hw, Sq * hw, hw), "k": ("kv", S * W, S * W, W), "v": ("kv", S * W + hw, S * W, W)},
                {"q": G * Sq * hw, "kv": G * S * W})
    assert kind == "padded"
    ts = hw + 8
    spec, sizes = {}, {}
    for n in "qkv":
        bs = (Sq if n == "q" else S) * ts + 16
        spec[n], sizes[n] = (n, bs, bs, ts), G * bs
    return spec, sizes


def _nan_bf16(n, dev):
    return torch.full((n,), BF16_NAN, dtype=torch.int16, device=dev).view(torch.bfloat16)


class _Launch:
    """One forward + backward of a family on CPU operands q [B, Sq, H, 32], k, v [B, 17, H, 32], dout [B, Sq, H, 32]."""

    def __init__(self, dev, B, H, Sq, kind):
        self.dev, self.B, self.H, self.Sq = dev, B, H, Sq
        self.spec, self.sizes = _layout(kind, B, H, Sq)
        self.rows = {"q": Sq, "k": S, "v": S}

    def _view(self, bufs, n):
        b, off, sb, ss = self.spec[n]
        return bufs[b].as_strided((self.B, self.rows[n], self.H, HD), (sb, ss, HD, 1), off)

    def _ptrs(self, bufs):
        return [bufs[self.spec[n][0]].data_ptr() + 2 * self.spec[n][1] for n in "qkv"]

    def strides(self):
        return [x for n in "qkv" for x in self.spec[n][2:]]

    def inputs(self, q, k, v):
        bufs = {b: _nan_bf16(n, self.dev) for b, n in self.sizes.items()}
        for n, t in zip("qkv", (q, k, v)):
            self._view(bufs, n).copy_(t.to(self.dev))
        return bufs

    def run(self, monkeypatch, env, q, k, v, dout, p, seed, seed_state=0, lse_from=None):
        """-> dict of CPU tensors: o [B, Sq, H, 32], lse [B, H, Sq], dq / dk / dv shaped like q / k / v.  Asserts the footprint.
        ``lse_from``: skip the forward and feed the backward this lse (of another family's forward)."""
        from src.g2048 import native as nv

        for name, val in zip(ENV, env):
            monkeypatch.setenv(name, val)
        B, H, Sq, dev = self.B, self.H, self.Sq, self.dev
        bufs = self.inputs(q, k, v)
        out = {}
        og = _nan_bf16((B + 2) * Sq * H * HD, dev).view(B + 2, Sq, H, HD)
        lg = torch.full((B + 2, H, Sq), F32_NAN, dtype=torch.int32, device=dev).view(torch.float32)
        if lse_from is None:
            nv.attn_fwd(*self._ptrs(bufs), og[1:-1], lg[1:-1], B, H, Sq, self.strides(), SCALE, p, seed, seed_state)
            for guard, pat in ((og.view(torch.int16), BF16_NAN), (lg.view(torch.int32), F32_NAN)):
                assert (guard[0] == pat).all() and (guard[-1] == pat).all(), "forward wrote outside its outputs"
            out["o"], out["lse"] = og[1:-1].cpu(), lg[1:-1].cpu()
            assert torch.isfinite(out["o"].float()).all() and torch.isfinite(out["lse"]).all(), "forward left elements unwritten"
        else:
            lg[1:-1].copy_(lse_from.to(dev))
        grads = {b: _nan_bf16(n, dev) for b, n in self.sizes.items()}
        nv.attn_bwd(*self._ptrs(bufs), dout.to(dev).contiguous(), lg[1:-1], *self._ptrs(grads), B, H, Sq, self.strides(), SCALE, p,
                    seed, seed_state)
        for n in "qkv":
            out["d" + n] = self._view(grads, n).cpu()
            assert torch.isfinite(out["d" + n].float()).all(), f"backward left elements of d{n} unwritten"
            self._view(grads, n).view(torch.int16).fill_(BF16_NAN)  # what is left must be the untouched pattern
        for b, g in grads.items():
            assert (g.view(torch.int16) == BF16_NAN).all(), f"backward wrote outside the rows of its gradients (buffer {b})"
        for name in ENV:
            monkeypatch.setenv(name, "0")
        return out


def _to_ref(out):
    """The kernels' [B, S, H, 32] outputs in the reference's [B, H, S, 32]."""
    return dict(o=ar.bhsd(out["o"]), lse=out["lse"], dq=ar.bhsd(out["dq"]), dk=ar.bhsd(out["dk"]), dv=ar.bhsd(out["dv"]))


def _keep_probability(p):
    return 1.0 - int(np.float32(p) * np.float32(16777216.0)) / 16777216.0  # the kernels' thr = (uint32)(p * 2^24), p in f32


def _probe_masks(dev, monkeypatch, L, fams, p, seed, seed_state=0):
    """The masks every family's forward and backward applied for (seed, seed_state): all asserted equal; returns the mask."""
    B, H, Sq = L.B, L.H, L.Sq
    q, k, v, dout = ar.probe_operands(B, H, Sq)
    vr = (torch.randn(B, S, H, HD, generator=torch.Generator().manual_seed(9)) * 1.5).to(torch.bfloat16)
    gr = torch.randn(B, Sq, H, HD, generator=torch.Generator().manual_seed(10)).to(torch.bfloat16)
    keep, prev_lse = None, None
    for name, env in fams.items():
        fwd = L.run(monkeypatch, env, q, k, v, gr, p, seed, seed_state)
        kf = ar.keep_from_forward_probe(fwd["o"])
        # the backward's mask, with this family's lse and with the previous family's (forward / backward of different families)
        for lse_from in ([None] if prev_lse is None else [None, prev_lse]):
            bwd = L.run(monkeypatch, env, q, k, vr, dout, p, seed, seed_state, lse_from=lse_from)
            kb = ar.keep_from_backward_probe(bwd["dv"], Sq)
            assert torch.equal(kb, kf), f"{name}: the backward's mask differs from the forward's"
        if keep is not None:
            assert torch.equal(kf, keep), f"{name}: forward mask differs from the other families'"
        keep, prev_lse = kf, fwd["lse"]
    if not p > 0:
        assert keep.all()
        return None
    N, pk = keep.numel(), _keep_probability(p)
    assert abs(int(keep.sum()) - N * pk) <= 5.0 * (N * pk * (1 - pk)) ** 0.5, (int(keep.sum()), N, pk)
    return keep


def _cell(dev, monkeypatch, tag, Sq, H, B, p, qk_std=1.5, kind=None):
    kind = kind or ("packed" if Sq == S else "cls")
    L = _Launch(dev, B, H, Sq, kind)
    fams = _families(Sq, H)
    seed = 0x9E3779B97F4A7C15 ^ (B * 1000003 + H * 101 + Sq)
    keep = _probe_masks(dev, monkeypatch, L, fams, p, seed)
    q, k, v, dout = ar.make_operands(B, H, Sq, 1000 * H + B + Sq, qk_std)
    rq, rk, rv, rg = (ar.bhsd(t) for t in (q, k, v, dout))
    ref = ar.attention_ref(rq, rk, rv, rg, keep, p, SCALE)
    model = ar.attention_rounding_model(rq, rk, rv, rg, keep, p, SCALE)
    floor = ar.model_floor(Sq, p, qk_std) if B * H < 256 else None
    bound = ar.lse_bound(rq, rk, SCALE)
    failures = []
    for name, env in fams.items():
        got = _to_ref(L.run(monkeypatch, env, q, k, v, dout, p, seed))
        fig = {}
        bad = ar.accept(got, ref, model, floor, fig)
        lse_err = (got["lse"].double() - ref["lse"]).abs()
        fig["lse"] = dict(err=lse_err.max().item(), of_bound=(lse_err / bound).max().item())
        print("ATTNFIG " + json.dumps(dict(tag=tag, Sq=Sq, H=H, B=B, p=p, family=name, fig=fig)))
        if not (lse_err <= bound).all():
            bad.append(f"lse: error {fig['lse']['err']:.3e} is {fig['lse']['of_bound']:.2f} x the derived bound")
        if qk_std > 2 and not p > 0:
            # rows whose softmax is one-hot far below f32 resolution (every other probability < 1e-20): o is the selected V row, bit for bit
            P = torch.exp(torch.einsum("bhqd,bhkd->bhqk", rq.double(), rk.double()) * SCALE - ref["lse"].unsqueeze(-1))
            top2 = P.topk(2, dim=-1).values
            onehot = top2[..., 1] < 1e-20
            assert onehot.any()
            want = torch.gather(rv.float(), 2, P.argmax(-1).unsqueeze(-1).expand(-1, -1, -1, HD))
            if not torch.equal(got["o"].float()[onehot], want[onehot]):
                bad.append("o of a one-hot row is not the selected V row")
        failures += [f"{name}: {b}" for b in bad]
    assert not failures, failures


GRID_H, GRID_B = (1, 2, 3, 4, 6, 8, 12, 16), (1, 5, 13, 683, 2048)
P_SET_CELLS = ((3, 13), (4, 683), (8, 2048), (12, 5), (16, 1))
EXTREME_CELLS = ((8, 2048), (3, 13), (6, 683))


@pytest.mark.parametrize("B", GRID_B)
@pytest.mark.parametrize("H", GRID_H)
@pytest.mark.parametrize("Sq", [S, 1])
def test_grid_every_head_count_and_batch(dev, monkeypatch, Sq, H, B):
    _cell(dev, monkeypatch, "grid", Sq, H, B, 0.1)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("H,B", P_SET_CELLS)
@pytest.mark.parametrize("Sq", [S, 1])
def test_dropout_probabilities(dev, monkeypatch, Sq, H, B, p):
    _cell(dev, monkeypatch, "p_set", Sq, H, B, p)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("H,B", EXTREME_CELLS)
@pytest.mark.parametrize("Sq", [S, 1])
def test_extreme_logits(dev, monkeypatch, Sq, H, B, p):
    """Q, K = randn * 8: scaled scores with sigma about 64, row maxima beyond 88 (a bare f32 exp overflows there).  The mask is probed
    at the probe's own moderate operands."""
    _cell(dev, monkeypatch, "extreme", Sq, H, B, p, qk_std=8.0)


@pytest.mark.parametrize("H,B", [(3, 13), (8, 683)])
@pytest.mark.parametrize("Sq", [S, 1])
def test_padded_strides(dev, monkeypatch, Sq, H, B):
    """Three separate q, k, v tensors, token stride H * 32 + 8 elements, batch stride rows * token stride + 16; the gradients are
    written with the same strides into NaN-patterned buffers whose padding must stay untouched (``_Launch.run`` asserts it)."""
    _cell(dev, monkeypatch, "strides", Sq, H, B, 0.1, kind="padded")


def test_layouts_are_interchangeable(dev, monkeypatch):
    """The same operands through the packed, the q + packed-kv and the padded layout: bit-identical results (Sq = 17, MFMA)."""
    B, H, p, seed = 37, 6, 0.1, 4321
    q, k, v, dout = ar.make_operands(B, H, S, 77)
    res = [_Launch(dev, B, H, S, kind).run(monkeypatch, ("0", "0"), q, k, v, dout, p, seed) for kind in ("packed", "cls", "padded")]
    for other in res[1:]:
        for n in res[0]:
            assert torch.equal(res[0][n], other[n]), n


def test_mask_follows_the_seed_word_and_the_documented_index(dev, monkeypatch):
    """With a device-resident seed word the mask repeats while the word stands and changes when it is advanced by one; the seed
    itself selects the mask; and the Sq = 1 kernels index their elements pair * 32 + key, the Sq = 17 kernels (pair * 17 + query) *
    32 + key - so for one (seed, word) the CLS-row mask of pair n is row n of the flattened [pairs * 17, 17] mask of the 17-token
    kernels (NOT the query-0 row of the same pair)."""
    B, H, p, seed = 40, 6, 0.5, 0x1234_5678_9ABC
    word = torch.tensor([0x0123_4567_89AB_CDEF], dtype=torch.int64, device=dev)
    L17, L1 = _Launch(dev, B, H, S, "packed"), _Launch(dev, B, H, 1, "cls")
    masks = {}
    for tag, ptr in (("none", 0), ("word", word.data_ptr())):
        masks[tag, 17] = _probe_masks(dev, monkeypatch, L17, _families(S, H), p, seed, ptr)
        masks[tag, 1] = _probe_masks(dev, monkeypatch, L1, _families(1, H), p, seed, ptr)
    again = _probe_masks(dev, monkeypatch, L17, {"mfma32": ("0", "0")}, p, seed, word.data_ptr())
    assert torch.equal(again, masks["word", 17])
    assert not torch.equal(masks["none", 17], masks["word", 17])
    word.add_(1)
    torch.cuda.synchronize()
    advanced = _probe_masks(dev, monkeypatch, L17, _families(S, H), p, seed, word.data_ptr())
    assert not torch.equal(advanced, masks["word", 17])
    assert abs((advanced == masks["word", 17]).double().mean().item() - 0.5) < 0.02  # two independent p = 0.5 masks agree on half
    other_seed = _probe_masks(dev, monkeypatch, L17, {"scalar": ("1", "0")}, p, seed + 1)
    assert not torch.equal(other_seed, masks["none", 17])
    for tag in ("none", "word"):
        rows = masks[tag, 17].reshape(B * H * S, S)
        assert torch.equal(masks[tag, 1].reshape(B * H, S), rows[:B * H])
    # H == 8: both CLS-row families (asserted equal inside) against the same relation
    L17, L1 = _Launch(dev, 11, 8, S, "packed"), _Launch(dev, 11, 8, 1, "cls")
    m17 = _probe_masks(dev, monkeypatch, L17, {"mfma32": ("0", "0")}, p, seed)
    m1 = _probe_masks(dev, monkeypatch, L1, _families(1, 8), p, seed)
    assert torch.equal(m1.reshape(88, S), m17.reshape(88 * S, S)[:88])


def test_refusals_launch_nothing(dev, monkeypatch):
    """Misaligned pointers, strides that are no multiple of 8 elements, Sq outside {1, 17} and p_drop outside [0, 1) are refused with
    G2048_EINVAL (a NativeError) and nothing is written."""
    from src.g2048 import native as nv

    B, H = 4, 3
    hw, W = H * HD, 3 * H * HD
    qkv = torch.randn(B, S, W, device=dev).to(torch.bfloat16)
    dout = torch.randn(B, S + 1, hw, device=dev).to(torch.bfloat16)  # (sized for the refused Sq = 18 too: the wrapper checks sizes first)
    base, good = qkv.data_ptr(), (S * W, W) * 3
    o = _nan_bf16(B * (S + 1) * hw + 8, dev)
    lse = torch.full((B * H * (S + 1),), F32_NAN, dtype=torch.int32, device=dev).view(torch.float32)
    lse_in = torch.zeros(B * H * (S + 1), device=dev)
    dqkv = _nan_bf16(B * S * W + 8, dev)
    db = dqkv.data_ptr()

    def refused(ptrs=(0, 2 * hw, 4 * hw), strides=good, Sq=S, p=0.1, o_off=0, d_off=0):
        q, k, v = (base + x for x in ptrs)
        with pytest.raises(nv.NativeError, match="invalid argument"):
            nv.attn_fwd(q, k, v, o[o_off:], lse, B, H, Sq, strides, SCALE, p, 1, 0)
        with pytest.raises(nv.NativeError, match="invalid argument"):
            nv.attn_bwd(q, k, v, dout, lse_in, db + d_off, db + 2 * hw, db + 4 * hw, B, H, Sq, strides, SCALE, p, 1, 0)
        torch.cuda.synchronize()
        assert (o.view(torch.int16) == BF16_NAN).all() and (lse.view(torch.int32) == F32_NAN).all()
        assert (dqkv.view(torch.int16) == BF16_NAN).all()

    for ptrs in ((2, 2 * hw, 4 * hw), (0, 2 * hw + 8, 4 * hw), (0, 2 * hw, 4 * hw + 14)):
        refused(ptrs=ptrs)
    for i in range(6):
        refused(strides=tuple(x + (4 if j == i else 0) for j, x in enumerate(good)))
    for Sq in (0, 2, 5, 16, 18):
        refused(Sq=Sq)
    for p in (1.0, 1.5, -0.1, float("nan")):
        refused(p=p)
    refused(o_off=1, d_off=2)  # misaligned outputs
    # and the call they all vary is legal
    nv.attn_fwd(base, base + 2 * hw, base + 4 * hw, o, lse, B, H, S, good, SCALE, 0.1, 1, 0)
    nv.attn_bwd(base, base + 2 * hw, base + 4 * hw, dout, lse, db, db + 2 * hw, db + 4 * hw, B, H, S, good, SCALE, 0.1, 1, 0)
    assert torch.isfinite(o[:B * S * hw].float()).all() and torch.isfinite(dqkv[:B * S * W].float()).all()


# ------------------------------------------------------------------------------------------------------ module level
def _module_gradient_errors(dev, d_model, nhead, reduction):
    """A two-layer PPOAgent of the given width with the weights of tests/golden/weights_recipe.py, minibatch 2048, random downstream
    gradients on logits and values (the set-up of test_update_path_gradients_per_tensor_at_minibatch_size): -> the (H, Sq) of every
    ``native.attn_fwd`` call of the HIP update path, {parameter: (e_hip, e_torch)} against an fp32 backward, and the largest
    deviations of logits and values from fp32."""
    import copy
    import sys

    from src.g2048 import native as nv
    from src.ppo import PPOAgent
    from test_gpu_reference_vectors import _torch_forward

    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from weights_recipe import fill_state_dict

    agent = PPOAgent(observation_dim=31, action_dim=4, hidden_dim=2 * d_model, d_model=d_model, nhead=nhead, num_layers=2,
                     dim_feedforward=4 * d_model, dropout=0.0, reduction=reduction)
    sd = agent.state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in fill_state_dict({k: tuple(v.shape) for k, v in sd.items()}).items()})
    agent.load_state_dict(sd)
    agent = agent.to(dev).train()
    g = torch.Generator(device="cpu").manual_seed(5)
    boards = torch.randint(0, 12, (2048, 16), generator=g, dtype=torch.uint8).to(dev)
    gl, gv = torch.randn(2048, 4, generator=g).to(dev), torch.randn(2048, generator=g).to(dev)

    def grads(model, fwd, autocast):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            lo, va = fwd(model)
        ((lo.float() * gl).sum() + (va.float().flatten() * gv).sum()).backward()
        return [prm.grad.detach().float().clone() for prm in model.parameters()], lo.detach().float(), va.detach().float().flatten()

    ref = copy.deepcopy(agent).float()
    ref.transformer._shadow, ref._head_shadow = None, None
    g32, l32, v32 = grads(ref, lambda m: _torch_forward(m, boards, reduction), False)
    g16, _, _ = grads(ref, lambda m: _torch_forward(m, boards, reduction), True)
    seen = []
    orig = nv.attn_fwd

    def spy(*a, **kw):
        seen.append((a[6], a[7]))  # (H, Sq)
        return orig(*a, **kw)

    nv.attn_fwd = spy
    try:
        gh, lh, vh = grads(agent, lambda m: m(boards, None), True)
    finally:
        nv.attn_fwd = orig
    rel = lambda a, b: ((a - b).norm() / b.norm().clamp_min(1e-12)).item()
    errs = {}
    for (n, _), a32, a16, ah in zip(agent.named_parameters(), g32, g16, gh):
        assert torch.isfinite(ah).all(), n
        errs[n] = (rel(ah, a32), rel(a16, a32))
    return seen, errs, (lh - l32).abs().max().item(), (vh - v32).abs().max().item()


@pytest.mark.parametrize("reduction", ["cls", "mean"])
@pytest.mark.parametrize("d_model,nhead", [(128, 4), (96, 3), (512, 16)])
def test_update_path_gradients_with_head_dim_32_away_from_8_heads(dev, d_model, nhead, reduction):
    """PPOAgents whose head_dim is 32 with 4, 3 and 16 heads: the HIP attention runs (Sq = 17 in every full layer and, for "cls", Sq = 1
    in the last) and every parameter gradient at minibatch 2048 is as close to an fp32 backward as torch's own bf16 autocast backward
    (e_hip < 1.3 e_torch + 0.01 per tensor: the form of test_update_path_gradients_per_tensor_at_minibatch_size)."""
    seen, errs, dl, dv = _module_gradient_errors(dev, d_model, nhead, reduction)
    assert (nhead, S) in seen and all(h == nhead for h, _ in seen), seen
    assert ((nhead, 1) in seen) == (reduction == "cls"), seen
    assert dl < 0.05 and dv < 0.05, (dl, dv)
    bad = {n: (round(e_hip, 4), round(e_torch, 4)) for n, (e_hip, e_torch) in errs.items() if not e_hip < 1.3 * e_torch + 0.01}
    assert not bad, (d_model, nhead, reduction, bad)
