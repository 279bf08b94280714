"""The float64 attention reference of tests/attention_ref.py has teeth (host only, no kernel runs here).

It agrees with torch.autograd through a float64 softmax-attention; the acceptance function the GPU tests use
(``attention_ref.accept``) takes the rounding model and rejects four subtly wrong implementations on the very operands of
tests/test_gpu_attention.py; the workgroup -> item map of the attention kernels is a bijection.
"""
import pytest
import torch

import attention_ref as ar

SCALE = ar.HD ** -0.5


def _operands(B, H, Sq, seed, qk_std=1.5):
    return tuple(ar.bhsd(t) for t in ar.make_operands(B, H, Sq, seed, qk_std))


def _random_keep(B, H, Sq, p, seed=7):
    return torch.rand(B, H, Sq, ar.SK, generator=torch.Generator().manual_seed(seed)) >= p


@pytest.mark.parametrize("Sq", [17, 1])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_reference_equals_autograd(Sq, p):
    """keep=None: autograd through softmax(QK^T scale) V; with a mask: autograd through P * keep / (1 - p).  1e-12."""
    B, H = 5, 3
    q, k, v, dout = _operands(B, H, Sq, 11)
    keep = _random_keep(B, H, Sq, p) if p > 0 else None
    ref = ar.attention_ref(q, k, v, dout, keep, p, SCALE)
    q64, k64, v64 = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    s = q64 @ k64.transpose(-1, -2) * SCALE
    P = torch.softmax(s, dim=-1)
    if keep is not None:
        P = P * keep.double() / (1 - p)
    o = P @ v64
    o.backward(dout.double())
    for name, want in (("o", o.detach()), ("lse", torch.logsumexp(s.detach(), dim=-1)), ("dq", q64.grad), ("dk", k64.grad),
                       ("dv", v64.grad)):
        assert (ref[name] - want).abs().max().item() < 1e-12 * max(1.0, want.abs().max().item()), name


def _mutant(q, k, v, dout, keep, p, scale, kind):
    """Float64 attention with one defect, outputs rounded to bf16 as a kernel stores them.
    no_inv_keep: dP misses 1/(1-p);  no_mask: dP misses the mask;  transposed: dK / dV computed with the mask indexed [key][query];
    no_max: the softmax exponentials are taken in f32 without subtracting the row maximum."""
    q, k, v, dout = (t.double() for t in (q, k, v, dout))
    inv = 1.0 / (1.0 - p)
    w = keep.double()
    s = q @ k.transpose(-1, -2) * scale
    if kind == "no_max":
        e = torch.exp(s.float()).double()
        P = e / e.sum(-1, keepdim=True)
    else:
        P = torch.softmax(s, dim=-1)
    o = (P * w * inv) @ v
    dp_raw = dout @ v.transpose(-1, -2)
    dp = {"no_inv_keep": dp_raw * w, "no_mask": dp_raw * inv}.get(kind, dp_raw * w * inv)
    ds = P * (dp - (P * dp).sum(-1, keepdim=True)) * scale
    dq = ds @ k
    w2 = w.transpose(-1, -2) if kind == "transposed" else w
    dp2 = dp_raw * w2 * inv
    ds2 = P * (dp2 - (P * dp).sum(-1, keepdim=True)) * scale
    dk = ds2.transpose(-1, -2) @ q
    dv = (P * w2 * inv).transpose(-1, -2) @ dout
    r = lambda t: t.float().to(torch.bfloat16)
    return dict(o=r(o), dq=r(dq), dk=r(dk), dv=r(dv))


# the cell of the GPU grid with the most pairs per launch at H = 8 is B = 2048; 256 samples of the same draw are enough here
CASES = [(17, 0.1, 1.5, "no_inv_keep"), (17, 0.1, 1.5, "no_mask"), (17, 0.1, 1.5, "transposed"), (17, 0.5, 1.5, "no_inv_keep"),
         (1, 0.1, 1.5, "no_inv_keep"), (1, 0.1, 1.5, "no_mask"), (17, 0.1, 8.0, "no_max"), (1, 0.1, 8.0, "no_max"),
         (17, 0.1, 8.0, "no_inv_keep"), (17, 0.1, 8.0, "transposed")]


@pytest.mark.parametrize("Sq,p,qk_std,kind", CASES)
def test_acceptance_rejects_mutants(Sq, p, qk_std, kind):
    B, H = 256, 8
    q, k, v, dout = _operands(B, H, Sq, 100 + Sq, qk_std)
    keep = _random_keep(B, H, Sq, p)
    ref = ar.attention_ref(q, k, v, dout, keep, p, SCALE)
    model = ar.attention_rounding_model(q, k, v, dout, keep, p, SCALE)
    bad = ar.accept(_mutant(q, k, v, dout, keep, p, SCALE, kind), ref, model, ar.model_floor(Sq, p, qk_std))
    assert bad, f"{kind} was accepted"
    if kind != "no_max":  # the defect moves a gradient by far more than any rounding: the WHOLE-tensor bound must see it
        assert any("whole-tensor" in b for b in bad), bad


@pytest.mark.parametrize("qk_std", [1.5, 8.0])
@pytest.mark.parametrize("Sq", [17, 1])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_acceptance_takes_the_rounding_model_and_the_exact_result(Sq, p, qk_std):
    B, H = 256, 8
    q, k, v, dout = _operands(B, H, Sq, 100 + Sq, qk_std)
    keep = _random_keep(B, H, Sq, p) if p > 0 else None
    ref = ar.attention_ref(q, k, v, dout, keep, p, SCALE)
    model = ar.attention_rounding_model(q, k, v, dout, keep, p, SCALE)
    fig = {}
    assert ar.accept(model, ref, model, ar.model_floor(Sq, p, qk_std), fig) == [], fig
    assert all(f["whole"] < 3e-3 for f in fig.values()), fig  # the model alone leaves room below the 4e-3 bound
    assert ar.accept(ref, ref, model) == []
    assert (model["lse"] - ref["lse"]).abs().le(ar.lse_bound(q, k, SCALE)).all()  # the derived lse bound covers the model's f32 path


def test_probes_recover_a_known_mask():
    """The probe operands turn a forward's o and a backward's dv into the mask: run the float64 reference (rounded to bf16) on them
    with a known mask and read it back both ways; no kept probability of the probe's Q, K rounds to zero."""
    for Sq in (17, 1):
        B, H, p = 64, 4, 0.5
        q, k, v, dout = ar.probe_operands(B, H, Sq)
        keep = _random_keep(B, H, Sq, p)
        out = ar.attention_ref(ar.bhsd(q), ar.bhsd(k), ar.bhsd(v), ar.bhsd(dout), keep, p, SCALE)
        o = ar.bhsd(out["o"]).float().to(torch.bfloat16)
        dv = ar.bhsd(out["dv"]).float().to(torch.bfloat16)
        assert torch.equal(ar.keep_from_forward_probe(o), keep)
        assert torch.equal(ar.keep_from_backward_probe(dv, Sq), keep)


def test_xcd_block_is_a_bijection():
    for n in range(1, 101):
        assert sorted(ar.xcd_block(n, b) for b in range(n)) == list(range(n)), n
