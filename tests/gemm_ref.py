"""Float64 references, operand generators and acceptance rules for the GEMM kernels of the update (csrc/g2048_linear.hip,
csrc/g2048_dweight.hip): tests/test_gpu_gemm.py runs the kernels against them, tests/test_gemm_ref.py holds them to an f32 emulation
and to planted defects on the CPU.  Everything here is the textbook operation on torch tensors and runs on any device.

Two tiers of operands:

* Tier A, exactly representable.  Operands are small integers stored in bf16, biases integers stored in f32.  Every product and every
  partial sum in ANY order is then an integer below 2^24, so the f32 accumulator of any correct kernel holds the exact result and the
  output must equal the reference bit for bit: the round-to-nearest-even bf16 of the float64 result for bf16 outputs, the float64 result
  itself for f32 outputs.  The precondition is asserted from the reference (``assert_exact``: sum |products| + |bias| < 2^24), and so is
  that the case exercises the rounding (``assert_exercises_rounding``: at least 25 % of the results need rounding to bf16 and at least
  1 % are exact ties between two bf16 neighbours).  A result of magnitude in [2^e, 2^(e+1)) has a bf16 spacing of 2^(e-7): an integer
  needs rounding from 256 on, and is a tie with probability 1 / spacing, so the results should sit between 2^8 and 2^14.  A large integer
  bias puts them there; without one ``int_range`` moves the operands' mean with the reduction length.
* Tier B, realistic ranges.  Non-zero means (x + 0.3, w + 0.02), per-row scales 2^[-6, 3], an f32 randn bias.  Acceptance is per element,
      |y - ref| <= (1 + 2^-8) (2^-8 |ref| + (n + 1) 2^-23 (|x| |w|^T + |bias|)),
  n the reduction length: half a bf16 unit in the last place, plus the any-order summation bound at unit roundoff 2^-23 (which also
  covers an accumulator that truncates); the factor in front because the rounding acts on the accumulated value, not on ref.  bf16 x bf16
  products are exact in f32.  For f32 outputs the summation term alone.  Derived, not measured; the f32 emulation of the self-test sits
  at 0.95-0.98 of it, so a second rounding or a bf16 intermediate breaks it.
"""
import numpy as np
import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
BF16_NAN, F32_NAN, U8_PAT = 0x7FE5, 0x7FC12345, 0xE5  # the patterns unwritten memory holds in the GPU tests
EXACT = 2.0 ** 24
REL_LIMIT = 4e-3


def f64(t):
    return t.to(F64)


# ------------------------------------------------------------------------------------------------------------ references
def linear(x, w, bias=None):
    """x [T, K] w [N, K]^T (+ bias [N]) in float64."""
    y = f64(x) @ f64(w).t()
    return y if bias is None else y + f64(bias)


def relu(v):
    return torch.clamp_min(v, 0.0)


def masked_bwd(dy, w2t, bit, inv_keep):
    """where(bit, (dy [T, K] w2t [N, K]^T) inv_keep, 0) in float64 -> [T, N]."""
    g = (f64(dy) @ f64(w2t).t()) * inv_keep
    return torch.where(bit, g, torch.zeros((), dtype=F64, device=g.device))


def colsum(v):
    return f64(v).sum(0)


def dweight(dy, x, slices):
    """-> (parts [slices, N, K], column sums [slices, N]) in float64: dY^T X and the column sums of dY over each of ``slices`` equal,
    consecutive token slices of dy [T, N], x [T, K]."""
    T = dy.shape[0]
    assert T % slices == 0
    d, xx = f64(dy).reshape(slices, T // slices, -1), f64(x).reshape(slices, T // slices, -1)
    return d.transpose(1, 2) @ xx, d.sum(1)


def bf16_rne(v):
    """Values that f32 holds exactly (asserted) -> the nearest bf16, ties to even."""
    f = v.to(F32)
    assert torch.equal(f.to(F64), f64(v)), "not representable in f32: the cast below would round twice"
    return f.to(BF16)


def scaled_f32(v, inv_keep):
    """The kernels' dropout scaling of an exactly held f32 value: ONE f32 multiply by the f32 ``inv_keep``."""
    f = v.to(F32)
    assert torch.equal(f.to(F64), f64(v))
    return f * torch.tensor(np.float32(inv_keep), dtype=F32, device=f.device)


def inv_keep_f32(p):
    """1 / (1 - p) as the entry points compute it: in f32 from the f32 p."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def thr16(p):
    """The keep threshold on 16 hash bits: (uint32)(p * 65536 + 0.5) in f32; an element is kept with probability 1 - thr16 / 65536."""
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


# ----------------------------------------------------------------------------------------------------- tier A: preconditions
def assert_exact(abs_sum):
    """``abs_sum``: the reference of the same operation on the operands' absolute values (sum |products| + |bias|, or sum_t |value| for
    column sums).  Below 2^24 every partial sum in any order is an integer that f32 holds."""
    m = float(abs_sum.max())
    assert m < EXACT, f"tier A precondition: a sum of magnitudes reaches {m:.0f} >= 2^24"


def rounding_shares(v):
    """-> (share of the values that are no bf16 numbers, share that lie exactly between two bf16 neighbours)."""
    r = f64(v).abs()
    _, e = torch.frexp(r)  # r = m 2^e, m in [0.5, 1): the bf16 spacing at r is 2^(e - 8)
    # 2^(8 - e) built from its exponent bits, exact on every device.  (torch.ldexp did not scale exactly there: on the MI355X this
    # function reported 100 % of the integers around 3000 of a K = 768 product as needing rounding and no tie, where the CPU counts 94 % and 6.7 %.)
    q = r * ((8 - e).to(torch.int64) + 1023 << 52).view(F64)
    frac = q - q.floor()
    return (frac != 0).double().mean().item(), (frac == 0.5).double().mean().item()


def assert_exercises_rounding(v, need=0.25, ties=0.01):
    got = rounding_shares(v)
    assert got[0] >= need and got[1] >= ties, f"tier A precondition: {got[0]:.3f} of the results need rounding, {got[1]:.4f} are ties"
    return got


# ----------------------------------------------------------------------------------------------------- tier A: operands
def ints(shape, lo, hi, gen):
    """Integers in [lo, hi] as bf16 (|value| <= 8: exact)."""
    assert -8 <= lo <= hi <= 8
    return torch.randint(lo, hi + 1, shape, generator=gen).to(BF16)


def int_range(n):
    """The operand range of a bias-free tier-A product of reduction length ``n``: the mean of the result, n * mean^2, and its spread
    put it between 2^8 and 2^14 (module docstring)."""
    if n <= 64:
        return 0, 8
    if n <= 128:
        return -2, 8
    if n <= 640:
        return -4, 8
    return -8, 8


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def tier_a_linear(T, K, N, bias, tag=0):
    """x [T, K], w [N, K] bf16 integers, bias f32 integers in [-4096, 4096] or None (CPU tensors).  With a bias |x|, |w| <= 4 and the
    bias spreads the results; without, ``int_range(K)``."""
    g = _gen(T, K, N, int(bias), tag, 1)
    lo, hi = (-4, 4) if bias else int_range(K)
    x, w = ints((T, K), lo, hi, g), ints((N, K), lo, hi, g)
    b = torch.randint(-4096, 4097, (N,), generator=g).to(F32) if bias else None
    return x, w, b


def tier_a_grad(T, K, N, tag=0):
    """dy [T, K], w2t [N, K] for the masked backward: integers in [-2, 2], so that the column sums of dz over 34 821 tokens stay exact."""
    g = _gen(T, K, N, tag, 2)
    return ints((T, K), -2, 2, g), ints((N, K), -2, 2, g)


def tier_a_dweight(T, N, K, slices, tag=0):
    """dy [T, N], x [T, K]: integers in ``int_range`` of the slice's token count."""
    g = _gen(T, N, K, slices, tag, 3)
    lo, hi = int_range(T // slices)
    return ints((T, N), lo, hi, g), ints((T, K), lo, hi, g)


# ----------------------------------------------------------------------------------------------------- tier B: operands, bound
def tier_b_rows(T, K, gen, mean):
    """[T, K] bf16: randn rows at scales 2^[-6, 3], shifted by ``mean``."""
    scale = torch.exp2(torch.randint(-6, 4, (T, 1), generator=gen).float())
    return (torch.randn(T, K, generator=gen) * scale + mean).to(BF16)


def tier_b_linear(T, K, N, tag=0):
    g = _gen(T, K, N, tag, 4)
    x = tier_b_rows(T, K, g, 0.3)
    w = (torch.randn(N, K, generator=g) / K ** 0.5 + 0.02).to(BF16)
    return x, w, torch.randn(N, generator=g)


def tier_b_dweight(T, N, K, tag=0):
    g = _gen(T, N, K, tag, 5)
    return (tier_b_rows(T, N, g, 0.16) / 8).to(BF16), tier_b_rows(T, K, g, 0.3)


def bound(ref, mag, n, half_ulp=True):
    """The per-element tier-B bound (module docstring).  ``mag``: the reference on the operands' absolute values; ``n``: the reduction
    length; ``half_ulp`` False for f32 outputs."""
    s = (n + 1) * 2.0 ** -23 * f64(mag)
    return (1 + 2.0 ** -8) * (2.0 ** -8 * f64(ref).abs() + s) if half_ulp else s


def rel(got, ref):
    return ((f64(got) - f64(ref)).norm() / f64(ref).norm().clamp_min(1e-300)).item()


# ----------------------------------------------------------------------------------------------------- acceptance
def _where(bad, got, want, shape):
    idx = bad.nonzero()
    lo, hi = idx.min(0).values.tolist(), idx.max(0).values.tolist()
    first = [(tuple(i.tolist()), float(got[tuple(i)]), float(want[tuple(i)])) for i in idx[:4]]
    span = ", ".join(f"axis {a}: {l}..{h}" for a, (l, h) in enumerate(zip(lo, hi)))
    return f"{idx.shape[0]} of {bad.numel()} elements of {tuple(shape)} ({span}); first (index, got, want): {first}"


def accept_exact(got, want, what):
    """Tier A: ``got`` equals ``want`` bit for bit (bf16 against bf16, f32 against the float64 result).  -> [] or [message]."""
    if tuple(got.shape) != tuple(want.shape):
        return [f"{what}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"]
    if got.dtype == BF16:
        assert want.dtype == BF16
        bad = got.contiguous().view(torch.int16) != want.contiguous().view(torch.int16)
    else:
        assert got.dtype == F32 and want.dtype == F64
        bad = ~(f64(got) == want)  # (a NaN is a mismatch)
    if not bad.any():
        return []
    return [f"{what}: not bit-equal in {_where(bad, got, want, got.shape)}"]


def accept_bound(got, ref, bnd, what, fig=None):
    """Tier B: every element within its bound of the float64 ``ref``, and the whole tensor within 4e-3.  -> [] or messages; ``fig``
    receives the worst error / bound and the whole-tensor error under ``what``."""
    err = (f64(got) - ref).abs()
    bad = ~(err <= bnd)
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.zeros_like(err)).max().item()
    whole = rel(got, ref)
    if fig is not None:
        fig[what] = dict(ratio=ratio, rel=whole)
    out = []
    if bad.any():
        out.append(f"{what}: beyond the bound (worst {ratio:.3f} x) in {_where(bad, f64(got), ref, got.shape)}")
    if not whole < REL_LIMIT:
        out.append(f"{what}: whole-tensor error {whole:.3e} >= {REL_LIMIT}")
    return out


def accept_dropout(y, expected, active, p, what):
    """``y`` (bf16) of a ReLU + dropout launch against ``expected`` (bf16: the kept value of every element): every element is 0 or
    exactly the expected value (so 0 wherever relu(ref) is 0), and the keep rate among the ``active`` elements is within 5 binomial
    standard deviations of 1 - thr16 / 65536."""
    yi, ei = y.contiguous().view(torch.int16), expected.contiguous().view(torch.int16)
    bad = (yi != ei) & (yi != 0)
    out = []
    if bad.any():
        out.append(f"{what}: neither 0 nor the expected value in {_where(bad, y, expected, y.shape)}")
    n, kept, pk = int(active.sum()), int(((yi != 0) & active).sum()), 1.0 - thr16(p) / 65536.0
    if abs(kept - n * pk) > 5.0 * (n * pk * (1 - pk)) ** 0.5:
        out.append(f"{what}: {kept} of {n} active elements kept, expected {n * pk:.1f} +- {(n * pk * (1 - pk)) ** 0.5:.1f}")
    return out
