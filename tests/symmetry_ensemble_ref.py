"""numpy restatement of the eight-view ensemble (include/g2048.h, "eight-view ensemble").  Written from the definitions, not from the
kernels:

  views(boards)[b][g] = view_g(boards[b])                                 rows r = 8 b + g of one forward
  L(s)[a] = 1/8 sum_g logits[8 b + g][sigma_g(a)],  V(s) = 1/8 sum_g values[8 b + g]
  the sum: the eight addends sorted by the total order of their f32 bit patterns (-NaN < -inf < .. < -0 < +0 < .. < +inf < +NaN),
  added in ascending order, every add rounded to f32 on its own; then times 0.125 in f32
"""
import numpy as np

import symmetry_ref as R

# view_g(view_h(s)) = view_c(s) and sigma_g(sigma_h(a)) = sigma_c(a) with c = TAB[h][g]
TAB = np.array([[0, 1, 2, 3, 4, 5, 6, 7],
                [1, 2, 3, 0, 7, 4, 5, 6],
                [2, 3, 0, 1, 6, 7, 4, 5],
                [3, 0, 1, 2, 5, 6, 7, 4],
                [4, 5, 6, 7, 0, 1, 2, 3],
                [5, 6, 7, 4, 3, 0, 1, 2],
                [6, 7, 4, 5, 2, 3, 0, 1],
                [7, 4, 5, 6, 1, 2, 3, 0]], np.int64)


def views(boards: np.ndarray) -> np.ndarray:
    """boards u8 [B,16] -> u8 [B,8,16], [b][g] = view_g(boards[b])."""
    boards = np.asarray(boards, np.uint8).reshape(-1, 16)
    return np.ascontiguousarray(np.stack([R.view(boards, g) for g in range(8)], axis=1))


def sort_key(bits: np.ndarray) -> np.ndarray:
    """f32 bit patterns (u32) -> u32 keys whose unsigned order is the total order of the patterns."""
    bits = np.asarray(bits, np.uint32)
    return bits ^ np.where(bits >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def sort_unkey(key: np.ndarray) -> np.ndarray:
    key = np.asarray(key, np.uint32)
    return key ^ np.where(key >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))


def ordered_mean8(bits: np.ndarray) -> np.ndarray:
    """u32 [..., 8] -> u32 [...]: the eight f32 added in the order they lie, each add rounded to f32, times 0.125."""
    x = np.ascontiguousarray(bits, np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        s = x[..., 0].copy()
        for i in range(1, 8):
            s = (s + x[..., i]).astype(np.float32)  # f32 + f32 in numpy is one IEEE add
        s = (s * np.float32(0.125)).astype(np.float32)
    return np.ascontiguousarray(s).view(np.uint32)


def sorted_mean8(bits: np.ndarray) -> np.ndarray:
    """u32 [..., 8] (f32 bit patterns) -> u32 [...]: the mean as a function of the multiset of the eight."""
    keys = np.sort(sort_key(bits), axis=-1)
    return ordered_mean8(sort_unkey(keys))


def gather(logit_bits: np.ndarray) -> np.ndarray:
    """u32 [8 B,4] in the row order of views() -> u32 [B,4,8]: [b][a][g] = logits[8 b + g][sigma_g(a)]."""
    x = np.asarray(logit_bits, np.uint32).reshape(-1, 8, 4)
    idx = R.sigma(np.arange(8)[:, None], np.arange(4)[None, :])  # [g][a]
    return np.stack([x[:, np.arange(8), idx[:, a]] for a in range(4)], axis=1)


def fold(logit_bits=None, value_bits=None, mean8=sorted_mean8):
    """-> (u32 [B,4] or None, u32 [B] or None).  ``mean8=ordered_mean8`` is the g-ordered sum the kernel must NOT compute."""
    out_l = None if logit_bits is None else mean8(gather(logit_bits))
    out_v = None if value_bits is None else mean8(np.asarray(value_bits, np.uint32).reshape(-1, 8))
    return out_l, out_v


SPECIALS = np.array([0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x7FC00001, 0xFFFFFFFF, 0x00000001, 0x3F800000,
                     0x80000001, 0x007FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800001, 0xFFC00000], np.uint32)


def test_patterns(n: int, seed: int = 0) -> np.ndarray:
    """u32 [n, 8]: a third random bit patterns (NaNs and denormals among them), a third finite data across 60 binades with mixed
    signs (where the order of the adds shows), a third all-finite rows with specials (+-inf, +-0, NaNs, denormals, +-max, 1.0)
    planted at random places; every special kind appears even for small n."""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    third = n // 3
    fin = (rng.standard_normal((n - third, 8)) * np.exp2(rng.integers(-30, 30, (n - third, 8)))).astype(np.float32)
    out[third:] = fin.view(np.uint32)
    for i in range(2 * third, n):
        k = rng.integers(1, 4)
        out[i, rng.choice(8, k, replace=False)] = SPECIALS[(i + np.arange(k)) % len(SPECIALS)]
    return out


test_patterns.__test__ = False  # a helper with a pytest-looking name


def is_nan(bits: np.ndarray) -> np.ndarray:
    bits = np.asarray(bits, np.uint32)
    return (bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def assert_same_bits(got: np.ndarray, want: np.ndarray, what=""):
    """Bits where the restatement is not NaN, NaN-ness where it is (the payload is unspecified)."""
    got, want = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = is_nan(want)
    assert np.array_equal(is_nan(got), nan), what
    assert np.array_equal(got[~nan], want[~nan]), what
