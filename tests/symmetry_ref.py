"""numpy restatement of the canonical frame (include/g2048.h, "canonical frame"): the eight views of a board, the action map
that turns with them, the canonical representative and its frame.  Written from the definitions, not from the kernels:

  view_g(board) = np.rot90(T_f(board.reshape(4, 4)), k), g = 4 f + k, T_1 the transpose
  sigma_g(a)    = ((a ^ f) - k) mod 4                     (0 left, 1 up, 2 right, 3 down)
  canon(s)      = the view whose 16 bytes are lexicographically largest, frame(s) = the smallest g that attains it
"""
import numpy as np


def view(boards: np.ndarray, g: int) -> np.ndarray:
    """boards u8 [N,16] -> view_g of every board, [N,16]."""
    m = np.asarray(boards, np.uint8).reshape(-1, 4, 4)
    f, k = g >> 2, g & 3
    if f:
        m = m.transpose(0, 2, 1)
    return np.ascontiguousarray(np.rot90(m, k, axes=(1, 2))).reshape(-1, 16)


def sigma(g, a):
    """The action that does in view_g what ``a`` does in the env's frame (g, a: ints or arrays)."""
    g, a = np.asarray(g, np.int64), np.asarray(a, np.int64)
    return ((a ^ (g >> 2)) - (g & 3)) & 3


def canon(boards: np.ndarray):
    """-> (canonical boards u8 [N,16], frame u8 [N]).  Python's bytes compare as the definition does: from cell 0 upward."""
    boards = np.asarray(boards, np.uint8).reshape(-1, 16)
    views = np.stack([view(boards, g) for g in range(8)], axis=1)  # [N,8,16]
    out, frame = np.empty_like(boards), np.empty(len(boards), np.uint8)
    for i in range(len(boards)):
        keys = [views[i, g].tobytes() for g in range(8)]
        g = keys.index(max(keys))  # the first, hence smallest, g that attains the maximum
        out[i], frame[i] = views[i, g], g
    return out, frame


def perm_actions(actions: np.ndarray, frame: np.ndarray) -> np.ndarray:
    return sigma(frame, np.asarray(actions, np.int64) & 3).astype(np.uint8)


def perm_mask(masks: np.ndarray, frame: np.ndarray) -> np.ndarray:
    """Bit sigma_g(a) of the result = bit a of the env mask; high bits zero."""
    masks, frame = np.asarray(masks, np.int64), np.asarray(frame, np.int64)
    out = np.zeros(masks.shape, np.int64)
    for a in range(4):
        out |= ((masks >> a) & 1) << sigma(frame, a)
    return out.astype(np.uint8)


def logits_back(logits: np.ndarray, frame: np.ndarray) -> np.ndarray:
    """logits_env[b][a] = logits_canon[b][sigma_frame[b](a)] (any 4-column array; elements are moved, not recomputed)."""
    idx = sigma(np.asarray(frame, np.int64)[:, None] & 7, np.arange(4)[None, :])
    return np.take_along_axis(np.asarray(logits), idx, axis=1)


def stabiliser_is_trivial(boards: np.ndarray) -> np.ndarray:
    """True where the 8 views are pairwise distinct."""
    boards = np.asarray(boards, np.uint8).reshape(-1, 16)
    views = np.stack([view(boards, g) for g in range(8)], axis=1)
    return np.array([len({views[i, g].tobytes() for g in range(8)}) == 8 for i in range(len(boards))])


def hand_made_boards() -> np.ndarray:
    b = np.zeros((9, 16), np.uint8)
    # 0: empty.  1: all cells equal
    b[1] = 3
    # 2: transpose-symmetric
    b[2] = np.array([[5, 1, 2, 0], [1, 4, 3, 0], [2, 3, 0, 1], [0, 0, 1, 2]], np.uint8).reshape(-1)
    # 3: 180-degree-symmetric
    b[3] = np.array([[1, 2, 3, 4], [5, 6, 7, 0], [0, 7, 6, 5], [4, 3, 2, 1]], np.uint8).reshape(-1)
    # 4: equal maxima in two corners (the rest decides).  5: in four corners
    b[4] = np.array([[9, 1, 0, 9], [2, 0, 0, 3], [0, 0, 1, 0], [1, 0, 0, 2]], np.uint8).reshape(-1)
    b[5] = np.array([[9, 1, 2, 9], [0, 3, 0, 1], [1, 0, 0, 0], [9, 0, 4, 9]], np.uint8).reshape(-1)
    # 6: one tile in the centre 2x2.  7: a two-tile opening board on a diagonal.  8: a large tile (2^17) off the corners
    b[6, 5] = 1
    b[7, 0], b[7, 15] = 1, 2
    b[8] = np.array([[1, 17, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15]], np.uint8).reshape(-1)
    return b


def random_boards(n: int, seed: int = 0) -> np.ndarray:
    """Mixed fill: every board draws its own share of empty cells, so sparse openings and full boards both occur."""
    rng = np.random.default_rng(seed)
    vals = rng.integers(1, 12, size=(n, 16))
    fill = rng.uniform(0.05, 1.0, size=(n, 1))
    return np.where(rng.random((n, 16)) < fill, vals, 0).astype(np.uint8)


def test_boards() -> np.ndarray:
    """The hand-made symmetric boards, a few hundred random ones, and all eight views of each (u8 [N,16])."""
    base = np.concatenate([hand_made_boards(), random_boards(300, seed=2048)])
    return np.concatenate([view(base, g) for g in range(8)])


test_boards.__test__ = False  # a helper with a pytest-looking name
