"""The lookahead entry points (g2048_lookahead_expand / _children / _reduce): declared, bound, exported, their argument checks run
before any device work; the numpy restatement the GPU tests compare against is sane on its own.  CPU only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import lookahead_ref as R  # noqa: E402
from oracle import g2048_oracle as npo  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("g2048_lookahead_expand", "g2048_lookahead_children", "g2048_lookahead_reduce")


def test_symbols_are_declared_bound_and_exported():
    from src.g2048 import native as nv

    header = open(os.path.join(ROOT, "include", "g2048.h")).read()
    lib = C.CDLL(nv.LIB_PATH)
    for name in NAMES:
        assert f"int {name}(" in header
        assert name in nv.SIGNATURES
        assert hasattr(lib, name)
    assert "#define G2048_ABI_VERSION 4" in header
    assert nv.load().g2048_abi_version() == 4  # additive: the version stays
    for fn in ("lookahead_expand", "lookahead_children", "lookahead_reduce"):
        assert callable(getattr(nv, fn))


def test_entry_points_reject_bad_arguments_without_touching_a_device():
    from src.g2048 import native as nv

    lib = nv.load()
    a = 1 << 20  # a fake, 16-byte aligned "device address": must be rejected before any use
    assert lib.g2048_lookahead_expand(None, 8, a, a, a, None) == -1
    assert lib.g2048_lookahead_expand(a, 8, None, a, a, None) == -1
    assert lib.g2048_lookahead_expand(a, 0, a, a, a, None) == -1
    assert lib.g2048_lookahead_expand(a, (1 << 24) + 1, a, a, a, None) == -1
    assert lib.g2048_lookahead_expand(a + 4, 8, a, a, a, None) == -1
    assert lib.g2048_lookahead_expand(a, 8, a, a + 8, a, None) == -1
    assert lib.g2048_lookahead_children(None, a, a, 8, 16, a, a, None) == -1
    assert lib.g2048_lookahead_children(a, a, a, 0, 16, a, a, None) == -1
    assert lib.g2048_lookahead_children(a, a, a, 8, -1, a, a, None) == -1
    assert lib.g2048_lookahead_children(a, a, a, 8, 8 * 120 + 1, a, a, None) == -1   # more children than 8 boards can have
    assert lib.g2048_lookahead_children(a, a, a, 8, 16, None, a, None) == -1
    assert lib.g2048_lookahead_children(a, a, a, 8, 16, a + 8, a, None) == -1        # children not 16-byte aligned
    assert lib.g2048_lookahead_children(a, a, a, 8, 0, None, None, None) == 0        # nothing to write, nothing launched
    assert lib.g2048_lookahead_reduce(None, a, a, a, a, 0.99, 8, 16, a, None) == -1
    assert lib.g2048_lookahead_reduce(a, a, a, None, a, 0.99, 8, 16, a, None) == -1
    assert lib.g2048_lookahead_reduce(a, a, a, a, a, 0.99, 8, 16, None, None) == -1
    assert lib.g2048_lookahead_reduce(a, a, a, a + 4, a, 0.99, 8, 16, a, None) == -1  # values not 8-byte aligned
    assert lib.g2048_lookahead_reduce(a, a, a, a, a + 1, 0.99, 8, 16, a, None) == -1  # terminal not 2-byte aligned
    assert lib.g2048_lookahead_reduce(a, a, a, a, a, 0.99, 0, 16, a, None) == -1


def test_wrappers_refuse_host_tensors():
    import torch

    from src.g2048 import native as nv

    b = torch.zeros((4, 16), dtype=torch.uint8)
    with pytest.raises(nv.NativeError):
        nv.lookahead_expand(b, torch.zeros((4, 4, 16), dtype=torch.uint8), torch.zeros((4, 4)), torch.zeros((4, 4), dtype=torch.int32))


def test_depth_and_exports_without_a_device():
    from src.ppo import LookaheadActionFunction, PPOAgent, TorchActionFunction

    assert issubclass(LookaheadActionFunction, TorchActionFunction)
    agent = PPOAgent(hidden_dim=32, d_model=32, nhead=2, num_layers=1, dim_feedforward=64)
    fn = LookaheadActionFunction(agent)
    assert fn.use_mask and not fn.sample_actions and fn.depth == 1 and fn.gamma == 0.99 and fn.compact
    for depth in (0, 2, 3):
        with pytest.raises(ValueError):
            LookaheadActionFunction(agent, depth=depth)
    with pytest.raises(ValueError):
        LookaheadActionFunction(agent, max_children=0)


def test_numpy_restatement_is_sane():
    boards = np.concatenate([R.hand_made_boards(), npo.Runner(1, 1).run(8, "random")["boards"].reshape(-1, 16)])
    after, reward, nchild = R.expand(boards)
    children, terminal, offset = R.children(after, nchild)
    legal = npo.legal_mask(boards)
    assert np.array_equal(nchild > 0, legal)
    assert np.array_equal(nchild, np.where(legal, 2 * (after == 0).sum(axis=2), 0))  # children count is 2 * empties
    assert len(children) == nchild.sum() and nchild.max() <= 30 and (nchild % 2 == 0).all()
    # every child is its afterstate plus one tile 2 or 4 on a cell that was empty
    pair = np.repeat(np.arange(nchild.size), nchild.reshape(-1))
    diff = children != after.reshape(-1, 16)[pair]
    assert (diff.sum(axis=1) == 1).all()
    assert np.array_equal(children[diff], np.tile(np.array([1, 2], np.uint8), len(children) // 2))
    assert (after.reshape(-1, 16)[pair][diff] == 0).all()
    cells = diff.argmax(axis=1)
    same_pair = pair[1:] == pair[:-1]
    assert (np.diff(cells)[same_pair] >= 0).all() and np.array_equal(cells[0::2], cells[1::2])  # ascending cells, 2 before 4
    # the probabilities of the children of one (b, a) sum to 1
    p = R.spawn_probabilities(nchild)
    starts = offset.reshape(-1)[nchild.reshape(-1) > 0]
    np.testing.assert_allclose(np.add.reduceat(p, starts), 1.0, rtol=0, atol=1e-12)
    # Q with a constant value function: reward + gamma * c wherever no child is terminal; terminal children count as 0
    q = R.q_values(reward, nchild, offset, np.full(len(children), 2.0), np.zeros_like(terminal), 0.5, np.float64)
    np.testing.assert_allclose(q[nchild > 0], (reward + 1.0)[nchild > 0], rtol=1e-7)  # 0.9f + 0.1f is 1 + 2e-8
    assert (q[nchild == 0] == 0).all()
    q0 = R.q_values(reward, nchild, offset, np.full(len(children), 2.0), np.ones_like(terminal), 0.5, np.float64)
    assert np.array_equal(q0, np.where(nchild > 0, reward, 0.0))
    # the step the env would take: reward of a legal move equals the oracle's env_step reward
    a = legal.argmax(axis=1)
    keys = npo.split(npo.key(0), len(boards), 1)
    _, r, _, _ = npo.env_step(boards, legal, ~legal.any(axis=1), a, keys, 1)
    live = legal.any(axis=1)
    assert np.array_equal(r[live], reward[np.arange(len(boards)), a][live])
