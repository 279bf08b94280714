"""QPlayer.__call__ on the device: for the n-tuple, two-ply and Monte-Carlo players the un-batched protocol, with and without a
leading batch dimension, plays the masked argmax of ``policy_fn``'s q and returns its v bit for bit (the one-ply player has this
test in test_gpu_lookahead.py); an rng mode given as a string works in ``__call__``."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

import ntuple_ref as N  # noqa: E402
from oracle import g2048_oracle as npo  # noqa: E402
from src.ppo import (ExpectimaxActionFunction, LookaheadActionFunction, MonteCarloActionFunction, NTupleActionFunction,  # noqa: E402
                     NTupleNetwork)
from test_gpu_lookahead2 import GAMMA, TableCritic  # noqa: E402
from weights_recipe import sample_boards  # noqa: E402

pytestmark = pytest.mark.gpu
TUPLES = ((0, 1, 2), (5, 6, 10))  # m = 2 tuples of L = 3 cells


@pytest.fixture(scope="module")
def inputs():
    """16 boards with at least one legal move each, their masks, one-hot observations and keys; left unchanged."""
    boards = sample_boards(24, seed=3)
    boards = boards[npo.legal_mask(boards).any(axis=1)][:16]
    assert len(boards) == 16
    masks = npo.legal_mask(boards)
    assert 0 < (~masks).sum()  # some moves are illegal: the mask matters
    return dict(boards=boards, masks=masks, obs=npo.observation(boards), keys=np.stack([npo.key(i) for i in range(16)]))


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _scores(fn, boards_np, dev):
    q, v = fn.policy_fn(torch.from_numpy(boards_np).to(dev), None)
    return q.cpu().numpy(), v.cpu().numpy()


def _check_batched(out, q, v, masks):
    a, lp, val = out
    assert a.shape == lp.shape == val.shape == (len(q),) and a.dtype == np.int32
    assert np.array_equal(a, np.where(masks, q, -np.inf).argmax(axis=1))  # (numpy: the first maximum, as in the kernel)
    assert np.array_equal(_bits(val), _bits(v)) and np.isfinite(lp).all()


def _check_single(out, q_row, v_i, mask):
    a, lp, val = out
    assert isinstance(a, np.int32) and isinstance(lp, np.float32) and isinstance(val, np.float32)
    assert int(a) == int(np.where(mask, q_row, -np.inf).argmax()) and _bits(val) == _bits(v_i) and np.isfinite(lp)


def _check_stateless_player(fn, inputs, dev):
    q, v = _scores(fn, inputs["boards"], dev)
    for i in range(16):
        _check_single(fn(inputs["keys"][i], inputs["obs"][i], inputs["masks"][i]), q[i], v[i], inputs["masks"][i])
    _check_batched(fn(inputs["keys"], inputs["obs"], inputs["masks"]), q, v, inputs["masks"])


def test_ntuple_player(dev, inputs):
    net = NTupleNetwork(TUPLES, device=dev)
    net.weights.copy_(torch.from_numpy(N.random_weights(TUPLES, seed=4)).to(dev))
    _check_stateless_player(NTupleActionFunction(net, device=dev), inputs, dev)


def test_two_ply_player(dev, inputs):
    fn = ExpectimaxActionFunction(TableCritic().to(dev), gamma=GAMMA, device=dev)
    assert fn.plies == 2 and fn.dedup
    _check_stateless_player(fn, inputs, dev)


def test_monte_carlo_player(dev, inputs):
    """Every call advances the player's own key chain, so what is compared are players built with the same seed."""
    new = lambda: MonteCarloActionFunction(None, playouts=2, depth=4, playout_policy="drul", seed=6, device=dev)
    q, v = _scores(new(), inputs["boards"], dev)
    assert (q != 0).any()
    _check_batched(new()(inputs["keys"], inputs["obs"], inputs["masks"]), q, v, inputs["masks"])
    q1, v1 = _scores(new(), inputs["boards"][:1], dev)
    _check_single(new()(inputs["keys"][0], inputs["obs"][0], inputs["masks"][0]), q1[0], v1[0], inputs["masks"][0])


def test_a_string_mode_works_in_call(dev, inputs):
    critic = TableCritic().to(dev)
    k, o, m = inputs["keys"], inputs["obs"], inputs["masks"]
    want = LookaheadActionFunction(critic, gamma=GAMMA, device=dev, rng_mode=0)(k, o, m)
    got = LookaheadActionFunction(critic, gamma=GAMMA, device=dev, rng_mode="legacy")(k, o, m)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    one = LookaheadActionFunction(critic, gamma=GAMMA, device=dev, rng_mode="legacy")(k[0], o[0], m[0])
    assert int(one[0]) == int(want[0][0]) and _bits(one[1]) == _bits(want[1][0]) and _bits(one[2]) == _bits(want[2][0])
    with pytest.raises(ValueError, match="rng_mode"):
        LookaheadActionFunction(critic, device=dev, rng_mode="legacyy")(k, o, m)
