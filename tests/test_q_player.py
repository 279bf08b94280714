"""The host-side parts the score players share: the one rng-mode resolver, QPlayer's masked max bit for bit, and that the one-ply,
two-ply, Monte-Carlo and n-tuple players take their un-batched protocol from QPlayer and nowhere else.  CPU only."""
import numpy as np
import pytest
import torch

from src.actions import _common as C
from src.g2048 import native as nv
from src.ppo import (ExpectimaxActionFunction, LookaheadActionFunction, MonteCarloActionFunction, NTupleActionFunction,
                     TorchActionFunction, expectimax, lookahead, monte_carlo, ntuple)
from src.ppo.q_player import QPlayer
from src.runs import batch_runner

PLAYERS = (LookaheadActionFunction, ExpectimaxActionFunction, MonteCarloActionFunction, NTupleActionFunction)


@pytest.mark.parametrize("env,want", [(None, nv.RNG_PARTITIONABLE), ("legacy", nv.RNG_LEGACY), ("LEGACY", nv.RNG_LEGACY),
                                      ("0", nv.RNG_LEGACY)])
def test_none_asks_the_environment(monkeypatch, env, want):
    if env is None:
        monkeypatch.delenv("G2048_RNG_MODE", raising=False)
    else:
        monkeypatch.setenv("G2048_RNG_MODE", env)
    assert C.resolve_rng_mode(None) == want and C.resolve_rng_mode() == want
    assert type(C.resolve_rng_mode(None)) is int


def test_spellings_and_ints(monkeypatch):
    monkeypatch.setenv("G2048_RNG_MODE", "legacy")  # an explicit argument wins over the environment
    assert (nv.RNG_LEGACY, nv.RNG_PARTITIONABLE) == (0, 1)
    for given, want in (("legacy", 0), ("partitionable", 1), ("0", 0), ("1", 1), ("Legacy", 0), ("PARTITIONABLE", 1), (0, 0), (1, 1),
                        (np.int64(1), 1)):
        got = C.resolve_rng_mode(given)
        assert got == want and type(got) is int, given


@pytest.mark.parametrize("bad", ["threefry", "", "2", "partitionable ", "legacy1"])
def test_unknown_spellings_raise(monkeypatch, bad):
    monkeypatch.delenv("G2048_RNG_MODE", raising=False)
    with pytest.raises(ValueError, match="rng_mode"):
        C.resolve_rng_mode(bad)
    monkeypatch.setenv("G2048_RNG_MODE", bad)
    with pytest.raises(ValueError, match="rng_mode"):
        C.resolve_rng_mode(None)
    assert C.resolve_rng_mode("legacy") == nv.RNG_LEGACY  # (the environment is not asked when an argument is given)


def test_every_caller_resolves_through_the_same_function(monkeypatch):
    assert batch_runner.resolve_rng_mode is C.resolve_rng_mode
    assert not hasattr(batch_runner, "_resolve_rng_mode") and not hasattr(C, "default_rng_mode")
    monkeypatch.delenv("G2048_RNG_MODE", raising=False)
    net = ntuple.NTupleNetwork(((0, 1),), device="cpu")
    for cls, args in ((MonteCarloActionFunction, ()), (NTupleActionFunction, (net,))):
        assert cls(*args, rng_mode="legacy")._rng_mode() == nv.RNG_LEGACY
        assert cls(*args, rng_mode="1")._rng_mode() == nv.RNG_PARTITIONABLE
        assert cls(*args)._rng_mode() == nv.RNG_PARTITIONABLE
        with pytest.raises(ValueError):  # used to mean "partitionable" in these two classes
            cls(*args, rng_mode="legacyy")._rng_mode()
    with pytest.raises(ValueError):
        ntuple.NTupleTrainer(net, num_envs=4, rng_mode="legacyy", device="cpu")


def _bits(x):
    return x.view(torch.int32)


def test_best_legal_keeps_the_bits():
    neg0 = -0.0
    q = torch.tensor([[5.0, -3.0, 2.0, 9.0],          # no legal action -> +0.0
                      [-4.0, -1.5, -8.0, -2.0],       # all q negative
                      [1.0, 100.0, 3.0, 2.0],         # the illegal action is larger than every legal one
                      [-7.0, neg0, -1.0, 50.0],       # the best legal q is -0.0
                      [neg0, neg0, neg0, neg0],       # nothing but -0.0, none legal: still +0.0
                      [3.0, 4.0, 6.0, 5.0],           # a single legal action
                      [float("-inf"), 1e30, -1e30, 0.0]], dtype=torch.float32)
    legal = torch.tensor([[0, 0, 0, 0], [1, 1, 1, 1], [1, 0, 1, 1], [1, 1, 1, 0], [0, 0, 0, 0], [0, 1, 0, 0], [1, 0, 1, 0]],
                         dtype=torch.bool)
    v = torch.where(legal, q, torch.full_like(q, float("-inf"))).max(dim=1).values
    want = torch.where(legal.any(dim=1), v, torch.zeros_like(v))
    got = QPlayer.best_legal(q, legal)
    assert got.dtype == torch.float32 and got.shape == (7,)
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(got), _bits(torch.tensor([0.0, -1.5, 3.0, neg0, 0.0, 4.0, -1e30])))
    assert _bits(got)[0].item() == 0 and _bits(got)[4].item() == 0 and _bits(got)[3].item() == -(1 << 31)  # +0, +0, -0


def test_the_players_share_one_unbatched_protocol():
    for cls in PLAYERS:
        assert issubclass(cls, QPlayer) and cls.__call__ is QPlayer.__call__, cls
        assert cls.best_legal is QPlayer.best_legal and cls._rng_mode is QPlayer._rng_mode
        for name in ("__call__", "_mode", "_rng_mode", "best_legal", "use_mask", "sample_actions"):
            assert name not in vars(cls), (cls, name)
        assert cls.use_mask is True and cls.sample_actions is False
        assert cls.policy_fn.needs_masks is False
    assert LookaheadActionFunction.__mro__[1:3] == (QPlayer, TorchActionFunction)
    assert TorchActionFunction.__call__ is not QPlayer.__call__ and not issubclass(TorchActionFunction, QPlayer)
    for mod in (lookahead, expectimax, monte_carlo, ntuple):
        assert not hasattr(mod, "_mode") and not hasattr(mod, "default_rng_mode"), mod
    assert set(vars(QPlayer)) - {"__module__", "__dict__", "__weakref__", "__doc__", "__qualname__", "__firstlineno__",
                                 "__static_attributes__"} == {"use_mask", "sample_actions", "_rng_mode", "best_legal", "__call__"}
