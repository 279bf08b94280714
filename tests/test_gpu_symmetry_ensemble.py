"""Eight-view ensemble on the GPU: the two kernels bit-exact against the numpy restatement (tests/symmetry_ensemble_ref.py), the
fold blind to the order of a board's rows, the wrappers exactly what they are made of, a slot-independent agent exactly
equivariant under them, chunked search equal to unchunked, and whole evaluations that obey the env."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import symmetry_ensemble_ref as E  # noqa: E402
import symmetry_ref as R  # noqa: E402
from oracle import g2048_oracle as npo  # noqa: E402
from src.g2048 import native as nv  # noqa: E402
from src.ppo import LookaheadActionFunction, PPOAgent, TorchActionFunction  # noqa: E402
from src.runs import BatchRunner, evaluate_agent  # noqa: E402

pytestmark = pytest.mark.gpu
# views: one lane per row, 8 B rows: a partial wave (1, 7), exactly one wave of rows (8), one more (9), partial workgroups, several.
# fold: one lane per board: the same numbers are a partial wave, one wave (64), one more, a workgroup and a bit, seventeen workgroups
SIZES = (1, 7, 8, 9, 63, 64, 65, 257, 4099)
GUARD = 0xA5
GUARD_F32 = -7.0


def _to_f32(bits, dev):
    """u32 numpy -> f32 device tensor with those bit patterns."""
    return torch.from_numpy(np.array(bits, np.uint32).view(np.int32)).to(dev).view(torch.float32)


def _bits_of(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def ref():
    """The restatement, computed once for the longest input and shared (a prefix of the rows folds to a prefix of the result)."""
    n = max(SIZES)
    tb = R.test_boards()
    boards = tb[np.arange(n) % len(tb)]
    # the eight addends of every output are one row of test_patterns(): random patterns, finite data across 60 binades, specials
    addends = E.test_patterns(4 * n, seed=21).reshape(n, 4, 8)
    idx = R.sigma(np.arange(8)[:, None], np.arange(4)[None, :])  # [g][a]
    logits = np.empty((n, 8, 4), np.uint32)
    for a in range(4):
        logits[:, np.arange(8), idx[:, a]] = addends[:, a, :]
    logits = logits.reshape(8 * n, 4)
    assert np.array_equal(E.gather(logits), addends)
    values = E.test_patterns(n, seed=22).reshape(8 * n)
    fold_l, fold_v = E.fold(logits, values)
    assert E.is_nan(fold_l).any() and E.is_nan(fold_v).any() and not E.is_nan(fold_l).all()
    out = dict(boards=boards, views=E.views(boards), logits=logits, values=values, fold_logits=fold_l, fold_values=fold_v)
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("B", SIZES)
def test_sym_views_is_bit_exact(dev, ref, B):
    boards = torch.from_numpy(ref["boards"][:B].copy()).to(dev)
    out = torch.full((8 * B + 64, 16), GUARD, dtype=torch.uint8, device=dev)
    nv.sym_views(boards, out[:8 * B])
    assert np.array_equal(out[:8 * B].cpu().numpy().reshape(B, 8, 16), ref["views"][:B])
    assert (out[8 * B:] == GUARD).all()                               # rows at or past 8 B are not touched
    assert np.array_equal(boards.cpu().numpy(), ref["boards"][:B])    # the input is read only
    shaped = torch.empty((B, 8, 16), dtype=torch.uint8, device=dev)   # the [B][8][16] spelling of the same buffer
    nv.sym_views(boards, shaped)
    assert torch.equal(shaped.view(8 * B, 16), out[:8 * B])


@pytest.mark.parametrize("B", SIZES)
def test_sym_fold_is_bit_exact(dev, ref, B):
    logits, values = _to_f32(ref["logits"][:8 * B], dev), _to_f32(ref["values"][:8 * B], dev)
    for with_logits, with_values in ((True, False), (False, True), (True, True)):
        ol = torch.full((B + 64, 4), GUARD_F32, dtype=torch.float32, device=dev)
        ov = torch.full((B + 64,), GUARD_F32, dtype=torch.float32, device=dev)
        nv.sym_fold(logits if with_logits else None, values if with_values else None, ol[:B] if with_logits else None,
                    ov[:B] if with_values else None)
        if with_logits:
            E.assert_same_bits(_bits_of(ol[:B]), ref["fold_logits"][:B], "logits")
            assert (ol[B:] == GUARD_F32).all()
        else:
            assert (ol == GUARD_F32).all()  # an output that was not asked for is not written
        if with_values:
            E.assert_same_bits(_bits_of(ov[:B]), ref["fold_values"][:B], "values")
            assert (ov[B:] == GUARD_F32).all()
        else:
            assert (ov == GUARD_F32).all()
    assert np.array_equal(_bits_of(logits), ref["logits"][:8 * B]) and np.array_equal(_bits_of(values), ref["values"][:8 * B])


def test_sym_fold_does_not_see_the_order_of_a_boards_rows(dev, ref):
    """Seen from view_h(s) the forward's rows are the rows of s in the order tab[h], and the result is asked for at sigma_h(a):
    the device returns the same bits for all h, NaN payloads included (equal keys are equal patterns, so the sorted sequence and
    hence every add is the same)."""
    B = 257
    lg = ref["logits"][:8 * B].reshape(B, 8, 4)
    vl = ref["values"][:8 * B].reshape(B, 8)
    base_l = torch.empty((B, 4), dtype=torch.float32, device=dev)
    base_v = torch.empty(B, dtype=torch.float32, device=dev)
    nv.sym_fold(_to_f32(lg.reshape(-1, 4), dev), _to_f32(vl.reshape(-1), dev), base_l, base_v)
    for h in range(1, 8):
        ol, ov = torch.empty_like(base_l), torch.empty_like(base_v)
        nv.sym_fold(_to_f32(lg[:, E.TAB[h]].reshape(-1, 4), dev), _to_f32(vl[:, E.TAB[h]].reshape(-1), dev), ol, ov)
        idx = torch.from_numpy(R.sigma(h, np.arange(4))).to(dev)
        assert torch.equal(ol[:, idx].view(torch.int32), base_l.view(torch.int32)), h
        assert torch.equal(ov.view(torch.int32), base_v.view(torch.int32)), h


# ---------------------------------------------------------------------------------------------- the wrappers
def _perturb(agent):
    with torch.no_grad():
        for p in agent.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.05)  # non-trivial biases / LayerNorm affine
    return agent


def _check_composition(agent, dev, **kw):
    """policy_fn / _values under the mode == the restated fold of the unchanged forward on the restated views, bit for bit."""
    S = R.test_boards()[:96]  # the hand-made symmetric boards come first
    views = torch.from_numpy(E.views(S).reshape(-1, 16)).to(dev)
    fn = TorchActionFunction(agent, use_mask=True, device=dev, symmetry="ensemble", **kw)
    inner_l, inner_v = fn._policy(views)
    assert inner_l.shape == (768, 4) and torch.isfinite(inner_l).all()
    want_l, want_v = E.fold(_bits_of(inner_l.float()), _bits_of(inner_v.float().reshape(-1)))
    got_l, got_v = fn.policy_fn(torch.from_numpy(S).to(dev), None)
    assert got_l.shape == (96, 4) and got_v.shape == (96,) and got_l.dtype == got_v.dtype == torch.float32
    assert np.array_equal(_bits_of(got_l), want_l) and np.array_equal(_bits_of(got_v), want_v)
    assert len(np.unique(want_v)) > 8  # a forward that tells boards apart
    la = LookaheadActionFunction(agent, device=dev, symmetry="ensemble", **kw)
    assert (la._fused is None) == (fn._fused is None)
    want = E.fold(None, _bits_of(la._policy(views)[1].float().reshape(-1)))[1]  # (read back before the next forward runs)
    got = la._values(torch.from_numpy(S).to(dev))
    assert got.shape == (96,) and np.array_equal(_bits_of(got), want)
    return fn


@pytest.mark.parametrize("reduction", ["cls", "mean"])
def test_fused_wrapper_is_views_forward_fold(dev, reduction):
    torch.manual_seed(0)
    agent = _perturb(PPOAgent(hidden_dim=512, d_model=256, nhead=8, num_layers=2, dim_feedforward=1024, reduction=reduction))
    fn = _check_composition(agent, dev, amp_dtype=torch.bfloat16)
    assert fn._fused is not None


def test_module_wrapper_is_views_forward_fold(dev):
    torch.manual_seed(0)
    agent = _perturb(PPOAgent(hidden_dim=32, d_model=32, nhead=4, num_layers=1, dim_feedforward=64, dropout=0.0))
    fn = _check_composition(agent, dev, use_fused=False)
    assert fn._fused is None


class _CellwiseAgent(torch.nn.Module):
    """A stand-in actor-critic made of elementwise torch operators only, so that its output for a row cannot depend on the slot the
    row sits in (which the fused encoder does not promise for moved slots): per output, sixteen terms (x_c w + b) x_c of the
    cells added one after the other.  Position-dependent weights: it is NOT equivariant by itself."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.w = torch.nn.Parameter(torch.randn(5, 16, generator=g))
        self.b = torch.nn.Parameter(torch.randn(5, 16, generator=g))

    def forward(self, boards, action_mask=None):
        x = boards.reshape(-1, 16).to(torch.float32)
        outs = []
        for j in range(5):
            s = (x[:, 0] * self.w[j, 0] + self.b[j, 0]) * x[:, 0]
            for c in range(1, 16):
                s = s + (x[:, c] * self.w[j, c] + self.b[j, c]) * x[:, c]
            outs.append(s)
        return torch.stack(outs[:4], dim=1), outs[4].reshape(-1, 1)


def test_slot_independent_agent_is_exactly_equivariant(dev):
    tb = R.test_boards()
    n = len(tb) // 8
    m = 40  # boards 0 .. 8 are the hand-made ones, six of them self-symmetric
    fn = TorchActionFunction(_CellwiseAgent(), use_mask=True, device=dev, symmetry="ensemble")
    plain = TorchActionFunction(_CellwiseAgent(), use_mask=True, device=dev, symmetry="none")
    base_l, base_v = (x.clone() for x in fn.policy_fn(torch.from_numpy(tb[:m]).to(dev), None))
    assert torch.isfinite(base_l).all()
    # four different logits on most boards (not on self-symmetric ones, the empty board among them): a wrong permutation shows
    assert (base_l.max(dim=1).values > base_l.min(dim=1).values).float().mean() > 0.5
    p0 = plain.policy_fn(torch.from_numpy(tb[:m]).to(dev), None)[1].clone()
    for h in range(1, 8):
        Sh = torch.from_numpy(tb[h * n:h * n + m]).to(dev)  # view_h of the same boards
        l, v = fn.policy_fn(Sh, None)
        idx = torch.from_numpy(R.sigma(h, np.arange(4))).to(dev)
        assert torch.equal(l[:, idx].view(torch.int32), base_l.view(torch.int32)), h  # l[:, sigma_h(a)] == base[:, a], bit for bit
        assert torch.equal(v.view(torch.int32), base_v.view(torch.int32)), h
        assert not torch.equal(plain.policy_fn(Sh, None)[1], p0)  # the agent itself is not invariant
    # the un-batched protocol goes down policy_fn: the greedy move turns with the board
    greedy = TorchActionFunction(_CellwiseAgent(), use_mask=True, sample_actions=False, device=dev, symmetry="ensemble")
    # (on boards without a symmetry of their own: on the others exact equivariance makes logits equal, and the argmax's first-index
    # tie-break does not turn with the board)
    pick = 9 + np.flatnonzero(R.stabiliser_is_trivial(tb[9:m]))[:8]
    assert len(pick) == 8
    S = tb[pick]
    key = np.tile(npo.key(5), (8, 1))
    a0, _, v0 = greedy(key, npo.observation(S), npo.legal_mask(S))
    Sh = R.view(S, 6)
    a6, _, v6 = greedy(key, npo.observation(Sh), npo.legal_mask(Sh))
    assert np.array_equal(a6, R.sigma(6, a0)) and np.array_equal(v6, v0)
    assert np.array_equal(v0.view(np.uint32), _bits_of(base_v)[pick])


def test_lookahead_chunks_hold_boards_and_do_not_change_a_bit(dev):
    S = torch.from_numpy(R.random_boards(48, seed=12)).to(dev)
    agent = _CellwiseAgent()
    whole = LookaheadActionFunction(agent, device=dev, symmetry="ensemble")
    chunked = LookaheadActionFunction(agent, device=dev, max_children=64, symmetry="ensemble")  # 64 forward rows: 8 boards a chunk
    plain = LookaheadActionFunction(agent, device=dev, symmetry="none")
    calls = []
    inner = chunked._policy
    chunked._policy = lambda rows: (calls.append(rows.shape[0]), inner(rows))[1]
    q0, v0 = whole.policy_fn(S)
    q1, v1 = chunked.policy_fn(S)
    plain.policy_fn(S)
    N = plain.last_children
    assert N > 64 and whole.last_children == N and chunked.last_children == N  # boards, not forward rows
    assert max(calls) == 64 and sum(calls) == 8 * N and len(calls) == -(-N // 8)
    assert torch.equal(q1.view(torch.int32), q0.view(torch.int32)) and torch.equal(v1.view(torch.int32), v0.view(torch.int32))
    assert torch.isfinite(q0).all() and q0.shape == (48, 4)


# ---------------------------------------------------------------------------------------------- whole evaluations
def _tiny_agent():
    torch.manual_seed(0)
    return _perturb(PPOAgent(hidden_dim=32, d_model=32, nhead=4, num_layers=1, dim_feedforward=64, dropout=0.0))


def _bits(legal):
    return (legal.astype(np.uint8) * np.array([1, 2, 4, 8], np.uint8)).sum(axis=1).astype(np.uint8)


@pytest.mark.parametrize("search", [dict(), dict(lookahead=1)], ids=["greedy", "one_ply"])
def test_evaluate_agent_runs_under_the_mode(dev, search):
    ev = evaluate_agent(_tiny_agent(), dev, 8, seed=42, symmetry="ensemble", **search)
    assert set(ev) == {"episodes", "mean_max_tile", "counts", "percent", "mean_episode_length"}
    assert ev["episodes"] == 8 and sum(ev["counts"].values()) == 8
    assert ev["mean_max_tile"] >= 4 and ev["mean_episode_length"] > 10
    assert all(k & (k - 1) == 0 for k in ev["counts"])


def test_env_and_key_stream_are_untouched(dev):
    fn = TorchActionFunction(_tiny_agent(), use_mask=True, sample_actions=False, device=dev, symmetry="ensemble")
    traj = BatchRunner(init_seed=3, act_fn=fn, device=dev).collect(8)
    final = traj.final_boards.cpu().numpy()
    assert final.shape == (8, 16) and not npo.legal_mask(final).any()  # every episode was played to its end
    keep = np.arange(traj.T)[None, :] < traj.ep_len.cpu().numpy()[:, None]
    env_major = lambda x: np.swapaxes(x.cpu().numpy(), 0, 1)[keep]
    boards, actions, masks, rewards = (env_major(x) for x in (traj.boards, traj.actions, traj.masks, traj.rewards))
    assert len(boards) == int(traj.ep_len.sum()) > 8 * 10
    assert np.array_equal(masks, _bits(npo.legal_mask(boards)))  # the env-frame trajectory obeys the oracle
    assert ((masks >> actions) & 1).all()                        # masked argmax of env-frame logits: always a legal move
    assert np.array_equal(rewards, npo.move(boards, actions.astype(np.int32))[1])
    # the same seed without the mode starts from the same boards: the mode draws nothing from the key stream
    plain = TorchActionFunction(_tiny_agent(), use_mask=True, sample_actions=False, device=dev, symmetry="none")
    traj0 = BatchRunner(init_seed=3, act_fn=plain, device=dev).collect(8)
    assert torch.equal(traj0.boards[0], traj.boards[0])
