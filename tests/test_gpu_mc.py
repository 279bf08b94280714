"""Monte-Carlo playouts on the GPU: the playout kernel and the reduction bit-exact against the numpy restatement (tests/mc_ref.py),
continuation and slicing included; the player end to end, with a stand-in critic, through the engine, and its playing strength."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import mc_ref as M  # noqa: E402
from oracle import g2048_oracle as npo  # noqa: E402
from src.actions import act_drul  # noqa: E402
from src.g2048 import native as nv  # noqa: E402
from src.ppo import MonteCarloActionFunction  # noqa: E402
from src.runs import BatchRunner, evaluate_max_tile  # noqa: E402

pytestmark = pytest.mark.gpu
SLACK = 4099
GUARD = 0xA5
GUARD_F32 = np.array([0xA5A5A5A5], np.uint32).view(np.float32)[0]


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _f32(a, dev):
    return torch.from_numpy(np.array(a, np.float32).view(np.int32)).to(dev).view(torch.float32)


class Lanes:
    """Lane arrays of n lanes with SLACK guarded rows behind them."""

    def __init__(self, n, dev, state=None):
        self.n = n
        rows = n + SLACK
        self.boards = torch.full((rows, 16), GUARD, dtype=torch.uint8, device=dev)
        self.masks = torch.full((rows,), GUARD, dtype=torch.uint8, device=dev)
        self.done = torch.full((rows,), GUARD, dtype=torch.uint8, device=dev)
        self.ret = torch.full((rows,), float(GUARD_F32), dtype=torch.float32, device=dev)
        self.disc = torch.full((rows,), float(GUARD_F32), dtype=torch.float32, device=dev)
        if state is not None:
            self.boards[:n] = torch.from_numpy(np.array(state["boards"])).to(dev)
            self.masks[:n] = torch.from_numpy(np.array(state["masks"])).to(dev)
            self.done[:n] = torch.from_numpy(np.array(state["done"])).to(dev)
            self.ret[:n] = _f32(state["ret"], dev)
            self.disc[:n] = _f32(state["disc"], dev)

    def args(self):
        n = self.n
        return self.boards[:n], self.masks[:n], self.done[:n], self.ret[:n], self.disc[:n]

    def check(self, want, rows=slice(None), what=""):
        n = self.n
        assert np.array_equal(self.boards[:n].cpu().numpy(), want["boards"][rows]), (what, "boards")
        assert np.array_equal(self.masks[:n].cpu().numpy(), want["masks"][rows]), (what, "masks")
        assert np.array_equal(self.done[:n].cpu().numpy(), want["done"][rows]), (what, "done")
        assert np.array_equal(_bits(self.ret[:n]), want["ret"][rows].view(np.uint32)), (what, "ret")
        assert np.array_equal(_bits(self.disc[:n]), want["disc"][rows].view(np.uint32)), (what, "disc")
        assert (self.boards[n:] == GUARD).all() and (self.masks[n:] == GUARD).all() and (self.done[n:] == GUARD).all(), what
        assert (_bits(self.ret[n:]) == 0xA5A5A5A5).all() and (_bits(self.disc[n:]) == 0xA5A5A5A5).all(), what


def _live(want):
    return int((want["done"] == 0).sum())


@pytest.mark.parametrize("policy,mode,gamma,B,R", M.matrix())
def test_playout_is_bit_exact(dev, policy, mode, gamma, B, R):
    c = M.matrix_case(policy, mode, gamma, B, R)
    n = c["n"]
    roots = torch.from_numpy(c["roots"].copy()).to(dev)
    live = torch.zeros(1, dtype=torch.int32, device=dev)
    # 12 steps in one launch
    L = Lanes(n, dev)
    nv.mc_playout(c["subs"], 0, roots, B, R, 0, n, policy, gamma, *L.args(), mode, live)
    L.check(c["full"], what="12 steps")
    assert int(live.item()) == _live(c["full"])
    # 5 + 7, continued from the stored state; the second launch without roots and without a counter
    L = Lanes(n, dev)
    live.zero_()
    nv.mc_playout(c["subs"][:M.CUT], 0, roots, B, R, 0, n, policy, gamma, *L.args(), mode, live)
    L.check(c["first"], what="5 steps")
    assert int(live.item()) == _live(c["first"])
    nv.mc_playout(c["subs"][M.CUT:], M.CUT, None, B, R, 0, n, policy, gamma, *L.args(), mode, None)
    L.check(c["full"], what="5 + 7 steps")
    live.zero_()
    L2 = Lanes(n, dev, c["first"])
    nv.mc_playout(c["subs"][M.CUT:], M.CUT, roots, B, R, 0, n, policy, gamma, *L2.args(), mode, live)
    L2.check(c["full"], what="5 + 7 steps from an uploaded state")
    assert int(live.item()) == _live(c["full"])
    # the same roots as a slice of a larger call
    L = Lanes(n, dev)
    nv.mc_playout(c["subs"], 0, roots, B, R, c["lane0"], c["n_ext"], policy, gamma, *L.args(), mode, None)
    L.check(c["ext"], slice(c["lane0"], c["lane0"] + n), what="lane0 > 0")
    assert np.array_equal(roots.cpu().numpy(), c["roots"])  # read only


@pytest.fixture(scope="module")
def big():
    B, R, steps, mode = 300, 7, 16, npo.MODE_PARTITIONABLE
    roots = M.root_boards(B, seed=11)
    _, subs = M.chain_keys(npo.key(99), 2 * steps, mode)
    subs = subs.reshape(steps, 4)
    want = M.playout(subs, 0, roots, R, 0, 4 * B * R, M.POLICY_RANDOM, 0.99, mode)
    return dict(B=B, R=R, mode=mode, roots=roots, subs=subs, want=want)


def test_playout_over_many_workgroups(dev, big):
    B, R = big["B"], big["R"]
    n = 4 * B * R
    assert n == 8400 and n % 256 != 0
    L = Lanes(n, dev)
    live = torch.zeros(1, dtype=torch.int32, device=dev)
    nv.mc_playout(big["subs"], 0, torch.from_numpy(big["roots"]).to(dev), B, R, 0, n, M.POLICY_RANDOM, 0.99, *L.args(), big["mode"], live)
    L.check(big["want"], what="8400 lanes")
    assert int(live.item()) == _live(big["want"]) > 0


@pytest.mark.parametrize("R", (1, 3, 64, 130))
def test_reduce_is_bit_exact(dev, R):
    B = 37
    n = 4 * B * R
    rng = np.random.default_rng(R)
    ret = (rng.integers(0, 5000, n) * rng.choice([1.0, 0.97, 0.5], n)).astype(np.float32)
    disc = (0.99 ** rng.integers(1, 40, n)).astype(np.float32)
    done = (rng.random(n) < 0.4).astype(np.uint8)
    values = (rng.standard_normal(n) * 400).astype(np.float32)
    illegal = np.zeros(4 * B, bool)
    illegal[::5] = True  # whole pairs that never ran: done, +0, disc 1
    lanes = np.repeat(illegal, R)
    ret[lanes], disc[lanes], done[lanes] = 0.0, 1.0, 1
    poisoned = np.where(done != 0, np.float32(1e30), values).astype(np.float32)
    t_ret, t_disc, t_done = _f32(ret, dev), _f32(disc, dev), torch.from_numpy(done).to(dev)
    for v, ref_v in ((None, None), (values, values), (poisoned, values)):
        q = torch.full((B + SLACK, 4), float(GUARD_F32), dtype=torch.float32, device=dev)
        nv.mc_reduce(t_ret, t_disc, t_done, None if v is None else _f32(v, dev), R, q[:B])
        want = M.reduce(ret, disc, done, ref_v, R)
        assert np.array_equal(_bits(q[:B]).reshape(-1), want.view(np.uint32))
        assert (_bits(q[:B]).reshape(-1)[illegal] == 0).all()  # +0
        assert (_bits(q[B:]) == 0xA5A5A5A5).all()
    assert np.array_equal(_bits(t_ret), ret.view(np.uint32)) and np.array_equal(t_done.cpu().numpy(), done)


def test_played_to_the_end(dev):
    boards = M.root_boards(16, seed=4)
    fn = MonteCarloActionFunction(playouts=8, seed=3, rng_mode=npo.MODE_PARTITIONABLE)
    ref = M.Player(3, npo.MODE_PARTITIONABLE, 8)
    want = ref.playout(boards)
    assert ref.last_steps > M.MAX_LAUNCH and not (want["done"] == 0).any()  # more than one launch
    (b0, b1, state), = fn.playout(torch.from_numpy(boards).to(dev))
    assert (b0, b1) == (0, 16) and fn.last_steps == ref.last_steps and fn.last_lanes == 4 * 16 * 8
    got = dict(zip(("boards", "masks", "done", "ret", "disc"), (x.cpu().numpy() for x in state)))
    for k in ("boards", "masks", "done"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("ret", "disc"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    assert np.array_equal(fn._key, ref.key)  # the chain advanced by the launches that ran, no more
    with pytest.raises(RuntimeError):
        MonteCarloActionFunction(playouts=8, seed=3, max_steps=1).policy_fn(torch.from_numpy(boards).to(dev), None)


def test_policy_fn_end_to_end_slices_and_seeds(dev):
    boards = M.root_boards(50, seed=6)
    tb = torch.from_numpy(boards).to(dev)
    kw = dict(playouts=4, depth=10, playout_policy="random", rng_mode=npo.MODE_PARTITIONABLE)
    fn, sliced, other = (MonteCarloActionFunction(seed=5, **kw), MonteCarloActionFunction(seed=5, max_lanes=16 * 17, **kw),
                         MonteCarloActionFunction(seed=6, **kw))
    ref = M.Player(5, npo.MODE_PARTITIONABLE, 4, depth=10)
    differs = False
    for call in range(2):  # the second call draws the next keys of the chain
        want_q, want_v, _ = ref.policy_fn(boards)
        q, v = fn.policy_fn(tb, None)
        assert np.array_equal(_bits(q), want_q.view(np.uint32)), call
        assert np.array_equal(_bits(v), want_v.view(np.uint32)), call
        qs, vs = sliced.policy_fn(tb, None)  # 17 + 17 + 16 boards
        assert torch.equal(qs.view(torch.int32), q.view(torch.int32)) and torch.equal(vs.view(torch.int32), v.view(torch.int32))
        differs |= not torch.equal(other.policy_fn(tb, None)[0], q)
        assert fn.last_steps == 10 and fn.last_lanes == 800
    assert differs
    drul = MonteCarloActionFunction(seed=5, playouts=2, depth=9, playout_policy="drul", gamma=0.99)
    want_q, want_v, _ = M.Player(5, npo.MODE_PARTITIONABLE, 2, depth=9, policy=M.POLICY_DRUL, gamma=0.99).policy_fn(boards)
    q, v = drul.policy_fn(tb, None)
    assert np.array_equal(_bits(q), want_q.view(np.uint32)) and np.array_equal(_bits(v), want_v.view(np.uint32))


class _CellwiseCritic(torch.nn.Module):
    """A stand-in actor-critic made of elementwise torch operators only, so that its value of a row cannot depend on the slot the row
    sits in: sixteen terms (x_c w + b) x_c of the cells added one after the other."""

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
        return torch.stack(outs[:4], dim=1), outs[4]


def test_critic_bootstrap_equals_the_restatement(dev):
    boards = M.root_boards(40, seed=8)
    agent = _CellwiseCritic()
    fn = MonteCarloActionFunction(agent, playouts=3, depth=6, seed=2, device=dev, rng_mode=npo.MODE_PARTITIONABLE, max_children=100)
    assert fn.gamma == 0.99

    def critic(rows):
        with torch.no_grad():
            return agent(torch.from_numpy(np.ascontiguousarray(rows)).to(dev))[1].cpu().numpy()

    want_q, want_v, st = M.Player(2, npo.MODE_PARTITIONABLE, 3, depth=6, gamma=0.99).policy_fn(boards, critic)
    q, v = fn.policy_fn(torch.from_numpy(boards).to(dev), None)
    assert np.array_equal(_bits(q), want_q.view(np.uint32)) and np.array_equal(_bits(v), want_v.view(np.uint32))
    done = st["done"].reshape(-1, 3) != 0
    assert done.all(axis=1).any() and (~done).all(axis=1).any() and (done.any(axis=1) & ~done.all(axis=1)).any()
    # finished leaves contribute no value: a pair whose lanes have all ended has the plain mean of its returns
    plain = M.reduce(st["ret"], st["disc"], st["done"], None, 3)
    assert np.array_equal(want_q.reshape(-1)[done.all(axis=1)].view(np.uint32), plain[done.all(axis=1)].view(np.uint32))
    assert not np.array_equal(want_q.reshape(-1)[(~done).all(axis=1)], plain[(~done).all(axis=1)])


def test_through_the_engine(dev):
    fn = MonteCarloActionFunction(playouts=8, depth=6, rng_mode=npo.MODE_PARTITIONABLE)
    inner, calls = fn.policy_fn, []

    def recording(boards, masks):
        q, v = inner(boards, masks)
        calls.append((boards.cpu().numpy().copy(), q.cpu().numpy().copy()))
        return q, v

    recording.needs_masks = False
    fn.policy_fn = recording
    traj = BatchRunner(init_seed=7, act_fn=fn, rng_mode="partitionable", device=dev).collect(4)
    assert traj.T >= 24 and len(calls) >= 24
    ref = M.Player(0, npo.MODE_PARTITIONABLE, 8, depth=6)
    t_boards, t_actions, t_masks = traj.boards.cpu().numpy(), traj.actions.cpu().numpy(), traj.masks.cpu().numpy()
    for t in range(24):
        boards, q = calls[t]
        assert np.array_equal(boards, t_boards[t]), t  # nobody has finished yet: the call saw the whole batch
        want_q, _, _ = ref.policy_fn(boards)
        assert np.array_equal(q.view(np.uint32), want_q.view(np.uint32)), t
        masked = (q - np.where(M.bits_mask(t_masks[t]), np.float32(0), np.float32(1e8))).astype(np.float32)
        assert np.array_equal(t_actions[t], masked.argmax(axis=1)), t
    plain = BatchRunner(init_seed=7, act_fn=act_drul, rng_mode="partitionable", device=dev).collect(4)
    assert torch.equal(plain.init_boards, traj.init_boards)  # the env's own key stream is untouched


def test_strength(dev):
    mc = evaluate_max_tile(MonteCarloActionFunction(playouts=16, depth=40, seed=0), num_episodes=16, seed=42, device=dev)
    drul = evaluate_max_tile(act_drul, num_episodes=16, seed=42, device=dev)
    print(f"mean max tile over 16 episodes: monte carlo (R=16, depth 40) {mc['mean_max_tile']:.1f}, DRUL {drul['mean_max_tile']:.1f}")
    assert mc["mean_max_tile"] >= 2 * drul["mean_max_tile"]
