"""Multi-stage n-tuple network (g2048_ntuple_staged_*): declared, bound, exported; every argument check runs before any device work;
the wrappers refuse host tensors; the network's and the trainer's settings, promotion, save / load and state without a device; the
per-lane code of the kernels, compiled for the host, equals the numpy restatement (tests/ntuple_stage_ref.py) bit for bit; and the
restatement's training loop promotes.  CPU only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import ntuple_ref as N  # noqa: E402
import ntuple_search_ref as NS  # noqa: E402
import ntuple_stage_ref as G  # noqa: E402
import ntuple_tc_ref as T  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# name -> (arguments, the wrapper)
NAMES = {"g2048_ntuple_staged_values": (11, "ntuple_values"), "g2048_ntuple_staged_scores": (12, "ntuple_scores"),
         "g2048_ntuple_staged_expectimax": (15, "ntuple_expectimax"), "g2048_ntuple_staged_td_accumulate": (16, "ntuple_td_accumulate"),
         "g2048_ntuple_staged_td_apply": (12, "ntuple_td_apply"), "g2048_ntuple_staged_tc_accumulate": (17, "ntuple_tc_accumulate"),
         "g2048_ntuple_staged_tc_apply": (15, "ntuple_tc_apply")}
F32 = np.float32


def test_symbols_are_declared_bound_and_exported():
    import inspect

    from src.g2048 import native as nv

    header = open(os.path.join(ROOT, "include", "g2048.h")).read()
    lib = C.CDLL(nv.LIB_PATH)
    for name, (nargs, wrapper) in NAMES.items():
        assert f"int {name}(" in header
        assert name in nv.SIGNATURES and len(nv.SIGNATURES[name]) == nargs
        assert len(nv.SIGNATURES[name]) == len(nv.SIGNATURES[name.replace("_staged", "")]) + 2  # (stage_tiles, n_stages) after L
        assert hasattr(lib, name)
        params = list(inspect.signature(getattr(nv, wrapper)).parameters.values())
        assert params[-1].name == "stage_tiles" and params[-1].default is None
    assert "#define G2048_ABI_VERSION 4" in header
    assert nv.load().g2048_abi_version() == 4  # additive: the version stays


def test_entry_points_reject_bad_arguments_without_touching_a_device():
    from src.g2048 import native as nv

    lib = nv.load()
    a = 1 << 20  # a fake, 16-byte aligned "device address": rejected before any use
    good = np.array([[0, 1, 2], [4, 5, 6]], np.uint8)
    hi = np.array([[0, 1, 2], [4, 16, 6]], np.uint8)
    gp = good.ctypes.data
    arrays = [np.array(x, np.uint8) for x in ([3, 5, 9], [5, 3, 9], [3, 3, 9], [0, 5, 9], [3, 5, 18], [1, 2, 3, 4, 5, 6, 7, 8])]
    ok, desc, equal, zero, high, eight = (x.ctypes.data for x in arrays)
    # the stage checks, on top of every check of the unstaged functions (a few of those follow: they are still made)
    stage_bad = [dict(S=0), dict(S=-1), dict(S=9), dict(tiles=eight, S=9), dict(tiles=None, S=2), dict(tiles=None, S=4),
                 dict(tiles=desc), dict(tiles=equal), dict(tiles=zero), dict(tiles=high), dict(tiles=high, S=4)]
    net_bad = [dict(cells=None), dict(m=0), dict(m=9), dict(L=0), dict(L=7), dict(cells=hi.ctypes.data)]

    def values(boards=a, n=8, w=a, cells=gp, m=2, L=3, tiles=ok, S=4, F=12, out=a):
        return lib.g2048_ntuple_staged_values(boards, n, w, cells, m, L, tiles, S, F, out, None)

    def scores(boards=a, n=8, w=a, cells=gp, m=2, L=3, tiles=ok, S=4, F=12, q=a, v=a):
        return lib.g2048_ntuple_staged_scores(boards, n, w, cells, m, L, tiles, S, F, q, v, None)

    def expectimax(boards=a, n=8, w=a, cells=gp, m=2, L=3, tiles=ok, S=4, F=12, plies=2, gamma=1.0, ws=a, q=a, v=a):
        return lib.g2048_ntuple_staged_expectimax(boards, n, w, cells, m, L, tiles, S, F, plies, gamma, ws, q, v, None)

    def td_accumulate(prev=a, flag=a, target=a, n=8, w=a, cells=gp, m=2, L=3, tiles=ok, S=4, F=12, alpha=0.1, acc=a, cnt=a, err=a):
        return lib.g2048_ntuple_staged_td_accumulate(prev, flag, target, n, w, cells, m, L, tiles, S, F, alpha, acc, cnt, err, None)

    def td_apply(prev=a, flag=a, n=8, cells=gp, m=2, L=3, tiles=ok, S=4, w=a, acc=a, cnt=a):
        return lib.g2048_ntuple_staged_td_apply(prev, flag, n, cells, m, L, tiles, S, w, acc, cnt, None)

    def tc_accumulate(prev=a, flag=a, target=a, n=8, w=a, cells=gp, m=2, L=3, tiles=ok, S=4, F=12, alpha=1.0, acc=a, abs_acc=a, cnt=a,
                      err=a):
        return lib.g2048_ntuple_staged_tc_accumulate(prev, flag, target, n, w, cells, m, L, tiles, S, F, alpha, acc, abs_acc, cnt, err,
                                                     None)

    def tc_apply(prev=a, flag=a, n=8, cells=gp, m=2, L=3, tiles=ok, S=4, w=a, acc=a, abs_acc=a, cnt=a, coh_e=a, coh_a=a):
        return lib.g2048_ntuple_staged_tc_apply(prev, flag, n, cells, m, L, tiles, S, w, acc, abs_acc, cnt, coh_e, coh_a, None)

    frac_bad = [dict(F=-1), dict(F=21)]
    own = {values: frac_bad + [dict(boards=None), dict(out=None), dict(n=0), dict(n=(1 << 28) + 1), dict(boards=a + 8), dict(w=a + 2)],
           scores: frac_bad + [dict(q=None), dict(v=None), dict(n=0), dict(q=a + 2)],
           expectimax: frac_bad + [dict(plies=0), dict(plies=3), dict(ws=None), dict(gamma=-1.0), dict(gamma=float("nan")),
                                   dict(n=(1 << 20) + 1), dict(ws=a + 4)],
           td_accumulate: frac_bad + [dict(prev=None), dict(acc=None), dict(alpha=0.0), dict(alpha=float("inf")), dict(acc=a + 4)],
           td_apply: [dict(flag=None), dict(w=None), dict(n=-3), dict(cnt=a + 1)],
           tc_accumulate: frac_bad + [dict(abs_acc=None), dict(alpha=-0.1), dict(abs_acc=a + 4), dict(err=a + 1)],
           tc_apply: [dict(coh_e=None), dict(coh_a=None), dict(n=0), dict(coh_a=a + 1)]}
    for fn, more in own.items():
        for kw in stage_bad + net_bad + more:
            assert fn(**kw) == -1, (fn.__name__, kw)


def test_wrappers_refuse_host_tensors():
    import torch

    from src.g2048 import native as nv

    B, cells, tiles = 4, np.array(N.SMALL, np.uint8), (3, 5)
    boards = torch.zeros((B, 16), dtype=torch.uint8)
    w = torch.zeros((3, 3, 256), dtype=torch.int32)
    acc, cnt = torch.zeros((3, 3, 256), dtype=torch.int64), torch.zeros((3, 3, 256), dtype=torch.int32)
    flag, f, q = torch.zeros(B, dtype=torch.uint8), torch.zeros(B), torch.zeros((B, 4))
    calls = [lambda: nv.ntuple_values(boards, w, cells, 12, f, tiles),
             lambda: nv.ntuple_scores(boards, w, cells, 12, q, f, tiles),
             lambda: nv.ntuple_expectimax(boards, w, cells, 12, 1, 1.0, None, q, f, tiles),
             lambda: nv.ntuple_td_accumulate(boards, flag, f, w, cells, 12, 0.1, acc, cnt, f, tiles),
             lambda: nv.ntuple_td_apply(boards, flag, cells, w, acc, cnt, tiles),
             lambda: nv.ntuple_tc_accumulate(boards, flag, f, w, cells, 12, 1.0, acc, acc.clone(), cnt, f, tiles),
             lambda: nv.ntuple_tc_apply(boards, flag, cells, w, acc, acc.clone(), cnt, cnt.clone(), cnt.clone(), tiles),
             lambda: nv.ntuple_values(boards, w, cells, 12, f, ((3, 5),))]  # stage_tiles is a flat sequence
    for call in calls:
        with pytest.raises(nv.NativeError):
            call()


# ---------------------------------------------------------------------------------------------- Python settings without a device
def test_network_settings_promotion_and_files(tmp_path):
    import torch

    from src.ppo import NTupleNetwork

    for bad in ((5, 3), (3, 3), (0, 3), (3, 18), (1, 2, 3, 4, 5, 6, 7, 8), (3.5,), ("a",), (), 3, (True, 3)):
        with pytest.raises(ValueError):
            NTupleNetwork(N.SMALL, device="cpu", stage_tiles=bad)
    assert "1.34 GB" in NTupleNetwork.__doc__
    plain = NTupleNetwork(N.SMALL, device="cpu")
    assert plain.stage_tiles is None and plain.stages == 1 and plain.active_stages == 1 and tuple(plain.weights.shape) == (3, 256)
    assert plain.active_tiles is None
    with pytest.raises(ValueError):
        plain.promote()
    net = NTupleNetwork(N.SMALL, 10, "cpu", (3, 4, 5))  # the positional order of the constructor
    assert net.stage_tiles == (3, 4, 5) and net.stages == 4 and net.active_stages == 1 and net.frac_bits == 10
    assert tuple(net.weights.shape) == (4, 3, 256) and net.weights.dtype == torch.int32 and not net.weights.any()
    assert net.active_tiles.dtype == np.uint8 and net.active_tiles.tolist() == []
    for bad in (0, 5, -1, 1.0, None, True):
        with pytest.raises(ValueError):
            net.active_stages = bad
    assert net.active_stages == 1
    boards = torch.from_numpy(np.array(G.threshold_boards((3, 4, 5))))
    assert net.stage_of(boards).dtype == torch.uint8 and not net.stage_of(boards).any()  # one active stage serves every board
    net.weights[0] = torch.arange(3 * 256, dtype=torch.int32).reshape(3, 256) - 300
    assert net.promote() == 2 and net.active_stages == 2 and net.active_tiles.tolist() == [3]
    assert torch.equal(net.weights[1], net.weights[0]) and not net.weights[2:].any()
    net.weights[1, 0, 0] = 77
    assert net.promote() == 3 and int(net.weights[2, 0, 0]) == 77 and int(net.weights[0, 0, 0]) == -300
    assert np.array_equal(net.stage_of(boards).numpy(), np.minimum(G.stage(boards.numpy(), (3, 4, 5)), 2))
    path = str(tmp_path / "net.pt")
    net.save(path)
    back = NTupleNetwork.load(path, device="cpu")
    assert back.stage_tiles == (3, 4, 5) and back.active_stages == 3 and back.frac_bits == 10 and back.tuples == net.tuples
    assert torch.equal(back.weights, net.weights)
    assert net.promote() == 4
    with pytest.raises(ValueError):
        net.promote()  # the top stage
    net.active_stages = 2
    assert net.active_tiles.tolist() == [3]
    # a file of before: no stage keys -> an unstaged network
    old = str(tmp_path / "old.pt")
    torch.save({"weights": plain.weights + 5, "tuples": plain.tuples, "frac_bits": 12}, old)
    o = NTupleNetwork.load(old, device="cpu")
    assert o.stage_tiles is None and o.stages == 1 and tuple(o.weights.shape) == (3, 256) and int(o.weights[0, 0]) == 5
    plain.save(old)
    assert NTupleNetwork.load(old, device="cpu").stage_tiles is None
    bad = str(tmp_path / "bad.pt")
    torch.save({"weights": plain.weights, "tuples": plain.tuples, "frac_bits": 12, "stage_tiles": (3,), "active_stages": 1}, bad)
    with pytest.raises(ValueError):
        NTupleNetwork.load(bad, device="cpu")  # [m, 16^L] weights do not fit two stages


def test_trainer_settings_and_state_without_a_device():
    import torch

    from src.ppo import NTupleNetwork, NTupleTrainer

    net = NTupleNetwork(N.SMALL, device="cpu", stage_tiles=(3, 4, 5))
    for bad in (-1, 1.5, None, "8", True):
        with pytest.raises(ValueError):
            NTupleTrainer(net, 4, promote_every=bad)
    assert "11.5 GB" in NTupleTrainer.__doc__
    tc = NTupleTrainer(net, 4, alpha=1.0, learner="tc", promote_every=8)
    assert NTupleTrainer(net, 4).promote_every == 64 and tc.promote_every == 8 and tc.promotions == []
    for t in (tc.acc, tc.abs_acc, tc.cnt, tc.coh_e, tc.coh_a):
        assert t.shape == net.weights.shape == (4, 3, 256)
    tc.coh_a[3, 1, 7], tc.lock_steps, tc.promotions = 12, 24, [(8, 2), (16, 3)]
    state = tc.state_dict()
    assert state["promotions"] == [(8, 2), (16, 3)] and state["stages"] == 4 and state["lock_steps"] == 24
    fresh = NTupleTrainer(net, 8, learner="tc")
    fresh.load_state_dict(state)
    assert fresh.promotions == [(8, 2), (16, 3)] and fresh.lock_steps == 24 and torch.equal(fresh.coh_a, tc.coh_a)
    tc.promotions.append((24, 4))  # the state is a copy
    assert state["promotions"] == [(8, 2), (16, 3)]
    # another stage count's state is refused, for both learners, and nothing is changed then
    for other_net in (NTupleNetwork(N.SMALL, device="cpu", stage_tiles=(3, 4)), NTupleNetwork(N.SMALL, device="cpu")):
        for learner in ("tc", "td0"):
            other = NTupleTrainer(other_net, 4, learner=learner)
            with pytest.raises(ValueError):
                other.load_state_dict(dict(state, learner=learner))
            assert other.lock_steps == 0 and other.promotions == []
            with pytest.raises(ValueError):
                NTupleTrainer(net, 4, learner=learner).load_state_dict(other.state_dict())
    # the unstaged trainer's state is what it was
    assert set(NTupleTrainer(NTupleNetwork(N.SMALL, device="cpu"), 4).state_dict()) == {"learner", "alpha", "lock_steps"}


# ---------------------------------------------------------------------------------------------- the kernels' per-lane code on the host
HOST_SRC = os.path.join(ROOT, "tests", "host_swar", "ntuple_stage_host.cpp")
CSRC = os.path.join(ROOT, "2048-ppo-agent_amd", "csrc")


def _build(name, src):
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, name)
    subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", "-I", CSRC, "-o", so, src])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def host():
    return _build("libntuple_stage_host.so", HOST_SRC)


@pytest.fixture(scope="module")
def plain_hosts():
    """The unstaged host builds of the existing tests: the other side of the single-stage equivalence."""
    d = os.path.join(ROOT, "tests", "host_swar")
    return (_build("libntuple_host_for_stage.so", os.path.join(d, "ntuple_host.cpp")),
            _build("libntuple_search_host_for_stage.so", os.path.join(d, "ntuple_search_host.cpp")),
            _build("libntuple_tc_host_for_stage.so", os.path.join(d, "ntuple_tc_host.cpp")))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


class Host:
    """The staged host functions on one network: (tuples, tiles, F)."""

    def __init__(self, lib, tuples, tiles, F):
        self.lib, self.cells, self.F = lib, N.cells_array(tuples), F
        self.tiles = None if tiles is None else np.array(tiles, np.uint8)
        self.S = 1 if tiles is None else len(tiles) + 1
        self.net = (_p(self.cells), C.c_int(self.cells.shape[0]), C.c_int(self.cells.shape[1]), _p(self.tiles), C.c_int(self.S))

    def stage(self, boards):
        out = np.full(len(boards), 99, np.uint8)
        assert self.lib.hst_nts_stage(_p(boards), C.c_int64(len(boards)), *self.net, _p(out)) == 0
        return out

    def values(self, boards, w):
        out = np.full(len(boards), np.nan, F32)
        assert self.lib.hst_nts_values(_p(boards), C.c_int64(len(boards)), _p(w), *self.net, C.c_int(self.F), _p(out)) == 0
        return out

    def scores(self, boards, w):
        q, v = np.full((len(boards), 4), np.nan, F32), np.full(len(boards), np.nan, F32)
        assert self.lib.hst_nts_scores(_p(boards), C.c_int64(len(boards)), _p(w), *self.net, C.c_int(self.F), _p(q), _p(v)) == 0
        return q, v

    def expectimax(self, boards, w, plies, gamma):
        B = len(boards)
        ws = np.full(128 * B, np.nan, F32)
        q, v = np.full((B, 4), np.nan, F32), np.full(B, np.nan, F32)
        assert self.lib.hst_nts_expectimax(_p(boards), C.c_int64(B), _p(w), *self.net, C.c_int(self.F), C.c_int(plies), C.c_double(gamma),
                                           _p(ws), _p(q), _p(v)) == 0
        return q, v

    def td_step(self, prev, flag, target, w, alpha):
        B = len(prev)
        acc, cnt, err = np.zeros(w.shape, np.int64), np.zeros(w.shape, np.int32), np.full(B, -7, F32)
        assert self.lib.hst_nts_td_accumulate(_p(prev), _p(flag), _p(target), C.c_int64(B), _p(w), *self.net, C.c_int(self.F),
                                              C.c_double(alpha), _p(acc), _p(cnt), _p(err)) == 0
        assert cnt.sum() == 8 * self.cells.shape[0] * int((flag != 0).sum())
        assert self.lib.hst_nts_td_apply(_p(prev), _p(flag), C.c_int64(B), *self.net, _p(w), _p(acc), _p(cnt)) == 0
        assert not acc.any() and not cnt.any()
        return err

    def tc_step(self, prev, flag, target, w, coh_e, coh_a, alpha):
        B = len(prev)
        acc, abs_acc, cnt = np.zeros(w.shape, np.int64), np.zeros(w.shape, np.int64), np.zeros(w.shape, np.int32)
        err = np.full(B, -7, F32)
        assert self.lib.hst_nts_tc_accumulate(_p(prev), _p(flag), _p(target), C.c_int64(B), _p(w), *self.net, C.c_int(self.F),
                                              C.c_double(alpha), _p(acc), _p(abs_acc), _p(cnt), _p(err)) == 0
        assert cnt.sum() == 8 * self.cells.shape[0] * int((flag != 0).sum())
        assert self.lib.hst_nts_tc_apply(_p(prev), _p(flag), C.c_int64(B), *self.net, _p(w), _p(acc), _p(abs_acc), _p(cnt), _p(coh_e),
                                         _p(coh_a)) == 0
        assert not acc.any() and not abs_acc.any() and not cnt.any()
        return err


def _host_for(host, name):
    return Host(host, *G.NETWORKS[name])


def test_the_restatement_is_built_on_the_unstaged_ones():
    """With one stage (no thresholds) the restatement IS ntuple_ref / ntuple_search_ref."""
    w, boards = N.small_weights(), N.boards_for(60)
    assert np.array_equal(_bits(G.values(boards, w[None], N.SMALL, 12, ())), _bits(N.values(boards, w, N.SMALL, 12)))
    for got, want in zip(G.scores(boards, w[None], N.SMALL, 12, ()), N.scores(boards, w, N.SMALL, 12)):
        assert np.array_equal(got.view(np.uint32) if got.dtype == F32 else got, want.view(np.uint32) if want.dtype == F32 else want)
    res, _ = G.expectimax(boards[:12], w[None], N.SMALL, 12, (), 1)
    want, _, _ = NS.one_ply(boards[:12], N.SMALL, w)
    assert all(np.array_equal(_bits(res[g][0]), _bits(want[g][0])) for g in G.GAMMAS)


@pytest.mark.parametrize("name", list(G.NETWORKS))
def test_stage_values_and_scores_equal_the_restatement(host, name):
    tuples, tiles, F = G.NETWORKS[name]
    c = G.values_case(name)  # asserts on the CPU: every stage looked up, an afterstate in another stage than its board
    h = _host_for(host, name)
    boards = np.array(c["boards"])
    assert np.array_equal(h.stage(boards), G.stage(boards, tiles).astype(np.uint8))
    w = np.array(G.staged_weights(name))
    assert np.array_equal(_bits(h.values(boards, w)), _bits(c["v"]))
    q, v = h.scores(boards, w)
    assert np.array_equal(_bits(q), _bits(c["q"])) and np.array_equal(_bits(v), _bits(c["qv"]))
    # the stage matters: the same boards on the stage-0 tables alone give other bits
    assert (_bits(h.values(boards, w)) != _bits(N.values(boards, w[0], tuples, F))).any()


def test_the_max_tile_is_unclamped_and_view_invariant(host):
    """Tile 16 and tile 17 against thresholds 16 and 17 (idx clamps them to 15, the stage must not), every cell position, and all
    eight views of the random boards."""
    import symmetry_ref as S

    h = Host(host, N.SMALL, (15, 16, 17), 12)
    boards = np.zeros((64, 16), np.uint8)
    for c in range(16):
        for j, k in enumerate((14, 15, 16, 17)):
            boards[4 * c + j, c] = k
            boards[4 * c + j, (c + 7) % 16] = 3
    assert np.array_equal(h.stage(boards), np.tile(np.array([0, 1, 2, 3], np.uint8), 16))
    rnd = np.ascontiguousarray(N.boards_for(200, seed=3))
    h5 = _host_for(host, "small5")
    for g in range(8):
        assert np.array_equal(h5.stage(np.ascontiguousarray(S.view(rnd, g))), G.stage(rnd, G.NETWORKS["small5"][1]).astype(np.uint8))


@pytest.mark.parametrize("plies", [1, 2])
@pytest.mark.parametrize("name", list(G.NETWORKS))
def test_expectimax_equals_the_restatement(host, name, plies):
    c = G.search_case(name, plies)  # asserts on the CPU that a leaf's stage differs from its root's (two plies)
    h = _host_for(host, name)
    w = np.array(G.staged_weights(name))
    for gamma in G.GAMMAS:
        q, v = h.expectimax(np.array(c["boards"]), w, plies, gamma)
        assert np.array_equal(_bits(q), _bits(c["q"][gamma])) and np.array_equal(_bits(v), _bits(c["v"][gamma])), gamma


def test_td_and_tc_step_under_collision_in_two_orders(host):
    """1000 envs, 300 of them identical, over at least three stages, flags 0 / 1 / 2: both learners equal the restatement, in two env
    orders, and the tables of the stage no env was in are untouched."""
    c = G.collision_case()
    h = _host_for(host, "small5")
    w0 = G.staged_weights("small5")
    assert len(c["stages_hit"]) >= 3 and 4 not in c["stages_hit"]
    perm = np.random.default_rng(1).permutation(1000)
    for order in (np.arange(1000), perm):
        prev, flag, target = (np.ascontiguousarray(c[k][order]) for k in ("prev", "flag", "target"))
        w = w0.copy()
        err = h.td_step(prev, flag, target, w, 0.1)
        assert np.array_equal(w, c["td_w"]) and np.array_equal(_bits(err), _bits(c["td_e"][order]))
        assert np.array_equal(w[4], w0[4]) and all((w[s] != w0[s]).any() for s in c["stages_hit"])
        w, ce, ca = w0.copy(), np.zeros(w0.shape, np.int32), np.zeros(w0.shape, np.int32)
        err = h.tc_step(prev, flag, target, w, ce, ca, 0.1)
        assert np.array_equal(w, c["tc_w"]) and np.array_equal(ce, c["tc_ce"]) and np.array_equal(ca, c["tc_ca"])
        assert np.array_equal(_bits(err), _bits(c["tc_e"][order])) and (_bits(err[flag == 0]) == 0).all()
        assert np.array_equal(w[4], w0[4]) and not ce[4].any() and not ca[4].any()
    assert np.array_equal(c["tc_w"], c["td_w"])  # from zero coherence the first TC step is TD(0)'s


@pytest.mark.parametrize("alpha,scale,extreme", [(0.1, 500.0, False), (1000.0, 1e9, True)])
def test_six_tc_steps_equal_the_restatement(host, alpha, scale, extreme):
    c = G.sequence_case(alpha, scale, extreme)
    assert c["stats"]["slowed"] > 0
    if extreme:
        assert c["stats"]["saturated"] > 0 and c["stats"]["clamped"] > 0 and c["stats"]["halved"] > 0
    h = Host(host, c["tuples"], c["tiles"], c["F"])
    w = c["w0"].copy()
    ce, ca = np.zeros(w.shape, np.int32), np.zeros(w.shape, np.int32)
    for t, want in enumerate(c["after"]):
        err = h.tc_step(np.array(c["prev"]), np.array(c["flag"]), np.array(c["targets"][t]), w, ce, ca, alpha)
        assert np.array_equal(w, want["weights"]) and np.array_equal(ce, want["coh_e"]) and np.array_equal(ca, want["coh_a"]), t
        assert np.array_equal(_bits(err), _bits(want["td_error"])), t
    assert ca[0].any() and ca[1].any()  # both stages learned


def test_single_stage_equals_the_unstaged_functions(host, plain_hosts):
    """n_stages = 1 (null stage_tiles): every staged host function gives the bits of the unstaged host build."""
    nt, search, tc = plain_hosts
    cells = N.cells_array(N.SMALL)
    net = (_p(cells), C.c_int(3), C.c_int(2))
    h = Host(host, N.SMALL, None, 12)
    boards, w = np.ascontiguousarray(N.boards_for(200)), N.small_weights().copy()
    B = len(boards)
    v = np.empty(B, F32)
    nt.hst_nt_values(_p(boards), C.c_int64(B), _p(w), *net, C.c_int(12), _p(v))
    assert np.array_equal(_bits(h.values(boards, w)), _bits(v))
    q = np.empty((B, 4), F32)
    nt.hst_nt_scores(_p(boards), C.c_int64(B), _p(w), *net, C.c_int(12), _p(q), _p(v))
    got_q, got_v = h.scores(boards, w)
    assert np.array_equal(_bits(got_q), _bits(q)) and np.array_equal(_bits(got_v), _bits(v))
    for plies in (1, 2):
        ws = np.zeros(128 * 24, F32)
        search.hst_nt_expectimax(_p(boards), C.c_int64(24), _p(w), *net, C.c_int(12), C.c_int(plies), C.c_double(0.99), _p(ws), _p(q),
                                 _p(v))
        got_q, got_v = h.expectimax(boards[:24], w, plies, 0.99)
        assert np.array_equal(_bits(got_q), _bits(q[:24])) and np.array_equal(_bits(got_v), _bits(v[:24]))
    c = N.collision_case()
    prev, flag, target = (np.array(c[k]) for k in ("prev", "flag", "target"))
    w1 = N.small_weights().copy()
    err = h.td_step(prev, flag, target, w1, 0.1)
    assert np.array_equal(w1, c["weights_after"]) and np.array_equal(_bits(err), _bits(c["td_error"]))
    w2, acc, cnt, err2 = N.small_weights().copy(), np.zeros((3, 256), np.int64), np.zeros((3, 256), np.int32), np.empty(1000, F32)
    nt.hst_nt_td_accumulate(_p(prev), _p(flag), _p(target), C.c_int64(1000), _p(w2), *net, C.c_int(12), C.c_double(0.1), _p(acc), _p(cnt),
                            _p(err2))
    nt.hst_nt_td_apply(_p(prev), _p(flag), C.c_int64(1000), *net, _p(w2), _p(acc), _p(cnt))
    assert np.array_equal(w1, w2) and np.array_equal(_bits(err), _bits(err2))
    w3, (ce, ca) = N.small_weights().copy(), T.zero_coherence(N.small_weights())
    w4, (ce4, ca4) = N.small_weights().copy(), T.zero_coherence(N.small_weights())
    for _ in range(2):
        h.tc_step(prev, flag, target, w3, ce, ca, 0.1)
        acc, abs_acc, cnt = np.zeros((3, 256), np.int64), np.zeros((3, 256), np.int64), np.zeros((3, 256), np.int32)
        tc.hst_nt_tc_accumulate(_p(prev), _p(flag), _p(target), C.c_int64(1000), _p(w4), *net, C.c_int(12), C.c_double(0.1), _p(acc),
                                _p(abs_acc), _p(cnt), _p(err2))
        tc.hst_nt_tc_apply(_p(prev), _p(flag), C.c_int64(1000), *net, _p(w4), _p(acc), _p(abs_acc), _p(cnt), _p(ce4), _p(ca4))
    assert np.array_equal(w3, w4) and np.array_equal(ce, ce4) and np.array_equal(ca, ca4)


def test_equal_tables_in_all_stages_give_the_unstaged_results(host):
    """Promotion invariance: with every stage holding the same table, staged values, scores and two-ply results are the unstaged
    ones (what makes ``promote()`` safe in the middle of training)."""
    tuples, tiles, F = G.NETWORKS["small5"]
    w1 = N.small_weights()
    w = np.ascontiguousarray(np.broadcast_to(w1, (len(tiles) + 1,) + w1.shape))
    h, boards = _host_for(host, "small5"), np.array(G.boards_for("small5", 257))
    assert len(set(h.stage(boards).tolist())) == 5
    assert np.array_equal(_bits(h.values(boards, w)), _bits(N.values(boards, w1, tuples, F)))
    want_q, want_v, _ = N.scores(boards, w1, tuples, F)
    q, v = h.scores(boards, w)
    assert np.array_equal(_bits(q), _bits(want_q)) and np.array_equal(_bits(v), _bits(want_v))
    want, _, _ = NS.two_plies(boards[:24], tuples, w1, gammas=(0.99,), frac_bits=F)
    q, v = h.expectimax(boards[:24], w, 2, 0.99)
    assert np.array_equal(_bits(q), _bits(want[0.99][0])) and np.array_equal(_bits(v), _bits(want[0.99][1]))


def test_host_program_runs_clean_under_sanitizers(tmp_path):
    """The per-lane code as a stand-alone program under ASan + UBSan on tables of exactly [8][m][16^L]: an offset that left them or
    a signed overflow would abort it."""
    exe = str(tmp_path / "ntuple_stage_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-DNTUPLE_STAGE_HOST_MAIN", "-I", CSRC, "-o", exe, HOST_SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ntuple_stage_host ok" in out.stdout, out.stderr[-2000:]


# ---------------------------------------------------------------------------------------------- promotion on the restatement
def test_the_unstaged_loop_reaches_the_tiles_the_promotion_test_needs():
    """The unstaged numpy loop (SMALL, 64 envs, TD(0) at alpha 0.1) on seeds 0 to 2: some afterstate holds tile 8 before lock-step 8,
    tile 16 before lock-step 16 and tile 32 before lock-step 24 (on seed 0 they first appear at lock-steps 1, 5 and 14, counted
    from 0), so with a check every 8 lock-steps the three promotions of the test below fall at lock-step 24 at the latest, well
    inside its 48."""
    for seed in (0, 1, 2):
        rng = np.random.default_rng(seed)
        w = N.zero_weights(N.SMALL)
        boards = N._fresh(64, rng)
        prev, flag = np.zeros((64, 16), np.uint8), np.zeros(64, np.uint8)
        first = {}
        from oracle import g2048_oracle as npo

        for t in range(24):
            a, v, _ = N._greedy(boards, w, N.SMALL, 12)
            N.td_step(prev, flag, v, w, N.SMALL, 12, 0.1)
            after, _ = npo.move(boards, a.astype(np.int32))
            for k in (3, 4, 5):
                if after.max() >= k:
                    first.setdefault(k, t)
            nxt = N._spawn(after, rng)
            done = ~npo.legal_mask(nxt).any(axis=1)
            prev, flag = after, np.where(done, 2, 1).astype(np.uint8)
            nxt[done] = N._fresh(int(done.sum()), rng)
            boards = nxt
        print(f"seed {seed}: tiles 8 / 16 / 32 first among the afterstates at lock-steps {first.get(3)} / {first.get(4)} / {first.get(5)}")
        assert first[3] < 8 and first[4] < 16 and first[5] < 24, (seed, first)


@pytest.mark.parametrize("learner", ["td0", "tc"])
def test_the_restatement_promotes_while_it_trains(learner):
    """SMALL with stage_tiles (3, 4, 5), 64 envs, promote_every 8, 48 lock-steps: all three promotions happen, in order, at checks;
    each new stage starts as a copy and then goes its own way; 20 + 28 lock-steps cannot differ because the count is global."""
    net = G.Net(np.zeros((4, 3, 256), np.int32), N.SMALL, (3, 4, 5), 12)
    episodes, promotions = G.simulate_training(net, 64, 48, alpha=1.0 if learner == "tc" else 0.1, seed=0, learner=learner,
                                               promote_every=8)
    assert net.active == 4
    assert [p[1] for p in promotions] == [2, 3, 4] and all(c > 0 and c % 8 == 0 for c, _ in promotions)
    assert promotions[0][0] == 8 and promotions == sorted(promotions)
    assert all(net.w[s].any() for s in range(4)) and all((net.w[s] != net.w[s + 1]).any() for s in range(3))
    # promote_every = 0: never
    net0 = G.Net(np.zeros((4, 3, 256), np.int32), N.SMALL, (3, 4, 5), 12)
    assert G.simulate_training(net0, 64, 20, seed=0, learner=learner, promote_every=0)[1] == [] and net0.active == 1
    assert not net0.w[1:].any() and net0.w[0].any()
