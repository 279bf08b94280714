"""N-tuple searched episodes (g2048_ntuple_search_episodes): declared, bound, exported; every argument check runs before any device
work; the classes refuse bad settings without a device; the wave of the kernel, compiled for the host and run lane by lane and phase
by phase, n_steps per call with the state carried between the calls, equals the numpy restatement
(tests/ntuple_search_episodes_ref.py) bit for bit.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import ntuple_ref as N  # noqa: E402
import ntuple_search_episodes_ref as S  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = {"g2048_ntuple_search_episodes": 20, "g2048_ntuple_staged_search_episodes": 22}
STATE = ("boards", "masks", "ep_len", "score", "chain")
STEPS = (1, 7, 4096)


def test_symbols_are_declared_bound_and_exported():
    from src.g2048 import native as nv

    header = open(os.path.join(ROOT, "include", "g2048.h")).read()
    lib = C.CDLL(nv.LIB_PATH)
    for name, nargs in NAMES.items():
        assert f"int {name}(" in header
        assert name in nv.SIGNATURES and len(nv.SIGNATURES[name]) == nargs
        greedy = nv.SIGNATURES[name.replace("search_", "")]
        at = 9 if "staged" not in name else 11  # plies and gamma follow frac_bits
        assert nv.SIGNATURES[name] == greedy[:at] + [C.c_int, C.c_float] + greedy[at:]
        assert hasattr(lib, name)
    assert callable(nv.ntuple_search_episodes)
    assert "#define G2048_ABI_VERSION 4" in header
    assert nv.load().g2048_abi_version() == 4  # additive: the version stays


def test_entry_points_reject_bad_arguments_without_touching_a_device():
    from src.g2048 import native as nv

    lib = nv.load()
    a = 1 << 20  # a fake, 16-byte aligned "device address": rejected before any use
    good = np.array([[0, 1, 2], [4, 5, 6]], np.uint8)
    hi = np.array([[0, 1, 2], [4, 16, 6]], np.uint8)
    dup = np.array([[0, 1, 2], [4, 6, 6]], np.uint8)
    tiles = np.array([3, 5], np.uint8)

    def call(staged, start=1, n_steps=16, n=8, bs=4, w=a, cells=good.ctypes.data, m=2, L=3, st=tiles.ctypes.data, S=3, F=12, plies=1,
             gamma=1.0, chain=a, boards=a, masks=a, done=a, ep_len=a, score=a, mode=1, live=a):
        if staged:
            return lib.g2048_ntuple_staged_search_episodes(start, n_steps, n, bs, w, cells, m, L, st, S, F, plies, gamma, chain, boards, masks,
                                                           done, ep_len, score, mode, live, None)
        return lib.g2048_ntuple_search_episodes(start, n_steps, n, bs, w, cells, m, L, F, plies, gamma, chain, boards, masks, done, ep_len,
                                                score, mode, live, None)

    bad = [dict(w=None), dict(cells=None), dict(chain=None), dict(boards=None), dict(masks=None), dict(done=None), dict(ep_len=None),
           dict(score=None),
           dict(n=0), dict(n=-1), dict(n=(1 << 24) + 1), dict(bs=0), dict(bs=-2), dict(bs=(1 << 20) + 1),
           dict(n_steps=0), dict(n_steps=-1), dict(n_steps=65537),
           dict(m=0), dict(m=9), dict(L=0), dict(L=7), dict(cells=hi.ctypes.data), dict(cells=dup.ctypes.data), dict(F=-1), dict(F=21),
           dict(mode=2), dict(mode=-1),
           dict(boards=a + 8), dict(score=a + 4), dict(chain=a + 2), dict(ep_len=a + 2), dict(w=a + 2), dict(live=a + 2),
           dict(plies=0), dict(plies=2), dict(plies=-1),
           dict(gamma=float("nan")), dict(gamma=-0.5), dict(gamma=float("inf")), dict(gamma=float("-inf"))]
    for staged in (False, True):
        for start in (0, 1):
            for kw in bad:
                assert call(staged, start=start, **kw) == -1, (staged, start, kw)
    down = np.array([5, 3], np.uint8)
    high = np.array([3, 18], np.uint8)
    zero = np.array([0, 3], np.uint8)
    for start in (0, 1):
        for kw in (dict(S=0), dict(S=9), dict(st=None), dict(st=down.ctypes.data), dict(st=high.ctypes.data), dict(st=zero.ctypes.data)):
            assert call(True, start=start, **kw) == -1, kw


def test_classes_refuse_bad_settings_without_a_device():
    import inspect

    from src.ppo import NTupleNetwork
    from src.ppo.ntuple import SEARCH_EPISODE_STEPS
    from src.runs import evaluate_ntuple_episodes

    net = NTupleNetwork(N.SMALL, device="cpu")
    sig = inspect.signature(net.play_search_episodes)
    assert [(k, p.default) for k, p in sig.parameters.items()] == [
        ("num_episodes", inspect.Parameter.empty), ("seed", 42), ("batch_size", 100), ("rng_mode", None), ("steps_per_launch", None),
        ("max_steps", 1 << 20), ("plies", 0), ("gamma", 1.0)]
    assert sig.parameters["plies"].kind is sig.parameters["gamma"].kind is inspect.Parameter.KEYWORD_ONLY
    assert 1 <= SEARCH_EPISODE_STEPS <= 65536
    for kw in (dict(plies=2), dict(plies=True), dict(plies=-1), dict(plies=3), dict(plies=1.5), dict(plies=1, gamma=-0.1),
               dict(plies=1, gamma=float("nan")), dict(plies=1, gamma=float("inf")), dict(plies=1, gamma="high"), dict(plies=0, gamma=-1.0)):
        with pytest.raises(ValueError):
            net.play_search_episodes(10, **kw)
    for plies in (0, 1):
        for kw in (dict(num_episodes=0), dict(num_episodes=-5), dict(num_episodes=10, batch_size=0), dict(num_episodes=10, batch_size=-1),
                   dict(num_episodes=10, steps_per_launch=0), dict(num_episodes=10, steps_per_launch=-3), dict(num_episodes=2.5),
                   dict(num_episodes=True)):
            with pytest.raises(ValueError):
                net.play_search_episodes(plies=plies, **kw)
        with pytest.raises(ValueError):
            net.play_search_episodes(10, rng_mode="no such mode", plies=plies)
    for kw in (dict(plies=2), dict(plies=True), dict(plies=1, gamma=float("nan")), dict(num_episodes=0), dict(num_episodes=0, plies=1),
               dict(num_episodes=True, plies=1)):
        with pytest.raises(ValueError):
            evaluate_ntuple_episodes(net, **kw)
    sig = inspect.signature(evaluate_ntuple_episodes)
    assert [(k, p.default) for k, p in sig.parameters.items()] == [
        ("network", inspect.Parameter.empty), ("num_episodes", 1000), ("seed", 42), ("rng_mode", None), ("plies", 0), ("gamma", 1.0)]


# ---------------------------------------------------------------------------------------------- the kernel's wave on the host
HOST_SRC = os.path.join(ROOT, "tests", "host_swar", "ntuple_search_episodes_host.cpp")
CSRC = os.path.join(ROOT, "2048-ppo-agent_amd", "csrc")


@pytest.fixture(scope="module")
def host():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libntuple_search_episodes_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", CSRC, "-o", so, HOST_SRC])
    lib = C.CDLL(so)
    lib.hst_nt_search_episodes.restype = C.c_int64
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_state(n, bs):
    """Exactly sized state arrays, every output filled with a value no game produces."""
    return dict(chain=S.chain_heads(n, bs).copy(), boards=np.full((n, 16), 0xEE, np.uint8), masks=np.full(n, 0xEE, np.uint8),
                done=np.full(n, 0xEE, np.uint8), ep_len=np.full(n, -7, np.int32), score=np.full(n, -7, np.int64))


def host_call(host, name, mode, gamma, n, bs, st, start, n_steps):
    tuples, w, F, tiles = S.network(name)
    cells = N.cells_array(tuples)
    t = None if tiles is None else np.array(tiles, np.uint8)
    return host.hst_nt_search_episodes(C.c_int(int(start)), C.c_int(n_steps), C.c_int64(n), C.c_int64(bs), _p(w), _p(cells),
                                       C.c_int(cells.shape[0]), C.c_int(cells.shape[1]), _p(t), C.c_int(1 if t is None else len(t) + 1),
                                       C.c_int(F), C.c_float(gamma), _p(st["chain"]), _p(st["boards"]), _p(st["masks"]), _p(st["done"]),
                                       _p(st["ep_len"]), _p(st["score"]), C.c_int(mode))


def host_play(host, name, mode, gamma, n, bs, n_steps, max_calls=1 << 16):
    st = host_state(n, bs)
    live, calls = host_call(host, name, mode, gamma, n, bs, st, True, n_steps), 1
    while live > 0 and calls < max_calls:
        live, calls = host_call(host, name, mode, gamma, n, bs, st, False, n_steps), calls + 1
    assert live == 0
    return st, calls


def _same(st, ref):
    return all(np.array_equal(st[k], ref[k]) for k in STATE) and (st["done"] == 1).all()


@pytest.mark.parametrize("gamma", S.GAMMAS)
@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("name", S.NETWORKS)
def test_host_build_equals_the_restatement(host, name, mode, gamma):
    """Every (N, bs) of ``S.SIZES`` at 1, 7 and 4 096 steps per call: final boards, masks, lengths, int64 scores and chain heads."""
    for n, bs in S.SIZES:
        ref = S.case(name, mode, gamma, n, bs)
        assert not ref["illegal"].any() and ref["ep_len"].min() >= 1
        for n_steps in STEPS:
            st, calls = host_play(host, name, mode, gamma, n, bs, n_steps)
            assert _same(st, ref), (n, bs, n_steps)
            assert calls == -(-int(ref["ep_len"].max()) // n_steps)  # the call that ends the last game reports 0 live games
    if name == S.STAGED:
        tuples, w, F, tiles = S.network(name)
        final = S.case(name, mode, gamma, 30, 10)["boards"]
        assert len({int(s) for s in S.SR.stage(final, tiles)}) >= 2  # the games cross a threshold: more than one stage is looked up


def test_the_search_changes_the_games():
    """The restatement is not the greedy player's under another name: on the same seeds the searched games differ from the greedy ones."""
    import ntuple_episodes_ref as E

    tuples, w, F, _ = S.network("small")
    greedy = E.play(w, tuples, F, 30, 10, S.MODES[0])
    searched = S.case("small", S.MODES[0], 1.0, 30, 10)
    assert not np.array_equal(greedy["ep_len"], searched["ep_len"])


@pytest.mark.parametrize("mode", S.MODES)
def test_one_call_and_many_calls_agree(host, mode):
    """The same games in one call, in calls of 1 step, and in calls whose size changes on the way; a call on the finished state
    changes nothing."""
    n, bs, name, gamma = 23, 10, "small", 0.99
    one, calls = host_play(host, name, mode, gamma, n, bs, 65536)
    assert calls == 1
    for sizes in ((1,), (3, 50, 1, 4096)):
        st = host_state(n, bs)
        live, k = host_call(host, name, mode, gamma, n, bs, st, True, sizes[0]), 1
        while live > 0:
            live, k = host_call(host, name, mode, gamma, n, bs, st, False, sizes[min(k, len(sizes) - 1)]), k + 1
        assert all(np.array_equal(st[x], one[x]) for x in one), sizes
    again = {k: v.copy() for k, v in one.items()}
    assert host_call(host, name, mode, gamma, n, bs, again, False, 9) == 0
    assert all(np.array_equal(again[x], one[x]) for x in one)


@pytest.mark.parametrize("mode", S.MODES)
def test_scores_below_the_mask_penalty_play_an_illegal_move(host, mode):
    """frac_bits 0 and every weight at INT32_MIN: V0 of a child with a legal move is about -5.2e10 (24 entries of -2^31), so is the
    mean over the children, and every Q1 of a legal move lies below the -1e8 of a move the mask forbids: the masked argmax takes the first
    illegal action wherever the board has one, as the engine's does.  That step ends the game with reward -1 and env_step's spawn.
    Every game of this network ends that way; some meet an illegal direction on their first board (length 1, score -1), the others
    first play legal moves on boards where all four directions are legal."""
    n, bs = 30, 10
    for gamma in S.GAMMAS:
        ref = S.case("floor", mode, gamma, n, bs)
        assert ref["illegal"].all()
        first, later = ref["ep_len"] == 1, ref["ep_len"] > 1
        assert first.any() and later.any() and (ref["score"][first] == -1).all() and (ref["score"][later] > -1).any()
        assert (ref["score"] >= -1).all() and (ref["masks"] == 0xF).all()
        for n_steps in STEPS:
            st, _ = host_play(host, "floor", mode, gamma, n, bs, n_steps)
            assert _same(st, ref), (gamma, n_steps)


def test_host_program_runs_clean_under_sanitizers(tmp_path):
    """The wave's code as a stand-alone program under ASan + UBSan on exactly sized arrays: an access outside a table, the list, the
    leaf array or a state array would abort it."""
    assert shutil.which("g++") is not None
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-static-libasan", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = str(tmp_path / "ntuple_search_episodes_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-DNTUPLE_SEARCH_EPISODES_HOST_MAIN", "-I", CSRC, "-o", exe, HOST_SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ntuple_search_episodes_host ok" in out.stdout, out.stderr[-2000:]
