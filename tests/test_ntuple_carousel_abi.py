"""Carousel shaping for the n-tuple trainer (g2048_ntuple_carousel_record / _restart): declared, bound, exported; every argument
check runs before any device work; the wrappers refuse host tensors; the trainer's settings and state without a device; the per-lane
code of the two kernels, compiled for the host, equals the numpy restatement (tests/ntuple_carousel_ref.py) bit for bit in both rng
modes; and the restatement's whole loop on the C oracle's env starts episodes at every stage.  CPU only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import ntuple_carousel_ref as K  # noqa: E402
import ntuple_ref as N  # noqa: E402
import ntuple_stage_ref as G  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = {"g2048_ntuple_carousel_record": 10, "g2048_ntuple_carousel_restart": 15}


def test_symbols_are_declared_bound_and_exported():
    from src.g2048 import native as nv

    header = open(os.path.join(ROOT, "include", "g2048.h")).read()
    lib = C.CDLL(nv.LIB_PATH)
    for name, nargs in NAMES.items():
        assert f"int {name}(" in header
        assert name in nv.SIGNATURES and len(nv.SIGNATURES[name]) == nargs
        assert hasattr(lib, name) and callable(getattr(nv, name.replace("g2048_", "")))
    assert nv.SIGNATURES["g2048_ntuple_carousel_restart"][:2] == [C.c_uint32, C.c_uint32]
    assert "#define G2048_ABI_VERSION 4" in header
    assert nv.load().g2048_abi_version() == 4  # additive: the version stays


def test_entry_points_reject_bad_arguments_without_touching_a_device():
    from src.g2048 import native as nv

    lib = nv.load()
    a = 1 << 20  # a fake, 16-byte aligned "device address": rejected before any use
    arrays = [np.array(x, np.uint8) for x in ([3, 5, 9], [5, 3, 9], [3, 3, 9], [0, 5, 9], [3, 5, 18], [1, 2, 3, 4, 5, 6, 7, 8])]
    ok, desc, equal, zero, high, eight = (x.ctypes.data for x in arrays)

    def record(boards=a, masks=a, flag=a, B=8, tiles=ok, n=3, reached=a, pool_boards=a, pool_masks=a):
        return lib.g2048_ntuple_carousel_record(boards, masks, flag, B, tiles, n, reached, pool_boards, pool_masks, None)

    def restart(flag=a, B=8, n=3, pool_boards=a, pool_masks=a, boards=a, masks=a, reached=a, turn=a, starts=a, start_stage=a, mode=1):
        return lib.g2048_ntuple_carousel_restart(1, 2, flag, B, n, pool_boards, pool_masks, boards, masks, reached, turn, starts,
                                                 start_stage, mode, None)

    size_bad = [dict(B=0), dict(B=-1), dict(B=(1 << 28) + 1), dict(n=0), dict(n=-1), dict(n=8)]
    own = {record: [dict(boards=None), dict(masks=None), dict(flag=None), dict(tiles=None), dict(reached=None), dict(pool_boards=None),
                    dict(pool_masks=None), dict(tiles=eight, n=8), dict(tiles=desc), dict(tiles=equal), dict(tiles=zero), dict(tiles=high),
                    dict(tiles=zero, n=1), dict(boards=a + 8), dict(pool_boards=a + 4), dict(pool_boards=a + 1)],
           restart: [dict(flag=None), dict(pool_boards=None), dict(pool_masks=None), dict(boards=None), dict(masks=None),
                     dict(reached=None), dict(turn=None), dict(starts=None), dict(mode=2), dict(mode=-1), dict(boards=a + 8),
                     dict(pool_boards=a + 8), dict(turn=a + 2), dict(turn=a + 1), dict(starts=a + 4), dict(starts=a + 1)]}
    for fn, more in own.items():
        for kw in size_bad + more:
            assert fn(**kw) == -1, (fn.__name__, kw)


def test_wrappers_refuse_host_tensors_and_wrong_shapes():
    import torch

    from src.g2048 import native as nv

    B, n, u8 = 4, 2, torch.uint8
    boards, masks, flag, reached = torch.zeros((B, 16), dtype=u8), torch.zeros(B, dtype=u8), torch.zeros(B, dtype=u8), torch.zeros(B, dtype=u8)
    pb, pm = torch.zeros((n, B, 16), dtype=u8), torch.zeros((n, B), dtype=u8)
    turn, starts = torch.zeros(B, dtype=torch.int32), torch.zeros(n + 1, dtype=torch.int64)
    sub = np.array([1, 2], np.uint32)
    calls = [lambda: nv.ntuple_carousel_record(boards, masks, flag, (3, 5), reached, pb, pm),
             lambda: nv.ntuple_carousel_restart(sub, flag, pb, pm, boards, masks, reached, turn, starts, 1),
             lambda: nv.ntuple_carousel_restart(sub, flag, pb, pm, boards, masks, reached, turn, starts, 1, torch.zeros(B, dtype=u8)),
             lambda: nv.ntuple_carousel_record(boards, masks, flag, ((3, 5),), reached, pb, pm),  # thresholds are a flat sequence
             lambda: nv.ntuple_carousel_record(boards, masks, flag, (3, 5, 7), reached, pb, pm),  # pools of another threshold count
             lambda: nv.ntuple_carousel_record(boards, masks, flag, (3, 5), reached, pb.reshape(n, B * 16), pm),
             lambda: nv.ntuple_carousel_restart(sub, flag, pb, pm, boards, masks, reached, turn, starts[:n], 1),
             lambda: nv.ntuple_carousel_restart(sub, flag, pb, pm[:, :3], boards, masks, reached, turn, starts, 1)]
    for call in calls:
        with pytest.raises(nv.NativeError):
            call()


# ---------------------------------------------------------------------------------------------- Python settings without a device
def test_trainer_settings_and_state_without_a_device():
    import torch

    from src.ppo import NTupleNetwork, NTupleTrainer

    plain = NTupleNetwork(N.SMALL, device="cpu")
    staged = NTupleNetwork(N.SMALL, device="cpu", stage_tiles=(3, 4, 5))
    with pytest.raises(ValueError):
        NTupleTrainer(plain, 4, carousel_tiles="stages")  # an unstaged network has no stages to take
    for bad in ((5, 3), (3, 3), (0, 3), (3, 18), (1, 2, 3, 4, 5, 6, 7, 8), True, (True, 3), (3.5,), (), 3, "stage", ("a",)):
        for net in (plain, staged):
            with pytest.raises(ValueError):
                NTupleTrainer(net, 4, carousel_tiles=bad)
    # off: nothing is allocated, and the state's keys are what they were
    off = NTupleTrainer(plain, 4)
    assert off.carousel_tiles is None
    assert all(getattr(off, k) is None for k in ("pool_boards", "pool_masks", "reached", "turn", "starts"))
    assert set(off.state_dict()) == {"learner", "alpha", "lock_steps"}
    assert "carousel_tiles" not in NTupleTrainer(staged, 4).state_dict()
    # "stages" takes the network's thresholds, all of them, whatever is active; a sequence works on any network
    on = NTupleTrainer(staged, 5, carousel_tiles="stages")
    assert on.carousel_tiles == (3, 4, 5) and staged.active_stages == 1
    own = NTupleTrainer(plain, 5, carousel_tiles=[4, np.uint8(6), 8], learner="tc")
    assert own.carousel_tiles == (4, 6, 8) and NTupleTrainer(staged, 5, carousel_tiles=(17,)).carousel_tiles == (17,)
    for tr, n in ((on, 3), (own, 3)):
        assert tr.pool_boards.shape == (n, 5, 16) and tr.pool_boards.dtype == torch.uint8 and not tr.pool_boards.any()
        assert tr.pool_masks.shape == (n, 5) and tr.pool_masks.dtype == torch.uint8 and not tr.pool_masks.any()
        assert tr.reached.shape == (5,) and tr.reached.dtype == torch.uint8 and not tr.reached.any()
        assert tr.turn.shape == (5,) and tr.turn.element_size() == 4 and not tr.turn.any()
        assert tr.starts.shape == (n + 1,) and tr.starts.dtype == torch.int64 and not tr.starts.any()
    # the state carries the thresholds only (the pools are env state), and another carousel's state is refused unchanged
    state = own.state_dict()
    assert state["carousel_tiles"] == (4, 6, 8) and set(state) == {"learner", "alpha", "lock_steps", "carousel_tiles", "coh_e", "coh_a"}
    assert set(on.state_dict()) == {"learner", "alpha", "lock_steps", "stages", "promotions", "carousel_tiles"}
    own.lock_steps = 24
    fresh = NTupleTrainer(plain, 8, carousel_tiles=(4, 6, 8), learner="tc")
    fresh.load_state_dict(own.state_dict())
    assert fresh.lock_steps == 24 and not fresh.pool_masks.any() and not fresh.starts.any()
    for other in (NTupleTrainer(plain, 4, learner="tc"), NTupleTrainer(plain, 4, carousel_tiles=(4, 6), learner="tc"),
                  NTupleTrainer(plain, 4, carousel_tiles=(4, 6, 9), learner="tc")):
        with pytest.raises(ValueError):
            other.load_state_dict(own.state_dict())
        assert other.lock_steps == 0
        with pytest.raises(ValueError):
            NTupleTrainer(plain, 4, carousel_tiles=(4, 6, 8), learner="tc").load_state_dict(other.state_dict())
    doc = NTupleTrainer.__doc__
    assert "start afresh on resume" in doc and "11.5 GB" in doc and "One lock-step is five launches" in doc


# ---------------------------------------------------------------------------------------------- the kernels' per-lane code on the host
HOST_SRC = os.path.join(ROOT, "tests", "host_swar", "ntuple_carousel_host.cpp")
CSRC = os.path.join(ROOT, "2048-ppo-agent_amd", "csrc")


@pytest.fixture(scope="module")
def host():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libntuple_carousel_host.so")
    subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", "-I", CSRC, "-o", so, HOST_SRC])
    return C.CDLL(so)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_record(lib, st, boards, masks, flag, tiles):
    """In place on st (a copy of the arrays goes in and comes back: the shared cases are not written)."""
    t = np.array(tiles, np.uint8)
    assert lib.hst_csl_record(_p(boards), _p(masks), _p(flag), C.c_int64(st.B), _p(t), C.c_int(len(t)), _p(st.reached), _p(st.pool_boards),
                              _p(st.pool_masks)) == 0


def host_restart(lib, st, sub, flag, boards, masks, mode, want_start=True):
    start = np.full(st.B, 0x77, np.uint8) if want_start else None
    assert lib.hst_csl_restart(C.c_uint32(int(sub[0])), C.c_uint32(int(sub[1])), _p(flag), C.c_int64(st.B), C.c_int(st.n), _p(st.pool_boards),
                               _p(st.pool_masks), _p(boards), _p(masks), _p(st.reached), _p(st.turn), _p(st.starts), _p(start),
                               C.c_int(mode)) == 0
    return start


def test_stage_equals_the_restatement_and_the_network_stage(host):
    """cs is nt_stage: tiles 16 and 17 against thresholds 16 and 17 at every cell, and random boards against ntuple_stage_ref."""
    boards = np.zeros((64, 16), np.uint8)
    for c in range(16):
        for j, k in enumerate((14, 15, 16, 17)):
            boards[4 * c + j, c] = k
            boards[4 * c + j, (c + 7) % 16] = 3
    rnd = np.ascontiguousarray(N.boards_for(200, seed=3))
    for tiles, bs in (((15, 16, 17), boards), (K.TILES, boards), (K.TILES, rnd), ((1, 2, 3, 4, 5, 6, 7), rnd), ((17,), boards)):
        t, out = np.array(tiles, np.uint8), np.full(len(bs), 99, np.uint8)
        assert host.hst_csl_stage(_p(bs), C.c_int64(len(bs)), _p(t), C.c_int(len(t)), _p(out)) == 0
        assert np.array_equal(out, K.cs(bs, tiles)) and np.array_equal(out, G.stage(bs, tiles))
    assert np.array_equal(K.cs(boards, (15, 16, 17)), np.tile([0, 1, 2, 3], 16))


@pytest.mark.parametrize("B", K.SIZES)
def test_record_equals_the_restatement(host, B):
    c = K.record_case(B)
    if B >= 63:
        cover = c["cover"]
        assert cover.pop("flags") == {0, 1, 2} and all(cover.values()), cover
    st = c["st0"].copy()
    host_record(host, st, c["boards"], c["masks"], c["flag"], K.TILES)
    assert st.equal(c["st"]) and not st.equal(c["st0"])


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("B", K.SIZES)
def test_restart_equals_the_restatement(host, B, mode):
    c = K.restart_case(B, mode)
    if B >= 63:
        cover = c["cover"]
        assert cover["pool"] == {1, 2, 3} and cover["fallback"] == {1, 2, 3} and cover["stage0"] and cover["wrapped"]
        assert cover["flags"] == {0, 1, 2}
    for want_start in (True, False):
        st, boards, masks = c["st0"].copy(), c["boards0"].copy(), c["masks0"].copy()
        start = host_restart(host, st, c["sub"], c["flag"], boards, masks, mode, want_start)
        assert st.equal(c["st"]) and np.array_equal(boards, c["boards"]) and np.array_equal(masks, c["masks"])
        assert start is None or np.array_equal(start, c["start_stage"])
    assert np.array_equal(st.pool_boards, c["st0"].pool_boards) and np.array_equal(st.pool_masks, c["st0"].pool_masks)


def test_the_two_rng_modes_draw_other_donors():
    a, b = (K.restart_case(257, mode) for mode in K.MODES)
    st, boards, masks = a["st0"].copy(), a["boards0"].copy(), a["masks0"].copy()
    other = K.restart(st, a["sub"], a["flag"], boards, masks, K.MODES[1])
    assert not np.array_equal(other, a["start_stage"]) and b is not None


@pytest.mark.parametrize("mode", K.MODES)
def test_restart_in_a_permuted_env_order(host, mode):
    """The restatement: the permuted input gives the permuted boards, masks and start stages and identical starts; the host build
    equals it on both inputs."""
    c = K.permuted_case()
    p = c["p"]
    ba, ma, sa, starts_a, ra = K.run_permuted(c, "a", mode)
    bb, mb, sb, starts_b, rb = K.run_permuted(c, "b", mode)
    assert np.array_equal(bb[p], ba) and np.array_equal(mb[p], ma) and np.array_equal(sb[p], sa) and np.array_equal(rb[p], ra)
    assert np.array_equal(starts_a, starts_b) and starts_a[2] == 0 and starts_a[0] > 0 and starts_a[1] > 0 and starts_a[3] > 0
    assert (ba != c["a"]["boards0"]).any()
    for which, (wb, wm, ws, wstarts, wr) in (("a", (ba, ma, sa, starts_a, ra)), ("b", (bb, mb, sb, starts_b, rb))):
        st = c["pools"].copy()
        st.turn = c[which]["turn"].copy()
        boards, masks = c[which]["boards0"].copy(), c[which]["masks0"].copy()
        start = host_restart(host, st, c["sub"], c[which]["flag"], boards, masks, mode)
        assert np.array_equal(boards, wb) and np.array_equal(masks, wm) and np.array_equal(start, ws)
        assert np.array_equal(st.starts, wstarts) and np.array_equal(st.reached, wr)


def test_host_program_runs_clean_under_sanitizers(tmp_path):
    """The per-lane code as a stand-alone program under ASan + UBSan on pools of exactly [n][B][16] and [n][B]: an index that left
    them would abort it."""
    exe = str(tmp_path / "ntuple_carousel_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-DNTUPLE_CAROUSEL_HOST_MAIN", "-I", CSRC, "-o", exe, HOST_SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ntuple_carousel_host ok" in out.stdout, (out.returncode, out.stderr[-2000:])


# ---------------------------------------------------------------------------------------------- the whole loop on the restatement
def test_the_restatement_loop_starts_episodes_at_every_stage():
    """The trainer's loop on the C oracle's env and the engine's key chain (SMALL, TD(0) at alpha 0.1, 65 envs, thresholds (4, 6, 8),
    600 lock-steps): every stage gets pool starts, some draws fall back, and a started env's ``reached`` is its stage."""
    w = N.zero_weights(N.SMALL)
    st, start, episodes = K.engine_training(w, N.SMALL, 65, 600, (4, 6, 8))
    f2 = start != K.NO_START
    print(f"{episodes} episodes, starts per stage {st.starts.tolist()}, first restart at lock-step {int(np.nonzero(f2.any(axis=1))[0][0])}")
    assert episodes == int(f2.sum()) == int(st.starts.sum()) and (st.starts[1:] > 0).all() and st.starts[0] > 0
    assert np.array_equal(np.bincount(start[f2], minlength=4), st.starts)
    assert int(st.turn.sum()) == episodes and (st.reached <= 3).all()
