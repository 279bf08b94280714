"""N-tuple TC learning (g2048_ntuple_tc_*): declared, bound, exported; every argument check runs before any device work; the wrappers
refuse host tensors and the trainer bad settings without a device; the per-lane code of the kernels, compiled for the host, equals the
numpy restatement (tests/ntuple_tc_ref.py) bit for bit; the restatement has the properties the definition promises.  CPU only."""
import ctypes as C
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import ntuple_ref as N  # noqa: E402
import ntuple_tc_ref as T  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = {"g2048_ntuple_tc_accumulate": 15, "g2048_ntuple_tc_apply": 13}
F32 = np.float32


def test_symbols_are_declared_bound_and_exported():
    from src.g2048 import native as nv

    header = open(os.path.join(ROOT, "include", "g2048.h")).read()
    lib = C.CDLL(nv.LIB_PATH)
    for name, nargs in NAMES.items():
        assert f"int {name}(" in header
        assert name in nv.SIGNATURES and len(nv.SIGNATURES[name]) == nargs
        assert hasattr(lib, name)
        assert callable(getattr(nv, name[len("g2048_"):]))
    assert "#define G2048_ABI_VERSION 4" in header
    assert nv.load().g2048_abi_version() == 4  # additive: the version stays


def test_entry_points_reject_bad_arguments_without_touching_a_device():
    from src.g2048 import native as nv

    lib = nv.load()
    a = 1 << 20  # a fake, 16-byte aligned "device address": rejected before any use
    good = np.array([[0, 1, 2], [4, 5, 6]], np.uint8)  # tuple_cells is a host pointer that the checks read: a real array
    hi = np.array([[0, 1, 2], [4, 16, 6]], np.uint8)
    dup = np.array([[0, 1, 2], [4, 6, 6]], np.uint8)
    gp = good.ctypes.data
    net_bad = [dict(cells=None), dict(m=0), dict(m=9), dict(L=0), dict(L=7), dict(cells=hi.ctypes.data), dict(cells=dup.ctypes.data)]
    frac_bad = [dict(F=-1), dict(F=21)]

    def accumulate(prev=a, flag=a, target=a, B=8, w=a, cells=gp, m=2, L=3, F=12, alpha=1.0, acc=a, abs_acc=a, cnt=a, err=a):
        return lib.g2048_ntuple_tc_accumulate(prev, flag, target, B, w, cells, m, L, F, alpha, acc, abs_acc, cnt, err, None)

    for kw in net_bad + frac_bad + [dict(prev=None), dict(flag=None), dict(target=None), dict(w=None), dict(acc=None),
                                    dict(abs_acc=None), dict(cnt=None), dict(B=0), dict(B=-3), dict(B=(1 << 28) + 1), dict(alpha=0.0),
                                    dict(alpha=-0.1), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(prev=a + 8),
                                    dict(target=a + 2), dict(w=a + 2), dict(acc=a + 4), dict(abs_acc=a + 4), dict(cnt=a + 2),
                                    dict(err=a + 1)]:
        assert accumulate(**kw) == -1, kw

    def apply(prev=a, flag=a, B=8, cells=gp, m=2, L=3, w=a, acc=a, abs_acc=a, cnt=a, coh_e=a, coh_a=a):
        return lib.g2048_ntuple_tc_apply(prev, flag, B, cells, m, L, w, acc, abs_acc, cnt, coh_e, coh_a, None)

    for kw in net_bad + [dict(prev=None), dict(flag=None), dict(w=None), dict(acc=None), dict(abs_acc=None), dict(cnt=None),
                         dict(coh_e=None), dict(coh_a=None), dict(B=0), dict(B=-1), dict(B=(1 << 28) + 1), dict(prev=a + 1),
                         dict(w=a + 2), dict(acc=a + 4), dict(abs_acc=a + 4), dict(cnt=a + 1), dict(coh_e=a + 2), dict(coh_a=a + 1)]:
        assert apply(**kw) == -1, kw


def test_wrappers_refuse_host_tensors():
    import torch

    from src.g2048 import native as nv

    B, cells = 4, np.array(N.SMALL, np.uint8)
    boards = torch.zeros((B, 16), dtype=torch.uint8)
    w = torch.zeros((3, 256), dtype=torch.int32)
    acc, cnt = torch.zeros((3, 256), dtype=torch.int64), torch.zeros((3, 256), dtype=torch.int32)
    flag, f = torch.zeros(B, dtype=torch.uint8), torch.zeros(B)
    with pytest.raises(nv.NativeError):
        nv.ntuple_tc_accumulate(boards, flag, f, w, cells, 12, 1.0, acc, acc.clone(), cnt, f)
    with pytest.raises(nv.NativeError):
        nv.ntuple_tc_apply(boards, flag, cells, w, acc, acc.clone(), cnt, cnt.clone(), cnt.clone())
    with pytest.raises(nv.NativeError):
        nv.ntuple_tc_apply(boards, flag, np.zeros(3, np.uint8), w, acc, acc.clone(), cnt, cnt.clone(), cnt.clone())  # cells is [m, L]


def test_trainer_settings_and_state_without_a_device():
    import torch

    from src.ppo import NTupleNetwork, NTupleTrainer

    net = NTupleNetwork(N.SMALL, device="cpu")
    for bad in ("x", "TC", None, 0):
        with pytest.raises(ValueError):
            NTupleTrainer(net, 4, learner=bad)
    with pytest.raises(ValueError):
        NTupleTrainer(None, 4, learner="tc")
    assert "2.3 GB" in NTupleTrainer.__doc__ and "alpha=1.0" in NTupleTrainer.__doc__
    td = NTupleTrainer(net, 4)
    assert td.learner == "td0" and td.abs_acc is None and td.coh_e is None and td.coh_a is None
    assert set(td.state_dict()) == {"learner", "alpha", "lock_steps"}
    with pytest.raises(ValueError):
        td.coherence()
    tc = NTupleTrainer(net, 4, alpha=1.0, learner="tc")
    assert tc.abs_acc.dtype == torch.int64 and tc.coh_e.dtype == torch.int32 and tc.coh_a.dtype == torch.int32
    assert tc.abs_acc.shape == tc.coh_e.shape == tc.coh_a.shape == net.weights.shape and not tc.coh_a.any()
    c = tc.coherence()
    assert int(c["entries"]) == 0 and float(c["mean_rate"]) == 0.0
    tc.coh_e[1, 7], tc.coh_a[1, 7], tc.coh_a[2, 0], tc.lock_steps = -3, 12, 5, 17
    c = tc.coherence()
    assert int(c["entries"]) == 2 and float(c["mean_rate"]) == 0.125
    state = tc.state_dict()
    assert state["learner"] == "tc" and state["alpha"] == 1.0 and state["lock_steps"] == 17
    fresh = NTupleTrainer(net, 8, alpha=0.5, learner="tc")
    fresh.load_state_dict(state)
    assert torch.equal(fresh.coh_e, tc.coh_e) and torch.equal(fresh.coh_a, tc.coh_a) and fresh.alpha == 1.0 and fresh.lock_steps == 17
    tc.coh_e[1, 7] = 9  # the state is a copy
    assert int(state["coh_e"][1, 7]) == -3
    with pytest.raises(ValueError):
        td.load_state_dict(state)  # another learner
    with pytest.raises(ValueError):
        fresh.load_state_dict(td.state_dict())
    other = NTupleTrainer(NTupleNetwork(((0, 1), (5, 6)), device="cpu"), 4, learner="tc")
    with pytest.raises(ValueError):
        other.load_state_dict(state)  # another shape
    assert not other.coh_a.any() and other.lock_steps == 0
    with pytest.raises(ValueError):
        fresh.load_state_dict(dict(state, coh_a=state["coh_a"].long()))


# ---------------------------------------------------------------------------------------------- the kernels' per-lane code on the host
HOST_SRC = os.path.join(ROOT, "tests", "host_swar", "ntuple_tc_host.cpp")
CSRC = os.path.join(ROOT, "2048-ppo-agent_amd", "csrc")


@pytest.fixture(scope="module")
def host():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libntuple_tc_host.so")
    subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", "-I", CSRC, "-o", so, HOST_SRC])
    return C.CDLL(so)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def host_tc_step(host, prev, flag, target, w, coh_e, coh_a, tuples, F, alpha):
    """accumulate + apply on the host build, in place on w, coh_e, coh_a -> td_error; acc, abs_acc and cnt must be zero after."""
    cells = N.cells_array(tuples)
    m, L = cells.shape
    B = len(prev)
    acc, abs_acc, cnt = np.zeros(w.shape, np.int64), np.zeros(w.shape, np.int64), np.zeros(w.shape, np.int32)
    err = np.full(B, -7, F32)
    host.hst_nt_tc_accumulate(_p(prev), _p(flag), _p(target), C.c_int64(B), _p(w), _p(cells), C.c_int(m), C.c_int(L), C.c_int(F),
                              C.c_double(alpha), _p(acc), _p(abs_acc), _p(cnt), _p(err))
    assert (cnt >= 0).all() and cnt.sum() == 8 * m * int((flag != 0).sum())
    assert (abs_acc >= np.abs(acc)).all()
    host.hst_nt_tc_apply(_p(prev), _p(flag), C.c_int64(B), _p(cells), C.c_int(m), C.c_int(L), _p(w), _p(acc), _p(abs_acc), _p(cnt),
                         _p(coh_e), _p(coh_a))
    assert not acc.any() and not abs_acc.any() and not cnt.any()
    return err


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("tuples,F", T.CASES)
def test_one_step_from_zero_coherence_equals_the_restatement(host, tuples, F):
    prev, flag, target, w0 = T.one_step_inputs(tuples, F)
    assert set(flag.tolist()) == {0, 1, 2} and prev.max() == 17
    want, (want_e, want_a) = w0.copy(), T.zero_coherence(w0)
    want_err = T.tc_step(prev, flag, target, want, want_e, want_a, tuples, F, 0.1)
    w, (ce, ca) = w0.copy(), T.zero_coherence(w0)
    err = host_tc_step(host, prev, flag, target, w, ce, ca, tuples, F, 0.1)
    assert _same((w, ce, ca, _bits(err)), (want, want_e, want_a, _bits(want_err)))
    assert (w != w0).any() and ca.any() and (_bits(err[flag == 0]) == 0).all()


def test_step_under_collision_equals_the_restatement_and_td0(host):
    c = N.collision_case()
    want, (want_e, want_a) = N.small_weights().copy(), T.zero_coherence(N.small_weights())
    want_err = T.tc_step(c["prev"], c["flag"], c["target"], want, want_e, want_a, N.SMALL, 12, 0.1)
    w, (ce, ca) = N.small_weights().copy(), T.zero_coherence(N.small_weights())
    err = host_tc_step(host, c["prev"], c["flag"], c["target"], w, ce, ca, N.SMALL, 12, 0.1)
    assert _same((w, ce, ca, _bits(err)), (want, want_e, want_a, _bits(want_err)))
    # from zero coherence the rate is 1 everywhere: exactly the weights of ntuple_ref.td_step
    assert np.array_equal(want, c["weights_after"]) and np.array_equal(_bits(want_err), _bits(c["td_error"]))
    assert (np.abs(want_e) < want_a).any()  # the envs of the one lock-step disagreed somewhere: a rate below 1 from then on


@pytest.mark.parametrize("alpha,scale,extreme", [(0.1, 500.0, False), (1000.0, 1e9, True)])
def test_six_steps_equal_the_restatement(host, alpha, scale, extreme):
    """Six consecutive steps on the same 200 boards: rates below 1 are read; with alpha = 1000, targets of 1e9 and weights preset near
    +-2^31 the weights saturate, delta sits on the +-2^30 clamp and A is halved."""
    c = T.sequence_case(alpha, scale, extreme)
    assert c["stats"]["slowed"] > 0
    if extreme:
        assert c["stats"]["saturated"] > 0 and c["stats"]["clamped"] > 0 and c["stats"]["halved"] > 0
        last = c["after"][-1]["weights"]
        assert (last == 2 ** 31 - 1).any() and (last == -2 ** 31).any()
    w, (ce, ca) = c["w0"].copy(), T.zero_coherence(c["w0"])
    for t, want in enumerate(c["after"]):
        err = host_tc_step(host, c["prev"], c["flag"], c["targets"][t], w, ce, ca, N.SMALL, 12, alpha)
        assert _same((w, ce, ca, _bits(err)), (want["weights"], want["coh_e"], want["coh_a"], _bits(want["td_error"]))), t


def test_one_step_on_wide_tables(host):
    rng = np.random.default_rng(11)
    prev = N.boards_for(65, seed=12)
    flag = rng.integers(0, 3, 65).astype(np.uint8)
    target = (rng.standard_normal(65) * 800).astype(F32)
    want, (want_e, want_a) = N.wide_weights().copy(), T.zero_coherence(N.wide_weights())
    want_err = T.tc_step(prev, flag, target, want, want_e, want_a, N.WIDE, 12, 0.1)
    w, (ce, ca) = N.wide_weights().copy(), T.zero_coherence(N.wide_weights())
    err = host_tc_step(host, prev, flag, target, w, ce, ca, N.WIDE, 12, 0.1)
    assert _same((w, ce, ca, _bits(err)), (want, want_e, want_a, _bits(want_err)))
    assert (w != N.wide_weights()).any()


def test_host_program_runs_clean_under_sanitizers(tmp_path):
    """The per-lane code as a stand-alone program under ASan + UBSan: an index that left a table or a signed overflow would abort it."""
    exe = str(tmp_path / "ntuple_tc_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-DNTUPLE_TC_HOST_MAIN", "-I", CSRC, "-o", exe, HOST_SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ntuple_tc_host ok" in out.stdout, out.stderr[-2000:]


# ---------------------------------------------------------------------------------------------- properties of the restatement
def test_the_first_step_is_td0():
    for tuples, F in T.CASES[:2]:
        prev, flag, target, w0 = T.one_step_inputs(tuples, F, n=120)
        td = w0.copy()
        td_err = N.td_step(prev, flag, target, td, tuples, F, 0.1)
        tc, (ce, ca) = w0.copy(), T.zero_coherence(w0)
        tc_err = T.tc_step(prev, flag, target, tc, ce, ca, tuples, F, 0.1)
        assert np.array_equal(tc, td) and np.array_equal(_bits(tc_err), _bits(td_err)) and (td != w0).any()


def _single(weights, ce, ca, i, deltas):
    """One step on the flat entry i hit by ``deltas`` -> the entry's move."""
    acc, abs_acc, cnt = np.zeros(weights.shape, np.int64), np.zeros(weights.shape, np.int64), np.zeros(weights.shape, np.int32)
    acc.reshape(-1)[i], abs_acc.reshape(-1)[i], cnt.reshape(-1)[i] = sum(deltas), sum(abs(d) for d in deltas), len(deltas)
    before = int(weights.reshape(-1)[i])
    T.tc_apply(weights, acc, abs_acc, cnt, ce, ca, np.array([i]))
    assert not acc.any() and not abs_acc.any() and not cnt.any()
    return int(weights.reshape(-1)[i]) - before


def test_an_entry_whose_deltas_agree_keeps_rate_one():
    """Through the whole step: a board that hits entry 3 | 2 << 4 once, alone, with a target far above V at every step."""
    tuples, F = ((0, 1),), 4
    prev = np.zeros((1, 16), np.uint8)
    prev[0, 0], prev[0, 1] = 3, 2
    i = 3 | (2 << 4)
    assert (T.hit_entries(prev, np.ones(1, np.uint8), tuples) == i).sum() == 1
    w = N.zero_weights(tuples)
    ce, ca = T.zero_coherence(w)
    for t in range(8):
        target = np.array([1e4 * (t + 1)], F32)
        delta, _ = N.td_deltas(prev, np.ones(1, np.uint8), target, w, tuples, F, 1.0)
        before = int(w[0, i])
        T.tc_step(prev, np.ones(1, np.uint8), target, w, ce, ca, tuples, F, 1.0)
        assert delta[0] > 0 and int(w[0, i]) - before == int(delta[0]) and abs(int(ce[0, i])) == int(ca[0, i]) > 0


def test_an_entry_whose_deltas_alternate_slows_down():
    """+x, -x, +x, ...: by the rule E is x, 0, x, 0, ... and A is x, 2x, 3x, ... after the steps, so the rates read are 1 (A == 0), 1, 0,
    1/3, 0, 1/5, ... and the moves x, -x, 0, -x/3, 0, -x/5, ...: ever smaller."""
    x = 3000
    w = np.zeros((1, 16), np.int32)
    ce, ca = T.zero_coherence(w)
    moves = [_single(w, ce, ca, 5, [x if t % 2 == 0 else -x]) for t in range(8)]
    assert moves == [x, -x, 0, -1000, 0, -600, 0, -429]  # 3000 / 7 = 428.57
    assert int(ce[0, 5]) == 0 and int(ca[0, 5]) == 8 * x
    # disagreement inside one lock-step lowers the rate too: the mean of +x and -x is 0 but the mean magnitude is x
    w2 = np.zeros((1, 16), np.int32)
    e2, a2 = T.zero_coherence(w2)
    assert _single(w2, e2, a2, 5, [x, -x]) == 0 and int(e2[0, 5]) == 0 and int(a2[0, 5]) == x
    assert _single(w2, e2, a2, 5, [x]) == 0  # rate 0


def test_the_halving_keeps_the_rate():
    """A + a in [2^31, 2^31 + 2^30): one halving; |E| / A changes by at most 1 / (A - 1) < 2^-30, and |E| <= A < 2^31 after."""
    rng = np.random.default_rng(0)
    n = 2000
    w = np.zeros((1, n), np.int32)
    A0 = (2 ** 31 - 1 - rng.integers(0, 2 ** 29, n)).astype(np.int64)
    A0[:4] = 2 ** 31 - 1
    E0 = (rng.integers(-1000, 1001, n) * A0 // 1000).astype(np.int64)
    d = rng.integers(-2 ** 30, 2 ** 30 + 1, n).astype(np.int64)
    d[:4] = [2 ** 30, -2 ** 30, 1, 0]
    a = np.maximum(np.abs(d), 2 ** 31 - A0)  # a >= |d| and A0 + a >= 2^31
    a[:2] = 2 ** 30
    assert (a <= 2 ** 30).all() and (np.abs(E0) <= A0).all()
    ce, ca = E0.astype(np.int32).reshape(1, n), A0.astype(np.int32).reshape(1, n)
    acc, abs_acc, cnt = d.reshape(1, n).copy(), a.reshape(1, n).copy(), np.ones((1, n), np.int32)
    stats = {}
    T.tc_apply(w, acc, abs_acc, cnt, ce, ca, np.arange(n), stats)
    assert stats["halved"] == n
    for k in range(n):
        before = Fraction(abs(int(E0[k] + d[k])), int(A0[k] + a[k]))
        after = Fraction(abs(int(ce[0, k])), int(ca[0, k]))
        assert abs(after - before) <= Fraction(1, 2 ** 30), k
        assert abs(int(ce[0, k])) <= int(ca[0, k]) < 2 ** 31 and int(ca[0, k]) == (int(A0[k] + a[k]) >> 1)
        assert (int(ce[0, k]) >= 0) == (int(E0[k] + d[k]) >= 0) or int(ce[0, k]) == 0


def test_the_restatement_learns_with_tc():
    """300 lock-steps of the CPU loop on a small network at alpha = 1 (at 150 no episode has ended yet): episodes end, the weights
    move and stay bounded, rates below 1 appear."""
    tuples = ((0, 1, 2), (4, 5, 6))
    w = N.zero_weights(tuples)
    ce, ca = T.zero_coherence(w)
    episodes = T.simulate_training(w, tuples, 64, 300, alpha=1.0, seed=0, learner="tc", coh_e=ce, coh_a=ca)
    entries, rate = T.coherence(ce, ca)
    assert episodes > 0 and w.any() and np.abs(w).max() < 2 ** 30 and entries > 0 and 0.0 < rate < 1.0
