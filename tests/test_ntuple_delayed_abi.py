"""Delayed TD(lambda) / TC(lambda) on the n-tuple network (g2048_ntuple_delayed_*): declared, bound, exported; every argument check runs
before any device work; the wrappers refuse host tensors and the trainer bad settings without a device; the per-lane code of the
kernels, compiled for the host, equals the numpy restatement (tests/ntuple_delayed_ref.py) bit for bit; the restatement has the
properties the definition promises.  CPU only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import ntuple_delayed_ref as D  # noqa: E402
import ntuple_ref as N  # noqa: E402
import ntuple_tc_ref as T  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = {"g2048_ntuple_delayed_accumulate": 22, "g2048_ntuple_delayed_apply": 18, "g2048_ntuple_delayed_link": 10}
F32 = np.float32
LEARNERS = [("td0", 0.1), ("tc", 1.0)]


def test_symbols_are_declared_bound_and_exported():
    from src.g2048 import native as nv

    header = open(os.path.join(ROOT, "include", "g2048.h")).read()
    lib = C.CDLL(nv.LIB_PATH)
    for name, nargs in NAMES.items():
        assert f"int {name}(" in header
        assert name in nv.SIGNATURES and len(nv.SIGNATURES[name]) == nargs
        assert hasattr(lib, name)
        assert callable(getattr(nv, name[len("g2048_"):]))
    assert "n-tuple delayed TD(lambda)" in header
    assert "#define G2048_ABI_VERSION 4" in header
    assert nv.load().g2048_abi_version() == 4  # additive: the version stays


def test_entry_points_reject_bad_arguments_without_touching_a_device():
    from src.g2048 import native as nv

    lib = nv.load()
    a = 1 << 20  # a fake, 16-byte aligned "device address": rejected before any use
    good = np.array([[0, 1, 2], [4, 5, 6]], np.uint8)  # tuple_cells and stage_tiles are host pointers that the checks read
    hi = np.array([[0, 1, 2], [4, 16, 6]], np.uint8)
    dup = np.array([[0, 1, 2], [4, 6, 6]], np.uint8)
    tiles, desc, big = np.array([3, 9], np.uint8), np.array([9, 3], np.uint8), np.array([3, 18], np.uint8)
    gp, tp = good.ctypes.data, tiles.ctypes.data
    net_bad = [dict(cells=None), dict(m=0), dict(m=9), dict(L=0), dict(L=7), dict(cells=hi.ctypes.data), dict(cells=dup.ctypes.data),
               dict(S=0), dict(S=9), dict(S=3, tiles=None), dict(S=3, tiles=desc.ctypes.data), dict(S=3, tiles=big.ctypes.data)]
    ring_bad = [dict(h=0), dict(h=9), dict(h=-1), dict(pos=-1), dict(pos=4), dict(h=1, pos=1), dict(h=8, pos=8)]
    size_bad = [dict(B=0), dict(B=-3), dict(B=(1 << 28) + 1)]

    def accumulate(hist=a, herr=a, hlen=a, flag=a, target=a, B=8, h=4, pos=3, lam=0.5, w=a, cells=gp, m=2, L=3, tiles=None, S=1, F=12,
                   alpha=1.0, acc=a, abs_acc=a, cnt=a, err=a):
        return lib.g2048_ntuple_delayed_accumulate(hist, herr, hlen, flag, target, B, h, pos, lam, w, cells, m, L, tiles, S, F, alpha, acc,
                                                   abs_acc, cnt, err, None)

    for kw in net_bad + ring_bad + size_bad + [
            dict(hist=None), dict(herr=None), dict(hlen=None), dict(flag=None), dict(target=None), dict(w=None), dict(acc=None),
            dict(cnt=None), dict(lam=-0.01), dict(lam=1.01), dict(lam=float("nan")), dict(lam=float("inf")), dict(lam=-float("inf")),
            dict(F=-1), dict(F=21), dict(alpha=0.0), dict(alpha=-0.1), dict(alpha=float("nan")), dict(alpha=float("inf")),
            dict(hist=a + 8), dict(herr=a + 2), dict(target=a + 2), dict(w=a + 2), dict(acc=a + 4), dict(abs_acc=a + 4), dict(cnt=a + 2),
            dict(err=a + 1)]:
        assert accumulate(**kw) == -1, kw

    def apply(hist=a, hlen=a, flag=a, B=8, h=4, pos=0, cells=gp, m=2, L=3, tiles=tp, S=3, w=a, acc=a, abs_acc=a, cnt=a, coh_e=a, coh_a=a):
        return lib.g2048_ntuple_delayed_apply(hist, hlen, flag, B, h, pos, cells, m, L, tiles, S, w, acc, abs_acc, cnt, coh_e, coh_a, None)

    mixed = [dict(abs_acc=None), dict(coh_e=None), dict(coh_a=None), dict(abs_acc=None, coh_e=None), dict(abs_acc=None, coh_a=None),
             dict(coh_e=None, coh_a=None)]
    for kw in net_bad + ring_bad + size_bad + mixed + [
            dict(hist=None), dict(hlen=None), dict(flag=None), dict(w=None), dict(acc=None), dict(cnt=None), dict(hist=a + 1),
            dict(w=a + 2), dict(acc=a + 4), dict(abs_acc=a + 4), dict(cnt=a + 1), dict(coh_e=a + 2), dict(coh_a=a + 1)]:
        assert apply(**kw) == -1, kw

    def link(row=a, meta=a, B=8, h=4, pos=2, prev=a, flag=a, hist=a, hlen=a):
        return lib.g2048_ntuple_delayed_link(row, meta, B, h, pos, prev, flag, hist, hlen, None)

    for kw in ring_bad + size_bad + [dict(row=None), dict(meta=None), dict(prev=None), dict(flag=None), dict(hist=None), dict(hlen=None),
                                     dict(row=a + 8), dict(prev=a + 4), dict(hist=a + 1)]:
        assert link(**kw) == -1, kw


def test_wrappers_refuse_host_tensors_and_wrong_shapes():
    import torch

    from src.g2048 import native as nv

    B, h, cells = 4, 3, np.array(N.SMALL, np.uint8)
    hist, herr, hlen = torch.zeros((h, B, 16), dtype=torch.uint8), torch.zeros((h, B)), torch.zeros(B, dtype=torch.uint8)
    w = torch.zeros((3, 256), dtype=torch.int32)
    acc, cnt = torch.zeros((3, 256), dtype=torch.int64), torch.zeros((3, 256), dtype=torch.int32)
    flag, f, prev = torch.zeros(B, dtype=torch.uint8), torch.zeros(B), torch.zeros((B, 16), dtype=torch.uint8)
    with pytest.raises(nv.NativeError):
        nv.ntuple_delayed_accumulate(hist, herr, hlen, flag, f, 0, 0.5, w, cells, 12, 1.0, acc, None, cnt, f)
    with pytest.raises(nv.NativeError):
        nv.ntuple_delayed_apply(hist, hlen, flag, 0, cells, w, acc, None, cnt, None, None)
    with pytest.raises(nv.NativeError):
        nv.ntuple_delayed_link(prev, flag, 0, prev.clone(), flag.clone(), hist, hlen)
    with pytest.raises(nv.NativeError, match="hist"):
        nv.ntuple_delayed_link(prev, flag, 0, prev.clone(), flag.clone(), hist[:, :3], hlen)  # the ring is [h, B, 16] exactly
    with pytest.raises(nv.NativeError, match="hist"):
        nv.ntuple_delayed_apply(hist.reshape(h * B, 16), hlen, flag, 0, cells, w, acc, None, cnt, None, None)


def test_trainer_settings_and_state_without_a_device():
    import torch

    from src.ppo import NTupleNetwork, NTupleTrainer
    from src.ppo import ntuple as nt

    net = NTupleNetwork(N.SMALL, device="cpu")
    for kw in (dict(horizon=2), dict(lam=-0.1), dict(lam=1.5), dict(lam=float("nan")), dict(lam=True), dict(lam="0.5"),
               dict(lam=0.5, horizon=0), dict(lam=0.5, horizon=9), dict(lam=0.5, horizon=True), dict(lam=0.5, horizon=2.0)):
        with pytest.raises(ValueError):
            NTupleTrainer(net, 4, **kw)
    assert [nt.default_horizon(x) for x in (0.0, 0.1, 0.3, 0.5, 0.7, 0.75, 0.9, 1.0)] == [1, 1, 2, 4, 7, 8, 8, 8]
    assert [D.default_horizon(x) for x in (0.0, 0.1, 0.3, 0.5, 0.7, 0.75, 0.9, 1.0)] == [1, 1, 2, 4, 7, 8, 8, 8]
    for word in ("lam", "horizon", "hist_err", "flushed"):
        assert word in NTupleTrainer.__doc__
    off = NTupleTrainer(net, 4)
    assert off.lam is None and off.horizon is None and off.hist is None and off.hist_err is None and off.hist_len is None
    assert set(off.state_dict()) == {"learner", "alpha", "lock_steps"}
    on = NTupleTrainer(net, 4, lam=0.5)
    assert on.lam == 0.5 and on.horizon == 4 and NTupleTrainer(net, 4, lam=0).horizon == 1
    assert on.hist.shape == (4, 4, 16) and on.hist.dtype == torch.uint8 and on.hist_err.shape == (4, 4) and on.hist_err.dtype == torch.float32
    assert on.hist_len.shape == (4,) and on.hist_len.dtype == torch.uint8 and not on.hist.any() and not on.hist_err.any()
    assert on.prev_after.shape == (4, 16)
    on.lock_steps = 17
    state = on.state_dict()
    assert state["lam"] == 0.5 and state["horizon"] == 4 and set(state) == {"learner", "alpha", "lock_steps", "lam", "horizon"}
    fresh = NTupleTrainer(net, 8, alpha=0.5, lam=0.5, horizon=4)
    fresh.load_state_dict(state)
    assert fresh.lock_steps == 17 and fresh.alpha == 0.1 and not fresh.hist_len.any()
    for other in (off, NTupleTrainer(net, 4, lam=0.25, horizon=4), NTupleTrainer(net, 4, lam=0.5, horizon=3)):
        before = (other.alpha, other.lock_steps)
        with pytest.raises(ValueError):
            other.load_state_dict(state)
        assert (other.alpha, other.lock_steps) == before
    with pytest.raises(ValueError):
        on.load_state_dict(off.state_dict())  # none counts as other
    assert on.lock_steps == 17
    tc = NTupleTrainer(net, 4, alpha=1.0, learner="tc", lam=1.0, horizon=8)
    assert tc.hist.shape == (8, 4, 16) and tc.abs_acc is not None
    tc2 = NTupleTrainer(net, 4, alpha=1.0, learner="tc", lam=1.0)
    tc2.load_state_dict(tc.state_dict())


# ---------------------------------------------------------------------------------------------- the kernels' per-lane code on the host
HOST_SRC = os.path.join(ROOT, "tests", "host_swar", "ntuple_delayed_host.cpp")
CSRC = os.path.join(ROOT, "2048-ppo-agent_amd", "csrc")


@pytest.fixture(scope="module")
def host():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libntuple_delayed_host.so")
    subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", "-I", CSRC, "-o", so, HOST_SRC])
    return C.CDLL(so)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def host_step(host, ring, flag, target, head, lam, w, tuples, F, alpha, tiles=(), learner="td0", coh_e=None, coh_a=None):
    """accumulate + apply on the host build, in place on ring.err, w, coh_e, coh_a -> td_error; the accumulators must be zero after,
    and the ring's boards and lengths untouched."""
    cells = N.cells_array(tuples)
    m, L = cells.shape
    B, h = ring.B, ring.h
    st = np.array(tiles, np.uint8) if len(tiles) else None
    acc, cnt = np.zeros(w.shape, np.int64), np.zeros(w.shape, np.int32)
    abs_acc = np.zeros(w.shape, np.int64) if learner == "tc" else None
    err = np.full(B, -7, F32)
    hist0, len0 = ring.hist.copy(), ring.len.copy()
    host.hst_nt_dl_accumulate(_p(ring.hist), _p(ring.err), _p(ring.len), _p(flag), _p(target), C.c_int64(B), C.c_int(h), C.c_int(head),
                              C.c_double(lam), _p(w), _p(cells), C.c_int(m), C.c_int(L), _p(st), C.c_int(len(tiles) + 1), C.c_int(F),
                              C.c_double(alpha), _p(acc), _p(abs_acc), _p(cnt), _p(err))
    assert (cnt >= 0).all() and cnt.sum() % (8 * m) == 0
    if learner == "tc":
        assert (abs_acc >= np.abs(acc)).all()
    host.hst_nt_dl_apply(_p(ring.hist), _p(ring.len), _p(flag), C.c_int64(B), C.c_int(h), C.c_int(head), _p(cells), C.c_int(m), C.c_int(L),
                         _p(st), C.c_int(len(tiles) + 1), _p(w), _p(acc), _p(abs_acc), _p(cnt), _p(coh_e if learner == "tc" else None),
                         _p(coh_a if learner == "tc" else None))
    assert not acc.any() and not cnt.any() and (abs_acc is None or not abs_acc.any())
    assert np.array_equal(ring.hist, hist0) and np.array_equal(ring.len, len0)
    return err


def both_steps(host, case, head, lam, tuples, F, alpha, tiles, learner):
    """One step of the restatement and one of the host build from the same case -> its stats; asserts equal bits."""
    stats = {}
    want_ring, want = case["ring"].copy(), case["w0"].copy()
    want_e, want_a = T.zero_coherence(want)
    want_e[...] = 1000  # a rate of 1000 / 4000 wherever TC reads one
    want_a[...] = 4000
    want_err = D.step(want_ring, case["flag"], case["target"], head, lam, want, tuples, F, alpha, tiles, learner, want_e, want_a, stats)
    ring, w = case["ring"].copy(), case["w0"].copy()
    ce, ca = np.full(w.shape, 1000, np.int32), np.full(w.shape, 4000, np.int32)
    err = host_step(host, ring, case["flag"], case["target"], head, lam, w, tuples, F, alpha, tiles, learner, ce, ca)
    assert np.array_equal(w, want) and np.array_equal(_bits(err), _bits(want_err)) and np.array_equal(_bits(ring.err), _bits(want_ring.err))
    if learner == "tc":
        assert np.array_equal(ce, want_e) and np.array_equal(ca, want_a)
    stats["moved"] = bool((w != case["w0"]).any())
    return stats


@pytest.mark.parametrize("learner,alpha", LEARNERS)
@pytest.mark.parametrize("lam", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("h", [1, 2, 3, 8])
@pytest.mark.parametrize("B", [1, 257])
def test_one_step_at_every_ring_position_equals_the_restatement(host, B, h, lam, learner, alpha):
    """SMALL (m = 3, L = 2), ``head`` at every ring position (the wrap included), hist_len at every value 0 .. h under flags 0, 1 and
    2 (asserted on the case), the due-at-h state and flushes shorter than h, one env with the same board at every ring position."""
    case = D.ring_case(N.SMALL, 12, h, B)
    if B == 257:
        seen = set(zip(case["flag"].tolist(), case["ring"].len.tolist()))
        assert seen >= {(f, n) for f in (0, 1, 2) for n in range(h + 1)}
        assert (case["ring"].hist[:, 1] == case["ring"].hist[0, 1]).all() and case["flag"][1] == 2 and case["ring"].len[1] == h
        assert case["ring"].hist.max() == 17
    total = {}
    for head in range(h):
        for k, v in both_steps(host, case, head, lam, N.SMALL, 12, alpha, (), learner).items():
            total[k] = total.get(k, 0) + v
    if B == 257:
        assert total["moved"] == h and total["due"] > 0 and (h == 1 or total["flushed_short"] > 0)  # h = 1: no ring is shorter


@pytest.mark.parametrize("learner,alpha", LEARNERS)
@pytest.mark.parametrize("tuples,F", D.SHAPES)
def test_every_table_shape_equals_the_restatement(host, tuples, F, learner, alpha):
    """(m, L) in (1, 2), (3, 2), (8, 2), (2, 6) at h = 3, lam = 0.5, every head."""
    assert (len(tuples), len(tuples[0])) in {(1, 2), (3, 2), (8, 2), (2, 6)}
    case = D.ring_case(tuples, F, 3, 65 if len(tuples[0]) == 6 else 257)
    for head in range(3):
        assert both_steps(host, case, head, 0.5, tuples, F, alpha, (), learner)["moved"]


@pytest.mark.parametrize("learner,alpha", LEARNERS)
@pytest.mark.parametrize("h", [2, 3, 8])
def test_staged_network_uses_the_stage_of_the_updated_board(host, h, learner, alpha):
    """Three stages; env 0 holds a top-stage board between stage-0 neighbours and is flushed: the top stage's tables move."""
    case = D.ring_case(N.SMALL, 12, h, 257, tiles=D.STAGE_TILES)
    from ntuple_stage_ref import stage
    assert stage(case["ring"].hist[:, 0], D.STAGE_TILES).tolist().count(2) == 1 and case["flag"][0] == 2
    for head in range(h):
        both_steps(host, case, head, 0.5, N.SMALL, 12, alpha, D.STAGE_TILES, learner)
    want = case["w0"].copy()
    D.step(case["ring"].copy(), case["flag"], case["target"], 0, 0.5, want, N.SMALL, 12, 0.1, D.STAGE_TILES, "td0")
    assert all((want[s] != case["w0"][s]).any() for s in range(3))


@pytest.mark.parametrize("learner", ["td0", "tc"])
def test_errors_on_the_clamp(host, learner):
    """Errors of 1e9 at alpha 1000: delta sits on +-2^30 (counted by the restatement) and the weights saturate."""
    case = D.ring_case(N.SMALL, 12, 3, 257, scale=1e9)
    stats = both_steps(host, case, 1, 1.0, N.SMALL, 12, 1000.0, (), learner)
    assert stats["clamped"] > 0 and stats["moved"]


@pytest.mark.parametrize("learner,alpha", LEARNERS)
def test_collision_across_envs_in_two_lane_orders(host, learner, alpha):
    """200 of 600 envs hold identical rings, so their due states hit the same entries; the same envs in another order give the same
    tables and the permuted td_error and hist_err."""
    c = D.collision_case()
    assert np.unique(c["ring"].hist.transpose(1, 0, 2).reshape(600, -1), axis=0, return_counts=True)[1].max() >= 200
    perm = np.random.default_rng(1).permutation(600)
    results = []
    for case in (c, D.permuted(c, perm)):
        want_ring, want = case["ring"].copy(), N.small_weights().copy()
        want_e, want_a = T.zero_coherence(want)
        want_err = D.step(want_ring, case["flag"], case["target"], 2, 0.5, want, N.SMALL, 12, alpha, (), learner, want_e, want_a)
        ring, w = case["ring"].copy(), N.small_weights().copy()
        ce, ca = T.zero_coherence(w)
        err = host_step(host, ring, case["flag"], case["target"], 2, 0.5, w, N.SMALL, 12, alpha, (), learner, ce, ca)
        assert np.array_equal(w, want) and np.array_equal(ce, want_e) and np.array_equal(ca, want_a)
        assert np.array_equal(_bits(err), _bits(want_err)) and np.array_equal(_bits(ring.err), _bits(want_ring.err))
        results.append((w, ce, ca, err, ring.err))
    (w1, e1, a1, err1, herr1), (w2, e2, a2, err2, herr2) = results
    assert np.array_equal(w1, w2) and np.array_equal(e1, e2) and np.array_equal(a1, a2) and (w1 != N.small_weights()).any()
    assert np.array_equal(_bits(err1[perm]), _bits(err2)) and np.array_equal(_bits(herr1[:, perm]), _bits(herr2))


@pytest.mark.parametrize("learner", ["td0", "tc"])
def test_six_lock_steps_with_link_equal_the_restatement(host, learner):
    c = D.sequence_case(learner)
    ring, flag, w = c["ring0"].copy(), c["flag0"].copy(), c["w0"].copy()
    ce, ca = T.zero_coherence(w)
    prev = np.zeros((ring.B, 16), np.uint8)
    ends = 0
    for t, ((row, meta, target, head, slot), want) in enumerate(zip(c["rows"], c["after"])):
        err = host_step(host, ring, flag, target, head, c["lam"], w, N.SMALL, 12, c["alpha"], (), learner, ce, ca)
        host.hst_nt_dl_link(_p(row), _p(meta), C.c_int64(ring.B), C.c_int(ring.h), C.c_int(slot), _p(prev), _p(flag), _p(ring.hist),
                            _p(ring.len))
        ends += int((flag == 2).sum())
        assert np.array_equal(w, want["weights"]) and np.array_equal(_bits(err), _bits(want["td_error"])), t
        assert np.array_equal(ce, want["coh_e"]) and np.array_equal(ca, want["coh_a"]), t
        assert np.array_equal(ring.hist, want["ring"].hist) and np.array_equal(ring.len, want["ring"].len), t
        assert np.array_equal(_bits(ring.err), _bits(want["ring"].err)), t
        assert np.array_equal(prev, want["prev"]) and np.array_equal(flag, want["flag"]), t
        assert np.array_equal(prev, ring.hist[slot]) and ring.len.min() >= 1 and ring.len.max() <= ring.h
    assert ends > 0 and (c["after"][-1]["ring"].len == 1).any()  # a ring restarted after an episode end


@pytest.mark.parametrize("learner,alpha", LEARNERS)
@pytest.mark.parametrize("lam", [0.0, 0.7])
def test_horizon_one_is_the_plain_learner(host, lam, learner, alpha):
    """h = 1: the delayed lanes on the ring [1][B][16] give the weights, coherence tables and td_error of ``ntuple_ref.td_step`` /
    ``ntuple_tc_ref.tc_step`` on prev_after = hist[0], whatever lam is (every env holds its one state here)."""
    prev, flag, target, w0 = T.one_step_inputs(N.SMALL, 12, n=257)
    ring = D.Ring(1, 257)
    ring.hist[0], ring.len[:] = prev, 1
    ring.err[:] = 123.0
    want = w0.copy()
    want_e, want_a = T.zero_coherence(want)
    if learner == "tc":
        want_err = T.tc_step(prev, flag, target, want, want_e, want_a, N.SMALL, 12, alpha)
    else:
        want_err = N.td_step(prev, flag, target, want, N.SMALL, 12, alpha)
    w = w0.copy()
    ce, ca = T.zero_coherence(w)
    err = host_step(host, ring, flag, target, 0, lam, w, N.SMALL, 12, alpha, (), learner, ce, ca)
    assert np.array_equal(w, want) and np.array_equal(_bits(err), _bits(want_err)) and (w != w0).any()
    assert np.array_equal(ce, want_e) and np.array_equal(ca, want_a)


def test_ring_argument_check(host):
    ok = {(h, p) for h in range(-1, 11) for p in range(-1, 11) if host.hst_nt_dl_ring_ok(h, p)}
    assert ok == {(h, p) for h in range(1, 9) for p in range(h)}


def test_host_program_runs_clean_under_sanitizers(tmp_path):
    """The per-lane code as a stand-alone program under ASan + UBSan on a ring of exactly [8][B][16] / [8][B] / [B] and tables of
    exactly [S][m][16^L]: a slot or an offset that left them, or a signed overflow, would abort it."""
    exe = str(tmp_path / "ntuple_delayed_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-DNTUPLE_DELAYED_HOST_MAIN", "-I", CSRC, "-o", exe, HOST_SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ntuple_delayed_host ok" in out.stdout, out.stderr[-2000:]


# ---------------------------------------------------------------------------------------------- properties of the restatement
def test_lambda_sums_are_the_truncated_horner_sums():
    xs = D.lambda_sums([F32(1), F32(2), F32(4), F32(8)], 0.5)
    assert [float(x) for x in xs] == [1.0, 2.5, 5.25, 10.625]  # e_j + lam x_{j-1}, from the newest back
    assert [float(x) for x in D.lambda_sums([F32(3), F32(5), F32(7)], 0.0)] == [3.0, 5.0, 7.0]
    assert [float(x) for x in D.lambda_sums([F32(3), F32(5), F32(7)], 1.0)] == [3.0, 8.0, 15.0]


def test_lambda_zero_is_td0_applied_late():
    """lam = 0, h = 3: the due state's delta comes from its OWN stored error alone, whatever the newer errors are."""
    case = D.ring_case(N.SMALL, 12, 3, 120)
    a, b = case["ring"].copy(), case["ring"].copy()
    head = 1
    flag = np.where(case["flag"] == 2, 1, case["flag"]).astype(np.uint8)  # steady state only: the state h - 1 steps back is due
    b.err[(head - 1) % 3] += 1000.0  # a newer error that lam = 0 must not see (the newest one, in head, is recomputed)
    wa, wb = case["w0"].copy(), case["w0"].copy()
    D.step(a, flag, case["target"], head, 0.0, wa, N.SMALL, 12, 0.1)
    D.step(b, flag, case["target"], head, 0.0, wb, N.SMALL, 12, 0.1)
    assert np.array_equal(wa, wb) and (wa != case["w0"]).any()
    wc = case["w0"].copy()
    D.step(b, flag, case["target"], head, 0.5, wc, N.SMALL, 12, 0.1)
    assert not np.array_equal(wa, wc)


def test_the_whole_loop_on_the_oracle_env_replays_and_flushes():
    """``engine_training`` (the trainer's whole loop on the C oracle's env and the engine's key chain) with lam = 0.5, h = 4 from
    ``crowding_weights``: episodes end inside 48 lock-steps, rings shorter than h are flushed, and ``replay_training`` fed its record
    reproduces scores, targets, weights and coherence tables."""
    tuples = ((0, 1, 2), (4, 5, 6))
    for learner, alpha in LEARNERS:
        w = N.crowding_weights(tuples).copy()
        ce, ca = T.zero_coherence(w)
        ref = D.engine_training(w, tuples, 64, 48, alpha=alpha, seed=0, learner=learner, lam=0.5, coh_e=ce, coh_a=ca)
        lr = ref["learner"]
        assert lr.h == 4 and ref["episodes"] >= 1 and lr.stats["episode_ends"] == ref["episodes"] and lr.stats["due"] > 64
        w2 = N.crowding_weights(tuples).copy()
        e2, a2 = T.zero_coherence(w2)
        q, v, lr2 = D.replay_training(w2, tuples, ref["boards"], ref["meta"], alpha, learner=learner, lam=0.5, coh_e=e2, coh_a=a2)
        assert np.array_equal(_bits(q), _bits(ref["scores"])) and np.array_equal(_bits(v), _bits(ref["targets"]))
        assert np.array_equal(w, w2) and np.array_equal(ce, e2) and np.array_equal(ca, a2) and lr2.stats == lr.stats


def test_the_restatement_learns_with_delayed_tc():
    """The small network of the TC section, 64 envs, 300 lock-steps of TC(0.5) at alpha 1.0 on numpy's RNG, then 100 greedy games on
    seed 42 against the all-zero network: the condition ``test_gpu_ntuple_delayed.test_it_learns`` asserts on the device.  This
    network is too small for a margin (478.7 against 226.6 here, a ratio of 2.11; 2.44 and 2.14 on training seeds 1 and 2); the
    margin of the device test's own size, 7.9, is recorded there."""
    tuples = ((0, 1, 2), (4, 5, 6))
    w = N.zero_weights(tuples)
    ce, ca = T.zero_coherence(w)
    episodes, lr = D.simulate_training(w, tuples, 64, 300, alpha=1.0, seed=0, learner="tc", lam=0.5, coh_e=ce, coh_a=ca)
    assert lr.h == 4 and episodes > 0 and w.any() and np.abs(w).max() < 2 ** 30 and lr.stats["due"] > 0
    zero = N.simulate_evaluation(N.zero_weights(tuples), tuples, 100)
    trained = N.simulate_evaluation(w, tuples, 100)
    print(f"mean max tile over 100 episodes: zero network {zero:.1f}, after 300 lock-steps of TC(0.5) {trained:.1f}")
    assert trained >= 2 * zero
