"""The eight-view ensemble without a GPU: the entry points (g2048_sym_views / g2048_sym_fold) declared, bound, exported, their
argument checks run before any device work; the mode word accepted for play and refused for training; the group facts the fold's
order-free sum rests on; the restated ensemble bit-identical under all eight views where the g-ordered sum is not; the per-lane
code of the kernels, compiled for the host, equal to the restatement.  CPU only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import symmetry_ensemble_ref as E  # noqa: E402
import symmetry_ref as R  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("g2048_sym_views", "g2048_sym_fold")
OPTIM = dict(opt_name="adamw", max_lr=4e-4, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, warmup_steps_ratio=0.025,
             scheduler_names=["constant", "constant"], blacklist_weight_modules=["norm", "embedding"])


def test_symbols_are_declared_bound_and_exported():
    from src.g2048 import native as nv

    header = open(os.path.join(ROOT, "include", "g2048.h")).read()
    lib = C.CDLL(nv.LIB_PATH)
    for name in NAMES:
        assert f"int {name}(" in header
        assert name in nv.SIGNATURES
        assert hasattr(lib, name)
    assert len(nv.SIGNATURES["g2048_sym_views"]) == 4 and len(nv.SIGNATURES["g2048_sym_fold"]) == 6
    assert "#define G2048_ABI_VERSION 4" in header
    assert nv.load().g2048_abi_version() == 4  # additive: the version stays
    assert callable(nv.sym_views) and callable(nv.sym_fold)


def test_entry_points_reject_bad_arguments_without_touching_a_device():
    from src.g2048 import native as nv

    lib = nv.load()
    a = 1 << 20  # a fake, 16-byte aligned "device address": must be rejected before any use
    views, fold = lib.g2048_sym_views, lib.g2048_sym_fold
    big = (1 << 27) + 1
    assert views(None, 8, a, None) == -1            # no boards
    assert views(a, 8, None, None) == -1            # no views
    assert views(a, 0, a, None) == -1               # B = 0
    assert views(a, -1, a, None) == -1
    assert views(a, big, a, None) == -1             # B past 2^27
    assert views(a + 8, 8, a, None) == -1           # boards not 16-byte aligned
    assert views(a, 8, a + 4, None) == -1           # views not 16-byte aligned
    assert fold(a, None, 8, None, None, None) == -1    # logits without out_logits
    assert fold(None, None, 8, a, None, None) == -1    # out_logits without logits
    assert fold(None, a, 8, None, None, None) == -1    # values without out_values
    assert fold(None, None, 8, None, a, None) == -1    # out_values without values
    assert fold(a, a, 8, a, None, None) == -1          # a full pair next to half a pair
    assert fold(a, None, 8, a, a, None) == -1
    assert fold(None, None, 8, None, None, None) == -1  # both pairs null
    for bad in (0, -1, big):
        assert fold(a, a, bad, a, a, None) == -1
        assert fold(None, a, bad, None, a, None) == -1
        assert fold(a, None, bad, a, None, None) == -1
    assert fold(a + 8, a, 8, a, a, None) == -1         # logits not 16-byte aligned
    assert fold(a, a, 8, a + 4, a, None) == -1         # out_logits not 16-byte aligned
    assert fold(a + 4, None, 8, a, None, None) == -1
    assert fold(None, a + 2, 8, None, a, None) == -1   # a float pointer off its 4 bytes
    assert fold(None, a, 8, None, a + 1, None) == -1


def test_wrappers_refuse_host_tensors():
    import torch

    from src.g2048 import native as nv

    b = torch.zeros((4, 16), dtype=torch.uint8)
    with pytest.raises(nv.NativeError):
        nv.sym_views(b, torch.zeros((4, 8, 16), dtype=torch.uint8))
    lg, vl = torch.zeros((32, 4)), torch.zeros(32)
    with pytest.raises(nv.NativeError):
        nv.sym_fold(lg, vl, torch.zeros((4, 4)), torch.zeros(4))
    with pytest.raises(nv.NativeError):
        nv.sym_fold(None, vl, None, torch.zeros(4))
    with pytest.raises(nv.NativeError):
        nv.sym_fold(lg, None, torch.zeros((4, 4)), None)
    with pytest.raises(nv.NativeError):
        nv.sym_fold(lg, vl, None, None)  # nothing asked for


def test_the_mode_is_for_play_and_refused_for_training(monkeypatch):
    from src.ppo import ExpectimaxActionFunction, LookaheadActionFunction, PPOAgent, PPOTrainer, RolloutBuffer, TorchActionFunction
    from src.ppo import resolve_symmetry
    from src.ppo.torch_action_wrapper import SYMMETRY_MODES

    assert SYMMETRY_MODES == ("none", "canonical", "ensemble")
    assert resolve_symmetry("ensemble", {}) == "ensemble"
    assert resolve_symmetry(None, {"G2048_SYMMETRY": "ensemble"}) == "ensemble"
    assert resolve_symmetry(None, {"G2048_SYMMETRY": " Ensemble "}) == "ensemble"
    assert resolve_symmetry("none", {"G2048_SYMMETRY": "ensemble"}) == "none"  # the explicit argument wins
    for word in ("canonical+ensemble", "canonical,ensemble", "8", "all", ""):  # one word, one mode: no combination can be spelled
        with pytest.raises(ValueError):
            resolve_symmetry(word, {})
    agent = PPOAgent(hidden_dim=32, d_model=32, nhead=2, num_layers=1, dim_feedforward=64)
    monkeypatch.delenv("G2048_SYMMETRY", raising=False)
    for cls in (TorchActionFunction, LookaheadActionFunction, ExpectimaxActionFunction):
        assert cls(agent, symmetry="ensemble").symmetry == "ensemble"
    la = LookaheadActionFunction(agent, max_children=64, symmetry="ensemble")
    assert la.max_children == 64 and la._chunk == 8          # max_children counts forward rows: eight per board
    assert LookaheadActionFunction(agent, max_children=5, symmetry="ensemble")._chunk == 1
    assert LookaheadActionFunction(agent, max_children=64, symmetry="none")._chunk == 64
    assert ExpectimaxActionFunction(agent, max_children=128, symmetry="ensemble")._chunk == 16
    with pytest.raises(ValueError, match="ensemble") as e:
        PPOTrainer(agent, None, RolloutBuffer(31, 16, 4), dict(OPTIM), max_steps=10, symmetry="ensemble")  # (before the runner is used)
    assert "play" in str(e.value) and "log_prob" in str(e.value)  # says why
    monkeypatch.setenv("G2048_SYMMETRY", "ensemble")  # what an unmodified training CLI would see
    assert TorchActionFunction(agent).symmetry == "ensemble"
    with pytest.raises(ValueError, match="ensemble"):
        PPOTrainer(agent, None, RolloutBuffer(31, 16, 4), dict(OPTIM), max_steps=10)


def test_eval_ensemble_flag_is_refused_with_the_canonical_frame():
    script = os.path.join(ROOT, "2048-ppo-agent_amd", "run", "train_to_2048.py")
    env = {k: v for k, v in os.environ.items() if k != "G2048_SYMMETRY"}
    for extra, extra_env in ((["--symmetry", "canonical"], {}), ([], {"G2048_SYMMETRY": "canonical"})):
        p = subprocess.run([sys.executable, script, "--eval-ensemble", *extra], env={**env, **extra_env}, capture_output=True, text=True)
        assert p.returncode == 2 and "--eval-ensemble" in p.stderr and "canonical" in p.stderr, p.stderr[-2000:]
    p = subprocess.run([sys.executable, script, "--symmetry", "ensemble"], env=env, capture_output=True, text=True)
    assert p.returncode == 2 and "invalid choice" in p.stderr  # training under the ensemble cannot be asked for


# ---------------------------------------------------------------------------------------------- the group facts and the order-free sum
def test_views_and_action_maps_compose_by_the_table():
    boards = np.concatenate([R.hand_made_boards(), R.random_boards(200, seed=4)])
    acts = np.arange(4)
    for h in range(8):
        assert sorted(E.TAB[h].tolist()) == list(range(8))  # view_h permutes the eight views of a board
        vh = R.view(boards, h)
        for g in range(8):
            c = int(E.TAB[h][g])
            assert np.array_equal(R.view(vh, g), R.view(boards, c)), (h, g)
            assert np.array_equal(R.sigma(g, R.sigma(h, acts)), R.sigma(c, acts)), (h, g)
    v = E.views(boards)
    assert v.shape == (len(boards), 8, 16) and v.dtype == np.uint8
    for g in range(8):
        assert np.array_equal(v[:, g], R.view(boards, g))  # the [B][8][16] row order
    assert np.array_equal(v.reshape(-1, 16)[8 * 5 + 3], R.view(boards[5:6], 3)[0])


def _stand_in_network(rows, seed=0):
    """A network whose output for a row depends on that row alone: five outputs (4 logits, 1 value), each 16 sequential f32 table
    adds over the cells.  rows u8 [n,16] -> (logit bits u32 [n,4], value bits u32 [n])."""
    table = np.random.default_rng(seed).standard_normal((5, 16, 32)).astype(np.float32)
    out = np.empty((len(rows), 5), np.float32)
    for j in range(5):
        s = table[j, 0, rows[:, 0]]
        for c in range(1, 16):
            s = (s + table[j, c, rows[:, c]]).astype(np.float32)
        out[:, j] = s
    return np.ascontiguousarray(out[:, :4]).view(np.uint32), np.ascontiguousarray(out[:, 4]).view(np.uint32)


def test_restated_ensemble_is_exactly_equivariant_and_the_g_ordered_sum_is_not():
    tb = R.test_boards()  # the eight views of its first n boards, view by view; self-symmetric boards included
    n = len(tb) // 8
    assert not R.stabiliser_is_trivial(tb[:n]).all()
    results = {}
    for name, mean8 in (("sorted", E.sorted_mean8), ("ordered", E.ordered_mean8)):
        per_view = []
        for h in range(8):
            lb, vb = _stand_in_network(E.views(tb[h * n:(h + 1) * n]).reshape(-1, 16))
            per_view.append(E.fold(lb, vb, mean8=mean8))
        results[name] = per_view
    base_l, base_v = results["sorted"][0]
    assert not E.is_nan(base_l).any() and len(np.unique(base_v)) > n // 2
    for h in range(8):
        l, v = results["sorted"][h]
        assert np.array_equal(l[:, R.sigma(h, np.arange(4))], base_l), h  # L(view_h(s))[sigma_h(a)] == L(s)[a], bit for bit
        assert np.array_equal(v, base_v), h
    # taken in ascending g instead, the same eight addends round differently: the sort cannot be dropped quietly
    ol, ov = results["ordered"][0]
    worst = 0.0
    for h in range(1, 8):
        l, v = results["ordered"][h]
        differs = (v != ov) | (l[:, R.sigma(h, np.arange(4))] != ol).any(axis=1)
        worst = max(worst, differs.mean())
    l5, v5 = results["ordered"][5]
    assert (v5 != ov).mean() > 0.10, (v5 != ov).mean()
    assert worst > 0.10


def test_sorted_mean8_restatement_is_order_free_and_handles_the_specials():
    x = E.test_patterns(3000, seed=1)
    want = E.sorted_mean8(x)
    rng = np.random.default_rng(2)
    for _ in range(4):
        perm = np.argsort(rng.random(x.shape), axis=1)
        E.assert_same_bits(E.sorted_mean8(np.take_along_axis(x, perm, axis=1)), want)
    keys = E.sort_key(E.SPECIALS)
    assert np.array_equal(E.sort_unkey(keys), E.SPECIALS)
    order = E.SPECIALS[np.argsort(keys)]
    assert order[0] == 0xFFFFFFFF and order[-1] == 0x7FC00001  # -NaN first, +NaN last
    i = {int(b): k for k, b in enumerate(order)}
    assert i[0xFF800000] < i[0xFF7FFFFF] < i[0x80000001] < i[0x80000000] < i[0x00000000] < i[0x00000001] < i[0x3F800000] < i[0x7F800000]
    one, inf, ninf, nan, nz = 0x3F800000, 0x7F800000, 0xFF800000, 0x7FC00001, 0x80000000
    row = lambda *v: np.array([list(v) + [one] * (8 - len(v))], np.uint32)
    assert E.sorted_mean8(row())[0] == one                     # eight ones: 8 * 0.125
    assert E.sorted_mean8(row(inf))[0] == inf and E.sorted_mean8(row(ninf, ninf))[0] == ninf
    assert E.is_nan(E.sorted_mean8(row(inf, ninf)))[0] and E.is_nan(E.sorted_mean8(row(nan)))[0]
    assert E.sorted_mean8(np.array([[nz] * 8], np.uint32))[0] == nz and E.sorted_mean8(np.array([[nz] * 7 + [0]], np.uint32))[0] == 0
    assert E.sorted_mean8(np.array([[8] * 8], np.uint32))[0] == 8  # denormals: 64 * 2^-149 / 8


# ---------------------------------------------------------------------------------------------- the kernels' per-lane code on the host
@pytest.fixture(scope="module")
def host():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libsymmetry_ensemble_host.so")
    subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "2048-ppo-agent_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "host_swar", "symmetry_ensemble_host.cpp")])
    return C.CDLL(so)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_per_lane_sym_view_equals_the_restatement(host):
    boards = R.test_boards()
    got = np.empty((len(boards), 8, 16), np.uint8)
    host.hst_sym_views(_p(boards), C.c_int64(len(boards)), _p(got))
    assert np.array_equal(got, E.views(boards))


def test_per_lane_sorted_mean8_equals_the_restatement(host):
    x = np.concatenate([E.test_patterns(30000, seed=3),
                        np.array([[s] * 8 for s in E.SPECIALS], np.uint32),                       # eight of each special
                        np.array([[s] + [0x3F800000] * 7 for s in E.SPECIALS], np.uint32),          # one among ones
                        np.array([[0x7F800000, 0xFF800000] + [0x3F800000] * 6], np.uint32)])      # both infinities
    out = np.empty(len(x), np.uint32)
    host.hst_sym_sorted_mean8(_p(x), C.c_int64(len(x)), _p(out))
    want = E.sorted_mean8(x)
    assert E.is_nan(want).any() and (~E.is_nan(want)).sum() > 20000
    E.assert_same_bits(out, want)
    # all 256 zero / one inputs: the 19 compare-exchanges sort (the 0-1 principle), seen through the sum
    zo = np.array([[0x3F800000 if (m >> i) & 1 else 0x4B800000 for i in range(8)] for m in range(256)], np.uint32)  # 1.0 / 2^24
    out = np.empty(256, np.uint32)
    host.hst_sym_sorted_mean8(_p(zo), C.c_int64(256), _p(out))
    assert np.array_equal(out, E.sorted_mean8(zo))


def test_per_lane_fold_equals_the_restatement(host):
    B = 500
    lb = E.test_patterns(4 * B, seed=4).reshape(8 * B, 4)
    vb = E.test_patterns(B, seed=5).reshape(8 * B)
    want_l, want_v = E.fold(lb, vb)
    ol, ov = np.zeros((B, 4), np.uint32), np.zeros(B, np.uint32)
    host.hst_sym_fold(_p(lb), _p(vb), C.c_int64(B), _p(ol), _p(ov))
    E.assert_same_bits(ol, want_l)
    E.assert_same_bits(ov, want_v)
    ol2, ov2 = np.zeros((B, 4), np.uint32), np.zeros(B, np.uint32)
    host.hst_sym_fold(_p(lb), None, C.c_int64(B), _p(ol2), None)
    host.hst_sym_fold(None, _p(vb), C.c_int64(B), None, _p(ov2))
    assert np.array_equal(ol2, ol) and np.array_equal(ov2, ov)
