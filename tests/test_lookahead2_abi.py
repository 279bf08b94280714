"""The two-ply entry points (g2048_lookahead_dedup / _backup): declared, bound, exported, their argument checks run before any
device work; ExpectimaxActionFunction and evaluate_agent(expectimax=) refuse what they do not implement; the numpy restatement
the GPU tests compare against (tests/lookahead2_ref.py) is sane on its own.  CPU only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import lookahead2_ref as R2  # noqa: E402
import lookahead_ref as R  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("g2048_lookahead_dedup", "g2048_lookahead_backup")
GAMMA = 0.99


def test_symbols_are_declared_bound_and_exported():
    from src.g2048 import native as nv

    header = open(os.path.join(ROOT, "include", "g2048.h")).read()
    lib = C.CDLL(nv.LIB_PATH)
    for name in NAMES:
        assert f"int {name}(" in header
        assert name in nv.SIGNATURES
        assert hasattr(lib, name)
    assert "#define G2048_ABI_VERSION 4" in header
    assert nv.load().g2048_abi_version() == 4  # additive: the version stays
    for fn in ("lookahead_dedup", "lookahead_backup"):
        assert callable(getattr(nv, fn))


def test_entry_points_reject_bad_arguments_without_touching_a_device():
    from src.g2048 import native as nv

    lib = nv.load()
    a = 1 << 20  # a fake, 16-byte aligned "device address": must be rejected before any use
    dedup, backup = lib.g2048_lookahead_dedup, lib.g2048_lookahead_backup
    for k in range(5):  # after, nchild, group_start, rep, nuniq: each null in turn
        ptrs = [a] * 5
        ptrs[k] = None
        assert dedup(ptrs[0], ptrs[1], ptrs[2], 2, 64, ptrs[3], ptrs[4], None) == -1
    assert dedup(a, a, a, 0, 64, a, a, None) == -1                    # no group
    assert dedup(a, a, a, (1 << 24) + 1, 64, a, a, None) == -1
    assert dedup(a, a, a, 2, -4, a, a, None) == -1
    assert dedup(a, a, a, 2, 62, a, a, None) == -1                    # pairs come in fours
    assert dedup(a, a, a, 2, 2 * 480 + 4, a, a, None) == -1           # some group would be larger than 480 pairs
    assert dedup(a, a, a, 1 << 24, (1 << 26) + 4, a, a, None) == -1   # more pairs than 2^24 level-1 children have
    assert dedup(a + 8, a, a, 2, 64, a, a, None) == -1                # after not 16-byte aligned
    for k in range(1, 5):                                             # the i32 arrays not 4-byte aligned
        ptrs = [a] * 5
        ptrs[k] = a + 2
        assert dedup(ptrs[0], ptrs[1], ptrs[2], 2, 64, ptrs[3], ptrs[4], None) == -1
    assert dedup(a, a, a, 2, 0, a, a, None) == 0                      # no pair, nothing launched
    for k in range(5):  # reward, nchild, rep, e, v1
        ptrs = [a] * 5
        ptrs[k] = None
        assert backup(ptrs[0], ptrs[1], ptrs[2], ptrs[3], 8, ptrs[4], None) == -1
    assert backup(a, a, a, a, 0, a, None) == -1
    assert backup(a, a, a, a, (1 << 24) + 1, a, None) == -1
    for k in range(3):                                                # the 16-byte loads
        ptrs = [a] * 5
        ptrs[k] = a + 8
        assert backup(ptrs[0], ptrs[1], ptrs[2], ptrs[3], 8, ptrs[4], None) == -1
    assert backup(a, a, a, a + 2, 8, a, None) == -1
    assert backup(a, a, a, a, 8, a + 2, None) == -1


def test_wrappers_refuse_host_tensors():
    import torch

    from src.g2048 import native as nv

    i4 = lambda: torch.zeros((4, 4), dtype=torch.int32)
    with pytest.raises(nv.NativeError):
        nv.lookahead_dedup(torch.zeros((4, 4, 16), dtype=torch.uint8), i4(), torch.zeros(2, dtype=torch.int32), i4(), i4())
    with pytest.raises(nv.NativeError):
        nv.lookahead_backup(torch.zeros((4, 4)), i4(), i4(), torch.zeros((4, 4)), torch.zeros(4))


def test_plies_depth_and_exclusive_keywords_without_a_device():
    import torch

    from src.ppo import ExpectimaxActionFunction, LookaheadActionFunction, PPOAgent
    from src.runs import evaluate_agent

    assert issubclass(ExpectimaxActionFunction, LookaheadActionFunction)
    agent = PPOAgent(hidden_dim=32, d_model=32, nhead=2, num_layers=1, dim_feedforward=64)
    fn = ExpectimaxActionFunction(agent)
    assert fn.plies == 2 and fn.dedup and fn.depth == 1 and fn.gamma == 0.99 and fn.max_children == 1 << 18
    assert fn.use_mask and not fn.sample_actions and fn.last_children == 0 and fn.last_children_full == 0
    assert ExpectimaxActionFunction(agent, plies=1, max_children=7).plies == 1  # the parent's only demand: a positive row count
    for plies in (0, 3):
        with pytest.raises(ValueError):
            ExpectimaxActionFunction(agent, plies=plies)
    with pytest.raises(ValueError):
        ExpectimaxActionFunction(agent, max_children=119)  # a board can have 120 level-1 children
    with pytest.raises(ValueError):
        LookaheadActionFunction(agent, depth=2)
    cpu = torch.device("cpu")
    with pytest.raises(ValueError):
        evaluate_agent(agent, cpu, 4, lookahead=2)
    with pytest.raises(ValueError):
        evaluate_agent(agent, cpu, 4, lookahead=1, expectimax=2)
    for plies in (1, 3, -2):
        with pytest.raises(ValueError):
            evaluate_agent(agent, cpu, 4, expectimax=plies)


@pytest.fixture(scope="module")
def boards():
    return R2.test_boards()


def test_reference_dedup_changes_no_bit_and_removes_rows(boards):
    T = R2.table(5)
    vf = lambda rows: R2.table_values(T, rows)
    for dtype in (np.float64, np.float32):
        with_, without = (R2.pipeline(boards, vf, GAMMA, dtype, d) for d in (True, False))
        view = np.uint64 if dtype is np.float64 else np.uint32
        assert np.array_equal(with_["q2"].view(view), without["q2"].view(view))
        assert np.array_equal(with_["v1"].view(view), without["v1"].view(view))
    p = with_
    assert 0 < p["nuniq"].sum() < p["nchild2"].sum()
    ratio = p["nuniq"].sum() / p["nchild2"].sum()
    print(f"{len(boards)} boards, N1 = {len(p['children1'])}, rows {p['nuniq'].sum()} of {p['nchild2'].sum()} = {ratio:.3f}")
    assert 0.3 < ratio < 0.8  # 0.525 on 200 mid-game boards of a DRUL rollout
    # every rep points to a pair of the same group with children and equal afterstate bytes, and is the first such
    rep, n2 = p["rep"].reshape(-1), p["nchild2"].reshape(-1)
    keys, gs = p["after2"].reshape(-1, 16), p["group_start"]
    group = np.searchsorted(gs, np.arange(len(rep)), side="right") - 1
    assert np.array_equal(group[rep], group) and (rep <= np.arange(len(rep))).all()
    assert np.array_equal(keys[rep][n2 > 0], keys[n2 > 0]) and (n2[rep][n2 > 0] > 0).all()
    assert np.array_equal(rep[n2 == 0], np.arange(len(rep))[n2 == 0])
    assert (rep[rep] == rep).all()
    sizes = np.diff(gs)
    assert sizes.max() == R2.MAX_GROUP and sizes.min() == 0  # the largest group and an empty one are among the cases
    for g in np.flatnonzero(sizes > 0)[:40]:  # first occurrence: no two representatives of a group share a key
        reps = np.unique(rep[gs[g]:gs[g + 1]][n2[gs[g]:gs[g + 1]] > 0])
        assert len({keys[r].tobytes() for r in reps}) == len(reps)


def test_reference_two_ply_against_a_direct_recursion(boards):
    """q2 of the array pipeline equals a plain recursive evaluation, board by board, in float64 up to summation order."""
    from oracle import g2048_oracle as npo

    T = R2.table(5)
    q2 = R2.q2_values(boards, lambda rows: R2.table_values(T, rows), GAMMA, np.float64)

    def spawn_children(after):
        for cell in np.flatnonzero(after == 0):
            for tile, pr in ((1, 0.9), (2, 0.1)):
                c = after.copy()
                c[cell] = tile
                yield c, pr / (after == 0).sum()

    def moves(b):
        for a in range(4):
            moved, score = npo.move(b[None], np.array([a], np.int32))
            if (moved[0] != b).any():
                yield a, moved[0], float(score[0])

    g = float(np.float32(GAMMA))
    assert len(R.hand_made_boards()) == 25
    # no board, full without a move, full with merges, one merge, one legal move, double merges with gaps, big tiles, late-game play
    for i in (9, 10, 12, 14, 21, 24, len(boards) - 7):
        want = np.zeros(4)
        for a, after, r in moves(boards[i]):
            ev = 0.0
            for c1, p1 in spawn_children(after):
                best = [r2 + g * sum(p2 * (R2.table_values(T, c2[None])[0] if npo.legal_mask(c2[None]).any() else 0.0)
                                     for c2, p2 in spawn_children(after2))
                        for _, after2, r2 in moves(c1)]
                ev += p1 * (max(best) if best else 0.0)
            want[a] = r + g * ev
        np.testing.assert_allclose(q2[i], want, rtol=1e-6, atol=1e-6)  # 0.9f + 0.1f is 1 + 2e-8, and the order of the sums differs
