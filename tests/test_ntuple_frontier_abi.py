"""N-tuple frontier search (g2048_ntuple_search): declared, bound, exported; every argument check runs before any device work; the
wrappers refuse host tensors and the classes, evaluate_ntuple and the scripts a bad depth without a device; the numpy composition
(tests/ntuple_frontier_ref.py) checks itself; the per-lane code with a serial emulation of the kernels, compiled for the host, equals
it bit for bit, also when the dedup table is too small to merge everything.  CPU only."""
import ctypes as C
import importlib.util
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import lookahead2_ref as R2  # noqa: E402
import lookahead_ref as R  # noqa: E402
import ntuple_frontier_ref as FR  # noqa: E402
import ntuple_ref as N  # noqa: E402
import ntuple_search_ref as X  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = {"g2048_ntuple_search_workspace_bytes": 2, "g2048_ntuple_search": 16, "g2048_ntuple_staged_search": 18}
F32 = np.float32


def test_symbols_are_declared_bound_and_exported():
    from src.g2048 import native as nv

    header = open(os.path.join(ROOT, "include", "g2048.h")).read()
    lib = C.CDLL(nv.LIB_PATH)
    assert "int64_t g2048_ntuple_search_workspace_bytes(" in header
    assert "int g2048_ntuple_search(" in header and "int g2048_ntuple_staged_search(" in header
    for name, nargs in NAMES.items():
        assert name in nv.SIGNATURES and len(nv.SIGNATURES[name]) == nargs
        assert hasattr(lib, name)
    for name in ("ntuple_search_workspace_bytes", "ntuple_search"):
        assert callable(getattr(nv, name))
    assert nv.PROTOTYPES["g2048_ntuple_search_workspace_bytes"][0] is C.c_int64
    assert "#define G2048_ABI_VERSION 4" in header
    assert nv.load().g2048_abi_version() == 4  # additive: the version stays


def test_workspace_bytes_has_three_kinds_of_answer_and_is_monotone():
    from src.g2048 import native as nv

    f = nv.load().g2048_ntuple_search_workspace_bytes
    for depth, limit in ((1, 1 << 20), (2, 1 << 16), (3, 1 << 12)):
        sizes = [f(B, depth) for B in (1, 2, 3, 100, 256, limit)]
        assert all(s > 0 and s % 16 == 0 for s in sizes)
        assert all(a < b for a, b in zip(sizes, sizes[1:])), depth  # monotone in B
        assert f(limit + 1, depth) == -1 and f(0, depth) == -1 and f(-1, depth) == -1
    assert f(8, 1) < f(8, 2) < f(8, 3)
    # the lists alone: 16 bytes per afterstate of the worst case, and no more than 1.5 MB per root at depth 3
    assert 16 * 256 * (4 + 480 + 57600) < f(256, 3) < 256 * 1.5 * (1 << 20)
    for depth in (0, 4, -1):
        assert f(8, depth) == -1
    assert nv.ntuple_search_workspace_bytes(7, 2) == f(7, 2)
    with pytest.raises(nv.NativeError):
        nv.ntuple_search_workspace_bytes(7, 4)


def test_entry_points_reject_bad_arguments_without_touching_a_device():
    from src.g2048 import native as nv

    lib = nv.load()
    a = 1 << 20  # a fake, 16-byte aligned "device address": rejected before any use
    good = np.array([[0, 1, 2], [4, 5, 6]], np.uint8)
    hi = np.array([[0, 1, 2], [4, 16, 6]], np.uint8)
    dup = np.array([[0, 1, 2], [4, 6, 6]], np.uint8)
    tiles = np.array([3, 5], np.uint8)
    flat = np.array([5, 5], np.uint8)
    big = 1 << 40

    def call(boards=a, B=8, w=a, cells=good.ctypes.data, m=2, L=3, F=12, depth=2, gamma=1.0, dedup=1, ws=a, nbytes=big, q=a, v=a, cnt=a):
        return lib.g2048_ntuple_search(boards, B, w, cells, m, L, F, depth, gamma, dedup, ws, nbytes, q, v, cnt, None)

    def staged(st=tiles.ctypes.data, S=3, boards=a, B=8, depth=2, gamma=1.0, nbytes=big):
        return lib.g2048_ntuple_staged_search(boards, B, a, good.ctypes.data, 2, 3, st, S, 12, depth, gamma, 1, a, nbytes, a, a, None, None)

    need = lib.g2048_ntuple_search_workspace_bytes(8, 2)
    bad = [dict(boards=None), dict(w=None), dict(q=None), dict(v=None), dict(ws=None), dict(cells=None),
           dict(B=0), dict(B=-3), dict(B=(1 << 16) + 1), dict(B=(1 << 20) + 1, depth=1), dict(B=(1 << 12) + 1, depth=3),
           dict(m=0), dict(m=9), dict(L=0), dict(L=7), dict(cells=hi.ctypes.data), dict(cells=dup.ctypes.data),
           dict(F=-1), dict(F=21), dict(depth=0), dict(depth=4), dict(depth=-1),
           dict(gamma=-0.5), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(gamma=float("-inf")),
           dict(nbytes=need - 1), dict(nbytes=0), dict(nbytes=-1), dict(nbytes=need, depth=3),
           dict(boards=a + 8), dict(ws=a + 8), dict(ws=a + 4), dict(w=a + 2), dict(q=a + 2), dict(v=a + 1), dict(cnt=a + 2)]
    for kw in bad:
        assert call(**kw) == -1, kw
    for kw in (dict(st=None), dict(S=0), dict(S=9), dict(st=flat.ctypes.data), dict(boards=None), dict(B=0), dict(depth=4),
               dict(gamma=-1.0), dict(nbytes=need - 1)):
        assert staged(**kw) == -1, kw


def test_wrappers_refuse_host_tensors_and_wrong_shapes():
    import torch

    from src.g2048 import native as nv

    B, cells = 4, np.array(N.SMALL, np.uint8)
    boards = torch.zeros((B, 16), dtype=torch.uint8)
    w = torch.zeros((3, 256), dtype=torch.int32)
    q, v = torch.zeros((B, 4)), torch.zeros(B)
    ws = torch.zeros(nv.ntuple_search_workspace_bytes(B, 3), dtype=torch.uint8)
    for depth in (1, 2, 3):
        for workspace in (ws, None):
            with pytest.raises(nv.NativeError):
                nv.ntuple_search(boards, w, cells, 12, depth, 1.0, True, workspace, q, v)
    with pytest.raises(nv.NativeError):
        nv.ntuple_search(boards, w, cells, 12, 4, 1.0, True, ws, q, v)  # no such depth
    with pytest.raises(nv.NativeError):
        nv.ntuple_search(boards, w, np.zeros(3, np.uint8), 12, 1, 1.0, True, ws, q, v)  # tuple_cells is [m, L]
    with pytest.raises(nv.NativeError):
        nv.ntuple_search(boards, w, cells, 12, 1, 1.0, True, ws, q, v, stage_tiles=np.zeros((2, 2), np.uint8))  # stage_tiles is flat


def _script(name):
    spec = importlib.util.spec_from_file_location("_frontier_" + name, os.path.join(ROOT, "2048-ppo-agent_amd", "run", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_classes_evaluation_and_scripts_refuse_a_bad_depth_without_a_device(capsys):
    import torch

    from src.ppo import NTupleNetwork, NTupleSearchActionFunction
    from src.ppo.q_player import QPlayer
    from src.runs import evaluate_ntuple

    net = NTupleNetwork(N.SMALL, device="cpu")
    fn = NTupleSearchActionFunction(net)
    assert isinstance(fn, QPlayer) and fn.depth == 1 and fn.gamma == 1.0 and fn.dedup is True
    fn = NTupleSearchActionFunction(net, depth=3, gamma=0.5, dedup=False)
    assert fn.depth == 3 and fn.gamma == 0.5 and fn.dedup is False
    assert fn.use_mask is True and fn.sample_actions is False and fn.compact is True and fn.policy_fn.needs_masks is False
    boards = torch.zeros((2, 16), dtype=torch.uint8)
    for kw in (dict(depth=0), dict(depth=4), dict(depth=-1), dict(depth=1.5), dict(depth=2.0), dict(depth="1"), dict(depth=None),
               dict(depth=True), dict(depth=1, gamma=-0.1), dict(depth=2, gamma=float("nan")), dict(depth=3, gamma=float("inf")),
               dict(depth=1, gamma="x")):
        with pytest.raises(ValueError):
            NTupleSearchActionFunction(net, **kw)
        with pytest.raises(ValueError):
            net.search(boards, kw["depth"], kw.get("gamma", 1.0))
        if kw["depth"] != 0:  # 0 is evaluate_ntuple's "off"
            with pytest.raises(ValueError):
                evaluate_ntuple(net, "cpu", num_episodes=1, **kw)
    for plies in (1, 2):
        with pytest.raises(ValueError):
            evaluate_ntuple(net, "cpu", num_episodes=1, depth=2, plies=plies)
    with pytest.raises(TypeError):
        NTupleSearchActionFunction(net, None, None, 1)  # depth, gamma and dedup are keyword-only

    train, distill = _script("train_ntuple"), _script("distill_ntuple")
    assert train.parse_args(["--eval-depth", "1", "3"]).eval_depth == [1, 3] and train.parse_args([]).eval_depth == []
    assert distill.parse_args(["--teacher-depth", "3"]).teacher_depth == 3 and distill.parse_args([]).teacher_depth == 0
    assert distill.parse_args(["--teacher-depth", "2", "--teacher-plies", "0"]).teacher_depth == 2
    for mod, argv in ((train, ["--eval-depth", "0"]), (train, ["--eval-depth", "4"]), (train, ["--eval-depth", "x"]),
                      (distill, ["--teacher-depth", "4"]), (distill, ["--teacher-depth", "-1"]),
                      (distill, ["--teacher-depth", "2", "--teacher-plies", "1"])):
        with pytest.raises(SystemExit):
            mod.parse_args(argv)
    capsys.readouterr()


# ---------------------------------------------------------------------------------------------- the reference checks itself
def test_reference_depth_two_equals_the_two_ply_restatement():
    c = FR.case("small", 2)
    FR_boards = c["boards"]
    X.check_inputs(FR_boards, c["legal"], c["nchild"])
    want, legal, _ = X.two_plies(FR_boards, c["tuples"], c["weights"])
    for g in X.GAMMAS:
        assert np.array_equal(c["q"][g].view(np.uint32), want[g][0].view(np.uint32))
        assert np.array_equal(c["v"][g].view(np.uint32), want[g][1].view(np.uint32))
    one, _, _ = X.one_ply(FR_boards, c["tuples"], c["weights"])
    assert np.array_equal(FR.case("small", 1)["q"][0.99].view(np.uint32), one[0.99][0].view(np.uint32))
    assert np.array_equal(legal, c["legal"])


def test_reference_depth_three_does_not_depend_on_dedup():
    """Two hand-made and two rollout boards: merging compounds down the levels and changes no bit."""
    tuples, w = X.network("small")
    hand, roll = R.hand_made_boards(), R2.test_boards()[FR.N_HAND_MADE:]
    boards = np.stack([hand[0], hand[21], roll[len(roll) // 2], roll[-1]])
    q1, v1, n1 = FR.search(boards, tuples, w, 3, 0.99, True)
    q0, v0, n0 = FR.search(boards, tuples, w, 3, 0.99, False)
    assert np.array_equal(q1.view(np.uint32), q0.view(np.uint32)) and np.array_equal(v1.view(np.uint32), v0.view(np.uint32))
    assert np.array_equal(n0, FR.plain_counts(boards, 3))
    assert n1[0] <= n0[0] and n1[1] < n0[1] and 4 * n1[2] < n0[2]
    assert (n0 <= len(boards) * np.array([4, 480, 57600])).all()


# ---------------------------------------------------------------------------------------------- the kernels' per-lane code on the host
HOST_SRC = os.path.join(ROOT, "tests", "host_swar", "ntuple_frontier_host.cpp")
CSRC = os.path.join(ROOT, "2048-ppo-agent_amd", "csrc")
SMALL_TABLE = 16


def _build(name, *flags):
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, name)
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", *flags, "-I", CSRC, "-o", so, HOST_SRC])
    lib = C.CDLL(so)
    lib.hst_ntf_workspace_bytes.restype = C.c_int64
    return lib


@pytest.fixture(scope="module")
def host():
    return _build("libntuple_frontier_host.so")


@pytest.fixture(scope="module")
def host_small_table():
    return _build("libntuple_frontier_host_t16.so", f"-DNTF_TABLE_CAP={SMALL_TABLE}")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def host_search(host, boards, w, tuples, depth, gamma, dedup, fill=0xFF):
    from src.g2048 import native as nv

    cells = N.cells_array(tuples)
    B = len(boards)
    need = host.hst_ntf_workspace_bytes(C.c_int64(B), C.c_int(depth))
    assert need == nv.load().g2048_ntuple_search_workspace_bytes(B, depth)  # one layout
    raw = np.full(need + 16 + 64, fill, np.uint8)
    at = (-raw.ctypes.data) % 16
    ws = raw[at:at + need + 64]  # 16-byte aligned, with a guard tail
    ws[need:] = 0x5A
    q, v, counts = np.full((B, 4), -7, F32), np.full(B, -7, F32), np.full(3, -7, np.int32)
    host.hst_ntf_search(_p(boards), C.c_int64(B), _p(w), _p(cells), C.c_int(cells.shape[0]), C.c_int(cells.shape[1]), None, C.c_int(1),
                        C.c_int(X.FRAC_BITS), C.c_int(depth), C.c_double(gamma), C.c_int(int(dedup)), _p(ws), _p(q), _p(v), _p(counts))
    assert (ws[need:] == 0x5A).all()
    return q, v, counts


def _boards(c, depth, dedup):
    """Without merging, level 3 of all the boards of a shape is half a million entries, a minute of the sequential host build: that
    one case runs on the boards whose unmerged third level has at most 2 500 entries (at most 8 of them, at least the 3 with the
    smallest), the board without a move among them.  The large levels without merging (the one-tile boards: 50 000 entries a root)
    are the GPU test's."""
    sel = np.arange(len(c["boards"]))
    if depth == 3 and not dedup:
        per_board = np.array([FR.plain_counts(c["boards"][i:i + 1], 3)[2] for i in sel])
        order = np.argsort(per_board, kind="stable")
        sel = np.sort(order[:min(8, max(3, int((per_board <= 2500).sum())))])
        assert not c["legal"][sel].any(axis=1).all() and c["legal"][sel].any()
    return sel


@pytest.mark.parametrize("dedup", [True, False])
@pytest.mark.parametrize("depth", FR.DEPTHS)
@pytest.mark.parametrize("shape", ["small", "wide", "eight"])
def test_host_build_equals_the_composed_reference(host, shape, depth, dedup):
    c = FR.case(shape, depth)
    X.check_inputs(c["boards"], c["legal"], c["nchild"])
    sel = _boards(c, depth, dedup)
    boards, legal = np.ascontiguousarray(c["boards"][sel]), c["legal"][sel]
    want_counts = c["counts"][dedup] if len(sel) == len(c["boards"]) else FR.plain_counts(boards, depth)
    seen = []
    for gamma in X.GAMMAS:
        q, v, counts = host_search(host, boards, c["weights"], c["tuples"], depth, gamma, dedup)
        assert np.array_equal(_bits(q), _bits(c["q"][gamma][sel])) and np.array_equal(_bits(v), _bits(c["v"][gamma][sel])), gamma
        assert (_bits(q)[~legal] == 0).all() and (_bits(v)[~legal.any(axis=1)] == 0).all()  # +0
        assert np.array_equal(counts, want_counts)
        seen.append(q)
    assert (seen[0] != seen[1]).any()  # gamma reaches the result
    # the workspace's initial contents do not matter
    q0, v0, counts0 = host_search(host, boards, c["weights"], c["tuples"], depth, X.GAMMAS[-1], dedup, fill=0)
    assert np.array_equal(_bits(q0), _bits(seen[-1])) and np.array_equal(counts0, want_counts)


def test_a_full_dedup_table_appends_unmerged_and_keeps_the_bits(host_small_table):
    """The host build again with a table of 16 entries, at depth 3: a table is only found full at the start of a round, levels 1
    and 2 are built in one round each and merge completely, so the third level is where entries are appended unmerged.  On the
    boards of the unmerged depth-3 case (the third level comes out nearly unmerged here)."""
    assert host_small_table.hst_ntf_table_cap() == SMALL_TABLE
    c = FR.case("small", 3)
    sel = _boards(c, 3, False)
    boards = np.ascontiguousarray(c["boards"][sel])
    merged, plain = FR.search(boards, c["tuples"], c["weights"], 3, 0.99, True)[2], FR.plain_counts(boards, 3)
    q, v, counts = host_search(host_small_table, boards, c["weights"], c["tuples"], 3, 0.99, True)
    assert np.array_equal(_bits(q), _bits(c["q"][0.99][sel])) and np.array_equal(_bits(v), _bits(c["v"][0.99][sel]))
    assert (merged <= counts).all() and (counts <= plain).all()
    assert np.array_equal(counts[:2], merged[:2]) and counts[2] > merged[2]  # the fallback ran


def test_host_program_runs_clean_under_sanitizers(tmp_path):
    """The per-lane code and the serial emulation as a stand-alone program under ASan + UBSan, the workspace on the heap at exactly
    its documented size: an access outside a table, a list, a link row or the workspace would abort it; a NaN in an output (an entry
    read that was never written) fails it."""
    assert shutil.which("g++") is not None
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-static-libasan", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = str(tmp_path / "ntuple_frontier_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-DNTUPLE_FRONTIER_HOST_MAIN", "-I", CSRC, "-o", exe, HOST_SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ntuple_frontier_host ok" in out.stdout, out.stderr[-2000:]
