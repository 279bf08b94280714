"""N-tuple budgeted search (g2048_ntuple_budget_search): declared, bound, exported; every argument check runs before any device work;
the method, the class, evaluate_ntuple_budget and the script flags refuse bad settings without a device; the numpy reference
(tests/ntuple_budget_ref.py) reproduces the recorded depth histograms; the per-lane code with a serial emulation of the kernels,
compiled for the host, equals it bit for bit in scores, values, depth_used and entries, also with a table so small that probing wraps
and with regions of one round.  CPU only."""
import ctypes as C
import importlib.util
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import ntuple_budget_ref as BR  # noqa: E402
import ntuple_frontier_ref as FR  # noqa: E402
import ntuple_ref as N  # noqa: E402
import ntuple_search_ref as X  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = {"g2048_ntuple_budget_search_workspace_bytes": 3, "g2048_ntuple_budget_search": 17, "g2048_ntuple_staged_budget_search": 19}
F32 = np.float32


def test_symbols_are_declared_bound_and_exported():
    from src.g2048 import native as nv

    header = open(os.path.join(ROOT, "include", "g2048.h")).read()
    lib = C.CDLL(nv.LIB_PATH)
    assert "n-tuple budgeted search" in header
    assert "int64_t g2048_ntuple_budget_search_workspace_bytes(" in header
    assert "int g2048_ntuple_budget_search(" in header and "int g2048_ntuple_staged_budget_search(" in header
    for name, nargs in NAMES.items():
        assert name in nv.SIGNATURES and len(nv.SIGNATURES[name]) == nargs
        assert hasattr(lib, name)
    for name in ("ntuple_budget_search_workspace_bytes", "ntuple_budget_search"):
        assert callable(getattr(nv, name))
    assert nv.PROTOTYPES["g2048_ntuple_budget_search_workspace_bytes"][0] is C.c_int64
    assert "#define G2048_ABI_VERSION 4" in header
    assert nv.load().g2048_abi_version() == 4  # additive: the version stays
    build = open(os.path.join(ROOT, "2048-ppo-agent_amd", "build.py")).read()
    assert '"g2048_ntuple_budget.hip"' in build


def _limit(max_depth, budget):
    """The per-call limit as include/g2048.h states it."""
    cap = max([4, min(480, budget + 512), budget + 512][:min(max_depth, 3)])
    return min(1 << 20, ((1 << 31) - 1) // (128 * cap))


def test_workspace_bytes_has_three_kinds_of_answer_and_is_monotone():
    from src.g2048 import native as nv

    f = nv.load().g2048_ntuple_budget_search_workspace_bytes
    for max_depth, budget in ((1, 4), (2, 8), (3, 600), (4, 8192), (5, 24576), (6, 24576), (6, 4)):
        limit = _limit(max_depth, budget)
        sizes = [f(B, max_depth, budget) for B in (1, 2, 3, 50, limit)]
        assert all(s > 0 and s % 16 == 0 for s in sizes)
        assert all(a < b for a, b in zip(sizes, sizes[1:])), (max_depth, budget)  # monotone in B
        assert sizes[-1] < 1 << 36
        assert f(limit + 1, max_depth, budget) == -1 and f(0, max_depth, budget) == -1 and f(-1, max_depth, budget) == -1
    assert _limit(6, 24576) == 668 and _limit(4, 8192) == 1927 and _limit(2, 8) == 34952 and _limit(1, 4) == 1 << 20
    by_depth = [f(8, d, 600) for d in range(1, 7)]
    assert all(a < b for a, b in zip(by_depth, by_depth[1:]))  # monotone in max_depth
    by_budget = [f(8, 4, k) for k in (4, 5, 8, 70, 600, 2100, 8192, 24576)]
    assert all(a < b for a, b in zip(by_budget, by_budget[1:]))  # monotone in the budget
    # the regions: a level with links is 532 bytes an entry (list, E, 128 links), the last level 20
    assert f(1, 4, 8192) >= 532 * (4 + 480 + 8704) + 20 * 8704 and f(1, 4, 8192) < 532 * (4 + 480 + 8704) + 20 * 8704 + 1024
    for max_depth in (0, 7, -1):
        assert f(8, max_depth, 600) == -1
    for budget in (3, 24577, -1, 0):
        assert f(8, 4, budget) == -1
    assert nv.ntuple_budget_search_workspace_bytes(7, 2, 9) == f(7, 2, 9)
    for bad in ((7, 7, 9), (7, 2, 3), (0, 2, 9)):
        with pytest.raises(nv.NativeError):
            nv.ntuple_budget_search_workspace_bytes(*bad)


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

    def call(boards=a, B=8, w=a, cells=good.ctypes.data, m=2, L=3, F=12, depth=4, budget=600, gamma=1.0, ws=a, nbytes=big, q=a, v=a, used=a,
             ent=a):
        return lib.g2048_ntuple_budget_search(boards, B, w, cells, m, L, F, depth, budget, gamma, ws, nbytes, q, v, used, ent, None)

    def staged(st=tiles.ctypes.data, S=3, boards=a, B=8, depth=4, budget=600, gamma=1.0, nbytes=big):
        return lib.g2048_ntuple_staged_budget_search(boards, B, a, good.ctypes.data, 2, 3, st, S, 12, depth, budget, gamma, a, nbytes, a, a,
                                                     None, None, None)

    need = lib.g2048_ntuple_budget_search_workspace_bytes(8, 4, 600)
    settings = [dict(depth=0), dict(depth=7), dict(depth=-1), dict(budget=3), dict(budget=24577), dict(budget=-1),
                dict(gamma=float("nan")), dict(gamma=-0.5), dict(gamma=float("inf")), dict(gamma=float("-inf"))]
    bad = settings + [dict(boards=None), dict(w=None), dict(q=None), dict(v=None), dict(ws=None), dict(cells=None),
                      dict(B=0), dict(B=-3), dict(B=_limit(4, 600) + 1), dict(B=669, depth=6, budget=24576), dict(B=(1 << 20) + 1, depth=1),
                      dict(m=0), dict(m=9), dict(L=0), dict(L=7), dict(cells=hi.ctypes.data), dict(cells=dup.ctypes.data),
                      dict(F=-1), dict(F=21), dict(nbytes=need - 1), dict(nbytes=0), dict(nbytes=-1), dict(nbytes=need, depth=5),
                      dict(nbytes=need, budget=601), dict(boards=a + 8), dict(ws=a + 8), dict(ws=a + 4), dict(w=a + 2), dict(q=a + 2),
                      dict(v=a + 1), dict(ent=a + 2)]
    for kw in bad:
        assert call(**kw) == -1, kw
    for kw in settings + [dict(st=None), dict(S=0), dict(S=9), dict(st=flat.ctypes.data), dict(boards=None), dict(B=0), dict(nbytes=need - 1)]:
        assert staged(**kw) == -1, kw


def test_wrappers_refuse_host_tensors_and_wrong_shapes():
    import torch

    from src.g2048 import native as nv

    B, cells = 4, np.array(N.SMALL, np.uint8)
    boards = torch.zeros((B, 16), dtype=torch.uint8)
    w = torch.zeros((3, 256), dtype=torch.int32)
    q, v = torch.zeros((B, 4)), torch.zeros(B)
    ws = torch.zeros(nv.ntuple_budget_search_workspace_bytes(B, 3, 70), dtype=torch.uint8)
    for workspace in (ws, None):
        with pytest.raises(nv.NativeError):
            nv.ntuple_budget_search(boards, w, cells, 12, 3, 70, 1.0, workspace, q, v)
    for depth, budget in ((7, 70), (0, 70), (3, 3), (3, 24577)):
        with pytest.raises(nv.NativeError):
            nv.ntuple_budget_search(boards, w, cells, 12, depth, budget, 1.0, ws, q, v)
    with pytest.raises(nv.NativeError):
        nv.ntuple_budget_search(boards, w, np.zeros(3, np.uint8), 12, 1, 4, 1.0, ws, q, v)  # tuple_cells is [m, L]
    with pytest.raises(nv.NativeError):
        nv.ntuple_budget_search(boards, w, cells, 12, 1, 4, 1.0, ws, q, v, stage_tiles=np.zeros((2, 2), np.uint8))  # stage_tiles is flat


def _script(name):
    spec = importlib.util.spec_from_file_location("_budget_" + name, os.path.join(ROOT, "2048-ppo-agent_amd", "run", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_method_class_evaluation_and_script_refuse_bad_settings_without_a_device(capsys):
    import inspect

    import torch

    from src.ppo import NTupleBudgetSearchActionFunction, NTupleNetwork
    from src.ppo import ntuple as M
    from src.ppo.q_player import QPlayer
    from src.runs import evaluate_ntuple_budget

    net = NTupleNetwork(N.SMALL, device="cpu")
    fn = NTupleBudgetSearchActionFunction(net)
    assert isinstance(fn, QPlayer) and (fn.max_depth, fn.budget, fn.gamma) == (M.BUDGET_DEFAULT_DEPTH, M.BUDGET_DEFAULT, 1.0)
    fn = NTupleBudgetSearchActionFunction(net, max_depth=6, budget=4, gamma=0.5)
    assert (fn.max_depth, fn.budget, fn.gamma) == (6, 4, 0.5)
    assert fn.use_mask is True and fn.sample_actions is False and fn.compact is True and fn.policy_fn.needs_masks is False
    # one pair of defaults everywhere
    for f in (net.search_budget, NTupleBudgetSearchActionFunction.__init__, evaluate_ntuple_budget):
        p = inspect.signature(f).parameters
        assert (p["max_depth"].default, p["budget"].default, p["gamma"].default) == (M.BUDGET_DEFAULT_DEPTH, M.BUDGET_DEFAULT, 1.0), f
    assert M.BUDGET_WORKSPACE_BYTES == 4 << 30
    boards = torch.zeros((2, 16), dtype=torch.uint8)
    for kw in (dict(max_depth=0), dict(max_depth=7), dict(max_depth=-1), dict(max_depth=1.5), dict(max_depth=2.0), dict(max_depth="1"),
               dict(max_depth=None), dict(max_depth=True), dict(budget=3), dict(budget=24577), dict(budget=-1), dict(budget=600.0),
               dict(budget="600"), dict(budget=None), dict(budget=True), dict(gamma=-0.1), dict(gamma=float("nan")),
               dict(gamma=float("inf")), dict(gamma="x")):
        with pytest.raises(ValueError):
            NTupleBudgetSearchActionFunction(net, **kw)
        with pytest.raises(ValueError):
            net.search_budget(boards, **kw)
        with pytest.raises(ValueError):
            evaluate_ntuple_budget(net, "cpu", num_episodes=1, **kw)
    with pytest.raises(TypeError):
        NTupleBudgetSearchActionFunction(net, None, None, 4)  # max_depth, budget and gamma are keyword-only
    with pytest.raises(ValueError):
        NTupleBudgetSearchActionFunction(object())

    train = _script("train_ntuple")
    args = train.parse_args(["--eval-budget", "600", "--eval-max-depth", "5"])
    assert args.eval_budget == 600 and args.eval_max_depth == 5
    assert train.parse_args(["--eval-budget", "24576"]).eval_max_depth is None and train.parse_args([]).eval_budget is None
    for argv in (["--eval-budget", "3"], ["--eval-budget", "24577"], ["--eval-budget", "x"], ["--eval-budget", "8.5"],
                 ["--eval-budget", "600", "--eval-max-depth", "0"], ["--eval-budget", "600", "--eval-max-depth", "7"],
                 ["--eval-max-depth", "4"]):
        with pytest.raises(SystemExit):
            train.parse_args(argv)
    capsys.readouterr()


def test_chunks_keep_the_workspace_at_or_below_the_bound():
    from src.g2048 import native as nv
    from src.ppo import ntuple as M

    f = nv.load().g2048_ntuple_budget_search_workspace_bytes
    for max_depth, budget in ((1, 4), (2, 70), (3, 24576), (4, 8192), (5, 24576), (6, 24576), (6, 4)):
        n = M.budget_chunk(max_depth, budget)
        assert n >= 1 and 0 < f(n, max_depth, budget) <= M.BUDGET_WORKSPACE_BYTES
        assert not 0 < f(n + 1, max_depth, budget) <= M.BUDGET_WORKSPACE_BYTES  # the most roots that do


# ---------------------------------------------------------------------------------------------- the reference checks itself
@pytest.mark.parametrize("shape", ["small", "other"])
def test_reference_reproduces_the_recorded_depths(shape):
    boards = FR.boards_for(shape)
    dead = ~(FR.R.expand(boards)[2] > 0).any(axis=1)
    assert dead.sum() == (5 if shape == "small" else 1)
    for budget, hist in BR.HISTOGRAMS[shape].items():
        d, entries, over = BR.depths(boards, 4, budget, with_over=True)
        assert tuple(int((d == k).sum()) for k in (1, 2, 3, 4)) == hist, budget
        assert (d[dead] == 4).all() and (entries[dead] == 0).all()  # no move: U_j = 0 everywhere, d = max_depth
        assert (entries <= budget).all() and ((over == 0) | (over > budget)).all() and ((over > 0) == (d < 4))[~dead].all()
        for i in range(len(boards)):
            assert (entries[i, d[i]:] == 0).all() and (entries[i, :d[i]] > 0).all() != dead[i]
    if shape == "small":
        d, entries = BR.depths(boards, 4, 8)
        assert entries[14, 1] == 8 and d[14] == 2  # U_2 = 8 sits on the boundary of <=
        assert BR.depths(boards[14:15], 4, 7)[0][0] == 1


def test_reference_reaches_depth_five():
    deep = BR.DEEP
    boards = FR.boards_for("small")[list(deep["boards"])]
    d, entries, over = BR.depths(boards, deep["max_depth"], deep["budget"], with_over=True)
    assert tuple(d) == deep["depth"] and over[3] == deep["u5_of_27"]
    for i, want in enumerate(deep["entries"]):
        assert tuple(entries[i, :5]) == want


def test_reference_equals_the_frontier_reference_where_the_rule_admits_every_root():
    """A budget every level fits is the fixed depth: the same bits as ntuple_frontier_ref's case, the same counts summed."""
    c = FR.case("small", 3)
    b = BR.case("small", 3, 24576)
    assert (b["depth"] == 3).all()
    for g in X.GAMMAS:
        assert np.array_equal(b["q"][g].view(np.uint32), c["q"][g].view(np.uint32))
        assert np.array_equal(b["v"][g].view(np.uint32), c["v"][g].view(np.uint32))
    assert np.array_equal(b["entries"][:, :3].sum(axis=0), c["counts"][True])


# ---------------------------------------------------------------------------------------------- the kernels' per-lane code on the host
HOST_SRC = os.path.join(ROOT, "tests", "host_swar", "ntuple_budget_host.cpp")
CSRC = os.path.join(ROOT, "2048-ppo-agent_amd", "csrc")
SMALL_TABLE = dict(slots=600, max_budget=70)  # 70 + 511 entries at the most in 600 slots: probe sequences wrap
SMALL_BLOCK = 16  # regions of budget + 16 entries


def _build(name, *flags):
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, name)
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", *flags, "-I", CSRC, "-o", so, HOST_SRC])
    lib = C.CDLL(so)
    lib.hst_ntb_workspace_bytes.restype = C.c_int64
    return lib


@pytest.fixture(scope="module")
def host():
    return _build("libntuple_budget_host.so")


@pytest.fixture(scope="module")
def host_small_table():
    return _build("libntuple_budget_host_t600.so", f"-DNTB_TABLE_SLOTS={SMALL_TABLE['slots']}", f"-DNTB_MAX_BUDGET={SMALL_TABLE['max_budget']}")


@pytest.fixture(scope="module")
def host_small_block():
    return _build("libntuple_budget_host_b16.so", f"-DNTB_BLOCK={SMALL_BLOCK}")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def host_search(host, c, max_depth, budget, gamma, fill=0xFF, same_layout=True, outputs=True):
    from src.g2048 import native as nv

    boards, cells = c["boards"], N.cells_array(c["tuples"])
    tiles = None if c["tiles"] is None else np.array(c["tiles"], np.uint8)
    B = len(boards)
    need = host.hst_ntb_workspace_bytes(C.c_int64(B), C.c_int(max_depth), C.c_int(budget))
    assert need > 0
    if same_layout:
        assert need == nv.load().g2048_ntuple_budget_search_workspace_bytes(B, max_depth, budget)  # one layout
    raw = np.full(need + 16 + 64, fill, np.uint8)
    at = (-raw.ctypes.data) % 16
    ws = raw[at:at + need + 64]  # 16-byte aligned, with a guard tail
    ws[need:] = 0x5A
    q, v = np.full((B + 1, 4), -7, F32), np.full(B + 1, -7, F32)
    used, entries = (np.full(B + 1, 0xEE, np.uint8), np.full((B + 1, 6), -7, np.int32)) if outputs else (None, None)
    rc = host.hst_ntb_search(_p(boards), C.c_int64(B), _p(c["weights"]), _p(cells), C.c_int(cells.shape[0]), C.c_int(cells.shape[1]),
                             _p(tiles), C.c_int(1 if tiles is None else len(tiles) + 1), C.c_int(c["frac_bits"]), C.c_int(max_depth),
                             C.c_int(budget), C.c_double(gamma), _p(ws), _p(q), _p(v), _p(used), _p(entries))
    assert rc == 0 and (ws[need:] == 0x5A).all() and (q[B:] == -7).all() and v[B] == -7  # nothing past the documented sizes
    if not outputs:
        return q[:B], v[:B], None, None
    assert used[B] == 0xEE and (entries[B] == -7).all()
    return q[:B], v[:B], used[:B], entries[:B]


def _check(c, got, gamma):
    q, v, used, entries = got
    legal = c["legal"]
    assert np.array_equal(used, c["depth"]) and np.array_equal(entries, c["entries"]), (used, c["depth"])
    assert np.array_equal(_bits(q), _bits(c["q"][gamma])) and np.array_equal(_bits(v), _bits(c["v"][gamma])), gamma
    assert (_bits(q)[~legal] == 0).all() and (_bits(v)[~legal.any(axis=1)] == 0).all()  # +0


@pytest.mark.parametrize("budget", BR.BUDGETS)
@pytest.mark.parametrize("name", BR.NETWORKS)
def test_host_build_equals_the_reference(host, name, budget):
    """The 35 boards under the m = 3, L = 2 network, the 12 under the others: depth_used, entries, scores and values at both gammas."""
    c = BR.case(name, 4, budget)
    hist = BR.HISTOGRAMS["small" if name == "small" else "other"][budget]
    assert tuple(int((c["depth"] == k).sum()) for k in (1, 2, 3, 4)) == hist
    seen = []
    for gamma in X.GAMMAS:
        got = host_search(host, c, 4, budget, gamma)
        _check(c, got, gamma)
        seen.append(got[0])
    assert (seen[0] != seen[1]).any()  # gamma reaches the result
    if budget > 600:  # the largest case runs the serial host build twice, not four times
        return
    # the workspace's initial contents do not matter, and the two optional outputs are optional
    _check(c, host_search(host, c, 4, budget, X.GAMMAS[-1], fill=0), X.GAMMAS[-1])
    q, v, _, _ = host_search(host, c, 4, budget, X.GAMMAS[-1], fill=0x7F, outputs=False)
    assert np.array_equal(_bits(q), _bits(seen[-1]))


def test_host_build_reaches_depth_five(host):
    deep = BR.DEEP
    c = BR.case("small", deep["max_depth"], deep["budget"], deep["boards"])
    assert tuple(c["depth"]) == deep["depth"]
    for gamma in X.GAMMAS:
        _check(c, host_search(host, c, deep["max_depth"], deep["budget"], gamma), gamma)


def test_the_stages_reach_the_result():
    c = BR.case("small5", 4, 600)
    unstaged = BR.search(c["boards"], c["tuples"], c["weights"][0], 4, 600, 0.99, frac_bits=c["frac_bits"])[0]
    assert (unstaged.view(np.uint32) != c["q"][0.99].view(np.uint32)).any()


@pytest.mark.parametrize("budget", (8, 70))
def test_a_small_table_wraps_and_keeps_every_bit(host_small_table, budget):
    """600 slots for up to 70 + 511 entries: probe sequences run past the table's end and long.  Same depths, entries and bits."""
    assert host_small_table.hst_ntb_table_slots() == SMALL_TABLE["slots"] and host_small_table.hst_ntb_max_budget() == SMALL_TABLE["max_budget"]
    c = BR.case("small", 4, budget)
    over = BR.depths(c["boards"], 4, budget, with_over=True)[2]
    assert over.max() > (SMALL_TABLE["slots"] if budget == 70 else budget)  # a level larger than the table was begun and abandoned
    _check(c, host_search(host_small_table, c, 4, budget, 0.99), 0.99)
    assert host_small_table.hst_ntb_workspace_bytes(C.c_int64(4), C.c_int(4), C.c_int(SMALL_TABLE["max_budget"] + 1)) == -1


def test_regions_of_one_small_round_at_the_smallest_budget(host_small_block):
    """Rounds of 16 lanes: every region from level 2 on is 4 + 16 entries, level 2 takes 32 rounds, and the test against the budget is
    what keeps a level inside its region (a guard tail follows the workspace)."""
    assert host_small_block.hst_ntb_block() == SMALL_BLOCK
    assert [host_small_block.hst_ntb_level_cap(j, 4) for j in (1, 2, 3, 6)] == [4, 20, 20, 20]
    boards = FR.boards_for("small")
    tuples, w, F, tiles, _ = BR.network("small")
    for max_depth in (4, 6):
        q, v, d, entries = BR.search(boards, tuples, w, max_depth, 4, 0.99)
        c = dict(boards=boards, tuples=tuples, weights=w, frac_bits=F, tiles=tiles, legal=FR.R.expand(boards)[2] > 0, q={0.99: q}, v={0.99: v},
                 depth=d, entries=entries)
        assert (d == 1).sum() > 20 and (d == max_depth).sum() >= 5
        _check(c, host_search(host_small_block, c, max_depth, 4, 0.99, same_layout=False), 0.99)


def test_host_program_runs_clean_under_sanitizers(tmp_path):
    """The per-lane code and the serial emulation as a stand-alone program under ASan + UBSan, once in the device's shape and once
    with rounds of 16 lanes and a table of 600 slots; the workspace and every output are on the heap at exactly their documented
    sizes: an access outside a table, a list, a link row, the workspace or an output would abort it; a NaN in an output (an entry read
    that was never written) fails it."""
    assert shutil.which("g++") is not None
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-static-libasan", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    for tag, flags in (("", []), ("_small", [f"-DNTB_BLOCK={SMALL_BLOCK}", f"-DNTB_TABLE_SLOTS={SMALL_TABLE['slots']}", "-DNTB_MAX_BUDGET=500"])):
        exe = str(tmp_path / ("ntuple_budget_host_asan" + tag))
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-DNTUPLE_BUDGET_HOST_MAIN", *flags, "-I", CSRC, "-o", exe, HOST_SRC])
        out = subprocess.run([exe], capture_output=True, text=True)
        assert out.returncode == 0 and "ntuple_budget_host ok" in out.stdout, (tag, out.stdout[-500:], out.stderr[-2000:])
