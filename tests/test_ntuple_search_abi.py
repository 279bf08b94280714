"""N-tuple expectimax (g2048_ntuple_expectimax): declared, bound, exported; every argument check runs before any device work; the
wrappers refuse host tensors and the classes bad settings without a device; the per-lane code of the two kernels, compiled for the
host and run slot by slot, equals the composed numpy restatements (tests/ntuple_search_ref.py) bit for bit.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import ntuple_ref as N  # noqa: E402
import ntuple_search_ref as X  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = {"g2048_ntuple_expectimax_workspace_floats": 2, "g2048_ntuple_expectimax": 13}
F32 = np.float32


def test_symbols_are_declared_bound_and_exported():
    from src.g2048 import native as nv

    header = open(os.path.join(ROOT, "include", "g2048.h")).read()
    lib = C.CDLL(nv.LIB_PATH)
    assert "int64_t g2048_ntuple_expectimax_workspace_floats(" in header and "int g2048_ntuple_expectimax(" in header
    for name, nargs in NAMES.items():
        assert name in nv.SIGNATURES and len(nv.SIGNATURES[name]) == nargs
        assert hasattr(lib, name)
        assert callable(getattr(nv, name[len("g2048_"):]))
    assert nv.PROTOTYPES["g2048_ntuple_expectimax_workspace_floats"][0] is C.c_int64
    assert "#define G2048_ABI_VERSION 4" in header
    assert nv.load().g2048_abi_version() == 4  # additive: the version stays


def test_workspace_floats_has_three_kinds_of_answer():
    from src.g2048 import native as nv

    f = nv.load().g2048_ntuple_expectimax_workspace_floats
    assert f(1, 1) == 0 and f(1 << 24, 1) == 0                       # one ply: none
    assert f(1, 2) == 128 and f(5, 2) == 640 and f(1 << 20, 2) == 128 << 20  # two plies: 128 per root
    for B, plies in ((0, 1), (-1, 2), ((1 << 24) + 1, 1), ((1 << 20) + 1, 2), (8, 0), (8, 3), (8, -1)):
        assert f(B, plies) == -1, (B, plies)
    assert nv.ntuple_expectimax_workspace_floats(7, 2) == 896
    with pytest.raises(nv.NativeError):
        nv.ntuple_expectimax_workspace_floats(7, 3)


def test_entry_point_rejects_bad_arguments_without_touching_a_device():
    from src.g2048 import native as nv

    lib = nv.load()
    a = 1 << 20  # a fake, 16-byte aligned "device address": rejected before any use
    good = np.array([[0, 1, 2], [4, 5, 6]], np.uint8)
    hi = np.array([[0, 1, 2], [4, 16, 6]], np.uint8)
    dup = np.array([[0, 1, 2], [4, 6, 6]], np.uint8)

    def call(boards=a, B=8, w=a, cells=good.ctypes.data, m=2, L=3, F=12, plies=2, gamma=1.0, ws=a, q=a, v=a):
        return lib.g2048_ntuple_expectimax(boards, B, w, cells, m, L, F, plies, gamma, ws, q, v, None)

    bad = [dict(boards=None), dict(w=None), dict(q=None), dict(v=None), dict(ws=None), dict(cells=None),
           dict(B=0), dict(B=-3), dict(B=(1 << 20) + 1), dict(B=(1 << 24) + 1, plies=1), dict(B=(1 << 24) + 1, plies=1, ws=None),
           dict(m=0), dict(m=9), dict(L=0), dict(L=7), dict(cells=hi.ctypes.data), dict(cells=dup.ctypes.data),
           dict(F=-1), dict(F=21), dict(plies=0), dict(plies=3), dict(plies=-1),
           dict(gamma=-0.5), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(gamma=float("-inf")),
           dict(boards=a + 8), dict(w=a + 2), dict(q=a + 2), dict(v=a + 1), dict(ws=a + 4), dict(ws=a + 4, plies=1)]
    for kw in bad:
        assert call(**kw) == -1, kw


def test_wrappers_refuse_host_tensors():
    import torch

    from src.g2048 import native as nv

    B, cells = 4, np.array(N.SMALL, np.uint8)
    boards = torch.zeros((B, 16), dtype=torch.uint8)
    w = torch.zeros((3, 256), dtype=torch.int32)
    q, v, ws = torch.zeros((B, 4)), torch.zeros(B), torch.zeros(128 * B)
    for plies, workspace in ((1, None), (1, ws), (2, ws), (2, None)):
        with pytest.raises(nv.NativeError):
            nv.ntuple_expectimax(boards, w, cells, 12, plies, 1.0, workspace, q, v)
    with pytest.raises(nv.NativeError):
        nv.ntuple_expectimax(boards, w, cells, 12, 3, 1.0, ws, q, v)  # no such depth
    with pytest.raises(nv.NativeError):
        nv.ntuple_expectimax(boards, w, np.zeros(3, np.uint8), 12, 1, 1.0, None, q, v)  # tuple_cells is [m, L]


def test_classes_refuse_bad_plies_and_gamma_without_a_device():
    import torch

    from src.ppo import NTupleActionFunction, NTupleNetwork
    from src.runs import evaluate_ntuple

    net = NTupleNetwork(N.SMALL, device="cpu")
    fn = NTupleActionFunction(net)
    assert fn.plies == 0 and fn.gamma == 1.0
    fn = NTupleActionFunction(net, plies=2, gamma=0.5)
    assert fn.plies == 2 and fn.gamma == 0.5 and fn.use_mask is True and fn.sample_actions is False and fn.compact is True
    assert fn.policy_fn.needs_masks is False
    boards = torch.zeros((2, 16), dtype=torch.uint8)
    for kw in (dict(plies=3), dict(plies=-1), dict(plies=1.5), dict(plies="1"), dict(plies=None), dict(plies=True),
               dict(plies=1, gamma=-0.1), dict(plies=1, gamma=float("nan")), dict(plies=2, gamma=float("inf")), dict(gamma="x"),
               dict(plies=0, gamma=-1.0)):
        with pytest.raises(ValueError):
            NTupleActionFunction(net, **kw)
        with pytest.raises(ValueError):
            net.expectimax(boards, kw.get("plies", 0), kw.get("gamma", 1.0))
        with pytest.raises(ValueError):
            evaluate_ntuple(net, "cpu", num_episodes=1, **kw)
    with pytest.raises(TypeError):
        NTupleActionFunction(net, None, None, 1)  # plies and gamma are keyword-only


# ---------------------------------------------------------------------------------------------- the kernels' per-lane code on the host
HOST_SRC = os.path.join(ROOT, "tests", "host_swar", "ntuple_search_host.cpp")
CSRC = os.path.join(ROOT, "2048-ppo-agent_amd", "csrc")


@pytest.fixture(scope="module")
def host():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libntuple_search_host.so")
    subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", "-I", CSRC, "-o", so, HOST_SRC])
    return C.CDLL(so)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def host_expectimax(host, boards, w, tuples, plies, gamma, fill=np.nan):
    cells = N.cells_array(tuples)
    B = len(boards)
    ws = np.full(128 * B, fill, F32)
    q, v = np.full((B, 4), -7, F32), np.full(B, -7, F32)
    host.hst_nt_expectimax(_p(boards), C.c_int64(B), _p(w), _p(cells), C.c_int(cells.shape[0]), C.c_int(cells.shape[1]),
                           C.c_int(X.FRAC_BITS), C.c_int(plies), C.c_double(gamma), _p(ws), _p(q), _p(v))
    return q, v, ws


@pytest.mark.parametrize("plies", [1, 2])
@pytest.mark.parametrize("shape", ["small", "wide", "eight"])
def test_host_build_equals_the_composed_restatement(host, shape, plies):
    c = X.case(shape, plies)
    X.check_inputs(c["boards"], c["legal"], c["nchild"])
    assert len(c["tuples"]) == {"small": 3, "wide": 2, "eight": 8}[shape]
    legal = c["legal"]
    seen = []
    for gamma in X.GAMMAS:
        q, v, ws = host_expectimax(host, c["boards"], c["weights"], c["tuples"], plies, gamma)
        assert np.array_equal(_bits(q), _bits(c["q"][gamma])) and np.array_equal(_bits(v), _bits(c["v"][gamma])), gamma
        assert (_bits(q)[~legal] == 0).all() and (_bits(v)[~legal.any(axis=1)] == 0).all()  # +0
        want_v = np.where(legal, q, -np.inf).max(axis=1)
        assert np.array_equal(v[legal.any(axis=1)], want_v[legal.any(axis=1)])
        seen.append(q)
        if gamma != X.GAMMAS[0]:
            continue
        # the workspace's initial contents do not matter, and slots that do not exist are not written
        q0, v0, ws0 = host_expectimax(host, c["boards"], c["weights"], c["tuples"], plies, gamma, fill=0.0)
        assert np.array_equal(_bits(q0), _bits(q)) and np.array_equal(_bits(v0), _bits(v))
        if plies == 2:
            live = ~np.isnan(ws).reshape(-1, 128)
            assert np.array_equal(live.sum(axis=1), c["nchild"]) and np.array_equal(_bits(ws[live.reshape(-1)]), _bits(ws0[live.reshape(-1)]))
        else:
            assert np.isnan(ws).all()
    assert (seen[0] != seen[1]).any()  # gamma reaches the result


def test_one_ply_with_gamma_zero_is_the_reward(host):
    """gamma = 0 leaves the merge reward of every legal move: the search term is multiplied, not dropped."""
    import lookahead_ref as R

    c = X.case("small", 1)
    q, _, _ = host_expectimax(host, c["boards"], c["weights"], c["tuples"], 1, 0.0)
    _, reward, _ = R.expand(c["boards"])
    assert np.array_equal(q, np.where(c["legal"], reward, 0).astype(F32))


def test_host_program_runs_clean_under_sanitizers(tmp_path):
    """The per-lane code as a stand-alone program under ASan + UBSan: an access outside a table, the leaf array or the workspace
    would abort it; a NaN in an output (a workspace entry read that was never written) fails it."""
    assert shutil.which("g++") is not None
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-static-libasan", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = str(tmp_path / "ntuple_search_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-DNTUPLE_SEARCH_HOST_MAIN", "-I", CSRC, "-o", exe, HOST_SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ntuple_search_host ok" in out.stdout, out.stderr[-2000:]
