"""The rollout encoder's features, bit for bit, against a fixture recorded on the MI355X from the parent commit's library (every MFMA
of csrc/g2048_policy.hip in its AGPR form): moving the accumulators to arch VGPRs changes which registers hold a value, never the value.

Fixture: tests/golden/encoder_vgpr_acc.npz, written by tests/golden/make_golden_encoder_vgpr_acc.py (which calls compute() below with
G2048_LIB pointing at the parent's library).  Full f32 rows for B <= 23, sha256 of the rows' bytes above that.

Agent: the default shape (d_model 256, 8 heads, 4 layers, feed-forward 1024) with the weights of tests/golden/weights_recipe.py.
Boards: the first B of a fixed pool of 120 (board_pool()): game-like boards, empty boards, boards with a 2^17 tile, boards whose 16
cells are equal (0, 1, 11, 17 among the values).
B = 1 (a lone partial tile), 6, 7 (a full 7-board tile), 8 (tile + 1), 15, 23 (several tiles, ragged last one), 120 (more tiles than one
wave's window), each in three forms: one kernel (k_encoder_main<FULL>), two kernels (<CLS> + k_encoder_tail<false>), and the two-kernel
form under G2048_ENCODER_KV_WS=1 (<HEAD> + k_encoder_tail<true>); the "mean" agent (k_encoder_main<MEAN>) at B = 1, 8, 23.
"""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

from src.ppo import PPOAgent  # noqa: E402
from src.ppo.fused_policy import FusedPolicy  # noqa: E402
from weights_recipe import fill_state_dict, sample_boards  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "encoder_vgpr_acc.npz")
SWITCH = "G2048_ENCODER_KV_WS"
BOARD_COUNTS = (1, 6, 7, 8, 15, 23, 120)
MEAN_COUNTS = (1, 8, 23)
FORMS = ("one_kernel", "two_kernel", "kv_ws")
FULL_ROWS_MAX = 23  # rows stored up to this B, sha256 above
POOL = 120


def board_pool() -> np.ndarray:
    """u8 [120, 16] exponents.  Row 0 carries a 2^17 tile (B = 1 sees one), row 1 is empty, rows 2..4 have 16 equal cells (1, 17, 11);
    behind them game-like boards, every 9th with a 2^17 tile somewhere, every 13th empty, every 11th all equal (value row % 18)."""
    e = sample_boards(POOL, seed=41).copy()
    e[0] = sample_boards(3, seed=42)[2]
    e[0, 5] = 17
    e[1] = 0
    e[2], e[3], e[4] = 1, 17, 11
    for i in range(5, POOL):
        if i % 9 == 0:
            e[i, i % 16] = 17
        if i % 13 == 0:
            e[i] = 0
        if i % 11 == 0:
            e[i] = i % 18
    return e.astype(np.uint8)


def _policy(reduction, dev):
    agent = PPOAgent(hidden_dim=512, d_model=256, nhead=8, num_layers=4, dim_feedforward=1024, reduction=reduction)
    sd = agent.state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in fill_state_dict({k: tuple(v.shape) for k, v in sd.items()}).items()})
    agent.load_state_dict(sd)
    return FusedPolicy(agent.to(dev).eval())


def _features(fp, boards, form):
    prev = os.environ.pop(SWITCH, None)
    try:
        if form == "kv_ws":
            os.environ[SWITCH] = "1"  # read by the library at every call
        split = None if form == "mean" else form != "one_kernel"
        out = fp.features(boards, split=split)
        torch.cuda.synchronize()
        return out.cpu().numpy()
    finally:
        os.environ.pop(SWITCH, None)
        if prev is not None:
            os.environ[SWITCH] = prev


def compute(dev) -> dict:
    """{case name: f32 [B, 256]} of every case, from the library the binding loaded"""
    pool = torch.from_numpy(board_pool()).to(dev)
    out = {}
    fp = _policy("cls", dev)
    for B in BOARD_COUNTS:
        for form in FORMS:
            out[f"{form}/{B}"] = _features(fp, pool[:B], form)
    fp = _policy("mean", dev)
    for B in MEAN_COUNTS:
        out[f"mean/{B}"] = _features(fp, pool[:B], "mean")
    return out


def digest(rows: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(rows, dtype=np.float32).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def got(dev):
    return compute(dev)


@pytest.fixture(scope="module")
def want():
    with np.load(FIXTURE) as z:
        w = {k: z[k] for k in z.files}
    assert np.array_equal(w.pop("boards"), board_pool()), "the fixture was recorded from another board pool"
    return w


CASES = [f"{form}/{B}" for B in BOARD_COUNTS for form in FORMS] + [f"mean/{B}" for B in MEAN_COUNTS]


def test_pool_has_the_edge_boards():
    p = board_pool()
    assert p.shape == (POOL, 16) and (p[0] == 17).any()
    for B in (6, 23, 120):
        q = p[:B]
        assert (q == 0).all(axis=1).any() and (q == 17).any() and ((q == q[:, :1]).all(axis=1) & (q[:, 0] > 0)).any()


@pytest.mark.parametrize("case", CASES)
def test_bits_of_the_parent_library(got, want, case):
    B = int(case.split("/")[1])
    rows = got[case]
    assert rows.shape == (B, 256) and np.isfinite(rows).all()
    if B <= FULL_ROWS_MAX:
        ref = want[case]
        assert ref.shape == rows.shape and ref.dtype == np.float32
        diff = rows.view(np.uint32) != ref.view(np.uint32)
        assert not diff.any(), (case, int(diff.sum()), float(np.abs(rows - ref).max()))
    else:
        assert digest(rows) == str(want[case + "/sha256"]), case


def test_fixture_holds_every_case(want):
    for case in CASES:
        B = int(case.split("/")[1])
        assert (case if B <= FULL_ROWS_MAX else case + "/sha256") in want, case
