"""Numpy restatement of carousel shaping for the n-tuple trainer (include/g2048.h, "n-tuple carousel"): record and restart, one env
at a time in plain integer arithmetic, the donor draw from the numpy oracle's split / bits_scalar.  No SWAR: the largest tile is a
plain maximum over the 16 cells.  Also the shared test cases, a replay of a recorded device run and the trainer's whole loop on the C
oracle's env."""
import itertools

import numpy as np

import ntuple_ref as N
from oracle import g2048_oracle as npo

U32 = np.uint32
NO_START = 0xFF
TILES = (3, 6, 17)  # the cases' thresholds: tile 16 against 17 stays in stage 2, tile 17 is stage 3
MODES = (npo.MODE_LEGACY, npo.MODE_PARTITIONABLE)


def cs(boards, tiles) -> np.ndarray:
    """boards u8 [B,16] -> the carousel stage of each: the number of thresholds at or below its largest (unclamped) tile."""
    mx = np.asarray(boards, np.uint8).reshape(-1, 16).max(axis=1).astype(np.int64)
    return sum((mx >= int(k)).astype(np.int64) for k in tiles)


class State:
    """The carousel's state, all-zero at the start."""

    def __init__(self, n: int, B: int):
        self.n, self.B = n, B
        self.pool_boards = np.zeros((n, B, 16), np.uint8)
        self.pool_masks = np.zeros((n, B), np.uint8)
        self.reached = np.zeros(B, np.uint8)
        self.turn = np.zeros(B, U32)
        self.starts = np.zeros(n + 1, np.int64)

    def copy(self):
        out = State(self.n, self.B)
        for k in ("pool_boards", "pool_masks", "reached", "turn", "starts"):
            setattr(out, k, getattr(self, k).copy())
        return out

    def equal(self, other) -> bool:
        return all(np.array_equal(getattr(self, k), getattr(other, k)) for k in ("pool_boards", "pool_masks", "reached", "turn", "starts"))


def record(st: State, boards, masks, flag, tiles) -> None:
    """In place on st.  boards / masks: the envs' state for the next step; flag as link left it."""
    s = cs(boards, tiles)
    for b in range(st.B):
        if flag[b] == 1 and s[b] > st.reached[b]:
            st.pool_boards[s[b] - 1, b] = boards[b]
            st.pool_masks[s[b] - 1, b] = masks[b]
            st.reached[b] = s[b]


def restart(st: State, sub, flag, boards, masks, mode: int) -> np.ndarray:
    """In place on st (reached, turn, starts; never a pool), boards and masks -> start_stage u8 [B]."""
    B, n = st.B, st.n
    u = npo.bits_scalar(npo.split(np.asarray(sub, U32), B, mode), mode)
    out = np.full(B, NO_START, np.uint8)
    for b in range(B):
        if flag[b] != 2:
            continue
        turn = (int(st.turn[b]) + 1) & 0xFFFFFFFF
        st.turn[b] = turn
        c = ((b + turn) & 0xFFFFFFFF) % (n + 1)
        stage = 0
        if c >= 1:
            j = int(u[b]) % B
            if st.pool_masks[c - 1, j] != 0:
                boards[b] = st.pool_boards[c - 1, j]
                masks[b] = st.pool_masks[c - 1, j]
                stage = c
        st.reached[b] = stage
        st.starts[stage] += 1
        out[b] = stage
    return out


# ---------------------------------------------------------------------------------------------- the shared cases
SIZES = (1, 63, 64, 65, 257)
_TOPS = (0, 3, 5, 6, 16, 17, 10, 2)  # the largest tile put on a board: stages 0 1 1 2 2 3 2 0 under TILES


def record_case(B: int) -> dict:
    """One record step on B envs under TILES: flags 0 / 1 / 2 mixed, largest tiles 16 and 17 against threshold 17, jumps of two and
    three stages, reached at or above the board's stage, flag-1 envs with mask 0, and slots that already hold a board.  For B >= 63
    the first seed at which the case contains all of that.  -> the inputs, the state before ("st0") and after ("st"), and "cover",
    what the case contains (asserted by the tests for B >= 63)."""
    for seed in itertools.count():
        c = _record_case(B, seed)
        if B < 63 or (all(v for k, v in c["cover"].items() if k != "flags") and c["cover"]["flags"] == {0, 1, 2}):
            return c


def _record_case(B: int, seed: int) -> dict:
    rng = np.random.default_rng(1000 + 7 * B + seed)
    boards = rng.integers(0, 3, size=(B, 16)).astype(np.uint8)
    top = np.array([_TOPS[(b + seed) % len(_TOPS)] for b in range(B)], np.uint8)
    cell = rng.integers(0, 16, size=B)
    boards[np.arange(B), cell] = np.maximum(boards[np.arange(B), cell], top)
    flag = rng.integers(0, 3, size=B).astype(np.uint8)
    masks = rng.integers(1, 16, size=B).astype(np.uint8)
    masks[rng.random(B) < 0.2] = 0
    st0 = State(len(TILES), B)
    st0.reached = rng.integers(0, len(TILES) + 1, size=B).astype(np.uint8)
    st0.pool_boards = rng.integers(0, 12, size=st0.pool_boards.shape).astype(np.uint8)
    st0.pool_masks = (rng.integers(1, 16, size=st0.pool_masks.shape) * (rng.random(st0.pool_masks.shape) < 0.5)).astype(np.uint8)
    if B == 1:  # the one env records: tile 16 against threshold 17 is stage 2, a jump of two
        boards[0, 5], flag[0], st0.reached[0], masks[0] = 16, 1, 0, 9
    st = st0.copy()
    record(st, boards, masks, flag, TILES)
    s, f1, mx = cs(boards, TILES), flag == 1, boards.max(axis=1)
    wrote = f1 & (s > st0.reached)
    cover = dict(flags=set(flag.tolist()), tile16_stage2=bool((wrote & (mx == 16) & (s == 2)).any()),
                 tile17_stage3=bool((wrote & (mx == 17) & (s == 3)).any()), jump_two=bool((wrote & (s - st0.reached == 2)).any()),
                 jump_three=bool((wrote & (s - st0.reached == 3)).any()), reached_equal=bool((f1 & (s == st0.reached) & (s > 0)).any()),
                 reached_above=bool((f1 & (s < st0.reached)).any()), mask0_written=bool((wrote & (masks == 0)).any()),
                 other_flags_skipped=bool((~f1 & (s > st0.reached)).any()))
    # only slot s - 1 of a recording env changes, nothing of any other env
    changed = (st.pool_boards != st0.pool_boards).any(axis=2) | (st.pool_masks != st0.pool_masks)
    allowed = np.zeros_like(changed)
    allowed[s[wrote] - 1, np.nonzero(wrote)[0]] = True
    assert not (changed & ~allowed).any()
    return dict(boards=boards, masks=masks, flag=flag, st0=st0, st=st, cover=cover)


def _restart_inputs(B: int, rng):
    n = len(TILES)
    st0 = State(n, B)
    st0.pool_masks = (rng.integers(1, 16, size=(n, B)) * (rng.random((n, B)) < 0.5)).astype(np.uint8)
    st0.pool_boards = rng.integers(0, 14, size=(n, B, 16)).astype(np.uint8)  # also in the empty slots: they must not be copied
    st0.reached = rng.integers(0, n + 1, size=B).astype(np.uint8)
    st0.turn = rng.integers(0, 1 << 32, size=B, dtype=np.uint64).astype(U32)
    st0.turn[rng.random(B) < 0.15] = 0xFFFFFFFF
    st0.starts = np.array([5, 1 << 40, 7, -3], np.int64)
    flag = rng.choice(np.array([0, 1, 2, 2, 2], np.uint8), size=B)
    boards = rng.integers(0, 3, size=(B, 16)).astype(np.uint8)
    masks = rng.integers(1, 16, size=B).astype(np.uint8)
    return st0, flag, boards, masks


def restart_case(B: int, mode: int) -> dict:
    """One restart step on B envs: pools part empty, ``turn`` at random with 0xFFFFFFFF among them, starts not zero before.  For
    B >= 63 the first seed at which every stage has both a pool start and a fallback, stage 0 is chosen too and an env at turn
    0xFFFFFFFF restarts; for B = 1 the env is its own donor and starts at its own stage-1 board.  -> inputs ("st0", "flag", "boards0",
    "masks0", "sub"), results ("st", "boards", "masks", "start_stage") and "cover"."""
    for seed in itertools.count():
        rng = np.random.default_rng(2000 + 11 * B + seed)
        st0, flag, boards0, masks0 = _restart_inputs(B, rng)
        sub = rng.integers(0, 1 << 32, size=2, dtype=np.uint64).astype(U32)
        if B == 1:
            st0.turn[0], flag[0], st0.pool_masks[0, 0] = 0, 2, 6  # c = (0 + 1) % 4 = 1
        st, boards, masks = st0.copy(), boards0.copy(), masks0.copy()
        start = restart(st, sub, flag, boards, masks, mode)
        f2 = flag == 2
        c = ((np.arange(B, dtype=np.uint64) + st.turn.astype(np.uint64)) & 0xFFFFFFFF) % (len(TILES) + 1)
        cover = dict(pool={int(x) for x in start[f2 & (start > 0)]}, fallback={int(x) for x in c[f2 & (start == 0) & (c > 0)]},
                     stage0=bool((f2 & (c == 0)).any()), wrapped=bool((f2 & (st0.turn == 0xFFFFFFFF)).any()),
                     flags=set(flag.tolist()))
        full = {1, 2, 3}
        if B == 1 or (cover["pool"] == full and cover["fallback"] == full and cover["stage0"] and cover["wrapped"]):
            break
    assert (start[~f2] == NO_START).all() and (start[f2] <= len(TILES)).all()
    assert np.array_equal(st.starts - st0.starts, np.bincount(start[f2], minlength=len(TILES) + 1))
    assert np.array_equal(boards[~f2], boards0[~f2]) and np.array_equal(boards[start == 0], boards0[start == 0])
    assert (masks[f2 & (start > 0)] != 0).all()
    if B == 1:
        assert start[0] == 1 and np.array_equal(boards[0], st0.pool_boards[0, 0]) and masks[0] == 6
    return dict(st0=st0, flag=flag, boards0=boards0, masks0=masks0, sub=sub, st=st, boards=boards, masks=masks, start_stage=start,
                cover=cover)


def permuted_case(B: int = 257, seed: int = 3) -> dict:
    """The same restart input with the envs in another lane order.  An env's outcome depends on its lane b through its carousel
    position c = (b + turn) % (n + 1) and through its donor draw.  So that "the same input" is defined, an env keeps its position
    when it moves from lane b to lane p[b] (its turn becomes turn + b - p[b]; turns are in B .. 2 B, so nothing wraps), and the
    donor cannot matter: stages 1 and 3 hold one board each in every slot, stage 2 is empty throughout (every draw falls back).
    Then boards, masks and start_stage are the permuted ones and starts is identical.  -> the two inputs ("a", "b": flag, boards0,
    masks0, turn), the shared pools and sub-key, and "p" with b[...][p] = a[...]."""
    rng = np.random.default_rng(3000 + seed)
    n = len(TILES)
    pools = State(n, B)
    for i in (0, 2):
        pools.pool_boards[i, :] = rng.integers(0, 14, size=16).astype(np.uint8)
        pools.pool_masks[i, :] = 5 + i
    pools.pool_boards[1] = rng.integers(0, 14, size=(B, 16)).astype(np.uint8)  # masks 0: empty
    flag = rng.choice(np.array([0, 1, 2, 2], np.uint8), size=B)
    boards0 = rng.integers(0, 3, size=(B, 16)).astype(np.uint8)
    masks0 = rng.integers(1, 16, size=B).astype(np.uint8)
    turn = rng.integers(B, 2 * B, size=B).astype(np.int64)
    p = rng.permutation(B)
    a = dict(flag=flag, boards0=boards0, masks0=masks0, turn=turn.astype(U32))
    b = dict(flag=np.empty_like(flag), boards0=np.empty_like(boards0), masks0=np.empty_like(masks0), turn=np.empty(B, U32))
    b["flag"][p], b["boards0"][p], b["masks0"][p] = flag, boards0, masks0
    b["turn"][p] = (turn + np.arange(B) - p).astype(U32)
    return dict(a=a, b=b, p=p, pools=pools, sub=rng.integers(0, 1 << 32, size=2, dtype=np.uint64).astype(U32))


def run_permuted(case: dict, which: str, mode: int):
    """-> (boards, masks, start_stage, starts, reached) of input ``which`` of a permuted case on the restatement."""
    x = case[which]
    st = case["pools"].copy()
    st.turn = x["turn"].copy()
    boards, masks = x["boards0"].copy(), x["masks0"].copy()
    start = restart(st, case["sub"], x["flag"], boards, masks, mode)
    return boards, masks, start, st.starts, st.reached


# ---------------------------------------------------------------------------------------------- whole runs
def replay(rec_boards, rec_meta, rec_start, final_boards, final_masks, subs, tiles, mode: int):
    """A recorded device run (``train(record=True)``: boards u8 [T,B,16] before each step, meta u8 [T,B], start_stage u8 [T,B]; the
    envs' boards and masks after the last lock-step; subs u32 [2 T, 2], the run's sub-keys) through record and restart.  After step
    t the envs' state is row t + 1's board and the mask in its meta byte; for a restarted env that is already the board it started
    at, which the restatement must reproduce from its own pools.  Asserts every start_stage, board and mask -> the final State and
    the counts {"pool": starts per stage >= 1, "fallback": n, "fresh": n}."""
    T, B = rec_meta.shape
    st = State(len(tiles), B)
    fallback = fresh = 0
    for t in range(T):
        flag = np.where((rec_meta[t] >> 6) & 1, 2, 1).astype(np.uint8)
        nxt_b = final_boards if t + 1 == T else rec_boards[t + 1]
        nxt_m = final_masks if t + 1 == T else (rec_meta[t + 1] >> 2) & 15
        record(st, nxt_b, nxt_m, flag, tiles)
        boards, masks = np.array(nxt_b), np.array(nxt_m, np.uint8)
        turn_before = st.turn.copy()
        start = restart(st, subs[2 * t], flag, boards, masks, mode)
        assert np.array_equal(start, rec_start[t]), t
        assert np.array_equal(boards, nxt_b) and np.array_equal(masks, nxt_m), t
        f2 = flag == 2
        c = ((np.arange(B, dtype=np.uint64) + turn_before.astype(np.uint64) + 1) & 0xFFFFFFFF) % (len(tiles) + 1)
        fallback += int((f2 & (start == 0) & (c > 0)).sum())
        fresh += int((f2 & (c == 0)).sum())
    return st, dict(pool=st.starts[1:].copy(), fallback=fallback, fresh=fresh)


def engine_training(weights, tuples, num_envs: int, lock_steps: int, tiles, alpha: float = 0.1, frac_bits: int = 12, seed: int = 0,
                    mode: int = npo.MODE_PARTITIONABLE):
    """``ntuple_ref.engine_training`` (TD(0) on the C oracle's env and the engine's key chain) with the carousel's two steps after
    link.  In place on weights -> (State, start_stage u8 [T,B], episodes)."""
    from oracle import c_oracle as orc

    B = num_envs
    _, subs = orc.chain(npo.key(seed), 1 + 2 * lock_steps, mode)
    b, m, _ = orc.init(orc.split(subs[0], B, mode), mode)
    prev, flag = np.zeros((B, 16), np.uint8), np.zeros(B, np.uint8)
    st, starts, episodes = State(len(tiles), B), [], 0
    for t in range(lock_steps):
        q, v, legal = N.scores(b, weights, tuples, frac_bits)
        N.td_step(prev, flag, v, weights, tuples, frac_bits, alpha)
        a = N.masked_argmax(q, legal)
        nb, nm, nd, _ = orc.step(b, m, np.zeros(B, np.uint8), a, orc.split(subs[2 + 2 * t], B, mode), mode)
        meta = (a.astype(np.uint8) | (m.astype(np.uint8) << 2) | (nd.astype(np.uint8) << 6)).astype(np.uint8)
        prev, flag = N.link(b, meta)
        if nd.any():
            fb, fm, _ = orc.init(orc.split(npo.fold_in(subs[2 + 2 * t], 0xFFFFFFFF), B, mode), mode)
            nb, nm = np.where(nd[:, None] != 0, fb, nb), np.where(nd != 0, fm, nm)
            episodes += int(nd.sum())
        b, m = np.ascontiguousarray(nb, np.uint8), np.ascontiguousarray(nm, np.uint8)
        record(st, b, m, flag, tiles)
        starts.append(restart(st, subs[1 + 2 * t], flag, b, m, mode))
    return st, np.stack(starts), episodes
