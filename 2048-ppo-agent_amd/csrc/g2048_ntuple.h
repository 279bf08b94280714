// Per-lane code of the n-tuple afterstate value network (include/g2048.h, "n-tuple network"): table lookups over the eight
// views of a board, and batch-synchronous TD(0) on afterstates with integer accumulation.
//
//   idx(x, t)  = sum_j min(x[c_tj], 15) << 4 j                       (the clamp keeps a 2^16 .. tile inside the table)
//   S(board)   = sum over g < 8, t < m of weights[t][idx(view_g(board), t)]          (int64)
//   V(board)   = (float)S * 2^-F                                     (one int64 -> f32 conversion, one exact multiply)
//
// Multi-stage network (include/g2048.h, "multi-stage n-tuple network"): one [m][16^L] set of tables per stage of the game,
//
//   stage(x)     = #{ i : max over the 16 cells of x[c] >= k_i }     (the UNCLAMPED log2 tile against the n ascending thresholds)
//   off(x, g, t) = ((stage(x) * m + t) << 4 L) + idx(view_g(x), t)   (the position in the flat [S][m][16^L] arrays, S = n + 1)
//
// The stage is that of the board being looked up: the afterstate in nt_score (a merge that creates tile k_i is valued by stage
// i's tables), each leaf's afterstate in expectimax, prev_after in the learners.  The maximum is invariant under the eight
// views, so it is computed once per board.  With S <= 8, m <= 8 and L <= 6 an offset is below 2^30: the u32 offsets stay.  Every
// table access of the three kernel files goes through nt_offsets, so the stage enters there and nowhere else.  The thresholds
// travel in NtNet; their count is wave-uniform and nt_offsets branches on it: a network without thresholds (all-zero, what a
// memset leaves) is the single-stage network and skips the max-tile computation.  The kernels carry a template flag on top
// (nt_kernel_net<STAGED>): launched with STAGED = false the count is a compile-time 0, the branch and everything behind it fold
// away, and the single-stage kernels do no stage work at all.  The lane code itself needs no flag.
//
// The number of tuples M is a template parameter (1 .. 8): the 8 M table offsets of a lane are register arrays with
// constant indices, so all 8 M gathers are in flight before the first is used.  The cells per tuple L stay a run-time
// value (a wave-uniform trip count).  Built on g2048_device.h and g2048_symmetry.h only; every f32 operation is one
// individually rounded IEEE operation and every accumulation is an integer one, so the device, the host build
// (G2048_HOST_TEST) and the numpy restatement of tests/ agree bit for bit whatever the scheduling.
#pragma once
#include "g2048_device.h"
#include "g2048_symmetry.h"

namespace g2048 {

enum { NT_MAX_TUPLES = 8, NT_MAX_CELLS = 6, NT_MAX_FRAC_BITS = 20, NT_MAX_STAGES = 8, NT_MAX_STAGE_TILE = 17 };

// the network's shape: travels in the kernarg (wave-uniform -> SGPRs).  All-zero stage fields: a single stage.
struct NtNet {
    uint8_t cell[NT_MAX_TUPLES][NT_MAX_CELLS];
    int L;
    uint8_t stage_tile[NT_MAX_STAGES];  // the first n_stage_tiles are k_1 < k_2 < ...; the rest stay 0
    int n_stage_tiles;                  // 0 .. NT_MAX_STAGES - 1 thresholds: n_stage_tiles + 1 stages
};

// the network as a kernel instance sees it: STAGED = false pins the threshold count to a compile-time 0
template <bool STAGED>
G_DEV NtNet nt_kernel_net(NtNet net) {
    if (!STAGED) net.n_stage_tiles = 0;
    return net;
}

// ---- the entry points' readers of the network (host code, one definition for the three .hip files) ----------------------------
// the shape, checked and copied into the kernarg struct: m in 1 .. 8, L in 1 .. 6, cells < 16, distinct in a tuple.  Clears net.
inline bool nt_read_net(const uint8_t *tuple_cells, int m, int L, NtNet &net) {
    if (!tuple_cells || m < 1 || m > NT_MAX_TUPLES || L < 1 || L > NT_MAX_CELLS) return false;
    memset(&net, 0, sizeof(net));
    net.L = L;
    for (int t = 0; t < m; ++t) {
        unsigned seen = 0;
        for (int j = 0; j < L; ++j) {
            const uint8_t c = tuple_cells[t * L + j];
            if (c > 15 || ((seen >> c) & 1u)) return false;
            seen |= 1u << c;
            net.cell[t][j] = c;
        }
    }
    return true;
}

// the stages, after nt_read_net: n_stages in 1 .. 8 with n_stages - 1 thresholds in 1 .. 17, strictly ascending.  One stage takes
// no thresholds (stage_tiles may be null and is not read).
inline bool nt_read_stages(const uint8_t *stage_tiles, int n_stages, NtNet &net) {
    if (n_stages < 1 || n_stages > NT_MAX_STAGES || (n_stages > 1 && !stage_tiles)) return false;
    for (int i = 0; i + 1 < n_stages; ++i) {
        const uint8_t k = stage_tiles[i];
        if (k < 1 || k > NT_MAX_STAGE_TILE || (i > 0 && k <= stage_tiles[i - 1])) return false;
        net.stage_tile[i] = k;
    }
    net.n_stage_tiles = n_stages - 1;
    return true;
}

// what every staged entry point asks of its network arguments
inline bool nt_read_staged(const uint8_t *tuple_cells, int m, int L, const uint8_t *stage_tiles, int n_stages, NtNet &net) {
    return nt_read_net(tuple_cells, m, L, net) && nt_read_stages(stage_tiles, n_stages, net);
}

inline bool nt_frac_ok(int frac_bits) { return frac_bits >= 0 && frac_bits <= NT_MAX_FRAC_BITS; }

// ---- memory operations: the compiler's global atomics on the device, plain accesses in the sequential host build -------------
G_DEV void nt_add_i64(int64_t *p, int64_t v) {
#if G2048_ON_DEVICE
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);  // two's complement: the same sum
#else
    *p = (int64_t)((uint64_t)*p + (uint64_t)v);
#endif
}
G_DEV void nt_add_i32(int32_t *p, int32_t v) {
#if G2048_ON_DEVICE
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
G_DEV int32_t nt_exch_i32(int32_t *p, int32_t v) {
#if G2048_ON_DEVICE
    return atomicExch(p, v);
#else
    const int32_t old = *p;
    *p = v;
    return old;
#endif
}

G_DEV float nt_sub_rn(float a, float b) {
#if G2048_ON_DEVICE
    return __fsub_rn(a, b);
#else
    volatile float r = a - b;
    return r;
#endif
}

// ---- index and value ---------------------------------------------------------------------------------------------------
// min(cell c of bd, 15); c is wave-uniform, the row is picked by selects (a register array indexed by a run-time value would
// go to scratch)
G_DEV u32 nt_cell(const Board &bd, u32 c) {
    const u32 row = c >> 2;
    const u32 x = row == 0 ? bd.r[0] : (row == 1 ? bd.r[1] : (row == 2 ? bd.r[2] : bd.r[3]));
    const u32 v = (x >> (8u * (c & 3u))) & 0xFFu;
    return v < 15u ? v : 15u;
}

G_DEV u32 nt_index(const NtNet &net, int t, const Board &bd) {
    u32 idx = 0;
#pragma unroll
    for (int j = 0; j < NT_MAX_CELLS; ++j)
        if (j < net.L) idx |= nt_cell(bd, net.cell[t][j]) << (4 * j);
    return idx;
}

// ---- stage --------------------------------------------------------------------------------------------------------------
// the byte-wise maximum of two words whose bytes are below 128 (log2 tiles are at most 17): SWAR, no cell loop.  (a | 0x80) - b
// never borrows across bytes and keeps bit 7 of a byte exactly where a >= b.
G_DEV u32 nt_max_bytes(u32 a, u32 b) {
    const u32 ge = ((a | 0x80808080u) - b) & 0x80808080u;
    const u32 mask = ge | (ge - (ge >> 7));  // 0xFF in the bytes where a >= b
    return b ^ ((a ^ b) & mask);
}

// the largest log2 tile of the board, unclamped: three byte-wise maxima over the four row words, two folds of the last word
G_DEV u32 nt_max_tile(const Board &bd) {
    u32 x = nt_max_bytes(nt_max_bytes(bd.r[0], bd.r[1]), nt_max_bytes(bd.r[2], bd.r[3]));
    x = nt_max_bytes(x, x >> 16);
    x = nt_max_bytes(x & 0xFFFFu, (x >> 8) & 0xFFu);
    return x & 0xFFu;
}

// stage(bd) = the number of thresholds at or below the largest tile: 0 .. n_stage_tiles, whatever the bytes of bd are (so an
// offset never leaves the [n_stage_tiles + 1][m][16^L] arrays).  The trip count is wave-uniform.
G_DEV u32 nt_stage(const NtNet &net, const Board &bd) {
    const u32 mx = nt_max_tile(bd);
    u32 s = 0;
#pragma unroll
    for (int i = 0; i < NT_MAX_STAGES - 1; ++i)
        if (i < net.n_stage_tiles) s += mx >= (u32)net.stage_tile[i] ? 1u : 0u;
    return s;
}

// off[g M + t] = (stage(bd) M + t) 16^L + idx(view_g(bd), t): the entry's position in the flat [S][m][16^L] arrays (< 2^30).
// The single-stage network (no thresholds) takes the scalar branch around the max-tile computation: base 0, the old offset.
template <int M>
G_DEV void nt_offsets(const NtNet &net, const Board &bd, u32 off[8 * M]) {
    u32 base = 0;
    if (net.n_stage_tiles) base = nt_stage(net, bd) * (u32)M;
#pragma unroll
    for (u32 g = 0; g < 8; ++g) {
        const Board v = sym_view(bd, g);
#pragma unroll
        for (int t = 0; t < M; ++t) off[g * M + t] = ((base + (u32)t) << (4 * net.L)) + nt_index(net, t, v);
    }
}

template <int M>
G_DEV int64_t nt_sum(const int32_t *weights, const NtNet &net, const Board &bd) {
    u32 off[8 * M];
    int32_t w[8 * M];
    nt_offsets<M>(net, bd, off);
#pragma unroll
    for (int k = 0; k < 8 * M; ++k) w[k] = weights[off[k]];  // all gathers issued ...
    int64_t s = 0;
#pragma unroll
    for (int k = 0; k < 8 * M; ++k) s += w[k];  // ... before the first use
    return s;
}

G_DEV float nt_scale(int frac_bits) { return u32_as_float((u32)(127 - frac_bits) << 23); }  // 2^-F
G_DEV float nt_value(int64_t s, float scale) { return mul_rn((float)s, scale); }

G_DEV float nt_vmax(float a, float b) { return a > b ? a : b; }
G_DEV float nt_neg_inf() { return u32_as_float(0xFF800000u); }

// ---- scores: one lane per (board, action) --------------------------------------------------------------------------------
// q of action a on bd: reward + V(afterstate) where the move changes the board, +0 where it does not
template <int M>
G_DEV float nt_score(const int32_t *weights, const NtNet &net, float scale, const Board &bd, u32 a, bool &legal) {
    Board after = bd;
    const u32 r = board_move(after, a);
    legal = ((after.r[0] ^ bd.r[0]) | (after.r[1] ^ bd.r[1]) | (after.r[2] ^ bd.r[2]) | (after.r[3] ^ bd.r[3])) != 0;
    if (!legal) return 0.0f;
    return add_rn((float)r, nt_value(nt_sum<M>(weights, net, after), scale));
}

// ---- TD(0) ---------------------------------------------------------------------------------------------------------------
// e = target - V(prev_after) (target 0 for flag 2), delta = (int32) rint(clamp(e c, +-2^30))
G_DEV int32_t nt_td_delta(float target, u32 flag, float v_prev, float c, float &e) {
    const float lim = 1073741824.0f;
    e = nt_sub_rn(flag == 1u ? target : 0.0f, v_prev);
    float d = mul_rn(e, c);
    d = d < -lim ? -lim : d;
    d = d > lim ? lim : d;
    return (int32_t)rintf(d);  // round half to even
}

// one env of the accumulate launch; returns e (the caller stores it).  flag != 0.  Weights are only read.
template <int M>
G_DEV float nt_td_accumulate_lane(const Board &prev, u32 flag, float target, const int32_t *weights, const NtNet &net,
                                  float scale, float c, int64_t *acc, int32_t *cnt) {
    u32 off[8 * M];
    int32_t w[8 * M];
    nt_offsets<M>(net, prev, off);
#pragma unroll
    for (int k = 0; k < 8 * M; ++k) w[k] = weights[off[k]];
    int64_t s = 0;
#pragma unroll
    for (int k = 0; k < 8 * M; ++k) s += w[k];
    float e;
    const int32_t delta = nt_td_delta(target, flag, nt_value(s, scale), c, e);
#pragma unroll
    for (int k = 0; k < 8 * M; ++k) {
        nt_add_i64(acc + off[k], (int64_t)delta);
        nt_add_i32(cnt + off[k], 1);
    }
    return e;
}

// sign(a) * ((2 |a| + c) / (2 c)): the mean a / c rounded half away from zero (c > 0, |a| < 2^61)
G_DEV int64_t nt_rdiv(int64_t a, int64_t c) {
    const int64_t mag = a < 0 ? -a : a;
    const int64_t q = (2 * mag + c) / (2 * c);
    return a < 0 ? -q : q;
}

G_DEV int32_t nt_sat_i32(int64_t x) {
    const int64_t lo = -2147483647LL - 1, hi = 2147483647LL;
    return (int32_t)(x < lo ? lo : (x > hi ? hi : x));
}

// one env of the apply launch (flag != 0): the lane whose exchange finds cnt > 0 owns the entry
template <int M>
G_DEV void nt_td_apply_lane(const Board &prev, const NtNet &net, int32_t *weights, int64_t *acc, int32_t *cnt) {
    u32 off[8 * M];
    int32_t old[8 * M];
    nt_offsets<M>(net, prev, off);
#pragma unroll
    for (int k = 0; k < 8 * M; ++k) old[k] = nt_exch_i32(cnt + off[k], 0);  // a second hit of the same lane gets 0
#pragma unroll
    for (int k = 0; k < 8 * M; ++k) {
        if (old[k] > 0) {
            const int64_t a = acc[off[k]];
            acc[off[k]] = 0;
            weights[off[k]] = nt_sat_i32((int64_t)weights[off[k]] + nt_rdiv(a, (int64_t)old[k]));
        }
    }
}

// ---- link: the afterstate of the move the engine just recorded ------------------------------------------------------------
// meta = action | mask_before << 2 | done_after << 6; returns the flag (1: the episode goes on, 2: the step ended it)
G_DEV u32 nt_link_lane(Board &bd, u32 meta) {
    board_move(bd, meta & 3u);
    return ((meta >> 6) & 1u) ? 2u : 1u;
}

}  // namespace g2048
