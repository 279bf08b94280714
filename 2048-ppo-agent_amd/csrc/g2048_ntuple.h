// Per-lane code of the n-tuple afterstate value network (include/g2048.h, "n-tuple network"): table lookups over the eight
// views of a board, and batch-synchronous TD(0) on afterstates with integer accumulation.
//
//   idx(x, t)  = sum_j min(x[c_tj], 15) << 4 j                       (the clamp keeps a 2^16 .. tile inside the table)
//   S(board)   = sum over g < 8, t < m of weights[t][idx(view_g(board), t)]          (int64)
//   V(board)   = (float)S * 2^-F                                     (one int64 -> f32 conversion, one exact multiply)
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

enum { NT_MAX_TUPLES = 8, NT_MAX_CELLS = 6, NT_MAX_FRAC_BITS = 20 };

// the network's shape: travels in the kernarg (wave-uniform -> SGPRs)
struct NtNet {
    uint8_t cell[NT_MAX_TUPLES][NT_MAX_CELLS];
    int L;
};

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

// off[g M + t] = t 16^L + idx(view_g(bd), t): the entry's position in the flat [m][16^L] arrays (< 2^27)
template <int M>
G_DEV void nt_offsets(const NtNet &net, const Board &bd, u32 off[8 * M]) {
#pragma unroll
    for (u32 g = 0; g < 8; ++g) {
        const Board v = sym_view(bd, g);
#pragma unroll
        for (int t = 0; t < M; ++t) off[g * M + t] = ((u32)t << (4 * net.L)) + nt_index(net, t, v);
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
