// Per-lane code of temporal-coherence (TC) learning on the n-tuple network (include/g2048.h, "n-tuple TC learning"): TD(0)'s e,
// delta and c (nt_td_delta), and per table entry a step size |E| / A made of two more integer tables:
//
//   accumulate : acc += delta, abs_acc += |delta|, cnt += 1 at each of the env's 8 m entries
//   apply      : n = cnt (> 0), d = rdiv(acc, n), a = rdiv(abs_acc, n)               (|acc| <= abs_acc, so a >= |d|)
//                step = A == 0 ? d : rdiv(d |E|, A);  weights = sat_i32(weights + step)   (the rate is read before the update)
//                E += d, A += a;  if A >= 2^31: E = sign(E) (|E| / 2), A >>= 1
//
// Ranges: |d| <= 2^30 (delta is clamped there and d is a mean of deltas), |E| <= A < 2^31 on entry, so d |E| < 2^61, the range
// nt_rdiv states.  |E + d| <= A + a < 2^31 + 2^30, so one halving brings A below 2^31 again and floor keeps |E| / 2 <= A >> 1:
// both fit int32 for ever.  Built on g2048_ntuple.h; integer arithmetic only after nt_td_delta, so the device, the host build
// (G2048_HOST_TEST) and the numpy restatement of tests/ agree bit for bit whatever the scheduling.
#pragma once
#include "g2048_ntuple.h"

namespace g2048 {

// one env of the accumulate launch; returns e (the caller stores it).  flag != 0.  Weights are only read.
template <int M>
G_DEV float nt_tc_accumulate_lane(const Board &prev, u32 flag, float target, const int32_t *weights, const NtNet &net, float scale,
                                  float c, int64_t *acc, int64_t *abs_acc, int32_t *cnt) {
    u32 off[8 * M];
    int32_t w[8 * M];
    nt_offsets<M>(net, prev, off);
#pragma unroll
    for (int k = 0; k < 8 * M; ++k) w[k] = weights[off[k]];  // all gathers issued ...
    int64_t s = 0;
#pragma unroll
    for (int k = 0; k < 8 * M; ++k) s += w[k];  // ... before the first use
    float e;
    const int64_t delta = nt_td_delta(target, flag, nt_value(s, scale), c, e);
    const int64_t mag = delta < 0 ? -delta : delta;
#pragma unroll
    for (int k = 0; k < 8 * M; ++k) {
        nt_add_i64(acc + off[k], delta);
        nt_add_i64(abs_acc + off[k], mag);
        nt_add_i32(cnt + off[k], 1);
    }
    return e;
}

// the owner's update of entry i, n = the count it exchanged out (> 0): plain accesses
G_DEV void nt_tc_update_entry(u32 i, int32_t n, int32_t *weights, int64_t *acc, int64_t *abs_acc, int32_t *coh_e, int32_t *coh_a) {
    const int64_t d = nt_rdiv(acc[i], (int64_t)n), a = nt_rdiv(abs_acc[i], (int64_t)n);
    int64_t E = coh_e[i], A = coh_a[i];
    const int64_t step = A == 0 ? d : nt_rdiv(d * (E < 0 ? -E : E), A);
    weights[i] = nt_sat_i32((int64_t)weights[i] + step);
    E += d;
    A += a;
    if (A >= 2147483648LL) {
        E = E < 0 ? -((-E) >> 1) : E >> 1;
        A >>= 1;
    }
    coh_e[i] = (int32_t)E;
    coh_a[i] = (int32_t)A;
    acc[i] = 0;
    abs_acc[i] = 0;
}

// one env of the apply launch (flag != 0): the lane whose exchange finds cnt > 0 owns the entry
template <int M>
G_DEV void nt_tc_apply_lane(const Board &prev, const NtNet &net, int32_t *weights, int64_t *acc, int64_t *abs_acc, int32_t *cnt,
                            int32_t *coh_e, int32_t *coh_a) {
    u32 off[8 * M];
    int32_t old[8 * M];
    nt_offsets<M>(net, prev, off);
#pragma unroll
    for (int k = 0; k < 8 * M; ++k) old[k] = nt_exch_i32(cnt + off[k], 0);  // a second hit of the same lane gets 0
#pragma unroll
    for (int k = 0; k < 8 * M; ++k)
        if (old[k] > 0) nt_tc_update_entry(off[k], old[k], weights, acc, abs_acc, coh_e, coh_a);
}

}  // namespace g2048
