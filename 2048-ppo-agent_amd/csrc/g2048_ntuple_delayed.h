// Per-lane code of delayed TD(lambda) / TC(lambda) on the n-tuple network (include/g2048.h, "n-tuple delayed TD(lambda)"): every
// env keeps a ring of its last h afterstates and of their TD errors, and an afterstate is updated ONCE, h - 1 lock-steps after it
// was reached (or when its episode ends), by the lambda-weighted sum of the errors seen since.
//
//   ring       : hist u8 [h][B][16], hist_err f32 [h][B], hist_len u8 [B].  The position is global: at lock-step n the newest
//                afterstate A_{n-1} sits in slot head = (n - 1) mod h, the state j steps back (j = 1 .. hist_len) in slot
//                (head - j + 1) mod h, and link writes A_n to slot n mod h.
//   accumulate : e = sub_rn(flag == 1 ? target : 0, V(hist[head]))  (TD(0)'s e), stored to td_error and hist_err[head];
//                x_1 = e, x_{j+1} = add_rn(hist_err[(head - j) mod h], mul_rn(lam, x_j)) for j + 1 <= hist_len;
//                state j is DUE if flag == 2 (the episode ended: flush) or j == h (which needs hist_len == h);
//                a due state gets delta_j = (int32) rint(clamp(mul_rn(x_j, c), +-2^30)) at each of its 8 m entries:
//                acc += delta_j, cnt += 1, for TC also abs_acc += |delta_j|.  The stage is the updated board's own.
//   apply      : the same due set from flag, hist_len and head; per due board nt_td_apply_lane or nt_tc_apply_lane, unchanged.
//   link       : prev_after = hist[slot] = the new afterstate, hist_len = min((old flag == 2 ? 0 : hist_len) + 1, h).
//
// With h = 1 the only state is the newest one, due at every step with x_1 = e: the TD(0) / TC lanes exactly, whatever lam is.
// The loop over j is a run-time loop (h <= 8) and is not unrolled: the recurrence runs every trip, the heavy body (a 16-byte board
// load, 8 M offsets, the atomics or exchanges) only for a due j, so the steady state of an env (flag 1, one due state) pays one
// such body.  The gathers for V happen once, on the newest board.  Built on g2048_ntuple.h and g2048_ntuple_tc.h only; every f32
// operation is one individually rounded IEEE operation and everything after delta is integer, so the device, the host build
// (G2048_HOST_TEST) and the numpy restatement of tests/ agree bit for bit whatever the scheduling.
#pragma once
#include "g2048_ntuple_tc.h"

namespace g2048 {

enum { NT_MAX_HORIZON = 8 };

// the arguments of the ring every entry point takes: h in 1 .. 8, the position in 0 .. h - 1
inline bool nt_dl_ring_ok(int h, int pos) { return h >= 1 && h <= NT_MAX_HORIZON && pos >= 0 && pos < h; }

// board i of a flat [n][16] array: the device's 16-byte load, a copy in the host build
G_DEV Board nt_dl_board(const uint8_t *p, int64_t i) {
#if G2048_ON_DEVICE
    return load_board(p, i);
#else
    Board b;
    memcpy(b.r, p + 16 * i, 16);
    return b;
#endif
}

// the slot of the state j steps back (j = 1: the newest, in head); head < h and j <= h keep head + h - (j - 1) positive
G_DEV int nt_dl_slot(int head, int h, int j) {
    const int s = head + 1 - j;
    return s < 0 ? s + h : s;
}

// delta from a lambda-sum: nt_td_delta's second half
G_DEV int32_t nt_dl_delta(float x, float c) {
    const float lim = 1073741824.0f;
    float d = mul_rn(x, c);
    d = d < -lim ? -lim : d;
    d = d > lim ? lim : d;
    return (int32_t)rintf(d);  // round half to even
}

// one env of the accumulate launch (flag != 0); returns e (the caller stores it to td_error).  Weights are only read.
template <int M, bool TC>
G_DEV float nt_dl_accumulate_lane(const uint8_t *hist, float *hist_err, int64_t b, int64_t B, int h, int head, int len, u32 flag,
                                  float target, float lam, const int32_t *weights, const NtNet &net, float scale, float c, int64_t *acc,
                                  int64_t *abs_acc, int32_t *cnt) {
    const float v = nt_value(nt_sum<M>(weights, net, nt_dl_board(hist, (int64_t)head * B + b)), scale);
    const float e = nt_sub_rn(flag == 1u ? target : 0.0f, v);
    hist_err[(int64_t)head * B + b] = e;
    float x = e;
#pragma unroll 1
    for (int j = 1; j <= len; ++j) {
        const int64_t at = (int64_t)nt_dl_slot(head, h, j) * B + b;
        if (j > 1) x = add_rn(hist_err[at], mul_rn(lam, x));
        if (flag == 2u || j == h) {
            u32 off[8 * M];
            nt_offsets<M>(net, nt_dl_board(hist, at), off);
            const int64_t delta = nt_dl_delta(x, c);
            const int64_t mag = delta < 0 ? -delta : delta;
#pragma unroll
            for (int k = 0; k < 8 * M; ++k) {
                nt_add_i64(acc + off[k], delta);
                if (TC) nt_add_i64(abs_acc + off[k], mag);
                nt_add_i32(cnt + off[k], 1);
            }
        }
    }
    return e;
}

// one env of the apply launch (flag != 0): the due states of accumulate, newest first
template <int M, bool TC>
G_DEV void nt_dl_apply_lane(const uint8_t *hist, int64_t b, int64_t B, int h, int head, int len, u32 flag, const NtNet &net,
                            int32_t *weights, int64_t *acc, int64_t *abs_acc, int32_t *cnt, int32_t *coh_e, int32_t *coh_a) {
#pragma unroll 1
    for (int j = flag == 2u ? 1 : h; j <= len; ++j) {
        const Board bd = nt_dl_board(hist, (int64_t)nt_dl_slot(head, h, j) * B + b);
        if (TC)
            nt_tc_apply_lane<M>(bd, net, weights, acc, abs_acc, cnt, coh_e, coh_a);
        else
            nt_td_apply_lane<M>(bd, net, weights, acc, cnt);
    }
}

// one env of the link launch: bd is the trajectory row's board and becomes the new afterstate; returns the new hist_len
G_DEV u32 nt_dl_link_lane(Board &bd, u32 meta, u32 old_flag, u32 old_len, int h, u32 &flag) {
    flag = nt_link_lane(bd, meta);
    const u32 len = (old_flag == 2u ? 0u : old_len) + 1u;
    return len < (u32)h ? len : (u32)h;
}

}  // namespace g2048
