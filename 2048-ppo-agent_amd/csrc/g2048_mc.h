// Per-lane code of the Monte-Carlo playout player (include/g2048.h, "Monte-Carlo playouts"): one lane = one playout.
//
//   Q(s, a) = mean over r < R of [ sum_t gamma^t r_t  (+ gamma^d V(leaf_r) where the playout was cut off alive) ]
//
// A call has B root boards and R playouts per (board, action) pair: n = 4 B R lanes, lane j = (4 b + a) R + r, and its keys are
// those of index g = lane0 + j of n_total (the env0 / B_total idea of the fused engine: a call cut into slices draws the keys
// of the uncut call).  Step 0 of a lane plays the root action a, every later step the playout policy.  Everything is built on
// g2048_device.h; every f32 operation is one individually rounded IEEE operation in a fixed order, so the device, the host
// build (G2048_HOST_TEST) and the numpy restatement of tests/ agree bit for bit.
#pragma once
#include "g2048_device.h"

namespace g2048 {

enum { MC_POLICY_DRUL = 0, MC_POLICY_RANDOM = 1 };  // the values of G2048_POLICY_DRUL / G2048_POLICY_RANDOM

struct McLane {
    Board bd;
    u32 mask, done;
    float ret, disc;  // discounted return so far, gamma^(steps played)
};

// Exactly-rounded single f32 division (a / b with b = (float)R: no reciprocal, no fast-math form)
G_DEV float mc_div_rn(float a, float b) {
#if G2048_ON_DEVICE
    return __fdiv_rn(a, b);
#else
    volatile float r = a / b;
    return r;
#endif
}

// global step 0: the lane of root action a on `root`.  A lane of an illegal root move is born finished and never runs.
G_DEV void mc_seed(McLane &L, const Board &root, u32 a) {
    L.bd = root;
    L.mask = board_legal(root);
    L.done = ((L.mask >> a) & 1u) ? 0u : 1u;
    L.ret = 0.0f;
    L.disc = 1.0f;
}

// One step of a lane.  first: this is global step 0, the action is the root action (the act sub-key of step 0 is unused).
// (as0, as1) / (ss0, ss1): act / step sub-key of the step, g of n_total: the lane's key index.  Finished lanes are frozen.
template <int MODE, int POLICY>
G_DEV void mc_step(McLane &L, bool first, u32 a_root, u32 as0, u32 as1, u32 ss0, u32 ss1, u32 n_total, u32 g, float gamma) {
    if (L.done) return;
    u32 k0, k1, a;
    if (first) {
        a = a_root;
    } else if (POLICY == MC_POLICY_RANDOM) {
        float lp;
        split_at<MODE>(as0, as1, n_total, g, k0, k1);
        a = policy_random<MODE>(k0, k1, L.mask, lp);
    } else {
        a = policy_drul(L.mask);
    }
    split_at<MODE>(ss0, ss1, n_total, g, k0, k1);
    const float r = env_step<MODE>(L.bd, L.mask, L.done, a, k0, k1);
    L.ret = add_rn(L.ret, mul_rn(L.disc, r));
    L.disc = mul_rn(L.disc, gamma);
}

// q of one (board, action) pair: its R consecutive lanes start at `base`.  x_r = ret_r, or ret_r + disc_r * v_r for a lane that
// is still alive when leaf values are given (a select: a finished lane's value is never read into the sum); the x_r are added
// in ascending r starting from +0, then one division by (float)R.  The order is part of the contract.
G_DEV float mc_reduce_pair(const float *ret, const float *disc, const uint8_t *done, const float *values, int64_t base, int R) {
    float acc = 0.0f;
    for (int r = 0; r < R; ++r) {
        const int64_t i = base + r;
        float x = ret[i];
        if (values && !done[i]) x = add_rn(x, mul_rn(disc[i], values[i]));
        acc = add_rn(acc, x);
    }
    return mc_div_rn(acc, (float)R);
}

}  // namespace g2048
