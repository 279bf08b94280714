// Per-lane code of the n-tuple episode player (include/g2048.h, "n-tuple episodes"): whole greedy games of an evaluation, the
// board resident in four VGPRs from the first move to the last.
//
// An evaluation is N games in batches of bs; game i is env g = i mod bs of batch j = i / bs, whose B_total = min(bs, N - j bs) and
// whose key chain starts at the batch's seed key.  What the game does is what BatchRunner(seed_j, NTupleActionFunction).collect
// does to env g of B_total:
//
//   seed   chain step -> init sub-key; board, mask = env_init(split_at(sub, B_total, g))
//   step   two chain steps (act sub-key: unused, nothing is sampled; step sub-key);  q[a] = nt_score of the board;
//          l[a] = max(q[a] - (mask bit a ? 0 : 1e8f), -FLT_MAX), act = the first maximum of l (policy_logits with use_mask = 1,
//          sample = 0, restated without its expf / logf tail);  r = env_step(act, split_at(step_sub, B_total, g));
//          ep_len += 1, score += (int64) r  (r is -1 or a merge score below 2^24: exact)
//
// Mapping: one quad per game, lane a of the quad computes l[a] (all 8 M gathers of the afterstate in flight together; a lane whose
// move does not change the board gathers nothing), the quad's argmax carries the action index so that a tie goes to the lower
// action, then the four lanes run the same env_step on the same keys.  The chain lives in the lane: two u32 per game, no host key
// table, so games of different batches share a wave.  A finished game is frozen, chain included.  Built on g2048_device.h,
// g2048_symmetry.h and g2048_ntuple.h only; every f32 operation is one individually rounded IEEE operation, so the device, the
// host build (G2048_HOST_TEST) and the numpy restatement of tests/ agree bit for bit.
#pragma once
#include "g2048_ntuple.h"

namespace g2048 {

struct NteGame {
    Board bd;
    u32 mask, done, len;
    int64_t score;
    u32 c0, c1;  // the head of the game's key chain
};

// game i of an evaluation of N games in batches of bs: its env index g in its batch and the batch's size B_total
G_DEV void nte_place(u32 i, u32 N, u32 bs, u32 &g, u32 &B_total) {
    const u32 first = (i / bs) * bs;
    g = i - first;
    B_total = N - first < bs ? N - first : bs;
}

// one step of the key chain (g2048_chain_keys): key, sub = split(key)
template <int MODE>
G_DEV void nte_chain(u32 &c0, u32 &c1, u32 &s0, u32 &s1) {
    u32 a0, a1;
    split2<MODE>(c0, c1, a0, a1, s0, s1);
    c0 = a0;
    c1 = a1;
}

// the game's first board: (c0, c1) is the batch's seed key
template <int MODE>
G_DEV void nte_seed(NteGame &G, u32 c0, u32 c1, u32 B_total, u32 g) {
    u32 s0, s1, k0, k1;
    G.c0 = c0;
    G.c1 = c1;
    nte_chain<MODE>(G.c0, G.c1, s0, s1);
    split_at<MODE>(s0, s1, B_total, g, k0, k1);
    env_init<MODE>(G.bd, G.mask, k0, k1);
    G.done = 0;
    G.len = 0;
    G.score = 0;
}

// lane a's logit: the engine's masked, clamped score of action a.  The mask is the game's, not nt_score's legal flag.
template <int M>
G_DEV float nte_logit(const int32_t *weights, const NtNet &net, float scale, const NteGame &G, u32 a) {
    const float FMIN = -3.40282347e38f;
    bool legal;
    const float q = nt_score<M>(weights, net, scale, G.bd, a, legal);
    const float v = nt_sub_rn(q, ((G.mask >> a) & 1u) ? 0.0f : 1e8f);
    return v > FMIN ? v : FMIN;
}

// the argmax that carries its index: does (xo, ao) beat (x, a)?  The larger logit, on a tie the lower action: over the four lanes
// in any order this is the first maximum of policy_logits' scan.
G_DEV bool nte_beats(float xo, u32 ao, float x, u32 a) { return xo > x || (xo == x && ao < a); }

// the step all four lanes of the quad take once the action is known.  A finished game changes nothing.
template <int MODE>
G_DEV void nte_step(NteGame &G, u32 act, u32 B_total, u32 g) {
    if (G.done) return;
    u32 s0, s1, k0, k1;
    nte_chain<MODE>(G.c0, G.c1, s0, s1);  // the act sub-key
    nte_chain<MODE>(G.c0, G.c1, s0, s1);  // the step sub-key
    split_at<MODE>(s0, s1, B_total, g, k0, k1);
    const float r = env_step<MODE>(G.bd, G.mask, G.done, act, k0, k1);
    G.len += 1u;
    G.score += (int64_t)r;
}

}  // namespace g2048
