// Per-lane and per-wave code of the searched n-tuple episode player (include/g2048.h, "n-tuple searched episodes"): whole games
// of an evaluation in which every move is chosen by one ply of expectimax, one wavefront per game.
//
// Nothing is restated: the game (placement, seed, key chain, env_step, the frozen finished game) is g2048_ntuple_episodes.h, the
// search (the fixed slots, the leaf, the serial reduction) is g2048_ntuple_search.h.  What is new is the wave's work split:
//
//   existence  lane l tests slots l and l + 64 (nts_child); the two ballots are the 128-bit set of existing slots, and every
//              existing slot writes itself into a list at its rank, the number of existing slots below it (ntse_rank)
//   leaf       pair p = round * 64 + lane is (rank p >> 2, action p & 3), so the four actions of a child share a quad; the lane
//              reads its slot from the list and scores one move on the child (ntse_leaf_pair); the quad's max over its legal
//              lanes is V0(child), stored at leaf[slot]: addressed by slot, so the packing order changes no bit.
//              ntse_rounds(n_live) rounds instead of the 8 of the fixed slots
//   choose     lanes 0 .. 3 reduce their action over leaf (nts_reduce_lane reads existing slots only, leaf is never cleared),
//              turn Q1 into the engine's logit under the game's own mask (ntse_logit) and take the first maximum (nte_beats)
//
// Every f32 operation is one individually rounded IEEE operation, so the device, the host build (G2048_HOST_TEST, the 64 lanes
// in sequence per phase) and the numpy restatement of tests/ agree bit for bit.
#pragma once
#include "g2048_ntuple_episodes.h"
#include "g2048_ntuple_search.h"

namespace g2048 {

enum { NTSE_WAVE = 64 };

// the engine's masked, clamped logit of action a from a given q (nte_logit's tail): the mask is the game's
G_DEV float ntse_logit(float q, u32 mask, u32 a) {
    const float FMIN = -3.40282347e38f;
    const float v = nt_sub_rn(q, ((mask >> a) & 1u) ? 0.0f : 1e8f);
    return v > FMIN ? v : FMIN;
}

G_DEV u32 ntse_popc64(uint64_t x) { return popc((u32)x) + popc((u32)(x >> 32)); }

// the position of an existing slot in the packed list: the existing slots below it.  lo = slots 0 .. 63, hi = slots 64 .. 127.
G_DEV u32 ntse_rank(uint64_t lo, uint64_t hi, u32 slot) {
    const uint64_t below = ((uint64_t)1 << (slot & 63u)) - 1u;
    return slot < 64u ? ntse_popc64(lo & below) : ntse_popc64(lo) + ntse_popc64(hi & below);
}

// rounds of 64 (rank, action) pairs that cover n_live children: 0 .. 8
G_DEV u32 ntse_rounds(u32 n_live) { return (4u * n_live + (NTSE_WAVE - 1)) / NTSE_WAVE; }

// pair p of the packed leaf pass: Q0(child list[p >> 2], action p & 3).  A pair past the list gathers nothing (legal = false, slot
// = 0); the four pairs of a child are the four lanes of a quad.
template <int M>
G_DEV float ntse_leaf_pair(const int32_t *weights, const NtNet &net, float scale, const Board &pos, const uint8_t *list, u32 n_live,
                           u32 p, u32 &slot, bool &legal) {
    legal = false;
    slot = 0;
    if ((p >> 2) >= n_live) return 0.0f;
    slot = list[p >> 2];
    return nts_leaf_lane<M>(weights, net, scale, pos, slot, p & 3u, legal);
}

}  // namespace g2048
