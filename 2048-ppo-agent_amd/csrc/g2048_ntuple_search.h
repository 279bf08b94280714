// Per-lane code of expectimax over the n-tuple network (include/g2048.h, "n-tuple expectimax"): one or two plies of search whose
// leaf is the network's own greedy value, without a child buffer.
//
//   Q0(s,a), V0(s)  = q and v of g2048_ntuple_scores
//   Q_k(s,a)        = (float)r(s,a) + gamma * (acc / n_empty),  acc = sum over the empty cells c of after_a(s), ascending, of
//                     0.9f V_{k-1}(after_a + 2 at c) + 0.1f V_{k-1}(after_a + 4 at c);  +0 where a is illegal
//   V_k(s)          = the max of Q_k(s, .) over the legal a, +0 if there is none
//
// The children of a board have FIXED slots: slot = a * 32 + cell * 2 + (tile - 1), 128 of them; a slot exists if move a is legal and
// the cell is empty in after_a.  Ascending cell index over the existing slots is the order of the enumerated pipeline
// (g2048_lookahead.hip), so no counts, offsets or scans are needed.  Every f32 operation is one individually rounded IEEE
// operation, in the order of k_lookahead_reduce; the device, the host build (G2048_HOST_TEST) and the numpy restatements of tests/
// agree bit for bit.  Built on g2048_device.h, g2048_symmetry.h and g2048_ntuple.h only.
#pragma once
#include "g2048_device.h"
#include "g2048_symmetry.h"
#include "g2048_ntuple.h"

namespace g2048 {

enum { NTS_SLOTS = 128 };

G_DEV float nts_div_rn(float a, float b) {
#if G2048_ON_DEVICE
    return __fdiv_rn(a, b);
#else
    volatile float r = a / b;
    return r;
#endif
}

// the (V(tile-2 child), V(tile-4 child)) pair of one cell: p is 8-byte aligned
G_DEV void nts_pair(const float *p, float &v2, float &v4) {
#if G2048_ON_DEVICE
    const float2 v = *reinterpret_cast<const float2 *>(p);
    v2 = v.x;
    v4 = v.y;
#else
    v2 = p[0];
    v4 = p[1];
#endif
}

G_DEV bool nts_differs(const Board &x, const Board &y) {
    return ((x.r[0] ^ y.r[0]) | (x.r[1] ^ y.r[1]) | (x.r[2] ^ y.r[2]) | (x.r[3] ^ y.r[3])) != 0;
}

// child = the board in `slot` of bd: one board_move and one OR.  Returns whether the slot exists (child is garbage if not).
G_DEV bool nts_child(const Board &bd, u32 slot, Board &child) {
    const u32 a = slot >> 5, cell = (slot >> 1) & 15u, tile = 1u + (slot & 1u);
    child = bd;
    board_move(child, a);
    const bool legal = nts_differs(child, bd);
    const u32 row = cell >> 2, sh = 8u * (cell & 3u);
    const u32 x = row == 0 ? child.r[0] : (row == 1 ? child.r[1] : (row == 2 ? child.r[2] : child.r[3]));
    const bool empty = ((x >> sh) & 0xFFu) == 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) child.r[i] |= (row == (u32)i) ? (tile << sh) : 0u;
    return legal && empty;
}

// One (slot, action) lane of the leaf pass: Q0(child in `slot` of pos, a).  A lane of an absent slot or an illegal move gathers
// nothing and returns legal = false.
template <int M>
G_DEV float nts_leaf_lane(const int32_t *weights, const NtNet &net, float scale, const Board &pos, u32 slot, u32 a, bool &legal) {
    Board child;
    legal = false;
    if (!nts_child(pos, slot, child)) return 0.0f;
    return nt_score<M>(weights, net, scale, child, a, legal);
}

// One action lane of the reduction: Q(pos, a) from v[128], the values of pos's children by slot.  Only existing slots are read.
G_DEV float nts_reduce_lane(const Board &pos, u32 a, const float *v, float gamma, bool &legal) {
    Board after = pos;
    const u32 r = board_move(after, a);
    legal = nts_differs(after, pos);
    if (!legal) return 0.0f;
    float acc = 0.0f;
    u32 n = 0;
#pragma unroll
    for (u32 c = 0; c < 16; ++c) {
        if (((after.r[c >> 2] >> (8u * (c & 3u))) & 0xFFu) == 0) {
            float v2, v4;
            nts_pair(v + a * 32u + c * 2u, v2, v4);
            acc = add_rn(acc, add_rn(mul_rn(0.9f, v2), mul_rn(0.1f, v4)));
            ++n;
        }
    }
    return add_rn((float)r, mul_rn(gamma, nts_div_rn(acc, (float)n)));  // a legal move leaves an empty cell: n >= 1
}

}  // namespace g2048
