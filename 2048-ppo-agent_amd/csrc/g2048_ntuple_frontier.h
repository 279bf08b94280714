// Per-lane code of the n-tuple frontier search (include/g2048.h, "n-tuple frontier search"): expectimax of 1 .. 3 plies over the
// n-tuple network on packed lists of afterstates, one list per level, with the equal afterstates of one root merged.
//
//   E_1(x)   = nts_div_rn(acc, n),  acc = sum over the empty cells c of x, ascending, from +0, of
//              0.9f V_0(x + tile 2 at c) + 0.1f V_0(x + tile 4 at c);  V_0 = v of g2048_ntuple_scores
//   E_j(x)   = the same over V_{j-1};  V_j(p) = max over the legal a of (float)r(p,a) + gamma E_j(after_a(p)), +0 if there is none
//   Q_d(s,a) = (float)r(s,a) + gamma E_d(after_a(s)) where a is legal, +0 where not
//
// A_1 holds the legal afterstates of the roots and A_{j+1} the afterstates after_a'(x + tile at c) over the entries x of A_j, their
// empty cells c, both tiles and the legal a'.  A parent has 128 fixed link slots, slot = (cell * 2 + tile - 1) * 4 + a'; a slot
// exists if the cell is empty in x and a' moves the child.  E_j is a pure function of the 16 bytes of x, so two equal entries of one
// root are one entry and no output bit depends on whether, or in which order, they were merged.  Every f32 operation is one
// individually rounded IEEE operation in the order of nts_reduce_lane (g2048_ntuple_search.h): the device, the host build
// (G2048_HOST_TEST) and the numpy composition of tests/ agree bit for bit.  Built on g2048_device.h, g2048_symmetry.h,
// g2048_ntuple.h and g2048_ntuple_search.h only.
#pragma once
#include "g2048_device.h"
#include "g2048_symmetry.h"
#include "g2048_ntuple.h"
#include "g2048_ntuple_search.h"

// the number of entries of one root's level that the dedup table takes: while a level has at most this many unique entries,
// merging is complete; past it the table is only looked up and new entries are appended unmerged
#ifndef NTF_TABLE_CAP
#define NTF_TABLE_CAP 8192
#endif

namespace g2048 {

enum {
    NTF_MAX_DEPTH = 3,
    NTF_LINKS = 128,          // link slots per parent afterstate
    NTF_ROOT_LINKS = 4,       // link slots per root: one per action
    NTF_BLOCK = 512,          // lanes of an expand workgroup = candidates of one round
    NTF_TABLE_SLOTS = 12288,  // open addressing, linear probing: holds at most NTF_TABLE_CAP - 1 + NTF_BLOCK entries
    NTF_EMPTY = -1,           // a free table slot; >= 0: an entry index; < -1: claimed in this round by lane (value & 0xFFFF)
    NTF_CAP1 = 4,             // the most entries of one root at level 1, 2, 3 without merging
    NTF_CAP2 = 480,
    NTF_CAP3 = 57600
};

static_assert(NTF_TABLE_CAP >= 1 && NTF_TABLE_CAP - 1 + NTF_BLOCK < NTF_TABLE_SLOTS, "the table must keep free slots");
static_assert(NTF_CAP1 * NTF_LINKS <= NTF_BLOCK, "the levels that are expanded again must be built in one round");

G_DEV int64_t ntf_level_cap(int level) { return level == 1 ? NTF_CAP1 : (level == 2 ? NTF_CAP2 : NTF_CAP3); }

G_DEV u32 ntf_row(const Board &x, u32 row) { return row == 0 ? x.r[0] : (row == 1 ? x.r[1] : (row == 2 ? x.r[2] : x.r[3])); }

// bit c is set where cell c of x is empty
G_DEV u32 ntf_empty_mask(const Board &x) {
    u32 m = 0;
#pragma unroll
    for (u32 c = 0; c < 16; ++c) m |= (((x.r[c >> 2] >> (8u * (c & 3u))) & 0xFFu) == 0 ? 1u : 0u) << c;
    return m;
}

// the cell of the set bit of mask with `rank` set bits below it (rank < popc(mask))
G_DEV u32 ntf_nth_cell(u32 mask, u32 rank) {
    u32 cell = 0, seen = 0;
#pragma unroll
    for (u32 c = 0; c < 16; ++c) {
        const bool here = ((mask >> c) & 1u) != 0;
        cell = (here && seen == rank) ? c : cell;
        seen += here ? 1u : 0u;
    }
    return cell;
}

// x with `tile` (1 or 2) in the empty cell `cell`
G_DEV Board ntf_spawn(const Board &x, u32 cell, u32 tile) {
    Board child = x;
    const u32 row = cell >> 2, sh = 8u * (cell & 3u);
#pragma unroll
    for (int i = 0; i < 4; ++i) child.r[i] |= (row == (u32)i) ? (tile << sh) : 0u;
    return child;
}

// the afterstate in link slot `slot` of the afterstate x, and its reward.  Returns whether the slot exists (after is garbage if not).
G_DEV bool ntf_candidate(const Board &x, u32 slot, Board &after, u32 &reward) {
    const u32 a = slot & 3u, tile = 1u + ((slot >> 2) & 1u), cell = slot >> 3;
    const bool empty = ((ntf_row(x, cell >> 2) >> (8u * (cell & 3u))) & 0xFFu) == 0;
    const Board child = ntf_spawn(x, cell, tile);
    after = child;
    reward = board_move(after, a);
    return empty && nts_differs(after, child);
}

// the afterstate of action a on the root, and its reward.  Returns whether the move is legal.
G_DEV bool ntf_root_candidate(const Board &root, u32 a, Board &after, u32 &reward) {
    after = root;
    reward = board_move(after, a);
    return nts_differs(after, root);
}

// where the probe sequence of a board starts; equality is always decided on the 16 bytes, never here
G_DEV u32 ntf_hash(const Board &x) {
    u32 h = x.r[0] * 0x9E3779B1u;
    h = (rotl(h, 13) ^ x.r[1]) * 0x85EBCA77u;
    h = (rotl(h, 13) ^ x.r[2]) * 0xC2B2AE3Du;
    h = (rotl(h, 13) ^ x.r[3]) * 0x27D4EB2Fu;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    return h % (u32)NTF_TABLE_SLOTS;
}

G_DEV int32_t ntf_clamp_i32(int32_t x, int32_t lo, int32_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

// One (child, action) lane of the leaf pass on the entry x: child k = rank * 2 + (tile - 1) among the empty cells of x (k < 2 n),
// Q0(child, a).  A lane of an illegal move gathers nothing.
template <int M>
G_DEV float ntf_leaf_lane(const int32_t *weights, const NtNet &net, float scale, const Board &x, u32 mask, u32 k, u32 a, bool &legal) {
    const Board child = ntf_spawn(x, ntf_nth_cell(mask, k >> 1), 1u + (k & 1u));
    return nt_score<M>(weights, net, scale, child, a, legal);
}

// E of an entry with n >= 1 empty cells from v[rank * 2 + (tile - 1)], the values of its children: the ascending-cell serial sum
G_DEV float ntf_expect_ranked(const float *v, u32 n) {
    float acc = 0.0f;
    for (u32 r = 0; r < n; ++r) acc = add_rn(acc, add_rn(mul_rn(0.9f, v[2u * r]), mul_rn(0.1f, v[2u * r + 1u])));
    return nts_div_rn(acc, (float)n);
}

// the same from v[cell * 2 + (tile - 1)]: only the pairs of empty cells are read (mask != 0)
G_DEV float ntf_expect_cells(const float *v, u32 mask) {
    float acc = 0.0f;
    u32 n = 0;
#pragma unroll
    for (u32 c = 0; c < 16; ++c) {
        if ((mask >> c) & 1u) {
            float v2, v4;
            nts_pair(v + 2u * c, v2, v4);
            acc = add_rn(acc, add_rn(mul_rn(0.9f, v2), mul_rn(0.1f, v4)));
            ++n;
        }
    }
    return nts_div_rn(acc, (float)n);
}

// One link-slot lane of the backup pass on the entry x of level j: (float)r + gamma E_{j+1}(linked entry).  link is the entry's
// row of 128; only an existing slot's link is read, and it is clamped to the list it points into.
G_DEV float ntf_backup_lane(const Board &x, u32 slot, const int32_t *link, const float *e_next, int32_t cap_next, float gamma,
                            bool &legal) {
    Board after;
    u32 r;
    legal = ntf_candidate(x, slot, after, r);
    if (!legal) return 0.0f;
    return add_rn((float)r, mul_rn(gamma, e_next[ntf_clamp_i32(link[slot], 0, cap_next - 1)]));
}

// One action lane of the last pass: Q_d(root, a) from E_1 of the linked entry of A_1
G_DEV float ntf_root_lane(const Board &root, u32 a, const int32_t *link, const float *e1, int32_t cap1, float gamma, bool &legal) {
    Board after;
    u32 r;
    legal = ntf_root_candidate(root, a, after, r);
    if (!legal) return 0.0f;
    return add_rn((float)r, mul_rn(gamma, e1[ntf_clamp_i32(link[a], 0, cap1 - 1)]));
}

// ---- the workspace: one layout for the entry points, the kernels' host build and the size function ------------------------------
// counters i32[4] ([j] = |A_j| as built, [0] unused), then per level j <= depth the list u8[cap_j][16] and E f32[cap_j], per level
// j < depth the links i32[cap_j][128] and the roots' segments i32[B][2] (first entry, entries), and the roots' links i32[B][4].
// cap_j = B * NTF_CAPj.  Every array starts 16-byte aligned.
struct NtfLayout {
    int64_t counters, list[NTF_MAX_DEPTH + 1], e[NTF_MAX_DEPTH + 1], link[NTF_MAX_DEPTH + 1], seg[NTF_MAX_DEPTH + 1], root_link, bytes;
    int64_t cap[NTF_MAX_DEPTH + 1];
};

inline NtfLayout ntf_layout(int64_t B, int depth) {
    NtfLayout w;
    memset(&w, 0, sizeof(w));
    int64_t at = 0;
    auto take = [&at](int64_t bytes) {
        const int64_t here = at;
        at += (bytes + 15) & ~(int64_t)15;
        return here;
    };
    w.counters = take(16);
    w.root_link = take(B * NTF_ROOT_LINKS * 4);
    for (int j = 1; j <= depth; ++j) {
        w.cap[j] = B * ntf_level_cap(j);
        w.list[j] = take(w.cap[j] * 16);
        w.e[j] = take(w.cap[j] * 4);
        if (j < depth) {
            w.link[j] = take(w.cap[j] * NTF_LINKS * 4);
            w.seg[j] = take(B * 8);
        }
    }
    w.bytes = at;
    return w;
}

// roots per call: cap_3 and every link index stay below 2^31 and the workspace below 2^36 bytes
inline int64_t ntf_max_roots(int depth) { return depth == 1 ? (int64_t)1 << 20 : (depth == 2 ? (int64_t)1 << 16 : (int64_t)1 << 12); }

}  // namespace g2048
