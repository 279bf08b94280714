// Per-lane code of the n-tuple budgeted search (include/g2048.h, "n-tuple budgeted search"): the frontier search of
// g2048_ntuple_frontier.h with a node budget per root instead of one depth for every root.
//
//   U_j(s) = the number of distinct 16-byte afterstates in A_j(s)
//   d(s)   = the largest d in 1 .. D with U_j(s) <= K for every j <= d        (D = max_depth in 1 .. 6, K = budget in 4 .. 24 576)
//   scores(s, a) = Q_{d(s)}(s, a)
//
// A_j, E_j, V_j and Q_d are the frontier search's, every f32 operation in its order: the candidate, leaf, expectation, backup and
// root lanes are ntf_candidate .. ntf_root_lane themselves.  What is new is the layout (every root owns a fixed region per level, so
// workgroups share nothing), the rule that stops a root's build, and a table large enough that merging is always complete: U_j is
// then a function of the root's 16 bytes alone, and so are d(s) and every output bit.  Built on g2048_ntuple_frontier.h only.
#pragma once
#include "g2048_ntuple_frontier.h"

// lanes of a build workgroup = candidates of one round (the device build is 512; a host build may shrink it, and the regions with it)
#ifndef NTB_BLOCK
#define NTB_BLOCK 512
#endif
// slots of a build workgroup's dedup table (open addressing, linear probing) and the largest budget it serves
#ifndef NTB_TABLE_SLOTS
#define NTB_TABLE_SLOTS 32768
#endif
#ifndef NTB_MAX_BUDGET
#define NTB_MAX_BUDGET 24576
#endif

namespace g2048 {

enum {
    NTB_MAX_DEPTH = 6,
    NTB_MIN_BUDGET = 4,  // U_1 <= 4: level 1 always fits, d >= 1
    NTB_META = 8         // i32 per root: [0] = d(s), [j] = U_j for j <= d(s) and 0 beyond, [7] unused
};

// a level is abandoned as soon as it holds more than K entries, and a round adds at most NTB_BLOCK: K + NTB_BLOCK - 1 at the most
static_assert(NTB_MAX_BUDGET >= NTB_MIN_BUDGET && NTB_MAX_BUDGET + NTB_BLOCK - 1 < NTB_TABLE_SLOTS, "the table must keep a free slot");
static_assert(NTB_BLOCK >= 4 && NTB_BLOCK <= 65536 && (NTB_BLOCK & (NTB_BLOCK - 1)) == 0, "a claimed slot names its lane in 16 bits");

// entries of one root's region at level j: the worst case where that is smaller, else the budget plus one round
G_DEV int32_t ntb_level_cap(int level, int budget) {
    const int32_t grown = budget + NTB_BLOCK;
    const int32_t worst = level == 1 ? NTF_CAP1 : (level == 2 ? NTF_CAP2 : grown);
    return worst < grown ? worst : grown;
}

// where the probe sequence of a board starts in the build table (ntf_hash's mix over this table's slots)
G_DEV u32 ntb_hash(const Board &x) {
    u32 h = x.r[0] * 0x9E3779B1u;
    h = (rotl(h, 13) ^ x.r[1]) * 0x85EBCA77u;
    h = (rotl(h, 13) ^ x.r[2]) * 0xC2B2AE3Du;
    h = (rotl(h, 13) ^ x.r[3]) * 0x27D4EB2Fu;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    return h % (u32)NTB_TABLE_SLOTS;
}

// rounds of the build of level j from level j - 1 (level 1: from the root's 4 slots): fixed by the capacity, not by what is read
G_DEV int32_t ntb_max_rounds(int level, int budget) {
    const int64_t cand = level == 1 ? NTF_ROOT_LINKS : (int64_t)ntb_level_cap(level - 1, budget) * NTF_LINKS;
    return (int32_t)((cand + NTB_BLOCK - 1) / NTB_BLOCK);
}

// ---- the workspace: one layout for the entry points, the kernels, their host build and the size function ------------------------
// meta i32[B][8], the roots' links i32[B][4], then per level j <= D the lists u8[B][cap_j][16] and E f32[B][cap_j], and per level
// j < D the links i32[B][cap_j][128].  A link is an index into the SAME root's region of the next level.  Every array starts 16-byte
// aligned.  The struct travels in the kernarg.
struct NtbLayout {
    int64_t meta, root_link, list[NTB_MAX_DEPTH + 1], e[NTB_MAX_DEPTH + 1], link[NTB_MAX_DEPTH + 1], bytes;
    int32_t cap[NTB_MAX_DEPTH + 1];
    int32_t depth, budget;
};

inline NtbLayout ntb_layout(int64_t B, int max_depth, int budget) {
    NtbLayout w;
    memset(&w, 0, sizeof(w));
    int64_t at = 0;
    auto take = [&at](int64_t bytes) {
        const int64_t here = at;
        at += (bytes + 15) & ~(int64_t)15;
        return here;
    };
    w.depth = max_depth;
    w.budget = budget;
    w.meta = take(B * NTB_META * 4);
    w.root_link = take(B * NTF_ROOT_LINKS * 4);
    for (int j = 1; j <= max_depth; ++j) {
        w.cap[j] = ntb_level_cap(j, budget);
        w.list[j] = take(B * w.cap[j] * 16);
        w.e[j] = take(B * w.cap[j] * 4);
        if (j < max_depth) w.link[j] = take(B * w.cap[j] * NTF_LINKS * 4);
    }
    w.bytes = at;
    return w;
}

inline bool ntb_settings_ok(int max_depth, int budget) {
    return max_depth >= 1 && max_depth <= NTB_MAX_DEPTH && budget >= NTB_MIN_BUDGET && budget <= NTB_MAX_BUDGET;
}

// roots per call: B * cap_j * 128, the largest element index of any array, stays below 2^31, and B at or below 2^20.  The
// workspace then stays below 2^36 bytes: at most five levels have links, each below 2^33 bytes, and a level's list and E are
// 20 / 512 of its links.
inline int64_t ntb_max_roots(int max_depth, int budget) {
    int64_t cap = 1;
    for (int j = 1; j <= max_depth; ++j) cap = ntb_level_cap(j, budget) > cap ? ntb_level_cap(j, budget) : cap;
    const int64_t by_index = (((int64_t)1 << 31) - 1) / (cap * NTF_LINKS);
    return by_index < ((int64_t)1 << 20) ? by_index : (int64_t)1 << 20;
}

// the pieces of root b's workspace
G_DEV int32_t *ntb_meta(uint8_t *ws, const NtbLayout &w, int64_t b) { return reinterpret_cast<int32_t *>(ws + w.meta) + b * NTB_META; }
G_DEV int32_t *ntb_root_link(uint8_t *ws, const NtbLayout &w, int64_t b) {
    return reinterpret_cast<int32_t *>(ws + w.root_link) + b * NTF_ROOT_LINKS;
}
G_DEV uint8_t *ntb_list(uint8_t *ws, const NtbLayout &w, int j, int64_t b) { return ws + w.list[j] + b * w.cap[j] * 16; }
G_DEV float *ntb_e(uint8_t *ws, const NtbLayout &w, int j, int64_t b) { return reinterpret_cast<float *>(ws + w.e[j]) + b * w.cap[j]; }
G_DEV int32_t *ntb_link(uint8_t *ws, const NtbLayout &w, int j, int64_t b) {
    return reinterpret_cast<int32_t *>(ws + w.link[j]) + b * w.cap[j] * NTF_LINKS;
}

// d(s) and U_j as the later passes read them: clamped to what they index
G_DEV int32_t ntb_depth_used(const int32_t *meta, int max_depth) { return ntf_clamp_i32(meta[0], 1, max_depth); }
G_DEV int32_t ntb_count(const int32_t *meta, int level, int32_t cap) { return ntf_clamp_i32(meta[level], 0, cap); }

}  // namespace g2048
