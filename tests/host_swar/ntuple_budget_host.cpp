// Host build of 2048-ppo-agent_amd/csrc/g2048_ntuple_budget.h (G2048_HOST_TEST) for CPU-side logic tests.
// Test infrastructure only: the per-lane code of the budgeted search plus a serial emulation of its kernels
// (g2048_ntuple_budget.hip) over the same workspace layout: the rounds of a build workgroup, the insert into its table and the
// test against the budget run lane by lane in lane order, and all levels of a root are built in one call, as in the one launch.
// The product never builds or loads this.  -DNTB_TABLE_SLOTS=n -DNTB_MAX_BUDGET=k shrinks the table so that probing wraps;
// -DNTB_BLOCK=n shrinks the round and with it every region (budget + NTB_BLOCK entries).  With NTUPLE_BUDGET_HOST_MAIN it is a
// stand-alone program (for a sanitizer build).
#define G2048_HOST_TEST 1
#include "g2048_ntuple_budget.h"

#include <vector>
using namespace g2048;

namespace {

NtNet make_net(const uint8_t *cells, int m, int L, const uint8_t *stage_tiles, int n_stages) {
    NtNet net;
    memset(&net, 0, sizeof(net));
    net.L = L;
    for (int t = 0; t < m; ++t)
        for (int j = 0; j < L; ++j) net.cell[t][j] = cells[t * L + j];
    for (int i = 0; i + 1 < n_stages; ++i) net.stage_tile[i] = stage_tiles[i];
    net.n_stage_tiles = n_stages - 1;
    return net;
}

Board get(const uint8_t *p, int64_t i) {
    Board b;
    memcpy(b.r, p + 16 * i, 16);
    return b;
}

void put(uint8_t *p, int64_t i, const Board &b) { memcpy(p + 16 * i, b.r, 16); }

float quad_best(const float q[4], const bool legal[4]) {
    float x = nt_neg_inf();
    for (int a = 0; a < 4; ++a) x = nt_vmax(x, legal[a] ? q[a] : nt_neg_inf());
    return x == nt_neg_inf() ? 0.0f : x;
}

// one workgroup of k_ntb_build: the levels 1 .. D of root b
void build_root(int64_t b, const uint8_t *boards, uint8_t *ws, const NtbLayout &w) {
    std::vector<int32_t> table(NTB_TABLE_SLOTS), round_idx(NTB_BLOCK);
    std::vector<Board> round_key(NTB_BLOCK);
    const int32_t budget = w.budget;
    int32_t *meta = ntb_meta(ws, w, b);
    const uint8_t *parents = boards + 16 * b;
    int32_t *link_out = ntb_root_link(ws, w, b);
    int32_t n_parents = 1, depth_used = w.depth;
    u32 shift = 2;
    for (int level = 1; level <= w.depth; ++level) {
        std::fill(table.begin(), table.end(), (int32_t)NTF_EMPTY);
        const int32_t cap_out = w.cap[level];
        uint8_t *list_out = ntb_list(ws, w, level, b);
        const u32 n_cand = (u32)n_parents << shift;
        const int max_rounds = ntb_max_rounds(level, budget);
        int32_t count = 0;
        for (int round = 0; round < max_rounds; ++round) {
            if ((u32)round * NTB_BLOCK >= n_cand) break;
            std::vector<int> state(NTB_BLOCK, 0);
            std::vector<int32_t> ref(NTB_BLOCK, 0), rank(NTB_BLOCK, 0);
            std::vector<u32> my_slot(NTB_BLOCK, 0);
            int32_t round_n = 0;
            for (u32 tid = 0; tid < NTB_BLOCK; ++tid) {  // up to barrier (B)
                const u32 cand = (u32)round * NTB_BLOCK + tid;
                if (cand >= n_cand) continue;
                const u32 slot = cand & ((1u << shift) - 1u);
                const Board x = get(parents, (int64_t)(cand >> shift));
                Board key;
                u32 reward;
                if (!(level > 1 ? ntf_candidate(x, slot, key, reward) : ntf_root_candidate(x, slot, key, reward))) continue;
                round_key[tid] = key;
                state[tid] = 2;
                u32 h = ntb_hash(key);
                for (int probe = 0; probe < NTB_TABLE_SLOTS; ++probe) {
                    const int32_t seen = table[h];
                    if (seen == NTF_EMPTY) {
                        table[h] = (int32_t)(0x80000000u | tid);
                        state[tid] = 1;
                        my_slot[tid] = h;
                        break;
                    }
                    const bool known = seen < 0 || seen < cap_out;
                    if (known && !nts_differs(seen < 0 ? round_key[seen & 0xFFFF] : get(list_out, seen), key)) {
                        state[tid] = seen < 0 ? 4 : 3;
                        ref[tid] = seen < 0 ? (seen & 0xFFFF) : seen;
                        break;
                    }
                    h = h + 1 == NTB_TABLE_SLOTS ? 0 : h + 1;
                }
                if (state[tid] == 1 || state[tid] == 2) rank[tid] = round_n++;
            }
            const int32_t base = count;
            count += round_n;
            for (u32 tid = 0; tid < NTB_BLOCK; ++tid) {  // (B) .. (C)
                if (state[tid] != 1 && state[tid] != 2) continue;
                const int32_t idx = base + rank[tid];
                if (idx >= 0 && idx < cap_out) put(list_out, idx, round_key[tid]);
                if (state[tid] == 1) table[my_slot[tid]] = idx;
                round_idx[tid] = idx;
            }
            for (u32 tid = 0; tid < NTB_BLOCK; ++tid) {  // after (C)
                if (!state[tid]) continue;
                const u32 cand = (u32)round * NTB_BLOCK + tid;
                const int32_t idx = state[tid] == 3 ? ref[tid] : (state[tid] == 4 ? round_idx[ref[tid]] : round_idx[tid]);
                link_out[((int64_t)(cand >> shift) << shift) + (cand & ((1u << shift) - 1u))] = idx;
            }
            if (count > budget) break;
        }
        if (count > budget) {
            depth_used = level - 1;
            break;
        }
        meta[level] = count;
        parents = list_out;
        link_out = ntb_link(ws, w, level, b);
        n_parents = count;
        shift = 7;
    }
    meta[0] = depth_used;
    for (int level = depth_used + 1; level < NTB_META; ++level) meta[level] = 0;
}

// k_ntb_leaf: E_1 of every entry of the root's last level
template <int M>
void leaf_root(int64_t b, uint8_t *ws, const NtbLayout &w, const int32_t *weights, const NtNet &net, float scale) {
    const int32_t *meta = ntb_meta(ws, w, b);
    const int level = ntb_depth_used(meta, w.depth);
    const int32_t count = ntb_count(meta, level, w.cap[level]);
    const uint8_t *list = ntb_list(ws, w, level, b);
    float *e_out = ntb_e(ws, w, level, b);
    for (int32_t e = 0; e < count; ++e) {
        const Board x = get(list, e);
        const u32 mask = ntf_empty_mask(x), n2 = 2u * popc(mask);
        float v[32];
        for (u32 k = 0; k < n2; ++k) {  // the quads
            float q[4];
            bool legal[4];
            for (u32 a = 0; a < 4; ++a) q[a] = ntf_leaf_lane<M>(weights, net, scale, x, mask, k, a, legal[a]);
            v[k] = quad_best(q, legal);
        }
        e_out[e] = ntf_expect_ranked(v, n2 >> 1);
    }
}

// k_ntb_backup: E_j of every entry of level j of a root whose search goes below it
void backup_root(int64_t b, uint8_t *ws, const NtbLayout &w, int level, float gamma) {
    const int32_t *meta = ntb_meta(ws, w, b);
    if (ntb_depth_used(meta, w.depth) <= level) return;
    const int32_t count = ntb_count(meta, level, w.cap[level]), cap_next = w.cap[level + 1];
    const uint8_t *list = ntb_list(ws, w, level, b);
    const int32_t *link = ntb_link(ws, w, level, b);
    const float *e_next = ntb_e(ws, w, level + 1, b);
    float *e_out = ntb_e(ws, w, level, b);
    for (int32_t e = 0; e < count; ++e) {
        const Board x = get(list, e);
        alignas(8) float v[32];
        for (u32 quad = 0; quad < 32; ++quad) {
            float q[4];
            bool legal[4];
            for (u32 a = 0; a < 4; ++a) q[a] = ntf_backup_lane(x, quad * 4 + a, link + (int64_t)e * NTF_LINKS, e_next, cap_next, gamma, legal[a]);
            v[quad] = quad_best(q, legal);
        }
        e_out[e] = ntf_expect_cells(v, ntf_empty_mask(x));
    }
}

template <int M>
void search(const uint8_t *boards, int64_t B, const int32_t *weights, const NtNet &net, float scale, int max_depth, int budget,
            float gamma, uint8_t *ws, float *scores, float *values, uint8_t *depth_used, int32_t *entries) {
    const NtbLayout w = ntb_layout(B, max_depth, budget);
    for (int64_t b = 0; b < B; ++b) build_root(b, boards, ws, w);
    for (int64_t b = 0; b < B; ++b) leaf_root<M>(b, ws, w, weights, net, scale);
    for (int j = max_depth - 1; j >= 1; --j)
        for (int64_t b = 0; b < B; ++b) backup_root(b, ws, w, j, gamma);
    for (int64_t b = 0; b < B; ++b) {  // k_ntb_roots
        bool legal[4];
        const Board root = get(boards, b);
        for (u32 a = 0; a < 4; ++a)
            scores[4 * b + a] = ntf_root_lane(root, a, ntb_root_link(ws, w, b), ntb_e(ws, w, 1, b), w.cap[1], gamma, legal[a]);
        values[b] = quad_best(scores + 4 * b, legal);
        const int32_t *meta = ntb_meta(ws, w, b);
        const int d = ntb_depth_used(meta, w.depth);
        if (depth_used) depth_used[b] = (uint8_t)d;
        if (entries)
            for (int level = 1; level <= NTB_MAX_DEPTH; ++level)
                entries[b * NTB_MAX_DEPTH + level - 1] = level <= d ? ntb_count(meta, level, w.cap[level]) : 0;
    }
}

}  // namespace

#define NTB_SWITCH(FN, m, ...)             \
    switch (m) {                           \
        case 1: FN<1>(__VA_ARGS__); break; \
        case 2: FN<2>(__VA_ARGS__); break; \
        case 3: FN<3>(__VA_ARGS__); break; \
        case 4: FN<4>(__VA_ARGS__); break; \
        case 5: FN<5>(__VA_ARGS__); break; \
        case 6: FN<6>(__VA_ARGS__); break; \
        case 7: FN<7>(__VA_ARGS__); break; \
        default: FN<8>(__VA_ARGS__); break; \
    }

extern "C" {
// -1 for what the entry points refuse, as g2048_ntuple_budget_search_workspace_bytes
int64_t hst_ntb_workspace_bytes(int64_t B, int max_depth, int budget) {
    if (!ntb_settings_ok(max_depth, budget) || B < 1 || B > ntb_max_roots(max_depth, budget)) return -1;
    return ntb_layout(B, max_depth, budget).bytes;
}
int hst_ntb_table_slots() { return NTB_TABLE_SLOTS; }
int hst_ntb_block() { return NTB_BLOCK; }
int hst_ntb_max_budget() { return NTB_MAX_BUDGET; }
int hst_ntb_level_cap(int level, int budget) { return ntb_level_cap(level, budget); }

// workspace u8[hst_ntb_workspace_bytes(B, max_depth, budget)] (16-byte aligned), q f32[B][4], v f32[B], depth_used u8[B] or null,
// entries i32[B][6] or null.  Returns -1 and touches nothing for settings without a workspace size.
int hst_ntb_search(const uint8_t *boards, int64_t B, const int32_t *w, const uint8_t *cells, int m, int L, const uint8_t *stage_tiles,
                   int n_stages, int frac_bits, int max_depth, int budget, double gamma, uint8_t *workspace, float *q, float *v,
                   uint8_t *depth_used, int32_t *entries) {
    if (hst_ntb_workspace_bytes(B, max_depth, budget) < 0) return -1;
    const NtNet net = make_net(cells, m, L, stage_tiles, n_stages);
    NTB_SWITCH(search, m, boards, B, w, net, nt_scale(frac_bits), max_depth, budget, (float)gamma, workspace, q, v, depth_used, entries);
    return 0;
}
}

#ifdef NTUPLE_BUDGET_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>

// every max_depth 1 .. 4 at budgets on both sides of the small levels' sizes, on boards that include the one-tile board (the widest
// levels), a full board without a move and tiles 16 and 17, from a 0xFF-patterned workspace of exactly the documented size and
// outputs of exactly their sizes (on the heap: the sanitizer guards their ends).  Exits non-zero if an output is NaN, if the board
// without a move is not worth +0 at depth max_depth, if depth_used or entries break the rule's own consequences, or if a deeper
// max_depth changes what a shallower one reported about the levels both built.
int main() {
    const int m = 3, L = 2, F = 12;
    const uint8_t cells[m * L] = {0, 1, 5, 6, 3, 15};
    const int64_t E = (int64_t)m << (4 * L), B = 4;
    std::vector<int32_t> w(E);
    std::vector<uint8_t> boards(16 * B, 0);
    uint32_t s = 12345u;
    auto rnd = [&]() { return s = s * 1664525u + 1013904223u; };
    for (auto &x : w) x = (int32_t)(rnd() >> 11) - (1 << 20);
    boards[16 * 0 + 5] = 1;                                                                        // one tile
    for (int c = 0; c < 16; ++c) boards[16 * 1 + c] = (uint8_t)(1 + ((c + (c >> 2)) & 1));         // full, no move
    for (int c = 0; c < 16; ++c) boards[16 * 2 + c] = (uint8_t)(c & 1 ? 0 : 16 + ((c >> 1) & 1));  // tiles 16 and 17
    for (int64_t b = 3; b < B; ++b)
        for (int c = 0; c < 16; ++c) boards[16 * b + c] = (uint8_t)(rnd() >> 29);
    const int budgets[] = {NTB_MIN_BUDGET, 9, 70, NTB_MAX_BUDGET < 600 ? NTB_MAX_BUDGET : 600};
    for (int budget : budgets) {
        std::vector<int32_t> before;
        for (int max_depth = 1; max_depth <= 4; ++max_depth) {
            const int64_t bytes = hst_ntb_workspace_bytes(B, max_depth, budget);
            if (bytes <= 0) return 1;
            uint8_t *ws = static_cast<uint8_t *>(aligned_alloc(16, (size_t)bytes));
            memset(ws, 0xFF, (size_t)bytes);  // every f32 a NaN, every index out of range
            float *q = static_cast<float *>(malloc(sizeof(float) * 4 * B)), *v = static_cast<float *>(malloc(sizeof(float) * B));
            uint8_t *d = static_cast<uint8_t *>(malloc(B));
            int32_t *u = static_cast<int32_t *>(malloc(sizeof(int32_t) * 6 * B));
            for (int i = 0; i < 4 * B; ++i) q[i] = nanf("");
            for (int i = 0; i < B; ++i) v[i] = nanf("");
            int rc = hst_ntb_search(boards.data(), B, w.data(), cells, m, L, nullptr, 1, F, max_depth, budget, 0.99, ws, q, v, d, u) ? 9 : 0;
            for (int i = 0; i < 4 * B && !rc; ++i)
                if (!(q[i] == q[i])) rc = 2;
            for (int i = 0; i < B && !rc; ++i)
                if (!(v[i] == v[i])) rc = 3;
            if (!rc && (q[4] != 0.0f || q[5] != 0.0f || q[6] != 0.0f || q[7] != 0.0f || v[1] != 0.0f || d[1] != max_depth)) rc = 4;
            for (int64_t b = 0; b < B && !rc; ++b) {
                if (d[b] < 1 || d[b] > max_depth) rc = 5;
                for (int j = 1; j <= 6 && !rc; ++j) {
                    const int32_t n = u[6 * b + j - 1];
                    if (j > d[b] ? n != 0 : (n < 0 || n > budget)) rc = 6;
                    // what a shallower max_depth reported stays: the levels are the same, only more of them are built
                    if (!rc && !before.empty() && j <= before[7 * b] && before[7 * b] < max_depth - 1 && n != before[7 * b + j]) rc = 7;
                    if (!rc && !before.empty() && before[7 * b] < max_depth - 1 && b != 1 && d[b] != before[7 * b]) rc = 8;
                }
            }
            if (!rc) {
                before.assign(7 * B, 0);
                for (int64_t b = 0; b < B; ++b) {
                    before[7 * b] = d[b];
                    for (int j = 1; j <= 6; ++j) before[7 * b + j] = u[6 * b + j - 1];
                }
            }
            free(ws); free(q); free(v); free(d); free(u);
            if (rc) {
                printf("ntuple_budget_host: check %d failed at budget %d, max_depth %d\n", rc, budget, max_depth);
                return rc;
            }
        }
    }
    printf("ntuple_budget_host ok\n");
    return 0;
}
#endif
