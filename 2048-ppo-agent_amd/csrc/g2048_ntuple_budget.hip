// N-tuple budgeted search (include/g2048.h, "n-tuple budgeted search"): expectimax over the n-tuple network on packed, deduplicated
// lists of afterstates, every root searched as deep (1 .. max_depth <= 6) as its levels stay within a budget of unique entries.
//
//   build   one workgroup of 512 lanes per root builds the root's levels 1 .. D in ONE launch, each in the root's own region of the
//           workspace.  A level is built in the rounds of k_ntf_expand (g2048_ntuple_frontier.hip): a lane per link slot of a parent,
//           the afterstate looked up in the workgroup's LDS table of entry indices (open addressing, linear probing, claimed with a
//           32-bit LDS compare-and-swap), the new entries ranked with an LDS add, appended, and every existing slot linked.  The
//           table holds every entry a level can get, so merging is complete and a level's count is its number of DISTINCT
//           afterstates.  After the last barrier of a round all lanes compare that count with the budget: past it the level is
//           abandoned, the root's depth is the level before, and the workgroup leaves.  A level that completes becomes the parents
//           of the next one: the same workgroup reads back what it wrote, a barrier in between.  No global counter, no atomics on
//           global memory.
//   leaf    E_1 of the entries of every root's level d(root): grid (roots, slices), k_ntf_leaf's 16 lanes per entry.
//   backup  E_j of the entries of level j, for j = D-1 .. 1, of the roots with d(root) > j: grid (roots, slices), 128 lanes per entry.
//   roots   one lane per (root, action): Q, V, depth_used and entries.
//
// D + 2 launches.  Every loop has a trip count fixed by a capacity; every count and link read from memory is clamped to the capacity
// of what it indexes.  No host read, no device-side allocation, no spinning, no communication between workgroups, no float atomics.
// The per-lane code is g2048_ntuple_budget.h (on g2048_ntuple_frontier.h), shared with the host build of the CPU tests.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/g2048.h"
#include "g2048_device.h"
#include "g2048_host.h"
#include "g2048_ntuple_budget.h"

using namespace g2048;
using namespace g2048_host;

namespace {

static_assert(NTB_BLOCK == 512 && NTB_TABLE_SLOTS == 32768 && NTB_MAX_BUDGET == 24576, "the device build has one shape");

constexpr int kBlock = 256;          // leaf, backup, roots
constexpr int kLeafLanes = 16;       // lanes per entry of the leaf pass
constexpr int kLeafEntries = kBlock / kLeafLanes;
constexpr int kBackupEntries = kBlock / NTF_LINKS;
constexpr int kMaxSlices = 64;       // workgroups per root of the leaf and backup passes, at the most

template <int CTRL>
__device__ __forceinline__ float quad_swap(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}

// the max over the legal lanes of a quad, +0 if there is none (every lane of the quad must be active)
__device__ __forceinline__ float quad_best(float q, bool legal) {
    float x = legal ? q : nt_neg_inf();
    x = nt_vmax(x, quad_swap<0xB1>(x));
    x = nt_vmax(x, quad_swap<0x4E>(x));
    return x == nt_neg_inf() ? 0.0f : x;
}

__global__ void __launch_bounds__(NTB_BLOCK) k_ntb_build(const uint8_t *boards, uint8_t *ws, const NtbLayout w) {
    __shared__ int32_t table[NTB_TABLE_SLOTS];
    __shared__ uint4 round_key[NTB_BLOCK];
    __shared__ int32_t round_idx[NTB_BLOCK];
    __shared__ int32_t s_round_n;
    const u32 tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int32_t budget = w.budget;
    int32_t *meta = ntb_meta(ws, w, b);
    const uint8_t *parents = boards + 16 * b;  // level 1: the root is the one parent, with 4 link slots
    int32_t *link_out = ntb_root_link(ws, w, b);
    int32_t n_parents = 1, depth_used = w.depth;
    u32 shift = 2;  // log2 of the link slots per parent
#pragma unroll 1
    for (int level = 1; level <= w.depth; ++level) {
        for (u32 i = tid; i < NTB_TABLE_SLOTS; i += NTB_BLOCK) table[i] = NTF_EMPTY;
        if (tid == 0) s_round_n = 0;
        const int32_t cap_out = w.cap[level];
        uint8_t *list_out = ntb_list(ws, w, level, b);
        const u32 n_cand = (u32)n_parents << shift;
        const int max_rounds = ntb_max_rounds(level, budget);
        int32_t count = 0;  // the level's entries so far: the same in every lane
        __syncthreads();    // the table is clear; the level before is in its list
#pragma unroll 1
        for (int round = 0; round < max_rounds; ++round) {
            if ((u32)round * NTB_BLOCK >= n_cand) break;  // uniform, before the round's barriers
            const u32 cand = (u32)round * NTB_BLOCK + tid;
            const int64_t parent = (int64_t)(cand >> shift);
            const u32 slot = cand & ((1u << shift) - 1u);
            Board key;
            key.r[0] = key.r[1] = key.r[2] = key.r[3] = 0;
            bool exists = false;
            if (cand < n_cand) {
                u32 reward;
                const Board x = load_board(parents, parent);
                exists = level > 1 ? ntf_candidate(x, slot, key, reward) : ntf_root_candidate(x, slot, key, reward);
            }
            round_key[tid] = make_uint4(key.r[0], key.r[1], key.r[2], key.r[3]);
            __syncthreads();  // (A) this round's keys
            // what the lane is: 0 nothing; 1 a new entry that owns a table slot; 2 a new entry outside the table (a full table:
            // cannot happen below the budget's bound); 3 equal to the entry `ref` of an earlier round; 4 equal to the new entry of
            // lane `ref`
            int state = 0;
            int32_t ref = 0;
            u32 my_slot = 0;
            if (exists) {
                state = 2;
                u32 h = ntb_hash(key);
#pragma unroll 1
                for (int probe = 0; probe < NTB_TABLE_SLOTS; ++probe) {
                    int32_t seen = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (seen == NTF_EMPTY) {
                        seen = atomicCAS(&table[h], NTF_EMPTY, (int32_t)(0x80000000u | tid));
                        if (seen == NTF_EMPTY) {
                            state = 1;
                            my_slot = h;
                            break;
                        }
                    }
                    Board other;
                    bool known = true;
                    if (seen < 0) {
                        const uint4 o = round_key[seen & 0xFFFF];
                        other.r[0] = o.x; other.r[1] = o.y; other.r[2] = o.z; other.r[3] = o.w;
                    } else if (seen < cap_out) {
                        other = load_board(list_out, seen);
                    } else {
                        known = false;
                    }
                    if (known && !nts_differs(other, key)) {
                        state = seen < 0 ? 4 : 3;
                        ref = seen < 0 ? (seen & 0xFFFF) : seen;
                        break;
                    }
                    h = h + 1 == NTB_TABLE_SLOTS ? 0 : h + 1;
                }
            }
            int32_t rank = 0;
            if (state == 1 || state == 2) rank = atomicAdd(&s_round_n, 1);
            __syncthreads();  // (B) the round's new entries are counted
            const int32_t base = count;
            count += s_round_n;
            int32_t idx = ref;
            if (state == 1 || state == 2) {
                idx = base + rank;
                if (idx >= 0 && idx < cap_out) store_board(list_out, idx, key);  // a region holds the budget and one round: always true
                if (state == 1) table[my_slot] = idx;
                round_idx[tid] = idx;
            }
            __syncthreads();  // (C) this round's entries are in the list and their indices in LDS; everyone has read s_round_n
            if (state == 4) idx = round_idx[ref];
            if (exists) link_out[(parent << shift) + slot] = idx;
            if (tid == 0) s_round_n = 0;  // added to again only after (A) of the next round
            if (count > budget) break;    // uniform: the level does not fit
        }
        if (count > budget) {
            depth_used = level - 1;  // level 1 holds at most 4 <= budget entries: at least 1
            break;
        }
        if (tid == 0) meta[level] = count;
        parents = list_out;
        link_out = ntb_link(ws, w, level, b);  // read by the backup pass only if level < depth
        n_parents = count;
        shift = 7;
    }
    if (tid == 0) {
        meta[0] = depth_used;
        for (int level = depth_used + 1; level < NTB_META; ++level) meta[level] = 0;
    }
}

template <int M, bool STAGED>
__global__ void __launch_bounds__(kBlock) k_ntb_leaf(uint8_t *ws, const NtbLayout w, int iters, const int32_t *weights, const NtNet net_arg,
                                                     float scale) {
    const NtNet net = nt_kernel_net<STAGED>(net_arg);
    __shared__ float v[kLeafEntries][32];
    const int64_t b = blockIdx.x;
    const int32_t *meta = ntb_meta(ws, w, b);
    const int level = ntb_depth_used(meta, w.depth);
    const int32_t count = ntb_count(meta, level, w.cap[level]);
    const uint8_t *list = ntb_list(ws, w, level, b);
    float *e_out = ntb_e(ws, w, level, b);
    const u32 tid = threadIdx.x, g = tid / kLeafLanes, quad = (tid % kLeafLanes) >> 2, a = tid & 3u;
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
        const int32_t e0 = (it * (int32_t)gridDim.y + (int32_t)blockIdx.y) * kLeafEntries;
        if (e0 >= count) break;  // uniform
        const int32_t e = e0 + (int32_t)g;
        const bool live = e < count;
        Board x;
        x.r[0] = x.r[1] = x.r[2] = x.r[3] = 0x01010101u;  // a dead lane group: no empty cell, no child
        if (live) x = load_board(list, e);
        const u32 mask = ntf_empty_mask(x), n2 = 2u * popc(mask);
#pragma unroll 1
        for (u32 k = quad; k < 32u; k += kLeafLanes / 4) {
            if (!__builtin_amdgcn_ballot_w64(k < n2)) break;  // wave-uniform: the quads below stay whole
            bool legal = false;
            float q = 0.0f;
            if (k < n2) q = ntf_leaf_lane<M>(weights, net, scale, x, mask, k, a, legal);
            const float v0 = quad_best(q, legal);
            if (a == 0 && k < n2) v[g][k] = v0;
        }
        __syncthreads();
        if (live && (tid % kLeafLanes) == 0) e_out[e] = ntf_expect_ranked(v[g], n2 >> 1);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kBlock) k_ntb_backup(uint8_t *ws, const NtbLayout w, int level, int iters, float gamma) {
    __shared__ __align__(8) float v[kBackupEntries][32];
    const int64_t b = blockIdx.x;
    const int32_t *meta = ntb_meta(ws, w, b);
    if (ntb_depth_used(meta, w.depth) <= level) return;  // uniform: this root's search ends at or above the level
    const int32_t count = ntb_count(meta, level, w.cap[level]), cap_next = w.cap[level + 1];
    const uint8_t *list = ntb_list(ws, w, level, b);
    const int32_t *link = ntb_link(ws, w, level, b);
    const float *e_next = ntb_e(ws, w, level + 1, b);
    float *e_out = ntb_e(ws, w, level, b);
    const u32 tid = threadIdx.x, g = tid / NTF_LINKS, slot = tid % NTF_LINKS;
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
        const int32_t e0 = (it * (int32_t)gridDim.y + (int32_t)blockIdx.y) * kBackupEntries;
        if (e0 >= count) break;  // uniform
        const int32_t e = e0 + (int32_t)g;
        const bool live = e < count;
        Board x;
        x.r[0] = x.r[1] = x.r[2] = x.r[3] = 0x01010101u;
        bool legal = false;
        float q = 0.0f;
        if (live) {
            x = load_board(list, e);
            q = ntf_backup_lane(x, slot, link + (int64_t)e * NTF_LINKS, e_next, cap_next, gamma, legal);
        }
        const float v1 = quad_best(q, legal);
        if ((slot & 3u) == 0) v[g][slot >> 2] = v1;
        __syncthreads();
        if (live && slot == 0) e_out[e] = ntf_expect_cells(v[g], ntf_empty_mask(x));
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kBlock) k_ntb_roots(const uint8_t *boards, int64_t B, uint8_t *ws, const NtbLayout w, float gamma,
                                                      float *scores, float *values, uint8_t *depth_used, int32_t *entries) {
    // every lane stays to the end: the quad moves want whole quads
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool in_range = i < 4 * B;
    const int64_t b = in_range ? i >> 2 : 0;
    const u32 a = (u32)i & 3u;
    bool legal = false;
    float q = 0.0f;
    if (in_range) q = ntf_root_lane(load_board(boards, b), a, ntb_root_link(ws, w, b), ntb_e(ws, w, 1, b), w.cap[1], gamma, legal);
    const float v = quad_best(q, legal);
    if (!in_range) return;
    scores[i] = q;
    if (a == 0) values[b] = v;
    const int32_t *meta = ntb_meta(ws, w, b);
    const int d = ntb_depth_used(meta, w.depth);
    if (a == 0 && depth_used) depth_used[b] = (uint8_t)d;
    if (entries) {  // lane a writes levels a + 1 and a + 5
        for (int level = (int)a + 1; level <= NTB_MAX_DEPTH; level += 4)
            entries[b * NTB_MAX_DEPTH + level - 1] = level <= d ? ntb_count(meta, level, w.cap[level]) : 0;
    }
}

inline bool aligned4(const void *p) { return !((uintptr_t)p & 3); }

// workgroups per root for a pass over at most `cap` entries, `per_block` of them per iteration, and the iterations of each
inline unsigned slices_for(int32_t cap, int per_block, int &iters) {
    const int blocks = (cap + per_block - 1) / per_block;
    const int slices = blocks < kMaxSlices ? blocks : kMaxSlices;
    iters = (blocks + slices - 1) / slices;
    return (unsigned)slices;
}

}  // namespace

#define G2048_NTB_LAUNCH_M(STAGED, m, grid, stream, ...) \
    switch (m) { \
        case 1: hipLaunchKernelGGL((k_ntb_leaf<1, STAGED>), grid, dim3(kBlock), 0, stream, __VA_ARGS__); break; \
        case 2: hipLaunchKernelGGL((k_ntb_leaf<2, STAGED>), grid, dim3(kBlock), 0, stream, __VA_ARGS__); break; \
        case 3: hipLaunchKernelGGL((k_ntb_leaf<3, STAGED>), grid, dim3(kBlock), 0, stream, __VA_ARGS__); break; \
        case 4: hipLaunchKernelGGL((k_ntb_leaf<4, STAGED>), grid, dim3(kBlock), 0, stream, __VA_ARGS__); break; \
        case 5: hipLaunchKernelGGL((k_ntb_leaf<5, STAGED>), grid, dim3(kBlock), 0, stream, __VA_ARGS__); break; \
        case 6: hipLaunchKernelGGL((k_ntb_leaf<6, STAGED>), grid, dim3(kBlock), 0, stream, __VA_ARGS__); break; \
        case 7: hipLaunchKernelGGL((k_ntb_leaf<7, STAGED>), grid, dim3(kBlock), 0, stream, __VA_ARGS__); break; \
        default: hipLaunchKernelGGL((k_ntb_leaf<8, STAGED>), grid, dim3(kBlock), 0, stream, __VA_ARGS__); break; \
    }

extern "C" {

int64_t g2048_ntuple_budget_search_workspace_bytes(int64_t B, int max_depth, int budget) {
    if (!ntb_settings_ok(max_depth, budget) || B < 1 || B > ntb_max_roots(max_depth, budget)) return -1;
    return ntb_layout(B, max_depth, budget).bytes;
}

int g2048_ntuple_staged_budget_search(const uint8_t *boards, int64_t B, const int32_t *weights, const uint8_t *tuple_cells, int m, int L,
                                      const uint8_t *stage_tiles, int n_stages, int frac_bits, int max_depth, int budget, double gamma,
                                      void *workspace, int64_t workspace_bytes, float *scores, float *values, uint8_t *depth_used,
                                      int32_t *entries, void *stream) {
    NtNet net;
    const int64_t need = g2048_ntuple_budget_search_workspace_bytes(B, max_depth, budget);
    if (!boards || !weights || !workspace || !scores || !values || need < 0 || workspace_bytes < need ||
        !nt_read_staged(tuple_cells, m, L, stage_tiles, n_stages, net) || !nt_frac_ok(frac_bits) || !(gamma >= 0.0) || !isfinite(gamma))
        return G2048_EINVAL;
    if (!aligned16(boards, workspace) || !aligned4(weights) || !aligned4(scores) || !aligned4(values) || !aligned4(entries))
        return G2048_EINVAL;
    const NtbLayout w = ntb_layout(B, max_depth, budget);
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    hipStream_t s = (hipStream_t)stream;
    const float g = (float)gamma;

    hipLaunchKernelGGL(k_ntb_build, dim3((unsigned)B), dim3(NTB_BLOCK), 0, s, boards, ws, w);
    int iters;
    unsigned slices = slices_for(w.cap[max_depth], kLeafEntries, iters);  // the largest region a root's last level can be in
    const float scale = nt_scale(frac_bits);
    if (net.n_stage_tiles) {
        G2048_NTB_LAUNCH_M(true, m, dim3((unsigned)B, slices), s, ws, w, iters, weights, net, scale)
    } else {
        G2048_NTB_LAUNCH_M(false, m, dim3((unsigned)B, slices), s, ws, w, iters, weights, net, scale)
    }
    for (int j = max_depth - 1; j >= 1; --j) {
        slices = slices_for(w.cap[j], kBackupEntries, iters);
        hipLaunchKernelGGL(k_ntb_backup, dim3((unsigned)B, slices), dim3(kBlock), 0, s, ws, w, j, iters, g);
    }
    hipLaunchKernelGGL(k_ntb_roots, dim3((unsigned)((4 * B + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, boards, B, ws, w, g, scores, values,
                       depth_used, entries);
    return launch_status();
}

// the unstaged entry point: one stage, no thresholds
int g2048_ntuple_budget_search(const uint8_t *boards, int64_t B, const int32_t *weights, const uint8_t *tuple_cells, int m, int L,
                               int frac_bits, int max_depth, int budget, double gamma, void *workspace, int64_t workspace_bytes,
                               float *scores, float *values, uint8_t *depth_used, int32_t *entries, void *stream) {
    return g2048_ntuple_staged_budget_search(boards, B, weights, tuple_cells, m, L, nullptr, 1, frac_bits, max_depth, budget, gamma,
                                             workspace, workspace_bytes, scores, values, depth_used, entries, stream);
}

}  // extern "C"
