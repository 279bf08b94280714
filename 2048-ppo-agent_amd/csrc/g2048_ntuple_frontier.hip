// N-tuple frontier search (include/g2048.h, "n-tuple frontier search"): 1 .. 3 plies of expectimax over the n-tuple network on packed
// lists of afterstates, the equal afterstates of one root merged at every level.
//
//   init    the level counters to 0 (one wave).
//   expand  A_j -> A_{j+1} (j = 0: the roots -> A_1), one workgroup of 512 lanes per root.  A round gives every lane one link slot
//           of one parent; a lane whose slot exists builds the afterstate in registers and looks it up in the workgroup's table
//           of entry indices in LDS (open addressing, linear probing, claimed with a 32-bit LDS compare-and-swap).  A lane that
//           meets a claimed slot compares its 16 bytes with the owner's: the owner of this round keeps its board in LDS, the owner
//           of an earlier round has written it to the list (same workgroup, a barrier in between).  The lanes that claimed a
//           slot are ranked with an LDS add, ONE lane takes list space for all of them from the level's counter with one
//           integer atomic add, and they append their boards; every existing slot then gets its link.  Levels 1 and 2 are built
//           in one round, so a root's entries there are one contiguous segment, written down for the next expand.  A table that
//           holds NTF_TABLE_CAP entries takes no more: later rounds still find what is in it and append the rest unmerged.
//   leaf    E_1 of every entry of A_depth: 16 lanes per entry, a quad per (empty cell by rank, tile), a lane per action; 8 m
//           gathers per legal lane, the quad's max to LDS, one serial ascending pass per entry.
//   backup  E_j of every entry of A_j, j < depth: 128 lanes per entry, one per link slot, the quad's max to LDS, one serial pass.
//   roots   one lane per (root, action): Q and V; lane 0 also copies the counters to `counts`.
//
// Grids are fixed at launch from B and the capacities; the kernels walk the device-side counts with grid-stride loops whose trip
// counts are kernel arguments, and clamp every count and link they read to the capacity of the array it indexes.  No host read, no
// device-side allocation, no synchronisation, no float atomics, no scratch; the order of a list depends on scheduling, no value does.
// The per-lane code is g2048_ntuple_frontier.h, shared with the host build the CPU tests compare against the numpy composition.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/g2048.h"
#include "g2048_device.h"
#include "g2048_host.h"
#include "g2048_ntuple_frontier.h"

using namespace g2048;
using namespace g2048_host;

namespace {

constexpr int kBlock = 256;          // leaf, backup, roots
constexpr int kLeafLanes = 16;       // lanes per entry of the leaf pass
constexpr int kLeafEntries = kBlock / kLeafLanes;
constexpr int kBackupEntries = kBlock / NTF_LINKS;
constexpr int64_t kMaxGrid = 1 << 16;  // blocks of a grid-stride kernel

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

__device__ __forceinline__ int32_t clamped_count(const int32_t *counter, int32_t cap) { return ntf_clamp_i32(*counter, 0, cap); }

__global__ void k_ntf_init(int32_t *counters) {
    if (threadIdx.x < 4) counters[threadIdx.x] = 0;
}

// parents: the roots (seg_in == nullptr: one parent per workgroup, 4 link slots) or the list of level j (seg_in[2 b], seg_in[2 b + 1] =
// the root's first entry and entries there, at most seg_cap of them; 128 link slots each).  cap_in / cap_out: entries of the lists.
__global__ void __launch_bounds__(NTF_BLOCK) k_ntf_expand(const uint8_t *parents, const int32_t *seg_in, int32_t seg_cap, int32_t cap_in,
                                                          int max_rounds, int dedup, int32_t *counter, int32_t cap_out,
                                                          uint8_t *list_out, int32_t *link_out, int32_t *seg_out) {
    __shared__ int32_t table[NTF_TABLE_SLOTS];
    __shared__ uint4 round_key[NTF_BLOCK];
    __shared__ int32_t round_idx[NTF_BLOCK];
    __shared__ int32_t s_round_n, s_table_n, s_base;
    const u32 tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (dedup)
        for (u32 i = tid; i < NTF_TABLE_SLOTS; i += NTF_BLOCK) table[i] = NTF_EMPTY;
    if (tid == 0) {
        s_round_n = 0;
        s_table_n = 0;
    }
    int32_t first = (int32_t)b, n_parents = 1;
    u32 shift = 2;  // log2 of the link slots per parent
    if (seg_in) {
        n_parents = ntf_clamp_i32(seg_in[2 * b + 1], 0, seg_cap);
        first = ntf_clamp_i32(seg_in[2 * b], 0, cap_in - n_parents);
        shift = 7;
    }
    const u32 n_cand = (u32)n_parents << shift;
    __syncthreads();
#pragma unroll 1
    for (int round = 0; round < max_rounds; ++round) {
        if ((u32)round * NTF_BLOCK >= n_cand) break;  // uniform, before the round's barriers
        const u32 cand = (u32)round * NTF_BLOCK + tid;
        const bool may_insert = s_table_n < NTF_TABLE_CAP;  // uniform: written before the last barrier of the round before
        const int64_t parent = first + (int64_t)(cand >> shift);
        const u32 slot = cand & ((1u << shift) - 1u);
        Board key;
        key.r[0] = key.r[1] = key.r[2] = key.r[3] = 0;
        bool exists = false;
        if (cand < n_cand) {
            u32 reward;
            const Board x = load_board(parents, parent);
            exists = seg_in ? ntf_candidate(x, slot, key, reward) : ntf_root_candidate(x, slot, key, reward);
        }
        round_key[tid] = make_uint4(key.r[0], key.r[1], key.r[2], key.r[3]);
        __syncthreads();  // (A) this round's keys
        // what the lane is: 0 nothing; 1 a new entry that owns a table slot; 2 a new entry outside the table; 3 equal to the entry
        // `ref` of an earlier round; 4 equal to the new entry of lane `ref`
        int state = 0;
        int32_t ref = 0;
        u32 my_slot = 0;
        if (exists) {
            state = 2;
            if (dedup) {
                u32 h = ntf_hash(key);
#pragma unroll 1
                for (int probe = 0; probe < NTF_TABLE_SLOTS; ++probe) {
                    int32_t seen = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (seen == NTF_EMPTY) {
                        if (!may_insert) break;
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
                    h = h + 1 == NTF_TABLE_SLOTS ? 0 : h + 1;
                }
            }
        }
        int32_t rank = 0;
        if (state == 1 || state == 2) rank = atomicAdd(&s_round_n, 1);
        if (state == 1) atomicAdd(&s_table_n, 1);
        __syncthreads();  // (B) the round's new entries are counted
        if (tid == 0) s_base = s_round_n ? atomicAdd(counter, s_round_n) : 0;  // the one global atomic of the round
        __syncthreads();  // (C)
        int32_t idx = ref;
        if (state == 1 || state == 2) {
            idx = s_base + rank;
            if (idx >= 0 && idx < cap_out) store_board(list_out, idx, key);  // the lists hold the worst case: always true
            if (state == 1) table[my_slot] = idx;
            round_idx[tid] = idx;
        }
        __syncthreads();  // (D) this round's entries are in the list and their indices in LDS
        if (state == 4) idx = round_idx[ref];
        if (exists) link_out[(parent << shift) + slot] = idx;
        if (tid == 0) {
            if (seg_out && round == 0) {
                seg_out[2 * b] = s_base;
                seg_out[2 * b + 1] = s_round_n;
            }
            s_round_n = 0;  // read again only after (A) of the next round
        }
    }
    if (seg_out && n_cand == 0 && tid == 0) {
        seg_out[2 * b] = 0;
        seg_out[2 * b + 1] = 0;
    }
}

template <int M, bool STAGED>
__global__ void __launch_bounds__(kBlock) k_ntf_leaf(const uint8_t *list, const int32_t *counter, int32_t cap, int iters,
                                                     const int32_t *weights, const NtNet net_arg, float scale, float *e_out) {
    const NtNet net = nt_kernel_net<STAGED>(net_arg);
    __shared__ float v[kLeafEntries][32];
    const int32_t count = clamped_count(counter, cap);
    const u32 tid = threadIdx.x, g = tid / kLeafLanes, quad = (tid % kLeafLanes) >> 2, a = tid & 3u;
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
        const int64_t e0 = ((int64_t)it * gridDim.x + blockIdx.x) * kLeafEntries;
        if (e0 >= count) break;  // uniform
        const int64_t e = e0 + g;
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

__global__ void __launch_bounds__(kBlock) k_ntf_backup(const uint8_t *list, const int32_t *counter, int32_t cap, int iters,
                                                       const int32_t *link, const float *e_next, int32_t cap_next, float gamma,
                                                       float *e_out) {
    __shared__ __align__(8) float v[kBackupEntries][32];
    const int32_t count = clamped_count(counter, cap);
    const u32 tid = threadIdx.x, g = tid / NTF_LINKS, slot = tid % NTF_LINKS;
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
        const int64_t e0 = ((int64_t)it * gridDim.x + blockIdx.x) * kBackupEntries;
        if (e0 >= count) break;  // uniform
        const int64_t e = e0 + g;
        const bool live = e < count;
        Board x;
        x.r[0] = x.r[1] = x.r[2] = x.r[3] = 0x01010101u;
        bool legal = false;
        float q = 0.0f;
        if (live) {
            x = load_board(list, e);
            q = ntf_backup_lane(x, slot, link + e * NTF_LINKS, e_next, cap_next, gamma, legal);
        }
        const float v1 = quad_best(q, legal);
        if ((slot & 3u) == 0) v[g][slot >> 2] = v1;
        __syncthreads();
        if (live && slot == 0) e_out[e] = ntf_expect_cells(v[g], ntf_empty_mask(x));
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kBlock) k_ntf_roots(const uint8_t *boards, int64_t B, const int32_t *root_link, const float *e1,
                                                      int32_t cap1, float gamma, const int32_t *counters, int depth, int64_t cap_unit,
                                                      float *scores, float *values, int32_t *counts) {
    // every lane stays to the end: the quad moves want whole quads
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool in_range = i < 4 * B;
    bool legal = false;
    float q = 0.0f;
    if (in_range) q = ntf_root_lane(load_board(boards, i >> 2), (u32)i & 3u, root_link + (i >> 2) * NTF_ROOT_LINKS, e1, cap1, gamma, legal);
    const float v = quad_best(q, legal);
    if (in_range) {
        scores[i] = q;
        if (((u32)i & 3u) == 0) values[i >> 2] = v;
    }
    if (counts && i < NTF_MAX_DEPTH) {
        const int level = (int)i + 1;
        counts[i] = level <= depth ? clamped_count(counters + level, (int32_t)(cap_unit * ntf_level_cap(level))) : 0;
    }
}

inline bool aligned4(const void *p) { return !((uintptr_t)p & 3); }

inline unsigned stride_grid(int64_t cap, int per_block, int &iters) {
    const int64_t blocks = (cap + per_block - 1) / per_block;
    const int64_t grid = blocks < kMaxGrid ? blocks : kMaxGrid;
    iters = (int)((blocks + grid - 1) / grid);
    return (unsigned)grid;
}

}  // namespace

#define G2048_NTF_LAUNCH_M(KERNEL, STAGED, m, grid, stream, ...) \
    switch (m) { \
        case 1: hipLaunchKernelGGL((KERNEL<1, STAGED>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 2: hipLaunchKernelGGL((KERNEL<2, STAGED>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 3: hipLaunchKernelGGL((KERNEL<3, STAGED>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 4: hipLaunchKernelGGL((KERNEL<4, STAGED>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 5: hipLaunchKernelGGL((KERNEL<5, STAGED>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 6: hipLaunchKernelGGL((KERNEL<6, STAGED>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        case 7: hipLaunchKernelGGL((KERNEL<7, STAGED>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
        default: hipLaunchKernelGGL((KERNEL<8, STAGED>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
    }
// `net` is the network the entry point has just read: a single stage launches the kernel without stage work
#define G2048_NTF_LAUNCH(KERNEL, m, grid, stream, ...) \
    if (net.n_stage_tiles) { \
        G2048_NTF_LAUNCH_M(KERNEL, true, m, grid, stream, __VA_ARGS__) \
    } else { \
        G2048_NTF_LAUNCH_M(KERNEL, false, m, grid, stream, __VA_ARGS__) \
    }

extern "C" {

int64_t g2048_ntuple_search_workspace_bytes(int64_t B, int depth) {
    if (depth < 1 || depth > NTF_MAX_DEPTH || B < 1 || B > ntf_max_roots(depth)) return -1;
    return ntf_layout(B, depth).bytes;
}

int g2048_ntuple_staged_search(const uint8_t *boards, int64_t B, const int32_t *weights, const uint8_t *tuple_cells, int m, int L,
                               const uint8_t *stage_tiles, int n_stages, int frac_bits, int depth, double gamma, int dedup,
                               void *workspace, int64_t workspace_bytes, float *scores, float *values, int32_t *counts, void *stream) {
    NtNet net;
    const int64_t need = g2048_ntuple_search_workspace_bytes(B, depth);
    if (!boards || !weights || !workspace || !scores || !values || need < 0 || workspace_bytes < need ||
        !nt_read_staged(tuple_cells, m, L, stage_tiles, n_stages, net) || !nt_frac_ok(frac_bits) || !(gamma >= 0.0) || !isfinite(gamma))
        return G2048_EINVAL;
    if (!aligned16(boards, workspace) || !aligned4(weights) || !aligned4(scores) || !aligned4(values) || !aligned4(counts))
        return G2048_EINVAL;
    const NtfLayout w = ntf_layout(B, depth);
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    int32_t *counters = reinterpret_cast<int32_t *>(ws + w.counters), *root_link = reinterpret_cast<int32_t *>(ws + w.root_link);
    auto list = [&](int j) { return ws + w.list[j]; };
    auto e = [&](int j) { return reinterpret_cast<float *>(ws + w.e[j]); };
    auto link = [&](int j) { return reinterpret_cast<int32_t *>(ws + w.link[j]); };
    auto seg = [&](int j) { return j < depth ? reinterpret_cast<int32_t *>(ws + w.seg[j]) : nullptr; };
    hipStream_t s = (hipStream_t)stream;
    const float g = (float)gamma;

    hipLaunchKernelGGL(k_ntf_init, dim3(1), dim3(64), 0, s, counters);
    hipLaunchKernelGGL(k_ntf_expand, dim3((unsigned)B), dim3(NTF_BLOCK), 0, s, boards, (const int32_t *)nullptr, 1, (int32_t)B, 1, dedup,
                       counters + 1, (int32_t)w.cap[1], list(1), root_link, seg(1));
    for (int j = 1; j < depth; ++j) {
        const int32_t seg_cap = (int32_t)ntf_level_cap(j);
        const int max_rounds = (seg_cap * NTF_LINKS + NTF_BLOCK - 1) / NTF_BLOCK;
        hipLaunchKernelGGL(k_ntf_expand, dim3((unsigned)B), dim3(NTF_BLOCK), 0, s, (const uint8_t *)list(j), (const int32_t *)seg(j),
                           seg_cap, (int32_t)w.cap[j], max_rounds, dedup, counters + j + 1, (int32_t)w.cap[j + 1], list(j + 1), link(j),
                           seg(j + 1));
    }
    int iters;
    unsigned grid = stride_grid(w.cap[depth], kLeafEntries, iters);
    G2048_NTF_LAUNCH(k_ntf_leaf, m, grid, s, (const uint8_t *)list(depth), (const int32_t *)(counters + depth), (int32_t)w.cap[depth],
                     iters, weights, net, nt_scale(frac_bits), e(depth));
    for (int j = depth - 1; j >= 1; --j) {
        grid = stride_grid(w.cap[j], kBackupEntries, iters);
        hipLaunchKernelGGL(k_ntf_backup, dim3(grid), dim3(kBlock), 0, s, (const uint8_t *)list(j), (const int32_t *)(counters + j),
                           (int32_t)w.cap[j], iters, (const int32_t *)link(j), (const float *)e(j + 1), (int32_t)w.cap[j + 1], g, e(j));
    }
    hipLaunchKernelGGL(k_ntf_roots, dim3((unsigned)((4 * B + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, boards, B,
                       (const int32_t *)root_link, (const float *)e(1), (int32_t)w.cap[1], g, (const int32_t *)counters, depth, B, scores,
                       values, counts);
    return launch_status();
}

// the unstaged entry point: one stage, no thresholds
int g2048_ntuple_search(const uint8_t *boards, int64_t B, const int32_t *weights, const uint8_t *tuple_cells, int m, int L, int frac_bits,
                        int depth, double gamma, int dedup, void *workspace, int64_t workspace_bytes, float *scores, float *values,
                        int32_t *counts, void *stream) {
    return g2048_ntuple_staged_search(boards, B, weights, tuple_cells, m, L, nullptr, 1, frac_bits, depth, gamma, dedup, workspace,
                                      workspace_bytes, scores, values, counts, stream);
}

}  // extern "C"
