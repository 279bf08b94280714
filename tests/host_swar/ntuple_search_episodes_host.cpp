// Host build of 2048-ppo-agent_amd/csrc/g2048_ntuple_search_episodes.h (G2048_HOST_TEST) for CPU-side logic tests.
// Test infrastructure only: runs the wave of k_nt_search_episodes (g2048_ntuple_search_episodes.hip) game by game, the 64 lanes in
// sequence per phase: the existence pass with the two ballots as loops, the packed list, the leaf rounds with the quad's max in the
// kernel's two rounds (lane ^ 1, then lane ^ 2), the four reducing lanes and their argmax rounds, then nte_step; n_steps per call
// with the state carried in the caller's arrays between calls as on the device, so that tests/ can compare it with the numpy
// restatement (tests/ntuple_search_episodes_ref.py) without a GPU.  The product never builds or loads this.
// With NTUPLE_SEARCH_EPISODES_HOST_MAIN it is a stand-alone program (for a sanitizer build): exactly sized arrays, one call against many.
#define G2048_HOST_TEST 1
#include "g2048_ntuple_search_episodes.h"
using namespace g2048;

namespace {

// the two rounds of the kernel's quad max over the legal lanes of every quad of the wave; +0 where a quad has none
void wave_quad_best(const float q[NTSE_WAVE], const bool legal[NTSE_WAVE], float out[NTSE_WAVE]) {
    float x[NTSE_WAVE], y[NTSE_WAVE];
    for (u32 k = 0; k < NTSE_WAVE; ++k) x[k] = legal[k] ? q[k] : nt_neg_inf();
    for (u32 bit = 1; bit <= 2; bit <<= 1) {
        for (u32 k = 0; k < NTSE_WAVE; ++k) y[k] = nt_vmax(x[k], x[k ^ bit]);
        for (u32 k = 0; k < NTSE_WAVE; ++k) x[k] = y[k];
    }
    for (u32 k = 0; k < NTSE_WAVE; ++k) out[k] = x[k] == nt_neg_inf() ? 0.0f : x[k];
}

// the two rounds of the kernel's quad argmax on lanes 0 .. 3; every lane ends with the same pair
u32 quad_argmax(const float l[4]) {
    float x[4], y[4];
    u32 a[4], b[4];
    for (u32 k = 0; k < 4; ++k) { x[k] = l[k]; a[k] = k; }
    for (u32 bit = 1; bit <= 2; bit <<= 1) {
        for (u32 k = 0; k < 4; ++k) {
            const u32 o = k ^ bit;
            const bool take = nte_beats(x[o], a[o], x[k], a[k]);
            y[k] = take ? x[o] : x[k];
            b[k] = take ? a[o] : a[k];
        }
        for (u32 k = 0; k < 4; ++k) { x[k] = y[k]; a[k] = b[k]; }
    }
    return a[0];
}

// one step's move choice, phase by phase.  list and leaf are the workgroup's LDS: they keep what earlier steps left in them.
template <int M>
u32 choose(const int32_t *w, const NtNet &net, float scale, float gamma, const NteGame &G, uint8_t list[NTS_SLOTS], float leaf[NTS_SLOTS]) {
    uint64_t lo = 0, hi = 0;  // 1 existence: the two ballots
    for (u32 lane = 0; lane < NTSE_WAVE; ++lane) {
        Board child;
        if (nts_child(G.bd, lane, child)) lo |= (uint64_t)1 << lane;
        if (nts_child(G.bd, lane + NTSE_WAVE, child)) hi |= (uint64_t)1 << lane;
    }
    const u32 n_live = ntse_popc64(lo) + ntse_popc64(hi);
    for (u32 lane = 0; lane < NTSE_WAVE; ++lane) {
        if ((lo >> lane) & 1u) list[ntse_rank(lo, hi, lane)] = (uint8_t)lane;
        if ((hi >> lane) & 1u) list[ntse_rank(lo, hi, lane + NTSE_WAVE)] = (uint8_t)(lane + NTSE_WAVE);
    }
    for (u32 round = 0; round < ntse_rounds(n_live); ++round) {  // 2 leaf
        float q[NTSE_WAVE], v0[NTSE_WAVE];
        bool legal[NTSE_WAVE];
        u32 slot[NTSE_WAVE];
        for (u32 lane = 0; lane < NTSE_WAVE; ++lane)
            q[lane] = ntse_leaf_pair<M>(w, net, scale, G.bd, list, n_live, round * NTSE_WAVE + lane, slot[lane], legal[lane]);
        wave_quad_best(q, legal, v0);
        for (u32 lane = 0; lane < NTSE_WAVE; lane += 4)
            if (((round * NTSE_WAVE + lane) >> 2) < n_live) leaf[slot[lane]] = v0[lane];
    }
    float l[4];  // 3 choose
    for (u32 a = 0; a < 4; ++a) {
        bool legal;
        l[a] = ntse_logit(nts_reduce_lane(G.bd, a, leaf, gamma, legal), G.mask, a);
    }
    return quad_argmax(l);
}

template <int MODE, int M>
int64_t episodes(int start, int n_steps, u32 N, u32 bs, const int32_t *w, const NtNet &net, float scale, float gamma, uint32_t *chain,
                 uint8_t *boards, uint8_t *masks, uint8_t *done, int32_t *ep_len, int64_t *score) {
    int64_t live = 0;
    for (u32 i = 0; i < N; ++i) {
        NteGame G;
        u32 g, B_total;
        nte_place(i, N, bs, g, B_total);
        if (start) {
            nte_seed<MODE>(G, chain[2 * i], chain[2 * i + 1], B_total, g);
        } else {
            memcpy(G.bd.r, boards + 16 * (size_t)i, 16);
            G.mask = masks[i];
            G.done = done[i];
            G.len = (u32)ep_len[i];
            G.score = score[i];
            G.c0 = chain[2 * i];
            G.c1 = chain[2 * i + 1];
        }
        uint8_t list[NTS_SLOTS];
        alignas(8) float leaf[NTS_SLOTS];
        memset(list, 0xEE, sizeof(list));  // what a launch finds in LDS is arbitrary: a value that is no slot ...
        for (float &x : leaf) x = nt_neg_inf();  // ... and one that would wreck any sum it entered
        for (int s = 0; s < n_steps && !G.done; ++s) nte_step<MODE>(G, choose<M>(w, net, scale, gamma, G, list, leaf), B_total, g);
        chain[2 * i] = G.c0;
        chain[2 * i + 1] = G.c1;
        memcpy(boards + 16 * (size_t)i, G.bd.r, 16);
        masks[i] = (uint8_t)G.mask;
        done[i] = (uint8_t)G.done;
        ep_len[i] = (int32_t)G.len;
        score[i] = G.score;
        live += G.done == 0;
    }
    return live;
}

}  // namespace

#define NTSE_SWITCH(MODE, m, ...)                                 \
    switch (m) {                                                  \
        case 1: return episodes<MODE, 1>(__VA_ARGS__);            \
        case 2: return episodes<MODE, 2>(__VA_ARGS__);            \
        case 3: return episodes<MODE, 3>(__VA_ARGS__);            \
        case 4: return episodes<MODE, 4>(__VA_ARGS__);            \
        case 5: return episodes<MODE, 5>(__VA_ARGS__);            \
        case 6: return episodes<MODE, 6>(__VA_ARGS__);            \
        case 7: return episodes<MODE, 7>(__VA_ARGS__);            \
        default: return episodes<MODE, 8>(__VA_ARGS__);           \
    }

extern "C" {
// the arguments of g2048_ntuple_staged_search_episodes without plies, live_count and stream -> the games still running afterwards,
// or -1 where the entry point's reader refuses the network
int64_t hst_nt_search_episodes(int start, int n_steps, int64_t N, int64_t bs, const int32_t *w, const uint8_t *cells, int m, int L,
                               const uint8_t *stage_tiles, int n_stages, int frac_bits, float gamma, uint32_t *chain, uint8_t *boards,
                               uint8_t *masks, uint8_t *done, int32_t *ep_len, int64_t *score, int rng_mode) {
    NtNet net;
    if (!nt_read_staged(cells, m, L, stage_tiles, n_stages, net) || !nt_frac_ok(frac_bits) || N < 1 || bs < 1 || n_steps < 1) return -1;
    const float scale = nt_scale(frac_bits);
    if (rng_mode) {
        NTSE_SWITCH(RNG_PARTITIONABLE, m, start, n_steps, (u32)N, (u32)bs, w, net, scale, gamma, chain, boards, masks, done, ep_len, score)
    } else {
        NTSE_SWITCH(RNG_LEGACY, m, start, n_steps, (u32)N, (u32)bs, w, net, scale, gamma, chain, boards, masks, done, ep_len, score)
    }
}
}

#ifdef NTUPLE_SEARCH_EPISODES_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <vector>

namespace {

struct State {
    std::vector<uint32_t> chain;
    std::vector<uint8_t> boards, masks, done;
    std::vector<int32_t> len;
    std::vector<int64_t> score;
    State(int64_t N, int64_t bs, uint32_t seed) : chain(2 * N), boards(16 * N, 0xEE), masks(N, 0xEE), done(N, 0xEE), len(N, -7), score(N, -7) {
        for (int64_t i = 0; i < N; ++i) {
            chain[2 * i] = 0;
            chain[2 * i + 1] = seed + (uint32_t)((i / bs) * bs);
        }
    }
    bool operator==(const State &o) const {
        return chain == o.chain && boards == o.boards && masks == o.masks && done == o.done && len == o.len && score == o.score;
    }
};

int64_t play(State &s, int start, int n_steps, int64_t N, int64_t bs, const int32_t *w, const uint8_t *cells, int m, int L,
             const uint8_t *tiles, int n_stages, int F, float gamma, int mode) {
    return hst_nt_search_episodes(start, n_steps, N, bs, w, cells, m, L, tiles, n_stages, F, gamma, s.chain.data(), s.boards.data(),
                                  s.masks.data(), s.done.data(), s.len.data(), s.score.data(), mode);
}

}  // namespace

// 17 games in batches of 7 (a short last batch) on a three-stage network with exactly sized arrays, both RNG modes: the games played
// in one call equal the games played 5 steps per call, a call on the finished state changes nothing, and with every weight at
// INT32_MIN (frac_bits 0) some game ends by an illegal move (reward -1).  Under -fsanitize=address,undefined an access outside a
// table, the list, the leaf array or a state array aborts the run.
int main() {
    const int m = 3, L = 2;
    const uint8_t cells[m * L] = {0, 1, 5, 6, 3, 15};
    const uint8_t tiles[2] = {3, 5};
    const int64_t E = (int64_t)3 * m << (4 * L), N = 17, bs = 7;
    std::vector<int32_t> w(E);
    uint32_t r = 12345u;
    for (auto &x : w) x = (int32_t)((r = r * 1664525u + 1013904223u) >> 11) - (1 << 20);
    for (int mode = 0; mode < 2; ++mode) {
        State one(N, bs, 42), many(N, bs, 42);
        if (play(one, 1, 65536, N, bs, w.data(), cells, m, L, tiles, 3, 12, 0.99f, mode) != 0) return 2;
        int calls = 0;
        int64_t live = play(many, 1, 5, N, bs, w.data(), cells, m, L, tiles, 3, 12, 0.99f, mode);
        while (live > 0 && ++calls < 100000) live = play(many, 0, 5, N, bs, w.data(), cells, m, L, tiles, 3, 12, 0.99f, mode);
        if (live != 0 || !(one == many)) return 3;
        if (play(many, 0, 9, N, bs, w.data(), cells, m, L, tiles, 3, 12, 0.99f, mode) != 0 || !(one == many)) return 4;
        for (int64_t i = 0; i < N; ++i)
            if (!one.done[i] || one.len[i] < 1) return 5;
        std::vector<int32_t> low((int64_t)m << (4 * L), (int32_t)(-2147483647 - 1));
        State edge(N, bs, 42);
        if (play(edge, 1, 65536, N, bs, low.data(), cells, m, L, nullptr, 1, 0, 1.0f, mode) != 0) return 6;
        int illegal = 0;
        for (int64_t i = 0; i < N; ++i) illegal += edge.score[i] < 0;  // (a merge is worth at least 4: a negative score is the -1 of an illegal move)
        if (!illegal) return 7;
    }
    printf("ntuple_search_episodes_host ok\n");
    return 0;
}
#endif
