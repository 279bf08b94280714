// Host build of 2048-ppo-agent_amd/csrc/g2048_ntuple_search.h (G2048_HOST_TEST) for CPU-side logic tests.
// Test infrastructure only: runs the lane code of k_nt_q1 and k_nt_backup (g2048_ntuple_search.hip) sequentially, slot by slot, so
// that tests/ can compare it with the composed numpy restatements without a GPU.  The product never builds or loads this.
// With NTUPLE_SEARCH_HOST_MAIN it is a stand-alone program (for a sanitizer build): a small fixed case, checked for NaN.
#define G2048_HOST_TEST 1
#include "g2048_ntuple_search.h"
using namespace g2048;

namespace {

NtNet make_net(const uint8_t *cells, int m, int L) {
    NtNet net;
    memset(&net, 0, sizeof(net));
    net.L = L;
    for (int t = 0; t < m; ++t)
        for (int j = 0; j < L; ++j) net.cell[t][j] = cells[t * L + j];
    return net;
}

Board get(const uint8_t *p, int64_t i) {
    Board b;
    memcpy(b.r, p + 16 * i, 16);
    return b;
}

// the max over the legal lanes of a quad, +0 if there is none
float quad_best(const float q[4], const bool legal[4]) {
    float x = nt_neg_inf();
    for (int a = 0; a < 4; ++a) x = nt_vmax(x, legal[a] ? q[a] : nt_neg_inf());
    return x == nt_neg_inf() ? 0.0f : x;
}

// one block of k_nt_q1 on position pos: q[4] and the return value v
template <int M>
float q1(const Board &pos, const int32_t *w, const NtNet &net, float scale, float gamma, float q[4]) {
    alignas(8) float leaf[NTS_SLOTS];
    bool legal[4];
    for (u32 slot = 0; slot < NTS_SLOTS; ++slot) {  // the quads of the two rounds
        float x[4];
        for (u32 a = 0; a < 4; ++a) x[a] = nts_leaf_lane<M>(w, net, scale, pos, slot, a, legal[a]);
        leaf[slot] = quad_best(x, legal);
    }
    for (u32 a = 0; a < 4; ++a) q[a] = nts_reduce_lane(pos, a, leaf, gamma, legal[a]);  // the four lanes after the barrier
    return quad_best(q, legal);
}

template <int M>
void expectimax(const uint8_t *boards, int64_t B, const int32_t *w, const NtNet &net, float scale, int plies, float gamma,
                float *workspace, float *q, float *v) {
    for (int64_t b = 0; b < B; ++b) {
        const Board root = get(boards, b);
        if (plies == 1) {
            v[b] = q1<M>(root, w, net, scale, gamma, q + 4 * b);
            continue;
        }
        for (u32 slot = 0; slot < NTS_SLOTS; ++slot) {  // the blocks of root b
            Board pos;
            float q_pos[4];
            if (nts_child(root, slot, pos)) workspace[b * NTS_SLOTS + slot] = q1<M>(pos, w, net, scale, gamma, q_pos);
        }
        bool legal[4];
        for (u32 a = 0; a < 4; ++a) q[4 * b + a] = nts_reduce_lane(root, a, workspace + b * NTS_SLOTS, gamma, legal[a]);  // k_nt_backup
        v[b] = quad_best(q + 4 * b, legal);
    }
}

}  // namespace

#define NTS_SWITCH(FN, m, ...)             \
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
// workspace f32[128 B] (8-byte aligned; unused for plies == 1), q f32[B][4], v f32[B]
void hst_nt_expectimax(const uint8_t *boards, int64_t B, const int32_t *w, const uint8_t *cells, int m, int L, int frac_bits, int plies,
                       double gamma, float *workspace, float *q, float *v) {
    const NtNet net = make_net(cells, m, L);
    NTS_SWITCH(expectimax, m, boards, B, w, net, nt_scale(frac_bits), plies, (float)gamma, workspace, q, v);
}
}

#ifdef NTUPLE_SEARCH_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <vector>

// both depths on boards that include the one-tile board (120 children), a full board without a move and tiles 16 and 17, from a
// NaN-filled workspace; exits non-zero if an output is NaN.  Under -fsanitize=address,undefined an access outside a table, the
// leaf array or the workspace aborts the run.
int main() {
    const int m = 3, L = 2, F = 12;
    const uint8_t cells[m * L] = {0, 1, 5, 6, 3, 15};
    const int64_t E = (int64_t)m << (4 * L), B = 8;
    std::vector<int32_t> w(E);
    std::vector<uint8_t> boards(16 * B, 0);
    uint32_t s = 12345u;
    auto rnd = [&]() { return s = s * 1664525u + 1013904223u; };
    for (auto &x : w) x = (int32_t)(rnd() >> 11) - (1 << 20);
    boards[16 * 0 + 5] = 1;                                                                     // one tile: 120 children
    for (int c = 0; c < 16; ++c) boards[16 * 1 + c] = (uint8_t)(1 + ((c + (c >> 2)) & 1));      // full, no move
    for (int c = 0; c < 16; ++c) boards[16 * 2 + c] = (uint8_t)(c & 1 ? 0 : 16 + ((c >> 1) & 1));  // tiles 16 and 17
    for (int64_t b = 3; b < B; ++b)
        for (int c = 0; c < 16; ++c) boards[16 * b + c] = (uint8_t)(rnd() >> 29);
    for (int plies = 1; plies <= 2; ++plies) {
        std::vector<float> ws(NTS_SLOTS * B, nanf("")), q(4 * B, nanf("")), v(B, nanf(""));
        hst_nt_expectimax(boards.data(), B, w.data(), cells, m, L, F, plies, 0.99, ws.data(), q.data(), v.data());
        for (float x : q)
            if (!(x == x)) return 2;
        for (float x : v)
            if (!(x == x)) return 3;
        if (q[4] != 0.0f || q[5] != 0.0f || q[6] != 0.0f || q[7] != 0.0f || v[1] != 0.0f) return 4;  // the board without a move
    }
    printf("ntuple_search_host ok\n");
    return 0;
}
#endif
