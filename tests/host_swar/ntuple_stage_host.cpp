// Host build of the multi-stage n-tuple network (2048-ppo-agent_amd/csrc/g2048_ntuple.h, g2048_ntuple_search.h and
// g2048_ntuple_tc.h with G2048_HOST_TEST) for CPU-side logic tests.
// Test infrastructure only: runs the lane code of the values, scores, expectimax, TD(0) and TC kernels sequentially with the stage
// thresholds in NtNet, read by the entry points' own reader (nt_read_staged), so that tests/ can compare all of it with the numpy
// restatement (tests/ntuple_stage_ref.py) without a GPU.  Every function returns 0, or -1 where the reader refuses the network.
// The product never builds or loads this.
// With NTUPLE_STAGE_HOST_MAIN it is a stand-alone program (for a sanitizer build): every operation on an eight-stage network.
#define G2048_HOST_TEST 1
#include "g2048_ntuple_search.h"
#include "g2048_ntuple_tc.h"
using namespace g2048;

namespace {

Board get(const uint8_t *p, int64_t i) {
    Board b;
    memcpy(b.r, p + 16 * i, 16);
    return b;
}

float quad_best(const float q[4], const bool legal[4]) {
    float x = nt_neg_inf();
    for (int a = 0; a < 4; ++a) x = nt_vmax(x, legal[a] ? q[a] : nt_neg_inf());
    return x == nt_neg_inf() ? 0.0f : x;
}

template <int M>
void values(const uint8_t *boards, int64_t n, const int32_t *w, const NtNet &net, float scale, float *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = nt_value(nt_sum<M>(w, net, get(boards, i)), scale);  // the body of k_nt_values
}

template <int M>
void scores(const uint8_t *boards, int64_t B, const int32_t *w, const NtNet &net, float scale, float *q, float *v) {
    for (int64_t b = 0; b < B; ++b) {  // the four lanes of a quad of k_nt_scores
        bool legal[4];
        for (u32 a = 0; a < 4; ++a) q[4 * b + a] = nt_score<M>(w, net, scale, get(boards, b), a, legal[a]);
        v[b] = quad_best(q + 4 * b, legal);
    }
}

// one block of k_nt_q1 on position pos: q[4] and the return value v
template <int M>
float q1(const Board &pos, const int32_t *w, const NtNet &net, float scale, float gamma, float q[4]) {
    alignas(8) float leaf[NTS_SLOTS];
    bool legal[4];
    for (u32 slot = 0; slot < NTS_SLOTS; ++slot) {
        float x[4];
        for (u32 a = 0; a < 4; ++a) x[a] = nts_leaf_lane<M>(w, net, scale, pos, slot, a, legal[a]);
        leaf[slot] = quad_best(x, legal);
    }
    for (u32 a = 0; a < 4; ++a) q[a] = nts_reduce_lane(pos, a, leaf, gamma, legal[a]);
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

template <int M>
void td_accumulate(const uint8_t *prev, const uint8_t *flag, const float *target, int64_t B, const int32_t *w, const NtNet &net,
                   float scale, float c, int64_t *acc, int32_t *cnt, float *td_error) {
    for (int64_t b = 0; b < B; ++b) {  // the body of k_nt_td_accumulate
        float e = 0.0f;
        if (flag[b]) e = nt_td_accumulate_lane<M>(get(prev, b), flag[b], target[b], w, net, scale, c, acc, cnt);
        if (td_error) td_error[b] = e;
    }
}

template <int M>
void td_apply(const uint8_t *prev, const uint8_t *flag, int64_t B, const NtNet &net, int32_t *w, int64_t *acc, int32_t *cnt) {
    for (int64_t b = 0; b < B; ++b)  // the body of k_nt_td_apply
        if (flag[b]) nt_td_apply_lane<M>(get(prev, b), net, w, acc, cnt);
}

template <int M>
void tc_accumulate(const uint8_t *prev, const uint8_t *flag, const float *target, int64_t B, const int32_t *w, const NtNet &net,
                   float scale, float c, int64_t *acc, int64_t *abs_acc, int32_t *cnt, float *td_error) {
    for (int64_t b = 0; b < B; ++b) {  // the body of k_nt_tc_accumulate
        float e = 0.0f;
        if (flag[b]) e = nt_tc_accumulate_lane<M>(get(prev, b), flag[b], target[b], w, net, scale, c, acc, abs_acc, cnt);
        if (td_error) td_error[b] = e;
    }
}

template <int M>
void tc_apply(const uint8_t *prev, const uint8_t *flag, int64_t B, const NtNet &net, int32_t *w, int64_t *acc, int64_t *abs_acc,
              int32_t *cnt, int32_t *coh_e, int32_t *coh_a) {
    for (int64_t b = 0; b < B; ++b)  // the body of k_nt_tc_apply
        if (flag[b]) nt_tc_apply_lane<M>(get(prev, b), net, w, acc, abs_acc, cnt, coh_e, coh_a);
}

}  // namespace

#define NT_SWITCH(FN, m, ...)              \
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
// stage(board) of every board, as nt_offsets computes it
int hst_nts_stage(const uint8_t *boards, int64_t n, const uint8_t *cells, int m, int L, const uint8_t *tiles, int S, uint8_t *out) {
    NtNet net;
    if (!nt_read_staged(cells, m, L, tiles, S, net)) return -1;
    for (int64_t i = 0; i < n; ++i) out[i] = (uint8_t)nt_stage(net, get(boards, i));
    return 0;
}
int hst_nts_values(const uint8_t *boards, int64_t n, const int32_t *w, const uint8_t *cells, int m, int L, const uint8_t *tiles, int S,
                   int frac_bits, float *out) {
    NtNet net;
    if (!nt_read_staged(cells, m, L, tiles, S, net)) return -1;
    NT_SWITCH(values, m, boards, n, w, net, nt_scale(frac_bits), out);
    return 0;
}
int hst_nts_scores(const uint8_t *boards, int64_t B, const int32_t *w, const uint8_t *cells, int m, int L, const uint8_t *tiles, int S,
                   int frac_bits, float *q, float *v) {
    NtNet net;
    if (!nt_read_staged(cells, m, L, tiles, S, net)) return -1;
    NT_SWITCH(scores, m, boards, B, w, net, nt_scale(frac_bits), q, v);
    return 0;
}
// workspace f32[128 B] (8-byte aligned; unused for plies == 1)
int hst_nts_expectimax(const uint8_t *boards, int64_t B, const int32_t *w, const uint8_t *cells, int m, int L, const uint8_t *tiles,
                       int S, int frac_bits, int plies, double gamma, float *workspace, float *q, float *v) {
    NtNet net;
    if (!nt_read_staged(cells, m, L, tiles, S, net)) return -1;
    NT_SWITCH(expectimax, m, boards, B, w, net, nt_scale(frac_bits), plies, (float)gamma, workspace, q, v);
    return 0;
}
int hst_nts_td_accumulate(const uint8_t *prev, const uint8_t *flag, const float *target, int64_t B, const int32_t *w,
                          const uint8_t *cells, int m, int L, const uint8_t *tiles, int S, int frac_bits, double alpha, int64_t *acc,
                          int32_t *cnt, float *td_error) {
    NtNet net;
    if (!nt_read_staged(cells, m, L, tiles, S, net)) return -1;
    const float c = (float)(alpha * (double)(1u << frac_bits) / (8.0 * m));  // as the entry point computes it
    NT_SWITCH(td_accumulate, m, prev, flag, target, B, w, net, nt_scale(frac_bits), c, acc, cnt, td_error);
    return 0;
}
int hst_nts_td_apply(const uint8_t *prev, const uint8_t *flag, int64_t B, const uint8_t *cells, int m, int L, const uint8_t *tiles,
                     int S, int32_t *w, int64_t *acc, int32_t *cnt) {
    NtNet net;
    if (!nt_read_staged(cells, m, L, tiles, S, net)) return -1;
    NT_SWITCH(td_apply, m, prev, flag, B, net, w, acc, cnt);
    return 0;
}
int hst_nts_tc_accumulate(const uint8_t *prev, const uint8_t *flag, const float *target, int64_t B, const int32_t *w,
                          const uint8_t *cells, int m, int L, const uint8_t *tiles, int S, int frac_bits, double alpha, int64_t *acc,
                          int64_t *abs_acc, int32_t *cnt, float *td_error) {
    NtNet net;
    if (!nt_read_staged(cells, m, L, tiles, S, net)) return -1;
    const float c = (float)(alpha * (double)(1u << frac_bits) / (8.0 * m));
    NT_SWITCH(tc_accumulate, m, prev, flag, target, B, w, net, nt_scale(frac_bits), c, acc, abs_acc, cnt, td_error);
    return 0;
}
int hst_nts_tc_apply(const uint8_t *prev, const uint8_t *flag, int64_t B, const uint8_t *cells, int m, int L, const uint8_t *tiles,
                     int S, int32_t *w, int64_t *acc, int64_t *abs_acc, int32_t *cnt, int32_t *coh_e, int32_t *coh_a) {
    NtNet net;
    if (!nt_read_staged(cells, m, L, tiles, S, net)) return -1;
    NT_SWITCH(tc_apply, m, prev, flag, B, net, w, acc, abs_acc, cnt, coh_e, coh_a);
    return 0;
}
}

#ifdef NTUPLE_STAGE_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <vector>

// An eight-stage network (thresholds 2, 4, 6, 9, 12, 15, 17) whose tables are allocated at exactly [8][m][16^L]: values, scores,
// both search depths, a TD step and two TC steps on boards whose largest tile runs over 0 .. 17 (so every stage, the top one
// included, is read and written) plus random ones.  Exits non-zero if a stage is not what the definition says, if acc / abs_acc /
// cnt are not all zero after a step, if an output is NaN, or if the reader accepts a bad threshold list.  Under
// -fsanitize=address,undefined an offset that leaves the tables or a signed overflow aborts the run.
int main() {
    const int m = 3, L = 2, F = 12, S = 8;
    const uint8_t cells[m * L] = {0, 1, 5, 6, 3, 15};
    const uint8_t tiles[S - 1] = {2, 4, 6, 9, 12, 15, 17};
    const int64_t E = (int64_t)S * m << (4 * L), B = 40;
    std::vector<int32_t> w(E), cnt(E, 0), coh_e(E, 0), coh_a(E, 0);
    std::vector<int64_t> acc(E, 0), abs_acc(E, 0);
    std::vector<uint8_t> boards(16 * B, 0), flag(B), st(B);
    std::vector<float> q(4 * B), v(B), val(B), err(B), target(B);
    uint32_t s = 12345u;
    auto rnd = [&]() { return s = s * 1664525u + 1013904223u; };
    for (auto &x : w) x = (int32_t)(rnd() >> 11) - (1 << 20);
    for (int64_t b = 0; b < B; ++b) {
        for (int c = 0; c < 16; ++c) boards[16 * b + c] = (uint8_t)(b < 18 ? 0 : rnd() >> 28);
        if (b < 18) boards[16 * b + (b % 16)] = (uint8_t)b, boards[16 * b + ((b + 5) % 16)] = (uint8_t)(b ? 1 : 0);  // largest tile b
        flag[b] = (uint8_t)(b % 7 == 4 ? 0 : (b % 5 == 0 ? 2 : 1));
        target[b] = (rnd() & 4) ? 700.0f : -300.0f;
    }
    if (hst_nts_stage(boards.data(), B, cells, m, L, tiles, S, st.data())) return 1;
    for (int64_t b = 0; b < 18; ++b) {
        int want = 0;
        for (int i = 0; i < S - 1; ++i) want += b >= tiles[i];
        if (st[b] != want) return 2;
    }
    const uint8_t equal[2] = {5, 5}, descending[2] = {6, 5}, zero[1] = {0}, high[1] = {18};
    if (!hst_nts_stage(boards.data(), B, cells, m, L, equal, 3, st.data()) || !hst_nts_stage(boards.data(), B, cells, m, L, descending, 3, st.data()) ||
        !hst_nts_stage(boards.data(), B, cells, m, L, zero, 2, st.data()) || !hst_nts_stage(boards.data(), B, cells, m, L, high, 2, st.data()) ||
        !hst_nts_stage(boards.data(), B, cells, m, L, tiles, 9, st.data()) || !hst_nts_stage(boards.data(), B, cells, m, L, nullptr, 2, st.data()) ||
        !hst_nts_stage(boards.data(), B, cells, m, L, tiles, 0, st.data()) || hst_nts_stage(boards.data(), B, cells, m, L, nullptr, 1, st.data()))
        return 3;
    hst_nts_values(boards.data(), B, w.data(), cells, m, L, tiles, S, F, val.data());
    hst_nts_scores(boards.data(), B, w.data(), cells, m, L, tiles, S, F, q.data(), v.data());
    for (int64_t b = 0; b < B; ++b)
        if (!(val[b] == val[b]) || !(v[b] == v[b])) return 4;
    for (int plies = 1; plies <= 2; ++plies) {
        const int64_t R = 6;  // roots 12 .. 17: the search crosses the upper thresholds
        std::vector<float> ws(NTS_SLOTS * R, nanf("")), sq(4 * R, nanf("")), sv(R, nanf(""));
        hst_nts_expectimax(boards.data() + 16 * 12, R, w.data(), cells, m, L, tiles, S, F, plies, 0.99, ws.data(), sq.data(), sv.data());
        for (float x : sq)
            if (!(x == x)) return 5;
        for (float x : sv)
            if (!(x == x)) return 5;
    }
    hst_nts_td_accumulate(boards.data(), flag.data(), target.data(), B, w.data(), cells, m, L, tiles, S, F, 0.1, acc.data(), cnt.data(),
                          err.data());
    hst_nts_td_apply(boards.data(), flag.data(), B, cells, m, L, tiles, S, w.data(), acc.data(), cnt.data());
    for (int step = 0; step < 2; ++step) {
        for (int64_t i = 0; i < E; ++i)
            if (acc[i] != 0 || abs_acc[i] != 0 || cnt[i] != 0) return 6;
        hst_nts_tc_accumulate(boards.data(), flag.data(), target.data(), B, w.data(), cells, m, L, tiles, S, F, 1.0, acc.data(),
                              abs_acc.data(), cnt.data(), err.data());
        hst_nts_tc_apply(boards.data(), flag.data(), B, cells, m, L, tiles, S, w.data(), acc.data(), abs_acc.data(), cnt.data(),
                         coh_e.data(), coh_a.data());
    }
    for (int64_t i = 0; i < E; ++i) {
        if (acc[i] != 0 || abs_acc[i] != 0 || cnt[i] != 0) return 6;
        const int64_t e = coh_e[i], a = coh_a[i];
        if (a < 0 || (e < 0 ? -e : e) > a) return 7;
    }
    bool top = false;  // board 17 (flag 1) learned in the top stage's tables
    for (int64_t i = (int64_t)(S - 1) * m << (4 * L); i < E; ++i) top |= coh_a[i] != 0;
    if (!top) return 8;
    for (int64_t b = 0; b < B; ++b)
        if (!(err[b] == err[b])) return 9;
    printf("ntuple_stage_host ok\n");
    return 0;
}
#endif
