// Host build of 2048-ppo-agent_amd/csrc/g2048_ntuple.h (G2048_HOST_TEST) for CPU-side logic tests.
// Test infrastructure only: lets tests/ check the per-lane n-tuple code the kernels of g2048_ntuple.hip run against the numpy
// restatement without a GPU.  Accumulate and apply are emulated sequentially, env by env.  The product never builds or loads this.
// With NTUPLE_HOST_MAIN it is a stand-alone program (for a sanitizer build): a small fixed case, checked for its invariants.
#define G2048_HOST_TEST 1
#include "g2048_ntuple.h"
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

template <int M>
void values(const uint8_t *boards, int64_t n, const int32_t *w, const NtNet &net, float scale, float *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = nt_value(nt_sum<M>(w, net, get(boards, i)), scale);  // the body of k_nt_values
}

template <int M>
void scores(const uint8_t *boards, int64_t B, const int32_t *w, const NtNet &net, float scale, float *q, float *v) {
    for (int64_t b = 0; b < B; ++b) {  // the four lanes of a quad of k_nt_scores
        float x = nt_neg_inf();
        for (u32 a = 0; a < 4; ++a) {
            bool legal;
            q[4 * b + a] = nt_score<M>(w, net, scale, get(boards, b), a, legal);
            x = nt_vmax(x, legal ? q[4 * b + a] : nt_neg_inf());
        }
        v[b] = x == nt_neg_inf() ? 0.0f : x;
    }
}

template <int M>
void accumulate(const uint8_t *prev, const uint8_t *flag, const float *target, int64_t B, const int32_t *w, const NtNet &net,
                float scale, float c, int64_t *acc, int32_t *cnt, float *td_error) {
    for (int64_t b = 0; b < B; ++b) {  // the body of k_nt_td_accumulate
        float e = 0.0f;
        if (flag[b]) e = nt_td_accumulate_lane<M>(get(prev, b), flag[b], target[b], w, net, scale, c, acc, cnt);
        if (td_error) td_error[b] = e;
    }
}

template <int M>
void apply(const uint8_t *prev, const uint8_t *flag, int64_t B, const NtNet &net, int32_t *w, int64_t *acc, int32_t *cnt) {
    for (int64_t b = 0; b < B; ++b)  // the body of k_nt_td_apply
        if (flag[b]) nt_td_apply_lane<M>(get(prev, b), net, w, acc, cnt);
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
void hst_nt_values(const uint8_t *boards, int64_t n, const int32_t *w, const uint8_t *cells, int m, int L, int frac_bits, float *out) {
    const NtNet net = make_net(cells, m, L);
    NT_SWITCH(values, m, boards, n, w, net, nt_scale(frac_bits), out);
}
void hst_nt_scores(const uint8_t *boards, int64_t B, const int32_t *w, const uint8_t *cells, int m, int L, int frac_bits, float *q,
                   float *v) {
    const NtNet net = make_net(cells, m, L);
    NT_SWITCH(scores, m, boards, B, w, net, nt_scale(frac_bits), q, v);
}
void hst_nt_td_accumulate(const uint8_t *prev, const uint8_t *flag, const float *target, int64_t B, const int32_t *w,
                          const uint8_t *cells, int m, int L, int frac_bits, double alpha, int64_t *acc, int32_t *cnt, float *td_error) {
    const NtNet net = make_net(cells, m, L);
    const float c = (float)(alpha * (double)(1u << frac_bits) / (8.0 * m));  // as the entry point computes it
    NT_SWITCH(accumulate, m, prev, flag, target, B, w, net, nt_scale(frac_bits), c, acc, cnt, td_error);
}
void hst_nt_td_apply(const uint8_t *prev, const uint8_t *flag, int64_t B, const uint8_t *cells, int m, int L, int32_t *w, int64_t *acc,
                     int32_t *cnt) {
    const NtNet net = make_net(cells, m, L);
    NT_SWITCH(apply, m, prev, flag, B, net, w, acc, cnt);
}
void hst_nt_link(const uint8_t *boards_row, const uint8_t *meta_row, int64_t B, uint8_t *prev, uint8_t *flag) {
    for (int64_t b = 0; b < B; ++b) {  // the body of k_nt_link
        Board bd = get(boards_row, b);
        flag[b] = (uint8_t)nt_link_lane(bd, meta_row[b]);
        memcpy(prev + 16 * b, bd.r, 16);
    }
}
}

#ifdef NTUPLE_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <vector>

// one TD step on boards that include tiles above 15, self-symmetric boards and full boards; exits non-zero if acc / cnt are not
// all zero afterwards or a value is not finite.  Under -fsanitize=address,undefined any out-of-table access aborts the run.
int main() {
    const int m = 3, L = 2, F = 12;
    const uint8_t cells[m * L] = {0, 1, 5, 6, 3, 15};
    const int64_t E = (int64_t)m << (4 * L), B = 40;
    std::vector<int32_t> w(E), cnt(E, 0);
    std::vector<int64_t> acc(E, 0);
    std::vector<uint8_t> boards(16 * B), prev(16 * B), flag(B), meta(B);
    std::vector<float> q(4 * B), v(B), val(B), err(B);
    uint32_t s = 12345u;
    auto rnd = [&]() { return s = s * 1664525u + 1013904223u; };
    for (auto &x : w) x = (int32_t)(rnd() >> 11) - (1 << 20);
    w[0] = 2147483647;
    w[1] = -2147483647 - 1;
    for (int64_t b = 0; b < B; ++b)
        for (int c = 0; c < 16; ++c) boards[16 * b + c] = b == 0 ? 0 : (b == 1 ? 3 : (b == 2 ? 16 + (c & 1) : (uint8_t)(rnd() >> 28)));
    for (int64_t b = 0; b < B; ++b) meta[b] = (uint8_t)((b & 3) | (0xF << 2) | ((b % 5 == 0) << 6));
    hst_nt_values(boards.data(), B, w.data(), cells, m, L, F, val.data());
    hst_nt_scores(boards.data(), B, w.data(), cells, m, L, F, q.data(), v.data());
    hst_nt_link(boards.data(), meta.data(), B, prev.data(), flag.data());
    flag[7] = 0;
    hst_nt_td_accumulate(prev.data(), flag.data(), v.data(), B, w.data(), cells, m, L, F, 0.1, acc.data(), cnt.data(), err.data());
    hst_nt_td_apply(prev.data(), flag.data(), B, cells, m, L, w.data(), acc.data(), cnt.data());
    for (int64_t i = 0; i < E; ++i)
        if (acc[i] != 0 || cnt[i] != 0) return 2;
    for (int64_t b = 0; b < B; ++b)
        if (!(val[b] == val[b]) || !(v[b] == v[b]) || !(err[b] == err[b])) return 3;
    printf("ntuple_host ok\n");
    return 0;
}
#endif
