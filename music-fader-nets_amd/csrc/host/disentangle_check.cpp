// disentangle_check.cpp - stand-alone driver of the host twins of the six disentanglement entry points (disentangle_host.h), for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined disentangle_check.cpp -o disentangle_check  &&  ./disentangle_check in.bin out.bin
// in.bin starts with 10 int32 {op, ...}; out.bin with int32 rc, the outputs follow only for rc == 0.
//   op 0 range:  {0, N, P, ld}; x [(N-1)*ld + P] floats.                                 -> lo [P], hi [P] floats, status [P] int32
//   op 1 bin:    {1, N, P, ld, bins, n_pad, has_card}; x, lo [P], hi [P], card [P] int32 with has_card.
//                                                                                         -> img [(P-1)*n_pad + N] bytes (starts as 0xEE), status [P] (starts as 0)
//   op 2 hist:   {2, N, D, A, ldz, ldf}; bz [(D-1)*ldz + N], bf [(A-1)*ldf + N] bytes.   -> counts [D*A*4096] int32 (starts as -1)
//   op 3 ranks:  {3, N, P, ld, n_pad}; x.                                                 -> ranks [(P-1)*n_pad + N] floats (starts as CANARY)
//   op 4 corr:   {4, N, P, Q, x_rs, x_cs, y_rs, y_cs}; X [(N-1)*x_rs + (P-1)*x_cs + 1], Y [(N-1)*y_rs + (Q-1)*y_cs + 1] floats.
//                                                                                         -> mean_x [P], ss_x [P], mean_y [Q], ss_y [Q], cross [P*Q] doubles
//   op 5 mi:     {5, pairs}; counts [pairs*4096] int32.                                   -> out [pairs*3] doubles, hits [pairs] int32
// Every buffer has exactly the size the call may touch, so an access past an end is the sanitizer's to report.
#include <cstdio>
#include <vector>

#include "disentangle_host.h"

static const float CANARY = -777.25f;

template <typename T>
static bool get(std::FILE* f, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T>
static void put(std::FILE* f, const std::vector<T>& v) {
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
}
static size_t sz(long v) { return (size_t)(v > 0 ? v : 0); }
// an empty vector's data() may be null: that is another answer
template <typename T>
static T* ptr(std::vector<T>& v) {
    static T none[2] = {};
    return v.empty() ? none : v.data();
}
static size_t span(long rows, long rs, long cols, long cs) { return rows > 0 && cols > 0 ? sz((rows - 1) * rs + (cols - 1) * cs + 1) : 0; }

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[10];
    if (std::fread(hd, sizeof(int32_t), 10, f) != 10) return 2;
    for (int k = 1; k < 10; ++k)
        if (hd[k] < -1 || hd[k] > (1 << 23)) return 2;          // -1 and 0 are let through: the twins answer them
    const long CAP = 1L << 25;
    int32_t rc;
    std::vector<float> o_f32;
    std::vector<double> o_f64;
    std::vector<int32_t> o_i32;
    std::vector<uint8_t> o_u8;
    if (hd[0] == 0 || hd[0] == 3) {
        const int N = hd[1], P = hd[2], ld = hd[3], n_pad = hd[4];
        std::vector<float> x(span(N, ld, P, 1));
        if (x.size() > (size_t)CAP || !get(f, x)) return 2;
        if (hd[0] == 0) {
            o_f32.assign(2 * sz(P), CANARY), o_i32.assign(sz(P), -1);
            rc = fn_dis_host::column_range(ptr(x), ld, N, P, ptr(o_f32), ptr(o_f32) + sz(P), ptr(o_i32));
        } else {
            if (span(P, n_pad, N, 1) > (size_t)CAP) return 2;
            o_f32.assign(span(P, n_pad, N, 1), CANARY);
            rc = fn_dis_host::column_ranks(ptr(x), ld, N, P, ptr(o_f32), n_pad);
        }
    } else if (hd[0] == 1) {
        const int N = hd[1], P = hd[2], ld = hd[3], bins = hd[4], n_pad = hd[5], has_card = hd[6];
        std::vector<float> x(span(N, ld, P, 1)), lo(sz(P)), hi(sz(P));
        std::vector<int32_t> card(has_card ? sz(P) : 0);
        if (x.size() > (size_t)CAP || span(P, n_pad, N, 1) > (size_t)CAP || !get(f, x) || !get(f, lo) || !get(f, hi) || !get(f, card)) return 2;
        o_u8.assign(span(P, n_pad, N, 1), 0xEE), o_i32.assign(sz(P), 0);
        rc = fn_dis_host::bin_columns(ptr(x), ld, N, P, ptr(lo), ptr(hi), has_card ? ptr(card) : nullptr, bins, ptr(o_u8), n_pad, ptr(o_i32));
    } else if (hd[0] == 2) {
        const int N = hd[1], D = hd[2], A = hd[3], ldz = hd[4], ldf = hd[5];
        std::vector<uint8_t> bz(span(D, ldz, N, 1)), bf(span(A, ldf, N, 1));
        const int Dc = D > FN_DIS_MAX_D ? 0 : D, Ac = A > FN_DIS_MAX_A ? 0 : A;          // beyond the limits the twin answers before it touches counts
        if (bz.size() > (size_t)CAP || bf.size() > (size_t)CAP || sz(Dc) * sz(Ac) > 2048 || !get(f, bz) || !get(f, bf)) return 2;
        o_i32.assign(sz(Dc) * sz(Ac) * fn_dis_host::CELLS, -1);
        rc = fn_dis_host::joint_hist(ptr(bz), ldz, D, ptr(bf), ldf, A, N, ptr(o_i32));
    } else if (hd[0] == 4) {
        const int N = hd[1], P = hd[2], Q = hd[3], x_rs = hd[4], x_cs = hd[5], y_rs = hd[6], y_cs = hd[7];
        std::vector<float> X(span(N, x_rs, P, x_cs)), Y(span(N, y_rs, Q, y_cs));
        if (X.size() > (size_t)CAP || Y.size() > (size_t)CAP || !get(f, X) || !get(f, Y)) return 2;
        const size_t p = sz(P), q = sz(Q);
        o_f64.assign(2 * p + 2 * q + p * q, (double)CANARY);
        double* o = ptr(o_f64);
        rc = fn_dis_host::column_corr(ptr(X), x_rs, x_cs, P, ptr(Y), y_rs, y_cs, Q, N, o, o + p, o + 2 * p, o + 2 * p + q, o + 2 * p + 2 * q);
    } else if (hd[0] == 5) {
        const int pairs = hd[1];
        if (pairs > 2048) return 2;
        std::vector<int32_t> counts(sz(pairs) * fn_dis_host::CELLS);
        if (!get(f, counts)) return 2;
        o_f64.assign(sz(pairs) * FN_DIS_MI_COLS, (double)CANARY), o_i32.assign(sz(pairs), -1);
        rc = fn_dis_host::mi_scores(ptr(counts), pairs, ptr(o_f64), ptr(o_i32));
    } else {
        return 2;
    }
    std::fclose(f);
    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(&rc, sizeof(rc), 1, o);
    if (rc == 0) put(o, o_u8), put(o, o_f32), put(o, o_f64), put(o, o_i32);
    std::fclose(o);
    std::printf("disentangle twin op %d rc %d\n", (int)hd[0], (int)rc);
    return 0;
}
