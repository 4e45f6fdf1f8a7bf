// disentangle_host.h - the six entry points of the disentanglement report (fn_column_range, fn_bin_columns, fn_joint_hist, fn_column_ranks,
// fn_column_corr, fn_mi_scores) in plain C++: include/fadernets.h has the definitions these follow step by step, in the stated order of every fp64
// sum.  No dependencies: the stand-alone disentangle_check.cpp includes it for the twins, csrc/disentangle.hip for the argument checks the device
// entry points share with them.  The bin arithmetic and every term of the centred sums are single IEEE fp64 operations: build with -ffp-contract=off
// where the target has a fused multiply-add (the Makefile does for disentangle.hip, the CPU test for the driver).
#ifndef FADERNETS_DISENTANGLE_HOST_H
#define FADERNETS_DISENTANGLE_HOST_H

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../../include/fadernets.h"

#ifdef __HIPCC__
#define FN_DIS_HD __host__ __device__
#else
#define FN_DIS_HD
#endif

namespace fn_dis_host {

constexpr int CELLS = FN_DIS_MAX_BINS * FN_DIS_MAX_BINS;

inline bool aligned4(const void* p) { return (uintptr_t)p % 4 == 0; }
inline bool aligned8(const void* p) { return (uintptr_t)p % 8 == 0; }

// the xor butterfly of fn_wave_sum_f64 over the 64 lanes' partial sums
inline double wave_sum(const double part[64]) {
    double s[64], t[64];
    for (int l = 0; l < 64; ++l) s[l] = part[l];
    for (int o = 32; o > 0; o >>= 1) {
        for (int l = 0; l < 64; ++l) t[l] = s[l] + s[l ^ o];
        for (int l = 0; l < 64; ++l) s[l] = t[l];
    }
    return s[0];
}

// ---- the checks: NULL, sizes, limits, alignment - in this order ----
inline int matrix_check(int64_t ld, int N, int P, int max_p) {
    if (N < 1 || P < 1 || ld < P) return FN_E_SHAPE;
    if (N > FN_DIS_MAX_N || P > max_p) return FN_E_UNSUPPORTED;
    return FN_OK;
}

inline int range_check(const float* x, int64_t ld, int N, int P, const float* lo, const float* hi, const int32_t* status) {
    if (!x || !lo || !hi || !status) return FN_E_NULL;
    const int rc = matrix_check(ld, N, P, FN_DIS_MAX_D);
    if (rc != FN_OK) return rc;
    if (!aligned4(x) || !aligned4(lo) || !aligned4(hi) || !aligned4(status)) return FN_E_ALIGN;
    return FN_OK;
}

inline int bin_check(const float* x, int64_t ld, int N, int P, const float* lo, const float* hi, const int32_t* card, int bins, const uint8_t* img,
                     int64_t n_pad, const int32_t* status) {
    if (!x || !lo || !hi || !img || !status) return FN_E_NULL;
    if (N < 1 || P < 1 || ld < P || bins < 1 || n_pad < N) return FN_E_SHAPE;
    if (card)
        for (int c = 0; c < P && c < FN_DIS_MAX_A; ++c)
            if (card[c] < 0 || card[c] > FN_DIS_MAX_BINS) return FN_E_SHAPE;
    if (N > FN_DIS_MAX_N || P > (card ? FN_DIS_MAX_A : FN_DIS_MAX_D) || bins > FN_DIS_MAX_BINS) return FN_E_UNSUPPORTED;
    if (!aligned4(x) || !aligned4(lo) || !aligned4(hi) || !aligned4(status)) return FN_E_ALIGN;
    return FN_OK;
}

inline int hist_check(const uint8_t* bz, int64_t ldz, int D, const uint8_t* bf, int64_t ldf, int A, int N, const int32_t* counts) {
    if (!bz || !bf || !counts) return FN_E_NULL;
    if (N < 1 || D < 1 || A < 1 || ldz < N || ldf < N) return FN_E_SHAPE;
    if (N > FN_DIS_MAX_N || D > FN_DIS_MAX_D || A > FN_DIS_MAX_A) return FN_E_UNSUPPORTED;
    if (!aligned4(counts)) return FN_E_ALIGN;
    return FN_OK;
}

inline int ranks_check(const float* x, int64_t ld, int N, int P, const float* ranks, int64_t n_pad) {
    if (!x || !ranks) return FN_E_NULL;
    if (N < 1 || P < 1 || ld < P || n_pad < N) return FN_E_SHAPE;
    if (N > FN_DIS_MAX_N || P > FN_DIS_MAX_D) return FN_E_UNSUPPORTED;
    if (!aligned4(x) || !aligned4(ranks)) return FN_E_ALIGN;
    return FN_OK;
}

inline int corr_check(const float* X, int64_t x_rs, int64_t x_cs, int P, const float* Y, int64_t y_rs, int64_t y_cs, int Q, int N, const double* mean_x,
                      const double* ss_x, const double* mean_y, const double* ss_y, const double* cross) {
    if (!X || !Y || !mean_x || !ss_x || !mean_y || !ss_y || !cross) return FN_E_NULL;
    if (N < 1 || P < 1 || Q < 1 || x_rs < 1 || x_cs < 1 || y_rs < 1 || y_cs < 1) return FN_E_SHAPE;
    if (N > FN_DIS_MAX_N || P > FN_DIS_MAX_D || Q > FN_DIS_MAX_A) return FN_E_UNSUPPORTED;
    if (!aligned4(X) || !aligned4(Y) || !aligned8(mean_x) || !aligned8(ss_x) || !aligned8(mean_y) || !aligned8(ss_y) || !aligned8(cross)) return FN_E_ALIGN;
    return FN_OK;
}

inline int mi_check(const int32_t* counts, int pairs, const double* out, const int32_t* hits) {
    if (!counts || !out || !hits) return FN_E_NULL;
    if (pairs < 1) return FN_E_SHAPE;
    if (pairs > FN_DIS_MAX_D * FN_DIS_MAX_A) return FN_E_UNSUPPORTED;
    if (!aligned4(counts) || !aligned8(out) || !aligned4(hits)) return FN_E_ALIGN;
    return FN_OK;
}

// ---- fn_column_range ----
inline bool finite32(float v) { return std::fabs(v) <= 3.402823466e+38f; }          // false for a NaN

inline int column_range(const float* x, int64_t ld, int N, int P, float* lo, float* hi, int32_t* status) {
    const int rc = range_check(x, ld, N, P, lo, hi, status);
    if (rc != FN_OK) return rc;
    for (int c = 0; c < P; ++c) {
        float a = INFINITY, b = -INFINITY;
        int32_t st = 0;
        for (int i = 0; i < N; ++i) {
            const float v = x[(int64_t)i * ld + c] + 0.0f;
            if (!finite32(v)) {
                st = FN_DIS_NONFINITE;
                continue;
            }
            a = v < a ? v : a, b = v > b ? v : b;
        }
        lo[c] = a, hi[c] = b, status[c] = st;
    }
    return FN_OK;
}

// ---- fn_bin_columns ----
FN_DIS_HD inline int bin_of(float x, float lo, float hi, int bins) {
    if (hi == lo) return 0;
    const double num = (double)x - (double)lo;
    const double den = (double)hi - (double)lo;
    const double q = num / den;
    const double t = q * (double)bins;
    if (!(t >= 0.0)) return 0;          // below lo, or a NaN
    return t < (double)bins ? (int)t : bins - 1;
}

FN_DIS_HD inline bool level_of(float x, int card, int* bin) {
    const bool ok = x >= 0.0f && x < (float)card && x == floorf(x);
    *bin = ok ? (int)x : 0;
    return ok;
}

inline int bin_columns(const float* x, int64_t ld, int N, int P, const float* lo, const float* hi, const int32_t* card, int bins, uint8_t* img,
                       int64_t n_pad, int32_t* status) {
    const int rc = bin_check(x, ld, N, P, lo, hi, card, bins, img, n_pad, status);
    if (rc != FN_OK) return rc;
    for (int c = 0; c < P; ++c) {
        const int C = card ? card[c] : 0;
        for (int i = 0; i < N; ++i) {
            const float v = x[(int64_t)i * ld + c];
            int b;
            if (C == 0)
                b = bin_of(v, lo[c], hi[c], bins);
            else if (!level_of(v, C, &b))
                status[c] |= FN_DIS_BAD_LEVEL;
            img[(int64_t)c * n_pad + i] = (uint8_t)b;
        }
    }
    return FN_OK;
}

// ---- fn_joint_hist ----
inline int joint_hist(const uint8_t* bz, int64_t ldz, int D, const uint8_t* bf, int64_t ldf, int A, int N, int32_t* counts) {
    const int rc = hist_check(bz, ldz, D, bf, ldf, A, N, counts);
    if (rc != FN_OK) return rc;
    std::memset(counts, 0, sizeof(int32_t) * (size_t)D * A * CELLS);
    for (int d = 0; d < D; ++d)
        for (int a = 0; a < A; ++a) {
            int32_t* t = counts + ((size_t)d * A + a) * CELLS;
            for (int i = 0; i < N; ++i) t[(bz[d * ldz + i] & 63) * 64 + (bf[a * ldf + i] & 63)] += 1;
        }
    return FN_OK;
}

// ---- fn_column_ranks ----
inline int column_ranks(const float* x, int64_t ld, int N, int P, float* ranks, int64_t n_pad) {
    const int rc = ranks_check(x, ld, N, P, ranks, n_pad);
    if (rc != FN_OK) return rc;
    for (int c = 0; c < P; ++c)
        for (int i = 0; i < N; ++i) {
            const float v = x[(int64_t)i * ld + c];
            int less = 0, equal = 0;
            for (int j = 0; j < N; ++j) {
                const float w = x[(int64_t)j * ld + c];
                less += w < v, equal += w == v;
            }
            ranks[(int64_t)c * n_pad + i] = (float)(2 * less + equal + 1) * 0.5f;
        }
    return FN_OK;
}

// ---- fn_column_corr ----
// the lane-strided sum of f(i) over i < N, then the butterfly
template <class F>
inline double lane_sum(int N, F f) {
    double part[64];
    for (int l = 0; l < 64; ++l) part[l] = 0.0;
    for (int i = 0; i < N; ++i) {
        const double term = f(i);          // rounded before it is added
        part[i & 63] += term;
    }
    return wave_sum(part);
}

inline int column_corr(const float* X, int64_t x_rs, int64_t x_cs, int P, const float* Y, int64_t y_rs, int64_t y_cs, int Q, int N, double* mean_x,
                       double* ss_x, double* mean_y, double* ss_y, double* cross) {
    const int rc = corr_check(X, x_rs, x_cs, P, Y, y_rs, y_cs, Q, N, mean_x, ss_x, mean_y, ss_y, cross);
    if (rc != FN_OK) return rc;
    for (int q = 0; q < Q; ++q) {
        const float* y = Y + q * y_cs;
        const double m = lane_sum(N, [&](int i) { return (double)y[i * y_rs]; }) / (double)N;
        mean_y[q] = m;
        ss_y[q] = lane_sum(N, [&](int i) {
            const double d = (double)y[i * y_rs] - m;
            return d * d;
        });
    }
    for (int p = 0; p < P; ++p) {
        const float* x = X + p * x_cs;
        const double m = lane_sum(N, [&](int i) { return (double)x[i * x_rs]; }) / (double)N;
        mean_x[p] = m;
        ss_x[p] = lane_sum(N, [&](int i) {
            const double d = (double)x[i * x_rs] - m;
            return d * d;
        });
        for (int q = 0; q < Q; ++q) {
            const float* y = Y + q * y_cs;
            const double my = mean_y[q];
            cross[(size_t)p * Q + q] = lane_sum(N, [&](int i) {
                const double dx = (double)x[i * x_rs] - m, dy = (double)y[i * y_rs] - my;
                return dx * dy;
            });
        }
    }
    return FN_OK;
}

// ---- fn_mi_scores ----
inline int mi_scores(const int32_t* counts, int pairs, double* out, int32_t* hits) {
    const int rc = mi_check(counts, pairs, out, hits);
    if (rc != FN_OK) return rc;
    for (int e = 0; e < pairs; ++e) {
        const int32_t* t = counts + (size_t)e * CELLS;
        int64_t r[64], c[64], T = 0;
        int32_t h = 0;
        for (int k = 0; k < 64; ++k) r[k] = c[k] = 0;
        for (int bz = 0; bz < 64; ++bz) {
            int32_t mx = 0;
            for (int bf = 0; bf < 64; ++bf) {
                const int32_t n = t[bz * 64 + bf];
                r[bz] += n, c[bf] += n, mx = n > mx ? n : mx;
            }
            T += r[bz], h += mx;
        }
        double* o = out + (size_t)e * FN_DIS_MI_COLS;
        hits[e] = h;
        if (T == 0) {
            o[0] = o[1] = o[2] = 0.0;
            continue;
        }
        const double dT = (double)T;
        double pi[64], pz[64], pf[64];
        for (int l = 0; l < 64; ++l) {
            pi[l] = 0.0;
            for (int bz = 0; bz < 64; ++bz) {
                const int64_t n = t[bz * 64 + l];
                if (n > 0) {
                    const double term = ((double)n / dT) * std::log((double)(n * T) / (double)(r[bz] * c[l]));
                    pi[l] += term;
                }
            }
            pz[l] = pf[l] = 0.0;
            if (r[l] > 0) {
                const double p = (double)r[l] / dT, term = p * std::log(p);
                pz[l] += term;
            }
            if (c[l] > 0) {
                const double p = (double)c[l] / dT, term = p * std::log(p);
                pf[l] += term;
            }
        }
        o[0] = wave_sum(pi), o[1] = -wave_sum(pz), o[2] = -wave_sum(pf);
    }
    return FN_OK;
}

}  // namespace fn_dis_host
#endif
