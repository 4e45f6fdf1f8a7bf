// report_host.h - fn_token_score / fn_match_rows in plain C++ (include/fadernets.h has the definition these follow clause by clause, not the
// kernels).  No dependencies: the stand-alone report_check.cpp includes it.  The fp32 sum of exponentials and the fp64 sum of the nll run in
// the stated order: 64 partial sums, partial l over e = l, l + 64, ... ascending, then s[l] += s[l ^ o] for o = 32 .. 1.
#ifndef FADERNETS_REPORT_HOST_H
#define FADERNETS_REPORT_HOST_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

#include "../../../include/fadernets.h"

namespace fn_report_host {

template <typename T>
inline T butterfly(T* s) {
    for (int o = 32; o > 0; o >>= 1) {
        T n[64];
        for (int l = 0; l < 64; ++l) n[l] = s[l] + s[l ^ o];
        for (int l = 0; l < 64; ++l) s[l] = n[l];
    }
    return s[0];
}

inline int token_score(const float* x, int64_t stride_b, int64_t stride_t, int B, int T, int V, const int32_t* target, int tgt_ld, int32_t* pred,
                       float* nll, int32_t* rank, int out_ld) {
    if (!x || (!pred && !nll && !rank) || ((nll || rank) && !target)) return FN_E_NULL;
    if (B < 1 || T < 1 || V < 1 || V > FN_SAMPLE_MAX_V || out_ld < T || (target && tgt_ld < T)) return FN_E_SHAPE;
    for (int64_t b = 0; b < B; ++b)
        for (int64_t t = 0; t < T; ++t) {
            const float* xr = x + b * stride_b + t * stride_t;
            float mx = -std::numeric_limits<float>::infinity();
            int am = 0x7fffffff;
            for (int e = 0; e < V; ++e)
                if (xr[e] > mx) mx = xr[e], am = e;
            if (pred) pred[b * out_ld + t] = am;
            if (!target) continue;
            const int tg = std::min(std::max(target[b * tgt_ld + t], 0), V - 1);
            const float xt = xr[tg];
            float s[64];
            int cnt = 0;
            for (int l = 0; l < 64; ++l) {
                s[l] = 0.f;
                for (int e = l; e < V; e += 64) s[l] += std::exp(xr[e] - mx);
            }
            for (int e = 0; e < V; ++e) cnt += (xr[e] > xt || (xr[e] == xt && e < tg)) ? 1 : 0;
            if (nll) nll[b * out_ld + t] = (mx + std::log(butterfly(s))) - xt;
            if (rank) rank[b * out_ld + t] = cnt;
        }
    return FN_OK;
}

inline int match_rows(const int32_t* pred, int pred_ld, const int32_t* target, int tgt_ld, int rows, int T, int trim, const float* nll,
                      const int32_t* rank, int aux_ld, int topk, int32_t* lead, int32_t* len, int32_t* correct, int32_t* correct_topk, double* acc,
                      double* nll_sum, int32_t* status) {
    if (!pred || !target || !lead || !len || !correct || !acc || !status || (rank != nullptr) != (correct_topk != nullptr) ||
        (nll != nullptr) != (nll_sum != nullptr))
        return FN_E_NULL;
    if (rows < 1 || T < 1 || pred_ld < T || tgt_ld < T || ((nll || rank) && aux_ld < T) || (rank && topk < 1)) return FN_E_SHAPE;
    for (int64_t r = 0; r < rows; ++r) {
        const int32_t* tr = target + r * tgt_ld;
        const int32_t* pr = pred + r * pred_ld;
        int ld = 0, n = T;
        if (trim) {
            int first = T, last = -1;
            for (int j = 0; j < T; ++j)
                if (tr[j] != 0) first = std::min(first, j), last = j;
            ld = first, n = last >= 0 ? last + 1 - first : 0;
        }
        int ok = 0, ok_k = 0;
        double s[64];
        for (int l = 0; l < 64; ++l) s[l] = 0.0;
        for (int j = 0; j < n; ++j) {
            ok += pr[j] == tr[ld + j] ? 1 : 0;
            if (rank) ok_k += rank[r * aux_ld + ld + j] < topk ? 1 : 0;
            if (nll) s[j & 63] += (double)nll[r * aux_ld + ld + j];
        }
        lead[r] = ld, len[r] = n, correct[r] = ok;
        if (correct_topk) correct_topk[r] = ok_k;
        acc[r] = n > 0 ? (double)ok / (double)n : 0.0;
        if (nll_sum) nll_sum[r] = butterfly(s);
        status[r] = n > 0 ? 0 : FN_MATCH_EMPTY;
    }
    return FN_OK;
}

}  // namespace fn_report_host

#endif
