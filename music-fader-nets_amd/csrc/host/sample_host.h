// sample_host.h - the arithmetic of fn_vocab_sample_host (include/fadernets.h has the definition it follows step by step): one row of logits ->
// log-probs, first-index argmax, drawn token and the uniform.  Plain C++, no dependencies: fadernets_host.cpp and the stand-alone sample_check.cpp
// both include it.
#ifndef FADERNETS_SAMPLE_HOST_H
#define FADERNETS_SAMPLE_HOST_H

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../../include/fadernets.h"

namespace fn_sample_host {

inline void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

inline float uniform(uint32_t row, uint32_t step, const FnSampleParams& p) {
    const uint32_t ctr[4] = {row, step, p.offset_lo, p.offset_hi}, key[2] = {p.seed_lo, p.seed_hi};
    uint32_t out[4];
    philox4x32_10(ctr, key, out);
    return (float)(out[0] >> 8) * 0x1p-24f;
}

// the parameters as the kernel clamps them
inline void clamp_params(const FnSampleParams& p, int V, int* top_k, float* top_p, float* inv_t) {
    *top_k = p.top_k < 0 ? 0 : (p.top_k > V ? V : p.top_k);
    float tp = p.top_p;
    if (!(tp <= 1.0f)) tp = 1.0f;
    if (tp < FN_SAMPLE_MIN_P) tp = FN_SAMPLE_MIN_P;
    *top_p = tp;
    float it = p.inv_temperature;
    if (it != it) it = 1.0f;
    it = std::fmin(std::fmax(it, FN_SAMPLE_MIN_INV_T), FN_SAMPLE_MAX_INV_T);
    *inv_t = it;
}

// x [V] -> lp [V] (scratch of the caller), returns the first-index argmax through *own and the drawn token; u through *u_out
inline int sample_row(const float* x, int V, uint32_t row, int step, const FnSampleParams& p, float* lp, int* own, float* u_out) {
    float mx = -INFINITY;
    int am = 0x7fffffff;
    for (int e = 0; e < V; ++e)
        if (x[e] > mx) { mx = x[e]; am = e; }
    float s = 0.0f;
    for (int e = 0; e < V; ++e) s += std::exp(x[e] - mx);
    const float lse = mx + std::log(s);
    for (int e = 0; e < V; ++e) lp[e] = x[e] - lse;
    *own = am;
    int top_k;
    float top_p, inv_t;
    clamp_params(p, V, &top_k, &top_p, &inv_t);
    const float lp_max = mx - lse;
    std::vector<float> w((size_t)V, 0.0f), c((size_t)V);
    std::vector<int> idx((size_t)V, 0);
    for (int e = 0; e < V; ++e) {
        int rank = 0;
        for (int j = 0; j < V; ++j) rank += (lp[j] > lp[e] || (lp[j] == lp[e] && j < e)) ? 1 : 0;
        w[(size_t)rank] = std::exp((lp[e] - lp_max) * inv_t);
        idx[(size_t)rank] = e;
    }
    // blocked prefix sums in the kernel's order
    const int per = (V + 63) / 64;
    float tot[64], run[64];
    for (int l = 0; l < 64; ++l) {
        float r = 0.0f;
        for (int k = 0; k < per; ++k) {
            const int j = per * l + k;
            r += j < V ? w[(size_t)j] : 0.0f;
            if (j < V) c[(size_t)j] = r;
        }
        tot[l] = r;
    }
    for (int o = 1; o < 64; o <<= 1) {
        for (int l = 0; l < 64; ++l) run[l] = l >= o ? tot[l] + tot[l - o] : tot[l];
        for (int l = 0; l < 64; ++l) tot[l] = run[l];
    }
    for (int j = 0; j < V; ++j) {
        const int l = j / per;
        c[(size_t)j] = (l ? tot[l - 1] : 0.0f) + c[(size_t)j];
    }
    const int n = top_k ? top_k : V;
    int m = n;
    if (top_p < 1.0f) {
        const float thr = top_p * c[(size_t)n - 1];
        m = 1;
        for (int j = 0; j < n; ++j) m += c[(size_t)j] < thr ? 1 : 0;      // a count, as the definition: c may step down by an ulp at a block border
        if (m > n) m = n;
    }
    const float u = uniform(row, (uint32_t)step, p);
    const float t = u * c[(size_t)m - 1];
    int j = 0;
    for (int i = 0; i < m; ++i) j += !(c[(size_t)i] > t) ? 1 : 0;
    if (j > m - 1) j = m - 1;
    *u_out = u;
    const int tok = idx[(size_t)j];
    return tok < 0 ? 0 : (tok > V - 1 ? V - 1 : tok);
}

inline int vocab_sample(const float* logits, int B, int V, int ld, const FnSampleParams* params, int step, float* logp_out, int64_t logp_ld,
                        int32_t* own_out, int own_ld, int32_t* tok_out, int tok_ld, float* u_out) {
    if (!logits || !params || !tok_out) return FN_E_NULL;
    if (B <= 0 || V < 1 || V > FN_SAMPLE_MAX_V || ld < V || step < 0) return FN_E_SHAPE;
    std::vector<float> lp((size_t)V);
    for (int b = 0; b < B; ++b) {
        int own;
        float u;
        tok_out[(long)b * tok_ld] = sample_row(logits + (long)b * ld, V, (uint32_t)b, step, *params, lp.data(), &own, &u);
        if (logp_out)
            for (int e = 0; e < V; ++e) logp_out[(long)b * logp_ld + e] = lp[(size_t)e];
        if (own_out) own_out[(long)b * own_ld] = own;
        if (u_out) u_out[b] = u;
    }
    return FN_OK;
}

}  // namespace fn_sample_host
#endif
