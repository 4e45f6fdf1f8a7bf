// beam_host.h - the arithmetic of fn_beam_step / fn_beam_gather / fn_beam_backtrack in plain C++ (include/fadernets.h has the definition these follow
// clause by clause).  No dependencies: the stand-alone beam_check.cpp includes it.  The log-sum-exp is summed in index order here (the kernel sums
// lane-wise), so log-prob rows may differ from the kernel's in their last bits; the selection is exact on whatever rows it is given.
#ifndef FADERNETS_BEAM_HOST_H
#define FADERNETS_BEAM_HOST_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../../include/fadernets.h"

namespace fn_beam_host {

inline uint64_t pack(float s, int i, int n) {
    uint32_t b;
    std::memcpy(&b, &s, 4);
    const uint32_t key = b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
    return ((uint64_t)key << 32) | (uint32_t)(n - 1 - i);
}

inline float unkey(uint32_t key) {
    const uint32_t b = key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu);
    float s;
    std::memcpy(&s, &b, 4);
    return s;
}

inline int beam_step(const float* logits, int B, int W, int V, int ld, int step, int eos, const float* score_prev, const int32_t* token_prev,
                     int prev_ld, float* score, int32_t* parent, int32_t* token, int out_ld, float* logp_out, int64_t logp_ld) {
    if (!logits || !score || !parent || !token) return FN_E_NULL;
    if (step > 0 && (!score_prev || !token_prev)) return FN_E_NULL;
    if (B < 1 || V < 1 || V > FN_SAMPLE_MAX_V || W < 1 || W > FN_BEAM_MAX_W || W > V || ld < V || step < 0 || eos >= V || eos < -1 || out_ld < W ||
        (step > 0 && prev_ld < W))
        return FN_E_SHAPE;
    const int n = W * V;
    std::vector<float> lp((size_t)V);
    std::vector<uint64_t> cand;
    for (int b = 0; b < B; ++b) {
        cand.clear();
        for (int w = 0; w < W; ++w) {
            const long r = (long)b * W + w;
            const float* x = logits + r * ld;
            float mx = -INFINITY;
            for (int e = 0; e < V; ++e)
                if (x[e] > mx) mx = x[e];
            float s = 0.0f;
            for (int e = 0; e < V; ++e) s += std::exp(x[e] - mx);
            const float lse = mx + std::log(s);
            for (int e = 0; e < V; ++e) lp[(size_t)e] = x[e] - lse;
            if (logp_out)
                for (int e = 0; e < V; ++e) logp_out[r * logp_ld + e] = lp[(size_t)e];
            if (!(step > 0 || w == 0)) continue;
            const float sp = step > 0 ? score_prev[(long)b * prev_ld + w] : 0.0f;
            if (step > 0 && eos >= 0 && token_prev[(long)b * prev_ld + w] == eos) {
                cand.push_back(pack(sp, w * V + eos, n));
                continue;
            }
            for (int e = 0; e < V; ++e) cand.push_back(pack(sp + lp[(size_t)e], w * V + e, n));
        }
        std::partial_sort(cand.begin(), cand.begin() + W, cand.end(), [](uint64_t a, uint64_t c) { return a > c; });
        for (int j = 0; j < W; ++j) {
            const uint32_t lo = std::min((uint32_t)cand[(size_t)j], (uint32_t)(n - 1));
            const int i = n - 1 - (int)lo;
            score[(long)b * out_ld + j] = unkey((uint32_t)(cand[(size_t)j] >> 32));
            parent[(long)b * out_ld + j] = std::min(std::max(i / V, 0), W - 1);
            token[(long)b * out_ld + j] = std::min(std::max(i % V, 0), V - 1);
        }
    }
    return FN_OK;
}

inline int beam_gather(const FnBeamGatherJob* jobs, int n_jobs, int rows, int W, const int32_t* parent) {
    if (!jobs || !parent) return FN_E_NULL;
    if (n_jobs < 1 || n_jobs > FN_BEAM_GATHER_MAX_JOBS) return FN_E_COUNT;
    if (rows < 1 || W < 1 || W > FN_BEAM_MAX_W || rows % W != 0) return FN_E_SHAPE;
    for (int k = 0; k < n_jobs; ++k) {
        if (!jobs[k].src || !jobs[k].dst) return FN_E_NULL;
        if (jobs[k].cols < 1 || jobs[k].src_ld < jobs[k].cols || jobs[k].dst_ld < jobs[k].cols || jobs[k].src == jobs[k].dst) return FN_E_SHAPE;
    }
    for (int k = 0; k < n_jobs; ++k)
        for (long r = 0; r < rows; ++r) {
            const int p = std::min(std::max(parent[r], 0), W - 1);
            const float* s = jobs[k].src + ((r / W) * W + p) * (long)jobs[k].src_ld;
            float* d = jobs[k].dst + r * (long)jobs[k].dst_ld;
            for (int c = 0; c < jobs[k].cols; ++c) d[c] = s[c];
        }
    return FN_OK;
}

inline int beam_backtrack(const int32_t* parent, const int32_t* token, const float* score, int steps, int B, int W, int eos, int32_t* tokens_out,
                          int32_t* beam_out, float* cum_out, int32_t* len_out, float* score_out) {
    if (!parent || !token || !score || !tokens_out || !len_out || !score_out) return FN_E_NULL;
    if (steps < 1 || B < 1 || W < 1 || W > FN_BEAM_MAX_W || eos < -1) return FN_E_SHAPE;
    const long slab = (long)B * W;
    for (long h = 0; h < slab; ++h) {
        const long b = h / W;
        int cur = (int)(h % W), first = -1;
        score_out[h] = score[(steps - 1) * slab + h];
        for (int t = steps - 1; t >= 0; --t) {
            const long i = t * slab + b * W + cur;
            const int p = std::min(std::max(parent[i], 0), W - 1);
            tokens_out[h * steps + t] = token[i];
            if (cum_out) cum_out[h * steps + t] = score[i];
            if (beam_out) beam_out[h * steps + t] = p;
            if (eos >= 0 && token[i] == eos) first = t;
            cur = p;
        }
        len_out[h] = first >= 0 ? first + 1 : steps;
    }
    return FN_OK;
}

}  // namespace fn_beam_host
#endif
