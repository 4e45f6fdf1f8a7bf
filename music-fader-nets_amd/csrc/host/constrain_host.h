// constrain_host.h - the arithmetic of fn_constrain_apply / fn_constrain_advance in plain C++ (include/fadernets.h has the definition these follow
// clause by clause).  No dependencies: the stand-alone constrain_check.cpp includes it, fadernets_host.cpp exports it as the *_host twins.  One fp32
// add and selects: the results are the kernels' bit for bit.
#ifndef FADERNETS_CONSTRAIN_HOST_H
#define FADERNETS_CONSTRAIN_HOST_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../../include/fadernets.h"

namespace fn_constrain_host {

inline int n_pitch(const FnConstrainParams& p) { return std::min(std::max(p.n_pitch, 0), FN_CONSTRAIN_MAX_PITCH); }

// pitch of token e in the range that starts at lo, or -1
inline int pitch(int e, int lo, int n) {
    const int64_t p = (int64_t)e - (int64_t)lo;
    return (p >= 0 && p < n) ? (int)p : -1;
}

inline bool sounds(const uint32_t* h, int p) { return (h[p >> 5] >> (p & 31)) & 1u; }

inline int constrain_apply(float* logits, int rows, int V, int ld, int step, const FnConstrainParams* params, const float* bias, int64_t bias_rs,
                           const uint32_t* held, int32_t* stuck) {
    if (!logits || !params) return FN_E_NULL;
    if (rows < 1 || V < 1 || V > FN_SAMPLE_MAX_V || ld < V || step < 0 || (bias && bias_rs != 0 && bias_rs < V)) return FN_E_SHAPE;
    const FnConstrainParams c = *params;
    const int n = n_pitch(c);
    const float ninf = -std::numeric_limits<float>::infinity();
    std::vector<float> y((size_t)V);
    std::vector<char> g((size_t)V);
    for (int64_t r = 0; r < rows; ++r) {
        float* x = logits + r * ld;
        for (int e = 0; e < V; ++e) y[e] = bias ? x[e] + bias[r * bias_rs + e] : x[e];
        std::fill(g.begin(), g.end(), 0);
        if (c.eos >= 0 && c.eos < V && step < c.min_len) g[c.eos] = 1;
        if (held && n > 0) {
            const uint32_t* h = held + r * 4;
            int count = 0;
            for (int k = 0; k < 4; ++k)
                for (uint32_t w = h[k]; w; w &= w - 1) ++count;
            const bool full = c.max_poly > 0 && count >= c.max_poly;
            for (int e = 0; e < V; ++e) {
                int p = pitch(e, c.on_lo, n);
                if (p >= 0) {
                    if (sounds(h, p) ? (c.flags & FN_CONSTRAIN_NO_REONSET) != 0 : full) g[e] = 1;
                } else if ((p = pitch(e, c.off_lo, n)) >= 0) {
                    if ((c.flags & FN_CONSTRAIN_OFF_NEEDS_ON) && !sounds(h, p)) g[e] = 1;
                }
            }
        }
        bool left = false;
        for (int e = 0; e < V; ++e) left = left || (y[e] > ninf && !g[e]);
        if (!left && stuck) stuck[r] += 1;
        for (int e = 0; e < V; ++e) x[e] = (left && g[e]) ? ninf : y[e];
    }
    return FN_OK;
}

inline int constrain_advance(int32_t* tok_io, int tok_ld, int rows, int V, const FnConstrainParams* params, const float* logits, int ld,
                             const int32_t* fallback, int fb_ld, const uint32_t* held_in, uint32_t* held_out, int32_t* fixed) {
    if (!tok_io || !params || (logits && !fallback) || (held_in && !held_out)) return FN_E_NULL;
    if (rows < 1 || V < 1 || V > FN_SAMPLE_MAX_V || tok_ld < 1 || (logits && (ld < V || fb_ld < 1))) return FN_E_SHAPE;
    const FnConstrainParams c = *params;
    const int n = n_pitch(c);
    const float ninf = -std::numeric_limits<float>::infinity();
    for (int64_t r = 0; r < rows; ++r) {
        int tok = tok_io[r * tok_ld];
        if (logits && (tok < 0 || tok >= V || logits[r * ld + tok] == ninf)) {
            tok = std::min(std::max(fallback[r * fb_ld], 0), V - 1);
            tok_io[r * tok_ld] = tok;
            if (fixed) fixed[r] += 1;
        }
        if (!held_in) continue;
        uint32_t h[4] = {held_in[r * 4 + 0], held_in[r * 4 + 1], held_in[r * 4 + 2], held_in[r * 4 + 3]};
        if (tok >= 0 && tok < V) {
            int p = pitch(tok, c.on_lo, n);
            if (p >= 0)
                h[p >> 5] |= 1u << (p & 31);
            else if ((p = pitch(tok, c.off_lo, n)) >= 0)
                h[p >> 5] &= ~(1u << (p & 31));
        }
        for (int k = 0; k < 4; ++k) held_out[r * 4 + k] = h[k];
    }
    return FN_OK;
}

}  // namespace fn_constrain_host

#endif
