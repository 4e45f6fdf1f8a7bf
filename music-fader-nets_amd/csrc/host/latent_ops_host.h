// latent_ops_host.h - fn_latent_draw / fn_latent_mix in plain C++ (include/fadernets.h has the definitions these follow step by step).  No dependencies:
// fadernets_host.cpp and the stand-alone latent_ops_check.cpp include it for the twins, csrc/latent_ops.hip for the argument checks and the column plan
// of the mix, which the device entry points share with the twins.  The Philox rounds are sample_host.h's.
#ifndef FADERNETS_LATENT_OPS_HOST_H
#define FADERNETS_LATENT_OPS_HOST_H

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../../include/fadernets.h"
#include "sample_host.h"

namespace fn_latent_host {

constexpr int MIX_COPY = 3;                       // the plan's own mode: columns in no segment, written as a's
constexpr int MIX_PLAN_MAX = 2 * FN_MIX_MAX_SEGS + 1;

inline bool aligned4(const void* p) { return (uintptr_t)p % 4 == 0; }

// ---- fn_latent_draw ----
inline int draw_check(const FnDrawJob* jobs, int n_jobs, int rows, int Z, int64_t z_ld, const FnDrawParams* params) {
    if (!jobs || !params) return FN_E_NULL;
    const int n = n_jobs < FN_DRAW_MAX_JOBS ? n_jobs : FN_DRAW_MAX_JOBS;
    for (int k = 0; k < n; ++k)
        if (!jobs[k].mu_lk || !jobs[k].lv_lk || !jobs[k].z) return FN_E_NULL;
    if (n_jobs < 1 || n_jobs > FN_DRAW_MAX_JOBS) return FN_E_COUNT;
    if (rows < 1 || Z < 1 || z_ld < Z) return FN_E_SHAPE;
    for (int k = 0; k < n; ++k)
        if (jobs[k].K < 1 || jobs[k].stream_id < 0 || jobs[k].stream_id >= 65535) return FN_E_SHAPE;
    if (Z > FN_DRAW_MAX_Z || (int64_t)rows * ((Z + 3) / 4) > INT32_MAX) return FN_E_UNSUPPORTED;
    for (int k = 0; k < n; ++k)
        if (jobs[k].K > FN_DRAW_MAX_K) return FN_E_UNSUPPORTED;
    if (!aligned4(params)) return FN_E_ALIGN;
    for (int k = 0; k < n; ++k) {
        const FnDrawJob& j = jobs[k];
        if (!aligned4(j.mu_lk) || !aligned4(j.lv_lk) || !aligned4(j.comp) || !aligned4(j.z) || !aligned4(j.eps_out) || !aligned4(j.comp_out)) return FN_E_ALIGN;
    }
    return FN_OK;
}

inline float clamp_tau(float tau) {
    if (tau != tau) tau = 1.0f;
    return std::fmin(std::fmax(tau, 0.0f), FLT_MAX);
}

// cos(pi x), sin(pi x) for x in [0, 2): x is cut at the nearest multiple of 1/2 (exact in binary), so the zeros and ones are exact
inline void sincospi(double x, double* s, double* c) {
    const int k = (int)std::floor(2.0 * x + 0.5);
    const double y = M_PI * (x - 0.5 * k), sy = std::sin(y), cy = std::cos(y);
    switch (k & 3) {
        case 0: *s = sy, *c = cy; break;
        case 1: *s = cy, *c = -sy; break;
        case 2: *s = -sy, *c = -cy; break;
        default: *s = -cy, *c = sy; break;
    }
}

// step 2: four Philox words -> four normals.  In double, rounded once: the definition's fp32 steps lie within its stated bounds of this
inline void quad_normals(const uint32_t w[4], float n[4]) {
    for (int h = 0; h < 2; ++h) {
        const float ua = (float)((w[2 * h] >> 8) + 1u) * 0x1p-24f, ub = (float)(w[2 * h + 1] >> 8) * 0x1p-24f;
        const double r = std::sqrt(-2.0 * std::log((double)ua));
        double s, c;
        sincospi(2.0 * (double)ub, &s, &c);
        n[2 * h] = (float)(r * c);
        n[2 * h + 1] = (float)(r * s);
    }
}

inline int latent_draw(const FnDrawJob* jobs, int n_jobs, int rows, int Z, int64_t z_ld, const FnDrawParams* params) {
    const int rc = draw_check(jobs, n_jobs, rows, Z, z_ld, params);
    if (rc != FN_OK) return rc;
    const FnDrawParams p = *params;
    const uint32_t key[2] = {p.seed_lo, p.seed_hi};
    const double tau = clamp_tau(p.tau);
    for (int s = 0; s < n_jobs; ++s) {
        const FnDrawJob& j = jobs[s];
        const uint32_t sid = (uint32_t)j.stream_id << 16;
        for (int b = 0; b < rows; ++b) {
            int k = j.comp ? j.comp[b] : -1;
            if (k < 0) {
                const uint32_t ctr[4] = {(uint32_t)b, sid | 0xFFFFu, p.offset_lo, p.offset_hi};
                uint32_t w[4];
                fn_sample_host::philox4x32_10(ctr, key, w);
                k = (int)(((uint64_t)(w[0] >> 8) * (uint64_t)j.K) >> 24);
            }
            if (k > j.K - 1) k = j.K - 1;
            if (j.comp_out) j.comp_out[b] = k;
            for (int q = 0; 4 * q < Z; ++q) {
                const uint32_t ctr[4] = {(uint32_t)b, sid | (uint32_t)q, p.offset_lo, p.offset_hi};
                uint32_t w[4];
                float n[4];
                fn_sample_host::philox4x32_10(ctr, key, w);
                quad_normals(w, n);
                for (int c = 0; c < 4 && 4 * q + c < Z; ++c) {
                    const int col = 4 * q + c;
                    const double mu = j.mu_lk[(size_t)k * Z + col], lv = j.lv_lk[(size_t)k * Z + col];
                    j.z[(int64_t)b * z_ld + col] = (float)(mu + (tau * std::exp(0.5 * lv)) * (double)n[c]);
                    if (j.eps_out) j.eps_out[(int64_t)b * Z + col] = n[c];
                }
            }
        }
    }
    return FN_OK;
}

// ---- fn_latent_mix ----
// the columns of a row as the kernel walks them: the caller's n_segs segments in the caller's order, then what they leave of [0, D) as MIX_COPY
struct MixPlan {
    FnMixSeg seg[MIX_PLAN_MAX];
    int n_segs, n_all;
};

inline int mix_check(const float* a, const float* b, int64_t ab_ld, int pairs, int D, const float* t, int P, const FnMixSeg* segs, int n_segs,
                     const float* out, int64_t out_ld, const float* omega_out, MixPlan* plan) {
    if (!a || !b || !t || !segs || !out) return FN_E_NULL;
    if (n_segs < 1 || n_segs > FN_MIX_MAX_SEGS) return FN_E_COUNT;
    if (pairs < 1 || D < 1 || P < 1 || ab_ld < D || out_ld < D) return FN_E_SHAPE;
    FnMixSeg by_off[FN_MIX_MAX_SEGS];
    for (int g = 0; g < n_segs; ++g) {
        const FnMixSeg& s = segs[g];
        if (s.off < 0 || s.len < 1 || s.off > D - s.len || s.mode < FN_MIX_LERP || s.mode > FN_MIX_STEP) return FN_E_SHAPE;
        for (int h = 0; h < g; ++h)
            if (s.off < segs[h].off + segs[h].len && segs[h].off < s.off + s.len) return FN_E_SHAPE;
        int at = g;                                 // insertion by offset
        while (at > 0 && by_off[at - 1].off > s.off) by_off[at] = by_off[at - 1], --at;
        by_off[at] = s;
        plan->seg[g] = s;
    }
    if ((int64_t)pairs * P > INT32_MAX) return FN_E_UNSUPPORTED;
    if (!aligned4(a) || !aligned4(b) || !aligned4(t) || !aligned4(out) || !aligned4(omega_out)) return FN_E_ALIGN;
    plan->n_segs = plan->n_all = n_segs;
    int pos = 0;
    for (int g = 0; g <= n_segs; ++g) {
        const int end = g < n_segs ? by_off[g].off : D;
        if (end > pos) plan->seg[plan->n_all++] = FnMixSeg{pos, end - pos, MIX_COPY, 0};
        if (g < n_segs) pos = by_off[g].off + by_off[g].len;
    }
    return FN_OK;
}

inline int latent_mix(const float* a, const float* b, int64_t ab_ld, int pairs, int D, const float* t, int P, int t_per_pair, const FnMixSeg* segs,
                      int n_segs, float* out, int64_t out_ld, float* omega_out) {
    MixPlan plan;
    const int rc = mix_check(a, b, ab_ld, pairs, D, t, P, segs, n_segs, out, out_ld, omega_out, &plan);
    if (rc != FN_OK) return rc;
    for (int i = 0; i < pairs; ++i)
        for (int g = 0; g < plan.n_all; ++g) {
            const FnMixSeg& sg = plan.seg[g];
            const float *x = a + (int64_t)i * ab_ld + sg.off, *y = b + (int64_t)i * ab_ld + sg.off;
            float om = 0.0f, s = 0.0f;
            bool slerp = false;
            if (sg.mode == FN_MIX_SLERP) {
                float saa = 0.0f, sbb = 0.0f, sab = 0.0f;
                for (int j = 0; j < sg.len; ++j) saa += x[j] * x[j], sbb += y[j] * y[j], sab += x[j] * y[j];
                const float na = std::sqrt(saa), nb = std::sqrt(sbb);
                const float c = std::fmin(std::fmax((float)((double)sab / std::sqrt((double)saa * (double)sbb)), -1.0f), 1.0f);
                om = std::acos(c);
                s = std::sin(om);
                slerp = na != 0.0f && nb != 0.0f && s >= FN_MIX_MIN_SIN;          // a NaN compares false
                if (!slerp) om = -1.0f;
            }
            if (omega_out && g < plan.n_segs) omega_out[(int64_t)i * plan.n_segs + g] = om;
            for (int p = 0; p < P; ++p) {
                const float tt = t[t_per_pair ? (int64_t)i * P + p : p];
                float* o = out + ((int64_t)i * P + p) * out_ld + sg.off;
                if (slerp) {
                    const float wa = std::sin((1.0f - tt) * om) / s, wb = std::sin(tt * om) / s;
                    for (int j = 0; j < sg.len; ++j) o[j] = std::fma(wb, y[j], wa * x[j]);
                } else if (sg.mode == FN_MIX_STEP) {
                    for (int j = 0; j < sg.len; ++j) o[j] = tt < 0.5f ? x[j] : y[j];
                } else if (sg.mode == MIX_COPY) {
                    for (int j = 0; j < sg.len; ++j) o[j] = x[j];
                } else {
                    for (int j = 0; j < sg.len; ++j) o[j] = std::fma(tt, y[j], (1.0f - tt) * x[j]);
                }
            }
        }
    return FN_OK;
}

}  // namespace fn_latent_host
#endif
