// likelihood_host.h - fn_posterior_draw / fn_iw_reduce in plain C++ (include/fadernets.h has the definitions these follow step by step, in the stated
// orders of every sum).  No dependencies: fadernets_host.cpp and the stand-alone likelihood_check.cpp include it for the twins, csrc/likelihood.hip for
// the argument checks the device entry points share with them.  The normals are latent_ops_host.h's, the ones fn_latent_draw's twin draws.
#ifndef FADERNETS_LIKELIHOOD_HOST_H
#define FADERNETS_LIKELIHOOD_HOST_H

#include <cmath>
#include <cstdint>

#include "../../../include/fadernets.h"
#include "latent_ops_host.h"

namespace fn_lik_host {

constexpr double LOG_2PI = 1.8378770664093454835606594728112;

inline bool aligned8(const void* p) { return (uintptr_t)p % 8 == 0; }
using fn_latent_host::aligned4;

// the xor butterfly of fn_wave_sum_f64 over the 64 lanes' partial sums (every lane ends with the same value: fp addition commutes)
inline double wave_sum(const double part[64]) {
    double s[64], t[64];
    for (int l = 0; l < 64; ++l) s[l] = part[l];
    for (int o = 32; o > 0; o >>= 1) {
        for (int l = 0; l < 64; ++l) t[l] = s[l] + s[l ^ o];
        for (int l = 0; l < 64; ++l) s[l] = t[l];
    }
    return s[0];
}

inline double wave_max(const double part[64]) {
    double m = part[0];
    for (int l = 1; l < 64; ++l) m = std::fmax(m, part[l]);          // the maximum does not depend on the order
    return m;
}

// ---- fn_posterior_draw ----
inline int post_check(const FnPostJob* jobs, int n_jobs, int B, int S, int Z, int64_t z_ld, const FnDrawParams* params) {
    if (!jobs || !params) return FN_E_NULL;
    const int n = n_jobs < FN_DRAW_MAX_JOBS ? n_jobs : FN_DRAW_MAX_JOBS;
    for (int k = 0; k < n; ++k)
        if (!jobs[k].pre || !jobs[k].mu_lk || !jobs[k].lv_lk || !jobs[k].z || !jobs[k].logq || !jobs[k].logp) return FN_E_NULL;
    if (n_jobs < 1 || n_jobs > FN_DRAW_MAX_JOBS) return FN_E_COUNT;
    if (B < 1 || S < 1 || Z < 1 || z_ld < Z) return FN_E_SHAPE;
    for (int k = 0; k < n; ++k)
        if (jobs[k].K < 1 || jobs[k].stream_id < 0 || jobs[k].stream_id >= 65535) return FN_E_SHAPE;
    for (int k = 0; k < n; ++k)
        if (jobs[k].K > FN_POST_MAX_K) return FN_E_UNSUPPORTED;
    if (Z > FN_DRAW_MAX_Z || (int64_t)B * S > INT32_MAX) return FN_E_UNSUPPORTED;
    if (!aligned4(params)) return FN_E_ALIGN;
    for (int k = 0; k < n; ++k) {
        const FnPostJob& j = jobs[k];
        if (!aligned4(j.pre) || !aligned4(j.mu_lk) || !aligned4(j.lv_lk) || !aligned4(j.z) || !aligned4(j.eps_out) || !aligned8(j.logq) || !aligned8(j.logp))
            return FN_E_ALIGN;
    }
    return FN_OK;
}

inline int posterior_draw(const FnPostJob* jobs, int n_jobs, int B, int S, int Z, int64_t z_ld, const FnDrawParams* params) {
    const int rc = post_check(jobs, n_jobs, B, S, Z, z_ld, params);
    if (rc != FN_OK) return rc;
    const FnDrawParams p = *params;
    const uint32_t key[2] = {p.seed_lo, p.seed_hi};
    const float tau = fn_latent_host::clamp_tau(p.tau);
    const uint64_t offset = ((uint64_t)p.offset_hi << 32) | p.offset_lo;
    for (int e = 0; e < n_jobs; ++e) {
        const FnPostJob& j = jobs[e];
        const uint32_t sid = (uint32_t)j.stream_id << 16;
        const double logpk = std::log(1.0 / (double)j.K);
        for (int b = 0; b < B; ++b)
            for (int s = 0; s < S; ++s) {
                const int64_t i = (int64_t)b * S + s;
                const uint64_t off = offset + (uint64_t)s;                                  // wraps
                const float *mu = j.pre + (int64_t)b * 2 * Z, *v = mu + Z;
                float* z = j.z + i * z_ld;
                double accq[64], acck[FN_POST_MAX_K][64];
                for (int l = 0; l < 64; ++l) {
                    accq[l] = 0.0;
                    for (int k = 0; k < j.K; ++k) acck[k][l] = 0.0;
                }
                for (int q = 0; 4 * q < Z; ++q) {
                    const uint32_t ctr[4] = {(uint32_t)b, sid | (uint32_t)q, (uint32_t)off, (uint32_t)(off >> 32)};
                    uint32_t w[4];
                    float n[4];
                    fn_sample_host::philox4x32_10(ctr, key, w);
                    fn_latent_host::quad_normals(w, n);
                    for (int c = 0; c < 4 && 4 * q + c < Z; ++c) {
                        const int col = 4 * q + c, l = col & 63;                             // ascending columns: lane l adds l, l + 64, ... in order
                        const float sg = tau * (float)std::exp((double)v[col]);
                        const float zz = mu[col] + sg * n[c];
                        z[col] = zz;
                        if (j.eps_out) j.eps_out[i * Z + col] = n[c];
                        const double d = ((double)zz - (double)mu[col]) / (double)sg;
                        accq[l] += -0.5 * (d * d + LOG_2PI) - std::log((double)sg);
                        for (int k = 0; k < j.K; ++k) {
                            const double lv = (double)j.lv_lk[(size_t)k * Z + col], dz = (double)zz - (double)j.mu_lk[(size_t)k * Z + col];
                            acck[k][l] += -0.5 * (dz * dz * std::exp(-lv) + lv + LOG_2PI);
                        }
                    }
                }
                j.logq[i] = wave_sum(accq);
                double ll[FN_POST_MAX_K], m = -INFINITY;
                for (int k = 0; k < j.K; ++k) {
                    ll[k] = wave_sum(acck[k]) + logpk;
                    m = std::fmax(m, ll[k]);
                }
                double den = 0.0;
                for (int k = 0; k < j.K; ++k) den += std::exp(ll[k] - m);
                j.logp[i] = m + std::log(den);
            }
    }
    return FN_OK;
}

// ---- fn_iw_reduce ----
inline int iw_check(const float* nll_tb, int T, int64_t nll_ld, const int32_t* t0, const int32_t* t1, const double* logp_z, const double* logq_z, int n_lat,
                    int64_t lat_stride, int B, int S, const double* lw, const double* out, int out_ld) {
    if (!nll_tb || !logp_z || !logq_z || !lw || !out || (t0 == nullptr) != (t1 == nullptr)) return FN_E_NULL;
    if (n_lat < 1 || n_lat > FN_IW_MAX_LAT) return FN_E_COUNT;
    if (B < 1 || S < 1 || T < 1 || nll_ld < (int64_t)B * S || lat_stride < (int64_t)B * S || out_ld < FN_IW_COLS + n_lat) return FN_E_SHAPE;
    if ((int64_t)B * S > INT32_MAX) return FN_E_UNSUPPORTED;
    if (!aligned4(nll_tb) || !aligned4(t0) || !aligned4(t1) || !aligned8(logp_z) || !aligned8(logq_z) || !aligned8(lw) || !aligned8(out)) return FN_E_ALIGN;
    return FN_OK;
}

inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

inline int iw_reduce(const float* nll_tb, int T, int64_t nll_ld, const int32_t* t0, const int32_t* t1, const double* logp_z, const double* logq_z, int n_lat,
                     int64_t lat_stride, int B, int S, double* lw, double* out, int out_ld) {
    const int rc = iw_check(nll_tb, T, nll_ld, t0, t1, logp_z, logq_z, n_lat, lat_stride, B, S, lw, out, out_ld);
    if (rc != FN_OK) return rc;
    for (int b = 0; b < B; ++b) {
        const int ta = t0 ? clampi(t0[b], 0, T) : 0, tb = t0 ? clampi(t1[b], 0, T) : T;
        double mx[64], slw[64], srec[64], skl[FN_IW_MAX_LAT][64], w1[64], w2[64];
        for (int l = 0; l < 64; ++l) {
            mx[l] = -INFINITY, slw[l] = srec[l] = w1[l] = w2[l] = 0.0;
            for (int e = 0; e < n_lat; ++e) skl[e][l] = 0.0;
        }
        for (int s = 0; s < S; ++s) {
            const int l = s & 63;
            const int64_t i = (int64_t)b * S + s;
            double nl = 0.0;
            for (int t = ta; t < tb; ++t) nl += (double)nll_tb[(int64_t)t * nll_ld + i];
            const double recon = -nl;
            double w = recon;
            for (int e = 0; e < n_lat; ++e) {
                const double lp = logp_z[e * lat_stride + i], lq = logq_z[e * lat_stride + i];
                w += lp - lq;
                skl[e][l] += lq - lp;
            }
            lw[i] = w;
            mx[l] = std::fmax(mx[l], w), slw[l] += w, srec[l] += recon;
        }
        const double m = wave_max(mx), sum_lw = wave_sum(slw), sum_rec = wave_sum(srec);
        double* o = out + (int64_t)b * out_ld;
        o[1] = sum_lw / (double)S;
        o[3] = sum_rec / (double)S;
        for (int e = 0; e < n_lat; ++e) o[FN_IW_COLS + e] = wave_sum(skl[e]) / (double)S;
        if (m == -INFINITY) {
            o[0] = o[1] = -INFINITY, o[2] = 0.0;
            continue;
        }
        for (int s = 0; s < S; ++s) {
            const double x = std::exp(lw[(int64_t)b * S + s] - m);
            w1[s & 63] += x, w2[s & 63] += x * x;
        }
        const double W1 = wave_sum(w1), W2 = wave_sum(w2);
        o[0] = m + std::log(W1) - std::log((double)S);
        o[2] = W1 * W1 / W2;
    }
    return FN_OK;
}

}  // namespace fn_lik_host
#endif
