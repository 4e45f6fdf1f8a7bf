// likelihood.hip - the device side of the importance-weighted log-likelihood (likelihood.py): fn_posterior_draw samples q(z|x) S times per piece into the
// teacher-forced decoder's latent rows and evaluates log q(z|x) and the mixture log p(z) at the stored z in fp64; fn_iw_reduce turns the decoder's per-token
// nll and those densities into the per-sample log-weights and reduces them per piece.  OURS - the reference has neither; include/fadernets.h has the
// definitions.  The argument checks are host/likelihood_host.h's, shared with the host twins.
#include <cfloat>

#include "common.h"
#include "host/likelihood_host.h"

namespace {

constexpr double LOG_2PI = fn_lik_host::LOG_2PI;
constexpr int KMAX = FN_POST_MAX_K;

struct PostArgs {
    FnPostJob job[FN_DRAW_MAX_JOBS];
};

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// one wavefront per (b, s) row, 4 rows per workgroup (no barrier: a wavefront past the last row leaves), blockIdx.y = job.  Lane l owns the columns
// l, l + 64, ...: it draws the quad of its column (four lanes draw the same quad - the rounds are cheap beside the fp64 densities) and keeps one term
// of every sum per column.
__global__ __launch_bounds__(256) void posterior_draw_kernel(PostArgs a, long rows, int S, int Z, long z_ld, const FnDrawParams* __restrict__ params) {
    const FnPostJob jb = a.job[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const int b = (int)(i / S), s = (int)(i % S);
    const FnDrawParams pr = *params;
    float tau = pr.tau;
    if (tau != tau) tau = 1.0f;
    tau = fminf(fmaxf(tau, 0.0f), FLT_MAX);
    const unsigned long long off = (((unsigned long long)pr.offset_hi << 32) | pr.offset_lo) + (unsigned long long)s;          // wraps
    const uint32_t sid = (uint32_t)jb.stream_id << 16;
    const int K = jb.K;
    const float *mu = jb.pre + (long)b * 2 * Z, *v = mu + Z;
    double accq = 0.0, acck[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) acck[k] = 0.0;
    for (int j = lane; j < Z; j += 64) {
        uint32_t w[4];
        fn_philox4x32_10((uint32_t)b, sid | (uint32_t)(j >> 2), (uint32_t)off, (uint32_t)(off >> 32), pr.seed_lo, pr.seed_hi, w);
        float n[4];
        fn_quad_normals(w, n);
        const int c = j & 3;
        const float eps = c == 0 ? n[0] : (c == 1 ? n[1] : (c == 2 ? n[2] : n[3]));
        const float m = mu[j];
        const float sg = tau * expf(v[j]);
        const float zz = m + sg * eps;
        jb.z[i * z_ld + j] = zz;
        if (jb.eps_out) jb.eps_out[i * Z + j] = eps;
        const double d = ((double)zz - (double)m) / (double)sg;
        accq += -0.5 * (d * d + LOG_2PI) - log((double)sg);
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (k < K) {
                const double lv = (double)jb.lv_lk[(long)k * Z + j], dz = (double)zz - (double)jb.mu_lk[(long)k * Z + j];
                acck[k] += -0.5 * (dz * dz * exp(-lv) + lv + LOG_2PI);
            }
        }
    }
    accq = fn_wave_sum_f64(accq);
    const double logpk = log(1.0 / (double)K);
    double mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k < K) {
            acck[k] = fn_wave_sum_f64(acck[k]) + logpk;
            mx = fmax(mx, acck[k]);
        }
    }
    double den = 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < K) den += exp(acck[k] - mx);
    if (lane == 0) {
        jb.logq[i] = accq;
        jb.logp[i] = mx + log(den);
    }
}

// one wavefront per source row b, 4 per workgroup.  Lane l owns the samples s = l, l + 64, ...: consecutive lanes read consecutive floats of a step's nll.
// lw is not __restrict__: the second pass re-reads what the same lane stored in the first.
__global__ __launch_bounds__(256) void iw_reduce_kernel(const float* __restrict__ nll_tb, int T, long nll_ld, const int* __restrict__ t0,
                                                        const int* __restrict__ t1, const double* __restrict__ logp_z, const double* __restrict__ logq_z,
                                                        int n_lat, long lat_stride, int B, int S, double* lw, double* __restrict__ out, int out_ld) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    int ta = 0, tb = T;
    if (t0) ta = min(max(t0[b], 0), T), tb = min(max(t1[b], 0), T);
    double mx = -INFINITY, slw = 0.0, srec = 0.0, skl[FN_IW_MAX_LAT];
#pragma unroll
    for (int e = 0; e < FN_IW_MAX_LAT; ++e) skl[e] = 0.0;
    for (int s = lane; s < S; s += 64) {
        const long i = (long)b * S + s;
        double nl = 0.0;
        for (int t = ta; t < tb; ++t) nl += (double)nll_tb[(long)t * nll_ld + i];
        const double recon = -nl;
        double w = recon;
#pragma unroll
        for (int e = 0; e < FN_IW_MAX_LAT; ++e) {
            if (e < n_lat) {
                const double lp = logp_z[e * lat_stride + i], lq = logq_z[e * lat_stride + i];
                w += lp - lq;
                skl[e] += lq - lp;
            }
        }
        lw[i] = w;
        mx = fmax(mx, w), slw += w, srec += recon;
    }
    const double m = wave_max_f64(mx);
    slw = fn_wave_sum_f64(slw), srec = fn_wave_sum_f64(srec);
#pragma unroll
    for (int e = 0; e < FN_IW_MAX_LAT; ++e)
        if (e < n_lat) skl[e] = fn_wave_sum_f64(skl[e]);
    double* o = out + (long)b * out_ld;
    if (lane == 0) {
        o[1] = slw / (double)S;
        o[3] = srec / (double)S;
#pragma unroll
        for (int e = 0; e < FN_IW_MAX_LAT; ++e)
            if (e < n_lat) o[FN_IW_COLS + e] = skl[e] / (double)S;
    }
    if (m == -INFINITY) {          // the same in every lane
        if (lane == 0) o[0] = o[1] = -INFINITY, o[2] = 0.0;
        return;
    }
    double w1 = 0.0, w2 = 0.0;
    for (int s = lane; s < S; s += 64) {
        const double x = exp(lw[(long)b * S + s] - m);
        w1 += x, w2 += x * x;
    }
    w1 = fn_wave_sum_f64(w1), w2 = fn_wave_sum_f64(w2);
    if (lane == 0) {
        o[0] = m + log(w1) - log((double)S);
        o[2] = w1 * w1 / w2;
    }
}

}  // namespace

extern "C" {

int fn_posterior_draw(const FnPostJob* jobs, int n_jobs, int B, int S, int Z, int64_t z_ld, const FnDrawParams* params_dev, void* stream) {
    const int rc = fn_lik_host::post_check(jobs, n_jobs, B, S, Z, z_ld, params_dev);
    if (rc != FN_OK) return rc;
    PostArgs a = {};
    for (int k = 0; k < n_jobs; ++k) a.job[k] = jobs[k];
    const long rows = (long)B * S;
    hipLaunchKernelGGL(posterior_draw_kernel, dim3((unsigned)((rows + 3) / 4), (unsigned)n_jobs), dim3(256), 0, (hipStream_t)stream, a, rows, S, Z, (long)z_ld,
                       params_dev);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

int fn_iw_reduce(const float* nll_tb, int T, int64_t nll_ld, const int32_t* t0, const int32_t* t1, const double* logp_z, const double* logq_z, int n_lat,
                 int64_t lat_stride, int B, int S, double* lw, double* out, int out_ld, void* stream) {
    const int rc = fn_lik_host::iw_check(nll_tb, T, nll_ld, t0, t1, logp_z, logq_z, n_lat, lat_stride, B, S, lw, out, out_ld);
    if (rc != FN_OK) return rc;
    hipLaunchKernelGGL(iw_reduce_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, nll_tb, T, (long)nll_ld, t0, t1, logp_z, logq_z,
                       n_lat, (long)lat_stride, B, S, lw, out, out_ld);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

}  // extern "C"
