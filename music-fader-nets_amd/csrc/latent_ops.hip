// latent_ops.hip - latent-side work in front of a decode (latent.py): fn_latent_draw samples z_r / z_n from a component of the mixture prior,
// fn_latent_mix interpolates the latents of two pieces.  OURS - the reference has neither; include/fadernets.h has the definitions.  The argument
// checks and the mix's column plan are host/latent_ops_host.h's, shared with the host twins.
#include <cfloat>

#include "common.h"
#include "host/latent_ops_host.h"

namespace {

struct DrawArgs {
    FnDrawJob job[FN_DRAW_MAX_JOBS];
};

// one thread per (row, quad of columns), blockIdx.y = job: a row's numbers depend on (row, column, stream, seed, offset) and on nothing of the launch
__global__ __launch_bounds__(256) void latent_draw_kernel(DrawArgs a, int rows, int Z, long z_ld, const FnDrawParams* __restrict__ params) {
    const FnDrawJob jb = a.job[blockIdx.y];
    const int nq = (Z + 3) >> 2;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)rows * nq) return;
    const int b = (int)(t / nq), q = (int)(t % nq);
    const FnDrawParams pr = *params;
    float tau = pr.tau;
    if (tau != tau) tau = 1.0f;
    tau = fminf(fmaxf(tau, 0.0f), FLT_MAX);
    const uint32_t sid = (uint32_t)jb.stream_id << 16;
    // 1. + 2. the quad's four words -> four normals
    uint32_t w[4];
    fn_philox4x32_10((uint32_t)b, sid | (uint32_t)q, pr.offset_lo, pr.offset_hi, pr.seed_lo, pr.seed_hi, w);
    float n[4];
    fn_quad_normals(w, n);
    // 3. the row's component: given, or drawn from the row's own counter
    int k = jb.comp ? jb.comp[b] : -1;
    if (k < 0) {
        uint32_t wk[4];
        fn_philox4x32_10((uint32_t)b, sid | 0xFFFFu, pr.offset_lo, pr.offset_hi, pr.seed_lo, pr.seed_hi, wk);
        k = (int)(((unsigned long long)(wk[0] >> 8) * (unsigned long long)jb.K) >> 24);
    }
    k = min(k, jb.K - 1);
    if (jb.comp_out && q == 0) jb.comp_out[b] = k;
    // 4. the quad's columns below Z
    const float *mu = jb.mu_lk + (long)k * Z, *lv = jb.lv_lk + (long)k * Z;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int j = 4 * q + c;
        if (j < Z) {
            jb.z[(long)b * z_ld + j] = mu[j] + (tau * expf(0.5f * lv[j])) * n[c];
            if (jb.eps_out) jb.eps_out[(long)b * Z + j] = n[c];
        }
    }
}

// one wavefront per pair, 4 pairs per workgroup (no barrier: a wavefront past the last pair leaves).  Per plan entry: the slice's three sums over
// the lanes (xor butterfly, the same in every lane), the angle, then the pair's P points.
__global__ __launch_bounds__(256) void latent_mix_kernel(const float* __restrict__ a, const float* __restrict__ b, long ab_ld, int pairs,
                                                         const float* __restrict__ t, int P, int t_per_pair, fn_latent_host::MixPlan plan,
                                                         float* __restrict__ out, long out_ld, float* __restrict__ omega_out) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= pairs) return;
    for (int g = 0; g < plan.n_all; ++g) {
        const FnMixSeg sg = plan.seg[g];
        const float *x = a + (long)i * ab_ld + sg.off, *y = b + (long)i * ab_ld + sg.off;
        float om = 0.0f, s = 0.0f;
        bool slerp = false;
        if (sg.mode == FN_MIX_SLERP) {
            float saa = 0.0f, sbb = 0.0f, sab = 0.0f;
            for (int j = lane; j < sg.len; j += 64) {
                const float xv = x[j], yv = y[j];
                saa += xv * xv, sbb += yv * yv, sab += xv * yv;
            }
            saa = fn_wave_sum(saa), sbb = fn_wave_sum(sbb), sab = fn_wave_sum(sab);
            const float na = sqrtf(saa), nb = sqrtf(sbb);
            const float c = fminf(fmaxf((float)((double)sab / sqrt((double)saa * (double)sbb)), -1.0f), 1.0f);          // fp64: a == +-b gives +-1 exactly
            om = acosf(c);
            s = sinf(om);
            slerp = na != 0.0f && nb != 0.0f && s >= FN_MIX_MIN_SIN;          // a NaN compares false
            if (!slerp) om = -1.0f;
        }
        if (omega_out && g < plan.n_segs && lane == 0) omega_out[(long)i * plan.n_segs + g] = om;
        for (int p = 0; p < P; ++p) {
            const float tt = t[t_per_pair ? (long)i * P + p : p];
            float* o = out + ((long)i * P + p) * out_ld + sg.off;
            if (slerp) {
                const float wa = sinf((1.0f - tt) * om) / s, wb = sinf(tt * om) / s;
                for (int j = lane; j < sg.len; j += 64) o[j] = fmaf(wb, y[j], wa * x[j]);
            } else if (sg.mode == FN_MIX_STEP) {
                for (int j = lane; j < sg.len; j += 64) o[j] = tt < 0.5f ? x[j] : y[j];
            } else if (sg.mode == fn_latent_host::MIX_COPY) {
                for (int j = lane; j < sg.len; j += 64) o[j] = x[j];
            } else {
                for (int j = lane; j < sg.len; j += 64) o[j] = fmaf(tt, y[j], (1.0f - tt) * x[j]);
            }
        }
    }
}

}  // namespace

extern "C" {

int fn_latent_draw(const FnDrawJob* jobs, int n_jobs, int rows, int Z, int64_t z_ld, const FnDrawParams* params_dev, void* stream) {
    const int rc = fn_latent_host::draw_check(jobs, n_jobs, rows, Z, z_ld, params_dev);
    if (rc != FN_OK) return rc;
    DrawArgs a = {};
    for (int k = 0; k < n_jobs; ++k) a.job[k] = jobs[k];
    const long threads = (long)rows * ((Z + 3) / 4);
    hipLaunchKernelGGL(latent_draw_kernel, dim3((unsigned)((threads + 255) / 256), (unsigned)n_jobs), dim3(256), 0, (hipStream_t)stream, a, rows, Z,
                       (long)z_ld, params_dev);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

int fn_latent_mix(const float* a, const float* b, int64_t ab_ld, int pairs, int D, const float* t, int P, int t_per_pair, const FnMixSeg* segs,
                  int n_segs, float* out, int64_t out_ld, float* omega_out, void* stream) {
    fn_latent_host::MixPlan plan = {};
    const int rc = fn_latent_host::mix_check(a, b, ab_ld, pairs, D, t, P, segs, n_segs, out, out_ld, omega_out, &plan);
    if (rc != FN_OK) return rc;
    hipLaunchKernelGGL(latent_mix_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a, b, (long)ab_ld, pairs, t, P,
                       t_per_pair ? 1 : 0, plan, out, (long)out_ld, omega_out);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

}  // extern "C"
