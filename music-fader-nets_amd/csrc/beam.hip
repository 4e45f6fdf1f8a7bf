// beam.hip - beam search beside the per-token decode launches (decode.beam_decode): the top-W selection over the W x V continuations of a
// sequence (fn_beam_step), the reorder of the decoder states by parent beam (fn_beam_gather) and the backtrack (fn_beam_backtrack).
// include/fadernets.h has the definition; there is no reference counterpart (gmm_model.py:73-80,119-149 feeds back one argmax stream).
// Plain HIP: no inline assembly, no hand-counted waits, no spins across workgroups, no atomics.
#include "common.h"

namespace {

// the score back from the high half of a word of fn_pack_best (common.h; here over n = W * V columns)
__device__ __forceinline__ float beam_unkey(uint32_t key) {
    return __uint_as_float(key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu));
}

// One workgroup of W wavefronts per sequence, wavefront w on beam row w: lane l holds e = l, l + 64, ... in NE registers, takes the row's lse from
// fn_row_head, packs its V candidates and leaves the row's own top W words (only they can reach the sequence's top W) in LDS by W rounds
// of wave-max with removal; a non-live row leaves W empty words (0: below every real candidate, whose key is at least key(-inf)), a finished row its
// one candidate.  After the barrier thread t < W * W ranks word t by counting the larger ones (the words of real candidates are distinct) and the
// threads of rank < W store the slabs.  (The row loop strides by the number of wavefronts, whatever the launch gives it.)
template <int NE>      // entries per lane: V <= 64 NE
__global__ __launch_bounds__(64 * FN_BEAM_MAX_W) void beam_step_kernel(const float* __restrict__ logits, int W, int V, int ld, int step, int eos,
                                                                        const float* __restrict__ score_prev, const int* __restrict__ token_prev,
                                                                        int prev_ld, float* __restrict__ score, int* __restrict__ parent,
                                                                        int* __restrict__ token, int out_ld, float* __restrict__ logp_out, long logp_ld) {
    __shared__ unsigned long long top[FN_BEAM_MAX_W * FN_BEAM_MAX_W];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    const int b = blockIdx.x;
    const int n = W * V;
    for (int w = wv; w < W; w += nwv) {
        const long r = (long)b * W + w;
        const float* x = logits + r * ld;
        const float lse = fn_row_head(x, V, lane).lse;          // lp = x[e] - lse, as vocab_argmax_kernel forms it
        if (logp_out)
            for (int e = lane; e < V; e += 64) logp_out[r * logp_ld + e] = x[e] - lse;
        const bool live = step > 0 || w == 0;
        const float sp = step > 0 ? score_prev[(long)b * prev_ld + w] : 0.0f;
        const bool finished = step > 0 && eos >= 0 && token_prev[(long)b * prev_ld + w] == eos;
        unsigned long long wd[NE];
#pragma unroll
        for (int k = 0; k < NE; ++k) {
            const int e = lane + 64 * k;
            wd[k] = (live && !finished && e < V) ? fn_pack_best(sp + (x[e] - lse), w * V + e, n) : 0ull;
        }
        if (finished && lane == 0) wd[0] = fn_pack_best(sp, w * V + eos, n);
        for (int j = 0; j < W; ++j) {
            unsigned long long m = wd[0];
#pragma unroll
            for (int k = 1; k < NE; ++k) m = wd[k] > m ? wd[k] : m;
            m = fn_wave_max_u64(m);
            // the low halves differ from candidate to candidate: exactly one register of one lane holds m (or m is the empty word)
#pragma unroll
            for (int k = 0; k < NE; ++k) wd[k] = wd[k] == m ? 0ull : wd[k];
            if (lane == 0) top[w * W + j] = m;
        }
    }
    __syncthreads();
    // at least W words are real candidates and so above 0: an empty word never ranks below W.  (Only a row of NaNs can make a real word 0; the threads
    // holding 0 then store the same in-range values.)
    const int t = threadIdx.x;
    if (t >= W * W) return;
    const unsigned long long mine = top[t];
    int rank = 0;
    for (int k = 0; k < W * W; ++k) rank += top[k] > mine ? 1 : 0;
    if (rank < W) {
        const int i = n - 1 - (int)min((uint32_t)mine, (uint32_t)(n - 1));      // in range whatever a row of NaNs left
        const long o = (long)b * out_ld + rank;
        score[o] = beam_unkey((uint32_t)(mine >> 32));
        parent[o] = min(max(i / V, 0), W - 1);
        token[o] = min(max(i % V, 0), V - 1);
    }
}

struct BeamGatherArgs {
    FnBeamGatherJob job[FN_BEAM_GATHER_MAX_JOBS];
    int vec[FN_BEAM_GATHER_MAX_JOBS];      // 1: src, dst 16-byte aligned and both leading dimensions multiples of 4
};

// one wavefront per (row, job): blockIdx.y = job, 4 rows per workgroup
__global__ __launch_bounds__(256) void beam_gather_kernel(BeamGatherArgs a, int rows, int W, const int* __restrict__ parent) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const FnBeamGatherJob j = a.job[blockIdx.y];
    const int p = min(max(parent[r], 0), W - 1);
    const float* s = j.src + ((r / W) * W + p) * (long)j.src_ld;
    float* d = j.dst + r * (long)j.dst_ld;
    int c0 = 0;
    if (a.vec[blockIdx.y]) {
        const int n4 = j.cols >> 2;
        for (int c = lane; c < n4; c += 64) reinterpret_cast<float4*>(d)[c] = reinterpret_cast<const float4*>(s)[c];
        c0 = n4 << 2;
    }
    for (int c = c0 + lane; c < j.cols; c += 64) d[c] = s[c];
}

// one thread per final hypothesis (b, j)
__global__ __launch_bounds__(256) void beam_backtrack_kernel(const int* __restrict__ parent, const int* __restrict__ token,
                                                             const float* __restrict__ score, int steps, int B, int W, int eos,
                                                             int* __restrict__ tokens_out, int* __restrict__ beam_out, float* __restrict__ cum_out,
                                                             int* __restrict__ len_out, float* __restrict__ score_out) {
    const long h = (long)blockIdx.x * 256 + threadIdx.x;
    if (h >= (long)B * W) return;
    const long b = h / W;
    int cur = (int)(h % W);
    const long slab = (long)B * W;
    score_out[h] = score[(steps - 1) * slab + h];
    int first = -1;
    for (int t = steps - 1; t >= 0; --t) {
        const long i = t * slab + b * W + cur;
        const int tk = token[i];
        const int p = min(max(parent[i], 0), W - 1);
        tokens_out[h * steps + t] = tk;
        if (cum_out) cum_out[h * steps + t] = score[i];
        if (beam_out) beam_out[h * steps + t] = p;
        if (eos >= 0 && tk == eos) first = t;
        cur = p;
    }
    len_out[h] = first >= 0 ? first + 1 : steps;
}

}  // namespace

extern "C" {

int fn_beam_step(const float* logits, int B, int W, int V, int ld, int step, int eos, const float* score_prev, const int32_t* token_prev,
                 int prev_ld, float* score, int32_t* parent, int32_t* token, int out_ld, float* logp_out, int64_t logp_ld, void* stream) {
    if (!logits || !score || !parent || !token) return FN_E_NULL;
    if (step > 0 && (!score_prev || !token_prev)) return FN_E_NULL;
    if (B < 1 || V < 1 || V > FN_SAMPLE_MAX_V || W < 1 || W > FN_BEAM_MAX_W || W > V || ld < V || step < 0 || eos >= V || eos < -1 || out_ld < W ||
        (step > 0 && prev_ld < W))
        return FN_E_SHAPE;
    if (V <= 384)
        hipLaunchKernelGGL(beam_step_kernel<6>, dim3(B), dim3(64 * W), 0, (hipStream_t)stream, logits, W, V, ld, step, eos, score_prev, token_prev,
                           prev_ld, score, parent, token, out_ld, logp_out, (long)logp_ld);
    else
        hipLaunchKernelGGL(beam_step_kernel<16>, dim3(B), dim3(64 * W), 0, (hipStream_t)stream, logits, W, V, ld, step, eos, score_prev, token_prev,
                           prev_ld, score, parent, token, out_ld, logp_out, (long)logp_ld);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

int fn_beam_gather(const FnBeamGatherJob* jobs, int n_jobs, int rows, int W, const int32_t* parent, void* stream) {
    if (!jobs || !parent) return FN_E_NULL;
    if (n_jobs < 1 || n_jobs > FN_BEAM_GATHER_MAX_JOBS) return FN_E_COUNT;
    if (rows < 1 || W < 1 || W > FN_BEAM_MAX_W || rows % W != 0) return FN_E_SHAPE;
    BeamGatherArgs a = {};
    for (int k = 0; k < n_jobs; ++k) {
        const FnBeamGatherJob& j = jobs[k];
        if (!j.src || !j.dst) return FN_E_NULL;
        if (j.cols < 1 || j.src_ld < j.cols || j.dst_ld < j.cols || j.src == j.dst) return FN_E_SHAPE;
        a.job[k] = j;
        a.vec[k] = ((uintptr_t)j.src % 16 == 0 && (uintptr_t)j.dst % 16 == 0 && j.src_ld % 4 == 0 && j.dst_ld % 4 == 0) ? 1 : 0;
    }
    hipLaunchKernelGGL(beam_gather_kernel, dim3((unsigned)((rows + 3) / 4), (unsigned)n_jobs), dim3(256), 0, (hipStream_t)stream, a, rows, W, parent);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

int fn_beam_backtrack(const int32_t* parent, const int32_t* token, const float* score, int steps, int B, int W, int eos,
                      int32_t* tokens_out, int32_t* beam_out, float* cum_out, int32_t* len_out, float* score_out, void* stream) {
    if (!parent || !token || !score || !tokens_out || !len_out || !score_out) return FN_E_NULL;
    if (steps < 1 || B < 1 || W < 1 || W > FN_BEAM_MAX_W || eos < -1) return FN_E_SHAPE;
    const long n = (long)B * W;
    hipLaunchKernelGGL(beam_backtrack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, parent, token, score, steps, B,
                       W, eos, tokens_out, beam_out, cum_out, len_out, score_out);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

}  // extern "C"
