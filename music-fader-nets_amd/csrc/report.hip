// report.hip - the reconstruction report (report.py): per-token prediction, negative log-likelihood and rank of a target straight from the logits
// (fn_token_score: every logit is read once, nothing of width V is written) and the per-sample reduction of the reference's acc() with its
// np.trim_zeros quirk (fn_match_rows, trainer_gmm.py:545-565).  include/fadernets.h has the definition.
// Plain HIP: no inline assembly, no atomics, no LDS, no barrier, nothing between workgroups.  A wavefront past the last row leaves as a whole, so
// every shuffle sits in wave-uniform control flow.
#include "common.h"

namespace {

// One wavefront per row (row = b T + t, the order of the outputs), 4 rows per workgroup, lane l holds e = l, l + 64, ... in NE registers (V <= 64 NE):
// the geometry of vocab_sample_kernel.  The row stays in registers, so this is fn_row_head (common.h) written over v[]: the same per-lane order, the
// same fn_wave_argmax butterfly, expf sum and logf, so pred is vocab_argmax_kernel's token and nll the value of vocab_logsoftmax_kernel on the same
// floats.  x[tg] is picked up in the load loop by the lane that owns it and broadcast: the register array is never indexed by a runtime value.
template <int NE>
__global__ __launch_bounds__(256) void token_score_kernel(const float* __restrict__ x, long stride_b, long stride_t, int B, int T, int V,
                                                          const int32_t* __restrict__ target, int tgt_ld, int32_t* __restrict__ pred,
                                                          float* __restrict__ nll, int32_t* __restrict__ rank, int out_ld) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)B * T) return;
    const long b = row / T, t = row % T;
    const float* xr = x + b * stride_b + t * stride_t;
    const int tg = target ? min(max(target[b * tgt_ld + t], 0), V - 1) : -1;
    float v[NE];
    float mx = -INFINITY, xt = 0.f;
    int am = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        const int e = lane + 64 * k;
        v[k] = e < V ? xr[e] : -INFINITY;
        if (e < V && v[k] > mx) { mx = v[k]; am = e; }
        if (e == tg) xt = v[k];
    }
    fn_wave_argmax(mx, am);
    if (pred && lane == 0) pred[b * out_ld + t] = am;
    if (!target) return;                                   // wave-uniform
    xt = __shfl(xt, tg & 63, 64);
    float s = 0.f;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        const int e = lane + 64 * k;
        if (e < V) {
            s += expf(v[k] - mx);
            cnt += (v[k] > xt || (v[k] == xt && e < tg)) ? 1 : 0;
        }
    }
    s = fn_wave_sum(s);
    cnt = fn_wave_sum_i32(cnt);
    if (lane == 0) {
        if (nll) nll[b * out_ld + t] = (mx + logf(s)) - xt;
        if (rank) rank[b * out_ld + t] = cnt;
    }
}

// One wavefront per row, 4 rows per workgroup.  First and last non-zero of the target by a lane-strided scan and a wave min / max, then the counts
// and the fp64 sum in the stated order: lane l takes j = l, l + 64, ... ascending, then the xor butterfly 32 .. 1.
__global__ __launch_bounds__(256) void match_rows_kernel(const int32_t* __restrict__ pred, int pred_ld, const int32_t* __restrict__ target, int tgt_ld,
                                                         int rows, int T, int trim, const float* __restrict__ nll, const int32_t* __restrict__ rank,
                                                         int aux_ld, int topk, int32_t* __restrict__ lead_out, int32_t* __restrict__ len_out,
                                                         int32_t* __restrict__ correct, int32_t* __restrict__ correct_topk, double* __restrict__ acc,
                                                         double* __restrict__ nll_sum, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int32_t* tr = target + r * tgt_ld;
    const int32_t* pr = pred + r * pred_ld;
    int lead = 0, len = T;
    if (trim) {
        int first = T, last = -1;
        for (int j = lane; j < T; j += 64)
            if (tr[j] != 0) { first = min(first, j); last = j; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            first = min(first, __shfl_xor(first, o, 64));
            last = max(last, __shfl_xor(last, o, 64));
        }
        lead = first;
        len = last >= 0 ? last + 1 - first : 0;
    }
    int ok = 0, ok_k = 0;
    double sum = 0.0;
    for (int j = lane; j < len; j += 64) {                 // lead + j <= last < T
        ok += pr[j] == tr[lead + j] ? 1 : 0;
        if (rank) ok_k += rank[r * aux_ld + lead + j] < topk ? 1 : 0;
        if (nll) sum += (double)nll[r * aux_ld + lead + j];
    }
    ok = fn_wave_sum_i32(ok);
    if (rank) ok_k = fn_wave_sum_i32(ok_k);
    if (nll) sum = fn_wave_sum_f64(sum);
    if (lane == 0) {
        lead_out[r] = lead, len_out[r] = len, correct[r] = ok;
        if (correct_topk) correct_topk[r] = ok_k;
        acc[r] = len > 0 ? (double)ok / (double)len : 0.0;
        if (nll_sum) nll_sum[r] = sum;
        status[r] = len > 0 ? 0 : FN_MATCH_EMPTY;
    }
}

}  // namespace

extern "C" {

int fn_token_score(const float* x, int64_t stride_b, int64_t stride_t, int B, int T, int V, const int32_t* target, int tgt_ld, int32_t* pred, float* nll,
                   int32_t* rank, int out_ld, void* stream) {
    if (!x || (!pred && !nll && !rank) || ((nll || rank) && !target)) return FN_E_NULL;
    if (B < 1 || T < 1 || V < 1 || V > FN_SAMPLE_MAX_V || out_ld < T || (target && tgt_ld < T) || (long)B * T > 0x7fffffffL * 4) return FN_E_SHAPE;
    const dim3 grid((unsigned)(((long)B * T + 3) / 4)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (V <= 64)
        hipLaunchKernelGGL(token_score_kernel<1>, grid, block, 0, s, x, (long)stride_b, (long)stride_t, B, T, V, target, tgt_ld, pred, nll, rank, out_ld);
    else if (V <= 384)
        hipLaunchKernelGGL(token_score_kernel<6>, grid, block, 0, s, x, (long)stride_b, (long)stride_t, B, T, V, target, tgt_ld, pred, nll, rank, out_ld);
    else
        hipLaunchKernelGGL(token_score_kernel<16>, grid, block, 0, s, x, (long)stride_b, (long)stride_t, B, T, V, target, tgt_ld, pred, nll, rank, out_ld);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

int fn_match_rows(const int32_t* pred, int pred_ld, const int32_t* target, int tgt_ld, int rows, int T, int trim, const float* nll, const int32_t* rank,
                  int aux_ld, int topk, int32_t* lead, int32_t* len, int32_t* correct, int32_t* correct_topk, double* acc, double* nll_sum,
                  int32_t* status, void* stream) {
    if (!pred || !target || !lead || !len || !correct || !acc || !status || (rank != nullptr) != (correct_topk != nullptr) ||
        (nll != nullptr) != (nll_sum != nullptr))
        return FN_E_NULL;
    if (rows < 1 || T < 1 || pred_ld < T || tgt_ld < T || ((nll || rank) && aux_ld < T) || (rank && topk < 1)) return FN_E_SHAPE;
    hipLaunchKernelGGL(match_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, pred, pred_ld, target, tgt_ld, rows, T, trim,
                       nll, rank, aux_ld, topk, lead, len, correct, correct_topk, acc, nll_sum, status);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

}  // extern "C"
