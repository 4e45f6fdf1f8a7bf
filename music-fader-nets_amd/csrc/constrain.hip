// constrain.hip - constrained decode around the per-token heads (decode.Constraints): the logit processor in front of fn_vocab_argmax / fn_vocab_sample /
// fn_beam_step (fn_constrain_apply) and the fix-up + sounding-pitch update behind them (fn_constrain_advance).  include/fadernets.h has the
// definition; there is no reference counterpart (gmm_model.py:73-80,119-149 feeds back its argmax).
// Plain HIP: no inline assembly, no hand-counted waits, no LDS, no barriers, no atomics, no spins across workgroups.
#include "events.h"

namespace {

// the parameters as the definition clamps them
struct ConstrainView {
    int on_lo, off_lo, n, max_poly, eos, min_len;
    uint32_t flags;
};

__device__ __forceinline__ ConstrainView constrain_view(const FnConstrainParams* __restrict__ p) {
    ConstrainView c;
    c.on_lo = p->on_lo, c.off_lo = p->off_lo;
    c.n = min(max(p->n_pitch, 0), FN_CONSTRAIN_MAX_PITCH);
    c.max_poly = p->max_poly, c.eos = p->eos, c.min_len = p->min_len, c.flags = p->flags;
    return c;
}

__device__ __forceinline__ bool constrain_bit(uint32_t h0, uint32_t h1, uint32_t h2, uint32_t h3, int p) {
    const int k = p >> 5;
    const uint32_t w = k == 0 ? h0 : k == 1 ? h1 : k == 2 ? h2 : h3;
    return (w >> (p & 31)) & 1u;
}

// Geometry of vocab_argmax_kernel: one wavefront per row, 4 rows per workgroup, lane l on e = l, l + 64, ...  Two passes over the row: the first
// only asks whether anything stays, the second writes.  Every lane reads the 32 parameter bytes and the 16 bytes of held[r]; an element is read and
// written by one lane only, so the in-place update needs no ordering.
__global__ __launch_bounds__(256) void constrain_apply_kernel(float* __restrict__ logits, int rows, int V, int ld, int step,
                                                              const FnConstrainParams* __restrict__ params, const float* __restrict__ bias,
                                                              long bias_rs, const uint32_t* __restrict__ held, int* __restrict__ stuck) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const ConstrainView c = constrain_view(params);
    float* x = logits + r * ld;
    const float* bz = bias ? bias + r * bias_rs : nullptr;
    const bool grammar = held != nullptr && c.n > 0;
    uint32_t h0 = 0, h1 = 0, h2 = 0, h3 = 0;
    if (grammar) h0 = held[r * 4 + 0], h1 = held[r * 4 + 1], h2 = held[r * 4 + 2], h3 = held[r * 4 + 3];
    const bool full = c.max_poly > 0 && (__popc(h0) + __popc(h1) + __popc(h2) + __popc(h3)) >= c.max_poly;
    const bool ban_eos = c.eos >= 0 && c.eos < V && step < c.min_len;
    const bool off_needs_on = (c.flags & FN_CONSTRAIN_OFF_NEEDS_ON) != 0, no_reonset = (c.flags & FN_CONSTRAIN_NO_REONSET) != 0;

    auto in_g = [&](int e) -> bool {
        if (ban_eos && e == c.eos) return true;
        if (!grammar) return false;
        int p = fn_token_offset(e, c.on_lo, c.n);
        if (p >= 0) return constrain_bit(h0, h1, h2, h3, p) ? no_reonset : full;
        p = fn_token_offset(e, c.off_lo, c.n);
        return p >= 0 && off_needs_on && !constrain_bit(h0, h1, h2, h3, p);
    };

    bool left = false;
    for (int e = lane; e < V; e += 64) {
        const float y = bz ? x[e] + bz[e] : x[e];
        left = left || (y > -INFINITY && !in_g(e));
    }
    const bool is_stuck = __ballot(left) == 0ull;           // all 64 lanes are here: the loop above has ended for every one of them
    for (int e = lane; e < V; e += 64) {
        const float y = bz ? x[e] + bz[e] : x[e];
        x[e] = (!is_stuck && in_g(e)) ? -INFINITY : y;
    }
    if (is_stuck && stuck && lane == 0) stuck[r] = stuck[r] + 1;
}

// one thread per row
__global__ __launch_bounds__(256) void constrain_advance_kernel(int* tok_io, int tok_ld, int rows, int V,
                                                                const FnConstrainParams* __restrict__ params, const float* __restrict__ logits, int ld,
                                                                const int* fallback, int fb_ld, const uint32_t* held_in,
                                                                uint32_t* held_out, int* __restrict__ fixed) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const ConstrainView c = constrain_view(params);
    int tok = tok_io[r * tok_ld];
    if (logits) {
        const bool in_range = tok >= 0 && tok < V;
        if (!in_range || logits[r * ld + tok] == -INFINITY) {
            tok = min(max(fallback[r * fb_ld], 0), V - 1);
            tok_io[r * tok_ld] = tok;
            if (fixed) fixed[r] = fixed[r] + 1;
        }
    }
    if (!held_in) return;
    uint32_t h[4] = {held_in[r * 4 + 0], held_in[r * 4 + 1], held_in[r * 4 + 2], held_in[r * 4 + 3]};
    if (tok >= 0 && tok < V) {
        int p = fn_token_offset(tok, c.on_lo, c.n);
        if (p >= 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) h[k] |= (k == (p >> 5)) ? (1u << (p & 31)) : 0u;
        } else if ((p = fn_token_offset(tok, c.off_lo, c.n)) >= 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) h[k] &= (k == (p >> 5)) ? ~(1u << (p & 31)) : 0xffffffffu;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) held_out[r * 4 + k] = h[k];
}

}  // namespace

extern "C" {

int fn_constrain_apply(float* logits, int rows, int V, int ld, int step, const FnConstrainParams* params_dev, const float* bias, int64_t bias_rs,
                       const uint32_t* held, int32_t* stuck, void* stream) {
    if (!logits || !params_dev) return FN_E_NULL;
    if (rows < 1 || V < 1 || V > FN_SAMPLE_MAX_V || ld < V || step < 0 || (bias && bias_rs != 0 && bias_rs < V)) return FN_E_SHAPE;
    hipLaunchKernelGGL(constrain_apply_kernel, dim3((unsigned)(((long)rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, rows, V, ld, step,
                       params_dev, bias, (long)bias_rs, held, stuck);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

int fn_constrain_advance(int32_t* tok_io, int tok_ld, int rows, int V, const FnConstrainParams* params_dev, const float* logits, int ld,
                         const int32_t* fallback, int fb_ld, const uint32_t* held_in, uint32_t* held_out, int32_t* fixed, void* stream) {
    if (!tok_io || !params_dev || (logits && !fallback) || (held_in && !held_out)) return FN_E_NULL;
    if (rows < 1 || V < 1 || V > FN_SAMPLE_MAX_V || tok_ld < 1 || (logits && (ld < V || fb_ld < 1))) return FN_E_SHAPE;
    hipLaunchKernelGGL(constrain_advance_kernel, dim3((unsigned)(((long)rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tok_io, tok_ld, rows, V,
                       params_dev, logits, ld, fallback, fb_ld, held_in, held_out, fixed);
    FN_CHECK_LAUNCH();
    return FN_OK;
}

}  // extern "C"
