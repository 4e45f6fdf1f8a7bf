// decode_plan.h - what fn_decode_greedy / fn_decode_forced / fn_out_argmax_f32 launch, decided in one place: the argument checks in the order that
// decides which code a call with several faults returns, the role set of the one-launch decode, its row blocks, replicas, grid and LDS size, the
// carve-up of FnDecode.ws, and the kernel, grid and LDS size of the fused output layer - pure functions of the arguments and the number of compute
// units.  Plain C++17 without HIP headers: decode_persist.hip / gru.hip launch from the plans, fn_decode_plan / fn_out_argmax_plan hand them out, and
// csrc/host/decode_plan_check.cpp compiles this file for the host under sanitizers.  Addresses are integers: inspected for NULL-ness and alignment,
// never dereferenced.
#pragma once
#include "gru_plan.h"

// ---- the one-launch decode (decode_persist.hip) -----------------------------------------------------------------------------------------------
constexpr int DECODE_NT = 256;                      // threads of a role workgroup
constexpr int C1 = 0, C2 = 32, C3 = 64, C4 = 96, C5 = 128;               // word offsets inside a block's counters (one 128-byte line each)
constexpr int BLKW = 160;                           // counter words per block
constexpr int MAXBLK = 32;                          // blocks of 32 / 64 rows: up to 1024 / 2048 sequences
constexpr int ERRW = MAXBLK * BLKW;                 // sticky error word behind all counters
constexpr int DECODE_MAX_V = 384;                   // six vocabulary columns per lane of the argmax wave
constexpr int DECODE_MAX_LDS = 160 * 1024 - 64;     // dynamic LDS the decode kernel may ask for
// from this many sequences on: 64-row blocks (measured crossover, profiles/r03_decode_block_pipeline.txt: 320 rows 34.5 vs 36.4 us per token,
// 384 rows 41.8 vs 35.9)
constexpr int DECODE_MT4_ROWS = 353;

// f of fn_decode_forced: its own members, answered before anything of d is looked at
inline int decode_force_validate(const FnDecode* d, const FnDecodeForce* f) {
    if (!f->forced || !f->force) return FN_E_NULL;
    if (f->forced_ld < d->steps) return FN_E_SHAPE;
    return FN_OK;
}
// the clauses the host twins share with the device: required members, then the sizes
inline int decode_members_validate(const FnDecode* d) {
    if (!d->w_hh1_frag || !d->b_hh1 || !d->table1 || !d->h0 || !d->w_ih2_frag || !d->w_hh2_frag || !d->b_hh2 || !d->w_out_frag || !d->b_out || !d->tokens ||
        !d->ws || !d->sync_ws)
        return FN_E_NULL;
    if (d->B <= 0 || d->B > MAXBLK * 64 || d->steps <= 0 || d->H <= 0 || (d->H % 32) != 0 || d->H > 512 || d->V <= 0 || d->tok_ld < d->steps) return FN_E_SHAPE;
    return FN_OK;
}
// fn_decode_greedy (f == nullptr) / fn_decode_forced: the forced members, the NULL members, the shape, the alignment - in this order.  start_token is
// not looked at: the kernel reads the table row it names, the caller answers for it (the host twin refuses one outside [0, V))
inline int decode_validate(const FnDecode* d, const FnDecodeForce* f) {
    if (!d) return FN_E_NULL;
    if (f)
        if (const int rc = decode_force_validate(d, f)) return rc;
    if (const int rc = decode_members_validate(d)) return rc;
    if (d->V > DECODE_MAX_V) return FN_E_SHAPE;
    const uintptr_t al = gru_addr(d->w_hh1_frag) | gru_addr(d->w_ih2_frag) | gru_addr(d->w_hh2_frag) | gru_addr(d->w_out_frag) | gru_addr(d->b_hh1) |
                         gru_addr(d->b_ih1) | gru_addr(d->table1) | gru_addr(d->rowbias1) | gru_addr(d->h0) | gru_addr(d->b_ih2) | gru_addr(d->b_hh2) | gru_addr(d->ws);
    return (al & 15) ? FN_E_ALIGN : FN_OK;
}

// FnDecode.ws in floats, for `rows` padded rows: x1 and x2 = two slots of fragment-major states each, g2 = layer 2's input pre-activations, logits
struct DecodeWsLayout {
    size_t x1, x2, g2, logits, total;
};
inline DecodeWsLayout decode_ws_layout(size_t rows, int H, int V) {
    const size_t vp = (size_t)(V + 15) / 16 * 16;
    DecodeWsLayout l;
    l.x1 = 0;
    l.x2 = l.x1 + 2 * rows * H;
    l.g2 = l.x2 + 2 * rows * H;
    l.logits = l.g2 + rows * 3 * H;
    l.total = l.logits + rows * vp;
    return l;
}
// rows fn_decode_ws_bytes provides for B sequences: whole blocks of whichever height (16 / 32 / 64) the plan picks
inline size_t decode_ws_rows(int B) { return B <= 16 ? 16 : (size_t)(B + 63) / 64 * 64; }
inline size_t decode_ws_bytes(int B, int H, int V) { return decode_ws_layout(decode_ws_rows(B), H, V).total * sizeof(float); }
inline size_t decode_sync_ws_bytes() { return (size_t)(ERRW + 32) * 4; }

// the weight slice [48 x H] + the partial tiles of 4 waves x mt row tiles x 3 gates + the give-up word (16 bytes) and the 64 tokens of the step
inline int lds_decode(int H, int mt) { return (3 * H * 16 + 4 * mt * 3 * RT) * 4 + 16 + 64 * 4; }

// fn_decode_greedy (f == nullptr) / fn_decode_forced.  cus: compute units of the device.  The kernel spins on counters that other workgroups of the
// same launch advance: every workgroup of the grid must be resident, one per compute unit
inline FnDecodePlan decode_plan(const FnDecode* d, const FnDecodeForce* f, int cus) {
    FnDecodePlan p{};
    if ((p.status = decode_validate(d, f)) != FN_OK) return p;
    p.forced = f != nullptr;
    p.threads = DECODE_NT;
    p.nslices = d->H / 16;
    p.nvt = (d->V + 15) / 16;
    p.per_rep = 3 * p.nslices + p.nvt + 1;                      // the role set: L1, P2, L2 slices, output slices, ARG
    if (p.per_rep > cus) {
        p.status = FN_E_UNSUPPORTED;
        return p;
    }
    // row tiles per block.  Latency regime (few blocks per replica): a block's time is its hand-over chain, 32-row blocks give the chain
    // more blocks to overlap.  Throughput regime: a role's busy time per block is ~8.6 k cycles of latency + 6.1 k of MFMA per 32 rows, so
    // 64-row blocks halve the latency share per row
    p.mt = d->B <= 16 ? 1 : (d->B >= DECODE_MT4_ROWS ? 4 : 2);
    p.block_rows = p.mt * 16;
    p.nblk = (d->B + p.block_rows - 1) / p.block_rows;
    if (p.nblk > MAXBLK) {
        p.status = FN_E_SHAPE;
        return p;
    }
    p.nrep = cus / p.per_rep < p.nblk ? cus / p.per_rep : p.nblk;      // replicas of the role set that fit (replica r: blocks r, r + nrep, ...)
    p.grid = p.nrep * p.per_rep;
    p.lds_bytes = lds_decode(d->H, p.mt);
    const DecodeWsLayout l = decode_ws_layout((size_t)p.nblk * p.block_rows, d->H, d->V);
    p.x1_off = (int64_t)l.x1; p.x2_off = (int64_t)l.x2; p.g2_off = (int64_t)l.g2; p.logits_off = (int64_t)l.logits; p.ws_floats = (int64_t)l.total;
    return p;
}

// ---- the output layer with the argmax in its epilogue (gru.hip) --------------------------------------------------------------------------------
constexpr int OUT_ARGMAX_WLDS_MAX = 128 * 1024;     // a workgroup's weight slice (48 rows x K) stays in LDS up to this many bytes

// the clauses the host twin shares with the device
inline int out_argmax_members_validate(const void* h, int ldh, const void* W, int ldw, const void* bias, int B, int V, int K, const void* best) {
    if (!h || !W || !bias || !best) return FN_E_NULL;
    if (B <= 0 || V <= 0 || K <= 0 || (K % 16) != 0 || ldh < K || ldw < K || (ldh & 3) || (ldw & 3)) return FN_E_SHAPE;
    return FN_OK;
}

// fn_out_argmax_f32: NULL, shape, the spans below 4 GB (32-bit lane offsets), alignment - in this order
inline FnOutArgmaxPlan out_argmax_plan(const void* h, int ldh, const void* W, int ldw, const void* bias, int B, int V, int K, const void* best) {
    FnOutArgmaxPlan p{};
    if ((p.status = out_argmax_members_validate(h, ldh, W, ldw, bias, B, V, K, best)) != FN_OK) return p;
    if ((long)B * ldh * 4 >= (1L << 32) || (long)V * ldw * 4 >= (1L << 32)) return p.status = FN_E_SHAPE, p;
    if (((gru_addr(h) | gru_addr(W)) & 15) || (gru_addr(best) & 7)) return p.status = FN_E_ALIGN, p;
    const long slice = 48L * K * 4;
    if (slice <= OUT_ARGMAX_WLDS_MAX) {           // weight slice of a workgroup resident in LDS: 64 rows x 48 columns per workgroup
        const bool eight = (K % 32) == 0;         // eight waves: waves 4-7 take the second half of K and hand their accumulators over through LDS
        p.kernel = eight ? FN_OUT_ARGMAX_LDS8 : FN_OUT_ARGMAX_LDS;
        p.grid = ((B + 63) / 64) * ((V + 47) / 48);
        p.threads = eight ? 2 * GRU_NT : GRU_NT;
        p.lds_bytes = (int)slice + (eight ? 4 * 3 * 64 * 16 : 0);
    } else {                                      // the LDS-free loop: 32 rows x 96 columns per workgroup
        p.kernel = FN_OUT_ARGMAX_DIRECT;
        p.grid = ((B + 31) / 32) * ((V + 95) / 96);
        p.threads = GRU_NT;
    }
    return p;
}
