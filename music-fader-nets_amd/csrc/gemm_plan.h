// gemm_plan.h - what fn_gemm_f32 / fn_gru_dwhh_f32 launch, decided in one place: the kernel instance, the K ranges, the grid and the slab reduction
// as a pure function of the shapes, the leading dimensions, the alignment of the addresses, the flag bits and the number of compute units.
// Plain C++17 without HIP headers: gemm.hip launches from the plan, fn_gemm_plan / fn_gru_dwhh_plan hand it out, and csrc/host/gemm_plan_check.cpp
// compiles this file for the host under sanitizers.  Addresses are integers: inspected for alignment, never dereferenced.
#pragma once
#include "../../include/fadernets.h"

// the flag bits that ride on the `splitk` argument of fn_gemm_f32 / fn_gru_dwhh_f32 (fadernets.h)
struct SplitkFlags {
    static constexpr int X6_MODES = FN_GEMM_X6_PERWAVE | FN_GEMM_X6_WIDE | FN_GEMM_X6_PERTILE;
    bool lean, x6;
    int x6_mode, xflags, splitk;                         // xflags: the bf16 x 6 bits as they came, to hand on; splitk: the number of K ranges asked for
    explicit SplitkFlags(int v)
        : lean((v & FN_GEMM_LEAN) != 0), x6((v & FN_GEMM_BF16X6) != 0), x6_mode(v & X6_MODES), xflags(v & (FN_GEMM_BF16X6 | X6_MODES)),
          splitk(v & ~(FN_GEMM_LEAN | FN_GEMM_BF16X6 | X6_MODES)) {}
};

// tile shape and wave grid of a staged instance: the template arguments of gemm_kernel<BM, BN, BK, WM, WN, ..>
struct StagedTile {
    int bm, bn, bk, wm, wn;
};
constexpr StagedTile staged_tile(int kernel) {
    switch (kernel) {
        case FN_PLAN_STAGED_64_64_32: return {64, 64, 32, 2, 2};
        case FN_PLAN_STAGED_32_64_32: return {32, 64, 32, 2, 2};
        case FN_PLAN_STAGED_64_16_16: return {64, 16, 16, 4, 1};
        case FN_PLAN_STAGED_128_128_32: return {128, 128, 32, 2, 2};
        default: return {64, 64, 16, 2, 2};
    }
}

// K ranges of whole `gran`-k blocks, the last one short: klen rows each, as many as it then takes (fewer than asked for when K is short)
inline void plan_split(FnGemmPlan& p, int K, int splitk, int gran) {
    p.klen = K;
    p.ranges = 1;
    if (splitk > 1) {
        p.klen = ((K + splitk - 1) / splitk + gran - 1) / gran * gran;
        p.ranges = (K + p.klen - 1) / p.klen;
    }
}

// split-K slabs -> C: the float4 form where everything is 16-byte aligned (same summation order per element), none for an unsplit launch
inline void plan_reduce(FnGemmPlan& p, int M, int N, int ldc, uintptr_t C, uintptr_t bias, uintptr_t ws) {
    p.reduce = FN_PLAN_REDUCE_NONE;
    p.reduce_blocks = 0;
    if (p.ranges <= 1) return;
    const bool v4 = (N & 3) == 0 && (ldc & 3) == 0 && ((ws | C | bias) & 15) == 0;
    const long total = v4 ? (long)M * N / 4 : (long)M * N;
    p.reduce = v4 ? FN_PLAN_REDUCE_SLAB4 : FN_PLAN_REDUCE_SLAB;
    p.reduce_blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
}

// the TN product (both operands with K as their slow dimension, 16-byte aligned): bf16 x 6 or fp32 kernel over K ranges, then the slab reduce
inline FnGemmPlan plan_tn(const SplitkFlags& f, int M, int N, int K, int ldc, uintptr_t C, uintptr_t bias, uintptr_t ws, int msplit, int cus) {
    FnGemmPlan p{};
    // K ranges of whole 32-k blocks for the bf16 x 6 kernels (no fp32-MFMA tail inside a range), of 4 rows otherwise
    plan_split(p, K, f.splitk, f.x6 ? 32 : 4);
    p.msplit = msplit;
    p.tiles = ((M + 127) / 128) * ((N + 127) / 128);
    // bf16 x 6: the producer / consumer kernels (512 threads) on 128 x 128 or, FN_GEMM_X6_WIDE, 128 x 256 tiles, or the per-wave kernel on request
    const bool walks = f.x6 && !(f.x6_mode & FN_GEMM_X6_PERWAVE);
    if (!f.x6) {
        p.kernel = f.lean ? FN_PLAN_TN_LEAN : FN_PLAN_TN;
    } else if (!walks) {
        p.kernel = FN_PLAN_TN_X6;
    } else if (f.x6_mode & FN_GEMM_X6_WIDE) {
        p.kernel = FN_PLAN_TN_X6V;
        p.tiles = ((M + 127) / 128) * ((N + 255) / 256);
    } else {
        p.kernel = FN_PLAN_TN_X6W;
    }
    // 1-D (K ranges dealt to the XCDs, see gemm_tn_body) when the K ranges divide by 8, else tiles x 1 x K ranges
    const bool one_d = p.ranges > 1 && (p.ranges & 7) == 0;
    p.grid_x = one_d ? p.tiles * p.ranges : p.tiles;
    p.grid_y = 1;
    p.grid_z = one_d ? 1 : p.ranges;
    // 1-D launches of the producer / consumer kernels: one workgroup per CU walking its (tile, K range) items instead of one workgroup per item - the
    // next item's first blocks are requested and cut while the consumers store the finished one (FN_GEMM_X6_PERTILE: one workgroup per item, A/B and
    // tests), unless the CU count is not a multiple of the 8 XCDs
    if (walks && one_d && !(f.x6_mode & FN_GEMM_X6_PERTILE) && cus >= 8 && (cus & 7) == 0 && p.grid_x > cus) p.grid_x = cus;
    plan_reduce(p, M, N, ldc, C, bias, ws);
    return p;
}

// fn_gemm_f32.  splitk_and_flags: the `splitk` argument as it came; cus: compute units of the device
inline FnGemmPlan gemm_plan(int a_k, int b_k, int M, int N, int K, int lda, int ldb, int ldc, uintptr_t A, uintptr_t B, uintptr_t C, uintptr_t bias,
                            uintptr_t ws, int splitk_and_flags, int cus) {
    const SplitkFlags f(splitk_and_flags);
    const int splitk = f.splitk;
    if (!a_k && !b_k && (lda % 4) == 0 && (ldb % 4) == 0 && lda >= 4 && ldb >= 4 && ((A | B) & 15) == 0) return plan_tn(f, M, N, K, ldc, C, bias, ws, 0, cus);
    FnGemmPlan p{};
    p.klen = K;
    p.ranges = p.grid_y = p.grid_z = 1;
    // K-contiguous operands, whole 128 x 128 tiles, 16-byte aligned rows, no split: what the two kernels without a bounds check ask for
    const bool whole = a_k && b_k && splitk <= 1 && (M % 128) == 0 && (N % 128) == 0 && (lda % 4) == 0 && (ldb % 4) == 0 && (ldc % 4) == 0 &&
                       ((A | B | C | bias) & 15) == 0;
    const long whole_tiles = (long)(M / 128) * (N / 128);
    // bf16 x 6, 32-k blocks: the producer / consumer kernel - one workgroup per CU (144 KB of LDS each) walking its tiles, unless asked for one
    // workgroup per tile (FN_GEMM_X6_PERTILE) or the CU count is not a multiple of the 8 XCDs
    if (f.x6 && whole && (K % 32) == 0 && K >= 128 && whole_tiles >= 128) {
        p.kernel = FN_PLAN_NT_X6W;
        p.tiles = (int)whole_tiles;
        p.grid_x = (p.tiles > cus && cus >= 8 && (cus & 7) == 0 && !(f.x6_mode & FN_GEMM_X6_PERTILE)) ? cus : p.tiles;
        return p;
    }
    // tiles that fill the chip, short K: the LDS-free kernel; lean: <= 128 registers, one of its wavefronts fits a SIMD beside a wavefront of the
    // decoder-shaped forward scans (377 registers)
    if (whole && (K % 16) == 0 && K >= 64 && (long)M * lda < (1L << 30) && (long)N * ldb < (1L << 30) && whole_tiles >= 256) {
        p.kernel = f.lean ? FN_PLAN_NT_DIRECT_1_4 : FN_PLAN_NT_DIRECT_4_2;
        p.tiles = p.grid_x = (int)whole_tiles;
        return p;
    }
    const long tiles128 = (long)((M + 127) / 128) * ((N + 127) / 128);
    if (N <= 16 && a_k && b_k && splitk <= 1 && M >= 64) {
        // skinny outputs (the attribute decoders' output layers: 16384 x 3 / 16 x 512): 64 x 16 tiles, 12.8 KB of LDS - a workgroup fits a CU beside one
        // of the bf16 x 6 producer / consumer kernels (144 of 160 KB), so the loss chain of the step runs beside the dhx1 product instead of behind it;
        // same k order
        p.kernel = FN_PLAN_STAGED_64_16_16;
    } else if (tiles128 * (splitk > 1 ? splitk : 1) >= 256) {
        // 128 x 128 tiles only when they fill the chip (one workgroup per CU); below that the 64 x 64 kernel's 4x more workgroups win
        // (decode at 2048 rows: 192 big tiles -> 55 us, 768 small ones -> 40 us per W_ih2 projection)
        p.kernel = FN_PLAN_STAGED_128_128_32;
    } else if (splitk <= 1 && (K % 32) == 0 && K >= 128) {
        // 64 x 64 tiles: K tiles of 32 when K allows it - one barrier per 32 MFMAs of a wave instead of per 16 (the decode's output layer,
        // 2048 x 342 x 512: 20.5 -> see profiles); same k order ... and 32 x 64 tiles when even the 64 x 64 ones leave CUs empty (the decode's output
        // layer at 2048 rows: 192 workgroups -> 384; same k order per output element: bit-identical)
        const long tiles64 = (long)((M + 63) / 64) * ((N + 63) / 64);
        p.kernel = a_k && b_k && tiles64 < 240 && M >= 64 ? FN_PLAN_STAGED_32_64_32 : FN_PLAN_STAGED_64_64_32;
    } else {
        p.kernel = FN_PLAN_STAGED_64_64_16;
    }
    const StagedTile t = staged_tile(p.kernel);
    plan_split(p, K, splitk, t.bk);
    p.tiles = p.grid_x = ((M + t.bm - 1) / t.bm) * ((N + t.bn - 1) / t.bn);
    p.grid_z = p.ranges;
    plan_reduce(p, M, N, ldc, C, bias, ws);
    return p;
}

// fn_gru_dwhh_f32, dW [3H][H] = beta dW + [dgx[:, :2H] | dghn]^T hprev: one split-A launch of the TN product when the band of dghn starts on a tile
// boundary, else two products (rows [0, 2H) from dgx, rows [2H, 3H) from dghn), which do not carry the lean bit on
struct DwhhPlan {
    int n;
    FnGemmPlan launch[2];
};
inline DwhhPlan dwhh_plan(int H, int rows, uintptr_t dgx, uintptr_t dghn, uintptr_t hprev, uintptr_t dW, uintptr_t ws, int splitk_and_flags, int cus) {
    const SplitkFlags f(splitk_and_flags);
    DwhhPlan d{};
    if ((2 * H) % 128 == 0 && (H % 4) == 0 && ((dgx | dghn | hprev) & 15) == 0) {
        d.n = 1;
        d.launch[0] = plan_tn(f, 3 * H, H, rows, H, dW, 0, ws, 2 * H, cus);
        return d;
    }
    const int fl = f.splitk | f.xflags;
    d.n = 2;
    d.launch[0] = gemm_plan(0, 0, 2 * H, H, rows, 3 * H, H, H, dgx, hprev, dW, 0, ws, fl, cus);
    d.launch[1] = gemm_plan(0, 0, H, H, rows, H, H, H, dghn, hprev, dW + (uintptr_t)2 * H * H * sizeof(float), 0, ws, fl, cus);
    return d;
}
