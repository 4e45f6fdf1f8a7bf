// x6w_core.h - shared pieces of the bf16 x 6 producer / consumer kernels (gemm.hip: gemm_tn_x6w_kernel, gemm_tn_x6v_kernel, gemm_nt_x6w_kernel;
// gru.hip: gru_cell_x6_kernel): the exact three-piece split of fp32 values, the LDS stage geometry, the barriers, the producer wavefronts' trip
// schedule and the consumer wavefront.
// gfx950 only.  See gemm.hip for the design notes and the measurements behind them.
#pragma once
#include <type_traits>
#include <utility>

#include "mma_core.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
FN_DEVINL unsigned fn_pack_top16(float a, float b) {          // top 16 bits of a | top 16 bits of b << 16
    return __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
}
FN_DEVINL float fn_top16(float x) { return __uint_as_float(__float_as_uint(x) & 0xffff0000u); }
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
// THE split: N fp32 values (4 or 8 consecutive k of one operand row / column) -> their exact bf16 triples, each piece as N / 2 dwords of two packed
// bf16.  RN = rounded pieces (fn_rn16: one integer add more per level), else truncated ones.  One ROUNDED operand is enough to make the dropped
// partial products zero-mean (mid_a lo_b, lo_a mid_b: lo_b and mid_b then carry random signs); with both operands truncated they all have the sign of
// a b and bias a sum by ~2^-24 sum |a||b| towards zero (tests/test_gpu_parity.py::test_bf16x6_adversarial_operands_vs_float64).  The kernels are bound
// by these VALU operations: B rounded, A truncated.
// Two cheaper-on-paper forms measured SLOWER in one session (round 5, dW_hh product 1536 x 512 x 65280 at 16 / 32 K ranges; this form 698-736 / 603-610 us):
// v_cvt_pk_bf16_f32 for every piece (both halves of a dword rounded to nearest even by one instruction, 4.5 operations per value: 740 / 665 us) and
// two-element vector arithmetic that makes the remainders packed subtractions (v_pk_add_f32; 882 / 846 us: the compiler shuffles registers around them).
template <bool RN, int N, class V>
FN_DEVINL void fn_split(const float (&x)[N], V& h, V& m, V& l) {                     // V = u32x4 (N = 8) or u32x2 (N = 4)
    static_assert(sizeof(V) == 2 * N, "two bf16 per dword");
    float hi[N], r1[N], mi[N], r2[N];
#pragma unroll
    for (int j = 0; j < N; ++j) { hi[j] = RN ? fn_rn16(x[j]) : fn_top16(x[j]); r1[j] = x[j] - hi[j]; }
#pragma unroll
    for (int j = 0; j < N; ++j) { mi[j] = RN ? fn_rn16(r1[j]) : fn_top16(r1[j]); r2[j] = r1[j] - mi[j]; }
#pragma unroll
    for (int j = 0; j < N / 2; ++j) {
        h[j] = fn_pack_top16(hi[2 * j], hi[2 * j + 1]);
        m[j] = fn_pack_top16(mi[2 * j], mi[2 * j + 1]);
        l[j] = fn_pack_top16(r2[2 * j], r2[2 * j + 1]);
    }
}
// element `e` of N float4 vectors (N consecutive k of one column: the TN kernels load column-wise) -> the three pieces
template <bool RN, int N, class V>
FN_DEVINL void fn_split_col(const f32x4 (&v)[N], int e, V& h, V& m, V& l) {
    float x[N];
#pragma unroll
    for (int j = 0; j < N; ++j) x[j] = v[j][e];
    fn_split<RN>(x, h, m, l);
}
template <bool RN>
FN_DEVINL void fn_split8(const f32x4 (&v)[8], int e, bf16x8& h, bf16x8& m, bf16x8& l) {
    u32x4 H, M, L;
    fn_split_col<RN>(v, e, H, M, L);
    h = __builtin_bit_cast(bf16x8, H);
    m = __builtin_bit_cast(bf16x8, M);
    l = __builtin_bit_cast(bf16x8, L);
}
template <bool RN>
FN_DEVINL void fn_split4(const f32x4 (&v)[4], int e, u32x2& h, u32x2& m, u32x2& l) { fn_split_col<RN>(v, e, h, m, l); }
// row `e` of a set loaded row-wise (two float4 = 8 consecutive k per row: the NT and cell producers), or zeros -> the three pieces
template <bool RN>
FN_DEVINL void fn_split_row(const f32x4 (&v)[8], int e, bool zero, u32x4& h, u32x4& m, u32x4& l) {
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = zero ? 0.f : v[2 * e + (j >> 2)][j & 3];
    fn_split<RN>(x, h, m, l);
}
// The three pieces of operand tile `a` of a set go to slots (3 a + piece) * 64 of the set (MFMA operand order: consumer lane l reads slot + l):
// 16-byte slots, or - two lanes per slot - their 8-byte halves (the half sets of gemm_tn_x6v_kernel)
template <class V>
FN_DEVINL void x6w_put(V* dst, int a, const V& h, const V& m, const V& l) {
    constexpr int per = sizeof(u32x4) / sizeof(V);
    dst[((a * 3 + 0) * 64) * per] = h;
    dst[((a * 3 + 1) * 64) * per] = m;
    dst[((a * 3 + 2) * 64) * per] = l;
}
template <bool RN, int N, class V>
FN_DEVINL void x6w_cut(V* dst, int a, const f32x4 (&v)[N]) {                         // column-wise set (TN): 8 vectors -> 16-byte slots, 4 -> 8-byte halves
    V h, m, l;
    fn_split_col<RN>(v, a, h, m, l);
    x6w_put(dst, a, h, m, l);
}
template <bool RN>
FN_DEVINL void x6w_cut_row(u32x4* dst, int e, const f32x4 (&v)[8], bool zero = false) {       // row-wise set (NT, cell)
    u32x4 h, m, l;
    fn_split_row<RN>(v, e, zero, h, m, l);
    x6w_put(dst, e, h, m, l);
}

constexpr int X6W_NT = 512;
constexpr int X6W_NS = 3;                        // register sets of a producer wavefront (blocks in flight: NS - 1)
constexpr int X6W_SET = 4 * 3 * 64;              // u32x4 vectors of one set (64 operand columns x 32 k as triples: 12 KB)
constexpr int X6W_STAGE = 4 * X6W_SET;           // ... of one stage (48 KB)
constexpr int X6W_STAGES = 3;
// producers: every ds_write of the block has to be in LDS before the barrier; consumers: a bare s_barrier (their reads of the block the barrier
// retires were consumed by MFMAs long before; the reads in flight belong to the NEXT block, whose stage nobody writes for two more blocks)
FN_DEVINL void x6w_barrier_p() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}
FN_DEVINL void x6w_barrier_c() {
    asm volatile("s_barrier" ::: "memory");
}

template <int I>
using x6w_ic = std::integral_constant<int, I>;
template <int... I, class F>
FN_DEVINL void x6w_for_impl(std::integer_sequence<int, I...>, F&& f) { (f(x6w_ic<I>{}), ...); }
template <int N, class F>
FN_DEVINL void x6w_for(F&& f) { x6w_for_impl(std::make_integer_sequence<int, N>{}, f); }      // f(integral_constant<0>) .. f(integral_constant<N - 1>), unrolled
FN_DEVINL f32x4 x6w_ld(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// THE trip schedule of a producer wavefront (gemm_tn_x6w_kernel, gemm_tn_x6v_kernel, gemm_nt_x6w_kernel, gru_cell_x6_kernel).  Block b lives in register
// set b % NS on its way from memory and in LDS stage b % (LEAD + 1) once cut; the consumers multiply block t while the producers work on trip t:
//   prologue   request blocks 0 .. NS - 1, cut blocks 0 .. LEAD - 1, request blocks NS .. NS + LEAD - 2 into the sets that freed, barrier;
//   trip t     request block t + NS + LEAD - 1 | cut block t + LEAD (requested NS - 1 trips ago) | barrier          - 1 + nblk barriers in all.
// What a kernel supplies (SET, LS, CS are x6w_ic<register set>):
//   request(SET, blk)                 the loads of ANY block (behind the matrix' last row: clamped addresses);
//   cut(SET, blk, stage)              ANY block -> LDS (rows behind the matrix count as zeros);
//   fused(LS, lblk, CS, cblk, stage)  request of WHOLE block lblk and cut of WHOLE block cblk in one piece of straight-line code.  The kernels
//                                     interleave them - the loads of the new block in quarters, one in front of every quarter of the cut: issued as one
//                                     burst the loads keep the wave at the vector-memory queue until most of them have been taken (a CU's address path
//                                     takes ~30 clocks per 1 KB wave load: measured, the loads of a block cost the CU ~1000 clocks), and the address path
//                                     then idles while the wave splits - loads + cut ran as long as their sum.
// PLAIN loads, the compiler counts vmcnt: the steady state runs `fused` only - NS trips per pass with static register sets, no clamping, no branch
// between a request and its use - and for such code hipcc emits exactly `s_waitcnt vmcnt(loads per block x (NS - 1))` in front of the cut (read in the
// ISA).  A first version with asm-statement loads and hand-counted waits passed every test, but its ISA showed whole register sets copied (`v_mov_b64`)
// at the control-flow merges of the partial-block / tail paths while asm loads into them could be in flight - the compiler cannot know: the hazard
// class of profiles/r05_x6_suite_soak.txt.
// The two parameters give the loop bound and the tail length: a pass that starts at t requests up to block t + 2 NS + LEAD - 2, and the steady state
// may only request whole blocks - blocks <= nblk - 1, or <= nblk - 2 when the last one may be PARTIAL: the pass runs while
// t + 2 NS + LEAD - 2 + PARTIAL < nblk.  At most 2 NS + LEAD - 2 + PARTIAL trips are left then; they run unrolled through the guarded `request` and
// `cut`, and as t is a multiple of NS there the register sets stay static in them too.
template <int NS, int LEAD, bool PARTIAL, class RQ, class CUT, class FUSED>
FN_DEVINL void x6w_trips(int nblk, RQ&& request, CUT&& cut, FUSED&& fused) {
    static_assert(LEAD >= 1 && LEAD <= NS, "a block is cut LEAD trips ahead, out of one of NS register sets");
    constexpr int REST = 2 * NS + LEAD - 2 + (PARTIAL ? 1 : 0);
    x6w_for<NS>([&](auto I) __attribute__((always_inline)) {
        if (decltype(I)::value < nblk) request(I, decltype(I)::value);
    });
    x6w_for<LEAD>([&](auto I) __attribute__((always_inline)) {
        constexpr int i = decltype(I)::value;
        if (i == 0 || i < nblk) cut(I, i, i);            // (nblk >= 1)
    });
    x6w_for<LEAD - 1>([&](auto I) __attribute__((always_inline)) {
        if (NS + decltype(I)::value < nblk) request(I, NS + decltype(I)::value);
    });
    x6w_barrier_p();
    // stage of block b = b % (LEAD + 1): a mask where that is a power of two, else a counter that follows the trips (no division in the loop; the mask
    // form, which is not carried around the loop, keeps gemm_tn_x6v_kernel at the 252 registers it had with its own loop: the counter cost two more)
    constexpr int STAGES = LEAD + 1;
    int next_stage = LEAD % STAGES, t = 0;
    auto stage_of = [&](int blk) __attribute__((always_inline)) { return (STAGES & (STAGES - 1)) == 0 ? (blk & (STAGES - 1)) : next_stage; };
    auto done = [&]() __attribute__((always_inline)) {
        next_stage = next_stage == STAGES - 1 ? 0 : next_stage + 1;
        x6w_barrier_p();
    };
#pragma unroll 1
    for (; t + REST < nblk; t += NS) {
        x6w_for<NS>([&](auto R) __attribute__((always_inline)) {
            constexpr int r = decltype(R)::value;
            fused(x6w_ic<(r + LEAD - 1) % NS>{}, t + r + NS + LEAD - 1, x6w_ic<(r + LEAD) % NS>{}, t + r + LEAD, stage_of(t + r + LEAD));
            done();
        });
    }
    x6w_for<REST>([&](auto I) __attribute__((always_inline)) {
        constexpr int i = decltype(I)::value, r = i % NS;
        if (t + i < nblk) {
            if (t + i + NS + LEAD - 1 < nblk) request(x6w_ic<(r + LEAD - 1) % NS>{}, t + i + NS + LEAD - 1);
            if (t + i + LEAD < nblk) cut(x6w_ic<(r + LEAD) % NS>{}, t + i + LEAD, stage_of(t + i + LEAD));
            done();
        }
    });
}

// Consumer wavefront of gemm_tn_x6w_kernel / gemm_nt_x6w_kernel: wave (wm, wn) multiplies sets wm (A) and 2 + wn (B) of every block into its 4 x 4
// accumulator tiles.  Operand registers: A triples of the current block and of the next one (two banks, block parity), B triples of output columns
// 0, 1 (first half of a block) and 2, 3 (second half).  While the first half of block t runs, B[2..3] of block t and A[0..1] of block t + 1 are
// read; during the second half A[2..3] and B[0..1] of block t + 1: no LDS latency is ever exposed, and no read of block t is in flight at the
// barrier that hands its stage back to the producers.
FN_DEVINL void x6w_consume(const u32x4* __restrict__ x6w_lds, int wm, int wn, int lane, int nblk, f32x4 (&acc)[4][4]) {
    bf16x8 Af[2][4][3], Bf[4][3];
    const u32x4* lA = x6w_lds + wm * X6W_SET + lane;
    const u32x4* lB = x6w_lds + (2 + wn) * X6W_SET + lane;
    auto rdA = [&](auto BANK, int stage, int a) __attribute__((always_inline)) {
        constexpr int bank = decltype(BANK)::value;
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) Af[bank][a][pc] = __builtin_bit_cast(bf16x8, lA[stage * X6W_STAGE + (a * 3 + pc) * 64]);
    };
    auto rdB = [&](int stage, int b) __attribute__((always_inline)) {
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) Bf[b][pc] = __builtin_bit_cast(bf16x8, lB[stage * X6W_STAGE + (b * 3 + pc) * 64]);
    };
    // the six products of a 32-k block, smallest first (piece 0 = hi, 1 = mid, 2 = lo): lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
    auto half = [&](auto BANK, auto B0) __attribute__((always_inline)) {      // 48 MFMAs: output columns b0, b0 + 1 of all four row tiles
        constexpr int bank = decltype(BANK)::value, b0 = decltype(B0)::value;
#pragma unroll
        for (int ap = 0; ap < 2; ++ap)                   // row tiles 0, 1 first (their A triples were read half a block earlier than those of 2, 3)
#pragma unroll
            for (int c = 0; c < 6; ++c)
#pragma unroll
                for (int a = 2 * ap; a < 2 * ap + 2; ++a)
#pragma unroll
                    for (int b = b0; b < b0 + 2; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Af[bank][a][PA[c]], Bf[b][PB[c]], acc[a][b], 0, 0, 0);
    };
    // block t (stage st), reading ahead in block t + 1 (stage st1).  The reads are unconditional - straight-line code, so that the compiler can
    // spread them between the MFMAs (sched_group_barrier) and count its LDS waits exactly; behind the last block they fetch a stage nobody uses
    auto step = [&](auto BANK, int st, int st1) __attribute__((always_inline)) {
        constexpr int bank = decltype(BANK)::value;
        const std::integral_constant<int, bank ^ 1> NB;
        rdB(st, 2);
        rdB(st, 3);
        rdA(NB, st1, 0);
        rdA(NB, st1, 1);
        half(BANK, std::integral_constant<int, 0>{});
#pragma unroll
        for (int q = 0; q < 12; ++q) {                   // 3 MFMAs : 1 read, the last 12 MFMAs of the half without (the reads land before the next half needs them)
            __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);
        rdB(st1, 0);
        rdB(st1, 1);
        rdA(NB, st1, 2);
        rdA(NB, st1, 3);
        half(BANK, std::integral_constant<int, 2>{});
#pragma unroll
        for (int q = 0; q < 12; ++q) {                   // 3 MFMAs : 1 read, the last 12 MFMAs of the half without (the reads land before the next half needs them)
            __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);
        x6w_barrier_c();
    };
    const std::integral_constant<int, 0> K0;
    const std::integral_constant<int, 1> K1;
    x6w_barrier_c();                                     // stages 0 and 1 hold blocks 0 and 1
    rdA(K0, 0, 0);                                       // (same order as the read-ahead of a step: the loop's wait counts hold for the first trip)
    rdA(K0, 0, 1);
    rdB(0, 0);
    rdB(0, 1);
    rdA(K0, 0, 2);
    rdA(K0, 0, 3);
    int st = 0;
#pragma unroll 1
    for (int t = 0; t < nblk; t += 2) {                  // one barrier per block, as many as the producers execute: 1 + nblk
        const int s1 = st == 2 ? 0 : st + 1, s2 = s1 == 2 ? 0 : s1 + 1;
        step(K0, st, s1);
        if (t + 1 < nblk) step(K1, s1, s2);
        st = s2;
    }
}

