// gemm_plan_check.cpp - the GEMM dispatch plan (csrc/gemm_plan.h, the header fn_gemm_f32 / fn_gru_dwhh_f32 launch from) on the CPU.
// Stand-alone: g++ -std=c++17 -fsanitize=address,undefined -Wall -Werror gemm_plan_check.cpp.
// Sweeps shapes, layouts, leading dimensions, address alignments, K ranges asked for, flag bits and compute-unit counts - the edges of every
// threshold of the plan and a seeded random sweep - and asks of every plan what a launch relies on:
//   the K ranges cover K exactly: (ranges - 1) klen < K <= ranges klen, no more ranges than asked for;
//   klen is a multiple of the instance's granularity (its BK, 4 rows for the TN kernels, 32 for the bf16 x 6 ones) whenever ranges > 1;
//   tiles = the output in the instance's tile shape; the grid is tiles x 1 x ranges, or tiles * ranges x 1 x 1 with ranges % 8 == 0, or - the
//   producer / consumer kernels only, compute units a multiple of 8, no FN_GEMM_X6_PERTILE - as many workgroups as compute units walking more items;
//   a reduction exists if and only if ranges > 1; the float4 one only with N % 4 == 0, ldc % 4 == 0 and aligned C / bias / workspace; its grid is
//   min(ceil(elements / 256), 2048);
//   the kernels without bounds checks get whole aligned tiles only, the TN kernels aligned row-contiguous operands only; the flags select
//   the instance they name; fn_gru_dwhh_f32 is one launch with msplit = 2H or two products without the lean instance.
#include <cstdio>
#include <initializer_list>

#include "../gemm_plan.h"

namespace {

long findings = 0, plans = 0, walked = 0;
long reached[FN_PLAN_KERNELS][2];          // per instance: unsplit / split plans seen

struct Call {
    int a_k, b_k, M, N, K, lda, ldb, ldc;
    uintptr_t A, B, C, bias, ws;
    int splitk, flags, cus;
};

void fail(const Call& c, const FnGemmPlan& p, const char* what) {
    ++findings;
    if (findings <= 20)
        std::printf("FINDING %s: a_k %d b_k %d M %d N %d K %d lda %d ldb %d ldc %d A %lu B %lu C %lu bias %lu ws %lu splitk %d flags %#x cus %d -> kernel %d klen %d "
                    "ranges %d grid %d %d %d tiles %d reduce %d x %d msplit %d\n",
                    what, c.a_k, c.b_k, c.M, c.N, c.K, c.lda, c.ldb, c.ldc, (unsigned long)c.A, (unsigned long)c.B, (unsigned long)c.C, (unsigned long)c.bias,
                    (unsigned long)c.ws, c.splitk, (unsigned)c.flags, c.cus, p.kernel, p.klen, p.ranges, p.grid_x, p.grid_y, p.grid_z, p.tiles, p.reduce,
                    p.reduce_blocks, p.msplit);
}

// tile shape and K granularity of every instance, written down here a second time on purpose
struct Shape {
    int tm, tn, gran;
};
const Shape SHAPES[FN_PLAN_KERNELS] = {{64, 64, 16}, {64, 64, 32}, {32, 64, 32}, {64, 16, 16}, {128, 128, 32}, {128, 128, 0}, {128, 128, 0},
                                       {128, 128, 0}, {128, 128, 4}, {128, 128, 4}, {128, 128, 32}, {128, 128, 32}, {128, 256, 32}};

bool al(uintptr_t bits) { return (bits & 15) == 0; }

// the invariants of one plan; `c` describes the product the plan is for (for fn_gru_dwhh_f32: the product of that launch)
void check(const Call& c, const FnGemmPlan& p, int msplit) {
    ++plans;
    if (p.kernel < 0 || p.kernel >= FN_PLAN_KERNELS) return fail(c, p, "kernel out of range");
    const Shape s = SHAPES[p.kernel];
    ++reached[p.kernel][p.ranges > 1];
    const bool x6 = (c.flags & FN_GEMM_BF16X6) != 0, pertile = (c.flags & FN_GEMM_X6_PERTILE) != 0;
    const bool walker = p.kernel == FN_PLAN_NT_X6W || p.kernel == FN_PLAN_TN_X6W || p.kernel == FN_PLAN_TN_X6V;
    const bool tn = p.kernel >= FN_PLAN_TN && p.kernel <= FN_PLAN_TN_X6V;
    const bool whole = p.kernel == FN_PLAN_NT_DIRECT_4_2 || p.kernel == FN_PLAN_NT_DIRECT_1_4 || p.kernel == FN_PLAN_NT_X6W;
    // K ranges
    if (p.klen < 1 || p.ranges < 1 || (long)(p.ranges - 1) * p.klen >= c.K || (long)p.ranges * p.klen < c.K) fail(c, p, "the K ranges do not cover K");
    if (p.ranges > (c.splitk > 1 ? c.splitk : 1)) fail(c, p, "more K ranges than asked for");
    if (p.ranges > 1 && (s.gran == 0 || p.klen % s.gran != 0)) fail(c, p, "klen is not a multiple of the instance's granularity");
    // tiles and grid
    const long tiles = (long)((c.M + s.tm - 1) / s.tm) * ((c.N + s.tn - 1) / s.tn);
    if (p.tiles != tiles) fail(c, p, "tiles");
    const long items = tiles * p.ranges;
    const bool g3 = p.grid_x == tiles && p.grid_y == 1 && p.grid_z == p.ranges;
    const bool g1 = tn && p.ranges > 1 && (p.ranges & 7) == 0 && p.grid_x == items && p.grid_y == 1 && p.grid_z == 1;
    const bool walk = walker && !pertile && c.cus >= 8 && (c.cus & 7) == 0 && items > c.cus && p.grid_x == c.cus && p.grid_y == 1 && p.grid_z == 1 &&
                      (p.kernel == FN_PLAN_NT_X6W || (p.ranges & 7) == 0);
    walked += walk;
    if (!g3 && !g1 && !walk) fail(c, p, "the grid neither covers tiles x ranges nor is the walking form");
    if (tn && p.ranges > 1 && (p.ranges & 7) == 0 && g3) fail(c, p, "K ranges in multiples of 8 belong on the 1-D grid");
    if (walker && !pertile && c.cus >= 8 && (c.cus & 7) == 0 && items > c.cus && (p.kernel == FN_PLAN_NT_X6W || (p.ranges & 7) == 0) && !walk)
        fail(c, p, "more items than compute units: one workgroup per compute unit");
    // reduction
    if ((p.reduce != FN_PLAN_REDUCE_NONE) != (p.ranges > 1)) fail(c, p, "a reduction exists if and only if ranges > 1");
    if (p.reduce == FN_PLAN_REDUCE_NONE) {
        if (p.reduce_blocks != 0) fail(c, p, "reduce_blocks without a reduction");
    } else {
        const bool v4 = (c.N % 4) == 0 && (c.ldc % 4) == 0 && al(c.C | c.bias | c.ws);
        if (p.reduce != (v4 ? FN_PLAN_REDUCE_SLAB4 : FN_PLAN_REDUCE_SLAB)) fail(c, p, "the float4 reduction exactly where everything is aligned");
        const long total = (long)c.M * c.N / (v4 ? 4 : 1), blocks = (total + 255) / 256;
        if (p.reduce_blocks != (blocks < 2048 ? blocks : 2048) || p.reduce_blocks < 1) fail(c, p, "reduce_blocks");
    }
    // what the kernels rely on
    if (whole && !(c.a_k && c.b_k && c.M % 128 == 0 && c.N % 128 == 0 && c.lda % 4 == 0 && c.ldb % 4 == 0 && c.ldc % 4 == 0 && al(c.A | c.B | c.C | c.bias) &&
                   p.ranges == 1 && c.K % (p.kernel == FN_PLAN_NT_X6W ? 32 : 16) == 0))
        fail(c, p, "a kernel without bounds checks on ragged or misaligned operands");
    if (tn && !(!c.a_k && !c.b_k && c.lda % 4 == 0 && c.ldb % 4 == 0 && al(c.A | c.B))) fail(c, p, "a TN kernel on operands that are not aligned and row-contiguous");
    if ((p.kernel == FN_PLAN_STAGED_32_64_32 || p.kernel == FN_PLAN_STAGED_64_16_16) && !(c.a_k && c.b_k)) fail(c, p, "an NT-only staged instance in another layout");
    if ((p.kernel == FN_PLAN_NT_X6W || p.kernel >= FN_PLAN_TN_X6) && !x6) fail(c, p, "a bf16 x 6 kernel without FN_GEMM_BF16X6");
    if (tn && x6 != (p.kernel >= FN_PLAN_TN_X6)) fail(c, p, "FN_GEMM_BF16X6 on the TN form selects a bf16 x 6 kernel");
    if (tn && x6 && ((c.flags & FN_GEMM_X6_PERWAVE) != 0) != (p.kernel == FN_PLAN_TN_X6)) fail(c, p, "FN_GEMM_X6_PERWAVE");
    if (p.kernel == FN_PLAN_TN_X6V && !(c.flags & FN_GEMM_X6_WIDE)) fail(c, p, "wide tiles without FN_GEMM_X6_WIDE");
    if ((p.kernel == FN_PLAN_TN || p.kernel == FN_PLAN_TN_LEAN) && ((c.flags & FN_GEMM_LEAN) != 0) != (p.kernel == FN_PLAN_TN_LEAN)) fail(c, p, "FN_GEMM_LEAN on the TN form");
    if (p.kernel == FN_PLAN_NT_DIRECT_1_4 && !(c.flags & FN_GEMM_LEAN)) fail(c, p, "the lean LDS-free instance without FN_GEMM_LEAN");
    if (p.msplit != msplit) fail(c, p, "msplit");
}

void run(const Call& c) { check(c, gemm_plan(c.a_k, c.b_k, c.M, c.N, c.K, c.lda, c.ldb, c.ldc, c.A, c.B, c.C, c.bias, c.ws, c.splitk | c.flags, c.cus), 0); }

void run_dwhh(int H, int rows, uintptr_t dgx, uintptr_t dghn, uintptr_t hp, uintptr_t dW, uintptr_t ws, int splitk, int flags, int cus) {
    const DwhhPlan d = dwhh_plan(H, rows, dgx, dghn, hp, dW, ws, splitk | flags, cus);
    Call c{0, 0, 3 * H, H, rows, 3 * H, H, H, dgx, hp, dW, 0, ws, splitk, flags, cus};
    const bool one = (2 * H) % 128 == 0 && H % 4 == 0 && al(dgx | dghn | hp);
    if (d.n != (one ? 1 : 2)) {
        ++plans;
        return fail(c, d.launch[0], "fn_gru_dwhh_f32: one launch exactly when the dghn band starts on a tile boundary and the sources are aligned");
    }
    if (d.n == 1) return check(c, d.launch[0], 2 * H);
    c.flags &= ~FN_GEMM_LEAN;                 // the two products do not carry the lean bit on
    c.M = 2 * H;
    check(c, d.launch[0], 0);
    c.M = H; c.lda = H; c.A = dghn; c.C = dW + (uintptr_t)8 * H * H;
    check(c, d.launch[1], 0);
}

unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
unsigned rnd(unsigned n) {          // [0, n)
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)((rng_state >> 33) % n);
}

const int FLAGS[] = {0, FN_GEMM_LEAN, FN_GEMM_BF16X6, FN_GEMM_BF16X6 | FN_GEMM_LEAN, FN_GEMM_BF16X6 | FN_GEMM_X6_WIDE, FN_GEMM_BF16X6 | FN_GEMM_X6_PERWAVE,
                     FN_GEMM_BF16X6 | FN_GEMM_X6_PERTILE, FN_GEMM_BF16X6 | FN_GEMM_X6_WIDE | FN_GEMM_X6_PERTILE, FN_GEMM_BF16X6 | FN_GEMM_X6_WIDE | FN_GEMM_X6_PERWAVE};
const int CUS[] = {256, 250, 304, 8, 7, 1, 64};
const int SPLITS[] = {1, 2, 3, 8, 12, 16, 42, 43, 64, 0};
const int DIMS[] = {1, 3, 15, 16, 17, 63, 64, 65, 70, 127, 128, 130, 200, 256, 342, 512, 1536, 1920, 2048, 4096, 16384};
const int KS[] = {1, 3, 4, 15, 16, 31, 32, 37, 63, 64, 80, 96, 127, 128, 160, 513, 1031, 4096, 4100, 65536};

template <class T, int n>
T pick(const T (&a)[n]) {
    return a[rnd(n)];
}

}  // namespace

int main() {
    // every pair of sizes around the thresholds, dense and aligned, in every layout, flag set and split
    for (int lay = 0; lay < 4; ++lay)
        for (int M : DIMS)
            for (int N : DIMS)
                for (int K : KS)
                    for (int fl : FLAGS)
                        for (int sk : {1, 8, 12}) {
                            const int a_k = lay & 1, b_k = lay >> 1;
                            run(Call{a_k, b_k, M, N, K, a_k ? K : M, b_k ? K : N, N, 0, 0, 0, 0, 0, sk, fl, 256});
                        }
    // the seeded sweep: ragged sizes, padded and odd leading dimensions, addresses on and off 16-byte boundaries, every compute-unit count
    for (int i = 0; i < 400000; ++i) {
        const int a_k = rnd(2), b_k = rnd(2);
        const int M = rnd(4) ? 1 + rnd(600) : pick(DIMS), N = rnd(4) ? 1 + rnd(600) : pick(DIMS), K = rnd(4) ? 1 + rnd(4096) : pick(KS);
        const int pad[] = {0, 0, 4, 1, 2, 8};
        const uintptr_t off[] = {0, 0, 0, 4, 8, 16};
        run(Call{a_k, b_k, M, N, K, (a_k ? K : M) + pick(pad), (b_k ? K : N) + pick(pad), N + pick(pad), 4096 + pick(off), 8192 + pick(off), 12288 + pick(off),
                 rnd(3) ? 16384 + pick(off) : 0, 1 << 20 | pick(off), pick(SPLITS), pick(FLAGS), pick(CUS)});
    }
    // fn_gru_dwhh_f32
    for (int H : {4, 30, 32, 64, 96, 100, 128, 192, 256, 512, 1000})
        for (int rows : {1, 37, 1030, 4096, 65280, 65536})
            for (int fl : FLAGS)
                for (int sk : SPLITS)
                    for (int cus : CUS)
                        for (uintptr_t o : {0, 4}) {
                            run_dwhh(H, rows, 4096, 8192 + o, 12288, 16384, 1 << 20, sk, fl, cus);
                            run_dwhh(H, rows, 4096 + o, 8192, 12288, 16384 + 8, 1 << 20, sk, fl, cus);
                        }
    for (int i = 0; i < 100000; ++i)
        run_dwhh(1 + rnd(600), 1 + rnd(70000), 4096 + 4 * rnd(5), 8192 + 4 * rnd(5), 12288 + 4 * rnd(5), 16384 + 4 * rnd(5), 1 << 20 | 4 * rnd(5), pick(SPLITS),
                 pick(FLAGS), pick(CUS));
    // the sweep reached every instance, every instance that can split in a split launch too, and the walking form
    for (int k = 0; k < FN_PLAN_KERNELS; ++k)
        if (!reached[k][0] || (SHAPES[k].gran != 0 && k != FN_PLAN_STAGED_32_64_32 && k != FN_PLAN_STAGED_64_16_16 && k != FN_PLAN_STAGED_64_64_32 && !reached[k][1])) {
            ++findings;
            std::printf("FINDING the sweep never reached kernel %d (unsplit %ld, split %ld)\n", k, reached[k][0], reached[k][1]);
        }
    if (!walked) {
        ++findings;
        std::printf("FINDING the sweep never reached the walking form\n");
    }
    std::printf("%ld plans, %ld findings\n", plans, findings);
    return findings ? 1 : 0;
}
