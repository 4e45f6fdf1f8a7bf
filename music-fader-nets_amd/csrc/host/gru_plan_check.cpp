// gru_plan_check.cpp - the GRU launch plans (csrc/gru_plan.h, the header fn_gru_seq_fwd / fn_gru_seq_bwd / fn_gru_cell_f32 launch from) on the CPU.
// Stand-alone: g++ -std=c++17 -fsanitize=address,undefined -Wall -Werror gru_plan_check.cpp.
//
// 1. The return codes, written down before the code moved: which FN_E_* a call with one or several faults returns (the order of the checks).
// 2. Scans, forward and backward: n_scans 1-8 x B x H x T x variant bits and forced row blocks x compute units x cu_budget, each operand of the
//    16-byte epilogue vectors misaligned in turn, gates / input sources present or absent, and a seeded sweep of mixed scans.  Of every plan:
//      grid == groups x slices, groups = sum ceil(B / rows_per_group); groups <= FN_MAX_GROUPS, 2 groups <= FN_MAX_GROUPS for the ping-pong kernels;
//      LDS <= 160 KB - 64; a resident candidate has groups x slices <= the launch's compute units; full row groups where the kernel has no partial ones;
//      no resident candidate with a misaligned operand, without sync_ws, at H > 512, mixed H or T < 2; the per-step candidate is the last one and is
//      there unless bf16 x 6 was asked for; bf16 x 6: one candidate or FN_E_UNSUPPORTED; fn_gru_*_x6_ok <=> the bf16 x 6 plan of the same shapes with
//      aligned operands and a sync_ws has a candidate; the per-step configuration is one of the two instances per direction.
// 3. The cell: B x H x K1 x variants 0-19 with and without FN_GRU_BF16X6 x alignments x token table / row bias.  Of every plan: the grid covers
//    B x H in the family's tile, LDS <= 160 KB, a family without bounds-checked staging only on aligned operands, forced_honoured exactly when the
//    variant names a form of the family that runs.
#include <cstdio>
#include <initializer_list>

#include "../gru_plan.h"

namespace {

long findings = 0, plans = 0;
long reached[FN_GRU_KERNELS], cell_reached[5][2];

void fail(const char* what, const char* dir, int n, int B, int H, int T, int variant, int cus, int budget, const FnGruPlan& p) {
    if (++findings > 20) return;
    std::printf("FINDING %s: %s n %d B %d H %d T %d variant %#x cus %d budget %d -> status %d n %d absent %d", what, dir, n, B, H, T, (unsigned)variant, cus, budget,
                p.status, p.n, p.ws_absent);
    for (int i = 0; i < p.n; ++i)
        std::printf(" [kernel %d rows %d groups %d slices %d grid %d lds %d]", p.cand[i].kernel, p.cand[i].rows_per_group, p.cand[i].groups, p.cand[i].slices,
                    p.cand[i].grid, p.cand[i].lds_bytes);
    std::printf("\n");
}

// what the instances are, written down here a second time on purpose: slices (0 = H / 16), ping-pong (two groups per counter pair), full row groups only
struct Inst {
    int slices, pingpong, full_groups, x6, rows;      // rows: the row block of the instance (0: per-step)
};
const Inst INSTS[FN_GRU_KERNELS] = {
    {0, 1, 1, 1, 128}, {0, 1, 1, 1, 64}, {0, 0, 1, 1, 64}, {0, 0, 1, 1, 128}, {0, 1, 1, 0, 128}, {0, 1, 1, 0, 64},
    {0, 0, 0, 0, 128}, {0, 0, 0, 0, 64}, {0, 0, 0, 0, 64}, {0, 0, 0, 0, 32}, {0, 0, 0, 0, 16}, {0, 0, 0, 0, 0},
    {16, 0, 1, 1, 32}, {16, 0, 1, 1, 64}, {16, 0, 1, 0, 32}, {16, 0, 1, 0, 64},
    {0, 0, 0, 0, 128}, {0, 0, 0, 0, 64}, {0, 0, 0, 0, 64}, {0, 0, 0, 0, 32}, {0, 0, 0, 0, 16}, {0, 0, 0, 0, 0},
};

alignas(16) char mem[64];
void* const OK = mem;            // a 16-byte aligned address
void* const OFF = mem + 4;       // ... and one 4 bytes behind it

struct Case {
    int n, variant, cus, budget, bad;      // bad: index of the epilogue operand that is misaligned (-1: none)
    bool gates, table, dense, sync;
    int B[FN_MAX_SCANS], H[FN_MAX_SCANS], T[FN_MAX_SCANS];
};

void make_fwd(const Case& c, FnGruFwd* sc) {
    for (int s = 0; s < c.n; ++s) {
        FnGruFwd d{};
        d.B = c.B[s]; d.T = c.T[s]; d.H = c.H[s];
        d.w_hh_frag = (const float*)OK; d.frag_ws = (float*)OK;
        const void* ops[8] = {OK, OK, OK, c.dense ? OK : nullptr, c.table ? OK : nullptr, OK, OK, c.gates ? OK : nullptr};
        if (c.bad >= 0 && c.bad < 8 && s == c.n - 1 && ops[c.bad]) ops[c.bad] = OFF;
        d.b_hh = (const float*)ops[0]; d.b_ih = (const float*)ops[1]; d.h0 = (const float*)ops[2]; d.gx_dense = (const float*)ops[3];
        d.gx_table = (const float*)ops[4]; d.gx_rowbias = (const float*)ops[5]; d.h_all = (float*)ops[6]; d.gates = (float*)ops[7];
        d.idx = (const int32_t*)OK; d.idx_ld = 1;
        d.sync_ws = c.sync ? OK : nullptr;
        d.cu_budget = c.budget; d.variant = c.variant;
        sc[s] = d;
    }
}
void make_bwd(const Case& c, FnGruBwd* sc) {
    for (int s = 0; s < c.n; ++s) {
        FnGruBwd d{};
        d.B = c.B[s]; d.T = c.T[s]; d.H = c.H[s];
        d.w_hh_t_frag = (const float*)OK; d.frag_ws = (float*)OK; d.scratch = (float*)OK;
        const void* ops[10] = {OK, OK, OK, OK, c.dense ? OK : nullptr, OK, OK, c.table ? OK : nullptr, OK, OK};      // dense: dh_ext, table: dh0
        if (c.bad >= 0 && s == c.n - 1 && ops[c.bad]) ops[c.bad] = OFF;
        d.h0 = (const float*)ops[0]; d.h_all = (const float*)ops[1]; d.gates = (const float*)ops[2]; d.dh_last = (const float*)ops[3];
        d.dh_ext = (const float*)ops[4]; d.dgx_all = (float*)ops[5]; d.dghn_all = (float*)ops[6]; d.dh0 = (float*)ops[7];
        d.dgx_rowsum = (float*)ops[8]; d.dghn_rowsum = (float*)ops[9];
        d.sync_ws = c.sync ? OK : nullptr;
        d.cu_budget = c.budget; d.variant = c.variant;
        sc[s] = d;
    }
}

// the invariants of one scan plan
void check(const Case& c, const FnGruPlan& p, bool back, bool misaligned) {
    ++plans;
    const char* dir = back ? "bwd" : "fwd";
#define FAIL(what) return fail(what, dir, c.n, c.B[0], c.H[0], c.T[0], c.variant, c.cus, c.budget, p)
    const bool x6 = (c.variant & FN_GRU_BF16X6) != 0;
    if (p.status != FN_OK && !(x6 && p.status == FN_E_UNSUPPORTED && p.n == 0)) FAIL("status of valid arguments");
    if (p.status != FN_OK) return;
    const int cus = c.budget > 0 && c.budget < c.cus ? c.budget : c.cus;
    if (p.cus != cus) FAIL("compute units of the launch");
    if (p.n < 1 || p.n > 3) FAIL("candidate count");
    if (x6 && (p.n != 1 || !p.cand[0].resident)) FAIL("bf16 x 6: exactly one resident candidate");
    int Tmax = 0, Tmin = 1 << 30;
    bool mixed = false;
    for (int s = 0; s < c.n; ++s) {
        Tmax = c.T[s] > Tmax ? c.T[s] : Tmax;
        Tmin = c.T[s] < Tmin ? c.T[s] : Tmin;
        mixed = mixed || c.H[s] != c.H[0];
    }
    for (int i = 0; i < p.n; ++i) {
        const FnGruCandidate& k = p.cand[i];
        const int lo = back ? FN_GRU_BWD_X6_1 : 0, hi = back ? FN_GRU_BWD_STEP : FN_GRU_FWD_STEP;
        if (k.kernel < lo || k.kernel > hi) FAIL("kernel of the other direction");
        ++reached[k.kernel];
        const Inst& in = INSTS[k.kernel];
        if (!k.resident) {
            if (i != p.n - 1 || k.kernel != hi) FAIL("the per-step candidate is not the last one");
            if (x6) FAIL("bf16 x 6 with a per-step candidate");
            const bool two = back ? ((k.tm == 4 && k.tn == 1 && k.d == 2) || (k.tm == 2 && k.tn == 1 && k.d == 3)) : ((k.tm == 4 && k.d == 1) || (k.tm == 2 && k.d == 3)) && k.tn == 0;
            if (!two) FAIL("a per-step configuration that is not built");
            if (k.ns != 1 && k.ns != 3 && k.ns != 4 && k.ns != 8) FAIL("scan slots");
            if (k.ns < c.n && k.launches > 0 && Tmin == Tmax && !back) FAIL("fewer scan slots than active scans");
            if (k.tiles < 1 || k.launches < Tmax || k.launches > Tmax + 1) FAIL("per-step tiles / launches");
            continue;
        }
        if (i == p.n - 1 && !x6) FAIL("no per-step candidate behind the resident ones");
        if (k.kernel == hi) FAIL("a resident per-step candidate");
        if (x6 != (in.x6 != 0)) FAIL("arithmetic of the instance");
        if ((k.h0_triples != 0) != x6) FAIL("packing of the initial states");
        const int slices = in.slices ? in.slices : c.H[0] / 16;
        long groups = 0;
        bool full = true;
        for (int s = 0; s < c.n; ++s) {
            groups += (c.B[s] + k.rows_per_group - 1) / k.rows_per_group;
            full = full && c.B[s] % k.rows_per_group == 0;
        }
        if (k.rows_per_group != in.rows) FAIL("row block of the instance");
        if (k.groups != groups || k.slices != slices || k.grid != groups * slices) FAIL("grid != groups x slices");
        if (groups > FN_MAX_GROUPS || (in.pingpong && 2 * groups > FN_MAX_GROUPS) || (in.slices == 16 && groups > 16)) FAIL("more row groups than counter lines");
        if (k.lds_bytes <= 0 || k.lds_bytes > 160 * 1024 - 64) FAIL("LDS");
        if (k.grid > cus) FAIL("a resident candidate beyond one workgroup per compute unit");
        if (in.full_groups && (!full || Tmin < 2 || c.H[0] != 512)) FAIL("partial row groups / T < 2 / H != 512 for a kernel without them");
        if (misaligned || !c.sync || c.H[0] > 512 || mixed || Tmax < 2) FAIL("a resident candidate that must be absent");
        if ((c.variant & FN_GRU_ROWS_MASK) && !x6 && k.rows_per_group != (c.variant & FN_GRU_ROWS_MASK)) FAIL("not the forced row block");
        if (k.no_hand != ((c.variant & FN_GRU_COMPILER_LOOPS) && !x6 ? 1 : 0) && in.slices == 0) FAIL("no_hand");
        if ((c.variant & (FN_GRU_COMPILER_LOOPS | FN_GRU_NO_PINGPONG)) && !x6 && (in.pingpong || in.slices == 16)) FAIL("a ping-pong form although switched off");
    }
    if ((p.ws_absent == FN_GRU_WS_PRESENT) != (p.cand[0].resident != 0)) FAIL("ws_absent");
#undef FAIL
}

void run_case(Case c) {
    FnGruFwd f[FN_MAX_SCANS];
    FnGruBwd b[FN_MAX_SCANS];
    make_fwd(c, f);
    make_bwd(c, b);
    bool fbad = false, bbad = false;
    for (int s = 0; s < c.n; ++s) {
        fbad = fbad || (ws_align_mask(f[s]) & 15);
        bbad = bbad || (ws_align_mask(b[s]) & 15);
    }
    const FnGruPlan pf = gru_fwd_plan(f, c.n, c.cus), pb = gru_bwd_plan(b, c.n, c.cus);
    check(c, pf, false, fbad);
    check(c, pb, true, bbad);
    if ((c.variant & FN_GRU_BF16X6) && c.bad < 0 && c.sync) {      // shapes only: the answer of fn_gru_*_x6_ok is the plan's
        if ((gru_fwd_x6_ok(f, c.n, c.cus) != 0) != (pf.n == 1)) fail("fn_gru_fwd_x6_ok disagrees with the plan", "fwd", c.n, c.B[0], c.H[0], c.T[0], c.variant, c.cus, c.budget, pf);
        // (backward: on fewer than 32 compute units fn_gru_bwd_x6_ok goes by the 16 slices of the kernel while the launch asks for H / 16 = 32 of them -
        // the answers differ there, as they always did; callers repeat a refused launch on the fp32 kernels)
        if (pb.cus < 32 ? pb.n != 0 : (gru_bwd_x6_ok(b, c.n, c.cus) != 0) != (pb.n == 1)) fail("fn_gru_bwd_x6_ok disagrees with the plan", "bwd", c.n, c.B[0], c.H[0], c.T[0], c.variant, c.cus, c.budget, pb);
    }
}

const int BS[] = {1, 16, 31, 32, 33, 64, 128, 200, 256, 512}, HS[] = {32, 64, 96, 512, 544}, TS[] = {1, 2, 3, 70};
const int CUS[] = {16, 31, 32, 128, 248, 256, 304}, BUDGETS[] = {0, 128}, ROWS[] = {0, 16, 32, 64, 128, 5};
const int BITS[] = {0, FN_GRU_ALT_TILING, FN_GRU_SYNC_ZEROED, FN_GRU_COMPILER_LOOPS, FN_GRU_NO_PINGPONG, FN_GRU_SPREAD_XCDS, FN_GRU_NO_RS_BWD, FN_GRU_BF16X6,
                    FN_GRU_BF16X6 | FN_GRU_X6_SINGLE_GROUP};

void sweep_scans() {
    for (int n = 1; n <= FN_MAX_SCANS; ++n)
        for (const int B : BS)
            for (const int H : HS)
                for (const int T : TS)
                    for (const int cus : CUS)
                        for (const int budget : BUDGETS) {
                            Case c{};
                            c.n = n; c.cus = cus; c.budget = budget; c.bad = -1;
                            c.gates = c.table = c.sync = true;
                            for (int s = 0; s < n; ++s) c.B[s] = B, c.H[s] = H, c.T[s] = T;
                            for (const int bits : BITS)
                                for (const int rows : ROWS) {
                                    c.variant = bits | rows;
                                    run_case(c);
                                }
                            // every alignment mask on and off; gates / sources / sync_ws present or absent (on two chip sizes: the masks do not depend on it)
                            if (budget || (cus != 128 && cus != 256)) continue;
                            for (const int bits : {0, (int)FN_GRU_BF16X6}) {
                                c.variant = bits;
                                for (c.bad = 0; c.bad < 10; ++c.bad) run_case(c);
                                c.bad = -1;
                                for (int src = 1; src < 4; ++src)
                                    for (int g = 0; g < 4; ++g) {
                                        c.table = src & 1; c.dense = src & 2; c.gates = g & 1; c.sync = g & 2;
                                        run_case(c);
                                    }
                                c.gates = c.table = c.sync = true; c.dense = false;
                            }
                        }
    // seeded sweep of mixed scans
    unsigned long long st = 0x9E3779B97F4A7C15ull;
    auto rnd = [&st](int m) { st = st * 6364136223846793005ull + 1442695040888963407ull; return (int)((st >> 33) % (unsigned)m); };
    for (int it = 0; it < 100000; ++it) {
        Case c{};
        c.n = 1 + rnd(8); c.cus = CUS[rnd(7)]; c.budget = BUDGETS[rnd(2)]; c.bad = rnd(4) ? -1 : rnd(10);
        c.variant = BITS[rnd(9)] | BITS[rnd(7)] | ROWS[rnd(6)];
        c.gates = rnd(8) != 0; c.table = rnd(2); c.dense = !c.table || !rnd(8); c.sync = rnd(16) != 0;
        const int H = HS[rnd(5)], T = TS[rnd(4)], B = BS[rnd(10)];
        for (int s = 0; s < c.n; ++s) c.B[s] = rnd(3) ? B : BS[rnd(10)], c.H[s] = rnd(40) ? H : HS[rnd(5)], c.T[s] = rnd(3) ? T : TS[rnd(4)];
        run_case(c);
    }
}

// ---- the return codes ---------------------------------------------------------------------------------------------------------------------
int codes = 0;
void expect(int got, int want, const char* what) {
    ++codes;
    if (got != want) {
        ++findings;
        std::printf("FINDING return code of `%s`: %d, expected %d\n", what, got, want);
    }
}

void check_codes() {
    Case c{};
    c.n = 2; c.cus = 256; c.bad = -1; c.gates = c.table = c.sync = true;
    for (int s = 0; s < 2; ++s) c.B[s] = 256, c.H[s] = 512, c.T[s] = 8;
    FnGruFwd f[FN_MAX_SCANS + 1];
    auto fwd = [&](auto&& edit) { make_fwd(c, f); edit(); return gru_fwd_plan(f, c.n, 256).status; };
    expect(gru_fwd_plan(nullptr, 1, 256).status, FN_E_NULL, "fwd: no scans");
    expect(gru_fwd_plan(f, 0, 256).status, FN_E_COUNT, "fwd: n_scans 0");
    expect(gru_fwd_plan(f, FN_MAX_SCANS + 1, 256).status, FN_E_COUNT, "fwd: n_scans 9");
    expect(fwd([] {}), FN_OK, "fwd: valid");
    expect(fwd([&] { f[0].b_hh = nullptr; f[0].B = 0; }), FN_E_NULL, "fwd: b_hh NULL before B = 0");
    expect(fwd([&] { f[0].h_all = nullptr; }), FN_E_NULL, "fwd: h_all NULL");
    expect(fwd([&] { f[0].frag_ws = nullptr; }), FN_E_NULL, "fwd: frag_ws NULL");
    expect(fwd([&] { f[0].w_hh_frag = nullptr; }), FN_E_NULL, "fwd: w_hh_frag NULL");
    expect(fwd([&] { f[0].H = 48; f[0].idx = nullptr; }), FN_E_SHAPE, "fwd: H % 32 before a table without idx");
    expect(fwd([&] { f[0].T = 0; }), FN_E_SHAPE, "fwd: T = 0");
    expect(fwd([&] { f[0].idx = nullptr; f[0].frag_ws = (float*)OFF; }), FN_E_NULL, "fwd: table without idx before a misaligned frag_ws");
    expect(fwd([&] { f[0].w_hh_frag = (const float*)OFF; }), FN_E_ALIGN, "fwd: misaligned w_hh_frag");
    expect(fwd([&] { f[0].h_last_frag = (float*)OFF; f[0].h0_frag = (const float*)OK; f[0].h0 = nullptr; }), FN_E_ALIGN, "fwd: misaligned h_last_frag before h0_frag without h0");
    expect(fwd([&] { f[0].h0_frag = (const float*)OK; f[0].h0 = nullptr; }), FN_E_NULL, "fwd: h0_frag without h0");
    expect(fwd([&] { f[0].h0_frag = (const float*)OFF; f[1].b_hh = nullptr; }), FN_E_ALIGN, "fwd: scan 0's fault before scan 1's");
    expect(fwd([&] { f[1].B = -1; }), FN_E_SHAPE, "fwd: scan 1's B");
    expect(fwd([&] { f[0].h_all = (float*)OFF; }), FN_OK, "fwd: a misaligned epilogue operand runs per step");
    expect(fwd([&] { f[0].variant = FN_GRU_BF16X6; }), FN_OK, "fwd: bf16 x 6, eligible");
    expect(fwd([&] { f[0].variant = FN_GRU_BF16X6; f[0].h_all = (float*)OFF; }), FN_E_UNSUPPORTED, "fwd: bf16 x 6, misaligned epilogue operand");
    expect(fwd([&] { f[0].variant = FN_GRU_BF16X6; f[0].sync_ws = nullptr; }), FN_E_UNSUPPORTED, "fwd: bf16 x 6 without sync_ws");
    expect(fwd([&] { f[0].variant = FN_GRU_BF16X6; f[1].gates = nullptr; }), FN_E_UNSUPPORTED, "fwd: bf16 x 6 without saved gates");
    expect(fwd([&] { f[0].variant = FN_GRU_BF16X6; f[1].B = 200; }), FN_E_UNSUPPORTED, "fwd: bf16 x 6, partial row group");
    expect(fwd([&] { f[0].variant = FN_GRU_BF16X6; f[0].B = 0; }), FN_E_SHAPE, "fwd: bf16 x 6, B = 0 first");

    FnGruBwd b[FN_MAX_SCANS + 1];
    auto bwd = [&](auto&& edit) { make_bwd(c, b); edit(); return gru_bwd_plan(b, c.n, 256).status; };
    expect(gru_bwd_plan(nullptr, 1, 256).status, FN_E_NULL, "bwd: no scans");
    expect(gru_bwd_plan(b, 0, 256).status, FN_E_COUNT, "bwd: n_scans 0");
    expect(gru_bwd_plan(b, FN_MAX_SCANS + 1, 256).status, FN_E_COUNT, "bwd: n_scans 9");
    expect(bwd([] {}), FN_OK, "bwd: valid");
    expect(bwd([&] { b[0].gates = nullptr; b[0].H = 48; }), FN_E_NULL, "bwd: gates NULL before H % 32");
    expect(bwd([&] { b[0].scratch = nullptr; }), FN_E_NULL, "bwd: scratch NULL");
    expect(bwd([&] { b[0].dgx_all = nullptr; }), FN_E_NULL, "bwd: dgx_all NULL");
    expect(bwd([&] { b[0].H = 48; b[0].frag_ws = (float*)OFF; }), FN_E_SHAPE, "bwd: H % 32 before a misaligned frag_ws");
    expect(bwd([&] { b[0].w_hh_t_frag = (const float*)OFF; b[1].h_all = nullptr; }), FN_E_ALIGN, "bwd: scan 0's fault before scan 1's");
    expect(bwd([&] { b[1].dghn_all = (float*)OFF; }), FN_OK, "bwd: a misaligned epilogue operand runs per step");
    expect(bwd([&] { b[0].variant = FN_GRU_BF16X6; }), FN_E_UNSUPPORTED, "bwd: bf16 x 6, 8 groups on the whole chip");
    expect(bwd([&] { b[0].variant = FN_GRU_BF16X6; b[0].cu_budget = 128; }), FN_OK, "bwd: bf16 x 6, 8 groups on half of the chip");
    expect(bwd([&] { b[0].variant = FN_GRU_BF16X6 | FN_GRU_X6_BWD_32ROWS; }), FN_OK, "bwd: bf16 x 6, 32-row groups on request");
    expect(bwd([&] { b[0].variant = FN_GRU_BF16X6 | FN_GRU_X6_BWD_32ROWS; b[0].sync_ws = nullptr; }), FN_E_UNSUPPORTED, "bwd: bf16 x 6 without sync_ws");

    alignas(16) static char big[64];
    FnGruCell k{};
    auto cell = [&](auto&& edit) {
        k = FnGruCell{};
        k.B = 1024; k.H = 512; k.ldh = k.ldo = k.ldw_hh = 512;
        k.h_prev = (const float*)OK; k.w_hh = (const float*)OK; k.b_hh = (const float*)OK; k.h_out = (float*)big;
        edit();
        return gru_cell_plan(&k).status;
    };
    expect(gru_cell_plan(nullptr).status, FN_E_NULL, "cell: no descriptor");
    expect(cell([] {}), FN_OK, "cell: valid");
    expect(cell([&] { k.b_hh = nullptr; k.B = 0; }), FN_E_NULL, "cell: b_hh NULL before B = 0");
    expect(cell([&] { k.H = 48; }), FN_E_SHAPE, "cell: H % 32");
    expect(cell([&] { k.ldo = 500; }), FN_E_SHAPE, "cell: ldo < H");
    expect(cell([&] { k.x = (const float*)OK; k.K1 = 16; k.ldx = 16; k.ldw_ih = 16; }), FN_E_SHAPE, "cell: x without w_ih");
    expect(cell([&] { k.x = (const float*)OK; k.w_ih = (const float*)OK; k.K1 = 16; k.ldx = 8; k.ldw_ih = 16; }), FN_E_SHAPE, "cell: ldx < K1");
    expect(cell([&] { k.gx_table = (const float*)OK; k.idx = (const int32_t*)OK; }), FN_E_SHAPE, "cell: idx with idx_ld 0");
    expect(cell([&] { k.h_out = (float*)OK; }), FN_E_SHAPE, "cell: h_out aliases h_prev");
    expect(cell([&] { k.idx_best = (const uint64_t*)OK; k.best_v = 4; }), FN_E_SHAPE, "cell: idx_best without a table");
    expect(cell([&] { k.idx_best = (const uint64_t*)OK; k.gx_table = (const float*)OK; }), FN_E_SHAPE, "cell: idx_best with best_v 0");
    expect(cell([&] { k.h_prev = (const float*)OFF; k.variant = 5; }), FN_OK, "cell: a misaligned operand runs the staged default");
}

// ---- the cell -----------------------------------------------------------------------------------------------------------------------------
void cell_fail(const char* what, const FnGruCell& c, bool aligned, const FnGruCellPlan& p) {
    if (++findings > 20) return;
    std::printf("FINDING cell %s: B %d H %d K1 %d variant %#x aligned %d tab %d rb %d -> family %d <%d, %d, %d> grid %d lds %d honoured %d\n", what, c.B, c.H,
                c.x ? c.K1 : 0, (unsigned)c.variant, aligned, c.gx_table != nullptr, c.gx_rowbias != nullptr, p.family, p.t0, p.t1, p.t2, p.grid, p.lds_bytes,
                p.forced_honoured);
}

void sweep_cells() {
    alignas(16) static char out[64];
    for (const int B : {1, 70, 512, 513, 1024, 1025, 1536, 1537, 2048, 2049})
        for (const int H : {32, 96, 288, 512})
            for (const int K1 : {0, 16, 48, 272, 512, 1024})
                for (int v = 0; v < 20; ++v)
                    for (const int x6 : {0, (int)FN_GRU_BF16X6})
                        for (int bad = -1; bad < 12; ++bad)
                            for (int tr = 0; tr < 4; ++tr) {
                                FnGruCell c{};
                                c.B = B; c.H = H; c.variant = v | x6;
                                c.ldh = c.ldo = c.ldw_hh = H; c.ldx = c.ldw_ih = K1;
                                // 0-8: one address off; 9-11: a row stride that is no multiple of 4 floats
                                const void* a[9] = {K1 ? OK : nullptr, K1 ? OK : nullptr, OK, OK, out, OK, OK, (tr & 1) ? OK : nullptr, (tr & 2) ? OK : nullptr};
                                bool aligned = true;
                                if (bad >= 0 && bad < 9 && a[bad]) a[bad] = (const char*)a[bad] + 4, aligned = false;
                                if (bad == 9) c.ldh = H + 1, aligned = false;
                                if (bad == 10) c.ldo = H + 2, aligned = false;
                                if (bad == 11) c.ldw_hh = H + 3, aligned = false;
                                c.x = (const float*)a[0]; c.w_ih = (const float*)a[1]; c.h_prev = (const float*)a[2]; c.w_hh = (const float*)a[3];
                                c.h_out = (float*)a[4]; c.b_hh = (const float*)a[5]; c.b_ih = (const float*)a[6]; c.gx_table = (const float*)a[7];
                                c.gx_rowbias = (const float*)a[8]; c.K1 = K1;
                                const FnGruCellPlan p = gru_cell_plan(&c);
                                ++plans;
#define CFAIL(what) { cell_fail(what, c, aligned, p); continue; }
                                if (p.status != FN_OK) CFAIL("status of valid arguments");
                                if (p.family < 0 || p.family > FN_CELL_X6) CFAIL("family");
                                ++cell_reached[p.family][p.forced_honoured != 0];
                                const int kmax = K1 > H ? K1 : H;
                                const int rows = p.family == FN_CELL_STAGED ? p.t0 : p.family == FN_CELL_DIRECT ? 32 * p.t0 : p.family == FN_CELL_X6 ? 128 : 64 * p.t0;
                                const int units = p.family == FN_CELL_STAGED || p.family == FN_CELL_DIRECT || p.family == FN_CELL_X6 ? 32 : 16;
                                if (rows < 1 || p.grid != ((B + rows - 1) / rows) * (H / units)) CFAIL("the grid does not cover B x H");
                                if (p.lds_bytes < 0 || p.lds_bytes > 160 * 1024 || (p.family == FN_CELL_DIRECT) != (p.lds_bytes == 0)) CFAIL("LDS");
                                if (p.threads != (p.family == FN_CELL_X6 ? 512 : 256) || p.kmax != kmax) CFAIL("threads / kmax");
                                if (p.has_tab != (tr & 1) || p.has_rb != ((tr >> 1) & 1)) CFAIL("HAS_TAB / HAS_RB");
                                if (p.family != FN_CELL_STAGED && (!aligned || (K1 % 16) != 0)) CFAIL("a kernel without staging on operands it cannot read");
                                if (p.family == FN_CELL_X6 && (!x6 || B % 128 || H < 64 || K1 % 32)) CFAIL("the bf16 x 6 cell on a shape it does not take");
                                if (p.family == FN_CELL_WLDS_OVL && (H != 512 || (K1 != 0 && K1 != 512))) CFAIL("the overlapped fill without K1 = H = 512");
                                if (p.family == FN_CELL_WLDS && 48L * kmax * 4 + 20480 > 160 * 1024) CFAIL("a weight slice beyond LDS");
                                // forms 1-18 by family, a second time
                                const int want = v == 0 || v > 18 ? -1 : (v <= 3 || v == 8) ? FN_CELL_STAGED : v <= 7 ? FN_CELL_DIRECT : v <= 14 ? FN_CELL_WLDS : FN_CELL_WLDS_OVL;
                                if (p.forced_honoured && (want < 0 || p.family != want)) CFAIL("forced_honoured without the named form");
                                if (!p.forced_honoured && want >= 0 && p.family != FN_CELL_X6 && !(p.family == FN_CELL_STAGED && p.t0 == 64 && p.t1 == 2 && p.t2 == 2))
                                    CFAIL("neither the named form nor the staged default");
                                if (!p.forced_honoured && want == FN_CELL_STAGED && p.family != FN_CELL_X6) CFAIL("a staged form is always eligible");
                                if (!p.forced_honoured && want > FN_CELL_STAGED && p.family != FN_CELL_X6 && aligned && K1 % 16 == 0 &&
                                    (want == FN_CELL_DIRECT || (want == FN_CELL_WLDS ? kmax <= 512 : (H == 512 && (K1 == 0 || K1 == 512)))))
                                    CFAIL("an eligible form was not honoured");
                                if (v == 0 && !x6 && p.family != FN_CELL_STAGED && B <= 512) CFAIL("the automatic choice below 513 rows is the staged kernel");
#undef CFAIL
                            }
}

}  // namespace

int main() {
    check_codes();
    sweep_scans();
    sweep_cells();
    for (int k = 0; k < FN_GRU_KERNELS; ++k)
        if (!reached[k]) {
            ++findings;
            std::printf("FINDING the sweep never reaches scan instance %d\n", k);
        }
    for (int f = 0; f <= FN_CELL_X6; ++f)
        if (!(cell_reached[f][0] + cell_reached[f][1])) {
            ++findings;
            std::printf("FINDING the sweep never reaches cell family %d\n", f);
        }
    std::printf("%d return codes, %ld plans, %ld findings\n", codes, plans, findings);
    return findings ? 1 : 0;
}
