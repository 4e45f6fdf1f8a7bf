// decode_plan_check.cpp - the decode launch plans (csrc/decode_plan.h, the header fn_decode_greedy / fn_decode_forced / fn_out_argmax_f32 launch from) on
// the CPU.  Stand-alone: g++ -std=c++17 -fsanitize=address,undefined -Wall -Werror decode_plan_check.cpp.
//
// 1. The return codes, written down before the code moved: which FN_E_* a call with one or several faults returns (the order of the checks).
// 2. The one-launch decode: B 1 .. 2049 x H x V x compute units x forced or not.  Of every FN_OK plan:
//      grid == nrep x per_rep <= cus;  1 <= nrep <= nblk <= MAXBLK;  (nblk - 1) block_rows < B <= nblk block_rows;  block_rows 16 / 32 / 64 by the three
//      row ranges;  LDS <= 160 KB - 64;  the four workspace regions disjoint, in order, each as large as the kernel indexes it, ending at or before
//      fn_decode_ws_bytes(B, H, V);  every counter word of every block below the error word, the error word inside fn_decode_sync_ws_bytes().
//    A plan that is not FN_OK: FN_E_UNSUPPORTED exactly when the role set is larger than the compute units, FN_E_SHAPE exactly for what is refused.
//    fn_decode_ws_bytes against the formula it had before the layout function existed.
// 3. A literal table worked out by hand from the formulas (H = 512, V = 342, 256 compute units: 3 x 32 + 22 + 1 = 119 workgroups per role set; H = 64:
//    3 x 4 + 22 + 1 = 35).
// 4. The fused output layer: return codes, and over B x V x K the kernel by K, its grid covering B x V in the kernel's tile, threads and LDS.
#include <cstdio>
#include <initializer_list>

#include "../decode_plan.h"

namespace {

long findings = 0, plans = 0;
int codes = 0;

alignas(16) char mem[64];
void* const OK = mem;            // a 16-byte aligned address
void* const OFF = mem + 4;       // ... one 4 bytes behind it
void* const OFF8 = mem + 8;      // ... and one 8 bytes behind it

void expect(long got, long want, const char* what) {
    ++codes;
    if (got != want) {
        ++findings;
        std::printf("FINDING `%s`: %ld, expected %ld\n", what, got, want);
    }
}

FnDecode make(int B, int H, int V, int steps = 8) {
    FnDecode d{};
    d.B = B; d.steps = steps; d.H = H; d.V = V; d.start_token = V - 1;
    d.w_hh1_frag = d.b_hh1 = d.b_ih1 = d.table1 = d.rowbias1 = d.h0 = d.w_ih2_frag = d.b_ih2 = d.w_hh2_frag = d.b_hh2 = d.w_out_frag = d.b_out = (const float*)OK;
    d.tokens = (int32_t*)OK; d.tok_ld = steps; d.ws = (float*)OK; d.sync_ws = OK;
    return d;
}
FnDecodeForce make_force(int ld = 8) {
    FnDecodeForce f{};
    f.forced = (const int32_t*)OK; f.forced_ld = ld; f.force = (const uint8_t*)OK;
    return f;
}

// ---- 1. the return codes --------------------------------------------------------------------------------------------------------------------------
void check_codes() {
    FnDecode d;
    FnDecodeForce f;
    auto run = [&](auto&& edit, bool forced = false, int cus = 256) {
        d = make(40, 512, 342);
        f = make_force();
        edit();
        return (long)decode_plan(&d, forced ? &f : nullptr, cus).status;
    };
    expect(decode_plan(nullptr, nullptr, 256).status, FN_E_NULL, "decode: no descriptor");
    expect(run([] {}), FN_OK, "decode: valid");
    expect(run([] {}, true), FN_OK, "decode: valid, forced");
    for (int m = 0; m < 12; ++m)
        expect(run([&] {
                   const float** req[12] = {&d.w_hh1_frag, &d.b_hh1, &d.table1, &d.h0, &d.w_ih2_frag, &d.w_hh2_frag, &d.b_hh2, &d.w_out_frag, &d.b_out, nullptr, nullptr, nullptr};
                   if (m < 9) *req[m] = nullptr;
                   else if (m == 9) d.tokens = nullptr;
                   else if (m == 10) d.ws = nullptr;
                   else d.sync_ws = nullptr;
                   d.B = 0;
               }),
               FN_E_NULL, "decode: a required member NULL before B = 0");
    expect(run([&] { d.b_ih1 = d.rowbias1 = d.b_ih2 = nullptr; d.logp = nullptr; }), FN_OK, "decode: the optional members NULL");
    expect(run([&] { d.B = 0; }), FN_E_SHAPE, "decode: B = 0");
    expect(run([&] { d.B = 2049; }), FN_E_SHAPE, "decode: B = 2049");
    expect(run([&] { d.B = 2048; }), FN_OK, "decode: B = 2048");
    expect(run([&] { d.steps = 0; d.tok_ld = 0; }), FN_E_SHAPE, "decode: steps = 0");
    expect(run([&] { d.H = 48; d.ws = (float*)OFF; }), FN_E_SHAPE, "decode: H % 32 before a misaligned ws");
    expect(run([&] { d.H = 544; }), FN_E_SHAPE, "decode: H = 544");
    expect(run([&] { d.H = 0; }), FN_E_SHAPE, "decode: H = 0");
    expect(run([&] { d.V = 0; }), FN_E_SHAPE, "decode: V = 0");
    expect(run([&] { d.V = 385; }), FN_E_SHAPE, "decode: V = 385");
    expect(run([&] { d.V = 385; }, false, 16), FN_E_SHAPE, "decode: V = 385 before too few compute units");
    expect(run([&] { d.tok_ld = 7; }), FN_E_SHAPE, "decode: tok_ld < steps");
    expect(run([&] { d.start_token = -5; }), FN_OK, "decode: start_token is the caller's");
    expect(run([&] { d.ws = (float*)OFF; }), FN_E_ALIGN, "decode: misaligned ws");
    expect(run([&] { d.rowbias1 = (const float*)OFF8; }), FN_E_ALIGN, "decode: misaligned rowbias1");
    expect(run([&] { d.b_out = (const float*)OFF; d.tokens = (int32_t*)OFF; d.logp = (float*)OFF; d.sync_ws = OFF; }), FN_OK,
           "decode: b_out, tokens, logp, sync_ws need 4 bytes only");
    expect(run([&] { d.ws = (float*)OFF; }, false, 16), FN_E_ALIGN, "decode: misaligned ws before too few compute units");
    expect(run([] {}, false, 118), FN_E_UNSUPPORTED, "decode: 118 compute units for 119 role workgroups");
    expect(run([] {}, false, 119), FN_OK, "decode: 119 compute units");
    expect(run([] {}, false, 0), FN_E_UNSUPPORTED, "decode: no device (0 compute units)");
    // the forced members are answered first, as fn_decode_forced did in front of the common checks
    expect(run([&] { f.forced = nullptr; d.B = 0; }, true), FN_E_NULL, "forced: forced NULL before B = 0");
    expect(run([&] { f.force = nullptr; d.H = 48; }, true), FN_E_NULL, "forced: force NULL before H % 32");
    expect(run([&] { f.forced_ld = 7; d.h0 = nullptr; }, true), FN_E_SHAPE, "forced: forced_ld < steps before h0 NULL");
    expect(run([&] { f.forced = nullptr; f.forced_ld = 7; }, true), FN_E_NULL, "forced: forced NULL before forced_ld");
    expect(run([&] { d.h0 = nullptr; d.ws = (float*)OFF; }, true), FN_E_NULL, "forced: h0 NULL before a misaligned ws");
    expect(run([&] { f.forced = (const int32_t*)OFF; f.force = (const uint8_t*)OFF + 1; }, true), FN_OK, "forced: its members need no 16 bytes");
    expect(run([] {}, true, 118), FN_E_UNSUPPORTED, "forced: 118 compute units");

    auto arg = [](const void* h, int ldh, const void* W, int ldw, const void* bias, int B, int V, int K, const void* best) {
        return (long)out_argmax_plan(h, ldh, W, ldw, bias, B, V, K, best).status;
    };
    expect(arg(OK, 512, OK, 512, OK, 2048, 342, 512, OK), FN_OK, "out_argmax: valid");
    expect(arg(nullptr, 512, OK, 512, OK, 0, 342, 512, OK), FN_E_NULL, "out_argmax: h NULL before B = 0");
    expect(arg(OK, 512, nullptr, 512, OK, 8, 342, 512, OK), FN_E_NULL, "out_argmax: W NULL");
    expect(arg(OK, 512, OK, 512, nullptr, 8, 342, 512, OK), FN_E_NULL, "out_argmax: bias NULL");
    expect(arg(OK, 512, OK, 512, OK, 8, 342, 512, nullptr), FN_E_NULL, "out_argmax: best NULL");
    expect(arg(OK, 512, OK, 512, OK, 8, 0, 512, OK), FN_E_SHAPE, "out_argmax: V = 0");
    expect(arg(OFF, 512, OK, 512, OK, 8, 342, 40, OK), FN_E_SHAPE, "out_argmax: K % 16 before a misaligned h");
    expect(arg(OK, 500, OK, 512, OK, 8, 342, 512, OK), FN_E_SHAPE, "out_argmax: ldh < K");
    expect(arg(OK, 512, OK, 514, OK, 8, 342, 512, OK), FN_E_SHAPE, "out_argmax: ldw % 4");
    expect(arg(OFF, 1 << 20, OK, 512, OK, 1024, 342, 512, OK), FN_E_SHAPE, "out_argmax: a 4 GB span of h before its alignment");
    expect(arg(OK, 1 << 20, OK, 512, OK, 1023, 342, 512, OK), FN_OK, "out_argmax: a span of h just below 4 GB");
    expect(arg(OK, 512, OK, 1 << 22, OK, 8, 256, 512, OK), FN_E_SHAPE, "out_argmax: a 4 GB span of W");
    expect(arg(OFF, 512, OK, 512, OK, 8, 342, 512, OK), FN_E_ALIGN, "out_argmax: misaligned h");
    expect(arg(OK, 512, OFF8, 512, OK, 8, 342, 512, OK), FN_E_ALIGN, "out_argmax: misaligned W");
    expect(arg(OK, 512, OK, 512, OK, 8, 342, 512, OFF), FN_E_ALIGN, "out_argmax: best off its 8 bytes");
    expect(arg(OK, 512, OK, 512, OFF, 8, 342, 512, OFF8), FN_OK, "out_argmax: bias needs 4 bytes, best 8");
}

// ---- 2. the one-launch decode ---------------------------------------------------------------------------------------------------------------------
void fail(const char* what, int B, int H, int V, int cus, int forced, const FnDecodePlan& p) {
    if (++findings > 20) return;
    std::printf("FINDING %s: B %d H %d V %d cus %d forced %d -> status %d mt %d rows %d nblk %d nvt %d nslices %d per_rep %d nrep %d grid %d lds %d ws %ld %ld %ld %ld %ld\n",
                what, B, H, V, cus, forced, p.status, p.mt, p.block_rows, p.nblk, p.nvt, p.nslices, p.per_rep, p.nrep, p.grid, p.lds_bytes, (long)p.x1_off,
                (long)p.x2_off, (long)p.g2_off, (long)p.logits_off, (long)p.ws_floats);
}

long reached_mt[5];

void sweep_decode() {
    const FnDecodeForce f = make_force();
    for (int B = 1; B <= 2049; ++B)
        for (const int H : {32, 64, 256, 512, 544})
            for (const int V : {1, 16, 17, 342, 384, 385})
                for (const int cus : {0, 34, 35, 118, 119, 238, 256, 304})
                    for (int forced = 0; forced < 2; ++forced) {
                        const FnDecode d = make(B, H, V);
                        const FnDecodePlan p = decode_plan(&d, forced ? &f : nullptr, cus);
                        ++plans;
#define FAIL(what) { fail(what, B, H, V, cus, forced, p); continue; }
                        // the role set, a second time
                        const int per_rep = 3 * (H / 16) + (V + 15) / 16 + 1;
                        const bool refused = B > 2048 || H > 512 || V > 384;
                        if (refused != (p.status == FN_E_SHAPE)) FAIL("FN_E_SHAPE exactly for what is refused");
                        if (refused) continue;
                        if ((per_rep > cus) != (p.status == FN_E_UNSUPPORTED)) FAIL("FN_E_UNSUPPORTED exactly when the role set is larger than the compute units");
                        if (per_rep > cus) continue;
                        if (p.status != FN_OK) FAIL("status of valid arguments");
                        if (p.forced != forced || p.threads != 256) FAIL("forced / threads");
                        if (p.nslices != H / 16 || p.nvt != (V + 15) / 16 || p.per_rep != per_rep) FAIL("the role set");
                        if (p.grid != p.nrep * p.per_rep || p.grid > cus) FAIL("grid == nrep x per_rep <= cus");
                        if (p.nrep < 1 || p.nrep > p.nblk || p.nblk > MAXBLK) FAIL("1 <= nrep <= nblk <= MAXBLK");
                        if (p.nrep != (cus / per_rep < p.nblk ? cus / per_rep : p.nblk)) FAIL("as many replicas as fit, at most one per block");
                        if ((long)(p.nblk - 1) * p.block_rows >= B || B > (long)p.nblk * p.block_rows) FAIL("(nblk - 1) block_rows < B <= nblk block_rows");
                        if (p.block_rows != (B <= 16 ? 16 : B >= 353 ? 64 : 32) || p.block_rows != 16 * p.mt) FAIL("block_rows by the three row ranges");
                        ++reached_mt[p.mt];
                        if (p.lds_bytes <= 0 || p.lds_bytes > 160 * 1024 - 64) FAIL("LDS");
                        if (p.lds_bytes != (3 * H * 16 + 4 * p.mt * 3 * 272) * 4 + 16 + 256) FAIL("LDS: slice + partial tiles + give-up word + tokens");
                        // the regions as the kernel indexes them: two slots of nblk slabs of block_rows x H floats (x1, x2), [rows][3H] (g2), [rows][16 nvt] (logits)
                        const long rows = (long)p.nblk * p.block_rows, vp = 16L * p.nvt;
                        if (p.x1_off != 0 || p.x2_off - p.x1_off < 2 * rows * H || p.g2_off - p.x2_off < 2 * rows * H || p.logits_off - p.g2_off < rows * 3 * H ||
                            p.ws_floats - p.logits_off < rows * vp)
                            FAIL("workspace regions overlap or are out of order");
                        if ((p.x2_off | p.g2_off | p.logits_off) & 3) FAIL("a workspace region off its 16 bytes");
                        if ((size_t)p.ws_floats * 4 > decode_ws_bytes(B, H, V)) FAIL("the workspace ends behind fn_decode_ws_bytes");
                        bool counters_ok = true;
                        for (int blk = 0; blk < p.nblk; ++blk)
                            for (const int c : {C1, C2, C3, C4, C5}) counters_ok = counters_ok && c >= 0 && c + 32 <= BLKW && blk * BLKW + c + 32 <= ERRW;
                        if (!counters_ok) FAIL("a counter line leaves its block or reaches the error word");
#undef FAIL
                    }
    if ((size_t)(ERRW + 1) * 4 > decode_sync_ws_bytes()) ++findings, std::printf("FINDING the error word lies behind fn_decode_sync_ws_bytes\n");
    for (const int mt : {1, 2, 4})
        if (!reached_mt[mt]) ++findings, std::printf("FINDING the sweep never reaches %d row tiles\n", mt);
    // fn_decode_ws_bytes: the formula it had before the layout function
    for (int B = 1; B <= 2049; ++B)
        for (const int H : {32, 64, 256, 512, 544})
            for (const int V : {1, 16, 17, 342, 384, 385}) {
                const size_t bp = B <= 16 ? 16 : (size_t)(B + 63) / 64 * 64, vp = (size_t)(V + 15) / 16 * 16;
                ++plans;
                if (decode_ws_bytes(B, H, V) != (4 * bp * H + bp * 3 * H + bp * vp) * sizeof(float) && ++findings <= 20)
                    std::printf("FINDING fn_decode_ws_bytes(%d, %d, %d) = %zu\n", B, H, V, decode_ws_bytes(B, H, V));
            }
}

// ---- 3. the literal table -------------------------------------------------------------------------------------------------------------------------
void check_table() {
    struct Row {
        int H, B, mt, nblk, nrep, grid;
    };
    const Row rows[] = {
        {512, 16, 1, 1, 1, 119}, {512, 17, 2, 1, 1, 119}, {512, 33, 2, 2, 2, 238}, {512, 352, 2, 11, 2, 238}, {512, 353, 4, 6, 2, 238},
        {512, 2048, 4, 32, 2, 238},
        // H = 64: 35 workgroups per role set, min(256 / 35 = 7, nblk) replicas
        {64, 16, 1, 1, 1, 35}, {64, 33, 2, 2, 2, 70}, {64, 200, 2, 7, 7, 245}, {64, 352, 2, 11, 7, 245}, {64, 353, 4, 6, 6, 210}, {64, 2048, 4, 32, 7, 245},
    };
    for (const Row& r : rows) {
        const FnDecode d = make(r.B, r.H, 342);
        const FnDecodePlan p = decode_plan(&d, nullptr, 256);
        expect(p.status, FN_OK, "table: status");
        expect(p.per_rep, r.H == 512 ? 119 : 35, "table: per_rep");
        expect(p.mt, r.mt, "table: mt");
        expect(p.nblk, r.nblk, "table: nblk");
        expect(p.nrep, r.nrep, "table: nrep");
        expect(p.grid, r.grid, "table: grid");
    }
    const FnDecode d = make(2048, 512, 342);
    const FnDecodePlan p = decode_plan(&d, nullptr, 256);
    expect(p.lds_bytes, (3 * 512 * 16 + 4 * 4 * 3 * 272) * 4 + 272, "table: LDS of 64-row blocks at H = 512");      // 150800
    expect(p.lds_bytes, 150800, "table: LDS of 64-row blocks at H = 512, in bytes");
    expect(p.x2_off, 2L * 2048 * 512, "table: x2");
    expect(p.g2_off, 4L * 2048 * 512, "table: g2");
    expect(p.logits_off, 7L * 2048 * 512, "table: logits");
    expect(p.ws_floats, 7L * 2048 * 512 + 2048L * 352, "table: end of the workspace");
    expect((long)decode_ws_bytes(2048, 512, 342), (7L * 2048 * 512 + 2048L * 352) * 4, "table: fn_decode_ws_bytes(2048, 512, 342)");
    expect((long)decode_sync_ws_bytes(), (32 * 160 + 32) * 4, "table: fn_decode_sync_ws_bytes");
}

// ---- 4. the fused output layer --------------------------------------------------------------------------------------------------------------------
long reached_kernel[3];

void sweep_out_argmax() {
    for (const int B : {1, 31, 32, 33, 63, 64, 65, 77, 2048, 2049})
        for (const int V : {1, 47, 48, 49, 95, 96, 97, 342, 384})
            for (int K = 16; K <= 1024; K += 16)
                for (const int pad : {0, 4}) {
                    const FnOutArgmaxPlan p = out_argmax_plan(OK, K + pad, OK, K + pad, OK, B, V, K, OK);
                    ++plans;
#define FAIL(what) { if (++findings <= 20) std::printf("FINDING out_argmax %s: B %d V %d K %d -> status %d kernel %d grid %d threads %d lds %d\n", what, B, V, K, p.status, p.kernel, p.grid, p.threads, p.lds_bytes); continue; }
                    if (p.status != FN_OK) FAIL("status of valid arguments");
                    const int want = 48L * K * 4 > 128 * 1024 ? FN_OUT_ARGMAX_DIRECT : (K % 32 == 0 ? FN_OUT_ARGMAX_LDS8 : FN_OUT_ARGMAX_LDS);
                    if (p.kernel != want) FAIL("kernel by K");
                    ++reached_kernel[p.kernel];
                    const int rows = want == FN_OUT_ARGMAX_DIRECT ? 32 : 64, cols = want == FN_OUT_ARGMAX_DIRECT ? 96 : 48;
                    if (p.grid != ((B + rows - 1) / rows) * ((V + cols - 1) / cols)) FAIL("the grid does not cover B x V");
                    if (p.threads != (want == FN_OUT_ARGMAX_LDS8 ? 512 : 256)) FAIL("threads");
                    const int lds = want == FN_OUT_ARGMAX_DIRECT ? 0 : 48 * K * 4 + (want == FN_OUT_ARGMAX_LDS8 ? 12288 : 0);
                    if (p.lds_bytes != lds || lds > 144 * 1024) FAIL("LDS");
#undef FAIL
                }
    for (int k = 0; k < 3; ++k)
        if (!reached_kernel[k]) ++findings, std::printf("FINDING the sweep never reaches output-layer kernel %d\n", k);
}

}  // namespace

int main() {
    check_codes();
    check_table();
    sweep_decode();
    sweep_out_argmax();
    std::printf("%d return codes and table entries, %ld plans, %ld findings\n", codes, plans, findings);
    return findings ? 1 : 0;
}
