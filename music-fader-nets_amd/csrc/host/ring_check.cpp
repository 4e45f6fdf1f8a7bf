// ring_check.cpp - the schedule of ring_core.h on the CPU: the header's own text with recording stubs for the counted wait and the
// scheduling barrier, replayed under the in-order retirement model of check_isa_waits.py (loads complete in issue order; "vmcnt(n)"
// returns once at most n are outstanding).  Stand-alone: g++ -std=c++17 -fsanitize=address,undefined -Wall -Werror ring_check.cpp.
// For PF in {1, 2, 4, 8}, NL in {1, 4, 7}, nks = 0 .. 3 PF + 2, both entry forms (and the parity form where PF is even):
//   every step requested exactly once; multiplied exactly once, in increasing order, from the slot it was requested into; the wait in
//   front of a step's multiply allows no more outstanding loads than were issued behind the step's own; no slot refilled before its step
//   was multiplied; slot parity = step parity (parity form: throughout; plain form: in the ring steps - its leftover steps use slot 0);
//   nothing outstanding at the end; every slot kept behind its last wait.
#include <cstdio>
#include <vector>

struct Rec {
    int PF = 0, NL = 0, nks = 0;
    bool parity = false;
    long issued = 0, retired = 0;          // loads issued / completed so far (in order)
    int last_wait = -1;                    // n of the latest wait, -1: a load was issued since
    int next_step = 0, next_mma = 0, fences = 0;
    std::vector<int> slot_step;            // step held by a slot (-1: none)
    std::vector<char> slot_done, slot_kept;
    std::vector<long> step_last;           // issue index behind the step's last load
    std::vector<int> requested, multiplied;
    int findings = 0;
    void fail(const char* what, int a = 0, int b = 0) {
        ++findings;
        std::printf("FINDING PF=%d NL=%d nks=%d parity=%d: %s (%d, %d)\n", PF, NL, nks, (int)parity, what, a, b);
    }
    void reset(int pf, int nl, int n, bool par) {
        *this = Rec();
        PF = pf; NL = nl; nks = n; parity = par;
        slot_step.assign(pf, -1);
        slot_done.assign(pf, 1);
        slot_kept.assign(pf, 1);
        step_last.assign(n + 1, 0);
        requested.assign(n + 1, 0);
        multiplied.assign(n + 1, 0);
    }
    void plain_loads(int n) { issued += n; last_wait = -1; }      // a caller's fill between the request and the run
    void load(int slot) {
        if (slot < 0 || slot >= PF) return fail("slot out of range", slot);
        if (next_step >= nks) return fail("request past the last step", next_step);
        if (!slot_done[slot]) fail("slot refilled before its step was multiplied", slot, slot_step[slot]);
        const int step = next_step++;
        ++requested[step];
        slot_step[slot] = step;
        slot_done[slot] = 0;
        slot_kept[slot] = 0;
        issued += NL;
        step_last[step] = issued;
        last_wait = -1;
        const bool ring_step = step < nks / PF * PF;
        if ((PF % 2) == 0 && (parity || ring_step) && ((slot ^ step) & 1)) fail("slot parity != step parity", slot, step);
    }
    void wait(int n) {
        if (n < 0) return fail("negative wait", n);
        if (issued - retired > n) retired = issued - n;
        last_wait = n;
    }
    void fence() { ++fences; }
    void mma(int slot, int step) {
        if (slot < 0 || slot >= PF) return fail("slot out of range", slot);
        if (step != next_mma) fail("steps multiplied out of order", step, next_mma);
        next_mma = step + 1;
        if (step < 0 || step >= nks) return fail("multiply of a step that does not exist", step);
        ++multiplied[step];
        if (slot_step[slot] != step) return fail("multiplied from another slot than requested into", slot, step);
        if (last_wait < 0 && issued > retired) fail("no wait between the last request and the multiply", step);
        if (last_wait > issued - step_last[step]) fail("the wait allows more than was issued behind the step", last_wait, (int)(issued - step_last[step]));
        if (retired < step_last[step]) fail("multiply of a step whose loads may be in flight", step);
        slot_done[slot] = 1;
    }
    void keep(int slot) {
        if (slot < 0 || slot >= PF) return fail("slot out of range", slot);
        if (!slot_done[slot] || retired < issued) fail("slot kept in front of the wait that covers it", slot);
        slot_kept[slot] = 1;
    }
    void finish() {
        for (int s = 0; s < nks; ++s) {
            if (requested[s] != 1) fail("step not requested exactly once", s, requested[s]);
            if (multiplied[s] != 1) fail("step not multiplied exactly once", s, multiplied[s]);
        }
        if (issued != retired) fail("loads outstanding at the end", (int)(issued - retired));
        for (int u = 0; u < PF; ++u)
            if (!slot_kept[u]) fail("slot not kept behind its last wait", u);
    }
};
static Rec g_rec;

#define FN_RING_INL static inline
#define FN_RING_WAIT(n) g_rec.wait(n)
#define FN_RING_FENCE() g_rec.fence()
#define FN_RING_UNROLL
#include "../ring_core.h"

static int g_cases = 0;

template <int PF, int NL, bool REQUESTED, bool PARITY>
static void run_one(int nks) {
    g_rec.reset(PF, NL, nks, PARITY);
    auto load = [&](int slot) { g_rec.load(slot); };
    auto mma = [&](int slot, int step) { g_rec.mma(slot, step); };
    auto keep = [&](int slot) { g_rec.keep(slot); };
    if (REQUESTED) {
        fn_ring_request<PF>(nks, load);
        g_rec.plain_loads(5);
    }
    fn_ring_run<PF, NL, REQUESTED, PARITY>(nks, load, mma, keep);
    g_rec.finish();
    ++g_cases;
}

template <int PF, int NL>
static int run_pf_nl() {
    int findings = 0;
    for (int nks = 0; nks <= 3 * PF + 2; ++nks) {
        run_one<PF, NL, false, false>(nks);
        findings += g_rec.findings;
        run_one<PF, NL, true, false>(nks);
        findings += g_rec.findings;
        if constexpr ((PF % 2) == 0) {
            run_one<PF, NL, false, true>(nks);
            findings += g_rec.findings;
            run_one<PF, NL, true, true>(nks);
            findings += g_rec.findings;
        }
    }
    return findings;
}

template <int PF>
static int run_pf() { return run_pf_nl<PF, 1>() + run_pf_nl<PF, 4>() + run_pf_nl<PF, 7>(); }

int main() {
    const int findings = run_pf<1>() + run_pf<2>() + run_pf<4>() + run_pf<8>();
    std::printf("ring_check: %d schedules, %d findings\n", g_cases, findings);
    return findings ? 1 : 0;
}
