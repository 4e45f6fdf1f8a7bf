// ring_core.h - the software-pipelined register ring of the K loops that read operands straight from memory (decode cells and output argmax of
// gru.hip; gemm_nt_direct_kernel of gemm.hip keeps a copy of its own, see there).
//
// A K loop of nks steps keeps PF steps of asm-issued loads (NL loads per step, mma_core.h: fn_gld4_s) in flight in PF register sets ("slots")
// and counts their completion itself: loads retire in issue order, so "at most n outstanding" (s_waitcnt vmcnt(n)) in front of a step's
// multiply is safe when no more than n loads were issued behind that step's own.  The callables get the slot as a plain int that is a
// constant after unrolling - the slots stay in registers:
//   load(slot)       requests the next step of the caller's K walk into the slot (the caller advances its own pointers)
//   mma(slot, step)  multiplies step `step` out of the slot
//   keep(slot)       fn_keep of every register of the slot (behind the wait that covers it, mma_core.h)
// Schedule: steps [0, nmain = nks / PF * PF) run through the ring - step s in slot s % PF; the steady state is "wait / multiply / refill
// own slot / sched_barrier" with PF - 1 steps outstanding, the last PF steps count down (for u = 0, 1, 2, then everything), then the
// < PF leftover steps run unpipelined in slot 0 (PARITY: in slot step & 1, for a caller whose second buffer follows the step parity; PF
// even then, so that the ring steps have slot parity = step parity too).
// Two entry forms:
//   REQUESTED = false  fn_ring_run issues the first PF requests itself (none when nks < PF: all steps are leftover steps)
//   REQUESTED = true   the caller has issued fn_ring_request (the first min(PF, nks) steps) ahead of other work - a weight fill - whose
//                      plain loads are younger than those requests and older than every later one, so the counted waits cover them;
//                      nks < PF multiplies the requested steps after one full wait; the form ends with a vmcnt(0) where its branches meet
//
// The header compiles for the host: host/ring_check.cpp defines the four macros below as recording stubs and replays the schedule under
// the in-order retirement model of check_isa_waits.py.
#pragma once

#ifndef FN_RING_WAIT
#define FN_RING_INL FN_DEVINL
#define FN_RING_WAIT(n) fn_wait_vm<(n)>()
#define FN_RING_FENCE() __builtin_amdgcn_sched_barrier(0)
#define FN_RING_UNROLL _Pragma("unroll")
#endif

template <int PF, class Load>
FN_RING_INL void fn_ring_request(int nks, Load&& load) {
    FN_RING_UNROLL
    for (int s = 0; s < PF; ++s)
        if (s < (nks < PF ? nks : PF)) load(s);
}

template <int PF, int NL, bool REQUESTED, bool PARITY = false, class Load, class Mma, class Keep>
FN_RING_INL void fn_ring_run(int nks, Load&& load, Mma&& mma, Keep&& keep) {
    static_assert(PF >= 1 && NL >= 1 && (!PARITY || (PF % 2) == 0), "slot parity = step parity needs an even ring");
    const int nmain = nks / PF * PF;
    int done = nmain;
    if (nmain > 0) {
        int s = 0;
        if (!REQUESTED) {
            FN_RING_UNROLL
            for (int u = 0; u < PF; ++u) load(u);
        }
        for (; s + PF < nmain; s += PF) {            // steady state: every step refills its own ring slot
            FN_RING_UNROLL
            for (int u = 0; u < PF; ++u) {
                FN_RING_WAIT(NL * (PF - 1));
                mma(u, s + u);
                load(u);
                FN_RING_FENCE();
            }
        }
        FN_RING_UNROLL
        for (int u = 0; u < PF; ++u) {               // the ring holds the last PF steps s .. s + PF - 1: everything has been requested
            if (u == 0) FN_RING_WAIT(NL * (PF - 1));
            else if (u == 1 && PF > 1) FN_RING_WAIT(PF > 1 ? NL * (PF - 2) : 0);
            else if (u == 2 && PF > 2) FN_RING_WAIT(PF > 2 ? NL * (PF - 3) : 0);
            else FN_RING_WAIT(0);
            mma(u, s + u);
            FN_RING_FENCE();
        }
    } else if (REQUESTED) {
        FN_RING_WAIT(0);                             // fewer steps than ring slots (K < 16 PF)
        FN_RING_UNROLL
        for (int u = 0; u < PF; ++u)
            if (u < (nks < PF ? nks : PF)) mma(u, u);
        done = nks;
    }
    if (REQUESTED || nmain > 0) {
        // (REQUESTED: nothing is outstanding here on either branch.  The wait says so where the branches meet: hipcc leaves a never-taken edge
        // from the ring's entry to this point in out_argmax_lds_kernel<8>, and check_isa_waits.py walks every edge)
        if (REQUESTED) FN_RING_WAIT(0);
        FN_RING_UNROLL
        for (int u = 0; u < PF; ++u) keep(u);
    }
    for (int s = done; s < nks; ++s) {               // < PF leftover steps, unpipelined
        if (PARITY && (s & 1)) {
            load(1);
            FN_RING_WAIT(0);
            mma(1, s);
        } else {
            load(0);
            FN_RING_WAIT(0);
            mma(0, s);
        }
        keep(0);
        if (PARITY) keep(1);
    }
}
