#!/usr/bin/env python3
"""Generates kloop4_asm.h: the K loops of the PING-PONG, register-stationary BACKWARD scan on the bf16 MFMA with exact bf16 triple splits
("bf16 x 6", gru_persist.hip: gru_bwd_x6_kernel) at H = 512.

Round 5.  Decomposition of gru_bwd_rs_kernel (gen_kloop2.py, GenRS): a workgroup owns 32 dh columns (16 slices) of a 32 TH-row group, two halves of
TH row tiles; every wave multiplies the current half over ITS K quarter (12 blocks of 32 gate-gradient columns) against both column tiles; the four
partial sums meet in LDS.  What the triple arithmetic changes:

  * the exchanged operand - the gate gradients [dr' | dz' | dn' r] of a row, 3H columns - travels as bf16 TRIPLES (6 instead of 4 bytes per value:
    [row tile][48 K blocks][piece][64 lanes][8 bf16]); pipeline unit = one K block of ONE row tile: 3 operand loads (1 KB each), 12
    v_mfma_f32_16x16x32_bf16 (6 partial products x 2 column tiles, smallest first, the column tiles take turns).  One 1 KB load feeds 4 MFMAs of
    16 cycles: the CU's address path (64 B per clock, four waves) is as busy as the MFMA pipes - this loop is bound by the operand stream;
  * W_hh^T slice as triples: column tile 0 of the wave's K quarter in AGPRs (12 blocks x 3 pieces x 4 = 144 registers, loaded once), column tile 1
    in LDS (blocks 0..10 of every quarter: 132 KB) with block 11 in AGPRs too (an LDS image of all 12 would leave no room for the accumulator tiles);
  * register budget (256 AGPRs): W 144 + 12, ring 6 x 12, the epilogue operands of the NEXT phase 24.  Accumulators and the LDS weight fragments
    live in VGPRs that only exist inside a statement (v208..v255: clobbered, nothing crosses a statement in them);
  * the epilogue operands (saved gates, previous state, external gradient: 6 HBM reads per item) are requested ONE PHASE AHEAD into AGPRs
    behind the last refill of the loop and are NOT waited for at its end (vmcnt retires in order: they stand in front of nothing but the next
    phase's ring, which is needed a whole epilogue later); the NEXT K loop statement hands them to the compiler: behind its arrival barrier the
    wave's own accumulator tiles in LDS are free until the end of the loop, so the 128-bit values bounce through them (ds_write_b128 from the
    AGPRs, ds_read_b128 into the output operands - inline asm cannot name a component of a 128-bit operand, v_accvgpr_read would need 24
    scalar outputs and the statement is limited to 30 operands);
  * the exchange-slab stores of an epilogue (9 x 8 bytes per item, write-through: ~30 cycles of the CU's address path each - 1.2 k cycles per phase
    when the four waves issue them back to back, measured) ride in the NEXT K loop, three per unit in front of the arrival; the four 16-byte
    stores nobody waits for (dgx, dghn) are a small statement of their own right behind the epilogue (`*_out`: counted, so that they enter the
    vmcnt arithmetic) - with both store sets the K loop statement would need 33 operands (inline asm takes 30);
  * counter of the other half: loaded near the end of the loop, looked at behind it; the ring request is a statement of its own (as kloop3_asm.h).

State that crosses statements: W (a0..a155), the ring (RU - 1 units in flight), the next phase's epilogue operands (in flight), the slab stores,
and the vmcnt arithmetic: between two statements the compiler issues NO vector-memory instruction (scratch/check_pp_isa.py).

AGPR map: W0[blk][piece] a[12 blk + 4 piece ..] (blk 0..11), W1[11][piece] a[144 + 4 piece ..], ring[slot][piece] a[156 + 12 slot + 4 piece ..],
ext[j] a[228 + 4 j ..] (j = 0..3 saved gates r, z, n, hn; 4 previous state; 5 external gradient).
VGPR temporaries: acc[m][ct] v[208 + 4 (2 m + ct) ..], wfrag[bs][piece] v[224 + 12 bs + 4 piece ..], v255 = offset of the second row tile.  Scalars s84..s87.
"""
import sys

from kloop_common import PROD, SB, SLAB, UB, Slots, VmQueue, advance, clobber, lanes32, rng, statement

TILE = 48 * UB       # bytes of one row tile on the exchange slab
W0, W1X, RING0, EXT0 = 0, 144, 156, 228
VACC, VWF, VO2 = 208, 224, 255
NBLK = 12
NEXT = 6             # epilogue-operand loads per phase
NSLAB = 9            # exchange-slab stores per item (3 gates x 3 pieces)
NOUT = 4             # dgx r / z / n and dghn stores per item


class GenX6B:
    def __init__(self, name, TH, RU, stores, u_arr, poll_unit):
        self.name, self.TH, self.RU, self.stores = name, TH, RU, stores
        self.masked = TH == 1
        self.units = NBLK * TH
        self.u_arr, self.poll_unit = u_arr, poll_unit
        assert RING0 + 12 * RU <= EXT0 and poll_unit + 1 < self.units and poll_unit > self.units - RU
        self.nacc = 2 * TH

    def ring(self, u, pc):
        return RING0 + 12 * (u % self.RU) + 4 * pc

    def blk_m(self, u):
        return u // self.TH, u % self.TH

    def vo(self, m):
        return "%[vo]" if m == 0 else "v%d" % VO2

    def wfrag(self, blk, pc):
        """B operand of column tile 1 for K block blk: LDS-fed VGPR double buffer, or the resident block 11"""
        if blk == NBLK - 1:
            return rng(W1X + 4 * pc)
        return rng(VWF + 12 * (blk & 1) + 4 * pc, f="v")

    def wread(self, blk):
        assert blk < NBLK - 1
        return ["ds_read_b128 %s, %%[lp] offset:%d" % (self.wfrag(blk, pc), blk * UB + pc * 1024) for pc in range(3)]

    def mfmas(self, u):
        blk, m = self.blk_m(u)
        out = []
        for pa, pb in PROD:
            a = self.ring(u, pa)
            for ct in range(2):
                c = rng(VACC + 4 * (2 * m + ct), f="v")
                b = rng(W0 + 12 * blk + 4 * pb) if ct == 0 else self.wfrag(blk, pb)
                out.append("v_mfma_f32_16x16x32_bf16 %s, %s, %s, %s" % (c, rng(a), b, c))
        return out

    def load_unit(self, u):
        """the three operand loads of unit u off the running base (which must point at unit u's K block)"""
        blk, m = self.blk_m(u)
        return ["global_load_dwordx4 %s, %s, s[%d:%d] offset:%d sc1" % (rng(self.ring(u, pc)), self.vo(m), SB, SB + 1, pc * 1024) for pc in range(3)]

    def arrive_block(self):
        """every wave's exchange-slab stores (issued by this statement's first units) have completed -> barrier (also the fence between the previous epilogue's reads of the accumulator tiles and this phase's writes) -> one
        arrival (arr: 0 = none due, 1 = due, 2 = due and this wave issues it).  `_first`: the stores it would wait for were drained by the caller."""
        L = [self.q.wait_slab_store()] if self.stores else []
        return L + ["s_barrier", "s_cmp_lt_u32 %[arr], 2", "s_cbranch_scc1 .Lnoarr_%=",
                    "s_mov_b64 s[%d:%d], exec" % (SB + 2, SB + 3), "s_mov_b64 exec, 1", "v_mov_b32 %[pv], 1",
                    "global_atomic_add %[pcnt], %[pv], off", "s_mov_b64 exec, s[%d:%d]" % (SB + 2, SB + 3), ".Lnoarr_%=:"]

    def body(self):
        RU, units, TH = self.RU, self.units, self.TH
        # in flight when the statement starts, oldest first: this phase's epilogue operands (requested by the previous statement, or `_ext`), the ring
        # request (`_pro`), the previous epilogue's dgx / dghn stores (`_out`)
        self.q = VmQueue([("ext", 0)] * NEXT + [("ring", u) for u in range(RU - 1) for _ in range(3)] + ([("store", "out")] * NOUT if self.stores else []))
        L = []
        if TH == 2:
            L.append("v_add_u32 v%d, 0x%x, %%[vo]" % (VO2, TILE))
        base_blk = (RU - 1) // TH
        L += ["s_mov_b64 s[%d:%d], %%[xin]" % (SB, SB + 1)] + advance(base_blk * UB)
        L += self.wread(0)
        for c in range(4 * self.nacc):
            L.append("v_mov_b32 v%d, 0" % (VACC + c))
        slabs = []
        if self.stores:      # previous epilogue's gate gradients as triples: gate g at byte offset 0xC000 g (16 K blocks), piece p 1 KB further
            for g in range(3):
                for pc in range(3):
                    pre = ["v_add_u32 v%d, 0x%x, %%[so0]" % (VO2 - 1, 0xC000 * g)] if (g and pc == 0) else []
                    slabs.append(pre + ["global_store_dwordx2 %s, %%[t%d%d], %%[sbase] offset:%d sc1" % ("%[so0]" if g == 0 else "v%d" % (VO2 - 1), g, pc, pc * 1024)])
        ext_out = ["gt0", "gt1", "gt2", "gt3", "hp", "xt"]
        done_arr = False
        for u in range(units):
            blk, m = self.blk_m(u)
            slots = Slots(12)
            v = u + RU - 1
            if v < units:
                nb = v // TH
                if nb != base_blk:
                    L += advance((nb - base_blk) * UB)
                    base_blk = nb
                for pc, ins in enumerate(self.load_unit(v)):
                    slots.put(pc, ins, ("ring", v))
            if m == TH - 1 and blk + 1 < NBLK - 1:       # last unit of a K block: the LDS half of the next block's weights
                for i, ins in enumerate(self.wread(blk + 1)):
                    slots.put(4 + i, ins)
            # hand-over of this phase's epilogue operands (they landed long ago: older than unit 0's ring loads): AGPRs -> own accumulator tiles in LDS ->
            # output operands, nacc vectors per unit, in the units behind the arrival barrier (a wave's LDS operations execute in order, every lane
            # reads back its own 16 bytes: no wait in between)
            rounds = [list(range(i, min(i + self.nacc, NEXT))) for i in range(0, NEXT, self.nacc)]
            if self.u_arr < u <= self.u_arr + len(rounds):
                js = rounds[u - self.u_arr - 1]
                for i, j in enumerate(js):
                    slots.put(i, "ds_write_b128 %%[red], %s offset:%d" % (rng(EXT0 + 4 * j), i * 1088))
                for i, j in enumerate(js):
                    slots.put(6 + i, "ds_read_b128 %%[%s], %%[red] offset:%d" % (ext_out[j], i * 1088))
            if slabs and u < 3:                          # three slab stores per unit in units 0..2 (gate u)
                for i in range(3):
                    slots.put(5 + 2 * i, lanes32(slabs[3 * u + i], self.masked), SLAB)
            if u == self.poll_unit:
                slots.put(8, "global_load_dword %[pv], %[pcnt], off sc1", ("poll", 0))
            if u == self.poll_unit + 1:                  # the NEXT phase's epilogue operands: behind the counter load, they stay in flight past the end
                for i, ins in enumerate(ext_loads()):
                    slots.put(3 + i, ins, ("next_ext", 0))
            L.append(self.q.wait_for(("ring", u)))
            if m == 0 and blk < NBLK - 1:
                L.append("s_waitcnt lgkmcnt(0)")
            L += self.q.unit(self.mfmas(u), slots)
            if u == self.u_arr:
                L += self.arrive_block()
                done_arr = True
        assert done_arr
        # the counter value and everything older have landed; the next phase's epilogue operands may still be in flight
        assert self.q.ops[-NEXT:] == [("next_ext", 0)] * NEXT
        L += ["s_waitcnt vmcnt(%d)" % NEXT, "s_waitcnt lgkmcnt(0)", "s_nop 7"]
        L += ["ds_write_b128 %%[red], %s offset:%d" % (rng(VACC + 4 * j, f="v"), j * 1088) for j in range(self.nacc)]
        L.append("s_waitcnt lgkmcnt(0)")
        return L

    def emit_main(self):
        sig = ("const void* xin_, unsigned vo, unsigned lp, unsigned red, int arr, u32* pcnt,\n"
               "        const float* ga, const float* ha, const float* xa")
        ins = '[ga] "v"(ga), [ha] "v"(ha), [xa] "v"(xa)'
        pre = ["const void* xin = fn_uniform_ptr(reinterpret_cast<const float*>(xin_));", "arr = __builtin_amdgcn_readfirstlane(arr);"]
        if self.stores:
            sig += ",\n        void* sbase_, unsigned so0, " + ", ".join("const u32x2& t%d%d" % (g, pc) for g in range(3) for pc in range(3))
            ins += ', [sbase] "s"(sbase), [so0] "v"(so0), ' + ", ".join('[t%d%d] "v"(t%d%d)' % (g, pc, g, pc) for g in range(3) for pc in range(3))
            pre.append("void* sbase = const_cast<float*>(fn_uniform_ptr(reinterpret_cast<const float*>(sbase_)));")
        sig += ",\n        f32x4 (&gt)[4], f32x4& hp, f32x4& xt, unsigned& pv"
        outs = ", ".join(['[gt%d] "=&v"(gt[%d])' % (q, q) for q in range(4)] + ['[hp] "=&v"(hp)', '[xt] "=&v"(xt)', '[pv] "=&v"(pv)'])
        comment = """// %s: K loop of one backward phase on the bf16 MFMA (%d row tile(s) x 2 column tiles, %d units = this wave's K quarter, ring of %d, 12 MFMAs per unit; %s).
// xin = this wave's first K block of THIS phase's operand slab (uniform), vo = byte offset of the half's first row tile (+ lane * 16); lp = LDS byte
// address of this wave's first weight block of column tile 1.  In flight at the start, oldest first: this phase's epilogue operands, the ring (`_pro`)%s.
// arr / pcnt: arrival for the previous phase's epilogue (0 none, 1 due, 2 due and this wave issues it) - its half is the half of the NEXT phase, whose
// counter pcnt also is: the value the loop loads near its end is returned in pv.  ga / ha / xa: epilogue operands of the NEXT phase (saved gates, previous
// state, external gradient): requested here into %s, still in flight at the end, handed over by the NEXT statement; gt / hp / xt: those of THIS phase.%s""" % (
            self.name, self.TH, self.units, self.RU, "issues the previous epilogue's exchange-slab stores" if self.stores else "no stores to issue",
            ", the previous epilogue's dgx / dghn stores (`_out`)" if self.stores else "", rng(EXT0, 24),
            "\n// sbase + so0: exchange slab of the previous epilogue (uniform) and this lane's byte offset of gate 0 in it; t<gate><piece>: its gate gradients dr', dz', dn' r as bf16 triples" if self.stores else "")
        clob = clobber("a", range(RING0, EXT0 + 24)) + clobber("v", range(VACC, VACC + 4 * self.nacc)) + clobber("v", range(VWF, VWF + 24)) + clobber("v", (VO2, VO2 - 1))
        return statement(comment, self.name, sig, pre, self.body(), outs,
                         '[xin] "s"(xin), [vo] "v"(vo), [red] "v"(red), [lp] "v"(lp), [arr] "s"(arr), [pcnt] "v"(pcnt), ' + ins,
                         ['"memory"', '"scc"', '"vcc"'] + clobber("s", range(SB, SB + 4)) + clob)

    def emit_pro(self, name):
        L = (["v_add_u32 v%d, 0x%x, %%[vo]" % (VO2, TILE)] if self.TH == 2 else []) + ["s_mov_b64 s[%d:%d], %%[xin]" % (SB, SB + 1), "s_nop 4"]
        base_blk = 0
        for u in range(self.RU - 1):
            nb = u // self.TH
            if nb != base_blk:
                L += advance((nb - base_blk) * UB, nop=True)
                base_blk = nb
            L += self.load_unit(u)
        comment = "// ring request of a backward phase (units 0 .. %d, three pieces each, %d row tile(s))" % (self.RU - 2, self.TH)
        return statement(comment, name, "const void* xin_, unsigned vo", ["const void* xin = fn_uniform_ptr(reinterpret_cast<const float*>(xin_));"], L, "",
                         '[xin] "s"(xin), [vo] "v"(vo)',
                         ['"memory"', '"scc"'] + clobber("s", (SB, SB + 1)) + clobber("a", range(RING0, RING0 + 12 * (self.RU - 1))) + clobber("v", [VO2]))


def ext_loads():
    """epilogue operands of a phase: saved gates r, z, n, hn (1 KB apart), previous state, external gradient -> a[EXT0 ..]"""
    return (["global_load_dwordx4 %s, %%[ga], off offset:%d" % (rng(EXT0 + 4 * q), q * 1024) for q in range(4)] +
            ["global_load_dwordx4 %s, %%[ha], off" % rng(EXT0 + 16), "global_load_dwordx4 %s, %%[xa], off" % rng(EXT0 + 20)])


def emit_ext(name):
    comment = """// the epilogue operands of the FIRST K phase of a launch (every later phase's are requested by the statement in front of it): saved gates r, z, n, hn
// (1 KB apart), previous state, external gradient -> %s, left in flight""" % rng(EXT0, 24)
    return statement(comment, name, "const float* ga, const float* ha, const float* xa", [], ext_loads(), "", '[ga] "v"(ga), [ha] "v"(ha), [xa] "v"(xa)',
                     ['"memory"'] + clobber("a", range(EXT0, EXT0 + 24)))


def emit_out(name, masked):
    L = ["global_store_dwordx4 %[sg], %[d0], off offset:-2048", "global_store_dwordx4 %[sg], %[d1], off",
         "global_store_dwordx4 %[sg], %[d2], off offset:2048", "global_store_dwordx4 %[sn], %[d3], off"]
    comment = """// the stores of an epilogue item%s nobody in the launch waits for: dgx r / z / n (sg = the middle gate, 2 KB apart) and dghn (sn); d0..d3 = dr', dz', dn', dn' r.
// Counted by the next K loop statement (four operations behind the ring request).""" % (" (lanes 0-31)" if masked else "")
    return statement(comment, name, "float* sg, float* sn, const f32x4& d0, const f32x4& d1, const f32x4& d2, const f32x4& d3", [], lanes32(L, masked), "",
                     '[sg] "v"(sg), [sn] "v"(sn), [d0] "v"(d0), [d1] "v"(d1), [d2] "v"(d2), [d3] "v"(d3)', ['"memory"'] + clobber("s", (SB + 2, SB + 3)))


def emit_pub(name, masked):
    """the 9 exchange-slab stores of an epilogue item: gate g at byte offset 0xC000 g (16 K blocks), piece p 1 KB further"""
    # sbase reaches the statement through v_readfirstlane: a VALU-written SGPR needs 5 wait states before a vector-memory instruction may use it as its
    # scalar base, and the compiler inserts none in front of inline asm (found the hard way: the first store went to {high word, 0} + offset)
    L = ["s_nop 4"]
    for g in range(3):
        if g:
            L.append("v_add_u32 v%d, 0x%x, %%[so0]" % (VO2, 0xC000 * g))
        for pc in range(3):
            L.append("global_store_dwordx2 %s, %%[t%d%d], %%[sbase] offset:%d sc1" % ("%[so0]" if g == 0 else "v%d" % VO2, g, pc, pc * 1024))
    sig = ", ".join("const u32x2& t%d%d" % (g, pc) for g in range(3) for pc in range(3))
    ins = ", ".join('[t%d%d] "v"(t%d%d)' % (g, pc, g, pc) for g in range(3) for pc in range(3))
    comment = """// publication of an epilogue item%s outside of a K loop (iteration 0 of a launch): its gate gradients dr', dz', dn' r as bf16 triples (t<gate><piece>, four
// packed values each) on the exchange slab sbase (uniform) at this lane's byte offset so0 - write-through""" % (" (lanes 0-31)" if masked else "")
    return statement(comment, name, "void* sbase_, unsigned so0, " + sig, ["void* sbase = const_cast<float*>(fn_uniform_ptr(reinterpret_cast<const float*>(sbase_)));"],
                     lanes32(L, masked), "", '[sbase] "s"(sbase), [so0] "v"(so0), ' + ins, ['"memory"'] + clobber("s", (SB + 2, SB + 3)) + clobber("v", [VO2]))


def emit_wload(name):
    """one-time: this wave's K quarter of column tile 0 (12 blocks x 3 KB, contiguous in the fn_frag3_pack image) -> a[0:143] and block 11 of column
    tile 1 -> a[144:155]"""
    L = ["s_mov_b64 s[%d:%d], %%[src0]" % (SB, SB + 1), "s_nop 4"]
    for blk in range(NBLK):
        if blk:
            L += advance(UB, nop=True)
        for pc in range(3):
            L.append("global_load_dwordx4 %s, %%[vo], s[%d:%d] offset:%d" % (rng(W0 + 12 * blk + 4 * pc), SB, SB + 1, pc * 1024))
    L += ["s_mov_b64 s[%d:%d], %%[src1]" % (SB, SB + 1), "s_nop 4"]
    for pc in range(3):
        L.append("global_load_dwordx4 %s, %%[vo], s[%d:%d] offset:%d" % (rng(W1X + 4 * pc), SB, SB + 1, pc * 1024))
    L.append("s_waitcnt vmcnt(0)")
    comment = """// one-time: the register-stationary part of the W_hh^T slice.  src0 = this wave's first K block of column tile 0 in the triple image, src1 = block 11 of
// its quarter of column tile 1 (both uniform), vo = lane * 16.  a[0:155] are read by every K loop statement and never written again."""
    pre = ["const void* src0 = fn_uniform_ptr(reinterpret_cast<const float*>(src0_));", "const void* src1 = fn_uniform_ptr(reinterpret_cast<const float*>(src1_));"]
    return statement(comment, name, "const void* src0_, const void* src1_, unsigned vo", pre, L, "", '[src0] "s"(src0), [src1] "s"(src1), [vo] "v"(vo)',
                     ['"memory"', '"scc"'] + clobber("s", (SB, SB + 1)) + clobber("a", range(W0, W1X + 12)))


HEAD = """// GENERATED by gen_kloop4.py - do not edit.  K loops of the ping-pong, register-stationary backward scan on the bf16 MFMA with exact bf16 triple splits (H = 512).
#pragma once
#include "kloop3_asm.h"
"""

# TH -> (ring depth, unit of the arrival, unit whose MFMAs load the other half's counter)
CONFIG = {"t2": (2, 6, 6, 21), "t1": (1, 6, 6, 10)}


def main(path, overrides=()):
    out = [HEAD]
    cfg = dict(CONFIG)
    for o in overrides:                               # tuning builds: t1=RU,u_arr,poll
        tag, vals = o.split("=")
        cfg[tag] = cfg[tag][:1] + tuple(int(v) for v in vals.split(","))
    for tag in ("t2", "t1"):
        TH, RU, u_arr, poll = cfg[tag]
        for stores in (1, 0):
            out.append(GenX6B("fn_x6_bwd_%s_%s" % (tag, "main" if stores else "first"), TH, RU, stores, u_arr, poll).emit_main())
        out.append(GenX6B("x", TH, RU, 0, u_arr, poll).emit_pro("fn_x6_bwd_%s_pro" % tag))
        out.append(emit_pub("fn_x6_bwd_%s_pub" % tag, TH == 1))
        out.append(emit_out("fn_x6_bwd_%s_out" % tag, TH == 1))
    out.append(emit_ext("fn_x6_bwd_ext"))
    out.append(emit_wload("fn_x6_bwd_wload"))
    open(path, "w").write("\n".join(out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "kloop4_asm.h", sys.argv[2:])
