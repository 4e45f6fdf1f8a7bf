// gru_plan.h - what fn_gru_seq_fwd / fn_gru_seq_bwd / fn_gru_cell_f32 launch, decided in one place: the argument checks, the kernel instances in the
// order they are tried, their row groups, grids and LDS sizes, the per-step configuration and the cell's kernel family - pure functions of the
// descriptors and the number of compute units.  Plain C++17 without HIP headers: gru.hip / gru_persist.hip launch from the plans, fn_gru_fwd_plan /
// fn_gru_bwd_plan / fn_gru_cell_plan hand them out, and csrc/host/gru_plan_check.cpp compiles this file for the host under sanitizers.
// Addresses are integers: inspected for NULL-ness and alignment, never dereferenced.
#pragma once
#include <initializer_list>

#include "../../include/fadernets.h"

constexpr int FN_MAX_GROUPS = 64;                   // row groups of a weight-stationary launch: one 128-byte counter line each in sync_ws
constexpr int RT = 256 + 16;                        // floats of one 16x16 accumulator tile in LDS: MFMA C layout + 4 floats per 16 lanes
constexpr int GRU_WS_MAX_LDS = 160 * 1024 - 64;     // dynamic LDS a weight-stationary scan kernel may ask for
constexpr int GRU_CELL_MAX_LDS = 160 * 1024;        // ... and a cell kernel
constexpr int GRU_NT = 256;                         // threads of every scan workgroup and of the fp32 cells

inline uintptr_t gru_addr(const void* p) { return (uintptr_t)p; }

// ---- scans: argument checks, in the order that decides which code a call with several faults returns --------------------------------
inline int gru_fwd_validate(const FnGruFwd* scans, int n_scans) {
    if (!scans) return FN_E_NULL;
    if (n_scans <= 0 || n_scans > FN_MAX_SCANS) return FN_E_COUNT;
    for (int s = 0; s < n_scans; ++s) {
        const FnGruFwd& d = scans[s];
        if (!d.w_hh_frag || !d.b_hh || !d.h_all || !d.frag_ws) return FN_E_NULL;
        if (d.B <= 0 || d.T <= 0 || d.H <= 0 || (d.H % 32) != 0) return FN_E_SHAPE;
        if (d.gx_table && !d.idx) return FN_E_NULL;
        if ((gru_addr(d.w_hh_frag) | gru_addr(d.frag_ws) | gru_addr(d.h0_frag) | gru_addr(d.h_last_frag)) & 15) return FN_E_ALIGN;
        if (d.h0_frag && !d.h0) return FN_E_NULL;            // the gate epilogue reads the row-major state
    }
    return FN_OK;
}
inline int gru_bwd_validate(const FnGruBwd* scans, int n_scans) {
    if (!scans) return FN_E_NULL;
    if (n_scans <= 0 || n_scans > FN_MAX_SCANS) return FN_E_COUNT;
    for (int s = 0; s < n_scans; ++s) {
        const FnGruBwd& d = scans[s];
        if (!d.w_hh_t_frag || !d.h_all || !d.gates || !d.dgx_all || !d.dghn_all || !d.scratch || !d.frag_ws) return FN_E_NULL;
        if (d.B <= 0 || d.T <= 0 || d.H <= 0 || (d.H % 32) != 0) return FN_E_SHAPE;
        if ((gru_addr(d.w_hh_t_frag) | gru_addr(d.frag_ws)) & 15) return FN_E_ALIGN;
    }
    return FN_OK;
}

// ---- scans: the shape predicates -----------------------------------------------------------------------------------------------------
// compute units the launch of these scans may occupy: the device's, or scans[0].cu_budget when that is smaller
template <class Scan>
int budget_cus(const Scan* scans, int cus) {
    return scans[0].cu_budget > 0 && scans[0].cu_budget < cus ? scans[0].cu_budget : cus;
}

// row groups that fit with one workgroup per compute unit and slice
inline int max_groups(int cus, int nslices) { return cus / nslices < FN_MAX_GROUPS ? cus / nslices : FN_MAX_GROUPS; }

// the operands the 16-byte vectors of the weight-stationary epilogues touch
inline uintptr_t ws_align_mask(const FnGruFwd& d) {
    return gru_addr(d.b_hh) | gru_addr(d.b_ih) | gru_addr(d.h0) | gru_addr(d.gx_dense) | gru_addr(d.gx_table) | gru_addr(d.gx_rowbias) | gru_addr(d.h_all) |
           gru_addr(d.gates);
}
inline uintptr_t ws_align_mask(const FnGruBwd& d) {
    return gru_addr(d.h0) | gru_addr(d.h_all) | gru_addr(d.gates) | gru_addr(d.dh_last) | gru_addr(d.dh_ext) | gru_addr(d.dgx_all) | gru_addr(d.dghn_all) |
           gru_addr(d.dh0) | gru_addr(d.dgx_rowsum) | gru_addr(d.dghn_rowsum);
}

// why a call cannot be ONE weight-stationary launch whatever its row blocks (FN_GRU_WS_PRESENT: it can); cus: after the budget
template <class Scan>
int ws_absent(const Scan* scans, int n_scans, int cus) {
    const int H = scans[0].H;
    if (H > 512) return FN_GRU_WS_H_OVER_512;
    if (!scans[0].sync_ws) return FN_GRU_WS_NO_SYNC_WS;
    int Tmax = 0;
    for (int s = 0; s < n_scans; ++s) {
        if (scans[s].H != H) return FN_GRU_WS_MIXED_H;
        if (ws_align_mask(scans[s]) & 15) return FN_GRU_WS_UNALIGNED;      // the epilogue moves 16-byte vectors
        Tmax = scans[s].T > Tmax ? scans[s].T : Tmax;
    }
    if (Tmax < 2) return FN_GRU_WS_T_BELOW_2;                               // nothing to keep stationary
    if (cus <= 0 || H / 16 > cus) return FN_GRU_WS_SLICES_OVER_CUS;
    return FN_GRU_WS_PRESENT;
}

// bf16 x 6 forward scans: row tiles per wave (1 = 64-row groups, 2 = 128-row groups) of the launch, 0 = not eligible.  H = 512, every scan in
// full row groups, saved gates, T >= 2, all row groups resident at once.
inline int x6_row_tiles(const FnGruFwd* scans, int n_scans, int maxgroups) {
    if (scans[0].H != 512) return 0;
    long g64 = 0, g128 = 0;
    bool d64 = true, d128 = true;
    for (int s = 0; s < n_scans; ++s) {
        const FnGruFwd& d = scans[s];
        if (d.H != 512 || !d.gates || d.T < 2) return 0;
        d64 = d64 && d.B % 64 == 0; d128 = d128 && d.B % 128 == 0;
        g64 += d.B / 64; g128 += d.B / 128;
    }
    return (d64 && g64 <= maxgroups) ? 1 : ((d128 && g128 <= maxgroups) ? 2 : 0);
}

// The shapes of the register-stationary backward (gru_bwd_rs_kernel and its bf16 x 6 form gru_bwd_x6_kernel): row tiles per half (2 = 64-row groups,
// 1 = 32-row groups), 0 = not eligible.  H = 512, every scan in full row groups, T >= 2, more than half of the chip and at most all of it (16 slices
// x <= 16 groups, all resident).  half_chip_ok: exactly half of the chip too (g64 * 16 == cus: the caller asked for exactly this with a CU budget -
// the half-chip launches of the decoder pipeline's backward, 8 groups on 128 CUs); rows32_ok: 32-row groups too.
inline int bwd_rs_tiles(const FnGruBwd* scans, int n_scans, int cus, bool half_chip_ok, bool rows32_ok) {
    if (scans[0].H != 512) return 0;
    long g64 = 0, g32 = 0;
    bool d64 = true, d32 = true;
    for (int s = 0; s < n_scans; ++s) {
        const FnGruBwd& d = scans[s];
        if (d.H != 512 || d.T < 2) return 0;
        g64 += d.B / 64; g32 += d.B / 32;
        d64 = d64 && d.B % 64 == 0;
        d32 = d32 && d.B % 32 == 0;
    }
    if (d64 && (g64 > 8 || (half_chip_ok && g64 * 16 == cus)) && g64 <= 16 && g64 * 16 <= cus) return 2;
    return (rows32_ok && d32 && g32 > 8 && g32 <= 16 && g32 * 16 <= cus) ? 1 : 0;
}

// bf16 x 6 backward scans.  64-row groups (the encoder shape: 4 scans x 256 rows): 3.05 ms against 3.5 ms on the fp32 MFMA.  32-row groups (a
// decoder-pipeline launch: 2 scans x 256 rows x 32 steps) measured SLOWER than the fp32 kernel (353 against 322-337 us: both are bound by the exchange
// stream through the XCD's L2, which the triples make 1.5 x wider, and the 12-unit K loops are too short for the store -> arrival -> counter chain):
// only on request (FN_GRU_X6_BWD_32ROWS)
inline int x6_bwd_tiles(const FnGruBwd* scans, int n_scans, int cus) {
    return bwd_rs_tiles(scans, n_scans, cus, true, (scans[0].variant & FN_GRU_X6_BWD_32ROWS) != 0);
}

// smallest row block of the 32-slice kernels whose group count fits on the chip with one workgroup per CU (FN_GRU_ROWS_MASK: that block or none);
// 0 = none fits
template <class Scan>
int pick_rows(const Scan* scans, int n_scans, int maxgroups) {
    const int force_rows = scans[0].variant & FN_GRU_ROWS_MASK;
    for (const int rpw : {16, 32, 64, 128}) {
        if (force_rows && force_rows != rpw) continue;
        long groups = 0;
        for (int s = 0; s < n_scans; ++s) groups += (scans[s].B + rpw - 1) / rpw;
        if (groups <= maxgroups) return rpw;
    }
    return 0;
}

// K split of the 32-slice kernels' tiling for a row block
inline int k_split(int rpw, int variant) { return rpw == 16 ? 4 : rpw == 32 ? 2 : (rpw == 64 && !(variant & FN_GRU_ALT_TILING)) ? 2 : 1; }

// would fn_gru_seq_fwd / fn_gru_seq_bwd take this call with FN_GRU_BF16X6?  Shapes only: pointers are not looked at beyond NULL-ness of `gates`.
// cus: of the device
inline int gru_fwd_x6_ok(const FnGruFwd* scans, int n_scans, int cus) {
    if (!scans || n_scans < 1 || n_scans > FN_MAX_SCANS) return 0;
    cus = budget_cus(scans, cus);
    return cus >= 32 && x6_row_tiles(scans, n_scans, max_groups(cus, 32)) != 0;
}
inline int gru_bwd_x6_ok(const FnGruBwd* scans, int n_scans, int cus) {
    if (!scans || n_scans < 1 || n_scans > FN_MAX_SCANS) return 0;
    return x6_bwd_tiles(scans, n_scans, budget_cus(scans, cus)) != 0;
}

// ---- scans: dynamic LDS of the weight-stationary kernels (bytes) ------------------------------------------------------------------------
// bf16 x 6 forward: 3 stages of 16 x 3 KB weight triples + the accumulator tiles of the 4 waves x 3 gates
inline int lds_fwd_x6() { return 3 * 16 * 3 * 1024 + 4 * 3 * RT * 4 + 16; }
// 32-slice forward: the W_hh slice (48 rows x H) + per K-split wave and row tile the 3 gates' accumulator tiles
inline int lds_fwd_ws(int H, int rpw, int wk) { return (3 * H * 16 + wk * (rpw / 16) * 3 * RT) * 4 + 16; }
// bf16 x 6 backward: 4 x 11 blocks of 3 KB + the tiles of th row tiles per half
inline int lds_bwd_x6(int th) { return 4 * 11 * 3072 + 4 * (2 * th) * RT * 4 + 16; }
// register-stationary backward: the W_hh^T slice + 2 x 4 waves x (2 th) tiles
inline int lds_bwd_rs(int H, int th) { return (3 * H * 16 + 2 * 4 * (2 * th) * RT) * 4 + 16; }
// 32-slice backward: the W_hh^T slice + 2 tiles per K-split wave and row tile
inline int lds_bwd_ws(int H, int rpw, int wk) { return (3 * H * 16 + 2 * wk * (rpw / 16) * RT) * 4 + 16; }

// ---- scans: the per-step kernels ----------------------------------------------------------------------------------------------------------
// (TM, TN, D) = M-tiles per workgroup, N-tiles (backward only), chunks in flight per wave; NS = the scan slots of the instance; tiles = the
// workgroups.  Picked by measurement on MI355X (profiles/).  active = 0: nothing runs at this step.
struct StepCfg {
    int tm, tn, d, ns, active, tiles;
};
inline int step_slots(int active) { return active == 1 ? 1 : active <= 3 ? 3 : active == 4 ? 4 : 8; }
// forward step p: row-tile height 64 rows when the launch already fills the chip, 32 otherwise (more workgroups)
inline StepCfg gru_fwd_step_cfg(const FnGruFwd* scans, int n_scans, int p) {
    long big_tiles = 0;
    int active = 0;
    for (int s = 0; s < n_scans; ++s)
        if (p < scans[s].T) {
            big_tiles += (long)((scans[s].B + 63) / 64) * (scans[s].H / 16);
            ++active;
        }
    StepCfg c = big_tiles >= 256 ? StepCfg{4, 0, 1, 0, 0, 0} : StepCfg{2, 0, 3, 0, 0, 0};
    c.active = active;
    c.ns = step_slots(active);
    for (int s = 0; s < n_scans; ++s)
        if (p < scans[s].T) c.tiles += ((scans[s].B + 16 * c.tm - 1) / (16 * c.tm)) * (scans[s].H / 16);
    return c;
}
// backward iteration it in [0, Tmax]: the gate backward of step T - 1 - it of every scan that still has one, and the dh0 product of a scan at it == T
inline bool gru_bwd_step_active(const FnGruBwd& d, int it) { return !(it > d.T || (it == d.T && !d.dh0)); }
inline StepCfg gru_bwd_step_cfg(const FnGruBwd* scans, int n_scans, int it) {
    long big_tiles = 0;
    int active = 0;
    for (int s = 0; s < n_scans; ++s)
        if (gru_bwd_step_active(scans[s], it)) {
            big_tiles += (long)((scans[s].B + 63) / 64) * ((scans[s].H + 31) / 32);
            ++active;
        }
    StepCfg c = big_tiles >= 192 ? StepCfg{4, 1, 2, 0, 0, 0} : StepCfg{2, 1, 3, 0, 0, 0};
    c.active = active;
    c.ns = step_slots(active);
    for (int s = 0; s < n_scans; ++s)
        if (gru_bwd_step_active(scans[s], it)) c.tiles += ((scans[s].B + 16 * c.tm - 1) / (16 * c.tm)) * ((scans[s].H + 16 * c.tn - 1) / (16 * c.tn));
    return c;
}

// ---- scans: the plans ---------------------------------------------------------------------------------------------------------------------
template <class Scan>
FnGruCandidate ws_candidate(const Scan* scans, int n_scans, int kernel, int rows_per_group, int slices, int lds_bytes, bool triples) {
    FnGruCandidate c{};
    c.kernel = kernel;
    c.rows_per_group = rows_per_group;
    for (int s = 0; s < n_scans; ++s) c.groups += (scans[s].B + rows_per_group - 1) / rows_per_group;
    c.slices = slices;
    c.grid = c.groups * slices;
    c.lds_bytes = lds_bytes;
    c.h0_triples = triples;
    c.resident = 1;
    c.fits = -1;
    return c;
}
inline FnGruCandidate step_candidate(int kernel, const StepCfg& first, int launches) {
    FnGruCandidate c{};
    c.kernel = kernel;
    c.fits = 1;
    c.tm = first.tm; c.tn = first.tn; c.d = first.d; c.ns = first.ns; c.tiles = first.tiles;
    c.launches = launches;
    return c;
}
// the tiling <WM, WK, MT> of the 32-slice kernels for a row block, as an offset into the five FN_GRU_*_WS_* entries
inline int ws_tiling(int rpw, int variant) { return rpw == 128 ? 0 : rpw == 64 ? ((variant & FN_GRU_ALT_TILING) ? 1 : 2) : rpw == 32 ? 3 : 4; }
// a plan whose only candidate is the per-step one launches it
inline void plan_close(FnGruPlan& p) { p.chosen = p.n == 1 && !p.cand[0].resident ? 0 : -1; }

// fn_gru_seq_fwd.  cus: compute units of the device
inline FnGruPlan gru_fwd_plan(const FnGruFwd* scans, int n_scans, int cus) {
    FnGruPlan p{};
    p.chosen = -1;
    if ((p.status = gru_fwd_validate(scans, n_scans)) != FN_OK) return p;
    p.cus = budget_cus(scans, cus);
    const int H = scans[0].H, variant = scans[0].variant, nslices = H / 16;
    p.ws_absent = ws_absent(scans, n_scans, p.cus);
    if (variant & FN_GRU_BF16X6) {
        // exact split products on the bf16 MFMA (gru_fwd_x6_kernel).  The caller hands over w_hh_frag = fn_frag3_pack image and frag_ws of
        // 3 * fn_frag_floats(B, H) floats.  The per-step kernels do not read triple images: this candidate or none.
        const int mt = p.ws_absent ? 0 : x6_row_tiles(scans, n_scans, max_groups(p.cus, nslices));
        if (!mt) {
            p.ws_absent = p.ws_absent ? p.ws_absent : FN_GRU_WS_NO_ROW_BLOCK;
            p.status = FN_E_UNSUPPORTED;
            return p;
        }
        FnGruCandidate c = ws_candidate(scans, n_scans, 0, 64 * mt, nslices, lds_fwd_x6(), true);
        // ping-pong form (kloop3_asm.h): exactly one input source per scan; FN_GRU_X6_SINGLE_GROUP keeps the single-group kernel (tests)
        bool pp = !(variant & FN_GRU_X6_SINGLE_GROUP) && 2 * c.groups <= FN_MAX_GROUPS;
        for (int s = 0; s < n_scans && pp; ++s) pp = (scans[s].gx_table != nullptr) != (scans[s].gx_dense != nullptr);
        c.kernel = pp ? (mt == 1 ? FN_GRU_FWD_X6PP_2 : FN_GRU_FWD_X6PP_1) : (mt == 1 ? FN_GRU_FWD_X6_1 : FN_GRU_FWD_X6_2);
        p.cand[p.n++] = c;
        return p;
    }
    const int rpw = p.ws_absent ? 0 : pick_rows(scans, n_scans, max_groups(p.cus, nslices));
    if (rpw) {
        const int wk = k_split(rpw, variant);
        FnGruCandidate c = ws_candidate(scans, n_scans, 0, rpw, nslices, lds_fwd_ws(H, rpw, wk), false);
        c.no_hand = (variant & FN_GRU_COMPILER_LOOPS) ? 1 : 0;
        // ping-pong form (two halves per workgroup, kloop2_asm.h): H = 512, 128- or 64-row groups, full row groups, saved gates, one input source
        bool pp = H == 512 && (rpw == 128 || (rpw == 64 && wk == 2)) && !(variant & (FN_GRU_COMPILER_LOOPS | FN_GRU_NO_PINGPONG)) &&
                  2 * c.groups <= FN_MAX_GROUPS;
        for (int s = 0; s < n_scans && pp; ++s) {
            const FnGruFwd& d = scans[s];
            pp = d.B % rpw == 0 && d.gates && d.T >= 2 && ((d.gx_table != nullptr) != (d.gx_dense != nullptr));
        }
        c.kernel = pp ? (rpw == 128 ? FN_GRU_FWD_PP_1 : FN_GRU_FWD_PP_2) : FN_GRU_FWD_WS_4_1_2 + ws_tiling(rpw, variant);
        p.cand[p.n++] = c;
    } else if (!p.ws_absent) {
        p.ws_absent = FN_GRU_WS_NO_ROW_BLOCK;
    }
    int Tmax = 0;
    for (int s = 0; s < n_scans; ++s) Tmax = scans[s].T > Tmax ? scans[s].T : Tmax;
    p.cand[p.n++] = step_candidate(FN_GRU_FWD_STEP, gru_fwd_step_cfg(scans, n_scans, 0), Tmax);
    plan_close(p);
    return p;
}

// fn_gru_seq_bwd.  cus: compute units of the device
inline FnGruPlan gru_bwd_plan(const FnGruBwd* scans, int n_scans, int cus) {
    FnGruPlan p{};
    p.chosen = -1;
    if ((p.status = gru_bwd_validate(scans, n_scans)) != FN_OK) return p;
    p.cus = budget_cus(scans, cus);
    const int H = scans[0].H, variant = scans[0].variant, nslices = H / 16;
    p.ws_absent = ws_absent(scans, n_scans, p.cus);
    if (variant & FN_GRU_BF16X6) {
        // exact split products on the bf16 MFMA (gru_bwd_x6_kernel): w_hh_t_frag = the bf16 triple image of W_hh^T (fn_weight_images kind 4), frag_ws of
        // 3 * fn_frag_floats(B, 3H) floats (the gate gradients are exchanged as triples).  This candidate or none.
        const int th = p.ws_absent ? 0 : x6_bwd_tiles(scans, n_scans, p.cus);
        if (!th) {
            p.ws_absent = p.ws_absent ? p.ws_absent : FN_GRU_WS_NO_ROW_BLOCK;
            p.status = FN_E_UNSUPPORTED;
            return p;
        }
        p.cand[p.n++] = ws_candidate(scans, n_scans, th == 2 ? FN_GRU_BWD_X6_2 : FN_GRU_BWD_X6_1, 32 * th, 16, lds_bwd_x6(th), true);
        return p;
    }
    if (!p.ws_absent) {
        // Register-stationary ping-pong form (gru_bwd_rs_kernel): 16 slices of 32 columns x up to 16 groups of 64 (or 32) rows, the shapes of
        // bwd_rs_tiles (smaller problems keep the 32-slice kernels).  FN_GRU_COMPILER_LOOPS / _NO_PINGPONG / _NO_RS_BWD and a forced row block select
        // the 32-slice loops.
        const int th = (variant & (FN_GRU_COMPILER_LOOPS | FN_GRU_NO_PINGPONG | FN_GRU_NO_RS_BWD | FN_GRU_ROWS_MASK)) ? 0 : bwd_rs_tiles(scans, n_scans, p.cus, false, true);
        if (th) p.cand[p.n++] = ws_candidate(scans, n_scans, th == 2 ? FN_GRU_BWD_RS_2 : FN_GRU_BWD_RS_1, 32 * th, 16, lds_bwd_rs(H, th), false);
        const int rpw = pick_rows(scans, n_scans, max_groups(p.cus, nslices));
        if (rpw) {
            FnGruCandidate c = ws_candidate(scans, n_scans, FN_GRU_BWD_WS_4_1_2 + ws_tiling(rpw, variant), rpw, nslices, lds_bwd_ws(H, rpw, k_split(rpw, variant)), false);
            c.no_hand = (variant & FN_GRU_COMPILER_LOOPS) ? 1 : 0;
            p.cand[p.n++] = c;
        } else if (!p.n) {
            p.ws_absent = FN_GRU_WS_NO_ROW_BLOCK;
        }
    }
    int Tmax = 0, launches = 0;
    for (int s = 0; s < n_scans; ++s) Tmax = scans[s].T > Tmax ? scans[s].T : Tmax;
    for (int it = 0; it <= Tmax; ++it) launches += gru_bwd_step_cfg(scans, n_scans, it).active != 0;      // (iteration 0 always runs: T >= 1)
    p.cand[p.n++] = step_candidate(FN_GRU_BWD_STEP, gru_bwd_step_cfg(scans, n_scans, 0), launches);
    plan_close(p);
    return p;
}

// ---- the cell -----------------------------------------------------------------------------------------------------------------------------
inline int cell_k1(const FnGruCell& c) { return c.x ? c.K1 : 0; }
inline int cell_kmax(const FnGruCell& c) { return c.x ? (c.K1 > c.H ? c.K1 : c.H) : c.H; }

// the LDS-free loop: 16-byte aligned operands, K1 % 16 == 0, row strides % 4 == 0, spans below 4 GB (32-bit lane offsets)
inline bool cell_direct_ok(const FnGruCell& a) {
    auto al = [](const void* p) { return (gru_addr(p) & 15) == 0; };
    if ((a.H % 32) != 0 || !al(a.h_prev) || !al(a.w_hh) || (a.ldh & 3) || (a.ldw_hh & 3)) return false;
    if (!al(a.h_out) || (a.ldo & 3) || !al(a.b_hh) || (a.b_ih && !al(a.b_ih)) || (a.gx_table && !al(a.gx_table)) || (a.gx_rowbias && !al(a.gx_rowbias))) return false;
    if ((long)a.B * a.ldh * 4 >= (1L << 32) || 3L * a.H * a.ldw_hh * 4 >= (1L << 32)) return false;
    if (a.x) {
        if ((a.K1 % 16) != 0 || !al(a.x) || !al(a.w_ih) || (a.ldx & 3) || (a.ldw_ih & 3)) return false;
        if ((long)a.B * a.ldx * 4 >= (1L << 32) || 3L * a.H * a.ldw_ih * 4 >= (1L << 32)) return false;
    }
    return true;
}
// dynamic LDS of the cell families (bytes): two stages of a BM x 32 and a 96 x 32 operand tile, rows padded by 4 floats (Stage<ROWS, 32, true, NT>);
// the 48 weight rows of a workgroup's 16 units over the longer K + 4 waves x 4 tiles of 320 floats; the three 48 KB stages of the bf16 x 6 kernels
inline int lds_cell_staged(int bm) { return 2 * (bm * (32 + 4) + 96 * (32 + 4)) * 4; }
inline long lds_cell_wlds(int kmax) { return (long)48 * kmax * 4 + 4 * 4 * 320 * 4; }
inline int lds_cell_x6() { return 3 * (4 * (4 * 3 * 64)) * 16; }
// the weight slice of a workgroup fits LDS
inline bool cell_wlds_ok(const FnGruCell& a) { return lds_cell_wlds(cell_kmax(a)) <= GRU_CELL_MAX_LDS; }
// ... and fills under the K loops: K1 = H = 512
inline bool cell_wlds_ovl_ok(const FnGruCell& a) { return a.H == 512 && (!a.x || a.K1 == 512); }
inline bool cell_x6_ok(const FnGruCell& a) {
    const uintptr_t al = gru_addr(a.x) | gru_addr(a.w_ih) | gru_addr(a.h_prev) | gru_addr(a.w_hh) | gru_addr(a.h_out) | gru_addr(a.b_hh) | gru_addr(a.b_ih) |
                         gru_addr(a.gx_table) | gru_addr(a.gx_rowbias);
    return (a.B % 128) == 0 && (a.H % 32) == 0 && a.H >= 64 && (!a.x || ((a.K1 % 32) == 0 && (a.ldx & 3) == 0 && (a.ldw_ih & 3) == 0)) && (a.ldh & 3) == 0 &&
           (a.ldw_hh & 3) == 0 && (a.ldo & 3) == 0 && (al & 15) == 0;
}
inline bool cell_family_ok(int family, const FnGruCell& a) {
    return family == FN_CELL_STAGED || (cell_direct_ok(a) && (family == FN_CELL_DIRECT || (family == FN_CELL_WLDS ? cell_wlds_ok(a) : cell_wlds_ovl_ok(a))));
}

// tuning / tests: the forced forms, by kernel family (the staged forms agree bit for bit, the LDS-free forms 4-7 among themselves: another k order).
// A form this shape is not eligible for, and any other variant, runs the staged default (form 8).
struct CellForm {
    int variant, family, t0, t1, t2;
};
constexpr CellForm CELL_FORMS[] = {
    {15, FN_CELL_WLDS_OVL, 2, 4, 0}, {16, FN_CELL_WLDS_OVL, 3, 2, 0}, {17, FN_CELL_WLDS_OVL, 4, 2, 0}, {18, FN_CELL_WLDS_OVL, 2, 2, 0},
    {13, FN_CELL_WLDS, 3, 4, 0},     {14, FN_CELL_WLDS, 3, 2, 0},     {9, FN_CELL_WLDS, 4, 2, 0},           // (<4, 4> needs AGPR copies: not built)
    {10, FN_CELL_WLDS, 2, 4, 0},     {11, FN_CELL_WLDS, 4, 2, 0},     {12, FN_CELL_WLDS, 2, 8, 0},
    {4, FN_CELL_DIRECT, 4, 1, 0},    {5, FN_CELL_DIRECT, 2, 4, 0},    {6, FN_CELL_DIRECT, 4, 2, 0},    {7, FN_CELL_DIRECT, 2, 2, 0},
    {1, FN_CELL_STAGED, 128, 4, 1},  {2, FN_CELL_STAGED, 128, 2, 2},  {3, FN_CELL_STAGED, 64, 4, 1},   {8, FN_CELL_STAGED, 64, 2, 2},
};

inline int gru_cell_validate(const FnGruCell* c) {
    if (!c || !c->h_prev || !c->w_hh || !c->b_hh || !c->h_out) return FN_E_NULL;
    if (c->B <= 0 || c->H <= 0 || (c->H % 32) != 0 || c->ldh < c->H || c->ldo < c->H || c->ldw_hh < c->H) return FN_E_SHAPE;
    if (c->x && (!c->w_ih || c->K1 <= 0 || c->ldx < c->K1 || c->ldw_ih < c->K1)) return FN_E_SHAPE;
    if (c->gx_table && c->idx && c->idx_ld <= 0) return FN_E_SHAPE;
    if (c->h_out == c->h_prev) return FN_E_SHAPE;              // other workgroups still read the old state
    if (c->idx_best && (c->best_v <= 0 || !c->gx_table)) return FN_E_SHAPE;
    return FN_OK;
}

// fn_gru_cell_f32
inline FnGruCellPlan gru_cell_plan(const FnGruCell* cell) {
    FnGruCellPlan p{};
    if ((p.status = gru_cell_validate(cell)) != FN_OK) return p;
    const FnGruCell& c = *cell;
    p.has_tab = c.gx_table != nullptr;
    p.has_rb = c.gx_rowbias != nullptr;
    p.kmax = cell_kmax(c);
    p.threads = GRU_NT;
    auto form = [&p](int family, int t0, int t1, int t2) { p.family = family; p.t0 = t0; p.t1 = t1; p.t2 = t2; };
    // FN_GRU_BF16X6 (as in FnGruFwd): the cell on the bf16 MFMA with exact triple splits where the shape allows it (else the fp32 cells below, as if
    // the bit were clear)
    const int variant = c.variant & ~FN_GRU_BF16X6;
    if ((c.variant & FN_GRU_BF16X6) && cell_x6_ok(c)) {
        form(FN_CELL_X6, 0, 0, 0);
    } else if (variant == 0 && c.B > 512 && c.B <= 2048 && cell_direct_ok(c) && cell_wlds_ovl_ok(c)) {
        // measured (us per token of the tokens-only decode, profiles/r04_decode_cells_lds_free.txt): the form with the weight slice in LDS wants ONE
        // workgroup per CU: 64 RT rows x 16 units with RT = ceil(rows / 512) - 1024 rows 71.5 (staged 82, LDS-free 77), 1152-1536 rows 88-89 (LDS-free
        // 101-102); at 2048 rows (RT = 4) it is behind the LDS-free 128-row form (108 against 103).
        // K1 = H = 512: the slice fills under the K loops - 640-1024 rows 60 (71), 1280-1536 rows 78-80 (88), 2048 rows 99.8 (102.9 LDS-free)
        form(FN_CELL_WLDS_OVL, c.B <= 1024 ? 2 : c.B <= 1536 ? 3 : 4, 2, 0);
    } else if (variant == 0 && c.B > 512 && cell_direct_ok(c)) {
        if (c.B > 1536 || !cell_wlds_ok(c)) form(FN_CELL_DIRECT, c.B > 1024 ? 4 : 2, c.B > 1024 ? 2 : 4, 0);
        else form(FN_CELL_WLDS, c.B > 1024 ? 3 : 2, c.B > 1024 ? 2 : 4, 0);
    } else {
        form(FN_CELL_STAGED, 64, 2, 2);
        for (const CellForm& f : CELL_FORMS)
            if (f.variant == variant && cell_family_ok(f.family, c)) {
                form(f.family, f.t0, f.t1, f.t2);
                p.forced_honoured = 1;
                break;
            }
    }
    switch (p.family) {
        case FN_CELL_STAGED:
            p.grid = ((c.B + p.t0 - 1) / p.t0) * (c.H / 32);
            p.lds_bytes = lds_cell_staged(p.t0);
            break;
        case FN_CELL_DIRECT: p.grid = ((c.B + 32 * p.t0 - 1) / (32 * p.t0)) * (c.H / 32); break;
        case FN_CELL_WLDS:
        case FN_CELL_WLDS_OVL:
            p.grid = ((c.B + 64 * p.t0 - 1) / (64 * p.t0)) * (c.H / 16);
            p.lds_bytes = (int)lds_cell_wlds(p.family == FN_CELL_WLDS ? p.kmax : 512);
            break;
        default:
            p.grid = (c.B / 128) * (c.H / 32);
            p.threads = 512;
            p.lds_bytes = lds_cell_x6();
    }
    return p;
}
