"""CPU half of the bf16 x 6 GEMM suite (the GPU half: tests/test_gpu_gemm_x6_paths.py): the mirror of a bf16 x 6 launch against the library's
own plan over every case and a seeded sweep, what the case table reaches, the trip schedule against a literal replay of x6w_trips, the exact conditions,
the placement and the pieces of the wide values, the restatement on every case, and planted faults - each an edit of the restatement's arrays - that the
whole-tensor metric of tests/test_gpu_parity.py (2e-6 of max |A|^T |B|) accepts and the passes here reject with the tile named."""
import random

import numpy as np
import pytest
import torch

from helpers import SCAN_MIN_REF
from helpers_gemm import (GEMM_SENTINEL, NTX6, PLAN_CUS, X6_TRIPS, X6P, X6V, X6W, assert_dwhh_mirror_matches_library, assert_mirror_matches_library, c_buffer,
                          check_exact, check_normal, dwhh_plan, gemm_instance, k_ranges, lib_dwhh_plan, lib_gemm_plan, make_problem, trip_schedule)
from helpers_gemm_x6 import (AB2_K, EXACT_MODES, MAX_ABS, PA, PASS_OF_PRODUCT, PB, PRODUCT_NAMES, WIDE_PER_VECTOR, X6_BY_ID, X6_CASES, X6_F, X6_MODES,
                             X6_NT_BELOW, ab2_positions, assert_x6_plan_matches_case, case_ranges, dwhh_tensors, split3, x6_case_plan,
                             x6_coverage_reached, x6_coverage_wanted, x6_cut, x6_flags, x6_operands, x6_problem, x6_restate)

IDS = [c["id"] for c in X6_CASES]


def _filled(prob, out, c0=0, ldc=None):
    buf = c_buffer(prob, c0, ldc if ldc is not None else c0 + prob["N"] + 4)
    buf[:prob["M"], c0:c0 + prob["N"]] = out
    return buf


def _lib_plan(case, kern, pertile, cus=PLAN_CUS):
    fl = x6_flags(kern, pertile)
    if case["kind"] == "dwhh":
        return lib_dwhh_plan(case["H"], case["rows"], (0, 0, 0, 0, 0), case["splitk"], False, fl, cus)
    ptrs = (4 * case["a_off"], 4 * case["b_off"], 4 * case["c0"], 4 * case["bias_off"] if case["bias"] else 0, 0)
    return lib_gemm_plan(case["a_k"], case["b_k"], case["M"], case["N"], case["K"], case["lda"], case["ldb"], case["ldc"], ptrs, case["splitk"], False, fl, cus)


# ---- the mirror -------------------------------------------------------------------------------------------------------------------------------------
def test_every_case_reaches_what_its_id_names_and_the_library_agrees():
    """every case x kernel x (walking | FN_GEMM_X6_PERTILE) on its nominal addresses at 256 compute units, and at 250 / 64 / 304: the mirror is what the id
    names and what fn_gemm_plan / fn_gru_dwhh_plan decide, field by field"""
    for case in X6_CASES:
        for kern in case["kernels"]:
            for pertile in (False, True):
                for cus in (PLAN_CUS, 250, 64, 304):
                    mp, lp = x6_case_plan(case, kern, pertile=pertile, cus=cus), _lib_plan(case, kern, pertile, cus)
                    assert_x6_plan_matches_case(case, kern, mp, pertile, cus)
                    if case["kind"] == "dwhh":
                        assert_dwhh_mirror_matches_library(mp, lp, case["H"], case["id"])
                    else:
                        assert_mirror_matches_library(mp, lp, case["M"], case["N"], case["id"])
    walk = x6_case_plan(X6_BY_ID["x-256x256-K2279-split72-1d-288-items-walk"], "128")
    assert (walk["items"], walk["grid_xyz"], walk["walks"], walk["klen"]) == (288, (256, 1, 1), True, 32) and walk["blocks"][-1][:2] == (1, 7)
    assert x6_case_plan(X6_BY_ID["x-256x256-K2279-split72-1d-288-items-walk"], "128", cus=250)["grid_xyz"] == (288, 1, 1)      # no multiple of the 8 XCDs
    assert x6_case_plan(X6_BY_ID["x-256x256-K2279-split72-1d-288-items-walk"], "256")["grid_xyz"] == (144, 1, 1)
    nt = x6_case_plan(X6_BY_ID["xn-4096x1152-K256-nblk8-288-tiles-walk-padded-alpha-beta-bias"], "nt")
    assert (nt["tiles"], nt["grid_xyz"], nt["walks"]) == (288, (256, 1, 1), True)


def test_the_table_reaches_every_kernel_grid_walk_reduction_and_trip_count():
    want, got = x6_coverage_wanted(), x6_coverage_reached()
    assert not want - got, sorted(want - got, key=str)


def test_just_below_each_condition_of_the_nt_dispatch_the_plan_names_an_fp32_kernel():
    for what, M, N, K in X6_NT_BELOW:
        for cus in (PLAN_CUS, 64):
            mp = gemm_instance(True, True, M, N, K, K, K, N, (0, 0, 0, 0, 0), 1, False, x6_flags("nt"), cus)
            lp = lib_gemm_plan(True, True, M, N, K, K, K, N, (0, 0, 0, 0, 0), 1, False, x6_flags("nt"), cus)
            assert mp["family"] in ("staged", "nt-direct") and "x6" not in lp["kernel"] and lp["kernel"] == mp["kernel"], (what, mp, lp)
    lp = lib_gemm_plan(True, True, 2048, 1024, 128, 128, 128, 1024, (0, 0, 0, 0, 0), 1, False, x6_flags("nt"))
    assert lp["kernel"] == NTX6 and lp["grid"] == (128, 1, 1)


def test_mirror_matches_the_library_on_a_seeded_sweep_of_mode_bits():
    """3000 fn_gemm_f32 calls with the bf16 x 6 bit and every combination of the three mode bits - row-contiguous operands of 1 .. 700 x 1 .. 700 x 1 .. 9000
    with 1 .. 80 K ranges asked for, whole-tile K-contiguous ones around the NT kernel's conditions, aligned and not, on 256 / 250 / 64 / 304 / 8 / 0-mod-8
    compute units - and 1000 fn_gru_dwhh_f32 calls: mirror == library in every field; all four kernels, both grid forms, walking and both reductions seen"""
    lib = __import__("helpers_gemm")._lib()
    rnd = random.Random(20261020)
    seen = set()
    for i in range(3000):
        bits = lib.GEMM_BF16X6 | rnd.choice((0, lib.GEMM_X6_PERWAVE)) * (rnd.random() < 0.4) | lib.GEMM_X6_WIDE * (rnd.random() < 0.4) | lib.GEMM_X6_PERTILE * (rnd.random() < 0.3)
        cus = rnd.choice((256, 256, 250, 64, 304, 8, 12))
        if i < 2200:
            a_k = b_k = False
            M, N, K, splitk = rnd.randint(1, 700), rnd.randint(1, 700), rnd.randint(1, 9000), rnd.choice((1, 2, 3, 5, 8, 16, 24, 40, 72, 80))
        else:
            a_k = b_k = True
            M, N, K, splitk = 128 * rnd.choice((8, 15, 16, 32, 36)), 128 * rnd.choice((8, 9, 16)), rnd.choice((96, 128, 144, 160, 416)), rnd.choice((1, 1, 1, 2))
        lda, ldb, ldc = (K if a_k else M) + rnd.choice((0, 0, 1, 2, 3, 4, 8)), (K if b_k else N) + rnd.choice((0, 0, 1, 2, 3, 4, 8)), N + rnd.choice((0, 0, 2, 4))
        if not a_k:
            lda, ldb = (lda + 3) // 4 * 4 if rnd.random() < 0.9 else lda, (ldb + 3) // 4 * 4 if rnd.random() < 0.9 else ldb
        off = lambda: rnd.choice((0, 0, 0, 0, 4, 8, 16))                                                                 # noqa: E731
        ptrs = (1 << 20 | off(), 2 << 20 | off(), 3 << 20 | off(), (4 << 20 | off()) if rnd.random() < 0.7 else 0, 5 << 20 | off())
        mp = gemm_instance(a_k, b_k, M, N, K, lda, ldb, ldc, ptrs, splitk, False, bits, cus)
        lp = lib_gemm_plan(a_k, b_k, M, N, K, lda, ldb, ldc, ptrs, splitk, False, bits, cus)
        assert_mirror_matches_library(mp, lp, M, N, (i, a_k, M, N, K, lda, ldb, ldc, ptrs, splitk, bits, cus))
        if mp["family"] == "x6":
            seen.add((mp["kernel"], mp["grid"], mp["walks"], mp["reduce"]))
    assert {s[0] for s in seen} == {X6P, X6W, X6V, NTX6} and {s[3] for s in seen} == {None, "slab_reduce_kernel", "slab_reduce4_kernel"}
    assert {(k, True) for k in (X6W, X6V, NTX6)} <= {(s[0], s[2]) for s in seen} and (X6P, True) not in {(s[0], s[2]) for s in seen}
    assert {(k, g) for k in (X6P, X6W, X6V) for g in ("1d", "3d")} <= {(s[0], s[1]) for s in seen}
    for i in range(1000):
        H, rows, splitk = rnd.choice((4, 32, 64, 96, 100, 128, 192, 256, 512, rnd.randint(1, 300))), rnd.randint(1, 70000), rnd.choice((1, 2, 3, 8, 16, 32))
        bits = lib.GEMM_BF16X6 | lib.GEMM_X6_PERWAVE * (rnd.random() < 0.3) | lib.GEMM_X6_WIDE * (rnd.random() < 0.4) | lib.GEMM_X6_PERTILE * (rnd.random() < 0.3)
        ptrs = tuple((j + 1) << 24 | rnd.choice((0, 0, 0, 4, 8, 16)) for j in range(5))
        cus = rnd.choice((256, 250, 64))
        mp, lp = dwhh_plan(H, rows, ptrs, splitk, False, bits, cus), lib_dwhh_plan(H, rows, ptrs, splitk, False, bits, cus)
        assert_dwhh_mirror_matches_library(mp, lp, H, (i, H, rows, ptrs, splitk, bits, cus))


def _replay_trips(nblk, NS, LEAD, PARTIAL):
    """x6w_trips (x6w_core.h) replayed line by line: the list of ('request', set, block) / ('cut', set, block, stage) / ('barrier',) / ('fused', ..) events"""
    REST = 2 * NS + LEAD - 2 + (1 if PARTIAL else 0)
    STAGES = LEAD + 1
    ev = []
    for i in range(NS):
        if i < nblk:
            ev.append(("request", i, i))
    for i in range(LEAD):
        if i == 0 or i < nblk:
            ev.append(("cut", i, i, i))
    for i in range(LEAD - 1):
        if NS + i < nblk:
            ev.append(("request", i, NS + i))
    ev.append(("barrier",))
    state = dict(next_stage=LEAD % STAGES)

    def stage_of(blk):
        return blk & (STAGES - 1) if STAGES & (STAGES - 1) == 0 else state["next_stage"]

    def done():
        state["next_stage"] = 0 if state["next_stage"] == STAGES - 1 else state["next_stage"] + 1
        ev.append(("barrier",))

    t = passes = 0
    while t + REST < nblk:
        for r in range(NS):
            ev.append(("fused",))
            ev.append(("request", (r + LEAD - 1) % NS, t + r + NS + LEAD - 1))
            ev.append(("cut", (r + LEAD) % NS, t + r + LEAD, stage_of(t + r + LEAD)))
            done()
        t += NS
        passes += 1
    tail = 0
    for i in range(REST):
        r = i % NS
        if t + i < nblk:
            tail += 1
            if t + i + NS + LEAD - 1 < nblk:
                ev.append(("request", (r + LEAD - 1) % NS, t + i + NS + LEAD - 1))
            if t + i + LEAD < nblk:
                ev.append(("cut", (r + LEAD) % NS, t + i + LEAD, stage_of(t + i + LEAD)))
            done()
    return ev, passes, tail


@pytest.mark.parametrize("kernel", [X6W, X6V, NTX6])
def test_trip_schedule_is_what_x6w_trips_runs(kernel):
    """the mirror's schedule against a replay of the template for nblk = 1 .. 40, and the invariants the kernels rest on: every block is requested once into
    register set b mod NS and cut once from it into stage b mod (LEAD + 1), before the barrier behind which the consumers multiply it and not before the
    barrier that retires the block that held the stage; a register set is not requested again before it was cut; 1 + nblk barriers; the steady state (fused
    trips) touches whole blocks only - never the last one where it may be partial.  gemm_tn_x6v_kernel: x6w_trips<2, 1, true>"""
    NS, LEAD, PARTIAL = X6_TRIPS[kernel]
    assert (NS, LEAD, PARTIAL) == {X6W: (3, 2, True), X6V: (2, 1, True), NTX6: (3, 2, False)}[kernel]
    for nblk in range(1, 41):
        ev, passes, tail = _replay_trips(nblk, NS, LEAD, PARTIAL)
        s = trip_schedule(nblk, NS, LEAD, PARTIAL)
        assert (s["passes"], s["tail"], s["barriers"]) == (passes, tail, sum(e[0] == "barrier" for e in ev)) and s["barriers"] == 1 + nblk
        assert s["passes"] * NS + s["tail"] == nblk and 1 <= s["tail"] <= s["rest"] and s["prologue_only"] == (not any(e[0] == "cut" for e in ev[ev.index(("barrier",)):]))
        nbar, req_at, cut_at, in_set, fused = 0, {}, {}, {}, False
        for e in ev:
            if e[0] == "barrier":
                nbar, fused = nbar + 1, False
            elif e[0] == "fused":
                fused = True
            elif e[0] == "request":
                _, st, b = e
                assert b < nblk and b not in req_at and st == b % NS and in_set.get(st) is None, (nblk, e)
                assert not fused or b < nblk - (1 if PARTIAL else 0), (nblk, e)
                req_at[b], in_set[st] = nbar, b
            else:
                _, st, b, stage = e
                assert b not in cut_at and in_set.get(st) == b and stage == b % (LEAD + 1), (nblk, e)
                assert nbar <= max(0, b - LEAD + 1) and nbar >= b - LEAD, (nblk, e, nbar)            # ready in time, and the stage was free
                assert not fused or b < nblk - (1 if PARTIAL else 0), (nblk, e)
                cut_at[b], in_set[st] = nbar, None
        assert sorted(req_at) == sorted(cut_at) == list(range(nblk))


# ---- the passes: conditions, placement, pieces -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_exact_conditions_wide_value_placement_and_piece_counts(cid):
    """per case: sum |a||b| + |bias| + |beta c| < 2^24 in all four exact passes (make_problem asserts it), and for the wide passes: every (K range, 32-k
    block) holds wide values in each 64-column producer set; across the case they fall on all 32 in-block positions, on blocks of every LDS stage (block
    mod 3, mod 2) and register set; the pieces are what the pass is for - the split computed here: A3 a = three non-zero pieces, b = one; B3 the mirror
    image with a floor on the share of non-zero lo pieces; AB2 two pieces each at the common k set"""
    case = X6_BY_ID[cid]
    M, N, K = case["M"], case["N"], case["K"]
    ranges = case_ranges(case)
    blocks = [(k0 + 32 * j, min(k0 + 32 * j + 32, k1)) for k0, k1 in ranges for j in range((k1 - k0 + 31) // 32)]
    for mode in EXACT_MODES:
        prob = x6_problem(case, mode)                       # asserts the condition and the spans
        a, b = prob["pieces"][0]
        (ah, am, al), (bh, bm, bl) = split3(a.numpy(), False), split3(b.numpy(), True)
        if mode == "small":
            assert not am.any() and not al.any() and not bm.any() and not bl.any()
            continue
        if mode == "AB2":
            ks = ab2_positions(K)
            assert len(ks) <= AB2_K and (am[:, ks] != 0).all() and (bm[ks] != 0).all() and not al.any() and not bl.any()
            rest = np.setdiff1d(np.arange(K), ks)
            assert not am[:, rest].any() and not bm[rest].any()
            assert len({k % 32 for k in ks}) == min(32, K)
            continue
        wide, mid, lo, other = (a.abs() > 8, am, al, (bm, bl)) if mode == "A3" else (b.t().abs() > 8, bm.T, bl.T, (am, al))
        assert not other[0].any() and not other[1].any()                    # the narrow operand is one piece
        nvec = wide.shape[0]
        assert int(wide.sum(1).max()) <= WIDE_PER_VECTOR and int(wide.sum(1).min()) >= 1
        for s0 in range(0, nvec, 64):
            per_block = [bool(wide[s0:s0 + 64, k0:k1].any()) for k0, k1 in blocks]
            assert all(per_block), "%s %s: set %d has no wide value in block %d" % (cid, mode, s0 // 64, per_block.index(False))
        kk = torch.nonzero(wide.any(0)).flatten().tolist()
        assert {k % 32 for k in kk} == set(range(min(32, K))) or K < 32 and len(kk) == K
        nb = {k // 32 for k in kk}
        assert {x % 3 for x in nb} == set(range(min(3, len(blocks)))) and {x % 2 for x in nb} == set(range(min(2, len(blocks))))
        w = wide.numpy()
        assert (mid[w] != 0).all()
        share = float((lo[w] != 0).mean())
        # truncating split: the low 10 bits of an odd value with bit 9 set leave an odd 2-bit rest - always; rounding split: the remainder is an odd
        # integer of [-512, -1] and leaves a rest when it has 9 bits, half of them: a floor of 0.4
        assert share == 1.0 if mode == "A3" else share >= 0.4, (cid, mode, share)
    for name, mode in PASS_OF_PRODUCT.items():              # the product a pass is named for is non-zero there
        c = PRODUCT_NAMES.index(name)
        pa, pb = x6_cut(*x6_problem(case, mode)["pieces"][0])
        assert np.abs(pa[PA[c]]).max() > 0 and np.abs(pb[PB[c]]).max() > 0, (cid, name, mode)


def test_twenty_bit_values_sixteen_per_row_would_leave_the_condition():
    assert 16 * 2 ** 20 * 4 >= 2 ** 24 > WIDE_PER_VECTOR * MAX_ABS["A3"][0] * 4 + 9000 * 32


# ---- the restatement passes its own checks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_restatement_is_exact_on_integers_and_within_its_own_error_on_normals(cid):
    case = X6_BY_ID[cid]
    for perwave in ({False, "perwave" in case["kernels"]}):
        for mode in X6_MODES:
            prob = x6_problem(case, mode, perwave)
            if mode != "normal":
                fake = prob["restate"]()
                assert fake.dtype == torch.float32 and bool((fake.double() == prob["ref64"]).all()), "%s %s: the six-product model is not float64" % (cid, mode)
                assert check_exact(prob, _filled(prob, fake)) == case["M"] * case["N"]
            else:
                assert 0.0 <= check_normal(prob, _filled(prob, prob["fake32"]), F=1)[0] <= 1.0
                assert prob["den"].min() >= SCAN_MIN_REF and len(prob["ranges"]) == len(case_ranges(case))
    if case["kind"] == "dwhh":
        dgx, dghn, hp = dwhh_tensors(case, prob)
        H = case["H"]
        want = case["beta"] * prob["C0"].double() + torch.cat([dgx[:, :2 * H], dghn], 1).double().t() @ hp.double()
        assert float((prob["ref64"] - want).abs().max()) < 1e-9 and not bool((dgx[:, 2 * H:] == dghn).all())


# ---- planted faults ----------------------------------------------------------------------------------------------------------------------------------
SPLIT = X6_BY_ID["x-132x260-K300-split3-3d-last-range-44"]              # ranges of 128, 128 and 44 rows: 4, 4 and 2 blocks, the last one of 12 rows
TILE = (slice(16, 32), slice(32, 48))


def _old_metric_accepts(out, prob):
    """tests/test_gpu_parity.py: max |C - ref64| / max(|A|^T |B|) < 2e-6 over the whole tensor (NaN: not accepted)"""
    a, b = prob["pieces"][0]
    scale = float((a.double().abs() @ b.double().abs()).max())
    return float((out.double() - prob["ref64"]).abs().max()) / scale < 2e-6


def _restated(prob, **kw):
    a, b = prob["pieces"][0]
    return x6_restate(a, b, prob["ranges"], prob["perwave"], prob["alpha"], prob["bias"], prob["beta"], prob["C0"], **kw)


def _good(prob):
    return prob["fake32"] if prob["mode"] == "normal" else prob["restate"]()


def _rejected(prob, out=None, buf=None, tile=None):
    with pytest.raises(AssertionError) as e:
        (check_exact if prob["mode"] == "exact" else check_normal)(prob, _filled(prob, out) if buf is None else buf)
    if tile is not None:
        assert "rows %d.., columns %d.." % tile in str(e.value), str(e.value)
    return True


def _band_problem(case, rows=slice(16, 32), tag="band"):
    """standard normals with the rows `rows` of A^T at 1e-6 of the others (the gradient rows of units that hardly fire): whatever goes wrong in those rows is
    1e-6 of the whole tensor's scale"""
    a, b, _, _ = x6_operands(case["id"] + tag, "normal", case["M"], case["N"], case["K"], False)
    a[rows] *= 1e-6
    ranges = case_ranges(case)
    C0 = torch.zeros(case["M"], case["N"])
    prob = make_problem(case["id"] + "/" + tag, "normal", case["M"], case["N"], [(a, b)], [[(a, b, k0, k1)] for k0, k1 in ranges], 1.0, 0.0, None, C0,
                        restate=lambda: x6_restate(a, b, ranges, False, 1.0, None, 0.0, C0))
    prob.update(ranges=ranges, perwave=False)
    assert _old_metric_accepts(prob["fake32"], prob)
    check_normal(prob, _filled(prob, prob["fake32"]), F=1)
    return prob


def _in_tile(ri, blk, c=None, f=lambda d: 0.0 * d):
    """hook: product c (None: all six) of block blk of range ri, in TILE only"""
    def hook(r, b, cc, dot):
        if (r, b) == (ri, blk) and (c is None or cc == c):
            dot = dot.copy()
            dot[TILE] = f(dot[TILE])
        return dot
    return hook


@pytest.mark.parametrize("name", PRODUCT_NAMES)
def test_fault_one_piece_product_dropped_in_one_block_of_one_tile(name):
    """each of the six, in block 2 of the second K range, rows 16 .. 31 x columns 32 .. 47.  The three with a lo or two mid pieces are, at the K of a training
    step, below the normal pass' bound (5.8e-8, 1.5e-8, 2.9e-8 of the scale at K = 4096, the size of an fp32 product's own error) and invisible to the small
    pass, whose operands are one piece: A3 catches lo*hi, B3 hi*lo, AB2 mid*mid bit for bit at any K - and the whole-tensor metric accepts each, there.  The three larger ones are caught by the
    normal pass in a tile whose rows are small (and by the exact pass named in PASS_OF_PRODUCT)"""
    c = PRODUCT_NAMES.index(name)
    hook = _in_tile(1, 2, c)
    small = x6_problem(SPLIT, "small")
    caught_by_small = not bool((_restated(small, hook=hook) == _good(small)).all())
    assert caught_by_small == (name == "hi*hi")
    exact = x6_problem(SPLIT, PASS_OF_PRODUCT[name])
    out = _restated(exact, hook=hook)
    assert bool((out != _good(exact))[TILE].any()) and int((out != _good(exact)).sum()) == int((out != _good(exact))[TILE].sum())
    assert _rejected(exact, out, tile=(16, 32))
    if name in ("lo*hi", "hi*lo", "mid*mid"):
        assert _old_metric_accepts(out, exact), name
        normal = x6_problem(SPLIT, "normal")                # on normals the same edit is 2^-16 of one block's share: accepted by the whole-tensor metric too
        assert _old_metric_accepts(_restated(normal, hook=hook), normal), name
    else:
        band = _band_problem(SPLIT)
        out = _restated(band, hook=hook)
        assert _old_metric_accepts(out, band) and _rejected(band, out, tile=(16, 32))


def test_fault_mid_and_lo_pieces_of_a_swapped_in_one_block():
    """lo*hi + mid*hi is symmetric in the two pieces, so only products with b's mid see the swap: AB2 (mid*mid is lost), not A3"""
    for mode, caught in (("AB2", True), ("A3", False)):
        prob = x6_problem(SPLIT, mode)
        Ap, Bp = x6_cut(*prob["pieces"][0])
        k0 = 128 + 64
        assert k0 // 32 * 32 in [k // 32 * 32 for k in ab2_positions(SPLIT["K"])]
        Ap[1][16:32, k0:k0 + 32], Ap[2][16:32, k0:k0 + 32] = Ap[2][16:32, k0:k0 + 32].copy(), Ap[1][16:32, k0:k0 + 32].copy()
        out = _restated(prob, cut=(Ap, Bp))
        if caught:
            assert _old_metric_accepts(out, prob) and _rejected(prob, out, tile=(16, 0))
        else:
            assert bool((out == _good(prob)).all())


def test_faults_in_the_block_walk_the_tail_and_the_slabs():
    """in one tile of small rows, accepted by the whole-tensor metric and rejected by the normal pass; the same edit is rejected by the small pass"""
    band, small = _band_problem(SPLIT), x6_problem(SPLIT, "small")
    K = SPLIT["K"]

    def tail_not_zeroed(prob):
        Ap, Bp = x6_cut(*prob["pieces"][0])
        for p in Ap:
            p[16:32, K] = p[16:32, K - 1]
        for p in Bp:
            p[K] = p[K - 1]
        return dict(cut=(Ap, Bp))

    def slab_twice(slabs):
        slabs = [s.copy() for s in slabs]
        slabs[1][TILE] = slabs[1][TILE] * np.float32(2)
        return slabs

    faults = {
        "the last block of the second K range dropped": lambda prob: dict(hook=_in_tile(1, 3)),
        "the last (partial) block of the last K range dropped": lambda prob: dict(hook=_in_tile(2, 1)),
        "the first block of the next pass multiplied twice": lambda prob: dict(hook=_in_tile(1, 3, None, lambda d: 2.0 * d)),
        "the rows of the K tail not zeroed: the last row counted again": tail_not_zeroed,
        "one range's slab added twice": lambda prob: dict(slab_edit=slab_twice),
    }
    for what, edit in faults.items():
        for prob in (band, small):
            out = _restated(prob, **edit(prob))
            assert bool((out != _good(prob)).any()), what
            assert _rejected(prob, out, tile=(16, 32) if "tail" not in what else None), what
        assert _old_metric_accepts(_restated(band, **edit(band)), band), what
    # a 16 x 16 tile transposed, a NaN (which the whole-tensor metric sees too: NaN < 2e-6 is false)
    for prob in (band, small):
        out = _good(prob).clone()
        out[TILE] = out[TILE].t()
        assert _rejected(prob, out, tile=(16, 32))
        nan = _good(prob).clone()
        nan[131, 259] = float("nan")
        assert _rejected(prob, nan, tile=(128, 256)) and not _old_metric_accepts(nan, prob)
    out = band["fake32"].clone()
    out[TILE] = out[TILE].t()
    assert _old_metric_accepts(out, band)


def test_fault_dghn_band_taken_from_dgx():
    """rows [2H, 3H) of dW from dgx[:, 2H:] instead of dghn (the switch to the second A source missed), with the band at 1e-6 of the other gates' scale"""
    case = X6_BY_ID["xd-H64-one-launch-msplit128-ragged-dghn-band-rows1030-split4-beta0"]
    H = case["H"]
    band = _band_problem(case, rows=slice(2 * H, 3 * H), tag="dghn-band")
    dgx, dghn, hp = dwhh_tensors(case, band)
    assert float(dgx[:, 2 * H:].abs().max()) < 1.1
    a2 = torch.cat([dgx[:, :2 * H], dgx[:, 2 * H:] - 1.0], 1).t().contiguous()            # the other values at the band's scale
    out = x6_restate(a2, hp, band["ranges"], False, 1.0, None, 0.0, band["C0"])
    assert bool((out[:2 * H] == band["fake32"][:2 * H]).all())
    assert _old_metric_accepts(out, band) and _rejected(band, out)
    small = x6_problem(case, "small")
    dgx, dghn, hp = dwhh_tensors(case, small)
    a2 = torch.cat([dgx[:, :2 * H], dgx[:, 2 * H:]], 1).t().contiguous()
    assert _rejected(small, x6_restate(a2, hp, small["ranges"], False, 1.0, None, 0.0, small["C0"]), tile=(128, 0))


def test_fault_last_column_window_shifted_instead_of_clamped():
    """M = 342 = 4 x 85 + 2: the window of rows 340 .. 343 must be read where it is; moved back to 338 .. 341 it gives rows 340, 341 the operand columns 338, 339"""
    case = X6_BY_ID["x-342x72-lda344-K75-window-clamp"]
    band = _band_problem(case, rows=slice(336, 342), tag="window")
    for prob in (band, x6_problem(case, "small")):
        a, b = prob["pieces"][0]
        a2 = a.clone()
        a2[340:342] = a[338:340]
        out = x6_restate(a2, b, prob["ranges"], False, prob["alpha"], prob["bias"], prob["beta"], prob["C0"])
        assert bool((out[:340] == _good(prob)[:340]).all()) and _rejected(prob, out)
    assert _old_metric_accepts(out if prob is band else x6_restate(torch.cat([band["pieces"][0][0][:340], band["pieces"][0][0][338:340]]), band["pieces"][0][1],
                                                                   band["ranges"], False, 1.0, None, 0.0, band["C0"]), band)


def test_fault_a_write_outside_the_view():
    """a column >= N, a row >= M: outside what the whole-tensor metric looks at"""
    case = X6_BY_ID["x-342x72-lda344-K500-split8-C-column-342-scalar-reduce"]
    for mode in ("small", "normal"):
        prob = x6_problem(case, mode)
        good = _good(prob)
        for r, c in ((5, case["c0"] + case["N"]), (case["M"], case["c0"]), (0, case["c0"] - 1)):
            buf = _filled(prob, good, case["c0"], case["ldc"])
            assert float(buf[r, c]) == GEMM_SENTINEL
            buf[r, c] = 0.0
            with pytest.raises(AssertionError, match="outside"):
                (check_exact if mode != "normal" else check_normal)(prob, buf, case["c0"])
        assert _old_metric_accepts(good, prob)


def test_beta_zero_starts_from_nan():
    case = X6_BY_ID["x-64x128-K75-second-A-set-beyond-the-matrix"]
    prob = x6_problem(case, "small")
    buf = c_buffer(prob, 0, case["ldc"])
    assert case["beta"] == 0.0 and bool(torch.isnan(buf[:64, :128]).all()) and _rejected(prob, buf=buf)
    assert X6_F and k_ranges(75, 75) == [(0, 75)]
