"""CPU self-test of tests/helpers_gemm.py, which tests/test_gpu_gemm_paths.py applies to the LDS-staged gemm_kernel, gemm_multi_kernel, gemm_tn_kernel /
gemm_tn_lean_kernel (also behind fn_gru_dwhh_f32) and the two slab reductions: the float32 restatement stands in for the kernels.

It shows that the mirror of the dispatch sends every case to the kernel instance, load path, grid form and reduction its id names and that together
the cases reach every combination the mirror can name (one is unreachable, and the table says why); that the restatement passes both passes on every
case - the integer pass bit for bit - and that FakeOps.gemm passes the normal pass too; and that planted faults, each an edit of the restatement, are
rejected, one of which the whole-tensor metric of test_gemm accepts."""
import pytest
import torch

from fake_ops import FakeOps
from helpers import SCAN_F_CAP, SCAN_MIN_REF
from helpers_gemm import (DWHH_BY_ID, DWHH_CASES, G16, G32, G128, G3264, G6416, GEMM_BY_ID, GEMM_CASES, GEMM_F, GEMM_FAMILIES, GEMM_SENTINEL, MULTI_BY_ID, MULTI_CASES,
                          NN, NT, STAGED_CASES, TN, TN_CASES, TN_NFULL, TN_PF, TNK, TNL, TT, UNREACHABLE, assert_multi_plan_matches_case, assert_plan_matches_case,
                          c_buffer, case_family, case_plan, check_exact, check_normal, coverage_reached, coverage_wanted, dwhh_case_plan, dwhh_operands, dwhh_plan,
                          dwhh_problem, gemm_instance, gemm_problem, k_ranges, make_problem, multi_case_plan, multi_plan, multi_problems, old_metric_accepts,
                          restate32, slab_reduction, split_ranges)

IDS = [c["id"] for c in GEMM_CASES]
MODES = ("exact", "normal")


def _filled(prob, out, c0=0, ldc=None):
    buf = c_buffer(prob, c0, prob["N"] + c0 + 4 if ldc is None else ldc)
    buf[:prob["M"], c0:c0 + prob["N"]] = out.float()
    return buf


# ---- the mirror and the tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_gemm_case_reaches_what_its_id_names(cid):
    case = GEMM_BY_ID[cid]
    plan = case_plan(case)
    assert_plan_matches_case(case, plan)
    fam = case_family(case)
    assert cid.startswith({"staged": "s-", "tn": "t-", "tn-lean": "tl-"}[fam]) and plan["family"] == fam
    assert case["ldc"] > case["N"] and case["K"] <= 4104                    # C is a view with ldc > N; exactness needs 64 K < 2^24 by a wide margin
    if fam == "staged":
        BM, BN, BK = [int(x) for x in plan["kernel"].split("<")[1].rstrip(">").split(",")]
        assert "s-%dx%dx%d-" % (BM, BN, BK) in cid and "-%dx%dx%d" % (case["M"], case["N"], case["K"]) in cid
        if "-nk" in cid:
            assert int(cid.split("-nk")[1].split("-")[0]) == max(plan["nk"])
        if "-split" in cid:
            assert int(cid.split("-split")[1].split("-")[0]) == case["splitk"] == plan["ranges"]
    else:
        assert (case["a_k"], case["b_k"]) == TN and case["lda"] % 4 == 0 and case["ldb"] % 4 == 0
        if "-nfull" in cid:
            nfull, r = int(cid.split("-nfull")[1].split("-")[0]), int(cid.split("-r")[1])
            PF = TN_PF[plan["kernel"]]
            assert plan["steps"] == [(nfull, r, nfull // PF * PF)] and case["K"] == 4 * nfull + r
        if "-split" in cid:
            assert int(cid.split("-split")[1].split("-")[0]) == case["splitk"] == plan["ranges"]
            assert plan["steps"][-1][0] * 4 + plan["steps"][-1][1] < plan["klen"]          # a short last range


def test_the_tables_reach_every_instance_load_path_and_reduction():
    want, got = coverage_wanted(), coverage_reached()
    assert want <= got, sorted(map(str, want - got))
    assert len(want) >= 50
    # the one combination that cannot be reached, by the dispatch itself: aligned TN operands never get to a staged instance
    assert list(UNREACHABLE) == [("staged", TN, "fast")]
    for M, N, K, sk in ((70, 50, 80, 1), (2048, 2048, 40, 1), (300, 200, 1376, 43), (64, 16, 128, 1), (4096, 4096, 128, 1)):
        assert gemm_instance(False, False, M, N, K, (M + 3) // 4 * 4, (N + 3) // 4 * 4, N + 4, (0, 0, 0, 0), sk, False)["kernel"] == TNK
    for c in STAGED_CASES:
        if (c["a_k"], c["b_k"]) == TN:
            assert case_plan(c)["loads"]["fast"] == 0 and (c["lda"] % 4 or c["ldb"] % 4 or c["a_off"] % 4 or c["b_off"] % 4)
    # nk in {1, 2, 3, 5} against the two-deep prefetch on both load paths of the default instance; 33 as a long chain
    nk = {(max(case_plan(c)["nk"]), c["loads"]) for c in STAGED_CASES if c["kernel"] == G16 and c["splitk"] == 1}
    assert {(n, p) for n in (1, 2, 3, 5) for p in (("fast",), ("checked",))} <= nk and (33, ("checked",)) in nk
    # every staged instance in each of its reasons
    assert {c["K"] for c in STAGED_CASES if c["kernel"] in (G32, G3264)} == {128, 160}
    assert {(c["M"], c["N"]) for c in STAGED_CASES if c["kernel"] == G6416} == {(m, n) for m in (64, 70) for n in (1, 3, 16)}
    assert {(2048, 2048, 40), (1930, 2040, 40)} <= {(c["M"], c["N"], c["K"]) for c in STAGED_CASES if c["kernel"] == G128}
    assert any(c["a_off"] % 4 for c in STAGED_CASES) and any(c["b_off"] % 4 for c in STAGED_CASES) and any(c["ldb"] % 4 for c in STAGED_CASES if c["b_k"])
    # alpha in {1, 0.5}, beta in {0, 2}, C views at a column offset
    assert {c["alpha"] for c in GEMM_CASES} == {1.0, 0.5} and {c["beta"] for c in GEMM_CASES} == {0.0, 2.0} and any(c["c0"] for c in GEMM_CASES)
    for fam in ("staged", "tn", "tn-lean"):
        assert {c["beta"] for c in GEMM_CASES if case_family(c) == fam} == {0.0, 2.0}
    assert set(GEMM_F) == set(GEMM_FAMILIES) == {"staged", "multi", "tn", "tn-lean", "dwhh"} and max(GEMM_F.values()) <= SCAN_F_CAP


def test_tn_cases_cover_every_pipeline_shape_grid_and_reduction():
    for kern, PF in TN_PF.items():
        assert TN_NFULL[kern] == (0, 1, PF - 1, PF, PF + 1, 2 * PF - 1, 2 * PF, 2 * PF + 1, 3 * PF)
        unsplit = {case_plan(c)["steps"][0][:2] for c in TN_CASES if c["kernel"] == kern and c["splitk"] == 1 and (c["M"], c["N"]) == (200, 130)}
        assert unsplit == {(nf, r) for nf in TN_NFULL[kern] for r in (0, 1, 3)} - {(0, 0)}
        shapes = {(c["M"], c["N"]) for c in TN_CASES if c["kernel"] == kern}
        assert {(200, 130), (342, 70), (5, 1)} <= shapes
        assert any(c["M"] == 342 and c["lda"] == 344 for c in TN_CASES if c["kernel"] == kern)
        grids = {(case_plan(c)["ranges"], case_plan(c)["grid"]) for c in TN_CASES if c["kernel"] == kern}
        assert {(4, "3d"), (42, "3d"), (8, "1d"), (16, "1d")} <= grids
    r4 = {case_plan(c)["ranges"] for c in TN_CASES if c["reduce"] == "slab_reduce4_kernel" and c["kernel"] == TNK}
    assert {2, 7, 8, 9, 16, 17} <= r4
    assert {c["reduce"] for c in TN_CASES if c["trips"] == 2} == {"slab_reduce4_kernel", "slab_reduce_kernel"}
    assert any(c["c0"] == 342 and c["reduce"] == "slab_reduce_kernel" and c["N"] % 4 == 0 and c["ldc"] % 4 == 0 for c in TN_CASES)


def test_mirror_on_single_conditions():
    ok = dict(a_k=True, b_k=True, M=70, N=50, K=80, lda=80, ldb=80, ldc=56, ptrs=(0, 0, 0, 0, 0), splitk=1, lean=False)
    p = gemm_instance(**ok)
    assert (p["kernel"], p["loads"], p["nk"], p["ranges"], p["reduce"]) == (G16, {"fast": 2, "checked": 0}, [5], 1, None)
    for k, v in (("ptrs", (4, 0, 0, 0, 0)), ("ptrs", (0, 8, 0, 0, 0)), ("lda", 82), ("ldb", 81), ("K", 75)):
        d = dict(ok, **{k: v})
        if k == "K":
            d.update(lda=76, ldb=76)
        assert gemm_instance(**d)["loads"]["fast"] == 0, (k, v)
    assert gemm_instance(**dict(ok, ptrs=(0, 0, 4, 8, 0)))["loads"]["fast"] == 2            # C and bias do not matter to the loads
    assert gemm_instance(**dict(ok, K=128, lda=128, ldb=128))["kernel"] == G3264
    assert gemm_instance(**dict(ok, K=128, lda=128, ldb=128, M=63))["kernel"] == G32
    assert gemm_instance(**dict(ok, K=128, lda=128, ldb=128, splitk=2))["kernel"] == G16
    assert gemm_instance(**dict(ok, K=96, lda=96, ldb=96))["kernel"] == G16
    assert gemm_instance(**dict(ok, N=16))["kernel"] == G6416 and gemm_instance(**dict(ok, N=16, M=63))["kernel"] == G16
    assert gemm_instance(**dict(ok, N=17))["kernel"] == G16 and gemm_instance(**dict(ok, N=16, b_k=False, ldb=16))["kernel"] == G16
    assert gemm_instance(**dict(ok, M=2048, N=2048, ldc=2048))["kernel"] == "gemm_nt_direct_kernel<4, 2>"
    assert gemm_instance(**dict(ok, M=2048, N=2048, ldc=2048, K=40, lda=40, ldb=40))["kernel"] == G128
    assert gemm_instance(**dict(ok, M=2048, N=1920, ldc=2048))["kernel"] == G16                # 240 tiles of 128
    assert gemm_instance(**dict(ok, M=300, N=200, ldc=204, splitk=43))["kernel"] == G128 and gemm_instance(**dict(ok, M=300, N=200, ldc=204, splitk=42))["kernel"] == G16
    # K ranges as the launchers recompute them
    assert split_ranges(4100, 8, 16) == (528, 8) and k_ranges(4100, 528)[-1] == (3696, 4100)
    assert split_ranges(16, 2, 16) == (16, 1) and split_ranges(37, 8, 4) == (8, 5) and split_ranges(1376, 43, 32) == (32, 43)
    # the reduction
    assert slab_reduction(1, 8, 8, 8, 0, 0, 0) == (None, 0)
    assert slab_reduction(2, 136, 72, 76, 0, 0, 0) == ("slab_reduce4_kernel", 1)
    for args in ((136, 70, 76, 0, 0, 0), (136, 72, 75, 0, 0, 0), (136, 72, 76, 4, 0, 0), (136, 72, 76, 0, 8, 0), (136, 72, 76, 0, 0, 4)):
        assert slab_reduction(2, *args)[0] == "slab_reduce_kernel", args
    assert slab_reduction(2, 2048, 1024, 1024, 0, 0, 0)[1] == 1 and slab_reduction(2, 2048, 1028, 1028, 0, 0, 0)[1] == 2
    # TN: alignment sends it to the TN kernels, anything else to the staged <false, false> instance
    tn = dict(a_k=False, b_k=False, M=200, N=130, K=37, lda=200, ldb=132, ldc=136, ptrs=(0, 0, 0, 0, 0), splitk=1, lean=False)
    assert gemm_instance(**tn)["kernel"] == TNK and gemm_instance(**dict(tn, lean=True))["kernel"] == TNL
    for k, v in (("lda", 202), ("ldb", 130), ("ptrs", (4, 0, 0, 0, 0)), ("ptrs", (0, 8, 0, 0, 0))):
        assert gemm_instance(**dict(tn, **{k: v}))["kernel"] == G16
    assert gemm_instance(**dict(tn, splitk=8, K=1031))["grid"] == "1d" and gemm_instance(**dict(tn, splitk=4, K=515))["grid"] == "3d"
    # fn_gru_dwhh_f32
    assert dwhh_plan(64, 37, (0, 0, 0, 0), 1, True)["launches"][0]["kernel"] == TNL and dwhh_plan(64, 37, (0, 0, 0, 0), 1, True)["launches"][0]["msplit"] == 128
    two = dwhh_plan(96, 37, (0, 0, 0, 0), 1, True)
    assert two["form"] == "two-products" and [l["kernel"] for l in two["launches"]] == [TNK, TNK]         # the lean flag is not carried on
    assert dwhh_plan(64, 37, (0, 4, 0, 0), 1, False)["form"] == "two-products"
    # fn_gemm_multi
    mp = multi_plan(False, False, [dict(M=130, N=70, segs=[(32, 132, 72, 0, 0)]), dict(M=7, N=3, segs=[(32, 8, 4, 0, 0)])])
    assert mp["grid"] == 6 and mp["jobs"][0]["segs"][0]["loads"] == {"fast": 2, "checked": 4} and mp["jobs"][1]["idle"] == 5


def test_dwhh_and_multi_tables():
    for c in DWHH_CASES:
        p = dwhh_case_plan(c)
        assert p["form"] == c["form"] and len(p["launches"]) == (1 if c["form"] == "one-launch" else 2)
        assert all(l["kernel"] == (TNL if c["lean"] and c["form"] == "one-launch" else TNK) for l in p["launches"])
    assert {(c["H"], c["rows"], c["splitk"], c["beta"], c["lean"]) for c in DWHH_CASES} == {
        (H, r, s, b, l) for H in (64, 128, 96) for r in (37, 1030) for s in (1, 4, 8) for b, l in ((0.0, False), (1.0, True))}
    assert dwhh_case_plan(DWHH_BY_ID["d-H128-one-launch-three-tiles-rows37-split1-beta0"])["launches"][0]["tiles"] == 3
    assert {dwhh_case_plan(c)["launches"][0]["grid"] for c in DWHH_CASES} == {"1d", "3d"}
    dgx, dghn, _, _ = dwhh_operands(DWHH_CASES[0], "exact")
    H = DWHH_CASES[0]["H"]
    assert int((dgx[:, 2 * H:] != dghn).sum()) > dghn.numel() // 2 and len(set(dgx[0, 2 * H:].tolist())) > 8
    for c in MULTI_CASES:
        assert_multi_plan_matches_case(c, multi_case_plan(c))
    assert {c["lay"] for c in MULTI_CASES} == {NT, NN, TT, TN}
    nk = {(s["nk"], p) for c in MULTI_CASES for j in multi_case_plan(c)["jobs"] for s in j["segs"] for p, n in s["loads"].items() if n}
    assert {(n, p) for n in (1, 2, 3, 4, 5) for p in ("fast", "checked")} <= nk
    assert {3, 16} <= {s[0] for c in MULTI_CASES for j in c["jobs"] for s in j["segs"]}
    assert any(len(j["segs"]) == 4 and j["beta"] == 1.0 and j["bias"] and {s[3] for s in j["segs"]} == {"fast", "checked"} for c in MULTI_CASES for j in c["jobs"])
    assert any(j["idle"] > 0 for c in MULTI_CASES for j in multi_case_plan(c)["jobs"])
    assert {len(c["jobs"]) for c in MULTI_CASES} >= {12, 13}
    assert any(c["lay"] == TN and (j["M"], j["N"]) == (130, 70) for c in MULTI_CASES for j in c["jobs"])
    assert any(s[1][0] and s[2][0] and j["c0"] for c in MULTI_CASES for j in c["jobs"] for s in j["segs"])


# ---- the restatement passes both passes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_gemm_restatement_passes(cid):
    case = GEMM_BY_ID[cid]
    for mode in MODES:
        prob = gemm_problem(case, mode)
        buf = _filled(prob, prob["fake32"], case["c0"], case["ldc"])
        if mode == "exact":
            assert check_exact(prob, buf, case["c0"]) == case["M"] * case["N"]
        else:
            assert 0.0 <= check_normal(prob, buf, case["c0"], F=1)[0] <= 1.0
        assert prob["den"].min() >= SCAN_MIN_REF and len(prob["chains"]) == case_plan(case)["ranges"]
    a, b = prob["pieces"][0]
    want = case["alpha"] * (a[0].double() @ b.double()) + (prob["bias"].double() if case["bias"] else 0.0) + case["beta"] * prob["C0"][0].double()
    assert float((prob["ref64"][0] - want).abs().max()) < 1e-10


@pytest.mark.parametrize("cid", [c["id"] for c in DWHH_CASES])
def test_dwhh_restatement_passes(cid):
    case = DWHH_BY_ID[cid]
    for mode in MODES:
        prob = dwhh_problem(case, mode)
        buf = _filled(prob, prob["fake32"], 0, case["H"])
        assert check_exact(prob, buf) if mode == "exact" else check_normal(prob, buf, F=1)[0] <= 1.0
    dgx, dghn, hp, W0 = dwhh_operands(case, "normal")
    H = case["H"]
    want = case["beta"] * W0.double() + torch.cat([dgx[:, :2 * H], dghn], 1).double().t() @ hp.double()
    assert float((prob["ref64"] - want).abs().max()) < 1e-10


@pytest.mark.parametrize("cid", [c["id"] for c in MULTI_CASES])
def test_multi_restatement_passes(cid):
    case = MULTI_BY_ID[cid]
    for mode in MODES:
        for j, prob in zip(case["jobs"], multi_problems(case, mode)):
            buf = _filled(prob, prob["fake32"], j["c0"], j["ldc"])
            assert check_exact(prob, buf, j["c0"]) if mode == "exact" else check_normal(prob, buf, j["c0"], F=1)[0] <= 1.0
            assert len(prob["chains"]) == 1 and len(prob["chains"][0]) == len(j["segs"])


@pytest.mark.parametrize("cid", ["s-64x64x16-nt-300x200x4100-split8-last-range-checked", "s-64x64x16-nt-7x3x513-ragged-nk33-checked",
                                 "t-200x130-K4104-split16-1d-scalar-reduce", "s-128x128x32-nt-2048x2048x40-nk2-checked", "t-200x130-K99-nfull24-r3"])
def test_fakeops_gemm_passes_against_the_sequential_restatement(cid):
    """e_ref comes from a restatement that adds K sequentially; a library matmul (FakeOps.gemm: blocked on most hosts, which flatters long chains) must not
    be the only thing that can meet the bound, nor fail it: it passes the same check.  A split launch is restated the way it runs - FakeOps.gemm per K range,
    the slabs added in order, then the epilogue; one matmul over all of K = 4100 is another algorithm (sequential on some hosts: 17 x the split sum's e_ref)."""
    case = GEMM_BY_ID[cid]
    prob = gemm_problem(case, "normal")
    a, b = prob["pieces"][0]
    if len(prob["chains"]) == 1:
        Cm = prob["C0"].clone()
        FakeOps().gemm(a, b, Cm, a_k=True, b_k=False, alpha=case["alpha"], beta=case["beta"], bias=prob["bias"])
    else:
        total = torch.zeros(case["M"], case["N"])
        for (_, _, k0, k1), in prob["chains"]:
            slab = torch.zeros(case["M"], case["N"])
            FakeOps().gemm(a[:, k0:k1], b[k0:k1], slab, a_k=True, b_k=False)
            total = total + slab
        Cm = case["alpha"] * total + prob["bias"] + case["beta"] * prob["C0"]
    assert Cm.dtype == torch.float32
    F = GEMM_F[case_family(case)]
    assert check_normal(prob, _filled(prob, Cm, case["c0"], case["ldc"]), case["c0"], F=F)[0] <= F


# ---- planted faults: each an edit of the restatement --------------------------------------------------------------------------------------------
SPLIT = "s-64x64x16-nt-300x200x4100-split8-last-range-checked"


def _rejected_by(prob, out=None, buf=None, c0=0):
    """which pass turns the edited result down ('exact' / 'normal' problems: the one pass that applies)"""
    buf = _filled(prob, out, c0) if buf is None else buf
    with pytest.raises(AssertionError):
        (check_exact if prob["mode"] == "exact" else check_normal)(prob, buf, c0)
    return True


def _restated(prob, chains=None, bias="same", C0=None):
    return restate32(prob["chains"] if chains is None else chains, prob["alpha"], prob["bias"] if isinstance(bias, str) else bias, prob["beta"],
                     prob["C0"] if C0 is None else C0, prob["M"], prob["N"])


@pytest.mark.parametrize("mode", MODES)
def test_faults_in_the_k_walk_are_rejected(mode):
    prob = gemm_problem(GEMM_BY_ID[SPLIT], mode)
    a, b = prob["pieces"][0]
    good = prob["fake32"]
    # 1. one k row dropped in one tile
    a2 = a.clone()
    a2[:, 2077] = 0.0
    out = good.clone()
    out[16:32, 32:48] = _restated(prob, [[(a2, b, k0, k1)] for (_, _, k0, k1), in prob["chains"]])[16:32, 32:48]
    assert int((out != good).sum()) > 200 and bool((out[:16] == good[:16]).all())
    assert _rejected_by(prob, out)
    # 2. the last K range dropped   3. a range added twice   4. bias added once per range
    assert _rejected_by(prob, _restated(prob, prob["chains"][:-1]))
    assert _rejected_by(prob, _restated(prob, prob["chains"] + [prob["chains"][3]]))
    assert _rejected_by(prob, _restated(prob, bias=prob["bias"] * len(prob["chains"])))
    # 5. beta C applied with the C of another row
    assert _rejected_by(prob, _restated(prob, C0=prob["C0"].roll(1, 0)))
    # 6. a 16 x 16 tile written transposed
    out = good.clone()
    out[48:64, 16:32] = good[48:64, 16:32].t()
    assert _rejected_by(prob, out)
    # 10. a NaN
    out = good.clone()
    out[299, 199] = float("nan")
    assert _rejected_by(prob, out)
    # the unedited restatement passes through the same helper's checks
    (check_exact if mode == "exact" else check_normal)(prob, _filled(prob, good))


@pytest.mark.parametrize("mode", MODES)
def test_fault_dghn_band_taken_from_dgx(mode):
    """7. rows [2H, 3H) of dW from dgx[:, 2H:] instead of dghn (the split-A source switch missed)"""
    for cid in ("d-H64-one-launch-msplit128-ragged-dghn-band-rows37-split1-beta0", "d-H128-one-launch-three-tiles-rows1030-split8-beta1-lean"):
        case = DWHH_BY_ID[cid]
        prob, wrong = dwhh_problem(case, mode), dwhh_problem(case, mode, band_from_dgx=True)
        H = case["H"]
        assert bool((wrong["fake32"][:2 * H] == prob["fake32"][:2 * H]).all())
        assert _rejected_by(prob, wrong["fake32"])


@pytest.mark.parametrize("mode", MODES)
def test_fault_last_column_window_shifted_instead_of_clamped(mode):
    """8. M = 342 = 4 x 85 + 2: the window of rows 340 .. 343 holds two valid columns and must be read where it is; moved back to 338 .. 341 it gives
    rows 340, 341 the operand columns 338, 339"""
    case = GEMM_BY_ID["t-342x70-lda344-K37-window-clamp"]
    prob = gemm_problem(case, mode)
    a, b = prob["pieces"][0]
    a2 = a.clone()
    a2[340:342] = a[338:340]
    out = _restated(prob, [[(a2, b, k0, k1)] for (_, _, k0, k1), in prob["chains"]])
    assert bool((out[:340] == prob["fake32"][:340]).all())
    assert _rejected_by(prob, out)


@pytest.mark.parametrize("mode", MODES)
def test_fault_a_write_outside_the_view(mode):
    """9. a column >= N, a row >= M, a column before the view"""
    case = GEMM_BY_ID["t-342x72-lda344-K95-split8-C-column-342-scalar-reduce"]
    prob = gemm_problem(case, mode)
    for r, c in ((5, case["c0"] + case["N"]), (case["M"], case["c0"]), (0, case["c0"] - 1), (case["M"] + 2, case["ldc"] - 1)):
        buf = _filled(prob, prob["fake32"], case["c0"], case["ldc"])
        buf[r, c] = 0.0
        with pytest.raises(AssertionError, match="outside"):
            (check_exact if mode == "exact" else check_normal)(prob, buf, case["c0"])
    buf = _filled(prob, prob["fake32"], case["c0"], case["ldc"])
    assert float(buf[0, 0]) == GEMM_SENTINEL and float(buf[case["M"], case["c0"]]) == GEMM_SENTINEL


def test_beta_zero_starts_from_nan_and_a_kept_nan_is_rejected():
    case = GEMM_BY_ID["s-64x64x16-nt-7x3x513-ragged-nk33-checked"]
    for mode in MODES:
        prob = gemm_problem(case, mode)
        buf = c_buffer(prob, case["c0"], case["ldc"])
        assert case["beta"] == 0.0 and bool(torch.isnan(buf[:7, :3]).all())
        assert _rejected_by(prob, buf=buf, c0=case["c0"])                 # an output that was never written, or read into the result


def test_what_the_whole_tensor_metric_accepts():
    """One k row missing from the products of one 16-row band whose values are small (rows of A at 1e-6 of the others: the gradient rows of units that
    hardly fire): 1e-5 of the WHOLE tensor's maximum, what test_gemm asks, accepts it; the per-tile bound does not."""
    case = GEMM_BY_ID[SPLIT]
    a, b = [t.clone() for t in gemm_problem(case, "normal")["pieces"][0]]
    a[16:32] *= 1e-6
    C0 = torch.zeros(case["M"], case["N"])
    chains = [[(a, b, k0, k1)] for k0, k1 in k_ranges(case["K"], case_plan(case)["klen"])]
    prob = make_problem("small-band", "normal", case["M"], case["N"], [(a, b)], chains, 1.0, 0.0, None, C0)
    a2 = a.clone()
    a2[:, 2077] = 0.0
    out = prob["fake32"].clone()
    out[16:32, 32:48] = restate32([[(a2, b, k0, k1)] for (_, _, k0, k1), in chains], 1.0, None, 0.0, C0, case["M"], case["N"])[16:32, 32:48]
    assert old_metric_accepts(out, prob["ref64"]) and old_metric_accepts(prob["fake32"], prob["ref64"])
    with pytest.raises(AssertionError, match=r"rows 16\.\., columns 32\.\..*; 1 of 247 tiles"):
        check_normal(prob, _filled(prob, out))
    check_normal(prob, _filled(prob, prob["fake32"]), F=1)
