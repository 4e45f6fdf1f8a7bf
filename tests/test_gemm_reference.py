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
                          NN, NT, PLAN_CUS, STAGED, STAGED_CASES, TN, TN_CASES, TN_NFULL, TN_PF, TNK, TNL, TT, UNREACHABLE, _lib, assert_dwhh_mirror_matches_library,
                          assert_mirror_matches_library, assert_multi_plan_matches_case, assert_plan_matches_case, c_buffer, case_family, case_plan, check_exact,
                          check_normal, coverage_reached, coverage_wanted, dwhh_case_plan, dwhh_operands, dwhh_plan, dwhh_problem, gemm_instance, gemm_problem,
                          k_ranges, lib_dwhh_plan, lib_gemm_plan, make_problem, multi_case_plan, multi_plan, multi_problems, old_metric_accepts, restate32,
                          slab_reduction, split_ranges)

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


# ---- the mirror against the library's own plan (fn_gemm_plan / fn_gru_dwhh_plan: pure host functions, no device) ------------------------------
def test_plan_kernel_names_follow_the_header_enum():
    import os
    import re
    from mfn_import import ROOT
    lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "fadernets.h")).read()
    body = hdr.split("enum FnGemmKernel {")[1].split("};")[0]
    names = re.findall(r"^\s*(FN_PLAN_[A-Z0-9_]+)", body, re.M)
    assert names[-1] == "FN_PLAN_KERNELS" and len(names) - 1 == len(lib.GEMM_PLAN_KERNELS) == 13

    def kernel_name(n):
        n = n[len("FN_PLAN_"):]
        if n.startswith("STAGED_"):
            return "gemm_kernel<%s>" % n[len("STAGED_"):].replace("_", ",")
        if n.startswith("NT_DIRECT_"):
            return "gemm_nt_direct_kernel<%s>" % n[len("NT_DIRECT_"):].replace("_", ", ")
        return "gemm_%s_kernel" % n.lower()
    assert tuple(kernel_name(n) for n in names[:-1]) == lib.GEMM_PLAN_KERNELS
    assert set(STAGED) | set(TN_PF) <= set(lib.GEMM_PLAN_KERNELS) and lib.GEMM_PLAN_REDUCES == (None, "slab_reduce_kernel", "slab_reduce4_kernel")
    src = open(os.path.join(ROOT, "music-fader-nets_amd", "csrc", "gemm.hip")).read()
    for k in lib.GEMM_PLAN_KERNELS:                          # every name is a kernel of gemm.hip
        assert re.search(r"\b%s\b" % k.split("<")[0], src), k
    import ctypes
    plan = lib.FnGemmPlan()
    fn = lib.load().fn_gemm_plan
    assert fn(1, 1, 8, 8, 8, 8, 8, 8, 0, 0, 0, 0, 0, 1, PLAN_CUS, None) == lib.FN_E_NULL
    for bad in (dict(M=0), dict(K=0), dict(lda=0), dict(ldc=7), dict(cus=-1)):
        a = dict(dict(M=8, N=8, K=8, lda=8, ldb=8, ldc=8, cus=PLAN_CUS), **bad)
        assert fn(1, 1, a["M"], a["N"], a["K"], a["lda"], a["ldb"], a["ldc"], 0, 0, 0, 0, 0, 1, a["cus"], ctypes.byref(plan)) == lib.FN_E_SHAPE, bad
    n, plans = ctypes.c_int32(), (lib.FnGemmPlan * 2)()
    dw = lib.load().fn_gru_dwhh_plan
    assert dw(0, 0, 0, 0, 0, 37, 64, 1, PLAN_CUS, None, plans) == lib.FN_E_NULL and dw(0, 0, 0, 0, 0, 37, 64, 1, PLAN_CUS, ctypes.byref(n), None) == lib.FN_E_NULL
    assert dw(0, 0, 0, 0, 0, 0, 64, 1, PLAN_CUS, ctypes.byref(n), plans) == lib.FN_E_SHAPE and dw(0, 0, 0, 0, 0, 1 << 31, 64, 1, PLAN_CUS, ctypes.byref(n), plans) == lib.FN_E_SHAPE
    assert dw(0, 0, 0, 0, 0, 37, 0, 1, PLAN_CUS, ctypes.byref(n), plans) == lib.FN_E_SHAPE and dw(0, 0, 0, 0, 0, 37, 64, 1, -1, ctypes.byref(n), plans) == lib.FN_E_SHAPE


def test_mirror_matches_the_library_on_every_case():
    """every case of GEMM_CASES and DWHH_CASES on its nominal addresses, 256 compute units: the mirror's kernel, klen, ranges, grid, reduction and tiles are
    what the library's dispatch decides (the lean cases also without the lean bit, as the GPU test runs them)"""
    for c in GEMM_CASES:
        ptrs = (4 * c["a_off"], 4 * c["b_off"], 4 * c["c0"], 4 * c["bias_off"] if c["bias"] else 0, 0)
        for lean in {c["lean"], False}:
            mp = gemm_instance(c["a_k"], c["b_k"], c["M"], c["N"], c["K"], c["lda"], c["ldb"], c["ldc"], ptrs, c["splitk"], lean)
            lp = lib_gemm_plan(c["a_k"], c["b_k"], c["M"], c["N"], c["K"], c["lda"], c["ldb"], c["ldc"], ptrs, c["splitk"], lean)
            assert_mirror_matches_library(mp, lp, c["M"], c["N"], c["id"])
            assert lp["kernel"] == (c["kernel"] if lean == c["lean"] else TNK)
    for c in DWHH_CASES:
        mp, lp = dwhh_case_plan(c), lib_dwhh_plan(c["H"], c["rows"], (0, 0, 0, 0, 0), c["splitk"], c["lean"])
        assert_dwhh_mirror_matches_library(mp, lp, c["H"], c["id"])
        assert lp["form"] == c["form"] and [l["msplit"] for l in lp["launches"]] == ([2 * c["H"]] if c["form"] == "one-launch" else [0, 0])


def test_mirror_matches_the_library_on_a_seeded_sweep():
    """4000 random calls - all four layouts, M and N in 1 .. 600, K in 1 .. 4096, leading dimensions with and without % 4, addresses on and off 16-byte
    boundaries, 1 / 2 / 3 / 8 / 12 / 16 K ranges asked for, lean and the bf16 x 6 bit on and off - and 300 of whole 128-tiles up to 4096 x 4096 (the
    LDS-free and the bf16 x 6 NT kernels take nothing smaller), then 1000 fn_gru_dwhh_f32 calls: mirror == library in every one"""
    import random
    rnd = random.Random(20261020)
    seen = set()
    for i in range(4300):
        a_k, b_k = rnd.random() < 0.5, rnd.random() < 0.5
        if i < 4000:
            M, N, K, splitk = rnd.randint(1, 600), rnd.randint(1, 600), rnd.randint(1, 4096), rnd.choice((1, 2, 3, 8, 12, 16))
        else:
            a_k, b_k = (True, True) if rnd.random() < 0.8 else (a_k, b_k)
            M, N, K, splitk = 128 * rnd.choice((8, 15, 16, 32)), 128 * rnd.choice((8, 15, 16, 32)), 16 * rnd.randint(1, 12), rnd.choice((1, 1, 1, 2))
        lda, ldb, ldc = (K if a_k else M) + rnd.choice((0, 0, 1, 2, 4, 8)), (K if b_k else N) + rnd.choice((0, 0, 1, 2, 4, 8)), N + rnd.choice((0, 0, 1, 2, 4, 8))
        off = lambda: rnd.choice((0, 0, 0, 4, 8, 16))                                                                    # noqa: E731
        ptrs = (1 << 20 | off(), 2 << 20 | off(), 3 << 20 | off(), (4 << 20 | off()) if rnd.random() < 0.7 else 0, 5 << 20 | off())
        lean, x6 = rnd.random() < 0.5, rnd.random() < 0.3
        mp = gemm_instance(a_k, b_k, M, N, K, lda, ldb, ldc, ptrs, splitk, lean, x6)
        lp = lib_gemm_plan(a_k, b_k, M, N, K, lda, ldb, ldc, ptrs, splitk, lean, x6)
        assert_mirror_matches_library(mp, lp, M, N, (i, a_k, b_k, M, N, K, lda, ldb, ldc, ptrs, splitk, lean, x6))
        seen.add((lp["kernel"], lp["reduce"]))
    assert {k for k, _ in seen} == set(_lib().GEMM_PLAN_KERNELS) - {"gemm_tn_x6_kernel", "gemm_tn_x6v_kernel"}, sorted(seen, key=str)     # (those two: by flag only)
    assert {r for _, r in seen} == {None, "slab_reduce_kernel", "slab_reduce4_kernel"}
    forms = set()
    for i in range(1000):
        H, rows, splitk, lean = rnd.choice((4, 30, 32, 64, 96, 100, 128, 192, 256, rnd.randint(1, 300))), rnd.randint(1, 5000), rnd.choice((1, 2, 3, 8, 12, 16)), rnd.random() < 0.5
        ptrs = tuple((j + 1) << 24 | rnd.choice((0, 0, 0, 4, 8, 16)) for j in range(5))
        mp, lp = dwhh_plan(H, rows, ptrs, splitk, lean), lib_dwhh_plan(H, rows, ptrs, splitk, lean)
        assert_dwhh_mirror_matches_library(mp, lp, H, (i, H, rows, ptrs, splitk, lean))
        forms.add((lp["form"],) + tuple(l["kernel"] for l in lp["launches"]))
    assert {f[0] for f in forms} == {"one-launch", "two-products"} and ("two-products", TNK, G16) in forms and not any(TNL in f[1:] for f in forms if f[0] == "two-products")


X6W, X6V, X6P, NTX6 = "gemm_tn_x6w_kernel", "gemm_tn_x6v_kernel", "gemm_tn_x6_kernel", "gemm_nt_x6w_kernel"


def test_bf16x6_plans_are_what_the_launchers_computed():
    """Literal expectations for the bf16 x 6 launches, worked out by hand from launch_tn / launch_tn_x6 / fn_gemm_f32 as they stood before the plan
    existed (the mirror restates these launches too: x6_tn_plan / x6_nt_plan, checked against the library in test_gemm_x6_reference.py).  TN, 1536 x 512 x 65536 (48 tiles of 128 x 128, 24 of 128 x 256): 16 ranges asked for -> klen =
    ceil(4096 / 32) 32 = 4096, 16 ranges, a 1-D grid of 48 x 16 = 768 items that one workgroup per compute unit walks (256) - unless FN_GEMM_X6_PERTILE, the
    per-wave kernel, or 250 compute units (not a multiple of the 8 XCDs); 12 ranges -> klen = ceil(5462 / 32) 32 = 5472, 12 ranges, not a multiple of 8:
    48 x 1 x 12; no split: 48 x 1 x 1 and no reduction.  The reduction of 1536 x 512 aligned floats: float4, 196608 / 256 = 768 blocks.
    NT: 128 tiles at 2048 x 1024 (the least the kernel takes) - 128 workgroups; 256 at 4096 x 1024, not above 256 compute units - 256; 512 at 8192 x 1024 -
    256 walking; misaligned, or 64 tiles, or K % 32 != 0: whatever the fp32 chain picks."""
    lib = _lib()
    X6, WIDE, PERTILE, PERWAVE = lib.GEMM_BF16X6, lib.GEMM_X6_WIDE, lib.GEMM_X6_PERTILE, lib.GEMM_X6_PERWAVE
    R4 = ("slab_reduce4_kernel", 768)

    def tn(flags, splitk, cus=256, M=1536, N=512, K=65536):
        p = lib_gemm_plan(False, False, M, N, K, (M + 3) // 4 * 4, (N + 3) // 4 * 4, N, (0, 0, 0, 0, 0), splitk, False, flags, cus)
        return p["kernel"], p["klen"], p["ranges"], p["grid"], p["tiles"], (p["reduce"], p["reduce_blocks"]), p["msplit"]

    assert tn(X6, 16) == (X6W, 4096, 16, (256, 1, 1), 48, R4, 0)
    assert tn(X6 | PERTILE, 16) == (X6W, 4096, 16, (768, 1, 1), 48, R4, 0)
    assert tn(X6 | WIDE, 16) == (X6V, 4096, 16, (256, 1, 1), 24, R4, 0)
    assert tn(X6 | WIDE | PERTILE, 16) == (X6V, 4096, 16, (384, 1, 1), 24, R4, 0)
    assert tn(X6 | PERWAVE, 16) == (X6P, 4096, 16, (768, 1, 1), 48, R4, 0)
    assert tn(X6 | PERWAVE | WIDE, 16) == (X6P, 4096, 16, (768, 1, 1), 48, R4, 0)            # the per-wave kernel has no wide form
    assert tn(X6, 16, cus=250) == (X6W, 4096, 16, (768, 1, 1), 48, R4, 0)
    assert tn(X6 | WIDE, 16, cus=250) == (X6V, 4096, 16, (384, 1, 1), 24, R4, 0)
    assert tn(X6, 16, cus=1024) == (X6W, 4096, 16, (768, 1, 1), 48, R4, 0)                   # fewer items than compute units: one workgroup per item
    assert tn(X6, 12) == (X6W, 5472, 12, (48, 1, 12), 48, R4, 0)
    assert tn(X6 | WIDE, 12) == (X6V, 5472, 12, (24, 1, 12), 24, R4, 0)
    assert tn(X6, 1) == (X6W, 65536, 1, (48, 1, 1), 48, (None, 0), 0)
    assert tn(X6 | WIDE, 1) == (X6V, 65536, 1, (24, 1, 1), 24, (None, 0), 0)
    assert tn(X6, 32) == (X6W, 2048, 32, (256, 1, 1), 48, R4, 0)
    # K ranges of whole 32-k blocks: K = 4100 over 16 -> ceil(257 / 32) 32 = 288 rows, 15 ranges (3-D); the fp32 kernel: 260 rows, 16 ranges (1-D)
    assert tn(X6, 16, K=4100)[1:5] == (288, 15, (48, 1, 15), 48) and tn(0, 16, K=4100)[:5] == (TNK, 260, 16, (768, 1, 1), 48)
    assert tn(X6 | lib.GEMM_LEAN, 16)[0] == X6W and tn(lib.GEMM_LEAN, 16)[:4] == (TNL, 4096, 16, (768, 1, 1))     # no walking form on the fp32 kernels
    # ragged 342 x 130: 3 x 2 tiles of 128 x 128, 3 x 1 of 128 x 256; N % 4 != 0: the scalar reduction, ceil(44460 / 256) = 174 blocks
    assert tn(X6, 8, M=342, N=130, K=8192) == (X6W, 1024, 8, (48, 1, 1), 6, ("slab_reduce_kernel", 174), 0)
    assert tn(X6 | WIDE, 8, M=342, N=130, K=8192) == (X6V, 1024, 8, (24, 1, 1), 3, ("slab_reduce_kernel", 174), 0)
    # fn_gru_dwhh_f32 at H = 512: the same launch with the dghn band from row 1024 on
    d = lib_dwhh_plan(512, 65536, (0, 0, 0, 0, 0), 16, False, X6)
    assert d["form"] == "one-launch" and d["launches"] == [dict(kernel=X6W, klen=4096, ranges=16, grid=(256, 1, 1), tiles=48, reduce=R4[0], reduce_blocks=768, msplit=1024)]
    d = lib_dwhh_plan(96, 4096, (0, 0, 0, 0, 0), 8, True, X6 | WIDE)                    # two products, 192 x 96 and 96 x 96: both on the wide kernel, 1 tile x 8 ranges
    assert d["form"] == "two-products" and [(l["kernel"], l["klen"], l["grid"], l["tiles"], l["msplit"]) for l in d["launches"]] == [
        (X6V, 512, (16, 1, 1), 2, 0), (X6V, 512, (8, 1, 1), 1, 0)]

    def nt(M, N, K, flags=X6, ptrs=(0, 0, 0, 0, 0), cus=256, lean=False):
        p = lib_gemm_plan(True, True, M, N, K, K, K, N, ptrs, 1, lean, flags, cus)
        assert (p["klen"], p["ranges"], p["reduce"], p["msplit"]) == (K, 1, None, 0)
        return p["kernel"], p["grid"], p["tiles"]

    assert nt(2048, 1024, 512) == (NTX6, (128, 1, 1), 128)
    assert nt(4096, 1024, 512) == (NTX6, (256, 1, 1), 256)
    assert nt(8192, 1024, 512) == (NTX6, (256, 1, 1), 512)
    assert nt(8192, 1024, 512, X6 | PERTILE) == (NTX6, (512, 1, 1), 512) and nt(8192, 1024, 512, cus=250) == (NTX6, (512, 1, 1), 512)
    assert nt(8192, 1024, 512, cus=304) == (NTX6, (304, 1, 1), 512)
    assert nt(2048, 1024, 512, lean=True)[0] == NTX6                                          # the lean bit is moot there
    for ptrs in ((4, 0, 0, 0, 0), (0, 8, 0, 0, 0), (0, 0, 4, 0, 0), (0, 0, 0, 4, 0)):        # misaligned: the fp32 chain - 128 big tiles, 512 of 64 x 64
        assert nt(2048, 1024, 512, ptrs=ptrs) == (G32, (512, 1, 1), 512), ptrs
    assert nt(1024, 1024, 512) == (G32, (256, 1, 1), 256)                                     # 64 tiles
    assert nt(1024, 1024, 512, 0) == (G32, (256, 1, 1), 256) and nt(2048, 1024, 512, 0) == (G32, (512, 1, 1), 512)      # and what the chain picks without the flag
    assert nt(4096, 1024, 80) == ("gemm_nt_direct_kernel<4, 2>", (256, 1, 1), 256)            # K % 32 != 0, 256 tiles: the LDS-free kernel
    assert nt(4096, 1024, 80, lean=True)[0] == "gemm_nt_direct_kernel<1, 4>" and nt(4096, 1024, 512, 0)[0] == "gemm_nt_direct_kernel<4, 2>"
    assert nt(2048, 1024, 80) == (G16, (512, 1, 1), 512)                                      # K % 32 != 0, 128 tiles
    assert nt(2048, 1024, 96)[0] == G16 and nt(2048, 1024, 128)[0] == NTX6                    # K >= 128


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
