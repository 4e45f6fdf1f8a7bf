"""CPU self-test of the per-tile checker (helpers_head.check_head_vs_f64 / check_nt_vs_f64) that tests/test_gpu_head_paths.py applies to
out_head_kernel and gemm_nt_direct_kernel: the float32 restatement stands in for the kernel, on every GPU case's inputs.

It shows that the restatement passes its own check on every case and that the inputs satisfy the checker's input condition, that the shape
mirrors (head_path, nt_direct_instance) send every case to the K loop / kernel instance its id names and that together the cases reach every
loop shape, and that the checker rejects planted faults - one of which the whole-tensor metric of test_out_head_fused accepts.  The planted faults
are edits of CPU arrays.
"""
import numpy as np
import pytest
import torch

from helpers import SCAN_F_CAP, SCAN_MIN_REF
from helpers_gemm import lib_gemm_plan
from helpers_head import (HEAD_BY_ID, HEAD_CASES, HEAD_GRAD_SCALE, HEAD_SENTINEL, NT_BY_ID, NT_CASES, NT_ALPHA, NT_M, NT_N, check_head_vs_f64, check_nll_agree,
                          check_nt_vs_f64, head_buffers, head_case_path, head_fill_from, head_inputs, head_layout, head_path, head_reference, head_references,
                          head_tile_errors, nt_buffer, nt_case_instance, nt_direct_instance, nt_direct_steps, nt_layout, nt_references, old_metric_accepts,
                          tile_errors)

IDS = [c["id"] for c in HEAD_CASES]
NT_IDS = [c["id"] for c in NT_CASES]


def _restated(case, out=None):
    """buffers filled from the float32 restatement of a case (or from `out`)"""
    nll_buf, dl_buf = head_buffers(case)
    head_fill_from(case, head_references(case)["fake32"] if out is None else out, nll_buf, dl_buf)
    return nll_buf, dl_buf


def _fault_out(case, h=None, W=None, target=None):
    """the float32 restatement on edited inputs"""
    inp = head_inputs(case)
    nll, dl = head_reference(inp["h"] if h is None else h, inp["W"] if W is None else W, inp["bias"], inp["target"] if target is None else target,
                             case["B"], case["T"], HEAD_GRAD_SCALE, torch.float32)
    return {"nll": nll, "dlogits": dl}


# ---- the restatement passes, the inputs satisfy the condition -------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_restatement_passes_and_inputs_satisfy_the_condition(cid):
    """ratio <= 1 by construction; head_references asserts that every tile maximum of the float64 reference is >= 2**-100 - or, for the two kinds
    of case whose exact result is zero (V = 1, grad_scale = 0), that reference and restatement are exactly zero there"""
    case = HEAD_BY_ID[cid]
    ref = head_references(case)
    worst = check_head_vs_f64(case, *_restated(case), F=1)
    assert 0.0 <= worst[0] <= 1.0
    R, V = case["B"] * case["T"], case["V"]
    for k, den in ref["den"].items():
        assert den.shape == ((R + 15) // 16, (V + 15) // 16 if k == "dlogits" else 1)
        assert (den.max() == 0.0) if k in case["zero"] else (den.min() >= SCAN_MIN_REF)
    assert set(ref["ref64"]) == {"both": {"nll", "dlogits"}, "gs0": {"nll", "dlogits"}, "nll": {"nll"}, "dl": {"dlogits"}}[case["form"]]
    assert case["zero"] == (("dlogits", "nll") if V == 1 else ("dlogits",) if case["form"] == "gs0" else ())
    assert SCAN_F_CAP == 16


def test_reference_against_an_explicit_loop():
    """head_reference_f64 against the definition written out row by row (time-major rows, target at [b, t])"""
    case = HEAD_BY_ID["direct-rows-R33-B3"]
    inp, ref = head_inputs(case), head_references(case)["ref64"]
    B, T = case["B"], case["T"]
    for row in (0, 1, 2, 3, 17, 32):
        t, b = divmod(row, B)
        x = inp["h"][row].double() @ inp["W"].double().t() + inp["bias"].double()
        p = torch.exp(x - torch.logsumexp(x, 0))
        tg = int(inp["target"][b, t])
        want = HEAD_GRAD_SCALE * (p - torch.nn.functional.one_hot(torch.tensor(tg), case["V"]).double())
        assert abs(float(ref["nll"][row]) + float(torch.log(p[tg]))) < 1e-12
        assert float((ref["dlogits"][row] - want).abs().max()) < 1e-14


# ---- every case reaches the path its id names ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_head_case_reaches_its_path(cid):
    case = HEAD_BY_ID[cid]
    path, nks, nmain = head_case_path(case)
    assert path == case["path"] and cid.startswith({"direct": "direct-", "staged_checked": "checked-", "staged_fast": "fast-"}[path])
    if path == "direct":
        assert nks == case["H"] // 16 and nmain == nks // 2 * 2
        if "-nks" in cid:
            assert int(cid.split("-nks")[1].split("-")[0]) == nks
    else:
        assert nks is None and nmain is None
    assert case["V"] <= case["ld"] <= 384 and case["ld"] % 4 == 0


def test_head_cases_cover_every_loop_shape_and_edge():
    paths = {c["id"]: head_case_path(c) for c in HEAD_CASES}
    direct = {(nks, nmain) for p, nks, nmain in paths.values() if p == "direct"}
    assert {(1, 0), (2, 2), (3, 2), (4, 4), (5, 4), (7, 6), (33, 32)} <= direct
    #        ^ tail only   ^ zero steady iterations, without / with the tail      ^ steady iterations (nmain > 2) with an odd tail
    assert {"direct", "staged_fast", "staged_checked"} == {p for p, _, _ in paths.values()}
    # the four reasons for the checked loop
    chk = [c for c in HEAD_CASES if c["path"] == "staged_checked"]
    assert {75, 513} <= {c["H"] for c in chk} and {"off1", "ld66"} <= {c["h_view"] for c in chk}
    for c in chk:
        if c["h_view"] in ("off1", "ld66"):
            assert c["H"] % 16 == 0 and c["twin"]                               # only the pointer / the leading dimension keeps it off the direct loop
            assert head_path(0, c["H"], 0, c["H"], c["H"], c["B"] * c["T"], c["V"])[0] == "direct"        # ... which its dense twin takes
    # the fast loop: aligned, K % 16 == 0, span of exactly 2^30 elements
    (f,) = [c for c in HEAD_CASES if c["path"] == "staged_fast"]
    assert f["B"] * f["T"] * head_layout(f)[1] == 1 << 30 and (f["B"], f["T"], f["H"], f["V"]) == (256, 256, 32, 19)
    # rows, batch sizes, columns
    R = {c["B"] * c["T"] for c in HEAD_CASES}
    assert {1, 31, 33, 63, 64, 65, 4 * 64 + 1, 2 * 64 + 33} <= R and {1, 31, 33, 63, 0} <= {r % 64 for r in R}
    assert {1, 3, 5, 7} <= {c["B"] for c in HEAD_CASES}
    assert any(c["B"] in (3, 5, 7) and c["B"] * c["T"] > 64 and 64 % c["B"] for c in HEAD_CASES)
    cols = {(c["V"], c["ld"]) for c in HEAD_CASES}
    assert {(1, 4), (15, 16), (16, 16), (17, 20), (96, 96), (97, 100), (288, 288), (289, 292), (342, 344), (383, 384), (384, 384), (289, 384)} <= cols
    # forms on both loops
    assert {(c["path"], c["form"]) for c in HEAD_CASES} >= {(p, f) for p in ("direct", "staged_checked") for f in ("both", "nll", "dl", "gs0")}
    # targets pinned to the first and the last column
    for c in HEAD_CASES:
        t = head_inputs(c)["target"]
        assert int((t == 0).sum()) > 0 and (t.numel() == 1 or int((t == c["V"] - 1).sum()) > 0) and int(t.min()) >= 0 and int(t.max()) < c["V"]
    assert len(set(IDS)) == len(IDS)


def test_head_path_mirror_on_single_conditions():
    assert head_path(0, 64, 0, 64, 64, 161, 342) == ("direct", 4, 4)
    assert head_path(4, 64, 0, 64, 64, 161, 342)[0] == "staged_checked"          # pointer
    assert head_path(0, 64, 8, 64, 64, 161, 342)[0] == "staged_checked"
    assert head_path(0, 66, 0, 64, 64, 161, 342)[0] == "staged_checked"          # ld % 4
    assert head_path(0, 64, 0, 70, 64, 161, 342)[0] == "staged_checked"
    assert head_path(0, 76, 0, 76, 75, 161, 342)[0] == "staged_checked"          # K % 16
    assert head_path(0, 16384, 0, 32, 32, 65536, 19)[0] == "staged_fast"         # span of h
    assert head_path(0, 16384, 0, 32, 32, 65535, 19)[0] == "direct"
    assert head_path(0, 32, 0, 1 << 22, 32, 64, 256)[0] == "staged_fast"         # span of W


@pytest.mark.parametrize("cid", NT_IDS)
def test_nt_case_reaches_its_instance(cid):
    case = NT_BY_ID[cid]
    inst = nt_case_instance(case)
    assert inst == ("gemm_nt_direct_kernel<1, 4>" if case["lean"] else "gemm_nt_direct_kernel<4, 2>")
    nks, nmain, steady, rem = nt_direct_steps(case["K"], case["lean"])
    assert "-nks%d-steady%d-rem%d" % (nks, steady, rem) in cid and nks == case["K"] // 16
    lda, ldb, ldc = nt_layout(case)
    # the bf16 x 6 route would take the K % 32 == 0 cases if its flag were set: the calls switch it off
    assert nt_direct_instance(NT_M, NT_N, case["K"], lda, ldb, ldc, (0, 0, 0, 0), case["lean"], 1, x6=True) == (None if case["K"] % 32 == 0 and case["K"] >= 128 else inst)
    # ... and the library's own dispatch (fn_gemm_plan, 256 compute units) decides the same, with and without the bf16 x 6 bit: one workgroup per tile
    for x6 in (False, True):
        lp = lib_gemm_plan(True, True, NT_M, NT_N, case["K"], lda, ldb, ldc, (0, 0, 0, 0, 0), 1, case["lean"], x6)
        want = nt_direct_instance(NT_M, NT_N, case["K"], lda, ldb, ldc, (0, 0, 0, 0), case["lean"], 1, x6=x6)
        assert lp["kernel"] == ("gemm_nt_x6w_kernel" if want is None else want)
        assert (lp["klen"], lp["ranges"], lp["grid"], lp["tiles"], lp["reduce"], lp["reduce_blocks"], lp["msplit"]) == (case["K"], 1, (256, 1, 1), 256, None, 0, 0)


def test_nt_cases_cover_every_remainder_with_and_without_a_steady_iteration():
    pf4 = {nt_direct_steps(c["K"], False)[2:] for c in NT_CASES if not c["lean"]}
    assert {(s, r) for s in (0, 1) for r in (0, 1, 2, 3)} <= pf4
    lean = {nt_direct_steps(c["K"], True) for c in NT_CASES if c["lean"]}
    assert all(nmain == nks and rem == 0 and steady == nks - 1 for nks, nmain, steady, rem in lean) and {n for n, _, _, _ in lean} == set(range(4, 12))
    assert any(c["beta"] == 0.0 for c in NT_CASES) and any(c["views"] for c in NT_CASES)
    assert (NT_M // 128) * (NT_N // 128) == 256
    # single conditions of the dispatch
    ok = dict(M=2048, N=2048, K=80, lda=80, ldb=80, ldc=2048, ptrs=(0, 0, 0, 0), lean=False, splitk=1)
    assert nt_direct_instance(**ok) == "gemm_nt_direct_kernel<4, 2>"
    for k, v in (("M", 1920), ("K", 48), ("K", 72), ("lda", 82), ("ldc", 2050), ("ptrs", (0, 4, 0, 0)), ("ptrs", (0, 0, 0, 8)), ("splitk", 2), ("lda", 1 << 19)):
        assert nt_direct_instance(**dict(ok, **{k: v})) is None, (k, v)
        d = dict(ok, **{k: v})
        lp = lib_gemm_plan(True, True, d["M"], d["N"], d["K"], d["lda"], d["ldb"], d["ldc"], d["ptrs"] + (0,), d["splitk"], False)
        assert lp["kernel"].startswith("gemm_kernel<"), (k, v, lp)                 # the library sends each of them to a staged instance too
    assert nt_direct_instance(**dict(ok, a_k=False)) is None
    assert lib_gemm_plan(True, True, 2048, 2048, 80, 80, 80, 2048, (0, 0, 0, 0, 0), 1, False)["kernel"] == "gemm_nt_direct_kernel<4, 2>"


# ---- planted faults ------------------------------------------------------------------------------------------------------------------------
def _rejected(case, nll_buf, dl_buf, match):
    with pytest.raises(AssertionError, match=match):
        check_head_vs_f64(case, nll_buf, dl_buf)


def test_fault_1_one_tile_among_low_probability_columns_lacks_a_k_step():
    """one 16 x 16 dlogits tile (rows 16..31, columns 32..47: probabilities ~1e-8) computed from logits that lack the 16-k step k = 80..95.  The old
    metric - 1e-5 of the whole tensor's maximum, which is ~grad_scale in the target columns - accepts it; the per-tile bound does not."""
    case = HEAD_BY_ID["direct-nks33-lowprob-columns"]
    ref = head_references(case)
    inp = head_inputs(case)
    h = inp["h"].clone()
    h[:, 80:96] = 0.0
    out = {k: v.clone() for k, v in ref["fake32"].items()}
    out["dlogits"][16:32, 32:48] = _fault_out(case, h=h)["dlogits"][16:32, 32:48]
    assert float((out["dlogits"] - ref["fake32"]["dlogits"]).abs().max()) > 0.0
    assert old_metric_accepts(out["dlogits"], ref["ref64"]["dlogits"]) and old_metric_accepts(out["dlogits"], ref["fake32"]["dlogits"])
    assert old_metric_accepts(out["nll"], ref["ref64"]["nll"])
    _rejected(case, *_restated(case, out), match=r"dlogits: err .* \(rows 16\.\., columns 32\.\.\)")
    err = head_tile_errors(out, ref["ref64"])["dlogits"][0]
    assert int((err > SCAN_F_CAP * np.maximum(ref["e_ref"]["dlogits"], 2.0 ** -23)).sum()) == 1            # that tile and no other


@pytest.mark.parametrize("cid", ["direct-nks3-drain+tail", "direct-nks33-15steady+tail", "direct-nks1-tail-only"])
def test_fault_2_last_k_step_dropped_for_an_odd_step_count(cid):
    case = HEAD_BY_ID[cid]
    h = head_inputs(case)["h"].clone()
    h[:, -16:] = 0.0
    _rejected(case, *_restated(case, _fault_out(case, h=h)), match="over F")


def test_fault_3_targets_read_transposed_in_one_64_row_group():
    case = HEAD_BY_ID["direct-nks4-1steady"]
    B, T = case["B"], case["T"]
    tgt = head_inputs(case)["target"]
    flat = tgt.reshape(-1)
    wrong = tgt.clone()
    for rc in range(64, 128):                                   # row rc reads target.flat[(rc / B) B + rc % B] = [t, b] instead of [(rc % B) T + rc / B]
        wrong[rc % B, rc // B] = flat[rc]
    assert int((wrong != tgt).sum()) > 8
    good = head_references(case)["fake32"]
    bad = _fault_out(case, target=wrong)
    out = {k: v.clone() for k, v in good.items()}
    for k in out:
        out[k][64:128] = bad[k][64:128]
    _rejected(case, *_restated(case, out), match="over F")
    out = {"nll": out["nll"], "dlogits": good["dlogits"]}      # nll alone
    _rejected(case, *_restated(case, out), match="nll: err")


def test_fault_4_a_padding_column_is_not_zero():
    for cid in ("direct-nks4-1steady", "direct-cols-V289-ld384", "direct-cols-V1-ld4"):
        case = HEAD_BY_ID[cid]
        nll_buf, dl_buf = _restated(case)
        dl_buf[5, case["ld"] - 1] = 1e-30
        _rejected(case, nll_buf, dl_buf, match="padding column %d" % (case["ld"] - 1))
    case = HEAD_BY_ID["direct-nks4-1steady"]                    # and the rows past R
    nll_buf, dl_buf = _restated(case)
    dl_buf[case["B"] * case["T"], 0] = 0.0
    _rejected(case, nll_buf, dl_buf, match="rows >= R were written")
    nll_buf, dl_buf = _restated(case)
    nll_buf[case["B"] * case["T"]] = 0.0
    _rejected(case, nll_buf, dl_buf, match="nll rows >= R were written")


def test_fault_5_nll_of_the_last_row_left_at_its_sentinel():
    for cid in ("direct-rows-R65-B5", "direct-rows-R1-B1", "direct-form-nll", "direct-cols-V1-ld4"):
        case = HEAD_BY_ID[cid]
        nll_buf, dl_buf = _restated(case)
        nll_buf[case["B"] * case["T"] - 1] = HEAD_SENTINEL
        _rejected(case, nll_buf, dl_buf, match="nll: err")


def test_exact_zero_cases_reject_anything_but_zero():
    for cid, k in (("direct-form-gs0", "dlogits"), ("direct-cols-V1-ld4", "dlogits"), ("direct-cols-V1-ld4", "nll")):
        case = HEAD_BY_ID[cid]
        nll_buf, dl_buf = _restated(case)
        (dl_buf[3] if k == "dlogits" else nll_buf[3:4])[0] = 1e-38
        _rejected(case, nll_buf, dl_buf, match="%s: err" % k)
    case = HEAD_BY_ID["direct-form-gs0"]
    nll_buf, dl_buf = _restated(case)
    dl_buf[7, 11] = float("nan")
    _rejected(case, nll_buf, dl_buf, match="dlogits: err")


def test_missing_output_and_nan_are_rejected():
    case = HEAD_BY_ID["direct-nks4-1steady"]
    nll_buf, dl_buf = _restated(case)
    with pytest.raises(AssertionError, match="missing"):
        check_head_vs_f64(case, None, dl_buf)
    dl_buf[40, 100] = float("nan")
    _rejected(case, nll_buf, dl_buf, match=r"rows 32\.\., columns 96\.\.")


def test_nll_agreement_bound():
    case = HEAD_BY_ID["checked-ldh66"]
    nll = head_references(case)["fake32"]["nll"]
    assert check_nll_agree(case, nll, nll) == 0.0
    off = nll.clone()
    off[50] *= 1.0 + 1e-4
    with pytest.raises(AssertionError, match=r"rows 48\.\."):
        check_nll_agree(case, nll, off)


# ---- the GEMM ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted({c["key"] for c in NT_CASES}))
def test_nt_restatement_passes(key):
    case = [c for c in NT_CASES if c["key"] == key and not c["lean"]][-1]           # (the views case where a key has one)
    ref = nt_references(case)
    buf = nt_buffer(case, ref["C0"])
    buf[:NT_M, :NT_N] = ref["fake32"]
    assert 0.0 <= check_nt_vs_f64(case, buf, F=1)[0] <= 1.0
    assert ref["den"].shape == (NT_M // 16, NT_N // 16) and ref["den"].min() >= SCAN_MIN_REF
    row = ref["A"][5].double() @ ref["B"].double().t()
    want = NT_ALPHA * row + ref["bias"].double() + case["beta"] * ref["C0"][5].double()
    assert float((ref["ref64"][5] - want).abs().max()) < 1e-12


def test_fault_6_one_tile_of_c_lacks_the_beta_c_term():
    case = NT_BY_ID["nt-pf4-K80-nks5-steady0-rem1"]
    ref = nt_references(case)
    buf = nt_buffer(case, ref["C0"])
    buf[:NT_M, :NT_N] = ref["fake32"]
    buf[1024:1040, 48:64] -= case["beta"] * ref["C0"][1024:1040, 48:64]
    with pytest.raises(AssertionError, match=r"rows 1024\.\., columns 48\.\..*; 1 of 16384 tiles"):
        check_nt_vs_f64(case, buf)
    buf = nt_buffer(case, ref["C0"])
    buf[:NT_M, :NT_N] = ref["fake32"]
    buf[NT_M, 3] = 0.0
    with pytest.raises(AssertionError, match="outside"):
        check_nt_vs_f64(case, buf)
    e, _ = tile_errors(ref["fake32"], ref["ref64"])
    assert np.array_equal(e, ref["e_ref"])
