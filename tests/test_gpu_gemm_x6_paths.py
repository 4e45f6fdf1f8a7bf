"""The bf16 x 6 GEMMs of csrc/gemm.hip - gemm_tn_x6_kernel, gemm_tn_x6w_kernel, gemm_tn_x6v_kernel (also behind fn_gru_dwhh_f32) and gemm_nt_x6w_kernel -
bit for bit on integers in four passes and per 16 x 16 tile against float64.

The cases, the operands of the passes, the restatement and the mirror are tests/helpers_gemm_x6.py and tests/helpers_gemm.py; tests/test_gemm_x6_reference.py
shows on the CPU that the table reaches what it claims, that the exact conditions and the placement of the wide values hold, that the restatement passes
and that planted faults are rejected.  Every launch here goes through the C ABI with the mode bits set explicitly (the wrapper picks the bf16 x 6 kernels
only from K = 1024 on), asserts through the mirror AND the library's plan, on the real addresses and the device's compute-unit count, that it reaches the
kernel, ranges, grid form, walk and reduction its id names, runs the five passes and prints its line of profiles/gemm_fp64_errors.txt.  Per case the
bit-identity claims of gemm.hip: the three TN kernels agree on K ranges of whole blocks, the two producer / consumer kernels agree with a K tail too,
walking agrees with one workgroup per item, a repeated launch agrees with the first."""
import ctypes as C

import pytest
import torch

from helpers_gemm import (assert_dwhh_mirror_matches_library, assert_mirror_matches_library, c_buffer, check, dwhh_plan, stored)
from helpers_gemm_x6 import (X6_DWHH_CASES, X6_F, X6_MODES, X6_NT_CASES, X6_TN_CASES, assert_x6_plan_matches_case, case_family, dwhh_tensors,
                             has_tail, x6_case_plan, x6_flags, x6_line, x6_problem)
from mfn_import import load_package
from test_gpu_gemm_paths import DEV, _ld, _p, _vec, _view

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    return HipOps(torch.device(DEV))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _lib_plan(ops, fn, *args):
    from music_fader_nets_amd import _lib
    if fn == "gemm":
        plan = _lib.FnGemmPlan()
        assert ops.lib.fn_gemm_plan(*args, 0, C.byref(plan)) == 0
        return plan.as_dict()
    n, plans = C.c_int32(), (_lib.FnGemmPlan * 2)()
    assert ops.lib.fn_gru_dwhh_plan(*args, 0, C.byref(n), plans) == 0
    return dict(form="one-launch" if n.value == 1 else "two-products", launches=[plans[i].as_dict() for i in range(n.value)])


def _run_gemm(ops, case, kern, prob, pertile=False):
    """one fn_gemm_f32 launch with the kernel's mode bits -> (C buffer on the CPU, the mirror's plan on the real addresses)"""
    M, N, K = case["M"], case["N"], case["K"]
    a, b = prob["pieces"][0]
    As, Bs = stored(case, a, b)
    A, Bm = _view(As, case["a_off"], case["lda"]), _view(Bs, case["b_off"], case["ldb"])
    bias = _vec(prob["bias"], case["bias_off"])
    cbuf = c_buffer(prob, case["c0"], case["ldc"], DEV)
    Cv = cbuf[:M, case["c0"]:case["c0"] + N]
    assert (_ld(A), _ld(Bm), _ld(Cv)) == (case["lda"], case["ldb"], case["ldc"])
    wsb = int(ops.lib.fn_gemm_ws_bytes(M, N, case["splitk"]))
    ws = ops.workspace(wsb, "gemm") if wsb else None
    flags = case["splitk"] | x6_flags(kern, pertile)
    plan = x6_case_plan(case, kern, (_p(A), _p(Bm), _p(Cv), _p(bias), _p(ws)), pertile, _cus())
    lp = _lib_plan(ops, "gemm", int(case["a_k"]), int(case["b_k"]), M, N, K, case["lda"], case["ldb"], case["ldc"], _p(A), _p(Bm), _p(Cv), _p(bias) or None,
                   _p(ws) or None, flags)
    assert_mirror_matches_library(plan, lp, M, N, case["id"])
    rc = ops.lib.fn_gemm_f32(int(case["a_k"]), int(case["b_k"]), M, N, K, case["alpha"], _p(A), case["lda"], _p(Bm), case["ldb"], case["beta"], _p(Cv),
                             case["ldc"], _p(bias) or None, flags, _p(ws) or None, wsb, ops.stream())
    assert rc == 0, (case["id"], kern, rc)
    torch.cuda.synchronize()
    return cbuf.cpu(), plan


def _run_dwhh(ops, case, kern, prob, pertile=False):
    H, rows = case["H"], case["rows"]
    dgx, dghn, hp = (_view(t, 0, t.shape[1]) for t in dwhh_tensors(case, prob))
    cbuf = c_buffer(prob, 0, H, DEV)
    dW = cbuf[:3 * H]
    wsb = int(ops.lib.fn_gru_dwhh_ws_bytes(H, case["splitk"]))
    ws = ops.workspace(wsb, "gemm") if wsb else None
    flags = case["splitk"] | x6_flags(kern, pertile)
    plan = dwhh_plan(H, rows, (_p(dgx), _p(dghn), _p(hp), _p(dW), _p(ws)), case["splitk"], False, x6_flags(kern, pertile), _cus())
    lp = _lib_plan(ops, "dwhh", _p(dgx), _p(dghn), _p(hp), _p(dW), _p(ws) or None, rows, H, flags)
    assert_dwhh_mirror_matches_library(plan, lp, H, case["id"])
    rc = ops.lib.fn_gru_dwhh_f32(_p(dgx), _p(dghn), _p(hp), rows, H, case["beta"], _p(dW), flags, _p(ws) or None, wsb, ops.stream())
    assert rc == 0, (case["id"], kern, rc)
    torch.cuda.synchronize()
    return cbuf.cpu(), plan


def _same(x, y):
    return torch.equal(x.view(torch.int32), y.view(torch.int32))


def _case(ops, case):
    """the five passes of one case on each of its kernels, the plan assertions and the bit-identity claims; prints one line per kernel"""
    run = _run_dwhh if case["kind"] == "dwhh" else _run_gemm
    c0 = case.get("c0", 0)
    worst, plans, nexact = {}, {}, {k: 0 for k in case["kernels"]}
    for mode in X6_MODES:
        bufs = {}
        for kern in case["kernels"]:
            prob = x6_problem(case, mode, perwave=kern == "perwave")
            cbuf, plan = run(ops, case, kern, prob)
            assert plan == x6_case_plan(case, kern, cus=_cus())            # the real addresses reach what the nominal layout does ...
            assert_x6_plan_matches_case(case, kern, plan, cus=_cus())      # ... which is what the id names
            res = check(prob, cbuf, c0, X6_F[case_family(case, kern)])
            if mode == "normal":
                worst[kern] = res
                again, _ = run(ops, case, kern, prob)
                assert _same(cbuf, again), "%s: %s: a repeated launch differs from the first" % (case["id"], kern)
            else:
                nexact[kern] += res
            bufs[kern], plans[kern] = cbuf, plan
            if case.get("pertile") and kern != "perwave":
                one, p1 = run(ops, case, kern, prob, pertile=True)
                assert_x6_plan_matches_case(case, kern, p1, pertile=True, cus=_cus())
                assert not (p1["launches"][0] if case["kind"] == "dwhh" else p1)["walks"]
                assert _same(cbuf, one), "%s: %s (%s): walking items and one workgroup per item differ" % (case["id"], kern, mode)
        agree = [k for k in case["kernels"] if k != "perwave" or not has_tail(case)]
        for k in agree[1:]:
            assert _same(bufs[agree[0]], bufs[k]), "%s (%s): %s and %s differ" % (case["id"], mode, agree[0], k)
    print()
    for kern in case["kernels"]:
        print(x6_line(case, kern, plans[kern], worst[kern], nexact[kern]))


@pytest.mark.parametrize("case", X6_TN_CASES, ids=[c["id"] for c in X6_TN_CASES])
def test_tn_bf16x6_exact_and_every_tile_vs_fp64(ops, case):
    """fn_gemm_f32 | FN_GEMM_BF16X6 on row-contiguous operands, in the per-wave, the 128 x 128 and the 128 x 256 kernel: one K range of 1 .. 13 whole blocks and
    partial last blocks on either side of every boundary of both trip schedules, ragged outputs, the column-window clamp, 3-D and 1-D grids, workgroups that
    walk items, both slab reductions, the epilogues: small, A3, B3, AB2 bit for bit, normals within X6_F x max(e_ref, 2**-23) in every tile"""
    _case(ops, case)


@pytest.mark.parametrize("case", X6_DWHH_CASES, ids=[c["id"] for c in X6_DWHH_CASES])
def test_gru_dwhh_bf16x6_exact_and_every_tile_vs_fp64(ops, case):
    """fn_gru_dwhh_f32 | FN_GEMM_BF16X6, default and per-wave: the two-source A operand (H = 64: the dghn band a ragged 64 rows of the second tile, H = 128),
    two products (H = 96), 1, 4 and 8 K ranges asked for, beta in {0, 1}; dgx carries other values in its unused columns [2H, 3H)"""
    _case(ops, case)


@pytest.mark.parametrize("case", X6_NT_CASES, ids=[c["id"] for c in X6_NT_CASES])
def test_nt_bf16x6_exact_and_every_tile_vs_fp64(ops, case):
    """gemm_nt_x6w_kernel at the threshold of 128 tiles with 4 .. 13 blocks (no steady pass .. three), and 288 tiles that workgroups walk, with padded leading
    dimensions, alpha / beta / bias, and FN_GEMM_X6_PERTILE for the same bits"""
    _case(ops, case)


def test_gru_dwhh_wrapper_picks_the_wide_kernel_on_twice_the_ranges(ops):
    """HipOps.gru_dwhh with the package's default arithmetic at H = 256, 32768 rows, 8 K ranges asked for: the wrapper's automatic choice - the 128 x 256 kernel
    on 16 ranges (the mirror with those bits == the library's plan of the wrapper's own arguments); small pass bit for bit, normals per tile"""
    from music_fader_nets_amd import _lib
    H, rows = 256, 32768
    case = dict(id="xd-H256-rows32768-split8-wrapper-wide", kind="dwhh", H=H, rows=rows, splitk=16, beta=1.0, form="one-launch", kernels=("256",), M=3 * H,
                N=H, K=rows, alpha=1.0, bias=False)
    assert ops.dw_x6 and ops.x6_wide is True and not ops.x6_perwave and not ops.x6_per_tile
    res = {}
    for mode in ("small", "normal"):
        prob = x6_problem(case, mode)
        dgx, dghn, hp = (t.to(DEV) for t in dwhh_tensors(case, prob))
        cbuf = c_buffer(prob, 0, H, DEV)
        dW = cbuf[:3 * H]
        lp = ops.gru_dwhh_plan(dgx, dghn, hp, dW, splitk=8)
        ws = ops.workspace(int(ops.lib.fn_gru_dwhh_ws_bytes(H, 16)), "gemm")
        plan = dwhh_plan(H, rows, (_p(dgx), _p(dghn), _p(hp), _p(dW), _p(ws)), 16, False, _lib.GEMM_BF16X6 | _lib.GEMM_X6_WIDE, _cus())
        assert_dwhh_mirror_matches_library(plan, lp, H, case["id"])
        p = plan["launches"][0]
        assert (p["kernel"], p["ranges"], p["klen"], p["grid_xyz"], p["msplit"]) == ("gemm_tn_x6v_kernel", 16, 2048, (6 * 16, 1, 1), 512), p
        ops.gru_dwhh(dgx, dghn, hp, dW, beta=1.0, splitk=8)
        torch.cuda.synchronize()
        res[mode] = check(prob, cbuf.cpu(), 0, X6_F["dwhh"])
    print()
    print(x6_line(case, "256", plan, res["normal"], res["small"], modes=("small",)))
