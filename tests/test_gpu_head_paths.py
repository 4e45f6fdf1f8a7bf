"""out_head_kernel (fn_out_head_f32) and gemm_nt_direct_kernel<PF, WGS> (fn_gemm_f32) on every K-loop path, per 16 x 16 tile against float64.

The shapes, the reference, the metric and the bound are tests/helpers_head.py; tests/test_head_reference.py shows on the CPU that the checker
accepts the float32 restatement and rejects planted faults.  Each case asserts that its operands reach the K loop / kernel instance it names
(the device-side / host-side conditions of csrc/gemm.hip restated on the real addresses; the host-side one also asked of the library, fn_gemm_plan) and prints its line of
profiles/out_head_fp64_errors.txt."""
import pytest
import torch

from helpers_head import (HEAD_CASES, NT_ALPHA, NT_CASES, NT_M, NT_N, SPAN_LD, check_head_vs_f64, check_nll_agree, check_nt_vs_f64, head_buffers, head_case_path,
                          head_grad_scale, head_layout, head_line, head_path, head_references, nt_buffer, nt_case_instance, nt_direct_instance, nt_layout, nt_line,
                          nt_references)
from mfn_import import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    return HipOps(torch.device(DEV))


def _x6_default():
    """what a kernel table starts with: the package default arithmetic"""
    from music_fader_nets_amd import arith
    return arith.default() == arith.BF16X6


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))          # as hipops._mat


def _h_view(case, h):
    """the case's view of h on the device; the allocation behind it is 16-byte aligned (asserted through head_layout)"""
    R, H = h.shape
    kind = case["h_view"]
    if kind == "dense":
        return h.to(DEV)
    if kind == "off1":
        flat = torch.zeros(R * H + 4, device=DEV)
        v = flat[1:1 + R * H].view(R, H)
    else:
        width, c0 = {"wide": (H + 16, 4), "ld66": (H + 2, 0), "span": (SPAN_LD, 0)}[kind]
        # span: 4 GiB, never initialised outside the view (the kernel reads columns [0, H) only); an allocation failure fails the case
        base = torch.empty(R, width, device=DEV) if kind == "span" else torch.full((R, width), float("nan"), device=DEV)
        v = base[:, c0:c0 + H]
    v.copy_(h)
    return v


def _w_view(case, W):
    if case["w_view"] == "dense":
        return W.to(DEV)
    V, H = W.shape
    v = torch.full((V, H + 4), float("nan"), device=DEV)[:, :H]
    v.copy_(W)
    return v


def _launch(ops, case, h, W, inp):
    nll_buf, dl_buf = head_buffers(case, DEV)
    R = case["B"] * case["T"]
    ops.out_head(h, W, inp["bias"].to(DEV), case["B"], case["T"], inp["target"].to(DEV), nll_rows=None if nll_buf is None else nll_buf[:R],
                 grad_scale=head_grad_scale(case), dlogits=None if dl_buf is None else dl_buf[:R])
    torch.cuda.synchronize()
    return (None if nll_buf is None else nll_buf.cpu()), (None if dl_buf is None else dl_buf.cpu())


@pytest.mark.parametrize("case", HEAD_CASES, ids=[c["id"] for c in HEAD_CASES])
def test_out_head_paths_every_tile_vs_fp64(ops, case):
    """fn_out_head_f32 on the LDS-free loop at every shape of its prologue / steady loop / drain / odd tail, on the staged loop with bounds-checked
    loads (K % 16 != 0, a misaligned pointer, ld % 4 != 0) and with unconditional loads (a 2^30-element span), at ragged row and column counts,
    with empty column groups, strided operand views and every output form: nll and dlogits within SCAN_F_CAP x max(e_ref, 2**-23) of the float64
    head in every 16 x 16 tile, padding columns exactly zero, nothing written past R rows (helpers_head.check_head_vs_f64)."""
    ref = head_references(case)
    inp = ref["inputs"]
    R, V, H = case["B"] * case["T"], case["V"], case["H"]
    h, W = _h_view(case, inp["h"]), _w_view(case, inp["W"])
    off_h, ldh, off_w, ldw = head_layout(case)
    assert (h.data_ptr() % 16, _ld(h), W.data_ptr() % 16, _ld(W)) == (off_h % 16, ldh, off_w % 16, ldw)
    path = head_path(h.data_ptr(), _ld(h), W.data_ptr(), _ld(W), H, R, V)
    assert path == head_case_path(case) and path[0] == case["path"], (path, case["path"])      # the operands reach the loop the case is for
    nll, dl = _launch(ops, case, h, W, inp)
    worst = check_head_vs_f64(case, nll, dl)
    print()
    print(head_line(case, path, worst))
    if case["twin"]:
        hd = inp["h"].to(DEV)
        assert head_path(hd.data_ptr(), _ld(hd), W.data_ptr(), _ld(W), H, R, V)[0] == "direct"
        nll_d, dl_d = _launch(ops, case, hd, W, inp)
        check_head_vs_f64(case, nll_d, dl_d)
        r = check_nll_agree(case, nll[:R], nll_d[:R])          # the staged and the LDS-free loop on the same values: within the bound, not bit-equal by contract
        print("%-34s nll vs the direct loop: %.3f x max(e_ref, 2**-23)" % (case["id"], r))


@pytest.mark.parametrize("case", NT_CASES, ids=[c["id"] for c in NT_CASES])
def test_gemm_nt_direct_every_tile_vs_fp64(ops, case):
    """gemm_nt_direct_kernel<4, 2> and the lean <1, 4> (the layer-2 projection of the fp32 leg) at 4..11 steps of 16 k: every remainder of the
    ring depth without and with a steady iteration, alpha, beta C and a bias, beta = 0, lda / ldc views; the bf16 x 6 NT route off."""
    ref = nt_references(case)
    K = case["K"]
    lda, ldb, ldc = nt_layout(case)
    A = torch.full((NT_M, lda), float("nan"), device=DEV)[:, :K]
    A.copy_(ref["A"])
    Bm, bias = ref["B"].to(DEV), ref["bias"].to(DEV)
    cbuf = nt_buffer(case, ref["C0"], DEV)
    Cv = cbuf[:NT_M, :NT_N]
    assert (_ld(A), _ld(Bm), _ld(Cv)) == (lda, ldb, ldc)
    inst = nt_direct_instance(NT_M, NT_N, K, _ld(A), _ld(Bm), _ld(Cv), (A.data_ptr(), Bm.data_ptr(), Cv.data_ptr(), bias.data_ptr()), case["lean"], 1)
    assert inst is not None and inst == nt_case_instance(case)
    prev = ops.nt_x6
    try:
        ops.nt_x6 = False
        lp = ops.gemm_plan(A, Bm, Cv, a_k=True, b_k=True, bias=bias, lean=case["lean"], nt_x6=False)              # the library's own decision for these tensors
        assert (lp["kernel"], lp["klen"], lp["ranges"], lp["grid"], lp["tiles"], lp["reduce"]) == (inst, K, 1, (256, 1, 1), 256, None), lp
        ops.gemm(A, Bm, Cv, a_k=True, b_k=True, alpha=NT_ALPHA, beta=case["beta"], bias=bias, lean=case["lean"], nt_x6=False)
        torch.cuda.synchronize()
    finally:
        ops.nt_x6 = prev
    assert ops.nt_x6 == prev and ops.dw_x6 == _x6_default()           # the table is as it was found
    worst = check_nt_vs_f64(case, cbuf.cpu())
    print()
    print(nt_line(case, inst, worst))
