"""Parity of the HIP path (through the C ABI) against the oracle / golden fixtures on a real MI355X.

Tolerances (fp32): kernel outputs vs the fp32 CPU restatement of the same op (tests/fake_ops.py) or fp64 torch: 2e-5 relative to the tensor's
max (backward scans 5e-5); the GRU scan kernels additionally at EVERY step and 32-row block against an fp64 scan + autograd, normalised by that
block of that step alone: err <= SCAN_F x max(the fp32 restatement's own error there, 2**-23) (helpers.check_scan_vs_f64);
end-to-end gradients vs the reference's autograd: 5e-4 relative to each tensor's max; greedy-decode token ids
bit-exact wherever the reference's own top-2 log-prob gap exceeds 1e-4 (a flipped near-tie changes every later token,
so rows are compared up to the first sub-threshold gap); past those near-ties, every step of every decode path against an fp64 replay
of its own tokens (helpers.replay_decode_check).  The large-batch GRU cells additionally per 16 x 16 tile of h_out against float64, on operand
views, K tails and exact piece passes, in tests/test_gpu_cell_paths.py.
"""
import math
import os

import numpy as np
import pytest
import torch

from fake_ops import FakeOps
from helpers import (NOISE_PARAMS, case_forward_only, case_kernel, ONE_LAUNCH_BLOCKS, REPLAY_CASES, REPLAY_GRAPH_PATHS, SCAN_CASES, PlanRecorder, _unblock_gates, _ws_scans, batch_of, check_scan_vs_f64, chosen_kernels,
                     grad_tolerances, load_golden,
                     make_model, oracle_grads_f64, relerr, replay_decode_check, replay_inputs, replay_line, replay_z, run_scans, scan_inputs, scan_kernel_names,
                     scan_lines, sd_from)
from mfn_import import load_package
from oracle import gmvae_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    return HipOps(torch.device(DEV))


@pytest.fixture(scope="module")
def small():
    return load_golden("small")


@pytest.fixture(scope="module")
def c0():
    return load_golden("c0")


def g(t):
    return None if t is None else t.to(DEV)


def _x6_default():
    """what a kernel table starts with (tests that switch ops.dw_x6 put it back): the package default arithmetic"""
    from music_fader_nets_amd import arith
    return arith.default() == arith.BF16X6


def close(a, b, tol=2e-5, msg=""):
    e = relerr(a.detach().cpu().numpy() if torch.is_tensor(a) else a, b.detach().cpu().numpy() if torch.is_tensor(b) else b)
    assert e < tol, "%s rel err %.3e" % (msg, e)


# ----------------------------------------------------------------------------------------------
# kernels one by one, against the documented semantics (tests/fake_ops.py) or fp64 torch
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a_k,b_k", [(True, True), (True, False), (False, False), (False, True)])
@pytest.mark.parametrize("M,N,K,splitk", [(64, 48, 32, 1), (256, 1536, 512, 1), (130, 342, 75, 1), (7, 3, 513, 1),
                                          (300, 200, 4100, 8), (1536, 512, 2048, 4), (1536, 512, 4104, 16), (136, 392, 1031, 24), (384, 128, 999, 42),
                                          (2048, 2048, 80, 1), (4096, 1024, 512, 1), (8192, 512, 48, 1),
                                          (16384, 3, 512, 1), (16384, 16, 512, 1), (200, 13, 70, 1)])      # (the last three: skinny outputs, 64 x 16 tiles)
def test_gemm(ops, a_k, b_k, M, N, K, splitk):
    torch.manual_seed(M * 7 + N * 3 + K)
    A = torch.randn((M, K) if a_k else (K, M))
    B = torch.randn((N, K) if b_k else (K, N))
    C0 = torch.randn(M, N)
    bias = torch.randn(N)
    ref = 0.5 * ((A if a_k else A.t()).double() @ (B.t() if b_k else B).double()) + 2.0 * C0.double() + bias.double()
    Cd = g(C0.clone())
    ops.gemm(g(A), g(B), Cd, a_k=a_k, b_k=b_k, alpha=0.5, beta=2.0, bias=g(bias), splitk=splitk)
    close(Cd, ref.float(), 1e-5, "gemm")


@pytest.mark.parametrize("M,N,K,splitk", [(1536, 512, 4099, 8), (342, 512, 2048, 4), (200, 130, 515, 1)])
def test_gemm_lean_instance(ops, M, N, K, splitk):
    """fn_gemm_f32 with splitk | FN_GEMM_LEAN (the <= 128-register weight-gradient instance that fits beside a scan wavefront): same k
    order, so the result is bit-identical to the default instance; also through fn_gru_dwhh_f32."""
    torch.manual_seed(M + K)
    A, B = g(torch.randn(K, M)), g(torch.randn(K, N))
    C0, C1 = torch.zeros(M, N, device=DEV), torch.zeros(M, N, device=DEV)
    ops.gemm(A, B, C0, a_k=False, b_k=False, splitk=splitk)
    ops.gemm(A, B, C1, a_k=False, b_k=False, splitk=splitk, lean=True)
    assert torch.equal(C0, C1)
    close(C1, (A.double().t() @ B.double()).float(), 1e-5, "lean gemm")
    if M == 1536:
        H = 512
        dgx, dghn, hp = g(torch.randn(K, 3 * H)), g(torch.randn(K, H)), g(torch.randn(K, H))
        W0, W1 = torch.zeros(3 * H, H, device=DEV), torch.zeros(3 * H, H, device=DEV)
        ops.gru_dwhh(dgx, dghn, hp, W0, splitk=splitk)
        ops.gru_dwhh(dgx, dghn, hp, W1, splitk=splitk, lean=True)
        assert torch.equal(W0, W1)


@pytest.mark.parametrize("B,T,H,V,ld", [(256, 8, 512, 342, 344), (5, 7, 64, 342, 344), (3, 4, 96, 19, 20), (64, 1, 512, 384, 384)])
def test_out_head_fused(ops, B, T, H, V, ld):
    """fn_out_head_f32 (projection + log-softmax + NLL + gradient seed in one kernel) against the unfused pair fn_gemm_f32 ->
    fn_vocab_logsoftmax and against fp64 torch; rows that do not fill a 64-row workgroup, padding columns, V = the tile width."""
    torch.manual_seed(B * 31 + T)
    h = g(torch.randn(T * B, H))
    W, bias = g(torch.randn(V, H) * 0.2), g(torch.randn(V))
    tgt = g(torch.randint(0, V, (B, T), dtype=torch.int32))
    logits = torch.zeros(T * B, ld, device=DEV)
    ops.gemm(h, W, logits[:, :V], bias=bias)
    nll0, nll1 = torch.zeros(T * B, device=DEV), torch.full((T * B,), -1.0, device=DEV)
    dl0 = torch.zeros(T * B, ld, device=DEV)
    ops.vocab_logsoftmax(logits, B, T, V, target=tgt, nll_rows=nll0, grad_scale=0.37, dlogits=dl0)
    dl1 = torch.full((T * B, ld), 7.0, device=DEV)
    ops.out_head(h, W, bias, B, T, tgt, nll_rows=nll1, grad_scale=0.37, dlogits=dl1)
    close(nll1, nll0, 1e-5, "fused nll vs unfused")            # (the fused head sums k in the LDS-free loop's order, the GEMM in the staged loop's)
    close(dl1[:, :V], dl0[:, :V], 1e-5, "fused dlogits vs unfused")
    assert float(dl1[:, V:].abs().max()) == 0.0 if ld > V else True
    ref = torch.log_softmax(h.double() @ W.double().t() + bias.double(), dim=-1).view(T, B, V)
    tg = tgt.long().t()
    close(nll1.view(T, B), -ref.gather(2, tg.unsqueeze(-1)).squeeze(-1).float(), 1e-5, "fused nll vs fp64")
    nll2 = torch.zeros(T * B, device=DEV)
    ops.out_head(h, W, bias, B, T, tgt, nll_rows=nll2)                       # evaluation form: no gradient seed
    assert torch.equal(nll1, nll2)


@pytest.mark.parametrize("variant", [0, 2, 8, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18])
@pytest.mark.parametrize("B,H,K1,mode", [(300, 64, 64, "dense"), (2048, 512, 512, "dense"), (130, 96, 0, "table"), (1030, 512, 0, "table0"), (77, 64, 48, "dense"), (700, 512, 0, "table")])
def test_gru_cell_dense(ops, B, H, K1, mode, variant):
    """fn_gru_cell_f32 (one GRUCell step of a large batch: a staged GEMM - variants 0-3 - or the LDS-free loop - variants 4-7 - with the gates
    in the epilogue) against tests/fake_ops.py (= torch nn.GRUCell semantics with the optional token-row / row-constant input parts), ragged
    row / unit tiles, K tails of the pipelined loop."""
    from fake_ops import FakeOps
    torch.manual_seed(B + H)
    V = 50
    hp = torch.randn(B, H) * 0.5
    whh, bhh, bih = torch.randn(3 * H, H) / H ** 0.5, torch.randn(3 * H) * 0.1, torch.randn(3 * H) * 0.1
    kw = dict(b_ih=bih)
    if mode == "dense":
        kw.update(x=torch.randn(B, K1), w_ih=torch.randn(3 * H, K1) / K1 ** 0.5)
    else:
        toks = torch.randint(0, V, (B, 7), dtype=torch.int32)
        kw.update(gx_table=torch.randn(V, 3 * H) * 0.3, gx_rowbias=torch.randn(B, 3 * H) * 0.3, start_token=V - 1,
                  idx=toks[:, 3] if mode == "table" else None)
    ref = torch.zeros(B, H)
    FakeOps().gru_cell(hp, whh, bhh, ref, **kw)
    out = torch.zeros(B, H, device=DEV)
    args = (g(hp), g(whh), g(bhh), out)
    dkw = dict({k: (g(v) if torch.is_tensor(v) and k != "idx" else v) for k, v in kw.items() if k != "idx"},
               idx=(g(toks)[:, 3] if mode == "table" else None) if mode != "dense" else None, variant=variant)
    ops.gru_cell(*args, **dkw)
    close(out, ref, 2e-5, "gru_cell")
    # the library's plan for the same descriptor: a forced form is honoured exactly where the hand rule says so, and the family that ran
    plan = ops.gru_cell_plan(*args, **dkw)
    if variant:
        assert plan["forced_honoured"] == (variant in (2, 8) or _cell_runs_forced_family(variant, H, K1)), plan
        assert plan["family"] == _cell_forced_family(variant) if plan["forced_honoured"] else (plan["family"], plan["template"]) == ("staged", (64, 2, 2)), plan
    else:               # automatic: the staged kernel up to 512 rows; above, at H = 512 and K1 in {0, 512}, the overlapped fill with ceil(B / 512) row tiles
        assert not plan["forced_honoured"]
        assert (plan["family"], plan["template"]) == (("staged", (64, 2, 2)) if B <= 512 else ("wlds-overlap", (-(-B // 512), 2, 0))), plan


# The K-loop tails and the four epilogue forms of the LDS-free and weight-slice cells at 70 rows (ragged against every row tile).  nks = K / 16 steps
# of a K phase against a ring of PF slots: dense K1 = 16 .. 272 at H = 32 gives nks = 1, 2, 3, 5, 9, 17 (fewer steps than slots, exactly one ring,
# ring + leftover, one steady pass, steady pass + odd leftover for PF up to 8); without a dense input the recurrent phase alone: H = 32, 96 = nks 2, 6.
# H = 272 (17 steps) is no multiple of 32: fn_gru_cell_f32 refuses it by its contract, whatever the variant, and the test pins that answer; H = 288
# (18 steps: two / four rings + two leftover steps for PF 8 / 4) is the nearest size the entry point takes.  The overlapped-fill cells (15-18) exist
# for H = 512, K1 in {0, 512} only.
CELL_TAIL_SHAPES = [(32, k1) for k1 in (16, 32, 48, 80, 144, 272)] + [(32, 0), (96, 0), (272, 0), (288, 0)]
CELL_TAIL_VARIANTS = (4, 5, 6, 7, 10, 12, 14)               # direct PF 1 / 4 / 2 / 2, wlds PF 4 / 8 / 2
CELL_OVL_SHAPES = [(512, 512), (512, 0)]
CELL_OVL_VARIANTS = (15, 16, 17, 18)
CELL_FORMS = ((False, False), (False, True), (True, True), (True, False))      # (token table, row constant): dense only, + row constant, table + row constant, table alone
CELL_TAIL_ROWS = 70


def _cell_runs_forced_family(variant, H, K1):
    """fn_gru_cell_f32's eligibility rules for a forced variant on contiguous 16-byte aligned fp32 operands (what torch allocates): the LDS-free
    cells 4-7 need H % 32 == 0 and K1 % 16 == 0; the weight-slice cells 9-14 also 48 max(K1, H) floats + four 16 x 20 tiles per wave within 160 KB of
    LDS; the overlapped-fill cells 15-18 H == 512 and K1 in {0, 512}.  Anything else runs the staged default; H % 32 != 0 is refused (FN_E_SHAPE)."""
    direct = H % 32 == 0 and K1 % 16 == 0
    if 4 <= variant <= 7:
        return direct
    if 9 <= variant <= 14:
        return direct and 48 * max(K1, H) * 4 + 4 * 4 * 320 * 4 <= 160 * 1024
    if 15 <= variant <= 18:
        return direct and H == 512 and K1 in (0, 512)
    return False


def _cell_forced_family(variant):
    """the kernel family a forced cell variant names"""
    return "staged" if variant in (1, 2, 3, 8) else "direct" if 4 <= variant <= 7 else "wlds" if 9 <= variant <= 14 else "wlds-overlap" if 15 <= variant <= 18 else None


_cell_tail_cache = {}


def _cell_tail_case(H, K1, tab, rb):
    key = (H, K1, tab, rb)
    if key not in _cell_tail_cache:
        B, V = CELL_TAIL_ROWS, 50
        gen = torch.Generator().manual_seed(1000 * H + K1)
        rn = lambda *s: torch.randn(*s, generator=gen)
        hp = rn(B, H) * 0.5
        whh, bhh, bih = rn(3 * H, H) / H ** 0.5, rn(3 * H) * 0.1, rn(3 * H) * 0.1
        kw = dict(b_ih=bih)
        if K1:
            kw.update(x=rn(B, K1), w_ih=rn(3 * H, K1) / K1 ** 0.5)
        toks = torch.randint(0, V, (B, 7), generator=gen, dtype=torch.int32)
        if tab:
            kw.update(gx_table=rn(V, 3 * H) * 0.3, idx=toks[:, 3])
        if rb:
            kw.update(gx_rowbias=rn(B, 3 * H) * 0.3)
        ref = torch.zeros(B, H)
        FakeOps().gru_cell(hp, whh, bhh, ref, **kw)
        dkw = {k: g(v) for k, v in kw.items() if k != "idx"}
        if tab:
            dkw["idx"] = g(toks)[:, 3]
        _cell_tail_cache[key] = (g(hp), g(whh), g(bhh), dkw, ref)
    return _cell_tail_cache[key]


def test_cell_tail_cases_run_the_forced_kernels():
    """more than half of the (shape, variant, form) cases below launch the kernel family their variant names (all of them, by the rules)"""
    cases = [(v, H, K1) for H, K1 in CELL_TAIL_SHAPES for v in CELL_TAIL_VARIANTS] + [(v, H, K1) for H, K1 in CELL_OVL_SHAPES for v in CELL_OVL_VARIANTS]
    forced = sum(_cell_runs_forced_family(*c) for c in cases)
    assert len(cases) == 10 * 7 + 2 * 4 and forced == len(cases) - 7 and 2 * forced > len(cases), (forced, len(cases))      # all but the refused H = 272
    # the hand rule against the library's plan (fn_gru_cell_plan: a pure host function) for all 78, on 16-byte aligned made-up addresses
    import ctypes
    from mfn_import import load_package
    load_package()
    from music_fader_nets_amd import _lib
    lib, A = _lib.load(), 0x10000
    for v, H, K1 in cases:
        c = _lib.FnGruCell(B=CELL_TAIL_ROWS, H=H, K1=K1, ldx=K1, ldw_ih=K1, ldh=H, ldw_hh=H, ldo=H, variant=v, h_prev=A, w_hh=A, b_hh=A, b_ih=A, h_out=2 * A)
        if K1:
            c.x = c.w_ih = A
        plan = _lib.FnGruCellPlan()
        assert lib.fn_gru_cell_plan(ctypes.byref(c), ctypes.byref(plan)) == 0
        if H % 32:
            assert plan.status == _lib.FN_E_SHAPE and not _cell_runs_forced_family(v, H, K1), (v, H, K1)
            continue
        p = plan.as_dict()
        assert p["status"] == 0 and p["forced_honoured"] == _cell_runs_forced_family(v, H, K1), (v, H, K1, p)
        assert p["family"] == (_cell_forced_family(v) if p["forced_honoured"] else "staged"), (v, H, K1, p)


@pytest.mark.parametrize("variant,H,K1", [(v, H, K1) for H, K1 in CELL_TAIL_SHAPES for v in CELL_TAIL_VARIANTS]
                         + [(v, H, K1) for H, K1 in CELL_OVL_SHAPES for v in CELL_OVL_VARIANTS])
def test_gru_cell_ring_tails_and_epilogue_forms(ops, variant, H, K1):
    """fn_gru_cell_f32, forced LDS-free (4-7), weight-slice (10, 12, 14) and overlapped-fill (15-18) cells at 70 rows: every K tail of the shared ring
    (CELL_TAIL_SHAPES) in the four input forms - dense only, dense + row constant, token table + row constant, token table alone; the second and the
    fourth are the HAS_TAB != HAS_RB instantiations - against tests/fake_ops.py at 2e-5, and a second launch bit for bit."""
    for tab, rb in CELL_FORMS:
        hp, whh, bhh, kw, ref = _cell_tail_case(H, K1, tab, rb)
        out = torch.zeros(2, CELL_TAIL_ROWS, H, device=DEV)
        if H % 32:
            with pytest.raises(RuntimeError, match="fn_gru_cell_f32 failed.*sizes"):
                ops.gru_cell(hp, whh, bhh, out[0], variant=variant, **kw)
            continue
        ops.gru_cell(hp, whh, bhh, out[0], variant=variant, **kw)
        ops.gru_cell(hp, whh, bhh, out[1], variant=variant, **kw)
        plan = ops.gru_cell_plan(hp, whh, bhh, out[0], variant=variant, **kw)
        assert plan["forced_honoured"] == _cell_runs_forced_family(variant, H, K1) and (plan["has_tab"], plan["has_rb"]) == (int(tab), int(rb)), plan
        assert plan["family"] == (_cell_forced_family(variant) if plan["forced_honoured"] else "staged"), plan
        close(out[0], ref, 2e-5, "gru_cell variant %d H %d K1 %d table %d row constant %d" % (variant, H, K1, tab, rb))
        assert torch.equal(out[0], out[1]), (variant, H, K1, tab, rb)


@pytest.mark.parametrize("B,H,K1,mode", [(2048, 512, 512, "dense"), (1024, 512, 0, "table"), (768, 512, 0, "table0"), (128, 64, 32, "dense"), (256, 96, 64, "dense"),
                                         (1280, 512, 512, "dense_rb")])
def test_gru_cell_bf16x6(ops, B, H, K1, mode):
    """gru_cell_x6_kernel (round 6; FnGruCell.variant | FN_GRU_BF16X6): one GRUCell step of a large batch on the bf16 MFMA with exact triple splits - producer / consumer
    form, [r | z | n_x | n_h] column tiles, gate epilogue on the producer wavefronts - against tests/fake_ops.py (torch nn.GRUCell semantics) at the fp32
    cells' tolerance and against the fp32 cell itself (agreement to fp32 rounding: the products are exact, the sums run in another order); dense input,
    token row + row bias, start token, both; repeated launches bit-identical; a shape it does not take (B % 128 != 0) falls back to the fp32 cells."""
    from fake_ops import FakeOps
    torch.manual_seed(B + H + K1)
    V = 50
    hp = torch.randn(B, H) * 0.5
    whh, bhh, bih = torch.randn(3 * H, H) / H ** 0.5, torch.randn(3 * H) * 0.1, torch.randn(3 * H) * 0.1
    kw = dict(b_ih=bih)
    toks = torch.randint(0, V, (B, 7), dtype=torch.int32)
    if mode.startswith("dense"):
        kw.update(x=torch.randn(B, K1), w_ih=torch.randn(3 * H, K1) / K1 ** 0.5)
        if mode == "dense_rb":
            kw.update(gx_rowbias=torch.randn(B, 3 * H) * 0.3)
    else:
        kw.update(gx_table=torch.randn(V, 3 * H) * 0.3, gx_rowbias=torch.randn(B, 3 * H) * 0.3, start_token=V - 1, idx=toks[:, 3] if mode == "table" else None)
    ref = torch.zeros(B, H)
    FakeOps().gru_cell(hp, whh, bhh, ref, **kw)
    dkw = {k: (g(v) if torch.is_tensor(v) and k != "idx" else v) for k, v in kw.items() if k != "idx"}
    dkw["idx"] = g(toks)[:, 3] if mode == "table" else None
    outs = {}
    try:
        for x6 in (False, True, True):
            ops.dw_x6, ops.cell_x6, ops.cell_x6_rows = x6, x6, 0
            out = torch.full((B, H), float("nan"), device=DEV)
            ops.gru_cell(g(hp), g(whh), g(bhh), out, **dkw)
            close(out, ref, 2e-5, "gru_cell x6=%s" % x6)
            if x6 in outs:
                assert torch.equal(out, outs[x6])
            outs[x6] = out
        assert float((outs[True] - outs[False]).abs().max()) < 5e-6
        if B > 128:                                       # ragged batch: the bf16 x 6 kernel does not take it, the call must still work
            out = torch.zeros(B - 3, H, device=DEV)
            rk = {k: (v[:B - 3] if torch.is_tensor(v) and v.shape[0] == B else v) for k, v in dkw.items()}
            ops.gru_cell(g(hp)[:B - 3], g(whh), g(bhh), out, **rk)
            close(out, ref[:B - 3], 2e-5, "ragged")
    finally:
        ops.dw_x6, ops.cell_x6, ops.cell_x6_rows = _x6_default(), True, 2048


def test_gemm_tn_column_view_at_the_end_of_its_allocation(ops):
    """weight-gradient form on a COLUMN-OFFSET view whose last row ends with the allocation (dpre[:, Z:2Z] of the latent block, K = batch rows):
    the operand loads must stay inside the view's columns - clamped to the leading dimension they ran 128 bytes past the buffer (a memory fault
    whenever that buffer closed a mapped segment; found in round 4).  Results against float64; a canary buffer allocated right behind stays intact."""
    torch.manual_seed(3)
    K, Z, H = 6, 32, 64
    for x6 in (False, True):
        ops.dw_x6 = x6
        parent = torch.randn(K, 2 * Z, device=DEV)
        canary = torch.full((64,), 7.0, device=DEV)
        hf = torch.randn(K, H, device=DEV)
        dW = torch.zeros(Z, 2 * H, device=DEV)
        ops.gemm(parent[:, Z:], hf, dW[:, :H], a_k=False, b_k=False)
        ops.gemm(parent[:, Z:], hf, dW[:, H:], a_k=False, b_k=False)
        want = parent[:, Z:].double().t() @ hf.double()
        close(dW[:, :H], want.float(), 2e-5)
        close(dW[:, H:], want.float(), 2e-5)
        assert bool((canary == 7.0).all())
    ops.dw_x6 = _x6_default()


def test_gemm_is_transpose_detecting(ops):
    """identity A with an ASYMMETRIC B: catches a swapped C-write (cdna guide rule 16)."""
    n = 96
    A = torch.eye(n)
    B = torch.arange(n * n, dtype=torch.float32).view(n, n) / 7.0          # B[k][j], asymmetric
    C = torch.zeros(n, n, device=DEV)
    ops.gemm(g(A), g(B), C, a_k=True, b_k=False)
    assert torch.equal(C.cpu(), B)


def test_gemm_strided_views(ops):
    """sub-matrix views with odd leading dimensions (W_ih[:, 342:], logits[:, :342]) take the scalar-load path."""
    torch.manual_seed(3)
    W = torch.randn(192, 622)
    z = torch.randn(37, 280)
    out = torch.zeros(37, 200, device=DEV)
    ops.gemm(g(z), g(W)[:, 342:], out[:, :192])
    close(out[:, :192], (z.double() @ W[:, 342:].double().t()).float(), 1e-5)
    assert float(out[:, 192:].abs().max()) == 0.0
    dl = torch.randn(50, 344)
    Wo = torch.randn(342, 64)
    dh = torch.zeros(50, 64, device=DEV)
    ops.gemm(g(dl)[:, :342], g(Wo), dh, a_k=True, b_k=False)
    close(dh, (dl[:, :342].double() @ Wo.double()).float(), 1e-5)


def test_small_dense_helpers(ops):
    torch.manual_seed(5)
    X = torch.randn(1000, 342)
    dst = torch.zeros(342, 1004, device=DEV)
    ops.transpose(g(X), dst[:, :1000])
    assert torch.equal(dst[:, :1000].cpu(), X.t())
    out = torch.ones(342, device=DEV)
    ops.colsum(g(X), out, beta=1.0)
    close(out, (X.double().sum(0) + 1).float(), 1e-5)
    big = torch.randn(70000, 96)
    out = torch.zeros(96, device=DEV)
    ops.colsum(g(big), out)
    close(out, big.double().sum(0).float(), 2e-5)
    y = torch.randn(5000, device=DEV)
    x = torch.randn(5000, device=DEV)
    y0 = y.clone()
    ops.axpy(0.25, x, y)
    close(y, y0 + 0.25 * x, 1e-6)
    s = torch.zeros(3, device=DEV)
    ops.sum(x, s[1:2], 0.5)
    close(s[1], 0.5 * x.double().sum().float(), 1e-5)
    gbuf = torch.randn(1234567, device=DEV)
    ss = torch.zeros(1, device=DEV)
    ops.sumsq(gbuf, ss)
    close(ss, (gbuf.double() ** 2).sum().float().view(1), 1e-6)
    oh = torch.zeros(40, 342)
    ids = torch.randint(0, 342, (40,))
    oh[torch.arange(40), ids] = 1
    idx = torch.zeros(40, dtype=torch.int32, device=DEV)
    ops.onehot_to_index(g(oh), idx)
    assert torch.equal(idx.cpu().long(), ids)


def _scan_inputs(B, T, H, V, seed, with_table=True, reverse=0, shift=0):
    torch.manual_seed(seed)
    s = dict(B=B, T=T, H=H, reverse=reverse, w_hh=torch.randn(3 * H, H) / math.sqrt(H), b_hh=torch.randn(3 * H) * 0.1,
             b_ih=torch.randn(3 * H) * 0.1, h0=torch.randn(B, H) * 0.5, gx_rowbias=torch.randn(B, 3 * H) * 0.3,
             idx_shift=shift, start_token=V - 1)
    if with_table:
        s["gx_table"] = torch.randn(V, 3 * H) * 0.5
        s["idx"] = torch.randint(0, V, (B, T), dtype=torch.int32)
    else:
        s["gx_dense"] = torch.randn(T, B, 3 * H) * 0.5
    s["h_all"] = torch.zeros(T, B, H)
    s["gates"] = torch.zeros(T, FakeOps.gates_floats(B, H))
    return s


def _to_dev(s):
    return {k: (g(v) if torch.is_tensor(v) else v) for k, v in s.items()}


def _pack(backend, mat, device):
    """weights in the backend's (opaque) operand image"""
    out = torch.zeros(backend.frag_floats(*mat.shape), device=device)
    backend.frag_pack(mat.to(device).contiguous(), out)
    return out


@pytest.mark.parametrize("mode", ["per_step", "stationary", "stationary_half_chip"])
@pytest.mark.parametrize("B,T,H", [(6, 5, 64), (70, 9, 96), (256, 4, 512), (40, 37, 512)])
def test_gru_scan_fwd_bwd_kernels(ops, B, T, H, mode):
    """fn_gru_seq_fwd / fn_gru_seq_bwd: three concurrent scans (table+reverse, table+shift, dense; different T), through
    the per-step launches, the weight-stationary single launch, and the latter restricted to half of the CUs."""
    fake = FakeOps()
    kw = dict(persistent=mode != "per_step", cu_budget=128 if mode.endswith("half_chip") else 0)
    cpu = [_scan_inputs(B, T, H, 21, 1, True, reverse=1), _scan_inputs(B, T + 2, H, 21, 2, True, shift=-1),
           _scan_inputs(B, max(1, T - 2), H, 21, 3, False)]
    cpu[2]["h0"] = None
    dev = [_to_dev(s) for s in cpu]
    for c, d in zip(cpu, dev):
        c["w_hh_frag"], d["w_hh_frag"] = _pack(fake, c["w_hh"], "cpu"), _pack(ops, c["w_hh"], DEV)
    fake.gru_seq_fwd(cpu)
    ops.gru_seq_fwd(dev, **kw)
    for i, (c, d) in enumerate(zip(cpu, dev)):
        close(d["h_all"], c["h_all"], 2e-5, "h_all[%d]" % i)
        close(_unblock_gates(d["gates"].cpu(), B, H), c["gates"][:, : B * 4 * H].reshape(c["T"], B, 4, H), 2e-5, "gates[%d]" % i)
    bc, bd = [], []
    for i, c in enumerate(cpu):
        Ti = c["T"]
        torch.manual_seed(10 + i)
        b = dict(B=B, T=Ti, H=H, w_hh_t_frag=_pack(fake, c["w_hh"].t().contiguous(), "cpu"), h0=c.get("h0"), h_all=c["h_all"], gates=c["gates"],
                 dh_last=torch.randn(B, H) if i != 1 else None, dh_ext=torch.randn(Ti, B, H) if i != 0 else None,
                 dgx_all=torch.zeros(Ti, B, 3 * H), dghn_all=torch.zeros(Ti, B, H), dh0=torch.zeros(B, H) if i != 2 else None,
                 dgx_rowsum=torch.zeros(B, 3 * H) if i == 1 else None, dghn_rowsum=torch.zeros(B, H) if i != 0 else None,
                 scratch=torch.zeros(B, H))
        bc.append(b)
        bdev = _to_dev(b)
        bdev["gates"], bdev["h_all"] = dev[i]["gates"], dev[i]["h_all"]      # each backend consumes its OWN saved gates
        bdev["w_hh_t_frag"] = _pack(ops, c["w_hh"].t().contiguous(), DEV)
        bd.append(bdev)
    fake.gru_seq_bwd(bc)
    ops.gru_seq_bwd(bd, **kw)
    assert not ops.gru_sync_error()
    for i, (c, d) in enumerate(zip(bc, bd)):
        for k in ("dgx_all", "dghn_all", "dh0", "dgx_rowsum", "dghn_rowsum"):
            if c[k] is not None:
                close(d[k], c[k], 5e-5, "%s[%d]" % (k, i))
    # token-segment sums of dgx (one-hot W_ih columns)
    for i in (0, 1):
        out_c, out_d = torch.zeros(21, 3 * H), torch.zeros(21, 3 * H, device=DEV)
        fake.embed_grad(bc[i]["dgx_all"], cpu[i]["idx"], cpu[i]["idx_shift"], 20, cpu[i]["reverse"], 21, out_c)
        ops.embed_grad(bd[i]["dgx_all"], dev[i]["idx"], cpu[i]["idx_shift"], 20, cpu[i]["reverse"], 21, out_d)
        close(out_d, out_c, 5e-5, "embed_grad[%d]" % i)


@pytest.mark.parametrize("case", SCAN_CASES, ids=[c["id"] for c in SCAN_CASES])
def test_scans_every_step_vs_fp64(ops, case):
    """Every scan kernel instance fn_gru_seq_fwd / fn_gru_seq_bwd can launch, at its production launch shape, against an fp64 scan and torch
    autograd through it (helpers.scan_reference_f64, evaluated by plain torch in float64), at EVERY step and 32-row block of the checked rows
    (two rows of every 16-row tile, all columns): h_all, the four saved-gate planes, dgx_all, dghn_all, dh0 and both row sums within
    SCAN_F x max(e_ref, 2**-23) of the reference, e_ref = the fp32 CPU restatement's own error at that step and block, and within the whole-tensor
    bound as before (helpers.check_scan_vs_f64).  The cases (helpers.SCAN_CASES): the encoder launch (4 x 256 rows x 256 steps, dh_last only), the
    decoder pipeline (2 x 256 rows, 256 and 226 steps as chained 32-step launches with operand-image and state-gradient hand-overs, backward on
    the whole and on half of the chip), the attribute decoders (64 steps, dL/dh0), the 32-slice kernels in every forced row block and switch at
    70 steps with ragged batches, the per-step kernels, T = 2 and T = 1, 8 scans of different lengths.  The arithmetic and the variant bits are
    asked for explicitly, so a launch that cannot take the bf16 x 6 kernel raises; a bf16 x 6 case must also differ in some bit from the fp32
    kernels' result (it really ran).  The fo-* cases are forward only (gates = NULL, as every save=False caller launches): no backward runs, h_all is
    checked at every step, and the plans must name a gru_fwd_persist_kernel tiling or the per-step kernel, never a ping-pong or bf16 x 6 one.
    Each case prints the lines of profiles/scan_fp64_errors.txt."""
    scans, rows, chunk = scan_inputs(case["inputs"])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    Ts = [None] if chunk is None else sorted({chunk, scans[0]["T"] % chunk or chunk})
    names = [scan_kernel_names(scans, case["variants"], case["x6"], case["budget"], case["persistent"], T=T, cus=cus) for T in Ts]
    fo = case_forward_only(case)                                 # gates = NULL: forward launches only, h_all alone (helpers.run_scans)
    for T, nm in zip(Ts, names):
        for i, have in enumerate(nm):
            want = case_kernel(case, i, T)
            assert want is None or want == have, (want, have)      # the shape reaches the kernel the case is for on this device
    kw = [dict(persistent=case["persistent"], cu_budget=case["budget"][i], variant=case["variants"][i]) for i in (0, 1)]
    try:
        ops.dw_x6 = case["x6"]
        rec = PlanRecorder(ops)
        got = run_scans(rec, scans, rows, device=DEV, chunk=chunk, x6=case["x6"], fwd_kw=kw[0], bwd_kw=kw[1])
        torch.cuda.synchronize()
        assert not ops.gru_sync_error()
        # the library's own plan on the real descriptors: the candidate every launch of the case took on this device is the kernel the case is for
        for i, plans in enumerate((rec.fwd, rec.bwd)):
            if fo and i == 1:
                assert not plans                                  # a forward-only case launches no backward
                continue
            assert len(plans) == (1 if chunk is None else -(-scans[0]["T"] // chunk))
            want = {case_kernel(case, i, T) for T in Ts}
            assert None in want or set(chosen_kernels(plans)) == want, (want, plans)
            # ... and what the hand restatement names (a case without named kernels included)
            assert set(chosen_kernels(plans)) == {nm[i] for nm in names}, (names, plans)
        if fo:
            assert not any(k.startswith(("gru_fwd_pp", "gru_fwd_x6")) for k in chosen_kernels(rec.fwd))
        if case["x6"]:
            ops.dw_x6 = False
            f32 = run_scans(ops, scans, rows, device=DEV, chunk=chunk, x6=False)
            torch.cuda.synchronize()
            assert not ops.gru_sync_error()
            assert any(not torch.equal(a[k], b[k]) for a, b in zip(got, f32) for k in ("h_all", "dgx_all"))      # results are not bit-identical
    finally:
        ops.dw_x6 = _x6_default()
    worst = check_scan_vs_f64(scans, got, rows, chunk, key=case["inputs"], ref_device=DEV)
    print()
    label = tuple("+".join(sorted({nm[i] for nm in names})) for i in (0, 1))        # (a chain whose tail chunk takes another kernel names both)
    for line in scan_lines(case["id"], label, worst):
        print(line)


def test_scan_with_a_misaligned_h_all_runs_per_step(ops):
    """B = 33, H = 64, T = 3, one scan, h_all a view 4 bytes behind a 16-byte boundary: the weight-stationary kernels' epilogues move 16-byte vectors, so
    the plan of the forward and of the backward call has the per-step candidate only; the results are bit-identical to the per-step kernels on aligned
    buffers and within the bound of the CPU restatement"""
    from fake_ops import FakeOps
    scans = _ws_scans(torch.Generator().manual_seed(3364), 33, 64, T=3, n=1)
    ref = run_scans(FakeOps(), scans)
    try:
        ops.dw_x6 = False
        rec = PlanRecorder(ops)
        off = run_scans(rec, scans, device=DEV, h_all_off=1)
        aligned = run_scans(ops, scans, device=DEV, fwd_kw=dict(persistent=False), bwd_kw=dict(persistent=False))
        torch.cuda.synchronize()
        assert not ops.gru_sync_error()
    finally:
        ops.dw_x6 = _x6_default()
    for plans, step in ((rec.fwd, "gru_fwd_step_kernel"), (rec.bwd, "gru_bwd_step_kernel")):
        assert len(plans) == 1 and plans[0]["ws_absent"] == "unaligned" and plans[0]["chosen"] == 0, plans
        assert [c["kernel"] for c in plans[0]["candidates"]] == [step], plans
    assert set(off[0]) == set(aligned[0]) == set(ref[0]) and {"h_all", "dgx_all", "dghn_all", "dh0", "dgx_rowsum"} <= set(off[0])
    for k in off[0]:
        assert torch.equal(off[0][k], aligned[0][k]), k
        close(off[0][k], ref[0][k], 2e-5 if k in ("h_all", "gate_r", "gate_z", "gate_n", "gate_hn") else 5e-5, "misaligned h_all: " + k)
        close(aligned[0][k], ref[0][k], 2e-5 if k in ("h_all", "gate_r", "gate_z", "gate_n", "gate_hn") else 5e-5, "per-step: " + k)


def test_nine_scans_in_one_call_are_refused(ops):
    """fn_gru_seq_fwd / fn_gru_seq_bwd take at most 8 scans: FN_E_COUNT, nothing launched"""
    scans, rows, _ = scan_inputs("eight")
    with pytest.raises(RuntimeError, match=r"code -5"):
        run_scans(ops, scans + scans[:1], rows + rows[:1], device=DEV)
    torch.cuda.synchronize()
    assert not ops.gru_sync_error()
    fwd_only = [{k: v for k, v in s.items() if k not in ("dh_last", "dh_ext")} for s in scans]
    done = run_scans(ops, fwd_only, rows, device=DEV)
    b = dict(B=64, T=3, H=512, w_hh_t_frag=torch.zeros(ops.frag_floats(512, 1536), device=DEV), h_all=torch.zeros(3, 64, 512, device=DEV),
             gates=torch.zeros(3, ops.gates_floats(64, 512), device=DEV), dh_last=torch.zeros(64, 512, device=DEV), dgx_all=torch.zeros(3, 64, 1536, device=DEV),
             dghn_all=torch.zeros(3, 64, 512, device=DEV), scratch=torch.zeros(64, 512, device=DEV))
    with pytest.raises(RuntimeError, match=r"code -5"):
        ops.gru_seq_bwd([b] * 9)
    assert len(done) == 8 and not ops.gru_sync_error()


def test_weight_stationary_scans_random_configurations(ops):
    """60 random (scans, rows, lengths, H, input kinds, CU budgets) drawn with a fixed seed: the single-launch scans, run three times
    in a row on the same buffers (cache-warm exchange slabs), must reproduce the per-step kernels (forward state + saved gates)."""
    rng = np.random.RandomState(5)
    V = 57
    for case in range(60):
        H = int(rng.choice([64, 96, 128, 512]))
        B = int(rng.choice([1, 5, 16, 33, 64, 100, 200, 256]))
        budget = int(rng.choice([0, 0, 128]))
        scans = []
        for s in range(int(rng.randint(1, 5))):
            T = int(rng.randint(2, 24))
            wf = torch.zeros(ops.frag_floats(3 * H, H), device=DEV)
            ops.frag_pack((torch.randn(3 * H, H, device=DEV) / H ** 0.5).contiguous(), wf)
            d = dict(B=B, T=T, H=H, reverse=int(rng.randint(2)), w_hh_frag=wf, b_hh=torch.randn(3 * H, device=DEV) * 0.1,
                     h_all=torch.zeros(T, B, H, device=DEV), gates=torch.zeros(T, ops.gates_floats(B, H), device=DEV))
            if rng.rand() < 0.6:
                d["h0"] = torch.randn(B, H, device=DEV) * 0.3
            if rng.rand() < 0.5:
                d["gx_table"] = torch.randn(V, 3 * H, device=DEV) * 0.3
                d["idx"] = torch.randint(0, V, (B, T + 1), dtype=torch.int32, device=DEV)
                if rng.rand() < 0.3:
                    d["idx_shift"], d["start_token"] = -1, V - 1
            else:
                d["gx_dense"] = torch.randn(T, B, 3 * H, device=DEV) * 0.3
            if rng.rand() < 0.5:
                d["gx_rowbias"] = torch.randn(B, 3 * H, device=DEV) * 0.2
            scans.append(d)
        ops.gru_seq_fwd(scans, persistent=False)
        ref = [(d["h_all"].clone(), d["gates"].clone()) for d in scans]
        for rep in range(3):
            for d in scans:
                d["h_all"].fill_(float("nan"))
            ops.gru_seq_fwd(scans, persistent=True, cu_budget=budget)
            for (h, gt), d in zip(ref, scans):
                close(d["h_all"], h, 2e-5, "case %d rep %d h_all" % (case, rep))
                close(d["gates"], gt, 2e-5, "case %d rep %d gates" % (case, rep))
    assert not ops.gru_sync_error()


@pytest.mark.parametrize("rows,H,splitk,beta", [(37, 64, 1, 0.0), (1030, 64, 4, 1.0), (300, 96, 4, 0.0), (5000, 512, 8, 1.0)])
def test_gru_weight_gradient(ops, rows, H, splitk, beta):
    """fn_gru_dwhh_f32: dW_hh = beta dW_hh + [dgx[:, :2H] | dghn]^T hprev (one split-A launch when 2H % 128 == 0, else two products)."""
    torch.manual_seed(rows + H)
    dgx, dghn, hp = torch.randn(rows, 3 * H), torch.randn(rows, H), torch.randn(rows, H)
    dW0 = torch.randn(3 * H, H)
    ref = beta * dW0.double() + torch.cat([dgx[:, : 2 * H], dghn], 1).double().t() @ hp.double()
    dW = g(dW0)
    ops.gru_dwhh(g(dgx), g(dghn), g(hp), dW, beta=beta, splitk=splitk)
    close(dW, ref.float(), 2e-5 * max(1.0, (rows ** 0.5)))


@pytest.mark.parametrize("M,N,K,splitk", [(1536, 512, 4100, 16), (342, 512, 8192, 8), (1536, 512, 65280, 16), (200, 130, 1031, 1)])
def test_gemm_tn_bf16x6(ops, M, N, K, splitk):
    """FN_GEMM_BF16X6 (opt-in): the weight-gradient product with exact bf16 triple splits on the bf16 MFMA is AS ACCURATE as the default fp32
    MFMA kernel - both measured against float64: its error must stay below the same bound the fp32 kernel is tested with and within 2 x of
    the fp32 kernel's own error (K tails below 32, ragged tiles, the [dgx | dghn] two-source form of fn_gru_dwhh_f32 and split-K slabs)."""
    torch.manual_seed(M + K)
    A = torch.randn(K, M, device=DEV)
    B = torch.randn(K, N, device=DEV) * 0.3
    ref = (A.double().t() @ B.double())
    scale = float((A.double().abs().t() @ B.double().abs()).max())
    out = {}
    for x6 in (False, True):
        ops.dw_x6 = x6
        C = torch.full((M, N), float("nan"), device=DEV)
        kern = ops.gemm_plan(A, B, C, a_k=False, b_k=False, splitk=splitk)["kernel"]          # what the library's dispatch launches for this very call
        if M % 4 == 0 and N % 4 == 0:
            assert kern.startswith("gemm_tn_x6") if x6 else kern == "gemm_tn_kernel", (x6, kern)
        else:                                       # 342 x 512 and 200 x 130 dense: a leading dimension % 4 != 0, so neither arithmetic reaches a TN kernel - a staged fp32 instance runs both
            assert kern.startswith("gemm_kernel<"), (x6, kern)
        ops.gemm(A, B, C, a_k=False, b_k=False, splitk=splitk)
        out[x6] = float((C.double() - ref).abs().max()) / scale
    ops.dw_x6 = _x6_default()
    assert out[True] < 2e-6 and out[True] <= 2.0 * out[False] + 1e-9, out
    if M == 1536:                                          # the one-launch [dr' dz' | dn' r]^T h form (A2 second source)
        H = 512
        dgx, dghn, hp = A, torch.randn(K, H, device=DEV), B
        want = torch.cat([dgx[:, :2 * H], dghn], 1).double().t() @ hp.double()
        sc = float((torch.cat([dgx[:, :2 * H], dghn], 1).double().abs().t() @ hp.double().abs()).max())
        err = {}
        for x6 in (False, True):
            ops.dw_x6 = x6
            dW = torch.zeros(3 * H, H, device=DEV)
            ops.gru_dwhh(dgx, dghn, hp, dW, splitk=splitk)
            err[x6] = float((dW.double() - want).abs().max()) / sc
        ops.dw_x6 = _x6_default()
        assert err[True] < 2e-6 and err[True] <= 2.0 * err[False] + 1e-9, err


@pytest.mark.parametrize("M,N,K,splitk", [(1536, 512, 1024, 32), (1536, 512, 2048, 32), (342, 512, 3072, 32), (256, 384, 4096, 32), (130, 70, 5120, 32),
                                          (1536, 512, 65280, 16), (342, 512, 65536, 42), (128, 128, 1024, 1), (200, 130, 1031, 1), (1536, 512, 4100, 16),
                                          (64, 48, 1056, 3)])
def test_gemm_tn_x6_producer_consumer_vs_per_wave_kernel(ops, M, N, K, splitk):
    """gemm_tn_x6w_kernel / gemm_tn_x6v_kernel (round 6: producer wavefronts split every operand value once per workgroup, consumer wavefronts only
    multiply; 128 x 128 and 128 x 256 output tiles) against the round-5 kernel in which every wavefront splits its own operands (FN_GEMM_X6_PERWAVE):
    the same products in the same order per accumulator, so on K ranges of whole 32-k blocks the results are BIT-IDENTICAL (1 .. 5 blocks per range:
    every prologue / tail path of the loops; ragged tiles; 1-D and 3-D grids; the two-source form of fn_gru_dwhh_f32); with a K tail (which the
    per-wave kernel runs on the fp32 MFMA and these as a zero-padded block) all stay within the fp32 kernel's error bound against float64.
    beta / bias / alpha on an unsplit product."""
    torch.manual_seed(M * 7 + K)
    A = torch.randn(K, M, device=DEV)
    B = torch.randn(K, N, device=DEV) * 0.3
    ref = (A.double().t() @ B.double())
    scale = float((A.double().abs().t() @ B.double().abs()).max())
    # (the two producer / consumer kernels both as one workgroup per CU walking its (tile, K range) items - the default - and as one workgroup per item)
    MODES = (("perwave", False, True, False), ("tile128", False, False, False), ("tile256", "force", False, False),
             ("tile128_item", False, False, True), ("tile256_item", "force", False, True))
    ops.dw_x6 = True
    probe = torch.empty(M, N, device=DEV)

    def run(fn):
        out = {}
        for name, wide, pw, item in MODES:
            ops.x6_wide, ops.x6_perwave, ops.x6_per_tile = wide, pw, item
            kern = ops.gemm_plan(A, B, probe, a_k=False, b_k=False, splitk=splitk)["kernel"]          # the library's dispatch names the kernel the mode is for
            if M % 4 == 0 and N % 4 == 0:
                assert kern == {"perwave": "gemm_tn_x6_kernel", "tile128": "gemm_tn_x6w_kernel", "tile256": "gemm_tn_x6v_kernel"}[name.split("_")[0]], (name, kern)
            else:                                   # 342 x 512, 200 x 130 and 130 x 70 dense: a leading dimension % 4 != 0 keeps every mode off the TN kernels (a staged fp32 instance)
                assert kern.startswith("gemm_kernel<"), (name, kern)
            out[name] = fn()
        ops.x6_per_tile = False
        assert torch.equal(out["tile128"], out["tile128_item"]) and torch.equal(out["tile256"], out["tile256_item"])
        return out
    try:
        def plain():
            C = torch.full((M, N), float("nan"), device=DEV)
            ops.gemm(A, B, C, a_k=False, b_k=False, splitk=splitk)
            return C
        out = run(plain)
        klen = K if splitk <= 1 else ((K + splitk - 1) // splitk + 31) // 32 * 32
        whole = all(min(K, k0 + klen) % 32 == 0 for k0 in range(0, K, klen))
        for name in out:
            assert float((out[name].double() - ref).abs().max()) / scale < 2e-6, name
        if whole:
            assert torch.equal(out["perwave"], out["tile128"]) and torch.equal(out["perwave"], out["tile256"])
        else:
            assert torch.equal(out["tile128"], out["tile256"])      # both multiply the K tail as a zero-padded block
        if splitk <= 1:                                   # epilogue without slabs: alpha, beta, bias
            bias = torch.randn(N, device=DEV)
            C0 = torch.randn(M, N, device=DEV)

            def full():
                C = C0.clone()
                ops.gemm(A, B, C, a_k=False, b_k=False, alpha=0.5, beta=2.0, bias=bias)
                return C
            res = run(full)
            want = 0.5 * ref + 2.0 * C0.double() + bias.double()
            for name in res:
                assert float((res[name].double() - want).abs().max()) / (scale + float(C0.abs().max()) * 2) < 2e-6, name
            if whole:
                assert torch.equal(res["perwave"], res["tile128"]) and torch.equal(res["perwave"], res["tile256"])
        if M == 1536:                                     # the one-launch [dr' dz' | dn' r]^T h form (A2 second source)
            H = 512
            dgx, dghn, hp = A, torch.randn(K, H, device=DEV), B

            def dwhh():
                dW = torch.zeros(3 * H, H, device=DEV)
                ops.gru_dwhh(dgx, dghn, hp, dW, splitk=splitk)
                return dW
            dws = run(dwhh)
            want = torch.cat([dgx[:, :2 * H], dghn], 1).double().t() @ hp.double()
            sc = float((torch.cat([dgx[:, :2 * H], dghn], 1).double().abs().t() @ hp.double().abs()).max())
            for name in dws:
                assert float((dws[name].double() - want).abs().max()) / sc < 2e-6, name
            if whole:
                assert torch.equal(dws["perwave"], dws["tile128"]) and torch.equal(dws["perwave"], dws["tile256"])
            # the automatic choice (twice the K ranges with the wide tiles) against the per-wave kernel on the same ranges
            ops.x6_wide = True
            auto = {}
            for pw in (True, False):
                ops.x6_perwave = pw
                auto[pw] = dwhh()
            for pw in auto:
                assert float((auto[pw].double() - want).abs().max()) / sc < 2e-6, pw
            if K % 32 == 0 and splitk > 1 and (K // (2 * splitk)) % 32 == 0:
                assert torch.equal(auto[True], auto[False])
    finally:
        ops.dw_x6, ops.x6_perwave, ops.x6_wide, ops.x6_per_tile = _x6_default(), False, True, False


@pytest.mark.parametrize("M,N,K", [(8192, 1536, 512), (8192, 512, 1536), (65536, 512, 352), (2048, 1024, 128), (2048, 1024, 160), (4096, 512, 32 * 7),
                                   (8192, 1024, 160), (4096, 1152, 32 * 7), (16384, 256, 128)])      # (the last three: 512 / 288 / 256 tiles of 5 / 7 / 4 blocks - a workgroup walks 2, 1 or 2, 1 tiles)
def test_gemm_nt_bf16x6(ops, M, N, K):
    """gemm_nt_x6w_kernel (round 6): the Linear-forward form C = alpha A B^T + bias + beta C with both operands K-contiguous, exact bf16 triple splits
    on the bf16 MFMA - the decoder pipeline's layer-2 input projection and the state-gradient products.  Against float64 it is as accurate as the fp32
    MFMA kernels (error bound of the fp32 tests, within 2 x of the fp32 kernel's own error); 4 .. 48 blocks of 32 k (every prologue / tail path of the
    producer loop), alpha / beta / bias; repeated launches are bit-identical."""
    torch.manual_seed(M + N + K)
    A = torch.randn(M, K, device=DEV)
    W = torch.randn(N, K, device=DEV) * 0.2
    bias = torch.randn(N, device=DEV)
    C0 = torch.randn(M, N, device=DEV)
    ref = A.double() @ W.double().t()
    scale = float((A.double().abs() @ W.double().abs().t()).max())
    err, outs = {}, {}
    try:
        for x6 in (False, True):
            ops.dw_x6, ops.nt_x6 = x6, x6
            C = torch.full((M, N), float("nan"), device=DEV)
            kern = ops.gemm_plan(A, W, C, a_k=True, b_k=True)["kernel"]          # what the library's dispatch launches for this very call
            assert (kern == "gemm_nt_x6w_kernel") == x6 and (x6 or kern.startswith(("gemm_nt_direct_kernel", "gemm_kernel"))), (x6, kern)
            ops.gemm(A, W, C, a_k=True, b_k=True)
            err[x6] = float((C.double() - ref).abs().max()) / scale
            C2 = C0.clone()
            ops.gemm(A, W, C2, a_k=True, b_k=True, alpha=0.5, beta=2.0, bias=bias)
            want = 0.5 * ref + 2.0 * C0.double() + bias.double()
            assert float((C2.double() - want).abs().max()) / (scale + 2 * float(C0.abs().max())) < 2e-6, x6
            outs[x6] = C
        assert err[True] < 2e-6 and err[True] <= 2.0 * err[False] + 1e-9, err
        ops.dw_x6, ops.nt_x6 = True, True
        C = torch.empty(M, N, device=DEV)
        ops.gemm(A, W, C, a_k=True, b_k=True)
        assert torch.equal(C, outs[True])
        # one workgroup per CU walking its tiles (more tiles than CUs) == one workgroup per tile, bit for bit
        ops.x6_per_tile = True
        C = torch.full((M, N), float("nan"), device=DEV)
        ops.gemm(A, W, C, a_k=True, b_k=True)
        assert torch.equal(C, outs[True])
    finally:
        ops.dw_x6, ops.nt_x6, ops.x6_per_tile = _x6_default(), True, False


@pytest.mark.parametrize("nblk", range(1, 14))
def test_bf16x6_producer_trips_at_every_block_count(ops, nblk):
    """The shared producer trip schedule (x6w_trips, csrc/x6w_core.h) at its boundaries: 1 .. 13 blocks of 32 k per K range = no steady-state pass, one
    pass (NS = 3 trips) with every tail length, two passes - for every kernel that runs on it.
    TN (128 x 256 x 32 nblk, one K range): gemm_tn_x6w_kernel and gemm_tn_x6v_kernel bit-identical to the per-wave kernel; with K = 32 nblk - 5 (the last
    block partial) bit-identical to each other and within the fp32 kernels' float64 bound.  NT (2048 x 1024 - 128 tiles, the dispatch threshold -, from 4
    blocks on: the dispatch takes K >= 128): the float64 bound of test_gemm_nt_bf16x6, one workgroup per tile == one per CU.  Cell (128 rows, no dense
    input, H = 32 nblk; H = 32 is below what the bf16 x 6 cell takes and runs on the fp32 cell): against the fp32 cell, tolerance of test_gru_cell_bf16x6."""
    torch.manual_seed(1000 + nblk)
    try:
        ops.dw_x6 = True
        M, N = 128, 256
        for K in (32 * nblk, 32 * nblk - 5):
            A = torch.randn(K, M, device=DEV)
            B = torch.randn(K, N, device=DEV) * 0.3
            ref = A.double().t() @ B.double()
            scale = float((A.double().abs().t() @ B.double().abs()).max())
            out = {}
            for name, wide, pw in (("perwave", False, True), ("tile128", False, False), ("tile256", "force", False)):
                ops.x6_wide, ops.x6_perwave = wide, pw
                out[name] = torch.full((M, N), float("nan"), device=DEV)
                ops.gemm(A, B, out[name], a_k=False, b_k=False, splitk=1)
            ops.x6_wide, ops.x6_perwave = True, False
            for name in out:
                err = float((out[name].double() - ref).abs().max()) / scale
                print("TN nblk %d K %d %s err %.3e" % (nblk, K, name, err))
                assert err < 2e-6, (name, K)
            if K % 32 == 0:
                assert torch.equal(out["tile128"], out["perwave"]) and torch.equal(out["tile256"], out["perwave"]), K
            else:                                         # both multiply the K tail as a zero-padded block
                assert torch.equal(out["tile128"], out["tile256"]), K
        if nblk >= 4:
            M, N, K = 2048, 1024, 32 * nblk
            A = torch.randn(M, K, device=DEV)
            W = torch.randn(N, K, device=DEV) * 0.2
            ref = A.double() @ W.double().t()
            scale = float((A.double().abs() @ W.double().abs().t()).max())
            err, outs = {}, {}
            for x6 in (False, True):
                ops.dw_x6, ops.nt_x6 = x6, x6
                outs[x6] = torch.full((M, N), float("nan"), device=DEV)
                ops.gemm(A, W, outs[x6], a_k=True, b_k=True)
                err[x6] = float((outs[x6].double() - ref).abs().max()) / scale
            print("NT nblk %d err fp32 %.3e bf16x6 %.3e" % (nblk, err[False], err[True]))
            assert err[True] < 2e-6 and err[True] <= 2.0 * err[False] + 1e-9, err
            ops.x6_per_tile = True
            C = torch.full((M, N), float("nan"), device=DEV)
            ops.gemm(A, W, C, a_k=True, b_k=True)
            assert torch.equal(C, outs[True])
        Bc, H, V = 128, 32 * nblk, 50
        hp = torch.randn(Bc, H) * 0.5
        whh, bhh, bih = torch.randn(3 * H, H) / H ** 0.5, torch.randn(3 * H) * 0.1, torch.randn(3 * H) * 0.1
        kw = dict(b_ih=bih, gx_table=torch.randn(V, 3 * H) * 0.3, gx_rowbias=torch.randn(Bc, 3 * H) * 0.3, start_token=V - 1)
        ref = torch.zeros(Bc, H)
        idx = torch.randint(0, V, (Bc,), dtype=torch.int32)
        FakeOps().gru_cell(hp, whh, bhh, ref, idx=idx, **kw)
        dkw = {k: (g(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
        outs = {}
        for x6 in (False, True):
            ops.dw_x6, ops.cell_x6, ops.cell_x6_rows = x6, x6, 0
            outs[x6] = torch.full((Bc, H), float("nan"), device=DEV)
            ops.gru_cell(g(hp), g(whh), g(bhh), outs[x6], idx=g(idx), **dkw)
            close(outs[x6], ref, 2e-5, "gru_cell x6=%s" % x6)
        d = float((outs[True] - outs[False]).abs().max())
        print("cell nblk %d max |x6 - fp32| %.3e" % (nblk, d))
        assert d < 5e-6
    finally:
        ops.dw_x6, ops.x6_perwave, ops.x6_wide, ops.x6_per_tile, ops.nt_x6, ops.cell_x6, ops.cell_x6_rows = _x6_default(), False, True, False, True, True, 2048


def test_gemm_bf16x6_kernels_random_shapes():
    """scratch/r6_fuzz_gemm.py (the randomised sweep behind profiles/r06_gemm_fuzz.txt) with a small case count: ragged M / N, K tails, every split depth,
    padded leading dimensions, the two-source form, the Linear-forward form with alpha / beta / bias - the three weight-gradient kernels agree bit for bit
    on whole-block K ranges (the two producer / consumer kernels always) and every result stays within the fp32 kernels' float64 error bound"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scratch", "r6_fuzz_gemm.py"), "60", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "TN: 60 cases, 0 mismatches" in r.stdout and "NT: 30 cases, 0 mismatches" in r.stdout, r.stdout[-1000:]


@pytest.mark.parametrize("n,B,T", [(4, 256, 14), (2, 256, 9), (1, 128, 6), (3, 64, 5)])
def test_forward_scan_bf16x6(ops, n, B, T):
    """the opt-in forward scan with exact split products on the bf16 MFMA (FnGruFwd.variant | FN_GRU_BF16X6: weights and exchanged state as bf16 triples,
    fn_frag3_pack) against the default weight-stationary kernels at H = 512: states and saved gates agree to fp32 rounding (the products are
    exact, the sums run in another order); 128-row groups (4 x 256 rows), 64-row groups, table / dense inputs, reverse scans, row biases,
    shifted tokens, initial states, two chunks with the state handed over as a triple image (bit-identical to one launch); repeated launches on warm
    slabs are bit-identical; a scan without saved gates makes the call fall back to the default kernels"""
    from music_fader_nets_amd import _lib
    H, V = 512, 57
    rng = np.random.RandomState(n * 100 + B + T)
    torch.manual_seed(n + B)
    scans = []
    for s_ in range(n):
        w = (torch.randn(3 * H, H, device=DEV) / (H ** 0.5)).contiguous()
        wf = torch.zeros(ops.frag_floats(3 * H, H), device=DEV)
        ops.frag_pack(w, wf)
        wf3 = torch.zeros(ops.frag_floats(3 * H, H) * 3 // 2, device=DEV)
        ops.frag3_pack(w, wf3)
        d = dict(B=B, T=T, H=H, reverse=int(rng.randint(2)), w_hh_frag=wf, w_hh_frag3=wf3, b_hh=torch.randn(3 * H, device=DEV) * 0.1,
                 b_ih=torch.randn(3 * H, device=DEV) * 0.1, h_all=torch.zeros(T, B, H, device=DEV), gates=torch.zeros(T, ops.gates_floats(B, H), device=DEV))
        if s_ % 2 == 0:
            d["gx_table"] = torch.randn(V, 3 * H, device=DEV) * 0.3
            d["idx"] = torch.randint(0, V, (B, T + 3), dtype=torch.int32, device=DEV)
            if not d["reverse"] and s_ == 0:
                d["idx_shift"], d["start_token"] = -1, V - 1
        else:
            d["gx_dense"] = torch.randn(T, B, 3 * H, device=DEV) * 0.3
        if s_ != 1:
            d["gx_rowbias"] = torch.randn(B, 3 * H, device=DEV) * 0.2
        scans.append(d)

    def run(x6, variant=0):
        ops.dw_x6, ops.variant = x6, variant
        for d in scans:
            d["h_all"].fill_(float("nan")); d["gates"].fill_(float("nan"))
        ops.gru_seq_fwd(scans)
        torch.cuda.synchronize()
        ops.variant = 0
        return [d["h_all"].clone() for d in scans] + [d["gates"].clone() for d in scans]
    try:
        ref = run(False)
        got = run(True)
        again = run(True)
        single = run(True, _lib.GRU_X6_SINGLE_GROUP)       # the single-group bf16 x 6 kernel (no ping-pong)
        assert not ops.gru_sync_error()
        differs = False
        for a, b, c, e in zip(ref, got, again, single):
            assert torch.equal(b, c)
            assert not torch.isnan(b).any()
            differs |= not torch.equal(a, b)
            assert float((a - b).abs().max()) <= 5e-5 * float(a.abs().max()), float((a - b).abs().max())
            if n * B > 512:                                # 128-row groups: no K split in either kernel, the same accumulation order - bit for bit
                assert torch.equal(b, e)
            else:
                assert float((e - b).abs().max()) <= 5e-5 * float(a.abs().max())
        assert differs                                     # the x6 kernel really ran (another summation order)
        # initial state + two chunks with the state handed over as a triple image (what the decoder pipeline does)
        for d in scans:
            d["h0"] = torch.randn(B, H, device=DEV) * 0.1
        ref = run(False)
        got = run(True)
        for a, b in zip(ref, got):
            assert float((a - b).abs().max()) <= 5e-5 * float(a.abs().max())
        T1 = T // 2
        hand = [torch.zeros(ops.frag_floats(B, H) * 3 // 2, device=DEV) for _ in scans]

        def chunk(d, t0, t1, first):
            c = dict(d)
            c.update(T=t1 - t0, h_all=d["h_all"][t0:t1], gates=d["gates"][t0:t1])
            if d.get("gx_dense") is not None:
                c["gx_dense"] = d["gx_dense"][t0:t1]
            if d.get("idx") is not None:
                c["idx_shift"] = d.get("idx_shift", 0) + t0
            if not first:
                c["h0"] = d["h_all"][t0 - 1]
            return c
        if all(not d["reverse"] for d in scans) or True:
            fw = [d for d in scans if not d["reverse"]]
            if fw:
                ops.dw_x6 = True
                for d in fw:
                    d["h_all"].fill_(float("nan")); d["gates"].fill_(float("nan"))
                part = [chunk(d, 0, T1, True) for d in fw]
                for c, hb in zip(part, hand):
                    c["h_last_frag"] = hb
                assert ops.gru_fwd_x6_ok(part)
                ops.gru_seq_fwd(part, x6=True)
                part = [chunk(d, T1, T, False) for d in fw]
                for c, hb in zip(part, hand):
                    c["h0_frag"] = hb
                ops.gru_seq_fwd(part, x6=True)
                torch.cuda.synchronize()
                for d in fw:
                    i = scans.index(d)
                    assert torch.equal(d["h_all"], got[i]) and torch.equal(d["gates"], got[len(scans) + i])      # chunked == one launch, bit for bit
        scans[0]["gates"] = None                               # not eligible (no saved gates): falls back to the default kernels, bit for bit
        ops.dw_x6 = _x6_default()
        ops.gru_seq_fwd(scans); torch.cuda.synchronize()
        ref = [d["h_all"].clone() for d in scans]
        ops.dw_x6 = True
        ops.gru_seq_fwd(scans); torch.cuda.synchronize()
        assert all(torch.equal(a, d["h_all"]) for a, d in zip(ref, scans))
    finally:
        ops.dw_x6, ops.variant = _x6_default(), 0


@pytest.mark.parametrize("n,B,Ts", [(4, 256, (7, 7, 7, 7)), (4, 256, (2, 9, 5, 3)), (2, 256, (6, 4)), (3, 128, (5, 8, 3)), (2, 512, (4, 4))])
def test_backward_scan_bf16x6(ops, n, B, Ts):
    """the backward scan with exact split products on the bf16 MFMA (FnGruBwd.variant | FN_GRU_BF16X6: gate gradients exchanged as bf16 triples, W_hh^T as a
    triple image, gru_bwd_x6_kernel) against the default register-stationary fp32 kernel on the SAME saved activations at H = 512: gate gradients,
    dL/dh0 and the per-sequence row sums agree to fp32 rounding (exact products, another summation order); 64-row groups (4 x 256 rows: 16
    groups) and 32-row groups (2 x 256, 3 x 128, 2 x 512 rows), scans of different lengths in one launch, with / without dh_last, dh_ext, h0, dh0;
    repeated launches on warm slabs are bit-identical; the sync-error word stays clear"""
    from music_fader_nets_amd import _lib
    H, V = 512, 57
    torch.manual_seed(n * 1000 + B)
    fwd, bwd = [], []
    for s_ in range(n):
        T = Ts[s_]
        w = (torch.randn(3 * H, H, device=DEV) / (H ** 0.5)).contiguous()
        wf = torch.zeros(ops.frag_floats(3 * H, H), device=DEV); ops.frag_pack(w, wf)
        wt = torch.zeros(ops.frag_floats(H, 3 * H), device=DEV)
        wt3 = torch.zeros(ops.frag_floats(H, 3 * H) * 3 // 2, device=DEV)
        ops.weight_images([("frag_t", w, wt), ("frag3_t", w, wt3)])
        wt3_ref = torch.zeros_like(wt3)
        ops.frag3_pack(w.t().contiguous(), wt3_ref)                  # the transposing job == the plain pack of the transposed matrix
        assert torch.equal(wt3, wt3_ref)
        h0 = torch.randn(B, H, device=DEV) * 0.3 if s_ % 2 == 0 else None
        f = dict(B=B, T=T, H=H, w_hh_frag=wf, b_hh=torch.randn(3 * H, device=DEV) * 0.1, b_ih=torch.randn(3 * H, device=DEV) * 0.1, h0=h0,
                 gx_dense=torch.randn(T, B, 3 * H, device=DEV) * 0.5, h_all=torch.zeros(T, B, H, device=DEV), gates=torch.zeros(T, ops.gates_floats(B, H), device=DEV))
        fwd.append(f)
        bwd.append(dict(B=B, T=T, H=H, w_hh_t_frag=wt, w_hh_t_frag3=wt3, h0=h0, h_all=f["h_all"], gates=f["gates"],
                        dh_last=torch.randn(B, H, device=DEV) if s_ != 1 else None, dh_ext=torch.randn(T, B, H, device=DEV) * 0.5 if s_ != 0 else None,
                        dgx_all=torch.zeros(T, B, 3 * H, device=DEV), dghn_all=torch.zeros(T, B, H, device=DEV),
                        dh0=torch.zeros(B, H, device=DEV) if s_ != 2 else None, dgx_rowsum=torch.zeros(B, 3 * H, device=DEV),
                        dghn_rowsum=torch.zeros(B, H, device=DEV) if s_ != 3 else None, scratch=torch.zeros(B, H, device=DEV)))
    ops.gru_seq_fwd(fwd)
    keys = ("dgx_all", "dghn_all", "dh0", "dgx_rowsum", "dghn_rowsum")

    def run(x6):
        ops.dw_x6 = x6
        ops.variant = _lib.GRU_X6_BWD_32ROWS if x6 else 0  # the 32-row-group form too (not chosen on its own: no faster than the fp32 kernel)
        for b in bwd:
            for k in keys:
                if b[k] is not None:
                    b[k].zero_() if "rowsum" in k else b[k].fill_(float("nan"))
        if x6:
            assert ops.gru_bwd_x6_ok(bwd)
        ops.gru_seq_bwd(bwd)
        torch.cuda.synchronize()
        ops.variant = 0
        return [[None if b[k] is None else b[k].clone() for k in keys] for b in bwd]
    try:
        ref = run(False)
        got = run(True)
        again = run(True)
        assert not ops.gru_sync_error()
        differs = False
        for i, (rs_, gs_, as_) in enumerate(zip(ref, got, again)):
            for k, a, b, c in zip(keys, rs_, gs_, as_):
                if a is None:
                    continue
                assert not torch.isnan(b).any(), (i, k)
                assert torch.equal(b, c), (i, k)
                differs |= not torch.equal(a, b)
                assert float((a - b).abs().max()) <= 5e-5 * float(a.abs().max()), (i, k, float((a - b).abs().max()), float(a.abs().max()))
        assert differs                                     # the x6 kernel really ran
    finally:
        ops.dw_x6, ops.variant = _x6_default(), 0


@pytest.mark.parametrize("x6", [False, True])
@pytest.mark.parametrize("n,B,T", [(2, 256, 12), (4, 256, 9)])
def test_scan_results_do_not_depend_on_the_xcd_placement(ops, n, B, T, x6):
    """the weight-stationary scans deal their workgroups so that a row group (its exchange slab, its arrival counters) sits on ONE XCD - speed
    only: with FnGruFwd / FnGruBwd.variant | FN_GRU_SPREAD_XCDS the slices of every row group are spread over all 8 XCDs and every hand-over crosses
    XCDs; forward states, saved gates, gate gradients and row sums must come out bit-identical (ping-pong forward on both arithmetics,
    register-stationary backward with 32- and 64-row groups, the bf16 x 6 backward), the sync-error word clear"""
    from music_fader_nets_amd import _lib
    H = 512
    torch.manual_seed(77 + n)
    fwd, bwd = [], []
    for s_ in range(n):
        w = (torch.randn(3 * H, H, device=DEV) / (H ** 0.5)).contiguous()
        wf = torch.zeros(ops.frag_floats(3 * H, H), device=DEV)
        wf3 = torch.zeros(ops.frag_floats(3 * H, H) * 3 // 2, device=DEV)
        wt = torch.zeros(ops.frag_floats(H, 3 * H), device=DEV)
        wt3 = torch.zeros(ops.frag_floats(H, 3 * H) * 3 // 2, device=DEV)
        ops.weight_images([("frag", w, wf), ("frag3", w, wf3), ("frag_t", w, wt), ("frag3_t", w, wt3)])
        h0 = torch.randn(B, H, device=DEV) * 0.3
        f = dict(B=B, T=T, H=H, w_hh_frag=wf, w_hh_frag3=wf3, b_hh=torch.randn(3 * H, device=DEV) * 0.1, b_ih=torch.randn(3 * H, device=DEV) * 0.1, h0=h0,
                 gx_dense=torch.randn(T, B, 3 * H, device=DEV) * 0.5, h_all=torch.zeros(T, B, H, device=DEV), gates=torch.zeros(T, ops.gates_floats(B, H), device=DEV))
        fwd.append(f)
        bwd.append(dict(B=B, T=T, H=H, w_hh_t_frag=wt, w_hh_t_frag3=wt3, h0=h0, h_all=f["h_all"], gates=f["gates"], dh_last=torch.randn(B, H, device=DEV),
                        dh_ext=torch.randn(T, B, H, device=DEV) * 0.5, dgx_all=torch.zeros(T, B, 3 * H, device=DEV), dghn_all=torch.zeros(T, B, H, device=DEV),
                        dh0=torch.zeros(B, H, device=DEV), dgx_rowsum=torch.zeros(B, 3 * H, device=DEV), dghn_rowsum=torch.zeros(B, H, device=DEV),
                        scratch=torch.zeros(B, H, device=DEV)))
    fk, bk = ("h_all", "gates"), ("dgx_all", "dghn_all", "dh0", "dgx_rowsum", "dghn_rowsum")

    def run(variant):
        ops.dw_x6, ops.variant = x6, variant
        for f in fwd:
            f["h_all"].fill_(float("nan"))
        ops.gru_seq_fwd(fwd)
        out = [f[k].clone() for f in fwd for k in fk]
        for b in bwd:
            for k in bk:
                b[k].zero_() if "rowsum" in k else b[k].fill_(float("nan"))
        ops.gru_seq_bwd(bwd)
        torch.cuda.synchronize()
        return out + [b[k].clone() for b in bwd for k in bk]
    try:
        ref, spread = run(0), run(_lib.GRU_SPREAD_XCDS)
        assert not ops.gru_sync_error()
        for i, (a, b) in enumerate(zip(ref, spread)):
            assert not torch.isnan(b).any(), i
            assert torch.equal(a, b), i
    finally:
        ops.dw_x6, ops.variant = _x6_default(), 0


@pytest.mark.parametrize("lo,hi", [(-100, 60), (-120, -90), (-30, 30)])
@pytest.mark.parametrize("K,splitk", [(65536, 16), (4096, 4)])
def test_bf16x6_adversarial_operands_vs_float64(ops, lo, hi, K, splitk):
    """the bf16 x 6 product against float64 on operands chosen to hurt it: magnitudes spread over 2^lo .. 2^hi (per k the exponents of a and b are
    tied so that the PRODUCTS stay within 2^-20 .. 2^20 - the sum must not overflow -, i.e. tiny a meet huge b: every piece of the split
    travels the full exponent range; (-120, -90): lo pieces of values below 2^-103 are subnormal as bf16), heavy cancellation (every
    product has a partner of opposite sign that differs in its last bits only, the exact sum is ~1e-7 of sum |a||b|), K = 65 536.  Bound:
    the error in units of sum |a||b| - maximum and root mean square over the 65 536 outputs - is at most 1.25 x the fp32-MFMA kernel's own."""
    M = N = 256
    g = torch.Generator(device="cpu").manual_seed(1000 * K + hi - lo)
    half = K // 2
    ea = torch.randint(lo, hi + 1, (half, 1), generator=g).double()
    ma = 1.0 + torch.rand(half, M, generator=g, dtype=torch.float64)
    sa = torch.where(torch.rand(half, M, generator=g) < 0.5, -1.0, 1.0).double()
    a = (sa * ma * torch.pow(torch.tensor(2.0, dtype=torch.float64), ea)).float()
    eb = -ea + torch.randint(-20, 21, (half, 1), generator=g).double()
    eb = eb.clamp(-126 + 24, 120)
    mb = 1.0 + torch.rand(half, N, generator=g, dtype=torch.float64)
    b = (torch.where(torch.rand(half, N, generator=g) < 0.5, -1.0, 1.0).double() * mb * torch.pow(torch.tensor(2.0, dtype=torch.float64), eb)).float()
    # partners: -a (1 + a few ulps), same b  -> pairwise the products cancel to ~2^-22 of their size
    jitter = 1.0 + torch.randint(-3, 4, (half, M), generator=g).double() * 2.0 ** -23
    a2 = (-(a.double() * jitter)).float()
    perm = torch.randperm(K, generator=g)
    A = torch.cat([a, a2], 0)[perm].contiguous().to(DEV)
    Bm = torch.cat([b, b], 0)[perm].contiguous().to(DEV)
    assert torch.isfinite(A).all() and torch.isfinite(Bm).all()
    ref = A.double().t() @ Bm.double()
    scale = A.double().abs().t() @ Bm.double().abs()
    assert float((ref.abs() / scale).median()) < 1e-5          # heavy cancellation indeed
    err, rms = {}, {}
    try:
        for x6 in (False, True):
            ops.dw_x6 = x6
            C = torch.full((M, N), float("nan"), device=DEV)
            ops.gemm(A, Bm, C, a_k=False, b_k=False, splitk=splitk)
            e = (C.double() - ref).abs() / scale
            err[x6], rms[x6] = float(e.max()), float((e * e).mean().sqrt())
    finally:
        ops.dw_x6 = _x6_default()
    print("bf16x6 adversarial 2^%d..2^%d K=%d: max err / sum|a||b| fp32 %.3e x6 %.3e (x %.2f), rms fp32 %.3e x6 %.3e (x %.2f)"
          % (lo, hi, K, err[False], err[True], err[True] / err[False], rms[False], rms[True], rms[True] / rms[False]))
    # Measured (round 5, profiles/r05_bf16x6_adversarial.txt): the bf16 x 6 error is 1.0 - 1.45 x the fp32-MFMA kernel's in this setting (both are
    # 1e-8 .. 1e-7 of sum |a||b|, a fraction of an fp32 ulp of that sum); the review's 1.25 x is met by the maximum in most cases and not by
    # the root mean square.  With rounded pieces the DROPPED products are zero-mean and ~2^-26 |a b| each - what remains is how a
    # 16x16x32 MFMA adds its 32 exact products (one rounding per MFMA, addends aligned to the largest) against 32 chained fp32 FMAs.
    # Round 6 (128 x 256 tiles, twice the K ranges - same products, 32 instead of 16 partial sums): 0.79 - 1.11 x in all six cases (profiles/r06_bf16x6_adversarial.txt):
    # the bar is the round-4 review's 1.25 x again
    assert rms[True] <= 1.25 * rms[False] + 2.0 ** -32, (lo, hi, K, rms, err)
    assert err[True] <= 1.25 * err[False] + 2.0 ** -30, (lo, hi, K, err)
    assert err[True] < 2e-6, err


def _block_gates(gt, B, H, n_floats):
    """[T][B][4][H] -> the HIP kernels' private gate layout (inverse of _unblock_gates)"""
    T = gt.shape[0]
    nrt = (B + 15) // 16
    b = torch.arange(B).view(B, 1, 1)
    q = torch.arange(4).view(1, 4, 1)
    u = torch.arange(H).view(1, 1, H)
    off = ((((u // 16) * nrt + (b // 16)) * 4 + q) * 4 + (b % 4)) * 64 + ((b % 16) // 4) * 16 + (u % 16)
    g = torch.zeros(T, n_floats, dtype=gt.dtype, device=gt.device)
    g[:, off.reshape(-1).to(gt.device)] = gt.reshape(T, -1)
    return g


def _adversarial_pairs(rows, K, lo, hi, gen):
    """[rows][K] x [cols = rows][K] operand pair as in test_bf16x6_adversarial_operands_vs_float64, along K: magnitudes spread over 2^lo .. 2^hi with the
    partner's exponent tied (products within 2^-10 .. 2^10), every product with a partner of opposite sign that differs in its last bits"""
    half = K // 2
    ea = torch.randint(lo, hi + 1, (1, half), generator=gen).double()
    a = (torch.where(torch.rand(rows, half, generator=gen) < 0.5, -1.0, 1.0).double() * (1.0 + torch.rand(rows, half, generator=gen, dtype=torch.float64)) * 2.0 ** ea).float()
    eb = -ea + torch.randint(-10, 11, (1, half), generator=gen).double()
    b = (torch.where(torch.rand(rows, half, generator=gen) < 0.5, -1.0, 1.0).double() * (1.0 + torch.rand(rows, half, generator=gen, dtype=torch.float64)) * 2.0 ** eb).float()
    a2 = (-(a.double() * (1.0 + torch.randint(-3, 4, (rows, half), generator=gen).double() * 2.0 ** -23))).float()
    perm = torch.randperm(K, generator=gen)
    return torch.cat([a, a2], 1)[:, perm].contiguous(), torch.cat([b, b], 1)[:, perm].contiguous()


@pytest.mark.parametrize("n,lo,hi", [(4, -30, 10), (2, -30, 10), (4, -6, 6)])
def test_bf16x6_forward_scan_adversarial_operands_vs_float64(ops, n, lo, hi):
    """review r5: the bf16 x 6 SCANS had no adversarial test.  The forward scan saves W_hn h_{t-1} + b_hn - a RAW product of its recurrent GEMM - with the gates
    (slot 3 of the saved gates): step 0 of a scan started from an initial state h0 therefore exposes h0 W_hn^T.  h0 and W_hn are the adversarial pair of the
    GEMM test along K = 512 (magnitudes over 2^lo .. 2^hi, every product with a cancelling partner); the error against float64 in units of sum |h||w| must be
    within 1.6 x the fp32-MFMA scan's own (maximum and rms), on the 128-row-group kernel (n = 4: gru_fwd_x6pp_kernel<1>) and the 64-row-group one with its
    K split (n = 2: <2>).  Step 1 checks the same product on the state the kernel itself produced (|h| <= ~2^hi, no engineered cancellation)."""
    H, B, T = 512, 256, 2
    gen = torch.Generator(device="cpu").manual_seed(100 * n + hi - lo)
    scans, W, H0 = [], [], []
    for s_ in range(n):
        h0, whn = _adversarial_pairs(max(B, H), H, lo, hi, gen)
        h0, whn = h0[:B].contiguous(), whn[:H].contiguous()
        w = torch.cat([torch.randn(2 * H, H, generator=gen) / H ** 0.5, whn], 0).contiguous().to(DEV)
        wf = torch.zeros(ops.frag_floats(3 * H, H), device=DEV); ops.frag_pack(w, wf)
        wf3 = torch.zeros(ops.frag_floats(3 * H, H) * 3 // 2, device=DEV); ops.frag3_pack(w, wf3)
        scans.append(dict(B=B, T=T, H=H, reverse=0, w_hh_frag=wf, w_hh_frag3=wf3, b_hh=torch.zeros(3 * H, device=DEV), b_ih=torch.zeros(3 * H, device=DEV), h0=h0.to(DEV),
                          gx_dense=torch.zeros(T, B, 3 * H, device=DEV), h_all=torch.zeros(T, B, H, device=DEV), gates=torch.zeros(T, ops.gates_floats(B, H), device=DEV)))
        W.append(w[2 * H:].double()); H0.append(h0.to(DEV).double())
    err = {}
    try:
        for x6 in (False, True):
            ops.dw_x6 = x6
            if x6:
                assert ops.gru_fwd_x6_ok(scans)
            ops.gru_seq_fwd(scans)
            torch.cuda.synchronize()
            assert not ops.gru_sync_error()
            e0, e1 = [], []
            for d, w, h0 in zip(scans, W, H0):
                ghn = _unblock_gates(d["gates"].cpu(), B, H)[:, :, 3, :].to(DEV).double()
                for t, hin, acc in ((0, h0, e0), (1, d["h_all"][0].double(), e1)):
                    ref, scale = hin @ w.t(), hin.abs() @ w.abs().t()
                    if t == 0:
                        assert float((ref.abs() / scale).median()) < 1e-4          # heavy cancellation indeed
                    acc.append(((ghn[t] - ref).abs() / scale).flatten())
            e0, e1 = torch.cat(e0), torch.cat(e1)
            err[x6] = (float(e0.max()), float((e0 * e0).mean().sqrt()), float(e1.max()), float((e1 * e1).mean().sqrt()))
    finally:
        ops.dw_x6 = _x6_default()
    print("x6 forward scan adversarial n=%d 2^%d..2^%d: step 0 max / rms fp32 %.3e %.3e x6 %.3e %.3e; step 1 fp32 %.3e %.3e x6 %.3e %.3e" % ((n, lo, hi) + err[False][:2] + err[True][:2] + err[False][2:] + err[True][2:]))
    for i in range(4):
        assert err[True][i] <= 1.6 * err[False][i] + 2.0 ** -30, (i, err)
    assert err[True][0] < 2e-6 and err[True][2] < 2e-6, err


def test_bf16x6_backward_scan_wide_operands_vs_float64(ops):
    """the backward scan's recurrent product dh = [dr' dz' | dn' r] W_hh on bf16 x 6 (gru_bwd_x6_kernel<2>, the encoder shape) against float64: with z = 0 in
    the saved gates of step 0 the gradient wrt the initial state IS that product of the gate gradients the kernel itself wrote (dgx_all / dghn_all of step 0:
    exact fp32 operands, magnitudes spread over ~2^40 by the incoming gradient's scales), so dh0 can be checked against a float64 evaluation - error in
    units of sum |dg||w| within 1.6 x the fp32 kernel's own"""
    H, B, T, n = 512, 256, 2, 4
    gen = torch.Generator(device="cpu").manual_seed(77)
    bwd, W = [], []
    for s_ in range(n):
        w = (torch.randn(3 * H, H, generator=gen) * 2.0 ** torch.randint(-12, 5, (3 * H, 1), generator=gen).float()).contiguous().to(DEV)
        wt = torch.zeros(ops.frag_floats(H, 3 * H), device=DEV)
        wt3 = torch.zeros(ops.frag_floats(H, 3 * H) * 3 // 2, device=DEV)
        ops.weight_images([("frag_t", w, wt), ("frag3_t", w, wt3)])
        gt = torch.rand(T, B, 4, H, generator=gen)
        gt[:, :, 2] = gt[:, :, 2] * 2 - 1                  # n in (-1, 1)
        gt[:, :, 3] = torch.randn(T, B, H, generator=gen)  # W_hn h + b_hn
        gt[0, :, 1] = 0.0                                  # z = 0 at step 0: nothing of dh flows past the gates into dh0
        gates = _block_gates(gt, B, H, ops.gates_floats(B, H)).to(DEV)
        scale_u = 2.0 ** torch.randint(-25, 15, (1, H), generator=gen).float()
        bwd.append(dict(B=B, T=T, H=H, w_hh_t_frag=wt, w_hh_t_frag3=wt3, h0=(torch.rand(B, H, generator=gen) * 2 - 1).to(DEV),
                        h_all=(torch.rand(T, B, H, generator=gen) * 2 - 1).to(DEV), gates=gates, dh_last=(torch.randn(B, H, generator=gen) * scale_u).to(DEV), dh_ext=None,
                        dgx_all=torch.zeros(T, B, 3 * H, device=DEV), dghn_all=torch.zeros(T, B, H, device=DEV), dh0=torch.zeros(B, H, device=DEV),
                        dgx_rowsum=torch.zeros(B, 3 * H, device=DEV), dghn_rowsum=torch.zeros(B, H, device=DEV), scratch=torch.zeros(B, H, device=DEV)))
        W.append(w.double())
    err = {}
    try:
        for x6 in (False, True):
            ops.dw_x6 = x6
            if x6:
                assert ops.gru_bwd_x6_ok(bwd)
            for b in bwd:
                b["dgx_rowsum"].zero_(); b["dghn_rowsum"].zero_()
            ops.gru_seq_bwd(bwd)
            torch.cuda.synchronize()
            assert not ops.gru_sync_error()
            es = []
            for b, w in zip(bwd, W):
                dg = torch.cat([b["dgx_all"][0][:, :2 * H], b["dghn_all"][0]], 1).double()
                ref, scale = dg @ w, dg.abs() @ w.abs()
                assert torch.isfinite(ref).all() and float(scale.min()) > 0
                es.append(((b["dh0"].double() - ref).abs() / scale).flatten())
            e = torch.cat(es)
            err[x6] = (float(e.max()), float((e * e).mean().sqrt()))
    finally:
        ops.dw_x6 = _x6_default()
    print("x6 backward scan wide operands: max / rms error in units of sum |dg||w|: fp32 %.3e %.3e  x6 %.3e %.3e" % (err[False] + err[True]))
    assert err[True][0] <= 1.6 * err[False][0] + 2.0 ** -30 and err[True][1] <= 1.6 * err[False][1] + 2.0 ** -32, err
    assert err[True][0] < 2e-6, err


@pytest.mark.parametrize("B,T,Tr,fill", [(64, 33, 9, True), (128, 65, 33, True), (1024, 96, 8, False), (192, 64, 16, True)])
def test_bf16x6_is_decided_once_per_decoder_pipeline(B, T, Tr, fill):
    """the chunks of the decoder pipeline hand their state from launch to launch as operand images whose layout depends on the
    arithmetic (bf16 triples / fp32 fragments), and single launches can be ineligible for the bf16 x 6 kernels - a one-step tail chunk
    (T % 32 == 1, Tr % 32 == 1), more row groups than compute units in the two-scan launches (B = 1024 without the edge fill: launches 0, 1
    hold one scan, the others two).  The engine asks for every launch first and runs the WHOLE pipeline on one arithmetic: loss and
    gradients with set_arith("bf16x6") must agree with the fp32-MFMA step to rounding, never to garbage."""
    pkg = load_package()
    from music_fader_nets_amd.synth import synth_batch
    m = make_model(512, 32, device=DEV)
    tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
    b = synth_batch(np.random.RandomState(3), B, T, Tr)
    batch = tr.prepare_batch(b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
    torch.manual_seed(7)
    eps = tr.draw_eps(B, T)
    out = {}
    for ar in ("f32", "bf16x6"):
        m.set_arith(ar)
        m.engine().fill_edges = fill
        tup = tr.loss_and_grads(20000, batch, eps)
        assert not m.engine().ops.gru_sync_error()
        out[ar] = (tup, {k: tr.flat.G[k].clone() for k in ("grucell_g.weight_hh", "grucell_g_2.weight_hh", "gru_d_r.weight_hh_l0", "gru_r.weight_hh_l0", "linear_out_g.weight")},
                   m.engine().saved["dec"]["hx1"].clone())
    np.testing.assert_allclose(out["bf16x6"][0], out["f32"][0], rtol=2e-5)
    assert float((out["bf16x6"][2] - out["f32"][2]).abs().max()) <= 1e-4 * float(out["f32"][2].abs().max())
    for k, g32 in out["f32"][1].items():
        g6 = out["bf16x6"][1][k]
        assert torch.isfinite(g6).all()
        assert float((g6 - g32).abs().max()) <= 2e-4 * float(g32.abs().max()), (k, float((g6 - g32).abs().max()), float(g32.abs().max()))


def test_time_sum(ops):
    torch.manual_seed(4)
    X = torch.randn(67, 37, 96)
    out = torch.zeros(37, 96, device=DEV)
    ops.time_sum(g(X), out)
    close(out, X.double().sum(0).float(), 2e-6)


def test_embed_grad_full_vocab(ops):
    torch.manual_seed(8)
    T, B, N3, V = 33, 130, 200, 342
    dgx = torch.randn(T, B, N3)
    idx = torch.randint(0, V, (B, T), dtype=torch.int32)
    idx[:, T // 2:] = 0                                        # heavy padding token, like real batches
    ref, out = torch.zeros(V, N3), torch.zeros(V, N3, device=DEV)
    FakeOps().embed_grad(dgx, idx, 0, 0, 0, V, ref)
    ops.embed_grad(g(dgx), g(idx), 0, 0, 0, V, out)
    close(out, ref, 2e-5)
    out2 = torch.zeros(V, N3, device=DEV)
    ops.embed_grad(g(dgx), g(idx), 0, 0, 0, V, out2)
    assert torch.equal(out, out2)                  # deterministic: sorted segments, no float atomics
    # reverse direction and decoder shift (start token at tau < 0), tokens absent from the batch -> zero rows
    idx2 = torch.randint(5, 40, (B, T), dtype=torch.int32)
    for rev, shift, start in ((1, 0, 0), (0, -1, 341)):
        ref, out = torch.zeros(V, N3), torch.zeros(V, N3, device=DEV)
        FakeOps().embed_grad(dgx, idx2, shift, start, rev, V, ref)
        ops.embed_grad(g(dgx), g(idx2), shift, start, rev, V, out)
        close(out, ref, 2e-5)
        assert float(out[100].abs().max()) == 0.0
    # one sort, several scans per launch, tables written TRANSPOSED into a wider matrix (dW_ih[:, :V] in place)
    for Bx, Tx in ((130, 33), (256, 70), (3, 5)):
        dg = [torch.randn(Tx, Bx, N3) for _ in range(3)]
        ix = torch.randint(0, V, (Bx, Tx), dtype=torch.int32)
        ix[:, Tx // 2:] = 0
        h = ops.token_sort(g(ix), V)
        dW = [torch.full((N3, V + 10), 7.0, device=DEV) for _ in range(3)]
        cfg = [dict(reverse=0), dict(reverse=1), dict(idx_shift=-1, start_token=V - 1)]
        ops.embed_grad_sorted(h, [dict(dgx=g(dg[i]), out=dW[i][:, :V], transposed=True, **cfg[i]) for i in range(3)])
        for i in range(3):
            ref = torch.zeros(V, N3)
            FakeOps().embed_grad(dg[i], ix, cfg[i].get("idx_shift", 0), cfg[i].get("start_token", 0), cfg[i].get("reverse", 0), V, ref)
            close(dW[i][:, :V].t(), ref, 2e-5, "sorted job %d (%d x %d)" % (i, Bx, Tx))
            assert float((dW[i][:, V:] - 7.0).abs().max()) == 0.0          # columns beyond V untouched


def test_head_kernels(ops):
    fake = FakeOps()
    torch.manual_seed(11)
    B, T, E = 9, 7, 342
    logits = torch.randn(T * B, 344) * 3
    target = torch.randint(0, E, (B, T), dtype=torch.int32)
    lp_c, nll_c, dl_c = torch.zeros(B, T, E), torch.zeros(T * B), torch.zeros(T * B, 344)
    fake.vocab_logsoftmax(logits, B, T, E, lp_c, target, nll_c, 0.37, dl_c)
    ld = g(logits)
    lp_d, nll_d = torch.zeros(B, T, E, device=DEV), torch.zeros(T * B, device=DEV)
    ops.vocab_logsoftmax(ld, B, T, E, lp_d, g(target), nll_d, 0.37, ld)       # dlogits in place
    close(lp_d, lp_c), close(nll_d, nll_c), close(ld[:, :E], dl_c[:, :E], 2e-5)
    gout = torch.randn(B, T, E)
    d1c, d1d = torch.zeros(T * B, 344), torch.zeros(T * B, 344, device=DEV)
    fake.vocab_logsoftmax_bwd(lp_c, gout, d1c)
    ops.vocab_logsoftmax_bwd(lp_d, g(gout), d1d)
    close(d1d[:, :E], d1c[:, :E], 2e-5)
    # time axis (Tr <= 64: one wavefront per column, lane = time step; longer: the loop kernel; 3 classes = the rhythm decoder's width)
    for Tr, Cc in ((64, 3), (33, 16), (70, 5), (8, 16)):
        lg = torch.randn(Tr, B, Cc) * 2
        tg = torch.randint(0, Cc, (B, Tr), dtype=torch.int32)
        lpc, nc, dc = torch.zeros(B, Tr, Cc), torch.zeros(B, Cc), torch.zeros(Tr, B, Cc)
        lpd, nd, dd = (torch.zeros_like(x, device=DEV) for x in (lpc, nc, dc))
        fake.time_logsoftmax(lg, lpc, tg, nc, 0.11, dc)
        ops.time_logsoftmax(g(lg), lpd, g(tg), nd, 0.11, dd)
        close(lpd, lpc), close(nd, nc), close(dd, dc, 2e-5)
        lp_only = torch.zeros_like(lpd)
        ops.time_logsoftmax(g(lg), logp_bt=lp_only)             # eval form: no target, no gradient
        assert torch.equal(lp_only, lpd)
    go = torch.randn(B, Tr, Cc)
    d2c, d2d = torch.zeros(Tr, B, Cc), torch.zeros(Tr, B, Cc, device=DEV)
    fake.time_logsoftmax_bwd(lpc, go, d2c)
    ops.time_logsoftmax_bwd(lpd, g(go), d2d)
    close(d2d, d2c, 2e-5)
    # greedy head incl. exact ties -> first index
    lg2 = torch.randn(13, 344)
    lg2[3, 100] = lg2[3, 200] = 50.0
    lg2[5, 0] = lg2[5, 341] = 60.0
    tok = torch.zeros(13, 4, dtype=torch.int32, device=DEV)
    lp2 = torch.zeros(13, 4, E, device=DEV)
    ops.vocab_argmax(g(lg2), E, lp2[:, 2, :], tok[:, 2])
    assert torch.equal(tok[:, 2].cpu().long(), lg2[:, :E].max(1)[1])
    assert int(tok[3, 2]) == 100 and int(tok[5, 2]) == 0
    close(lp2[:, 2, :], torch.log_softmax(lg2[:, :E].double(), -1).float())


@pytest.mark.parametrize("sup", [False, True])
def test_latent_kernels(ops, sup):
    fake = FakeOps()
    torch.manual_seed(21)
    B, Z, K = 11, 128, 2
    pre = torch.randn(B, 2 * Z) * 0.3
    eps = torch.randn(B, Z)
    mu_lk = torch.randn(K, Z) * 0.2
    lv_lk = torch.full((K, Z), -4.0) + torch.randn(K, Z) * 0.01
    labels = torch.randint(0, K, (B,), dtype=torch.int32) if sup else None
    names = ("sigma", "z", "ll", "qy", "y", "terms")
    oc = dict(sigma=torch.zeros(B, Z), z=torch.zeros(B, Z), ll=torch.zeros(B, K), qy=torch.zeros(B, K),
              y=torch.zeros(B, dtype=torch.int32), terms=torch.zeros(B, 4))
    od = {k: g(v.clone()) for k, v in oc.items()}
    fake.latent_fwd(pre, eps, mu_lk, lv_lk, labels, *[oc[k] for k in names])
    ops.latent_fwd(g(pre), g(eps), g(mu_lk), g(lv_lk), g(labels), *[od[k] for k in names])
    for k in ("sigma", "z", "ll", "qy"):
        close(od[k], oc[k], 2e-5, k)
    assert torch.equal(od["y"].cpu(), oc["y"])
    cols = (0, 1, 2, 3) if sup else (0, 1)
    close(od["terms"][:, cols], oc["terms"][:, cols], 5e-5, "terms")
    ups = [torch.randn(B, Z), torch.randn(B, Z), torch.randn(B, Z), torch.randn(B, K), torch.randn(B, K)]
    w = (0.3, 0.0, 0.7) if sup else (0.3, 0.2, 0.0)
    dc, mc = torch.zeros(B, 2 * Z), torch.zeros(B, K * Z)
    dd, md = g(dc.clone()), g(mc.clone())
    w3 = torch.tensor(w)
    fake.latent_bwd(pre, eps, mu_lk, lv_lk, labels, oc["z"], oc["qy"], *ups, w3, dc, mc)
    ops.latent_bwd(g(pre), g(eps), g(mu_lk), g(lv_lk), g(labels), od["z"], od["qy"], *[g(u) for u in ups], g(w3), dd, md)
    close(dd, dc, 1e-4, "dpre")
    close(md, mc, 1e-4, "dmu_lk_rows")


def test_latent_kernel_saturated_posterior(ops):
    """q(y|x) underflows to exactly (1, 0) at initialisation (KL terms ~1500): gradients must stay finite."""
    torch.manual_seed(2)
    B, Z, K = 5, 128, 2
    pre, eps = torch.randn(B, 2 * Z) * 0.1, torch.randn(B, Z)
    mu_lk, lv_lk = torch.randn(K, Z) * 0.2, torch.full((K, Z), -4.0)
    o = [torch.zeros(B, Z, device=DEV), torch.zeros(B, Z, device=DEV), torch.zeros(B, K, device=DEV), torch.zeros(B, K, device=DEV),
         torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B, 4, device=DEV)]
    ops.latent_fwd(g(pre), g(eps), g(mu_lk), g(lv_lk), None, *o)
    assert float(o[3].min()) == 0.0                                # saturated
    dd, md = torch.zeros(B, 2 * Z, device=DEV), torch.zeros(B, K * Z, device=DEV)
    ops.latent_bwd(g(pre), g(eps), g(mu_lk), g(lv_lk), None, o[1], o[3], None, None, None, None, None, g(torch.tensor([0.1, 0.1, 0.0])), dd, md)
    assert bool(torch.isfinite(dd).all()) and bool(torch.isfinite(md).all())


def test_pairwise_and_adam_kernels(ops):
    fake = FakeOps()
    torch.manual_seed(31)
    n_all = 300
    z0 = torch.randn(n_all)
    attr = torch.randint(0, 17, (n_all,)).double() / 16.0            # many exact ties -> sign 0
    lc, gc = torch.zeros(100), torch.zeros(100)
    ld_, gd = torch.zeros(100, device=DEV), torch.zeros(100, device=DEV)
    fake.pairwise_reg(z0, attr, 150, 100, lc, 1e-3, gc)
    ops.pairwise_reg(g(z0), g(attr), 150, 100, ld_, 1e-3, gd)
    close(ld_, lc, 2e-5), close(gd, gc, 5e-5)
    n = 100003
    p, gr, m, v = torch.randn(n), torch.randn(n) * 3, torch.rand(n) * 0.1, torch.rand(n) * 0.01
    pc, mc, vc = p.clone(), m.clone(), v.clone()
    pd, md, vd = g(p.clone()), g(m.clone()), g(v.clone())
    ssc = torch.zeros(1)
    fake.sumsq(gr, ssc)
    # step-dependent scalars come from the device-resident counters (fn_step_params)
    cnt_c, cnt_d = torch.tensor([12345, 6], dtype=torch.int64), torch.tensor([12345, 6], dtype=torch.int64, device=DEV)
    sp_c, sp_d = torch.zeros(8), torch.zeros(8, device=DEV)
    fake.step_params(cnt_c, 0.2, 1e-3, 0.9, 0.999, False, 1.0 / 256, True, sp_c)
    ops.step_params(cnt_d, 0.2, 1e-3, 0.9, 0.999, False, 1.0 / 256, True, sp_d)
    assert cnt_d.tolist() == [12346, 7] == cnt_c.tolist()
    close(sp_d[:6], sp_c[:6], 2e-5)
    np.testing.assert_allclose(float(sp_d[5]), min((12345 - 10000) / 10000 * 0.2, 0.2), rtol=1e-6)
    fake.clip_adam(pc, gr, mc, vc, ssc, 1.0, sp_c[3:5], 0.9, 0.999, 1e-8)
    ops.clip_adam(pd, g(gr), md, vd, g(ssc), 1.0, sp_d[3:5], 0.9, 0.999, 1e-8)
    close(pd, pc, 1e-6), close(md, mc, 1e-5), close(vd, vc, 1e-5)


# ----------------------------------------------------------------------------------------------
# end to end against the golden fixtures (small: stored weights; c0: seeded H=512 weights)
# ----------------------------------------------------------------------------------------------
def _fw_check(res, gold, tol):
    (out, r_out, n_out, _, _), (dis_r, dis_n), (z_r, z_n), (ll_r, ll_n), (qy_r, qy_n), (y_r, y_n) = res
    got = dict(out=out, r_out=r_out, n_out=n_out, mu_r=dis_r.mean, sigma_r=dis_r.stddev, mu_n=dis_n.mean, sigma_n=dis_n.stddev,
               z_r=z_r, z_n=z_n, ll_r=ll_r, ll_n=ll_n, qy_r=qy_r, qy_n=qy_n)
    for k, v in got.items():
        np.testing.assert_allclose(v.detach().cpu().numpy(), gold["fw_" + k], rtol=tol, atol=tol, err_msg=k)
    assert np.array_equal(y_r.cpu().numpy(), gold["fw_y_r"]) and np.array_equal(y_n.cpu().numpy(), gold["fw_y_n"])
    return got


@pytest.mark.parametrize("case", ["small", "c0"])
def test_dropin_forward_backward_vs_reference(case, small, c0):
    gold = small if case == "small" else c0
    H, Z = int(gold["meta_dims"][0]), int(gold["meta_dims"][1])
    m = make_model(H, Z, sd_from(gold, "w0/") if case == "small" else None, device=DEV)
    pkg = load_package()
    b = batch_of(gold)
    d, r, n = (torch.from_numpy(b[k]).to(DEV) for k in ("d", "r", "n"))
    c = torch.from_numpy(b["c"]).to(DEV)
    eps = (torch.from_numpy(gold["eps_r"]).to(DEV), torch.from_numpy(gold["eps_n"]).to(DEV))
    res = m(pkg.convert_to_one_hot(d, 342), pkg.convert_to_one_hot(r, 3), pkg.convert_to_one_hot(n, 16), c, eps=eps)
    got = _fw_check(res, gold, 1e-4)
    # the reference's torch loss code on top of our outputs, then autograd through the fused node
    sd = {k: p for k, p in m.named_parameters()}
    got_cpu_free = {k: v for k, v in got.items()}
    import oracle.gmvae_oracle as o
    ls = o.loss_function(sd, got_cpu_free, d.long(), r.long(), n.long(), 20000, beta=0.2)
    zr, zn = got["z_r"], got["z_n"]
    l_r, l_n = [((torch.tanh(z[:, 0].reshape(-1, 1) - z[:, 0]) -
                  torch.sign(torch.from_numpy(np.subtract.outer(a, a)).float().to(DEV))) ** 2).mean()
                for z, a in ((zr, b["r_density"]), (zn, b["n_density"]))]
    loss = ls[0] + l_r + l_n
    np.testing.assert_allclose(float(loss.detach()), gold["total_loss_unsup_20000"][0], rtol=2e-5)
    loss.backward()
    sq = 0.0
    if case == "small":
        exact = oracle_grads_f64(gold, sd_from(gold, "w0/"))
        tol = grad_tolerances(gold, "unsup", exact)
    for k, p in m.named_parameters():
        if k.startswith(orc.UNUSED_PREFIXES) or k in orc.FROZEN:
            assert p.grad is None, k
            continue
        gcpu = p.grad.detach().cpu().double()
        sq += float((gcpu ** 2).sum())
        if case == "small":
            e = relerr(gcpu.numpy(), exact[k])
            assert e < tol[k] or np.abs(exact[k]).max() < 1e-6, (k, e, tol[k])
        else:
            ref = gold["gradsum_unsup/" + k]
            np.testing.assert_allclose(float(gcpu.abs().sum()), ref[1], rtol=5e-4, atol=1e-5, err_msg=k)
    np.testing.assert_allclose(math.sqrt(sq), gold["gradnorm_unsup_20000"][0], rtol=1e-3)
    if case == "c0":          # ... and every 16 x 32 block of every gradient against the float64 oracle (helpers_step.py)
        from helpers_step import c0_references, check_step_grads, cpu_state
        check_step_grads({k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}, c0_references(gold, cpu_state(m)))


@pytest.mark.parametrize("arith", ["f32", "bf16x6"])
@pytest.mark.parametrize("case,sup,chunk", [("small", False, 32), ("small", True, 32), ("small", False, 6), ("c0", False, 32), ("c0", False, 24)])
def test_fused_gradients_vs_reference(case, sup, chunk, arith, small, c0):
    gold = small if case == "small" else c0
    H, Z = int(gold["meta_dims"][0]), int(gold["meta_dims"][1])
    pkg = load_package()
    m = make_model(H, Z, sd_from(gold, "w0/") if case == "small" else None, device=DEV, arith=arith)
    tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
    m.engine().chunk = chunk                 # decoder-layer pipeline chunk (two HIP streams): results must not depend on it
    b = batch_of(gold)
    batch = tr.prepare_batch(b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"], b["a"] if sup else None)
    eps = (torch.from_numpy(gold["eps_r"]).to(DEV), torch.from_numpy(gold["eps_n"]).to(DEV))
    tup = tr.loss_and_grads(20000, batch, eps)
    tag = "sup" if sup else "unsup"
    np.testing.assert_allclose(tup[0], gold["total_loss_%s_20000" % tag][0], rtol=2e-5)
    if case == "small":
        exact = oracle_grads_f64(gold, sd_from(gold, "w0/"), sup)
        tol = grad_tolerances(gold, tag, exact)
    for k in tr.flat.names:
        gk = tr.flat.G[k].cpu().double()
        if case == "small":
            e = relerr(gk.numpy(), exact[k])
            assert e < tol[k] or np.abs(exact[k]).max() < 1e-6, (k, e, tol[k])
        else:
            ref = gold["gradsum_%s/%s" % (tag, k)]
            np.testing.assert_allclose(float(gk.abs().sum()), ref[1], rtol=5e-4, atol=1e-5, err_msg=k)
    np.testing.assert_allclose(tr.grad_norm(), gold["gradnorm_%s_20000" % tag][0], rtol=1e-3)
    if case == "c0":          # ... and every 16 x 32 block of every gradient against the float64 oracle (helpers_step.py)
        from helpers_step import c0_references, check_step_grads, cpu_state, flat_grads
        check_step_grads(flat_grads(tr), c0_references(gold, cpu_state(m), sup))


@pytest.mark.parametrize("arith", ["f32", "bf16x6"])
@pytest.mark.parametrize("case", ["small", "c0"])
def test_three_train_steps_vs_reference_train(case, arith, small, c0):
    """GMVAETrainer.train vs the reference's own train() (trainer_gmm.py:220-258), 3 steps from step 19999."""
    gold = small if case == "small" else c0
    H, Z = int(gold["meta_dims"][0]), int(gold["meta_dims"][1])
    pkg = load_package()
    m = make_model(H, Z, sd_from(gold, "w0/") if case == "small" else None, device=DEV, arith=arith)
    tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
    b = batch_of(gold)
    step = 19999
    for it in range(3):
        torch.manual_seed(99 + it)
        step, tup = tr.train(step, None, None, None, b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
        np.testing.assert_allclose(tup, gold["train_tuples"][it], rtol=5e-4, err_msg="step %d" % it)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    if case == "small":
        # Adam divides by |g|: an element whose gradient is ~noise moves by up to lr per step in a direction the reference
        # itself does not determine; 3 steps x lr = 3e-3 is the worst case, the bulk must agree to 1e-4.
        for k, v in sd_from(gold, "w3/").items():
            if k not in NOISE_PARAMS:
                diff = np.abs(sd[k].numpy() - v.numpy())
                assert float(diff.max()) <= 3.1e-3, k
                assert float((diff > 1e-4).mean()) < 2e-3, (k, float((diff > 1e-4).mean()))
    else:
        for k, v in sd.items():
            if k not in NOISE_PARAMS:
                vd = v.double()
                np.testing.assert_allclose([vd.abs().sum().item(), (vd * vd).sum().item()], gold["w3sum/" + k][1:], rtol=2e-5, err_msg=k)
    torch.manual_seed(123)
    ev = tr.evaluate(step - 1, None, None, None, b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
    np.testing.assert_allclose(ev, gold["eval_tuple"], rtol=5e-4)


def test_epoch_driver_vs_reference_training_phase(tmp_path):
    """the reference's training_phase (two epochs, supervised + unsupervised halves) on the HIP path: same log lines, same checkpoint"""
    from helpers import check_epoch_run
    g = load_golden("epoch")
    pkg = load_package()
    m = make_model(64, 32, device=DEV)
    saved = check_epoch_run(pkg, m, g, tmp_path, rtol=5e-4)
    for k, v in saved.items():
        if k not in NOISE_PARAMS:
            np.testing.assert_allclose(v.numpy(), g["wend/" + k], rtol=0, atol=1e-3, err_msg=k)
    assert not m.engine().ops.gru_sync_error()


def test_vae_sibling_vs_reference():
    """model_v2.MusicAttrRegVAE + trainer.py's step on the HIP path vs the reference run (tests/golden/vae.npz)"""
    from helpers import check_vae_against_reference, make_vae_model
    pkg = load_package()
    check_vae_against_reference(pkg, make_vae_model(64, 32, device=DEV), load_golden("vae"), DEV, rtol_fw=5e-5, tol_grad=5e-4,
                                rtol_tuple=5e-4, atol_w=1e-3)


@pytest.mark.parametrize("case", ["small", "c0"])
def test_greedy_decode_tokens(case, small, c0):
    gold = small if case == "small" else c0
    H, Z = int(gold["meta_dims"][0]), int(gold["meta_dims"][1])
    m = make_model(H, Z, sd_from(gold, "w0/") if case == "small" else None, device=DEV)
    m.eval()
    z = torch.from_numpy(gold["dec_z"]).to(DEV)
    steps = gold["dec_tokens"].shape[1]
    lp = m.global_decoder(z, steps)
    np.testing.assert_allclose(lp[:, 0].cpu().numpy(), gold["dec_logp_first"], rtol=1e-4, atol=1e-4)
    tok = lp.argmax(-1).cpu().numpy()
    ref, gap = gold["dec_tokens"], gold["dec_gap"]
    checked = 0
    for i in range(tok.shape[0]):
        tight = np.nonzero(gap[i] < 1e-4)[0]
        upto = int(tight[0]) if len(tight) else steps        # exact up to the first near-tie of the reference itself
        assert np.array_equal(tok[i, :upto], ref[i, :upto]), (i, upto)
        checked += upto
    assert checked >= 0.9 * tok.size
    pkg = load_package()
    d = torch.from_numpy(gold["d"]).to(DEV)
    c = torch.from_numpy(gold["c"]).to(DEV)
    eps = (torch.from_numpy(gold["eps_r"]), torch.from_numpy(gold["eps_n"]))
    tk, _ = pkg.fader_sweep(m, d, c, [0.75, -0.5], steps=steps, which="r", eps=eps)
    from helpers import tokens_match_upto_near_tie
    assert tokens_match_upto_near_tie(tk[:, 0].cpu().numpy(), ref, gap) >= 0.9 * ref.size      # full length, not a prefix


@pytest.mark.parametrize("path", ["pipeline", "cells"])
def test_batched_fader_sweep_vs_reference_decoder(path):
    """tests/golden/sweep.npz: the REFERENCE's eval-mode global_decoder (gmm_model.py:119-149, 73-80) on the (64, 280) batch that 8 samples x the 8
    fader values of test_class.py:84-85 make, hidden 512, 100 greedy steps - against the one-launch block pipeline (64 rows = two 32-row
    blocks) and against the per-token cells (fn_gru_cell_f32 + fn_out_argmax_f32, the path of thousands of rows): tokens bit-exact in every
    row up to the first position where the reference's own top-2 gap is below 1e-4, first-step log-probabilities to 1e-4"""
    g = load_golden("sweep")
    H, Z, K, NS, NV, steps = (int(x) for x in g["dims"])
    m = make_model(H, Z, device=DEV)
    for k, v in m.state_dict().items():                      # the seeded init IS the reference's (checksums of every tensor)
        vd = v.double()
        np.testing.assert_allclose([vd.sum().item(), vd.abs().sum().item(), (vd * vd).sum().item()], g["w0sum/" + k], rtol=1e-9, atol=1e-9, err_msg=k)
    m.eval()
    eng = m.engine()
    if path == "cells":
        eng.single_launch_decode, eng.cell_decode_rows = False, 1
    pkg = load_package()
    z = torch.from_numpy(g["z"]).to(DEV)
    lp, tok = pkg.greedy_decode(m, z, steps, want_logp=True)
    np.testing.assert_allclose(lp[:, 0].cpu().numpy(), g["logp_first"], rtol=1e-4, atol=1e-4)
    _, tok_only = pkg.greedy_decode(m, z, steps, want_logp=False)          # the tokens-only form (argmax in the output layer's epilogue on the cells path)
    from helpers import tokens_match_upto_near_tie
    for t in (tok, tok_only):
        assert tokens_match_upto_near_tie(t.cpu().numpy(), g["tokens"], g["gap"]) >= 0.9 * g["tokens"].size
    assert not eng.ops.gru_sync_error()


# ----------------------------------------------------------------------------------------------
# BASELINE size (B=256, T=256, Tr=64, H=512): size-independent properties
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Bi,steps", [(64, 1, 12), (64, 17, 30), (512, 3, 40), (512, 32, 25)])
def test_single_launch_decode_matches_per_token_kernels(H, Bi, steps, monkeypatch):
    """fn_decode_greedy (one launch, weight slices in LDS, five workgroup roles) vs the five-kernels-per-token path: same tokens,
    same log-probabilities; 1, 2 and 4 row tiles, H = 64 (4 slices per role) and 512 (32)."""
    pkg = load_package()
    m = make_model(H, 32 if H == 64 else 128, device=DEV, seed=7)
    m.eval()
    torch.manual_seed(3)
    z = torch.randn(Bi, 2 * m.latent_dim + 24, device=DEV)
    m.engine().single_launch_decode = False
    lp0, tk0 = pkg.greedy_decode(m, z, steps)
    m.engine().single_launch_decode = True
    lp1, tk1 = pkg.greedy_decode(m, z, steps)
    lp2, tk2 = pkg.greedy_decode(m, z, steps)                       # again on the warm buffers
    assert not m.engine().ops.gru_sync_error()
    assert torch.equal(tk1, tk2) and torch.equal(lp1, lp2)
    gap = lp0.topk(2, dim=-1).values
    clear = (gap[..., 0] - gap[..., 1]) > 1e-4                     # positions where the per-token path itself is not at a near-tie
    first_unclear = torch.where((~clear).any(0))[0]
    upto = int(first_unclear[0]) if len(first_unclear) else steps
    assert torch.equal(tk0[:, :upto], tk1[:, :upto])
    close(lp1[:, :upto], lp0[:, :upto], 2e-5)


@pytest.mark.parametrize("H,Bi,steps", [(64, 45, 20), (512, 64, 30), (512, 256, 25), (512, 400, 14), (512, 800, 12), (64, 1024, 9), (512, 1500, 6)])
def test_single_launch_decode_block_pipeline(H, Bi, steps):
    """fn_decode_greedy above 32 sequences: blocks of 32 rows (64 rows from 353 sequences on) travel through the role workgroups as a
    pipeline (two replicas of the role set at H = 512, more at H = 64 ... up to 12 blocks per replica, ragged last blocks of 13 / 16 / 28
    rows) - per row the tokens and log-probabilities of the per-token kernels up to that row's first near-tie, bit-reproducible on warm
    buffers, sync-error word clear."""
    pkg = load_package()
    m = make_model(H, 32 if H == 64 else 128, device=DEV, seed=13)
    m.eval()
    torch.manual_seed(4)
    z = torch.randn(Bi, 2 * m.latent_dim + 24, device=DEV)
    eng = m.engine()
    eng.single_launch_decode, eng.cell_decode_rows = False, 1 << 30
    lp0, tk0 = pkg.greedy_decode(m, z, steps)
    eng.single_launch_decode, eng.single_launch_rows, eng.single_launch_skip = True, 2048, (0, -1)       # force the one-launch pipeline whatever the default thresholds
    # what the docstring claims, from the library's plan for these tensors (fn_decode_plan on this device's compute units)
    from music_fader_nets_amd import decode as dec
    plan = dec.single_launch_plan(eng, Bi, steps)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = 64 if Bi >= 353 else 32
    assert plan is not None and plan["block_rows"] == rows and plan["nblk"] == -(-Bi // rows) and plan["nblk"] > 1, plan
    assert plan["per_rep"] == 3 * (H // 16) + 22 + 1 and plan["nrep"] == min(cus // plan["per_rep"], plan["nblk"]), (cus, plan)
    assert plan["nrep"] == (2 if H == 512 else min(7, plan["nblk"])) and plan["grid"] == plan["nrep"] * plan["per_rep"] <= cus, (cus, plan)      # 256 compute units
    assert Bi - (plan["nblk"] - 1) * rows == {45: 13, 64: 32, 256: 32, 400: 16, 800: 32, 1024: 64, 1500: 28}[Bi]                                 # rows of the last block
    assert -(-plan["nblk"] // plan["nrep"]) == {45: 1, 64: 1, 256: 4, 400: 4, 800: 7, 1024: 3, 1500: 12}[Bi]                                      # blocks per replica
    lp1, tk1 = pkg.greedy_decode(m, z, steps)
    lp2, tk2 = pkg.greedy_decode(m, z, steps)
    assert not eng.ops.gru_sync_error()
    assert torch.equal(tk1, tk2) and torch.equal(lp1, lp2)
    gap = lp0.topk(2, dim=-1).values
    unclear = ((gap[..., 0] - gap[..., 1]) <= 1e-4)
    first = torch.where(unclear.any(1), unclear.float().argmax(1), torch.full((Bi,), steps, device=DEV))
    keep = torch.arange(steps, device=DEV).view(1, -1) < first.view(-1, 1)
    assert bool(keep.float().mean() > 0.9)
    assert torch.equal(tk0[keep], tk1[keep])
    close(lp1[keep], lp0[keep], 2e-5)
    _, tk3 = pkg.greedy_decode(m, z, steps, want_logp=False)          # the ARG role without the log-probability output
    assert torch.equal(tk3, tk1)
    st = replay_decode_check({k: v.detach().cpu() for k, v in m.state_dict().items()}, z.cpu(), tk1, lp1)      # every position, past the near-ties too
    print("\n" + replay_line("block_pipeline", H, st))


@pytest.mark.parametrize("H,Bi,steps", [(64, 1100, 14), (512, 1024, 10)])
def test_large_batch_decode_cells_match_per_token_kernels(H, Bi, steps):
    """decode of >= Engine.cell_decode_rows sequences (fn_gru_cell_f32: every cell one staged-GEMM launch, layer 2's input projection in
    the same K loop) vs the scan-step kernels + projection GEMM: per row the same tokens and log-probabilities up to that row's first
    near-tie (the two paths sum the gate pre-activations in different orders)."""
    pkg = load_package()
    m = make_model(H, 32 if H == 64 else 128, device=DEV, seed=11)
    m.eval()
    torch.manual_seed(5)
    z = torch.randn(Bi, 2 * m.latent_dim + 24, device=DEV)
    eng = m.engine()
    eng.single_launch_decode = False                                          # (the one-launch pipeline takes these row counts otherwise)
    eng.cell_decode_rows = 1 << 30
    lp0, tk0 = pkg.greedy_decode(m, z, steps)
    eng.cell_decode_rows = 768
    lp1, tk1 = pkg.greedy_decode(m, z, steps)
    lp2, tk2 = pkg.greedy_decode(m, z, steps)
    assert torch.equal(tk1, tk2) and torch.equal(lp1, lp2)
    gap = lp0.topk(2, dim=-1).values
    unclear = ((gap[..., 0] - gap[..., 1]) <= 1e-4)                           # [Bi][steps]
    first = torch.where(unclear.any(1), unclear.float().argmax(1), torch.full((Bi,), steps, device=DEV))    # per row: first near-tie step
    keep = torch.arange(steps, device=DEV).view(1, -1) < first.view(-1, 1)
    assert bool(keep.float().mean() > 0.9)
    assert torch.equal(tk0[keep], tk1[keep])
    close(lp1[keep], lp0[keep], 2e-5)


@pytest.mark.parametrize("B,V,K", [(2048, 342, 512), (77, 342, 512), (300, 50, 64), (33, 97, 48), (130, 342, 112), (70, 60, 1024),
                                   (70, 97, 16), (70, 97, 32), (70, 97, 80)])      # K / 16 = 1, 2, 5 steps: below, at and above the ring of the eight-wave kernel (two steps per K half at 5), one-ring kernel for K = 16, 80
def test_out_argmax_packed_words(ops, B, V, K):
    """fn_out_argmax_f32 (output layer with the argmax in its epilogue: packed (logit, column) words by 64-bit atomic max) + fn_best_tokens
    against the fp64 logits: the winning column wherever the fp64 top-2 gap is above 1e-4, the packed key = the order-preserving image of a
    logit within 2e-5 of the fp64 one; ragged row / column tiles, K tails of the pipelined loop, exact ties -> first column, max-combining
    with what the word already holds."""
    torch.manual_seed(B + V)
    h, W, bias = torch.randn(B, K), torch.randn(V, K) / K ** 0.5, torch.randn(V) * 0.1
    W[V - 1] = W[3]
    bias[V - 1] = bias[3]                                   # an exact tie between columns 3 and V - 1 in every row
    ref = h.double() @ W.double().t() + bias.double()
    best = torch.zeros(2, B, dtype=torch.int64, device=DEV)
    # the kernel this K stands for in the table, from the library's plan for these tensors (fn_out_argmax_plan)
    plan = ops.out_argmax_plan(g(h), g(W), g(bias), best[0])
    want = {512: "out_argmax_lds8_kernel<4>", 64: "out_argmax_lds8_kernel<4>", 32: "out_argmax_lds8_kernel<4>", 48: "out_argmax_lds_kernel<8>",
            112: "out_argmax_lds_kernel<8>", 16: "out_argmax_lds_kernel<8>", 80: "out_argmax_lds_kernel<8>", 1024: "out_argmax_direct_kernel<4>"}[K]
    assert plan["kernel"] == want and plan["threads"] == (512 if "lds8" in want else 256), plan
    assert plan["grid"] == (-(-B // 32) * -(-V // 96) if "direct" in want else -(-B // 64) * -(-V // 48)), plan
    ops.out_argmax(g(h), g(W), g(bias), best[0])
    best[1].fill_(-1)                                       # the all-ones word is above every packed logit and stays
    best[1, : B // 2] = 0
    ops.out_argmax(g(h), g(W), g(bias), best[1])
    tok = torch.full((B, 3), -1, dtype=torch.int32, device=DEV)
    ops.best_tokens(best, V, tok)
    assert int(tok[:, 2].min()) == -1 and int(tok[:, 2].max()) == -1
    got = tok[:, 0].cpu().long()
    top2 = ref.topk(2, dim=1)
    clear = (top2.values[:, 0] - top2.values[:, 1]) > 1e-4
    assert float(clear.float().mean()) > 0.9
    assert torch.equal(got[clear], top2.indices[:, 0][clear])
    assert int((got == V - 1).sum()) == 0                   # the tie goes to column 3
    key = (best[0].cpu() >> 32) & 0xffffffff
    bits = torch.where(key >> 31 != 0, key ^ 0x80000000, key ^ 0xffffffff).to(torch.int32)
    val = bits.view(torch.float32)
    close(val, ref.gather(1, got.view(-1, 1)).squeeze(1).float(), 2e-5, "packed logit")
    assert torch.equal(tok[: B // 2, 1], tok[: B // 2, 0]) and bool((best[1, B // 2:] == -1).all())


def test_tokens_only_decode_on_the_cells_fused_argmax():
    """greedy_decode(want_logp=False) on the per-token cells (2048 rows, hidden 512): output layer + argmax as one launch, the next cell reads
    its token from the packed word - against the same path with the GEMM + fn_vocab_argmax launches (Engine.fused_argmax = False) up to each
    row's first near-tie, bit-reproducible, and directly against the oracle."""
    from oracle import gmvae_oracle as orc
    pkg = load_package()
    m = make_model(512, 128, device=DEV, seed=1234)
    m.eval()
    torch.manual_seed(22)
    Bi, steps = 2048, 20
    z = torch.randn(Bi, 2 * m.latent_dim + 24)
    eng = m.engine()
    eng.single_launch_decode, eng.cell_decode_rows = False, 768
    _, tk = pkg.greedy_decode(m, z.to(DEV), steps, want_logp=False)
    _, tk2 = pkg.greedy_decode(m, z.to(DEV), steps, want_logp=False)
    assert torch.equal(tk, tk2) and int(tk.min()) >= 0 and int(tk.max()) < 342
    eng.fused_argmax = False
    lp0, tk0 = pkg.greedy_decode(m, z.to(DEV), steps, want_logp=True)
    eng.fused_argmax = True
    gap = lp0.topk(2, dim=-1).values
    unclear = (gap[..., 0] - gap[..., 1]) <= 1e-4
    first = torch.where(unclear.any(1), unclear.float().argmax(1), torch.full((Bi,), steps, device=DEV))
    keep = torch.arange(steps, device=DEV).view(1, -1) < first.view(-1, 1)
    assert float(keep.float().mean()) > 0.95
    assert torch.equal(tk[keep], tk0[keep])
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    ref_lp, ref_tk = orc.greedy_decode(sd, z[:256], steps)
    top2 = ref_lp.topk(2, dim=-1).values
    unc = (top2[..., 0] - top2[..., 1]) < 1e-4
    fst = torch.where(unc.any(1), unc.float().argmax(1), torch.full((256,), steps))
    kp = torch.arange(steps).view(1, -1) < fst.view(-1, 1)
    assert torch.equal(tk[:256].cpu().long()[kp], ref_tk[kp])


@pytest.mark.parametrize("path,Bi,steps", [("cells", 2048, 20), ("cells", 1280, 12), ("cells", 1000, 12), ("pipeline", 800, 16), ("pipeline", 1536, 12)])
def test_large_decode_paths_vs_oracle(path, Bi, steps):
    """The decode paths BASELINE configs[4] is timed on, checked DIRECTLY against the oracle's eval-mode global_decoder (gmm_model.py:119-149,
    73-80; the oracle is pinned to the reference's greedy tokens by c0 / eval.npz) at hidden 512: the staged-GEMM cells (fn_gru_cell_f32,
    2048 rows = 256 sequences x 8 fader values, test_class.py:84-85) and the one-launch block pipeline (fn_decode_greedy, 800 and 1536
    rows).  Per row: the oracle's tokens up to the first step where the ORACLE's own top-2 gap is below 1e-4, log-probabilities to 1e-4."""
    from oracle import gmvae_oracle as orc
    pkg = load_package()
    m = make_model(512, 128, device=DEV, seed=1234)
    m.eval()
    torch.manual_seed(21)
    z = torch.randn(Bi, 2 * m.latent_dim + 24)
    eng = m.engine()
    if path == "cells":
        eng.single_launch_decode, eng.cell_decode_rows = False, 768
    else:
        eng.single_launch_decode, eng.single_launch_rows, eng.single_launch_skip = True, 2048, (0, -1)
    lp, tk = pkg.greedy_decode(m, z.to(DEV), steps)
    assert not eng.ops.gru_sync_error()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    ref_lp, ref_tk = orc.greedy_decode(sd, z, steps)
    top2 = ref_lp.topk(2, dim=-1).values
    unclear = (top2[..., 0] - top2[..., 1]) < 1e-4                                          # [Bi][steps]
    first = torch.where(unclear.any(1), unclear.float().argmax(1), torch.full((Bi,), steps))
    keep = torch.arange(steps).view(1, -1) < first.view(-1, 1)
    assert float(keep.float().mean()) > 0.95, float(keep.float().mean())
    got_tk, got_lp = tk.cpu().long(), lp.cpu()
    assert torch.equal(got_tk[keep], ref_tk[keep]), int((got_tk[keep] != ref_tk[keep]).sum())
    np.testing.assert_allclose(got_lp[keep].numpy(), ref_lp[keep].numpy(), rtol=0, atol=1e-4)
    st = replay_decode_check(sd, z, tk, lp)                                                  # and every position, past the near-ties too
    print("\n" + replay_line("large_decode_%s[%s]" % (path, _arith_tag(eng)), 512, st))


def _arith_tag(eng):
    return "bf16x6" if eng.ops.dw_x6 else "f32"


@pytest.mark.parametrize("path,weights,Bi,steps", REPLAY_CASES, ids=["%s-%s-%d" % (p, w, b) for p, w, b, _ in REPLAY_CASES])
def test_decode_paths_every_step_vs_fp64_replay(path, weights, Bi, steps):
    """Every decode path, forced by the engine switches, checked at EVERY position of its replayed rows against an fp64 replay of the
    tokens it chose (helpers.replay_decode_check): log-probs within tol_lp = min(1e-4, 16 x the fp32 restatement's own error), each token
    its own log-prob row's first argmax and within delta = 2 tol_lp of the fp64 best; the tokens-only form the same way.  The one-launch
    pipeline reuses its exchange slabs and per-block counters for every step, so 100 - 300 steps, ragged last blocks and up to 32 blocks;
    the graph paths replay their cached graph on a second latent batch, which must pass as well (nothing of the first call baked in).
    Weights: seeded with the output layer x 8 (fewer near-ties), or the trained H = 64 weights of epoch.npz."""
    pkg = load_package()
    from music_fader_nets_amd import decode as dec
    H, Z, sd = replay_inputs(weights)
    m = make_model(H, Z, sd, device=DEV, arith="bf16x6" if path == "cells_x6" else None)
    m.eval()
    eng = m.engine()
    one_launch = path in ("one_launch", "pipeline32", "pipeline64")
    if one_launch:
        eng.single_launch_decode, eng.single_launch_skip = True, (0, -1)
        if Bi > eng.single_launch_rows:
            eng.single_launch_rows = 2048
        # what the library launches for this engine's own tensors (fn_decode_plan) is what the case's name says
        for want_logp in (True, False):
            plan = dec.single_launch_plan(eng, Bi, steps, want_logp)
            assert plan is not None and dec._single_launch_ok(eng, torch.empty(Bi, 1, device=DEV)) and not plan["forced"]
            assert (plan["block_rows"], plan["nblk"]) == ONE_LAUNCH_BLOCKS[path](Bi) and (plan["nblk"] == 1) == (path == "one_launch"), (path, Bi, plan)
    elif path == "scan_steps":
        eng.single_launch_decode, eng.cell_decode_rows = False, 1 << 30
        assert dec.decode_path(eng, Bi, True, None, None) == "scan_steps" and dec.decode_path(eng, Bi, False, None, None) == "scan_steps"
    else:
        eng.single_launch_decode = False
        assert dec.decode_path(eng, Bi, True, None, None) == "cells" and dec.decode_path(eng, Bi, False, None, None) == "cells_fused"
        x6 = eng.ops.dw_x6 and eng.ops.cell_x6 and Bi >= eng.ops.cell_x6_rows
        assert x6 == (path == "cells_x6")
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    z = replay_z(Bi, Z, Bi)
    lp, tk = pkg.greedy_decode(m, z.to(DEV), steps, want_logp=True)
    _, tk_only = pkg.greedy_decode(m, z.to(DEV), steps, want_logp=False)
    assert not eng.ops.gru_sync_error()
    graphs = eng.__dict__.get("_decode_graphs", {})
    assert (len(graphs) == 0) == one_launch                  # the one-launch paths did not fall back to the per-token kernels
    tag = "%s[%s]/%s" % (path, _arith_tag(eng), weights)
    st = replay_decode_check(sd, z, tk, lp)
    print("\n" + replay_line(tag, H, st), end="")
    if not torch.equal(tk_only, tk):
        st = replay_decode_check(sd, z, tk_only)
        print("\n" + replay_line(tag + " tokens", H, st), end="")
    if path in REPLAY_GRAPH_PATHS:
        n = len(graphs)
        z2 = replay_z(Bi, Z, Bi + 1)
        lp2, tk2 = pkg.greedy_decode(m, z2.to(DEV), steps, want_logp=True)
        assert len(eng._decode_graphs) == n and not eng.ops.gru_sync_error()
        st = replay_decode_check(sd, z2, tk2, lp2)
        print("\n" + replay_line(tag + " graph z2", H, st), end="")
    print()


def test_configs4_sized_fader_sweep_properties():
    """BASELINE configs[4] at its full size - 256 sequences (T = 256) encoded, 8 fader values each on z_r[:, 0] (test_class.py:84-85), 2048 rows
    x 300 greedy steps - through the default dispatch of fader_sweep: token range, bit-reproducibility of a second pass, sync-error word
    clear, and the first 24 steps of 64 of the rows against the oracle's decode of the same latent rows"""
    from oracle import gmvae_oracle as orc
    from music_fader_nets_amd.synth import synth_batch
    pkg = load_package()
    m = make_model(512, 128, device=DEV, seed=1234)
    m.eval()
    b = synth_batch(np.random.RandomState(0), 256, 256, 64)
    d = torch.from_numpy(b["d"]).to(DEV).to(torch.int32)
    c = torch.from_numpy(b["c"]).to(DEV)
    torch.manual_seed(99)
    eps = (torch.randn(256, 128).to(DEV), torch.randn(256, 128).to(DEV))
    values = [-2.0 + 0.5 * k for k in range(8)]
    tok, z0 = pkg.fader_sweep(m, d, c, values, steps=300, which="r", eps=eps)
    tok2, _ = pkg.fader_sweep(m, d, c, values, steps=300, which="r", eps=eps)
    assert not m.engine().ops.gru_sync_error()
    assert tuple(tok.shape) == (256, 8, 300) and int(tok.min()) >= 0 and int(tok.max()) < 342
    assert torch.equal(tok, tok2)
    # the latent rows of 8 of the sequences, rebuilt as test_class.py:243-251 builds them, decoded by the oracle
    dis_r, dis_n = m.encode(d)
    np.testing.assert_allclose(z0.cpu().numpy(), (dis_r.mean + dis_r.stddev * eps[0])[:, 0].cpu().numpy(), rtol=1e-6, atol=1e-6)
    seqs = torch.arange(0, 256, 32, device=DEV)
    zr = (dis_r.mean + dis_r.stddev * eps[0])[seqs].unsqueeze(1).repeat(1, 8, 1)
    zn = (dis_n.mean + dis_n.stddev * eps[1])[seqs].unsqueeze(1).repeat(1, 8, 1)
    zr[:, :, 0] = torch.tensor(values, device=DEV)
    zc = torch.cat([zr, zn, c[seqs].unsqueeze(1).repeat(1, 8, 1)], dim=2).view(64, -1)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref_lp, ref_tk = orc.greedy_decode(sd, zc.cpu(), 24)
    top2 = ref_lp.topk(2, dim=-1).values
    unclear = (top2[..., 0] - top2[..., 1]) < 1e-4
    first = torch.where(unclear.any(1), unclear.float().argmax(1), torch.full((64,), 24))
    keep = torch.arange(24).view(1, -1) < first.view(-1, 1)
    assert float(keep.float().mean()) > 0.9
    assert torch.equal(tok[seqs].reshape(64, 300)[:, :24].cpu().long()[keep], ref_tk[keep])
    # every step of 256 of the 2048 rows against an fp64 replay of their tokens, the latent rows built the same way for all sequences
    zr = (dis_r.mean + dis_r.stddev * eps[0]).unsqueeze(1).repeat(1, 8, 1)
    zn = (dis_n.mean + dis_n.stddev * eps[1]).unsqueeze(1).repeat(1, 8, 1)
    zr[:, :, 0] = torch.tensor(values, device=DEV)
    z_all = torch.cat([zr, zn, c.unsqueeze(1).repeat(1, 8, 1)], dim=2).view(2048, -1)
    st = replay_decode_check(sd, z_all.cpu(), tok.reshape(2048, 300))
    print("\n" + replay_line("configs4_sweep[%s]" % _arith_tag(m.engine()), 512, st))


def test_full_size_properties():
    pkg = load_package()
    from music_fader_nets_amd.synth import synth_batch
    B, T, Tr = 256, 256, 64
    m = make_model(512, 128, device=DEV)
    tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
    b = synth_batch(np.random.RandomState(0), B, T, Tr)
    batch = tr.prepare_batch(b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
    torch.manual_seed(99)
    eps = tr.draw_eps(B, T)
    # (1) determinism: the same step twice from the same state gives bit-identical gradients
    t1 = tr.loss_and_grads(20000, batch, eps)
    g1 = tr.flat.grad.clone()
    tr.loss_and_grads(20000, batch, eps)
    beta0, Bg = 0.2, B
    assert bool(torch.isfinite(g1).all())
    assert torch.equal(g1, tr.flat.grad)          # no floating-point atomics anywhere on the path
    # (2) batch-row independence: the loss of the first 64 rows alone equals the same rows' share
    #     (CE terms are per-row means) -> CE_X of a sub-batch computed separately matches the row-slice mean
    nll = m.engine().buf("nll_rows", (T * B,)).view(T, B)
    sub = tr.prepare_batch(b["d"][:64], b["r"][:64], b["n"][:64], b["c"][:64], b["r_density"][:64], b["n_density"][:64])
    full_rows = float(nll[:, :64].double().sum()) / (64 * T)        # before: computed inside the full batch
    tr._forward_losses(20000, sub, (eps[0][:64].contiguous(), eps[1][:64].contiguous()), False)
    t_sub = tr._tuple8(beta0, 64, False)
    np.testing.assert_allclose(t_sub[1], full_rows, rtol=1e-5)
    # (3) directional derivative: loss(w + h*g/|g|) - loss(w - h*g/|g|) ~ 2h|g|
    gn = float(g1.double().norm())
    hstep = 2e-3
    p0 = tr.flat.param.clone()
    vals = []
    for sgn in (+1, -1):
        tr.flat.param.copy_(p0 + sgn * hstep * g1 / gn)
        m.weights_changed()
        tr._forward_losses(20000, batch, eps, False)
        vals.append(tr._tuple8(beta0, Bg, False)[0])
    tr.flat.param.copy_(p0)
    m.weights_changed()
    np.testing.assert_allclose((vals[0] - vals[1]) / (2 * hstep), gn, rtol=2e-2)
    # (4) a few optimisation steps reduce the training loss (KL-dominated at beta0 = 0.2)
    step, first = 20000, None
    for it in range(6):
        step, tup = tr.train(step, None, None, None, b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"], eps=eps)
        first = first or tup
    assert tup[0] < first[0] and all(math.isfinite(x) for x in tup)


# ----------------------------------------------------------------------------------------------
# eval-side callers: eval-mode forward, evaluator shifts, notebook transfer (300 steps), run_through_gmm
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,H,Z", [("s", 64, 32), ("c", 512, 128)])
def test_eval_side_callers_vs_reference(tag, H, Z):
    from helpers import check_eval_side, eval_golden
    pkg = load_package()
    m = make_model(H, Z, device=DEV)
    check_eval_side(pkg, m, eval_golden(tag), DEV, rtol=1e-4)
    assert not m.engine().ops.gru_sync_error()


# ----------------------------------------------------------------------------------------------
# the BENCHMARK configuration against the reference itself (tests/golden/c1.npz: B=256, T=256, Tr=64, hidden 512)
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["f32", "bf16x6"])
def test_benchmark_config_vs_reference_train(arith):
    """The kernels bench.py times (128-row weight-stationary scans at T=256, K=65536 weight-gradient GEMMs, 65536-row token-segment
    sums) compared with the reference's own forward / backward / train() at that size, on the seeds bench.py uses."""
    pkg = load_package()
    from music_fader_nets_amd.synth import synth_batch
    g = load_golden("c1")
    H, Z, K, B, T, Tr = (int(x) for x in g["meta_dims"])
    m = make_model(H, Z, device=DEV, arith=arith)
    tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
    b = synth_batch(np.random.RandomState(0), B, T, Tr)
    batch = tr.prepare_batch(b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
    torch.manual_seed(99)
    eps = tr.draw_eps(B, T)
    # forward checksums through the drop-in call (no_grad: forward only)
    with torch.no_grad():
        (o, r_out, n_out, _, _), dis, z_out, ll_out, qy_out, y_out = m(batch[0], batch[1], batch[2], batch[3], eps=eps)
    got = dict(out=o, r_out=r_out, n_out=n_out, mu_r=dis[0].mean, sigma_r=dis[0].stddev, mu_n=dis[1].mean, sigma_n=dis[1].stddev,
               z_r=z_out[0], z_n=z_out[1], ll_r=ll_out[0], ll_n=ll_out[1], qy_r=qy_out[0], qy_n=qy_out[1])
    for k, v in got.items():
        vd = v.double()
        np.testing.assert_allclose([vd.sum().item(), vd.abs().sum().item(), (vd * vd).sum().item()], g["fwsum_" + k], rtol=2e-5,
                                   atol=1e-6, err_msg=k)
    np.testing.assert_allclose(o[0, :4].cpu().numpy(), g["fw_out_row0"], rtol=1e-4, atol=1e-4)
    assert np.array_equal(y_out[0].cpu().numpy(), g["fw_y_r"]) and np.array_equal(y_out[1].cpu().numpy(), g["fw_y_n"])
    del o, got
    # raw gradients of the fused step
    tup = tr.loss_and_grads(20000, batch, eps)
    np.testing.assert_allclose(tup[0], g["total_loss_20000"][0], rtol=2e-5)
    np.testing.assert_allclose(tr.grad_norm(), g["gradnorm_20000"][0], rtol=1e-3)
    for k in tr.flat.names:
        gk = tr.flat.G[k].double()
        ref = g["gradsum/" + k]
        np.testing.assert_allclose(float(gk.abs().sum()), ref[1], rtol=1e-3, atol=1e-5, err_msg=k)
        np.testing.assert_allclose(float((gk * gk).sum()), ref[2], rtol=2e-3, atol=1e-9, err_msg=k)
    assert set(tr.flat.names) == {k[len("gradsum/"):] for k in g if k.startswith("gradsum/")}
    # the reference's own train(), twice (same eps every step, as bench.py runs it); step 1 eager, step 2 = graph capture + replay
    step = 20000
    for it in range(2):
        step, tup = tr.train(step, None, None, None, b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"], eps=eps)
        np.testing.assert_allclose(tup, g["train_tuples"][it], rtol=5e-4, err_msg="step %d" % it)
        if it == 0:
            for k, v in m.state_dict().items():
                if k not in NOISE_PARAMS:
                    vd = v.double()
                    np.testing.assert_allclose([vd.abs().sum().item(), (vd * vd).sum().item()], g["w1sum/" + k][1:], rtol=2e-5, err_msg=k)
    assert not m.engine().ops.gru_sync_error()


# ----------------------------------------------------------------------------------------------
# captured graphs vs changing batch shapes / changing weights
# ----------------------------------------------------------------------------------------------
def test_bf16x6_is_live_at_the_benchmark_shape():
    """set_arith really switches kernels (and back) on a live model: against the fp32-MFMA gradients of the same step the recurrent weight
    gradients differ - in their last bits only; the switch survives an engine rebuild (parameters re-homed by a second trainer) and captured
    steps are keyed by it (the comparison with the reference at this shape runs in test_benchmark_config_vs_reference_train[bf16x6])"""
    pkg = load_package()
    from music_fader_nets_amd.synth import synth_batch
    g = load_golden("c1")
    H, Z, K, B, T, Tr = (int(x) for x in g["meta_dims"])
    m = make_model(H, Z, device=DEV)
    tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
    b = synth_batch(np.random.RandomState(0), B, T, Tr)
    batch = tr.prepare_batch(b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
    torch.manual_seed(99)
    eps = tr.draw_eps(B, T)
    m.set_arith("bf16x6")
    tup6 = tr.loss_and_grads(20000, batch, eps)
    assert m.engine().ops.dw_x6 and m.engine().whh_f3
    g6 = tr.flat.G["gru_r.weight_hh_l0"].clone()
    m.set_arith("f32")
    tup32 = tr.loss_and_grads(20000, batch, eps)
    assert not m.engine().ops.dw_x6 and not m.engine().whh_f3
    g32 = tr.flat.G["gru_r.weight_hh_l0"]
    np.testing.assert_allclose(tup6, tup32, rtol=2e-5)
    assert not torch.equal(g6, g32)
    assert float((g6 - g32).abs().max()) <= 1e-5 * float(g32.abs().max())      # fp32 rounding through 256 recurrent steps (forward scans + products differ in their last bits)
    m.set_arith("bf16x6")
    tr2 = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)            # re-homes the parameters: a new engine and kernel table - the choice lives on the model
    tr2.loss_and_grads(20000, batch, eps)
    assert m.engine().ops.dw_x6
    assert torch.equal(tr2.flat.G["gru_r.weight_hh_l0"], g6)
    assert not m.engine().ops.gru_sync_error()


def test_graph_replay_survives_other_batch_shapes():
    """The epoch driver alternates shapes (train / validation / ragged last batch); every shape keeps its own captured graph and its
    own buffers.  Interleaving shapes must give the same numbers as running each shape alone."""
    pkg = load_package()
    from music_fader_nets_amd.synth import synth_batch
    shapes = [(12, 40, 16), (5, 24, 8), (12, 24, 8)]
    data = [synth_batch(np.random.RandomState(10 + i), *s) for i, s in enumerate(shapes)]
    seq = [0, 1, 0, 2, 1, 0, 2, 0, 1, 2, 0]                   # every shape is replayed after the others ran

    def run(order_filter):
        m = make_model(64, 32, device=DEV)
        tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
        outs, step = [], 20000
        for j, si in enumerate(seq):
            if order_filter is not None and si != order_filter:
                continue
            b = data[si]
            torch.manual_seed(500 + j)
            step, tup = tr.train(step, None, None, None, b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
            outs.append((j, tup))
            if si == 1:                                       # an eager evaluate at yet another shape in between
                bb = {k: v[:3] for k, v in data[0].items()}
                torch.manual_seed(900 + j)
                outs.append((j, tr.evaluate(step - 1, None, None, None, bb["d"], bb["r"], bb["n"], bb["c"], bb["r_density"], bb["n_density"])))
        assert len(tr._graphs) == (3 if order_filter is None else 1)
        return outs, {k: v.clone() for k, v in m.state_dict().items()}

    mixed, w_mixed = run(None)
    assert all(np.isfinite(t).all() for _, t in mixed)
    # reference: the same sequence on a fresh trainer with graphs disabled (eager launches, nothing captured)
    m2 = make_model(64, 32, device=DEV)
    tr2 = pkg.GMVAETrainer(m2, lr=1e-3, beta=0.2)
    tr2.use_graph = False
    step, k = 20000, 0
    for j, si in enumerate(seq):
        b = data[si]
        torch.manual_seed(500 + j)
        step, tup = tr2.train(step, None, None, None, b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
        np.testing.assert_allclose(mixed[k][1], tup, rtol=1e-6, err_msg="train %d" % j)
        k += 1
        if si == 1:
            bb = {kk: v[:3] for kk, v in data[0].items()}
            torch.manual_seed(900 + j)
            ev = tr2.evaluate(step - 1, None, None, None, bb["d"], bb["r"], bb["n"], bb["c"], bb["r_density"], bb["n_density"])
            np.testing.assert_allclose(mixed[k][1], ev, rtol=1e-6, err_msg="eval %d" % j)
            k += 1
    for kk, v in m2.state_dict().items():
        assert torch.equal(v, w_mixed[kk]), kk                # bit-identical weights: no replay touched a stale buffer


@pytest.mark.parametrize("Bi", [4, 40])
def test_decode_sees_the_trained_weights(Bi):
    """decode -> train -> decode: the second decode must use the updated weights (single-launch path: the fragment images of W_ih2 /
    W_out; graph path: the captured kernels read the live buffers) - compared with a fresh model loaded with the trained state_dict."""
    pkg = load_package()
    from music_fader_nets_amd.synth import synth_batch
    m = make_model(64, 32, device=DEV)
    tr = pkg.GMVAETrainer(m, lr=1e-2, beta=0.2)
    torch.manual_seed(1)
    z = torch.randn(Bi, 2 * 32 + 24, device=DEV)
    m.eval()
    lp0, tk0 = pkg.greedy_decode(m, z, 20)
    m.train()
    b = synth_batch(np.random.RandomState(0), 8, 24, 8)
    step = 20000
    for it in range(4):                                        # eager, capture, replay, replay
        torch.manual_seed(it)
        step, _ = tr.train(step, None, None, None, b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
    m.eval()
    lp1, tk1 = pkg.greedy_decode(m, z, 20)
    assert not torch.equal(lp0, lp1)
    fresh = make_model(64, 32, {k: v.cpu() for k, v in m.state_dict().items()}, device=DEV)
    fresh.eval()
    lp2, tk2 = pkg.greedy_decode(fresh, z, 20)
    np.testing.assert_allclose(lp1.cpu().numpy(), lp2.cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert torch.equal(tk1, tk2)


def test_dataloader_batches_feed_the_hip_trainer():
    """DataLoader batches of YamahaDataset / VGMIDIDataset (float32 token ids, float64 densities, arousal labels)
    go straight into GMVAETrainer.train / evaluate on the HIP path - no manual casts - and match the oracle on the same batch."""
    from torch.utils.data import DataLoader
    pkg = load_package()
    from music_fader_nets_amd import datasets as D
    g = load_golden("data")
    san = D.sanitize_chroma(g["y_in_data"], g["y_in_rhythm"], g["y_in_note"], g["y_in_chroma"])
    m = make_model(64, 32, device=DEV)
    sd0 = {k: v.cpu().clone() for k, v in m.state_dict().items()}
    tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
    d, r, n, c, rd, nd = next(iter(DataLoader(D.YamahaDataset(*san), batch_size=4)))
    torch.manual_seed(42)
    eps = (torch.randn(d.shape[0], 32), torch.randn(d.shape[0], 32))
    step, tup = tr.train(20000, None, None, None, d, r, n, c.float(), rd, nd, eps=tuple(e.to(DEV) for e in eps))
    opt = orc.AdamState(orc.trainable_used_keys(sd0))
    ob = dict(d=d.long().numpy(), r=r.long().numpy(), n=n.long().numpy(), c=c.float().numpy(), r_density=rd.numpy(), n_density=nd.numpy())
    _, ref, _ = orc.train_step(sd0, opt, ob, eps[0], eps[1], 20000, beta=0.2, lr=1e-3)
    np.testing.assert_allclose(tup, ref, rtol=5e-4)
    from test_datasets import _ragged as rag
    ds = D.VGMIDIDataset(rag(g["v_in_tokens"], g["v_in_lens"]), rag(g["v_in_rhythm"], g["v_in_rlens"]), rag(g["v_in_note"], g["v_in_rlens"]),
                         g["v_in_chroma"], g["v_in_arousal"].copy(), g["v_in_valence"])
    d, r, n, c, a, v, rd, nd = next(iter(DataLoader(ds, batch_size=4)))
    assert d.is_floating_point()                                # as the reference's dataset yields them
    torch.manual_seed(43)
    eps = (torch.randn(d.shape[0], 32), torch.randn(d.shape[0], 32))
    sd1 = {k: v.cpu().clone() for k, v in m.state_dict().items()}
    step, tup = tr.train(step, None, None, None, d, r, n, c.float(), rd, nd, is_supervised=True, y_label=a, eps=tuple(e.to(DEV) for e in eps))
    ob = dict(d=d.long().numpy(), r=r.long().numpy(), n=n.long().numpy(), c=c.float().numpy(), r_density=rd.numpy(), n_density=nd.numpy(),
              a=a.long().numpy())
    loss, ref, _ = orc.total_loss(sd1, ob, eps[0], eps[1], 20001, 0.2, is_supervised=True)
    np.testing.assert_allclose(tup, [float(x) for x in ref], rtol=5e-4)


# ----------------------------------------------------------------------------------------------
# single-encoder siblings of model_v2.py on the HIP kernels (SingleEncEngine, adv_head_kernel)
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["single", "cvae", "fader"])
def test_siblings_vs_reference(kind):
    from helpers import check_sibling, make_sibling, sibling_golden
    pkg = load_package()
    m = make_sibling(kind, 64, 32, device=DEV)
    check_sibling(pkg, kind, m, sibling_golden(kind), DEV, rtol_fw=1e-4, tol_grad=5e-4, rtol_tuple=5e-4)
    assert not m.engine().ops.gru_sync_error()


def test_adv_head_kernel(ops):
    torch.manual_seed(21)
    B, Z = 37, 96
    z, w_r, w_n = torch.randn(B, Z + 8), torch.randn(1, Z), torch.randn(1, Z)
    b_r, b_n = torch.randn(1), torch.randn(1)
    mask = (torch.rand(B, 2) > 0.3).float() / 0.7
    dens = torch.rand(B, 2)
    lam = torch.tensor([3e-2])
    g0 = torch.randn(B, Z + 8)
    outs_c = [torch.zeros(B, 2) for _ in range(3)]
    gz_c = g0.clone()
    FakeOps().adv_head(z[:, :Z], w_r, w_n, b_r, b_n, mask, dens, lam, 1.0 / B, outs_c[0], outs_c[1], outs_c[2], gz_c[:, :Z])
    outs_d = [torch.zeros(B, 2, device=DEV) for _ in range(3)]
    zd, gz_d = g(z), g(g0.clone())
    ops.adv_head(zd[:, :Z], g(w_r), g(w_n), g(b_r), g(b_n), g(mask), g(dens), g(lam), 1.0 / B, outs_d[0], outs_d[1], outs_d[2], gz_d[:, :Z])
    for a, b in zip(outs_d, outs_c):
        close(a, b, 1e-5)
    close(gz_d, gz_c, 1e-5)
    assert torch.equal(gz_d[:, Z:].cpu(), g0[:, Z:])              # columns beyond Z untouched (row views with a leading dimension)


@pytest.mark.parametrize("B,H,rows", [(256, 512, 0), (256, 512, 64), (40, 96, 0)])
def test_chunked_scan_with_fragment_handover_is_bit_identical(ops, B, H, rows):
    """a forward scan cut into time chunks whose state travels in the exchange layout (h_last_frag -> h0_frag, no packing launch)
    gives bit-identical states / gates to the same scan in one launch"""
    torch.manual_seed(B + H)
    T, V = 24, 50
    w = (torch.randn(3 * H, H) / H ** 0.5).to(DEV)
    wf = torch.zeros(ops.frag_floats(3 * H, H), device=DEV)
    ops.frag_pack(w, wf)
    base = dict(B=B, H=H, w_hh_frag=wf, b_hh=torch.randn(3 * H, device=DEV) * 0.1, b_ih=torch.randn(3 * H, device=DEV) * 0.1,
                h0=torch.randn(B, H, device=DEV) * 0.3, gx_table=torch.randn(V, 3 * H, device=DEV) * 0.3,
                idx=torch.randint(0, V, (B, T), dtype=torch.int32, device=DEV), idx_shift=-1, start_token=V - 1)
    ref = dict(base, T=T, h_all=torch.zeros(T, B, H, device=DEV), gates=torch.zeros(T, ops.gates_floats(B, H), device=DEV))
    ops.gru_seq_fwd([ref], variant=rows)
    h_all = torch.zeros(T, B, H, device=DEV)
    gates = torch.zeros(T, ops.gates_floats(B, H), device=DEV)
    hand = [torch.zeros(ops.frag_floats(B, H), device=DEV) for _ in range(2)]
    for ci, t0 in enumerate(range(0, T, 7)):
        t1 = min(T, t0 + 7)
        c = dict(base, T=t1 - t0, h_all=h_all[t0:t1], gates=gates[t0:t1], idx_shift=-1 + t0)
        if t0 > 0:
            c["h0"], c["h0_frag"] = h_all[t0 - 1], hand[(ci - 1) & 1]
        if t1 < T:
            c["h_last_frag"] = hand[ci & 1]
        ops.gru_seq_fwd([c], variant=rows)
    assert not ops.gru_sync_error()
    assert torch.equal(h_all, ref["h_all"]) and torch.equal(gates, ref["gates"])


def _pp_forward_scans(ops, n, B, H, Ts, seed, kinds):
    """n scan descriptors (device) for the ping-pong comparison; kinds[i] in {"table", "table_rev", "table_shift", "dense"}"""
    torch.manual_seed(seed)
    V = 50
    scans = []
    for i in range(n):
        T = Ts[i % len(Ts)]
        wf = torch.zeros(ops.frag_floats(3 * H, H), device=DEV)
        ops.frag_pack((torch.randn(3 * H, H, device=DEV) / H ** 0.5).contiguous(), wf)
        d = dict(B=B, T=T, H=H, reverse=0, w_hh_frag=wf, b_hh=torch.randn(3 * H, device=DEV) * 0.1,
                 h_all=torch.zeros(T, B, H, device=DEV), gates=torch.zeros(T, ops.gates_floats(B, H), device=DEV))
        kind = kinds[i % len(kinds)]
        if kind.startswith("table"):
            d["gx_table"] = torch.randn(V, 3 * H, device=DEV) * 0.3
            d["idx"] = torch.randint(0, V, (B, T), dtype=torch.int32, device=DEV)
            d["b_ih"] = torch.randn(3 * H, device=DEV) * 0.1
            if kind == "table_rev":
                d["reverse"] = 1
            if kind == "table_shift":
                d["idx_shift"], d["start_token"] = -1, V - 1
                d["gx_rowbias"] = torch.randn(B, 3 * H, device=DEV) * 0.2
                d["h0"] = torch.randn(B, H, device=DEV) * 0.3
        else:
            d["gx_dense"] = torch.randn(T, B, 3 * H, device=DEV) * 0.3
            if i & 1:
                d["h0"] = torch.randn(B, H, device=DEV) * 0.3
        scans.append(d)
    return scans


@pytest.mark.parametrize("n,B,Ts,kinds", [(4, 256, (9,), ("table", "table_rev")), (4, 256, (2, 5, 3, 7), ("table_rev", "dense", "table_shift", "table")),
                                          (2, 256, (8,), ("table_shift", "dense")), (2, 256, (3, 6), ("dense", "table")), (1, 512, (5,), ("table_shift",)),
                                          (3, 128, (4,), ("table", "dense", "table_rev")), (8, 128, (6, 3), ("table", "table_shift"))])
def test_ping_pong_scans_are_bit_identical_to_the_single_group_loops(ops, n, B, Ts, kinds):
    """round 4: the forward scans whose workgroups alternate between two halves of their row group (gru_fwd_pp_kernel: H = 512, 128- and 64-row
    groups) against the round-3 loops (variant FN_GRU_NO_PINGPONG), three launches in a row on the same buffers: bit-identical; the backward scans of
    the same shapes: the 32-slice loop bit-identical to the round-3 form, the register-stationary default within rounding and bit-stable from
    launch to launch.  (A ping-pong form of the 32-slice backward existed until round 4: never the default, and it differed from the loop in
    about 1 % of its launches at the encoder shape - removed, scratch/gru_bwd_pp_kernel_removed.hip.txt.)"""
    from music_fader_nets_amd import _lib
    H = 512
    scans = _pp_forward_scans(ops, n, B, H, Ts, 7 * n + B, kinds)
    ops.gru_seq_fwd(scans, variant=_lib.GRU_NO_PINGPONG)
    ref = [(d["h_all"].clone(), d["gates"].clone()) for d in scans]
    for rep in range(3):
        for d in scans:
            d["h_all"].fill_(float("nan"))
            d["gates"].fill_(float("nan"))
        ops.gru_seq_fwd(scans)
        assert not ops.gru_sync_error()
        for i, ((h, gt), d) in enumerate(zip(ref, scans)):
            assert torch.equal(d["h_all"], h), "rep %d scan %d h_all: max diff %g" % (rep, i, float((d["h_all"] - h).abs().max()))
            assert torch.equal(d["gates"], gt), "rep %d scan %d gates" % (rep, i)
    # backward of the same scans: gradient from the last state, from every step, or both; dL/dh0 and the per-sequence row sums optional
    torch.manual_seed(3 * n + B)
    bw = []
    for i, d in enumerate(scans):
        T = d["T"]
        wt = torch.zeros(ops.frag_floats(H, 3 * H), device=DEV)
        ops.frag_pack((torch.randn(H, 3 * H, device=DEV) / H ** 0.5).contiguous(), wt)
        bw.append(dict(B=B, T=T, H=H, w_hh_t_frag=wt, h0=d.get("h0"), h_all=d["h_all"], gates=d["gates"],
                       dh_last=torch.randn(B, H, device=DEV) if i % 3 != 1 else None, dh_ext=torch.randn(T, B, H, device=DEV) * 0.1 if i % 3 != 0 else None,
                       dgx_all=torch.zeros(T, B, 3 * H, device=DEV), dghn_all=torch.zeros(T, B, H, device=DEV),
                       dh0=torch.zeros(B, H, device=DEV) if (d.get("h0") is not None or i == 0) else None,
                       dgx_rowsum=torch.zeros(B, 3 * H, device=DEV) if i & 1 else None, dghn_rowsum=torch.zeros(B, H, device=DEV) if i != 2 else None,
                       scratch=torch.zeros(B, H, device=DEV)))
    outs = ("dgx_all", "dghn_all", "dh0", "dgx_rowsum", "dghn_rowsum")
    ops.gru_seq_bwd(bw, variant=_lib.GRU_NO_PINGPONG)
    refb = [{k: b[k].clone() for k in outs if b[k] is not None} for b in bw]
    for rep in range(3):
        for b in bw:
            for k in outs:
                if b[k] is not None:
                    b[k].zero_() if "rowsum" in k else b[k].fill_(float("nan"))
        ops.gru_seq_bwd(bw, variant=_lib.GRU_NO_RS_BWD)  # not the register-stationary kernel - the 32-slice loop of the automatic dispatch
        assert not ops.gru_sync_error()
        for i, (r, b) in enumerate(zip(refb, bw)):
            for k, v in r.items():
                assert torch.equal(b[k], v), "backward rep %d scan %d %s: max diff %g" % (rep, i, k, float((b[k] - v).abs().max()))
    # the default backward of these shapes: 16 slices of 32 columns, half of each W_hh^T slice register-stationary (gru_bwd_rs_kernel) - another
    # summation order over K, so equal within rounding
    for rep in range(3):
        for b in bw:
            for k in outs:
                if b[k] is not None:
                    b[k].zero_() if "rowsum" in k else b[k].fill_(float("nan"))
        ops.gru_seq_bwd(bw)
        assert not ops.gru_sync_error()
        for i, (r, b) in enumerate(zip(refb, bw)):
            for k, v in r.items():
                close(b[k], v, 2e-5, "register-stationary backward rep %d scan %d %s" % (rep, i, k))
        if rep == 0:
            first = [{k: b[k].clone() for k in outs if b[k] is not None} for b in bw]
        else:                                              # ... and the same bits from launch to launch
            assert all(torch.equal(b[k], v) for r, b in zip(first, bw) for k, v in r.items()), "register-stationary backward rep %d differs from rep 0" % rep


def test_masked_prob_kernel(ops):
    torch.manual_seed(31)
    rows, E, ld = 203, 342, 344
    logits = torch.randn(rows, ld) * 3
    w = torch.randn(rows, 2)
    ranges = ((2, 90), (180, 278))
    s_c, d_c = torch.zeros(rows, 2), torch.zeros(rows, ld)
    FakeOps().masked_prob(logits, E, ranges, sums=s_c, w=w, dlogits=d_c)
    ld_dev = g(logits.clone())
    s_d = torch.zeros(rows, 2, device=DEV)
    ops.masked_prob(ld_dev, E, ranges, sums=s_d)
    close(s_d, s_c, 1e-5)
    ops.masked_prob(ld_dev, E, ranges, w=g(w), dlogits=ld_dev)          # in place, as the GLSR backward seeds the decoder
    close(ld_dev[:, :E], d_c[:, :E], 2e-5)


def test_glsr_trainer_vs_reference():
    """trainer_glsr.py's step (four extra teacher-forced decodes + host walk + their backward) on the HIP kernels"""
    from helpers import check_glsr, glsr_fixture_weights, make_vae_model
    pkg = load_package()
    gold = load_golden("glsr")
    H, Z = int(gold["dims"][0]), int(gold["dims"][1])
    m = make_vae_model(H, Z, device=DEV)
    m.load_state_dict(glsr_fixture_weights(gold, H, Z))
    check_glsr(pkg, m, gold, DEV, tol_grad=2e-3, rtol_tuple=5e-4)
    assert not m.engine().ops.gru_sync_error()


def test_weight_images_one_launch(ops):
    """fn_weight_images (every transposed / fragment-major weight image of a step in one launch) == the single-matrix entry points"""
    torch.manual_seed(17)
    H, V = 96, 342
    w_ih = torch.randn(3 * H, V + 40, device=DEV)
    w_hh = torch.randn(3 * H, H, device=DEV)
    w_out = torch.randn(V, H, device=DEV)
    tab = torch.zeros(V, 3 * H, device=DEV)
    f1, f2 = torch.zeros(ops.frag_floats(3 * H, H), device=DEV), torch.zeros(ops.frag_floats(H, 3 * H), device=DEV)
    f3 = torch.zeros(ops.frag_floats(V, H), device=DEV)
    wz = torch.zeros(3 * H, 40, device=DEV)
    ops.weight_images([("transpose", w_ih[:, :V], tab), ("frag", w_hh, f1), ("frag_t", w_hh, f2), ("frag", w_out, f3), ("copy", w_ih[:, V:], wz)])
    assert torch.equal(tab, w_ih[:, :V].t())
    assert torch.equal(wz, w_ih[:, V:])                         # kind 5: the dense image of a column slice
    r1, r2, r3 = torch.zeros_like(f1), torch.zeros_like(f2), torch.zeros_like(f3)
    ops.frag_pack(w_hh, r1)
    ops.frag_pack(w_hh.t().contiguous(), r2)
    ops.frag_pack(w_out, r3)
    assert torch.equal(f1, r1) and torch.equal(f2, r2) and torch.equal(f3, r3)


@pytest.mark.parametrize("a_k,b_k", [(True, True), (True, False), (False, False), (False, True)])
def test_gemm_multi(ops, a_k, b_k):
    """several small GEMMs, each a sum of products over separate operands, in one launch (odd sizes, strided views, beta, bias)"""
    torch.manual_seed(77)
    jobs_d, refs = [], []
    # (aligned segments of whole 16-k tiles take the unconditional 16-byte loads with 4 tiles in flight, the others the element-wise checked loads:
    # the fifth job mixes both inside one accumulation, the last one walks 5 tiles - not a multiple of the prefetch depth)
    for M, N, Ks in ((256, 128, (512, 512)), (37, 70, (33,)), (256, 1536, (128,)), (130, 64, (20, 48, 16, 100)), (128, 64, (64, 20, 256)), (64, 192, (80,))):
        C0 = torch.randn(M, N + 6)
        bias = torch.randn(N)
        beta = 0.0 if len(Ks) == 1 else 1.0
        segs_d, acc = [], beta * C0[:, :N].double() + bias.double()
        for K in Ks:
            A = torch.randn((M, K + 4) if a_k else (K, M + 4))
            Bm = torch.randn((N, K + 8) if b_k else (K, N + 8))
            Av = A[:, :K] if a_k else A[:, :M]
            Bv = Bm[:, :K] if b_k else Bm[:, :N]
            acc = acc + (Av if a_k else Av.t()).double() @ (Bv.t() if b_k else Bv).double()
            Ad, Bd = g(A), g(Bm)
            segs_d.append((Ad[:, :K] if a_k else Ad[:, :M], Bd[:, :K] if b_k else Bd[:, :N]))
        Cd = g(C0.clone())
        jobs_d.append(dict(C=Cd[:, :N], segs=segs_d, beta=beta, bias=g(bias)))
        refs.append((Cd, acc.float(), C0, N))
    ops.gemm_multi(jobs_d, a_k=a_k, b_k=b_k)
    for Cd, ref, C0, N in refs:
        close(Cd[:, :N], ref, 2e-5)
        assert torch.equal(Cd[:, N:].cpu(), C0[:, N:])            # columns beyond N untouched


def test_glsr_full_size_keeps_the_scans_apart():
    """GLSRTrainer at hidden 512, B=256 (T=128 >= its 100 decode steps), step > 20: the four extra decoder passes are whole-chip weight-
    stationary launches; queued on a side stream they would be in flight together with the main decoder backward and starve each other
    into the bounded-spin error.  Two steps must finish with finite numbers and a clear sync-error word."""
    from helpers import make_vae_model
    load_package()
    from music_fader_nets_amd.synth import synth_batch
    pkg = load_package()
    m = make_vae_model(512, 128, device=DEV)
    tr = pkg.GLSRTrainer(m, lr=1e-3, beta=0.2)
    b = synth_batch(np.random.RandomState(3), 256, 128, 32)
    step = 5000
    for it in range(2):
        torch.manual_seed(11 + it)
        step, tup = tr.train(step, None, None, None, b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
        assert all(np.isfinite(tup)), tup
    assert m.engine().losses_on_side is False
    assert not m.engine().ops.gru_sync_error()
    assert tup[4] > 0 and tup[5] > 0            # both regularisers were active


# ----------------------------------------------------------------------------------------------
# element-wise gradient slices at hidden 512 (tests/golden/slices.npz, made by the reference itself): c0 / c1 hold per-parameter
# checksums only, which a row permutation or a sign pattern inside one tensor would pass
# ----------------------------------------------------------------------------------------------
def _check_grad_slices(g, pfx, named_grads, tol=5e-4, skip=()):
    """first 2 + last 2 rows and every 97th element of each parameter gradient, at `tol` of the tensor's max"""
    n_rows = n_stride = 0
    for k, G in named_grads:
        got = G.detach().cpu().numpy()
        scale = float(np.abs(got).max())
        if k in skip:
            continue
        ref = g[pfx + "gstride/" + k]
        assert np.abs(got.reshape(-1)[::97] - ref).max() <= tol * max(scale, np.abs(ref).max()) + 1e-7, (pfx, k, "stride-97 sample")
        n_stride += ref.size
        if pfx + "grad/" + k in g:
            ref = g[pfx + "grad/" + k]
            mine = np.concatenate([got[:2], got[-2:]], 0) if (got.ndim == 2 and got.shape[0] >= 8) else got
            assert mine.shape == ref.shape, (k, mine.shape, ref.shape)
            assert np.abs(mine - ref).max() <= tol * max(scale, np.abs(ref).max()) + 1e-7, (pfx, k, "rows")
            n_rows += ref.size
    return n_rows, n_stride


@pytest.mark.parametrize("arith", ["f32", "bf16x6"])
@pytest.mark.parametrize("pfx,sup", [("c0u/", False), ("c0s/", True), ("c1u/", False)])
def test_gradient_slices_vs_reference_at_hidden_512(pfx, sup, arith):
    """hidden 512: per-parameter gradient ROWS and a stride-97 sample of every gradient, plus d loss / d (encoder input) at sampled
    (batch, time) positions = both directions' gate-gradient rows of gru_r / gru_n projected through W_ih, against the reference's own
    backward (unsupervised and supervised loss at B=8, the benchmark shape B=256 / T=256: 128-row tiles, K = 65 280 weight-gradient GEMMs)"""
    pkg = load_package()
    from music_fader_nets_amd.synth import synth_batch
    g = load_golden("slices")
    H, Z, K, B, T, Tr = (int(x) for x in g[pfx + "dims"])
    m = make_model(H, Z, device=DEV, arith=arith)
    tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
    b = synth_batch(np.random.RandomState(0), B, T, Tr)
    lab = b["a"] if sup else None
    batch = tr.prepare_batch(b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"], lab)
    torch.manual_seed(99)
    eps = tr.draw_eps(B, T)
    tup = tr.loss_and_grads(20000, batch, eps)
    np.testing.assert_allclose(tup[0], g[pfx + "loss"][0], rtol=2e-5)
    np.testing.assert_allclose(tr.grad_norm(), g[pfx + "gradnorm"][0], rtol=1e-3)
    ref_keys = {k[len(pfx + "gstride/"):] for k in g if k.startswith(pfx + "gstride/")}
    assert set(tr.flat.names) == ref_keys
    # linear_out_{r,n}.bias: mathematically zero gradient (time-axis softmax), pure rounding noise in both implementations
    n_rows, n_stride = _check_grad_slices(g, pfx, [(k, tr.flat.G[k]) for k in tr.flat.names], skip=("linear_out_r.bias", "linear_out_n.bias"))
    assert n_rows > 30000 and n_stride > 50000
    # encoder input gradient: dgx rows of both directions through W_ih (dgx is stored in PROCESSING order: reverse scans run t = T-1 .. 0)
    eng = m.engine()
    bs, ts = g[pfx + "xg_b"], g[pfx + "xg_t"]
    for e in ("r", "n"):
        ref = g[pfx + "xgrad_" + e]                                # [len(bs)][len(ts)][342]
        dgx_f = eng.buf("enc_dgx_" + e, (T, B, 3 * H))
        dgx_b = eng.buf("enc_dgx_" + e + "_reverse", (T, B, 3 * H))
        Wf, Wb = eng.p["gru_%s.weight_ih_l0" % e].double(), eng.p["gru_%s.weight_ih_l0_reverse" % e].double()
        got = np.zeros_like(ref, dtype=np.float64)
        for i, bi in enumerate(bs):
            for j, t in enumerate(ts):
                got[i, j] = (dgx_f[int(t), int(bi)].double() @ Wf + dgx_b[T - 1 - int(t), int(bi)].double() @ Wb).cpu().numpy()
        assert np.abs(got - ref).max() <= 5e-4 * np.abs(ref).max(), (pfx, e, np.abs(got - ref).max(), np.abs(ref).max())


def test_fader_sibling_at_hidden_512_batch_256_vs_reference():
    """MusicAttrFaderNets at hidden 512, B=256, T=64 (the 128-row tiles of the single-encoder engine) against trainer_fader.py's own
    loss / backward / train() at that size: loss terms, gradient rows + stride-97 samples, one optimisation step"""
    from helpers import make_sibling
    pkg = load_package()
    g = load_golden("slices")
    pfx = "fader/"
    H, Z, B, T, Tr = (int(x) for x in g[pfx + "dims"])
    m = make_sibling("fader", H, Z, device=DEV)
    for k, v in m.state_dict().items():
        vd = v.double()
        np.testing.assert_allclose([vd.sum().item(), vd.abs().sum().item(), (vd * vd).sum().item()], g[pfx + "w0sum/" + k], rtol=1e-9, atol=1e-9, err_msg=k)
    from music_fader_nets_amd.synth import synth_batch
    b = synth_batch(np.random.RandomState(5), B, T, Tr)
    tr = pkg.FaderTrainer(m, lr=1e-3, beta=0.2)
    rd32 = torch.from_numpy(b["r_density"]).float().unsqueeze(-1).to(DEV)       # (B, 1) float32 device tensors, trainer_fader.py:180
    nd32 = torch.from_numpy(b["n_density"]).float().unsqueeze(-1).to(DEV)
    batch = tr.prepare_batch(b["d"], b["r"], b["n"], b["c"], rd32, nd32)
    torch.manual_seed(99)
    eps = tr.draw_eps(B, T)
    tup = tr.loss_and_grads(20000, batch, eps)
    np.testing.assert_allclose(tup, g[pfx + "loss_terms"], rtol=5e-4, atol=1e-9)
    np.testing.assert_allclose(tr.grad_norm(), g[pfx + "gradnorm"][0], rtol=1e-3)
    assert set(tr.flat.names) == {k[len(pfx + "gstride/"):] for k in g if k.startswith(pfx + "gstride/")}
    _check_grad_slices(g, pfx, [(k, tr.flat.G[k]) for k in tr.flat.names])
    torch.manual_seed(99)
    step, t1 = tr.train(19999, None, None, None, b["d"], b["r"], b["n"], b["c"], rd32, nd32)
    np.testing.assert_allclose(t1, g[pfx + "train_tuple"], rtol=5e-4, atol=1e-9)
    for k, v in m.state_dict().items():
        np.testing.assert_allclose([v.double().abs().sum().item()], g[pfx + "w1sum/" + k][1:2], rtol=1e-3, err_msg=k)
    assert not m.engine().ops.gru_sync_error()


@pytest.mark.parametrize("blocks", [8, 32])
def test_step_under_cu_contention_is_bit_identical(blocks):
    """A foreign kernel that HOLDS compute units while a step runs (fn_occupy_cus: `blocks` workgroups with 64 KB of LDS each, relaunched
    back to back on another stream - what an RCCL channel or another process' kernel looks like to the weight-stationary scans, whose
    256 workgroups need every CU): the scan's missing workgroups become resident late, the resident ones spin at their counters.  The
    step must come out bit-identical, the sync-error word must stay clear; the slow-down is printed (scratch/contention.py records it
    at the benchmark shape)."""
    import time
    pkg = load_package()
    from music_fader_nets_amd.synth import synth_batch
    B, T, Tr = 256, 64, 16
    m = make_model(512, 128, device=DEV)
    tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
    b = synth_batch(np.random.RandomState(0), B, T, Tr)
    batch = tr.prepare_batch(b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
    torch.manual_seed(99)
    eps = tr.draw_eps(B, T)
    ops = m.engine().ops

    def run(contend):
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if contend:
            with torch.cuda.stream(side):
                for _ in range(24):
                    ops.occupy_cus(blocks, 64 * 1024, 1_000_000)        # ~0.5 ms each, back to back: the CUs stay taken for the whole step
        t = tr.loss_and_grads(20000, batch, eps)
        torch.cuda.synchronize()
        return t, tr.flat.grad.clone(), time.perf_counter() - t0

    run(False)
    t_ref, g_ref, dt_ref = run(False)
    t_c, g_c, dt_c = run(True)
    assert not ops.gru_sync_error()
    assert t_c == t_ref and torch.equal(g_c, g_ref)
    print("contention: %d CUs held -> step %.2f ms vs %.2f ms alone" % (blocks, dt_c * 1e3, dt_ref * 1e3))


@pytest.mark.parametrize("spec", [dict(dw_order="side"), dict(dw_order="after"), dict(prepack_h0=False), dict(losses_early=True),
                                  dict(dw_order="side_late", prepack_h0=False, losses_early=True)])
def test_schedule_switches_change_no_bit_of_the_step(spec):
    """Engine.dw_order / prepack_h0 / losses_early decide WHERE launches are issued (which lane, in front of or behind which launch), never what they
    compute: three captured optimisation steps at the benchmark's hidden size leave bit-identical parameters and loss terms whatever the schedule
    (a lane that reads a buffer before its producer has finished shows up here)."""
    pkg = load_package()
    from music_fader_nets_amd.synth import synth_batch
    B, T, Tr = 256, 64, 32

    def run(sw):
        torch.manual_seed(5)
        m = make_model(512, 128, device=DEV)
        tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
        for k, v in sw.items():
            assert hasattr(m.engine(), k)
            setattr(m.engine(), k, v)
        b = synth_batch(np.random.RandomState(0), B, T, Tr)
        batch = tr.prepare_batch(b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
        torch.manual_seed(99)
        eps = tr.draw_eps(B, T)
        step, tups = 20000, []
        for _ in range(4):                       # eager, capture + replay, replay, replay
            b0, Bg = tr.step_device(step, batch, eps)
            tups.append(tr._tuple8(b0, Bg, False))
            step += 1
        torch.cuda.synchronize()
        assert not m.engine().ops.gru_sync_error()
        return tups, tr.flat.param.clone()

    t_ref, p_ref = run({})
    t_sw, p_sw = run(spec)
    assert t_sw == t_ref
    assert torch.equal(p_sw, p_ref)


def test_entry_driver_runs_an_epoch_from_the_reference_config(tmp_path, capsys):
    """`python train_gmm.py --config <the reference's gmm_model_config.json> --synthetic --epochs 1`: the module body of trainer_gmm.py
    (:21-96, :613) - config, model, resume, loaders, training_phase - on the HIP path, printing the reference's log format; a second run
    resumes from params/<name>.pt"""
    import os
    load_package()
    from music_fader_nets_amd.train import main
    cfg = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gmm_model_config.json")
    argv = ["--config", cfg, "--synthetic", "--synthetic-songs", "320", "--seq-len", "48", "--epochs", "1", "--out", str(tmp_path), "--seed", "3"]
    step = main(argv)
    out = capsys.readouterr().out
    assert step == 3 + 2                                       # 3 VGMIDI batches (72 songs: 32 + 32 + 8) + 2 Yamaha batches of 128 (256 songs)
    for needle in ("Save path: ", "Epoch 1 / 1", "batch loss: ", "train loss by term - D: ", "test loss by term - D: ", "KLD-C: ", "Saving model...",
                   "Model saved as "):
        assert needle in out, (needle, out)
    path = os.path.join(str(tmp_path), "params", "music_attr_vae_reg_gmm_long_v.pt")
    sd = torch.load(path)
    assert "gru_c.weight_ih_l0" in sd and "linear_out_g.weight" in sd and all(not v.is_cuda for v in sd.values())     # the reference's key set, CPU tensors
    assert os.path.isdir(os.path.join(str(tmp_path), "log"))
    main(argv)
    assert "Loading " + path in capsys.readouterr().out


@pytest.mark.parametrize("family", ["vae", "singlevae", "cvae", "fader", "glsr"])
def test_epoch_driver_v2_vs_reference_training_phase(family, tmp_path):
    """``training_phase`` of trainer.py / trainer_singlevae.py / trainer_cvae.py / trainer_fader.py / trainer_glsr.py (two epochs, executed
    unmodified for tests/golden/epoch_v2.npz) on the HIP path: same log lines, same checkpoint"""
    from helpers import check_epoch_v2_run
    m = check_epoch_v2_run(load_package(), family, load_golden("epoch_v2"), tmp_path, device=DEV, noise=NOISE_PARAMS)
    assert not m.engine().ops.gru_sync_error()


@pytest.mark.parametrize("family", ["vae", "singlevae", "cvae", "fader", "glsr"])
def test_entry_driver_v2_runs_an_epoch_from_model_config_v2(family, tmp_path, capsys):
    """`python train_gmm.py --config <the reference's model_config_v2.json> --model <family> --synthetic --epochs 1`: the module bodies of the
    five trainers that open model_config_v2.json (trainer.py:20-76 ...) - config (no ``num_clusters`` in it), model, resume, loaders,
    training_phase - on the HIP path at the config's own size (hidden 512, batch 128)"""
    import os
    load_package()
    from music_fader_nets_amd.train import main, read_config
    cfg = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_config_v2.json")
    assert "num_clusters" not in read_config(cfg, family)
    with pytest.raises(KeyError):
        read_config(cfg, "gmm")                                 # trainer_gmm.py indexes args['num_clusters']: that script needs the other file
    T = "112" if family == "glsr" else "48"                     # the GLSR decodes are teacher forced for 100 steps
    argv = ["--config", cfg, "--model", family, "--synthetic", "--synthetic-songs", "320", "--seq-len", T, "--epochs", "1", "--out", str(tmp_path), "--seed", "3"]
    if family == "fader":
        argv.append("--bf16x6")                                 # the bf16 x 6 arithmetic is reachable from the entry driver (= --arith bf16x6)
    step = main(argv)
    out = capsys.readouterr().out
    assert step == 2                                            # 256 training songs in batches of 128
    needles = ["Save path: ", "Train / Validation / Test", "256 32 32", "Epoch 1 / 1", "batch loss: ", "train loss by term - D: ", "test loss by term - D: ", "Model saved as "]
    needles += ["RA: "] if family == "fader" else ["RD: "]
    needles += ["Saving model..."] if family in ("vae", "singlevae", "glsr") else []
    for needle in needles:
        assert needle in out, (needle, out)
    path = os.path.join(str(tmp_path), "params", "music_attr_vae_singlevae_8.pt.pt")       # the config's name already ends in .pt (reproduced)
    sd = torch.load(path)
    assert "linear_out_g.weight" in sd and all(not v.is_cuda for v in sd.values())
    main(argv)
    assert "Loading " + path in capsys.readouterr().out


def test_direct_calls_have_autograd(small):
    """encode / sub_decoders / global_decoder / approx_qy_x called directly in train mode: one autograd node each whose backward runs the
    matching part of the HIP backward (the reference allows such calls anywhere, gmm_model.py:82-218)"""
    from helpers import check_direct_call_autograd
    pkg = load_package()
    m = make_model(64, 32, sd_from(small, "w0/"), device=DEV)
    check_direct_call_autograd(pkg, m, small, DEV, tol=5e-4)
    assert not m.engine().ops.gru_sync_error()


@pytest.mark.parametrize("kind", ["single", "cvae", "fader"])
def test_sibling_forward_has_autograd(kind):
    """single-encoder drop-ins in a reference-style loop (forward -> torch loss -> loss.backward() -> optimizer.step()) on the HIP kernels"""
    from helpers import check_sibling_autograd, make_sibling, sibling_golden
    pkg = load_package()
    g = sibling_golden(kind)
    H, Z = int(g["dims"][0]), int(g["dims"][1])
    m = make_sibling(kind, H, Z, device=DEV)
    check_sibling_autograd(pkg, kind, m, g, DEV, tol_grad=5e-4)
    assert not m.engine().ops.gru_sync_error()
