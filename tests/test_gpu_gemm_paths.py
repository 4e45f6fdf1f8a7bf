"""The fp32 GEMMs of csrc/gemm.hip other than the LDS-free NT kernel - the LDS-staged gemm_kernel in its five tile shapes, four layouts and two load
paths, gemm_multi_kernel, gemm_tn_kernel / gemm_tn_lean_kernel (also behind fn_gru_dwhh_f32) and the two slab reductions - bit for bit on integers and
per 16 x 16 tile against float64.

The cases, the references, the mirror of the dispatch and the checkers are tests/helpers_gemm.py; tests/test_gemm_reference.py shows on the CPU that
the tables reach what their ids claim, that the mirror agrees with the library's own dispatch plan (fn_gemm_plan), that the float32 restatement passes
and that planted faults are rejected.  Every case here asserts through the mirror, on the real device addresses and leading dimensions, that it reaches
the kernel instance, load path, grid form and reduction it names - and that the library's plan for the very same tensors says so too -, runs
both passes and prints its line of profiles/gemm_fp64_errors.txt.  The arithmetic of the kernel table is set to fp32 (a table of its own): the
bf16 x 6 kernels have their own tests."""
import ctypes as C

import pytest
import torch

from helpers_gemm import (DWHH_CASES, G16, G32, G128, G3264, G6416, GEMM_CASES, GEMM_F, GEMM_SENTINEL, MULTI_CASES, assert_dwhh_mirror_matches_library,
                          assert_mirror_matches_library, assert_multi_plan_matches_case, assert_plan_matches_case, c_buffer, case_family, case_plan, check, dwhh_case_plan, dwhh_line, dwhh_operands, dwhh_plan, dwhh_problem,
                          gemm_instance, gemm_line, gemm_problem, multi_case_plan, multi_line, multi_problems, stored)
from mfn_import import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("exact", "normal")


@pytest.fixture(scope="module")
def ops():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    o = HipOps(torch.device(DEV))
    o.dw_x6 = False                 # the fp32 kernels are what this file is about
    return o


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))          # as hipops._mat


def _view(t, off, ld):
    """t [R][Cc] on the device as rows of `ld` floats that start `off` floats into a 16-byte aligned, NaN-filled allocation"""
    R, Cc = t.shape
    assert ld >= Cc
    buf = torch.full((off + R * ld + 4,), float("nan"), device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + R * ld].view(R, ld)[:, :Cc]
    v.copy_(t)
    return v


def _vec(t, off=0):
    if t is None:
        return None
    buf = torch.full((off + t.numel(),), float("nan"), device=DEV)
    v = buf[off:]
    v.copy_(t)
    return v


def _ws(ops, nbytes):
    return ops.workspace(nbytes, "gemm") if nbytes else None


def _p(t):
    return 0 if t is None else t.data_ptr()


def _run_gemm(ops, case, prob, lean=None):
    """one launch of the case on the problem's operands -> (C buffer on the CPU, the mirror's plan on the real addresses)"""
    M, N = case["M"], case["N"]
    a, b = prob["pieces"][0]
    As, Bs = stored(case, a, b)
    A, Bm = _view(As, case["a_off"], case["lda"]), _view(Bs, case["b_off"], case["ldb"])
    bias = _vec(prob["bias"], case["bias_off"])
    cbuf = c_buffer(prob, case["c0"], case["ldc"], DEV)
    Cv = cbuf[:M, case["c0"]:case["c0"] + N]
    assert (_ld(A), _ld(Bm), _ld(Cv)) == (case["lda"], case["ldb"], case["ldc"])
    ws = _ws(ops, ops.lib.fn_gemm_ws_bytes(M, N, case["splitk"]))
    lean = case["lean"] if lean is None else lean
    plan = gemm_instance(case["a_k"], case["b_k"], M, N, case["K"], _ld(A), _ld(Bm), _ld(Cv), (_p(A), _p(Bm), _p(Cv), _p(bias), _p(ws)), case["splitk"], lean)
    # ... and the mirror is what the library itself decides for these tensors (fn_gemm_plan through the argument preparation of ops.gemm)
    assert_mirror_matches_library(plan, ops.gemm_plan(A, Bm, Cv, a_k=case["a_k"], b_k=case["b_k"], bias=bias, splitk=case["splitk"], lean=lean), M, N, case["id"])
    ops.gemm(A, Bm, Cv, a_k=case["a_k"], b_k=case["b_k"], alpha=case["alpha"], beta=case["beta"], bias=bias, splitk=case["splitk"], lean=lean)
    torch.cuda.synchronize()
    assert ws is None or _p(_ws(ops, 4)) == _p(ws)                   # the workspace the mirror saw is the one the launch used
    return cbuf.cpu(), plan


@pytest.mark.parametrize("case", GEMM_CASES, ids=[c["id"] for c in GEMM_CASES])
def test_gemm_paths_exact_and_every_tile_vs_fp64(ops, case):
    """fn_gemm_f32 on the staged kernel (five tile shapes x layouts x load_fast / load_checked, split-K with a checked last range, nk against the prefetch
    depth) and on gemm_tn_kernel / the lean instance (every prologue / steady / drain / leftover count, ragged tiles, the column-window clamp, 3-D and 1-D
    grids, both slab reductions and their second grid-stride trip): integers bit for bit, normals within GEMM_F x max(e_ref, 2**-23) in every tile,
    nothing written outside the [M][N] view; the lean instance gives the default's bits."""
    fam = case_family(case)
    res, plan = {}, None
    for mode in MODES:
        prob = gemm_problem(case, mode)
        cbuf, plan = _run_gemm(ops, case, prob)
        assert plan == case_plan(case)                  # the real addresses and leading dimensions reach what the nominal layout does ...
        assert_plan_matches_case(case, plan)            # ... which is what the id names
        res[mode] = check(prob, cbuf, case["c0"], GEMM_F[fam])
        if case["lean"]:
            cdef, pdef = _run_gemm(ops, case, prob, lean=False)
            assert pdef["kernel"] == "gemm_tn_kernel" and dict(pdef, kernel=0, family=0, steps=0) == dict(plan, kernel=0, family=0, steps=0)
            assert torch.equal(cbuf.view(torch.int32), cdef.view(torch.int32)), "%s: the lean instance and the default differ (%s)" % (case["id"], mode)
    print()
    print(gemm_line(case, plan, res))


@pytest.mark.parametrize("case", DWHH_CASES, ids=[c["id"] for c in DWHH_CASES])
def test_gru_dwhh_exact_and_every_tile_vs_fp64(ops, case):
    """fn_gru_dwhh_f32 as one split-A launch (H = 64: the dghn band a ragged 64 rows of the second tile; H = 128: three tiles) and as two products (H = 96),
    1, 4 and 8 K ranges asked for, beta in {0, 1}, default and lean; dgx carries other values in its unused columns [2H, 3H)"""
    H, rows = case["H"], case["rows"]
    res, plan = {}, None
    for mode in MODES:
        prob = dwhh_problem(case, mode)
        dgx, dghn, hp, _ = dwhh_operands(case, mode)
        dgx, dghn, hp = dgx.to(DEV), dghn.to(DEV), hp.to(DEV)
        cbuf = c_buffer(prob, 0, H, DEV)
        dW = cbuf[:3 * H]
        ws = _ws(ops, int(ops.lib.fn_gru_dwhh_ws_bytes(H, case["splitk"])))
        plan = dwhh_plan(H, rows, (_p(dgx), _p(dghn), _p(hp), _p(dW), _p(ws)), case["splitk"], case["lean"])
        assert plan == dwhh_case_plan(case) and plan["form"] == case["form"]
        assert_dwhh_mirror_matches_library(plan, ops.gru_dwhh_plan(dgx, dghn, hp, dW, splitk=case["splitk"], lean=case["lean"]), H, case["id"])
        ops.gru_dwhh(dgx, dghn, hp, dW, beta=case["beta"], splitk=case["splitk"], lean=case["lean"])
        torch.cuda.synchronize()
        res[mode] = check(prob, cbuf.cpu(), 0, GEMM_F["dwhh"])
    print()
    print(dwhh_line(case, plan, res))


def _multi_jobs(case, probs):
    """device views, C buffers and the addresses of one fn_gemm_multi case"""
    a_k, b_k = case["lay"]
    jobs, bufs, ptrs = [], [], []
    for j, prob in zip(case["jobs"], probs):
        segs, pj = [], []
        for (K, av, bv, _), (a, b) in zip(j["segs"], prob["pieces"]):
            As, Bs = (a if a_k else a.t()), (b.t() if b_k else b)
            A = _view(As, av[0], av[1] if av[1] is not None else As.shape[1])
            Bm = _view(Bs, bv[0], bv[1] if bv[1] is not None else Bs.shape[1])
            segs.append((A, Bm))
            pj.append((_p(A), _p(Bm)))
        cbuf = c_buffer(prob, j["c0"], j["ldc"], DEV)
        jobs.append(dict(C=cbuf[:j["M"], j["c0"]:j["c0"] + j["N"]], segs=segs, beta=j["beta"], bias=_vec(prob["bias"])))
        bufs.append(cbuf)
        ptrs.append(pj)
    return jobs, bufs, ptrs


@pytest.mark.parametrize("case", MULTI_CASES, ids=[c["id"] for c in MULTI_CASES])
def test_gemm_multi_exact_and_every_tile_vs_fp64(ops, case):
    """fn_gemm_multi in all four layouts: segments of 1 .. 5 tiles on the four-deep ring (load_fast) and on the checked loop, K = 3 and 16, fast and
    checked segments in one accumulation, four segments with beta = 1 and a bias, jobs narrower than the launch's grid, 12 jobs in one launch and 13 through
    the wrapper, ragged tiles with row-contiguous operands, strided A, B and C views"""
    res, plan = {}, None
    for mode in MODES:
        probs = multi_problems(case, mode)
        jobs, bufs, ptrs = _multi_jobs(case, probs)
        plan = multi_case_plan(case, ptrs)
        assert plan == multi_case_plan(case)
        assert_multi_plan_matches_case(case, plan)
        ops.gemm_multi(jobs, a_k=case["lay"][0], b_k=case["lay"][1])
        torch.cuda.synchronize()
        out = [check(prob, buf.cpu(), j["c0"], GEMM_F["multi"]) for prob, buf, j in zip(probs, bufs, case["jobs"])]
        if mode == "exact":
            res[mode] = sum(out)
        else:
            jx = max(range(len(out)), key=lambda i: out[i][0])
            res[mode] = (out[jx][0], jx, out[jx][1], out[jx][2])
    print()
    print(multi_line(case, plan, res))


# ---- the bit-identity claims written in gemm.hip, on the bare product (alpha 1, beta 0, no bias) ------------------------------------------------------
def _bare(ops, A, Bm, want_kernel, want_loads=None):
    M, N, K = A.shape[0], Bm.shape[0], A.shape[1]
    Cm = torch.full((M, N), float("nan"), device=DEV)
    plan = gemm_instance(True, True, M, N, K, _ld(A), _ld(Bm), _ld(Cm), (_p(A), _p(Bm), _p(Cm), 0, 0), 1, False)
    assert plan["kernel"] == want_kernel, plan
    if want_loads is not None:
        assert plan["loads"][want_loads] > 0 and plan["loads"]["checked" if want_loads == "fast" else "fast"] == 0, plan
    assert_mirror_matches_library(plan, ops.gemm_plan(A, Bm, Cm, a_k=True, b_k=True), M, N, want_kernel)
    ops.gemm(A, Bm, Cm, a_k=True, b_k=True)
    torch.cuda.synchronize()
    return Cm


def test_the_five_staged_instances_give_the_same_bits(ops):
    """"same k order: bit-identical" (fn_gemm_f32 on the 32 x 64, 64 x 64 x 32 and 64 x 16 instances), asked of all five: one pair of NT operands, K = 128, and
    the sub-blocks of its rows that the dispatch sends to each instance - <64,64,16> through 16 appended columns of zeros, which add exact zeros"""
    gen = torch.Generator().manual_seed(128)
    A, Bm = torch.randn(1930, 128, generator=gen).to(DEV), torch.randn(2040, 128, generator=gen).to(DEV)
    c128 = _bare(ops, A, Bm, G128)
    c3264 = _bare(ops, A[:70], Bm[:50], G3264)
    c32 = _bare(ops, A[:50], Bm[:50], G32)
    c6416 = _bare(ops, A[:70], Bm[:16], G6416)
    Az, Bz = torch.zeros(70, 144, device=DEV), torch.zeros(50, 144, device=DEV)
    Az[:, :128], Bz[:, :128] = A[:70], Bm[:50]
    c16 = _bare(ops, Az, Bz, G16)
    assert not bool(torch.isnan(c128).any())
    assert torch.equal(c128[:70, :50], c3264), "<128,128,32> and <32,64,32> differ"
    assert torch.equal(c3264[:50], c32), "<32,64,32> and <64,64,32> differ"
    assert torch.equal(c3264[:, :16], c6416), "<32,64,32> and <64,16,16> differ"
    assert torch.equal(c3264, c16), "<32,64,32> and <64,64,16> differ"
    ref = A[:70].double() @ Bm[:50].double().t()
    assert float((c3264.double() - ref).abs().max()) < 1e-4
    print()
    print("bit-identity: <128,128,32> == <32,64,32> == <64,64,32> == <64,16,16> == <64,64,16> on the same operand values (K = 128)")


@pytest.mark.parametrize("kernel,M,N,K", [(G16, 70, 50, 80), (G3264, 70, 50, 128), (G32, 50, 70, 160), (G6416, 70, 16, 80)])
def test_load_fast_and_load_checked_give_the_same_bits(ops, kernel, M, N, K):
    """the same values through a copy that starts one float off a 16-byte boundary: the checked loads, the two-deep loop, the same sums"""
    gen = torch.Generator().manual_seed(K + M)
    A, Bm = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen)
    fast = _bare(ops, A.to(DEV), Bm.to(DEV), kernel, "fast")
    chk_a = _bare(ops, _view(A, 1, K), Bm.to(DEV), kernel, "checked")
    chk_b = _bare(ops, A.to(DEV), _view(Bm, 1, K), kernel, "checked")
    assert torch.equal(fast, chk_a) and torch.equal(fast, chk_b)
    print()
    print("bit-identity: %s load_fast == load_checked (A one float off; B one float off) at %d x %d x %d" % (kernel, M, N, K))


def test_a_single_segment_multi_job_gives_the_staged_kernels_bits(ops):
    """gemm_multi_kernel's four-deep ring and the staged kernel's two-deep one: "the order of the summation is the same" """
    gen = torch.Generator().manual_seed(7)
    for M, N, K in ((70, 50, 80), (130, 70, 64), (64, 64, 16)):
        A, Bm = torch.randn(M, K, generator=gen).to(DEV), torch.randn(N, K, generator=gen).to(DEV)
        single = _bare(ops, A, Bm, G16 if K < 128 else G3264, "fast")
        Cm = torch.full((M, N), float("nan"), device=DEV)
        ops.gemm_multi([dict(C=Cm, segs=[(A, Bm)])], a_k=True, b_k=True)
        Cc = torch.full((M, N), float("nan"), device=DEV)
        ops.gemm_multi([dict(C=Cc, segs=[(_view(A.cpu(), 1, K), Bm)])], a_k=True, b_k=True)          # ... and its checked loop
        torch.cuda.synchronize()
        assert torch.equal(single, Cm) and torch.equal(single, Cc)
        print()
        print("bit-identity: single-segment gemm_multi job (fast loop; checked loop) == staged kernel at %d x %d x %d" % (M, N, K))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_their_code_and_write_nothing(ops):
    from music_fader_nets_amd import _lib
    lib, st = ops.lib, ops.stream()
    E_NULL, E_SHAPE, E_WS, E_COUNT = _lib.FN_E_NULL, _lib.FN_E_SHAPE, _lib.FN_E_WORKSPACE, _lib.FN_E_COUNT
    A, Bm = torch.ones(8, 8, device=DEV), torch.ones(8, 8, device=DEV)
    Cm = torch.full((8, 8), GEMM_SENTINEL, device=DEV)
    ws = torch.zeros(4096, device=DEV)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def gemm(A=A, Bm=Bm, Cm=Cm, M=8, N=8, K=8, lda=8, ldb=8, ldc=8, splitk=1, ws=None, wsb=0):
        return lib.fn_gemm_f32(1, 1, M, N, K, 1.0, vp(A), lda, vp(Bm), ldb, 0.0, vp(Cm), ldc, None, splitk, vp(ws), wsb, st)

    assert gemm(A=None) == E_NULL and gemm(Bm=None) == E_NULL and gemm(Cm=None) == E_NULL
    assert gemm(ldc=7) == E_SHAPE and gemm(lda=0) == E_SHAPE and gemm(ldb=0) == E_SHAPE and gemm(M=0) == E_SHAPE and gemm(K=0) == E_SHAPE
    assert gemm(splitk=2) == E_WS and gemm(splitk=2, ws=ws, wsb=2 * 8 * 8 * 4 - 4) == E_WS
    assert gemm(splitk=2 | _lib.GEMM_LEAN) == E_WS

    def multi(n_jobs=1, jobs="one", a_k=1, b_k=1, **kw):
        arr = (_lib.FnGemmJob * 13)()
        for d in arr:
            d.M, d.N, d.C, d.ldc, d.bias, d.beta, d.n_seg = 8, 8, vp(Cm), 8, None, 0.0, 1
            d.seg[0].A, d.seg[0].lda, d.seg[0].B, d.seg[0].ldb, d.seg[0].K = vp(A), 8, vp(Bm), 8, 8
        for k, v in kw.items():
            if k in ("A", "lda", "B", "ldb", "K"):
                setattr(arr[0].seg[0], k, v)
            else:
                setattr(arr[0], k, v)
        return lib.fn_gemm_multi(a_k, b_k, None if jobs is None else arr, n_jobs, st)

    assert multi(jobs=None) == E_NULL and multi(C=None) == E_NULL and multi(A=None) == E_NULL and multi(B=None) == E_NULL
    assert multi(n_jobs=0) == E_COUNT and multi(n_jobs=13) == E_COUNT
    assert multi(n_seg=0) == E_SHAPE and multi(n_seg=5) == E_SHAPE and multi(ldc=7) == E_SHAPE and multi(M=0) == E_SHAPE and multi(K=0) == E_SHAPE
    assert multi(lda=7) == E_SHAPE and multi(ldb=7) == E_SHAPE                                   # below K (K-contiguous operands)
    assert multi(a_k=0, b_k=0, K=4, lda=7) == E_SHAPE and multi(a_k=0, b_k=0, K=4, ldb=7) == E_SHAPE      # below M / N (row-contiguous operands)

    H = 8
    dgx, dghn, hp = torch.ones(4, 3 * H, device=DEV), torch.ones(4, H, device=DEV), torch.ones(4, H, device=DEV)
    dW = torch.full((3 * H, H), GEMM_SENTINEL, device=DEV)

    def dwhh(dgx=dgx, dghn=dghn, hp=hp, dW=dW, rows=4, H=H, splitk=1, ws=None, wsb=0):
        return lib.fn_gru_dwhh_f32(vp(dgx), vp(dghn), vp(hp), rows, H, 0.0, vp(dW), splitk, vp(ws), wsb, st)

    assert dwhh(dgx=None) == E_NULL and dwhh(dghn=None) == E_NULL and dwhh(hp=None) == E_NULL and dwhh(dW=None) == E_NULL
    assert dwhh(rows=0) == E_SHAPE and dwhh(rows=-3) == E_SHAPE and dwhh(rows=1 << 31) == E_SHAPE and dwhh(H=0) == E_SHAPE
    assert dwhh(splitk=4) == E_WS and dwhh(splitk=4, ws=ws, wsb=4 * 3 * H * H * 4 - 4) == E_WS
    torch.cuda.synchronize()
    assert bool((Cm == GEMM_SENTINEL).all()) and bool((dW == GEMM_SENTINEL).all())
    # and the same calls are accepted once the argument is right
    assert gemm(splitk=2, ws=ws, wsb=2 * 8 * 8 * 4) == 0 and multi(n_jobs=12) == 0 and dwhh(splitk=4, ws=ws, wsb=4 * 3 * H * H * 4) == 0
    torch.cuda.synchronize()
    assert bool((Cm == 8.0).all()) and bool((dW == 4.0).all())
