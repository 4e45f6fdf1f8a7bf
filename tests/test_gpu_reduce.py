"""The glue kernels of the training step against float64 on an MI355X: the embedding gradient (fn_token_sort, fn_embed_grad_sorted, fn_embed_grad_f32),
time_sum, colsum, colsum_multi, sum, axpy, transpose (csrc/embed.hip, the end of csrc/gemm.hip) and the optimiser (sumsq, step_params, clip_adam:
csrc/optim.hip).

The case tables, the float64 references, the bounds and the checkers are tests/helpers_reduce.py; tests/test_reduce_reference.py shows on the CPU
that the tables have the properties their ids claim, that the checkers accept the fp32 restatement and that they reject planted faults.  Every
summation kernel runs an integer pass that must be bit-exact and a random pass against the derived bound (n + 2) 2**-24 sum |terms|; every test
prints its lines of profiles/reduce_fp64_errors.txt."""
import numpy as np
import pytest
import torch

from helpers_reduce import (ADAM_CASES, AXPY_ALPHA, AXPY_N, CM_JOBS, CM_MAX_JOBS, COLSUM_CASES, EG_CASES, EG_MAX_JOBS, PASSES, RANDN_PASS, SENTINEL, SP_STEPS, SP_T, SUM_N,
                            SUMSQ_N, TIME_SUM_CASES, TRANSPOSE_SHAPES, adam_line, check_adam, check_colsum_multi, check_embed_case, check_pass, check_sort_image,
                            cm_inputs, cm_job, eg_inputs, eg_table, job_name, line, run_adam, run_axpy, run_colsum, run_colsum_multi, run_embed_onecall,
                            run_embed_sorted, run_step_params, run_sum, run_sumsq, run_time_sum, run_transpose, token_sort_ints)
from mfn_import import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    return HipOps(torch.device(DEV))


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.numpy().view(np.int32), b.numpy().view(np.int32))


# ---- embedding gradient ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", PASSES)
@pytest.mark.parametrize("case", EG_CASES, ids=[c["id"] for c in EG_CASES])
def test_embed_grad_vs_fp64(ops, case, kind):
    """one sort + one fn_embed_grad_sorted launch with every job of the case (forward, reverse, shift -1 with an absent / a present start token;
    plain, strided and transposed outputs into sentinel-filled buffers): the sort image equals numpy's stable argsort and the exclusive cumsums,
    every table is bit-exact on integers and within the summation bound on normals, rows of tokens that no step consumes are exactly zero, nothing
    is written outside a view; a second launch and the one-call form fn_embed_grad_f32 give the same bits."""
    V, rows = case["V"], case["B"] * case["T"]
    handle, bufs = run_embed_sorted(ops, case, kind, DEV)
    torch.cuda.synchronize()
    assert int(ops.lib.fn_token_sort_ints(rows, V)) == token_sort_ints(rows, V) == handle["img"].numel()
    check_sort_image(case["id"], handle["img"], eg_inputs(case, kind)["idx"].numpy(), V)
    worst = check_embed_case(case, kind, bufs)
    _, bufs2 = run_embed_sorted(ops, case, kind, DEV)
    for ji, (a, b) in enumerate(zip(bufs, bufs2)):
        assert _bits_equal(a, b), "%s job %d: two launches differ" % (case["id"], ji)
    for ji, j in enumerate(case["jobs"]):
        one = run_embed_onecall(ops, case, kind, ji, DEV)
        assert bool((one[V:] == SENTINEL).all()), "%s job %d: the one-call form wrote past V rows" % (case["id"], ji)
        assert _bits_equal(one[:V], eg_table(case, j, bufs[ji])), "%s job %d (%s): the one-call form and the sorted form differ" % (case["id"], ji, job_name(j))
        assert _bits_equal(one, run_embed_onecall(ops, case, kind, ji, DEV)), "%s job %d (%s): two one-call launches differ" % (case["id"], ji, job_name(j))
    print()
    print(line("embed_grad", "%s %d jobs" % (case["id"], len(case["jobs"])), kind, worst[0], "job %d %s" % (worst[1], worst[2]) if kind == RANDN_PASS else ""))


def test_embed_grad_rejects_bad_shapes(ops):
    """V = 1025, N3 = 6 and nine jobs are errors of the ABI, in the sort, the sorted form and the one-call form"""
    B, T = 3, 5
    idx = torch.zeros(B, T, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="fn_token_sort"):
        ops.token_sort(idx, 1025)
    with pytest.raises(RuntimeError, match="fn_embed_grad_f32"):
        ops.embed_grad(torch.zeros(T, B, 4, device=DEV), idx, 0, 0, 0, 1025, torch.zeros(1025, 4, device=DEV))
    with pytest.raises(RuntimeError, match="fn_embed_grad_f32"):
        ops.embed_grad(torch.zeros(T, B, 6, device=DEV), idx, 0, 0, 0, 4, torch.zeros(4, 6, device=DEV))
    h = ops.token_sort(idx, 4)
    with pytest.raises(RuntimeError, match="fn_embed_grad_sorted"):
        ops.embed_grad_sorted(h, [dict(dgx=torch.zeros(T, B, 6, device=DEV), out=torch.zeros(4, 6, device=DEV))])
    dgx = torch.zeros(T, B, 4, device=DEV)
    jobs = [dict(dgx=dgx, out=torch.zeros(4, 4, device=DEV)) for _ in range(EG_MAX_JOBS + 1)]
    with pytest.raises(RuntimeError, match="fn_embed_grad_sorted"):
        ops.embed_grad_sorted(h, jobs)
    ops.embed_grad_sorted(h, jobs[:EG_MAX_JOBS])                      # eight are fine
    torch.cuda.synchronize()


# ---- reductions -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", PASSES)
@pytest.mark.parametrize("case", TIME_SUM_CASES, ids=[c["id"] for c in TIME_SUM_CASES])
def test_time_sum_vs_fp64(ops, case, kind):
    """every T % 4 tail at one float4 column and at 888, and the second trip of the grid-stride loop"""
    w, at = run_time_sum(ops, case, kind, DEV)
    print()
    print(line("time_sum", case["id"], kind, w, at))


def test_time_sum_rejects_m_not_multiple_of_4(ops):
    with pytest.raises(RuntimeError, match="fn_time_sum_f32"):
        ops.time_sum(torch.zeros(3, 6, device=DEV), torch.zeros(6, device=DEV))


@pytest.mark.parametrize("kind", PASSES)
@pytest.mark.parametrize("case", COLSUM_CASES, ids=[c["id"] for c in COLSUM_CASES])
def test_colsum_vs_fp64(ops, case, kind):
    """row counts around the chunk thresholds (16385: empty last chunks), column counts around the 256-thread block, ld > N, beta = 0 on a NaN out
    (never read), beta = 1 and 0.5"""
    w, at = run_colsum(ops, case, kind, DEV)
    print()
    print(line("colsum", case["id"], kind, w, ("beta %g column %d" % at) if kind == RANDN_PASS else ""))


@pytest.mark.parametrize("kind", PASSES)
def test_colsum_multi_vs_fp64(ops, kind):
    """64 jobs of mixed widths and heights in ONE launch (narrow jobs beside the widest: their surplus workgroups must write nothing), ld > N,
    beta = 0 on a NaN out and beta = 1; then all 65 through HipOps.colsum_multi (two launches), the same bits; and every job against fn_colsum_f32
    within the bound (another summation order: not bit-equal by contract)"""
    assert len(CM_JOBS) == CM_MAX_JOBS + 1
    outs = run_colsum_multi(ops, kind, 0, CM_MAX_JOBS, DEV)
    worst = check_colsum_multi(kind, 0, outs)
    outs65 = run_colsum_multi(ops, kind, 0, len(CM_JOBS), DEV)
    w65 = check_colsum_multi(kind, 0, outs65)
    for i, (a, b) in enumerate(zip(outs, outs65)):
        assert _bits_equal(a, b), "job %d differs between the 64-job and the 65-job call" % i
    inp = cm_inputs(kind)
    for i in range(len(CM_JOBS)):
        X, out0, beta, (ref, sabs, n) = inp[i]
        out = out0.clone().to(DEV) if beta != 0.0 else torch.full((X.shape[1],), float("nan"), device=DEV)
        ops.colsum(X.to(DEV), out, beta=beta)
        one = out.cpu()
        check_pass("colsum (twin of colsum_multi job %d) %s" % (i, kind), kind, one, ref, sabs, n)
        # the two kernels against each other: each lies within the bound of ref64, possibly on opposite sides - twice the bound (triangle inequality)
        check_pass("colsum_multi vs colsum, job %d %s %s" % (i, cm_job(i), kind), kind, outs65[i], one.double().numpy(), 2.0 * sabs, n)
    print()
    print(line("colsum_multi", "64 jobs in one launch", kind, worst[0], ("job %d column %d" % worst[1]) if kind == RANDN_PASS else ""))
    print(line("colsum_multi", "65 jobs in two launches", kind, w65[0], ("job %d column %d" % w65[1]) if kind == RANDN_PASS else ""))


@pytest.mark.parametrize("kind", PASSES)
@pytest.mark.parametrize("n", SUM_N)
def test_sum_vs_fp64(ops, n, kind):
    w, _ = run_sum(ops, n, kind, DEV)
    print()
    print(line("sum", "n%d-scale0.5" % n, kind, w))


@pytest.mark.parametrize("kind", PASSES)
@pytest.mark.parametrize("n", SUMSQ_N)
def test_sumsq_vs_fp64(ops, n, kind):
    """the n % 4 tail that block 0 handles, fewer float4 than threads, and four trips of the grid-stride loop"""
    w, _ = run_sumsq(ops, n, kind, DEV)
    print()
    print(line("sumsq", "n%d" % n, kind, w))


def test_sumsq_rejects_a_misaligned_view(ops):
    g = torch.zeros(64, device=DEV)
    with pytest.raises(RuntimeError, match="fn_sumsq_f32"):
        ops.sumsq(g[1:], torch.zeros(1, device=DEV))


@pytest.mark.parametrize("alpha", AXPY_ALPHA)
@pytest.mark.parametrize("n", AXPY_N)
def test_axpy_vs_fp64(ops, n, alpha):
    w, at = run_axpy(ops, n, alpha, DEV)
    print()
    print("[reduce] %-13s %-46s        ratio %8.5f  at %d" % ("axpy", "n%d-alpha%g" % (n, alpha), w, at))


@pytest.mark.parametrize("R,Cc", TRANSPOSE_SHAPES)
def test_transpose_bit_exact(ops, R, Cc):
    run_transpose(ops, R, Cc, DEV)
    print()
    print("[reduce] %-13s %-46s        bit-exact" % ("transpose", "%dx%d-src_ld%d-dst_ld%d" % (R, Cc, Cc + 3, R + 5)))


# ---- optimiser ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("supervised", (0, 1))
@pytest.mark.parametrize("advance", (0, 1))
def test_step_params_vs_python_floats(ops, advance, supervised):
    """every corner of the annealing (999 / 1000, 9999 / 10000, 20000 / 20001), of the Fader weight (1999 / 2000) and a step past 2**31, at Adam
    t counters 0, 1, 1000 and 10**6: all eight outputs within 2**-23 relative of the formulas in Python floats, exact zeros, counters advanced only
    with advance = 1.  On steps 1000..9999 beta0 is negative: that is the reference trainer's formula (helpers_reduce.step_params_reference)."""
    worst = (0.0, 0, 0)
    for step in SP_STEPS:
        for t in SP_T:
            w = run_step_params(ops, step, t, advance, supervised, DEV)
            if w >= worst[0]:
                worst = (w, step, t)
    print()
    print("[reduce] %-13s %-46s        ratio %8.5f  at step %d t %d  (x 2**-23 relative, %d launches)" % (
        "step_params", "advance%d-supervised%d" % (advance, supervised), worst[0], worst[1], worst[2], len(SP_STEPS) * len(SP_T)))


@pytest.mark.parametrize("case", ADAM_CASES, ids=[c["id"] for c in ADAM_CASES])
def test_clip_adam_three_steps_vs_fp64(ops, case):
    """sumsq -> step_params -> clip_adam chained on the device for three steps against clip_grad_norm_ + Adam in float64: p, m and v after every
    step, in every block of 1024 elements (helpers_reduce.check_adam)"""
    got = run_adam(ops, case, DEV)
    worst = check_adam(case, got)
    print()
    print(adam_line(case, worst))
