"""The loss-head kernels of csrc/loss.hip against float64 on an MI355X: fn_vocab_logsoftmax, fn_vocab_logsoftmax_bwd, fn_vocab_argmax,
fn_time_logsoftmax (the wave kernel and the loop kernel), fn_time_logsoftmax_bwd, fn_masked_prob, fn_pairwise_reg, fn_adv_head, fn_onehot_to_index.

The case tables, the float64 references, the float32 restatement of the documented steps, the per-tile bound and the checkers are
tests/helpers_loss.py; tests/test_loss_reference.py shows on the CPU that the tables have the properties their ids claim, that the checkers accept
the restatement and FakeOps, and that they reject planted faults.  Each launch is checked for layout, for its exact parts, then for the tile bound;
every test prints its lines of profiles/loss_fp64_errors.txt."""
import ctypes as C
import types

import pytest
import torch

from helpers_loss import (ABI_REFUSALS, ADV_CASES, ARGMAX_CASES, EXACT_PASS, LOSS_F, MASKED_CASES, MASKED_FORMS, ONEHOT_CASES, PAIR_CASES, SENTINEL,
                          TIME_BWD_CASES, TIME_CASES, VOCAB_BWD_CASES, VOCAB_CASES, bits_equal, check_adv, check_argmax, check_masked, check_onehot, check_pair,
                          check_time, check_time_bwd, check_vocab, check_vocab_bwd, exact_line, line, run_adv, run_argmax, run_masked, run_onehot, run_pair,
                          run_time, run_time_bwd, run_vocab, run_vocab_bwd, time_identity_inputs, time_identity_views, time_kernel)
from mfn_import import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    return HipOps(torch.device(DEV))


def _ids(cases):
    return [c["id"] for c in cases]


def _same(cid, a, b, what):
    for k in a:
        if torch.is_tensor(a[k]):
            assert bits_equal(a[k], b[k]), "%s: %s of %s differs" % (cid, k, what)


@pytest.mark.parametrize("case", VOCAB_CASES, ids=_ids(VOCAB_CASES))
def test_vocab_logsoftmax_vs_fp64(ops, case):
    """rows % 4 in {0, 1, 2, 3} with B != T, vocabulary widths around the 64 lanes (empty lanes, a lane tail, 16 entries per lane), ld > E, every
    form of the launch, logits at +-90, a -inf logit per row and a tile of low-probability columns: logp_bt at [b][t], nll_rows and dlogits at
    row t B + b in every 16 x 16 tile; padding columns and rows past the last untouched; a second launch gives the same bits, and dlogits written
    over the logits the bits of the out-of-place launch"""
    bufs = run_vocab(ops, case, DEV)
    worst = check_vocab(case, bufs)
    _same(case["id"], bufs, run_vocab(ops, case, DEV), "a second launch")
    if case["form"] == "alias":
        out = run_vocab(ops, case, DEV, form="all")
        for k in ("logp", "nll", "dlogits"):
            assert bits_equal(bufs[k], out[k]), "%s: %s in place differs from the out-of-place launch" % (case["id"], k)
    print()
    print(line("vocab_logsoftmax", case["id"], worst))


@pytest.mark.parametrize("case", VOCAB_BWD_CASES, ids=_ids(VOCAB_BWD_CASES))
def test_vocab_logsoftmax_bwd_vs_fp64(ops, case):
    bufs = run_vocab_bwd(ops, case, DEV)
    worst = check_vocab_bwd(case, bufs)
    _same(case["id"], bufs, run_vocab_bwd(ops, case, DEV), "a second launch")
    print()
    print(line("vocab_logsoftmax_bwd", case["id"], worst))


@pytest.mark.parametrize("case", ARGMAX_CASES, ids=_ids(ARGMAX_CASES))
def test_vocab_argmax_vs_fp64(ops, case):
    """tokens equal the first-index argmax of the float32 logits exactly - exact ties in one lane, across lanes, at 0 and E - 1, +0.0 against -0.0,
    a constant row, rows with -inf entries - through strided logp_out / tok_out views, with logp_out given and NULL"""
    bufs = run_argmax(ops, case, DEV)
    worst = check_argmax(case, bufs)
    _same(case["id"], bufs, run_argmax(ops, case, DEV), "a second launch")
    print()
    print(line("vocab_argmax", case["id"], worst) if case["logp"] else exact_line("vocab_argmax", case["id"], "tokens exact"))


@pytest.mark.parametrize("case", TIME_CASES, ids=_ids(TIME_CASES))
def test_time_logsoftmax_vs_fp64(ops, case):
    """Tr in {1, 2, 63, 64} on the wave kernel and {65, 70} on the loop kernel, B Cc = 258 columns (258 % 4 = 2), eval and train form; columns without
    a hit have nll_bc and dlogits exactly 0"""
    bufs = run_time(ops, case, DEV)
    worst = check_time(case, bufs)
    _same(case["id"], bufs, run_time(ops, case, DEV), "a second launch")
    print()
    print(line("time_logsoftmax", "%s %s" % (case["id"], time_kernel(case["Tr"]).replace("time_logsoftmax_", "")), worst))


def test_time_logsoftmax_wave_and_loop_kernels_are_bit_identical(ops):
    """the comment of time_logsoftmax_wave_kernel claims the loop kernel's bits: Tr = 65 with a last step of -1e4 (expf gives exactly 0) against
    Tr = 64 on the first 64 steps"""
    case, x65 = time_identity_inputs()
    b64, b65 = run_time(ops, case, DEV), run_time(ops, case, DEV, x=x65)
    a, b = time_identity_views(case, b64, b65)
    diff = int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum())
    print()
    print(exact_line("time_logsoftmax", "Tr64 (wave) vs Tr65 with a last step of -1e4 (loop)", "bit-identical" if diff == 0 else "%d of %d logp differ" % (diff, a.numel())))
    assert diff == 0, "the wave kernel and the loop kernel differ in %d of %d log-probabilities, first at %s" % (
        diff, a.numel(), tuple(int(v) for v in torch.nonzero(a != b)[0]))


@pytest.mark.parametrize("case", TIME_BWD_CASES, ids=_ids(TIME_BWD_CASES))
def test_time_logsoftmax_bwd_vs_fp64(ops, case):
    bufs = run_time_bwd(ops, case, DEV)
    worst = check_time_bwd(case, bufs)
    _same(case["id"], bufs, run_time_bwd(ops, case, DEV), "a second launch")
    print()
    print(line("time_logsoftmax_bwd", case["id"], worst))


@pytest.mark.parametrize("case", MASKED_CASES, ids=_ids(MASKED_CASES))
def test_masked_prob_vs_fp64(ops, case):
    """sums only, gradient only, both, and the gradient written over the logits (the bits of the out-of-place launch); the sum of an empty range is
    exactly 0"""
    outs = {f: run_masked(ops, case, f, DEV) for f in MASKED_FORMS}
    worst = max((check_masked(case, outs[f]) for f in MASKED_FORMS), key=lambda w: w[0])
    for k in ("sums", "dlogits"):
        assert bits_equal(outs["inplace"][k], outs["both"][k]), "%s: %s in place differs from the out-of-place launch" % (case["id"], k)
    assert bits_equal(outs["sums"]["sums"], outs["both"]["sums"]) and bits_equal(outs["grad"]["dlogits"], outs["both"]["dlogits"]), "%s: the forms differ" % case["id"]
    print()
    print(line("masked_prob", case["id"], worst))


@pytest.mark.parametrize("case", PAIR_CASES, ids=_ids(PAIR_CASES))
def test_pairwise_reg_vs_fp64(ops, case):
    """the exact pass (z0 from {-64, .., 64}: every term an integer) bit for bit, the randn pass within the tile bound; attributes in float64 with
    exact ties and, in one case, differences of 2**-40 that float32 cannot see"""
    bufs = run_pair(ops, case, DEV)
    worst = check_pair(case, bufs)
    b2 = run_pair(ops, case, DEV)
    assert bits_equal(bufs["loss_rows"], b2["loss_rows"]) and (bufs["dz0"] is None or bits_equal(bufs["dz0"], b2["dz0"])), "%s: two launches differ" % case["id"]
    print()
    print(exact_line("pairwise_reg", case["id"]) if case["kind"] == EXACT_PASS else line("pairwise_reg", case["id"], worst))


@pytest.mark.parametrize("case", ADV_CASES, ids=_ids(ADV_CASES))
def test_adv_head_vs_fp64(ops, case):
    """Z around the 64 lanes, B % 4 != 0, masked rows, a row with pre == 0 exactly (o = 0, da = 0), lam_dev = NULL (da exactly 0, g_z unchanged bit
    for bit), da = NULL, g_z = NULL; columns >= Z of g_z untouched"""
    bufs = run_adv(ops, case, DEV)
    worst = check_adv(case, bufs)
    print()
    print(line("adv_head", case["id"], worst))


@pytest.mark.parametrize("case", ONEHOT_CASES, ids=_ids(ONEHOT_CASES))
def test_onehot_to_index_exact(ops, case):
    check_onehot(case, run_onehot(ops, case, DEV))
    print()
    print(exact_line("onehot_to_index", case["id"], "indices exact"))


def test_abi_refusals_return_their_code_and_write_nothing(ops):
    """the shape and NULL refusals of the nine entry points: the error code, and not one element of the buffers they were handed is written"""
    f = torch.full((4096,), SENTINEL, device=DEV)
    i = torch.full((4096,), -7, dtype=torch.int32, device=DEV)
    d = torch.full((4096,), SENTINEL, dtype=torch.float64, device=DEV)
    p = types.SimpleNamespace(f=C.c_void_p(f.data_ptr()), i=C.c_void_p(i.data_ptr()), d=C.c_void_p(d.data_ptr()))
    for name, fn, args, code in ABI_REFUSALS:
        got = getattr(ops.lib, fn)(*args(p))
        assert got == code, "%s: %s returned %d, expected %d" % (name, fn, got, code)
    torch.cuda.synchronize()
    assert bool((f == SENTINEL).all()) and bool((i == -7).all()) and bool((d == SENTINEL).all()), "a refused call wrote to a buffer"
    assert all(0 < F <= 16 for F in LOSS_F.values())
    print()
    print(exact_line("C ABI", "%d refusals" % len(ABI_REFUSALS), "error code returned, nothing written"))
