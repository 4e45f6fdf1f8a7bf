"""The assembled training step on the HIP kernels against the float64 oracle, per 16 x 32 block of every gradient (helpers_step.check_step_grads;
bound, references and the factor STEP_F: tests/helpers_step.py, derived on the CPU in test_step_reference.py).  The cases are the smallest shapes at
which each orchestration path of Engine exists; every case asserts from the library's own launch plans which scan kernels its decoder launches took,
so a case that silently ran another path fails instead of passing on it.  Each test prints its line of profiles/step_fp64_errors.txt."""
import pytest
import torch

from helpers_step import (GMVAE_CASES, GMVAE_WANT, SIBLING_CASES, StepRecorder, check_loss_terms, check_step_grads, check_step_kernels, cpu_state,
                          flat_grads, gmvae_case, gmvae_references, gmvae_trainer, run_sibling_case, step_line)
from mfn_import import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _recorder():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    return StepRecorder(HipOps(torch.device(DEV)))


def _step(case, step, arith, **switches):
    """one loss_and_grads of a case on the kernels -> (gradients, loss tuple, references, recorder)"""
    rec = _recorder()
    tr, eng, b, batch, eps = gmvae_trainer(case, ops=rec, device=DEV, arith=arith, **switches)
    assert eng.ops is rec
    sd = cpu_state(tr.model)
    tup = tr.loss_and_grads(step, batch, eps)
    torch.cuda.synchronize()
    assert not rec.gru_sync_error()
    ref = gmvae_references(case, step, sd, b, tuple(e.cpu() for e in eps), leak=case["leak"])
    return flat_grads(tr), tup, ref, rec


GPU_CASES = [(c["id"], a, s) for c in GMVAE_CASES for a in c["ariths"] for s in c["steps"]]


@pytest.mark.parametrize("cid,arith,step", GPU_CASES, ids=["%s-%s-%d" % c for c in GPU_CASES])
def test_step_gradients_per_block_vs_float64(cid, arith, step):
    case = gmvae_case(cid)
    got, tup, ref, rec = _step(case, step, arith)
    kernels = check_step_kernels(rec, GMVAE_WANT.get((cid, arith), "f32"), persist=case["persist"])
    st = check_step_grads(got, ref)
    check_loss_terms(tup, ref)
    print()
    print(step_line("gmvae-%s step %d" % (cid, step), arith, kernels, st))


@pytest.mark.parametrize("arith", ["f32", "bf16x6"])
def test_dw_order_changes_no_bit_of_case_g(arith):
    """where the decoder-side weight-gradient GEMMs are issued (side + aux lanes, side lane, behind the encoder block) changes no bit of the gradient
    at 256 rows; the per-block check runs on the "side" order"""
    case = gmvae_case("g")
    base = _step(case, 20000, arith)
    for order in ("side", "after"):
        got, tup, ref, rec = _step(case, 20000, arith, dw_order=order)
        assert tup == base[1], order
        for k, v in got.items():
            assert (v == base[0][k]).all() and v.tobytes() == base[0][k].tobytes(), (order, k)
        if order == "side":
            kernels = check_step_kernels(rec, GMVAE_WANT.get(("g", arith), "f32"))
            st = check_step_grads(got, ref)
            print()
            print(step_line("gmvae-g dw_order=side", arith, kernels, st))


def test_replayed_step_of_case_g_per_block_vs_float64():
    """what production runs: the captured step.  Three step_device calls on a fresh model (eager, capture + replay, replay) in the package's default
    arithmetic; the flat buffer then holds the unclipped gradient of the third step (fn_clip_adam reads it, never writes it), which is checked against
    the oracle on the weights that step started from."""
    case = gmvae_case("g")
    tr, eng, b, batch, eps = gmvae_trainer(case, device=DEV)
    assert tr.use_graph
    for i, step in enumerate((20000, 20001, 20002)):
        if i == 2:
            torch.cuda.synchronize()
            sd = cpu_state(tr.model)
        tr.step_device(step, batch, eps)
    torch.cuda.synchronize()
    assert not eng.ops.gru_sync_error()
    assert len(tr._graphs) == 1 and [s["runs"] for s in tr._static.values()] == [3]
    ref = gmvae_references(case, 20002, sd, b, tuple(e.cpu() for e in eps), key=("gmvae-g-replay",))
    st = check_step_grads(flat_grads(tr), ref)
    check_loss_terms(tr._tuple8(0.2, case["B"], False), ref)
    print()
    print(step_line("gmvae-g replayed step 3", "default", "captured graph", st))


SIB = [(c["id"], s) for c in SIBLING_CASES for s in c["steps"]]


@pytest.mark.parametrize("cid,step", SIB, ids=["%s-%d" % c for c in SIB])
def test_sibling_step_gradients_per_block_vs_float64(cid, step):
    case = next(c for c in SIBLING_CASES if c["id"] == cid)
    got, tup, ref, tr = run_sibling_case(case, step, device=DEV)
    torch.cuda.synchronize()
    assert not tr.model.engine().ops.gru_sync_error()
    st = check_step_grads(got, ref)
    check_loss_terms(tup, ref)
    print()
    print(step_line("sibling-%s step %d" % (cid, step), "default", "-", st))
