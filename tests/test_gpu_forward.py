"""The forward-only paths on the HIP kernels against the float64 oracle, per step and 16 x 32 block of every output and named engine buffer
(helpers_forward.check_forward_outputs; bound, references and the factor FORWARD_F: tests/helpers_forward.py, derived on the CPU in
test_forward_reference.py).  save=False hands gates = None to every scan launch, which keeps it off the ping-pong and bf16 x 6 kernels the training
step runs: every forward-only case asserts from the library's own launch plans which kernels it took.  The saved forward (save=True, the kernels
of the training step) is checked the same way at four cases.  Each test prints its line of profiles/forward_fp64_errors.txt."""
import pytest
import torch

from helpers_forward import (FORWARD_ONLY, PATH_NAMES, check_forward_only_kernels, check_forward_outputs, forward_line, forward_runs, recorded_launches,
                             run_forward_path)
from helpers_step import GMVAE_WANT, StepRecorder, check_step_kernels, gmvae_case
from mfn_import import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RUNS = forward_runs()


def _recorder():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    return StepRecorder(HipOps(torch.device(DEV)))


@pytest.mark.parametrize("path,cid,arith", RUNS, ids=["%s-%s-%s" % r for r in RUNS])
def test_forward_outputs_per_block_vs_float64(path, cid, arith):
    case, rec = gmvae_case(cid), _recorder()
    got, ref, eng = run_forward_path(path, case, ops=rec, device=DEV, arith=arith)
    torch.cuda.synchronize()
    assert eng.ops is rec and not rec.gru_sync_error()
    if path in FORWARD_ONLY:
        kernels = check_forward_only_kernels(recorded_launches(rec), case)
    else:
        kernels = check_step_kernels(rec, GMVAE_WANT.get((cid, arith), "f32"), persist=case["persist"])
    st = check_forward_outputs(got, ref, names=PATH_NAMES[path])
    print()
    print(forward_line(path, cid, arith, kernels, st))


def test_second_forward_only_call_of_case_g_is_bit_identical():
    """two Engine.forward(save=False, head=True) calls in a row at case g in f32: the second finds the buffers, the hand-over slots and the exchange
    slabs warm, and no bit of any output or named buffer may differ"""
    case, rec = gmvae_case("g"), _recorder()
    (first, second), ref, eng = run_forward_path("engine", case, ops=rec, device=DEV, arith="f32", calls=2)
    torch.cuda.synchronize()
    assert not rec.gru_sync_error() and len(rec.launches) % 2 == 0
    half = len(rec.launches) // 2
    assert rec.launches[:half] == rec.launches[half:]
    check_forward_only_kernels(recorded_launches(rec), case)
    for k, v in first.items():
        assert torch.equal(v, second[k]) and v.numpy().tobytes() == second[k].numpy().tobytes(), k
    check_forward_outputs(second, ref, names=PATH_NAMES["engine"])
