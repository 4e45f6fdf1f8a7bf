"""One scheduled-sampling train step of the drop-in class on a real MI355X (model.eps = 0.5), at H = 64 and H = 512, on both arithmetics:
the assertions of tests/test_scheduled_sampling.py (helpers_forced.check_scheduled_sampling) - mask, fed stream, `out` through the replay
checker with teacher = fed, parameter gradients against autograd through the fp64 oracle run with teacher = fed."""
import numpy as np
import pytest

from helpers import make_model, replay_inputs
from helpers_forced import check_scheduled_sampling, forced_line
from mfn_import import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("arith", ["f32", "bf16x6"])
@pytest.mark.parametrize("weights,B,T", [("h64", 8, 48), ("h512", 16, 64)])
def test_scheduled_sampling_train_step(weights, B, T, arith):
    pkg = load_package()
    from music_fader_nets_amd.synth import synth_batch
    H, Z, sd = replay_inputs(weights)
    m = make_model(H, Z, sd, device=DEV, arith=arith)
    st = check_scheduled_sampling(pkg, m, synth_batch(np.random.RandomState(2), B, T, 8), DEV)
    assert not m.engine().ops.gru_sync_error()
    print("\n" + forced_line("scheduled sampling [%s]" % arith, "rand<0.5", H, st) + "  grads checked %d" % st["grads_checked"])
