"""Cost of the controllability metrics behind a fader sweep (profiles/attributes.txt): H 512, 256 samples x 8 values = 2048 rows x 100 steps.
  1. fader_sweep alone (the parent commit's launches)        2. fader_sweep + event_attributes + sweep_scores (scalars to the host)
  3. the same tokens copied to the host and pushed through the numpy / Python restatement of tests/helpers_attributes.py
1 and 2 alternate round by round, host clock around work that ends in a device synchronise.  The decode is sampled (temperature 1, fixed seed): an
untrained model's greedy rows sound no notes, and the raster should have work.  `--trace`: a few launches only, for rocprofv3 --kernel-trace --stats."""
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch
from mfn_import import load_package

pkg = load_package()
dev = torch.device("cuda:0")
torch.manual_seed(0)
m = pkg.MusicAttrRegGMVAE(roll_dims=342, rhythm_dims=3, note_dims=16, chroma_dims=24, hidden_dims=512, z_dims=128, n_step=256, n_component=2).to(dev)
m.eval()
n, nv, steps, T = 256, 8, 100, 64
rs = np.random.RandomState(0)
x = torch.from_numpy(rs.randint(0, 342, (n, T))).to(dev)
c = torch.from_numpy(rs.rand(n, 24).astype(np.float32)).to(dev)
g = torch.Generator().manual_seed(1)
eps = (torch.randn(n, nv, 128, generator=g).to(dev), torch.randn(n, nv, 128, generator=g).to(dev))
values = np.array([-2.0 + k * 0.5 for k in range(nv)])
sample = dict(temperature=1.0, seed=1)


def sweep():
    return pkg.fader_sweep(m, x, c, values.astype(np.float32), steps=steps, which="r", eps=eps, sample=sample)[0]


def measured():
    tok = sweep()
    at = pkg.event_attributes(tok)
    return tok, at, pkg.sweep_scores(at.r_density, at.n_density, at.status, values, "r", 0.19, 1.4)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


if "--trace" in sys.argv:
    for _ in range(3):
        measured()
    torch.cuda.synchronize()
    sys.exit(0)

for _ in range(3):
    sweep(), measured()
rounds, t1, t2 = 12, [], []
for _ in range(rounds):
    t1.append(clock(sweep)[0])
    ms, (tok, at, sc) = clock(measured)
    t2.append(ms)
line = lambda name, t: print("   %-58s median %8.3f  min %8.3f  max %8.3f" % (name, statistics.median(t), min(t), max(t)), flush=True)
print("device %s, H 512, %d samples x %d values x %d steps, sampled decode; ms per call, call + synchronise, %d rounds, alternated" % (
    torch.cuda.get_device_name(0), n, nv, steps, rounds))
line("1. fader_sweep", t1)
line("2. fader_sweep + event_attributes + sweep_scores", t2)
a, b = statistics.median(t1), statistics.median(t2)
print("   -> +%.3f ms (%+.2f %%)" % (b - a, 100 * (b - a) / a))

# the two kernels alone, device events over 50 launches each
tok = tok.reshape(-1, steps).contiguous()
ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
ev[0].record()
for _ in range(50):
    at = pkg.event_attributes(tok)
ev[1].record()
st = at.status.view(n, nv)
rd, nd = at.r_density.view(n, nv), at.n_density.view(n, nv)
from music_fader_nets_amd.attributes import _sweep_scores_device
ev[2].record()
for _ in range(50):
    _sweep_scores_device(rd, nd, st, values, "r", 0.19, 1.4)
ev[3].record()
torch.cuda.synchronize()
print("   event_attributes (allocation + parameter upload + launch), device events / 50: %.1f us;  sweep_scores: %.1f us" % (
    ev[0].elapsed_time(ev[1]) * 20, ev[2].elapsed_time(ev[3]) * 20))
print("   rows with notes %d of %d, median n_cells %d, scores %s" % (int((at.status == 0).sum()), tok.shape[0], int(at.n_cells.median()), sc))

import helpers_attributes as ha
t0 = time.perf_counter()
host = tok.cpu().numpy()
t_copy = time.perf_counter() - t0
ref = ha.event_attributes_ref(host, steps, ha.DEFAULT, ha.cells_ld_for(steps, ha.DEFAULT))
sc_ref = ha.sweep_scores_ref(ref["r_density"].reshape(n, nv), ref["n_density"].reshape(n, nv), ref["status"].reshape(n, nv), values, 0, 0.19, 1.4)
t_host = time.perf_counter() - t0
print("   3. tokens to the host (%.3f ms) + the Python restatement: %.1f ms once" % (t_copy * 1e3, t_host * 1e3))
same = all(np.array_equal(at._asdict()[k].cpu().numpy().view(np.int32), ref[k].view(np.int32)) for k in ("r_density", "n_density", "status", "n_cells"))
print("   device results equal the restatement's bit for bit: %s; scores differ by at most %.1e" % (
    same, max(abs(sc[k] - sc_ref[k]) for k in ha.SCORE_KEYS)))
