"""The measured cost of whole-piece transfer (profiles/stitch.txt).  A: fn_notes_stitch alone at S = 256 windows, V = 8 pieces, 100 note
slots per decoded row - device events around 1000 back-to-back calls (three launches each) through the kernel table, 7 windows.  B: transfer_piece end to
end on a synthetic piece of 256 windows, V = 8, hidden 512 / Z 128 seeded weights, split by stage with device events around each stage."""
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch
import helpers_stitch as hs
from mfn_import import load_package
pkg = load_package()
from music_fader_nets_amd.hipops import HipOps

DEV = "cuda:0"
ops = HipOps(DEV)
S, V, LD = 256, 8, 100
g = np.random.RandomState(1)
# A: every window 200 ticks, 12 source notes; decoded rows of 10..40 notes; a third of the windows pass the source through, the others clip / fit
t0 = np.sort(g.randint(0, 200, (S, 12)), axis=1) + 200 * np.arange(S)[:, None]
src_np = np.stack([t0, t0 + g.randint(5, 120, (S, 12)), g.randint(20, 70, (S, 12)), g.randint(40, 110, (S, 12))], 2).astype(np.int32).reshape(-1, 4)
spans_np = np.stack([np.arange(S) * 12, np.full(S, 12), np.arange(S) * 200, np.arange(S) * 200 + 200], 1).astype(np.int32)
d0 = np.sort(g.randint(0, 260, (S * V, LD)), axis=1)
dec_np = np.stack([d0, d0 + g.randint(1, 90, (S * V, LD)), g.randint(20, 70, (S * V, LD)), g.randint(40, 110, (S * V, LD))], 2).astype(np.int32)
dec_n_np, dec_end_np = g.randint(10, 41, S * V).astype(np.int32), g.randint(150, 300, S * V).astype(np.int32)
mode_np = g.randint(0, 3, S * V).astype(np.int32)
case = dict(S=S, V=V, dec=dec_np, dec_ld=LD, dec_n=dec_n_np, dec_end=dec_end_np, src=src_np, spans=spans_np, mode=mode_np, out_ld=len(src_np) + S * LD)
dev = {k: torch.from_numpy(case[k]).to(DEV) for k in ("dec", "dec_n", "dec_end", "src", "spans", "mode")}
i32 = dict(dtype=torch.int32, device=DEV)
out, wf = torch.empty(V, case["out_ld"], 4, **i32), torch.empty(V, S + 1, **i32)
out_n, status = torch.empty(V, **i32), torch.empty(V, **i32)
call = lambda: ops.notes_stitch(dev["dec"], LD, dev["dec_n"], dev["dec_end"], dev["src"], dev["spans"], dev["mode"], out, wf, out_n, status)


def window(f, launches):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(launches):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000.0 / launches


for _ in range(50):
    call()
torch.cuda.synchronize()
v = np.array([window(call, 1000) for _ in range(7)])
ref = hs.stitch_ref(case)
same = all(np.array_equal(x.cpu().numpy(), ref[k]) for k, x in (("notes", out), ("n_notes", out_n), ("win_first", wf), ("status", status)))
lines = ["device %s; us per call, device events around 1000 back-to-back calls, 7 windows" % torch.cuda.get_device_name(0),
         "fn_notes_stitch  S %d V %d, %d slots per row, out_ld %d (zeroed tail included)   median %7.2f  min %7.2f  max %7.2f" % (
             S, V, LD, case["out_ld"], np.median(v), v.min(), v.max()),
         "notes per piece %s; equal to the restatement of tests/helpers_stitch.py: %s" % (out_n.tolist(), same)]

# B: transfer_piece by stage.  The stages are timed by wrapping what transfer.py calls; the sum of the stages against the whole call shows what is left
# to torch glue (cat, where, the latent arithmetic).
from music_fader_nets_amd import decode, transfer
torch.manual_seed(3)
m = pkg.MusicAttrRegGMVAE(342, 3, 16, 24, 512, 128, 32, n_component=2).to(DEV)
n_per = 16
p0 = np.sort(g.randint(0, 200, (S, n_per)) // 10 * 10, axis=1)
p0[:, 0] = 0
p0 = p0 + 200 * np.arange(S)[:, None]
notes = np.stack([p0, p0 + g.randint(5, 60, (S, n_per)), g.randint(20, 70, (S, n_per)), g.randint(40, 110, (S, n_per))], 2).astype(np.int32).reshape(-1, 4)
midi = pkg.MidiNotes(torch.from_numpy(notes), torch.arange(0, 200 * S + 1, 50, dtype=torch.int32), 0)
stages = {}


def timed(mod, name, key):
    fn = getattr(mod, name)

    def wrapper(*a, **k):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        r = fn(*a, **k)
        e.record()
        stages.setdefault(key, []).append((s, e))
        return r

    setattr(mod, name, wrapper)


timed(transfer, "midi_segments", "midi_segments"), timed(decode, "greedy_decode", "decode %d rows x 100 steps" % (S * V))
timed(transfer, "tokens_to_notes", "tokens_to_notes"), timed(transfer, "stitch_notes", "stitch_notes"), timed(transfer, "fader_latents", "latents")
enc = m.encode
timed(m, "encode", "encode %d rows" % S)
eps = (torch.randn(S, 128), torch.randn(S, 128))
lm = [0.25 * (k + 1) for k in range(V)]
for _ in range(2):
    res = pkg.transfer_piece(m, midi, lmbda=lm, eps=eps)
torch.cuda.synchronize()
stages.clear()
whole = []
for _ in range(5):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    res = pkg.transfer_piece(m, midi, lmbda=lm, eps=eps)
    e.record()
    whole.append((s, e))
torch.cuda.synchronize()
ms = lambda pairs: float(np.median([s.elapsed_time(e) for s, e in pairs]))
lines.append("transfer_piece  %d windows x %d amounts, hidden 512 / Z 128 seeded weights, greedy, 100 steps; ms, median of 5 calls, device events" % (S, V))
lines.append("   whole call %9.3f" % ms(whole))
for k, pairs in stages.items():
    lines.append("   %-32s %9.3f" % (k, ms(pairs)))
lines.append("   windows transferred %d of %d; notes per piece %s" % (int(res.used.sum()), S * V, res.n_notes.tolist()))
print("\n".join(lines))
