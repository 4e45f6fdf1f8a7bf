"""One measured cost of the reconstruction report (profiles/report.txt) at the headline shape H 512, B 256, T 256, Tr 64:
reconstruction_report per batch against the only way the parent commit offers the same numbers - the drop-in model(...) to (B, T, 342) log-probs,
torch.argmax, a copy to the host and the reference's acc() loop.  The two are alternated; device events around each call plus one synchronise, and the
wall clock beside them (both calls end on the host).  `--kernels N`: only N back-to-back launches of fn_token_score and fn_match_rows on the report's
shapes, for a kernel trace of their own."""
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch
from mfn_import import load_package
pkg = load_package()
from music_fader_nets_amd.synth import synth_batch

DEV = "cuda:0"
H, Z, B, T, Tr = 512, 128, 256, 256, 64


def acc_loop(a, b, trim):
    """the loop of the reference's acc() on host arrays (trainer_gmm.py:549-565)"""
    tot = 0.0
    for i in range(len(a)):
        bb = np.trim_zeros(b[i]) if trim else b[i]
        aa = a[i][:len(bb)]
        tot += sum(1 for j in range(len(aa)) if aa[j] == bb[j]) / len(aa)
    return tot


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
        from music_fader_nets_amd.hipops import HipOps
        ops = HipOps(DEV)
        g = torch.Generator().manual_seed(0)
        logits = (3 * torch.randn(T * B, 352, generator=g)).to(DEV)
        d = torch.randint(0, 342, (B, T), generator=g).to(torch.int32).to(DEV)
        for _ in range(int(sys.argv[2])):
            sc = pkg.token_scores(logits[:, :342], d, layout="time_major", B=B, ops=ops)
            pkg.match_rows(sc.pred, d, trim=True, nll=sc.nll, rank=sc.rank, ops=ops)
        torch.cuda.synchronize()
        print("launched fn_token_score and fn_match_rows %s times on (B %d, T %d, V 342, ld 352)" % (sys.argv[2], B, T))
        return
    torch.manual_seed(1234)
    model = pkg.MusicAttrRegGMVAE(342, 3, 16, 24, H, Z, 32, n_component=2).to(DEV)
    tr = pkg.GMVAETrainer(model, lr=1e-3, beta=0.2)
    b = synth_batch(np.random.RandomState(0), B, T, Tr)
    batch = (b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
    eps = tuple(torch.randn(B, Z).to(DEV) for _ in range(2))
    dev = [torch.from_numpy(b[k]).to(DEV) for k in ("d", "r", "n")] + [torch.from_numpy(b["c"]).to(DEV)]

    def ours():
        return pkg.reconstruction_report(tr, batch, step=20000, eps=eps)

    def parent():
        with torch.no_grad():
            (out, r_out, n_out, _, _), *_ = model(*dev, eps=eps)
        a = [torch.argmax(t, dim=-1).cpu().numpy() for t in (out, r_out, n_out)]
        return acc_loop(a[0], b["d"], True), acc_loop(a[1], b["r"], False), acc_loop(a[2], b["n"], False)

    def timed(f):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        s.record()
        res = f()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e), (time.perf_counter() - t0) * 1e3, res

    for _ in range(3):
        ours(), parent()
    rows = {"ours": [], "parent": []}
    for _ in range(9):
        rows["ours"].append(timed(ours)[:2]), rows["parent"].append(timed(parent)[:2])
    rep, par = ours(), parent()
    print("device %s; H %d, B %d, T %d, Tr %d; ms per batch, 9 alternated calls each, device events around the call / wall clock" % (
        torch.cuda.get_device_name(0), H, B, T, Tr))
    for k, name in (("ours", "reconstruction_report (one forward, the accuracies on the device, one copy)"),
                    ("parent", "model(...) -> (B, T, 342) log-probs, torch.argmax, copy, acc() loop on the host ")):
        v = np.array(rows[k])
        print("%s  events median %8.2f min %8.2f max %8.2f | wall median %8.2f" % (name, np.median(v[:, 0]), v[:, 0].min(), v[:, 0].max(), np.median(v[:, 1])))
    print("acc_x %.6f vs the host loop %.6f; acc_r %.6f vs %.6f; acc_n %.6f vs %.6f" % (rep["acc_x"], par[0], rep["acc_r"], par[1], rep["acc_n"], par[2]))


main()
