"""Latent disentanglement report on a real MI355X: the six kernels of csrc/disentangle.hip against the float64 restatement of
tests/helpers_disentangle.py on the case list (ranges, bin images, counts, hits and ranks bit-equal with canaries behind every output, the fp64 outputs
within the header's bounds), the mutated restatements each told apart, NaN / infinity / a bad level raising the right status bit, the planted structure
through pkg.disentanglement, and the report at hidden 64, Z 4, B 5, T 20, three batches."""
import numpy as np
import pytest
import torch

import helpers_disentangle as hd
from helpers import make_model
from mfn_import import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64          # entries behind every output buffer that must come back as they were


class DeviceBackend:
    """helpers_disentangle.run_pipeline's backend on HipOps: numpy in, numpy out, every output with GUARD untouched entries behind it"""

    def __init__(self):
        load_package()
        from music_fader_nets_amd.hipops import HipOps
        self.ops = HipOps(DEV)
        self.cache = {}

    def _dev(self, buf):
        key = id(buf)
        if key not in self.cache:
            self.cache[key] = (buf, torch.from_numpy(buf).to(DEV))
        return self.cache[key][1]

    @staticmethod
    def _guarded(n, fill, dtype):
        return torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)

    @staticmethod
    def _intact(t, n, fill):
        torch.cuda.synchronize()
        assert bool((t[n:] == fill).all()), "written past the end"
        return t[:n].cpu().numpy()

    def range(self, buf, off, P):
        lim, st = self._guarded(2 * P, float(hd.CANARY), torch.float32), self._guarded(P, -7, torch.int32)
        self.ops.column_range(self._dev(buf)[:, off:off + P], lim[:P], lim[P:2 * P], st[:P])
        v = self._intact(lim, 2 * P, float(hd.CANARY))
        return v[:P].copy(), v[P:].copy(), self._intact(st, P, -7)

    def bins(self, buf, off, P, lo, hi, bins, card, n_pad, status):
        img = self._guarded(P * n_pad, 0xEE, torch.uint8)
        st = self._guarded(P, -7, torch.int32)
        st[:P] = torch.from_numpy(np.ascontiguousarray(status)).to(DEV)
        lim = torch.from_numpy(np.stack([lo, hi])).to(DEV)
        self.ops.bin_columns(self._dev(buf)[:, off:off + P], lim[0], lim[1], bins, img[:P * n_pad].view(P, n_pad), st[:P], card=card)
        return self._intact(img, P * n_pad, 0xEE).reshape(P, n_pad), self._intact(st, P, -7)

    def hist(self, bz, bf, N):
        D, A = bz.shape[0], bf.shape[0]
        counts = self._guarded(D * A * 4096, -1, torch.int32)
        self.ops.joint_hist(torch.from_numpy(bz).to(DEV), torch.from_numpy(bf).to(DEV), N, counts[:D * A * 4096])
        return self._intact(counts, D * A * 4096, -1).reshape(D, A, 64, 64)

    def ranks(self, buf, off, P, n_pad):
        rk = self._guarded(P * n_pad, float(hd.CANARY), torch.float32)
        self.ops.column_ranks(self._dev(buf)[:, off:off + P], rk[:P * n_pad].view(P, n_pad))
        return self._intact(rk, P * n_pad, float(hd.CANARY)).reshape(P, n_pad)

    def corr(self, xf, x_rs, x_cs, P, yf, y_rs, y_cs, Q, N):
        X = torch.as_strided(torch.from_numpy(np.ascontiguousarray(xf)).to(DEV), (N, P), (x_rs, x_cs))
        Y = torch.as_strided(torch.from_numpy(np.ascontiguousarray(yf)).to(DEV), (N, Q), (y_rs, y_cs))
        n = 2 * P + 2 * Q + P * Q
        m = self._guarded(n, float(hd.CANARY), torch.float64)
        self.ops.column_corr(X, Y, m[:P], m[P:2 * P], m[2 * P:2 * P + Q], m[2 * P + Q:2 * P + 2 * Q], m[2 * P + 2 * Q:n])
        v = self._intact(m, n, float(hd.CANARY))
        return v[:P], v[P:2 * P], v[2 * P:2 * P + Q], v[2 * P + Q:2 * P + 2 * Q], v[2 * P + 2 * Q:].reshape(P, Q)

    def mi(self, counts):
        pairs = counts.shape[0]
        out, hits = self._guarded(3 * pairs, float(hd.CANARY), torch.float64), self._guarded(pairs, -1, torch.int32)
        self.ops.mi_scores(torch.from_numpy(np.ascontiguousarray(counts)).to(DEV), out[:3 * pairs], hits[:pairs])
        return self._intact(out, 3 * pairs, float(hd.CANARY)).reshape(pairs, 3), self._intact(hits, pairs, -1)


CASES = hd.cases()


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["tag"].replace(" ", "_") for c in CASES])
def test_kernels_against_the_restatement(k):
    c = CASES[k]
    share = hd.check_pipeline(c, hd.run_pipeline(c, DeviceBackend()))
    print("%s: share of the fp64 bounds %s" % (c["tag"], {n: round(v, 3) for n, v in share.items() if v}))


def test_every_mutated_restatement_is_told_apart():
    """an off-by-one bin edge, a dropped last row, a dropped last column, `<=` for `<` in the rank, a tie counted once: each differs from the device's
    output on at least one case of the list (the cases up to N 513 suffice)"""
    be, told = DeviceBackend(), set()
    for c in CASES[:9]:
        o = hd.run_pipeline(c, be)
        for name, (key, arr) in hd.mutants(c).items():
            if not np.array_equal(o[key] if key == "counts" else o[key][:, :c["N"]], arr):
                told.add(name)
    assert told == set(hd.mutants(CASES[0])), told


def test_status_bits_without_a_fault():
    """a NaN and an infinity set FN_DIS_NONFINITE of their column only and leave the range of the finite entries; what is no level sets FN_DIS_BAD_LEVEL;
    every kernel behind them runs on such columns and stays in bounds (the canaries)"""
    be = DeviceBackend()
    g = np.random.default_rng(9)
    x = g.standard_normal((300, 5)).astype(np.float32)
    x[17, 1], x[299, 3], x[0, 3] = np.nan, np.inf, -np.inf
    lo, hi, st = be.range(x, 0, 5)
    rl, rh, rs = hd.range_ref(x)
    assert st.tolist() == [0, 1, 0, 1, 0] == rs.tolist() and lo.tobytes() == rl.tobytes() and hi.tobytes() == rh.tobytes()
    img, st2 = be.bins(x, 0, 5, lo, hi, 20, None, 320, st)
    assert np.array_equal(img[:, :300], hd.bin_ref(x, rl, rh, 20)[0]) and st2.tolist() == st.tolist() and img[1, 17] == 0 and img[3, 299] == 19 and img[3, 0] == 0
    f = g.integers(0, 4, (300, 2)).astype(np.float32)
    f[5, 1], f[6, 0] = 4.0, np.nan
    flo, fhi, fst = be.range(f, 0, 2)
    fimg, fst2 = be.bins(f, 0, 2, flo, fhi, 20, [4, 4], 320, fst)
    want, bad = hd.bin_ref(f, flo, fhi, 20, [4, 4])
    assert fst.tolist() == [1, 0] and fst2.tolist() == [3, 2] and bad.tolist() == [2, 2] and np.array_equal(fimg[:, :300], want)
    counts = be.hist(img, fimg, 300)
    assert np.array_equal(counts, hd.hist_ref(img[:, :300], fimg[:, :300]))
    rk = be.ranks(x, 0, 5, 320)
    fine = [0, 2, 4]
    assert np.array_equal(rk[fine, :300], hd.ranks_ref(x[:, fine])) and rk[1, 17] == 0.5 and rk[3, 299] == 300.0 and rk[3, 0] == 1.0
    be.corr(x.reshape(-1), 5, 1, 5, f.reshape(-1), 2, 1, 2, 300)          # NaN results, in bounds
    pkg = load_package()
    with pytest.raises(ValueError, match="codes: column 1 "):
        pkg.disentanglement(torch.from_numpy(x).to(DEV), torch.from_numpy(f[:, 1:]).to(DEV))
    with pytest.raises(ValueError, match=r"factors: column 0 \(factor0\) holds a value that is not an integer in \[0, 4\)"):
        pkg.disentanglement(torch.from_numpy(x[:, [0, 2]]).to(DEV), torch.from_numpy(f[:, 1:]).to(DEV), card=[4])


def test_planted_structure_on_the_device():
    pkg = load_package()
    for seed in (0, 5):
        z, f, card = hd.planted(seed)
        wide = torch.from_numpy(np.concatenate([z, np.zeros((2048, 3), np.float32)], 1)).to(DEV)
        res = pkg.disentanglement(wide[:, :6], torch.from_numpy(f).to(DEV), card=card, bins=20)
        fig = hd.figures_ref(z, f, card, 20)
        zero = lambda m: np.where(np.isnan(m), 0.0, m)
        print(hd.check_planted(dict(mi=res.mi, h_factor=res.h_factor, r2=zero(res.r2), rho=zero(res.rho), accuracy=zero(res.accuracy)), "device seed %d" % seed))
        assert res.winner["mi"].tolist() == [1, 5] and res.winner["r2"].tolist() == [3, -1] and res.winner["rho"].tolist() == [1, -1]
        assert np.array_equal(res.accuracy[:, 1], fig["accuracy"][:, 1])
        assert np.allclose(res.mi, fig["mi"], rtol=0, atol=hd.K_I * hd.ULP * 8) and np.allclose(res.r2[:, 0], fig["r2"][:, 0], rtol=1e-12, atol=1e-15)
        assert np.allclose(res.rho[:, 0], fig["rho"][:, 0], rtol=1e-12, atol=1e-15)


def _loaders(rs, sizes=(5, 5, 5), T=20):
    from music_fader_nets_amd.synth import synth_batch
    out = []
    for B in sizes:
        b = synth_batch(rs, B, T, 8)
        out.append((b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"]))
    return out


def test_report_at_model_level():
    """the code tensor equals the concatenated model.encode means bit for bit, the result equals pkg.disentanglement on those tensors, and
    evaluation_phase(disentangle=False) prints what it prints without the argument"""
    pkg = load_package()
    m = make_model(64, 4, device=DEV)
    dl = _loaders(np.random.RandomState(5))
    rep = pkg.disentanglement_report(m, dl, bins=8)
    m.eval()
    with torch.no_grad():
        means = torch.cat([torch.cat([d.mean for d in m.encode(torch.as_tensor(x[0]).long().to(DEV))], 1) for x in dl])
    m.train()
    assert rep.codes.shape == (15, 8) and rep.codes.is_cuda and torch.equal(rep.codes, means)
    res = pkg.disentanglement(rep.codes, rep.factors, bins=8, names=["r_density", "n_density"])
    for a, b in zip(rep.result[:9], res[:9]):
        assert np.array_equal(a, b, equal_nan=True)
    assert all(np.array_equal(rep.result.winner[k], res.winner[k]) for k in ("mi", "r2", "rho")) and isinstance(rep.fader_ok, bool)
    fig = hd.figures_ref(rep.codes.cpu().numpy(), rep.factors.cpu().numpy(), [0, 0], 8)
    assert np.allclose(res.mi, fig["mi"], rtol=0, atol=hd.K_I * hd.ULP * 8) and np.array_equal(res.h_code.shape, (8,))

    def run(**kw):
        tr = pkg.GMVAETrainer(make_model(64, 4, device=DEV), lr=1e-3, beta=0.2)
        lines = []
        torch.manual_seed(4)
        pkg.evaluation_phase(tr, [dl], log=lines.append, step=20000, **kw)
        return lines

    base, off, on = run(), run(disentangle=False), run(disentangle=True)
    assert off == base and len(base) == 3 and on[:3] == base and len(on) == 4 and on[3].startswith("DIS: r_density ")
