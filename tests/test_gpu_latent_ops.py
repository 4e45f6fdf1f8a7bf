"""Generation from the mixture prior and morphing on a real MI355X: fn_latent_draw and fn_latent_mix against the float64 restatement of
tests/helpers_latent_ops.py within the bounds the CPU tests hold the host twins to (canaries around every output, components exact, rows bit-equal
whatever the launch), the statistics of the device's normals, the exact cases of the mix, and generate / morph / latent_classes end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers_latent_ops as hl
from helpers import make_model
from mfn_import import ROOT, load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64          # floats behind every output buffer that must come back as canaries
_NORMALS = {}


def _ops():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    return HipOps(DEV)


def _normals(Z, stream_id, seed, offset):
    """the restatement's normals for 257 rows, computed once per (Z, stream, seed, offset) and shared"""
    key = (Z, stream_id, seed, offset)
    if key not in _NORMALS:
        _NORMALS[key] = hl.draw_normals(257, Z, stream_id, seed, offset)
    return _NORMALS[key]


def _canaries(n, dtype=torch.float32):
    return torch.full((n + GUARD,), float(hl.CANARY) if dtype == torch.float32 else -9, dtype=dtype, device=DEV)


def _draw_on_device(ops, c, optional=True):
    rows, Z, z_ld = c["rows"], c["Z"], c["z_ld"]
    zbuf = _canaries(rows * z_ld)
    z2 = zbuf[:rows * z_ld].view(rows, z_ld)
    jobs, eps, comp_out = [], [], []
    for s, j in enumerate(c["jobs"]):
        eps.append(_canaries(rows * Z)), comp_out.append(_canaries(rows, torch.int32))
        jobs.append(dict(mu_lk=torch.from_numpy(j["mu_lk"]).to(DEV), lv_lk=torch.from_numpy(j["lv_lk"]).to(DEV),
                         comp=None if j["comp"] is None else torch.from_numpy(j["comp"]).to(DEV), z=z2[:, s * c["col_step"]:s * c["col_step"] + Z],
                         eps_out=eps[s][:rows * Z].view(rows, Z) if optional else None, comp_out=comp_out[s][:rows] if optional else None, stream_id=j["stream_id"]))
    ops.latent_draw(jobs, torch.from_numpy(hl.params_bytes(c["seed"], c["offset"], c["tau"])).to(DEV))
    torch.cuda.synchronize()
    assert bool((zbuf[rows * z_ld:] == float(hl.CANARY)).all()), c["tag"]
    for e, k in zip(eps, comp_out):
        assert bool((e[rows * Z:] == float(hl.CANARY)).all()) and bool((k[rows:] == -9).all()), c["tag"]
        assert optional or (bool((e == float(hl.CANARY)).all()) and bool((k == -9).all())), c["tag"]
    return zbuf[:rows * z_ld].cpu().numpy(), [e[:rows * Z].view(rows, Z).cpu().numpy() for e in eps], [k[:rows].cpu().numpy() for k in comp_out]


@pytest.mark.parametrize("Z", [1, 5, 64, 128, 130])
def test_latent_draw_kernel(Z):
    """rows in {1, 3, 65, 257} x K in {1, 2, 8} x {1, 2, 4} jobs at this Z: z_ld = Z for one job, 2Z+24 with the second job at column Z for two,
    4Z+3 for four; components drawn, given, given with holes; tau 1, 0.5, 0, NaN"""
    ops = _ops()
    worst = [0.0, 0.0]
    for c in hl.draw_cases((1, 3, 65, 257), (Z,), (1, 2, 8), (1, 2, 4), vary=False):
        z, eps, comp = _draw_on_device(ops, c)
        worst = [max(x, y) for x, y in zip(worst, hl.check_draw_case(c, z, eps, comp, _normals))]
    print("device draw Z %d: worst error / bound, eps %.3f z %.3f" % (Z, worst[0], worst[1]))


def test_latent_draw_seeds_offsets_and_optional_outputs():
    """the CPU case list (64-bit seeds and offsets) on the device, and a launch without eps_out / comp_out: the same z"""
    ops = _ops()
    cases = hl.draw_cases()
    for c in cases[::3]:
        z, eps, comp = _draw_on_device(ops, c)
        hl.check_draw_case(c, z, eps, comp)
    z, _, _ = _draw_on_device(ops, cases[4])
    assert np.array_equal(_draw_on_device(ops, cases[4], optional=False)[0], z)


def test_latent_draw_rows_do_not_depend_on_the_launch():
    """row b of a 257-row launch is row b of a 3-row launch, one job or two, bit for bit"""
    ops = _ops()
    g = np.random.RandomState(2)
    for Z in (5, 130):
        lk = [hl.lookups(g, 2, Z) for _ in range(2)]
        case = lambda rows, streams: dict(tag="invariance", rows=rows, Z=Z, z_ld=2 * Z + 24, col_step=Z, tau=0.8, seed=11, offset=5,
                                          jobs=[dict(mu_lk=lk[s][0], lv_lk=lk[s][1], comp=None, stream_id=s) for s in streams])
        big, small, one = (_draw_on_device(ops, case(r, st)) for r, st in ((257, (0, 1)), (3, (0, 1)), (257, (0,))))
        ld = 2 * Z + 24
        assert np.array_equal(big[0].reshape(257, ld)[:3, :2 * Z], small[0].reshape(3, ld)[:, :2 * Z])
        assert np.array_equal(big[0].reshape(257, ld)[:, :Z], one[0].reshape(257, ld)[:, :Z])
        for s in (0, 1):
            assert np.array_equal(big[1][s][:3], small[1][s]) and np.array_equal(big[2][s][:3], small[2][s])
        assert np.array_equal(big[1][0], one[1][0]) and np.array_equal(big[2][0], one[2][0])


def test_latent_draw_statistics_on_the_device():
    ops = _ops()
    for seed in (2024, 7):
        for K in (2, 3, 8):
            mu, lv = np.zeros((K, 128), np.float32), np.zeros((K, 128), np.float32)
            c = dict(tag="stats", rows=4096, Z=128, z_ld=256, col_step=128, tau=1.0, seed=seed, offset=0,
                     jobs=[dict(mu_lk=mu, lv_lk=lv, comp=None, stream_id=s) for s in (0, 1)])
            z, eps, comp = _draw_on_device(ops, c)
            figures, corr = hl.stats_ok(eps[0], eps[1])
            print("device seed %d: (mean, var, m4) %s corr %.2e; K %d counts %s %s" % (seed, figures, corr, K, hl.counts_ok(comp[0], K).tolist(),
                                                                                      hl.counts_ok(comp[1], K).tolist()))
            assert np.array_equal(z.reshape(4096, 256)[:, :128], eps[0]) and np.array_equal(z.reshape(4096, 256)[:, 128:], eps[1])      # mu 0, sigma 1, tau 1
            for s in (0, 1):
                assert np.array_equal(comp[s], hl.draw_components(4096, K, s, seed))


def _mix_on_device(ops):
    def run(a, b, t, segs, per_pair=False, ab_ld=None, out_ld=None):
        pairs, D = a.shape
        ab_ld, out_ld = ab_ld or D, out_ld or D
        tt = torch.from_numpy(np.ascontiguousarray(t, np.float32)).to(DEV)
        P = tt.shape[-1]
        wa, wb = (torch.from_numpy(hl.widen(x, ab_ld)).to(DEV) for x in (a, b))
        n_out = (pairs * P - 1) * out_ld + D
        obuf, om = _canaries(n_out), _canaries(pairs * len(segs))
        ops.latent_mix(torch.as_strided(wa, (pairs, D), (ab_ld, 1)), torch.as_strided(wb, (pairs, D), (ab_ld, 1)), tt, segs,
                       torch.as_strided(obuf, (pairs * P, D), (out_ld, 1)), omega_out=om[:pairs * len(segs)].view(pairs, len(segs)), per_pair=per_pair)
        torch.cuda.synchronize()
        assert bool((obuf[n_out:] == float(hl.CANARY)).all()) and bool((om[pairs * len(segs):] == float(hl.CANARY)).all())
        assert np.array_equal(wa.cpu().numpy(), hl.widen(a, ab_ld)) and np.array_equal(wb.cpu().numpy(), hl.widen(b, ab_ld))
        return hl.narrow(obuf[:n_out].cpu().numpy(), pairs * P, D, out_ld), om[:pairs * len(segs)].view(pairs, len(segs)).cpu().numpy()
    return run


def test_latent_mix_kernel():
    """pairs in {1, 2, 65} x P in {1, 2, 9} x (Z in {4, 128} with the three standard segments | D = 5 with one) x t_per_pair, in tight and in wider rows"""
    run = _mix_on_device(_ops())
    worst = 0.0
    for c in hl.mix_cases():
        out, omega = run(c["a"], c["b"], c["t"], c["segs"], c["per_pair"], c["ab_ld"], c["out_ld"])
        worst = max(worst, hl.check_mix(c["a"], c["b"], c["t"], c["segs"], out, omega, c["per_pair"], c["tag"]))
    print("device mix: max |out - out64| / (|a| + |b|) = %.3e" % worst)


def test_latent_mix_exact_cases():
    hl.exact_mix_checks(_mix_on_device(_ops()))


def test_generate_morph_and_classes_end_to_end():
    pkg = load_package()
    m = hl.set_apart(make_model(64, 8, device=DEV), sigmas=8.0)
    Z, rows, steps = 8, 6, 8
    tok, z, comps = pkg.generate(m, rows, steps=steps, rhythm=[0, 1, 0, 1, 1, 0], key=5, seed=3)
    assert tok.is_cuda and tok.shape == (rows, steps) and tok.dtype == torch.int32 and z.shape == (rows, 2 * Z + 24) and comps.shape == (rows, 2)
    assert comps[:, 0].tolist() == [0, 1, 0, 1, 1, 0] and torch.equal(tok, pkg.greedy_decode(m, z, steps, want_logp=False)[1])
    for s, e in enumerate("rn"):
        ref = hl.draw_ref(getattr(m, "mu_%s_lookup" % e).weight.data.cpu().numpy(), getattr(m, "logvar_%s_lookup" % e).weight.data.cpu().numpy(), rows, s, 3, 0, 1.0,
                          comps[:, s].cpu().numpy())
        hl.check_draw(ref, z[:, s * Z:(s + 1) * Z].cpu().numpy(), tag=e)
    assert float(z[:, 2 * Z + 5].min()) == 1.0 and float(z[:, 2 * Z:].sum()) == rows
    tok2, z2, comps2 = pkg.generate(m, rows, steps=steps, rhythm=[0, 1, 0, 1, 1, 0], key=5, seed=3)
    assert torch.equal(tok2, tok) and torch.equal(z2, z) and torch.equal(comps2, comps)
    assert not torch.equal(pkg.generate(m, rows, steps=steps, key=5, seed=4)[1], z) and not torch.equal(pkg.generate(m, rows, steps=steps, key=5, seed=3, offset=1)[1][:, :Z], z[:, :Z])
    for kw in (dict(sample=dict(seed=1)), dict(beam=dict(width=2))):
        t3, z3, _ = pkg.generate(m, rows, steps=steps, rhythm=[0, 1, 0, 1, 1, 0], key=5, seed=3, **kw)
        assert t3.shape == (rows, steps) and torch.equal(z3, z) and int(t3.min()) >= 0 and int(t3.max()) < 342
    # morph: the ends of the path are the decodes of the two pieces' latents
    rs = np.random.RandomState(11)
    n = 3
    xa, xb = (torch.from_numpy(rs.randint(0, 342, (n, 20))).to(DEV) for _ in range(2))
    ca, cb = (torch.from_numpy(rs.rand(n, 24).astype(np.float32)).to(DEV) for _ in range(2))
    tokm, zm, om = pkg.morph(m, xa, ca, xb, cb, points=3, steps=steps)
    assert tokm.shape == (n, 3, steps) and zm.shape == (n, 3, 2 * Z + 24) and om.shape == (n, 2) and bool((om > 0).all())
    m.eval()
    dr, dn = m.encode(torch.cat([xa, xb]))
    m.train()
    zab = torch.cat([dr.mean, dn.mean, torch.cat([ca, cb])], 1)
    assert torch.equal(zm[:, 0], zab[:n]) and torch.equal(zm[:, 2], zab[n:])
    assert torch.equal(tokm[:, 0], pkg.greedy_decode(m, zab[:n].contiguous(), steps, want_logp=False)[1])
    assert torch.equal(tokm[:, 2], pkg.greedy_decode(m, zab[n:].contiguous(), steps, want_logp=False)[1])
    hl.check_mix(zab[:n].cpu().numpy(), zab[n:].cpu().numpy(), [0.0, 0.5, 1.0], hl.std_segs(Z), zm.reshape(n * 3, -1).cpu().numpy())
    # latent_classes names the component a row was drawn from at temperature 0
    z0, c0 = pkg.prior_latents(m, 16, key=0, temperature=0.0, seed=9)
    qr, qn, yr, yn = pkg.latent_classes(m, z0)
    assert torch.equal(yr, c0[:, 0]) and torch.equal(yn, c0[:, 1]) and len(set(c0[:, 0].tolist())) == 2
    assert float(qr.gather(1, c0[:, :1].long()).min()) > 0.99 and float(qn.gather(1, c0[:, 1:].long()).min()) > 0.99


def test_the_script_writes_the_files(tmp_path):
    out = str(tmp_path / "out")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "generate_midi.py"), "--config", os.path.join(ROOT, "tests", "golden", "gmm_model_config.json"), out,
                        "--rows", "2", "--steps", "8", "--rhythm", "1", "--note", "0", "--key", "3", "--temperature", "0.8", "--seed", "4"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "seeded initial weights" in p.stdout and "components [[1, 0], [1, 0]]" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])
    assert sorted(os.listdir(out)) == ["00000.mid", "00001.mid"]
