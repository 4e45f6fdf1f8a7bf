"""Importance-weighted log-likelihood on a real MI355X: fn_posterior_draw and fn_iw_reduce against the float64 restatement of
tests/helpers_likelihood.py within the bounds the CPU tests hold the host twins to (canaries around every output, the normals bit-equal to the device's
own fn_latent_draw at offset + s, rows bit-equal whatever the launch), the conjugate Gaussian model whose log p(x) is known, and marginal_likelihood at
hidden 64, B 5, T 20, S 3 against the float64 oracle decoder at the device's own latent rows."""
import numpy as np
import pytest
import torch

import helpers_latent_ops as hl
import helpers_likelihood as hk
import helpers_report as hr
from helpers import make_model
from mfn_import import load_package
from oracle import gmvae_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64          # entries behind every output buffer that must come back as canaries
F64 = float(hk.CANARY)


def _ops():
    load_package()
    from music_fader_nets_amd.hipops import HipOps
    return HipOps(DEV)


def _canaries(n, dtype=torch.float32):
    return torch.full((n + GUARD,), F64, dtype=dtype, device=DEV)


def _device_sigma(ops, pre, mu_lk, lv_lk):
    """sigma = expf(v) as fn_latent_fwd stores it: the same expf the draw scales by tau"""
    B, Z, K = pre.shape[0], pre.shape[1] // 2, mu_lk.shape[0]
    f = lambda *s: torch.empty(*s, device=DEV)
    sigma = f(B, Z)
    ops.latent_fwd(pre, torch.zeros(B, Z, device=DEV), mu_lk, lv_lk, None, sigma, f(B, Z), f(B, K), f(B, K), torch.empty(B, dtype=torch.int32, device=DEV), f(B, 4))
    return sigma.cpu().numpy()


def _post_on_device(ops, c, with_eps=True):
    """-> (z buffer, [eps per job], [logq per job], [logp per job], [sg per job], [eps tensors on the device])"""
    B, S, Z, z_ld = c["B"], c["S"], c["Z"], c["z_ld"]
    rows = B * S
    zbuf = _canaries(rows * z_ld)
    z2 = zbuf[:rows * z_ld].view(rows, z_ld)
    jobs, eps, lq, lp, sg = [], [], [], [], []
    tau = np.float32(hl.clamp_tau(c["tau"]))
    for e, j in enumerate(c["jobs"]):
        eps.append(_canaries(rows * Z)), lq.append(_canaries(rows, torch.float64)), lp.append(_canaries(rows, torch.float64))
        pre, mu, lv = (torch.from_numpy(j[k]).to(DEV) for k in ("pre", "mu_lk", "lv_lk"))
        sg.append((tau * _device_sigma(ops, pre, mu, lv)).astype(np.float32))
        jobs.append(dict(pre=pre, mu_lk=mu, lv_lk=lv, z=z2[:, e * c["col_step"]:e * c["col_step"] + Z], logq=lq[e][:rows], logp=lp[e][:rows],
                         eps_out=eps[e][:rows * Z].view(rows, Z) if with_eps else None, stream_id=j["stream_id"]))
    ops.posterior_draw(jobs, S, torch.from_numpy(hl.params_bytes(c["seed"], c["offset"], c["tau"])).to(DEV))
    torch.cuda.synchronize()
    assert bool((zbuf[rows * z_ld:] == F64).all()), c["tag"]
    for e_, q_, p_ in zip(eps, lq, lp):
        assert bool((e_[rows * Z:] == F64).all()) and bool((q_[rows:] == F64).all()) and bool((p_[rows:] == F64).all()), c["tag"]
        assert with_eps or bool((e_ == F64).all()), c["tag"]
    return (zbuf[:rows * z_ld].cpu().numpy(), [e_[:rows * Z].view(rows, Z).cpu().numpy() for e_ in eps], [q_[:rows].cpu().numpy() for q_ in lq],
            [p_[:rows].cpu().numpy() for p_ in lp], sg, [e_[:rows * Z].view(B, S, Z) for e_ in eps])


def _prior_eps_on_device(ops, c, s):
    """eps_out of the device's own fn_latent_draw for the jobs' streams at offset + s -> [(B, Z) tensors]"""
    B, Z = c["B"], c["Z"]
    z = torch.empty(B, len(c["jobs"]) * Z, device=DEV)
    eps = [torch.empty(B, Z, device=DEV) for _ in c["jobs"]]
    jobs = [dict(mu_lk=torch.from_numpy(j["mu_lk"]).to(DEV), lv_lk=torch.from_numpy(j["lv_lk"]).to(DEV), z=z[:, e * Z:(e + 1) * Z], eps_out=eps[e], stream_id=j["stream_id"])
            for e, j in enumerate(c["jobs"])]
    ops.latent_draw(jobs, torch.from_numpy(hl.params_bytes(c["seed"], (c["offset"] + s) & hk.MASK64, c["tau"])).to(DEV))
    return eps


@pytest.mark.parametrize("Z", [1, 5, 64, 128, 130])
def test_posterior_draw_kernel(Z):
    """B in {1, 3} x S in {1, 2, 5, 65} x K in {1, 2, 8} x {1, 2, 4} jobs at this Z, in rows wider than what is written; tau 1, 1.5, 0.5, NaN; offsets
    that carry and wrap.  z and eps within helpers_latent_ops' bounds, log q and log p within 32 * 2^-52 of their magnitude sums of the float64
    recomputation from the returned z, eps bit-equal to the device's own fn_latent_draw at offset + s"""
    ops = _ops()
    worst = [0.0] * 4
    for c in hk.draw_cases(Z_set=(Z,), jobs_set=(1, 2, 4)):
        z, eps, lq, lp, sg, eps_dev = _post_on_device(ops, c)
        worst = [max(x, y) for x, y in zip(worst, hk.check_draw_case(c, z, eps, lq, lp, sg))]
        for s in sorted({0, 1, c["S"] // 2, c["S"] - 1} & set(range(c["S"]))):
            for a, b in zip(eps_dev, _prior_eps_on_device(ops, c, s)):
                assert torch.equal(a[:, s], b), (c["tag"], s)
    print("device draw Z %d: worst error / bound, eps %.3f z %.3f logq %.3f logp %.3f" % ((Z,) + tuple(worst)))


def test_posterior_draw_rows_do_not_depend_on_the_launch():
    """sample (b, s) of a (3, 65) launch is that of a (1, 2) launch, two jobs or one, with or without eps_out, bit for bit"""
    ops = _ops()
    g = np.random.RandomState(2)
    for Z in (5, 130):
        lk = [hl.lookups(g, 2, Z) for _ in range(2)]
        pre = [np.concatenate([g.randn(3, Z), -1.5 + 2 * g.rand(3, Z)], axis=1).astype(np.float32) for _ in range(2)]
        case = lambda B, S, streams: dict(tag="invariance", B=B, S=S, Z=Z, z_ld=2 * Z + 24, col_step=Z, tau=1.3, seed=11, offset=(1 << 32) - 1,
                                          jobs=[dict(pre=pre[e][:B], mu_lk=lk[e][0], lv_lk=lk[e][1], stream_id=e) for e in streams])
        big, small, one = (_post_on_device(ops, case(*a)) for a in ((3, 65, (0, 1)), (1, 2, (0, 1)), (3, 65, (0,))))
        bare = _post_on_device(ops, case(3, 65, (0, 1)), with_eps=False)
        ld = 2 * Z + 24
        zb, zs, zo = big[0].reshape(3, 65, ld), small[0].reshape(1, 2, ld), one[0].reshape(3, 65, ld)
        assert np.array_equal(zb[:1, :2, :2 * Z], zs[:, :, :2 * Z]) and np.array_equal(zb[:, :, :Z], zo[:, :, :Z]) and np.array_equal(bare[0], big[0])
        for k in (1, 2, 3):
            for e in (0, 1):
                assert np.array_equal(big[k][e].reshape(3, 65, -1)[0, :2].ravel(), small[k][e].ravel()), (Z, k, e)
                assert k == 1 or np.array_equal(big[k][e], bare[k][e]), (Z, k, e)
            assert np.array_equal(big[k][0], one[k][0]), (Z, k)


def _reduce_on_device(ops):
    def run(c):
        B, S, T, n_lat, rows = c["B"], c["S"], c["T"], c["n_lat"], c["B"] * c["S"]
        nll = torch.from_numpy(hk.widen64(c["nll"], c["nll_ld"], np.float32(np.nan))).to(DEV)
        lp, lq = (torch.from_numpy(hk.widen64(c[k], c["lat_stride"], np.nan)).to(DEV) for k in ("logp", "logq"))
        n_out = (B - 1) * c["out_ld"] + 4 + n_lat
        lw, out = _canaries(rows, torch.float64), _canaries(n_out, torch.float64)
        t0, t1 = (None if c[k] is None else torch.from_numpy(c[k]).to(DEV) for k in ("t0", "t1"))
        ops.iw_reduce(torch.as_strided(nll, (T, rows), (c["nll_ld"], 1)), B, S, torch.as_strided(lp, (n_lat, rows), (c["lat_stride"], 1)),
                      torch.as_strided(lq, (n_lat, rows), (c["lat_stride"], 1)), lw[:rows], torch.as_strided(out, (B, 4 + n_lat), (c["out_ld"], 1)), t0=t0, t1=t1)
        torch.cuda.synchronize()
        assert bool((lw[rows:] == F64).all()) and bool((out[n_out:] == F64).all()), c["tag"]
        full = torch.cat([out[:n_out], torch.full((B * c["out_ld"] - n_out,), F64, dtype=torch.float64, device=DEV)]).view(B, c["out_ld"])
        assert bool((full[:, 4 + n_lat:] == F64).all()), c["tag"]
        return lw[:rows].cpu().numpy(), full[:, :4 + n_lat].cpu().numpy()
    return run


def test_iw_reduce_kernel():
    """B in {1, 5} x S in {1, 2, 63, 64, 65, 257} x T in {1, 20} x n_lat in {1, 2}, spans NULL, given (clamped) and one empty, sentinels behind every
    used column: lw bit for bit, the columns within the stated bounds, a second launch with the same bits"""
    run = _reduce_on_device(_ops())
    worst = [0.0] * 3
    for c in hk.reduce_cases():
        lw, out = run(c)
        worst = [max(x, y) for x, y in zip(worst, hk.check_iw(c["nll"], c["B"], c["S"], c["logp"], c["logq"], c["t0"], c["t1"], lw, out, c["tag"]))]
        lw2, out2 = run(c)
        assert lw2.tobytes() == lw.tobytes() and out2.tobytes() == out.tobytes(), c["tag"]
    print("device reduce: worst error / bound, iwae %.3f elbo %.3f ess %.3f" % tuple(worst))


def test_iw_reduce_special_cases():
    run = _reduce_on_device(_ops())
    for c in hk.special_reduce_cases():
        lw, out = run(c)
        hk.check_iw(c["nll"], c["B"], c["S"], c["logp"], c["logq"], None, None, lw, out, c["tag"])
        hk.check_special(c, lw, out)


def test_conjugate_model_through_the_device_entry_points():
    """the exact-posterior identity at Z in {1, 5, 130}, S 257, and the mismatched proposal (tau 1.5, mean 0.3 off, Z 8, S 4096) with their conditions"""
    ops = _ops()
    red = _reduce_on_device(ops)

    def draw(pre, mu_lk, lv_lk, S, seed, offset, tau):
        B, Z = pre.shape[0], pre.shape[1] // 2
        c = dict(tag="conjugate", B=B, S=S, Z=Z, z_ld=Z, col_step=0, jobs=[dict(pre=pre, mu_lk=mu_lk, lv_lk=lv_lk, stream_id=0)], tau=tau, seed=seed, offset=offset)
        z, _, lq, lp, _, _ = _post_on_device(ops, c)
        return z.reshape(B * S, Z), lq[0], lp[0]

    def reduce(nll, B, S, logp, logq):
        return red(dict(tag="conjugate", B=B, S=S, T=nll.shape[0], n_lat=1, nll=nll, logp=logp, logq=logq, t0=None, t1=None, nll_ld=B * S, lat_stride=B * S, out_ld=5))

    def go(m, S, seed, offset, tau):
        z, logq, logp = draw(m["pre"], m["mu_lk"], m["lv_lk"], S, seed, offset, tau)
        nll64, nll = hk.conjugate_nll(m, z, S)
        lw, out = reduce(nll, m["truth"].size, S, logp[None], logq[None])
        return logq, logp, lw, out, nll64

    for Z in (1, 5, 130):
        m = hk.conjugate(3, Z, 40 + Z)
        logq, logp, lw, out, nll64 = go(m, 257, 11, 2, 1.0)
        print("device Z %d: worst |lw - log p(x)| / bound %.3f" % (Z, hk.check_identity(m, 257, logq, logp, lw, out, nll64)))
    m = hk.conjugate(4, 8, 100, shift=0.3)
    print("device mismatched proposal: deviation %.2f units, ess / S %.3f, gap %.2f" % hk.check_mismatch(m, 4096, go(m, 4096, 0, 0, 1.5)[3]))


def test_marginal_likelihood_end_to_end():
    """hidden 64, B 5, T 20, S 3 (the shape of test_gpu_report.py): recon per (b, s) against the float64 oracle decoder at the device's own latent rows
    within T * 1e-4; the columns from the device's own lw, logp, logq by the restatement; the draws bit-equal for one piece per pass and for all, iwae
    within T * 1e-4 across them; trim = the oracle's log-probabilities of the tokens inside the np.trim_zeros span, and the decoder run on the cut tokens"""
    pkg = load_package()
    from music_fader_nets_amd.likelihood import marginal_likelihood_detail
    m = make_model(64, 32, device=DEV)
    b = hr.report_batch()
    B, T, S, Z = 5, 20, 3, 32
    x = torch.from_numpy(np.asarray(b["d"])).long().clone()
    x[3, 12:] = 0
    c = torch.from_numpy(np.asarray(b["c"], np.float32))
    tol = T * 1e-4
    lik, d = marginal_likelihood_detail(m, x.to(DEV), c.to(DEV), samples=S, seed=6, offset=1)
    assert all(t.is_cuda for t in lik) and lik.lw.shape == (B, S) and lik.n_tokens.tolist() == [T] * B and m.training
    sd64 = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    teacher = x.repeat_interleave(S, 0)
    with torch.no_grad():
        lp64 = orc.global_decoder(sd64, d["z"].reshape(B * S, -1).double().cpu(), T, teacher=teacher)
    tok = lp64.gather(-1, teacher.unsqueeze(-1)).squeeze(-1).numpy()                      # (B*S, T) log-probabilities of the target tokens
    lw, logp, logq = lik.lw.cpu().numpy().reshape(-1), d["logp"].cpu().numpy().reshape(2, -1), d["logq"].cpu().numpy().reshape(2, -1)
    recon = lw - ((logp[0] - logq[0]) + (logp[1] - logq[1]))
    print("max |recon - oracle| %.3e (tolerance %.1e)" % (float(np.abs(recon - tok.sum(1)).max()), tol))
    assert (np.abs(recon - tok.sum(1)) <= tol).all()
    out = torch.stack(list(lik[:6]), 1).cpu().numpy()
    hk.check_iw(None, B, S, logp, logq, None, None, lw, out, "model", own_lw=True)
    assert np.allclose(out[:, 3], recon.reshape(B, S).mean(1), rtol=0, atol=1e-9)
    # the latent rows are the restatement's draws from the encoder's posterior; the densities hold their bounds at them
    m.eval()
    dis = m.encode(x.to(DEV))
    m.train()
    ops = m.engine().ops
    for k, (e, dd) in enumerate(zip("rn", dis)):
        pre = torch.cat([dd.mean, dd.stddev.log()], 1)
        mu_lk, lv_lk = (getattr(m, "%s_%s_lookup" % (w, e)).weight.data.float().contiguous() for w in ("mu", "logvar"))
        zz = np.ascontiguousarray(d["z"][:, :, k * Z:(k + 1) * Z].reshape(B * S, Z).cpu().numpy())
        hl.check_draw(hk.post_ref(pre.cpu().numpy(), S, k, 6, 1, 1.0), zz, tag=e)
    # passes
    one, d_one = marginal_likelihood_detail(m, x.to(DEV), c.to(DEV), samples=S, seed=6, offset=1, rows_per_pass=S)
    assert all(torch.equal(d[k], d_one[k]) for k in ("z", "logp", "logq"))
    assert float((one.iwae - lik.iwae).abs().max()) <= tol and float((one.lw - lik.lw).abs().max()) <= tol
    # trim
    lt, dt = marginal_likelihood_detail(m, x.to(DEV), c.to(DEV), samples=S, seed=6, offset=1, trim=True)
    assert all(torch.equal(d[k], dt[k]) for k in ("z", "logp", "logq"))
    spans = []
    for row in x.numpy():
        nz = np.nonzero(row)[0]
        spans.append((int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0))
    assert lt.n_tokens.tolist() == [e - a for a, e in spans] and [len(np.trim_zeros(r)) for r in x.numpy()] == lt.n_tokens.tolist()
    want = np.array([tok[i, spans[i // S][0]:spans[i // S][1]].sum() for i in range(B * S)])
    lwt = lt.lw.cpu().numpy().reshape(-1)
    assert (np.abs(lwt - ((logp[0] - logq[0]) + (logp[1] - logq[1])) - want) <= tol).all() and float(lt.recon[2]) == 0.0
    hk.check_iw(None, B, S, logp, logq, None, None, lwt, torch.stack(list(lt[:6]), 1).cpu().numpy(), "model trim", own_lw=True)
    # a piece whose span starts at 0 (the decoder is causal): the decoder run on the tokens cut to the span, at the same latent rows
    p, n = next((i, e) for i, (a, e) in enumerate(spans) if a == 0 and 2 <= e < T)
    eng = m.engine()
    xc = x[p:p + 1, :n].to(torch.int32).repeat(S, 1).contiguous().to(DEV)
    dec = eng.global_decoder_tf(xc, d["z"][p].contiguous(), save=False, head=False)
    nll = torch.empty(n * S, device=DEV)
    ops.out_head(dec["hx1"].view(n * S, eng.H), eng.p["linear_out_g.weight"], eng.p["linear_out_g.bias"], S, n, xc, nll_rows=nll)
    cut = -nll.view(n, S).double().sum(0) + (d["logp"][:, p] - d["logq"][:, p]).sum(0)
    assert float((cut - lt.lw[p]).abs().max()) <= tol
    # the loader report and the evaluation line
    rep = pkg.likelihood_report(m, [(x, None, None, c)], samples=S, seed=6, offset=1)
    assert rep["n_pieces"] == B and np.isclose(rep["nats_per_piece"], -float(lik.iwae.mean()), rtol=1e-12) and 1 <= rep["min_ess"] <= S
