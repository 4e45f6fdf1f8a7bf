"""Importance-weighted log-likelihood (likelihood.py, fn_posterior_draw / fn_iw_reduce), CPU side: the float64 restatement on the conjugate Gaussian
model whose log p(x) is known (the exact-posterior identity, the mismatched proposal), the host twins in a stand-alone sanitizer build against the
restatement on the case lists, the twin's normals against fn_latent_draw's twin, the entry points' answers to bad arguments, and the Python layer on
stand-in ops."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers_latent_ops as hl
import helpers_likelihood as hk
from helpers import make_model
from mfn_import import ROOT, load_package


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the restatement on the conjugate model
# ------------------------------------------------------------------------------------------------------------------------------
def _conjugate_run(draw, reduce, m, S, seed, offset, tau):
    """draw(pre, mu_lk, lv_lk, S, seed, offset, tau) -> (z, logq, logp); the test's own Gaussian nll at that z; reduce(nll, B, S, logp, logq) -> (lw, out)"""
    B = m["truth"].size
    z, logq, logp = draw(m["pre"], m["mu_lk"], m["lv_lk"], S, seed, offset, tau)
    nll64, nll = hk.conjugate_nll(m, z, S)
    lw, out = reduce(nll, B, S, logp[None], logq[None])
    return logq, logp, lw, out, nll64


def _ref_draw(pre, mu_lk, lv_lk, S, seed, offset, tau):
    z = hk.post_ref(pre, S, 0, seed, offset, tau)["z"].astype(np.float32)
    lq, lp, _, _ = hk.densities(z, pre, hk.sg_of(pre, tau), mu_lk, lv_lk, S)
    return z, lq, lp


@pytest.mark.parametrize("Z", [1, 5, 130])
def test_exact_posterior_identity_on_the_restatement(Z):
    """K = 1, v = 0, x = mu / p1: q is the true posterior, so every log-weight is log p(x) whatever z was drawn - the signs and constants of both densities"""
    S = 257
    m = hk.conjugate(3, Z, 40 + Z)
    logq, logp, lw, out, nll64 = _conjugate_run(_ref_draw, hk.iw_ref, m, S, 11, 2, 1.0)
    print("Z %d: worst |lw - log p(x)| / bound %.3f" % (Z, hk.check_identity(m, S, logq, logp, lw, out, nll64)))


def test_mismatched_proposal_on_the_restatement():
    """tau 1.5 and the proposal mean 0.3 off, Z 8, S 4096, with the Philox normals: the bound closes on log p(x) within 6 of its own standard error while
    the one-sample ELBO stays more than a nat below"""
    S, worst = 4096, [0.0, 1.0, np.inf]
    for seed in range(6):
        m = hk.conjugate(4, 8, 100 + seed, shift=0.3)
        _, _, _, out, _ = _conjugate_run(_ref_draw, hk.iw_ref, m, S, seed, 5 * seed, 1.5)
        w = hk.check_mismatch(m, S, out, "seed %d" % seed)
        worst = [max(worst[0], w[0]), min(worst[1], w[1]), min(worst[2], w[2])]
    print("mismatched proposal: worst deviation %.2f units, least ess / S %.3f, least gap %.2f" % tuple(worst))


def test_post_normals_are_the_prior_draws_rows():
    """sample (b, s) is row b of helpers_latent_ops.draw_normals at offset + s, across the carry into the high word and the wrap"""
    for off in (0, 5, (1 << 32) - 2, hk.MASK64 - 1):
        n, r = hk.post_normals(3, 4, 6, 1, 9, off)
        for s in range(4):
            n1, r1 = hl.draw_normals(3, 6, 1, 9, (off + s) & hk.MASK64)
            assert np.array_equal(n[:, s], n1) and np.array_equal(r[:, s], r1), (off, s)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the host twins in a stand-alone sanitizer build
# ------------------------------------------------------------------------------------------------------------------------------
def _run(exe, fin, fout, blob):
    with open(fin, "wb") as f:
        f.write(blob)
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout[-1000:], p.stderr[-3000:])
    return open(fout, "rb").read()


def _build(tmp, name):
    src = os.path.join(ROOT, "music-fader-nets_amd", "csrc", "host", name + ".cpp")
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Werror", src, "-o", exe],
                   check=True, capture_output=True, timeout=300)
    return lambda blob: _run(exe, str(tmp / (name + "_in.bin")), str(tmp / (name + "_out.bin")), blob)


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no AddressSanitizer runtime on this box (gcc -print-file-name=libasan.so)")
    tmp = tmp_path_factory.mktemp("likelihood")
    return _build(tmp, "likelihood_check"), _build(tmp, "latent_ops_check")


def _twin_draw(twin):
    def draw(pre, mu_lk, lv_lk, S, seed, offset, tau):
        B, Z = pre.shape[0], pre.shape[1] // 2
        c = dict(tag="twin", B=B, S=S, Z=Z, z_ld=Z, col_step=0, jobs=[dict(pre=pre, mu_lk=mu_lk, lv_lk=lv_lk, stream_id=0)], tau=tau, seed=seed, offset=offset)
        z, _, lq, lp = hk.parse_draw(c, twin(hk.draw_blob(c)))
        return z.reshape(B * S, Z), lq[0], lp[0]
    return draw


def _twin_reduce(twin):
    def reduce(nll, B, S, logp, logq, t0=None, t1=None):
        c = dict(tag="twin", B=B, S=S, T=nll.shape[0], n_lat=logp.shape[0], nll=nll, logp=logp, logq=logq, t0=t0, t1=t1, nll_ld=B * S, lat_stride=B * S,
                 out_ld=4 + logp.shape[0])
        return hk.parse_reduce(c, twin(hk.reduce_blob(c)))
    return reduce


def test_host_twin_draw_against_the_restatement(twins):
    twin = twins[0]
    worst = [0.0] * 4
    for c in hk.draw_cases():
        z, eps, lq, lp = hk.parse_draw(c, twin(hk.draw_blob(c)))
        worst = [max(x, y) for x, y in zip(worst, hk.check_draw_case(c, z, eps, lq, lp))]
    print("twin draw: worst error / bound, eps %.3f z %.3f logq %.3f logp %.3f" % tuple(worst))
    # without eps_out the other outputs are the same
    c = hk.draw_cases()[7]
    full, bare = twin(hk.draw_blob(c)), twin(hk.draw_blob(c, flags=0))
    a, b = hk.parse_draw(c, full), hk.parse_draw(c, bare, flags=0)
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[2] + a[3], b[2] + b[3])) and b[1] is None


def test_host_twin_normals_are_latent_draws_rows(twins):
    """eps of sample (b, s) equals, bit for bit, row b of the twin of fn_latent_draw at offset + s; a row is unchanged by another B or S"""
    post, prior = twins
    g = np.random.RandomState(3)
    for Z, off in ((5, 3), (130, (1 << 32) - 2), (64, hk.MASK64 - 1)):
        B, S = 3, 5
        mu, lv = hl.lookups(g, 2, Z)
        pre = np.concatenate([g.randn(B, Z), -1.0 + g.rand(B, Z)], axis=1).astype(np.float32)
        case = lambda b, s: dict(tag="eps", B=b, S=s, Z=Z, z_ld=Z + 3, col_step=0, jobs=[dict(pre=pre[:b], mu_lk=mu, lv_lk=lv, stream_id=1)], tau=0.8, seed=77, offset=off)
        big, small = (hk.parse_draw(case(b, s), post(hk.draw_blob(case(b, s)))) for b, s in ((B, S), (1, 2)))
        for s in range(S):
            c1 = dict(tag="prior", rows=B, Z=Z, z_ld=Z, col_step=0, jobs=[dict(mu_lk=mu, lv_lk=lv, comp=None, stream_id=1)], tau=0.8, seed=77, offset=(off + s) & hk.MASK64)
            raw = prior(hl.draw_blob(c1, flags=2))
            eps1 = np.frombuffer(raw[4 + 4 * B * Z:], np.float32).reshape(B, Z)
            assert np.array_equal(big[1][0].reshape(B, S, Z)[:, s], eps1), (Z, off, s)
        ld = Z + 3
        zb = np.concatenate([big[0], np.zeros(3, np.float32)]).reshape(B * S, ld)[:, :Z].reshape(B, S, Z)
        zs = np.concatenate([small[0], np.zeros(3, np.float32)]).reshape(2, ld)[:, :Z]
        assert np.array_equal(zb[0, :2], zs) and np.array_equal(big[1][0].reshape(B, S, Z)[0, :2], small[1][0])
        assert np.array_equal(big[2][0][:2], small[2][0]) and np.array_equal(big[3][0][:2], small[3][0])


def test_host_twin_reduce_against_the_restatement(twins):
    twin = twins[0]
    worst = [0.0] * 3
    for c in hk.reduce_cases():
        lw, out = hk.parse_reduce(c, twin(hk.reduce_blob(c)))
        worst = [max(x, y) for x, y in zip(worst, hk.check_iw(c["nll"], c["B"], c["S"], c["logp"], c["logq"], c["t0"], c["t1"], lw, out, c["tag"]))]
        if c["t0"] is not None:          # a span is the nll rows cut to it
            cut = np.zeros((c["T"], c["nll"].shape[1]), np.float32)
            for b in range(c["B"]):
                a, e = np.clip(c["t0"][b], 0, c["T"]), np.clip(c["t1"][b], 0, c["T"])
                cut[a:e, b * c["S"]:(b + 1) * c["S"]] = c["nll"][a:e, b * c["S"]:(b + 1) * c["S"]]
            c2 = dict(c, nll=cut, t0=None, t1=None)
            lw2, out2 = hk.parse_reduce(c2, twin(hk.reduce_blob(c2)))
            assert lw2.tobytes() == lw.tobytes() and out2.tobytes() == out.tobytes(), c["tag"]
    print("twin reduce: worst error / bound, iwae %.3f elbo %.3f ess %.3f" % tuple(worst))


def test_host_twin_reduce_special_cases(twins):
    for c in hk.special_reduce_cases():
        lw, out = hk.parse_reduce(c, twins[0](hk.reduce_blob(c)))
        hk.check_iw(c["nll"], c["B"], c["S"], c["logp"], c["logq"], None, None, lw, out, c["tag"])
        hk.check_special(c, lw, out)


def test_host_twin_on_the_conjugate_model(twins):
    draw, reduce = _twin_draw(twins[0]), _twin_reduce(twins[0])
    for Z in (1, 5, 130):
        m = hk.conjugate(3, Z, 40 + Z)
        logq, logp, lw, out, nll64 = _conjugate_run(draw, reduce, m, 257, 11, 2, 1.0)
        print("twin Z %d: worst |lw - log p(x)| / bound %.3f" % (Z, hk.check_identity(m, 257, logq, logp, lw, out, nll64)))
    m = hk.conjugate(4, 8, 100, shift=0.3)
    out = _conjugate_run(draw, reduce, m, 4096, 0, 0, 1.5)[3]
    print("twin mismatched proposal: deviation %.2f units, ess / S %.3f, gap %.2f" % hk.check_mismatch(m, 4096, out))


def test_host_twin_answers_to_bad_sizes(twins):
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    rc = lambda blob: np.frombuffer(twins[0](blob), np.int32).tolist()
    par = hl.params_bytes().tobytes()
    job = lambda K, sid, B, Z: i32(K, sid) + np.zeros(2 * max(B, 0) * max(Z, 0) + 2 * max(K, 0) * max(Z, 0), np.float32).tobytes()
    #          n_jobs B  S  Z z_ld  K  stream
    for hd, want in (((0, 2, 2, 4, 4, 2, 0), -5), ((5, 2, 2, 4, 4, 2, 0), -5), ((1, 0, 2, 4, 4, 2, 0), -2), ((1, 2, 0, 4, 4, 2, 0), -2), ((1, 2, 2, 0, 4, 2, 0), -2),
                     ((1, 2, 2, 4, 3, 2, 0), -2), ((1, 2, 2, 4, 4, 0, 0), -2), ((1, 2, 2, 4, 4, 2, -1), -2), ((1, 2, 2, 4, 4, 2, 65535), -2),
                     ((1, 1, 1, 4097, 4097, 1, 0), -6), ((1, 1, 1, 4, 4, 9, 0), -6)):
        n_jobs, B, S, Z, z_ld, K, sid = hd
        assert rc(i32(0, n_jobs, B, S, Z, z_ld, 0, 1, 0, 0) + par + job(K, sid, B, Z) * min(max(n_jobs, 0), 8)) == [want], hd
    #          B  S  T nll_ld n_lat lat_stride out_ld
    for hd, want in (((2, 3, 4, 6, 0, 6, 6), -5), ((2, 3, 4, 6, 5, 6, 9), -5), ((0, 3, 4, 6, 1, 6, 5), -2), ((2, 0, 4, 6, 1, 6, 5), -2), ((2, 3, 0, 6, 1, 6, 5), -2),
                     ((2, 3, 4, 5, 1, 6, 5), -2), ((2, 3, 4, 6, 2, 5, 6), -2), ((2, 3, 4, 6, 2, 6, 5), -2)):
        B, S, T, nll_ld, n_lat, ls, out_ld = hd
        rows, nl = max(B, 0) * max(S, 0), min(max(n_lat, 0), 8)
        n_nll = (T - 1) * nll_ld + rows if T > 0 and rows > 0 else 0
        n_lp = (nl - 1) * ls + rows if nl > 0 and rows > 0 else 0
        blob = i32(1, B, S, T, nll_ld, n_lat, ls, out_ld, 0, 0) + np.zeros(max(n_nll, 0), np.float32).tobytes() + np.zeros(2 * max(n_lp, 0), np.float64).tobytes()
        assert rc(blob) == [want], hd


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the ABI without a GPU
# ------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_argument_errors_without_gpu():
    load_package()
    from music_fader_nets_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "fadernets.h")).read()
    for name, text in (("FN_POST_MAX_K", "8"), ("FN_IW_MAX_LAT", "4"), ("FN_IW_COLS", "4")):
        assert re.search(r"^#define %s %s\b" % (name, re.escape(text)), hdr, re.M) and int(text) == getattr(_lib, name), name
    assert C.sizeof(_lib.FnPostJob) == 64 and lib.fn_version() == 6
    assert {"fn_posterior_draw", "fn_iw_reduce"} <= set(_lib.SIGNATURES)
    twins = open(os.path.join(ROOT, "include", "fadernets_host.h")).read()
    assert "fn_posterior_draw_host" in twins and "fn_iw_reduce_host" in twins
    buf = (C.c_int32 * 4096)()
    at = (C.addressof(buf) + 15) // 16 * 16
    odd, odd4 = at + 2, at + 4

    def draw(n_jobs=2, B=3, S=2, Z=8, z_ld=40, params=at, jobs=True, **kw):
        arr = (_lib.FnPostJob * 5)()
        for j in arr:
            j.pre, j.mu_lk, j.lv_lk, j.z, j.eps_out, j.logq, j.logp, j.K, j.stream_id = at, at, at, at, None, at, at, 2, 1
        for k, v in kw.items():
            setattr(arr[1], k, v)                                             # the second job carries the fault
        return lib.fn_posterior_draw(arr if jobs else None, n_jobs, B, S, Z, z_ld, params, None)

    assert draw(jobs=False) == -1 and draw(params=None) == -1
    for k in ("pre", "mu_lk", "lv_lk", "z", "logq", "logp"):
        assert draw(**{k: None}) == -1, k
    assert draw(n_jobs=0) == -5 and draw(n_jobs=5) == -5 and draw(n_jobs=-1) == -5
    for kw in (dict(B=0), dict(B=-1), dict(S=0), dict(S=-2), dict(Z=0), dict(z_ld=7), dict(K=0), dict(K=-3), dict(stream_id=-1), dict(stream_id=65535)):
        assert draw(**kw) == -2, kw
    for kw in (dict(Z=4097, z_ld=4097), dict(K=9), dict(B=1 << 16, S=1 << 15), dict(B=(1 << 31) - 1, S=2)):
        assert draw(**kw) == -6, kw
    for k in ("pre", "mu_lk", "lv_lk", "z", "eps_out"):
        assert draw(**{k: odd}) == -3, k
    for k in ("logq", "logp"):
        assert draw(**{k: odd}) == -3 and draw(**{k: odd4}) == -3, k          # doubles: 8-byte aligned
    assert draw(params=odd) == -3
    # the order: null pointers first (in every job the count admits), then the count, the sizes, the limits, the alignment
    assert draw(n_jobs=5, z=None) == -1 and draw(n_jobs=0, params=None) == -1 and draw(B=0, logq=None) == -1
    assert draw(n_jobs=5, B=0) == -5 and draw(S=0, Z=4097, z_ld=4097) == -2 and draw(K=9, z=odd) == -6 and draw(K=0, z=odd) == -2

    def red(nll=at, T=4, nll_ld=8, t0=at, t1=at, logp=at, logq=at, n_lat=2, ls=8, B=2, S=3, lw=at, out=at, out_ld=6):
        return lib.fn_iw_reduce(nll, T, nll_ld, t0, t1, logp, logq, n_lat, ls, B, S, lw, out, out_ld, None)

    for k in ("nll", "logp", "logq", "lw", "out"):
        assert red(**{k: None}) == -1, k
    assert red(t0=None) == -1 and red(t1=None) == -1
    assert red(n_lat=0) == -5 and red(n_lat=5, out_ld=9) == -5 and red(n_lat=-1) == -5
    for kw in (dict(B=0), dict(S=0), dict(T=0), dict(B=-1), dict(nll_ld=5), dict(ls=5), dict(out_ld=5), dict(n_lat=1, out_ld=4)):
        assert red(**kw) == -2, kw
    assert red(B=1 << 16, S=1 << 15, nll_ld=1 << 31, ls=1 << 31) == -6
    for k in ("nll", "t0", "t1"):
        assert red(**{k: odd}) == -3, k
    for k in ("logp", "logq", "lw", "out"):
        assert red(**{k: odd}) == -3 and red(**{k: odd4}) == -3, k
    assert red(nll=None, n_lat=0) == -1 and red(n_lat=0, B=0) == -5 and red(B=0, lw=odd) == -2 and red(B=1 << 16, S=1 << 15, nll_ld=1 << 31, ls=1 << 31, lw=odd) == -6


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the Python layer on stand-ins
# ------------------------------------------------------------------------------------------------------------------------------
def _pieces(B=5, T=20, seed=11):
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.randint(1, 342, (B, T)))
    x[1, :3] = 0
    x[1, 15:] = 0
    x[2, :] = 0
    if B > 3:
        x[3, 12:] = 0
    return x, torch.from_numpy(rs.rand(B, 24).astype(np.float32))


def test_python_value_errors_come_before_any_launch():
    pkg = load_package()
    ops = hk.lik_fake_ops()
    m = make_model(64, 8, ops=ops)
    x, c = _pieces()
    ok = dict(x=x, chroma=c, samples=3)
    for kw in (dict(x=x[0]), dict(x=torch.zeros(5, 20, 341)), dict(x=torch.zeros(0, 20, dtype=torch.long)), dict(x=None), dict(x="ab"), dict(x=torch.full((5, 20), 342)),
               dict(x=torch.full((5, 20), -1)), dict(x=torch.zeros(5, 20, dtype=torch.bool)), dict(chroma=c[:4]), dict(chroma=torch.zeros(5, 23)), dict(chroma=None),
               dict(chroma="c"), dict(samples=0), dict(samples=2.0), dict(samples=True), dict(samples=(1 << 16) + 1), dict(samples=None), dict(temperature=0),
               dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(temperature=1e-60),
               dict(temperature=1e60), dict(temperature="1"), dict(seed=-1), dict(seed=1 << 64), dict(seed=1.0), dict(offset=1.5), dict(offset=-1), dict(offset=1 << 64),
               dict(trim=1), dict(trim=None), dict(rows_per_pass=0), dict(rows_per_pass=2.5), dict(rows_per_pass=True)):
        with pytest.raises(ValueError):
            pkg.marginal_likelihood(m, **dict(ok, **kw))
    with pytest.raises(ValueError):
        pkg.marginal_likelihood(torch.nn.Linear(2, 2), x, c)
    with pytest.raises(ValueError):
        pkg.likelihood_report(m, [(x, None, None, c)], samples=0)
    from music_fader_nets_amd.epochs import evaluation_phase
    for bad in (-1, 1.0, True, None):
        with pytest.raises(ValueError):
            evaluation_phase(None, [], iw_samples=bad)
    assert ops.calls == [] and ops.seen == []


def test_marginal_likelihood_on_stand_ins():
    """one encode of B rows, at most two decoder row counts, the draws independent of the passes, the reduce's columns, trim = the span's tokens"""
    pkg = load_package()
    from music_fader_nets_amd.likelihood import default_rows_per_pass, marginal_likelihood_detail
    ops = hk.lik_fake_ops()
    m = make_model(64, 8, ops=ops)
    x, c = _pieces()
    B, T, S, Z = 5, 20, 3, 8
    was = m.training
    runs = {}
    for per in (None, S, 2 * S, B * S, 1):
        ops.calls.clear(), ops.seen.clear()
        lik, d = marginal_likelihood_detail(m, x, c, samples=S, seed=4, offset=9, rows_per_pass=per)
        enc = [s for s in ops.seen if s[1] == 4]
        dec = sorted({s[2] for s in ops.seen if s[0] in ("dec_l1", "dec_l2")})
        assert enc == [(None, 4, B)] and ops.calls.count("posterior_draw") == 1 and m.training == was, (per, ops.seen)
        want = {None: [B * S], S: [S], 2 * S: [S, 2 * S], B * S: [B * S], 1: [S]}[per]
        assert dec == want and len(dec) <= 2 and ops.calls.count("iw_reduce") == -(-B * S // want[-1]), (per, dec)
        assert [t.dtype for t in lik] == [torch.float64] * 6 + [torch.int32, torch.float64] and all(t.shape == (B,) for t in lik[:7]) and lik.lw.shape == (B, S)
        assert d["z"].shape == (B, S, 2 * Z + 24) and torch.equal(d["z"][:, :, 2 * Z:], c[:, None, :].expand(B, S, 24)) and lik.n_tokens.tolist() == [T] * B
        runs[per] = (lik, d)
    lik, d = runs[None]
    for per in (S, 2 * S, B * S, 1):
        l2, d2 = runs[per]
        assert all(torch.equal(d[k], d2[k]) for k in ("z", "logp", "logq")), per          # the draws do not depend on the passes
        assert torch.allclose(l2.lw, lik.lw, rtol=0, atol=1e-9) and torch.allclose(l2.iwae, lik.iwae, rtol=0, atol=1e-9), per
    # the columns follow from lw, logp, logq by the restatement; the draws are the restatement's at (seed, offset), stream 0 rhythm and 1 note
    lw, logp, logq = lik.lw.numpy().reshape(-1), d["logp"].numpy().reshape(2, -1), d["logq"].numpy().reshape(2, -1)
    recon = lw - ((logp[0] - logq[0]) + (logp[1] - logq[1]))
    got = torch.stack(list(lik[:6]), 1).numpy()
    assert np.allclose(got[:, 1], lik.lw.numpy().mean(1), rtol=1e-13) and np.allclose(got[:, 3], recon.reshape(B, S).mean(1), rtol=1e-12)
    assert np.allclose(got[:, 4], (logq[0] - logp[0]).reshape(B, S).mean(1), rtol=1e-13) and np.allclose(got[:, 5], (logq[1] - logp[1]).reshape(B, S).mean(1), rtol=1e-13)
    mx = lik.lw.numpy().max(1)
    w = np.exp(lik.lw.numpy() - mx[:, None])
    assert np.allclose(got[:, 0], mx + np.log(w.sum(1)) - np.log(S), rtol=1e-13) and np.allclose(got[:, 2], w.sum(1) ** 2 / (w * w).sum(1), rtol=1e-12)
    assert (got[:, 0] >= got[:, 1]).all() and (got[:, 2] >= 1).all() and (got[:, 2] <= S * (1 + 1e-12)).all() and (recon < 0).all()
    m.eval()
    dis = m.encode(x)
    m.train(was)
    for k, (e, dd) in enumerate(zip("rn", dis)):
        pre = torch.cat([dd.mean, dd.stddev.log()], 1).numpy()
        ref = hk.post_ref(pre, S, k, 4, 9, 1.0)
        hl.check_draw(ref, d["z"][:, :, k * Z:(k + 1) * Z].reshape(B * S, Z).numpy(), tag=e)
    # another seed, offset or temperature: other draws; offset + 1 shifts the samples by one
    for kw in (dict(seed=5, offset=9), dict(seed=4, offset=8), dict(seed=4, offset=9, temperature=1.5)):
        assert not torch.equal(marginal_likelihood_detail(m, x, c, samples=S, **kw)[1]["z"], d["z"]), kw
    d1 = marginal_likelihood_detail(m, x, c, samples=S, seed=4, offset=10)[1]
    assert torch.equal(d1["z"][:, :S - 1], d["z"][:, 1:]) and torch.equal(d1["logq"][:, :, :S - 1], d["logq"][:, :, 1:])
    # one-hot input is the ids'
    l1 = pkg.marginal_likelihood(m, pkg.convert_to_one_hot(x, 342), c, samples=S, seed=4, offset=9)
    assert torch.equal(l1.lw, lik.lw)
    # trim: the same draws, the np.trim_zeros spans, and per sample the log-weight of the tokens inside the span
    lt, dt = marginal_likelihood_detail(m, x, c, samples=S, seed=4, offset=9, trim=True)
    assert all(torch.equal(d[k], dt[k]) for k in ("z", "logp", "logq"))
    spans = [(0, 20), (3, 15), (0, 0), (0, 12), (0, 20)]
    assert dt["t0"].tolist() == [a for a, _ in spans] and dt["t1"].tolist() == [b for _, b in spans] and lt.n_tokens.tolist() == [b - a for a, b in spans]
    assert torch.equal(lt.lw[0], lik.lw[0]) and torch.equal(lt.lw[4], lik.lw[4]) and float(lt.recon[2]) == 0.0 and bool((lt.recon[[1, 3]] > lik.recon[[1, 3]]).all())
    # the span of piece 3 starts at 0 and the decoder is causal: the run on the tokens cut to the span, at the same latent rows, scores the same tokens
    eng = m.engine()
    zc = d["z"][3].contiguous()
    xc = x[3:4, :12].to(torch.int32).repeat(S, 1).contiguous()
    dec = eng.global_decoder_tf(xc, zc, save=False, head=False)
    nll = torch.empty(12 * S)
    ops.out_head(dec["hx1"].view(12 * S, eng.H), eng.p["linear_out_g.weight"], eng.p["linear_out_g.bias"], S, 12, xc, nll_rows=nll)
    cut = -nll.view(12, S).double().sum(0) + (d["logp"][:, 3] - d["logq"][:, 3]).sum(0)
    assert torch.allclose(cut, lt.lw[3], rtol=0, atol=1e-4 * 12)
    assert default_rows_per_pass(100, 512, 64) == 16 * 64 and default_rows_per_pass(100, 512, 4096) == 4096 and default_rows_per_pass(20, 64, 3) % 3 == 0


def test_likelihood_report_follows_from_its_pieces():
    pkg = load_package()
    ops = hk.lik_fake_ops()
    m = make_model(64, 8, ops=ops)
    loader = []
    for i, B in enumerate((4, 3)):
        x, c = _pieces(B, 12, seed=20 + i)
        loader.append((x.float(), None, None, c.numpy(), None, None))          # as the loaders yield them: float ids, numpy chroma
    S = 4
    rep = pkg.likelihood_report(m, loader, samples=S, seed=3, offset=100, trim=True)
    liks = [pkg.marginal_likelihood(m, b[0], b[3], samples=S, seed=3, offset=100 + i * S, trim=True) for i, b in enumerate(loader)]
    cat = lambda k: torch.cat([getattr(l, k).double() for l in liks]).numpy()
    n, tok = 7, cat("n_tokens").sum()
    want = dict(nats_per_piece=-cat("iwae").sum() / n, nats_per_token=-cat("iwae").sum() / tok, bits_per_token=-cat("iwae").sum() / tok / np.log(2),
                elbo_per_piece=-cat("elbo").sum() / n, kl_r=cat("kl_r").mean(), kl_n=cat("kl_n").mean(), mean_ess=cat("ess").mean(), min_ess=cat("ess").min(), n_pieces=n)
    assert set(rep) == set(want)
    for k, v in want.items():
        assert np.isclose(rep[k], v, rtol=1e-12), (k, rep[k], v)
    assert rep["elbo_per_piece"] >= rep["nats_per_piece"] > 0 and 1 <= rep["min_ess"] <= rep["mean_ess"] <= S
    with pytest.raises(RuntimeError):
        pkg.likelihood_report(m, [], samples=S)


def test_evaluation_phase_is_unchanged_without_iw_samples_and_adds_one_line_with():
    pkg = load_package()
    from music_fader_nets_amd.synth import synth_batch

    def run(**kw):
        ops = hk.lik_fake_ops()
        m = make_model(64, 32, ops=ops)
        tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
        rs = np.random.RandomState(8)
        loaders = [[], []]
        for B in (4, 3):
            b = synth_batch(rs, B, 12, 8)
            loaders[0].append((b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"]))
        b = synth_batch(rs, 3, 12, 8)
        loaders[1].append((b["d"], b["r"], b["n"], b["c"], b["a"], b["a"], b["r_density"], b["n_density"]))
        lines = []
        torch.manual_seed(4)
        res = pkg.evaluation_phase(tr, loaders, log=lines.append, step=20000, **kw)
        return lines, list(ops.calls), res

    base, zero, iw = run(), run(iw_samples=0), run(iw_samples=3)
    assert zero[0] == base[0] and zero[1] == base[1] and len(base[0]) == 6 and all("iw" not in r for r in zero[2])
    assert "posterior_draw" not in base[1] and "iw_reduce" not in base[1]
    num = r"(-?\d[\d.e+-]*|nan)"
    assert len(iw[0]) == 8 and [l for l in iw[0] if not l.startswith("IW: ")] == base[0]
    for at, r in ((3, iw[2][0]), (7, iw[2][1])):
        assert re.fullmatch(r"IW: %s  %s  %s  %s  %s" % ((num,) * 5), iw[0][at]), iw[0][at]
        assert iw[0][at] == "IW: {:.4}  {:.4}  {:.4}  {:.4}  {:.4}".format(*[r["iw"][k] for k in ("nats_per_piece", "nats_per_token", "bits_per_token", "elbo_per_piece", "mean_ess")])
    assert [r["iw"]["n_pieces"] for r in iw[2]] == [7, 3] and iw[1].count("posterior_draw") == 3 and iw[1].count("iw_reduce") == 3
