"""Checking tools of the importance-weighted log-likelihood (likelihood.py, fn_posterior_draw / fn_iw_reduce):

  post_normals / post_ref / densities   the draw of include/fadernets.h restated in float64 numpy, every sum in the stated order (lane-strided partial
                                        sums, then the xor butterfly); the Philox rounds are helpers_sampling's, the Box-Muller helpers_latent_ops'
  iw_ref                                the reduce restated the same way
  check_post / check_iw                 a result against the restatement within the bounds the issue of this feature sets (stated where they are checked)
  draw_cases / reduce_cases             the case lists the host twin and the device are put through, with the blobs of the stand-alone program
  conjugate                             the Gaussian model whose marginal likelihood is known in closed form (the exact-posterior identity, the
                                        mismatched proposal)
  lik_fake_ops                          helpers_report.report_fake_ops() + the two entry points as their restatement: likelihood.py on the CPU
"""
import numpy as np
import torch

import helpers_latent_ops as hl
import helpers_report as hr
from helpers_sampling import philox4x32_10

LOG_2PI = float(np.log(2.0 * np.pi))
EPS64 = 2.0 ** -52
CANARY = hl.CANARY
MASK64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------------------------------------
# the stated orders
# ------------------------------------------------------------------------------------------------------------------------------
def wave_sum(x):
    """the sum over the last axis as one wavefront forms it: lane l adds its entries l, l + 64, ... ascending from 0.0, then s[l] += s[l ^ o] for
    o = 32 .. 1 (entries past the end count as absent: a lane that has none keeps 0.0)"""
    x = np.asarray(x, np.float64)
    n = x.shape[-1]
    part = np.zeros(x.shape[:-1] + (64,))
    for j0 in range(0, n, 64):
        w = min(64, n - j0)
        part[..., :w] = part[..., :w] + x[..., j0:j0 + w]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[..., lanes ^ o]
    return part[..., 0]


# ------------------------------------------------------------------------------------------------------------------------------
# the draw
# ------------------------------------------------------------------------------------------------------------------------------
def post_normals(B, S, Z, stream_id, seed=0, offset=0):
    """steps 1 of fn_posterior_draw -> (eps (B, S, Z) float64, r (B, S, Z) float64: the radius behind every normal); sample (b, s) is row b of
    helpers_latent_ops.draw_normals at offset + s (the 64-bit add wraps)"""
    nq = (Z + 3) // 4
    off = [(offset + s) & MASK64 for s in range(S)]
    ctr = np.empty((B, S, nq, 4), np.uint64)
    ctr[..., 0] = np.arange(B, dtype=np.uint64).reshape(B, 1, 1)
    ctr[..., 1] = ((stream_id << 16) | np.arange(nq)).astype(np.uint64).reshape(1, 1, nq)
    ctr[..., 2] = np.array([o & 0xffffffff for o in off], np.uint64).reshape(1, S, 1)
    ctr[..., 3] = np.array([o >> 32 for o in off], np.uint64).reshape(1, S, 1)
    w = philox4x32_10(ctr, np.array([seed & 0xffffffff, seed >> 32], dtype=np.uint64)).astype(np.uint64)
    ua = ((w[..., 0::2] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    ub = (w[..., 1::2] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(ua))
    s, c = hl.sincospi(2.0 * ub)
    n = np.stack([r * c, r * s], axis=-1).reshape(B, S, 4 * nq)[..., :Z]
    return n, np.repeat(r, 2, axis=-1).reshape(B, S, 4 * nq)[..., :Z]


def sg_of(pre, tau):
    """sg = tau * expf(v) as float32 (B, Z): the exponential in float64 rounded once (what the host twin computes), times the clamped tau in float32.
    The device's expf may differ from this by an ulp: the GPU tests take sigma from fn_latent_fwd, which stores the same expf(v)"""
    Z = pre.shape[1] // 2
    return (np.float32(hl.clamp_tau(tau)) * np.exp(pre[:, Z:].astype(np.float64)).astype(np.float32)).astype(np.float32)


def post_ref(pre, S, stream_id, seed=0, offset=0, tau=1.0):
    """one job -> the dict helpers_latent_ops.check_draw takes (z, eps, r, sigma, mu (B*S, Z) float64, comp None, tau)"""
    B, Z = pre.shape[0], pre.shape[1] // 2
    n, r = post_normals(B, S, Z, stream_id, seed, offset)
    t = hl.clamp_tau(tau)
    mu = np.repeat(pre[:, :Z].astype(np.float64), S, axis=0)
    sigma = np.repeat(np.exp(pre[:, Z:].astype(np.float64)), S, axis=0)
    n, r = n.reshape(B * S, Z), r.reshape(B * S, Z)
    return dict(z=mu + (t * sigma) * n, eps=n, r=r, sigma=sigma, mu=mu, comp=None, tau=t)


def densities(z, pre, sg, mu_lk, lv_lk, S):
    """log q and the mixture log p at the STORED float32 z (B*S, Z), with mu = pre[:, :Z] and the float32 sg (B, Z), in float64 and in the stated
    orders -> (logq, logp (B*S,), mag_q, mag_p (B*S,): sum_j (|quadratic piece| + |lv| + LOG_2PI) / 2, what the bounds scale with; for q |lv| is
    2 |log sg|, for p the largest of the components, plus |log(1 / K)|)"""
    Z, K = z.shape[1], mu_lk.shape[0]
    z64 = z.astype(np.float64)
    mu = np.repeat(pre[:, :Z].astype(np.float64), S, axis=0)
    s64 = np.repeat(sg.astype(np.float64), S, axis=0)
    d = (z64 - mu) / s64
    logq = wave_sum(-0.5 * (d * d + LOG_2PI) - np.log(s64))
    mag_q = (0.5 * (d * d + LOG_2PI) + np.abs(np.log(s64))).sum(-1)
    ll, mags = [], []
    for k in range(K):
        lv, dz = lv_lk[k].astype(np.float64), z64 - mu_lk[k].astype(np.float64)
        quad = dz * dz * np.exp(-lv)
        ll.append(wave_sum(-0.5 * (quad + lv + LOG_2PI)) + np.log(1.0 / K))
        mags.append((0.5 * (quad + np.abs(lv) + LOG_2PI)).sum(-1) + abs(np.log(1.0 / K)))
    ll = np.stack(ll, 0)
    m = ll.max(0)
    den = np.zeros_like(m)
    for k in range(K):
        den = den + np.exp(ll[k] - m)
    return logq, m + np.log(den), mag_q, np.stack(mags, 0).max(0)


DENSITY_BOUND = 32 * EPS64
"""|log q - ref|, |log p - ref| <= 32 * 2^-52 * sum_j (|quadratic piece| + |lv| + LOG_2PI) / 2: a term takes at most 5 roundings, a lane's partial sum at
Z <= 130 three additions and the butterfly six more (at most 9 additions), the exponential of the variance errs by an ulp - 15 half-ulps of the
magnitude where the bound allows 64.  log p adds the maximum, K exponentials, a logarithm and an addition on sums that each hold their bound: the
log-sum-exp moves by no more than its largest argument does, and its own three roundings fit the same slack."""


def check_post(pre, S, sg, mu_lk, lv_lk, z, logq, logp, tag=""):
    """the densities a job returned against the float64 recomputation from the z it returned -> the largest error / bound ratios (q, p)"""
    rq, rp, mag_q, mag_p = densities(z, pre, sg, mu_lk, lv_lk, S)
    eq, ep = np.abs(logq - rq), np.abs(logp - rp)
    assert np.isfinite(logq).all() and np.isfinite(logp).all(), tag
    assert (eq <= DENSITY_BOUND * mag_q).all(), (tag, "logq", float((eq / (DENSITY_BOUND * mag_q)).max()))
    assert (ep <= DENSITY_BOUND * mag_p).all(), (tag, "logp", float((ep / (DENSITY_BOUND * mag_p)).max()))
    return float((eq / (DENSITY_BOUND * mag_q)).max()), float((ep / (DENSITY_BOUND * mag_p)).max())


def draw_cases(B_set=(1, 3), S_set=(1, 2, 5, 65), Z_set=(1, 5, 64, 128, 130), K_set=(1, 2, 8), jobs_set=None):
    """B x S x Z x K, turning through: one job at z_ld = Z + 3 | two jobs at z_ld = 2Z+24, the second at column Z | four jobs at z_ld = 4Z+3 (always
    wider than what is written: untouched sentinel columns); tau 1 | 1.5 | 0.5 | NaN (-> 1); seeds and offsets up to 64 bits, offsets whose offset + s
    carries into the high word and wraps.  jobs_set: every one of these job counts for every shape instead of turning through them"""
    g = np.random.RandomState(15)
    cases, i = [], 0
    for B in B_set:
        for S in S_set:
            for Z in Z_set:
                for K in K_set:
                    for n_jobs in jobs_set or [(1, 2, 4)[i % 3]]:
                        z_ld = {1: Z + 3, 2: 2 * Z + 24, 4: 4 * Z + 3}[n_jobs]
                        jobs = []
                        for e in range(n_jobs):
                            mu, lv = hl.lookups(g, K, Z)
                            pre = np.concatenate([g.randn(B, Z), -2.0 + 2.5 * g.rand(B, Z)], axis=1).astype(np.float32)
                            jobs.append(dict(pre=pre, mu_lk=mu, lv_lk=lv, stream_id=(0, 1, 7, 65534)[e]))
                        cases.append(dict(tag="B %d S %d Z %d K %d jobs %d" % (B, S, Z, K, n_jobs), B=B, S=S, Z=Z, z_ld=z_ld, col_step=Z if n_jobs > 1 else 0,
                                          jobs=jobs, tau=(1.0, 1.5, 0.5, float("nan"))[i % 4], seed=(2024, 7, MASK64, 1 << 40)[i % 4],
                                          offset=(0, 3, (1 << 32) - 2, MASK64 - 1)[(i // 2) % 4]))
                        i += 1
    return cases


def check_draw_case(c, z, eps, logq, logp, sg=None):
    """z: the whole buffer [(B*S-1)*z_ld + (n_jobs-1)*col_step + Z]; eps, logq, logp: per job; sg: per job (B, Z) float32 or None = sg_of
    -> worst ratios (eps, z, logq, logp)"""
    B, S, Z, z_ld = c["B"], c["S"], c["Z"], c["z_ld"]
    rows = B * S
    full = np.concatenate([z, np.full(rows * z_ld - z.size, CANARY, np.float32)]).reshape(rows, z_ld)
    used = np.zeros(z_ld, bool)
    worst = [0.0] * 4
    for e, j in enumerate(c["jobs"]):
        ref = post_ref(j["pre"], S, j["stream_id"], c["seed"], c["offset"], c["tau"])
        col = e * c["col_step"]
        used[col:col + Z] = True
        zz = np.ascontiguousarray(full[:, col:col + Z])
        w = hl.check_draw(ref, zz, None if eps is None else eps[e], None, c["tag"])
        w += list(check_post(j["pre"], S, sg_of(j["pre"], c["tau"]) if sg is None else sg[e], j["mu_lk"], j["lv_lk"], zz, logq[e], logp[e], c["tag"]))
        worst = [max(x, y) for x, y in zip(worst, w)]
    assert (full[:, ~used] == CANARY).all(), c["tag"]
    return worst


def draw_blob(c, flags=1):
    """the in.bin of likelihood_check.cpp for a draw case"""
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    blob = i32(0, len(c["jobs"]), c["B"], c["S"], c["Z"], c["z_ld"], c["col_step"], flags, 0, 0)
    blob += hl.params_bytes(c["seed"], c["offset"], c["tau"]).tobytes()
    for j in c["jobs"]:
        blob += i32(j["mu_lk"].shape[0], j["stream_id"]) + j["pre"].tobytes() + j["mu_lk"].tobytes() + j["lv_lk"].tobytes()
    return blob


def parse_draw(c, raw, flags=1):
    """out.bin of a draw case -> (z buffer, [eps per job] or None, [logq per job], [logp per job])"""
    rows, Z, n = c["B"] * c["S"], c["Z"], len(c["jobs"])
    assert np.frombuffer(raw[:4], np.int32)[0] == 0, c["tag"]
    nz = (rows - 1) * c["z_ld"] + (n - 1) * c["col_step"] + Z
    ne = n * rows * Z if flags & 1 else 0
    assert len(raw) == 4 + 4 * (nz + ne) + 16 * n * rows, c["tag"]
    f = np.frombuffer(raw[4:4 + 4 * (nz + ne)], np.float32)
    dd = np.frombuffer(raw[4 + 4 * (nz + ne):], np.float64).reshape(2, n, rows)
    eps = [f[nz + e * rows * Z:nz + (e + 1) * rows * Z].reshape(rows, Z) for e in range(n)] if flags & 1 else None
    return f[:nz], eps, list(dd[0]), list(dd[1])


# ------------------------------------------------------------------------------------------------------------------------------
# the reduce
# ------------------------------------------------------------------------------------------------------------------------------
def iw_ref(nll, B, S, logp, logq, t0=None, t1=None, with_recon=False, lw_given=None):
    """nll (T, >= B*S) float32, logp, logq (n_lat, B*S) float64, t0, t1 (B,) or None -> (lw (B*S,), out (B, 4 + n_lat)), in the stated orders; with_recon:
    and the per-row recon (B*S,); lw_given: these log-weights (B*S,) instead of the first pass's (a result's own lw: the second pass alone)"""
    T, rows, n_lat = nll.shape[0], B * S, logp.shape[0]
    ta = np.zeros(B, np.int64) if t0 is None else np.clip(np.asarray(t0, np.int64), 0, T)
    tb = np.full(B, T, np.int64) if t1 is None else np.clip(np.asarray(t1, np.int64), 0, T)
    ta, tb = np.repeat(ta, S), np.repeat(tb, S)
    nl = np.zeros(rows)
    for t in range(T):
        nl = np.where((t >= ta) & (t < tb), nl + nll[t, :rows].astype(np.float64), nl)
    recon = -nl
    lw = recon.copy()
    for e in range(n_lat):
        lw = lw + (logp[e] - logq[e])
    if lw_given is not None:
        lw = np.asarray(lw_given, np.float64).reshape(rows)
    out = np.zeros((B, 4 + n_lat))
    L = lw.reshape(B, S)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = L.max(1)
        x = np.exp(L - m[:, None])
        W1, W2 = wave_sum(x), wave_sum(x * x)
        out[:, 0] = m + np.log(W1) - np.log(float(S))
        out[:, 1] = wave_sum(L) / float(S)
        out[:, 2] = W1 * W1 / W2
    out[:, 3] = wave_sum(recon.reshape(B, S)) / float(S)
    for e in range(n_lat):
        out[:, 4 + e] = wave_sum((logq[e] - logp[e]).reshape(B, S)) / float(S)
    dead = m == -np.inf
    out[dead, 0], out[dead, 1], out[dead, 2] = -np.inf, -np.inf, 0.0
    return (lw, out, recon) if with_recon else (lw, out)


def _within(a, r, bound):
    """equal (infinities included), or finite and within the bound"""
    with np.errstate(invalid="ignore"):
        return (a == r) | (np.abs(a - r) <= bound)


def check_iw(nll, B, S, logp, logq, t0, t1, lw, out, tag="", own_lw=False):
    """own_lw: the columns iwae, elbo, ess and kl from the result's own lw (nll may be None; lw and the recon column are then not compared).  lw bit for bit (additions only, in the stated order); |iwae - ref| <= 2^-52 (16 + 2 |ref|); elbo within 16 * 2^-52 * mean |lw|, the means of
    recon and of log q - log p the same way on their own terms; ess within 32 * 2^-52 relative -> the largest error / bound ratios (iwae, elbo, ess)"""
    if own_lw:
        nll = np.zeros((1, B * S), np.float32)
    rl, ro, rec = iw_ref(nll, B, S, logp, logq, t0, t1, with_recon=True, lw_given=lw if own_lw else None)
    assert lw.tobytes() == rl.tobytes(), (tag, "lw", float(np.abs(lw - rl).max()))
    n_lat = logp.shape[0]
    L = rl.reshape(B, S)
    live = np.isfinite(ro[:, 0])
    assert np.array_equal(out[~live, :3], ro[~live, :3]), (tag, out[~live], ro[~live])
    b_iw = EPS64 * (16 + 2 * np.abs(ro[live, 0]))
    fin = np.where(np.isfinite(L), np.abs(L), 0.0)
    b_el = np.maximum(16 * EPS64 * fin.mean(1), 1e-300)
    e_iw, e_ess = np.abs(out[live, 0] - ro[live, 0]), np.abs(out[live, 2] - ro[live, 2]) / ro[live, 2]
    elbo_live = np.isfinite(ro[:, 1])
    assert np.array_equal(out[~elbo_live, 1], ro[~elbo_live, 1]), (tag, "elbo")
    e_el = np.abs(out[elbo_live, 1] - ro[elbo_live, 1])
    assert (e_iw <= b_iw).all(), (tag, "iwae", float((e_iw / b_iw).max()))
    assert (e_el <= b_el[elbo_live]).all(), (tag, "elbo", float((e_el / b_el[elbo_live]).max()))
    assert (e_ess <= 32 * EPS64).all() and (out[live, 2] >= 1 - 32 * EPS64).all() and (out[live, 2] <= S * (1 + 32 * EPS64)).all(), (tag, "ess", out[:, 2], ro[:, 2])
    assert own_lw or _within(out[:, 3], ro[:, 3], 16 * EPS64 * np.abs(rec).reshape(B, S).mean(1)).all(), (tag, "recon")
    for e in range(n_lat):
        assert _within(out[:, 4 + e], ro[:, 4 + e], 16 * EPS64 * np.abs(logq[e] - logp[e]).reshape(B, S).mean(1)).all(), (tag, "kl", e)
    ratio = lambda err, b: float((err / b).max()) if err.size else 0.0
    return ratio(e_iw, b_iw), ratio(e_el, b_el[elbo_live]), ratio(e_ess, 32 * EPS64)


def reduce_cases():
    """B in {1, 5} x S in {1, 2, 63, 64, 65, 257} x T in {1, 20} x n_lat in {1, 2}, turning through spans NULL | given (some beyond [0, T]: clamped) |
    given with one empty; nll_ld = B*S + 5, lat_stride = B*S + 3 and out_ld = 4 + n_lat + 2 with sentinels behind what is used; lw around -300 +- 50"""
    g = np.random.RandomState(21)
    cases, i = [], 0
    for B in (1, 5):
        for S in (1, 2, 63, 64, 65, 257):
            for T in (1, 20):
                for n_lat in (1, 2):
                    rows = B * S
                    nll = (g.uniform(200, 300, (1, rows)) / T * g.uniform(0.5, 1.5, (T, rows))).astype(np.float32)
                    logp = -(100.0 + 10.0 * g.randn(n_lat, rows)) / n_lat
                    logq = -(75.0 + 10.0 * g.randn(n_lat, rows)) / n_lat
                    how = ("null", "given", "empty")[i % 3]
                    t0 = t1 = None
                    if how != "null":
                        t0, t1 = g.randint(-2, T // 2 + 1, B).astype(np.int32), g.randint(T // 2 + 1, T + 3, B).astype(np.int32)
                        if how == "empty":
                            t0[B // 2], t1[B // 2] = T // 2, T // 2
                    cases.append(dict(tag="B %d S %d T %d n_lat %d spans %s" % (B, S, T, n_lat, how), B=B, S=S, T=T, n_lat=n_lat, nll=nll, logp=logp, logq=logq,
                                      t0=t0, t1=t1, nll_ld=rows + 5, lat_stride=rows + 3, out_ld=4 + n_lat + 2))
                    i += 1
    return cases


def special_reduce_cases():
    """what has an exact answer: S = 1; equal weights; one -inf weight; all -inf"""
    g = np.random.RandomState(22)
    out = []
    for S in (1, 2, 64, 65, 257):
        B, T, rows = 3, 4, 3 * S
        nll = g.uniform(0.5, 1.5, (T, rows)).astype(np.float32)
        logp, logq = -100.0 + g.randn(2, rows), -75.0 + g.randn(2, rows)
        for kind in ("plain", "equal", "one -inf", "all -inf"):
            n, p, q = nll.copy(), logp.copy(), logq.copy()
            if kind == "equal":
                n[:], p[:], q[:] = n[:, :1], p[:, :1], q[:, :1]
            elif kind == "one -inf":
                p[0, ::S] = -np.inf          # sample 0 of every piece
            elif kind == "all -inf":
                p[1, S:2 * S] = -np.inf      # piece 1
            out.append(dict(tag="special S %d %s" % (S, kind), kind=kind, B=B, S=S, T=T, n_lat=2, nll=n, logp=p, logq=q, t0=None, t1=None, nll_ld=rows,
                            lat_stride=rows, out_ld=6))
    return out


def check_special(c, lw, out):
    S, kind = c["S"], c["kind"]
    L = lw.reshape(c["B"], S)
    if S == 1 and kind in ("plain", "equal"):
        assert np.array_equal(out[:, 0], L[:, 0]) and np.array_equal(out[:, 1], L[:, 0]) and (out[:, 2] == 1.0).all(), (c["tag"], out)
    if kind == "equal":
        assert (out[:, 2] == float(S)).all(), (c["tag"], out[:, 2])
    if kind == "one -inf":
        assert (L[:, 0] == -np.inf).all() and (out[:, 1] == -np.inf).all(), c["tag"]
        if S == 1:
            assert (out[:, 0] == -np.inf).all() and (out[:, 2] == 0.0).all(), c["tag"]
        else:          # the -inf weight contributes 0: the sums are those of the other S - 1 samples
            m = L[:, 1:].max(1)
            x = np.exp(L[:, 1:] - m[:, None])
            np.testing.assert_allclose(out[:, 0], m + np.log(x.sum(1)) - np.log(S), rtol=1e-13, err_msg=c["tag"])
            np.testing.assert_allclose(out[:, 2], x.sum(1) ** 2 / (x * x).sum(1), rtol=1e-13, err_msg=c["tag"])
    if kind == "all -inf":
        assert out[1, 0] == -np.inf and out[1, 1] == -np.inf and out[1, 2] == 0.0 and np.isfinite(out[[0, 2], :3]).all(), (c["tag"], out)


def widen64(x, ld, fill):
    """rows of x at a row stride of ld, `fill` between them; the last row ends with its data"""
    rows, D = x.shape
    buf = np.full(rows * ld, fill, x.dtype)
    buf.reshape(rows, ld)[:, :D] = x
    return buf[:(rows - 1) * ld + D]


def reduce_blob(c):
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    rows = c["B"] * c["S"]
    blob = i32(1, c["B"], c["S"], c["T"], c["nll_ld"], c["n_lat"], c["lat_stride"], c["out_ld"], 0 if c["t0"] is None else 1, 0)
    blob += widen64(c["nll"], c["nll_ld"], np.float32(np.nan)).tobytes()
    if c["t0"] is not None:
        blob += c["t0"].tobytes() + c["t1"].tobytes()
    return blob + widen64(c["logp"], c["lat_stride"], np.nan).tobytes() + widen64(c["logq"], c["lat_stride"], np.nan).tobytes()


def parse_reduce(c, raw):
    """out.bin of a reduce case -> (lw (B*S,), out (B, 4 + n_lat)); the columns behind 4 + n_lat must still hold the canary"""
    B, rows, cols = c["B"], c["B"] * c["S"], 4 + c["n_lat"]
    assert np.frombuffer(raw[:4], np.int32)[0] == 0, c["tag"]
    dd = np.frombuffer(raw[4:], np.float64)
    assert dd.size == rows + (B - 1) * c["out_ld"] + cols, c["tag"]
    full = np.concatenate([dd[rows:], np.full(B * c["out_ld"] - (dd.size - rows), float(CANARY))]).reshape(B, c["out_ld"])
    assert (full[:, cols:] == float(CANARY)).all(), c["tag"]
    return dd[:rows].copy(), full[:, :cols].copy()


# ------------------------------------------------------------------------------------------------------------------------------
# the conjugate Gaussian model: prior N(0, e^lv) per dimension (K = 1, mu_lk = 0), likelihood x | z ~ N(z, 1 / p1) with p1 = 1 - e^-lv, so that the
# posterior is N(p1 x, 1) and log p(x) = log N(x; 0, e^lv + 1 / p1)
# ------------------------------------------------------------------------------------------------------------------------------
def conjugate(B, Z, seed, shift=0.0):
    """-> dict(pre (B, 2Z) float32: the posterior mean (+ shift) | v = 0, mu_lk = 0, lv_lk (1, Z) in [0.3, 1.5], x, p1 (B, Z) / (Z,) float64,
    truth (B,): log p(x))"""
    g = np.random.RandomState(seed)
    lv = g.uniform(0.3, 1.5, (1, Z)).astype(np.float32)
    mu = g.randn(B, Z).astype(np.float32)
    p1 = 1.0 - np.exp(-lv[0].astype(np.float64))
    x = mu.astype(np.float64) / p1
    var = np.exp(lv[0].astype(np.float64)) + 1.0 / p1
    truth = (-0.5 * (x * x / var + np.log(var) + LOG_2PI)).sum(1)
    pre = np.concatenate([(mu.astype(np.float64) + shift).astype(np.float32), np.zeros((B, Z), np.float32)], axis=1)
    return dict(pre=pre, mu_lk=np.zeros((1, Z), np.float32), lv_lk=lv, x=x, p1=p1, truth=truth)


def conjugate_nll(m, z, S):
    """-log N(x; z, 1 / p1) summed over the dimensions, at the stored z (B*S, Z) -> (nll64 (B*S,), nll (3, B*S) float32: three floats per row whose
    float64 sum, added ascending from 0.0, is nll64 exactly - so the fp32 nll rows of the entry point carry the float64 value)"""
    x = np.repeat(m["x"], S, axis=0)
    dz = x - z.astype(np.float64)
    v = (0.5 * (dz * dz * m["p1"] - np.log(m["p1"]) + LOG_2PI)).sum(1)
    hi = v.astype(np.float32)
    lo = (v - hi.astype(np.float64)).astype(np.float32)
    lo2 = (v - hi.astype(np.float64) - lo.astype(np.float64)).astype(np.float32)
    parts = np.stack([hi, lo, lo2], 0)
    assert np.array_equal(parts[0].astype(np.float64) + parts[1].astype(np.float64) + parts[2].astype(np.float64), v)
    return v, parts


def check_identity(m, S, logq, logp, lw, out, nll64, tag=""):
    """q is the true posterior: every lw[b, s] is log p(x) within 64 * 2^-52 (|recon| + |logp| + |logq|), ess == S to 1e-9 relative and iwae == elbo
    within the same bound -> the largest error / bound ratio"""
    B = m["truth"].size
    bound = 64 * EPS64 * (np.abs(nll64) + np.abs(logp) + np.abs(logq))
    err = np.abs(lw - np.repeat(m["truth"], S))
    assert (err <= bound).all(), (tag, float((err / bound).max()))
    assert (np.abs(out[:, 2] / S - 1.0) <= 1e-9).all(), (tag, out[:, 2])
    assert (np.abs(out[:, 0] - out[:, 1]) <= bound.reshape(B, S).max(1) + EPS64 * (16 + 2 * np.abs(out[:, 0]))).all(), (tag, out[:, :2])
    return float((err / bound).max())


def check_mismatch(m, S, out, tag=""):
    """the conditions on the mismatched proposal (tau 1.5, the mean shifted by 0.3, Z 8, S 4096)"""
    iwae, elbo, ess, truth = out[:, 0], out[:, 1], out[:, 2], m["truth"]
    unit = np.sqrt((S / ess - 1.0) / S)
    assert (np.abs(iwae - truth) <= 6 * unit).all(), (tag, "iwae", (np.abs(iwae - truth) / unit).tolist())
    assert (ess >= S / 8).all() and (truth - elbo >= 1).all() and (iwae >= elbo).all(), (tag, (ess / S).tolist(), (truth - elbo).tolist())
    return float((np.abs(iwae - truth) / unit).max()), float((ess / S).min()), float((truth - elbo).min())


# ------------------------------------------------------------------------------------------------------------------------------
# stand-in ops
# ------------------------------------------------------------------------------------------------------------------------------
def lik_fake_ops():
    """the report stand-ins + fn_posterior_draw / fn_iw_reduce as their restatement (z rounded to float32); `seen` records, per gru_seq_fwd call, the
    tag of its first scan, the number of scans and their row count"""
    base = type(hr.report_fake_ops())

    class LikFakeOps(base):
        def __init__(self):
            super().__init__()
            self.seen = []

        def gru_seq_fwd(self, scans, *a, **k):
            self.seen.append((scans[0].get("tag"), len(scans), int(scans[0]["B"])))
            return super().gru_seq_fwd(scans, *a, **k)

        def posterior_draw(self, jobs, S, params):
            self.calls.append("posterior_draw")
            raw = params.numpy().view(hl.PARAMS_DTYPE)[0]
            for j in jobs:
                pre, mu_lk, lv_lk = j["pre"].numpy(), j["mu_lk"].numpy(), j["lv_lk"].numpy()
                ref = post_ref(pre, S, j["stream_id"], int(raw["seed"]), int(raw["offset"]), float(raw["tau"]))
                z = ref["z"].astype(np.float32)
                lq, lp, _, _ = densities(z, pre, sg_of(pre, float(raw["tau"])), mu_lk, lv_lk, S)
                j["z"].copy_(torch.from_numpy(z))
                j["logq"].copy_(torch.from_numpy(lq)), j["logp"].copy_(torch.from_numpy(lp))
                if j.get("eps_out") is not None:
                    j["eps_out"].copy_(torch.from_numpy(ref["eps"].astype(np.float32)))

        def iw_reduce(self, nll, B, S, logp, logq, lw, out, t0=None, t1=None):
            self.calls.append("iw_reduce")
            rl, ro = iw_ref(nll.numpy(), B, S, logp.numpy(), logq.numpy(), None if t0 is None else t0.numpy(), None if t1 is None else t1.numpy())
            lw.copy_(torch.from_numpy(rl)), out.copy_(torch.from_numpy(ro))

    return LikFakeOps()
