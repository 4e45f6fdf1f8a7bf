"""Checking tools of the prior draw and the latent mix (latent.py, fn_latent_draw / fn_latent_mix):

  draw_ref / mix_ref   the two definitions of include/fadernets.h restated in float64 numpy (the Philox rounds in uint64: helpers_sampling's)
  check_draw / check_mix   a result against the restatement, within bounds that follow from the precision of the fp32 steps (stated where they are checked)
  draw_cases / mix_cases   the case lists the host twin and the device are put through, with the blobs of the stand-alone program
  latent_fake_ops      helpers_stitch.stitch_fake_ops() + the two entry points as their restatement: latent.py on the CPU
"""
import numpy as np
import torch

import helpers_stitch as hs
from helpers_sampling import philox4x32_10

LERP, SLERP, STEP = 0, 1, 2
MIN_SIN = 1e-4                    # FN_MIX_MIN_SIN
CANARY = np.float32(-777.25)
PARAMS_DTYPE = [("seed", "<u8"), ("offset", "<u8"), ("tau", "<f4"), ("reserved", "<i4", (3,))]      # FnDrawParams
ULP = 2.0 ** -23
FLT_MAX = float(np.finfo(np.float32).max)


def params_bytes(seed=0, offset=0, tau=1.0):
    raw = np.zeros(1, dtype=PARAMS_DTYPE)
    raw["seed"], raw["offset"], raw["tau"] = seed, offset, np.float32(tau)
    return raw.view(np.uint8).copy()


def clamp_tau(tau):
    tau = np.float32(tau)
    return 1.0 if np.isnan(tau) else float(min(max(float(tau), 0.0), FLT_MAX))


def _words(rows, second, seed, offset):
    """Philox words of counters (b, second[...], offset_lo, offset_hi) under the key seed: (rows, len(second), 4) uint32"""
    b = np.arange(rows, dtype=np.uint64).reshape(-1, 1)
    ctr = np.stack(np.broadcast_arrays(b, np.asarray(second, dtype=np.uint64).reshape(1, -1), np.uint64(offset & 0xffffffff), np.uint64(offset >> 32)), axis=-1)
    return philox4x32_10(ctr, np.array([seed & 0xffffffff, seed >> 32], dtype=np.uint64))


def sincospi(x):
    """sin(pi x), cos(pi x) for x in [0, 2), cut at the nearest multiple of 1/2 so that the zeros are exact"""
    k = np.floor(2.0 * x + 0.5).astype(np.int64)
    y = np.pi * (x - 0.5 * k)
    sy, cy = np.sin(y), np.cos(y)
    k &= 3
    return np.choose(k, [sy, cy, -sy, -cy]), np.choose(k, [cy, -sy, -cy, sy])


def draw_normals(rows, Z, stream_id, seed=0, offset=0):
    """steps 1 and 2 -> (n (rows, Z) float64, r (rows, Z) float64: the radius behind every normal)"""
    nq = (Z + 3) // 4
    w = _words(rows, (stream_id << 16) | np.arange(nq), seed, offset).astype(np.uint64)
    ua = ((w[..., 0::2] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    ub = (w[..., 1::2] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(ua))
    s, c = sincospi(2.0 * ub)
    n = np.stack([r * c, r * s], axis=-1).reshape(rows, 4 * nq)[:, :Z]
    return n, np.repeat(r, 2, axis=-1).reshape(rows, 4 * nq)[:, :Z]


def draw_components(rows, K, stream_id, seed=0, offset=0, comp=None):
    """step 3 -> (rows,) int32"""
    w0 = _words(rows, [(stream_id << 16) | 0xFFFF], seed, offset)[:, 0, 0].astype(np.uint64)
    k = (((w0 >> np.uint64(8)) * np.uint64(K)) >> np.uint64(24)).astype(np.int64)
    if comp is not None:
        comp = np.asarray(comp, dtype=np.int64)
        k = np.where(comp >= 0, comp, k)
    return np.minimum(k, K - 1).astype(np.int32)


def draw_ref(mu_lk, lv_lk, rows, stream_id, seed=0, offset=0, tau=1.0, comp=None, normals=None):
    """one job -> dict(z, eps, r, sigma (rows, Z) float64, mu (rows, Z), comp (rows,) int32, tau).  normals: (n, r) of draw_normals for at least
    these rows, to share them among cases"""
    K, Z = mu_lk.shape
    n, r = draw_normals(rows, Z, stream_id, seed, offset) if normals is None else (normals[0][:rows], normals[1][:rows])
    k = draw_components(rows, K, stream_id, seed, offset, comp)
    t = clamp_tau(tau)
    mu, sigma = mu_lk.astype(np.float64)[k], np.exp(0.5 * lv_lk.astype(np.float64)[k])
    return dict(z=mu + (t * sigma) * n, eps=n, r=r, sigma=sigma, mu=mu, comp=k, tau=t)


def check_draw(ref, z, eps=None, comp=None, tag=""):
    """components exact, |eps - eps64| <= 8 ulp (1 + r), |z - z64| <= 16 ulp (|mu| + tau sigma (1 + r)), ulp = 2^-23: logf, sqrtf, sincospif and expf
    each err by at most 2 ulp and r <= 5.77, so four of them in a row stay inside 8 ulp of the values they scale, and z adds one more chain of the
    same length -> the largest error / bound ratios (eps, z)"""
    if comp is not None:
        assert np.array_equal(comp, ref["comp"]), tag
    worst = [0.0, 0.0]
    if eps is not None:
        bound = 8 * ULP * (1 + ref["r"])
        err = np.abs(eps.astype(np.float64) - ref["eps"])
        assert (err <= bound).all(), (tag, float((err / bound).max()))
        worst[0] = float((err / bound).max())
    bound = 16 * ULP * (np.abs(ref["mu"]) + ref["tau"] * ref["sigma"] * (1 + ref["r"]))
    err = np.abs(z.astype(np.float64) - ref["z"])
    assert (err <= bound).all() and np.isfinite(z).all(), (tag, float(err.max()))
    worst[1] = float((err / np.maximum(bound, 1e-300)).max())
    return worst


def stats_ok(n0, n1):
    """5-sigma bounds on two streams of N normals each: |mean| <= 5 / sqrt(N), |var - 1| <= 5 sqrt(2 / N), |m4 - 3| <= 5 sqrt(96 / N) (m4 the mean of
    n^4), |corr| <= 5 / sqrt(N).  The draws are fixed by the seed, so the checks are deterministic -> the figures"""
    out = []
    for n in (n0, n1):
        n = n.astype(np.float64).ravel()
        N = n.size
        mean, var, m4 = n.mean(), n.var(), (n ** 4).mean()          # Var(n^2) = 2 and Var(n^4) = 105 - 9 = 96 are the bounds' sigmas
        assert abs(mean) <= 5 / np.sqrt(N) and abs(var - 1) <= 5 * np.sqrt(2 / N) and abs(m4 - 3) <= 5 * np.sqrt(96 / N), (mean, var, m4)
        out.append((mean, var, m4))
    corr = np.corrcoef(n0.astype(np.float64).ravel(), n1.astype(np.float64).ravel())[0, 1]
    assert abs(corr) <= 5 / np.sqrt(n0.size), corr
    return out, corr


def counts_ok(comp, K):
    rows = comp.size
    cnt = np.bincount(comp, minlength=K)
    assert cnt.size == K and (np.abs(cnt - rows / K) <= 5 * np.sqrt(rows * (1 / K) * (1 - 1 / K))).all(), (K, cnt)
    return cnt


# ------------------------------------------------------------------------------------------------------------------------------
# the mix
# ------------------------------------------------------------------------------------------------------------------------------
def mix_ref(a, b, t, segs, per_pair=False):
    """a, b (pairs, D), t (P,) or (pairs, P), segs [(off, len, mode)] -> (out (pairs*P, D) float64, omega (pairs, n_segs) float64: the fp64 angle of a
    SLERP segment (-1 where the fallback is taken), 0 of the others)"""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    pairs, D = a.shape
    tt = np.asarray(t, dtype=np.float32).astype(np.float64)
    tt = tt if per_pair else np.broadcast_to(tt.reshape(1, -1), (pairs, tt.size))
    P = tt.shape[1]
    out = np.repeat(a64, P, axis=0).reshape(pairs, P, D)
    omega = np.zeros((pairs, len(segs)))
    t3 = tt.reshape(pairs, P, 1)
    for g, (off, n, mode) in enumerate(segs):
        x, y = a64[:, None, off:off + n], b64[:, None, off:off + n]
        lerp = t3 * y + (1.0 - t3) * x
        if mode == STEP:
            out[:, :, off:off + n] = np.where(t3 < 0.5, x, y)
        elif mode == LERP:
            out[:, :, off:off + n] = lerp
        else:
            na, nb = np.sqrt((x * x).sum(-1)), np.sqrt((y * y).sum(-1))                  # (pairs, 1)
            with np.errstate(invalid="ignore", divide="ignore"):
                c = np.clip((x * y).sum(-1) / (na * nb), -1.0, 1.0)
                om = np.arccos(c)
                s = np.sin(om)
                fall = (na == 0) | (nb == 0) | ~(s >= MIN_SIN)
                s3, om3 = s[:, :, None], om[:, :, None]
                sl = (np.sin((1.0 - t3) * om3) / s3) * x + (np.sin(t3 * om3) / s3) * y
            out[:, :, off:off + n] = np.where(fall[:, :, None], lerp, sl)
            omega[:, g] = np.where(fall[:, 0], -1.0, om[:, 0])
    return out.reshape(pairs * P, D), omega


MIX_TOL = 2e-5                                     # |out - out64| <= MIX_TOL (|a_j| + |b_j|) on inputs with |c| <= 0.9
OMEGA_TOL = 2e-5 / np.sqrt(1 - 0.81)


def check_mix(a, b, t, segs, out, omega=None, per_pair=False, tag=""):
    """-> the largest |out - out64| / (|a_j| + |b_j|)"""
    ref, om = mix_ref(a, b, t, segs, per_pair)
    P = ref.shape[0] // a.shape[0]
    scale = np.repeat(np.abs(a.astype(np.float64)) + np.abs(b.astype(np.float64)), P, axis=0)
    err = np.abs(out.astype(np.float64) - ref)
    assert (err <= MIX_TOL * scale).all(), (tag, float(err.max()))
    if omega is not None:
        assert np.array_equal(omega == -1, om == -1) and (np.abs(omega - om) <= OMEGA_TOL).all(), (tag, omega, om)
    return float((err / np.maximum(scale, 1e-30)).max())


def pair_with_cosine(g, pairs, n, lo=-0.9, hi=0.9):
    """(a, b) float32 (pairs, n) whose cosines lie in [lo, hi] (n >= 2; drawn, then rejected)"""
    a, b = g.randn(pairs, n).astype(np.float32), g.randn(pairs, n).astype(np.float32)
    for i in range(pairs):
        while True:
            c = float(a[i].astype(np.float64) @ b[i].astype(np.float64)) / float(np.linalg.norm(a[i].astype(np.float64)) * np.linalg.norm(b[i].astype(np.float64)))
            if lo <= c <= hi:
                break
            b[i] = g.randn(n).astype(np.float32)
    return a, b


T_VALUES = {1: [0.3], 2: [0.0, 1.0], 9: [-0.5, 0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0, 1.5]}


def std_segs(Z, mode=SLERP):
    return [(0, Z, mode), (Z, Z, mode), (2 * Z, 24, STEP)]


def mix_cases():
    """pairs in {1, 2, 65} x P in {1, 2, 9} x (D = 2Z+24 with Z in {4, 128} and the three standard segments in both modes | D = 5 with one segment) x
    t_per_pair, in wider rows (ab_ld = D + 3, out_ld = D + 5) for half of them"""
    g = np.random.RandomState(77)
    cases = []
    for pairs in (1, 2, 65):
        for P in (1, 2, 9):
            for shape in ("z4", "z128", "d5"):
                for per_pair in (False, True):
                    if shape == "d5":
                        D, segs = 5, [(1, 3, SLERP if (pairs + P) % 2 else LERP)]
                        a, b = np.zeros((pairs, 5), np.float32), np.zeros((pairs, 5), np.float32)
                        a[:, 1:4], b[:, 1:4] = pair_with_cosine(g, pairs, 3)
                        a[:, [0, 4]], b[:, [0, 4]] = g.randn(pairs, 2), g.randn(pairs, 2)
                    else:
                        Z = 4 if shape == "z4" else 128
                        D, segs = 2 * Z + 24, std_segs(Z, SLERP if per_pair or P != 2 else LERP)
                        parts = [pair_with_cosine(g, pairs, Z), pair_with_cosine(g, pairs, Z), (g.rand(pairs, 24).astype(np.float32), g.rand(pairs, 24).astype(np.float32))]
                        a, b = (np.concatenate([p[k] for p in parts], axis=1) for k in (0, 1))
                    t = np.array(T_VALUES[P], np.float32)
                    if per_pair:
                        t = (t.reshape(1, P) + 0.01 * np.arange(pairs).reshape(pairs, 1)).astype(np.float32)
                    wide = (pairs + P + len(shape)) % 2 == 0
                    cases.append(dict(tag="pairs %d P %d %s per_pair %d wide %d" % (pairs, P, shape, per_pair, wide), a=a, b=b, t=t, segs=segs, per_pair=per_pair,
                                      ab_ld=D + 3 if wide else D, out_ld=D + 5 if wide else D))
    return cases


def widen(x, ld):
    """rows of x at a row stride of ld, canaries between them; the last row ends with its data"""
    rows, D = x.shape
    buf = np.full(rows * ld, CANARY, np.float32)
    buf.reshape(rows, ld)[:, :D] = x
    return buf[:(rows - 1) * ld + D]


def narrow(buf, rows, D, ld, tag=""):
    """the (rows, D) data of a buffer laid out by widen; asserts that everything between the rows still is the canary"""
    full = np.concatenate([buf, np.full(rows * ld - buf.size, CANARY, np.float32)]).reshape(rows, ld)
    assert (full[:, D:] == CANARY).all(), tag
    return full[:, :D]


def exact_mix_checks(run):
    """the exact cases of the mix, on whatever `run(a, b, t, segs, per_pair, ab_ld, out_ld) -> (out, omega)` drives"""
    g = np.random.RandomState(9)
    for n in (1, 5, 64, 130):
        a, b = g.randn(3, n).astype(np.float32), g.randn(3, n).astype(np.float32)
        for mode in (LERP, SLERP, STEP):
            out, _ = run(a, b, [0.0, 1.0], [(0, n, mode)])
            assert np.array_equal(out[0::2], a) and np.array_equal(out[1::2], b), (n, mode)          # t = 0 is a, t = 1 is b, exactly
        # STEP flips exactly at 0.5
        out, om = run(a, b, [np.nextafter(np.float32(0.5), np.float32(0)), 0.5], [(0, n, STEP)])
        assert np.array_equal(out[0::2], a) and np.array_equal(out[1::2], b) and (om == 0).all()
        # a == b, a == -b and a zero vector take the LERP fallback
        t = [-0.5, 0.0, 0.25, 1.0, 1.5]
        for bb in (a, -a, np.zeros_like(a)):
            for x, y in ((a, bb), (bb, a)):
                out, om = run(x, y, t, [(0, n, SLERP)])
                assert (om == -1).all(), (n, om)
                want = np.stack([np.float32(tt) * y.astype(np.float64) + (1.0 - np.float32(tt)) * x.astype(np.float64) for tt in t], axis=1).reshape(-1, n)
                assert (np.abs(out - want) <= MIX_TOL * np.repeat(np.abs(x) + np.abs(y), len(t), axis=0)).all(), n
                assert np.array_equal(out[1::5], x) and np.array_equal(out[3::5], y)
    # columns in no segment are a's; columns beyond D in wider rows keep their canary (narrow() looks); segments in any order
    a, b = g.randn(5, 12).astype(np.float32), g.randn(5, 12).astype(np.float32)
    a[:, 8:11], b[:, 8:11] = pair_with_cosine(g, 5, 3)
    segs = [(8, 3, SLERP), (1, 2, STEP), (4, 3, LERP)]
    out, om = run(a, b, [0.75], segs, False, 15, 17)
    assert np.array_equal(out[:, [0, 3, 7, 11]], a[:, [0, 3, 7, 11]]) and np.array_equal(out[:, 1:3], b[:, 1:3]) and (om[:, 1:] == 0).all() and (om[:, 0] > 0).all()
    check_mix(a, b, [0.75], segs, out, om)


def set_apart(m, sigmas=3.0):
    """the two components of both lookups `sigmas` standard deviations apart"""
    for e in "rn":
        mu, lv = getattr(m, "mu_%s_lookup" % e).weight.data, getattr(m, "logvar_%s_lookup" % e).weight.data
        Z = mu.shape[1]
        mu[1] = mu[0] + sigmas * torch.exp(0.5 * lv[0]) / np.sqrt(Z)
    m.weights_changed()
    return m


# ------------------------------------------------------------------------------------------------------------------------------
# the draw's cases
# ------------------------------------------------------------------------------------------------------------------------------
def lookups(g, K, Z):
    return g.randn(K, Z).astype(np.float32), (-4.0 + g.rand(K, Z)).astype(np.float32)


def draw_cases(rows_set=(1, 3, 65), Z_set=(1, 5, 64, 130), K_set=(1, 2, 8), jobs_set=None, vary=True):
    """rows x Z x K, turning through: one job at z_ld = Z | two jobs at z_ld = 2Z+24, the second at column Z | four jobs at z_ld = 4Z+3; components
    drawn | given | given with -1 holes and entries beyond K; tau 1 | 0.5 | 0 | NaN; seeds and offsets up to 64 bits.  jobs_set: every one of these
    job counts for every shape instead of turning through them; vary=False: one seed and offset for all cases (shared reference normals)"""
    g = np.random.RandomState(5)
    cases, i = [], 0
    for rows in rows_set:
        for Z in Z_set:
            for K in K_set:
                for n_jobs in jobs_set or [(1, 2, 4)[i % 3]]:
                    z_ld = {1: Z, 2: 2 * Z + 24, 4: 4 * Z + 3}[n_jobs]
                    how = ("drawn", "given", "holes")[(i // 3) % 3]
                    jobs = []
                    for s in range(n_jobs):
                        mu, lv = lookups(g, K, Z)
                        comp = None if how == "drawn" else g.randint(0, K, rows).astype(np.int32)
                        if how == "holes":
                            comp[::2] = -1
                            comp[rows // 2] = K + 3
                        jobs.append(dict(mu_lk=mu, lv_lk=lv, comp=comp, stream_id=(0, 1, 7, 65534)[s]))
                    cases.append(dict(tag="rows %d Z %d K %d jobs %d %s" % (rows, Z, K, n_jobs, how), rows=rows, Z=Z, z_ld=z_ld, col_step=Z if n_jobs > 1 else 0,
                                      jobs=jobs, tau=(1.0, 0.5, 0.0, float("nan"))[i % 4], seed=(2024, 7, (1 << 64) - 1, 1 << 40)[i % 4] if vary else 2024,
                                      offset=(0, 3, 1 << 33, (1 << 64) - 1)[(i // 2) % 4] if vary else 3))
                    i += 1
    return cases


def check_draw_case(c, z, eps, comp_out, normals=None):
    """z: the whole buffer [(rows-1)*z_ld + (n_jobs-1)*col_step + Z]; eps, comp_out: per job or None -> worst ratios"""
    rows, Z, z_ld = c["rows"], c["Z"], c["z_ld"]
    full = np.concatenate([z, np.full(rows * z_ld - z.size, CANARY, np.float32)]).reshape(rows, z_ld)
    used = np.zeros(z_ld, bool)
    worst = [0.0, 0.0]
    for s, j in enumerate(c["jobs"]):
        ref = draw_ref(j["mu_lk"], j["lv_lk"], rows, j["stream_id"], c["seed"], c["offset"], c["tau"], j["comp"],
                       None if normals is None else normals(Z, j["stream_id"], c["seed"], c["offset"]))
        col = s * c["col_step"]
        used[col:col + Z] = True
        w = check_draw(ref, full[:, col:col + Z], None if eps is None else eps[s], None if comp_out is None else comp_out[s], c["tag"])
        worst = [max(x, y) for x, y in zip(worst, w)]
        if clamp_tau(c["tau"]) == 0.0:
            assert np.array_equal(full[:, col:col + Z], j["mu_lk"][ref["comp"]]), c["tag"]          # tau = 0: the component means themselves
    assert (full[:, ~used] == CANARY).all(), c["tag"]
    return worst


def draw_blob(c, flags=7):
    """the in.bin of latent_ops_check.cpp for a draw case"""
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    blob = i32(0, len(c["jobs"]), c["rows"], c["Z"], c["z_ld"], c["col_step"], flags if c["jobs"][0]["comp"] is not None else flags & ~1, 0)
    blob += params_bytes(c["seed"], c["offset"], c["tau"]).tobytes()
    for j in c["jobs"]:
        blob += i32(j["mu_lk"].shape[0], j["stream_id"]) + j["mu_lk"].tobytes() + j["lv_lk"].tobytes()
        if j["comp"] is not None and flags & 1:
            blob += j["comp"].tobytes()
    return blob


def parse_draw(c, raw):
    """out.bin of a draw case (flags 7) -> (z buffer, [eps per job], [comp_out per job])"""
    rows, Z, n = c["rows"], c["Z"], len(c["jobs"])
    assert np.frombuffer(raw[:4], np.int32)[0] == 0, c["tag"]
    nz = (rows - 1) * c["z_ld"] + (n - 1) * c["col_step"] + Z
    assert len(raw) == 4 + 4 * (nz + n * rows * Z + n * rows), c["tag"]
    f = np.frombuffer(raw[4:4 + 4 * (nz + n * rows * Z)], np.float32)
    comp = np.frombuffer(raw[4 + 4 * (nz + n * rows * Z):], np.int32)
    return f[:nz], [f[nz + s * rows * Z:nz + (s + 1) * rows * Z].reshape(rows, Z) for s in range(n)], [comp[s * rows:(s + 1) * rows] for s in range(n)]


def mix_blob(c):
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    pairs, D = c["a"].shape
    P = c["t"].shape[-1]
    segs = b"".join(i32(off, n, mode, 0) for off, n, mode in c["segs"])
    return i32(1, pairs, D, c["ab_ld"], P, int(c["per_pair"]), len(c["segs"]), c["out_ld"]) + segs + widen(c["a"], c["ab_ld"]).tobytes() + widen(
        c["b"], c["ab_ld"]).tobytes() + np.ascontiguousarray(c["t"], np.float32).tobytes()


def parse_mix(c, raw):
    pairs, D = c["a"].shape
    P = c["t"].shape[-1]
    assert np.frombuffer(raw[:4], np.int32)[0] == 0, c["tag"]
    f = np.frombuffer(raw[4:], np.float32)
    n_out = (pairs * P - 1) * c["out_ld"] + D
    assert f.size == n_out + pairs * len(c["segs"]), c["tag"]
    return narrow(f[:n_out], pairs * P, D, c["out_ld"], c["tag"]), f[n_out:].reshape(pairs, len(c["segs"]))


# ------------------------------------------------------------------------------------------------------------------------------
# stand-in ops
# ------------------------------------------------------------------------------------------------------------------------------
def latent_fake_ops():
    """the decode / notes / stitch stand-ins + fn_latent_draw / fn_latent_mix as their restatement, rounded to float32"""
    base = type(hs.stitch_fake_ops())

    class LatentFakeOps(base):
        def latent_draw(self, jobs, params):
            self.calls.append("latent_draw")
            raw = params.numpy().view(PARAMS_DTYPE)[0]
            for j in jobs:
                rows = j["z"].shape[0]
                ref = draw_ref(j["mu_lk"].numpy(), j["lv_lk"].numpy(), rows, j["stream_id"], int(raw["seed"]), int(raw["offset"]), float(raw["tau"]),
                               None if j.get("comp") is None else j["comp"].numpy())
                j["z"].copy_(torch.from_numpy(ref["z"].astype(np.float32)))
                if j.get("eps_out") is not None:
                    j["eps_out"].copy_(torch.from_numpy(ref["eps"].astype(np.float32)))
                if j.get("comp_out") is not None:
                    j["comp_out"].copy_(torch.from_numpy(ref["comp"]))

        def latent_mix(self, a, b, t, segs, out, omega_out=None, per_pair=False):
            self.calls.append("latent_mix")
            ref, om = mix_ref(a.numpy(), b.numpy(), t.numpy(), segs, per_pair)
            out.copy_(torch.from_numpy(ref.astype(np.float32)))
            if omega_out is not None:
                omega_out.copy_(torch.from_numpy(om.astype(np.float32)))

    return LatentFakeOps()
