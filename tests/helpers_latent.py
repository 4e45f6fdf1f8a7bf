"""Shared code of tests/test_latent_reference.py (CPU) and tests/test_gpu_latent.py (MI355X): the latent block of csrc/loss.hip - fn_latent_fwd and
fn_latent_bwd - against float64.  No GPU import: every driver takes the backend (`ops`: HipOps on the GPU, FakeOps or LatentStepOps on the CPU) and
the device as arguments.  Layout, metric and the power-of-two bound follow tests/helpers_loss.py.

References.  latent_fwd_math is the documented forward with the reference model's quirks as include/fadernets.h and kl_dim state them: exp(logvar) is
the VARIANCE in the likelihood and the STANDARD DEVIATION in the KL, the prior log(1/K) is part of ll, terms = {sum_k q KLmean_k, mean_k(q log q),
KLmean_label, -log softmax(q)[label]}.  latent_bwd_math is the documented backward formula as a function of ALL the inputs fn_latent_bwd gets, the
float32 `z` and `qy` included: q_k (dq_k - sum_j q_j dq_j) cancels against sum q = 1, which a float32 qy meets to one ulp only, while dq carries KL
means of about 1e3 - a float64 gradient that recomputes the posterior from `pre` differs from the formula on the given qy by up to 2e-5 of a tile
maximum near saturation (tests/test_latent_reference.py puts the figure on record, and shows once that the formula on the unrounded float64 z / qy IS
autograd of the documented loss).  Both run in float64 on the float32 inputs (the reference) and, the same lines, in float32 (the restatement);
LatentStepOps wraps the float32 lines in the signatures of HipOps, so that the restatement - and a planted fault in it - runs through the drivers.

Metric (helpers_head.tile_errors / worst_ratio): per tile of 16 rows x tc columns  err = max |got - ref64| / max |ref64|  and
err <= F x max(e_ref, 2**-23), e_ref = err of the float32 restatement in that tile.  tc = 16 for sigma, z, dpre [B][2Z] and dmu_lk_rows [B][K Z], K
for ll and qy, 1 for each column of terms.  F = LATENT_F[family] <= helpers.SCAN_F_CAP, families fwd_sample (sigma, z), fwd_posterior (ll, qy),
fwd_terms, bwd_dpre, bwd_dmu.  No tile is exempt.

Input conditions (latent_condition, asserted on the CPU; the seed of a case is the first draw that meets them).  live: every row has max_k qy <= 0.9,
min_k qy >= 1e-7 and a top-two gap >= 1e-4 in float64 - y is decided and must be the reference's argmax in every row.  twin: the same, the gap taken
between distinct values.  saturated (lv = -4): every row's second-largest qy is below 2**-150 - the kernel's float32 qy must be exactly 1 and 0.
init (lv = -4, mu_lk = 0.2 randn as in test_gpu_parity.test_latent_kernels): rows may be half-saturated.  Every tile maximum of the float64 reference
is >= SCAN_MIN_REF, except where the operation itself makes entries exactly zero: those entries are declared from the launch's form alone
(fwd_exact0 / bwd_exact0), asserted to be exactly zero in the float64 reference, and must be exactly 0.0 in the output; a quantity declared `tiny`
(the entropy column of terms in the saturated case only) is asserted to be below SCAN_MIN_REF in the reference and must be below it in the output.

Layout.  Outputs are views of buffers filled with the sentinel (3 rows beyond B, y with the integer sentinel); rows >= B stay untouched; inputs are
not modified."""
import math

import numpy as np
import torch

from helpers import SCAN_F_CAP, SCAN_MIN_REF
from helpers_head import tile_errors, worst_ratio
from helpers_loss import (E_NULL, E_SHAPE, F32, F64, INT_SENTINEL, PAD_ROWS, SENTINEL, _buf, _gen, assert_F, bits_equal, check_sentinel, f32,
                          old_metric_accepts)

LOG_2PI = math.log(2.0 * math.pi)
FAMILIES = ("fwd_sample", "fwd_posterior", "fwd_terms", "bwd_dpre", "bwd_dmu")
FAMILY = dict(sigma="fwd_sample", z="fwd_sample", ll="fwd_posterior", qy="fwd_posterior", t0="fwd_terms", t1="fwd_terms", t2="fwd_terms", t3="fwd_terms",
              dpre="bwd_dpre", dmu="bwd_dmu")
# F per family: the smallest power of two that is at least 1.5 x the worst ratio measured on an MI355X (profiles/latent_fp64_errors.txt: 0.758, 0.551,
# 0.957, 4.565, 1.806), never above SCAN_F_CAP; 1.5 for the reason helpers_loss.LOSS_F gives (e_ref is formed by torch on the CPU that runs the test).
# fwd_posterior is below 1: the kernel sums ll in double, the restatement in float32.
LATENT_F = dict(fwd_sample=2, fwd_posterior=1, fwd_terms=2, bwd_dpre=8, bwd_dmu=4)
CAP_F = {k: SCAN_F_CAP for k in FAMILIES}
LIVE_QMAX, LIVE_QMIN, LIVE_GAP, SAT_SECOND = 0.9, 1e-7, 1e-4, 2.0 ** -150
# mu_lk = randn LIVE_SCALE / sqrt(Z) e^c: the log-likelihood gap between two components is sum_d (m1 - m0)(2 z - m0 - m1) e^-c / 2, with a standard
# deviation of about 1.6 LIVE_SCALE whatever Z and c are.  (randn 1.2 / sqrt(Z) e^(c/2) gives 1.9 e^(-c/2): no draw of 21 rows stays below 0.9 at c = -2.)
LIVE_SCALE = 0.4
UPS = ("g_z", "g_mu", "g_sigma", "g_ll", "g_qy")
BWD_W3 = (0.3, 0.2, 0.7)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# references in float64 and the same lines in float32
# ---------------------------------------------------------------------------------------------------------------------------------------------
def latent_core(pre, eps, mu_lk, lv_lk, fault=None):
    """the documented forward on tensors of one dtype (differentiable): dict(mu, s, z, ll [B][K], logq, q, klm [B][K]).  mu_lk [K][Z], or [B][K][Z]
    (a copy per row, for per-row gradients).  faults: kl_var | ll_std | no_prior | drop_last_dim"""
    Z, K = eps.shape[1], lv_lk.shape[0]
    mu, s = pre[:, :Z], torch.exp(pre[:, Z:])
    z = mu + s * eps
    m, lv = (mu_lk if mu_lk.dim() == 3 else mu_lk.unsqueeze(0)), lv_lk.unsqueeze(0)
    dzm = z.unsqueeze(1) - m
    if fault == "ll_std":
        per = -0.5 * (dzm * dzm * torch.exp(-2.0 * lv) + 2.0 * lv + LOG_2PI)
    else:
        per = -0.5 * (dzm * dzm * torch.exp(-lv) + lv + LOG_2PI)              # likelihood: exp(logvar) is the variance
    sp = torch.exp(0.5 * lv) if fault == "kl_var" else torch.exp(lv)          # KL: exp(logvar) is the standard deviation
    vr = (s.unsqueeze(1) / sp) ** 2
    t1 = ((mu.unsqueeze(1) - m) / sp) ** 2
    kl = 0.5 * (vr + t1 - 1.0 - torch.log(vr))
    if fault == "drop_last_dim":
        per, kl = per[..., :Z - 1], kl[..., :Z - 1]
    ll = per.sum(-1) + (0.0 if fault == "no_prior" else math.log(1.0 / K))
    klm = kl.sum(-1) / Z
    mx = ll.amax(1, keepdim=True)
    logq = ll - (mx + torch.log(torch.exp(ll - mx).sum(1, keepdim=True)))
    return dict(mu=mu, s=s, z=z, ll=ll, logq=logq, q=torch.exp(logq), klm=klm)


def latent_terms(c, labels, fault=None):
    """terms [B][4] of a latent_core result (differentiable); faults: ent_sum | clf_logq"""
    q, K = c["q"], c["q"].shape[1]
    t0 = (q * c["klm"]).sum(1)
    t1 = (q * c["logq"]).sum(1) / (1 if fault == "ent_sum" else K)
    t2 = t3 = torch.zeros_like(t0)
    if labels is not None:
        lb = labels.detach().cpu().long().view(-1, 1)
        t2 = c["klm"].gather(1, lb).view(-1)
        qm = q.amax(1, keepdim=True)
        lsq = c["logq"] if fault == "clf_logq" else q - qm - torch.log(torch.exp(q - qm).sum(1, keepdim=True))
        t3 = -lsq.gather(1, lb).view(-1)
    return torch.stack([t0, t1, t2, t3], 1)


def first_index_argmax(q, last=False):
    q = q.detach().cpu().numpy()
    if last:
        return (q.shape[1] - 1 - np.argmax(q[:, ::-1], axis=1)).astype(np.int32)
    return np.argmax(q, axis=1).astype(np.int32)


def latent_fwd_math(pre, eps, mu_lk, lv_lk, labels, dtype, fault=None):
    """-> dict(sigma, z [B][Z], ll, qy [B][K], terms [B][4], y int32 [B] = the first index of the maximum of this evaluation's own qy)"""
    t = lambda x: x.detach().cpu().to(dtype)                      # noqa: E731
    c = latent_core(t(pre), t(eps), t(mu_lk), t(lv_lk), fault)
    return dict(sigma=c["s"].clone(), z=c["z"].clone(), ll=c["ll"].clone(), qy=c["q"].clone(), terms=latent_terms(c, labels, fault),
                y=first_index_argmax(c["q"], last=fault == "y_last"))


def w3_values(w3):
    """the three floats the kernel reads (NULL: zeros)"""
    return (0.0, 0.0, 0.0) if w3 is None else tuple(f32(float(v)) for v in w3.detach().cpu().reshape(-1)[:3])


def latent_bwd_math(pre, eps, mu_lk, lv_lk, labels, z_in, qy_in, g_z, g_mu, g_sigma, g_ll, g_qy, w3, dtype, fault=None):
    """the documented backward formula on the given z_in and qy_in -> dict(dpre [B][2Z], dmu [B][K Z]).  w3: tensor of 3 or None.
    faults: no_dot | no_klk | no_inv_s | no_s_mul | dmu_no_kl | no_indicator"""
    t = lambda x: None if x is None else x.detach().cpu().to(dtype)           # noqa: E731
    pre, eps, m, lv, z, q = t(pre), t(eps), t(mu_lk), t(lv_lk), t(z_in), t(qy_in)
    g_z, g_mu, g_sigma, g_ll, g_qy = t(g_z), t(g_mu), t(g_sigma), t(g_ll), t(g_qy)
    w_lat, w_cls, w_clf = w3_values(w3)
    B, Z = eps.shape
    K = m.shape[0]
    mu, s = pre[:, :Z], torch.exp(pre[:, Z:])
    sp = torch.exp(lv).unsqueeze(0)                                           # [1][K][Z], the KL's standard deviation
    dmk_kl = (mu.unsqueeze(1) - m.unsqueeze(0)) / (sp * sp)                   # d KL_k / d mu per dimension, [B][K][Z]
    dsg_kl = s.unsqueeze(1) / (sp * sp) - (0.0 if fault == "no_inv_s" else 1.0 / s.unsqueeze(1))
    dq = torch.zeros(B, K, dtype=dtype) if g_qy is None else g_qy.clone()
    if labels is None:
        vr = (s.unsqueeze(1) / sp) ** 2
        t1 = ((mu.unsqueeze(1) - m.unsqueeze(0)) / sp) ** 2
        klm = (0.5 * (vr + t1 - 1.0 - torch.log(vr))).sum(-1) / Z
        if fault != "no_klk":
            dq = dq + w_lat * klm
        one = torch.ones((), dtype=dtype)
        dq = dq + w_cls * torch.where(q > 0, torch.log(torch.where(q > 0, q, one)) + 1.0, 0.0 * one) / K     # q == 0 contributes 0
        wk = w_lat * q
    else:
        lb = labels.detach().cpu().long().view(-1, 1)
        hot = torch.zeros(B, K, dtype=dtype).scatter_(1, lb, 1.0)
        qm = q.amax(1, keepdim=True)
        ex = torch.exp(q - qm)
        dq = dq + w_clf * (ex / ex.sum(1, keepdim=True) - (0.0 if fault == "no_indicator" else hot))
        wk = w_lat * hot
    dot = 0.0 if fault == "no_dot" else (q * dq).sum(1, keepdim=True)
    dll = q * (dq - dot)
    if g_ll is not None:
        dll = dll + g_ll
    tk = (z.unsqueeze(1) - m.unsqueeze(0)) * torch.exp(-lv).unsqueeze(0)      # (z - m_k) / exp(logvar): the likelihood's variance
    dz = -(dll.unsqueeze(-1) * tk).sum(1)
    if g_z is not None:
        dz = dz + g_z
    wkz = (wk / Z).unsqueeze(-1)
    dmu = (wkz * dmk_kl).sum(1) + dz
    dsg = (wkz * dsg_kl).sum(1) + dz * eps
    if g_mu is not None:
        dmu = dmu + g_mu
    if g_sigma is not None:
        dsg = dsg + g_sigma
    dmk = dll.unsqueeze(-1) * tk
    if fault != "dmu_no_kl":
        dmk = dmk - wkz * dmk_kl
    return dict(dpre=torch.cat([dmu, dsg if fault == "no_s_mul" else dsg * s], 1), dmu=dmk.reshape(B, K * Z))


class LatentStepOps:
    """the float32 restatement behind the signatures of HipOps.latent_fwd / latent_bwd.  `fault` plants one fault of latent_core, latent_terms,
    latent_bwd_math, or y_last | skip_last_row | nan"""
    name = "latent-steps-f32"

    def __init__(self, fault=None):
        self.fault = fault

    def latent_fwd(self, pre, eps, mu_lk, lv_lk, labels, sigma, z, ll, qy, y, terms):
        o = latent_fwd_math(pre, eps, mu_lk, lv_lk, labels, F32, self.fault)
        n = eps.shape[0] - (1 if self.fault == "skip_last_row" else 0)
        for dst, k in ((sigma, "sigma"), (z, "z"), (ll, "ll"), (qy, "qy"), (terms, "terms")):
            dst[:n].copy_(o[k][:n])
        y[:n].copy_(torch.from_numpy(o["y"])[:n])
        if self.fault == "nan":
            qy[eps.shape[0] // 2, 0] = float("nan")

    def latent_bwd(self, pre, eps, mu_lk, lv_lk, labels, z, qy, g_z, g_mu, g_sigma, g_ll, g_qy, w3, dpre, dmu_lk_rows):
        o = latent_bwd_math(pre, eps, mu_lk, lv_lk, labels, z, qy, g_z, g_mu, g_sigma, g_ll, g_qy, w3, F32, self.fault)
        n = eps.shape[0] - (1 if self.fault == "skip_last_row" else 0)
        dpre[:n].copy_(o["dpre"][:n])
        if dmu_lk_rows is not None:
            dmu_lk_rows[:n].copy_(o["dmu"][:n].view_as(dmu_lk_rows[:n]))
        if self.fault == "nan":
            dpre[eps.shape[0] // 2, 0] = float("nan")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _lc(B, Z, K, kind, c=None, twin=None):
    """kind: live (lv_lk = c + 0.01 randn, mu_lk = randn LIVE_SCALE / sqrt(Z) e^c) | k1 (the live recipe at K = 1: qy == 1) | twin (live, rows
    twin[0] < twin[1] of mu_lk and lv_lk equal) | saturated (lv_lk = -4 + 0.01 randn, mu_lk = randn) | init (lv_lk = -4 + 0.01 randn, mu_lk = 0.2 randn)"""
    cid = "B%d-Z%d-K%d-%s" % (B, Z, K, kind) + ("" if c is None else "-c%d" % c) + ("" if twin is None else "-k%d=k%d" % twin)
    return dict(id=cid, B=B, Z=Z, K=K, kind=kind, c=c, twin=twin)


SHAPES = [_lc(21, 128, 2, "live", -1), _lc(21, 1, 2, "live", 0), _lc(4, 5, 3, "live", -1), _lc(3, 63, 8, "live", 0), _lc(21, 64, 3, "live", -1),
          _lc(21, 65, 8, "live", -2), _lc(1, 200, 2, "live", 0), _lc(4, 200, 8, "live", -1), _lc(3, 128, 3, "live", -2),
          _lc(21, 65, 1, "k1", -1), _lc(1, 5, 1, "k1", 0), _lc(21, 65, 3, "twin", -1, (0, 2)), _lc(4, 5, 2, "twin", 0, (0, 1)),
          _lc(21, 128, 2, "saturated"), _lc(21, 128, 2, "init")]
SHAPE_BY_ID = {c["id"]: c for c in SHAPES}
assert len(SHAPE_BY_ID) == len(SHAPES)
LIVE_SHAPES = [c for c in SHAPES if c["kind"] == "live"]
FWD_CASES = [dict(c, id=c["id"] + ("-labels" if sup else "-unsup"), shape=c["id"], sup=sup) for c in SHAPES for sup in (False, True)]
FWD_BY_ID = {c["id"]: c for c in FWD_CASES}
# the forms of a backward launch: the upstream gradients given, w3 (None = NULL), dmu_lk_rows given
BWD_FORMS = dict([(u, dict(ups=(u,), w3=None, dmu=True)) for u in UPS],
                 all=dict(ups=UPS, w3=BWD_W3, dmu=True), w3only=dict(ups=(), w3=BWD_W3, dmu=True), now3=dict(ups=UPS, w3=None, dmu=True),
                 nodmu=dict(ups=UPS, w3=BWD_W3, dmu=False), null=dict(ups=(), w3=None, dmu=True),
                 k1w0=dict(ups=("g_z", "g_mu", "g_sigma", "g_qy"), w3=(0.0, 0.2, 0.7), dmu=True))
EVERY_FORM_SHAPES = ("B21-Z65-K8-live-c-2", "B3-Z63-K8-live-c0", "B21-Z128-K2-init")


def _bwd_forms_of(c):
    if c["shape"] in EVERY_FORM_SHAPES:
        return [f for f in BWD_FORMS if f != "k1w0"]
    return ["all", "w3only"] + (["k1w0", "g_qy"] if c["K"] == 1 else [])


BWD_CASES = [dict(c, id=c["id"] + "-" + form, fwd=c["id"], form=form) for c in FWD_CASES for form in _bwd_forms_of(c)]
BWD_BY_ID = {c["id"]: c for c in BWD_CASES}
CHAIN_CASES = [c for c in BWD_CASES if c["form"] in ("all", "w3only", "nodmu")]
MAX_DRAWS = 256
_INPUTS = {}


def _draw(c, k):
    B, Z, K, kind = c["B"], c["Z"], c["K"], c["kind"]
    gen = _gen("latent/%s/%d" % (c.get("shape", c["id"]), k))
    r = lambda *s: torch.randn(*s, generator=gen)                 # noqa: E731
    pre, eps = 0.3 * r(B, 2 * Z), r(B, Z)
    if kind in ("saturated", "init"):
        lv_lk, mu_lk = -4.0 + 0.01 * r(K, Z), r(K, Z) * (1.0 if kind == "saturated" else 0.2)
    else:
        lv_lk = float(c["c"]) + 0.01 * r(K, Z)
        mu_lk = r(K, Z) * (LIVE_SCALE / math.sqrt(Z) * math.exp(c["c"]))
    if c["twin"] is not None:
        k0, k1 = c["twin"]
        mu_lk[k1], lv_lk[k1] = mu_lk[k0], lv_lk[k0]
    labels = torch.randint(0, K, (B,), generator=gen, dtype=torch.int32)
    labels[0] = K - 1
    if B > 1:
        labels[1] = 0
    ups = dict(g_z=r(B, Z), g_mu=r(B, Z), g_sigma=r(B, Z), g_ll=r(B, K), g_qy=r(B, K))
    return dict(pre=pre, eps=eps, mu_lk=mu_lk, lv_lk=lv_lk, labels=labels, ups=ups, draw=k)


def latent_condition(c, inp):
    """(holds, dict of the figures) of the input condition of the case's kind, on the float64 posterior of the float32 inputs"""
    o = latent_fwd_math(inp["pre"], inp["eps"], inp["mu_lk"], inp["lv_lk"], None, F64)
    q, K = o["qy"], c["K"]
    srt = q.sort(1, descending=True)[0]
    info = dict(qmax=float(srt[:, 0].max()), qmin=float(srt[:, -1].min()), second=float(srt[:, 1].max()) if K > 1 else 0.0)
    if c["kind"] == "k1":
        return bool((q == 1.0).all()), info
    if c["kind"] == "saturated":
        return info["second"] < SAT_SECOND, info
    if c["kind"] == "init":
        ent = (q * (o["ll"] - torch.logsumexp(o["ll"], 1, keepdim=True))).sum(1).abs()
        info["ent_tile_min"] = min(float(ent[i:i + 16].max()) for i in range(0, c["B"], 16))
        return info["ent_tile_min"] >= SCAN_MIN_REF, info                     # every 16-row tile holds a half-saturated row
    if c["kind"] == "twin":
        k0, k1 = c["twin"]
        ok = bits_equal(q[:, k0].float(), q[:, k1].float()) and bool((q[:, k0] == q[:, k1]).all())
        d = q[:, [k for k in range(K) if k != k1]].sort(1, descending=True)[0]
        info["gap"] = float((d[:, 0] - d[:, 1]).min()) if K > 2 else 1.0
        info["twin_on_top"] = int((q[:, k0] == srt[:, 0]).sum())
        ok = ok and info["twin_on_top"] > 0
    else:
        info["gap"] = float((srt[:, 0] - srt[:, 1]).min())
        ok = True
    return ok and info["qmax"] <= LIVE_QMAX and info["qmin"] >= LIVE_QMIN and info["gap"] >= LIVE_GAP, info


def latent_inputs(c):
    """the first draw k = 0, 1, .. of the shape's generator that meets latent_condition; both label variants of a shape share it"""
    key = c.get("shape", c["id"])
    if key not in _INPUTS:
        base = SHAPE_BY_ID[key]
        for k in range(MAX_DRAWS):
            inp = _draw(base, k)
            if latent_condition(base, inp)[0]:
                break
        else:
            raise AssertionError("no draw of %s meets the input condition" % key)
        _INPUTS[key] = inp
    return _INPUTS[key]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# records and the tile metric
# ---------------------------------------------------------------------------------------------------------------------------------------------
def make_rec(cid, ref64, fake32, tc, exact0=None, tiny=()):
    """ref64 / fake32 {quantity: 2-D tensor}; exact0 {quantity: bool mask of the entries the operation makes exactly zero}; asserts the input
    conditions: declared zeros are zero in both, declared tiny quantities are below SCAN_MIN_REF in both, every tile that holds an undeclared entry has
    a reference maximum >= SCAN_MIN_REF"""
    rec = dict(id=cid, ref64=ref64, fake32=fake32, tc=tc, exact0={}, tiny=tuple(tiny), e_ref={}, den={})
    for k, r in ref64.items():
        f = fake32[k]
        assert r.dtype == F64 and f.dtype == F32 and r.dim() == 2 and r.shape == f.shape, (cid, k, r.dtype, f.dtype, tuple(r.shape), tuple(f.shape))
        assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(f).all()), (cid, k)
        m = (exact0 or {}).get(k)
        m = torch.zeros(r.shape, dtype=torch.bool) if m is None else m.expand(r.shape).clone()
        assert bool((r[m] == 0).all()) and bool((f[m] == 0).all()), "%s %s: declared exactly zero, but the reference or the restatement is not" % (cid, k)
        if k in tiny:
            assert float(r.abs().max()) < SCAN_MIN_REF and float(f.abs().max()) < SCAN_MIN_REF and not bool(m.any()), "%s %s: declared tiny, but is not" % (cid, k)
        e, den = tile_errors(f, r, tc=tc[k])
        if k not in tiny:
            free = tile_errors(r, (~m).double(), tc=tc[k])[1] > 0          # tiles with at least one entry that is not declared zero
            assert den[free].size == 0 or den[free].min() >= SCAN_MIN_REF, "input condition: %s %s has a tile maximum of %.3e < 2**-100" % (cid, k, den[free].min())
            assert np.isfinite(e).all(), (cid, k)
        rec["exact0"][k], rec["e_ref"][k], rec["den"][k] = m, e, den
    return rec


def check_rec(rec, got, F=None):
    """got {quantity: 2-D float32 CPU tensor} of one launch: declared zeros exactly 0.0, declared tiny quantities below SCAN_MIN_REF, then the tile bound
    of the quantity's family in EVERY tile.  A quantity the reference has and `got` lacks is an error.  Returns {family: (worst ratio, quantity,
    tile row, tile column)} of the families present."""
    F = LATENT_F if F is None else F
    cid, worst, bad = rec["id"], {}, []
    for k, r in rec["ref64"].items():
        g, fam = got.get(k), FAMILY[k]
        assert g is not None, "%s: output %s missing" % (cid, k)
        g = g.detach().cpu()
        assert g.dtype == F32 and g.shape == r.shape, (cid, k, g.dtype, tuple(g.shape), tuple(r.shape))
        worst.setdefault(fam, (0.0, "-", 0, 0))
        nz = rec["exact0"][k] & (g != 0)
        assert not bool(nz.any()), "%s %s: entry %s is exactly zero by the operation, got %r" % (cid, k, tuple(int(v) for v in torch.nonzero(nz)[0]), float(g[nz][0]))
        if k in rec["tiny"]:
            assert bool((g.abs() < SCAN_MIN_REF).all()), "%s %s: below 2**-100 in the reference, got up to %r" % (cid, k, float(g.abs().max()))
            continue
        e, den = tile_errors(g, r, tc=rec["tc"][k])
        ratio, i, j, n = worst_ratio(e, rec["e_ref"][k], assert_F(F[fam]))
        if ratio > worst[fam][0]:
            worst[fam] = (ratio, k, i, j)
        if not ratio <= F[fam]:
            bad.append("%s %s: err %.3e = %.1f x max(e_ref %.3e, 2**-23) in tile (rows %d.., columns %d..), tile max of the reference %.3e; %d of %d tiles over F = %g" % (
                cid, k, e[i, j], ratio, rec["e_ref"][k][i, j], 16 * i, rec["tc"][k] * j, den[i, j], n, e.size, F[fam]))
    assert not bad, "\n".join(bad)
    return worst


def line(test, cid, worst):
    """one line of profiles/latent_fp64_errors.txt"""
    parts = ["%s %6.3f %-5s (%d, %d) F = %g" % (fam, w[0], w[1], w[2], w[3], LATENT_F[fam]) for fam, w in worst.items()]
    return "[latent] %-13s %-44s %s" % (test, cid, "   ".join(parts))


def exact_line(test, cid, what):
    return "[latent] %-13s %-44s %s" % (test, cid, what)


def merge_worst(*ws):
    out = {}
    for w in ws:
        for fam, v in w.items():
            if fam not in out or v[0] > out[fam][0]:
                out[fam] = v
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------------------------
_FWD_CACHE = {}


def _split_terms(o):
    d = {k: o[k] for k in ("sigma", "z", "ll", "qy")}
    d.update({"t%d" % j: o["terms"][:, j:j + 1].clone() for j in range(4)})
    return d


def fwd_exact0(c):
    """the columns of terms the operation makes exactly zero: the label terms of an unsupervised launch; at K = 1 the entropy (log 1) and the
    cross-entropy of a one-class softmax"""
    one = torch.ones(1, 1, dtype=torch.bool)
    z = {}
    if not c["sup"]:
        z["t2"] = z["t3"] = one
    if c["K"] == 1:
        z["t1"] = z["t3"] = one
    return z


def fwd_tiny(c):
    return ("t1",) if c["kind"] == "saturated" else ()


def fwd_references(c):
    """the cached record of a forward case: float64 reference, float32 restatement, the reference's y and which rows decide it"""
    if c["id"] not in _FWD_CACHE:
        inp = latent_inputs(c)
        lab = inp["labels"] if c["sup"] else None
        o64, o32 = (latent_fwd_math(inp["pre"], inp["eps"], inp["mu_lk"], inp["lv_lk"], lab, dt) for dt in (F64, F32))
        K = c["K"]
        tc = dict(sigma=16, z=16, ll=K, qy=K, t0=1, t1=1, t2=1, t3=1)
        rec = make_rec(c["id"], _split_terms(o64), _split_terms(o32), tc, fwd_exact0(c), fwd_tiny(c))
        srt = o64["qy"].sort(1, descending=True)[0]
        rec["inputs"], rec["labels"], rec["y"], rec["out64"] = inp, lab, o64["y"], o64
        rec["decided"] = np.ones(c["B"], bool) if K == 1 else ((srt[:, 0] - srt[:, 1]) >= LIVE_GAP).numpy()
        _FWD_CACHE[c["id"]] = rec
    return _FWD_CACHE[c["id"]]


def run_fwd(ops, c, device="cpu", inputs=None):
    """one launch of ops.latent_fwd on the case's inputs (or `inputs`).  The sentinel-filled buffers on the CPU"""
    inp, B, Z, K = inputs or latent_inputs(c), c["B"], c["Z"], c["K"]
    names = ("pre", "eps", "mu_lk", "lv_lk")
    dev = {k: inp[k].to(device) for k in names}
    lab = inp["labels"].to(device) if c["sup"] else None
    out = dict(sigma=_buf((B + PAD_ROWS, Z), device), z=_buf((B + PAD_ROWS, Z), device), ll=_buf((B + PAD_ROWS, K), device), qy=_buf((B + PAD_ROWS, K), device),
               y=_buf((B + PAD_ROWS,), device, torch.int32), terms=_buf((B + PAD_ROWS, 4), device))
    ops.latent_fwd(dev["pre"], dev["eps"], dev["mu_lk"], dev["lv_lk"], lab, *[out[k][:B] for k in ("sigma", "z", "ll", "qy", "y", "terms")])
    for k in names:
        assert bits_equal(dev[k], inp[k]), "%s: input %s was modified" % (c["id"], k)
    assert lab is None or torch.equal(lab.cpu(), inp["labels"]), "%s: the labels were modified" % c["id"]
    return {k: v.cpu() for k, v in out.items()}


def fwd_views(c, bufs):
    """rows >= B untouched; -> the quantities of the record as [B][..] views"""
    B = c["B"]
    for k in ("sigma", "z", "ll", "qy", "terms"):
        check_sentinel(c["id"], "%s past its last row" % k, bufs[k][B:])
    check_sentinel(c["id"], "y past its last row", bufs["y"][B:], INT_SENTINEL)
    return _split_terms({k: bufs[k][:B] for k in ("sigma", "z", "ll", "qy", "terms")})


def check_fwd(c, bufs, F=None):
    """layout, y, the exact parts of the case's kind, then the tile bound.  Returns check_rec's worst"""
    rec, cid, B, K = fwd_references(c), c["id"], c["B"], c["K"]
    got = fwd_views(c, bufs)
    q, y = got["qy"], bufs["y"][:B].numpy()
    own = first_index_argmax(q)
    bad = np.nonzero(y != own)[0]
    assert bad.size == 0, "%s: row %d y = %d, the first index of the maximum of its own qy is %d" % (cid, bad[0], y[bad[0]], own[bad[0]])
    bad = np.nonzero((y != rec["y"]) & rec["decided"])[0]
    assert bad.size == 0, "%s: row %d y = %d, the reference's argmax (gap >= 1e-4) is %d" % (cid, bad[0], y[bad[0]], rec["y"][bad[0]])
    if c["kind"] in ("live", "k1", "saturated"):
        assert rec["decided"].all(), cid
    if c["kind"] == "k1":
        assert bool((q == 1.0).all()) and not y.any(), "%s: K = 1 must give qy == 1 and y == 0" % cid
    if c["kind"] == "saturated":
        hot = torch.zeros(B, K).scatter_(1, torch.from_numpy(rec["y"]).long().view(-1, 1), 1.0)
        assert torch.equal(q, hot), "%s: a saturated posterior must be exactly 1 and 0 in float32" % cid
    if c["kind"] == "twin":
        k0, k1 = c["twin"]
        for k in ("ll", "qy"):
            assert bits_equal(got[k][:, k0].contiguous(), got[k][:, k1].contiguous()), "%s: %s of the identical components %d and %d differ" % (cid, k, k0, k1)
        assert not (y == k1).any(), "%s: y names the second of two identical components" % cid
    return check_rec(rec, got, F)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------------------------
_BWD_CACHE = {}
BWD_TC = dict(dpre=16, dmu=16)


def bwd_w3(c, w3=None):
    w3 = BWD_FORMS[c["form"]]["w3"] if w3 is None else w3
    return None if w3 is None else torch.tensor(w3, dtype=F32)


def bwd_exact0(c, qy_in, w3=None):
    """the entries of dpre and dmu_lk_rows that the operation makes exactly zero in this form of the launch, from the form, K, the labels and the zeros
    and ones of the given qy alone:  dll_k = q_k (dq_k - sum q dq) + g_ll_k is zero without g_ll when nothing feeds dq, when q_k == 0, or when q_k == 1
    and every other q is 0;  the KL weight of component k is w_lat q_k (unsupervised) or w_lat [k == label]"""
    form, B, Z, K = BWD_FORMS[c["form"]], c["B"], c["Z"], c["K"]
    ups = form["ups"]
    w_lat, w_cls, w_clf = w3_values(bwd_w3(c, w3))
    q = qy_in.detach().cpu()
    feeds = "g_qy" in ups or ((w_clf != 0) if c["sup"] else (w_lat != 0 or w_cls != 0))
    alone = (q == 1) & ((q != 0).sum(1, keepdim=True) == 1)
    dll0 = torch.full((B, K), "g_ll" not in ups) & (torch.full((B, K), not feeds) | (q == 0) | alone)
    if c["sup"]:
        hot = torch.zeros(B, K, dtype=torch.bool).scatter_(1, latent_inputs(c)["labels"].long().view(-1, 1), True)
        wk0 = torch.full((B, K), w_lat == 0) | ~hot
    else:
        wk0 = torch.full((B, K), w_lat == 0) | (q == 0)
    dz0 = torch.full((B,), "g_z" not in ups) & dll0.all(1)
    kl0 = wk0.all(1)
    mu0, v0 = dz0 & kl0 & ("g_mu" not in ups), dz0 & kl0 & ("g_sigma" not in ups)
    return dict(dpre=torch.cat([mu0.view(B, 1).expand(B, Z), v0.view(B, 1).expand(B, Z)], 1),
                dmu=(dll0 & wk0).view(B, K, 1).expand(B, K, Z).reshape(B, K * Z))


def bwd_given(c):
    """(z_in, qy_in) of the launch driven from the reference: the float32 rounding of the float64 forward reference, independent of any kernel"""
    o = fwd_references(FWD_BY_ID[c["fwd"]])["out64"]
    return o["z"].float(), o["qy"].float()


def bwd_references(c, z_in=None, qy_in=None, w3=None):
    """the record of a backward case on the given z_in / qy_in (default, cached: bwd_given)"""
    key = c["id"] if z_in is None and w3 is None else None
    if key is not None and key in _BWD_CACHE:
        return _BWD_CACHE[key]
    if z_in is None:
        z_in, qy_in = bwd_given(c)
    inp, form = latent_inputs(c), BWD_FORMS[c["form"]]
    args = [inp["pre"], inp["eps"], inp["mu_lk"], inp["lv_lk"], inp["labels"] if c["sup"] else None, z_in, qy_in] + \
           [inp["ups"][u] if u in form["ups"] else None for u in UPS] + [bwd_w3(c, w3)]
    o64, o32 = (latent_bwd_math(*args, dt) for dt in (F64, F32))
    rec = make_rec(c["id"], o64, o32, BWD_TC, bwd_exact0(c, qy_in, w3))
    rec["args"] = args
    if key is not None:
        _BWD_CACHE[key] = rec
    return rec


def run_bwd(ops, c, device="cpu", z_in=None, qy_in=None, w3=None, dmu=None):
    """one launch of ops.latent_bwd in the case's form on z_in / qy_in (default: bwd_given).  dict(dpre [B + 3][2Z], dmu [B + 3][K Z] | None) on the CPU"""
    B, Z, K, form = c["B"], c["Z"], c["K"], BWD_FORMS[c["form"]]
    args = bwd_references(c, z_in, qy_in, w3)["args"]
    dev = [None if a is None else a.to(device) for a in args]
    dpre = _buf((B + PAD_ROWS, 2 * Z), device)
    dm = _buf((B + PAD_ROWS, K * Z), device) if (form["dmu"] if dmu is None else dmu) else None
    ops.latent_bwd(*dev, dpre[:B], None if dm is None else dm[:B])
    for a, d in zip(args, dev):
        assert a is None or torch.equal(d.cpu(), a), "%s: an input was modified" % c["id"]
    return dict(dpre=dpre.cpu(), dmu=None if dm is None else dm.cpu())


def check_bwd(c, bufs, F=None, z_in=None, qy_in=None, w3=None):
    rec, B = bwd_references(c, z_in, qy_in, w3), c["B"]
    check_sentinel(c["id"], "dpre past its last row", bufs["dpre"][B:])
    got = dict(dpre=bufs["dpre"][:B])
    if bufs["dmu"] is None:
        rec = dict(rec, ref64={"dpre": rec["ref64"]["dpre"]})
    else:
        check_sentinel(c["id"], "dmu_lk_rows past its last row", bufs["dmu"][B:])
        got["dmu"] = bufs["dmu"][:B]
    return check_rec(rec, got, F)


def chain(ops, c, device="cpu"):
    """(z, qy) [B][..] float32 on the CPU as the backend's own forward wrote them"""
    f = run_fwd(ops, FWD_BY_ID[c["fwd"]], device)
    return f["z"][:c["B"]].clone(), f["qy"][:c["B"]].clone()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# exact cases: bits, not bounds
# ---------------------------------------------------------------------------------------------------------------------------------------------
EXACT_SHAPE = "B21-Z65-K8-live-c-2"
EXACT_CASES = ("eps0-v0", "w_cls-unused-with-labels", "w_clf-unused-without-labels", "nodmu-same-dpre", "all-null-gives-zeros", "k1-no-g_ll-w_lat0",
               "second-launch-same-bits")


def run_exact(ops, name, device="cpu"):
    """asserts one exact property of the backend; returns the text of its profile line"""
    un, sup = BWD_BY_ID[EXACT_SHAPE + "-unsup-all"], BWD_BY_ID[EXACT_SHAPE + "-labels-all"]
    B, Z = un["B"], un["Z"]
    if name == "eps0-v0":
        c = FWD_BY_ID[EXACT_SHAPE + "-labels"]
        inp = dict(latent_inputs(c))
        inp["eps"], inp["pre"] = torch.zeros(B, Z), inp["pre"].clone()
        inp["pre"][:, Z:] = 0.0
        got = fwd_views(c, run_fwd(ops, c, device, inp))
        assert bits_equal(got["z"], inp["pre"][:, :Z]), "eps = 0 must give z the bits of mu"
        assert bool((got["sigma"] == 1.0).all()), "v = 0 must give sigma == 1"
        return "eps = 0: z has the bits of mu; v = 0: sigma == 1"
    if name in ("w_cls-unused-with-labels", "w_clf-unused-without-labels"):
        c, wa, wb = (sup, (0.3, 7.0, 0.7), (0.3, 0.0, 0.7)) if name.startswith("w_cls") else (un, (0.3, 0.2, 9.0), (0.3, 0.2, 0.0))
        a, b = run_bwd(ops, c, device, w3=wa), run_bwd(ops, c, device, w3=wb)
        assert bits_equal(a["dpre"], b["dpre"]) and bits_equal(a["dmu"], b["dmu"]), "w3 = %r must give the bits of %r" % (wa, wb)
        check_bwd(c, a, CAP_F, w3=wa)
        return "w3 = %r gives the bits of %r" % (wa, wb)
    if name == "nodmu-same-dpre":
        for c in (un, sup):
            a, b = run_bwd(ops, c, device), run_bwd(ops, c, device, dmu=False)
            assert b["dmu"] is None and bits_equal(a["dpre"], b["dpre"]), "%s: dpre without dmu_lk_rows differs from the launch with it" % c["id"]
        return "dmu_lk_rows = NULL: dpre has the bits of the launch with it"
    if name == "all-null-gives-zeros":
        for c in (BWD_BY_ID[EXACT_SHAPE + "-unsup-null"], BWD_BY_ID[EXACT_SHAPE + "-labels-null"]):
            b = run_bwd(ops, c, device)
            assert bool((b["dpre"][:B] == 0).all()) and bool((b["dmu"][:B] == 0).all()), "%s: no upstream gradient and w3 = NULL must give zeros" % c["id"]
            check_bwd(c, b, CAP_F)
        return "no upstream gradient, w3 = NULL: dpre == 0, dmu_lk_rows == 0"
    if name == "k1-no-g_ll-w_lat0":
        for c in (c for c in BWD_CASES if c["form"] == "k1w0"):
            b = run_bwd(ops, c, device)
            assert bool((b["dmu"][:c["B"]] == 0).all()), "%s: K = 1 without g_ll and w_lat must give dmu_lk_rows == 0" % c["id"]
            check_bwd(c, b, CAP_F)
        return "K = 1, g_ll = NULL, w_lat = 0: dmu_lk_rows == 0"
    assert name == "second-launch-same-bits"
    for c in (un, sup):
        f = FWD_BY_ID[c["fwd"]]
        a, b = run_fwd(ops, f, device), run_fwd(ops, f, device)
        assert all(torch.equal(a[k], b[k]) if k == "y" else bits_equal(a[k], b[k]) for k in a), "%s: two forward launches differ" % f["id"]
        a, b = run_bwd(ops, c, device), run_bwd(ops, c, device)
        assert bits_equal(a["dpre"], b["dpre"]) and bits_equal(a["dmu"], b["dmu"]), "%s: two backward launches differ" % c["id"]
    return "a second launch gives the same bits"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# what test_gpu_parity.test_latent_kernels checks today
# ---------------------------------------------------------------------------------------------------------------------------------------------
OLD_TOL = 1e-4


def old_check_inputs(sup=False):
    """the inputs of test_latent_kernels, drawn as it draws them: B = 11, Z = 128, K = 2, lv_lk = -4 + 0.01 randn"""
    B, Z, K = 11, 128, 2
    with torch.random.fork_rng():                                 # its torch.manual_seed(21), without touching the caller's generator
        torch.manual_seed(21)
        pre = torch.randn(B, 2 * Z) * 0.3
        eps = torch.randn(B, Z)
        mu_lk = torch.randn(K, Z) * 0.2
        lv_lk = torch.full((K, Z), -4.0) + torch.randn(K, Z) * 0.01
        labels = torch.randint(0, K, (B,), dtype=torch.int32) if sup else None
        ups = [torch.randn(B, Z), torch.randn(B, Z), torch.randn(B, Z), torch.randn(B, K), torch.randn(B, K)]
    w3 = torch.tensor((0.3, 0.0, 0.7) if sup else (0.3, 0.2, 0.0))
    return dict(pre=pre, eps=eps, mu_lk=mu_lk, lv_lk=lv_lk, labels=labels, ups=ups, w3=w3, B=B, Z=Z, K=K)


def old_check_accepts(fake, ops, sup=False):
    """(whether close(dpre, ., 1e-4) and close(dmu_lk_rows, ., 1e-4) of test_latent_kernels accept `ops` against `fake` (FakeOps), the two whole-tensor
    errors, the qy of the forward)"""
    i = old_check_inputs(sup)
    B, Z, K = i["B"], i["Z"], i["K"]
    o = [torch.zeros(B, Z), torch.zeros(B, Z), torch.zeros(B, K), torch.zeros(B, K), torch.zeros(B, dtype=torch.int32), torch.zeros(B, 4)]
    fake.latent_fwd(i["pre"], i["eps"], i["mu_lk"], i["lv_lk"], i["labels"], *o)
    res = []
    for be in (fake, ops):
        d, m = torch.zeros(B, 2 * Z), torch.zeros(B, K * Z)
        be.latent_bwd(i["pre"], i["eps"], i["mu_lk"], i["lv_lk"], i["labels"], o[1], o[3], *i["ups"], i["w3"], d, m)
        res.append((d, m))
    rel = lambda a, b: float((a.double() - b.double()).abs().max()) / max(1e-12, float(b.double().abs().max()))          # noqa: E731
    ok = old_metric_accepts(res[1][0], res[0][0], OLD_TOL) and old_metric_accepts(res[1][1], res[0][1], OLD_TOL)
    return ok, (rel(res[1][0], res[0][0]), rel(res[1][1], res[0][1])), o[3]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the refusals of the C ABI: (id, entry point, arguments from the pointers p.f / p.i, code).  B = 2, Z = 4, K = 2 inside 4096-element buffers
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _fwd_args(null=None, B=2, Z=4, K=2):
    names = ("pre", "eps", "mu_lk", "lv_lk", "labels", "sigma", "z", "ll", "qy", "y", "terms")
    return lambda p: tuple(None if n == null else (p.i if n in ("labels", "y") else p.f) for n in names[:4]) + (B, Z, K) + \
        tuple(None if n == null else (p.i if n in ("labels", "y") else p.f) for n in names[4:]) + (None,)


def _bwd_args(null=None, B=2, Z=4, K=2):
    names = ("pre", "eps", "mu_lk", "lv_lk", "labels", "z", "qy", "g_z", "g_mu", "g_sigma", "g_ll", "g_qy", "w3", "dpre", "dmu_lk_rows")
    return lambda p: tuple(None if n == null else p.f for n in names[:4]) + (B, Z, K) + \
        tuple(None if n == null else (p.i if n == "labels" else p.f) for n in names[4:]) + (None,)


FWD_REQUIRED = ("pre", "eps", "mu_lk", "lv_lk", "sigma", "z", "ll", "qy", "y", "terms")
BWD_REQUIRED = ("pre", "eps", "mu_lk", "lv_lk", "z", "qy", "dpre")
BAD_SHAPES = (("B = 0", dict(B=0)), ("B = -1", dict(B=-1)), ("Z = 0", dict(Z=0)), ("Z = -3", dict(Z=-3)), ("K = 0", dict(K=0)), ("K = -1", dict(K=-1)),
              ("K = 9", dict(K=9)))
LATENT_REFUSALS = [("latent_fwd %s NULL" % n, "fn_latent_fwd", _fwd_args(n), E_NULL) for n in FWD_REQUIRED]
LATENT_REFUSALS += [("latent_fwd %s NULL and K = 9" % n, "fn_latent_fwd", _fwd_args(n, K=9), E_NULL) for n in ("pre", "terms")]
LATENT_REFUSALS += [("latent_fwd %s" % s, "fn_latent_fwd", _fwd_args(**kw), E_SHAPE) for s, kw in BAD_SHAPES]
LATENT_REFUSALS += [("latent_bwd %s NULL" % n, "fn_latent_bwd", _bwd_args(n), E_NULL) for n in BWD_REQUIRED]
LATENT_REFUSALS += [("latent_bwd %s NULL and B = 0" % n, "fn_latent_bwd", _bwd_args(n, B=0), E_NULL) for n in ("qy", "dpre")]
LATENT_REFUSALS += [("latent_bwd %s" % s, "fn_latent_bwd", _bwd_args(**kw), E_SHAPE) for s, kw in BAD_SHAPES]
