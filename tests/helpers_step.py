"""The assembled training step (Engine / *Trainer.loss_and_grads) against the float64 oracle, per 16 x 32 block of every gradient.

The kernels of the step have per-tile checks of their own; what chains them - the chunked decoder pipeline and its hand-over slots, the attribute
decoders riding in the head / tail launches, the one bf16 x 6 decision per pipeline, the dw_order lanes, the beta-accumulated weight gradients, the
placement of every gradient in the flat buffer - was judged by whole-tensor numbers only (max |got - ref| / max |ref| at >= 5e-4, sum |g| at 5e-4, a
stride-97 / 4-row sample).  Inside one tensor the block maxima fall to 1e-5 of the tensor maximum, so a block that is zeroed, stale or a neighbour's
passes all of them.  check_step_grads() states the bound per block, relative to what float32 rounding costs THAT block:

    m = max |g64|,  e_ref = max |g32 - g64|,  e = max |got - g64|  over the block,      e <= STEP_F * max(e_ref, 2**-24 * m)

with g64 / g32 the oracle's gradients in float64 / float32 on the same weights, batch and eps.  STEP_F is one power of two for every case: at least
twice the worst ratio the CPU stand-in (tests/fake_ops.py: the documented semantics of every entry point, fp32, another summation order than the
oracle's autograd) reaches on the inputs of every case, capped at 32 (test_step_reference.py asserts the rule; profiles/step_fp64_errors.txt
records the figures).  Nothing measured on a GPU enters it.
"""
import os
import re

import numpy as np
import torch

from helpers import NOISE_PARAMS, PlanRecorder, make_model, make_sibling, make_vae_model, relerr
from mfn_import import load_package
from oracle import gmvae_oracle as orc

STEP_BLOCK = (16, 32)            # rows x columns of one block (ragged at the edges); a 1-D gradient is one row of 32-wide blocks
STEP_F_CAP = 32
# the smallest power of two >= 2 x the worst FakeOps ratio over every case below (worst 14.2: glsr at hidden 512, B 256, T 8; GMVAE worst 11.6: case i)
STEP_F = 32
STEP_EPS = 2.0 ** -24            # the denominator's floor, relative to the block's maximum: half an fp32 ulp
STEP_MIN_REF = 2.0 ** -100       # input condition: a block that is not exactly zero has a maximum of at least this
ENC_WIH = re.compile(r"^gru(_r|_n|_e)?\.weight_ih_l0(_reverse)?$")      # encoder input matrices: column v = token v (the first 342 columns)
E_VOCAB = 342


# ---- blocks ------------------------------------------------------------------------------------------------------------------------------
def block_absmax(a):
    """[row blocks][column blocks] maxima of |a| over 16 x 32 blocks (a NaN makes its block NaN)"""
    a = np.abs(np.asarray(a, np.float64))
    if a.ndim != 2:
        a = a.reshape(1, -1)
    br, bc = STEP_BLOCK
    R, C = a.shape
    nr, nc = -(-R // br), -(-C // bc)
    p = np.zeros((nr * br, nc * bc))
    p[:R, :C] = a
    return p.reshape(nr, br, nc, bc).max(axis=(1, 3))


def block_slice(shape, bi, bj):
    """index of block (bi, bj) in a gradient of `shape` (1-D: bi == 0)"""
    br, bc = STEP_BLOCK
    if len(shape) == 1:
        return (slice(bj * bc, min(shape[0], (bj + 1) * bc)),)
    return (slice(bi * br, min(shape[0], (bi + 1) * br)), slice(bj * bc, min(shape[1], (bj + 1) * bc)))


# ---- references --------------------------------------------------------------------------------------------------------------------------
_STEP_REF_CACHE = {}


def step_references(key, build, tokens):
    """dict(g64, g32, tup64, m, e_ref, den, absent, floor_share) of one case, cached by `key`.  build(dtype) -> ({name: gradient}, loss tuple) runs the
    oracle with torch's default dtype switched to `dtype` (and restored); tokens = the batch's d.  Asserts the input condition: every e_ref finite,
    every block that is not exactly zero has m >= 2**-100."""
    if key in _STEP_REF_CACHE:
        return _STEP_REF_CACHE[key]
    old, threads = torch.get_default_dtype(), torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    res = {}
    try:
        for dt in (torch.float64, torch.float32):
            torch.set_default_dtype(dt)
            grads, tup = build(dt)
            assert all(g.dtype == dt for g in grads.values()), "the oracle left %s" % dt
            res[dt] = ({k: g.detach().numpy().astype(np.float64) for k, g in grads.items()}, tuple(float(x.detach() if torch.is_tensor(x) else x) for x in tup))
    finally:
        torch.set_default_dtype(old)
        torch.set_num_threads(threads)
    g64, g32 = res[torch.float64][0], res[torch.float32][0]
    ref = dict(g64=g64, g32=g32, tup64=res[torch.float64][1], m={}, e_ref={}, den={})
    floor = total = 0
    for k, a in g64.items():
        m, e = block_absmax(a), block_absmax(g32[k] - a)
        assert np.isfinite(e).all() and np.isfinite(m).all(), "input condition: %s has a block whose e_ref is not finite" % k
        assert (m[m > 0] >= STEP_MIN_REF).all(), "input condition: %s has a non-zero block with a maximum below 2**-100" % k
        ref["m"][k], ref["e_ref"][k], ref["den"][k] = m, e, np.maximum(e, STEP_EPS * m)
        if k not in NOISE_PARAMS:
            floor += int(((e < STEP_EPS * m) & (m > 0)).sum())
            total += int((m > 0).sum())
    ref["floor_share"] = floor / max(1, total)
    ref["absent"] = np.setdiff1d(np.arange(E_VOCAB), np.unique(np.asarray(tokens)))
    _STEP_REF_CACHE[key] = ref
    return ref


def check_step_grads(got, ref, F=None):
    """{name: gradient} of the step under test against step_references(), block by block:
      ratio      e <= F * max(e_ref, 2**-24 m) in every block with m > 0;
      zeros      a block with m == 0 is exactly zero, and - independently - so is every column of an encoder input matrix whose token the batch
                 does not hold;
      noise      linear_out_{r,n}.bias (mathematically zero, rounding noise in float64 too): max |got| <= F * max |g32|, kept out of the ratios.
    Returns dict(worst=(ratio, name, (bi, bj)), per={name: (ratio, (bi, bj))}, zero_blocks, absent_tokens, floor_share, blocks)."""
    F = STEP_F if F is None else F
    assert F <= STEP_F_CAP
    assert set(got) == set(ref["g64"]), set(got) ^ set(ref["g64"])
    bad, per, zero_blocks, blocks = [], {}, 0, 0
    absent, checked_absent = ref["absent"], False
    for k, g64 in ref["g64"].items():
        a = np.asarray(got[k].detach().cpu().numpy() if torch.is_tensor(got[k]) else got[k], np.float64)
        assert a.shape == g64.shape, (k, a.shape, g64.shape)
        if k in NOISE_PARAMS:
            lim = F * float(np.abs(ref["g32"][k]).max())
            if not float(np.abs(a).max()) <= lim:
                bad.append("%s: noise-only tensor reaches %.3e > F x max |g32| = %.3e" % (k, float(np.abs(a).max()), lim))
            continue
        if ENC_WIH.match(k):
            checked_absent = True
            cols = np.nonzero(~(a[:, absent] == 0).all(0))[0]
            if len(cols):
                bad.append("%s: column of token %d, which the batch does not hold, is not exactly zero (%d such columns)" % (k, int(absent[cols[0]]), len(cols)))
        m, den = ref["m"][k], ref["den"][k]
        e, mag = block_absmax(a - g64), block_absmax(a)
        zero = m == 0
        zero_blocks += int(zero.sum())
        blocks += m.size
        nz = zero & ~(mag == 0)
        if nz.any():
            bi, bj = (int(x) for x in np.argwhere(nz)[0])
            bad.append("%s: block (%d, %d) is exactly zero in float64 and holds %.3e (%d such blocks)" % (k, bi, bj, mag[bi, bj], int(nz.sum())))
        if k in ref.get("leak", {}):                  # the proven share of fn_latent_bwd's softmax backward (latent_leak_allowance) comes off first
            e = np.maximum(e - ref["leak"][k], 0.0)
        ratio = np.where(zero, 0.0, e / np.where(zero, 1.0, den))
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        bi, bj = (int(x) for x in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
        per[k] = (float(ratio[bi, bj]), (bi, bj))
        if not ratio[bi, bj] <= F:
            bad.append("%s: block (%d, %d) err %.3e = %.1f x max(e_ref %.3e, 2**-24 x %.3e) (%d of %d blocks over F = %g; tensor max %.3e)" % (
                k, bi, bj, e[bi, bj], ratio[bi, bj], ref["e_ref"][k][bi, bj], m[bi, bj], int((~(ratio <= F)).sum()), ratio.size, F, float(m.max())))
    assert not bad, "\n".join(bad)
    wk = max(per, key=lambda k: per[k][0])
    return dict(worst=(per[wk][0], wk, per[wk][1]), per=per, zero_blocks=zero_blocks, absent_tokens=len(absent) if checked_absent else 0,
                floor_share=ref["floor_share"], blocks=blocks)


def check_loss_terms(tup, ref, rtol=2e-5):
    """the step's loss terms against the float64 oracle's tuple"""
    n = min(len(tup), len(ref["tup64"]))          # (the VAE family's trainers return GMVAETrainer's eight numbers, its oracle the reference's six)
    np.testing.assert_allclose(np.asarray(tup[:n], np.float64), np.asarray(ref["tup64"][:n]), rtol=rtol, atol=0)


def old_metric_findings(got, ref):
    """What the whole-tensor assertions the suite applied to the step so far find in `got`, with g32 in the place of the reference's own float32
    gradients: relerr < max(5e-4, 4 x relerr(g32, g64)) against g64 (test_fused_gradients_vs_reference, small), sum |g| at rtol 5e-4 (its hidden-512
    branch), and the first 2 + last 2 rows and every 97th element at 5e-4 of the tensor's maximum (test_gradient_slices_vs_reference_at_hidden_512).
    [] = they accept it."""
    out = []
    for k, ex in ref["g64"].items():
        if k in NOISE_PARAMS:
            continue
        a, r32 = np.asarray(got[k], np.float64), ref["g32"][k]
        tol = max(5e-4, 4.0 * relerr(r32, ex))
        if not (relerr(a, ex) < tol or np.abs(ex).max() < 1e-6):
            out.append((k, "relerr"))
        if not np.isclose(np.abs(a).sum(), np.abs(r32).sum(), rtol=5e-4, atol=1e-5):
            out.append((k, "abs-sum"))
        scale = float(np.abs(a).max())
        rs = r32.reshape(-1)[::97]
        if not np.abs(a.reshape(-1)[::97] - rs).max() <= 5e-4 * max(scale, np.abs(rs).max()) + 1e-7:
            out.append((k, "stride-97"))
        rows = (lambda x: np.concatenate([x[:2], x[-2:]], 0)) if (a.ndim == 2 and a.shape[0] >= 8) else (lambda x: x)
        if not np.abs(rows(a) - rows(r32)).max() <= 5e-4 * max(scale, np.abs(rows(r32)).max()) + 1e-7:
            out.append((k, "rows"))
    return out


def old_sample_touches(shape, bi, bj):
    """does the stride-97 sample or the first 2 + last 2 rows touch block (bi, bj) of a 2-D gradient of `shape`?"""
    rs, cs = block_slice(shape, bi, bj)
    r, c = np.meshgrid(np.arange(rs.start, rs.stop), np.arange(cs.start, cs.stop), indexing="ij")
    return bool(((r * shape[1] + c) % 97 == 0).any() or (r < 2).any() or (r >= shape[0] - 2).any())


def step_line(case, arith, kernels, st):
    """one line of profiles/step_fp64_errors.txt"""
    ratio, name, (bi, bj) = st["worst"]
    return "%-30s %-7s %-44s worst %-30s block (%3d, %2d) ratio %6.3f  zero blocks %4d  absent tokens %3d  floor share %.3f" % (
        case, arith, kernels, name, bi, bj, ratio, st["zero_blocks"], st["absent_tokens"], st["floor_share"])


# ---- recording which scan kernels a step ran --------------------------------------------------------------------------------------------------
class StepRecorder(PlanRecorder):
    """PlanRecorder as the ops object of an engine: the engine and the model SET attributes on their ops (the lane of the next launches, the
    arithmetic), which must reach the wrapped HipOps; .launches = per launch (direction, tags of its scans, their step counts, persistent asked)"""
    _OWN = ("ops", "fwd", "bwd", "launches")

    def __init__(self, ops):
        object.__setattr__(self, "launches", [])
        super().__init__(ops)

    def __setattr__(self, name, value):
        if name in self._OWN:
            object.__setattr__(self, name, value)
        else:
            setattr(self.ops, name, value)

    def gru_seq_fwd(self, scans, **kw):
        self.launches.append(("fwd", tuple(s.get("tag", "enc") for s in scans), tuple(s["T"] for s in scans), kw.get("persistent", True)))
        super().gru_seq_fwd(scans, **kw)

    def gru_seq_bwd(self, scans, **kw):
        self.launches.append(("bwd", tuple(s.get("tag", "enc") for s in scans), tuple(s["T"] for s in scans), kw.get("persistent", True)))
        super().gru_seq_bwd(scans, **kw)

    def decoder_kernels(self):
        """[(direction, tags, step counts, plan, chosen kernel)] of the launches that hold a decoder scan (pipeline layers, attribute decoders)"""
        plans = {"fwd": iter(self.fwd), "bwd": iter(self.bwd)}
        out = []
        for way, tags, steps, _ in self.launches:
            p = next(plans[way])
            assert p["status"] == 0 and p["chosen"] is not None and p["candidates"][p["chosen"]]["fits"] is not False, p
            if any(t.startswith(("dec_", "sd_")) for t in tags):
                out.append((way, tags, steps, p, p["candidates"][p["chosen"]]["kernel"]))
        return out


def kernel_family(name):
    return "x6" if "_x6" in name else ("step" if "_step_kernel" in name else "f32-ws")


def check_step_kernels(rec, want, persist=True):
    """The scan kernels the step's decoder launches took, from the library's own plan of every launch: want = "x6" (every pipeline launch on the
    bf16 x 6 kernels), "f32" (none of them, whatever was requested) - and the per-step kernels exactly where the engine asked for them
    (persist_dec off) or no weight-stationary candidate fits the launch (e.g. a one-step chunk).  Returns a label for the profile lines."""
    dk = rec.decoder_kernels()
    assert dk, "no decoder launch was recorded"
    fams = {}
    for way, tags, steps, p, kern in dk:
        fam = kernel_family(kern)
        fams.setdefault(way, set()).add(kern)
        pipeline = any(t in ("dec_l1", "dec_l2") for t in tags)
        if not persist:
            assert fam == "step", (way, tags, kern)
            continue
        if fam == "step":                             # only where every weight-stationary candidate tried in front of it does not fit
            assert all(c["fits"] is False for c in p["candidates"][:p["chosen"]]), (way, tags, steps, kern, p)
        if want == "x6" and way == "fwd" and pipeline:
            assert fam == "x6", (way, tags, steps, kern)
        if want == "f32":
            assert fam != "x6", (way, tags, steps, kern)
    # (a backward launch decides for itself, and the pipeline's 32-row groups stay on gru_bwd_rs_kernel unless FN_GRU_X6_BWD_32ROWS asks: gru_plan.h)
    return " ".join("+".join(sorted(re.sub(r"^gru_|_kernel", "", k) for k in fams.get(w, ()))) for w in ("fwd", "bwd"))


# ---- GMVAE cases ---------------------------------------------------------------------------------------------------------------------------
def _gc(cid, H, Z, B, T, Tr, chunk, sup=False, steps=(20000,), persist=True, ariths=("f32",), seed=0, what="", leak=False):
    return dict(id=cid, H=H, Z=Z, B=B, T=T, Tr=Tr, chunk=chunk, sup=sup, steps=steps, persist=persist, ariths=ariths, seed=seed, what=what, leak=leak)


GMVAE_CASES = [
    _gc("a", 64, 32, 8, 7, 3, 2, what="4 chunks, one-step tail, both hand-over slots reused, fill edges with 2 attribute chunks"),
    _gc("b", 64, 32, 5, 3, 2, 2, seed=1, what="2 chunks, T < 2 chunk: no fill, ragged batch, mostly zero blocks"),
    _gc("c", 64, 32, 8, 2, 1, 32, seed=2, what="one chunk, Tr = 1"),
    _gc("d", 64, 32, 70, 12, 5, 4, sup=True, seed=3, what="supervised, 3 chunks, fill with Tr in (chunk, 2 chunk]"),
    _gc("e", 64, 32, 8, 7, 3, 2, persist=False, what="persist_dec off: per-step kernels"),
    _gc("f", 512, 128, 8, 7, 3, 2, ariths=("f32", "bf16x6"), what="hidden 512 at few rows: fp32 kernels whatever is requested", leak=True),
    _gc("g", 512, 128, 256, 8, 4, 2, ariths=("f32", "bf16x6"), what="256-row weight-stationary launches"),
    _gc("h", 512, 128, 256, 9, 4, 4, ariths=("bf16x6",), what="one-step tail: the whole pipeline falls to fp32"),
    _gc("i", 512, 128, 128, 16, 8, 4, sup=True, steps=(20000, 500), seed=4, what="supervised, annealed beta at step 500"),
]
# which kernels the pipeline must take per (case, requested arithmetic)
GMVAE_WANT = {("g", "bf16x6"): "x6", ("f", "bf16x6"): "f32", ("h", "bf16x6"): "f32"}


def gmvae_case(cid):
    return next(c for c in GMVAE_CASES if c["id"] == cid)


def gmvae_batch(case):
    load_package()
    from music_fader_nets_amd.synth import synth_batch
    return synth_batch(np.random.RandomState(case["seed"]), case["B"], case["T"], case["Tr"])


def latent_leak_allowance(sd, b, eps, step, beta, sup):
    """{name: per-block bound} on what fn_latent_bwd's softmax backward adds to a gradient, from float64 reference quantities only.

    The kernel forms dll_k = q_k (dq_k - sum_j q_j dq_j) in double on the float32 qy it is handed (include/fadernets.h says so).  Write rho = 1 - sum_j q_j
    and dq_j = c + d_j with c the dq of the largest q.  Then dll_k = q_k (d_k - sum_j q_j d_j) + rho c q_k: the first term is the expression on
    differences of the dq_j (e_ref's order, as the oracle's), the second exists only because the float32 q_j sum to 1 to rounding: |rho| <= sum_j
    2**-24 q_j = 2**-24, while c = w_lat KLmean + w_cls (log q + 1) / K is about 1e3 w_lat.  ll_bk enters the loss of row b only, so adding rho_b c_b q_bk
    to dll_bk adds  rho_b c_b grad_theta (sum_k q_bk ll_bk)  (q held constant) to the gradient of every parameter theta behind the posterior, hence
    element by element    |got - (offset-free form)| <= sum_b |rho_b| |c_b| |grad_theta sum_k q_bk ll_bk|,   |rho_b| bounded per row (below).
    One backward pass through the encoder per row and encoder: used at 8 rows (cases with more rows are held to the bound without it).
    With labels dq holds no KL mean (c = w_clf (softmax(q) - [k == label]), order 1 / B) - the same formula."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        w = {k: v.double() for k, v in sd.items()}
        keys = [k for k in orc.trainable_used_keys(w) if k.startswith(("gru_r.", "gru_n.", "mu_r", "mu_n", "var_r", "var_n"))]
        leaves = {k: w[k].clone().requires_grad_(True) for k in keys}
        p = dict(w)
        p.update(leaves)
        d = torch.as_tensor(b["d"]).long()
        B = d.shape[0]
        enc = orc.encode(p, orc.convert_to_one_hot(d, orc.E))
        beta0 = orc.beta_schedule(step, beta)
        acc = {k: torch.zeros_like(w[k]) for k in keys}
        for i, e in enumerate(("r", "n")):
            mu, sg = enc[2 * i], enc[2 * i + 1]
            m_lk, lv_lk = p["mu_%s_lookup.weight" % e], p["logvar_%s_lookup.weight" % e]
            ll, qy = orc.approx_qy_x(mu + sg * eps[i].double(), m_lk, lv_lk)
            q = qy.detach()
            K = q.shape[1]
            if sup:
                hot = torch.zeros(B, K).scatter_(1, torch.as_tensor(b["a"]).long().view(-1, 1), 1.0)
                dq = (torch.softmax(q, 1) - hot) / B
            else:
                kl = torch.stack([orc._kl_normal(mu, sg, m_lk[k], torch.exp(lv_lk[k])).mean(-1) for k in range(K)], 1).detach()
                dq = beta0 / B * (kl + (torch.log(q.clamp_min(1e-300)) + 1.0) / K)
            # |rho_b|: 1.0 is a float32, so the largest q is rounded by at most min(2**-25, r), r = 1 - max q (a saturated row has nothing to leak), every
            # other q_j by at most 2**-24 q_j <= 2**-24 r in all.  r is taken twice: the kernel's own posterior - from its float32 z - may differ from this
            # float64 one by the few per cent that a 1e-2 shift of a log-likelihood difference makes
            r = 2.0 * (1.0 - q.max(1)[0])
            rho = torch.minimum(torch.full_like(r, 2.0 ** -25), r) + 2.0 ** -24 * r
            c = dq.gather(1, q.argmax(1, keepdim=True)).abs().view(-1) * rho
            mine = [k for k in keys if k.startswith(("gru_%s." % e, "mu_%s" % e, "var_%s" % e))]
            for row in range(B):
                gs = torch.autograd.grad((q[row] * ll[row]).sum(), [leaves[k] for k in mine], retain_graph=True, allow_unused=True)
                for k, g in zip(mine, gs):
                    if g is not None:
                        acc[k] += c[row] * g.abs()
        return {k: block_absmax(v.numpy()) for k, v in acc.items()}
    finally:
        torch.set_default_dtype(old)


def gmvae_references(case, step, sd, b, eps, key=None, leak=False):
    """step_references of a GMVAE case: weights sd (CPU float32 state dict), batch dict b, eps = (eps_r, eps_n) CPU float32.  leak: add
    latent_leak_allowance (the cases at which fn_latent_bwd's documented arithmetic exceeds F: f and the c0 fixture, 8 rows each)"""
    key = key or ("gmvae", case["H"], case["B"], case["T"], case["Tr"], case["seed"], case["sup"], step)

    def build(dt):
        grads, tup, _ = orc.gradients({k: v.to(dt) for k, v in sd.items()}, b, eps[0].to(dt), eps[1].to(dt), step, 0.2, is_supervised=case["sup"])
        return grads, tup
    ref = step_references(key, build, b["d"])
    if leak and "leak" not in ref:
        ref["leak"] = latent_leak_allowance(sd, b, eps, step, 0.2, case["sup"])
    return ref


def c0_references(gold, sd, sup=False):
    """step_references at the hidden-512 fixture tests/golden/c0.npz (seeded weights sd, the fixture's batch and eps, step 20000): what the c0 branches
    of test_fused_gradients_vs_reference / test_dropin_forward_backward_vs_reference hand to check_step_grads"""
    from helpers import batch_of
    eps = (torch.from_numpy(gold["eps_r"]), torch.from_numpy(gold["eps_n"]))
    return gmvae_references(dict(sup=sup), 20000, sd, batch_of(gold), eps, key=("c0", sup), leak=True)


def run_c0_case(ops, chunk=32):
    """the stand-in on the c0 fixture's inputs -> (gradients, loss tuple, references, trainer)"""
    from helpers import batch_of, load_golden
    gold = load_golden("c0")
    pkg = load_package()
    m = make_model(int(gold["meta_dims"][0]), int(gold["meta_dims"][1]), ops=ops)
    tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
    m.engine().chunk = chunk
    sd, b = cpu_state(m), batch_of(gold)
    batch = tr.prepare_batch(b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"], None)
    tup = tr.loss_and_grads(20000, batch, (torch.from_numpy(gold["eps_r"]), torch.from_numpy(gold["eps_n"])))
    return flat_grads(tr), tup, c0_references(gold, sd), tr


def gmvae_trainer(case, ops=None, device="cpu", arith=None, **switches):
    """(trainer, engine, batch dict, prepared batch, eps) of a case: seeded weights, synth_batch inputs, eps drawn after manual_seed(99)"""
    pkg = load_package()
    m = make_model(case["H"], case["Z"], device=device, ops=ops, arith=arith)
    tr = pkg.GMVAETrainer(m, lr=1e-3, beta=0.2)
    eng = m.engine()
    eng.chunk, eng.persist_dec = case["chunk"], case["persist"]
    for k, v in switches.items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    b = gmvae_batch(case)
    batch = tr.prepare_batch(b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"], b["a"] if case["sup"] else None)
    torch.manual_seed(99)
    eps = tr.draw_eps(case["B"], case["T"])
    return tr, eng, b, batch, eps


def cpu_state(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def flat_grads(tr):
    return {k: tr.flat.G[k].detach().cpu().numpy().copy() for k in tr.flat.names}


def run_gmvae_case(case, step, ops=None, device="cpu", arith=None, **switches):
    """one loss_and_grads of the case -> (gradients by name, loss tuple, references, trainer)"""
    tr, eng, b, batch, eps = gmvae_trainer(case, ops, device, arith, **switches)
    sd = cpu_state(tr.model)
    tup = tr.loss_and_grads(step, batch, eps)
    ref = gmvae_references(case, step, sd, b, tuple(e.cpu() for e in eps), leak=case["leak"])
    return flat_grads(tr), tup, ref, tr


# ---- siblings --------------------------------------------------------------------------------------------------------------------------------
def _sc(kind, H, Z, B, T, steps, seed=5):
    return dict(id="%s-%d" % (kind, H), kind=kind, H=H, Z=Z, B=B, T=T, Tr=min(T, 8), steps=steps, seed=seed)


SIBLING_CASES = [
    _sc("single", 64, 32, 8, 12, (20000,)), _sc("cvae", 64, 32, 8, 12, (20000,)), _sc("fader", 64, 32, 8, 12, (20000, 500)),
    _sc("vae", 64, 32, 8, 12, (20000,)),
    # the GLSR regulariser decodes 100 teacher-forced steps (trainer_glsr.py:183: T >= 100, GLSRTrainer raises below that): at these T the step that
    # exists is the one with the regulariser off (step <= 20) - GLSRTrainer's own schedule (loss terms on the main lane) on the VAE's engine
    _sc("glsr", 64, 32, 8, 12, (20,)),
    _sc("fader", 512, 128, 256, 8, (20000,)), _sc("glsr", 512, 128, 256, 8, (20,)),
]


def sibling_case(cid):
    return next(c for c in SIBLING_CASES if c["id"] == cid)


def run_sibling_case(case, step, ops=None, device="cpu"):
    """one loss_and_grads of a sibling family -> (gradients by name, loss tuple, references, trainer); eps, dropout masks and GLSR deltas are drawn
    once (the trainer's draw_eps: the oracle's order) and handed to both sides"""
    pkg = load_package()
    from music_fader_nets_amd.synth import synth_batch
    from helpers import SIBLINGS
    from oracle import siblings_oracle as so
    from oracle import vae_oracle as vo
    kind, B, T = case["kind"], case["B"], case["T"]
    if kind in SIBLINGS:
        m = make_sibling(kind, case["H"], case["Z"], device=device, ops=ops)
        tr = getattr(pkg, SIBLINGS[kind][1])(m, lr=1e-3, beta=0.2)
    else:
        m = make_vae_model(case["H"], case["Z"], device=device, ops=ops)
        tr = (pkg.VAETrainer if kind == "vae" else pkg.GLSRTrainer)(m, lr=1e-3, beta=0.2)
    b = synth_batch(np.random.RandomState(case["seed"]), B, T, case["Tr"])
    batch = tr.prepare_batch(b["d"], b["r"], b["n"], b["c"], b["r_density"], b["n_density"])
    torch.manual_seed(99)
    eps = tr.draw_eps(B, T, step=step) if kind == "glsr" else tr.draw_eps(B, T)
    sd = cpu_state(m)
    tup = tr.loss_and_grads(step, batch, eps)
    cpu = lambda x: None if x is None else x.cpu()

    def build(dt):
        w = {k: v.to(dt) for k, v in sd.items()}
        cast = lambda x: None if x is None else cpu(x).to(dt)
        if kind in SIBLINGS:
            grads, t, _ = so.gradients(w, kind, b, cast(eps[0]), cast(eps[1]), step, 0.2)
        elif kind == "vae":
            grads, t, _ = vo.gradients(w, b, cast(eps[0]), cast(eps[1]), 0.2)
        else:
            grads, t, _ = vo.glsr_gradients(w, b, cast(eps[0]), cast(eps[1]), [cast(x) for x in eps[2]], step, 0.2)
        return grads, t
    ref = step_references(("sibling", case["id"], step), build, b["d"])
    return flat_grads(tr), tup, ref, tr
