"""Shared code of tests/test_loss_reference.py (CPU) and tests/test_gpu_loss.py (MI355X): the loss-head kernels of csrc/loss.hip - fn_vocab_logsoftmax,
fn_vocab_logsoftmax_bwd, fn_vocab_argmax, fn_time_logsoftmax (both kernels), fn_time_logsoftmax_bwd, fn_masked_prob, fn_pairwise_reg, fn_adv_head and
fn_onehot_to_index - against float64.  No GPU import: every driver takes the backend (`ops`: HipOps on the GPU, FakeOps or StepOps on the CPU) and the
device as arguments.  fn_vocab_sample has tests/test_gpu_sampling.py; the latent block (fn_latent_fwd, fn_latent_bwd) has tests/helpers_latent.py,
tests/test_latent_reference.py and tests/test_gpu_latent.py, built on this module's layout.

References.  Every *_math function is the documented operation in plain torch on the CPU, in float64 on the float32 inputs (the reference) and, the same
lines, in float32 (the restatement).  StepOps wraps the float32 lines in the signatures of FakeOps / HipOps, so that the restatement - and a planted
fault in it - runs through the same drivers and checkers as the kernels.  Log-softmax quantities follow the steps the ABI documents and the kernels take:
    mx = max x;  s = sum exp(x - mx);  lse = mx + log(s);  l = x - lse
so the absolute error of l is about ulp(|lse|).  torch.log_softmax computes (x - mx) - log(s) and lacks that error; measured against it the kernels
would look up to 31 x worse than "float32" at |lse| = 90 although they are the formula's float32 evaluation.  The ratio against the torch.log_softmax
restatement is reported next to the asserted one, as information.

Metric (helpers_head.tile_errors / worst_ratio).  Every quantity is a 2-D array cut into tiles of 16 rows x tc columns from (0, 0), ragged last tiles:
    err = max |got - ref64| / max |ref64|  over that tile alone,     err <= F x max(e_ref, 2**-23),   e_ref = err of the float32 restatement there.
tc = 16 for matrices, 1 for per-row vectors (nll_rows, loss_rows, dz0), the quantity's own width for nll_bc, sums, o, adversarial loss_rows and da.
F = LOSS_F[family] <= helpers.SCAN_F_CAP (assert_F).  No tile is exempt.

Input conditions.  Every tile maximum of the float64 reference is >= SCAN_MIN_REF - or the case declares the quantity `zero` (E = 1, Tr = 1,
grad_scale = 0, lam_dev = NULL, n_all = 1: the reference is exactly zero) and the kernel's values must then be exactly 0.0.  Single entries the operation
makes exactly zero (nll_bc of a column without a hit, o and da behind a closed gate or a zero mask, the sum of an empty range, dlogits of a -inf logit)
must be exactly 0.0 too.  Where the reference holds -inf (logp of a -inf logit) the kernel must hold -inf at exactly those positions; they are set to
0 in both before the tile metric.  adv_head: |pre| >= 1e-3 in float64 for every (row, attribute) but the planted pre == 0, so that no ReLU gate can
flip on rounding; the seed of a case is the first one for which this holds.  masked_prob stays at randn x 3 logits: at x 8 single range sums fall to
1e-9 of the row, and the float32 restatement of the documented formula itself leaves a margin of only 2 below the bound.

Layout.  Outputs are views of over-allocated buffers filled with the sentinel -123.25 (3 extra rows).  Rows past the last row stay untouched; columns
>= E of dlogits stay untouched (fn_vocab_logsoftmax, fn_vocab_logsoftmax_bwd and fn_masked_prob leave the padding columns alone - unlike
fn_out_head_f32, which zeroes them: helpers_head.check_head_layout); columns >= Z of g_z stay untouched; inputs are not modified unless they alias an
output."""
import zlib

import numpy as np
import torch

from helpers import SCAN_F_CAP, SCAN_MIN_REF
from helpers_head import tile_errors, worst_ratio

SENTINEL = -123.25
INT_SENTINEL = -7
PAD_ROWS = 3
F32, F64 = torch.float32, torch.float64
# F per family: the smallest power of two that is at least 1.5 x the worst ratio measured on an MI355X (profiles/loss_fp64_errors.txt: 3.53, 7.17, 0.65,
# 5.38, 4.52, 10.94, 0.82, 2.03), never above SCAN_F_CAP.  The factor 1.5 is there because e_ref is formed by torch on the CPU that runs the test, and
# its float32 sums and exponentials differ between CPU vector widths; helpers_reduce.ADAM_F (4 for a measured 2.09) keeps the same distance.
LOSS_F = dict(vocab_logsoftmax=8, vocab_logsoftmax_bwd=SCAN_F_CAP, vocab_argmax=1, time_logsoftmax=SCAN_F_CAP, time_logsoftmax_bwd=8, masked_prob=SCAN_F_CAP,
              pairwise_reg=2, adv_head=4)


def assert_F(F):
    assert 0 < F <= SCAN_F_CAP, "F = %r: the margin never exceeds SCAN_F_CAP = %d" % (F, SCAN_F_CAP)
    return F


def f32(x):
    """the value a `float` argument of the C ABI carries"""
    return float(np.float32(x))


def _gen(cid):
    return torch.Generator().manual_seed(zlib.crc32(cid.encode()))


def ceil4(n):
    return (n + 3) // 4 * 4


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.numpy().view(np.int32), b.numpy().view(np.int32))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# references in float64 and the same lines in float32
# ---------------------------------------------------------------------------------------------------------------------------------------------
def lsm_steps(x, dim, drop_last=False):
    """(l, lse) of the documented steps along `dim`; drop_last plants a fault: the last entry along dim is left out of the sum"""
    mx = x.amax(dim, keepdim=True)
    ex = torch.exp(x - mx)
    if drop_last:
        ex = ex.narrow(dim, 0, x.shape[dim] - 1)
    lse = mx + torch.log(ex.sum(dim, keepdim=True))
    return x - lse, lse


def vocab_math(x, target, B, T, gs, dtype, fault=None, lsm="steps"):
    """x [T*B][E] (row = t B + b), target [B][T] or None -> dict(logp [B*T][E] in the order of logp_bt (row = b T + t), nll [R], dlogits [R][E]).
    lsm = "torch": torch.log_softmax instead of the documented steps (information only)"""
    x = x.detach().cpu().to(dtype)
    R, E = x.shape
    assert R == B * T
    if lsm == "torch":
        l = torch.log_softmax(x, 1)
        lse = x[:, :1] - l[:, :1]
    else:
        l, lse = lsm_steps(x, 1, drop_last=fault == "drop_tail_column")
    out = dict(logp=l.clone() if fault == "logp_tb" else l.view(T, B, E).permute(1, 0, 2).reshape(B * T, E).clone())
    if target is not None:
        tg = target.detach().cpu().long()
        tg = (tg.reshape(-1) if fault == "target_tb" else tg.t().reshape(-1)).view(R, 1)          # row t B + b <- target[b][t]
        out["nll"] = (-l.gather(1, tg) if lsm == "torch" else lse - x.gather(1, tg)).reshape(R)
        p = torch.exp(l)
        p.scatter_add_(1, tg, -torch.ones(R, 1, dtype=dtype))
        out["dlogits"] = gs * p
    return out


def vocab_bwd_math(lp_bt, g_bt, dtype):
    """lp_bt, g_bt [B][T][E] -> dlogits [T*B][E] = g - exp(lp) sum_e g"""
    lp, g = lp_bt.detach().cpu().to(dtype), g_bt.detach().cpu().to(dtype)
    B, T, E = lp.shape
    d = g - torch.exp(lp) * g.sum(-1, keepdim=True)
    return dict(dlogits=d.permute(1, 0, 2).reshape(T * B, E).clone())


def first_argmax(x, fault=None):
    """first-index argmax of the rows of a float32 matrix (numpy.argmax: the first occurrence; +0.0 == -0.0); fault "last_index": the last one"""
    x = x.detach().cpu().numpy()
    assert x.dtype == np.float32
    if fault == "last_index":
        return (x.shape[1] - 1 - np.argmax(x[:, ::-1], axis=1)).astype(np.int32)
    return np.argmax(x, axis=1).astype(np.int32)


def argmax_math(x, dtype, lsm="steps"):
    x = x.detach().cpu().to(dtype)
    return dict(logp=torch.log_softmax(x, 1) if lsm == "torch" else lsm_steps(x, 1)[0])


def time_math(x, target, gs, dtype, fault=None, lsm="steps"):
    """x [Tr][B][Cc], target [B][Tr] or None -> dict(logp [B*Tr][Cc] (logp_bt), nll_bc [B][Cc], dlogits [Tr*B][Cc], cnt [B][Cc])"""
    x = x.detach().cpu().to(dtype)
    Tr, B, Cc = x.shape
    l = torch.log_softmax(x, 0) if lsm == "torch" else lsm_steps(x, 0)[0]
    out = dict(logp=l.permute(1, 0, 2).reshape(B * Tr, Cc).clone())
    if target is not None:
        oh = torch.zeros(Tr, B, Cc, dtype=dtype).scatter_(2, target.detach().cpu().long().t().unsqueeze(-1), 1.0)
        out["nll_bc"] = -(l * oh).sum(0)
        cnt = (oh[:Tr - 1] if fault == "cnt_miss_last" else oh).sum(0, keepdim=True)
        out["dlogits"] = (gs * (torch.exp(l) * cnt - oh)).reshape(Tr * B, Cc)
        out["cnt"] = oh.sum(0)
    return out


def time_bwd_math(lp_bt, g_bt, dtype):
    """lp_bt, g_bt [B][Tr][Cc] -> dlogits [Tr*B][Cc] = g - exp(lp) sum_t g"""
    lp, g = lp_bt.detach().cpu().to(dtype), g_bt.detach().cpu().to(dtype)
    B, Tr, Cc = lp.shape
    d = g - torch.exp(lp) * g.sum(1, keepdim=True)
    return dict(dlogits=d.permute(1, 0, 2).reshape(Tr * B, Cc).clone())


def masked_math(x, ranges, w, dtype, fault=None):
    """x [rows][E], w [rows][2] or None -> dict(sums [rows][2], dlogits [rows][E]): p = exp(x - mx) / s, P_a = sum of p over [lo_a, hi_a),
    dlogits_u = p_u (a_u - (w0 P_0 + w1 P_1)).  fault "inclusive_hi": the ranges taken as [lo, hi]"""
    x = x.detach().cpu().to(dtype)
    E = x.shape[1]
    ex = torch.exp(x - x.amax(1, keepdim=True))
    s = ex.sum(1, keepdim=True)
    col = torch.arange(E).view(1, E)
    ins = [((col >= lo) & ((col <= hi) if fault == "inclusive_hi" else (col < hi))).to(dtype) for lo, hi in ranges]
    P = [(ex * m).sum(1, keepdim=True) / s for m in ins]
    out = dict(sums=torch.cat(P, 1))
    if w is not None:
        w = w.detach().cpu().to(dtype)
        dot = w[:, 0:1] * P[0] + w[:, 1:2] * P[1]
        out["dlogits"] = (ex / s) * (ins[0] * w[:, 0:1] + ins[1] * w[:, 1:2] - dot)
    return out


def pairwise_math(z0, attr, row0, nrows, gs, dtype, fault=None):
    """z0 [n_all] fp32, attr [n_all] float64 -> dict(loss_rows [nrows][1], dz0 [nrows][1]); the sign of the attribute difference is taken in float64
    whatever dtype is (fault "sign_f32": of the attributes rounded to float32)"""
    z = z0.detach().cpu().to(dtype)
    a = attr.detach().cpu()
    assert a.dtype == F64
    if fault == "sign_f32":
        a = a.float().double()
    th = torch.tanh(z[row0:row0 + nrows].view(-1, 1) - z.view(1, -1))
    sg = torch.sign(a[row0:row0 + nrows].view(-1, 1) - a.view(1, -1)).to(dtype)
    df = th - sg
    return dict(loss_rows=(df * df).sum(1, keepdim=True), dz0=gs * 4.0 * (df * (1.0 - th * th)).sum(1, keepdim=True))


def adv_math(inp, lam, g0, dtype, fault=None):
    """inp: dict(z [B][Z], w_r, w_n [Z], b_r, b_n [1], mask, dens [B][2], inv_bg); lam: float or None; g0 [B][Z] or None ->
    dict(pre, o, loss_rows, da [B][2], g_z [B][Z]).  faults: "gate_ge" (the gate as pre >= 0), "gz_add" (g_z += instead of -=)"""
    c = lambda t: t.detach().cpu().to(dtype)                      # noqa: E731
    z, w_r, w_n = c(inp["z"]), c(inp["w_r"]).view(-1), c(inp["w_n"]).view(-1)
    mask, dens = c(inp["mask"]), c(inp["dens"])
    pre = torch.stack([z @ w_r + c(inp["b_r"]).view(()), z @ w_n + c(inp["b_n"]).view(())], 1)
    o = torch.relu(pre) * mask
    df = o - dens
    gate = ((pre >= 0) if fault == "gate_ge" else (pre > 0)).to(dtype)
    da = (0.0 if lam is None else lam) * 2.0 * df * inp["inv_bg"] * mask * gate
    out = dict(pre=pre, o=o, loss_rows=df * df, da=da)
    if g0 is not None:
        upd = da[:, 0:1] * w_r.view(1, -1) + da[:, 1:2] * w_n.view(1, -1)
        out["g_z"] = c(g0) + upd if fault == "gz_add" else c(g0) - upd
    return out


class StepOps:
    """the float32 restatement behind the backend's signatures (the methods of HipOps that this module drives).  `fault` plants one fault:
    drop_tail_column | logp_tb | target_tb | cnt_miss_last | last_index | inclusive_hi | sign_f32 | gate_ge | gz_add | pad_write | nan"""
    name = "steps-f32"

    def __init__(self, fault=None):
        self.fault = fault

    def _spoil(self, t, E):
        if self.fault == "pad_write" and t.shape[1] > E:
            t[:, E:] = 0.0
        if self.fault == "nan":
            t[t.shape[0] // 2, E // 2] = float("nan")

    def vocab_logsoftmax(self, logits, B, T, E, logp_bt=None, target=None, nll_rows=None, grad_scale=0.0, dlogits=None):
        out = vocab_math(logits[:, :E], target, B, T, f32(grad_scale), F32, self.fault)
        if logp_bt is not None:
            logp_bt.copy_(out["logp"].view(B, T, E))
        if nll_rows is not None:
            nll_rows.copy_(out["nll"])
        if dlogits is not None:
            dlogits[:, :E].copy_(out["dlogits"])
            self._spoil(dlogits, E)

    def vocab_logsoftmax_bwd(self, logp_bt, gout_bt, dlogits):
        E = logp_bt.shape[2]
        dlogits[:, :E].copy_(vocab_bwd_math(logp_bt, gout_bt, F32)["dlogits"])
        self._spoil(dlogits, E)

    def vocab_argmax(self, logits, E, logp_out, tok_out):
        x = logits[:, :E].contiguous()
        if logp_out is not None:
            logp_out.copy_(argmax_math(x, F32)["logp"])
        tok_out.copy_(torch.from_numpy(first_argmax(x, self.fault)))

    def time_logsoftmax(self, logits, logp_bt=None, target=None, nll_bc=None, grad_scale=0.0, dlogits=None):
        Tr, B, Cc = logits.shape
        out = time_math(logits, target, f32(grad_scale), F32, self.fault)
        if logp_bt is not None:
            logp_bt.copy_(out["logp"].view(B, Tr, Cc))
        if nll_bc is not None:
            nll_bc.copy_(out["nll_bc"])
        if dlogits is not None:
            dlogits.copy_(out["dlogits"].view(Tr, B, Cc))

    def time_logsoftmax_bwd(self, logp_bt, gout_bt, dlogits):
        dlogits.copy_(time_bwd_math(logp_bt, gout_bt, F32)["dlogits"].view_as(dlogits))

    def masked_prob(self, logits, E, ranges, sums=None, w=None, dlogits=None):
        out = masked_math(logits[:, :E], ranges, w if dlogits is not None else None, F32, self.fault)
        if sums is not None:
            sums.copy_(out["sums"])
        if dlogits is not None:
            dlogits[:, :E].copy_(out["dlogits"])
            self._spoil(dlogits, E)

    def pairwise_reg(self, z0_all, attr_all, row0, nrows, loss_rows, grad_scale=0.0, dz0=None):
        out = pairwise_math(z0_all, attr_all, row0, nrows, f32(grad_scale), F32, self.fault)
        loss_rows.copy_(out["loss_rows"].view(-1))
        if dz0 is not None:
            dz0.copy_(out["dz0"].view(-1))

    def adv_head(self, z, w_r, w_n, b_r, b_n, mask, dens, lam_dev, inv_global_batch, o, loss_rows, da=None, g_z=None):
        Z = w_r.numel()
        inp = dict(z=z[:, :Z], w_r=w_r, w_n=w_n, b_r=b_r, b_n=b_n, mask=mask, dens=dens, inv_bg=f32(inv_global_batch))
        out = adv_math(inp, None if lam_dev is None else float(lam_dev[0]), None if g_z is None else g_z[:, :Z], F32, self.fault)
        o.copy_(out["o"]), loss_rows.copy_(out["loss_rows"])
        if da is not None:
            da.copy_(out["da"])
        if g_z is not None:
            g_z[:, :Z].copy_(out["g_z"])

    def onehot_to_index(self, oh, idx):
        idx.copy_(torch.from_numpy(first_argmax(oh.reshape(-1, oh.shape[-1]), self.fault)).view_as(idx))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the tile metric
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _clean(t, ninf):
    return torch.where(ninf, torch.zeros((), dtype=t.dtype), t)


def make_refs(cid, ref64, fake32, tc, zero=(), torch32=None, exact0=None):
    """the cached record of a case: ref64 / fake32 {quantity: 2-D tensor} in float64 / float32, e_ref = tile_errors(fake32, ref64) per quantity,
    e_torch the same for the torch.log_softmax restatement (information), exact0 {quantity: bool mask of entries that are exactly zero by the
    operation itself}.  Asserts the input conditions."""
    res = dict(id=cid, ref64=ref64, fake32=fake32, tc=tc, zero=tuple(zero), e_ref={}, e_torch={}, den={}, ninf={}, exact0=exact0 or {})
    for k, r in ref64.items():
        f = fake32[k]
        assert r.dtype == F64 and f.dtype == F32 and r.dim() == 2 and r.shape == f.shape, (cid, k, r.dtype, f.dtype, tuple(r.shape), tuple(f.shape))
        ninf = torch.isneginf(r)
        assert torch.equal(torch.isneginf(f), ninf), "%s %s: the restatement's -inf are not the reference's" % (cid, k)
        r0 = _clean(r, ninf)
        assert bool(torch.isfinite(r0).all()), (cid, k)
        e, den = tile_errors(_clean(f, ninf), r0, tc=tc[k])
        if k in zero:
            assert den.max() == 0.0 and e.max() == 0.0, "%s %s: declared exactly zero, but the reference or the restatement is not" % (cid, k)
        else:
            assert den.min() >= SCAN_MIN_REF, "input condition: %s %s has a tile maximum of %.3e < 2**-100" % (cid, k, den.min())
            assert np.isfinite(e).all(), (cid, k)
        if k in res["exact0"]:
            m = res["exact0"][k]
            assert m.shape == r.shape and bool((r[m] == 0).all()) and bool((f[m] == 0).all()), (cid, k)
        res["e_ref"][k], res["den"][k], res["ninf"][k] = e, den, ninf
        if torch32 is not None and k in torch32:
            t = torch32[k]
            assert t.dtype == F32 and torch.equal(torch.isneginf(t), ninf)
            res["e_torch"][k] = tile_errors(_clean(t, ninf), r0, tc=tc[k])[0]
    res["ref0"] = {k: _clean(r, res["ninf"][k]) for k, r in ref64.items()}
    return res


def check_quantities(refs, got, F):
    """got {quantity: 2-D float32 CPU tensor} of one launch against the record of its case: -inf positions, exact zeros, then the tile bound in EVERY
    tile.  A quantity the reference has and `got` lacks is an error.  Returns (worst ratio, quantity, tile row, tile column, the worst ratio of
    the log-softmax quantities against the torch.log_softmax restatement or None)."""
    assert_F(F)
    cid, worst, info, bad = refs["id"], (0.0, "-", 0, 0), None, []
    for k, r0 in refs["ref0"].items():
        g = got.get(k)
        assert g is not None, "%s: output %s missing" % (cid, k)
        g = g.detach().cpu()
        assert g.dtype == F32 and g.shape == r0.shape, (cid, k, g.dtype, tuple(g.shape), tuple(r0.shape))
        ninf = refs["ninf"][k]
        wrong = torch.isneginf(g) != ninf
        assert not bool(wrong.any()), "%s %s: -inf expected at exactly the reference's positions, first difference at %s" % (cid, k, tuple(int(v) for v in torch.nonzero(wrong)[0]))
        g0 = _clean(g, ninf)
        if k in refs["zero"]:
            nz = g0 != 0
            assert not bool(nz.any()), "%s %s: exactly zero by the operation, got %r at %s" % (cid, k, float(g0[nz][0]), tuple(int(v) for v in torch.nonzero(nz)[0]))
            continue
        if k in refs["exact0"]:
            nz = refs["exact0"][k] & (g0 != 0)
            assert not bool(nz.any()), "%s %s: entry %s is exactly zero by the operation, got %r" % (cid, k, tuple(int(v) for v in torch.nonzero(nz)[0]), float(g0[nz][0]))
        e, den = tile_errors(g0, r0, tc=refs["tc"][k])
        r, i, j, n = worst_ratio(e, refs["e_ref"][k], F)
        if r > worst[0]:
            worst = (r, k, i, j)
        if k in refs["e_torch"]:
            info = max(info or 0.0, worst_ratio(e, refs["e_torch"][k], F)[0])
        if not r <= F:
            bad.append("%s %s: err %.3e = %.1f x max(e_ref %.3e, 2**-23) in tile (rows %d.., columns %d..), tile max of the reference %.3e; %d of %d tiles over F = %g" % (
                cid, k, e[i, j], r, refs["e_ref"][k][i, j], 16 * i, refs["tc"][k] * j, den[i, j], n, e.size, F))
    assert not bad, "\n".join(bad)
    return worst + (info,)


def check_sentinel(cid, what, t, value=SENTINEL):
    assert t.numel() == 0 or bool((t.detach().cpu() == value).all()), "%s: %s was written" % (cid, what)


def old_metric_accepts(got, ref, tol=2e-5):
    """what test_head_kernels asks of dlogits: close(..., 2e-5) = max |got - ref| < 2e-5 of the WHOLE tensor's maximum"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max()) / max(1e-12, float(ref.abs().max())) < tol


def line(kernel, cid, worst):
    """one line of profiles/loss_fp64_errors.txt"""
    s = "[loss] %-19s %-46s ratio %6.3f  %-9s tile (%d, %d)" % (kernel, cid, worst[0], worst[1], worst[2], worst[3])
    if len(worst) > 4 and worst[4] is not None:
        s += "  vs torch.log_softmax in fp32: %7.3f" % worst[4]
    return s + "  (F = %d)" % LOSS_F[kernel]


def exact_line(kernel, cid, what="bit-exact"):
    return "[loss] %-19s %-46s %s" % (kernel, cid, what)


def _buf(shape, device, dtype=F32):
    return torch.full(tuple(shape), SENTINEL if dtype == F32 else INT_SENTINEL, dtype=dtype, device=device)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# vocab_logsoftmax, vocab_logsoftmax_bwd
# ---------------------------------------------------------------------------------------------------------------------------------------------
VOCAB_GS = 0.37
VOCAB_ROWS = ((7, 23), (1, 1), (3, 1), (1, 5), (5, 13), (2, 3), (4, 2))
VOCAB_E = (1, 2, 63, 64, 65, 128, 129, 342, 385, 1024)
VOCAB_FORMS = ("lp", "nll", "dl", "all", "alias", "gs0")
VOCAB_KINDS = ("randn3", "p90", "m90", "ninf", "lowp")
VOCAB_WANTED = dict(lp=("logp",), nll=("nll",), dl=("dlogits",), all=("logp", "nll", "dlogits"), alias=("logp", "nll", "dlogits"), gs0=("logp", "nll", "dlogits"))
VOCAB_TC = dict(logp=16, nll=1, dlogits=16)


def _vc(B, T, E, ld=None, form="all", kind="randn3"):
    """form: lp (logp only, no target) | nll | dl | all | alias (all three, dlogits written over the logits) | gs0 (all three, grad_scale = 0);
    kind: randn3 | p90 / m90 (randn x 3 +- 90: without the max subtraction the sum of expf overflows / falls to 1e-30) | ninf (one -inf logit per row, never the
    target) | lowp (columns 32..47 twelve units down, none of them a target)"""
    ld = ceil4(E) if ld is None else ld
    want = VOCAB_WANTED[form]
    zero = want if E == 1 else ("dlogits",) if form == "gs0" else ()
    return dict(id="B%d-T%d-E%d-ld%d-%s-%s" % (B, T, E, ld, form, kind), B=B, T=T, E=E, ld=ld, form=form, kind=kind, zero=tuple(zero))


VOCAB_CASES = [_vc(B, T, 342) for B, T in VOCAB_ROWS]
VOCAB_CASES += [_vc(7, 23, E) for E in VOCAB_E if E != 342] + [_vc(7, 23, 342, ld=346)]
VOCAB_CASES += [_vc(7, 23, 342, form=f) for f in VOCAB_FORMS if f != "all"]
VOCAB_CASES += [_vc(7, 23, 342, kind=k) for k in VOCAB_KINDS if k != "randn3"]
VOCAB_BY_ID = {c["id"]: c for c in VOCAB_CASES}
assert len(VOCAB_BY_ID) == len(VOCAB_CASES)
VOCAB_BWD_CASES = [c for c in VOCAB_CASES if c["form"] == "all"]


def vocab_grad_scale(case):
    return 0.0 if case["form"] == "gs0" else f32(VOCAB_GS)


def vocab_inputs(case):
    """dict(x [T*B][E] fp32, target [B][T] int32 with every seventh position pinned to column 0 and the next one to column E - 1 (as
    helpers_head.head_inputs), gout [B][T][E]) from the generator seeded with crc32(id)"""
    B, T, E, kind = case["B"], case["T"], case["E"], case["kind"]
    gen = _gen("vocab/" + case["id"])
    x = torch.randn(B * T, E, generator=gen) * 3
    tgt = torch.randint(0, E, (B, T), generator=gen, dtype=torch.int32)
    gout = torch.randn(B, T, E, generator=gen)
    pos = torch.arange(B * T).view(B, T)
    tgt[pos % 7 == 0] = 0
    tgt[pos % 7 == 1] = E - 1
    if kind == "p90":
        x += 90.0
    elif kind == "m90":
        x -= 90.0
    elif kind == "lowp":
        x[:, 32:48] -= 12.0
        tgt[(tgt >= 32) & (tgt < 48)] += 16
    elif kind == "ninf":
        assert E >= 3
        row = torch.arange(B * T)
        tg_row = tgt.long().t().reshape(-1)
        col = (5 * row + 3) % E
        col = torch.where(col == tg_row, (col + 1) % E, col)
        x[row, col] = float("-inf")
    else:
        assert kind == "randn3"
    return dict(x=x, target=tgt, gout=gout)


_VOCAB_CACHE, _VOCAB_BWD_CACHE = {}, {}


def vocab_references(case):
    if case["id"] not in _VOCAB_CACHE:
        inp, want = vocab_inputs(case), VOCAB_WANTED[case["form"]]
        tgt = None if case["form"] == "lp" else inp["target"]
        o = {n: vocab_math(inp["x"], tgt, case["B"], case["T"], vocab_grad_scale(case), dt, lsm=m) for n, dt, m in (("ref64", F64, "steps"), ("fake32", F32, "steps"), ("torch32", F32, "torch"))}
        pick = lambda d: {k: (v if v.dim() == 2 else v.view(-1, 1)) for k, v in d.items() if k in want}      # noqa: E731
        exact0 = {}
        if "dlogits" in want:
            exact0["dlogits"] = torch.isneginf(inp["x"])              # gs (exp(-inf) - 0)
        rec = make_refs(case["id"], pick(o["ref64"]), pick(o["fake32"]), VOCAB_TC, case["zero"], pick(o["torch32"]), exact0)
        rec["inputs"] = inp
        _VOCAB_CACHE[case["id"]] = rec
    return _VOCAB_CACHE[case["id"]]


def run_vocab(ops, case, device="cpu", form=None):
    """one launch of ops.vocab_logsoftmax in the case's form (or `form`).  Returns the sentinel-filled buffers on the CPU:
    dict(logits [R + 3][ld], logp [(R + 3) E] | None, nll [R + 3] | None, dlogits [R + 3][ld] | None (the logits buffer itself when aliased))"""
    form = case["form"] if form is None else form
    inp, B, T, E, ld = vocab_inputs(case), case["B"], case["T"], case["E"], case["ld"]
    R, want = B * T, VOCAB_WANTED[form]
    lbuf = _buf((R + PAD_ROWS, ld), device)
    lbuf[:R, :E] = inp["x"].to(device)
    lp = _buf(((R + PAD_ROWS) * E,), device) if "logp" in want else None
    nll = _buf((R + PAD_ROWS,), device) if "nll" in want else None
    dl = None if "dlogits" not in want else lbuf if form == "alias" else _buf((R + PAD_ROWS, ld), device)
    ops.vocab_logsoftmax(lbuf[:R], B, T, E, logp_bt=None if lp is None else lp[:R * E].view(B, T, E), target=None if form == "lp" else inp["target"].to(device),
                         nll_rows=None if nll is None else nll[:R], grad_scale=0.0 if form == "gs0" else VOCAB_GS, dlogits=None if dl is None else dl[:R])
    c = lambda t: None if t is None else t.cpu()                  # noqa: E731
    return dict(form=form, logits=c(lbuf), logp=c(lp), nll=c(nll), dlogits=c(dl))


def check_vocab(case, bufs, F=None):
    """layout, -inf positions, exact zeros, then the tile bound.  Returns check_quantities' worst"""
    F = LOSS_F["vocab_logsoftmax"] if F is None else F
    rec, cid, B, T, E, ld = vocab_references(case), case["id"], case["B"], case["T"], case["E"], case["ld"]
    R, want = B * T, VOCAB_WANTED[case["form"]]
    assert VOCAB_WANTED[bufs["form"]] == want
    got = {}
    if bufs["form"] != "alias":
        ref_l = torch.full((R + PAD_ROWS, ld), SENTINEL)
        ref_l[:R, :E] = rec["inputs"]["x"]
        assert bits_equal(bufs["logits"], ref_l), "%s: the logits were modified" % cid
    if "logp" in want:
        assert tuple(bufs["logp"].shape) == ((R + PAD_ROWS) * E,)
        check_sentinel(cid, "logp_bt past its last row", bufs["logp"][R * E:])
        got["logp"] = bufs["logp"][:R * E].view(R, E)
    if "nll" in want:
        check_sentinel(cid, "nll_rows past its last row", bufs["nll"][R:])
        got["nll"] = bufs["nll"][:R].view(R, 1)
    if "dlogits" in want:
        assert tuple(bufs["dlogits"].shape) == (R + PAD_ROWS, ld)
        check_sentinel(cid, "a row of dlogits past the last row", bufs["dlogits"][R:])
        check_sentinel(cid, "a padding column (>= E) of dlogits", bufs["dlogits"][:R, E:])
        got["dlogits"] = bufs["dlogits"][:R, :E]
    return check_quantities(rec, got, F)


def vocab_bwd_references(case):
    """inputs: logp_bt = the float32 restatement's forward logp of the case, gout = randn"""
    if case["id"] not in _VOCAB_BWD_CACHE:
        inp, B, T, E = vocab_inputs(case), case["B"], case["T"], case["E"]
        lp = vocab_math(inp["x"], None, B, T, 0.0, F32)["logp"].view(B, T, E).contiguous()
        rec = make_refs("bwd-" + case["id"], vocab_bwd_math(lp, inp["gout"], F64), vocab_bwd_math(lp, inp["gout"], F32), VOCAB_TC, ("dlogits",) if E == 1 else ())
        rec["inputs"] = dict(logp=lp, gout=inp["gout"])
        _VOCAB_BWD_CACHE[case["id"]] = rec
    return _VOCAB_BWD_CACHE[case["id"]]


def run_vocab_bwd(ops, case, device="cpu"):
    rec, R, ld = vocab_bwd_references(case), case["B"] * case["T"], case["ld"]
    dl = _buf((R + PAD_ROWS, ld), device)
    lp, go = rec["inputs"]["logp"].to(device), rec["inputs"]["gout"].to(device)
    ops.vocab_logsoftmax_bwd(lp, go, dl[:R])
    assert bits_equal(lp, rec["inputs"]["logp"]) and bits_equal(go, rec["inputs"]["gout"]), "%s: an input was modified" % case["id"]
    return dict(dlogits=dl.cpu())


def check_vocab_bwd(case, bufs, F=None):
    F = LOSS_F["vocab_logsoftmax_bwd"] if F is None else F
    rec, R, E = vocab_bwd_references(case), case["B"] * case["T"], case["E"]
    check_sentinel(rec["id"], "a row of dlogits past the last row", bufs["dlogits"][R:])
    check_sentinel(rec["id"], "a padding column (>= E) of dlogits", bufs["dlogits"][:R, E:])
    return check_quantities(rec, dict(dlogits=bufs["dlogits"][:R, :E]), F)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# vocab_argmax
# ---------------------------------------------------------------------------------------------------------------------------------------------
ARGMAX_B = (1, 3, 4, 13)
ARGMAX_E = (1, 63, 64, 65, 342, 1024)
ARGMAX_KINDS = ("tie-same-lane", "tie-across-lanes", "tie-first-last", "signed-zeros", "constant", "some-ninf", "all-but-one-ninf")
ARGMAX_CASES = [dict(id="B%d-E%d-ld%d-%s" % (B, E, ceil4(E), "logp" if lp else "nologp"), B=B, E=E, ld=ceil4(E), logp=lp, zero=("logp",) if E == 1 else ())
                for B in ARGMAX_B for E in ARGMAX_E for lp in (True, False)]


def argmax_row_kind(B, r):
    """the planted kind of row r of a B-row case, or None (randn x 3): B = 13 holds every kind, the smaller B a window of them"""
    k = (r + B) % 13
    return ARGMAX_KINDS[k] if k < len(ARGMAX_KINDS) else None


def argmax_inputs(case):
    """dict(x [B][E] fp32, expect {row: token} of the planted rows whose answer is known by construction)"""
    B, E = case["B"], case["E"]
    x = torch.randn(B, E, generator=_gen("argmax/B%d-E%d" % (B, E))) * 3
    expect = {}
    for r in range(B):
        kind = argmax_row_kind(B, r)
        if kind == "tie-same-lane" and E > 69:
            x[r, 5] = x[r, 69] = 50.0                              # lane 5 holds both: its own loop keeps the first
            expect[r] = 5
        elif kind == "tie-across-lanes" and E > 41:
            x[r, 41] = x[r, 10] = 50.0                             # lanes 41 and 10 meet in the xor tree
            expect[r] = 10
        elif kind == "tie-first-last":
            x[r, 0] = x[r, E - 1] = 50.0
            expect[r] = 0
        elif kind == "signed-zeros" and E > 7:
            x[r] = -x[r].abs() - 1.0
            x[r, 2], x[r, 7] = -0.0, 0.0                           # -0.0 == +0.0: the first index wins
            expect[r] = 2
        elif kind == "constant":
            x[r] = 1.25
            expect[r] = 0
        elif kind == "some-ninf":
            x[r, ::3] = float("-inf")
            if E == 1:
                x[r, 0] = 0.5                                      # a row of -inf alone has no log-softmax
        elif kind == "all-but-one-ninf":
            keep = float(x[r, E // 2])
            x[r] = float("-inf")
            x[r, E // 2] = keep
            expect[r] = E // 2
    return dict(x=x, expect=expect)


_ARGMAX_CACHE = {}


def argmax_references(case):
    key = (case["B"], case["E"])
    if key not in _ARGMAX_CACHE:
        inp = argmax_inputs(case)
        tok = first_argmax(inp["x"])
        for r, t in inp["expect"].items():
            assert int(tok[r]) == t, (case["id"], r, int(tok[r]), t)
        o = {n: argmax_math(inp["x"], dt, m) for n, dt, m in (("ref64", F64, "steps"), ("fake32", F32, "steps"), ("torch32", F32, "torch"))}
        rec = make_refs("B%d-E%d" % key, o["ref64"], o["fake32"], dict(logp=16), case["zero"], o["torch32"])
        rec["inputs"], rec["tokens"] = inp, tok
        _ARGMAX_CACHE[key] = rec
    return _ARGMAX_CACHE[key]


def run_argmax(ops, case, device="cpu"):
    """logp_out and tok_out as the strided views lp[:, 2, :] and tok[:, 2] of sentinel-filled [B + 3][4][E] / [B + 3][4] buffers"""
    B, E, ld = case["B"], case["E"], case["ld"]
    x = argmax_references(case)["inputs"]["x"]
    lbuf = _buf((B + PAD_ROWS, ld), device)
    lbuf[:B, :E] = x.to(device)
    lp = _buf((B + PAD_ROWS, 4, E), device) if case["logp"] else None
    tok = _buf((B + PAD_ROWS, 4), device, torch.int32)
    ops.vocab_argmax(lbuf[:B], E, None if lp is None else lp[:B, 2, :], tok[:B, 2])
    return dict(logits=lbuf.cpu(), logp=None if lp is None else lp.cpu(), tok=tok.cpu())


def check_argmax(case, bufs, F=None):
    """tokens equal the first-index argmax of the float32 logits exactly; logp within the tile bound, -inf where the logit is -inf"""
    F = LOSS_F["vocab_argmax"] if F is None else F
    rec, cid, B, E = argmax_references(case), case["id"], case["B"], case["E"]
    ref_l = torch.full((B + PAD_ROWS, case["ld"]), SENTINEL)
    ref_l[:B, :E] = rec["inputs"]["x"]
    assert bits_equal(bufs["logits"], ref_l), "%s: the logits were modified" % cid
    tok = bufs["tok"]
    keep = torch.ones_like(tok, dtype=torch.bool)
    keep[:B, 2] = False
    check_sentinel(cid, "tok_out outside its strided view", tok[keep], INT_SENTINEL)
    got = tok[:B, 2].numpy()
    bad = np.nonzero(got != rec["tokens"])[0]
    assert bad.size == 0, "%s: row %d (%s) token %d, the first-index argmax is %d" % (cid, bad[0], argmax_row_kind(B, int(bad[0])), got[bad[0]], rec["tokens"][bad[0]])
    if not case["logp"]:
        assert bufs["logp"] is None
        return (0.0, "-", 0, 0, None)
    lp = bufs["logp"]
    keep = torch.ones_like(lp, dtype=torch.bool)
    keep[:B, 2, :] = False
    check_sentinel(cid, "logp_out outside its strided view", lp[keep])
    return check_quantities(rec, dict(logp=lp[:B, 2, :].contiguous()), F)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# time_logsoftmax (wave kernel for Tr <= 64, loop kernel above), time_logsoftmax_bwd
# ---------------------------------------------------------------------------------------------------------------------------------------------
TIME_GS = 0.11
TIME_WAVE_MAX = 64
TIME_SHAPES = ((1, 3, 3), (2, 9, 3), (63, 9, 3), (64, 9, 3), (65, 9, 3), (70, 5, 5), (33, 9, 16), (8, 1, 16), (64, 86, 3))
TIME_TC = dict(logp=16, dlogits=16)
TIME_WANTED = dict(eval=("logp",), train=("logp", "nll_bc", "dlogits"))


def time_kernel(Tr):
    """the dispatch of fn_time_logsoftmax restated"""
    return "time_logsoftmax_wave_kernel" if Tr <= TIME_WAVE_MAX else "time_logsoftmax_kernel"


def time_grid(Tr, B, Cc):
    """(workgroups, columns the last workgroup's threads / wavefronts find past B Cc)"""
    n = B * Cc
    per = 4 if Tr <= TIME_WAVE_MAX else 256
    return (n + per - 1) // per, -n % per


TIME_CASES = [dict(id="Tr%d-B%d-C%d-%s-%s" % (Tr, B, Cc, "wave" if Tr <= TIME_WAVE_MAX else "loop", form), Tr=Tr, B=B, Cc=Cc, form=form,
                   zero=TIME_WANTED[form] if Tr == 1 else ()) for Tr, B, Cc in TIME_SHAPES for form in ("eval", "train")]
TIME_BY_ID = {c["id"]: c for c in TIME_CASES}
TIME_BWD_CASES = [c for c in TIME_CASES if c["form"] == "train"]


def time_inputs(case):
    """dict(x [Tr][B][Cc] = randn x 2, target [B][Tr]: b = 0 points at class 0 in every step (column (0, 0) has every hit, the other columns of
    b = 0 none), gout [B][Tr][Cc]); the shape alone seeds it: both forms of a shape share their inputs"""
    Tr, B, Cc = case["Tr"], case["B"], case["Cc"]
    gen = _gen("time/Tr%d-B%d-C%d" % (Tr, B, Cc))
    x = torch.randn(Tr, B, Cc, generator=gen) * 2
    tgt = torch.randint(0, Cc, (B, Tr), generator=gen, dtype=torch.int32)
    tgt[0] = 0
    return dict(x=x, target=tgt, gout=torch.randn(B, Tr, Cc, generator=gen))


_TIME_CACHE, _TIME_BWD_CACHE = {}, {}


def time_references(case):
    if case["id"] not in _TIME_CACHE:
        inp, want = time_inputs(case), TIME_WANTED[case["form"]]
        tgt = inp["target"] if case["form"] == "train" else None
        o = {n: time_math(inp["x"], tgt, f32(TIME_GS), dt, lsm=m) for n, dt, m in (("ref64", F64, "steps"), ("fake32", F32, "steps"), ("torch32", F32, "torch"))}
        pick = lambda d: {k: v for k, v in d.items() if k in want}      # noqa: E731
        exact0 = {}
        if tgt is not None:
            cnt = o["ref64"]["cnt"]
            assert bool((cnt[0, 0] == case["Tr"])) and bool((cnt[0, 1:] == 0).all())
            exact0["nll_bc"] = cnt == 0
            exact0["dlogits"] = (cnt == 0).unsqueeze(0).expand(case["Tr"], -1, -1).reshape(-1, case["Cc"])
        rec = make_refs(case["id"], pick(o["ref64"]), pick(o["fake32"]), dict(TIME_TC, nll_bc=case["Cc"]), case["zero"], pick(o["torch32"]), exact0)
        rec["inputs"] = inp
        _TIME_CACHE[case["id"]] = rec
    return _TIME_CACHE[case["id"]]


def run_time(ops, case, device="cpu", x=None):
    """one launch of ops.time_logsoftmax in the case's form on the case's inputs (or on x [Tr'][B][Cc], eval form).  Buffers on the CPU"""
    inp, B, Cc, train = time_inputs(case), case["B"], case["Cc"], case["form"] == "train" and x is None
    x = inp["x"] if x is None else x
    Tr = x.shape[0]
    xd = x.to(device)
    lp = _buf(((B * Tr + PAD_ROWS) * Cc,), device)
    nll = _buf((B + PAD_ROWS, Cc), device) if train else None
    dl = _buf((Tr + PAD_ROWS, B, Cc), device) if train else None
    if train:
        ops.time_logsoftmax(xd, lp[:B * Tr * Cc].view(B, Tr, Cc), inp["target"].to(device), nll[:B], TIME_GS, dl[:Tr])
    else:
        ops.time_logsoftmax(xd, logp_bt=lp[:B * Tr * Cc].view(B, Tr, Cc))
    assert bits_equal(xd, x), "%s: the logits were modified" % case["id"]
    c = lambda t: None if t is None else t.cpu()                  # noqa: E731
    return dict(logp=c(lp), nll_bc=c(nll), dlogits=c(dl))


def check_time(case, bufs, F=None):
    F = LOSS_F["time_logsoftmax"] if F is None else F
    rec, cid, Tr, B, Cc = time_references(case), case["id"], case["Tr"], case["B"], case["Cc"]
    check_sentinel(cid, "logp_bt past its end", bufs["logp"][B * Tr * Cc:])
    got = dict(logp=bufs["logp"][:B * Tr * Cc].view(B * Tr, Cc))
    if case["form"] == "train":
        check_sentinel(cid, "nll_bc past its last row", bufs["nll_bc"][B:])
        check_sentinel(cid, "dlogits past its last step", bufs["dlogits"][Tr:])
        got["nll_bc"], got["dlogits"] = bufs["nll_bc"][:B], bufs["dlogits"][:Tr].reshape(Tr * B, Cc)
    return check_quantities(rec, got, F)


IDENTITY_CASE = "Tr64-B9-C3-wave-eval"
IDENTITY_LAST = -1.0e4


def time_identity_inputs():
    """(case of Tr = 64, x65): x65 = the case's 64 steps and a 65th of -1e4.  The maximum is unchanged and expf(-1e4 - mx) is exactly 0, so the
    loop kernel adds 0 to the same sum in the same order: its logp_bt[:, :64, :] must be the wave kernel's logp_bt bit for bit"""
    case = TIME_BY_ID[IDENTITY_CASE]
    x = time_inputs(case)["x"]
    assert x.shape[0] == TIME_WAVE_MAX and float(x.min()) > -100.0
    x65 = torch.cat([x, torch.full((1,) + tuple(x.shape[1:]), IDENTITY_LAST)], 0)
    assert time_kernel(64) != time_kernel(65) and float(torch.exp(torch.tensor(IDENTITY_LAST) - x.amax())) == 0.0
    return case, x65


def time_identity_views(case, b64, b65):
    """the two [B][64][Cc] arrays to compare"""
    B, Cc = case["B"], case["Cc"]
    return b64["logp"][:B * 64 * Cc].view(B, 64, Cc), b65["logp"][:B * 65 * Cc].view(B, 65, Cc)[:, :64, :]


def time_bwd_references(case):
    """inputs: logp_bt = the float32 restatement's forward logp of the case, gout = randn"""
    if case["id"] not in _TIME_BWD_CACHE:
        inp, Tr, B, Cc = time_inputs(case), case["Tr"], case["B"], case["Cc"]
        lp = time_math(inp["x"], None, 0.0, F32)["logp"].view(B, Tr, Cc).contiguous()
        rec = make_refs("bwd-" + case["id"], time_bwd_math(lp, inp["gout"], F64), time_bwd_math(lp, inp["gout"], F32), TIME_TC, ("dlogits",) if Tr == 1 else ())
        rec["inputs"] = dict(logp=lp, gout=inp["gout"])
        _TIME_BWD_CACHE[case["id"]] = rec
    return _TIME_BWD_CACHE[case["id"]]


def run_time_bwd(ops, case, device="cpu"):
    rec, Tr, B, Cc = time_bwd_references(case), case["Tr"], case["B"], case["Cc"]
    dl = _buf((Tr + PAD_ROWS, B, Cc), device)
    ops.time_logsoftmax_bwd(rec["inputs"]["logp"].to(device), rec["inputs"]["gout"].to(device), dl[:Tr])
    return dict(dlogits=dl.cpu())


def check_time_bwd(case, bufs, F=None):
    F = LOSS_F["time_logsoftmax_bwd"] if F is None else F
    rec, Tr = time_bwd_references(case), case["Tr"]
    check_sentinel(rec["id"], "dlogits past its last step", bufs["dlogits"][Tr:])
    return check_quantities(rec, dict(dlogits=bufs["dlogits"][:Tr].reshape(Tr * case["B"], case["Cc"])), F)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# masked_prob
# ---------------------------------------------------------------------------------------------------------------------------------------------
MASKED_ROWS = (1, 5, 203)
MASKED_E = (65, 342)
MASKED_FORMS = ("sums", "grad", "both", "inplace")


def masked_ranges(name, E):
    """the two [lo, hi) token ranges of a case"""
    return {"reference": ((2, 90), (180, 278)),                     # trainer_glsr.py: played notes and time separators (E = 342 only)
            "empty": ((5, 5), (2, E // 2)),
            "full": ((0, E), (3, E // 3)),
            "overlap": ((2, E // 2), (E // 4, E - 3)),
            "ends-at-E": ((E - 20, E), (0, 1))}[name]


MASKED_CASES = [dict(id="rows%d-E%d-ld%d-%s" % (rows, E, E + 2, rn), rows=rows, E=E, ld=E + 2, ranges=masked_ranges(rn, E), range_name=rn)
                for rows in MASKED_ROWS for E in MASKED_E for rn in ("reference", "empty", "full", "overlap", "ends-at-E") if not (rn == "reference" and E < 278)]
MASKED_TC = dict(sums=2, dlogits=16)
_MASKED_CACHE = {}


def masked_inputs(case):
    gen = _gen("masked/" + case["id"])
    return dict(x=torch.randn(case["rows"], case["E"], generator=gen) * 3, w=torch.randn(case["rows"], 2, generator=gen))


def masked_references(case):
    if case["id"] not in _MASKED_CACHE:
        inp = masked_inputs(case)
        empty = torch.tensor([[lo >= hi for lo, hi in case["ranges"]]]).expand(case["rows"], 2)
        rec = make_refs(case["id"], masked_math(inp["x"], case["ranges"], inp["w"], F64), masked_math(inp["x"], case["ranges"], inp["w"], F32), MASKED_TC,
                        exact0=dict(sums=empty))
        rec["inputs"] = inp
        _MASKED_CACHE[case["id"]] = rec
    return _MASKED_CACHE[case["id"]]


def run_masked(ops, case, form, device="cpu"):
    """one launch: sums only | grad (dlogits only) | both | inplace (both, dlogits written over the logits)"""
    inp, rows, E, ld = masked_inputs(case), case["rows"], case["E"], case["ld"]
    lbuf = _buf((rows + PAD_ROWS, ld), device)
    lbuf[:rows, :E] = inp["x"].to(device)
    sums = _buf((rows + PAD_ROWS, 2), device) if form != "grad" else None
    dl = None if form == "sums" else lbuf if form == "inplace" else _buf((rows + PAD_ROWS, ld), device)
    ops.masked_prob(lbuf[:rows], E, case["ranges"], sums=None if sums is None else sums[:rows], w=None if dl is None else inp["w"].to(device),
                    dlogits=None if dl is None else dl[:rows])
    c = lambda t: None if t is None else t.cpu()                  # noqa: E731
    return dict(form=form, logits=c(lbuf), sums=c(sums), dlogits=c(dl))


def check_masked(case, bufs, F=None):
    F = LOSS_F["masked_prob"] if F is None else F
    rec, cid, rows, E, ld, form = masked_references(case), case["id"] + " " + bufs["form"], case["rows"], case["E"], case["ld"], bufs["form"]
    got = {}
    if form != "inplace":
        ref_l = torch.full((rows + PAD_ROWS, ld), SENTINEL)
        ref_l[:rows, :E] = rec["inputs"]["x"]
        assert bits_equal(bufs["logits"], ref_l), "%s: the logits were modified" % cid
    if form != "grad":
        check_sentinel(cid, "sums past its last row", bufs["sums"][rows:])
        got["sums"] = bufs["sums"][:rows]
    if form != "sums":
        check_sentinel(cid, "a row of dlogits past the last row", bufs["dlogits"][rows:])
        check_sentinel(cid, "a padding column (>= E) of dlogits", bufs["dlogits"][:rows, E:])
        got["dlogits"] = bufs["dlogits"][:rows, :E]
    sub = dict(rec, ref0={k: v for k, v in rec["ref0"].items() if k in got})
    return check_quantities(sub, got, F)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# pairwise_reg
# ---------------------------------------------------------------------------------------------------------------------------------------------
EXACT_PASS, RANDN_PASS = "exact", "randn"
PAIR_PASSES = (EXACT_PASS, RANDN_PASS)
PAIR_SHAPES = ((1, 0, 1), (63, 0, 63), (65, 1, 64), (300, 150, 100), (300, 297, 3))
PAIR_TINY = (65, 1, 64)                 # the case whose attributes differ by 2**-40 around 0.5
PAIR_EXACT_Z = (-64.0, -32.0, 0.0, 32.0, 64.0)
PAIR_GS = {EXACT_PASS: 0.25, RANDN_PASS: 0.37}                      # exact pass: 4 grad_scale = 1
PAIR_CASES = [dict(id="n%d-row0_%d-nrows%d-%s-%s%s" % (n, r0, nr, kind, "dz0" if dz else "nodz0", "-attr-2^-40" if (n, r0, nr) == PAIR_TINY else ""),
                   n_all=n, row0=r0, nrows=nr, kind=kind, dz0=dz, tiny=(n, r0, nr) == PAIR_TINY, zero=(("loss_rows", "dz0") if dz else ("loss_rows",)) if n == 1 else ())
              for n, r0, nr in PAIR_SHAPES for kind in PAIR_PASSES for dz in (True, False)]
PAIR_TC = dict(loss_rows=1, dz0=1)
_PAIR_CACHE = {}


def pair_inputs(case):
    """z0: the exact pass draws from {-64, -32, 0, 32, 64} - tanh of every difference is exactly 0 or +-1, every loss term is in {0, 1, 4}, every
    gradient term in {-1, 0, 1}, the sums are exact in any order; the randn pass is standard normal.  attr float64: quarters in [0, 1] (many exact
    ties), or 0.5 + {-1, 0, 1} x 2**-40 - distinct in float64, one value in float32"""
    n = case["n_all"]
    gen = _gen("pair/n%d-%s" % (n, case["kind"]))
    if case["kind"] == EXACT_PASS:
        z0 = torch.tensor(PAIR_EXACT_Z)[torch.randint(0, 5, (n,), generator=gen)]
    else:
        z0 = torch.randn(n, generator=gen)
    k = torch.randint(0, 5, (n,), generator=gen)
    attr = 0.5 + ((k % 3) - 1).double() * 2.0 ** -40 if case["tiny"] else k.double() / 4.0
    return dict(z0=z0, attr=attr)


def pair_references(case):
    key = (case["n_all"], case["row0"], case["nrows"], case["kind"])
    if key not in _PAIR_CACHE:
        inp, gs = pair_inputs(case), f32(PAIR_GS[case["kind"]])
        o64, o32 = (pairwise_math(inp["z0"], inp["attr"], case["row0"], case["nrows"], gs, dt) for dt in (F64, F32))
        if case["kind"] == EXACT_PASS:
            z = inp["z0"].double()
            th = torch.tanh(inp["z0"].view(-1, 1) - inp["z0"].view(1, -1))                       # in float32, as the kernel forms it
            assert set(th.unique().tolist()) <= {-1.0, 0.0, 1.0} and torch.equal(th.double(), torch.tanh(z.view(-1, 1) - z.view(1, -1)).round())
            for k in o64:
                assert bool((o64[k] == o64[k].round()).all()) and float(o64[k].abs().max()) < 2.0 ** 24 and torch.equal(o32[k].double(), o64[k]), (case["id"], k)
        rec = make_refs("n%d-row0_%d-nrows%d-%s" % key, o64, o32, PAIR_TC, ("loss_rows", "dz0") if case["n_all"] == 1 else ())
        rec["inputs"] = inp
        _PAIR_CACHE[key] = rec
    return _PAIR_CACHE[key]


def run_pair(ops, case, device="cpu"):
    inp, nr = pair_references(case)["inputs"], case["nrows"]
    loss = _buf((nr + PAD_ROWS,), device)
    dz = _buf((nr + PAD_ROWS,), device) if case["dz0"] else None
    ops.pairwise_reg(inp["z0"].to(device), inp["attr"].to(device), case["row0"], nr, loss[:nr], PAIR_GS[case["kind"]], None if dz is None else dz[:nr])
    return dict(loss_rows=loss.cpu(), dz0=None if dz is None else dz.cpu())


def check_pair(case, bufs, F=None):
    """exact pass: bit for bit the float64 reference (the sign of a zero is not compared); randn pass: the tile bound"""
    F = LOSS_F["pairwise_reg"] if F is None else F
    rec, cid, nr = pair_references(case), case["id"], case["nrows"]
    names = ("loss_rows", "dz0") if case["dz0"] else ("loss_rows",)
    got = {}
    for k in names:
        check_sentinel(cid, "%s past its last row" % k, bufs[k][nr:])
        got[k] = bufs[k][:nr].view(nr, 1)
    if case["kind"] == EXACT_PASS:
        for k in names:
            bad = torch.nonzero(got[k].double() != rec["ref64"][k])
            assert bad.numel() == 0, "%s %s: exact pass, row %d holds %r, the exact sum is %r (%d rows differ)" % (
                cid, k, int(bad[0, 0]), float(got[k][bad[0, 0], 0]), float(rec["ref64"][k][bad[0, 0], 0]), bad.shape[0])
        return (0.0, "-", 0, 0, None)
    sub = dict(rec, ref0={k: v for k, v in rec["ref0"].items() if k in names})
    return check_quantities(sub, got, F)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# adv_head
# ---------------------------------------------------------------------------------------------------------------------------------------------
ADV_SHAPES = ((1, 1, 1), (5, 63, 64), (37, 96, 104), (6, 128, 128), (9, 65, 72))
ADV_VARIANTS = ("full", "nolam", "noda", "nogz")
ADV_LAM = 0.03
ADV_MIN_PRE = 1e-3
ADV_ZROW = 2                            # the row with z = 0 (B >= 5): with b_r = 0 its pre_r is exactly 0
ADV_CASES = [dict(id="B%d-Z%d-ldz%d-%s" % (B, Z, ldz, v), B=B, Z=Z, ldz=ldz, variant=v) for B, Z, ldz in ADV_SHAPES for v in ADV_VARIANTS]
ADV_TC = dict(o=2, loss_rows=2, da=2, g_z=16)
_ADV_CACHE, _ADV_INPUTS = {}, {}


def adv_wanted(case):
    return ("o", "loss_rows") + (() if case["variant"] == "noda" else ("da",)) + (() if case["variant"] == "nogz" else ("g_z",))


def _adv_draw(B, Z, k):
    gen = _gen("adv/B%d-Z%d/%d" % (B, Z, k))
    z = torch.randn(B, Z, generator=gen)
    w_r, w_n = torch.randn(1, Z, generator=gen) * Z ** -0.5, torch.randn(1, Z, generator=gen) * Z ** -0.5
    b_r, b_n = torch.zeros(1), torch.randn(1, generator=gen)
    mask = (torch.rand(B, 2, generator=gen) > 0.3).float() / 0.7
    mask[torch.arange(B) % 5 == 3] = 0.0                            # rows 3, 8, ..: both attributes masked
    if B == 1:
        mask[:] = 1.0 / 0.7
    dens, g0 = torch.rand(B, 2, generator=gen), torch.randn(B, Z, generator=gen)
    if B >= 5:
        z[ADV_ZROW], mask[ADV_ZROW] = 0.0, 1.0 / 0.7
    return dict(z=z, w_r=w_r, w_n=w_n, b_r=b_r, b_n=b_n, mask=mask, dens=dens, g0=g0, inv_bg=f32(1.0 / 37), seed_index=k)


def adv_condition(inp):
    """|pre| >= 1e-3 in float64 for every (row, attribute) but the planted pre_r == 0 of row ADV_ZROW, and at least one open, unmasked gate in
    every tile of 16 rows (o, da and the change of g_z are not identically zero there)"""
    o = adv_math(inp, ADV_LAM, inp["g0"], F64)
    pre, B = o["pre"], inp["z"].shape[0]
    planted = torch.zeros(B, 2, dtype=torch.bool)
    if B >= 5:
        planted[ADV_ZROW, 0] = True
        if float(pre[ADV_ZROW, 0]) != 0.0:
            return False
    if not bool((pre.abs()[~planted] >= ADV_MIN_PRE).all()):
        return False
    return all(float(o["o"][i:i + 16].abs().max()) > 0 and float(o["da"][i:i + 16].abs().max()) > 0 for i in range(0, B, 16))


def adv_inputs(case):
    """the first draw k = 0, 1, .. of the shape's generator that meets adv_condition (chosen on the CPU, in float64)"""
    key = (case["B"], case["Z"])
    if key not in _ADV_INPUTS:
        for k in range(64):
            inp = _adv_draw(case["B"], case["Z"], k)
            if adv_condition(inp):
                break
        else:
            raise AssertionError("no draw of %s meets the input condition" % (key,))
        _ADV_INPUTS[key] = inp
    return _ADV_INPUTS[key]


def adv_references(case):
    if case["id"] not in _ADV_CACHE:
        inp, want = adv_inputs(case), adv_wanted(case)
        lam = None if case["variant"] == "nolam" else f32(ADV_LAM)
        g0 = None if case["variant"] == "nogz" else inp["g0"]
        o64, o32 = adv_math(inp, lam, g0, F64), adv_math(inp, lam, g0, F32)
        closed = (o64["pre"] <= 0) | (inp["mask"] == 0)
        exact0 = {k: closed for k in ("o", "da") if k in want}
        rec = make_refs(case["id"], {k: o64[k] for k in want}, {k: o32[k] for k in want}, ADV_TC, ("da",) if lam is None and "da" in want else (), exact0=exact0)
        rec["inputs"], rec["pre"] = inp, o64["pre"]
        _ADV_CACHE[case["id"]] = rec
    return _ADV_CACHE[case["id"]]


def run_adv(ops, case, device="cpu"):
    """z and g_z as the [:B, :Z] views of [B + 3][ldz] buffers (z: NaN outside the view, g_z: sentinel outside)"""
    inp, B, Z, ldz, v = adv_inputs(case), case["B"], case["Z"], case["ldz"], case["variant"]
    zb = torch.full((B + PAD_ROWS, ldz), float("nan"), device=device)
    zb[:B, :Z] = inp["z"].to(device)
    outs = {k: _buf((B + PAD_ROWS, 2), device) for k in ("o", "loss_rows") + (() if v == "noda" else ("da",))}
    gz = None
    if v != "nogz":
        gz = _buf((B + PAD_ROWS, ldz), device)
        gz[:B, :Z] = inp["g0"].to(device)
    d = lambda t: t.to(device)                                    # noqa: E731
    ops.adv_head(zb[:B, :Z], d(inp["w_r"]), d(inp["w_n"]), d(inp["b_r"]), d(inp["b_n"]), d(inp["mask"]), d(inp["dens"]),
                 None if v == "nolam" else torch.tensor([ADV_LAM], device=device), 1.0 / 37, outs["o"][:B], outs["loss_rows"][:B],
                 da=None if v == "noda" else outs["da"][:B], g_z=None if gz is None else gz[:B, :Z])
    res = {k: t.cpu() for k, t in outs.items()}
    res["g_z"] = None if gz is None else gz.cpu()
    return res


def check_adv(case, bufs, F=None):
    F = LOSS_F["adv_head"] if F is None else F
    rec, cid, B, Z = adv_references(case), case["id"], case["B"], case["Z"]
    got = {}
    for k in adv_wanted(case):
        check_sentinel(cid, "%s past its last row" % k, bufs[k][B:])
        if k == "g_z":
            check_sentinel(cid, "a column >= Z of g_z", bufs[k][:B, Z:])
            got[k] = bufs[k][:B, :Z]
        else:
            got[k] = bufs[k][:B]
    if B >= 5:
        assert float(rec["pre"][ADV_ZROW, 0]) == 0.0
        assert float(got["o"][ADV_ZROW, 0]) == 0.0 and ("da" not in got or float(got["da"][ADV_ZROW, 0]) == 0.0), "%s: pre == 0 must give o = 0 and da = 0" % cid
    if case["variant"] == "nolam" and "g_z" in got:
        assert bits_equal(got["g_z"], rec["inputs"]["g0"]), "%s: lam_dev = NULL must leave g_z unchanged bit for bit" % cid
    return check_quantities(rec, got, F)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# onehot_to_index
# ---------------------------------------------------------------------------------------------------------------------------------------------
ONEHOT_CASES = [dict(id="rows%d-V%d" % (rows, V), rows=rows, V=V) for rows in (1, 5, 161) for V in (1, 3, 64, 65, 342)]


def onehot_inputs(case):
    """rows in turn: a true one-hot, a soft row (a softmax), a tie of two maxima (the first index wins), a row of zeros (index 0)"""
    rows, V = case["rows"], case["V"]
    gen = _gen("onehot/" + case["id"])
    oh = torch.zeros(rows, V)
    hot = torch.randint(0, V, (rows,), generator=gen)
    soft = torch.softmax(torch.randn(rows, V, generator=gen), 1)
    expect = np.zeros(rows, np.int32)
    for r in range(rows):
        k, h = (r + rows) % 4, int(hot[r])
        if k == 0:
            oh[r, h], expect[r] = 1.0, h
        elif k == 1:
            oh[r] = soft[r]
            expect[r] = int(np.argmax(soft[r].numpy()))
        elif k == 2:
            h2 = (h + 1 + 63 % V) % V
            oh[r, h] = oh[r, h2] = 0.75
            expect[r] = min(h, h2)
    return dict(oh=oh, expect=expect)


def run_onehot(ops, case, device="cpu"):
    idx = _buf((case["rows"] + PAD_ROWS,), device, torch.int32)
    ops.onehot_to_index(onehot_inputs(case)["oh"].to(device), idx[:case["rows"]])
    return dict(idx=idx.cpu())


def check_onehot(case, bufs):
    inp, rows = onehot_inputs(case), case["rows"]
    want = first_argmax(inp["oh"])
    assert np.array_equal(want, inp["expect"]), case["id"]
    check_sentinel(case["id"], "idx past its last row", bufs["idx"][rows:], INT_SENTINEL)
    got = bufs["idx"][:rows].numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: row %d index %d, the first-index argmax is %d" % (case["id"], bad[0], got[bad[0]], want[bad[0]])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the refusals of the C ABI (the error branches csrc/loss.hip has today): (id, entry point, arguments from the pointers p.f / p.i / p.d, code)
# ---------------------------------------------------------------------------------------------------------------------------------------------
E_NULL, E_SHAPE = -1, -2
ABI_REFUSALS = [
    ("vocab_logsoftmax ld < E", "fn_vocab_logsoftmax", lambda p: (p.f, 2, 3, 8, 7, p.f, p.i, p.f, 1.0, p.f, None), E_SHAPE),
    ("vocab_logsoftmax B = 0", "fn_vocab_logsoftmax", lambda p: (p.f, 0, 3, 8, 8, p.f, p.i, p.f, 1.0, p.f, None), E_SHAPE),
    ("vocab_logsoftmax nll_rows without target", "fn_vocab_logsoftmax", lambda p: (p.f, 2, 3, 8, 8, p.f, None, p.f, 1.0, None, None), E_NULL),
    ("vocab_logsoftmax dlogits without target", "fn_vocab_logsoftmax", lambda p: (p.f, 2, 3, 8, 8, p.f, None, None, 1.0, p.f, None), E_NULL),
    ("vocab_logsoftmax logits NULL", "fn_vocab_logsoftmax", lambda p: (None, 2, 3, 8, 8, p.f, p.i, p.f, 1.0, p.f, None), E_NULL),
    ("vocab_logsoftmax_bwd ld < E", "fn_vocab_logsoftmax_bwd", lambda p: (p.f, p.f, 2, 3, 8, 7, p.f, None), E_SHAPE),
    ("vocab_logsoftmax_bwd dlogits NULL", "fn_vocab_logsoftmax_bwd", lambda p: (p.f, p.f, 2, 3, 8, 8, None, None), E_NULL),
    ("vocab_argmax ld < E", "fn_vocab_argmax", lambda p: (p.f, 2, 8, 7, p.f, 8, p.i, 1, None), E_SHAPE),
    ("vocab_argmax tok_out NULL", "fn_vocab_argmax", lambda p: (p.f, 2, 8, 8, p.f, 8, None, 1, None), E_NULL),
    ("time_logsoftmax Tr = 0", "fn_time_logsoftmax", lambda p: (p.f, 2, 0, 3, p.f, p.i, p.f, 1.0, p.f, None), E_SHAPE),
    ("time_logsoftmax nll_bc without target", "fn_time_logsoftmax", lambda p: (p.f, 2, 4, 3, p.f, None, p.f, 1.0, None, None), E_NULL),
    ("time_logsoftmax dlogits without target", "fn_time_logsoftmax", lambda p: (p.f, 2, 4, 3, p.f, None, None, 1.0, p.f, None), E_NULL),
    ("time_logsoftmax_bwd gout NULL", "fn_time_logsoftmax_bwd", lambda p: (p.f, None, 2, 4, 3, p.f, None), E_NULL),
    ("time_logsoftmax_bwd Cc = 0", "fn_time_logsoftmax_bwd", lambda p: (p.f, p.f, 2, 4, 0, p.f, None), E_SHAPE),
    ("masked_prob ld < E", "fn_masked_prob", lambda p: (p.f, 2, 8, 7, 0, 2, 3, 5, p.f, p.f, p.f, None), E_SHAPE),
    ("masked_prob hi0 > E", "fn_masked_prob", lambda p: (p.f, 2, 8, 8, 0, 9, 3, 5, p.f, p.f, p.f, None), E_SHAPE),
    ("masked_prob hi1 > E", "fn_masked_prob", lambda p: (p.f, 2, 8, 8, 0, 2, 3, 9, p.f, p.f, p.f, None), E_SHAPE),
    ("masked_prob lo1 < 0", "fn_masked_prob", lambda p: (p.f, 2, 8, 8, 0, 2, -1, 5, p.f, p.f, p.f, None), E_SHAPE),
    ("masked_prob neither sums nor dlogits", "fn_masked_prob", lambda p: (p.f, 2, 8, 8, 0, 2, 3, 5, None, p.f, None, None), E_NULL),
    ("masked_prob dlogits without w", "fn_masked_prob", lambda p: (p.f, 2, 8, 8, 0, 2, 3, 5, p.f, None, p.f, None), E_NULL),
    ("pairwise_reg row0 + nrows > n_all", "fn_pairwise_reg", lambda p: (p.f, p.d, 8, 6, 3, p.f, 1.0, p.f, None), E_SHAPE),
    ("pairwise_reg row0 < 0", "fn_pairwise_reg", lambda p: (p.f, p.d, 8, -1, 3, p.f, 1.0, p.f, None), E_SHAPE),
    ("pairwise_reg loss_rows NULL", "fn_pairwise_reg", lambda p: (p.f, p.d, 8, 0, 3, None, 1.0, p.f, None), E_NULL),
    ("adv_head ldz < Z", "fn_adv_head", lambda p: (p.f, 3, 4, 2, p.f, p.f, p.f, p.f, p.f, p.f, p.f, 0.5, p.f, p.f, p.f, p.f, 4, None), E_SHAPE),
    ("adv_head ldg < Z", "fn_adv_head", lambda p: (p.f, 4, 4, 2, p.f, p.f, p.f, p.f, p.f, p.f, p.f, 0.5, p.f, p.f, p.f, p.f, 3, None), E_SHAPE),
    ("adv_head o NULL", "fn_adv_head", lambda p: (p.f, 4, 4, 2, p.f, p.f, p.f, p.f, p.f, p.f, p.f, 0.5, None, p.f, p.f, p.f, 4, None), E_NULL),
    ("onehot_to_index V = 0", "fn_onehot_to_index", lambda p: (p.f, 2, 0, p.i, None), E_SHAPE),
    ("onehot_to_index idx NULL", "fn_onehot_to_index", lambda p: (p.f, 2, 4, None, None), E_NULL),
]
