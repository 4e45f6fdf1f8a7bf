"""How well a trained GM-VAE explains a piece: the importance-weighted bound on log p(x) (Burda et al., "Importance Weighted Autoencoders") with the
one-sample ELBO, a Monte-Carlo KL per latent and the effective sample size that says whether the estimate can be trusted.

    log p(x) >= E log (1/S) sum_s w_s,    w_s = p(x | z_s) p(z_r,s) p(z_n,s) / (q(z_r,s | x) q(z_n,s | x)),   z_s ~ q(z | x)

p(z) is the mixture prior (mu_lookup, logvar_lookup with equal weights, the likelihood approx_qy_x forms), q the encoder's Gaussians, p(x | z) the
teacher-forced global decoder.  ONE encode of the B pieces; fn_posterior_draw writes the S samples of every piece into the decoder's own latent rows with
log q and log p at the stored z; then per pass over whole pieces the decoder runs on its share of the B*S rows, the fused head yields the per-token nll
without materialising logits, and fn_iw_reduce reduces the S log-weights per piece (include/fadernets.h has the definitions).  OURS: the reference
prints the cross-entropy of one reparameterised sample and the analytic KL.

Scope: the attribute sub-decoders' terms are not part of this likelihood - their time-axis log-softmax, a quirk of the reference that this project
keeps, is not a normalised distribution over classes.  Not built: the v2 model families, a reduction over ranks, gradients through the bound."""
import collections
import math

import numpy as np
import torch

from .constrain import _int
from .decode import _is_finite, _is_int
from .engine import E_VOCAB

Likelihood = collections.namedtuple("Likelihood", ["iwae", "elbo", "ess", "recon", "kl_r", "kl_n", "n_tokens", "lw"])
CHROMA = 24
MAX_SAMPLES = 1 << 16
PASS_BYTES = 1 << 30          # what the decoder's per-step buffers of one pass may take (rows_per_pass=None)


def default_rows_per_pass(T, H, samples):
    """The decoder keeps 5 H floats per row and step (the states of both layers and the second layer's input gates): the default pass holds as many
    whole pieces as keep that within PASS_BYTES, and at least one."""
    return max(1, PASS_BYTES // (20 * T * H) // samples) * samples


def _args(model, x, chroma, samples, temperature, seed, offset, trim, rows_per_pass):
    """validated (x on the device, chroma (B, 24) fp32 on the device, S, the 32 bytes of FnDrawParams, trim, pieces per pass); ValueError before any launch"""
    if not all(hasattr(model, k) for k in ("mu_r_lookup", "logvar_n_lookup", "n_component", "engine")):
        raise ValueError("marginal_likelihood: a GM-VAE (MusicAttrRegGMVAE), got %s" % type(model).__name__)
    try:
        x = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    except (TypeError, ValueError, RuntimeError):
        raise ValueError("x: (B, T) token ids or (B, T, %d) one-hot, got %s" % (E_VOCAB, type(x).__name__))
    if x.dim() not in (2, 3) or x.shape[0] < 1 or x.shape[1] < 1 or (x.dim() == 3 and x.shape[2] != E_VOCAB) or x.is_complex() or x.dtype == torch.bool:
        raise ValueError("x: (B, T) token ids or (B, T, %d) one-hot, got %s %s" % (E_VOCAB, x.dtype, tuple(x.shape)))
    if x.dim() == 2 and not x.is_cuda and x.numel() and (float(x.min()) < 0 or float(x.max()) >= E_VOCAB or not bool(torch.isfinite(x.double()).all())):
        raise ValueError("x: token ids in [0, %d)" % E_VOCAB)
    B = x.shape[0]
    try:
        c = chroma.detach() if torch.is_tensor(chroma) else torch.as_tensor(np.asarray(chroma, dtype=np.float32))
    except (TypeError, ValueError, RuntimeError):
        raise ValueError("chroma: (%d, %d) numbers, got %r" % (B, CHROMA, chroma))
    if tuple(c.shape) != (B, CHROMA) or c.is_complex() or c.dtype == torch.bool:
        raise ValueError("chroma: (%d, %d) numbers, got shape %s" % (B, CHROMA, tuple(c.shape)))
    S = _int("samples", samples, 1, MAX_SAMPLES + 1)
    if B * S >= 1 << 31:
        raise ValueError("samples: B * samples < 2^31, got %d * %d" % (B, S))
    with np.errstate(over="ignore", under="ignore"):
        tau = float(np.float32(temperature)) if _is_finite(temperature) else float("nan")          # as the kernel reads it: fp32
    if not math.isfinite(tau) or not tau > 0:
        raise ValueError("temperature: a finite number > 0, got %r" % (temperature,))
    for name, v in (("seed", seed), ("offset", offset)):
        if not _is_int(v) or not 0 <= int(v) < 1 << 64:
            raise ValueError("%s: an int in [0, 2^64), got %r" % (name, v))
    if not isinstance(trim, (bool, np.bool_)):
        raise ValueError("trim: a bool, got %r" % (trim,))
    per = None if rows_per_pass is None else max(1, _int("rows_per_pass", rows_per_pass, 1, 1 << 31) // S)
    raw = np.zeros(1, dtype=[("seed", "<u8"), ("offset", "<u8"), ("tau", "<f4"), ("reserved", "<i4", (3,))])
    raw["seed"], raw["offset"], raw["tau"] = int(seed), int(offset), np.float32(temperature)
    dev = model._device()
    return x.to(dev), c.float().to(dev), S, torch.from_numpy(raw.view(np.uint8).copy()), bool(trim), per


def _spans(d):
    """the np.trim_zeros span of every row of d (B, T) int32: first to last non-zero token -> (t0, t1) int32 (B,); an all-zero row has t0 = t1 = 0"""
    T = d.shape[1]
    nz = (d != 0).to(torch.int32)
    some = nz.sum(1) > 0
    first = nz.argmax(1)
    last = T - 1 - nz.flip(1).argmax(1)
    zero = torch.zeros_like(first)
    return torch.where(some, first, zero).to(torch.int32).contiguous(), torch.where(some, last + 1, zero).to(torch.int32).contiguous()


def marginal_likelihood_detail(model, x, chroma, samples=64, temperature=1.0, seed=0, offset=0, trim=False, rows_per_pass=None):
    """marginal_likelihood with what stands behind it -> (Likelihood, dict(z (B, S, 2Z+24) fp32: the latent rows the decoder saw, logp, logq (2, B, S) fp64:
    the densities of the rhythm and the note latent at them, t0, t1 (B,) int32 or None: the scored spans))"""
    x, c, S, params, trim, per = _args(model, x, chroma, samples, temperature, seed, offset, trim, rows_per_pass)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            return _run(model, x, c, S, params, trim, per)
    finally:
        model.train(was_training)


def marginal_likelihood(model, x, chroma, samples=64, temperature=1.0, seed=0, offset=0, trim=False, rows_per_pass=None):
    """The importance-weighted bound on log p(x) of B pieces from `samples` posterior draws each.

    x            (B, T) token ids or (B, T, 342) one-hot, as encode takes them; chroma (B, 24): the decoder's condition.
    samples      S draws from q(z | x) per piece.  Sample (b, s) uses the Philox counter of fn_latent_draw's row b at offset + s under the key seed
                 (stream 0 the rhythm latent, stream 1 the note latent): it does not depend on B, S or the passes.
    temperature  tau > 0 widens (or narrows) the proposal to N(mu, (tau sigma)^2); the weights account for it, so the bound stays a bound.
    trim         False: all T steps are scored, as the training cross-entropy does.  True: the np.trim_zeros span of each piece, first to last non-zero
                 token (the encoder and the decoder still see the whole piece); n_tokens is the span's length, 0 for an all-zero piece.
    rows_per_pass  decoder rows per pass, rounded down to whole pieces (at least one piece); None: default_rows_per_pass.  A call creates at most two
                 decoder row counts: the full pass and the tail.

    -> Likelihood(iwae, elbo, ess, recon, kl_r, kl_n (B,) fp64; n_tokens (B,) int32; lw (B, S) fp64), device tensors: the bound log (1/S) sum_s w_s, the
    mean log-weight (the one-sample ELBO), the effective sample size (sum w)^2 / sum w^2 in [1, S], the mean log p(x | z), the Monte-Carlo KL
    mean(log q - log p) of either latent and the log-weights themselves.  iwae >= elbo always; an ess near 1 says that one sample carries the
    estimate and more samples (or a temperature above 1) are needed.  ValueError for anything that is not as described, before anything is launched."""
    return marginal_likelihood_detail(model, x, chroma, samples, temperature, seed, offset, trim, rows_per_pass)[0]


def _run(model, x, c, S, params, trim, per):
    eng = model.engine()
    ops, P, dev, Z, K, H = eng.ops, eng.p, model._device(), model.latent_dim, model.n_component, eng.H
    d = model._indices(x, E_VOCAB, ids_ndim=2)
    B, T = d.shape
    rows = B * S
    per = min(B, default_rows_per_pass(T, H, S) // S if per is None else per)
    pre = eng.encode(d, save=False)                               # the one encode: B rows
    pre = {e: pre[e] for e in ("r", "n")}
    tables = {e: tuple(P["%s_%s_lookup.weight" % (w, e)][:K].float().contiguous() for w in ("mu", "logvar")) for e in ("r", "n")}
    f64 = dict(dtype=torch.float64, device=dev)
    z = torch.empty(rows, 2 * Z + CHROMA, device=dev)
    z[:, 2 * Z:] = c.repeat_interleave(S, 0)                       # the chroma columns, broadcast over the samples
    d_rep = d.repeat_interleave(S, 0).contiguous()
    logp, logq = torch.empty(2, rows, **f64), torch.empty(2, rows, **f64)
    lw, out = torch.empty(rows, **f64), torch.empty(B, 6, **f64)
    t0, t1 = _spans(d) if trim else (None, None)
    # ONE draw for all B * S rows (a latent row is 2Z + 24 floats: small beside a pass of the decoder): the first counter word is the piece's row in the
    # launch, so a draw per pass would restart it and a piece's samples would depend on the passes
    ops.posterior_draw([dict(pre=pre[e], mu_lk=tables[e][0], lv_lk=tables[e][1], z=z[:, k * Z:(k + 1) * Z], logq=logq[k], logp=logp[k], stream_id=k)
                        for k, e in enumerate("rn")], S, params.to(dev))
    for b0 in range(0, B, per):
        b1 = min(B, b0 + per)
        r0, r1, n = b0 * S, b1 * S, (b1 - b0) * S
        dec = eng.global_decoder_tf(d_rep[r0:r1], z[r0:r1], save=False, head=False)
        nll = eng.buf("iw_nll", (T * n,))
        ops.out_head(dec["hx1"].view(T * n, H), P["linear_out_g.weight"], P["linear_out_g.bias"], n, T, d_rep[r0:r1], nll_rows=nll)
        ops.iw_reduce(nll.view(T, n), b1 - b0, S, logp[:, r0:r1], logq[:, r0:r1], lw[r0:r1], out[b0:b1],
                      t0=None if t0 is None else t0[b0:b1], t1=None if t1 is None else t1[b0:b1])
    cols = out.t().contiguous()
    n_tokens = torch.full((B,), T, dtype=torch.int32, device=dev) if t0 is None else t1 - t0
    lik = Likelihood(cols[0], cols[1], cols[2], cols[3], cols[4], cols[5], n_tokens, lw.view(B, S))
    return lik, dict(z=z.view(B, S, -1), logp=logp.view(2, B, S), logq=logq.view(2, B, S), t0=t0, t1=t1)


def likelihood_report(model, loader, samples=64, **kw):
    """marginal_likelihood over every batch of a loader (batches as the loaders yield them: x[0] the tokens, x[3] the chroma) -> dict of
    nats_per_piece, elbo_per_piece (the negated means of iwae and elbo over the pieces: costs in nats, elbo_per_piece >= nats_per_piece),
    nats_per_token (the negated sum of iwae over the sum of n_tokens), bits_per_token (that / ln 2), kl_r, kl_n, mean_ess (means over the pieces),
    min_ess and n_pieces.  Batch i draws at offset + i * samples, so that no two batches share a counter; **kw goes to marginal_likelihood.  One host
    copy per batch."""
    offset = kw.pop("offset", 0)
    S = _int("samples", samples, 1, MAX_SAMPLES + 1)
    if not _is_int(offset) or not 0 <= int(offset) < 1 << 64:
        raise ValueError("offset: an int in [0, 2^64), got %r" % (offset,))
    tot = dict.fromkeys(("iwae", "elbo", "kl_r", "kl_n", "ess", "n_tokens"), 0.0)
    min_ess, n = float("inf"), 0
    for i, x in enumerate(loader):
        lik = marginal_likelihood(model, x[0], x[3], samples=S, offset=(int(offset) + i * S) & ((1 << 64) - 1), **kw)
        rows = torch.stack([lik.iwae, lik.elbo, lik.kl_r, lik.kl_n, lik.ess, lik.n_tokens.double()])
        host = torch.cat([rows.sum(1), lik.ess.min().view(1)]).tolist()                    # the one copy
        for k, v in zip(("iwae", "elbo", "kl_r", "kl_n", "ess", "n_tokens"), host):
            tot[k] += v
        min_ess = min(min_ess, host[6])
        n += lik.iwae.shape[0]
    if n == 0:
        raise RuntimeError("likelihood_report: the loader yielded no batch")
    per_token = -tot["iwae"] / tot["n_tokens"] if tot["n_tokens"] else float("nan")
    return dict(nats_per_piece=-tot["iwae"] / n, nats_per_token=per_token, bits_per_token=per_token / math.log(2.0), elbo_per_piece=-tot["elbo"] / n,
                kl_r=tot["kl_r"] / n, kl_n=tot["kl_n"] / n, mean_ess=tot["ess"] / n, min_ess=min_ess, n_pieces=n)
