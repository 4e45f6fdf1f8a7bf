"""Reconstruction report: what the reference's evaluation_phase() computes behind its loss terms (trainer_gmm.py:470-610) - token accuracy over the
np.trim_zeros span of every sample, rhythm / note class accuracy, posterior-class accuracy - on the device, next to the forward that feeds it:
fn_token_score reads every logit once and writes prediction, negative log-likelihood and rank of the target per token, fn_match_rows is the per-sample
loop of acc() (include/fadernets.h has the definition).  The log-likelihood and the rank are ours: they re-rank decoded hypotheses (score_tokens) and
give top-k accuracy, which the reference does not report."""
import collections

import numpy as np
import torch

from . import _lib
from .constrain import _int
from .decode import greedy_decode
from .engine import E_VOCAB
from .trainer import S_CE_N, S_CE_R, S_CE_X, S_TERMS_N, S_TERMS_R, beta_schedule

TokenScores = collections.namedtuple("TokenScores", ["pred", "nll", "rank"])
RowMatches = collections.namedtuple("RowMatches", ["lead", "len", "correct", "correct_topk", "acc", "nll_sum", "status"])
ScoredTokens = collections.namedtuple("ScoredTokens", ["logp", "rank", "total"])
MAX_V, EMPTY = _lib.FN_SAMPLE_MAX_V, _lib.FN_MATCH_EMPTY
SUMS = ("acc_x", "acc_r", "acc_n", "acc_y_r", "acc_y_n", "topk_x", "nll_x", "n_tokens", "n_samples", "n_empty")


def _ops_of(t, ops=None):
    if ops is not None:
        return ops
    from .hipops import HipOps
    return HipOps(t.device)


def _what(t):
    return "%s %s" % (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__


def _rows_of(name, t, dtype, shape, like):
    """t as a (rows, T) tensor of `dtype` with contiguous rows on the device of `like`; ValueError otherwise"""
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != like.device:
        raise ValueError("%s: a %s tensor %s on %s, got %s" % (name, dtype, tuple(shape), like.device, _what(t)))
    return t.contiguous()


def token_scores(x, target=None, layout="bt", B=None, ops=None):
    """Prediction, negative log-likelihood and rank of the target for every row of logits (or log-probabilities: a log-softmax changes neither the
    argmax, the rank nor lse - x[target]).

    x       fp32 with unit stride along the last axis, V = x.shape[-1] <= 1024.  layout "bt": (B, T, V) with any strides of b and t - a decode's
            log-probs, the attribute decoders' logp_bt - or (rows, V) = (B, 1, V).  layout "time_major": (T*B, V), row t*B + b, any row stride - the
            train forward's logits[:, :342] - with `B` given.
    target  int32 of the outputs' shape, or None; a target outside [0, V) is clamped.

    -> TokenScores(pred int32, nll fp32, rank int32), each x.shape[:-1] ("bt") or (B, T) ("time_major"); nll and rank are None without a target.
    rank counts the entries in front of the target in descending order, ties to the lower index: 0 = the target is the first-index argmax, which
    pred is.  Device tensors; nothing is copied to the host.  ValueError for anything that is not as described, before anything is launched.  `ops`:
    the kernel table (tests); default HipOps(x.device)."""
    if layout not in ("bt", "time_major"):
        raise ValueError("layout in {bt, time_major}, got %r" % (layout,))
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.numel() == 0 or x.dim() not in ((2, 3) if layout == "bt" else (2,)):
        raise ValueError("x: a non-empty fp32 tensor (B, T, V) / (rows, V) for layout bt, (T*B, V) for time_major, got %s" % _what(x))
    V = x.shape[-1]
    if V > MAX_V or (V > 1 and x.stride(-1) != 1):
        raise ValueError("x: at most %d entries with unit stride along the last axis, got %d with stride %d" % (MAX_V, V, x.stride(-1)))
    if layout == "bt":
        if B is not None:
            raise ValueError("B goes with layout time_major")
        shape = tuple(x.shape[:-1])
        Bn, T = (x.shape[0], 1) if x.dim() == 2 else x.shape[:2]
        sb, st = (x.stride(0), 0) if x.dim() == 2 else x.stride()[:2]
    else:
        Bn = _int("B", B, 1, x.shape[0] + 1)
        if x.shape[0] % Bn:
            raise ValueError("x: T*B rows with B = %d, got %d" % (Bn, x.shape[0]))
        T = x.shape[0] // Bn
        shape, sb, st = (Bn, T), x.stride(0), Bn * x.stride(0)
    if sb < 0 or st < 0:
        raise ValueError("x: non-negative strides, got %s" % (x.stride(),))
    tg = None if target is None else _rows_of("target", target, torch.int32, shape, x).view(Bn, T)
    pred = torch.empty(Bn, T, dtype=torch.int32, device=x.device)
    nll = None if tg is None else torch.empty(Bn, T, dtype=torch.float32, device=x.device)
    rank = None if tg is None else torch.empty(Bn, T, dtype=torch.int32, device=x.device)
    _ops_of(x, ops).token_score(x, sb, st, Bn, T, V, target=tg, pred=pred, nll=nll, rank=rank)
    return TokenScores(pred.view(shape), None if nll is None else nll.view(shape), None if rank is None else rank.view(shape))


def match_rows(pred, target, trim=False, nll=None, rank=None, topk=5, ops=None):
    """The per-sample loop of the reference's acc() (trainer_gmm.py:549-565) for pred, target int32 (rows, T).

    trim    the reference's np.trim_zeros quirk, kept exactly: lead = the leading zeros of the target row, len = last non-zero + 1 - lead, and
            pred[j] is compared with target[lead + j], j < len (the reference cuts the prediction from its start, the target from its first
            non-zero).  False: lead = 0, len = T.
    nll, rank  fp32 / int32 (rows, T) of token_scores, or None; topk: a token counts for correct_topk when its rank < topk.

    -> RowMatches(lead, len, correct, correct_topk int32, acc = correct / len and nll_sum = the sum of nll[lead + j] fp64, status int32), each (rows,)
    on the device; correct_topk / nll_sum are None without rank / nll.  An all-zero target row under trim has len 0, acc 0, nll_sum 0 and status
    EMPTY (the reference divides by zero).  ValueError for anything that is not as described, before anything is launched."""
    if not isinstance(trim, (bool, np.bool_)):
        raise ValueError("trim: a bool, got %r" % (trim,))
    if not torch.is_tensor(pred) or pred.dtype != torch.int32 or pred.dim() != 2 or pred.numel() == 0:
        raise ValueError("pred: a non-empty int32 tensor (rows, T), got %s" % _what(pred))
    topk = _int("topk", topk, 1, 1 << 30)
    pred = pred if pred.stride(1) == 1 or pred.shape[1] == 1 else pred.contiguous()
    target = _rows_of("target", target, torch.int32, pred.shape, pred)
    nll = None if nll is None else _rows_of("nll", nll, torch.float32, pred.shape, pred)
    rank = None if rank is None else _rows_of("rank", rank, torch.int32, pred.shape, pred)
    rows, T = pred.shape
    i32, f64 = dict(dtype=torch.int32, device=pred.device), dict(dtype=torch.float64, device=pred.device)
    out = RowMatches(torch.empty(rows, **i32), torch.empty(rows, **i32), torch.empty(rows, **i32), None if rank is None else torch.empty(rows, **i32),
                     torch.empty(rows, **f64), None if nll is None else torch.empty(rows, **f64), torch.empty(rows, **i32))
    _ops_of(pred, ops).match_rows(pred, target, T, bool(trim), out.lead, out.len, out.correct, out.acc, out.status, nll=nll, rank=rank, topk=topk,
                                  correct_topk=out.correct_topk, nll_sum=out.nll_sum)
    return out


@torch.no_grad()
def score_tokens(model, z, tokens, constraints=None):
    """The log-probability and the rank of given tokens under a latent: one greedy_decode(z, forced=tokens, every step forced, want_logp=True) and
    token_scores on its log-probs, so step i is scored given tokens[:, :i].  tokens (Bi, steps) integers in [0, 342).

    -> ScoredTokens(logp (Bi, steps) fp32 = -nll, rank (Bi, steps) int32, total (Bi,) fp64 = the sum of logp over the steps, in fn_match_rows' order);
    device tensors.  Re-ranks the hypotheses of sample_decode / beam_decode; with constraints the scores are those of the constrained distribution."""
    if not torch.is_tensor(tokens) or tokens.dim() != 2 or tokens.shape[1] < 1:
        raise ValueError("tokens: an integer tensor (Bi, steps), got %s" % _what(tokens))
    steps = tokens.shape[1]
    res = greedy_decode(model, z, steps, want_logp=True, forced=tokens, force=steps, constraints=constraints)
    logp = res[0]
    tg = tokens.to(device=logp.device, dtype=torch.int32).contiguous()
    ops = model.engine().ops
    sc = token_scores(logp, tg, ops=ops)
    m = match_rows(sc.pred, tg, nll=sc.nll, rank=sc.rank, topk=1, ops=ops)
    return ScoredTokens(-sc.nll, sc.rank, -m.nll_sum)


@torch.no_grad()
def reconstruction_report(trainer, batch, step=0, eps=None, y_label=None, teacher_forced=True, topk=5):
    """One batch of the reference's evaluation_phase() (trainer_gmm.py:487-584) on a GMVAETrainer: ONE Engine.forward(save=False, head=True) - the
    logits exist even where the training step fuses the head - the loss terms of GMVAETrainer.evaluate, and the accuracies on the device.

    batch   (d, r, n, c, r_density, n_density) as the loaders yield them; y_label: the arousal labels of a supervised (VGMIDI-style) batch.
    teacher_forced  True: the token prediction is the argmax of the teacher-forced logits (the forward is train-mode, as evaluate's).  False: the
            tokens of greedy_decode(model, z, T, want_logp=False), the reference's eval-mode free run; nll_x and topk_x are then None.

    Tokens: pred against d over the np.trim_zeros span (match_rows(trim=True)), with nll and rank.  Rhythm and note classes: the argmax over the
    class axis of the TIME-axis log-softmax (trainer_gmm.py:546 on gmm_model.py:110,115 - the reference's quirk, kept).  Posterior class: y of
    fn_latent_fwd against y_label.
    -> dict of sums over the batch: acc_x, acc_r, acc_n (per-sample accuracies summed, as acc() returns them), acc_y_r, acc_y_n (samples whose
    posterior class is the label; 0 without y_label), topk_x (per-sample top-k accuracies summed), nll_x (the nll of the tokens inside the spans),
    n_tokens (their number), n_samples, n_empty (all-pad samples: accuracy 0), plus tuple8 = (loss, CE_X, CE_R, CE_N, l_r, l_n, kld_latent,
    kld_class) and tensors = the device tensors behind the sums (views of engine buffers: valid until the next forward).  Only the scalars reach the
    host, in one copy."""
    if trainer.dist is not None and trainer.dist.world > 1:
        raise NotImplementedError("reconstruction_report: multi-rank reporting is not implemented")
    if not isinstance(teacher_forced, (bool, np.bool_)):
        raise ValueError("teacher_forced: a bool, got %r" % (teacher_forced,))
    topk = _int("topk", topk, 1, E_VOCAB + 1)
    try:
        d, r, n, c, rd, nd = batch
    except (TypeError, ValueError):
        raise ValueError("batch: (d, r, n, c, r_density, n_density)")
    trainer._check_eps()
    model = trainer.model
    batch = trainer.prepare_batch(d, r, n, c, rd, nd, y_label)
    d, r, n, c, rd, nd, labels = batch
    B, T = d.shape
    Tr = r.shape[1]
    if eps is None:
        eps = trainer.draw_eps(B, T)
    eng = model.engine()
    ops, st = eng.ops, trainer.stats
    trainer._gather_densities(batch, None)
    S = eng.forward(d, r, n, c, eps[0], eps[1], labels, save=False, head=True)
    dec, lat = S["dec"], S["lat"]
    # the loss terms of GMVAETrainer.evaluate; CE_X from the nll fn_token_score writes (the arithmetic of fn_vocab_logsoftmax), so the logits are read once
    sx = token_scores(dec["logits"][:, :E_VOCAB], d, layout="time_major", B=B, ops=ops)
    ops.sum(sx.nll.view(-1), st[S_CE_X:S_CE_X + 1], 1.0 / (B * T))
    for slot, e in ((S_TERMS_R, "r"), (S_TERMS_N, "n")):
        ops.colsum(lat[e]["terms"], st[slot:slot + 4])
    trainer._regulariser(eng, S, batch, B, False)
    eng.sub_decoder_logits(S)
    logp, cls = {}, {}
    for slot, e, attr, Ce in ((S_CE_R, "r", r, 3), (S_CE_N, "n", n, 16)):
        nbc = eng.buf("nll_bc_" + e, (B, Ce))
        logp[e] = eng.buf("report_logp_" + e, (B, Tr, Ce))
        ops.time_logsoftmax(dec["sd"][e]["logits"], logp_bt=logp[e], target=attr, nll_bc=nbc)
        ops.sum(nbc, st[slot:slot + 1], 1.0 / (B * Tr))
        cls[e] = match_rows(token_scores(logp[e], ops=ops).pred, attr, ops=ops)
    if teacher_forced:
        mx = match_rows(sx.pred, d, trim=True, nll=sx.nll, rank=sx.rank, topk=topk, ops=ops)
        pred_x = sx.pred
    else:
        pred_x = greedy_decode(model, dec["zc"].clone(), T, want_logp=False)[1]
        mx = match_rows(pred_x, d, trim=True, ops=ops)
    f64 = dict(dtype=torch.float64, device=d.device)
    zero = torch.zeros((), **f64)
    my = {}
    for e in ("r", "n"):
        my[e] = None if labels is None else match_rows(lat[e]["y"].view(B, 1), labels.view(B, 1), ops=ops)
    sums = [mx.acc.sum(), cls["r"].acc.sum(), cls["n"].acc.sum()] + [zero if my[e] is None else my[e].correct.sum().double() for e in ("r", "n")]
    sums += [zero, zero] if not teacher_forced else [(mx.correct_topk.double() / mx.len.clamp(min=1).double()).sum(), mx.nll_sum.sum()]
    sums += [mx.len.sum().double(), torch.full((), float(B), **f64), (mx.status != 0).sum().double()]
    host = torch.cat([st.double(), torch.stack(sums)]).tolist()                  # the one copy
    out = dict(zip(SUMS, host[st.numel():]))
    for k in ("n_tokens", "n_samples", "n_empty"):
        out[k] = int(out[k])
    if not teacher_forced:
        out["topk_x"] = out["nll_x"] = None
    out["tuple8"] = trainer._terms8(host[:st.numel()], beta_schedule(step, trainer.beta), B, labels is not None)
    out["tensors"] = dict(logits=dec["logits"][:, :E_VOCAB], logp_r=logp["r"], logp_n=logp["n"], y_r=lat["r"]["y"], y_n=lat["n"]["y"], pred_x=pred_x,
                          nll_x=sx.nll, rank_x=sx.rank, match_x=mx, match_r=cls["r"], match_n=cls["n"], match_y_r=my["r"], match_y_n=my["n"])
    return out
