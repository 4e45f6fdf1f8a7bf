"""Which posterior dimension holds which attribute: the encoder-side figures of the disentanglement literature over a data set of codes (N, D) and
factors (N, A) - the mutual information gap (Chen et al., "Isolating Sources of Disentanglement in VAEs"), separated attribute predictability (Kumar
et al., "Variational Inference of Disentangled Latent Concepts from Unlabeled Observations"), modularity (Ridgeway & Mozer, "Learning Deep Disentangled
Embeddings with the F-Statistic Loss"), the R^2 interpretability score (Adel et al., "Discovering Interpretable Representations for Both Deep
Generative and Discriminative Models"; Pati & Lerch use it for AR-VAE) and Spearman's rho.

The work at data-set scale runs on the device, beside the encode that produced the codes: column ranges, the uint8 bin image, the joint histogram of
every (code column, factor) pair, the mutual information and entropies from it, the mid-ranks of every column by counting and the centred sums of raw
values and of ranks (include/fadernets.h has the definitions and the stated order of every fp64 sum).  One copy brings the (D, A) matrices to the
host; what remains is numpy on D x A numbers.  OURS: the reference's run_through_gmm copies every batch to the host and stops there.

The SAP of a DISCRETE factor is ours too: disentanglement_lib fits a linear SVM per code column there; here the classifier is the joint histogram's
(predict the most frequent level of the code's bin), so that nothing is fitted and the figure is a function of the counts.

Not built: the v2 model families in disentanglement_report, a reduction over ranks (one process sees the whole data set)."""
import collections

import numpy as np
import torch

from . import _lib
from .constrain import _int

Disentanglement = collections.namedtuple("Disentanglement", ["mi", "h_factor", "h_code", "r2", "rho", "accuracy", "mig", "sap", "modularity", "winner",
                                                             "interpretability", "names", "card", "n"])
MAX_N, MAX_D, MAX_A, MAX_BINS = _lib.FN_DIS_MAX_N, _lib.FN_DIS_MAX_D, _lib.FN_DIS_MAX_A, _lib.FN_DIS_MAX_BINS
PAD = 64          # the images' row stride is N rounded up to this many entries


def _ops_of(t, ops=None):
    if ops is not None:
        return ops
    from .hipops import HipOps
    return HipOps(t.device)


def _to_host(t):
    """the one copy of a call"""
    return t.cpu().numpy()


def _matrix(name, t, max_cols, like=None):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() not in (1, 2) or t.numel() == 0:
        raise ValueError("%s: a non-empty fp32 tensor (N, columns), got %s" % (name, "%s %s" % (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
    t = t.detach()
    t = t.unsqueeze(1) if t.dim() == 1 else t
    if t.shape[0] > MAX_N or t.shape[1] > max_cols:
        raise ValueError("%s: at most %d rows and %d columns, got %s" % (name, MAX_N, max_cols, tuple(t.shape)))
    if like is not None and (t.shape[0] != like.shape[0] or t.device != like.device):
        raise ValueError("%s: %d rows on %s, got %d on %s" % (name, like.shape[0], like.device, t.shape[0], t.device))
    return t if t.stride(1) == 1 or t.shape[1] == 1 else t.contiguous()


def _args(codes, factors, card, bins, names):
    codes = _matrix("codes", codes, MAX_D)
    factors = _matrix("factors", factors, MAX_A, codes)
    A = factors.shape[1]
    bins = _int("bins", bins, 1, MAX_BINS + 1)
    if card is None:
        card = [0] * A
    try:
        card = [_int("card", c, 0, MAX_BINS + 1) for c in card]
    except TypeError:
        raise ValueError("card: %d ints in [0, %d] (0: a continuous factor), got %r" % (A, MAX_BINS, card))
    if len(card) != A:
        raise ValueError("card: %d ints in [0, %d] (0: a continuous factor), got %r" % (A, MAX_BINS, card))
    if names is None:
        names = ["factor%d" % a for a in range(A)]
    if isinstance(names, str) or not all(isinstance(s, str) for s in names) or len(names) != A:
        raise ValueError("names: %d strings, got %r" % (A, names))
    return codes, factors, card, bins, list(names)


def _gap(m, D):
    """(top1 - top2 over the rows of every column, the argmax row); D == 1: the runner-up is 0.  A NaN column gives NaN and -1."""
    top = np.full(m.shape[1], np.nan)
    arg = np.full(m.shape[1], -1, np.int64)
    for a in range(m.shape[1]):
        col = m[:, a]
        if np.isnan(col).any():
            continue
        order = np.argsort(-col, kind="stable")
        arg[a] = order[0]
        top[a] = col[order[0]] - (col[order[1]] if D > 1 else 0.0)
    return top, arg


def _ratio(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def disentanglement(codes, factors, card=None, bins=20, names=None, ops=None):
    """The disentanglement figures of codes (N, D) against factors (N, A), fp32 tensors on one device (row-strided views work; a 1-D tensor is one column).

    card   None (every factor continuous) or A ints: 0 = continuous, C in [1, 64] = a discrete factor whose values are the integers 0 .. C-1.
    bins   equal-width bins over [min, max] of every code column and every continuous factor, 1 .. 64.
    names  A strings for the error messages and the result; default factor0, factor1, ...

    -> Disentanglement, numpy float64 unless stated:
      mi (D, A)          mutual information of the binned code column and the (binned) factor, nats
      h_factor (A,), h_code (D,)   the entropies of the binned factors and code columns
      r2 (D, A)          squared Pearson correlation, continuous factors; NaN for discrete ones
      rho (D, A)         Spearman's rho (Pearson on mid-ranks), continuous factors; NaN for discrete ones
      accuracy (D, A)    of the histogram classifier (per code bin, the most frequent level), discrete factors; NaN for continuous ones
      mig (A,)           (top1 - top2 of mi[:, a]) / h_factor[a]
      sap (A,)           top1 - top2 of r2[:, a] (continuous) or of accuracy[:, a] (discrete)
      modularity (D,)    1 - sum_{a != a*} mi[d, a]^2 / (mi[d, a*]^2 (A - 1)), a* the row's argmax
      winner             dict of int64 (A,): the argmax dimension under "mi", "r2" and "rho" (|rho|); -1 where the measure is not defined
      interpretability (A,)   max_d r2[d, a]
      names, card, n     as given; n = N
    Degenerate cases: D == 1: every runner-up is 0.  A constant factor: h_factor == 0 and mig is NaN; its r2 and rho are 0 (as are a constant code
    column's), so sap is 0.  A == 1: modularity is 1.  A code column that shares no information with any factor (a row of zeros): modularity NaN.
    Ties go to the lower dimension.
    ValueError for anything that is not as described before the first launch, and - after the one host copy - for a NaN or an infinity in a column or
    a discrete factor with a value that is not an integer in [0, card), naming the column.  `ops`: the kernel table (tests); default HipOps."""
    codes, factors, card, bins, names = _args(codes, factors, card, bins, names)
    with torch.no_grad():
        return _run(_ops_of(codes, ops), codes, factors, card, bins, names)


def _run(ops, codes, factors, card, bins, names):
    dev, (N, D), A = codes.device, codes.shape, factors.shape[1]
    n_pad = (N + PAD - 1) // PAD * PAD
    f32, f64, i32 = (dict(dtype=t, device=dev) for t in (torch.float32, torch.float64, torch.int32))
    cont = [a for a in range(A) if card[a] == 0]
    Q = len(cont)
    # 1. ranges and the bin images
    lim_z, lim_f = torch.empty(2, D, **f32), torch.empty(2, A, **f32)
    st_z, st_f = torch.empty(D, **i32), torch.empty(A, **i32)
    ops.column_range(codes, lim_z[0], lim_z[1], st_z)
    ops.column_range(factors, lim_f[0], lim_f[1], st_f)
    img_z, img_f = torch.empty(D, n_pad, dtype=torch.uint8, device=dev), torch.empty(A, n_pad, dtype=torch.uint8, device=dev)
    ops.bin_columns(codes, lim_z[0], lim_z[1], bins, img_z, st_z)
    ops.bin_columns(factors, lim_f[0], lim_f[1], bins, img_f, st_f, card=None if Q == A else card)
    # 2. the joint histograms and what follows from them
    counts = torch.empty(D * A, 64, 64, **i32)
    ops.joint_hist(img_z, img_f, N, counts)
    scores, hits = torch.empty(D * A, _lib.FN_DIS_MI_COLS, **f64), torch.empty(D * A, **i32)
    ops.mi_scores(counts, scores, hits)
    del counts
    parts = [st_z.double(), st_f.double(), scores.reshape(-1), hits.double()]
    # 3. Pearson on the raw values and on the mid-ranks, continuous factors only
    if Q:
        fc = factors if Q == A else factors[:, cont].contiguous()
        rk_z, rk_f = torch.empty(D, n_pad, **f32), torch.empty(Q, n_pad, **f32)
        ops.column_ranks(codes, rk_z)
        ops.column_ranks(fc, rk_f)
        for X, Y in ((codes, fc), (rk_z[:, :N].t(), rk_f[:, :N].t())):
            m = torch.empty(2 * D + 2 * Q + D * Q, **f64)
            ops.column_corr(X, Y, m[:D], m[D:2 * D], m[2 * D:2 * D + Q], m[2 * D + Q:2 * D + 2 * Q], m[2 * D + 2 * Q:])
            parts.append(m)
    host = _to_host(torch.cat(parts))
    # 4. D x A numbers
    at = [0]

    def take(n):
        at[0] += n
        return host[at[0] - n:at[0]]

    bad_z, bad_f = take(D).astype(np.int64), take(A).astype(np.int64)
    for c in np.nonzero(bad_z)[0]:
        raise ValueError("codes: column %d holds a NaN or an infinity" % c)
    for a in np.nonzero(bad_f)[0]:
        what = "a NaN or an infinity" if bad_f[a] & _lib.FN_DIS_NONFINITE else "a value that is not an integer in [0, %d)" % card[a]
        raise ValueError("factors: column %d (%s) holds %s" % (a, names[a], what))
    sc = take(D * A * 3).reshape(D, A, 3)
    mi, h_code, h_factor = sc[:, :, 0].copy(), sc[:, 0, 1].copy(), sc[0, :, 2].copy()
    hits_h = take(D * A).reshape(D, A)
    nan = np.full((D, A), np.nan)
    r2, rho, accuracy = nan.copy(), nan.copy(), nan.copy()
    for a in range(A):
        if card[a]:
            accuracy[:, a] = hits_h[:, a] / N
    if Q:
        for k, dst in enumerate((r2, rho)):
            m = take(2 * D + 2 * Q + D * Q)
            ss_x, ss_y, cross = m[D:2 * D], m[2 * D + Q:2 * D + 2 * Q], m[2 * D + 2 * Q:].reshape(D, Q)
            r = np.clip(_ratio(cross, np.sqrt(ss_x[:, None] * ss_y[None, :])), -1.0, 1.0)
            dst[:, cont] = r * r if k == 0 else r
    top_mi, win_mi = _gap(mi, D)
    with np.errstate(divide="ignore", invalid="ignore"):
        mig = np.where(h_factor > 0, top_mi / np.where(h_factor > 0, h_factor, 1.0), np.nan)
    top_r2, win_r2 = _gap(r2, D)
    top_acc, _ = _gap(accuracy, D)
    _, win_rho = _gap(np.abs(rho), D)
    sap = np.where(np.array(card) > 0, top_acc, top_r2)
    modularity = np.ones(D)
    if A > 1:
        sq = mi * mi
        best = sq.max(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            modularity = np.where(best > 0, 1.0 - (sq.sum(axis=1) - best) / (np.where(best > 0, best, 1.0) * (A - 1)), np.nan)
    interp = np.array([np.nan if card[a] else r2[:, a].max() for a in range(A)])
    return Disentanglement(mi, h_factor, h_code, r2, rho, accuracy, mig, sap, modularity, dict(mi=win_mi, r2=win_r2, rho=win_rho), interp, names,
                           list(card), N)


DisentanglementReport = collections.namedtuple("DisentanglementReport", ["result", "fader_ok", "codes", "factors"])


def disentanglement_report(model, loader, bins=20, extra=None):
    """disentanglement of a GM-VAE's posterior means over a loader (batches as the loaders yield them: x[0] the tokens, the last two fields r_density and
    n_density).  One Engine.encode per batch; the means mu_r | mu_n stay on the device and end in one (N, 2Z) tensor - no per-batch host copy, unlike
    run_through_gmm.  The factors are r_density and n_density (continuous); extra(batch) -> (columns (B, k), k cardinalities) adds factors.

    -> DisentanglementReport(result: the Disentanglement; fader_ok: whether the MI, R^2 and rho winners of r_density are all column 0 and those of
    n_density all column Z; codes (N, 2Z), factors (N, 2 + k): the device tensors behind it).  Prints nothing."""
    if not all(hasattr(model, k) for k in ("mu_r_lookup", "n_component", "engine", "latent_dim")):
        raise ValueError("disentanglement_report: a GM-VAE (MusicAttrRegGMVAE), got %s" % type(model).__name__)
    bins = _int("bins", bins, 1, MAX_BINS + 1)
    if extra is not None and not callable(extra):
        raise ValueError("extra: a callable batch -> (columns, cardinalities), got %r" % (extra,))
    dev, Z = model._device(), model.latent_dim
    eng = model.engine()
    codes, factors, card, names, seen = [], [], [0, 0], ["r_density", "n_density"], None
    with torch.no_grad():
        for x in loader:
            d = model._indices(torch.as_tensor(x[0]).to(dev), model.roll_dims, ids_ndim=2)
            pre = eng.encode(d, save=False)
            codes.append(torch.cat([pre["r"][:, :Z], pre["n"][:, :Z]], dim=1))
            cols = [torch.as_tensor(x[-2]).to(dev).float().reshape(-1, 1), torch.as_tensor(x[-1]).to(dev).float().reshape(-1, 1)]
            if extra is not None:
                more, cards = extra(x)
                more = torch.as_tensor(more).to(dev).float()
                more = more.reshape(d.shape[0], -1)
                cards = [int(c) for c in cards]
                if len(cards) != more.shape[1] or (seen is not None and seen != cards):
                    raise ValueError("extra: (columns (B, k), k cardinalities), the same k and cardinalities for every batch; got %s and %r" % (
                        tuple(more.shape), cards))
                seen, card = cards, [0, 0] + cards
                cols.append(more)
            factors.append(torch.cat(cols, dim=1))
            if factors[-1].shape[0] != d.shape[0]:
                raise ValueError("disentanglement_report: %d pieces with %d density rows" % (d.shape[0], factors[-1].shape[0]))
    if not codes:
        raise RuntimeError("disentanglement_report: the loader yielded no batch")
    codes, factors = torch.cat(codes), torch.cat(factors)
    names = names + ["extra%d" % k for k in range(len(card) - 2)]
    res = disentanglement(codes, factors, card=card, bins=bins, names=names, ops=eng.ops)
    ok = all(int(res.winner[k][0]) == 0 and int(res.winner[k][1]) == Z for k in ("mi", "r2", "rho"))
    return DisentanglementReport(res, bool(ok), codes, factors)
