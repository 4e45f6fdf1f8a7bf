"""Shared code of tests/test_report.py (CPU) and tests/test_gpu_report.py (MI355X): fn_token_score / fn_match_rows (include/fadernets.h has the
definition).  Both are stated twice here - a plain Python loop and vectorised numpy in float64 - the case lists both suites run are built here, and
report_fake_ops() supplies the two entry points to the CPU tests through the restatement.  No GPU import, no package import at module level (the golden
generator takes this module without the package).

nll.  The reference is the definition in float64 on the float32 inputs (mx + log(sum exp(x - mx)) - x[tg]); the float32 restatement evaluates the
same lines in float32.  The bound is the rule of tests/helpers_loss.py for the nll_rows of fn_vocab_logsoftmax - the same arithmetic -
    err <= F x max(e_ref, 2**-23),  F = LOSS_F["vocab_logsoftmax"],
with err = max |got - ref64| / max |ref64| over a tile of 16 consecutive rows x 1 (helpers_head.tile_errors, tc = 1: per-row vectors) and e_ref the
err of the float32 restatement on that tile.  Where the reference is +inf (a -inf target logit) the value must be +inf at exactly those rows; they
are set to 0 in both before the metric.  A tile whose reference is identically zero (V = 1) must be exactly zero.  pred, rank and every count are
exact; nll_sum is compared bit for bit with the stated-order fp64 sum (lane l adds j = l, l + 64, ... ascending, then the xor butterfly 32 .. 1)."""
import zlib

import numpy as np

EMPTY = 1
INT_SENTINEL = -9
TOPK_V = 342


# ------------------------------------------------------------------------------------------------------------------------------
# the definitions, stated twice
# ------------------------------------------------------------------------------------------------------------------------------
def clamp_target(target, V):
    return np.clip(np.asarray(target, np.int64), 0, V - 1)


def token_score_loop(x, target=None):
    """plain Python: x (B, T, V) float32, target (B, T) or None -> dict(pred, rank int32, nll float64)"""
    B, T, V = x.shape
    out = dict(pred=np.zeros((B, T), np.int32))
    if target is not None:
        out.update(rank=np.zeros((B, T), np.int32), nll=np.zeros((B, T), np.float64))
    for b in range(B):
        for t in range(T):
            row = [float(v) for v in x[b, t]]
            best, am = -np.inf, 0x7fffffff
            for e, v in enumerate(row):
                if v > best:
                    best, am = v, e
            out["pred"][b, t] = am
            if target is None:
                continue
            tg = min(max(int(target[b, t]), 0), V - 1)
            xt = row[tg]
            out["rank"][b, t] = sum(1 for j, v in enumerate(row) if v > xt or (v == xt and j < tg))
            s = 0.0
            for v in row:
                s += np.exp(v - best)
            out["nll"][b, t] = (best + np.log(s)) - xt
    return out


def token_score_ref(x, target=None, dtype=np.float64):
    """vectorised numpy, arithmetic in `dtype` (float64: the reference; float32: the restatement whose error is e_ref)"""
    B, T, V = x.shape
    out = dict(pred=np.argmax(x, axis=-1).astype(np.int32))              # the first occurrence of the maximum
    if target is None:
        return out
    tg = clamp_target(target, V)
    xd = x.astype(dtype)
    xt = np.take_along_axis(x, tg[..., None], axis=-1)
    idx = np.arange(V).reshape(1, 1, V)
    out["rank"] = ((x > xt) | ((x == xt) & (idx < tg[..., None]))).sum(-1).astype(np.int32)
    mx = xd.max(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.exp(xd - mx).sum(-1, keepdims=True, dtype=dtype)
        out["nll"] = ((mx + np.log(s)) - xt.astype(dtype))[..., 0]
    return out


def stated_sum_loop(vals):
    """the fp64 sum of float32 values in the order fn_match_rows states: 64 partial sums, then s[l] += s[l ^ o] for o = 32 .. 1"""
    s = [0.0] * 64
    for j, v in enumerate(vals):
        s[j & 63] += float(v)
    o = 32
    while o:
        s = [s[l] + s[l ^ o] for l in range(64)]
        o >>= 1
    return s[0]


def stated_sum(vals):
    """the same order, vectorised: a lane past the end adds +0.0, which changes no partial sum (they start at +0.0 and never hold -0.0)"""
    v = np.asarray(vals, np.float64)
    pad = np.zeros((len(v) + 63) // 64 * 64, np.float64)
    pad[:len(v)] = v
    s = np.zeros(64, np.float64)
    lanes = np.arange(64)
    with np.errstate(invalid="ignore"):
        for chunk in pad.reshape(-1, 64):
            s = s + chunk
        o = 32
        while o:
            s = s + s[lanes ^ o]
            o >>= 1
    return float(s[0])


def match_rows_loop(pred, target, trim, nll=None, rank=None, topk=1):
    """plain Python, the reference's acc() line by line where trim is set: np.trim_zeros on the target, the prediction cut from its start"""
    rows, T = pred.shape
    out = dict(lead=np.zeros(rows, np.int32), len=np.zeros(rows, np.int32), correct=np.zeros(rows, np.int32), acc=np.zeros(rows, np.float64),
               status=np.zeros(rows, np.int32))
    if rank is not None:
        out["correct_topk"] = np.zeros(rows, np.int32)
    if nll is not None:
        out["nll_sum"] = np.zeros(rows, np.float64)
    for r in range(rows):
        b = [int(v) for v in target[r]]
        lead = 0
        if trim:
            while lead < T and b[lead] == 0:
                lead += 1
            end = T
            while end > lead and b[end - 1] == 0:
                end -= 1
            b = b[lead:end]
        a = [int(v) for v in pred[r]][:len(b)]
        correct = sum(1 for j in range(len(a)) if a[j] == b[j])
        out["lead"][r], out["len"][r], out["correct"][r] = lead, len(b), correct
        out["acc"][r] = correct / len(b) if b else 0.0
        out["status"][r] = 0 if b else EMPTY
        if rank is not None:
            out["correct_topk"][r] = sum(1 for j in range(len(b)) if int(rank[r, lead + j]) < topk)
        if nll is not None:
            out["nll_sum"][r] = stated_sum_loop(nll[r, lead:lead + len(b)])
    return out


def match_rows_ref(pred, target, trim, nll=None, rank=None, topk=1):
    """vectorised numpy in float64"""
    rows, T = pred.shape
    nz = target != 0
    if trim:
        any_nz = nz.any(1)
        lead = np.where(any_nz, nz.argmax(1), T)
        last = np.where(any_nz, T - 1 - nz[:, ::-1].argmax(1), -1)
        ln = np.where(any_nz, last + 1 - lead, 0)
    else:
        lead, ln = np.zeros(rows, np.int64), np.full(rows, T, np.int64)
    j = np.arange(T).reshape(1, T)
    live = j < ln.reshape(-1, 1)
    src = np.minimum(lead.reshape(-1, 1) + j, T - 1)
    tsh = np.take_along_axis(target, src, axis=1)
    correct = ((pred == tsh) & live).sum(1)
    out = dict(lead=lead.astype(np.int32), len=ln.astype(np.int32), correct=correct.astype(np.int32),
               acc=np.where(ln > 0, correct.astype(np.float64) / np.maximum(ln, 1), 0.0), status=np.where(ln > 0, 0, EMPTY).astype(np.int32))
    if rank is not None:
        out["correct_topk"] = ((np.take_along_axis(rank, src, axis=1) < topk) & live).sum(1).astype(np.int32)
    if nll is not None:
        out["nll_sum"] = np.array([stated_sum(nll[r, lead[r]:lead[r] + ln[r]]) for r in range(rows)], np.float64)
    return out


def same_exact(got, ref, keys, tag):
    for k in keys:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape, (tag, k, g.shape, r.shape)
        if r.dtype == np.float64:
            assert g.dtype == np.float64 and np.array_equal(g.view(np.int64), r.view(np.int64)), (tag, k, g[:8], r[:8])
        else:
            assert np.array_equal(g, r), (tag, k, np.flatnonzero(g.reshape(-1) != r.reshape(-1))[:8])


def check_nll(got, x, target, tag):
    """the bound of the module docstring; returns the worst ratio"""
    from helpers_head import tile_errors, worst_ratio
    from helpers_loss import LOSS_F, assert_F
    import torch
    F = assert_F(LOSS_F["vocab_logsoftmax"])
    ref, f32 = token_score_ref(x, target)["nll"].reshape(-1), token_score_ref(x, target, np.float32)["nll"].reshape(-1).astype(np.float64)
    got = np.asarray(got, np.float64).reshape(-1)
    inf = np.isposinf(ref)
    assert np.array_equal(np.isposinf(got), inf) and np.array_equal(np.isposinf(f32), inf), (tag, "+inf exactly where the target's logit is -inf")
    assert np.isfinite(ref[~inf]).all() and np.isfinite(got[~inf]).all(), (tag, "a row that is not finite")
    col = lambda a: torch.from_numpy(np.where(inf, 0.0, a).reshape(-1, 1))
    err, _ = tile_errors(col(got), col(ref), tc=1)
    e_ref, _ = tile_errors(col(f32), col(ref), tc=1)
    assert np.isfinite(e_ref).all(), (tag, "the float32 restatement misses an exactly zero tile")
    worst, i, _, n_over = worst_ratio(err, e_ref, F)
    assert n_over == 0, "%s: nll of rows %d..%d is %.2f x max(e_ref, 2**-23) from float64 (F = %d)" % (tag, 16 * i, 16 * i + 15, worst, F)
    return worst


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
def _rs(tag):
    return np.random.RandomState(zlib.crc32(tag.encode()) & 0x7fffffff)


TOKEN_SHAPES = (  # B, T, V, layout, padding columns behind V
    (1, 1, 1, "bt", 0), (5, 7, 1, "time_major", 3), (5, 7, 3, "bt", 0), (5, 7, 16, "time_major", 5), (1, 7, 63, "bt", 2), (5, 1, 64, "time_major", 0),
    (5, 7, 65, "bt", 0), (5, 7, 342, "time_major", 10), (67, 1, 342, "bt", 0), (1, 65, 342, "bt", 10), (5, 3, 1024, "bt", 0), (1, 2, 1024, "time_major", 8),
    (2, 100, 16, "bt", 0), (1, 1024, 3, "bt", 1), (5, 63, 64, "time_major", 0), (1, 64, 65, "time_major", 7), (67, 1, 16, "time_major", 0), (1, 1, 342, "bt", 0))
KINDS = ("plain", "target 0", "target V-1", "target out of range", "duplicated maxima", "ties around the target", "-inf logits", "-inf target")


def token_cases():
    """x = 3 randn; row k of a case is of KINDS[(k + case number) % 8], so a one-row case has a kind of its own.  Storage behind V and the storage's
    tail hold NaN: a read there spoils pred, nll and rank."""
    cases = []
    for ci, (B, T, V, layout, pad) in enumerate(TOKEN_SHAPES):
        tag = "B%d T%d V%d %s ld%d" % (B, T, V, layout, V + pad)
        rs = _rs(tag)
        x = (3.0 * rs.randn(B, T, V)).astype(np.float32)
        target = rs.randint(0, V, (B, T)).astype(np.int32)
        seen = set()
        for k in range(B * T):
            b, t = divmod(k, T)
            kind = KINDS[(k + ci) % len(KINDS)]
            row = x[b, t]
            if kind == "target 0":
                target[b, t] = 0
            elif kind == "target V-1":
                target[b, t] = V - 1
            elif kind == "target out of range":
                target[b, t] = (-5, V, V + 1000, -(1 << 31))[k % 4]
            elif kind == "duplicated maxima":
                j = rs.randint(0, V, 3 if V > 2 else 1)
                if V > 64:
                    j[1] = (j[0] + 64) % V                       # the same lane, another register
                row[j] = np.float32(row.max() + 1.0)
                if k % 2:
                    target[b, t] = int(j.max())                     # a maximum that is not the first: rank > 0 with nll of a maximum
            elif kind == "ties around the target" and V >= 3:
                tg = int(rs.randint(1, V - 1))
                target[b, t] = tg
                row[tg - 1] = row[tg + 1] = row[tg]
                if V > 130:
                    row[(tg + 64) % V] = row[(tg + 128) % V] = row[tg]
            elif kind == "-inf logits" and V >= 3:
                drop = rs.rand(V) < 0.4
                drop[int(target[b, t])] = False
                row[drop] = -np.inf
            elif kind == "-inf target" and V >= 2:
                row[int(target[b, t])] = -np.inf
            seen.add(kind)
        ld = V + pad
        if layout == "bt":
            store = np.full((B, T, ld), np.nan, np.float32)
            store[:, :, :V] = x
            sb, st = T * ld, ld
        else:
            store = np.full((T, B, ld), np.nan, np.float32)
            store[:, :, :V] = x.transpose(1, 0, 2)
            sb, st = ld, B * ld
        cases.append(dict(tag=tag, B=B, T=T, V=V, layout=layout, ld=ld, x=x, target=target, store=store.reshape(-1), stride_b=sb, stride_t=st,
                          n_x=(B - 1) * sb + (T - 1) * st + V, kinds=seen))
    return cases


MATCH_ROWS = (1, 5, 67)
MATCH_T = (1, 7, 63, 64, 65, 100, 1024)
ROW_KINDS = ("no zeros", "trailing pads", "leading zeros", "interior zeros", "all zero", "both ends", "one token at the end", "one token at the start")


def match_cases():
    """rows x T of the lists above, each with and without trim; pred repeats the target under the reference's shift with about 30 % of its entries
    replaced; nll holds float32 of both signs' magnitudes (one +inf in one case), rank ints below 2 * TOPK_V; topk alternates 1 and V"""
    cases = []
    for ci, (rows, T) in enumerate((r, t) for r in MATCH_ROWS for t in MATCH_T):
        for trim in (True, False):
            tag = "rows%d T%d %s" % (rows, T, "trim" if trim else "whole")
            rs = _rs(tag)
            target = rs.randint(1, TOPK_V, (rows, T)).astype(np.int32)
            for r in range(rows):
                kind = ROW_KINDS[(r + ci) % len(ROW_KINDS)]
                a, b = sorted(rs.randint(0, T + 1, 2))
                if kind == "trailing pads":
                    target[r, a:] = 0
                elif kind == "leading zeros":
                    target[r, :a] = 0
                elif kind == "interior zeros":
                    target[r, a:b] = 0
                elif kind == "all zero":
                    target[r] = 0
                elif kind == "both ends":
                    target[r, :a] = 0
                    target[r, b:] = 0
                    target[r, (a + b) // 2:(a + b) // 2 + 2] = 0
                elif kind == "one token at the end":
                    target[r, :T - 1] = 0
                elif kind == "one token at the start":
                    target[r, 1:] = 0
            ref = match_rows_ref(np.zeros_like(target), target, trim)
            pred = rs.randint(0, TOPK_V, (rows, T)).astype(np.int32)
            for r in range(rows):
                n, lead = int(ref["len"][r]), int(ref["lead"][r])
                keep = rs.rand(n) < 0.7
                pred[r, :n] = np.where(keep, target[r, lead:lead + n], pred[r, :n])
            nll = (rs.rand(rows, T) * np.exp(4 * rs.randn(rows, T))).astype(np.float32)
            if (rows, T) == (5, 100):
                nll[3, 50] = np.inf
            rank = rs.randint(0, 2 * TOPK_V, (rows, T)).astype(np.int32)
            rank[rs.rand(rows, T) < 0.3] = 0
            cases.append(dict(tag=tag, rows=rows, T=T, trim=trim, pred=pred, target=target, nll=nll, rank=rank, topk=(1, TOPK_V)[ci % 2], pad=ci % 3))
    return cases


# ------------------------------------------------------------------------------------------------------------------------------
# the reference's acc() (tests/golden/report.npz, written by tests/golden/make_golden_report.py)
# ------------------------------------------------------------------------------------------------------------------------------
GOLDEN_B, GOLDEN_T = (2, 7), (2, 9, 100)


def golden_inputs():
    """seeded (tag, pred (B, T), target (B, T), trim) without an all-zero target row: trailing pads, leading zeros, interior zeros and no zeros"""
    out = []
    for B in GOLDEN_B:
        for T in GOLDEN_T:
            for trim in (True, False):
                tag = "acc B%d T%d %s" % (B, T, "trim" if trim else "whole")
                rs = _rs(tag)
                target = rs.randint(1, 342, (B, T)).astype(np.int64)
                for r in range(B):
                    kind = r % 4
                    a, b = sorted(rs.randint(0, T, 2))
                    if kind == 0:
                        target[r, max(a, 1):] = 0
                    elif kind == 1:
                        target[r, :min(a, T - 1)] = 0
                    elif kind == 2:
                        target[r, a:b] = 0
                    if not target[r].any():
                        target[r, rs.randint(0, T)] = 7
                pred = rs.randint(0, 342, (B, T)).astype(np.int64)
                for r in range(B):                                   # matches where this call compares: under the reference's shift with trim
                    nz = np.flatnonzero(target[r])
                    seg = target[r, nz[0]:nz[-1] + 1] if trim else target[r]
                    hit = rs.rand(len(seg)) < 0.6
                    pred[r, :len(seg)] = np.where(hit, seg, pred[r, :len(seg)])
                out.append((tag, pred, target, trim))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# CPU stand-ins
# ------------------------------------------------------------------------------------------------------------------------------
def report_fake_ops():
    """the decode stand-ins + fn_token_score / fn_match_rows as their restatement (float32 nll: the restatement's float32 lines)"""
    import torch
    from helpers_constrain import ConstrainFakeOps

    class ReportFakeOps(ConstrainFakeOps):
        def token_score(self, x, stride_b, stride_t, B, T, V, target=None, pred=None, nll=None, rank=None):
            self.calls.append("token_score")
            xs = torch.as_strided(x, (B, T, V), (stride_b, stride_t, 1), x.storage_offset()).numpy()
            tg = None if target is None else target[:, :T].numpy()
            ref = token_score_ref(xs, tg, np.float32)
            for k, t in (("pred", pred), ("nll", nll), ("rank", rank)):
                if t is not None:
                    t[:, :T].copy_(torch.from_numpy(np.ascontiguousarray(ref[k])))

        def match_rows(self, pred, target, T, trim, lead, len_, correct, acc, status, nll=None, rank=None, topk=1, correct_topk=None, nll_sum=None):
            self.calls.append("match_rows")
            ref = match_rows_ref(pred[:, :T].numpy(), target[:, :T].numpy(), trim, None if nll is None else nll[:, :T].numpy(),
                                 None if rank is None else rank[:, :T].numpy(), topk)
            for k, t in (("lead", lead), ("len", len_), ("correct", correct), ("acc", acc), ("status", status), ("correct_topk", correct_topk),
                         ("nll_sum", nll_sum)):
                if t is not None:
                    t.copy_(torch.from_numpy(ref[k]))

    return ReportFakeOps()


# ------------------------------------------------------------------------------------------------------------------------------
# the class-argmax rows: token_scores on the logp_bt fn_time_logsoftmax writes
# ------------------------------------------------------------------------------------------------------------------------------
CLASS_TR, CLASS_B, CLASS_GAP, CLASS_CAP = 16, 256, 1e-4, 0.01


def class_argmax_check(pkg, ops, device, Cc):
    """seeded unit-normal logits (Tr 16, B 256, Cc) -> logp_bt of ops.time_logsoftmax (float32) -> token_scores: pred is the first-index argmax of
    that float32 logp_bt exactly, and the argmax of the float64 time-axis log-softmax on every row whose float64 top-two gap is at least 1e-4 (float32
    rounding can order two nearer classes the other way); at most 1 % of the rows may be left out.  Returns the share left out."""
    import torch
    rs = _rs("class rows Cc%d" % Cc)
    logits = torch.from_numpy(rs.randn(CLASS_TR, CLASS_B, Cc).astype(np.float32))
    lp = torch.empty(CLASS_B, CLASS_TR, Cc, device=device)
    ops.time_logsoftmax(logits.to(device), logp_bt=lp)
    pred = pkg.token_scores(lp, ops=ops).pred.cpu().numpy()
    assert pred.shape == (CLASS_B, CLASS_TR) and np.array_equal(pred, lp.cpu().numpy().argmax(-1))
    l64 = torch.log_softmax(logits.double(), dim=0).permute(1, 0, 2).numpy()
    top = np.sort(l64, axis=-1)
    keep = (top[..., -1] - top[..., -2]) >= CLASS_GAP
    assert np.array_equal(pred[keep], l64.argmax(-1)[keep]), "Cc %d: %d rows with a clear float64 winner disagree" % (Cc, int((pred != l64.argmax(-1))[keep].sum()))
    left_out = 1.0 - float(keep.mean())
    assert left_out <= CLASS_CAP, "Cc %d: %.4f of the rows are left out (cap %.2f)" % (Cc, left_out, CLASS_CAP)
    return left_out


# ------------------------------------------------------------------------------------------------------------------------------
# reconstruction_report against the restatement applied to the tensors of the same forward
# ------------------------------------------------------------------------------------------------------------------------------
REPORT_SHAPE = dict(B=5, T=20, Tr=16)


def report_batch(seed=3):
    """synth_batch at B 5, T 20, Tr 16 with a row of leading zeros (the reference's shift) and an all-pad row (EMPTY)"""
    from music_fader_nets_amd.synth import synth_batch
    b = synth_batch(np.random.RandomState(seed), REPORT_SHAPE["B"], REPORT_SHAPE["T"], REPORT_SHAPE["Tr"])
    b["d"][1, :3] = 0
    b["d"][2, :] = 0
    return b


def check_report(rep, b, labels, teacher_forced, topk):
    """every sum of `rep` from the restatement on rep['tensors'] (the logits, logp_bt and y of the same forward); returns the worst nll ratio"""
    t = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in rep["tensors"].items()}
    B, T = b["d"].shape
    d, V = b["d"].astype(np.int32), t["logits"].shape[1]
    x = np.ascontiguousarray(t["logits"].reshape(T, B, V).transpose(1, 0, 2))
    ref = token_score_ref(x, d)
    assert np.array_equal(t["rank_x"], ref["rank"]) and t["nll_x"].dtype == np.float32
    worst = check_nll(t["nll_x"], x, d, "report nll")
    if teacher_forced:
        assert np.array_equal(t["pred_x"], ref["pred"])
        mx = match_rows_ref(t["pred_x"], d, True, t["nll_x"], t["rank_x"], topk)
    else:
        mx = match_rows_ref(t["pred_x"], d, True)
    same_exact({k: getattr(rep["tensors"]["match_x"], k).cpu().numpy() for k in mx}, mx, list(mx), "tokens")
    want = dict(acc_x=mx["acc"].sum(), n_tokens=int(mx["len"].sum()), n_samples=B, n_empty=int((mx["status"] != 0).sum()))
    assert want["n_empty"] == 1 and mx["lead"][1] == 3
    for e, attr in (("r", b["r"]), ("n", b["n"])):
        pred = t["logp_" + e].argmax(-1).astype(np.int32)
        m = match_rows_ref(pred, attr.astype(np.int32), False)
        same_exact({k: getattr(rep["tensors"]["match_" + e], k).cpu().numpy() for k in m}, m, list(m), e)
        want["acc_" + e] = m["acc"].sum()
        want["acc_y_" + e] = 0 if labels is None else int((t["y_" + e] == np.asarray(labels)).sum())
    if teacher_forced:
        want["topk_x"] = (mx["correct_topk"] / np.maximum(mx["len"], 1)).sum()
        want["nll_x"] = mx["nll_sum"].sum()
    else:
        assert rep["topk_x"] is None and rep["nll_x"] is None
    for k, v in want.items():
        assert rep[k] == v if isinstance(v, int) else abs(rep[k] - v) <= 1e-12 * max(1.0, abs(v)), (k, rep[k], v)
    return worst
